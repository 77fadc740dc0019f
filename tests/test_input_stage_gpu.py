"""Input stage on the MI355X (input_stage.hip behind vsp_input_rows): parity of every encoding with the fp64 sum over the
library's own taps and the exactly decoded input, exact decoding, independence of the window and of the batch, nothing read
outside a row's window, exact silence behind a row's outputs, and what the entry point refuses.
Bound (tests/test_output_stage_gpu.py): an fp32 dot product of N terms errs by at most (N + 2) 2^-24 sum |h| |x|.

Routes of the kernel (staging area 2048 words, tile 256): every rate of the list up to 192 kHz stages its tile in one
pass; 308700 Hz (M / L = 7) takes three passes, 352800 Hz (M / L = 8) decodes from global memory -- rates no caller has, here
only so that those two routes run."""
import functools

import numpy as np
import pytest
import torch

import input_stage_ref as ref
from input_stage_ref import ALAW, F32, S16, ULAW
from vispeech_amd import _lib, input_stage, output_stage

pytestmark = pytest.mark.gpu

MODEL = ref.MODEL_RATE
N_IN = (0, 1, 93, 1601, 4000)
STRIDE = max(N_IN) + 37                 # odd: with the base one element in, the rows start at every alignment
CASES = [(16000, S16, 32), (48000, F32, 32), (8000, ULAW, 32), (8000, ALAW, 32), (22050, S16, 32), (96000, F32, 32),
         (192000, F32, 16), (44100, F32, 32), (44100, S16, 32), (44100, ULAW, 32), (44100, ALAW, 32),
         (308700, S16, 32), (352800, ULAW, 32)]
ZEROS = {rate: zeros for rate, _, zeros in CASES}
PIECES = (1, 2, 159, 160, 161, 1024, 3)


def to_np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from vispeech_amd.engine import Engine
    from vispeech_amd.schema import ModelDims
    return Engine(ModelDims(), "cuda:0")                   # (the input stage needs no weights)


def configure(eng, rate):
    """The rate's filter (the context holds eight: the two route-only rates make room for each other)."""
    if rate not in eng.input_rates:
        for other in (308700, 352800):
            if other in eng.input_rates:
                eng.drop_input(other)
        eng.configure_input(rate, zeros=ZEROS[rate])
    return eng.input_plan(rate)


@functools.lru_cache(maxsize=None)
def recordings(rate, enc):
    rng = np.random.default_rng(1000 * enc + rate % 997)
    return [ref.random_raw(rng, n, enc) for n in N_IN]


@functools.lru_cache(maxsize=None)
def reference(rate, enc):
    """Per recording: (y fp64, bound), from the library's own fp32 taps and the exactly decoded samples."""
    L, M, H = ref.plan(rate, MODEL, ZEROS[rate])
    h = input_stage.taps(rate, MODEL, ZEROS[rate])
    out = []
    for raw in recordings(rate, enc):
        y, cnt, mag = ref.resample_fp64(raw, enc, h, L, M, with_bound=True)
        out.append((y, (cnt + 2) * 2.0 ** -24 * mag))
    return out


def padded(rows, enc, fill, lead=1):
    """The recordings as rows of a [B, STRIDE] device view whose base is ``lead`` elements into its buffer; everything that
    is not a recording's own sample holds ``fill``."""
    buf = np.full(len(rows) * STRIDE + lead + 64, fill, dtype=ref.DTYPES[enc])
    view = buf[lead:lead + len(rows) * STRIDE].reshape(len(rows), STRIDE)
    for b, r in enumerate(rows):
        view[b, :len(r)] = r
    dev = torch.from_numpy(buf).to("cuda:0")
    return dev[lead:lead + len(rows) * STRIDE].view(len(rows), STRIDE)


@pytest.mark.parametrize("rate,enc,zeros", CASES, ids=lambda v: str(v))
def test_parity_exact_decoding_and_nothing_outside_is_read(eng, rate, enc, zeros):
    L, M, H = configure(eng, rate)
    assert (L, M, H) == ref.plan(rate, MODEL, zeros)
    rows = recordings(rate, enc)
    n_out = [ref.out_len(n, L, M) for n in N_IN]
    got = {}
    for lead in (1, 3):                                    # both base alignments; with the odd stride every row differs
        audio, lens = eng.input_batch(padded(rows, enc, ref.poison(enc), lead), N_IN, rate, enc)
        assert audio.dtype == torch.float32 and audio.shape == (len(N_IN), max(n_out)) and lens == n_out
        got[lead] = to_np(audio)
    clean, _ = eng.input_batch(padded(rows, enc, 0, 2), N_IN, rate, enc)
    y = got[1]
    assert y.tobytes() == got[3].tobytes() == to_np(clean).tobytes()            # the poison, and the alignment, change nothing
    assert np.isfinite(y).all()
    worst = 0.0
    for b, (want, bound) in enumerate(reference(rate, enc)):
        assert len(want) == n_out[b]
        assert not y[b, n_out[b]:].any() and not np.signbit(y[b, n_out[b]:]).any()      # silence behind the row: +0.0f
        err = np.abs(y[b, :n_out[b]].astype(np.float64) - want)
        if len(want):
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
            assert len(want) < 100 or np.abs(want).max() > 0.01
    print(f"{rate} Hz enc {enc}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0
    if rate == MODEL:                                      # the pass-through only decodes
        for b, raw in enumerate(rows):
            assert y[b, :len(raw)].tobytes() == ref.decode(raw, enc).tobytes()


@pytest.mark.parametrize("rate", sorted({c[0] for c in CASES}))
def test_pcm16_is_the_float_path_fed_the_decoded_samples(eng, rate):
    configure(eng, rate)
    rows = recordings(rate, S16)
    a, _ = eng.input_batch(padded(rows, S16, ref.poison(S16)), N_IN, rate, S16)
    b, _ = eng.input_batch(padded([ref.decode(r, S16) for r in rows], F32, ref.poison(F32)), N_IN, rate, F32)
    assert to_np(a).tobytes() == to_np(b).tobytes()


def test_every_code_decodes_exactly(eng):
    configure(eng, MODEL)
    for enc, codes in ((S16, np.arange(-32768, 32768).astype(np.int16)), (ULAW, np.arange(256).astype(np.uint8)),
                       (ALAW, np.arange(256).astype(np.uint8))):
        y = to_np(input_stage.one_shot(eng, torch.from_numpy(codes).to("cuda:0"), len(codes), MODEL, enc))
        assert y.tobytes() == ref.decode(codes, enc).tobytes()
    np.testing.assert_array_equal(ref.decode(np.arange(256).astype(np.uint8), ULAW), input_stage.decode_table(ULAW))


@pytest.mark.parametrize("rate,enc", [(16000, S16), (48000, F32), (8000, ALAW)])
def test_windows_do_not_change_a_byte(eng, rate, enc):
    L, M, H = configure(eng, rate)
    raw = recordings(rate, enc)[-1]
    n = len(raw)
    dev = padded([raw], enc, ref.poison(enc))[0]
    whole = to_np(input_stage.one_shot(eng, dev, n, rate, enc))
    assert whole.shape == (ref.out_len(n, L, M),)
    ends = np.minimum(np.cumsum([PIECES[i % len(PIECES)] for i in range(200)]), n)
    ends = ends[:int(np.argmax(ends == n)) + 1]
    # 1. input_stage.Stream: each call sees the new piece and the history the stream kept
    s = input_stage.Stream(eng, rate, enc)
    got, at = [], 0
    for e in ends:
        y = s.push(dev[at:e])
        at = int(e)
        assert s.hist.numel() <= (2 * H) // L
        got += [] if y is None else [to_np(y)]
    tail = s.finish()
    got += [] if tail is None else [to_np(tail)]
    assert np.concatenate(got).tobytes() == whole.tobytes()
    # 2. raw input_rows calls over growing windows that start at sample 0: open rows, then the closed one
    got, m_next = [], 0
    for e in ends:
        m_done = output_stage.complete_outputs(int(e), L, M, H)
        if m_done > m_next:
            got.append(to_np(eng.input_rows([(dev[:e], 0, -1, m_next, m_done)], rate, enc)[0]))
            m_next = m_done
    k = output_stage.history_start(m_next, L, M, H)
    got.append(to_np(eng.input_rows([(dev[k:n], k, n, m_next, len(whole))], rate, enc)[0]))
    assert np.concatenate(got).tobytes() == whole.tobytes()


def test_batches_of_64_and_65_rows(eng):
    L, M, H = configure(eng, 16000)
    rng = np.random.default_rng(65)
    n = [50 + 3 * b for b in range(65)]
    rows = [ref.random_raw(rng, x, S16) for x in n]
    a64, l64 = eng.input_batch(padded(rows[:64], S16, ref.poison(S16)), n[:64], 16000, S16)
    a65, l65 = eng.input_batch(padded(rows, S16, ref.poison(S16)), n, 16000, S16)
    a64, a65 = to_np(a64), to_np(a65)
    assert l65[:64] == l64 and l65 == [ref.out_len(x, L, M) for x in n]
    assert a65[:64, :a64.shape[1]].tobytes() == a64.tobytes() and not a65[:64, a64.shape[1]:].any()
    for b in (0, 31, 32, 63, 64):                          # each row is what it is alone
        alone = to_np(input_stage.one_shot(eng, torch.from_numpy(rows[b]).to("cuda:0"), n[b], 16000, S16))
        assert a65[b, :l65[b]].tobytes() == alone.tobytes() and not a65[b, l65[b]:].any()


def test_refusals_come_before_anything_is_written(eng):
    L, M, H = configure(eng, 16000)
    lib = eng.lib
    raw = torch.zeros(4000, dtype=torch.int16, device="cuda:0")
    out = torch.full((12000,), float("nan"), dtype=torch.float32, device="cuda:0")
    total = ref.out_len(4000, L, M)

    def call(rate=16000, enc=S16, B=1, ptr=raw.data_ptr(), first=0, n=4000, n_total=4000, o=out.data_ptr(), m0=0, m1=total,
             fill=total, rows=True):
        arr = (_lib.VspInputRow * 2)()
        good = (raw.data_ptr(), 0, 4000, 4000, out.data_ptr(), 0, 0, 0)                  # row 0 is always a valid one
        for r, v in zip(arr, (good, (ptr, first, n, n_total, o, m0, m1, fill))):
            r.in_, r.in_first, r.in_len, r.n_total, r.out, r.m0, r.m1, r.out_fill = v
        return lib.vsp_input_rows(eng.ctx, eng._stream(), rate, enc, B, arr if rows else None)

    assert call(rate=12345, B=2) == -2                                                   # no such rate
    for kw in (dict(B=0), dict(B=65), dict(enc=4), dict(enc=-1), dict(rows=False)):
        assert call(**kw) == -1, kw
    for kw in (dict(ptr=None), dict(o=None), dict(ptr=raw.data_ptr() + 1), dict(o=out.data_ptr() + 2), dict(n=-1),
               dict(n_total=-2)):
        assert call(B=2, **kw) == -1, kw
    for kw in (dict(first=-1), dict(m0=-1), dict(m0=5, m1=4), dict(fill=total - 1), dict(n=4001), dict(m1=total + 1, fill=total + 1),
               dict(n_total=-1),                                                         # open: the last outputs are not complete
               dict(first=1, n=3999),                                                    # the window lacks sample 0 ...
               dict(n=3999, n_total=4000),                                               # ... or the recording's last sample
               dict(first=2000, n=2000, m0=0)):
        assert call(B=2, **kw) == -5, kw
    assert b"need input samples" in lib.vsp_last_error(eng.ctx)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())                                                  # nothing was launched
    done = output_stage.complete_outputs(4000, L, M, H)
    assert call(B=2, n_total=-1, m1=done, fill=done) == 0 and call(B=2) == 0
    torch.cuda.synchronize()
    assert not bool(out[:total].any()) and bool(torch.isnan(out[total:]).all())
    with pytest.raises(_lib.VspError, match="VSP_ERR_SHAPE"):
        eng.input_rows([(raw[1:], 1, 4000, 0, total)], 16000, S16)
    with pytest.raises(RuntimeError, match="not configured"):
        eng.input_rows([(raw, 0, 4000, 0, total)], 11025, S16)


def test_a_context_holds_eight_rates():
    from vispeech_amd.engine import Engine
    from vispeech_amd.schema import ModelDims
    e = Engine(ModelDims(), "cuda:0")
    rates = (8000, 11025, 16000, 22050, 32000, 44100, 48000, 96000)
    for r in rates:
        e.configure_input(r)
    with pytest.raises(_lib.VspError, match="VSP_ERR_STATE"):
        e.configure_input(192000)
    assert e.input_rates == rates
    e.configure_input(16000)                               # idempotent
    e.configure_input(16000, zeros=16)                     # ... and a rate's table can be replaced while all eight are held
    assert e.input_plan(16000) == (441, 160, 16 * 441)
    e.drop_input(8000)
    e.configure_input(192000)
    raw = torch.from_numpy(ref.random_raw(np.random.default_rng(8), 500, S16)).to("cuda:0")
    y = to_np(input_stage.one_shot(e, raw, 500, 16000, S16))
    want, cnt, mag = ref.resample_fp64(to_np(raw), S16, input_stage.taps(16000, MODEL, 16), 441, 160, with_bound=True)
    assert np.all(np.abs(y - want) <= (cnt + 2) * 2.0 ** -24 * mag)
