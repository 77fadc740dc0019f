"""Output rows on the MI355X (output_rows.hip behind ``vsp_output_rows``): rows of mixed rates and encodings in one launch.
Float rows against the double-precision restatement on the library's own taps -- an fp32 dot product of N terms errs by at
most (N + 2) 2^-24 sum |h| |x|, the bound of ``test_output_stage_gpu.py`` -- and, byte for byte, against the single stage
(``Engine.output``); PCM16 and G.711 rows byte for byte against the published rules applied to the device's own float row;
any split of the input against the one-shot call; every row of a large call against its solo call; refused calls against
the poison they must leave; and the services end to end.  All sizes are the smallest that reach each code path."""

import numpy as np
import pytest
import torch

import isolated_ref as iso
import output_stage_ref as ref
from test_output_rows_host import ALAW, F32, S16, ULAW, LAW_REF, encode_ref
from vispeech_amd import _lib, input_stage, output_stage

pytestmark = pytest.mark.gpu

MODEL = 44100
# 8000: the longest taps (P = 354); 48000: more outputs than inputs; 22050: L = 1; 16000: a large L; 44100: pass-through
RATES = (8000, 48000, 22050, 16000, 44100)
ENCS = (F32, S16, ULAW, ALAW)
LENGTHS = (1, 93, 1601, 4000)
TORCH = {F32: torch.float32, S16: torch.int16, ULAW: torch.uint8, ALAW: torch.uint8}
POISON = {F32: float("nan"), S16: 0x5A5A, ULAW: 0x5A, ALAW: 0x5A}
PIECES = (1, 2, 159, 160, 161, 1024, 3)


def to_np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from vispeech_amd.engine import Engine
    from vispeech_amd.schema import ModelDims
    e = Engine(ModelDims(), "cuda:0")                      # (the output stage needs no weights)
    for rate in RATES:
        e.configure_output_rate(rate)
    e.configure_output_rate(RATES[0])                      # idempotent
    assert e.output_rates == RATES
    return e


@pytest.fixture(scope="module")
def wave():
    return np.tanh(0.5 * np.random.default_rng(1700).standard_normal(max(LENGTHS))).astype(np.float32)


def poisoned(eng, n, enc, lead):
    """A poisoned device buffer and its view [lead, lead + n) of the encoding's dtype."""
    big = torch.full((n + lead + 8,), POISON[enc], dtype=TORCH[enc], device=eng.device)
    return big, big[lead:lead + n]


def is_poison(a, enc):
    return bool(np.isnan(a).all()) if enc == F32 else bool((a == POISON[enc]).all())


def place(eng, x, lead):
    """``x`` on the device, ``lead`` elements into a NaN buffer (every alignment of a row's first sample occurs)."""
    big, view = poisoned(eng, len(x), F32, lead)
    view.copy_(torch.from_numpy(np.ascontiguousarray(x)))
    return big, view


def run_rows(eng, jobs, extra=5):
    """``jobs``: (x numpy, rate, enc) whole utterances in ONE ``output_rows`` call, inputs and outputs inside poisoned
    buffers at shifting alignments.  Returns per row its ``count`` elements; checks the silence behind them and the poison."""
    xs, outs, counts = [], [], []
    for i, (x, rate, enc) in enumerate(jobs):
        L, M, _ = eng.output_rate_plan(rate)
        xs.append(place(eng, x, 1 + i % 4))
        counts.append(ref.out_len(len(x), L, M))
        outs.append(poisoned(eng, counts[-1] + extra, enc, 8 + i % 4))
    _, spans = eng.output_rows([(xv, True, rate, enc, None) for (_, xv), (_, rate, enc) in zip(xs, jobs)], outs=[o for _, o in outs])
    got = []
    for i, ((x, rate, enc), (xbig, _), (obig, _), cnt) in enumerate(zip(jobs, xs, outs, counts)):
        assert spans[i] == (0, cnt)
        o, lead = to_np(obig), 8 + i % 4
        assert is_poison(o[:lead], enc) and is_poison(o[lead + cnt + extra:], enc), (i, rate, enc, "poison around out")
        tail = o[lead + cnt:lead + cnt + extra]
        assert (tail == output_stage.silence(enc)).all(), (i, rate, enc, "silence behind the row's samples")
        xb, xl = to_np(xbig), 1 + i % 4
        assert np.isnan(xb[:xl]).all() and np.isnan(xb[xl + len(x):]).all() and np.array_equal(xb[xl:xl + len(x)], x)
        got.append(o[lead:lead + cnt].copy())
    return got


@pytest.fixture(scope="module")
def single_stage(eng, wave):
    """Per (n, rate): the float32 result of the single stage configured to the rate, one-shot -- computed once."""
    out = {}
    for rate in RATES:
        eng.configure_output(rate)
        for n in LENGTHS:
            y, _ = eng.output(torch.from_numpy(wave[:n]).to(eng.device)[None, :], pcm=False)
            out[n, rate] = to_np(y)[0]
    eng.configure_output(None)
    return out


@pytest.mark.parametrize("n", LENGTHS)
def test_mixed_rows_parity_and_exactness(eng, wave, single_stage, n):
    x = wave[:n]
    jobs = [(x, rate, enc) for k, rate in enumerate(RATES) for enc in ENCS[k % 4:] + ENCS[:k % 4]]      # rates and encodings mixed
    assert len({(r, e) for _, r, e in jobs}) == 20 and jobs[0][1:] != jobs[1][1:]
    got = {(rate, enc): y for (_, rate, enc), y in zip(jobs, run_rows(eng, jobs))}
    for rate in RATES:
        L, M, H = eng.output_rate_plan(rate)
        assert (L, M) == ref.plan(MODEL, rate)[:2]
        f = got[rate, F32]
        want, cnt, mag = ref.resample_fp64(x, output_stage.taps(MODEL, rate), L, M, with_bound=True)
        err, bound = np.abs(f.astype(np.float64) - want), (cnt + 2) * 2.0 ** -24 * mag
        print(f"n = {n}, {rate} Hz: worst error / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
        assert f.shape == want.shape and np.all(err <= bound)
        assert f.tobytes() == single_stage[n, rate].tobytes(), (rate, "float row differs from the single stage")
        if rate == MODEL:
            assert f.tobytes() == x.tobytes()
        assert got[rate, S16].tobytes() == ref.pcm16(f).tobytes()
        for enc in (ULAW, ALAW):
            assert got[rate, enc].tobytes() == LAW_REF[enc](got[rate, S16]).tobytes(), (rate, enc)
    torch.cuda.synchronize()
    assert eng.status() == 0


def test_every_code_through_the_pass_through(eng):
    s = np.arange(-32768, 32768).astype(np.int16)
    x = (s.astype(np.float32) / np.float32(32767.0)).astype(np.float32)
    assert np.array_equal(ref.pcm16(x), s)
    pcm, u, a = run_rows(eng, [(x, MODEL, S16), (x, MODEL, ULAW), (x, MODEL, ALAW)])
    assert np.array_equal(pcm, s)
    for codes, enc in ((u, ULAW), (a, ALAW)):
        assert codes.tobytes() == LAW_REF[enc](s).tobytes() == output_stage.encode(s, enc).tobytes()
        assert np.all(np.diff(input_stage.decode_table(enc)[codes]) >= 0)


def test_taps_in_two_passes_and_spans_too_long_for_the_staging_area(wave):
    """6300 Hz (M = 7): the tile's span leaves room for 248 of the 449 taps, two staging passes; 4900 Hz (M = 9): the span
    alone exceeds the staging area, samples come from global memory.  Same chain: the single stage's bytes."""
    from vispeech_amd.engine import Engine
    from vispeech_amd.schema import ModelDims
    e = Engine(ModelDims(), "cuda:0")
    x = wave[:1601]
    for rate in (6300, 4900):
        e.configure_output_rate(rate)
        e.configure_output(rate)
        want = to_np(e.output(torch.from_numpy(x).to(e.device)[None, :], pcm=False)[0])[0]
        f, s, u = run_rows(e, [(x, rate, F32), (x, rate, S16), (x, rate, ULAW)])
        assert f.tobytes() == want.tobytes() and np.abs(f).max() > 1e-2, rate
        assert s.tobytes() == ref.pcm16(f).tobytes() and u.tobytes() == LAW_REF[ULAW](s).tobytes(), rate


@pytest.mark.parametrize("flush", [False, True], ids=["ended_with_the_last_piece", "flushed_by_an_empty_call"])
def test_windows_do_not_change_a_byte(eng, wave, flush):
    formats = [(8000, ULAW), (48000, S16), (22050, F32)]
    n = 4000
    xd = place(eng, wave[:n], 1)[1]
    whole, spans = eng.output_batch(xd[None, :].expand(3, -1), None, formats)
    whole = output_stage.unpack(to_np(whole), spans, [e for _, e in formats])
    states = [output_stage.RowState(eng, rate) for rate, _ in formats]
    for st in states:
        st.buf.fill_(float("nan"))
    sizes, at = [], 0
    for p in PIECES:
        sizes.append(p)
        at += p
    sizes += [n - at] + ([0] if flush else [])
    got, at = [[] for _ in formats], 0
    for k, size in enumerate(sizes):
        ended = k == len(sizes) - 1
        piece = xd[at:at + size] if size else None
        plans = [output_stage.rows_plan(*st.plan, at, size, ended) for st in states]
        sides = [st.side for st in states]
        buf, spans = eng.output_rows([(piece, ended, rate, enc, st) for (rate, enc), st in zip(formats, states)])
        host = to_np(buf)
        for i, (y, st, (m0, m1, k0, k1)) in enumerate(zip(output_stage.unpack(host, spans, [e for _, e in formats]), states, plans)):
            assert spans[i][1] == m1 - m0 and spans[i][0] % 16 == 0 and st.side == 1 - sides[i] and st.x_first == at + size
            got[i].append(y.copy())
            hist = to_np(st.buf[st.side])
            assert np.array_equal(hist[: at + size - k1], wave[k1:at + size]), (i, k, "hist_out is not samples [k1, x_first + n)")
            assert np.isnan(hist[at + size - k1:]).all(), (i, k, "hist_out written behind its samples")
            st.buf[1 - st.side].fill_(float("nan"))                   # what the call read is not needed again
        at += size
    for i, (rate, enc) in enumerate(formats):
        mine = np.concatenate(got[i])
        assert mine.shape == whole[i].shape and mine.tobytes() == whole[i].tobytes(), (rate, enc)


def test_sixty_four_rows_and_sixty_five(eng):
    x = np.tanh(0.5 * np.random.default_rng(1701).standard_normal((65, 93))).astype(np.float32)
    xd = torch.from_numpy(x).to(eng.device)
    formats = [(RATES[b % 5], ENCS[(b // 5) % 4]) for b in range(65)]
    assert len(set(formats)) == 20
    solo = []
    for b, (rate, enc) in enumerate(formats):
        buf, spans = eng.output_rows([(xd[b], True, rate, enc, None)])
        solo.append(output_stage.unpack(to_np(buf), spans, [enc])[0].tobytes())
    assert len(set(solo)) == 65
    buf, spans = eng.output_rows([(xd[b], True, rate, enc, None) for b, (rate, enc) in enumerate(formats[:64])])
    assert all(off % 16 == 0 for off, _ in spans)
    rows = output_stage.unpack(to_np(buf), spans, [e for _, e in formats[:64]])
    assert [r.tobytes() for r in rows] == solo[:64]
    buf, spans = eng.output_batch(xd, [93] * 65, formats)
    rows = output_stage.unpack(to_np(buf), spans, [e for _, e in formats])
    assert [r.tobytes() for r in rows] == solo


def test_refusals_leave_memory_untouched(eng, wave):
    from vispeech_amd.engine import Engine
    from vispeech_amd.schema import ModelDims
    lib = eng.lib
    n = 600
    xd = place(eng, wave[:n], 4)[1]
    L, M, H = eng.output_rate_plan(8000)
    K = output_stage.history_samples(L, M, H)
    hist = torch.zeros((2, K), dtype=torch.float32, device=eng.device)
    a, b = hist[0].data_ptr(), hist[1].data_ptr()
    _, obuf = poisoned(eng, 256, S16, 8)
    m0, m1, k0, k1 = output_stage.rows_plan(L, M, H, 300, 300, False)
    assert m1 - m0 > 4 and 300 > k0 and 600 > k1

    def call(**kw):
        row = (_lib.VspOutputRow * 1)()
        r = row[0]
        r.x, r.x_first, r.n, r.ended, r.out_rate, r.enc = xd.data_ptr(), 300, 300, 0, 8000, S16
        r.hist_in, r.hist_out, r.out, r.out_fill = a, b, obuf.data_ptr(), 256
        for k, v in kw.items():
            setattr(r, k, v)
        with torch.cuda.device(eng.device):
            rc = lib.vsp_output_rows(eng.ctx, eng._stream(), 1, row)
        torch.cuda.synchronize()
        if rc != 0:
            assert lib.vsp_last_error(eng.ctx) and is_poison(to_np(obuf), S16), kw
        return rc

    assert call(hist_out=a) == -1                                    # hist_in == hist_out
    assert call(hist_in=None) == -1                                  # x_first > k0
    assert call(hist_out=None) == -1                                 # x_first + n > k1, not ended
    assert call(x=None) == -1 and call(out=None) == -1
    assert call(x=xd.data_ptr() + 2) == -1 and call(out=obuf.data_ptr() + 1) == -1 and call(hist_in=a + 2) == -1
    assert call(n=-1) == -1 and call(n=0) == -1 and call(enc=4) == -1 and call(x_first=-1) == -1
    assert call(out_rate=12000) == -2                                # not configured
    assert call(out_fill=m1 - m0 - 1) == -5                          # VSP_ERR_SHAPE
    assert call(out_fill=m1 - m0) == 0
    assert not is_poison(to_np(obuf)[: m1 - m0], S16) and is_poison(to_np(obuf)[m1 - m0:], S16)
    # a ninth rate; dropping; the set and the single stage do not see each other
    e2 = Engine(ModelDims(), "cuda:0")
    for rate in (8000, 48000, 22050, 16000, 44100, 24000, 11025, 32000):
        e2.configure_output_rate(rate)
    with torch.cuda.device(e2.device):
        assert lib.vsp_output_rate_configure(e2.ctx, MODEL, 12000, 32, 9.62, 0.0) == -2
        assert lib.vsp_output_rate_configure(e2.ctx, MODEL, 8000, 16, 9.62, 0.0) == 0        # again: replaces its table
        assert lib.vsp_output_rate_configure(e2.ctx, 0, 12000, 0, 0.0, 0.0) == 0             # never configured
    e2.drop_output_rate(32000)
    e2.configure_output_rate(12000)
    assert e2.output_plan is None and 32000 not in e2.output_rates
    with pytest.raises(RuntimeError):
        e2.output(xd[None, :], pcm=True)                             # the single stage is still off
    e2.configure_output(22050)
    e2.drop_output_rate(22050)
    assert e2.output(xd[None, :], pcm=True)[0].shape == (1, 300)     # ... and does not lose its table with the set's
    with pytest.raises(RuntimeError):
        e2.output_rows([(xd, True, 22050, S16, None)])


# ---------------------------------------------------------------------------------------------- the services
FRAMES, PHON, SEEDS = [33, 15, 5, 1], [7, 5, 2, 1], [401, 402, 403, 404]
SERVICE_FORMATS = [(8000, "ulaw"), (48000, "s16"), None, (22050, "f32")]


@pytest.fixture(scope="module")
def net():
    from vispeech_amd import config as vcfg
    from vispeech_amd.models import SynthesizerTrn
    from vispeech_amd.schema import dims_from_ctor
    from vispeech_amd.synth import synth_state_dict
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    ctor = vcfg.synthesizer_args(vcfg.default_hparams())
    m = SynthesizerTrn(*ctor[0], **ctor[1]).eval()
    m.load_state_dict(synth_state_dict(dims_from_ctor(*ctor[0], **ctor[1]), seed=1234), strict=True)
    return m


def _kw(fmt):
    return {} if fmt is None else {"output_rate": fmt[0], "output_encoding": fmt[1]}


def _collate(batch):
    return lambda rows: {k: batch[k][rows] for k in ("phonemes", "lengths", "sid", "duration", "f0", "energy")}


def run_streaming(net, batch, formats):
    """The four requests join at ticks 0, 1, 2 and 3; chunks of 8 frames; driven by step()."""
    from vispeech_amd.service import StreamingBatchService
    svc = StreamingBatchService(net, max_batch=4, chunk_frames=8, collate=_collate(batch), autostart=False)
    streams = []
    for b, fmt in enumerate(formats):
        streams.append(svc.submit(b, SEEDS[b], **_kw(fmt)))
        svc.step()
    svc.close()
    assert svc.stats["rows_per_tick"] == [1, 2, 3, 2, 1] and svc.stats["groups"] == 4
    return [b"".join(s) for s in streams]


def run_batching(net, batch, formats):
    from vispeech_amd.service import BatchingSynthesisService
    svc = BatchingSynthesisService(net, max_batch=4, max_wait_s=30.0, collate=_collate(batch))
    try:
        return [f.result(120) for f in [svc.submit(b, SEEDS[b], **_kw(fmt)) for b, fmt in enumerate(formats)]]
    finally:
        svc.close()


def one_shot_rows(eng, floats, formats):
    """``output_batch`` of the requests' float waveforms, each in its format ((the model's rate, PCM16) for None)."""
    fm = [(MODEL, "s16") if f is None else f for f in formats]
    x = torch.zeros((len(floats), max(len(f) for f in floats)), dtype=torch.float32, device=eng.device)
    for b, f in enumerate(floats):
        x[b, : len(f)] = torch.from_numpy(f)
    buf, spans = eng.output_batch(x, [len(f) for f in floats], fm)
    return [r.tobytes() for r in output_stage.unpack(to_np(buf), spans, [e for _, e in fm])]


def test_services_deliver_every_request_in_its_own_format(net, monkeypatch):
    batch = iso.make_batch(FRAMES, PHON, seed=2170)
    eng, up = net._engine, net.dims.total_upsample
    calls = []
    real = eng.output_rows
    monkeypatch.setattr(eng, "output_rows", lambda rows, **k: (calls.append(len(list(rows))), real(rows, **k))[1])
    got = run_streaming(net, batch, SERVICE_FORMATS)
    assert calls == [1, 2, 3, 2, 1]                                   # ONE call per tick, over all its rows
    monkeypatch.undo()
    floats = [np.frombuffer(b, "<f4").copy() for b in run_streaming(net, batch, [(MODEL, "f32")] * 4)]
    assert [len(f) for f in floats] == [n * up for n in FRAMES] and max(np.abs(f).max() for f in floats) > 1e-3
    assert got == one_shot_rows(eng, floats, SERVICE_FORMATS)
    assert len(got[0]) == ref.out_len(33 * up, 80, 441) and len(got[1]) == 2 * ref.out_len(15 * up, 160, 147)
    # the batching service: the same utterances, each the one-shot row of ITS float waveform (another launch shape of the
    # generator: equal to the streamed one only within the bound tests/test_stream_rows_gpu.py pins, one PCM16 step)
    b_got = run_batching(net, batch, SERVICE_FORMATS)
    assert [g.dtype for g in b_got] == [np.uint8, np.dtype("<i2"), np.dtype("<i2"), np.float32]
    b_floats = run_batching(net, batch, [(MODEL, "f32")] * 4)
    assert [g.tobytes() for g in b_got] == one_shot_rows(eng, b_floats, SERVICE_FORMATS)
    plain = run_batching(net, batch, [None] * 4)                       # nobody names a format: the bytes of the row that does not
    assert plain[2].dtype == np.dtype("<i2") and plain[2].tobytes() == b_got[2].tobytes()
    worst = int(np.abs(np.frombuffer(got[2], "<i2").astype(np.int64) - b_got[2].astype(np.int64)).max())
    print(f"request 2 (PCM16 at the model's rate): streamed and batched differ by at most {worst} PCM16 steps")
    assert worst <= 1
    assert eng.status() == 0


def test_live_conversion_mu_law_in_mu_law_out():
    import live_convert_ref as live
    from test_input_convert_gpu import Net, as_ulaw, cut, speech
    from vispeech_amd.engine import Engine
    from vispeech_amd.service import StreamingBatchService
    dims = live.small_dims()
    e = Engine(dims)
    e.set_weights(live.small_weights(dims), strict=True)
    e.finalize()
    net = Net(e, dims)
    n_model = 40 * live.HOP + 100
    raw = as_ulaw(speech(n_model * 8000 // dims.sampling_rate, 82, 8000))

    def run(enc):
        svc = StreamingBatchService(net, chunk_frames=16, first_chunk_frames=4, collate=lambda rows: None, autostart=False,
                                    sampling_rate=dims.sampling_rate)
        s = svc.open_conversion(5, 9, 77, sample_rate=8000, encoding="ulaw", output_rate=8000, output_encoding=enc)
        for piece in cut(raw, (1, 255, 4097)):
            s.feed(piece.tobytes())
            svc.step()
        s.end()
        while svc.step():
            pass
        assert svc._live == []
        return b"".join(s)

    codes, floats = run("ulaw"), np.frombuffer(run("f32"), "<f4")
    T = live.frames_of(len(to_np(input_stage.one_shot(e, e._raw(raw, ULAW), len(raw), 8000, ULAW))))
    L, M, _ = e.output_rate_plan(8000)
    assert T > 20 and len(floats) == ref.out_len(T * live.UP, L, M) and np.abs(floats).max() > 1e-3
    assert codes == encode_ref(floats, ULAW).tobytes() == output_stage.encode(ref.pcm16(floats), "ulaw").tobytes()
