"""Output stage on the MI355X (resample.hip behind vsp_output_chunk): parity with the double-precision restatement fed
the library's own fp32 taps, the PCM16 rule, the pass-through, independence of the window / chunk layout, and the service
end to end.  Bounds: an fp32 dot product of N terms, in any order, errs by at most (N + 2) 2^-24 sum |h| |x|."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import output_stage_ref as ref
from vispeech_amd import _lib, output_stage

pytestmark = pytest.mark.gpu

IN_RATE = 44100
N_VALID = (1, 23456, 110251)
N_MAX = max(N_VALID)


def to_np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def dims():
    from vispeech_amd.schema import ModelDims
    return ModelDims()


@pytest.fixture(scope="module")
def eng(dims):
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from vispeech_amd.engine import Engine
    return Engine(dims, "cuda:0")                          # (the output stage needs no weights)


@pytest.fixture(scope="module")
def weights(dims):
    from vispeech_amd.synth import synth_state_dict
    return synth_state_dict(dims, seed=1234)


def make_net(weights):
    from vispeech_amd import config as vcfg
    from vispeech_amd.models import SynthesizerTrn
    args, kwargs = vcfg.synthesizer_args(vcfg.default_hparams())
    m = SynthesizerTrn(*args, **kwargs).eval()
    m.load_state_dict(weights, strict=True)
    return m


@pytest.fixture(scope="module")
def net(weights):
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return make_net(weights)


def ragged_input(scale=1.0):
    """[3, N_MAX] float32, seeded tanh(0.5 N(0, 1)) * scale."""
    rng = np.random.default_rng(20240)
    return (np.tanh(0.5 * rng.standard_normal((len(N_VALID), N_MAX))) * scale).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(rate, scale=1.0):
    """Per utterance: (y_ref float64, bound) of the valid part, from the library's own fp32 taps."""
    L, M, H = ref.plan(IN_RATE, rate)
    h = output_stage.taps(IN_RATE, rate)
    x = ragged_input(scale)
    out = []
    for b, n in enumerate(N_VALID):
        y, cnt, mag = ref.resample_fp64(x[b, :n], h, L, M, with_bound=True)
        out.append((y, (cnt + 2) * 2.0 ** -24 * mag))
    return out


def on_device(x, stride):
    """x [B, n] as a view of a [B, stride] device tensor whose padding is garbage (never to be read)."""
    buf = torch.full((x.shape[0], stride), float("nan"), dtype=torch.float32, device="cuda:0")
    buf[:, :x.shape[1]] = torch.from_numpy(x)
    return buf[:, :x.shape[1]]


def poison_tails(xd):
    """NaN and 1e30 behind each utterance's valid length (what infer's padded rows may hold is not zero)."""
    for b, n in enumerate(N_VALID):
        xd[b, n::2] = float("nan")
        xd[b, n + 1::2] = 1e30
    return xd


@pytest.mark.parametrize("stride", (N_MAX + 37, N_MAX + 38), ids=("vector_rows", "odd_rows"))
@pytest.mark.parametrize("rate", ref.RATES)
def test_float_parity_with_the_fp64_restatement(eng, rate, stride):
    eng.configure_output(rate)
    L, M, H = eng.output_plan
    assert (L, M, H) == ref.plan(IN_RATE, rate)
    xd = poison_tails(on_device(ragged_input(), stride))
    nv = torch.tensor(N_VALID, device="cuda:0")
    y, lens = eng.output(xd, nv, pcm=False)
    assert y.dtype == torch.float32 and y.shape == (3, ref.out_len(N_MAX, L, M))
    assert to_np(lens).tolist() == [ref.out_len(n, L, M) for n in N_VALID]
    y = to_np(y)
    assert np.isfinite(y).all()
    worst = 0.0
    for b, (want, bound) in enumerate(reference(rate)):
        err = np.abs(y[b, :len(want)].astype(np.float64) - want)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        print(f"{rate} utt {b}: max abs err {err.max():.3e}, worst share of the bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
        assert np.all(err <= bound), (rate, b, float(err.max()))
        assert not y[b, len(want):].any()                      # behind the utterance's own output: silence
    assert worst <= 1.0


@pytest.mark.parametrize("rate", ref.RATES)
def test_pcm16_rule(eng, rate):
    eng.configure_output(rate)
    L, M, H = eng.output_plan
    nv = torch.tensor(N_VALID, device="cuda:0")
    for scale in (1.0, 1.7):                                   # 1.7: overshoots full scale, both clip edges occur
        xd = poison_tails(on_device(ragged_input(scale), N_MAX + 37))
        q, _ = eng.output(xd, nv, pcm=True)
        assert q.dtype == torch.int16
        q = to_np(q).astype(np.float64)
        for b, (want, bound) in enumerate(reference(rate, scale)):
            target = np.clip(32767.0 * want, -32768, 32767)
            err = np.abs(q[b, :len(want)] - target)
            assert np.all(err <= 0.5 + 32767.0 * bound), (rate, scale, b, float(err.max()))
            assert not q[b, len(want):].any()
        if scale > 1.0:
            assert q.max() == 32767 and q.min() == -32768


def test_pass_through_is_the_host_quantiser_bit_for_bit(eng):
    from vispeech_amd.service import pcm16
    eng.configure_output(IN_RATE)
    assert eng.output_plan == (1, 1, 0)
    rng = np.random.default_rng(7)
    # products that are exactly k + 0.5 in fp32 (ties: round half to even), found by construction
    k = np.arange(-33000, 33000, dtype=np.float64)
    cand = ((k + 0.5) / 32767.0).astype(np.float32)
    ties = cand[(cand * np.float32(32767.0)).astype(np.float64) == k + 0.5]
    assert len(ties) > 100 and (np.floor(ties * np.float32(32767.0)) % 2 == 0).any() \
        and (np.floor(ties * np.float32(32767.0)) % 2 == 1).any()
    x = np.concatenate([ties, rng.standard_normal(50001).astype(np.float32) * 0.6,            # |x| > 1 included
                        np.float32([0.0, -0.0, 1.0, -1.0, 1.00002, -1.00002, 3.5, -3.5, 1e-8, -1e-8, 65504.0, -1e30])])
    x = np.stack([x, -x[::-1]])
    want = np.stack([pcm16(r) for r in x])
    for stride in (x.shape[1] + 2, x.shape[1] + 5):
        xd = on_device(x, stride)
        q, lens = eng.output(xd, None, pcm=True)
        np.testing.assert_array_equal(to_np(q), want)
        assert to_np(lens).tolist() == [x.shape[1]] * 2
    # chunked through the streaming helper too
    pieces = list(eng.output_stream([torch.from_numpy(x[:, a:b]).cuda() for a, b in ((0, 1), (1, 1000), (1000, x.shape[1]))]))
    np.testing.assert_array_equal(np.concatenate([to_np(p) for p in pieces], axis=1), want)


@pytest.mark.parametrize("in_rate,out_rate,zeros", ((40000, 1000, 64), (35000, 1000, 58), (44100, 100, 64), (44100, 200, 32),
                                                   (30000, 44100, 16), (48000, 32000, 64)),
                         ids=("tile_in_passes", "one_phase_in_passes", "from_global_one_phase", "from_global", "up", "3_to_2"))
def test_uncommon_ratios_take_the_other_kernel_paths(eng, in_rate, out_rate, zeros):
    """Filters whose taps or input span do not fit the block's LDS are staged in several passes or read from global
    memory; the accumulation order is the same, so the same bound holds and windows still do not change a byte."""
    eng.configure_output(out_rate, zeros=zeros, in_rate=in_rate)
    L, M, H = eng.output_plan
    h = output_stage.taps(in_rate, out_rate, zeros)
    assert len(h) == 2 * H + 1
    n = 100001
    x = ragged_input()[2:3, :n]
    want, cnt, mag = ref.resample_fp64(x[0, :n - 77], h, L, M, with_bound=True)
    xd = on_device(x, n + 3)
    xd[0, n - 77:] = float("nan")
    nv = torch.tensor([n - 77], device="cuda:0")
    y = to_np(eng.output(xd, nv, pcm=False)[0])
    assert y.shape == (1, ref.out_len(n, L, M))
    err = np.abs(y[0, :len(want)].astype(np.float64) - want)
    assert np.all(err <= (cnt + 2) * 2.0 ** -24 * mag), float(err.max())
    assert not y[0, len(want):].any()
    pieces = list(eng.output_stream([xd[:, a:b] for a, b in _windows(n, "primes")], nv, pcm=False))
    assert np.concatenate([to_np(p) for p in pieces], axis=1).tobytes() == y.tobytes()


def _windows(n, kind):
    if kind == "primes":
        sizes, cuts, i = (997, 7, 4099, 1, 13001, 2, 257), [0], 0
        while cuts[-1] < n:
            cuts.append(min(n, cuts[-1] + sizes[i % len(sizes)]))
            i += 1
        return list(zip(cuts[:-1], cuts[1:]))
    if kind == "chunks":
        return [(a, min(n, a + 64 * 512)) for a in range(0, n, 64 * 512)]
    return [(0, n)]


@pytest.mark.parametrize("rate", (22050, 16000, 48000))
@pytest.mark.parametrize("pcm", (False, True), ids=("float", "pcm16"))
def test_window_layout_does_not_change_a_byte(eng, rate, pcm):
    eng.configure_output(rate)
    L, M, H = eng.output_plan
    xd = poison_tails(on_device(ragged_input(), N_MAX + 37))
    nv = torch.tensor(N_VALID, device="cuda:0")
    one, _ = eng.output(xd, nv, pcm=pcm)
    one = to_np(one)
    for kind in ("primes", "chunks", "whole"):
        pieces = list(eng.output_stream([xd[:, a:b] for a, b in _windows(N_MAX, kind)], nv, pcm=pcm))
        got = np.concatenate([to_np(p) for p in pieces], axis=1)
        assert got.shape == one.shape and got.tobytes() == one.tobytes(), (rate, kind)
    # a batch of one, another row stride: the same bytes again (nothing depends on the batch layout)
    solo, _ = eng.output(xd[1:2, :N_VALID[1]].contiguous(), None, pcm=pcm)
    m = ref.out_len(N_VALID[1], L, M)
    assert to_np(solo).tobytes() == one[1:2, :m].tobytes()


def test_a_window_that_lacks_a_needed_sample_is_refused_before_anything_is_written(eng):
    eng.configure_output(22050)
    L, M, H = eng.output_plan
    x = torch.zeros(1, 4096, device="cuda:0")
    out = torch.full((1, 4096), 0x1234, dtype=torch.int16, device="cuda:0")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda x_first, x_len, n_max, m0, m1, stride=4096: eng.lib.vsp_output_chunk(
        eng.ctx, st, 1, C.c_void_p(x.data_ptr()), 4096, x_first, x_len, None, n_max, m0, m1, C.c_void_p(out.data_ptr()), stride, 1)
    k_lo = output_stage.history_start(1000, L, M, H)
    assert call(k_lo + 1, 2000, 100000, 1000, 1100) == -5                    # the first needed sample is missing
    assert b"need input samples" in eng.lib.vsp_last_error(eng.ctx)
    k_hi = (1099 * M + H) // L
    assert call(k_lo, k_hi - k_lo, 100000, 1000, 1100) == -5                 # the last needed sample is missing
    assert call(0, 4096, 4096, 0, 2049) == -5                                # more outputs than ceil(n_max L / M)
    assert call(0, 4097, 8192, 0, 16) == -5                                  # window longer than its row
    assert call(0, 4096, 4096, 0, 2048, stride=2047) == -5                   # outputs longer than their row
    torch.cuda.synchronize()
    assert (out == 0x1234).all()
    assert call(k_lo, k_hi - k_lo + 1, 100000, 1000, 1100) == 0             # exactly the needed samples: served
    torch.cuda.synchronize()
    assert (out[0, :100] == 0).all() and (out[0, 100:] == 0x1234).all()


@pytest.mark.parametrize("rate", ref.RATES)
def test_nothing_behind_the_valid_length_is_read(eng, rate):
    eng.configure_output(rate)
    L, M, H = eng.output_plan
    nv = torch.tensor(N_VALID, device="cuda:0")
    clean = on_device(ragged_input(), N_MAX + 37)
    for b, n in enumerate(N_VALID):
        clean[b, n:] = 0.0
    dirty = poison_tails(on_device(ragged_input(), N_MAX + 37))
    for pcm in (False, True):
        a, b_ = to_np(eng.output(clean, nv, pcm=pcm)[0]), to_np(eng.output(dirty, nv, pcm=pcm)[0])
        assert np.isfinite(b_.astype(np.float64)).all() and a.tobytes() == b_.tobytes()
        for u, n in enumerate(N_VALID):
            assert not b_[u, ref.out_len(n, L, M):].any()
    # with no n_valid the whole padded row is the signal: the zero-filled rows give the same valid outputs' prefix
    full = to_np(eng.output(clean, None, pcm=False)[0])
    m_safe = output_stage.complete_outputs(N_VALID[1], L, M, H)             # outputs that see nothing behind sample n
    np.testing.assert_array_equal(full[1, :m_safe], to_np(eng.output(clean, nv, pcm=False)[0])[1, :m_safe])


def test_service_end_to_end(net, weights, golden_dir):
    from vispeech_amd.pipeline import InFlightPool
    from vispeech_amd.service import PooledSynthesisService, SynthesisService, pcm16
    g = np.load(os.path.join(golden_dir, "ragged_controls.npz"))
    batch = dict(phonemes=g["in_phonemes"], lengths=g["in_lengths"], sid=g["in_sid"], duration=g["in_duration"],
                 f0=g["in_f0"], energy=g["in_energy"])
    noise = torch.from_numpy(g["in_noise"]).to(net.device)
    t = lambda a: torch.from_numpy(np.asarray(a)).to(net.device)
    o, x_mask, *_ = net.infer(t(g["in_phonemes"]), t(g["in_lengths"]), sid=t(g["in_sid"]), noise_scale=0.667,
                              duration_control=t(g["in_duration"]), pitch_control=t(g["in_f0"]),
                              energy_control=t(g["in_energy"]), noise=noise)
    frames = x_mask.sum(dim=(1, 2)).cpu().tolist()
    o = to_np(o)
    plain = SynthesisService(net, chunk_frames=64)                          # built as before: today's bytes
    L, M, H = ref.plan(IN_RATE, 22050)
    h = output_stage.taps(IN_RATE, 22050)
    for utt in range(o.shape[0]):
        n = int(frames[utt]) * 512
        np.testing.assert_array_equal(plain.synthesize(batch, utt, noise=noise), pcm16(o[utt, 0, :n]))
    assert net._engine.output_plan is None                                   # ... and the stage was never configured
    for utt in range(o.shape[0]):
        n = int(frames[utt]) * 512
        want, cnt, mag = ref.resample_fp64(o[utt, 0, :n], h, L, M, with_bound=True)
        bound = (cnt + 2) * 2.0 ** -24 * mag
        for cf in (8, 64):
            svc = SynthesisService(net, chunk_frames=cf, output_rate=22050)
            pcm = svc.synthesize(batch, utt, noise=noise)
            assert pcm.dtype == np.dtype("<i2") and pcm.size == ref.out_len(n, L, M)
            err = np.abs(pcm.astype(np.float64) - np.clip(32767.0 * want, -32768, 32767))
            assert np.all(err <= 0.5 + 32767.0 * bound), (utt, float(err.max()))
            pieces = list(svc.stream(batch, utt, noise=noise))
            assert len(pieces) >= n // (cf * 512) and b"".join(pieces) == pcm.tobytes() and not svc.busy
    import io
    import wave
    with wave.open(io.BytesIO(svc.wav_bytes(batch, 0, noise=noise)), "rb") as w:
        assert (w.getframerate(), w.getsampwidth(), w.getnframes()) == (22050, 2, ref.out_len(int(frames[0]) * 512, L, M))
    # GPU quantisation at the model's rate: the plain service's bytes
    dp = SynthesisService(net, chunk_frames=64, device_pcm=True)
    np.testing.assert_array_equal(dp.synthesize(batch, 1, noise=noise), plain.synthesize(batch, 1, noise=noise))
    assert b"".join(dp.stream(batch, 1, noise=noise)) == plain.synthesize(batch, 1, noise=noise).tobytes()
    # the pooled service delivers the single service's bytes
    one = SynthesisService(net, chunk_frames=64, output_rate=22050).synthesize(batch, 1, noise=noise)
    pool = InFlightPool(lambda: make_net(weights), lambda m: None, n=2)
    pooled = PooledSynthesisService(pool, chunk_frames=64, output_rate=22050)
    nz = noise.to(pool.nets[0].device)
    np.testing.assert_array_equal(pooled.synthesize(batch, 1, noise=nz), one)
    assert b"".join(pooled.stream(batch, 1, noise=nz)) == one.tobytes() and not pooled.busy
