"""Output stage, host side (no GPU): the plan and the filter of the library against the published formula and its
design figures, the double-precision restatement of the resampling sum against scipy, and the host logic of the streamed
service path with an engine whose arithmetic is that restatement."""
import ctypes as C
import io
import wave

import numpy as np
import pytest

import output_stage_ref as ref
from vispeech_amd import _lib, output_stage

IN_RATE = 44100


def _plan(in_rate, out_rate, zeros):
    L, M, H = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    rc = _lib.lib().vsp_resample_plan(in_rate, out_rate, zeros, C.byref(L), C.byref(M), C.byref(H))
    return rc, L.value, M.value, H.value


def test_plan_matches_the_table_and_refuses_what_is_not_covered():
    lib = _lib.lib()
    for rate, (L, M, n_taps) in ref.TABLE.items():
        assert _plan(IN_RATE, rate, 32) == (0, L, M, (n_taps - 1) // 2), rate
        assert ref.plan(IN_RATE, rate) == (L, M, (n_taps - 1) // 2)
        assert output_stage.plan(IN_RATE, rate) == (L, M, (n_taps - 1) // 2)
    assert _plan(IN_RATE, IN_RATE, 32) == (0, 1, 1, 0)                      # the pass-through: one unit tap
    one = np.zeros(1, np.float32)
    assert lib.vsp_resample_filter(IN_RATE, IN_RATE, 32, 9.62, 0.0, one.ctypes.data_as(C.c_void_p)) == 0 and one[0] == 1.0
    for bad in ((0, 22050, 32), (IN_RATE, 0, 32), (-1, 22050, 32), (IN_RATE, 22050, 0), (IN_RATE, 22050, -3)):
        assert _plan(*bad)[0] == -1, bad
    assert _plan(IN_RATE, 22050, 64)[0] == 0
    assert _plan(IN_RATE, 22050, 65)[0] == -7                                # zeros > 64
    assert _plan(IN_RATE, 44000, 32)[0] == -7                                # L = 440
    assert _plan(48000, 44100, 32)[0] == 0                                   # 147 / 160
    assert _plan(96000, 44100, 32)[0] == 0                                   # 147 / 320
    assert _plan(44200, 100, 32)[0] == -7                                    # M = 442
    assert _plan(44100, 100, 32) == (0, 1, 441, 32 * 441)
    L, M, H = C.c_int(), C.c_int(), C.c_int()
    assert lib.vsp_resample_plan(IN_RATE, 22050, 32, None, C.byref(M), C.byref(H)) == -1
    assert lib.vsp_resample_filter(IN_RATE, 22050, 32, 9.62, 0.0, None) == -1
    assert lib.vsp_resample_filter(IN_RATE, 22050, 32, -1.0, 0.0, one.ctypes.data_as(C.c_void_p)) == -1
    assert lib.vsp_resample_filter(IN_RATE, 22050, 32, 9.62, 1.5, one.ctypes.data_as(C.c_void_p)) == -1
    for n, L_, M_ in ((0, 1, 2), (1, 1, 2), (2, 1, 2), (3, 1, 2), (37, 160, 441), (6000, 160, 147), (110251, 320, 441)):
        assert lib.vsp_resample_out_len(n, L_, M_) == -((-n * L_) // M_) == output_stage.out_len(n, L_, M_)
    assert lib.vsp_resample_out_len(-1, 1, 2) == -1 and lib.vsp_resample_out_len(4, 0, 2) == -1
    # a context without a configured stage refuses the kernel call on the host
    cfg = _lib.make_config(__import__("vispeech_amd.schema", fromlist=["ModelDims"]).ModelDims())
    h = C.c_void_p()
    assert lib.vsp_create(C.byref(cfg), 0, C.byref(h)) == 0
    assert lib.vsp_output_chunk(h, None, 1, C.c_void_p(16), 8, 0, 8, None, 8, 0, 4, C.c_void_p(16), 4, 1) == -2
    assert b"not configured" in lib.vsp_last_error(h)
    assert lib.vsp_output_configure(h, IN_RATE, 44000, 32, 9.62, 0.0) == -7
    assert lib.vsp_output_configure(h, IN_RATE, 0, 32, 9.62, 0.0) == 0      # "off" needs no device
    lib.vsp_destroy(h)


@pytest.mark.parametrize("rate", ref.RATES)
def test_filter_is_the_formula_and_meets_the_design(rate):
    L, M, H = ref.plan(IN_RATE, rate)
    h = output_stage.taps(IN_RATE, rate)
    want = ref.filter_fp64(IN_RATE, rate)
    assert h.dtype == np.float32 and h.shape == want.shape == (2 * H + 1,)
    assert np.all(np.abs(h.astype(np.float64) - want) <= 2.0 ** -23 * np.abs(want) + 1e-12)
    np.testing.assert_array_equal(h, h[::-1])
    # explicit parameters give the same taps as the defaults they name
    np.testing.assert_array_equal(output_stage.taps(IN_RATE, rate, 32, 9.62, 1.0 - 3.065 / 32), h)
    # frequency response of the fp32 taps at rate in_rate * L (>= 2^22 points); unity gain = L at DC
    n_fft = 1 << 22
    resp = np.abs(np.fft.rfft(h.astype(np.float64), n_fft)) / L
    f = np.arange(len(resp)) / n_fft                         # cycles per sample of the rate in_rate * L; Nyquist of the
    nyq = 0.5 / max(L, M)                                    # narrower side = 1 / (2 Q)
    zeros = 32
    pass_band = resp[f <= (1.0 - 6.13 / zeros) * nyq]
    ripple_db = 20 * np.log10(pass_band)
    stop_db = 20 * np.log10(resp[f >= nyq].max())
    print(f"{rate}: ripple {ripple_db.min():+.6f} .. {ripple_db.max():+.6f} dB, stop band {stop_db:.2f} dB")
    assert np.abs(ripple_db).max() <= 0.001
    assert stop_db <= -95.0


@pytest.mark.parametrize("rate", ref.RATES)
def test_restatement_equals_scipy_resample_poly(rate):
    from scipy.signal import resample_poly
    L, M, H = ref.plan(IN_RATE, rate)
    h = ref.filter_fp64(IN_RATE, rate)
    rng = np.random.default_rng(rate)
    for n in (1, 2, 37, 513, 6000):
        x = np.tanh(0.5 * rng.standard_normal(n))
        want = resample_poly(x, L, M, window=h / L)
        got = ref.resample_fp64(x, h, L, M)
        assert got.shape == want.shape == (ref.out_len(n, L, M),), (rate, n)
        assert np.abs(got - want).max() <= 1e-12, (rate, n)
        # any sub-range of the outputs is the same numbers
        a, b = len(got) // 3, len(got) - len(got) // 4
        np.testing.assert_array_equal(ref.resample_fp64(x, h, L, M, a, b), got[a:b])


def test_complete_outputs_and_history_are_exact():
    """The streaming rule against brute force: output m is complete iff every input sample it touches is known."""
    for L, M, H in ((1, 2, 64), (160, 441, 14112), (160, 147, 5120), (3, 2, 96)):
        for n in (0, 1, 5, 63, 64, 65, 200, 1000):
            done = output_stage.complete_outputs(n, L, M, H)
            total = output_stage.out_len(n, L, M)
            brute = 0
            while brute < total and (brute * M + H) // L < n:      # last input sample of output `brute` is known
                brute += 1
            assert done == brute, (L, M, H, n)
            assert output_stage.complete_outputs(n, L, M, H, ended=True) == total
            k = output_stage.history_start(done, L, M, H)
            assert k == max(0, -((H - done * M) // L)) and (k == 0 or (k * L >= done * M - H > (k - 1) * L))


# ---------------------------------------------------------------------------------------------- streamed service path
class _FakeEngine:
    """An engine whose output stage is the float64 restatement (numpy in, numpy out) and whose vocoder is a table."""
    device = "cpu"

    def __init__(self, wave_f32, hop):
        self.wave, self.hop = wave_f32, hop
        self.calls = []

    def configure_output(self, out_rate, zeros=32, beta=9.62, rolloff=None, in_rate=None):
        self.rates = (in_rate, out_rate)
        self.output_rate = out_rate
        if out_rate == in_rate:
            self.output_plan, self.h = (1, 1, 0), np.ones(1)
        else:
            self.output_plan, self.h = ref.plan(in_rate, out_rate, zeros), ref.filter_fp64(in_rate, out_rate, zeros, beta, rolloff)

    def output_chunk(self, x, x_first, n_max, m0, m1, n_valid=None, pcm=True):
        L, M, H = self.output_plan
        x = np.asarray(x)
        self.calls.append((x_first, x.shape[1], n_max, m0, m1))
        assert n_valid is None and x_first + x.shape[1] <= n_max
        rows = []
        for r in x:
            # the window must hold every sample the outputs need: outside it the restatement would see zeros, inside
            # it sees the window's own values -- a missing sample changes the result and fails the byte comparison
            full = np.zeros(n_max)
            full[x_first:x_first + len(r)] = r
            k_lo = max(0, -((H - m0 * M) // L))
            k_hi = min(n_max - 1, ((m1 - 1) * M + H) // L)
            assert x_first <= k_lo and k_hi < x_first + len(r), "window lacks a needed sample"
            y = ref.resample_fp64(full, self.h, L, M, m0, m1)
            rows.append(ref.pcm16(y) if pcm else y.astype(np.float32))
        return np.stack(rows)

    def output(self, o, sample_lengths=None, pcm=True):
        x = np.asarray(o).reshape(o.shape[0], -1)
        y = output_stage.one_shot(self, x, None, pcm)
        return y, [y.shape[1]] * x.shape[0]

    def output_stream(self, chunks, n_valid=None, pcm=True):
        return output_stage.stream(self, (np.asarray(c) for c in chunks), n_valid, pcm)

    # what SynthesisService._stream_chunks asks of the engine before the vocoder
    def encode(self, ph, ln, sid, *ctl):
        import torch
        return dict(x_var=torch.zeros(ph.shape[0], 1, ph.shape[1]), g=None, frame_lengths=None)

    def frame_lengths_host(self, _):
        return [self.wave.shape[2] // self.hop - 2, self.wave.shape[2] // self.hop], self.wave.shape[2] // self.hop

    def decode(self, enc, tf, noise, noise_scale, max_len=None):
        return dict(z=None)

    def generator_stream(self, z, g, chunk_frames):
        for f0 in range(0, self.wave.shape[2] // self.hop, chunk_frames):
            yield self.wave[:, :, f0 * self.hop:(f0 + chunk_frames) * self.hop]


class _FakeNet:
    class dims:
        total_upsample = 16
        inter_channels = 2
    device = "cpu"

    def __init__(self, frames=75):
        import torch
        rng = np.random.default_rng(5)
        w = np.tanh(0.5 * rng.standard_normal((2, 1, frames * 16))).astype(np.float32)
        self.wave = torch.from_numpy(w)
        self._engine = _FakeEngine(self.wave, 16)
        self.frames = frames

    def infer(self, ph, ln, **kw):
        import torch
        x_mask = torch.ones(2, 1, self.frames, dtype=torch.bool)
        x_mask[0, 0, self.frames - 2:] = False
        return (self.wave, x_mask, None, None, None, None)


@pytest.mark.parametrize("rate", ref.RATES + (IN_RATE,))
def test_pushed_stream_equals_one_shot(rate):
    """``output_stage.Stream``, window by window, against ``one_shot``: the same numbers, a result for exactly the windows
    that complete an output sample, and the ``output_chunk`` calls of ``stream()`` over the same windows."""
    eng = _FakeEngine(None, None)
    eng.configure_output(rate, in_rate=IN_RATE)
    L, M, H = eng.output_plan
    x = np.tanh(0.5 * np.random.default_rng(rate).standard_normal((1, 3001))).astype(np.float32)
    sizes, windows, at = (64, 1, 512, 3, 7, 2), [], 0               # 1, 2, 3, 7, 64 and 512 samples, shuffled once
    while at < x.shape[1]:
        windows.append(x[:, at:at + sizes[len(windows) % len(sizes)]])
        at += windows[-1].shape[1]
    s = output_stage.Stream(eng, None, pcm=False)
    got, seen, m_next, silent = [], 0, 0, 0
    for w in windows:
        seen += w.shape[1]
        m_done = output_stage.complete_outputs(seen, L, M, H)
        y = s.push(w)
        assert (y is None) == (m_done == m_next), (seen, m_done, m_next)
        if y is not None:
            assert y.shape == (1, m_done - m_next)
            got.append(y)
        silent += y is None
        m_next = m_done
    assert silent > 0 or L >= M                                      # when decimating, the first 64 samples complete nothing
    tail = s.finish()
    assert (tail is None) == (m_next == output_stage.out_len(seen, L, M))
    got += [] if tail is None else [tail]
    pushed_calls = list(eng.calls)
    eng.calls.clear()
    np.testing.assert_array_equal(np.concatenate(got, axis=1), output_stage.one_shot(eng, x, None, False))
    eng.calls.clear()
    pulled = list(output_stage.stream(eng, iter(windows), None, False))
    assert eng.calls == pushed_calls and len(pulled) == len(got)
    for a, b in zip(pulled, got):
        np.testing.assert_array_equal(a, b)


BATCH = dict(phonemes=np.zeros((2, 3), np.int64), lengths=np.array([3, 3]), sid=np.array([0, 1]))


@pytest.mark.parametrize("rate", (22050, 16000, 48000))
@pytest.mark.parametrize("chunk_frames", (1, 3, 64, 10 ** 6))
def test_streamed_service_equals_one_shot(rate, chunk_frames):
    from vispeech_amd.service import Busy, SynthesisService
    net = _FakeNet()
    svc = SynthesisService(net, chunk_frames=min(chunk_frames, net.frames), output_rate=rate)
    assert net._engine.rates == (44100, rate) and svc.delivered_rate == rate
    L, M, H = ref.plan(44100, rate)
    for utt, frames in ((0, net.frames - 2), (1, net.frames)):
        n = frames * 16
        one = svc.synthesize(BATCH, utterance=utt)
        assert one.dtype == np.dtype("<i2") and one.size == -((-n * L) // M)
        want = ref.pcm16(ref.resample_fp64(net.wave[utt, 0, :n].numpy(), net._engine.h, L, M))
        np.testing.assert_array_equal(one, want)
        net._engine.calls.clear()
        pieces = list(svc.stream(BATCH, utterance=utt))
        assert b"".join(pieces) == one.tobytes()
        assert all(len(p) > 0 for p in pieces) and not svc.busy
        if chunk_frames == 1:
            assert len(pieces) > 3                                   # really streamed: many calls, bounded windows
            assert max(c[1] for c in net._engine.calls) <= 2 * H // L + 2 * 16 + 2
    wav = svc.wav_bytes(BATCH, utterance=1)
    with wave.open(io.BytesIO(wav), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, rate)
        assert w.getnframes() == -((-net.frames * 16 * L) // M)
    # the lock rules of the plain path hold for the output-stage path
    it = svc.stream(BATCH)
    assert svc.busy
    with pytest.raises(Busy):
        svc.stream(BATCH)
    assert svc.synthesize(BATCH) is None
    del it
    import gc
    gc.collect()
    assert not svc.busy
    it = svc.stream(BATCH)
    next(it)
    it.close()
    assert not svc.busy and list(it) == []


def test_pass_through_and_untouched_default_path():
    """device_pcm without a rate quantises at the model's rate; a service built as before never touches the output stage."""
    from types import SimpleNamespace
    from vispeech_amd.service import PooledSynthesisService, SynthesisService, pcm16
    net = _FakeNet()
    svc = SynthesisService(net, device_pcm=True, chunk_frames=7)
    assert net._engine.rates == (44100, 44100) and svc.delivered_rate == 44100
    want = pcm16(net.wave[1, 0])
    np.testing.assert_array_equal(svc.synthesize(BATCH, utterance=1), want)
    assert b"".join(svc.stream(BATCH, utterance=1)) == want.tobytes()
    # one output rate per model context: a service whose engine was reconfigured by another refuses instead of
    # delivering the other's rate, and releases its lock
    other = SynthesisService(net, output_rate=16000)
    with pytest.raises(RuntimeError, match="one output rate"):
        svc.synthesize(BATCH)
    with pytest.raises(RuntimeError, match="one output rate"):
        list(svc.stream(BATCH))
    assert not svc.busy and other.synthesize(BATCH).size > 0
    net2 = _FakeNet()
    net2._engine.configure_output = None                              # would raise if the plain service called it
    plain = SynthesisService(net2, chunk_frames=7)
    np.testing.assert_array_equal(plain.synthesize(BATCH, utterance=0), pcm16(net2.wave[0, 0, :(net2.frames - 2) * 16]))
    assert b"".join(plain.stream(BATCH, utterance=1)) == pcm16(net2.wave[1, 0]).tobytes()
    assert net2._engine.calls == []
    pooled = PooledSynthesisService(SimpleNamespace(nets=[_FakeNet(), _FakeNet()], streams=[None]), output_rate=16000)
    assert [s.delivered_rate for s in pooled.slots] == [16000, 16000]
    L, M, _ = ref.plan(44100, 16000)
    assert pooled.synthesize(BATCH, utterance=1).size == -((-75 * 16 * L) // M)
    with wave.open(io.BytesIO(pooled.wav_bytes(BATCH)), "rb") as w:
        assert w.getframerate() == 16000
