"""Live voice conversion, host side (no GPU): the dependence bound of ``z_hat`` on the spectrogram, the window plan of
``vsp_convert_stream_rows`` against a brute-force enumeration of the samples every frame reads (the library and its
pure-Python twin), the argument checks that run before any launch, and the scheduling of live sessions in
``StreamingBatchService`` driven tick by tick over a recording stand-in for the engine."""
import ctypes as C

import numpy as np
import pytest
import torch

import live_convert_ref as ref
from live_convert_ref import HOP, H_SMALL, N_FFT, PAD, UP

from vispeech_amd import _lib, schema
from vispeech_amd.schema import ModelDims


# ---------------------------------------------------------------------------------------------- 1. the bound
def test_halo_of_the_two_configurations():
    assert schema.convert_halo_frames(ModelDims()) == 96
    assert schema.convert_halo_frames(ref.small_dims()) == H_SMALL == 22
    lib = _lib.lib()
    for dims in (ModelDims(), ref.small_dims()):
        h = C.c_void_p()
        assert lib.vsp_create(C.byref(_lib.make_config(dims)), 0, C.byref(h)) == 0
        try:
            assert lib.vsp_convert_halo_frames(h) == schema.convert_halo_frames(dims)
        finally:
            lib.vsp_destroy(h)
    assert lib.vsp_convert_halo_frames(None) == -1


def test_the_halo_bounds_what_a_spectrogram_column_reaches():
    """One column t0 of a (2 H + 9)-frame spectrogram perturbed: z_hat keeps its bits wherever |t - t0| > H, and changes
    at t0 (the test is not vacuous)."""
    from oracle.vispeech_oracle import Oracle
    dims = ref.small_dims()
    oracle = Oracle(ref.small_weights(dims), dims)
    H, T = H_SMALL, 2 * H_SMALL + 9
    t0 = T // 2
    r = np.random.Generator(np.random.PCG64(7))
    spec = r.uniform(0.0, 2.0, (1, dims.spec_channels, T)).astype(np.float32)
    noise = r.standard_normal((1, dims.inter_channels, T)).astype(np.float32)
    moved = spec.copy()
    moved[0, :, t0] += 1.0
    a, b = (oracle.voice_conversion(s, np.array([T]), np.array([3]), np.array([8]), noise)["z_hat"][0].numpy()
            for s in (spec, moved))
    t = np.arange(T)
    far = np.abs(t - t0) > H
    assert far.sum() == 8                                    # four frames on each side lie outside the bound
    assert np.array_equal(a[:, far], b[:, far])
    assert np.abs(a[:, t0] - b[:, t0]).max() > 1e-3


# ---------------------------------------------------------------------------------------------- 2. the window plan
N_KNOWN = [0, PAD, PAD + 1, N_FFT, 3 * HOP + 1, 40 * HOP, 40 * HOP + 255]


def c_plan(n_fft, hop, halo, n, closed, e0, e1):
    w0, w1, lo, hi = C.c_int(-7), C.c_int(-7), C.c_int64(-7), C.c_int64(-7)
    rc = _lib.lib().vsp_convert_window_plan(n_fft, hop, halo, n, int(closed), e0, e1, C.byref(w0), C.byref(w1), C.byref(lo),
                                            C.byref(hi))
    return rc, w0.value, w1.value, lo.value, hi.value


def spans(T):
    """Frames [e0, e1) at the start, in the middle and at the end of T frames (T 0: of what an open recording may ask)."""
    T = T or 45
    out = {(0, 1), (0, min(T, 4)), (T - 1, T), (max(T - 4, 0), T), (T // 2, T // 2 + 1), (T // 2, min(T, T // 2 + 3)), (0, T)}
    return sorted(s for s in out if 0 <= s[0] < s[1])


@pytest.mark.parametrize("closed", [False, True])
@pytest.mark.parametrize("n", N_KNOWN)
def test_plan_equals_brute_force(n, closed):
    T = ref.frames_of(n)
    cases = spans(T if closed else max(T, 0)) + ([] if closed else [(30, 34), (38, 41), (T, T + 2)])
    checked = 0
    for halo in (H_SMALL, 0, 3):
        for e0, e1 in cases:
            if closed and e1 > T:
                continue
            want = ref.brute_plan(N_FFT, HOP, halo, n, closed, e0, e1)
            rc, *got = c_plan(N_FFT, HOP, halo, n, closed, e0, e1)
            assert (rc, *got) == (int(want[0]), *want[1:]), (n, closed, halo, e0, e1)
            assert schema.convert_window_plan(N_FFT, HOP, halo, n, closed, e0, e1) == want
            if closed:
                assert rc == 1                               # a finished recording is always ready
            checked += 1
    assert checked or (closed and T == 0)


def test_plan_turns_ready_at_the_last_sample_the_window_reads():
    """Open, frames [2, 6): the window's last frame is 6 + H - 1; its last sample decides."""
    last = (6 + H_SMALL - 1) * HOP - PAD + N_FFT
    assert c_plan(N_FFT, HOP, H_SMALL, last - 1, False, 2, 6)[0] == 0
    assert c_plan(N_FFT, HOP, H_SMALL, last, False, 2, 6) == (1, 0, 6 + H_SMALL, 0, last)
    assert c_plan(N_FFT, HOP, H_SMALL, last, False, 30, 31)[:3] == (0, 30 - H_SMALL, 31 + H_SMALL)


def test_plan_refuses_bad_arguments():
    n = 40 * HOP
    assert c_plan(N_FFT, HOP, H_SMALL, n, False, 0, 4)[0] in (0, 1)
    for closed in (False, True):
        assert c_plan(N_FFT, HOP, H_SMALL, n, closed, -1, 4)[0] == -1            # e0 < 0
        assert c_plan(N_FFT, HOP, H_SMALL, n, closed, 4, 4)[0] == -1             # e1 <= e0
        assert c_plan(N_FFT, HOP, H_SMALL, n, closed, 5, 4)[0] == -1
        assert c_plan(N_FFT, 0, H_SMALL, n, closed, 0, 4)[0] == -1               # hop
        assert c_plan(HOP - 2, HOP, H_SMALL, n, closed, 0, 4)[0] == -1           # n_fft < hop
        assert c_plan(N_FFT, HOP, -1, n, closed, 0, 4)[0] == -1                  # halo
        assert c_plan(N_FFT, HOP, H_SMALL, -1, closed, 0, 4)[0] == -1            # n_known
        with pytest.raises(ValueError):
            schema.convert_window_plan(N_FFT, HOP, H_SMALL, n, closed, 4, 4)
    assert c_plan(N_FFT, HOP, H_SMALL, n, True, 39, 41)[0] == -1                 # closed: e1 > T = 40
    assert c_plan(N_FFT, HOP, H_SMALL, n, True, 39, 40)[0] == 1
    assert c_plan(N_FFT, HOP, H_SMALL, n, False, 39, 41)[0] == 0                 # ... open: not yet
    assert c_plan(N_FFT, HOP, H_SMALL, 100, True, 0, 1)[0] == -1                 # closed without a frame
    with pytest.raises(ValueError):
        schema.convert_window_plan(N_FFT, HOP, H_SMALL, n, True, 39, 41)
    lib = _lib.lib()
    assert lib.vsp_convert_window_plan(N_FFT, HOP, H_SMALL, n, 1, 0, 4, None, None, None, None) == 1   # outputs are optional


def test_rows_are_checked_before_anything_is_launched():
    """A context without weights: every argument error is reported as such, and a call whose rows are all ready gets as
    far as the state check."""
    lib = _lib.lib()
    assert C.sizeof(_lib.VspConvertRow) == 72
    for name in ("vsp_convert_halo_frames", "vsp_convert_window_plan", "vsp_convert_stream_rows_workspace_bytes",
                 "vsp_convert_stream_rows"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.vsp_abi_version() == 7
    dims = ref.small_dims()
    h = C.c_void_p()
    assert lib.vsp_create(C.byref(_lib.make_config(dims)), 0, C.byref(h)) == 0
    try:
        small, big = (lib.vsp_convert_stream_rows_workspace_bytes(h, 2, s) for s in (4, 8))
        assert 0 < small < big
        assert lib.vsp_convert_stream_rows_workspace_bytes(h, 0, 4) == -1
        assert lib.vsp_convert_stream_rows_workspace_bytes(h, 65, 4) == -1
        assert lib.vsp_convert_stream_rows_workspace_bytes(h, 1, 0) == -1
        # sized by the window, span + 2 H frames: the planes that dominate it, within a factor of two
        planes = 2 * (4 + 2 * H_SMALL) * 4 * (N_FFT + 3 * dims.spec_channels + 6 * dims.inter_channels)
        assert planes <= small <= 2 * planes

        def call(B=1, span=4, **kw):
            rows = (_lib.VspConvertRow * max(B, 1))()
            for r in rows:
                r.audio, r.first_sample, r.n_known, r.closed, r.e0, r.e1 = 8, 0, 40 * HOP, 1, 36, 40
                r.sid_src, r.sid_tgt, r.seed, r.noise_scale = 1, 2, 5, 1.0
                for k, v in kw.items():
                    setattr(r, k, v)
            return lib.vsp_convert_stream_rows(h, None, B, HOP, rows, span, C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), 1 << 30)

        assert call() == -2 and b"not finalised" in lib.vsp_last_error(h)        # every argument passes: the state check
        assert call(B=0) == -1 and call(B=65) == -1 and call(B=64) == -2
        assert call(span=3) == -1                                                # e1 - e0 > span_frames
        assert call(e1=41) == -1                                                 # closed: e1 > T
        assert call(closed=0) == -1 and b"read samples" in lib.vsp_last_error(h)  # open: the window is not ready
        assert call(closed=0, e0=4, e1=8) == -2                                  # ... this one is
        assert call(first_sample=(36 - H_SMALL) * HOP - PAD) == -2               # the buffer may start at s_lo
        assert call(first_sample=(36 - H_SMALL) * HOP - PAD + 1) == -1           # ... and no later
        assert call(audio=None) == -1 and call(sid_tgt=12) == -1 and call(sid_src=-1) == -1
        assert call(noise_scale=float("nan")) == -1
    finally:
        lib.vsp_destroy(h)


# ---------------------------------------------------------------------------------------------- 3. scheduling
G = 2                        # the stand-in's vocoder halo


class FakeEngine:
    """Records what the service asks for.  The 'latent' of frame t of a recording is t itself, and the 'waveform' of a frame
    is UP copies of that number: the bytes name the frames they belong to."""

    generator_halo = G

    def __init__(self):
        self.windows, self.calls = [], []

    def convert_stream_rows(self, rows, span_frames):
        z = torch.zeros((len(rows), 1, span_frames))
        tick = []
        for b, (audio, first, n, closed, e0, e1, src, tgt, seed, scale) in enumerate(rows):
            ready, w0, w1, lo, hi = schema.convert_window_plan(N_FFT, HOP, H_SMALL, n, closed, e0, e1)
            assert ready and e1 - e0 <= span_frames
            assert first <= lo and audio.numel() == n - first          # the buffer holds what the window reads
            assert torch.equal(audio[lo - first:hi - first], torch.arange(lo, hi, dtype=torch.float32))
            z[b, 0, : e1 - e0] = torch.arange(e0, e1)
            tick.append((e0, e1, bool(closed), int(n)))
        self.windows.append(tick)
        return z, torch.zeros((len(rows), 1))

    def generator_stream_rows(self, rows, chunk_frames, pcm=True):
        assert pcm
        out = np.zeros((len(rows), chunk_frames * UP), np.int16)
        tick = []
        for b, (z, g, L, f0, f1) in enumerate(rows):
            assert 0 <= f0 < f1 <= L and f1 - f0 <= chunk_frames
            assert max(0, f0 - G) == 0 and min(L, f1 + G) == L            # the window's ends are the row's lo / hi
            out[b, : (f1 - f0) * UP] = np.repeat(z[0, f0:f1].numpy(), UP)
            tick.append((int(z[0, f0]), int(z[0, f1 - 1]) + 1))
        self.calls.append(tick)
        return out


class FakeNet:
    def __init__(self):
        self._engine, self.dims = FakeEngine(), ref.small_dims()


def service(**kw):
    from vispeech_amd.service import StreamingBatchService
    net = FakeNet()
    kw.setdefault("chunk_frames", 4)
    return StreamingBatchService(net, collate=lambda rows: None, autostart=False, **kw), net._engine


def ramp(n):
    return np.arange(n, dtype=np.float32)                    # sample s has the value s: the stand-in checks its buffer


def expect(f0, f1):
    return np.repeat(np.arange(f0, f1), UP).astype("<i2").tobytes()


def ready_at(f1):
    """Samples that must have arrived for an open recording's chunk ending at frame f1."""
    return (f1 + G + H_SMALL - 1) * HOP - PAD + N_FFT


def test_a_starved_session_does_not_tick_and_feed_makes_it_ready():
    svc, eng = service()
    s = svc.open_conversion(1, 2, 9)
    assert not svc.step() and eng.windows == [] and svc.stats["ticks"] == 0
    s.feed(ramp(ready_at(4) - 1))
    assert not svc.step() and not svc.step()                 # one sample short: no tick, and no work reported
    assert eng.windows == [] and svc.stats["ticks"] == 0
    s.feed(ramp(ready_at(4))[-1:])
    assert svc.step()                                        # ... the tick; it may be ready again, so the service says so
    assert eng.windows == [[(0, 4 + G, False, ready_at(4))]] and eng.calls == [[(0, 4)]]
    assert next(s) == expect(0, 4)
    assert not svc.step() and svc.stats == {"ticks": 1, "rows_per_tick": [1], "groups": 0}


def test_end_flushes_the_remainder():
    svc, eng = service()
    s = svc.open_conversion(1, 2, 9)
    n = 40 * HOP + 17
    s.feed(ramp(n))
    while svc.step():
        pass
    done_open = eng.calls[-1][0][1]
    assert done_open == 12 and ready_at(16) > n >= ready_at(12)          # what can be delivered before the end is known
    s.end()
    with pytest.raises(RuntimeError):
        s.feed(ramp(3))
    while svc.step():
        pass
    assert [c[0] for c in eng.calls] == [(f, min(f + 4, 40)) for f in range(0, 40, 4)]
    assert eng.windows[-1] == [(36 - G, 40, True, n)] and eng.windows[3] == [(12 - G, 16 + G, True, n)]
    assert b"".join(s) == expect(0, 40) and svc._live == []


def feed_in_pieces(sizes, n, first_chunk_frames=None):
    svc, eng = service(first_chunk_frames=first_chunk_frames)
    s = svc.open_conversion(1, 2, 9)
    audio, at, k = ramp(n), 0, 0
    while at < n:
        size = sizes[k % len(sizes)]
        s.feed(audio[at:at + size])
        at, k = at + size, k + 1
        while svc.step():
            pass
    s.end()
    while svc.step():
        pass
    return eng, list(s)


def test_uneven_pieces_give_the_chunks_of_one_piece():
    n = 30 * HOP + 100
    whole, a = feed_in_pieces([n], n, first_chunk_frames=2)
    parts, b = feed_in_pieces([1, 255, 4097], n, first_chunk_frames=2)
    assert whole.calls == parts.calls == [[(0, 2)]] + [[(f, min(f + 4, 30))] for f in range(2, 30, 4)]
    assert [len(x) for x in a] == [len(x) for x in b] and b"".join(a) == b"".join(b) == expect(0, 30)


def test_a_session_keeps_the_window_and_nothing_older():
    svc, eng = service()
    s = svc.open_conversion(1, 2, 9)
    s.feed(ramp(200 * HOP))
    while svc.step():
        pass
    (req,) = svc._live
    next_w0 = req.done - G - H_SMALL
    assert req.done >= 160 and req.first == next_w0 * HOP - PAD and req.buf.numel() == req.n - req.first
    s.close()


def test_closing_a_session_removes_its_row():
    svc, eng = service()
    a, b = svc.open_conversion(1, 2, 9), svc.open_conversion(3, 4, 10)
    for s in (a, b):
        s.feed(ramp(ready_at(8)))
    svc.step()
    assert svc.stats["rows_per_tick"] == [2] and len(eng.windows[0]) == 2
    a.close()
    while svc.step():
        pass
    assert svc.stats["rows_per_tick"] == [2, 1] and len(svc._live) == 1 and list(a) == []
    b.end()
    svc.close()
    assert b"".join(b) == expect(0, ref.frames_of(ready_at(8))) and svc._live == []


def test_a_recording_without_a_frame_ends_with_no_bytes():
    svc, eng = service()
    s = svc.open_conversion(1, 2, 9)
    s.feed(ramp(100))
    s.end()
    assert not svc.step()
    assert list(s) == [] and eng.windows == [] and svc._live == []


def test_the_worker_sleeps_while_sessions_starve_and_wakes_on_feed():
    from vispeech_amd.service import StreamingBatchService
    net = FakeNet()
    svc = StreamingBatchService(net, collate=lambda rows: None, chunk_frames=4)
    looks = []
    ready_live = svc._ready_live
    svc._ready_live = lambda: (looks.append(1), ready_live())[1]
    s = svc.open_conversion(1, 2, 9)
    s.feed(ramp(ready_at(4)))
    assert next(s) == expect(0, 4)
    s.feed(ramp(ready_at(4) + HOP)[-HOP:])                   # not enough for the next chunk
    s.end()
    assert b"".join(s) == expect(4, ref.frames_of(ready_at(4) + HOP))
    svc.close()
    assert not svc._worker.is_alive()
    assert len(looks) <= 4 + len(net._engine.calls) * 2      # a look per feed / end / tick, not a spin
