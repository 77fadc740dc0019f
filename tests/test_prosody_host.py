"""Prosody from a recording, everything a CPU can check (no kernel is launched): the four entry points exist and refuse what
they must before a device is needed; the fp64 restatement (tests/prosody_ref.py) judged on its own -- energy against the
Parseval form the kernel computes, F0 on harmonic complexes of known pitch, noise and silence unvoiced, the interpolation's
edge cases, the per-phoneme means against a plain loop and against the reference's in-place loop (f0energy.py:89-96), with
the one row where the two differ --; the filelist line round trip; and the batching service's calls over a recording
stand-in for the engine."""
import ctypes as C

import numpy as np
import pytest

import prosody_ref as ref
import test_abi
from vispeech_amd import _lib
from vispeech_amd.schema import ModelDims

FS, HOP = ref.FS, ref.HOP


# ---------------------------------------------------------------------------------------------- symbols and ABI
def test_symbols_and_abi():
    lib = _lib.lib()
    for s in ("vsp_prosody_frames", "vsp_prosody_workspace_bytes", "vsp_prosody_contours", "vsp_prosody_phonemes"):
        assert hasattr(lib, s) and s in _lib.SIGNATURES, s
    assert lib.vsp_abi_version() == 7
    assert sorted(_lib.SIGNATURES) == test_abi.header_symbols()


# ---------------------------------------------------------------------------------------------- frames and refusals
@pytest.fixture()
def ctx():
    lib = _lib.lib()
    cfg = _lib.make_config(ModelDims())
    h = C.c_void_p()
    assert lib.vsp_create(C.byref(cfg), 0, C.byref(h)) == 0
    yield lib, h
    lib.vsp_destroy(h)


def test_frame_count():
    lib = _lib.lib()
    for n in (641, 1023, 1024, 1025, 20 * 512 + 300, 61 * 512, 61 * 512 - 1, 441000):
        assert lib.vsp_prosody_frames(n, HOP) == n // HOP + 1 == ref.frames(n)
    assert lib.vsp_prosody_frames(44100, 256) == 44100 // 256 + 1
    assert lib.vsp_prosody_frames(640, HOP) == -1 and lib.vsp_prosody_frames(0, HOP) == -1
    assert lib.vsp_prosody_frames(4096, 0) == -1


def _contours(lib, h, n_samples, params=None, L_max=None):
    """The call with pointers no kernel may ever see (8): every refusal below is decided before a device is needed."""
    B = len(n_samples)
    n = (C.c_int64 * B)(*n_samples)
    L = max(n_samples) if L_max is None else L_max
    p = None if params is None else C.byref(_lib.VspProsodyParams(*params))
    bad = C.c_void_p(8)
    return lib.vsp_prosody_contours(h, None, B, L, HOP, bad, L, n, p, bad, bad, bad, bad, 1 << 30)


def test_refusals_before_a_device_is_needed(ctx):
    lib, h = ctx
    assert _contours(lib, h, [4096, 640, 4096]) == -1                     # a row below n_fft / 2 + 1 = 641 samples ...
    assert b"row 1" in lib.vsp_last_error(h)                              # ... named
    assert _contours(lib, h, [4096], (39.9, 750, 0.6, 0.03, 0.01)) == -1
    assert b"floor" in lib.vsp_last_error(h)
    assert _contours(lib, h, [4096], (80, FS / 4 + 1, 0.6, 0.03, 0.01)) == -1
    assert b"ceiling" in lib.vsp_last_error(h)
    assert _contours(lib, h, [4096], (80, 80, 0.6, 0.03, 0.01)) == -1
    assert lib.vsp_prosody_workspace_bytes(1, 4096, HOP, 8, C.byref(_lib.VspProsodyParams(39.0, 750, 0.6, 0.03, 0.01))) == -1
    assert lib.vsp_prosody_workspace_bytes(1, 640, HOP, 8, None) == -1
    assert 0 < lib.vsp_prosody_workspace_bytes(1, 4096, HOP, 8, None) <= lib.vsp_prosody_workspace_bytes(4, 44100, HOP, 31, None)
    # durations that claim more frames than the row has: F = 9 for 4096 samples
    bad = C.c_void_p(8)

    def phonemes(frames, durations, lengths):
        B, Tp = len(durations), len(durations[0])
        d = np.ascontiguousarray(durations, dtype=np.int64)
        return lib.vsp_prosody_phonemes(h, None, B, max(frames), Tp, bad, bad, (C.c_int64 * B)(*frames),
                                        d.ctypes.data_as(C.POINTER(C.c_int64)), (C.c_int64 * B)(*lengths), bad, bad, bad, 1 << 30)
    assert phonemes([9, 9], [[3, 3, 3], [3, 3, 4]], [3, 3]) == -1
    assert b"row 1" in lib.vsp_last_error(h)
    assert phonemes([9, 9], [[3, 3, 3], [3, -1, 4]], [3, 3]) == -1
    assert phonemes([9, 9], [[3, 3, 3], [3, 3, 3]], [3, 4]) == -1         # more phonemes than the row has columns


# ---------------------------------------------------------------------------------------------- the restatement: energy
def test_energy_by_rfft_equals_the_parseval_form():
    rng = np.random.default_rng(3)
    for n in (641, 20 * 512 + 300, 61 * 512 - 1):
        x = rng.standard_normal(n) * 0.3 + 0.05
        a, b = ref.energy_frames(x), ref.energy_frames(x, parseval=True)
        assert a.shape == (n // HOP + 1,)
        assert np.abs(a - b).max() <= 1e-12 * a.max()


# ---------------------------------------------------------------------------------------------- the restatement: F0
TONES = (90.0, 100.0, 220.5, 333.0, 441.0, 700.0)
N_TONE = 20 * HOP + 300


@pytest.mark.parametrize("f", TONES)
def test_harmonic_complexes_give_their_f0(f):
    x = ref.harmonic(f, N_TONE)
    f0, margin = ref.f0_frames(x, with_margin=True)
    assert f0.shape == (21,)
    interior = f0[2:-2]                        # frames whose 1654 samples lie inside the row
    assert (interior > 0).all()
    assert np.abs(interior / f - 1.0).max() <= 1e-3, np.abs(interior / f - 1.0).max()
    assert margin[2:-2].min() > 1e-3


def test_noise_and_silence_are_unvoiced():
    rng = np.random.default_rng(5)
    assert not ref.f0_frames(rng.standard_normal(61 * HOP) * 0.1).any()
    assert not ref.f0_frames(np.zeros(61 * HOP - 1)).any()


# ---------------------------------------------------------------------------------------------- interpolation
def test_interpolation_edge_cases():
    z = np.zeros(7)
    np.testing.assert_array_equal(ref.interpolate(z), z)                                   # no voiced frame
    one = np.array([0, 0, 210.0, 0, 0])
    np.testing.assert_array_equal(ref.interpolate(one), one)                               # exactly one: stays as it is
    ends = np.array([100.0, 0, 0, 0, 200.0])
    np.testing.assert_allclose(ref.interpolate(ends), [100, 125, 150, 175, 200], rtol=1e-15)
    mid = np.array([0, 0, 100.0, 0, 130.0, 0, 0])
    np.testing.assert_allclose(ref.interpolate(mid), [100, 100, 100, 115, 130, 130, 130], rtol=1e-15)


# ---------------------------------------------------------------------------------------------- phoneme means
def reference_in_place(contour, durations):
    """The reference's loop (f0energy.py:89-96): averages written into the frame array it still reads from."""
    p = np.array(contour, np.float64)
    pos = 0
    for i, d in enumerate(durations):
        p[i] = np.mean(p[pos: pos + d]) if d > 0 else 0
        pos += d
    return p[: len(durations)]


def plain_loop(contour, durations):
    out, pos = [], 0
    for d in durations:
        out.append(sum(float(v) for v in contour[pos: pos + d]) / d if d > 0 else 0.0)
        pos += d
    return np.array(out)


def test_phoneme_means_on_the_val_filelist_durations(golden_dir):
    import os
    g = np.load(os.path.join(golden_dir, "val_filelist.npz"))
    dur = g["in_duration"].astype(np.int64)
    assert dur.shape == (2, 31) and list(dur.sum(1)) == [310, 479] and int((dur == 0).sum()) == 20
    rng = np.random.default_rng(11)
    for d in dur:
        c = rng.uniform(80.0, 400.0, int(d.sum()) + 1)
        got = ref.phoneme_means(c, d)
        np.testing.assert_allclose(got, plain_loop(c, d), rtol=1e-13)
        np.testing.assert_allclose(got, reference_in_place(c, d), rtol=1e-13)              # no row here triggers the difference
        assert (got[d == 0] == 0).all()


def test_the_documented_difference_from_the_reference_loop():
    """A leading zero-length phoneme: the reference writes p[0] = 0 and p[1] = mean(p[0:2]) then reads the 0 it just wrote;
    the specification averages the untouched contour."""
    c = np.array([100.0, 200.0, 300.0, 400.0])
    d = np.array([0, 2, 2])
    np.testing.assert_array_equal(ref.phoneme_means(c, d), [0.0, 150.0, 350.0])
    np.testing.assert_array_equal(reference_in_place(c, d), [0.0, 100.0, 350.0])


# ---------------------------------------------------------------------------------------------- file format
def test_filelist_row_round_trip(golden_dir):
    import os
    from vispeech_amd.text import format_filelist_row, parse_filelist_row, request_row
    for line in np.load(os.path.join(golden_dir, "val_filelist.npz"))["rows"]:
        assert format_filelist_row(parse_filelist_row(str(line))) == str(line)             # the reference's own lines
    row = request_row("spk", ["a", "b", "sp"], durations=[3, 0, 12], f0=[123.45678, 0.0, 99.9996], energy=[0.00049, 7.5, 12.0],
                      utt_id="u1")
    line = format_filelist_row(row)
    assert line == "spk|u1|a b sp|3 0 12|123.457 0.000 100.000|0.000 7.500 12.000"
    back = parse_filelist_row(line)
    assert back.phones == row.phones and list(back.durations) == [3, 0, 12]
    assert format_filelist_row(back) == line
    with pytest.raises(ValueError):
        format_filelist_row(request_row("spk", ["a"], durations=[3]))                       # no f0 / energy to write
    with pytest.raises(ValueError):
        format_filelist_row(request_row("s|k", ["a"], durations=[3], f0=[1.0], energy=[1.0]))


# ---------------------------------------------------------------------------------------------- the service's calls
from test_service_paths_host import RecordingEngine  # noqa: E402

SVC_HOP = 512                           # samples per frame of the stand-in model


class ProsodyEngine(RecordingEngine):
    """The recording engine with the two prosody calls: frame k of a recording 'measures' its k-th sample, so that a
    phoneme's values name the recording and the frames they were averaged over."""
    device = "cpu"

    def prosody_contours(self, audio, n_samples, params=None, hop_length=None):
        import torch
        n = [int(x) for x in n_samples]
        assert params is None and tuple(audio.shape) == (len(n), max(n)) and audio.dtype == torch.float32
        self.calls.append(("prosody_contours", n))
        frames = [x // SVC_HOP + 1 for x in n]
        f0 = torch.zeros((len(n), max(frames)))
        for b, F in enumerate(frames):
            f0[b, :F] = audio[b, :F]
        return f0, 2.0 * f0, None, frames

    def prosody_phonemes(self, f0_frames, energy_frames, frames_host, durations, lengths):
        import torch
        d = np.asarray(durations)
        self.calls.append(("prosody_phonemes", list(frames_host), d.astype(int).tolist(), [int(x) for x in lengths]))
        f0, en = torch.zeros(d.shape), torch.zeros(d.shape)
        for b in range(d.shape[0]):
            pos = 0
            for j in range(int(lengths[b])):
                n = int(d[b, j])
                if n:
                    f0[b, j], en[b, j] = f0_frames[b, pos: pos + n].mean(), energy_frames[b, pos: pos + n].mean()
                pos += n
        return f0, en


class InferNet:
    """A model whose ``infer`` records its arguments: one frame per unit of duration, a waveform of zeros."""
    device = "cpu"

    class dims:
        total_upsample = SVC_HOP

    def __init__(self):
        self._engine = ProsodyEngine()
        self.infers = []

    def infer(self, phonemes, lengths, sid=None, noise_scale=1, duration_control=None, pitch_control=None, energy_control=None,
              noise_seed=None, isolated=False, row_controls=None):
        import torch
        assert isolated
        self.infers.append(dict(duration=duration_control, f0=pitch_control, energy=energy_control, rows=row_controls,
                                seeds=list(noise_seed)))
        B = phonemes.shape[0]
        frames = [3] * B
        x_mask = torch.zeros((B, 1, 3))
        for b, F in enumerate(frames):
            x_mask[b, 0, :F] = 1
        return torch.zeros((B, 1, 3 * SVC_HOP)), x_mask


def _service(net, max_batch=3):
    from vispeech_amd.service import BatchingSynthesisService
    from vispeech_amd.text import SymbolTable
    return BatchingSynthesisService(net, max_batch=max_batch, max_wait_s=30.0, table=SymbolTable(["a", "b", "c"]), spk2id={"s": 0, "t": 1})


def test_service_runs_one_contour_and_one_phoneme_call_per_batch():
    import torch
    from vispeech_amd.text import request_row
    net = InferNet()
    rec_a = np.arange(1, 3 * SVC_HOP + 1, dtype=np.float32)                   # 4 frames; frame k 'measures' k + 1
    rec_b = 100.0 + np.arange(2 * SVC_HOP, dtype=np.float32)                  # 3 frames; 100 + k
    svc = _service(net)
    try:
        futs = [svc.submit(request_row("s", ["a", "b", "c"], durations=[1, 0, 2]), 7, prosody_audio=rec_a),
                svc.submit(request_row("t", ["a", "b"]), 8),
                svc.submit(request_row("s", ["c", "a"], durations=[2, 1], f0=[9.0, 9.0], energy=[9.0, 9.0]), 9,
                           prosody_audio=rec_b)]
        for f in futs:
            assert f.result(60).shape == (3 * SVC_HOP,)
    finally:
        svc.close()
    eng = net._engine
    assert eng.calls == [("prosody_contours", [3 * SVC_HOP, 2 * SVC_HOP]),
                         ("prosody_phonemes", [4, 3], [[1, 0, 2], [2, 1, 0]], [3, 2])]
    (call,) = net.infers
    assert call["seeds"] == [7, 8, 9]
    np.testing.assert_array_equal(call["rows"].given, [[True, True, True], [False, False, False], [True, True, True]])
    assert torch.is_tensor(call["f0"]) and torch.is_tensor(call["energy"])
    np.testing.assert_array_equal(call["f0"].numpy(), [[1.0, 0.0, 2.5], [0.0, 0.0, 0.0], [100.5, 102.0, 0.0]])
    np.testing.assert_array_equal(call["energy"].numpy(), 2.0 * call["f0"].numpy())      # the row's own 9.0 gave way


def test_service_without_a_recording_makes_the_calls_it_always_made():
    from vispeech_amd.text import request_row
    net = InferNet()
    svc = _service(net, max_batch=2)
    try:
        futs = [svc.submit(request_row("s", ["a", "b"], durations=[1, 2], f0=[5.0, 6.0], energy=[1.0, 2.0]), 1),
                svc.submit(request_row("t", ["c"], durations=[3], f0=[7.0], energy=[3.0]), 2)]
        [f.result(60) for f in futs]
    finally:
        svc.close()
    assert net._engine.calls == []
    (call,) = net.infers
    assert call["rows"] is None and call["seeds"] == [1, 2]
    np.testing.assert_array_equal(np.asarray(call["f0"]), [[5.0, 6.0], [7.0, 0.0]])


def test_service_refuses_a_recording_without_durations_in_submit():
    from vispeech_amd.text import request_row
    net = InferNet()
    svc = _service(net)
    try:
        with pytest.raises(ValueError, match="durations"):
            svc.submit(request_row("s", ["a"]), 1, prosody_audio=np.zeros(4096, np.float32))
        with pytest.raises(ValueError, match="frames"):
            svc.submit(request_row("s", ["a"], durations=[10]), 1, prosody_audio=np.zeros(4096, np.float32))
        with pytest.raises(ValueError):
            svc.submit(request_row("s", ["a"], durations=[1]), 1, prosody_sample_rate=16000)
    finally:
        svc.close()
    assert net._engine.calls == [] and net.infers == []
