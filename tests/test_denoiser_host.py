"""The denoiser and the inverse STFT without a GPU: the symbols, every refusal of ``vsp_denoise``,
``vsp_istft`` and ``vsp_denoise_bias`` (decided on the host before a device is touched), the restatement judged on its own
in fp64, and the batching service with recording stand-ins: which calls a batch makes with and without a ``denoise``
request, that a request naming none gets its old bytes, and the order denoise, loudness, limiter, encoding.

(The library exposes no host-side view of its synthesis basis, so the basis is judged on the GPU through ``vsp_istft``.)"""
import ctypes as C

import numpy as np
import pytest

import denoiser_ref as dr
import test_abi
from vispeech_amd import _lib
from vispeech_amd.schema import ModelDims

NEW = ("vsp_denoise_workspace_bytes", "vsp_denoise_bias", "vsp_istft", "vsp_denoise")
NAN = float("nan")
BAD = 8                                 # a pointer no kernel may ever see: every refusal is decided before a device is needed
BIG = 1 << 40
SPEC = 1025


def test_symbols_and_abi():
    lib = _lib.lib()
    for s in NEW:
        assert hasattr(lib, s) and s in _lib.SIGNATURES, s
    assert lib.vsp_abi_version() == 7
    assert sorted(_lib.SIGNATURES) == test_abi.header_symbols()


# ---------------------------------------------------------------------------------------------- refusals
def _ctx(**dims):
    lib = _lib.lib()
    cfg = _lib.make_config(ModelDims(**dims))
    h = C.c_void_p()
    assert lib.vsp_create(C.byref(cfg), 0, C.byref(h)) == 0
    return lib, h


@pytest.fixture()
def ctx():
    lib, h = _ctx()
    yield lib, h
    lib.vsp_destroy(h)


def _denoise(lib, h, n, strength, L_max=None, audio=BAD, stride=None, bias=BAD, out=BAD, o_stride=None, ws=BIG, wsp=BAD):
    B = len(n)
    L_max = max(list(n) + [5000]) if L_max is None else L_max
    return lib.vsp_denoise(h, None, B, L_max, audio, L_max if stride is None else stride, (C.c_int64 * max(B, 1))(*n), bias,
                           (C.c_float * max(B, 1))(*strength), out, L_max if o_stride is None else o_stride, wsp, ws)


def _istft(lib, h, n, L_max=None, ri=BAD, out=BAD, o_stride=None, ws=BIG, wsp=BAD):
    B = len(n)
    L_max = max(list(n) + [5000]) if L_max is None else L_max
    return lib.vsp_istft(h, None, B, L_max, ri, (C.c_int64 * max(B, 1))(*n), out, L_max if o_stride is None else o_stride, wsp, ws)


def test_refusals_before_a_device_is_needed(ctx):
    lib, h = ctx
    err = lambda: lib.vsp_last_error(h)
    # rows that pass every check: the next thing refused is the workspace, then the missing weights
    assert _denoise(lib, h, [769, 5000], [0.0, 1.0], ws=16) == -6 and _denoise(lib, h, [769], [0.5], wsp=None) == -6
    assert _denoise(lib, h, [769, 5000], [0.0, 1.0]) == -2
    assert _istft(lib, h, [769, 5000], ws=16) == -6 and _istft(lib, h, [5000]) == -2
    need = lib.vsp_denoise_workspace_bytes(h, 2, 5000)
    T = 1 + (5000 + 2 * 768 - 2048) // 512
    assert need >= 2 * (2048 + 2050 + 2048) * T * 4 and _denoise(lib, h, [769, 5000], [0.0, 1.0], ws=need - 1) == -6
    assert lib.vsp_denoise_workspace_bytes(h, 3, 5000) > need and lib.vsp_denoise_workspace_bytes(h, 2, 5000 + 64 * 512) > need
    # n_b <= pad, n_b > L_max, naming the row
    for n in (768, 0, -3):
        assert _denoise(lib, h, [5000, n], [1.0, 1.0], L_max=5000) == -1 and b"row 1" in err(), n
        assert _istft(lib, h, [5000, 900, n], L_max=5000) == -1 and b"row 2" in err(), n
    assert _denoise(lib, h, [5001, 4000], [1.0, 1.0], L_max=5000) == -1 and b"row 0" in err()
    # a negative or infinite strength
    for s in (-0.5, float("inf"), -float("inf")):
        assert _denoise(lib, h, [5000, 4000, 3000], [1.0, 0.0, s]) == -1 and b"row 2" in err() and b"strength" in err(), s
    # a NULL bias with any finite strength; with none it is no refusal, nor is whatever a NaN row holds
    assert _denoise(lib, h, [5000, 4000], [NAN, 0.0], bias=None) == -1 and b"row 1" in err() and b"bias" in err()
    assert _denoise(lib, h, [5000, 4000], [NAN, NAN], bias=None, ws=16) == -6
    assert _denoise(lib, h, [5000, -7, 1 << 40], [1.0, NAN, NAN], L_max=5000, ws=16) == -6
    # the call's own arguments
    assert _denoise(lib, h, [], []) == -1 and _denoise(lib, h, [5000], [1.0], audio=None) == -1
    assert _denoise(lib, h, [5000], [1.0], out=None) == -1 and _denoise(lib, h, [5000], [1.0], stride=4999) == -1
    assert _denoise(lib, h, [5000], [1.0], o_stride=4999) == -1 and _denoise(lib, h, [700], [1.0]) == -1
    assert lib.vsp_denoise(h, None, 1, 5000, BAD, 5000, None, BAD, (C.c_float * 1)(1.0), BAD, 5000, BAD, BIG) == -1
    assert lib.vsp_denoise(h, None, 1, 5000, BAD, 5000, (C.c_int64 * 1)(5000), BAD, None, BAD, 5000, BAD, BIG) == -1
    assert lib.vsp_denoise(None, None, 1, 5000, BAD, 5000, (C.c_int64 * 1)(5000), BAD, (C.c_float * 1)(1.0), BAD, 5000, BAD, BIG) == -1
    assert _istft(lib, h, [5000], ri=None) == -1 and _istft(lib, h, [5000], out=None) == -1 and _istft(lib, h, []) == -1
    for B, L in ((0, 5000), (1, 768), (1, 0), (1 << 16, 5000)):
        assert lib.vsp_denoise_workspace_bytes(h, B, L) == -1
    assert lib.vsp_denoise_workspace_bytes(None, 1, 5000) == -1
    # the bias
    assert lib.vsp_denoise_bias(h, None, 3, BAD, BAD, BAD, 16) == -6 and lib.vsp_denoise_bias(h, None, 3, BAD, BAD, None, BIG) == -6
    assert lib.vsp_denoise_bias(h, None, 3, BAD, BAD, BAD, lib.vsp_denoise_workspace_bytes(h, 3, 2048)) == -2
    assert lib.vsp_denoise_bias(h, None, 0, BAD, BAD, BAD, BIG) == -1 and lib.vsp_denoise_bias(h, None, 3, None, BAD, BAD, BIG) == -1
    assert lib.vsp_denoise_bias(h, None, 3, BAD, None, BAD, BIG) == -1


@pytest.mark.parametrize("dims,why", [
    (dict(spec_channels=0), b"no spectrogram"),
    (dict(spec_channels=1001), b"does not divide"),                                      # n_fft 2000, hop 512
    (dict(upsample_rates=[8, 8, 4, 4], upsample_kernel_sizes=[16, 16, 8, 8]), b"n_fft / hop < 4"),   # hop 1024: two frames a sample
    (dict(upsample_rates=[8, 8, 8, 8], upsample_kernel_sizes=[16, 16, 16, 16]), b"does not divide"),  # hop 4096 > n_fft
])
def test_a_context_without_the_geometry_is_refused(dims, why):
    lib, h = _ctx(**dims)
    try:
        assert lib.vsp_denoise_workspace_bytes(h, 1, 5000) == -1
        assert _denoise(lib, h, [5000], [1.0]) == -1 and why in lib.vsp_last_error(h)
        assert _istft(lib, h, [5000]) == -1 and why in lib.vsp_last_error(h)
        assert lib.vsp_denoise_bias(h, None, 1, BAD, BAD, BAD, BIG) == -1 and why in lib.vsp_last_error(h)
    finally:
        lib.vsp_destroy(h)


def test_the_engine_refuses_a_hop_that_is_not_the_generators_upsampling():
    from vispeech_amd.engine import Engine

    class Stub:
        dims = ModelDims(hop_length=256)
    with pytest.raises(ValueError, match="periodic"):
        Engine._denoise_ws(Stub(), 1, 5000, "denoise")


# ---------------------------------------------------------------------------------------------- the restatement
def test_geometry_and_window_sum():
    assert dr.pad_of() == 768 and [dr.frames(n) for n in (768, 769, 1023, 1024, 1535, 1536)] == [0, 1, 1, 2, 2, 3]
    for n in dr.LENGTHS + (2048, 3000, 16 * 512 + 1, 16 * 512 - 511):
        W = dr.window_sum(n)
        assert W.shape == (n,) and W.min() >= dr.W_FLOOR, n
        if dr.frames(n) >= 2:
            assert abs(W[0] - 0.75) < 1e-12, n                       # frames 0 and 1
        if dr.frames(n) >= 8:
            assert np.abs(W[2048:n - 2048] - 1.5).max() < 1e-12      # four frames over every interior sample
    # the smallest: the last sample of a row with 511 samples of slack, under the last frame alone
    w = dr.window_sum(1023)
    assert w.argmin() == 1022 and abs(w.min() - dr.hann()[1790] ** 2) < 1e-15 and 0.0220 < w.min() < 0.0222
    assert abs(dr.window_sum(16 * 512 - 1).min() - w.min()) < 1e-15
    f = dr.window_sum(9004, dtype=np.float32)
    assert f.dtype == np.float32 and np.abs(f - dr.window_sum(9004)).max() < 4 * 2.0 ** -24 * 1.5


def test_strength_zero_is_the_identity_in_fp64():
    for x, beta in dr.fixture_rows():
        y = dr.denoise(x, beta, 0.0)
        assert y.dtype == np.float64 and np.abs(y - x).max() <= 1e-12 * np.abs(x).max(), len(x)
        ri = dr.analysis(x)
        assert np.array_equal(dr.subtract(ri, beta, 0.0), ri)
    f = dr.denoise(dr.fixture_rows()[2][0], dr.fixture_rows()[2][1], 0.0, dtype=np.float32)
    assert f.dtype == np.float32


def test_a_tiled_period_is_its_own_bias_and_vanishes_at_strength_one():
    rng = np.random.default_rng(5)
    c = rng.standard_normal(512).astype(np.float32)
    x = np.tile(c, 28)[:14000]
    beta = dr.bias_of(c)
    assert beta.shape == (SPEC,) and np.all(beta >= 0)
    # a signal of period hop has energy at multiples of n_fft / hop only, between the window's own leakage
    ri = dr.analysis(x)
    t = 10                                                              # an interior frame: no reflected sample
    m = np.sqrt(ri[:SPEC, t] ** 2 + ri[SPEC:, t] ** 2)
    assert np.abs(m - beta).max() <= 1e-10 * beta.max()
    y = dr.denoise(x, beta, 1.0)
    peak = np.abs(x).max()
    assert np.abs(y[2048:-2048]).max() < 1e-10 * peak
    assert np.abs(y).max() > 0.01 * peak                                # (the ends see the reflection: not periodic)
    half = dr.denoise(x, beta, 0.5)
    assert np.abs(half[2048:-2048] - 0.5 * x[2048:-2048]).max() < 1e-10 * peak


def test_a_large_strength_zeroes_the_row():
    x, beta = dr.fixture_rows()[6]
    assert np.all(beta[1:-1] > 0)
    y = dr.denoise(x, beta + 1.0, 1e6)
    assert np.array_equal(y, np.zeros(len(x)))


# ---------------------------------------------------------------------------------------------- the service's calls
import math  # noqa: E402

import torch  # noqa: E402

import test_service_paths_host as paths_host  # noqa: E402
from test_limiter_host import LevelEngine  # noqa: E402
from test_loudness_host import LoudInferNet, _text_service  # noqa: E402
from test_prosody_host import SVC_HOP  # noqa: E402


def _record_denoise(net, waves, n_samples, sid, strength=0.01, out=None):
    """The stand-in's ``SynthesizerTrn.denoise``: records its rows and halves, in place, every row that has a strength."""
    assert waves.dim() == 2 and waves.shape[0] == len(n_samples) == len(sid) == len(strength) and out is None
    net._engine.calls.append(("denoise", [int(v) for v in n_samples], [int(s) for s in sid],
                              [None if math.isnan(s) else round(float(s), 4) for s in strength]))
    for b, s in enumerate(strength):
        if not math.isnan(s):
            waves[b, : int(n_samples[b])] *= 0.5
    return waves


class DenoiseInferNet(LoudInferNet):
    class dims:
        total_upsample = SVC_HOP
        spec_channels = SPEC

    denoise = _record_denoise

    def __init__(self):
        super().__init__()
        self._engine = LevelEngine()


def _q(v):
    return int(np.rint(np.float32(v) * 32767.0))


def _row(spk="s"):
    from vispeech_amd.text import request_row
    return request_row(spk, ["a", "b"], durations=[1, 2], f0=[5.0, 6.0], energy=[1.0, 2.0])


def test_batching_service_denoises_first_then_levels_then_encodes():
    net = DenoiseInferNet()
    svc = _text_service(net, max_batch=4)
    try:
        futs = [svc.submit(_row(), 1, denoise=True, loudness=dict(target_lufs=-16.0, peak_ceiling=0.8), limiter=True),
                svc.submit(_row("t"), 2, denoise=0.5), svc.submit(_row(), 3, loudness=-20.0), svc.submit(_row(), 4)]
        got = [f.result(60) for f in futs]
    finally:
        svc.close()
    n = 3 * SVC_HOP
    calls = net._engine.calls
    assert [c[0] for c in calls] == ["denoise", "loudness_normalize", "loudness_limit"] and len(net.infers) == 1
    assert calls[0] == ("denoise", [n] * 4, [0, 1, 0, 0], [0.01, 0.5, None, None])
    # the stand-ins: denoise halves, normalise doubles, normalise under a limiter times 1.5 -- and the PCM is taken last
    assert [set(g.tolist()) for g in got] == [{_q(0.1875)}, {_q(0.125)}, {_q(0.5)}, {_q(0.25)}]


def test_batching_service_in_which_nobody_names_a_denoiser_makes_the_old_calls():
    net = LoudInferNet()                                   # (its dims name no spec_channels: nothing asks for them)
    net._engine = LevelEngine()
    svc = _text_service(net, max_batch=2)
    try:
        futs = [svc.submit(_row(), 1, loudness=-16), svc.submit(_row(), 2, denoise=False)]
        got = [f.result(60) for f in futs]
        for bad in (-0.1, NAN, float("inf"), "strong", dict(strength=1.0)):
            with pytest.raises(ValueError):
                svc.submit(_row(), 3, denoise=bad)
    finally:
        svc.close()
    n = 3 * SVC_HOP
    assert net._engine.calls == [("loudness_normalize", [n, n], 44100, [(-16.0, 1.0, 30.0), (None, 1.0, 0.0)])]
    assert [set(g.tolist()) for g in got] == [{_q(0.5)}, {_q(0.25)}]
    with pytest.raises(ValueError):
        _text_service(LoudInferNet(), denoise=-1.0)


def test_batching_service_default_denoiser_and_opting_out():
    net = DenoiseInferNet()
    svc = _text_service(net, denoise=True)
    try:
        futs = [svc.submit(_row(), 1), svc.submit(_row(), 2, denoise=False), svc.submit(_row(), 3, denoise=2)]
        got = [f.result(60) for f in futs]
    finally:
        svc.close()
    assert net._engine.calls == [("denoise", [3 * SVC_HOP] * 3, [0, 0, 0], [0.01, None, 2.0])]
    assert [set(g.tolist()) for g in got] == [{_q(0.125)}, {_q(0.25)}, {_q(0.125)}]


class DenoiseRecordingNet(paths_host.RecordingNet):
    class dims:
        total_upsample = paths_host.UP
        spec_channels = 9                                  # n_fft 16, hop 4: pad 6 samples

    denoise = _record_denoise


def _mixed(named):
    from vispeech_amd.service import BatchingSynthesisService
    net = DenoiseRecordingNet()
    svc = BatchingSynthesisService(net, max_batch=5, max_wait_s=30.0, collate=paths_host._collate, output_rate=22050)
    kw = lambda v: {"denoise": v} if named else {}
    try:
        futs = [svc.submit({"id": 1, "frames": 6}, 7, **kw(2.0)),
                svc.submit_conversion(paths_host._audio(93), 3, 5, 21, **kw(True)),
                svc.submit_conversion(paths_host._audio(paths_host.PAD), 3, 9, 23, **kw(True)),      # too short for one frame: no row
                svc.submit({"id": 2, "frames": 3}, 8),
                svc.submit({"id": 4, "frames": 1}, 9, **kw(True))]                                   # 4 samples <= pad: left alone
        got = [f.result(60) for f in futs]
    finally:
        svc.close()
    return net._engine.calls, got


def test_batching_service_mixed_batch_denoises_between_the_generator_and_the_output_stage():
    UP = paths_host.UP
    plain, got_plain = _mixed(False)
    calls, got = _mixed(True)
    assert "denoise" not in [c[0] for c in plain]
    k = [c[0] for c in calls].index("denoise")
    assert calls[k - 1][0] == "generator_ragged" and calls[k + 1][0] == "output" and [c[0] for c in calls].count("denoise") == 1
    # a conversion's bias is its target speaker's
    assert calls[k] == ("denoise", [6 * UP, 9 * UP, 3 * UP, 1 * UP], [1, 5, 2, 4], [2.0, 0.01, None, None])
    rest = calls[:k] + calls[k + 1:]                                         # but for it, the calls of the plain batch
    assert [c for c in rest if c[0] != "output"] == [c for c in plain if c[0] != "output"]
    assert got[2].size == 0
    for i in (3, 4):
        np.testing.assert_array_equal(got[i], got_plain[i])                  # the requests that get nothing: their bytes
    for i in (0, 1):
        assert got[i].shape == got_plain[i].shape and not np.array_equal(got[i], got_plain[i])
        assert np.abs(got[i].astype(np.int64) - np.rint(got_plain[i] / 2.0).astype(np.int64)).max() <= 1
