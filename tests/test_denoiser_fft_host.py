"""The denoiser's FFT path without a GPU: the switch's symbols and every refusal of its setter (decided
on the host before a device is needed), the workspace the switch sizes, the float32 FFT restatement of
tests/denoiser_fft_ref.py judged against fp64 on its own, and the host layers with recording stand-ins -- a service given
``denoise_transform="fft"`` passes it to exactly the denoise call, one given none makes the recorded calls it made before,
``push_rows`` refuses mixed transforms, and the bias cache is keyed by transform."""
import ctypes as C
import os

import numpy as np
import pytest

import denoiser_fft_ref as fr
import denoiser_ref as dr
import test_abi
import test_denoiser_host as one_shot_host
import test_denoiser_stream_host as stream_host
from vispeech_amd import _lib, denoiser
from vispeech_amd.schema import ModelDims

NEW = ("vsp_set_stft_transform", "vsp_stft_transform")
DFT, FFT = 0, 1


def _ctx(**dims):
    lib = _lib.lib()
    cfg = _lib.make_config(ModelDims(**dims))
    h = C.c_void_p()
    assert lib.vsp_create(C.byref(cfg), 0, C.byref(h)) == 0
    return lib, h


# ---------------------------------------------------------------------------------------------- the switch
def test_symbols_and_abi():
    lib = _lib.lib()
    for s in NEW:
        assert hasattr(lib, s) and s in _lib.SIGNATURES, s
    assert lib.vsp_abi_version() == 7
    assert sorted(_lib.SIGNATURES) == test_abi.header_symbols()
    assert _lib.STFT_TRANSFORMS == {"dft": DFT, "fft": FFT}
    header = open(os.path.join(test_abi.ROOT, "include", "vispeech_hip.h")).read()
    assert "#define VSP_STFT_DFT 0" in header and "#define VSP_STFT_FFT 1" in header


def test_the_switch_is_off_on_a_fresh_context_and_sizes_the_workspace():
    lib, h = _ctx()
    try:
        assert lib.vsp_stft_transform(h) == DFT
        dft = (lib.vsp_denoise_workspace_bytes(h, 2, 5000), lib.vsp_denoise_rows_workspace_bytes(h, 2, 5000))
        assert lib.vsp_set_stft_transform(h, FFT) == 0 and lib.vsp_stft_transform(h) == FFT
        fft = (lib.vsp_denoise_workspace_bytes(h, 2, 5000), lib.vsp_denoise_rows_workspace_bytes(h, 2, 5000))
        # the FFT path keeps ONE frame tensor (transformed in place; RI stays in LDS): less, never more
        T = 1 + (5000 + 2 * 768 - 2048) // 512
        assert all(0 < f < d for f, d in zip(fft, dft)) and fft[0] >= 2 * 2048 * T * 4
        # the refusals of the calls themselves are those of the product path, in the same order
        assert one_shot_host._denoise(lib, h, [769, 5000], [0.0, 1.0], ws=fft[0] - 1) == -6
        assert one_shot_host._denoise(lib, h, [769, 5000], [0.0, 1.0], ws=fft[0]) == -2
        assert one_shot_host._istft(lib, h, [5000], ws=16) == -6 and one_shot_host._istft(lib, h, [5000]) == -2
        assert lib.vsp_denoise_bias(h, None, 3, 8, 8, 8, lib.vsp_denoise_workspace_bytes(h, 3, 2048)) == -2
        assert lib.vsp_set_stft_transform(h, DFT) == 0 and lib.vsp_stft_transform(h) == DFT
        assert (lib.vsp_denoise_workspace_bytes(h, 2, 5000), lib.vsp_denoise_rows_workspace_bytes(h, 2, 5000)) == dft
    finally:
        lib.vsp_destroy(h)


def test_an_unknown_kind_is_refused_and_changes_nothing():
    lib, h = _ctx()
    try:
        assert lib.vsp_set_stft_transform(h, FFT) == 0
        for kind in (2, -1, 7):
            assert lib.vsp_set_stft_transform(h, kind) == -1 and b"unknown kind" in lib.vsp_last_error(h), kind
            assert lib.vsp_stft_transform(h) == FFT
        assert lib.vsp_set_stft_transform(None, FFT) == -1 and lib.vsp_stft_transform(None) == -1
    finally:
        lib.vsp_destroy(h)


@pytest.mark.parametrize("dims,why", [
    (dict(spec_channels=0), b"no spectrogram"),
    (dict(spec_channels=1), b"no spectrogram"),
    (dict(spec_channels=1001), b"does not divide"),                                      # n_fft 2000, hop 512
    (dict(upsample_rates=[8, 8, 4, 4], upsample_kernel_sizes=[16, 16, 8, 8]), b"n_fft / hop < 4"),   # hop 1024
    (dict(upsample_rates=[8, 8, 8, 8], upsample_kernel_sizes=[16, 16, 16, 16]), b"does not divide"),  # hop 4096 > n_fft
    # a geometry the denoiser takes and the FFT does not: n_fft 1024 over hop 256
    (dict(spec_channels=513, upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4]), b"n_fft = 2048 only"),
])
def test_the_setter_refuses_a_context_the_fft_cannot_serve(dims, why):
    lib, h = _ctx(**dims)
    try:
        assert lib.vsp_set_stft_transform(h, FFT) == -1 and why in lib.vsp_last_error(h), lib.vsp_last_error(h)
        assert lib.vsp_stft_transform(h) == DFT                      # refused: the switch stays where it was
        assert lib.vsp_set_stft_transform(h, DFT) == 0               # the default is no request: nothing to refuse
    finally:
        lib.vsp_destroy(h)


def test_the_engine_refuses_an_unknown_transform_before_the_library():
    from vispeech_amd.engine import Engine

    class Stub:
        pass
    with pytest.raises(ValueError, match="'dft' or 'fft'"):
        Engine._set_transform(Stub(), "dct", "denoise")


# ---------------------------------------------------------------------------------------------- the restatement
def test_the_float32_transform_is_the_dft_sum():
    rng = np.random.default_rng(11)
    x = rng.standard_normal((64, 3)).astype(np.float32)
    y = rng.standard_normal((64, 3)).astype(np.float32)
    for sign in (-1, +1):
        re, im = fr.fft32(x, y, sign)
        k = np.arange(64)
        want = np.exp(sign * 2j * np.pi * np.outer(k, k) / 64) @ (x.astype(np.float64) + 1j * y)
        assert np.abs(re + 1j * im - want).max() <= 64 * dr.U32 * np.abs(want).max()


def test_the_float32_fft_restatement_is_within_its_gate_on_every_row_and_strength():
    """The gate is 4 x its own distance, so what is judged here is that the distance is a rounding error at all: it stays
    under the floor's own count of roundings on every row (no row's gate is decided by a restatement gone wrong), and the
    FFT gate is several times tighter than the DFT gate of tests/test_denoiser_gpu.py."""
    rows = dr.fixture_rows()
    for s, per in fr.restated().items():
        for b, ((x, _), (d, f, gate)) in enumerate(zip(rows, per)):
            dist = float(np.abs(f.astype(np.float64) - d).max())
            floor = fr.floor_of(x, len(x))
            assert f.dtype == np.float32 and f.shape == d.shape == (len(x),)
            assert dist <= gate and dist <= floor and gate <= max(4 * floor, floor), (s, b, dist, floor, gate)
            assert fr.floor_of(x, len(x)) < dr.floor_of(x, len(x)) / 6
    x, beta = rows[6]
    ri64, ri32 = dr.analysis(x), fr.analysis(x)
    assert ri32.dtype == np.float32 and np.abs(ri32 - ri64).max() <= np.sqrt(fr.ROUNDINGS) * dr.U32 * np.abs(ri64).max()
    c = (0.01 * np.random.default_rng(3).standard_normal(dr.HOP)).astype(np.float32)
    d, f = dr.bias_of(c), fr.bias_of(c)
    assert f.dtype == np.float32 and np.abs(f - d).max() <= np.sqrt(fr.ROUNDINGS) * dr.U32 * d.max()


# ---------------------------------------------------------------------------------------------- streams
class _TransformEngine:
    """``sr.RefEngine`` that records the keyword each call carries."""

    def __init__(self):
        import denoiser_stream_ref as sr
        self.ref, self.kw = sr.RefEngine(), []
        self.denoise_history, self.denoise_complete = self.ref.denoise_history, self.ref.denoise_complete

    def denoise_rows(self, rows, bias, **kw):
        self.kw.append(kw)
        return self.ref.denoise_rows(rows, bias)


def test_a_stream_carries_its_transform_and_push_rows_refuses_a_mix():
    x, beta = dr.fixture_rows()[5]
    eng = _TransformEngine()
    a, b = denoiser.Stream(eng, beta, 1.0, transform="fft"), denoiser.Stream(eng, beta, 1.0, transform="fft")
    c = denoiser.Stream(eng, beta, 1.0)
    assert (a.transform, c.transform) == ("fft", "dft")
    with pytest.raises(ValueError, match="one transform"):
        denoiser.push_rows(eng, [(a, x[:3000], False), (c, x[:3000], False)])
    assert a.seen == 0 and c.seen == 0 and eng.kw == []                      # refused before anything was taken
    denoiser.push_rows(eng, [(a, x[:3000], False), (b, x[:4000], False)])
    c.push(x[:3000])
    a.push(x[3000:], final=True)
    assert eng.kw == [{"transform": "fft"}, {}, {"transform": "fft"}]       # the default makes the call it always made
    with pytest.raises(ValueError, match="'dft' or 'fft'"):
        denoiser.Stream(eng, beta, 1.0, transform="czt")


# ---------------------------------------------------------------------------------------------- the model's bias cache
def test_the_bias_cache_is_keyed_by_transform():
    import torch
    from vispeech_amd.models import SynthesizerTrn

    class BiasEngine:
        def __init__(self):
            self.calls = []

        def denoise_bias(self, g, **kw):
            self.calls.append((g.shape[0], kw))
            return torch.full((g.shape[0], 3), 2.0 if kw else 1.0)

        def denoise(self, audio, n, bias, strength, out=None, **kw):
            self.calls.append(("denoise", float(bias[0, 0]), kw))
            return audio

        def denoise_history(self):
            return 1536, 2047

    net = SynthesizerTrn.__new__(SynthesizerTrn)
    net._engine = eng = BiasEngine()
    net._state = {"emb_g.weight": np.zeros((9, 4), np.float32)}
    assert float(net.denoiser_bias([3, 5])[0, 0]) == 1.0 and float(net.denoiser_bias([5, 3], "fft")[1, 0]) == 2.0
    assert float(net.denoiser_bias([5])[0, 0]) == 1.0 and float(net.denoiser_bias([3, 7], transform="fft")[0, 0]) == 2.0
    assert eng.calls == [(2, {}), (2, {"transform": "fft"}), (1, {"transform": "fft"})]      # (each speaker once per transform)
    del eng.calls[:]
    net.denoise(torch.zeros(1, 4000), [4000], [3], 1.0)
    net.denoise(torch.zeros(1, 4000), [4000], [3], 1.0, transform="fft")
    assert eng.calls == [("denoise", 1.0, {}), ("denoise", 2.0, {"transform": "fft"})]     # each path its own bias
    st = net.denoise_stream(7, 0.5, transform="fft")
    assert st.transform == "fft" and float(st.bias[0]) == 2.0 and net.denoise_stream(5).transform == "dft"
    with pytest.raises(ValueError, match="'dft' or 'fft'"):
        net.denoiser_bias([3], "dct")


# ---------------------------------------------------------------------------------------------- the services
def _record_denoise_kw(net, waves, n_samples, sid, strength=0.01, out=None, **kw):
    net._engine.calls.append(("denoise_kw", kw))
    return one_shot_host._record_denoise(net, waves, n_samples, sid, strength, out)


class _KwNet(one_shot_host.DenoiseInferNet):
    denoise = _record_denoise_kw


def _batch_calls(net_cls, **svc_kw):
    net = net_cls()
    svc = one_shot_host._text_service(net, max_batch=3, **svc_kw)      # (a full batch: the worker waits for nothing)
    try:
        futs = [svc.submit(one_shot_host._row(), 1, denoise=True, loudness=dict(target_lufs=-16.0, peak_ceiling=0.8), limiter=True),
                svc.submit(one_shot_host._row("t"), 2, denoise=0.5), svc.submit(one_shot_host._row(), 3, loudness=-20.0)]
        got = [f.result(60).tobytes() for f in futs]
    finally:
        svc.close()
    return net._engine.calls, got


def test_batching_service_passes_the_transform_to_exactly_the_denoise_call():
    old, old_bytes = _batch_calls(one_shot_host.DenoiseInferNet)              # (its denoise takes no keyword at all)
    none, none_bytes = _batch_calls(_KwNet)
    dft, _ = _batch_calls(_KwNet, denoise_transform="dft")
    fft, fft_bytes = _batch_calls(_KwNet, denoise_transform="fft")
    assert [c[0] for c in old] == ["denoise", "loudness_normalize", "loudness_limit"]
    strip = lambda calls: [c for c in calls if c[0] != "denoise_kw"]
    assert strip(none) == strip(dft) == strip(fft) == old and old_bytes == none_bytes == fft_bytes
    assert [c for c in none if c[0] == "denoise_kw"] == [("denoise_kw", {})] == [c for c in dft if c[0] == "denoise_kw"]
    assert [c for c in fft if c[0] == "denoise_kw"] == [("denoise_kw", {"transform": "fft"})]
    assert fft.index(("denoise_kw", {"transform": "fft"})) + 1 == [c[0] for c in fft].index("denoise")
    with pytest.raises(ValueError, match="denoise_transform"):
        one_shot_host._text_service(_KwNet(), denoise_transform="fast")


class _KwStreamEngine(stream_host.StreamDenoiseEngine):
    def denoise_rows(self, rows, bias, **kw):
        self.calls.append(("denoise_rows_kw", kw))
        return super().denoise_rows(rows, bias)


class _KwStreamNet(stream_host.StreamDenoiseNet):
    def __init__(self):
        super().__init__()
        self._engine = _KwStreamEngine()
        self.bias_kw = []

    def denoiser_bias(self, sid, *a, **kw):
        self.bias_kw.append((a, kw))
        return super().denoiser_bias(sid)


def _stream_calls(net, **svc_kw):
    from vispeech_amd.service import StreamingBatchService
    paths_host = stream_host.paths_host
    svc = StreamingBatchService(net, collate=paths_host._collate, autostart=False, chunk_frames=4, **svc_kw)
    a = svc.submit({"id": 1, "frames": 30}, 1, denoise=0.5)
    b = svc.submit({"id": 2, "frames": 9}, 2)
    svc.step(); svc.step()
    c = svc.submit({"id": 3, "frames": 14}, 3, denoise=True, output_rate=8000, output_encoding="ulaw")
    svc.close()
    return net._engine.calls, [b"".join(paths_host._pieces(s)) for s in (a, b, c)]


def test_streaming_service_passes_the_transform_to_the_one_call_per_tick():
    old, old_bytes = _stream_calls(stream_host.StreamDenoiseNet())           # (stand-ins that take no keyword at all)
    nets = {k: _KwStreamNet() for k in ("none", "dft", "fft")}
    none, none_bytes = _stream_calls(nets["none"])
    dft, _ = _stream_calls(nets["dft"], denoise_transform="dft")
    fft, fft_bytes = _stream_calls(nets["fft"], denoise_transform="fft")
    strip = lambda calls: [c for c in calls if c[0] != "denoise_rows_kw"]
    key = lambda calls: [(c[0], repr(c[1:])) for c in calls]
    assert key(strip(none)) == key(strip(dft)) == key(strip(fft)) == key(old) and old_bytes == none_bytes == fft_bytes
    n = [c[0] for c in old].count("denoise_rows")
    assert n > 2
    assert [c for c in none if c[0] == "denoise_rows_kw"] == [("denoise_rows_kw", {})] * n == [c for c in dft if c[0] == "denoise_rows_kw"]
    assert [c for c in fft if c[0] == "denoise_rows_kw"] == [("denoise_rows_kw", {"transform": "fft"})] * n
    # each request's bias comes from the transform its stream runs on
    assert nets["none"].bias_kw == [((), {})] * 2 == nets["dft"].bias_kw and nets["fft"].bias_kw == [(("fft",), {})] * 2
    from vispeech_amd.service import StreamingBatchService
    with pytest.raises(ValueError, match="denoise_transform"):
        StreamingBatchService(_KwStreamNet(), collate=stream_host.paths_host._collate, autostart=False, denoise_transform="fast")
