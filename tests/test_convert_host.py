"""Conversion from audio, host side (no GPU): the exported symbols, ``vsp_convert_frames`` against enumeration, the
argument checks of the new entry points, and the schedulers of ``StreamingBatchService`` (``autostart=False``) and
``BatchingSynthesisService`` with conversion requests, over a recording stand-in for the engine."""
import ctypes as C

import numpy as np
import pytest
import torch

from vispeech_amd import _lib
from vispeech_amd.schema import ModelDims

NEW = ("vsp_convert_frames", "vsp_spectrogram_ragged_workspace_bytes", "vsp_spectrogram_ragged",
       "vsp_convert_latent_workspace_bytes", "vsp_convert_latent")
ERR_ARG, ERR_STATE = -1, -2


def _ctx(**cfg_fields):
    lib = _lib.lib()
    cfg = _lib.make_config(ModelDims())
    for k, v in cfg_fields.items():
        setattr(cfg, k, v)
    h = C.c_void_p()
    assert lib.vsp_create(C.byref(cfg), 0, C.byref(h)) == 0, lib.vsp_last_error(h)
    return lib, h


@pytest.fixture(scope="module")
def ctx():
    lib, h = _ctx()
    yield lib, h
    lib.vsp_destroy(h)


def test_symbols_are_exported_and_the_abi_is_unchanged():
    lib = _lib.lib()
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.vsp_abi_version() == _lib.ABI_VERSION == 7


# ---------------------------------------------------------------------------------------------- frame counts
def _brute_frames(n, n_fft, hop):
    """Offsets 0, hop, 2 hop, ... at which a full window fits into the reflect-padded signal of n + 2 pad samples; 0 where
    the reflect padding is undefined (n <= pad)."""
    pad = (n_fft - hop) // 2
    if n <= pad:
        return 0
    total, count, off = n + 2 * pad, 0, 0
    while off + n_fft <= total:
        count, off = count + 1, off + hop
    return count


def test_convert_frames_default_configuration(ctx):
    lib, h = ctx
    got = [lib.vsp_convert_frames(h, n, 512) for n in range(4097)]
    assert got == [_brute_frames(n, 2048, 512) for n in range(4097)]
    assert got[768] == 0 and got[769] == 1 and got[1023] == 1 and got[1024] == 2 and got[4096] == 8
    assert all(g == (0 if n <= 768 else n // 512) for n, g in enumerate(got))
    assert lib.vsp_convert_frames(h, 2 ** 33, 512) == 2 ** 33 // 512           # (an int64 sample count)


def test_convert_frames_where_the_window_is_shorter_than_three_hops():
    """spec_channels 641, hop 512: n_fft 1280 < 3 hop, pad 384 -- for n in 385..511 the padded signal is shorter than one
    window: 0 frames (vsp_spectrogram_frames' truncating division says 1 there; that entry stays as it is)."""
    lib, h = _ctx(spec_channels=641)
    try:
        got = [lib.vsp_convert_frames(h, n, 512) for n in range(4097)]
        assert got == [_brute_frames(n, 1280, 512) for n in range(4097)]
        assert not any(got[:512]) and got[512] == 1
        assert lib.vsp_spectrogram_frames(h, 400, 512) == 1                    # the edge this change does not touch
    finally:
        lib.vsp_destroy(h)


def test_convert_frames_refuses_bad_arguments(ctx):
    lib, h = ctx
    assert lib.vsp_convert_frames(h, -1, 512) == ERR_ARG
    assert lib.vsp_convert_frames(h, 4096, 0) == ERR_ARG
    assert lib.vsp_convert_frames(h, 4096, -512) == ERR_ARG
    assert lib.vsp_convert_frames(h, 4096, 2049) == ERR_ARG                    # n_fft < hop
    assert lib.vsp_convert_frames(None, 4096, 512) == ERR_ARG
    lib2, h2 = _ctx(spec_channels=0)
    try:
        assert lib2.vsp_convert_frames(h2, 4096, 512) == ERR_ARG
    finally:
        lib2.vsp_destroy(h2)


# ---------------------------------------------------------------------------------------------- argument checks
P = C.c_void_p(256)         # a non-null pointer no check dereferences


def _spec(lib, h, B=2, L=4096, hop=512, audio=P, stride=4096, n=P, spec=P, frames=P, ws=P):
    return lib.vsp_spectrogram_ragged(h, None, B, L, hop, audio, stride, n, spec, frames, ws, 1 << 40)


def _latent(lib, h, B=2, L=4096, hop=512, audio=P, stride=4096, n=P, src=P, tgt=P, noise=None, scale=1.0, z_hat=P, g=P,
            frames=P, mask=P, z=None, z_p=None, ws=P):
    return lib.vsp_convert_latent(h, None, B, L, hop, audio, stride, n, src, tgt, noise, scale, z_hat, g, frames, mask, z,
                                  z_p, ws, 1 << 40)


def test_argument_checks_answer_without_a_device(ctx):
    lib, h = ctx
    for size in (lib.vsp_spectrogram_ragged_workspace_bytes, lib.vsp_convert_latent_workspace_bytes):
        assert size(h, 2, 4096, 512) > 0
        assert size(h, 4, 4096, 512) > size(h, 2, 4096, 512)
        assert size(h, 0, 4096, 512) == ERR_ARG and size(h, -1, 4096, 512) == ERR_ARG
        assert size(h, 2, 4096, 0) == ERR_ARG
        assert size(h, 2, 768, 512) == ERR_ARG                # no frame in the padded shape
        assert size(None, 2, 4096, 512) == ERR_ARG
    assert lib.vsp_convert_latent_workspace_bytes(h, 2, 4096, 512) > lib.vsp_spectrogram_ragged_workspace_bytes(h, 2, 4096, 512)
    for call in (_spec, _latent):
        assert call(lib, None) == ERR_ARG
        assert call(lib, h, B=0) == ERR_ARG and call(lib, h, B=-3) == ERR_ARG
        assert call(lib, h, hop=0) == ERR_ARG
        assert call(lib, h, L=768) == ERR_ARG
        assert call(lib, h, stride=4095) == ERR_ARG           # audio_stride < L_max
        for name in ("audio", "n", "frames", "ws"):
            assert call(lib, h, **{name: None}) == ERR_ARG, name
        assert b"bad argument" in lib.vsp_last_error(h)
    assert _spec(lib, h, spec=None) == ERR_ARG
    for name in ("src", "tgt", "z_hat", "g", "mask"):
        assert _latent(lib, h, **{name: None}) == ERR_ARG, name
    assert _latent(lib, h, scale=float("nan")) == ERR_ARG
    # good arguments, no weights: the state is what is wrong
    assert _spec(lib, h) == ERR_STATE and b"not finalised" in lib.vsp_last_error(h)
    assert _latent(lib, h) == ERR_STATE and b"not finalised" in lib.vsp_last_error(h)


def test_a_context_without_spec_channels_is_refused():
    lib, h = _ctx(spec_channels=0)
    try:
        assert lib.vsp_spectrogram_ragged_workspace_bytes(h, 2, 4096, 512) == ERR_ARG
        assert lib.vsp_convert_latent_workspace_bytes(h, 2, 4096, 512) == ERR_ARG
        assert _spec(lib, h) == ERR_ARG and _latent(lib, h) == ERR_ARG
    finally:
        lib.vsp_destroy(h)


# ---------------------------------------------------------------------------------------------- the schedulers
UP, HOP, PAD = 4, 10, 15      # the stand-in's vocoder rate and its front end: T(n) = 0 up to PAD samples, n // HOP behind


class RecordingEngine:
    """Records what the services ask for.  A text request is a dict(id, frames), a conversion a recording of n samples from
    speaker src to tgt; a request's latent holds (100 * id + frame) / 32767 with id = the text request's id or the target
    speaker, so that the PCM16 names the request and the frame."""

    def __init__(self):
        self.calls = []

    # -- text
    def encode(self, phonemes, lengths, sid, duration, f0, energy, isolated=False):
        assert isolated
        ids = [int(x) for x in np.asarray(sid)]
        self.calls.append(("encode", ids))
        return {"frame_lengths": [int(x) for x in np.asarray(lengths)],
                "g": torch.tensor(ids, dtype=torch.float32).reshape(-1, 1), "ids": ids}

    def frame_lengths_host(self, fl):
        self.calls.append(("frame_lengths_host",))
        return list(fl), max(fl)

    def decode(self, enc, tf, noise, noise_scale, max_len=None, noise_seed=None, isolated=False):
        assert isolated and max_len == 0 and noise is None
        self.calls.append(("decode", list(noise_seed)))
        return {"z": torch.stack([(100 * i + torch.arange(tf, dtype=torch.float32))[None, :] / 32767.0 for i in enc["ids"]])}

    # -- conversion
    def convert_frames(self, n):
        return 0 if n <= PAD else n // HOP

    def convert_latent(self, audio, n_samples, sid_src, sid_tgt, noise=None, noise_seed=None, noise_scale=1.0):
        n = [int(x) for x in n_samples]
        assert noise is None and audio.shape == (len(n), max(n)) and audio.dtype == np.float32
        self.calls.append(("convert_latent", n, list(sid_src), list(sid_tgt), list(noise_seed), float(noise_scale)))
        if any(s < 0 for s in sid_src):
            raise RuntimeError("bad recording")
        frames = [self.convert_frames(x) for x in n]
        T = max(frames)
        z = torch.stack([(100 * t + torch.arange(T, dtype=torch.float32))[None, :] / 32767.0 for t in sid_tgt])
        return {"z_hat": z, "g": torch.tensor(list(sid_tgt), dtype=torch.float32).reshape(-1, 1), "frames_host": frames}

    # -- vocoder
    def generator_stream_rows(self, rows, chunk_frames, pcm=True):
        assert pcm
        self.calls.append(("generator_stream_rows", [(int(g[0]), L, f0, f1) for _, g, L, f0, f1 in rows]))
        out = np.zeros((len(rows), chunk_frames * UP), np.int16)
        for b, (z, g, L, f0, f1) in enumerate(rows):
            assert 0 <= f0 < f1 <= L and f1 - f0 <= chunk_frames
            out[b, : (f1 - f0) * UP] = np.repeat(np.rint(z[0, f0:f1].numpy() * 32767.0), UP)
        return out

    def generator_ragged(self, z, g, lengths):
        self.calls.append(("generator_ragged", [int(x) for x in g.reshape(-1)], list(lengths), tuple(z.shape)))
        for b, L in enumerate(lengths):
            assert not z[b, :, L:].any()
        return torch.repeat_interleave(z[:, :1, :], UP, dim=2)


class RecordingNet:
    class dims:
        total_upsample = UP

    device = "cpu"

    def __init__(self):
        self._engine = RecordingEngine()

    def infer(self, phonemes, lengths, sid=None, noise_scale=1, duration_control=None, pitch_control=None,
              energy_control=None, noise_seed=None, isolated=False):
        assert isolated
        ids, fl = [int(x) for x in sid], [int(x) for x in lengths]
        self._engine.calls.append(("infer", ids, list(noise_seed)))
        tf = max(fl)
        o = torch.stack([torch.repeat_interleave((100 * i + torch.arange(tf, dtype=torch.float32)) / 32767.0, UP)[None, :]
                         for i in ids])
        x_mask = (torch.arange(tf)[None, None, :] < torch.tensor(fl)[:, None, None])
        return o, x_mask


def _collate(rows):
    return {"phonemes": np.zeros((len(rows), 1), np.int64), "lengths": np.asarray([r["frames"] for r in rows]),
            "sid": np.asarray([r["id"] for r in rows])}


def _expect(rid, frames):
    return np.repeat(100 * rid + np.arange(frames), UP).astype("<i2").tobytes()


def _streaming(**kw):
    from vispeech_amd.service import StreamingBatchService
    net = RecordingNet()
    kw.setdefault("chunk_frames", 4)
    return StreamingBatchService(net, collate=_collate, autostart=False, **kw), net._engine


def _audio(n):
    return np.linspace(-0.5, 0.5, n, dtype=np.float32)


def test_streaming_mixed_group_one_convert_latent_and_shared_ticks():
    svc, eng = _streaming()
    a = svc.submit({"id": 1, "frames": 6}, 7)
    c1 = svc.submit_conversion(_audio(93), 3, 5, 21)               # 9 frames, to speaker 5
    b = svc.submit({"id": 2, "frames": 3}, 8)
    c2 = svc.submit_conversion(_audio(50), 4, 6, 22)               # 5 frames, to speaker 6
    svc.close()
    assert eng.calls == [
        ("encode", [1, 2]), ("frame_lengths_host",), ("decode", [7, 8]),
        ("convert_latent", [93, 50], [3, 4], [5, 6], [21, 22], 1.0),
        ("generator_stream_rows", [(1, 6, 0, 4), (5, 9, 0, 4), (2, 3, 0, 3), (6, 5, 0, 4)]),
        ("generator_stream_rows", [(1, 6, 4, 6), (5, 9, 4, 8), (6, 5, 4, 5)]),
        ("generator_stream_rows", [(5, 9, 8, 9)]),
    ]
    assert svc.stats == {"ticks": 3, "rows_per_tick": [4, 3, 1], "groups": 1}
    assert b"".join(a) == _expect(1, 6) and b"".join(b) == _expect(2, 3)
    assert b"".join(c1) == _expect(5, 9) and b"".join(c2) == _expect(6, 5)


def test_streaming_text_only_group_makes_the_calls_it_always_made():
    """The sequence below is what the service made for this group before it knew conversion requests."""
    svc, eng = _streaming()
    a, b = svc.submit({"id": 1, "frames": 6}, 7), svc.submit({"id": 2, "frames": 3}, 8)
    svc.close()
    assert eng.calls == [
        ("encode", [1, 2]), ("frame_lengths_host",), ("decode", [7, 8]),
        ("generator_stream_rows", [(1, 6, 0, 4), (2, 3, 0, 3)]),
        ("generator_stream_rows", [(1, 6, 4, 6)]),
    ]
    assert b"".join(a) == _expect(1, 6) and b"".join(b) == _expect(2, 3)


def test_streaming_conversion_only_group_and_its_noise_scale():
    svc, eng = _streaming(first_chunk_frames=2)
    c = svc.submit_conversion(_audio(70), 1, 2, 5, noise_scale=0.5)
    svc.close()
    assert eng.calls[0] == ("convert_latent", [70], [1], [2], [5], 0.5)          # no encode, no decode
    assert [k[0] for k in eng.calls[1:]] == ["generator_stream_rows"] * 3
    assert eng.calls[1][1] == [(2, 7, 0, 2)] and eng.calls[2][1] == [(2, 7, 2, 6)]
    assert [len(p) for p in c] == [2 * UP * 2, 4 * UP * 2, 1 * UP * 2]


def test_streaming_zero_frame_recording_ends_with_no_bytes():
    svc, eng = _streaming()
    z, c = svc.submit_conversion(_audio(PAD), 1, 2, 5), svc.submit_conversion(_audio(40), 1, 3, 6)
    svc.step()
    assert list(z) == []
    assert eng.calls[0] == ("convert_latent", [40], [1], [3], [6], 1.0)          # the short one never reaches the device
    svc.close()
    assert b"".join(c) == _expect(3, 4)
    svc2, eng2 = _streaming()
    alone = svc2.submit_conversion(_audio(3), 1, 2, 5)
    assert not svc2.step()
    assert list(alone) == [] and eng2.calls == [] and svc2.stats["ticks"] == 0


def test_streaming_failing_convert_latent_fails_only_its_group():
    svc, eng = _streaming()
    a = svc.submit({"id": 1, "frames": 10}, 1)
    svc.step()
    bad, bad2 = svc.submit_conversion(_audio(40), -1, 2, 5), svc.submit({"id": 3, "frames": 6}, 3)
    svc.step()
    for s in (bad, bad2):
        with pytest.raises(RuntimeError, match="bad recording"):
            next(s)
        assert list(s) == []
    assert svc.stats["rows_per_tick"] == [1, 1]
    c = svc.submit_conversion(_audio(30), 1, 4, 6)                                # the service lives on
    svc.close()
    assert b"".join(a) == _expect(1, 10) and b"".join(c) == _expect(4, 3)


def _batching(**kw):
    from vispeech_amd.service import BatchingSynthesisService
    net = RecordingNet()
    return BatchingSynthesisService(net, max_wait_s=30.0, collate=_collate, **kw), net._engine


def test_batching_mixed_batch_one_convert_latent_one_generator_call():
    svc, eng = _batching(max_batch=5)
    try:
        futs = [svc.submit({"id": 1, "frames": 6}, 7), svc.submit_conversion(_audio(93), 3, 5, 21),
                svc.submit_conversion(_audio(PAD), 3, 9, 23), svc.submit({"id": 2, "frames": 3}, 8),
                svc.submit_conversion(_audio(50), 4, 6, 22, noise_scale=1.0)]
        got = [f.result(60) for f in futs]
    finally:
        svc.close()
    assert eng.calls == [
        ("encode", [1, 2]), ("frame_lengths_host",), ("decode", [7, 8]),
        ("convert_latent", [93, 50], [3, 4], [5, 6], [21, 22], 1.0),
        ("generator_ragged", [1, 5, 2, 6], [6, 9, 3, 5], (4, 1, 9)),
    ]
    want = [_expect(1, 6), _expect(5, 9), b"", _expect(2, 3), _expect(6, 5)]
    assert [g.tobytes() for g in got] == want and all(g.dtype == np.dtype("<i2") for g in got)


def test_batching_text_only_batch_makes_the_call_it_always_made():
    """One ``net.infer`` with the requests' seeds: the sequence the service made before it knew conversion requests."""
    svc, eng = _batching(max_batch=2)
    try:
        futs = [svc.submit({"id": 1, "frames": 6}, 7), svc.submit({"id": 2, "frames": 3}, 8)]
        got = [f.result(60) for f in futs]
    finally:
        svc.close()
    assert eng.calls == [("infer", [1, 2], [7, 8])]
    assert [g.tobytes() for g in got] == [_expect(1, 6), _expect(2, 3)]


def test_batching_failing_convert_latent_fails_only_its_batch():
    svc, eng = _batching(max_batch=2)
    try:
        bad = [svc.submit_conversion(_audio(40), -1, 2, 5), svc.submit({"id": 3, "frames": 6}, 3)]
        for f in bad:
            with pytest.raises(RuntimeError, match="bad recording"):
                f.result(60)
        ok = [svc.submit_conversion(_audio(30), 1, 4, 6), svc.submit_conversion(_audio(20), 1, 7, 7, noise_scale=0.25)]
        got = [f.result(60) for f in ok]
    finally:
        svc.close()
    assert [g.tobytes() for g in got] == [_expect(4, 3), _expect(7, 2)]
    assert [c for c in eng.calls if c[0] == "convert_latent"][1:] == [
        ("convert_latent", [20], [1], [7], [7], 0.25), ("convert_latent", [30], [1], [4], [6], 1.0)]


def test_conversion_requests_are_checked_at_submit():
    svc, _ = _streaming()
    with pytest.raises(ValueError):
        svc.submit_conversion(np.zeros((2, 40), np.float32), 1, 2, 5)
    svc.close()
    with pytest.raises(RuntimeError):
        svc.submit_conversion(_audio(40), 1, 2, 5)
