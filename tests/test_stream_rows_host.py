"""Streaming for batched requests, host side (no GPU): the window plan of ``vsp_generator_stream_rows`` against a
brute-force plan, its argument checks, the exported symbols, and the scheduler of ``StreamingBatchService`` driven tick by
tick (``autostart=False``) over a recording stand-in for the engine."""
import ctypes as C

import numpy as np
import pytest

from vispeech_amd import _lib
from vispeech_amd.schema import ModelDims

HALO = 14           # vsp_generator_halo_frames of the default configuration


@pytest.fixture(scope="module")
def ctx():
    lib = _lib.lib()
    cfg = _lib.make_config(ModelDims())
    h = C.c_void_p()
    assert lib.vsp_create(C.byref(cfg), 0, C.byref(h)) == 0
    assert lib.vsp_generator_halo_frames(h) == HALO
    yield lib, h
    lib.vsp_destroy(h)


def _plan(lib, h, triples):
    n = len(triples)
    rows = (_lib.VspStreamRow * max(n, 1))()
    for r, (L, f0, f1) in zip(rows, triples):
        r.L, r.f0, r.f1 = L, f0, f1
    lo, hi, span = (C.c_int32 * max(n, 1))(), (C.c_int32 * max(n, 1))(), C.c_int32(-1)
    rc = lib.vsp_stream_rows_plan(h, n, rows, lo, hi, C.byref(span))
    return rc, list(lo)[:n], list(hi)[:n], span.value


def _brute(L, f0, f1):
    """The frames of [0, L) within HALO frames of a delivered frame, by enumeration."""
    win = [t for t in range(L) if any(abs(t - f) <= HALO for f in range(f0, f1))]
    return win[0], win[-1] + 1


def test_symbols_are_exported():
    lib = _lib.lib()
    for name in ("vsp_stream_rows_plan", "vsp_generator_stream_rows_workspace_bytes", "vsp_generator_stream_rows"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert C.sizeof(_lib.VspStreamRow) == 40          # two pointers, an int64, three int32 and the tail padding


@pytest.mark.parametrize("chunk", [1, 8, 16])
def test_plan_equals_brute_force(ctx, chunk):
    lib, h = ctx
    triples = [(L, f0, f1) for L in range(1, 41) for f0 in range(L) for f1 in range(f0 + 1, min(L, f0 + chunk) + 1)]
    assert len(triples) > 64
    for i in range(0, len(triples), 64):
        part = triples[i:i + 64]
        rc, lo, hi, span = _plan(lib, h, part)
        assert rc == 0
        want = [_brute(*t) for t in part]
        assert list(zip(lo, hi)) == want, part
        assert span == max(b - a for a, b in want)
        assert span <= chunk + 2 * HALO


def test_plan_refuses_bad_arguments(ctx):
    lib, h = ctx
    ok = (10, 2, 5)
    assert _plan(lib, h, [ok])[0] == 0
    assert _plan(lib, h, [])[0] == -1                            # B = 0
    assert _plan(lib, h, [ok] * 64)[0] == 0
    assert _plan(lib, h, [ok] * 65)[0] == -1                     # B = 65
    assert _plan(lib, h, [ok, (10, 2, 11)])[0] == -1             # f1 > L
    assert _plan(lib, h, [(10, 4, 4), ok])[0] == -1              # f0 == f1
    assert _plan(lib, h, [(10, -1, 4)])[0] == -1
    assert _plan(lib, h, [(0, 0, 0)])[0] == -1
    rows = (_lib.VspStreamRow * 1)()
    assert lib.vsp_stream_rows_plan(None, 1, rows, None, None, None) == -1
    assert lib.vsp_stream_rows_plan(h, 1, None, None, None, None) == -1
    rows[0].L, rows[0].f0, rows[0].f1 = ok
    assert lib.vsp_stream_rows_plan(h, 1, rows, None, None, None) == 0      # every output is optional


def test_workspace_size_and_call_order(ctx):
    lib, h = ctx
    w8, w16 = (lib.vsp_generator_stream_rows_workspace_bytes(h, 3, c) for c in (8, 16))
    gen = lib.vsp_generator_workspace_bytes(h, 3, 16 + 2 * HALO)
    d = ModelDims()
    extra = 3 * (16 + 2 * HALO) * 4 * (d.inter_channels + d.total_upsample) + 3 * 4 * d.gin_channels + 3 * 8
    assert 0 < w8 < w16 and gen + extra <= w16 <= gen + extra + 4 * 256 + 3 * d.inter_channels * 3 * 4
    assert lib.vsp_generator_stream_rows_workspace_bytes(h, 0, 16) == -1
    assert lib.vsp_generator_stream_rows_workspace_bytes(h, 65, 16) == -1
    assert lib.vsp_generator_stream_rows_workspace_bytes(h, 1, 0) == -1
    rows = (_lib.VspStreamRow * 1)()
    rc = lib.vsp_generator_stream_rows(h, None, 1, rows, C.c_void_p(8), 512, 1, C.c_void_p(8), 1 << 20)
    assert rc == -2 and b"not finalised" in lib.vsp_last_error(h)


# ---------------------------------------------------------------------------------------------- the scheduler
UP = 4


class FakeEngine:
    """Records what the service asks for.  A request is a dict(id, frames); its latent holds 100 * id + frame, and the
    'waveform' of a frame is UP copies of that number: the bytes name the request and the frame they belong to."""

    def __init__(self):
        self.calls, self.encodes = [], []

    def encode(self, phonemes, lengths, sid, duration, f0, energy, isolated=False):
        assert isolated
        ids = [int(x) for x in np.asarray(sid)]
        self.encodes.append(ids)
        if any(i < 0 for i in ids):
            raise RuntimeError("bad request")
        return {"frame_lengths": [int(x) for x in np.asarray(lengths)], "g": np.asarray(ids, np.float32).reshape(-1, 1),
                "ids": ids}

    def frame_lengths_host(self, fl):
        return list(fl), max(fl)

    def decode(self, enc, tf, noise, noise_scale, max_len=None, noise_seed=None, isolated=False):
        assert isolated and max_len == 0 and noise is None and len(noise_seed) == len(enc["ids"])
        z = np.stack([100 * i + np.arange(tf, dtype=np.float32)[None, :] for i in enc["ids"]])
        return {"z": z}

    def generator_stream_rows(self, rows, chunk_frames, pcm=True):
        assert pcm
        self.calls.append([(int(g[0]), L, f0, f1) for _, g, L, f0, f1 in rows])
        out = np.zeros((len(rows), chunk_frames * UP), np.int16)
        for b, (z, g, L, f0, f1) in enumerate(rows):
            assert 0 <= f0 < f1 <= L and f1 - f0 <= chunk_frames
            out[b, : (f1 - f0) * UP] = np.repeat(z[0, f0:f1], UP)
        return out


class FakeNet:
    class dims:
        total_upsample = UP

    def __init__(self):
        self._engine = FakeEngine()


def _collate(rows):
    return {"phonemes": np.zeros((len(rows), 1), np.int64), "lengths": np.asarray([r["frames"] for r in rows]),
            "sid": np.asarray([r["id"] for r in rows])}


def _service(**kw):
    from vispeech_amd.service import StreamingBatchService
    net = FakeNet()
    kw.setdefault("chunk_frames", 4)
    return StreamingBatchService(net, collate=_collate, autostart=False, **kw), net._engine


def _expect(rid, frames):
    return np.repeat(100 * rid + np.arange(frames), UP).astype("<i2").tobytes()


def _drain(stream):
    return b"".join(stream)


def test_a_request_submitted_while_idle_streams_alone():
    svc, eng = _service()
    a = svc.submit({"id": 1, "frames": 10}, 7)
    assert svc.step() and svc.step()
    assert next(a) == _expect(1, 10)[: 4 * UP * 2] and next(a) == _expect(1, 10)[4 * UP * 2: 8 * UP * 2]
    assert not svc.step()
    assert _drain(a) == _expect(1, 10)[8 * UP * 2:]
    assert eng.calls == [[(1, 10, 0, 4)], [(1, 10, 4, 8)], [(1, 10, 8, 10)]]
    assert svc.stats == {"ticks": 3, "rows_per_tick": [1, 1, 1], "groups": 1}


def test_a_late_request_shares_the_next_tick_and_may_finish_first():
    svc, eng = _service()
    a = svc.submit({"id": 1, "frames": 18}, 7)
    svc.step(); svc.step()
    b = svc.submit({"id": 2, "frames": 5}, 8)
    svc.step()
    assert svc.stats["rows_per_tick"] == [1, 1, 2] and svc.stats["groups"] == 2
    assert eng.calls[2] == [(1, 18, 8, 12), (2, 5, 0, 4)]           # each row at its own position
    svc.step()
    assert eng.calls[3] == [(1, 18, 12, 16), (2, 5, 4, 5)]
    assert _drain(b) == _expect(2, 5)                               # B is complete, A is not
    svc.step()
    assert eng.calls[4] == [(1, 18, 16, 18)]
    assert _drain(a) == _expect(1, 18)
    assert svc.stats["rows_per_tick"] == [1, 1, 2, 2, 1]


def test_closing_an_iterator_removes_its_row_at_the_next_tick():
    svc, eng = _service()
    a = svc.submit({"id": 1, "frames": 40}, 1)
    b = svc.submit({"id": 2, "frames": 12}, 2)
    svc.step()
    assert svc.stats["rows_per_tick"] == [2]
    a.close()
    svc.step(); svc.step()
    assert eng.calls[1:] == [[(2, 12, 4, 8)], [(2, 12, 8, 12)]]
    assert not svc.step() and svc.stats["ticks"] == 3
    assert _drain(b) == _expect(2, 12) and list(a) == []


def test_a_failing_admission_fails_only_its_group():
    svc, eng = _service()
    a = svc.submit({"id": 1, "frames": 10}, 1)
    svc.step()
    bad, bad2 = svc.submit({"id": -1, "frames": 6}, 2), svc.submit({"id": 3, "frames": 6}, 3)
    svc.step()
    assert eng.encodes == [[1], [-1, 3]] and svc.stats["rows_per_tick"] == [1, 1]
    for s in (bad, bad2):
        with pytest.raises(RuntimeError, match="bad request"):
            next(s)
        assert list(s) == []
    c = svc.submit({"id": 4, "frames": 3}, 4)                       # the service lives on
    svc.close()
    assert _drain(a) == _expect(1, 10) and _drain(c) == _expect(4, 3)


def test_max_batch_is_never_exceeded():
    svc, eng = _service(max_batch=3)
    streams = [svc.submit({"id": i, "frames": 4 + 4 * (i % 3)}, i) for i in range(1, 9)]
    svc.step()
    assert eng.encodes == [[1, 2, 3]]
    svc.close()
    assert max(svc.stats["rows_per_tick"]) == 3 and all(len(c) <= 3 for c in eng.calls)
    for i, s in enumerate(streams, start=1):
        assert _drain(s) == _expect(i, 4 + 4 * (i % 3))
    assert sum(svc.stats["rows_per_tick"]) == sum(-(-(4 + 4 * (i % 3)) // 4) for i in range(1, 9))
    with pytest.raises(RuntimeError):
        svc.submit({"id": 9, "frames": 4}, 9)


def test_a_zero_frame_request_yields_nothing_and_ends():
    svc, eng = _service()
    z, a = svc.submit({"id": 1, "frames": 0}, 1), svc.submit({"id": 2, "frames": 3}, 2)
    svc.step()
    assert list(z) == [] and eng.calls == [[(2, 3, 0, 3)]]
    assert _drain(a) == _expect(2, 3)
    alone = svc.submit({"id": 3, "frames": 0}, 3)                   # a group of nothing but silence: no decode, no tick
    assert not svc.step()
    assert list(alone) == [] and svc.stats["ticks"] == 1


def test_first_chunk_frames_shortens_the_first_chunk():
    svc, eng = _service(chunk_frames=8, first_chunk_frames=2)
    a = svc.submit({"id": 1, "frames": 13}, 1)
    svc.step()
    b = svc.submit({"id": 2, "frames": 20}, 2)
    svc.close()
    assert eng.calls[0] == [(1, 13, 0, 2)] and eng.calls[1] == [(1, 13, 2, 10), (2, 20, 0, 2)]
    first, second = next(a), next(a)
    assert len(first) == 2 * UP * 2 and len(second) == 8 * UP * 2          # (int16: two bytes per sample)
    assert first + second + _drain(a) == _expect(1, 13)
    assert _drain(b) == _expect(2, 20)


def test_worker_thread_serves_and_close_joins():
    from vispeech_amd.service import StreamingBatchService
    net = FakeNet()
    svc = StreamingBatchService(net, collate=_collate, chunk_frames=4)
    streams = [svc.submit({"id": i, "frames": 3 * i}, i) for i in range(1, 5)]
    got = [_drain(s) for s in streams]
    svc.close()
    assert got == [_expect(i, 3 * i) for i in range(1, 5)]
    assert not svc._worker.is_alive()
