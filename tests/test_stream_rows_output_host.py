"""The ragged output stage of streamed batches, host side (no GPU): ``vsp_stream_rows_output_plan`` against the rule of
``vispeech_amd/output_stage.py`` by enumeration, the two size bounds against a simulation of that rule, the argument
refusals that need no device, and the ``fused_output`` scheduler of ``StreamingBatchService`` over a recording stand-in for
the engine whose numpy resampler follows the same rule."""
import ctypes as C

import numpy as np
import pytest

from vispeech_amd import _lib, output_stage
from vispeech_amd.schema import ModelDims

NEW_SYMBOLS = ("vsp_stream_rows_output_plan", "vsp_output_history_samples", "vsp_stream_rows_out_samples",
               "vsp_generator_stream_rows_output")
# (in_rate, out_rate, zeros): the L = 1 path, more outputs than inputs, a long filter, a history longer than a frame
PLANS = [(44100, 22050, 32), (44100, 48000, 32), (44100, 8000, 32), (44100, 8000, 64)]


def test_symbols_are_exported():
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert C.sizeof(_lib.VspStreamRow) == 40 and C.sizeof(_lib.VspStreamRowOut) == 56
    assert lib.vsp_abi_version() == 7


def _plan(lib, lmh, up, triples):
    n = len(triples)
    rows = (_lib.VspStreamRow * max(n, 1))()
    for r, (Lf, f0, f1) in zip(rows, triples):
        r.L, r.f0, r.f1 = Lf, f0, f1
    res = [(C.c_int64 * max(n, 1))() for _ in range(4)]
    rc = lib.vsp_stream_rows_output_plan(*lmh, up, n, rows, *res)
    return rc, [list(a)[:n] for a in res]


def _expected(lmh, up, Lf, f0, f1):
    x_first, x_end = f0 * up, f1 * up
    m0 = output_stage.complete_outputs(x_first, *lmh)
    m1 = output_stage.complete_outputs(x_end, *lmh, ended=f1 == Lf)
    return (m0, m1, min(x_first, output_stage.history_start(m0, *lmh)), min(x_end, output_stage.history_start(m1, *lmh)))


@pytest.mark.parametrize("up", [4, 512])
@pytest.mark.parametrize("rates", PLANS, ids=lambda p: f"{p[1]}z{p[2]}")
def test_plan_equals_the_rule_of_output_stage(rates, up):
    lib = _lib.lib()
    lmh = output_stage.plan(*rates)
    # every (Lf, f0, f1) with Lf <= 12 and a chunk of up to 5 frames: the chunks of 1, 2 and 5 frames at every position
    triples = [(Lf, f0, f1) for Lf in range(1, 13) for f0 in range(Lf) for f1 in range(f0 + 1, min(Lf, f0 + 5) + 1)]
    got = {}
    for i in range(0, len(triples), 64):
        part = triples[i:i + 64]
        rc, (m0, m1, k0, k1) = _plan(lib, lmh, up, part)
        assert rc == 0
        for t, *g in zip(part, m0, m1, k0, k1):
            assert tuple(g) == _expected(lmh, up, *t), (t, g)
            got[t] = tuple(g)
    L, M, H = lmh
    for (Lf, f0, f1), (m0, m1, k0, k1) in got.items():
        assert 0 <= m0 <= m1 and 0 <= k0 <= f0 * up and k0 <= k1 <= f1 * up
        if f1 == Lf:
            assert m1 == -(-Lf * up * L // M)                            # the final tick flushes the tail
        for g0 in range(max(0, f0 - 5), f0):                             # m0 is the m1 of whichever row ended at f0
            assert got[(Lf, g0, f0)][1] == m0 and got[(Lf, g0, f0)][3] == k0
    if up == 4 and H > 0:
        assert any(m1 == m0 for m0, m1, _, _ in got.values()), "no tick without output among the cases"
    assert any(m1 > m0 for m0, m1, _, _ in got.values())


def _simulate(lmh, up, Lf, chunk):
    """The rule of output_stage.stream, tick by tick: (longest history kept, most outputs of one tick)."""
    seen = m_next = hist = most = 0
    for f0 in range(0, Lf, chunk):
        f1 = min(Lf, f0 + chunk)
        seen = f1 * up
        m_done = output_stage.complete_outputs(seen, *lmh, ended=f1 == Lf)
        most, m_next = max(most, m_done - m_next), m_done
        hist = max(hist, seen - min(seen, output_stage.history_start(m_next, *lmh)))
    return hist, most


@pytest.mark.parametrize("rates", PLANS + [(44100, r, 32) for r in (16000, 24000, 11025, 32000, 44100)],
                         ids=lambda p: f"{p[1]}z{p[2]}")
def test_size_bounds_cover_a_simulation(rates):
    lib = _lib.lib()
    L, M, H = lmh = output_stage.plan(*rates)
    K = lib.vsp_output_history_samples(L, M, H)
    assert K == 2 * H // L
    want = {(22050, 32): 128, (8000, 32): 352, (8000, 64): 705, (44100, 32): 0}.get(rates[1:])
    assert want is None or K == want
    for up in (4, 512):
        for chunk in (1, 2, 16):
            bound = lib.vsp_stream_rows_out_samples(L, M, H, up, chunk)
            n = chunk * up
            assert bound % 4 == 0 and 0 <= bound - (-(-n * L // M) + -(-H // M)) < 4
            for Lf in (1, 2, 3, 16, 17, 33, 40):
                hist, most = _simulate(lmh, up, Lf, chunk)
                assert hist <= K, (up, chunk, Lf, hist, K)
                assert most <= bound, (up, chunk, Lf, most, bound)


def test_bad_arguments_are_refused():
    lib = _lib.lib()
    lmh, ok = (1, 2, 64), (10, 2, 5)
    assert _plan(lib, lmh, 512, [ok])[0] == 0
    assert _plan(lib, lmh, 512, [])[0] == -1                                  # B = 0
    assert _plan(lib, lmh, 512, [ok] * 64)[0] == 0
    assert _plan(lib, lmh, 512, [ok] * 65)[0] == -1                           # B = 65
    for bad in ((10, 2, 11), (10, 4, 4), (10, -1, 4), (0, 0, 0)):             # f1 > L, empty, f0 < 0, no frames
        assert _plan(lib, lmh, 512, [ok, bad])[0] == -1, bad
    for bad_lmh, up in (((0, 2, 64), 512), ((1, 0, 64), 512), ((1, 2, -1), 512), (lmh, 0)):
        assert _plan(lib, bad_lmh, up, [ok])[0] == -1
    rows = (_lib.VspStreamRow * 1)()
    rows[0].L, rows[0].f0, rows[0].f1 = ok
    assert lib.vsp_stream_rows_output_plan(1, 2, 64, 512, 1, None, None, None, None, None) == -1
    assert lib.vsp_stream_rows_output_plan(1, 2, 64, 512, 1, rows, None, None, None, None) == 0     # every output is optional
    assert lib.vsp_output_history_samples(0, 2, 64) == -1 and lib.vsp_output_history_samples(1, 2, -1) == -1
    assert lib.vsp_output_history_samples(1, 1, 0) == 0
    for args in ((0, 2, 64, 512, 8), (1, 0, 64, 512, 8), (1, 2, -1, 512, 8), (1, 2, 64, 0, 8), (1, 2, 64, 512, 0)):
        assert lib.vsp_stream_rows_out_samples(*args) == -1, args
    # the call itself: nothing runs on a context without weights
    cfg = _lib.make_config(ModelDims())
    h = C.c_void_p()
    assert lib.vsp_create(C.byref(cfg), 0, C.byref(h)) == 0
    try:
        orows = (_lib.VspStreamRowOut * 1)()
        rc = lib.vsp_generator_stream_rows_output(h, None, 1, orows, C.c_void_p(8), 512, 1, C.c_void_p(8), 1 << 20)
        assert rc == -2 and b"not finalised" in lib.vsp_last_error(h)
    finally:
        lib.vsp_destroy(h)


# ---------------------------------------------------------------------------------------------- the scheduler
UP = 4
LMH = (1, 2, 5)                                          # the stand-in stage: decimation by 2, eleven integer taps
TAPS = np.asarray([1, 2, 3, 4, 5, 6, 5, 4, 3, 2, 1], np.int64)       # h[-5 .. 5]
K = 2 * LMH[2] // LMH[0]


def resample_ref(x, m0, m1, sample_first=0):
    """y[m] = sum_k h[m M - k L] x[k] for m in [m0, m1), x holding samples [sample_first, ...), zero outside."""
    L, M, H = LMH
    y = np.zeros(m1 - m0, np.int64)
    for m in range(m0, m1):
        for k in range(-(-(m * M - H) // L), (m * M + H) // L + 1):
            if sample_first <= k < sample_first + len(x):
                y[m - m0] += TAPS[m * M - k * L + H] * int(x[k - sample_first])
    return y


class FakeHistory:
    def __init__(self, tag):
        self.buf, self.side, self.tag = [np.full(K, -7777, np.int64), np.full(K, -7777, np.int64)], 0, tag


class FakeEngine:
    """Records what the service asks for.  A request is a dict(id, frames); its latent holds 10 * id + frame and the
    'waveform' of a frame is UP copies of that number.  ``generator_stream_rows_output`` filters it with the rule of
    output_stage.py, reading and writing the request's history sides like the library does."""

    output_plan = LMH

    def __init__(self):
        self.calls, self.histories, self.configured = [], 0, []

    def configure_output(self, out_rate, in_rate=None):
        self.configured.append((out_rate, in_rate))

    def encode(self, phonemes, lengths, sid, duration, f0, energy, isolated=False):
        ids = [int(x) for x in np.asarray(sid)]
        return {"frame_lengths": [int(x) for x in np.asarray(lengths)], "g": np.asarray(ids, np.float32).reshape(-1, 1),
                "ids": ids}

    def frame_lengths_host(self, fl):
        return list(fl), max(fl)

    def decode(self, enc, tf, noise, noise_scale, max_len=None, noise_seed=None, isolated=False):
        return {"z": np.stack([10 * i + np.arange(tf, dtype=np.float32)[None, :] for i in enc["ids"]])}

    def output_history(self):
        self.histories += 1
        return FakeHistory(self.histories)

    def generator_stream_rows_output(self, rows, chunk_frames, pcm=True):
        assert pcm
        L, M, H = LMH
        width = -(-chunk_frames * UP * L // M) + -(-H // M)
        out, counts, call = np.zeros((len(rows), width), np.int16), [], []
        for b, (z, g, Lf, f0, f1, st) in enumerate(rows):
            assert 0 <= f0 < f1 <= Lf and f1 - f0 <= chunk_frames
            x_first, x_end = f0 * UP, f1 * UP
            m0, m1 = output_stage.complete_outputs(x_first, L, M, H), output_stage.complete_outputs(x_end, L, M, H, f1 == Lf)
            k0 = min(x_first, output_stage.history_start(m0, L, M, H))
            k1 = min(x_end, output_stage.history_start(m1, L, M, H))
            window = np.concatenate([st.buf[st.side][: x_first - k0], np.repeat(z[0, f0:f1], UP).astype(np.int64)])
            out[b, : m1 - m0] = resample_ref(window, m0, m1, k0)
            st.buf[1 - st.side][:] = -7777
            st.buf[1 - st.side][: x_end - k1] = window[k1 - k0:]
            call.append((int(g[0]), Lf, f0, f1, (st.tag, st.side), (st.tag, 1 - st.side)))
            st.side = 1 - st.side
            counts.append(m1 - m0)
        self.calls.append(call)
        return out, counts

    def generator_stream_rows(self, *a, **k):
        raise AssertionError("the fused tick must not run the collect path")

    def output_stream(self, *a, **k):
        raise AssertionError("the fused tick must not run a per-request output stream")

    output_chunk = output_stream


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
    svc = StreamingBatchService(net, collate=_collate, autostart=False, output_rate=22050, fused_output=True, **kw)
    assert net._engine.configured == [(22050, 44100)]
    return svc, net._engine


def _expect(rid, frames):
    x = np.repeat(10 * rid + np.arange(frames), UP)
    return resample_ref(x, 0, -(-len(x) * LMH[0] // LMH[1])).astype("<i2").tobytes()


def test_fused_output_needs_an_output_rate():
    from vispeech_amd.service import StreamingBatchService
    with pytest.raises(ValueError, match="fused_output"):
        StreamingBatchService(FakeNet(), collate=_collate, autostart=False, fused_output=True)


def test_one_call_per_tick_and_the_bytes_of_the_one_shot_stage():
    svc, eng = _service()
    a = svc.submit({"id": 1, "frames": 18}, 7)
    svc.step(); svc.step()
    b = svc.submit({"id": 2, "frames": 5}, 8)
    c = svc.submit({"id": 3, "frames": 1}, 9)                          # ends in its first tick: no history, the whole tail
    svc.close()
    assert svc.stats["rows_per_tick"] == [1, 1, 3, 2, 1] and len(eng.calls) == svc.stats["ticks"] == 5
    assert [[r[:4] for r in call] for call in eng.calls] == [
        [(1, 18, 0, 4)], [(1, 18, 4, 8)], [(1, 18, 8, 12), (2, 5, 0, 4), (3, 1, 0, 1)], [(1, 18, 12, 16), (2, 5, 4, 5)],
        [(1, 18, 16, 18)]]
    for s, (rid, frames) in ((a, (1, 18)), (b, (2, 5)), (c, (3, 1))):
        assert b"".join(s) == _expect(rid, frames), rid
    # a request's history: one object from admission on, each tick reads the side the previous tick wrote
    per_request = {}
    for call in eng.calls:
        for rid, _, _, _, h_in, h_out in call:
            per_request.setdefault(rid, []).append((h_in, h_out))
    assert eng.histories == 3 and len({hs[0][0][0] for hs in per_request.values()}) == 3
    for hs in per_request.values():
        assert all(i[0] == o[0] and i[1] != o[1] for i, o in hs)
        assert all(nxt[0] == prev[1] for prev, nxt in zip(hs, hs[1:]))


def test_a_tick_without_output_puts_nothing_on_the_queue():
    svc, eng = _service(chunk_frames=1)
    assert output_stage.complete_outputs(UP, *LMH) == 0               # H = 5: the first frame's 4 samples complete nothing
    a = svc.submit({"id": 4, "frames": 3}, 1)
    svc.close()
    pieces = list(a)
    assert len(eng.calls) == 3 and len(pieces) == 2 and all(pieces)    # three ticks, two pieces, none of them empty
    assert b"".join(pieces) == _expect(4, 3)


def test_closing_an_iterator_releases_its_row():
    svc, eng = _service()
    a = svc.submit({"id": 1, "frames": 40}, 1)
    b = svc.submit({"id": 2, "frames": 12}, 2)
    svc.step()
    a.close()
    svc.close()
    assert [[r[:4] for r in call] for call in eng.calls[1:]] == [[(2, 12, 4, 8)], [(2, 12, 8, 12)]]
    assert b"".join(b) == _expect(2, 12) and list(a) == []
    assert svc.stats["ticks"] == 3


def test_max_batch_and_many_requests():
    svc, eng = _service(max_batch=3)
    streams = [svc.submit({"id": i, "frames": 3 + 4 * (i % 3)}, i) for i in range(1, 9)]
    svc.close()
    assert max(svc.stats["rows_per_tick"]) == 3 and all(len(c) <= 3 for c in eng.calls)
    for i, s in enumerate(streams, start=1):
        assert b"".join(s) == _expect(i, 3 + 4 * (i % 3)), i
