"""The true-peak meter and the look-ahead limiter without a GPU: the restatement's own properties,
the library's host-only calls against it, every refusal of ``vsp_limiter_rows`` (decided on the host before any launch),
``limiter.Stream``'s bookkeeping against a numpy stand-in engine, and both services with recording stand-ins: which calls a
batch or a tick makes, that a request without a limiter gets its old bytes, and that nobody naming one means the old calls.

Two of the properties are stated with the slack the specification itself has.  ``s <= r`` holds in exact arithmetic with
the exact reciprocal; the specification's reciprocal is ONE float32 constant, off by at most 2^-24 relative, so the fp64
run shows s <= r (1 + 2^-23).  For the same reason the fp64 run's s where nothing exceeds the ceiling is 1 within 2^-24,
while the float32 run's is 1 exactly at every attack the tests use (fl32((A + 1) fl32(1 / (A + 1))) = 1 there)."""
import ctypes as C

import numpy as np
import pytest

import limiter_ref as lr
import test_abi
from vispeech_amd import _lib, limiter
from vispeech_amd.schema import ModelDims

NEW = ("vsp_true_peak_filter", "vsp_limiter_history", "vsp_limiter_workspace_bytes", "vsp_true_peak", "vsp_limiter_rows")
WINDOWS = ((66, 882), (0, 0), (1, 0), (16, 100), (1024, 8192))
NAN = float("nan")


def test_symbols_and_abi():
    lib = _lib.lib()
    for s in NEW:
        assert hasattr(lib, s) and s in _lib.SIGNATURES, s
    assert lib.vsp_abi_version() == 7
    assert sorted(_lib.SIGNATURES) == test_abi.header_symbols()
    assert C.sizeof(_lib.VspLimiterRow) == 64


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("A,H", WINDOWS)
def test_the_restatements_own_properties(A, H):
    for name, x, g, c in lr.fixture_rows():
        d, f = lr.limit(x, g, c, A, H), lr.limit(x, g, c, A, H, np.float32)
        assert np.all(d["s"] <= d["r"] * (1.0 + 2.0 ** -23)), name
        assert np.abs(d["out"]).max() <= np.float32(c) and np.abs(f["out"]).max() <= np.float32(c), name
        assert f["out"].dtype == np.float32
        if name in ("silence", "never_limited"):
            assert np.all(d["r"] == 1.0) and np.abs(d["s"] - 1.0).max() <= 2.0 ** -24
            assert np.all(f["s"] == 1.0) and np.array_equal(f["out"], np.float32(g) * x), name
        else:
            assert d["min_gain"] < 1.0, name
    # two peaks closer than the attack: the gain does not recover between them
    name, x, g, c = lr.fixture_rows()[6]
    d = lr.limit(x, g, c, 66, 0)
    assert name == "two_peaks" and d["s"][600:631].max() < 0.75


def test_the_fs4_sine_reads_its_amplitude():
    """EBU Tech 3341's meter tolerance: +0.2 / -0.4 dB.  The row's first samples overshoot (the sine starts abruptly):
    +0.09 dB; away from the ends the reading is -0.001 dB."""
    x = lr.fs4_sine(2000)
    assert abs(lr.db(np.abs(x).max()) + 3.0103) < 1e-3
    for dtype in (np.float64, np.float32):
        p = lr.peaks(x, dtype)
        assert -0.4 <= lr.db(p.max()) <= 0.2
        assert abs(lr.db(p[100:1900].max()) + 0.0012) < 5e-4
    click = np.zeros(50, np.float32)
    click[20] = 1.0
    assert lr.true_peak(click) == 1.0                       # the low-pass attenuates a lone click: |x| is in the maximum


def test_the_librarys_taps_are_the_formulas():
    got = np.zeros(97, np.float32)
    assert _lib.lib().vsp_true_peak_filter(got.ctypes.data_as(C.POINTER(C.c_float))) == 0
    want = lr.taps64()
    assert np.abs(got.astype(np.float64) - want).max() <= 2.0 ** -24 and got[48] == np.float32(4 * (1 - 3.065 / 12) / 4)
    assert np.array_equal(got, got[::-1]) and np.count_nonzero(got != lr.taps()) <= 2      # (libm against numpy: a last place)
    assert _lib.lib().vsp_true_peak_filter(None) == -1


def test_history_and_workspace():
    lib = _lib.lib()
    b, a = C.c_int64(), C.c_int64()
    for A, H in WINDOWS:
        assert lib.vsp_limiter_history(A, H, C.byref(b), C.byref(a)) == 0
        assert (b.value, a.value) == (A + H + 12, A + 12) == lr.history(A, H)
    for A, H in ((-1, 0), (1025, 0), (0, -1), (0, 8193)):
        assert lib.vsp_limiter_history(A, H, C.byref(b), C.byref(a)) == -1
        assert lib.vsp_limiter_workspace_bytes(1, 9, A, H) == -1
    assert lib.vsp_limiter_history(0, 0, None, C.byref(a)) == -1
    for B in (1, 2, 17):
        for L in (1, 63, 64, 2048, 44100, 1 << 24):
            for A, H in WINDOWS:
                v = lib.vsp_limiter_workspace_bytes(B, L, A, H)
                assert v >= B * (L + 2 * A + H) * 4
                assert lib.vsp_limiter_workspace_bytes(B + 1, L, A, H) > v and lib.vsp_limiter_workspace_bytes(B, L + 1, A, H) >= v
                assert lib.vsp_limiter_workspace_bytes(B, L + 64, A, H) > v
                if A < 1024 and H < 8192:
                    assert lib.vsp_limiter_workspace_bytes(B, L, A + 1, H) >= v and lib.vsp_limiter_workspace_bytes(B, L, A, H + 1) >= v
                    assert lib.vsp_limiter_workspace_bytes(B, L, A + 32, H) > v and lib.vsp_limiter_workspace_bytes(B, L, A, H + 64) > v
    assert lib.vsp_limiter_workspace_bytes(0, 9, 0, 0) == -1 and lib.vsp_limiter_workspace_bytes(1, 0, 0, 0) == -1
    assert lib.vsp_limiter_workspace_bytes(1, (1 << 30) + 1, 0, 0) == -1


# ---------------------------------------------------------------------------------------------- refusals
@pytest.fixture()
def ctx():
    lib = _lib.lib()
    cfg = _lib.make_config(ModelDims())
    h = C.c_void_p()
    assert lib.vsp_create(C.byref(cfg), 0, C.byref(h)) == 0
    yield lib, h
    lib.vsp_destroy(h)


BAD = 8                                 # a pointer no kernel may ever see: every refusal is decided before a device is needed
BIG = 1 << 40


def _row(first=0, count=1000, out_first=0, out_count=1000, total=1000, ceiling=0.9, inp=BAD, out=BAD):
    return _lib.VspLimiterRow(inp, first, count, out, out_first, out_count, total, ceiling)


def _call(lib, h, rows, A=66, H=882, ws=BIG, wsp=BAD):
    arr = (_lib.VspLimiterRow * max(len(rows), 1))(*rows)
    return lib.vsp_limiter_rows(h, None, len(rows), A, H, arr, None, None, wsp, ws)


def test_refusals_before_a_device_is_needed(ctx):
    lib, h = ctx
    err = lambda: lib.vsp_last_error(h)
    ok = _row()
    behind, ahead = 66 + 882 + 12, 66 + 12
    # (a whole utterance and a stream's middle piece pass the rows' checks: the next thing refused is the workspace)
    assert _call(lib, h, [ok, _row(first=5000 - behind, count=behind + 700 + ahead, out_first=5000, out_count=700, total=-1)], ws=16) == -6
    for A, H in ((-1, 0), (1025, 0), (0, -1), (0, 8193)):
        assert _call(lib, h, [ok], A=A, H=H) == -1 and b"attack" in err()
    assert _call(lib, h, []) == -1 and lib.vsp_limiter_rows(h, None, 1, 66, 882, None, None, None, BAD, BIG) == -1
    assert lib.vsp_limiter_rows(None, None, 1, 66, 882, (_lib.VspLimiterRow * 1)(ok), None, None, BAD, BIG) == -1
    # history is missing: first > max(0, out_first - behind)
    assert _call(lib, h, [ok, _row(first=5000 - behind + 1, count=3000, out_first=5000, out_count=700, total=-1)]) == -1
    assert b"row 1" in err() and b"before it" in err()
    assert _call(lib, h, [_row(first=1, count=999, out_first=1, out_count=999)]) == -1 and b"row 0" in err()
    assert _call(lib, h, [_row(first=0, count=3000, out_first=500, out_count=700, total=-1)], ws=16) == -6       # (the stream's start is enough)
    # look-ahead is missing while the stream goes on: total unknown, or total behind the provided samples
    for total in (-1, 1001, 5000):
        assert _call(lib, h, [ok, ok, _row(count=1000, out_count=1000 - ahead + 1, total=total)]) == -1
        assert b"row 2" in err() and b"look-ahead" in err()
        assert _call(lib, h, [_row(count=1000, out_count=1000 - ahead, total=total)], ws=16) == -6
    assert _call(lib, h, [_row(first=200, count=1800, out_first=200 + behind, out_count=1800 - behind, total=2000)], ws=16) == -6    # (the end is reached)
    # counts, positions, pointers, the ceiling
    for bad in (dict(count=-1), dict(out_count=-1), dict(first=-1), dict(out_first=-1), dict(total=-2), dict(count=(1 << 30) + 1, total=-1),
                dict(total=999), dict(out_first=0, out_count=1001), dict(first=100, count=900, out_first=99, out_count=5),
                dict(inp=None), dict(out=None), dict(ceiling=0.0), dict(ceiling=-0.5)):
        assert _call(lib, h, [ok, _row(**bad)]) == -1 and b"row 1" in err(), bad
    # a NaN ceiling is no refusal, whatever else the row holds: it is left alone
    assert _call(lib, h, [_row(ceiling=NAN, first=-7, count=-1, inp=None, out=None), ok], ws=16) == -6
    # the workspace
    need = lib.vsp_limiter_workspace_bytes(2, 1000, 66, 882)
    assert _call(lib, h, [ok, ok], ws=need - 1) == -6 and _call(lib, h, [ok], wsp=None) == -6
    assert lib.vsp_true_peak(h, None, 2, 9, BAD, 9, (C.c_int64 * 2)(9, 0), BAD, BAD, BIG) == -1 and b"row 1" in err()
    assert lib.vsp_true_peak(h, None, 1, 9, BAD, 8, (C.c_int64 * 1)(9), BAD, BAD, BIG) == -1
    assert lib.vsp_true_peak(h, None, 1, 9, None, 9, (C.c_int64 * 1)(9), BAD, BAD, BIG) == -1
    assert lib.vsp_true_peak(h, None, 1, 9, BAD, 9, (C.c_int64 * 1)(9), BAD, BAD, 16) == -6


# ---------------------------------------------------------------------------------------------- streams
class NumpyEngine:
    """The engine of ``vispeech_amd.limiter`` in numpy: the library's checks of a row, then the restatement's float32 run
    of the provided samples AS A ROW OF THEIR OWN (zero outside), of which the outputs are cut.  That equals the whole
    stream's output only if the stream provides every sample that reaches an output: what the bookkeeping is for."""

    def __init__(self):
        self.calls = []

    def limiter_history(self, A, H):
        return lr.history(A, H)

    def limiter_rows(self, rows, A, H, gains=None):
        behind, ahead = lr.history(A, H)
        outs, mg = [], []
        self.calls.append([(r[1], len(r[0]), r[2], r[3], r[4]) for r in rows])
        for b, (x, first, out_first, out_count, total, c) in enumerate(rows):
            end = first + len(x)
            assert out_count > 0 and first <= max(0, out_first - behind) and out_first >= first and out_first + out_count <= end
            assert end >= out_first + out_count + ahead or total == end
            d = lr.limit(x, 1.0 if gains is None else gains[b], c, A, H, np.float32)
            outs.append(d["out"][out_first - first:out_first - first + out_count].copy())
            mg.append(d["s"][out_first - first:out_first - first + out_count].min())
        return outs, np.array(mg, np.float32)


def _splits(N, rng):
    yield "ones", [1] * N
    yield "sevens", [7] * (N // 7) + [N % 7]
    yield "whole", [N]
    yield "whole, then an empty final push", [N, 0]
    for k in range(3):
        sizes = []
        while sum(sizes) < N:
            sizes.append(int(rng.integers(0, 400)))
        sizes[-1] -= sum(sizes) - N
        yield f"random {k}", sizes + ([0] if k == 2 else [])


@pytest.mark.parametrize("A,H", ((16, 100), (66, 882), (0, 0), (1, 0)))
def test_stream_bookkeeping_any_split_equals_the_whole(A, H):
    N = 1500
    x = lr.voiced(N, 81)
    g, c = 3.0, 0.9
    whole = lr.limit(x, g, c, A, H, np.float32)
    assert whole["min_gain"] < 1.0
    behind, ahead = lr.history(A, H)
    for name, sizes in _splits(N, np.random.default_rng(3)):
        eng = NumpyEngine()
        s = limiter.Stream(eng, c, gain=g, attack=A, hold=H)
        got, k = [], 0
        for i, m in enumerate(sizes):
            y = s.push(x[k:k + m], final=(i == len(sizes) - 1))
            k += m
            assert len(s.buf) <= behind + ahead and s.first + len(s.buf) == s.seen == k, name
            assert s.out_next == (k if i == len(sizes) - 1 else max(0, k - ahead)), name     # the delay: A + J samples
            got.append(y)
        got = np.concatenate(got)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), whole["out"].view(np.uint32)), name
        assert all(len(call) == 1 for call in eng.calls)
        with pytest.raises(ValueError):
            s.push(x[:1])


def test_push_rows_is_one_call_for_streams_at_their_own_positions():
    eng = NumpyEngine()
    xs = [lr.voiced(900, 91), lr.voiced(500, 92), lr.voiced(40, 93)]
    ss = [limiter.Stream(eng, 0.9, gain=3.0, attack=16, hold=100), limiter.Stream(eng, 0.5, gain=2.0, attack=16, hold=100),
          limiter.Stream(eng, 0.9, attack=16, hold=100)]
    a = limiter.push_rows(eng, [(ss[0], xs[0][:300], False), (ss[1], xs[1][:20], False), (ss[2], xs[2], True)])
    assert [len(y) for y in a] == [300 - 28, 0, 40] and len(eng.calls) == 1 and len(eng.calls[0]) == 2     # (a row that completes nothing is no row)
    b = limiter.push_rows(eng, [(ss[0], xs[0][300:], True), (ss[1], xs[1][20:], True)])
    assert len(eng.calls) == 2 and [r[0] for r in eng.calls[1]] == [300 - 28 - 128, 0]                       # the history kept: behind = 128
    for i, parts in enumerate(([a[0], b[0]], [a[1], b[1]], [a[2]])):
        want = lr.limit(xs[i], ss[i].gain, ss[i].ceiling, 16, 100, np.float32)["out"]
        assert np.array_equal(np.concatenate(parts), want)
    assert limiter.push_rows(eng, []) == [] and len(eng.calls) == 2
    with pytest.raises(ValueError):
        limiter.push_rows(eng, [(limiter.Stream(eng, 0.9, attack=16, hold=100), xs[0], False), (limiter.Stream(eng, 0.9, attack=17, hold=100), xs[0], False)])


def test_milliseconds_to_samples():
    assert limiter.samples(1.5, 44100) == 66 and limiter.samples(20.0, 44100) == 882 and limiter.samples(0, 8000) == 0
    assert limiter.samples(1.5, 8000) == 12 and limiter.samples(0.0625, 8000) == 1          # halves go up
    assert limiter.window(44100) == (66, 882) and limiter.window(22050, 2.0, 0.0) == (44, 0)
    for bad in (lambda: limiter.samples(-1.0, 44100), lambda: limiter.samples(NAN, 44100), lambda: limiter.window(44100, 30.0),
                lambda: limiter.window(44100, None, 200.0), lambda: limiter.spec(dict(release_ms=3), 44100),
                lambda: limiter.spec(0.5, 44100), lambda: limiter.spec(dict(ceiling=0.0), 44100), lambda: limiter.spec(dict(gain_db=NAN), 44100)):
        with pytest.raises(ValueError):
            bad()
    assert limiter.spec(None, 44100) is None and limiter.spec(False, 44100) is None
    assert limiter.spec(True, 44100) == (66, 882, 1.0, 1.0)
    A, H, c, g = limiter.spec(dict(attack_ms=1.0, hold_ms=10.0, ceiling=0.5, gain_db=6.0), 44100, default_ceiling=0.9)
    assert (A, H, c) == (44, 441, 0.5) and abs(g - 10 ** 0.3) < 1e-12
    assert limiter.spec({}, 22050, default_ceiling=0.9)[:3] == (33, 441, 0.9)


# ---------------------------------------------------------------------------------------------- the services' calls
import math  # noqa: E402

import output_stage_ref as oref  # noqa: E402
import test_output_rows_host as rows_host  # noqa: E402
import test_service_paths_host as paths_host  # noqa: E402
from test_loudness_host import LoudInferEngine, LoudInferNet, _record_normalize, _text_service  # noqa: E402
from vispeech_amd import output_stage  # noqa: E402


def _rows_of(params):
    return [(None if math.isnan(p.target_lufs) else round(p.target_lufs, 3), round(p.peak_ceiling, 3), round(p.max_gain_db, 3)) for p in params]


def _ceilings(c):
    return [None if v != v else round(v, 3) for v in c]


class LevelEngine(LoudInferEngine):
    """The loudness stand-in with the two limiter calls recorded: a limited row is multiplied by 3, a row normalised under a
    limiter by 1.5, in place."""
    loudness_normalize = _record_normalize

    def limit(self, waves, n, ceiling, gains=None, attack=66, hold=882, out=None):
        self.calls.append(("limit", [int(v) for v in n], _ceilings(ceiling), [round(float(g), 4) for g in gains], attack, hold))
        for b, c in enumerate(ceiling):
            if c == c:
                waves[b, : int(n[b])] *= 3.0

    def loudness_limit(self, waves, n, fs, params, attack=66, hold=882, ceilings=None, static_gains=None, out=None):
        self.calls.append(("loudness_limit", [int(v) for v in n], int(fs), _rows_of(params), _ceilings(ceilings),
                           None if static_gains is None else [round(float(g), 4) for g in static_gains], attack, hold))
        for b, c in enumerate(ceilings):
            if c == c:
                waves[b, : int(n[b])] *= 1.5


def _level_service(max_batch, **kw):
    net = LoudInferNet()
    net._engine = LevelEngine()
    return net, _text_service(net, max_batch=max_batch, **kw)


def _q(v):
    return int(np.rint(np.float32(v) * 32767.0))


def test_batching_service_makes_one_limiter_call_and_leaves_the_others_their_bytes():
    from vispeech_amd.text import request_row
    from test_prosody_host import SVC_HOP
    row = lambda: request_row("s", ["a", "b"], durations=[1, 2], f0=[5.0, 6.0], energy=[1.0, 2.0])
    n = 3 * SVC_HOP
    # a loudness and a limiter; a limiter only; a loudness only; nothing
    net, svc = _level_service(4)
    try:
        futs = [svc.submit(row(), 1, loudness=dict(target_lufs=-16.0, peak_ceiling=0.8), limiter=True),
                svc.submit(row(), 2, limiter=dict(gain_db=6.0, ceiling=0.5)), svc.submit(row(), 3, loudness=-20.0), svc.submit(row(), 4)]
        got = [f.result(60) for f in futs]
    finally:
        svc.close()
    g6 = round(10 ** 0.3, 4)
    assert net._engine.calls == [
        ("loudness_normalize", [n] * 4, 44100, [(None, 1.0, 0.0), (None, 1.0, 0.0), (-20.0, 1.0, 30.0), (None, 1.0, 0.0)]),
        ("loudness_limit", [n] * 4, 44100, [(-16.0, 0.8, 30.0), (None, 1.0, 0.0), (None, 1.0, 0.0), (None, 1.0, 0.0)],
         [0.8, 0.5, None, None], [1.0, g6, 1.0, 1.0], 66, 882)]
    assert [set(g.tolist()) for g in got] == [{_q(0.375)}, {_q(0.375)}, {_q(0.5)}, {_q(0.25)}]
    # limiters only: ONE limit call, nothing measured
    net, svc = _level_service(3, limiter=dict(attack_ms=1.0, hold_ms=0.0))
    try:
        futs = [svc.submit(row(), 1), svc.submit(row(), 2, limiter=False), svc.submit(row(), 3, limiter=dict(attack_ms=1.0, hold_ms=0.0, gain_db=-6.0))]
        got = [f.result(60) for f in futs]
    finally:
        svc.close()
    assert net._engine.calls == [("limit", [n] * 3, [1.0, None, 1.0], [1.0, 1.0, round(10 ** -0.3, 4)], 44, 0)]
    assert [set(g.tolist()) for g in got] == [{_q(0.75)}, {_q(0.25)}, {_q(0.75)}]


def test_batching_service_in_which_nobody_names_a_limiter_makes_the_old_calls():
    from vispeech_amd.text import request_row
    from test_prosody_host import SVC_HOP
    row = lambda: request_row("s", ["a"], durations=[3], f0=[5.0], energy=[1.0])
    net, svc = _level_service(2)
    try:
        futs = [svc.submit(row(), 1, loudness=-16), svc.submit(row(), 2)]
        [f.result(60) for f in futs]
        for bad in (dict(release_ms=1.0), 0.5, dict(attack_ms=50.0), dict(ceiling=-1.0)):
            with pytest.raises(ValueError):
                svc.submit(row(), 3, limiter=bad)
    finally:
        svc.close()
    n = 3 * SVC_HOP
    assert net._engine.calls == [("loudness_normalize", [n, n], 44100, [(-16.0, 1.0, 30.0), (None, 1.0, 0.0)])]
    with pytest.raises(ValueError):
        _text_service(LoudInferNet(), limiter=dict(hold_ms=500.0))


class StreamLimiterEngine(rows_host.StreamRowsEngine, NumpyEngine):
    def __init__(self):
        rows_host.StreamRowsEngine.__init__(self)
        self.limiter_calls = []

    def limiter_rows(self, rows, A, H, gains=None):
        self.calls.append(("limiter_rows", [(r[1], len(r[0]), r[2], r[3], r[4]) for r in rows], A, H))
        keep, self.calls = self.calls, []
        try:
            return NumpyEngine.limiter_rows(self, rows, A, H, gains)
        finally:
            self.calls = keep


LIMITED = dict(attack_ms=0.1, hold_ms=0.5, ceiling=25.0, gain_db=6.0)          # 4 and 22 samples: ahead = 16 samples = 4 frames


def _limited_one_shot(rid, frames, fmt):
    x = np.repeat(10 * rid + np.arange(frames), paths_host.UP).astype(np.float32)
    A, H, c, g = limiter.spec(LIMITED, rows_host.MODEL)
    y = lr.limit(x, g, c, A, H, np.float32)["out"]
    assert np.abs(y).max() <= np.float32(c) and np.abs(np.float32(g) * x).max() > 2 * c
    L, M, _ = output_stage.plan(rows_host.MODEL, fmt[0])
    z = oref.resample_fp64(y, output_stage.taps(rows_host.MODEL, fmt[0]), L, M).astype(np.float32)
    return rows_host.encode_ref(z, output_stage.encoding(fmt[1])).tobytes()


@pytest.mark.parametrize("chunk", [4, 3])
def test_streaming_service_limits_between_the_generator_and_the_output_rows(chunk):
    from vispeech_amd.service import StreamingBatchService
    net = paths_host.StreamNet()
    net._engine = eng = StreamLimiterEngine()
    svc = StreamingBatchService(net, collate=paths_host._collate, autostart=False, chunk_frames=chunk)
    a = svc.submit({"id": 1, "frames": 30}, 1, limiter=LIMITED)                      # a limiter, no format of its own
    b = svc.submit({"id": 2, "frames": 9}, 2)                                        # a neighbour that names nothing
    svc.step(); svc.step()
    c = svc.submit({"id": 3, "frames": 14}, 3, limiter=LIMITED, output_rate=8000, output_encoding="ulaw")
    svc.close()
    base = (rows_host.MODEL, "s16")
    assert b"".join(paths_host._pieces(a)) == _limited_one_shot(1, 30, base)
    assert b"".join(paths_host._pieces(c)) == _limited_one_shot(3, 14, (8000, "ulaw"))
    assert b"".join(paths_host._pieces(b)) == rows_host._one_shot_bytes(2, 9, None, base)      # the bytes of its own path
    names = [k[0] for k in eng.calls if k[0] in ("limiter_rows", "output_rows")]
    # at most ONE limiter call per tick, before the tick's rows (none in a first tick that completes no sample: 16 = ahead)
    assert names.count("output_rows") == svc.stats["ticks"] and names[-1] == "output_rows"
    assert all(b == "output_rows" for a, b in zip(names, names[1:]) if a == "limiter_rows")
    assert svc.stats["ticks"] - 1 <= names.count("limiter_rows") <= svc.stats["ticks"]
    lim = [k for k in eng.calls if k[0] == "limiter_rows"]
    assert max(len(k[1]) for k in lim) == 2 and all((k[2], k[3]) == (4, 22) for k in lim)
    totals = [row[4] for k in lim for row in k[1]]                                             # the last chunk carries the end
    assert sorted(t for t in totals if t >= 0) == [14 * paths_host.UP, 30 * paths_host.UP] and totals[0] == -1


def test_fused_output_refuses_a_limiter():
    from vispeech_amd.service import StreamingBatchService
    net = paths_host.StreamNet()
    svc = StreamingBatchService(net, collate=paths_host._collate, autostart=False, output_rate=22050, fused_output=True)
    with pytest.raises(ValueError, match="fused_output"):
        svc.submit({"id": 1, "frames": 3}, 1, limiter=True)
    with pytest.raises(ValueError, match="fused_output"):
        svc.submit_conversion(paths_host._audio(50), 1, 2, 3, limiter=dict(gain_db=3.0))
    with pytest.raises(ValueError, match="fused_output"):
        svc.open_conversion(1, 2, 3, limiter=True)
    svc.submit({"id": 1, "frames": 3}, 1, limiter=False).close()
