"""Loudness over time and the leveller, everything a CPU can check (no kernel is launched): the entry
points exist and refuse what they must before a device is needed, naming the row; the workspace sizes are monotone; the
restatement (tests/loudness_time_ref.py) judged on its own; ``vispeech_amd.loudness.Stream`` against a numpy engine -- any
split equals the whole --; the condition tests/test_loudness_time_gpu.py rests on: in every audio row, at EVERY prefix,
every block stays a factor 1.05 clear of both gates; and the streaming service's calls with and without ``loudness=``."""
import ctypes as C
import math

import numpy as np
import pytest

import loudness_ref as lr
import loudness_time_ref as ltr
import test_abi
from vispeech_amd import _lib, loudness
from vispeech_amd.schema import ModelDims

NEW = ("vsp_loudness_time_workspace_bytes", "vsp_loudness_segments_from", "vsp_loudness_time", "vsp_loudness_level_gains",
       "vsp_loudness_level_apply", "vsp_loudness_level")


# ---------------------------------------------------------------------------------------------- symbols and ABI
def test_symbols_and_abi():
    lib = _lib.lib()
    for s in NEW:
        assert hasattr(lib, s) and s in _lib.SIGNATURES, s
    assert lib.vsp_abi_version() == 7
    assert sorted(_lib.SIGNATURES) == test_abi.header_symbols()
    assert C.sizeof(_lib.VspLoudnessLevelParams) == 20 and C.sizeof(_lib.VspLoudnessRow) == 14 * 8


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
NAN = float("nan")
OK = (-23.0, 12.0, 12.0, 3.0, 0.0)


def _i64(v):
    return None if v is None else (C.c_int64 * len(v))(*v)


def _params(rows):
    return None if rows is None else (_lib.VspLoudnessLevelParams * len(rows))(*[_lib.VspLoudnessLevelParams(*r) for r in rows])


def _rows(rows):
    """rows: dicts of the fields that differ from a row that is fine for every call."""
    out = (_lib.VspLoudnessRow * len(rows))()
    for b, r in enumerate(rows):
        f = dict(seg=BAD, M=BAD, S=BAD, I=BAD, kept=BAD, c_db=BAD, c=BAD, first=0, count=2, entries=4, inp=BAD, out=BAD, pos=0, samples=9)
        f.update(r)
        out[b] = _lib.VspLoudnessRow(**f)
    return out


def _from(lib, h, n, L_max, fs=44100, first=None, ws=BIG):
    return lib.vsp_loudness_segments_from(h, None, len(n), L_max, fs, BAD, L_max, _i64(n), _i64(first), BAD, BAD, BAD, BAD, BAD, ws)


def _time(lib, h, rows, fs=44100, ws=BIG):
    return lib.vsp_loudness_time(h, None, len(rows), fs, _rows(rows), BAD, BAD, BAD, ws)


def _gains(lib, h, rows, params, ws=BIG):
    return lib.vsp_loudness_level_gains(h, None, len(rows), _rows(rows), _params(params), BAD, ws)


def _apply(lib, h, rows, params, fs=44100, ws=BIG):
    return lib.vsp_loudness_level_apply(h, None, len(rows), fs, _rows(rows), _params(params), BAD, ws)


def _level(lib, h, n, L_max, params, fs=44100, ws=BIG, stride=None):
    return lib.vsp_loudness_level(h, None, len(n), L_max, fs, BAD, L_max, BAD, L_max, _i64(n), _params(params), BAD, BAD, BAD, BAD, BAD, BAD,
                                  L_max // max(1, lr.segment_samples(fs)) if stride is None else stride, BAD, BAD, BAD, BAD, BAD, ws)


def test_refusals_before_a_device_is_needed(ctx):
    lib, h = ctx
    err = lambda: lib.vsp_last_error(h)
    # the rows' samples, as every loudness call
    for call in (lambda n: _from(lib, h, n, 9000), lambda n: _level(lib, h, n, 9000, [OK] * len(n)), lambda n: _level(lib, h, n, 9000, None)):
        assert call([9000, 0, 5]) == -1 and b"row 1" in err() and b"samples" in err()
        assert call([9000, 5, 9001]) == -1 and b"row 2" in err()
    # a piece that does not start on a segment boundary
    assert _from(lib, h, [9, 9, 9], 9, first=[0, 4410, 4409]) == -1 and b"row 2" in err() and b"segment boundary" in err()
    assert _from(lib, h, [9, 9], 9, first=[0, -4410]) == -1 and b"row 1" in err()
    assert _from(lib, h, [9, 9], 9, fs=8000, first=[800, 4410]) == -1 and b"row 1" in err()
    assert _from(lib, h, [9, 9], 9, first=[0, 441000], ws=16) == -6                     # (fine: the next refusal is the workspace)
    # first + count above the table
    for call in (lambda r: _time(lib, h, r), lambda r: _gains(lib, h, r, [OK] * len(r))):
        assert call([{}, dict(first=3, count=2)]) == -1 and b"row 1" in err() and b"table" in err()
        assert call([{}, {}, dict(first=-1)]) == -1 and b"row 2" in err()
        assert call([dict(count=-1)]) == -1 and b"row 0" in err()
        assert call([dict(entries=1 << 40, count=1)]) == -1 and b"row 0" in err()
    assert _apply(lib, h, [{}, dict(pos=4 * 4410, samples=4411)], [OK, OK]) == -1 and b"row 1" in err() and b"entries" in err()
    assert _apply(lib, h, [{}, dict(pos=4 * 4410, samples=4410)], [OK, OK], ws=16) == -6         # (the last sample is in segment 4)
    assert _apply(lib, h, [dict(pos=-1)], [OK]) == -1 and b"row 0" in err()
    # the leveller's parameters, in every call that takes them
    for bad, word in (((-23.0, -1.0, 12.0, 3.0, 0.0), b"max_gain_db"), ((-23.0, NAN, 12.0, 3.0, 0.0), b"max_gain_db"),
                      ((-23.0, 12.0, -0.5, 3.0, 0.0), b"max_cut_db"), ((-23.0, 12.0, NAN, 3.0, 0.0), b"max_cut_db"),
                      ((-23.0, 12.0, 12.0, 0.0, 0.0), b"slew_db_per_s"), ((-23.0, 12.0, 12.0, -3.0, 0.0), b"slew_db_per_s"),
                      ((-23.0, 12.0, 12.0, NAN, 0.0), b"slew_db_per_s"), ((-23.0, 12.0, 12.0, 3.0, NAN), b"initial_gain_db"),
                      ((-23.0, 12.0, 12.0, 3.0, float("inf")), b"initial_gain_db"), ((NAN, 12.0, 12.0, 0.0, 0.0), b"slew_db_per_s")):
        for call in (lambda p: _gains(lib, h, [{}, {}, {}], p), lambda p: _apply(lib, h, [{}, {}, {}], p),
                     lambda p: _level(lib, h, [9, 9, 9], 9, p)):
            assert call([OK, OK, bad]) == -1 and b"row 2" in err() and word in err()
    # a NaN target is no refusal: the row is left alone
    assert _gains(lib, h, [{}], [(NAN, 12.0, 12.0, 3.0, 0.0)], ws=16) == -6 and _level(lib, h, [9], 9, [(NAN, 12.0, 12.0, 3.0, 0.0)], ws=16) == -6
    # the sample rate
    for fs in (7999, 192001, 0, -44100):
        assert _from(lib, h, [5], 9, fs=fs) == -1 and b"sample_rate" in err()
        assert _time(lib, h, [{}], fs=fs) == -1 and b"sample_rate" in err()
        assert _apply(lib, h, [{}], [OK], fs=fs) == -1 and b"sample_rate" in err()
        assert _level(lib, h, [5], 9, [OK], fs=fs) == -1 and b"sample_rate" in err()
        assert lib.vsp_loudness_time_workspace_bytes(1, 9, fs) == -1
    # a workspace too small is a refusal of its own (-6); a table too narrow for the rows is not
    need = lib.vsp_loudness_time_workspace_bytes(1, 9000, 44100)
    assert _level(lib, h, [9000], 9000, [OK], ws=need - 1) == -6 and _level(lib, h, [9000], 9000, None, ws=need - 1) == -6
    assert _from(lib, h, [9000], 9000, ws=16) == -6 and _time(lib, h, [{}], ws=16) == -6 and _apply(lib, h, [{}], [OK], ws=16) == -6
    assert _level(lib, h, [9000], 9000, [OK], stride=1) == -1 and b"table_stride" in err()


def test_null_pointers_are_refused_after_the_rows(ctx):
    lib, h = ctx
    assert _time(lib, h, [dict(seg=None)]) == -1 and _time(lib, h, [dict(kept=None)]) == -1
    assert _gains(lib, h, [dict(c_db=None)], [OK]) == -1 and _apply(lib, h, [dict(out=None)], [OK]) == -1
    assert _gains(lib, h, [dict(c_db=None)], [(NAN, 12.0, 12.0, 3.0, 0.0)], ws=16) == -6             # (a row left alone needs none)
    assert lib.vsp_loudness_level_gains(h, None, 1, _rows([{}]), None, BAD, BIG) == -1
    assert lib.vsp_loudness_time(None, None, 1, 44100, _rows([{}]), BAD, BAD, BAD, BIG) == -1
    assert lib.vsp_loudness_time(h, None, 1, 44100, _rows([{}]), BAD, None, BAD, BIG) == -1          # the maxima come together


def test_workspace_sizes_are_monotone():
    lib = _lib.lib()
    for fs in (8000, 22050, 44100, 48000, 192000):
        for B in (1, 2, 16, 17):
            for L in (1, 799, 800, 4410, 4411, 44100, 441000, 1 << 24):
                v = lib.vsp_loudness_time_workspace_bytes(B, L, fs)
                assert v > lib.vsp_loudness_workspace_bytes(B, L, fs) + B * C.sizeof(_lib.VspLoudnessRow) - 256
                assert lib.vsp_loudness_time_workspace_bytes(B + 1, L, fs) >= v and lib.vsp_loudness_time_workspace_bytes(B, L + 1, fs) >= v
    assert lib.vsp_loudness_time_workspace_bytes(0, 9, 44100) == -1 and lib.vsp_loudness_time_workspace_bytes(1, 0, 44100) == -1


# ---------------------------------------------------------------------------------------------- the restatement
def test_the_running_level_ends_at_the_rows_loudness():
    for fs in (44100, 8000):
        h = lr.segment_samples(fs)
        for r in ltr.measured_rows(fs):
            F = r["n"] // h
            assert len(r["I"]) == len(r["M"]) == len(r["S"]) == F
            assert np.all(r["M"][:3] == -np.inf) and np.all(r["S"][:29] == -np.inf)
            if r["n"] >= 4 * h:
                assert r["I"][F - 1].tobytes() == np.float32(r["L"]).tobytes() and r["kept_s"][F - 1] == len(r["kept"]), r["name"]
    step = ltr.measured_rows(44100)[-1]
    assert step["name"] == "step" and step["n"] == 6 * 44100 + 7 and np.isfinite(step["S"][29:]).all() and len(step["S"]) == 60
    I = step["I"][np.isfinite(step["I"])]
    assert -24.0 < I.min() < -23.8 and -20.0 < I.max() < -19.8, (I.min(), I.max())       # the issue's -23.9 .. -19.9 LUFS


def test_a_steady_level_gives_a_constant_gain_and_silence_holds_the_initial_gain():
    fs = 8000
    h = lr.segment_samples(fs)
    x = lr.tone(fs, 3 * fs + 5, 1000.0, 0.1)
    I = np.full(30, np.float32(-23.0), np.float32)
    c_db, c = ltr.level_gains(I, target_lufs=-20.0, slew_db_per_s=20.0, initial_gain_db=3.0)
    assert (c_db == np.float32(3.0)).all() and len(set(c.tolist())) == 1
    out = ltr.level_apply(x, c, ltr.linear([3.0])[0], fs)
    assert out.tobytes() == (c[0] * x).astype(np.float32).tobytes()                         # a == c0 exactly: out = c x
    r = ltr.level(np.zeros(2 * fs + 3, np.float32), 2 * fs + 3, fs, target_lufs=-16.0, initial_gain_db=-2.5)
    assert (r["I"] == -np.inf).all() and (r["c_db"] == np.float32(-2.5)).all() and not r["out"].any()
    # the slew binds at 1 dB/s, the limits bind where the level is far off
    c_db, _ = ltr.level_gains(np.full(40, -40.0, np.float32), target_lufs=-23.0, slew_db_per_s=1.0)
    assert np.allclose(np.diff(c_db), 0.1, atol=1e-6) and c_db[-1] < 4.01
    c_db, _ = ltr.level_gains(np.full(80, -60.0, np.float32), target_lufs=-23.0, slew_db_per_s=20.0)
    assert c_db[-1] == np.float32(12.0)
    c_db, _ = ltr.level_gains(np.full(80, 0.0, np.float32), target_lufs=-23.0, slew_db_per_s=20.0, max_cut_db=6.0)
    assert c_db[-1] == np.float32(-6.0)
    # the gain ramps across a segment and is continuous across its end
    c = np.array([1.0, 2.0, 2.0], np.float32)
    out = ltr.level_apply(np.ones(4 * h, np.float32), c, np.float32(1.0), fs)
    assert (out[: 2 * h] == 1.0).all() and out[2 * h] == np.float32(1.0 + 1.0 / h) and out[3 * h - 1] == 2.0 and (out[3 * h:] == 2.0).all()


# ---------------------------------------------------------------------------------------------- the stream's host logic
def _split(n, cuts):
    edges = [0]
    for c in cuts:
        if edges[-1] >= n:
            break
        edges.append(min(n, edges[-1] + c))
    if edges[-1] < n:
        edges.append(n)
    return list(zip(edges[:-1], edges[1:]))


def test_stream_against_a_numpy_engine_any_split_equals_the_whole():
    fs = 8000
    h = lr.segment_samples(fs)
    x = ltr.step_row(fs)[: 34 * h + 13]
    spec = dict(target_lufs=-18.0, slew_db_per_s=20.0, initial_gain_db=1.5)
    whole = ltr.level(x, len(x), fs, **spec)
    rng = np.random.default_rng(5)
    for cuts in ([len(x)], [1, 7, h - 1, h, h + 1, 3 * h + 5] * 9, rng.integers(1, 3 * h, size=64).tolist()):
        eng = ltr.NumpyEngine()
        st = loudness.Stream(eng, fs, level=spec)
        pieces = _split(len(x), cuts)
        outs = [st.push(x[a:b], final=(b == len(x))) for a, b in pieces]
        assert [len(o) for o in outs] == [b - a for a, b in pieces]                       # every sample leaves in its own push
        assert np.concatenate(outs).tobytes() == whole["out"].tobytes()
        for k in ("M", "S", "I", "kept", "c_db", "c"):
            assert st.table[k].tobytes() == whole[k].tobytes(), k
        assert st.segments == 34 and st.seen == len(x) and st.open.shape == (13,)
        assert st.integrated == float(whole["I"][-1]) and st.gain_db == float(whole["c_db"][-1])
        assert st.momentary_max == float(whole["M"].max()) and st.short_term_max == float(whole["S"].max())
        with pytest.raises(ValueError):
            st.push(x[:1])
    # a meter hands back what it was given and makes no leveller call; three streams advance in one set of calls
    eng = ltr.NumpyEngine()
    a, b, c = loudness.Stream(eng, fs, level=True), loudness.Stream(eng, fs, level=-18.0), loudness.Stream(eng, fs)
    p = x[: h // 2]
    got = loudness.push_rows(eng, [(a, p, False), (b, x[: 2 * h + 1], False), (c, x[:h], False)])
    assert np.shares_memory(got[0], p) and got[0].shape == p.shape and a.gain_db is None and a.integrated == -math.inf and a.segments == 0
    assert [k[0] for k in eng.calls] == ["segments_from", "time", "level_gains", "level_apply"]
    assert eng.calls[0][1] == [2 * h, h] and eng.calls[1][1:] == ([0, 0], [2, 1]) and eng.calls[3][1:] == ([0], [2 * h + 1])
    eng.calls.clear()
    loudness.push_rows(eng, [(a, x[h // 2: h], False), (b, x[2 * h + 1: 2 * h + 5], False)])
    assert eng.calls == [("segments_from", [h]), ("time", [0], [1]), ("level_apply", [2 * h + 1], [4])]
    with pytest.raises(ValueError):
        loudness.push_rows(eng, [(a, p, False), (a, p, False)])
    with pytest.raises(ValueError):
        loudness.push_rows(eng, [(a, p, False), (loudness.Stream(eng, 44100), p, False)])


def test_stream_tables_grow_by_doubling_up_to_the_documented_cap(monkeypatch):
    fs = 8000
    h = lr.segment_samples(fs)
    assert min(loudness.max_segments(f) for f in (8000, 44100, 48000, 192000)) >= 36000
    monkeypatch.setattr(loudness, "FIRST_CAPACITY", 2)
    eng = ltr.NumpyEngine()
    st = loudness.Stream(eng, fs)
    x = lr.tone(fs, 9 * h, 440.0, 0.1)
    want = ltr.level(x, len(x), fs)
    for a in range(0, 9 * h, 3 * h):
        st.push(x[a: a + 3 * h])
        assert st.capacity in (4, 8, 16)
    assert st.capacity == 16 and st.table["I"].tobytes() == want["I"].tobytes()
    monkeypatch.setattr(loudness, "MAX_SAMPLES", 9 * h)
    with pytest.raises(ValueError, match="at most"):
        st.push(x[:1])


def test_the_spec_of_a_request():
    assert loudness.spec(None) is None and loudness.spec(False) is None and loudness.spec(True) == {}
    assert loudness.spec(-16) == dict(loudness.LEVEL_FIELDS, target_lufs=-16.0)
    assert loudness.spec(dict(target_lufs=-20, slew_db_per_s=1))["slew_db_per_s"] == 1.0
    for bad in (NAN, float("inf"), dict(max_gain_db=3), dict(target_lufs=-16, gain=3), dict(target_lufs=-16, max_gain_db=-1),
                dict(target_lufs=-16, max_cut_db=NAN), dict(target_lufs=-16, slew_db_per_s=0), dict(target_lufs=-16, initial_gain_db=NAN)):
        with pytest.raises(ValueError):
            loudness.spec(bad)
    from vispeech_amd.engine import Engine
    p = Engine.loudness_level_params(3, [-16.0, None, NAN], 6.0, [12.0, 0.0, 3.0])
    assert p[0].target_lufs == -16.0 and math.isnan(p[1].target_lufs) and p[2].max_cut_db == 3.0 and p[1].slew_db_per_s == 3.0
    for kw, word in ((dict(max_gain_db=-1), "max_gain_db"), (dict(max_cut_db=NAN), "max_cut_db"), (dict(slew_db_per_s=0), "slew_db_per_s"),
                     (dict(initial_gain_db=float("inf")), "initial_gain_db")):
        with pytest.raises(ValueError, match=f"row 0.*{word}"):
            Engine.loudness_level_params(1, **kw)


# ---------------------------------------------------------------------------------------------- the GPU tests' inputs
@pytest.mark.parametrize("fs", [44100, 22050, 8000])
def test_every_prefix_of_the_audio_rows_stays_clear_of_both_gates(fs):
    """At EVERY prefix of complete segments of every row, every block is a factor 1.05 from Z_abs and 10 E from that
    prefix's mean_abs: no rounding of a correct implementation moves a block across a gate, so ``kept[s]`` is exact."""
    rows = ltr.measured_rows(fs)
    assert [r["name"] for r in rows] == [n for n, _ in lr.audio_rows(fs)] + ["step"]
    fa, fr = zip(*(ltr.prefix_margins(r["seg"], r["n"], fs) for r in rows))
    print(f"fs {fs}: smallest absolute factor {min(fa):.3g} ({rows[int(np.argmin(fa))]['name']}), relative {min(fr):.3g} "
          f"({rows[int(np.argmin(fr))]['name']})")
    assert min(fa) >= 1.05 and min(fr) >= 1.05, (min(fa), min(fr))
    for r in rows:
        assert 1e-5 <= r["gate_lu"] <= 0.1
    if fs == 44100:
        step = rows[-1]
        I = step["I"][np.isfinite(step["I"])]
        c1, _ = ltr.level_gains(step["I"], target_lufs=-16.0, slew_db_per_s=1.0)
        c20, _ = ltr.level_gains(step["I"], target_lufs=-16.0, slew_db_per_s=20.0)
        d = np.float32(0.1)
        assert (np.abs(np.diff(c1)) >= d * 0.999).any() and (np.abs(np.diff(c20[5:])) < 2.0 * 0.999).all()   # 1 dB/s binds, 20 does not
        assert np.ptp(I) > 3.5


# ---------------------------------------------------------------------------------------------- the streaming service's calls
import output_stage_ref as oref  # noqa: E402
import test_output_rows_host as rows_host  # noqa: E402
import test_service_paths_host as paths_host  # noqa: E402
from vispeech_amd import output_stage  # noqa: E402

LOUD_CALLS = ("segments_from", "time", "level_gains", "level_apply")


class StreamLoudEngine(rows_host.StreamRowsEngine, ltr.NumpyEngine):
    """The recording stand-in of the streaming service with the numpy loudness engine: one list of calls."""

    def __init__(self):
        rows_host.StreamRowsEngine.__init__(self)


def _serve(eng, requests, chunk=500):
    from vispeech_amd.service import StreamingBatchService
    net = paths_host.StreamNet()
    net._engine = eng
    svc = StreamingBatchService(net, collate=paths_host._collate, autostart=False, chunk_frames=chunk)
    streams = [svc.submit({"id": rid, "frames": frames}, rid, **kw) for rid, frames, kw in requests]
    svc.close()
    return svc, streams, [b"".join(paths_host._pieces(s)) for s in streams]


def _frames_wave(rid, frames):
    return np.repeat(10 * rid + np.arange(frames), paths_host.UP).astype(np.float32)


F32 = dict(output_rate=rows_host.MODEL, output_encoding="f32")
LEVEL = dict(target_lufs=40.0, slew_db_per_s=20.0, max_cut_db=30.0)


def test_streaming_service_levels_between_the_generator_and_the_output_rows():
    fs = rows_host.MODEL
    requests = [(1, 2300, dict(loudness=LEVEL, **F32)), (2, 9, {}), (3, 1200, dict(loudness=True, **F32))]
    eng = StreamLoudEngine()
    svc, streams, got = _serve(eng, requests)
    # the levelled request: the one call on its whole waveform, then the output stage (an identity at the model's rate)
    x = _frames_wave(1, 2300)
    want = ltr.level(x, len(x), fs, **LEVEL)
    assert len(want["I"]) == 2 and np.isfinite(want["I"]).all() and want["c_db"][1] != want["c_db"][0] != 0.0
    assert got[0] == want["out"].tobytes() and got[0] != x.tobytes()
    assert got[2] == _frames_wave(3, 1200).tobytes()                                          # a meter changes no sample
    assert got[1] == rows_host._one_shot_bytes(2, 9, None, (fs, "s16"))                       # the bystander: the bytes of its own path
    assert streams[1].loudness is None
    assert streams[0].loudness == dict(integrated=float(want["I"][1]), momentary_max=-math.inf, short_term_max=-math.inf,
                                       gain_db=float(want["c_db"][1]))
    meter = ltr.level(_frames_wave(3, 1200), 4800, fs)
    assert streams[2].loudness == dict(integrated=float(meter["I"][0]), momentary_max=-math.inf, short_term_max=-math.inf, gain_db=None)
    # per tick: at most one call of each kind, all of them between the generator's call and output_rows
    names = [k[0] for k in eng.calls if k[0] in LOUD_CALLS + ("output_rows",)]
    ticks = "|".join(names).split("output_rows")
    assert names.count("output_rows") == svc.stats["ticks"] == 5 and names[-1] == "output_rows"
    for t in ticks[:-1]:
        t = [n for n in t.split("|") if n]
        assert len(set(t)) == len(t) and t == [n for n in LOUD_CALLS if n in t] and "level_apply" in t
    # requests 1 and 3 complete their segment 0 in the third tick, in ONE call; request 1 its segment 1 in the fifth
    assert [k[1] for k in eng.calls if k[0] == "segments_from"] == [[4410, 4410], [4410]] and names.count("level_gains") == 2
    assert [k for k in eng.calls if k[0] == "level_apply"][0][1:] == ([0], [500 * paths_host.UP])


def test_streaming_tick_in_which_nobody_names_a_loudness_makes_the_calls_it_always_made():
    requests = [(1, 30, dict(output_rate=48000, output_encoding="s16")), (2, 9, dict(output_rate=8000, output_encoding="ulaw"))]
    plain = rows_host.StreamRowsEngine()
    _, _, want = _serve(plain, requests, chunk=4)
    eng = StreamLoudEngine()
    _, streams, got = _serve(eng, requests, chunk=4)
    assert got == want and eng.calls == plain.calls and not [k for k in eng.calls if k[0] in LOUD_CALLS]
    assert all(s.loudness is None for s in streams)


def test_fused_output_refuses_a_loudness():
    from vispeech_amd.service import StreamingBatchService
    net = paths_host.StreamNet()
    svc = StreamingBatchService(net, collate=paths_host._collate, autostart=False, output_rate=22050, fused_output=True)
    with pytest.raises(ValueError, match="fused_output"):
        svc.submit({"id": 1, "frames": 3}, 1, loudness=-16)
    with pytest.raises(ValueError, match="fused_output"):
        svc.submit_conversion(paths_host._audio(50), 1, 2, 3, loudness=True)
    with pytest.raises(ValueError, match="fused_output"):
        svc.open_conversion(1, 2, 3, loudness=dict(target_lufs=-20.0))
    svc.submit({"id": 1, "frames": 3}, 1, loudness=False).close()
    plain = StreamingBatchService(paths_host.StreamNet(), collate=paths_host._collate, autostart=False)
    with pytest.raises(ValueError):
        plain.submit({"id": 1, "frames": 3}, 1, loudness=dict(target_lufs=-16, slew_db_per_s=0))
    plain.close()
