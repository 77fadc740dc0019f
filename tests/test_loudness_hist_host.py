"""Loudness range and the histogram gate, everything a CPU can check (no kernel is launched): the
entry points exist and refuse what they must before a device is needed; the restatement (tests/loudness_hist_ref.py) judged
on its own -- two-level tones, the bound against the exact gate --; ``vispeech_amd.loudness.Stream(gate="histogram")`` against
a numpy engine; and the conditions tests/test_loudness_hist_gpu.py rests on: in every audio row every block and every 3 s
window stays 1e-6 clear of every bin edge, and in every prefix the centre of no occupied bin lies within 1e-6 of a relative
gate, so that the device's counts, whose segment energies are within 6.2e-9 of fp64, can be compared exactly."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import loudness_hist_ref as hr
import loudness_ref as lr
import loudness_time_ref as ltr
import test_abi
from vispeech_amd import _lib, loudness
from vispeech_amd.schema import ModelDims

NEW = ("vsp_loudness_hist_tables", "vsp_loudness_hist_workspace_bytes", "vsp_loudness_time_hist", "vsp_loudness_range")
CUTS = (1, 2, 63, 64, 65)               # segments a piece; then a partial last piece


# ---------------------------------------------------------------------------------------------- symbols, tables, refusals
def test_symbols_and_abi():
    lib = _lib.lib()
    for s in NEW:
        assert hasattr(lib, s) and s in _lib.SIGNATURES, s
    assert lib.vsp_abi_version() == 7
    assert sorted(_lib.SIGNATURES) == test_abi.header_symbols()
    assert _lib.LOUDNESS_HIST_BINS == hr.NB == 1000
    with open(os.path.join(test_abi.ROOT, "include", "vispeech_hip.h")) as f:
        assert "#define VSP_LOUDNESS_HIST_BINS 1000\n" in f.read()


def library_tables():
    e, c = np.empty(hr.NB + 1), np.empty(hr.NB)
    assert _lib.lib().vsp_loudness_hist_tables(e.ctypes.data_as(C.POINTER(C.c_double)), c.ctypes.data_as(C.POINTER(C.c_double))) == 0
    return e, c


def test_the_librarys_tables_are_the_restatements_within_two_ulp():
    e, c = library_tables()
    assert np.abs(e / hr.EDGES - 1.0).max() <= 4.5e-16 and np.abs(c / hr.CENTRES - 1.0).max() <= 4.5e-16
    assert abs(e[0] / lr.Z_ABS - 1.0) <= 4.5e-16            # e_0 is section 4p's Z_abs, by its own expression
    assert (np.diff(e) > 0).all() and (np.diff(c) > 0).all() and (e[:-1] < c).all() and (c < e[1:]).all()
    lib = _lib.lib()
    assert lib.vsp_loudness_hist_tables(None, c.ctypes.data_as(C.POINTER(C.c_double))) == -1


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


def _rows(rows):
    out = (_lib.VspLoudnessRow * len(rows))()
    for b, r in enumerate(rows):
        f = dict(seg=BAD, M=BAD, S=BAD, I=BAD, kept=BAD, first=0, count=2, entries=4)
        f.update(r)
        out[b] = _lib.VspLoudnessRow(**f)
    return out


def _time_hist(lib, h, rows, fs=44100, ws=BIG, hist=BAD, m_max=BAD, s_max=BAD):
    hs = None if hist is None else (C.c_void_p * len(rows))(*(hist if isinstance(hist, list) else [hist] * len(rows)))
    return lib.vsp_loudness_time_hist(h, None, len(rows), fs, _rows(rows), hs, m_max, s_max, BAD, BAD, ws)


def _range(lib, h, n, L_max, fs=44100, ws=BIG, tables=(BAD,) * 4, stride=None, lra=BAD):
    return lib.vsp_loudness_range(h, None, len(n), L_max, fs, BAD, L_max, (C.c_int64 * len(n))(*n), lra, BAD, *tables,
                                  L_max // lr.segment_samples(max(fs, 10)) if stride is None else stride, BAD, ws)


def test_refusals_before_a_device_is_needed(ctx):
    lib, h = ctx
    err = lambda: lib.vsp_last_error(h)
    # the entries, as vsp_loudness_time refuses them, naming the row
    assert _time_hist(lib, h, [{}, dict(first=3, count=2)]) == -1 and b"row 1" in err() and b"table" in err()
    assert _time_hist(lib, h, [{}, {}, dict(first=-1)]) == -1 and b"row 2" in err()
    assert _time_hist(lib, h, [dict(count=-1)]) == -1 and b"row 0" in err()
    assert _time_hist(lib, h, [dict(entries=1 << 40, count=1)]) == -1 and b"row 0" in err()
    assert _time_hist(lib, h, [dict(seg=None)]) == -1 and _time_hist(lib, h, [dict(kept=None)]) == -1
    assert _time_hist(lib, h, [dict(seg=None, count=0)], ws=16) == -6                   # (a row without entries needs no tables)
    # a NULL histogram: the array, or one row's
    assert _time_hist(lib, h, [{}], hist=None) == -1 and b"histogram" in err()
    assert _time_hist(lib, h, [{}, {}, {}], hist=[BAD, BAD, None]) == -1 and b"row 2" in err() and b"histogram" in err()
    assert _time_hist(lib, h, [dict(count=0)], hist=[None]) == -1                       # (even for a row without entries)
    assert _time_hist(lib, h, [{}], m_max=None) == -1                                   # the maxima come together
    assert _time_hist(lib, h, [{}], m_max=None, s_max=None, ws=16) == -6
    assert lib.vsp_loudness_time_hist(None, None, 1, 44100, _rows([{}]), (C.c_void_p * 1)(BAD), BAD, BAD, BAD, BAD, BIG) == -1
    # whole rows
    assert _range(lib, h, [9000, 0, 5], 9000) == -1 and b"row 1" in err() and b"samples" in err()
    assert _range(lib, h, [9000, 5, 9001], 9000) == -1 and b"row 2" in err()
    assert _range(lib, h, [9000], 9000, tables=(BAD, BAD, None, BAD)) == -1 and b"come together" in err()
    assert _range(lib, h, [9000], 9000, tables=(None,) * 4, stride=0, ws=16) == -6      # (no tables: their stride is not looked at)
    assert _range(lib, h, [9000], 9000, stride=1) == -1 and b"table_stride" in err()
    assert _range(lib, h, [9000], 9000, lra=None) == -1
    for fs in (7999, 192001, 0, -44100):
        assert _time_hist(lib, h, [{}], fs=fs) == -1 and b"sample_rate" in err()
        assert _range(lib, h, [5], 9, fs=fs) == -1 and b"sample_rate" in err()
        assert lib.vsp_loudness_hist_workspace_bytes(1, 9, fs) == -1
    # a workspace too small is a refusal of its own (-6)
    need = lib.vsp_loudness_hist_workspace_bytes(1, 9000, 44100)
    assert _range(lib, h, [9000], 9000, ws=need - 1) == -6
    assert _time_hist(lib, h, [{}], ws=8 * (2 * hr.NB + 1)) == -6                       # (the tables alone are that large)


def test_workspace_sizes_are_monotone():
    lib = _lib.lib()
    for fs in (8000, 44100, 192000):
        for B in (1, 2, 16, 17):
            for L in (1, 800, 4411, 441000, 1 << 24):
                v = lib.vsp_loudness_hist_workspace_bytes(B, L, fs)
                assert v >= lib.vsp_loudness_time_workspace_bytes(B, L, fs) + 8 * (2 * hr.NB + 1) + B * (8 + 8 * hr.NB)
                assert lib.vsp_loudness_hist_workspace_bytes(B + 1, L, fs) >= v and lib.vsp_loudness_hist_workspace_bytes(B, L + 1, fs) >= v
    assert lib.vsp_loudness_hist_workspace_bytes(0, 9, 44100) == -1 and lib.vsp_loudness_hist_workspace_bytes(1, 0, 44100) == -1


def test_bad_gates_are_refused():
    from vispeech_amd.service import StreamingBatchService
    import test_service_paths_host as paths_host
    with pytest.raises(ValueError, match="gate"):
        loudness.Stream(hr.NumpyEngine(), 8000, gate="histograms")
    with pytest.raises(ValueError, match="loudness_gate"):
        StreamingBatchService(paths_host.StreamNet(), collate=paths_host._collate, autostart=False, loudness_gate="hist")
    for g in ("exact", "histogram"):
        StreamingBatchService(paths_host.StreamNet(), collate=paths_host._collate, autostart=False, loudness_gate=g).close()


# ---------------------------------------------------------------------------------------------- the restatement
def test_binning_is_by_comparisons_against_the_edges():
    e = hr.EDGES
    assert hr.bin_of(0.0) == hr.bin_of(float(np.nextafter(e[0], 0.0))) == hr.bin_of(float("nan")) == -1
    assert hr.bin_of(float(e[0])) == 0 and hr.bin_of(float(np.nextafter(e[1], 0.0))) == 0 and hr.bin_of(float(e[1])) == 1
    assert hr.bin_of(float(e[999])) == hr.bin_of(float(e[1000])) == hr.bin_of(1e9) == hr.bin_of(float("inf")) == 999
    # bin k covers [-70 + k / 10, -70 + (k + 1) / 10) LUFS, its centre sits in the middle
    for k in (0, 1, 437, 999):
        assert abs(ltr.lufs(e[k], 1.0) - (-70.0 + k / 10.0)) < 1e-9 and abs(ltr.lufs(hr.CENTRES[k], 1.0) - (-69.95 + k / 10.0)) < 1e-9
    assert hr.planted_ok() and hr.planted_ok(library_tables()[0])


def test_the_range_percentiles_by_hand():
    HS = np.zeros(hr.NB, np.int32)
    assert hr.range_of(HS) == 0.0
    HS[500] = 1
    assert hr.range_of(HS, detail=True)[2:] == (1, 500, 500) and hr.range_of(HS) == 0.0
    HS[:] = 0
    HS[400:500] = 1                                       # 100 windows, one a bin, all within 10 LU of each other: all kept
    lra, _, N, k10, k95 = hr.range_of(HS, detail=True)
    assert (N, k10, k95) == (100, 410, 494) and lra == np.float32(8.4)                  # lo = 10: the 11th; hi = 94: the 95th
    HS[100] = 50                                          # 30 LU below: the relative gate at -20 LU drops them
    assert hr.range_of(HS, detail=True)[2:] == (100, 410, 494)
    HS[100] = 0
    HS[350] = 50                                          # within 20 LU of the mean: they count
    assert hr.range_of(HS, detail=True)[2] == 150


@pytest.mark.parametrize("db_a, db_b, half_s, want", [(-20.0, -30.0, 20.0, 10.0), (-20.0, -30.0, 4.0, 10.0), (-20.0, -15.0, 4.0, 5.0),
                                                      (-40.0, -20.0, 4.0, 20.0)])
def test_two_level_tones(db_a, db_b, half_s, want):
    """1 kHz at 8 kHz in two equal halves: the range is the level difference within one bin of quantisation, 0.1 LU."""
    fs = 8000
    x = hr.two_level(fs, half_s, db_a, db_b)
    r = hr.measure(x, len(x), fs)
    print(f"{db_a} / {db_b} dBFS, halves of {half_s} s: LRA {float(r['lra'])!r}")
    assert abs(float(r["lra"]) - abs(db_a - db_b)) <= 0.1 + 1e-6
    assert float(r["lra"]) == float(np.float32(want))     # what this restatement reads


# ---------------------------------------------------------------------------------------------- the GPU tests' inputs
_MEASURED = {}


def measured(fs):
    """Per row of ``loudness_time_ref.measured_rows(fs)`` (the audio fixtures of the GPU tests): the histogram restatement."""
    if fs not in _MEASURED:
        _MEASURED[fs] = [(r, hr.whole(r["seg"], r["n"], fs)) for r in ltr.measured_rows(fs)]
    return _MEASURED[fs]


def clearances(seg, n, fs, tables=None):
    """``(edge, threshold)``: the smallest relative distance of any block's or 3 s window's mean square from any edge, and of
    the centre of any OCCUPIED bin from ``mean_abs / 10`` (blocks) or ``mean / 100`` (windows) in any prefix of complete
    segments.  An empty bin changes no value whichever side of a gate it is on -- and must be left out: while all counts
    sit in one bin k (a steady tone), mean_abs is c_k, and c_(k - 100) is mean_abs / 10 to the last bit or two."""
    edges, centres = tables or (hr.EDGES, hr.CENTRES)
    F = int(n) // lr.segment_samples(fs)
    zB, zS = hr.mean_squares(seg, F, fs)
    edge = min([hr.edge_distance(z, edges) for z in zB + zS if z is not None] + [math.inf])
    hist = np.zeros((2, hr.NB), np.int32)
    thr = math.inf
    for s in range(F):
        hr.advance(seg[: s + 1], s, 1, fs, hist, (edges, centres))
        mean_abs = hr.level_of(hist[0], centres, detail=True)[2]
        mean = hr.range_of(hist[1], centres, detail=True)[1]
        if mean_abs:
            thr = min(thr, hr.threshold_distance(mean_abs, 10.0, centres[hist[0] > 0]))
        if mean:
            thr = min(thr, hr.threshold_distance(mean, 100.0, centres[hist[1] > 0]))
    return edge, thr


@pytest.mark.parametrize("fs", [44100, 8000])
def test_audio_rows_stay_clear_of_every_edge_and_threshold(fs):
    tables = library_tables()
    worst_e, worst_t = (math.inf, None), (math.inf, None)
    for r in ltr.measured_rows(fs):
        e, t = clearances(r["seg"], r["n"], fs, tables)
        worst_e, worst_t = min(worst_e, (e, r["name"]), key=lambda v: v[0]), min(worst_t, (t, r["name"]), key=lambda v: v[0])
    print(f"fs {fs}: smallest distance from an edge {worst_e[0]:.3g} ({worst_e[1]}), from a threshold {worst_t[0]:.3g} ({worst_t[1]})")
    assert worst_e[0] >= 1e-6 and worst_t[0] >= 1e-6


def test_tone_pairs_and_constructed_rows_stay_clear():
    tables = library_tables()
    fs = 8000
    x = hr.two_level(fs, 4.0, -20.0, -30.0)
    e, t = clearances(lr.segments(lr.kfilter(x, fs), len(x), fs), len(x), fs, tables)
    print(f"tone pair: edge {e:.3g}, threshold {t:.3g}")
    assert e >= 1e-6 and t >= 1e-6
    # the constructed rows sit ON edges by design; their sums are the device's in every bit, so only the thresholds matter
    for seg in hr.edge_rows(tables[0]):
        assert clearances(seg, len(seg) * lr.segment_samples(lr.TABLE_FS), lr.TABLE_FS, tables)[1] >= 1e-6


@pytest.mark.parametrize("fs", [44100, 8000])
def test_the_histogram_gate_stays_within_half_a_bin_of_the_exact_gate(fs):
    """Where every prefix's blocks stay a factor 1.05 clear of both exact gates (test_loudness_time_host.py asserts it for
    these rows), the histogram gate keeps the same blocks and reads within 0.05 LU: each kept energy moves by at most half
    a bin (0.05 LU, a factor 1.0116), the threshold ``mean_abs / 10`` by as much, and a block against it by at most
    0.15 LU in all (a factor 1.035 < 1.05)."""
    worst = 0.0
    for r, g in measured(fs):
        F = r["n"] // lr.segment_samples(fs)
        fa, fr = ltr.prefix_margins(r["seg"], r["n"], fs)
        assert fa >= 1.05 and fr >= 1.05
        assert (g["kept"][:3] == 0).all() and np.isneginf(g["I"][:3]).all()             # no one-block rule
        assert (g["kept"][3:] == r["kept_s"][3:F]).all(), r["name"]
        both = np.isfinite(r["I"][3:F])
        assert (np.isfinite(g["I"][3:]) == both).all()
        if both.any():
            d = np.abs(np.array(g["I64"][3:])[both] - np.array(r["I64"][3:F])[both]).max()
            worst = max(worst, d)
            assert d <= 0.05 + 1e-4, (r["name"], d)
    print(f"fs {fs}: max |I_h - I| = {worst:.4f} LU")
    assert worst > 0.0


# ---------------------------------------------------------------------------------------------- streams on the numpy engine
def _pieces(n, h, cuts):
    edges = [0]
    for c in cuts:
        if edges[-1] + c * h >= n:
            break
        edges.append(edges[-1] + c * h)
    edges.append(n)
    return list(zip(edges[:-1], edges[1:]))


def test_histogram_stream_under_the_cuts_equals_the_one_call():
    fs = 8000
    h = lr.segment_samples(fs)
    F = sum(CUTS) + 1
    x = lr.main_signal(fs, F * h + 13)
    spec = dict(target_lufs=-18.0, slew_db_per_s=20.0, initial_gain_db=1.5)
    seg = lr.segments(lr.kfilter(x, fs), len(x), fs)
    want = hr.whole(seg, len(x), fs)
    c_db, c = ltr.level_gains(want["I"], **spec)
    out = ltr.level_apply(x, c, ltr.linear([1.5])[0], fs)
    assert float(want["lra"]) > 1.0 and want["hist"][1].sum() == F - 29
    for cuts in ([F], CUTS, CUTS[::-1], (7,) * 28):
        eng = hr.NumpyEngine()
        st = loudness.Stream(eng, fs, level=spec, gate="histogram")
        assert st.loudness_range == 0.0
        pieces = _pieces(len(x), h, cuts)
        outs = [st.push(x[a:b], final=(b == len(x))) for a, b in pieces]
        assert np.concatenate(outs).tobytes() == out.tobytes()
        for k, w in (("M", want["M"]), ("S", want["S"]), ("I", want["I"]), ("kept", want["kept"]), ("c_db", c_db), ("c", c)):
            assert st.table[k].tobytes() == w.tobytes(), k
        assert st.hist.tobytes() == want["hist"].tobytes() and st.loudness_range == float(want["lra"])
        assert st.integrated == float(want["I"][-1]) and st.segments == F
        names = [k[0] for k in eng.calls]
        assert "time" not in names and names.count("time_hist") == sum(b // h > a // h for a, b in pieces)
    # M and S are section 4r's in every bit
    exact = ltr.level(x, len(x), fs, **spec)
    assert want["M"].tobytes() == exact["M"].tobytes() and want["S"].tobytes() == exact["S"].tobytes()


def test_a_push_rows_call_may_mix_both_gates():
    fs = 8000
    h = lr.segment_samples(fs)
    x = ltr.step_row(fs)[: 34 * h]
    eng = hr.NumpyEngine()
    a, b, c = loudness.Stream(eng, fs, level=-18.0), loudness.Stream(eng, fs, level=-18.0, gate="histogram"), loudness.Stream(eng, fs)
    alone = loudness.Stream(ltr.NumpyEngine(), fs, level=-18.0)
    outs = [[], [], []]
    for t, (lo, hi) in enumerate(_pieces(len(x), h, (2, 5, 1, 26))):
        eng.calls.clear()
        got = loudness.push_rows(eng, [(a, x[lo:hi], False), (b, x[lo + 0: hi], False), (c, x[lo:hi], False)])
        for o, g in zip(outs, got):
            o.append(g)
        alone.push(x[lo:hi])
        names = [k[0] for k in eng.calls]
        assert names == ["segments_from", "time", "time_hist", "level_gains", "level_apply"]
        assert eng.calls[1][1:] == ([lo // h, lo // h], [(hi - lo) // h] * 2) and eng.calls[2][1:] == ([lo // h], [(hi - lo) // h])
    for k in ("M", "S", "I", "kept", "c_db", "c"):
        assert a.table[k].tobytes() == alone.table[k].tobytes()                         # the exact stream: as without its neighbour
    assert np.concatenate(outs[0]).tobytes() != np.concatenate(outs[1]).tobytes()         # 0.05 LU apart: other gains
    want = hr.whole(lr.segments(lr.kfilter(x, fs), len(x), fs), len(x), fs)
    assert b.table["I"].tobytes() == want["I"].tobytes() and b.loudness_range == float(want["lra"])
    assert a.loudness_range is None and c.loudness_range is None and a.hist is None


class Spy(ltr.NumpyEngine):
    """The numpy engine of section 4r, which has neither histogram method: a default stream must not ask for one."""

    def __getattr__(self, name):
        raise AssertionError(f"a default stream asked its engine for {name}")


def test_a_default_stream_makes_the_calls_it_always_made():
    fs = 8000
    h = lr.segment_samples(fs)
    x = ltr.step_row(fs)[: 5 * h + 3]
    spy, plain = Spy(), ltr.NumpyEngine()
    for eng in (spy, plain):
        st = loudness.Stream(eng, fs, level=-18.0)
        st.push(x[: 2 * h + 1])
        st.push(x[2 * h + 1:], final=True)
        assert st.loudness_range is None
    assert spy.calls == plain.calls and [k[0] for k in spy.calls].count("time") == 2
    with pytest.raises(AssertionError):
        loudness.Stream(Spy(), fs, gate="histogram")


# ---------------------------------------------------------------------------------------------- the streaming service's calls
def test_streaming_service_opens_histogram_streams_when_asked():
    import test_loudness_time_host as time_host
    from vispeech_amd.service import StreamingBatchService
    paths_host, rows_host = time_host.paths_host, time_host.rows_host

    class Engine(rows_host.StreamRowsEngine, hr.NumpyEngine):
        def __init__(self):
            rows_host.StreamRowsEngine.__init__(self)

    def serve(**kw):
        eng = Engine()
        net = paths_host.StreamNet()
        net._engine = eng
        svc = StreamingBatchService(net, collate=paths_host._collate, autostart=False, chunk_frames=500, **kw)
        stream = svc.submit({"id": 1, "frames": 2300}, 1, loudness=time_host.LEVEL, **time_host.F32)
        svc.close()
        return eng, stream, b"".join(paths_host._pieces(stream))

    fs = rows_host.MODEL
    x = time_host._frames_wave(1, 2300)
    eng, stream, got = serve(loudness_gate="histogram")
    names = [k[0] for k in eng.calls]
    assert names.count("time_hist") == 2 and "time" not in names
    want = hr.measure(x, len(x), fs)
    c_db, c = ltr.level_gains(want["I"], **time_host.LEVEL)
    assert got == ltr.level_apply(x, c, np.float32(1.0), fs).tobytes()
    assert stream.loudness == dict(integrated=float(want["I"][1]), momentary_max=-math.inf, short_term_max=-math.inf, gain_db=float(c_db[1]),
                                   range_lu=0.0)
    # the default: the calls and the dict of before
    eng, stream, _ = serve()
    names = [k[0] for k in eng.calls]
    assert names.count("time") == 2 and "time_hist" not in names and "range_lu" not in stream.loudness
