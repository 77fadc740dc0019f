"""Loudness over time and the leveller on the GPU against the restatement (tests/loudness_time_ref.py):
K-weighting carried across calls, on both end-state branches of lk_ends_kernel; the tables M, S, I and kept on audio and, the
table operator alone, on constructed double tables with exact ties; the leveller's gain in dB bit for bit against float32
numpy fed the device's own running level; apply in place and out of place; the fused call against the separate calls; and
streams under any split against the one call on the whole row, bit for bit.

Gates are those of tests/test_loudness_gpu.py: per row, 4 times the distance of the float32 CPU recurrence from the fp64
one, at least 1e-5 LU, at most 0.1 LU -- never derived from the library.  tests/test_loudness_time_host.py asserts that
every block of every PREFIX of every audio row stays a factor 1.05 clear of both gates, so ``kept[s]`` is compared exactly."""
import math

import numpy as np
import pytest
import torch

import loudness_ref as lr
import loudness_time_ref as ltr

pytestmark = pytest.mark.gpu

NAN = float("nan")


def to_np(t):
    return t.detach().cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from vispeech_amd.engine import Engine
    from vispeech_amd.schema import ModelDims
    return Engine(ModelDims(), "cuda:0")                   # (the loudness calls need no weights)


def dev(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


# ---------------------------------------------------------------------------------------------- carried segments
def carried_streams(fs, segs):
    h = lr.segment_samples(fs)
    return [lr.main_signal(fs, segs * h + 37), lr.tone(fs, segs * h + h - 1, 997.0, 0.25),
            (0.3 * np.cos(np.arange(segs * h + 1) * 0.01) + 0.01).astype(np.float32)]


CUTS = {195: ([1, 2, 63, 64, 65], [65, 64, 63, 2, 1], [64, 1, 65, 2, 63]), 130: ([1, 2, 63, 64], [65, 65], [64, 2, 63, 1])}


def in_pieces(eng, fs, xs, cuts):
    """Every stream cut at segment boundaries into pieces of ``cuts[i]`` segments and a partial last piece; every round is ONE
    call over the next piece of every stream that has one, NaN behind every piece.  ``(seg, peak)`` per stream."""
    h = lr.segment_samples(fs)
    pos = [0] * len(xs)
    todo = [list(c) for c in cuts]
    state = [torch.zeros(4, dtype=torch.float64, device=eng.device) for _ in xs]
    segs, peaks = [[] for _ in xs], [[] for _ in xs]
    while any(p < len(x) for p, x in zip(pos, xs)):
        live = [i for i, x in enumerate(xs) if pos[i] < len(x)]
        pieces = []
        for i in live:
            k = todo[i].pop(0) * h if todo[i] else len(xs[i]) - pos[i]
            pieces.append(xs[i][pos[i]: pos[i] + k])
        audio, n = lr.pack(pieces)
        seg, peak, out = eng.loudness_segments_from(dev(eng, audio), n, fs, state=torch.stack([state[i] for i in live]), first=[pos[i] for i in live])
        seg, peak = to_np(seg), to_np(peak)
        for j, i in enumerate(live):
            S = lr.segments_count(n[j], fs)
            assert not seg[j, S:].any(), "zeros behind the piece's segments"
            segs[i].append(seg[j, :S])
            peaks[i].append(peak[j])
            state[i] = out[j]
            pos[i] += n[j]
    return [np.concatenate(s) for s in segs], [np.max(p) for p in peaks]


@pytest.mark.parametrize("fs, segments", [(44100, 195), (22050, 195), (48000, 195), (8000, 130)])
def test_segments_carried_across_calls_equal_the_whole_call(eng, fs, segments):
    """44.1 and 8 kHz: the partial lane ends a segment; 48 kHz: 64 full lane runs end it (kw.p == 0), at 22.05 kHz 63 of them
    (lane 63 is empty)."""
    h = lr.segment_samples(fs)
    r = (h + 63) // 64
    assert (h % r == 0) == (fs in (22050, 48000)) and (h // r == 64) == (fs == 48000)
    xs = carried_streams(fs, segments)
    audio, n = lr.pack(xs)
    whole, peak = eng.loudness_segments(dev(eng, audio), n, fs)
    again, peak2, _ = eng.loudness_segments_from(dev(eng, audio), n, fs)
    assert same(to_np(whole), to_np(again)) and same(to_np(peak), to_np(peak2))          # no state in: the plain call's bits
    whole, peak = to_np(whole), to_np(peak)
    segs, peaks = in_pieces(eng, fs, xs, CUTS[segments])
    for b in range(len(xs)):
        S = lr.segments_count(n[b], fs)
        assert S == segments + 1 and same(segs[b], whole[b, :S]), (fs, b, "seg")
        assert np.float32(peaks[b]).tobytes() == peak[b].tobytes() == np.abs(xs[b]).max().tobytes(), (fs, b, "peak")
    if fs != 8000:
        return
    # against the restatement, within the row's gate (its yardstick: the float32 run of the same recurrence)
    x = xs[0]
    s64 = lr.segments(lr.kfilter(x, fs, np.float64), len(x), fs)
    L64 = lr.gate(s64, len(x), fs, detail=True)[-1]
    L32 = lr.gate(lr.segments(lr.kfilter(x, fs, np.float32), len(x), fs), len(x), fs, detail=True)[-1]
    gate_lu = min(max(4.0 * abs(L64 - L32), 1e-5), 0.1)
    err = np.abs(segs[0] - s64) / s64
    print(f"fs {fs}: {segments} segments in pieces, worst segment error {err.max():.3g} relative; gate {gate_lu:.3g} LU")
    assert err.max() <= 10.0 ** (gate_lu / 10.0) - 1.0


# ---------------------------------------------------------------------------------------------- the tables on audio
@pytest.fixture(scope="module")
def profiled(eng):
    """Per rate: the restatement's rows and the fused call's tables of them as ONE ragged batch (a meter: no params)."""
    out = {}
    for fs in (44100, 22050, 8000):
        rows = ltr.measured_rows(fs)
        audio, n = lr.pack([r["x"] for r in rows])
        d = dev(eng, audio)
        r = eng.loudness_level(d, n, fs)
        out[fs] = dict(rows=rows, audio=audio, n=n, dev=d, **{k: to_np(v) for k, v in r.items()})
    return out


@pytest.mark.parametrize("fs", [44100, 22050, 8000])
def test_tables_over_time_on_audio(profiled, eng, fs):
    p = profiled[fs]
    h = lr.segment_samples(fs)
    lufs, _, _ = eng.loudness(p["dev"], p["n"], fs)
    assert same(p["i_end"], to_np(lufs))                                                 # I_end IS the row's loudness
    assert same(to_np(p["dev"]), p["audio"])                                             # a meter writes no sample
    worst = 0.0
    for b, r in enumerate(p["rows"]):
        F = r["n"] // h
        assert p["M"].shape[1] == max(1, max(p["n"]) // h)
        assert np.isnan(p["M"][b, F:]).all() and np.isnan(p["S"][b, F:]).all() and np.isnan(p["I"][b, F:]).all() and (p["kept"][b, F:] == -1).all()
        assert np.array_equal(p["kept"][b, :F], r["kept_s"]), (r["name"], "kept at every prefix")
        for k, ref in (("M", r["M64"]), ("S", r["S64"]), ("I", r["I64"])):
            got, ref = p[k][b, :F].astype(np.float64), np.array(ref, np.float64)
            assert np.array_equal(got == -np.inf, ref == -np.inf), (r["name"], k, "-inf exactly where specified")
            fin = np.isfinite(ref)
            if fin.any():
                d = float(np.abs(got[fin] - ref[fin]).max())
                worst = max(worst, d / r["gate_lu"])
                assert d <= r["gate_lu"] <= 0.1, (r["name"], k, d, r["gate_lu"])
        fin = lambda v: v[np.isfinite(v)]
        for k, t in (("m_max", "M"), ("s_max", "S")):
            want = fin(p[t][b, :F]).max() if fin(p[t][b, :F]).size else -np.inf
            assert p[k][b] == want, (r["name"], k)
        if r["n"] >= 4 * h:
            assert bits(p["I"][b, F - 1: F])[0] == bits(p["i_end"][b: b + 1])[0], r["name"]
    print(f"fs {fs}: {len(p['rows'])} rows, worst |table - restatement| {worst:.3g} of the row's gate")


def test_a_row_alone_and_the_operators_give_the_bits_of_the_fused_batch(profiled, eng):
    fs = 22050
    p = profiled[fs]
    h = lr.segment_samples(fs)
    seg, _ = eng.loudness_segments(p["dev"], p["n"], fs)
    F = [n // h for n in p["n"]]
    M, S, I, kept, m_max, s_max = eng.loudness_time(seg, 0, F, fs)
    for k, t in (("M", M), ("S", S), ("I", I), ("kept", kept), ("m_max", m_max), ("s_max", s_max)):
        assert same(to_np(t), p[k]), k
    for b in (0, 4, len(p["rows"]) - 1):
        x = np.concatenate([p["rows"][b]["x"], np.full(3, NAN, np.float32)])[None, :]
        r = eng.loudness_level(dev(eng, x), [p["n"][b]], fs)
        for k in ("M", "S", "I", "kept"):
            assert same(to_np(r[k])[0, : F[b]], p[k][b, : F[b]]), (b, k)
        assert same(to_np(r["i_end"]), p["i_end"][b: b + 1])


# ---------------------------------------------------------------------------------------------- the table operator alone
def test_table_operator_on_constructed_tables(eng):
    fs = lr.TABLE_FS
    h = lr.segment_samples(fs)
    rows = ltr.time_tables_rows()
    assert {len(r) for r in rows} >= {1, 3, 4, 5, 29, 30, 31, 64, 65, 130}
    table = np.full((len(rows), 131), NAN)
    for b, seg in enumerate(rows):
        table[b, : len(seg)] = seg
    t = dev(eng, table)
    count = [len(r) for r in rows]
    M, S, I, kept, m_max, s_max = (to_np(v) for v in eng.loudness_time(t, 0, count, fs))
    worst = 0.0
    for b, seg in enumerate(rows):
        m, s, i, k, *_ = ltr.time_tables(seg, len(seg) * h, fs)
        assert np.array_equal(kept[b, : len(seg)], k), (b, "kept, its exact ties held at every prefix")
        for got, ref in ((M[b], m), (S[b], s), (I[b], i)):
            got = got[: len(seg)]
            assert np.array_equal(got == -np.inf, ref == -np.inf)
            fin = np.isfinite(ref)
            if fin.any():
                worst = max(worst, float(np.abs(got[fin].astype(np.float64) - ref[fin]).max()))
        assert np.isnan(M[b, len(seg):]).all() and (kept[b, len(seg):] == -1).all()
        assert m_max[b] == m.max() and s_max[b] == s.max()
    print(f"table operator: {len(rows)} tables, worst |value - restatement| {worst:.3g} LU")
    assert worst <= 1e-6
    # a call for [first, first + count) gives the same entries of the full call, bit for bit; rows given apart, as a stream's
    first = [min(len(r) - 1, f) for r, f in zip(rows, [0, 1, 3, 2, 40, 64, 100, 2, 0, 3, 28, 29, 30, 63, 1, 129])]
    cnt = [min(len(r) - f, c) for r, f, c in zip(rows, first, [1, 2, 1, 3, 24, 1, 30, 2, 5, 3, 1, 1, 1, 1, 64, 1])]
    segs = [dev(eng, r) for r in rows]
    tabs = tuple([torch.full((len(r),), 7, dtype=dt, device=eng.device) for r in rows] for dt in (torch.float32,) * 3 + (torch.int32,))
    _, _, _, _, m2, s2 = eng.loudness_time(segs, first, cnt, fs, tables=tabs)
    for b in range(len(rows)):
        f, c = first[b], cnt[b]
        for part, full in zip(tabs, (M, S, I, kept)):
            got = to_np(part[b])
            assert same(got[f: f + c], full[b, f: f + c]) and (got[:f] == 7).all() and (got[f + c:] == 7).all(), b
        assert to_np(m2)[b] == M[b, f: f + c].max() and to_np(s2)[b] == S[b, f: f + c].max()


# ---------------------------------------------------------------------------------------------- gains and apply
def level_rows(fs):
    """(samples, params, what binds)."""
    step = ltr.step_row(fs)
    d = lambda **k: dict(ltr.DEFAULTS, **k)
    quiet = np.concatenate([np.zeros(fs, np.float32), lr.tone(fs, 2 * fs + 11, 997.0, 0.1)])
    return [(step, d(target_lufs=-16.0, slew_db_per_s=1.0), "slew"), (step, d(target_lufs=-16.0, slew_db_per_s=20.0, initial_gain_db=-3.0), None),
            (lr.tone(fs, 3 * fs + 1, 997.0, 1e-3), d(slew_db_per_s=20.0), "max_gain"),
            (lr.tone(fs, 3 * fs, 997.0, 0.9), d(slew_db_per_s=20.0, max_cut_db=6.0), "max_cut"),
            (np.zeros(2 * fs + 5, np.float32), d(initial_gain_db=2.5), "zeros"), (quiet, d(target_lufs=-20.0, slew_db_per_s=10.0), "late"),
            (step[: fs + 3], d(target_lufs=NAN), "alone")]


@pytest.fixture(scope="module")
def levelled(eng):
    fs = 44100
    rows = level_rows(fs)
    audio, n = lr.pack([r[0] for r in rows])
    if audio.shape[1] % 2 == 0:                            # an odd stride: rows that are not 16-byte aligned
        audio = np.concatenate([audio, np.full((len(rows), 1), NAN, np.float32)], axis=1)
    d = dev(eng, audio)
    r = eng.loudness_level(d, n, fs, [p for _, p, _ in rows])                                 # in place
    assert r["out"] is d
    return dict(fs=fs, rows=rows, audio=audio, n=n, **{k: to_np(v) for k, v in r.items()})


def test_gains_equal_the_float32_restatement_on_the_devices_own_level(levelled):
    g = levelled
    h = lr.segment_samples(g["fs"])
    for b, (x, p, binds) in enumerate(g["rows"]):
        F = len(x) // h
        if binds == "alone":
            assert np.isnan(g["c_db"][b]).all() and np.isnan(g["c"][b]).all()                 # never written
            continue
        c_db, _ = ltr.level_gains(g["I"][b, :F], **p)
        assert same(g["c_db"][b, :F], c_db), (b, binds, "c_dB bit for bit")
        assert np.isnan(g["c_db"][b, F:]).all()
        want = 10.0 ** (g["c_db"][b, :F].astype(np.float64) / 20.0)
        assert (np.abs(g["c"][b, :F] - want) <= 1e-6 * want).all(), (b, "c")
        steps = np.abs(np.diff(np.concatenate([[np.float32(p["initial_gain_db"])], c_db]).astype(np.float64)))
        d = float(np.float32(p["slew_db_per_s"]) / np.float32(10.0))
        assert steps.max() <= d * (1 + 1e-4)                    # (the steps are differences of rounded float32 sums)
        if binds == "slew":
            assert (steps >= d * (1 - 1e-4)).sum() > 20
        elif binds is None:
            assert (steps[10:] < d * 0.999).all() and np.ptp(c_db) > 1.0                       # 20 dB/s does not bind: it follows I
        elif binds == "max_gain":
            assert c_db[-1] == np.float32(12.0) and g["I"][b, F - 1] < -50.0
        elif binds == "max_cut":
            assert c_db[-1] == np.float32(-6.0) and g["I"][b, F - 1] > -10.0
        elif binds == "zeros":
            assert (g["I"][b, :F] == -np.inf).all() and (c_db == np.float32(2.5)).all()
        elif binds == "late":
            assert (c_db[:10] == 0.0).all() and c_db[-1] != 0.0 and (g["I"][b, :10] == -np.inf).all()


def test_apply_is_the_float32_restatement_on_the_devices_own_gains(levelled, eng):
    g = levelled
    fs = g["fs"]
    h = lr.segment_samples(fs)
    for b, (x, p, binds) in enumerate(g["rows"]):
        n = g["n"][b]
        assert same(g["out"][b, n:], g["audio"][b, n:]), (b, "behind the row")                 # the NaN it held
        if binds == "alone":
            assert same(g["out"][b], g["audio"][b])
            continue
        want = ltr.level_apply(x, g["c"][b, : n // h], ltr.linear([p["initial_gain_db"]])[0], fs)
        assert same(g["out"][b, :n], want), (b, binds)
    assert not same(g["out"][0, : g["n"][0]], g["audio"][0, : g["n"][0]])
    # out of place on aligned rows, into a sentinel; the source is read only
    B, L = g["audio"].shape
    stride = (L + 3) // 4 * 4 + 4
    src = torch.full((B, stride), NAN, dtype=torch.float32, device=eng.device)
    src[:, :L] = dev(eng, g["audio"])
    dst = torch.full((B, stride), 7.0, dtype=torch.float32, device=eng.device)
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    r = eng.loudness_level(src, g["n"], fs, [p for _, p, _ in g["rows"]], out=dst)
    assert r["out"] is dst
    out = to_np(dst)
    for b in range(B):
        n = g["n"][b]
        if g["rows"][b][2] == "alone":
            assert (out[b] == 7.0).all()
            continue
        assert same(out[b, :n], g["out"][b, :n]) and (out[b, n:] == 7.0).all(), b
    for k in ("M", "S", "I", "kept", "c_db", "c", "i_end"):
        assert same(to_np(r[k]), g[k]), k
    assert same(to_np(src)[:, :L], g["audio"])


def test_apply_lengths_around_a_segment(eng):
    fs = 8000
    h = lr.segment_samples(fs)
    lengths = (1, h - 1, h, h + 1, 2 * h + 1)
    p = dict(ltr.DEFAULTS, target_lufs=-10.0, slew_db_per_s=20.0, initial_gain_db=-1.0)
    x = lr.tone(fs, max(lengths), 997.0, 0.1)
    for shift in (0, 1):                                   # rows at a multiple of 16 bytes, and not
        audio = np.full((len(lengths), max(lengths) + 3 + shift), NAN, np.float32)
        for b, n in enumerate(lengths):
            audio[b, :n] = x[:n]
        d = dev(eng, audio)
        r = eng.loudness_level(d, lengths, fs, [p] * len(lengths))
        out, c = to_np(d), to_np(r["c"])
        for b, n in enumerate(lengths):
            want = ltr.level_apply(x[:n], c[b, : n // h], ltr.linear([-1.0])[0], fs)
            assert same(out[b, :n], want) and np.isnan(out[b, n:]).all(), (shift, n)
        assert c[4, 1] > c[4, 0] > ltr.linear([-1.0])[0]
        assert out[4, 2 * h] != np.float32(ltr.linear([-1.0])[0] * x[2 * h])                   # the partial last segment is levelled too


def test_the_fused_call_gives_the_bits_of_the_separate_calls(levelled, eng):
    g = levelled
    fs = g["fs"]
    h = lr.segment_samples(fs)
    params = [p for _, p, _ in g["rows"]]
    d = dev(eng, g["audio"])
    seg, peak = eng.loudness_segments(d, g["n"], fs)
    F = [n // h for n in g["n"]]
    M, S, I, kept, m_max, s_max = eng.loudness_time(seg, 0, F, fs)
    c_db, c = eng.loudness_level_gains(I, 0, F, params)
    out = eng.loudness_level_apply(d, 0, c, F, fs, params, n_samples=g["n"], out=d)
    assert out is d
    for k, t in (("M", M), ("S", S), ("I", I), ("kept", kept), ("m_max", m_max), ("s_max", s_max), ("c_db", c_db), ("c", c), ("peak", peak),
                 ("out", out)):
        assert same(to_np(t), g[k]), k
    # gains in two calls continue from the row's own table
    c_db2, c2 = eng.loudness_level_gains(I, 0, [f // 2 for f in F], params)
    assert c_db2.shape[1] == max(F) // 2
    wide = (torch.full_like(c_db, NAN), torch.full_like(c, NAN))
    eng.loudness_level_gains(I, 0, [f // 2 for f in F], params, tables=wide)
    eng.loudness_level_gains(I, [f // 2 for f in F], [f - f // 2 for f in F], params, tables=wide)
    assert same(to_np(wide[0]), g["c_db"]) and same(to_np(wide[1]), g["c"])


# ---------------------------------------------------------------------------------------------- streams
def _split(n, cuts):
    edges = [0]
    for c in cuts:
        if edges[-1] >= n:
            break
        edges.append(min(n, edges[-1] + c))
    if edges[-1] < n:
        edges.append(n)
    return list(zip(edges[:-1], edges[1:]))


@pytest.fixture(scope="module")
def stream_rows(eng):
    """Three rows at 8 kHz and the ONE call on each whole row."""
    fs = 8000
    step = ltr.step_row(fs)
    rows = [(step, dict(target_lufs=-16.0, slew_db_per_s=20.0, initial_gain_db=-2.0)),
            (lr.tone(fs, 41 * 800 + 799, 997.0, 0.02), dict(target_lufs=-23.0, slew_db_per_s=5.0, max_gain_db=6.0)), (step[: 33 * 800 + 1], None)]
    whole = []
    for x, p in rows:
        r = eng.loudness_level(dev(eng, x[None, :].copy()), [len(x)], fs, None if p is None else [p])
        whole.append({k: to_np(v)[0] for k, v in r.items()})
    return fs, rows, whole


def _check_stream(st, outs, x, p, w, h):
    F = len(x) // h
    assert st.segments == F and st.seen == len(x)
    for k in ("M", "S", "I", "kept") + (("c_db", "c") if p else ()):
        assert same(to_np(st.table[k]), w[k][:F]), k
    got = np.concatenate([to_np(o) for o in outs])
    assert same(got, w["out"][: len(x)] if p else x)
    fin = lambda v: float(v[np.isfinite(v)].max()) if np.isfinite(v).any() else -math.inf
    assert st.integrated == float(w["I"][F - 1]) and st.momentary_max == fin(w["M"][:F]) == float(w["m_max"])
    assert st.short_term_max == fin(w["S"][:F]) == float(w["s_max"])
    assert st.gain_db == (float(w["c_db"][F - 1]) if p else None)


@pytest.mark.parametrize("cuts", ["whole", "pieces", "random"])
def test_a_stream_under_any_split_equals_the_one_call(stream_rows, eng, cuts):
    from vispeech_amd import loudness
    fs, rows, whole = stream_rows
    h = lr.segment_samples(fs)
    x, p = rows[0]
    cuts = {"whole": [len(x)], "pieces": [1, 7, h - 1, h, h + 1, 3 * h + 5] * 12,
            "random": np.random.default_rng(8).integers(1, 4 * h, size=64).tolist()}[cuts]
    st = loudness.Stream(eng, fs, level=p)
    d = dev(eng, x)
    pieces = _split(len(x), cuts)
    outs = [st.push(d[a:b], final=(b == len(x))) for a, b in pieces]
    assert [o.numel() for o in outs] == [b - a for a, b in pieces]                        # every sample leaves in its own push
    assert same(to_np(d), x)                                                              # the caller's samples are read only
    _check_stream(st, outs, x, p, whole[0], h)


def test_three_streams_at_their_own_positions_in_one_push_rows(stream_rows, eng):
    from vispeech_amd import loudness
    fs, rows, whole = stream_rows
    h = lr.segment_samples(fs)
    sts = [loudness.Stream(eng, fs, level=p if p else True) for _, p in rows]
    ds = [dev(eng, x) for x, _ in rows]
    plans = [_split(len(rows[0][0]), [3 * h + 5, 1, h - 1] * 40), _split(len(rows[1][0]), [h, 2 * h + 1, 7] * 40),
             _split(len(rows[2][0]), [h + 1, 5 * h] * 40)]
    outs = [[] for _ in rows]
    for t in range(max(len(pl) for pl in plans)):
        live = [i for i, pl in enumerate(plans) if t < len(pl)]
        got = loudness.push_rows(eng, [(sts[i], ds[i][plans[i][t][0]: plans[i][t][1]], t == len(plans[i]) - 1) for i in live])
        for i, o in zip(live, got):
            outs[i].append(o)
    for i, (x, p) in enumerate(rows):
        _check_stream(sts[i], outs[i], x, p, whole[i], h)


# ---------------------------------------------------------------------------------------------- the model and the service
TEXT_FRAMES, TEXT_PHONEMES, TEXT_SEEDS = [60, 48], [9, 7], [511, 512]
N_REC, SRC, TGT, CONV_SEED = 4708, 5, 20, 611             # a recording of 9 frames
MODEL = 44100


@pytest.fixture(scope="module")
def net():
    from vispeech_amd import config as vcfg
    from vispeech_amd.models import SynthesizerTrn
    from vispeech_amd.schema import dims_from_ctor
    from vispeech_amd.synth import synth_state_dict
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    ctor = vcfg.synthesizer_args(vcfg.default_hparams())
    m = SynthesizerTrn(*ctor[0], **ctor[1]).eval()
    m.load_state_dict(synth_state_dict(dims_from_ctor(*ctor[0], **ctor[1]), seed=1234), strict=True)
    return m


def test_the_models_two_calls(net, profiled):
    p = profiled[MODEL]
    M, S, I, m_max, s_max, i_end = net.loudness_profile(p["dev"], p["n"])
    for k, t in (("M", M), ("S", S), ("I", I), ("m_max", m_max), ("s_max", s_max), ("i_end", i_end)):
        assert same(to_np(t), p[k]), k
    x = p["rows"][-1]["x"]                                  # the step row
    wave, c_db = net.level(dev(net._engine, x[None, :].copy()), [len(x)], target_lufs=-16.0, slew_db_per_s=20)
    want_db, c = ltr.level_gains(p["I"][-1, : len(x) // 4410], target_lufs=-16.0, slew_db_per_s=20.0)
    assert same(to_np(c_db)[0], want_db)
    got = to_np(wave)[0]
    # (c is compared in bits elsewhere; here the restatement's own c, which may differ from the device's in its last place)
    assert np.abs(got - ltr.level_apply(x, c, np.float32(1.0), MODEL)).max() <= 2e-6 * np.abs(got).max() and not same(got, x)


def _streamed(net, batch, rec, kws):
    """A text request, a conversion and a second text request join at ticks 0, 1 and 2; chunks of 8 frames; driven by step()."""
    from vispeech_amd.service import StreamingBatchService
    collate = lambda rows: {k: batch[k][rows] for k in ("phonemes", "lengths", "sid", "duration", "f0", "energy")}
    svc = StreamingBatchService(net, max_batch=3, chunk_frames=8, collate=collate, autostart=False)
    streams = [svc.submit(0, TEXT_SEEDS[0], **kws[0])]
    svc.step()
    streams.append(svc.submit_conversion(rec, SRC, TGT, CONV_SEED, **kws[1]))
    svc.step()
    streams.append(svc.submit(1, TEXT_SEEDS[1], **kws[2]))
    svc.close()
    return streams, [b"".join(s) for s in streams]


def _row_bytes(eng, wave, fmt):
    from vispeech_amd import output_stage
    buf, spans = eng.output_batch(wave.reshape(1, -1), [wave.numel()], [fmt])
    return output_stage.unpack(to_np(buf), spans, [output_stage.encoding(fmt[1])])[0].tobytes()


def test_streaming_service_requests_equal_the_direct_path(net):
    import isolated_ref as iso
    batch = iso.make_batch(TEXT_FRAMES, TEXT_PHONEMES, seed=2230)
    t = np.arange(N_REC) / 44100.0
    rec = (0.4 * np.sin(2 * np.pi * 220.0 * t) + 0.1 * np.random.default_rng(33).standard_normal(N_REC)).astype(np.float32).clip(-1, 1)
    eng, up = net._engine, net.dims.total_upsample
    f32 = dict(output_rate=MODEL, output_encoding="f32")
    _, plain = _streamed(net, batch, rec, [{}, {}, {}])
    _, raw = _streamed(net, batch, rec, [f32] * 3)
    floats = [torch.from_numpy(np.frombuffer(b, "<f4").copy()).to(net.device) for b in raw]        # the whole generator output
    assert [f.numel() for f in floats] == [60 * up, 9 * up, 48 * up]
    ceiling = 0.5 * float(floats[0].abs().max())
    level = dict(target_lufs=-16.0, slew_db_per_s=20.0)
    streams, got = _streamed(net, batch, rec, [dict(loudness=level, limiter=dict(ceiling=ceiling), output_rate=8000, output_encoding="ulaw"),
                                               dict(loudness=-16), {}])
    # the text request: level, limit, output rows on its whole waveform
    n = floats[0].numel()
    wave, c_db = net.level(floats[0].clone().reshape(1, -1), [n], **level)
    assert not same(to_np(wave)[0], to_np(floats[0])) and np.ptp(to_np(c_db)[0]) > 1.0
    y, mg = net.limit(wave, [n], ceiling=ceiling)
    assert float(mg[0]) < 1.0
    assert got[0] == _row_bytes(eng, y[0], (8000, "ulaw"))
    info = streams[0].loudness
    F = n // 4410
    M, S, I, m_max, s_max, _ = net.loudness_profile(floats[0].reshape(1, -1), [n])
    assert info == dict(integrated=float(I[0, F - 1]), momentary_max=float(m_max[0]), short_term_max=float(s_max[0]),
                        gain_db=float(c_db[0, F - 1]))
    # the conversion: the leveller alone, at its defaults
    n = floats[1].numel()
    wave, c_db = net.level(floats[1].clone().reshape(1, -1), [n], target_lufs=-16.0)
    assert got[1] == _row_bytes(eng, wave[0], (MODEL, "s16")) and got[1] != plain[1]
    assert streams[1].loudness["gain_db"] == float(c_db[0, n // 4410 - 1])
    # the bystander equals the run in which nobody names a level
    assert got[2] == plain[2] and len(got[2]) == 2 * 48 * up and streams[2].loudness is None
