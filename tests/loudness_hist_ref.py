"""Loudness range and the histogram gate restated in numpy, on top of tests/loudness_ref.py and
tests/loudness_time_ref.py (whose K-weighting, segments, M and S are sections 4p / 4r's and are used as they are).  Nothing
here is shared with the library.  The state is two histograms of integer counts; every derived value is computed from the
counts alone, with exactly rounded sums (``math.fsum``): the specification leaves the summation order free, so a device
value may differ from this one in the last place of its float32 rounding, and in nothing else."""
from __future__ import annotations

import math

import numpy as np

import loudness_ref as lr
import loudness_time_ref as ltr

NB = 1000


def make_tables():
    """``(edges [1001], centres [1000])``: e_k = 10^((k - 693.09) / 100), c_k = 10^((k - 692.59) / 100), in double -- but
    e_0 by section 4p's own expression for Z_abs, 10^((-70 + 0.691) / 10): the same number, whose exponent rounds another
    way (the two differ by 2e-15), so that both gates share ONE absolute gate in every bit."""
    k = np.arange(NB + 1, dtype=np.float64)
    edges = np.power(10.0, (k - 693.09) / 100.0)
    edges[0] = lr.Z_ABS
    return edges, np.power(10.0, (k[:NB] - 692.59) / 100.0)


EDGES, CENTRES = make_tables()


def bin_of(z: float, edges=EDGES) -> int:
    """The bin of a mean square: -1 where ``not z >= e_0`` (the absolute gate), else the largest k <= 999 with e_k <= z.
    Comparisons against the table only."""
    if not z >= edges[0]:
        return -1
    return min(int(np.searchsorted(edges, z, side="right")) - 1, NB - 1)


def energies(seg, F: int):
    """``(E, T)`` per complete segment s < F: the energy of the 400 ms block and of the 3 s window that end at s (None before
    there is one), summed in section 4r's order."""
    seg = np.asarray(seg, np.float64)
    E, T = [], []
    for s in range(F):
        E.append(((float(seg[s - 3]) + float(seg[s - 2])) + float(seg[s - 1])) + float(seg[s]) if s >= 3 else None)
        t = 0.0
        if s >= 29:
            for k in range(s - 29, s + 1):
                t = t + float(seg[k])
        T.append(t if s >= 29 else None)
    return E, T


def mean_squares(seg, F: int, fs: int):
    """``(zB, zS)`` per complete segment s < F: E / (4 h) and T / (30 h), None before there is one."""
    h = lr.segment_samples(fs)
    E, T = energies(seg, F)
    return [None if e is None else e / (4.0 * h) for e in E], [None if t is None else t / (30.0 * h) for t in T]


def ms_tables(seg, F: int, fs: int):
    """``(M, S)`` float32 over the first F complete segments: section 4r's, without its running level."""
    h = lr.segment_samples(fs)
    E, T = energies(seg, F)
    f32 = lambda v: np.array(v, np.float64).astype(np.float32)
    return (f32([-math.inf if e is None else ltr.lufs(e, 4.0 * h) for e in E]),
            f32([-math.inf if t is None else ltr.lufs(t, 30.0 * h) for t in T]))


def level_of(HB, centres=CENTRES, detail: bool = False):
    """``(I_h as a python float before its rounding, kept)`` from the histogram of blocks; with ``detail`` also mean_abs."""
    HB = np.asarray(HB, np.int64)
    n_abs = int(HB.sum())
    if n_abs == 0:
        return (-math.inf, 0, None) if detail else (-math.inf, 0)
    mean_abs = math.fsum(HB * centres) / n_abs
    keep = 10.0 * centres > mean_abs
    kept = int(HB[keep].sum())
    I = -0.691 + 10.0 * math.log10(math.fsum(HB[keep] * centres[keep]) / kept) if kept else -math.inf
    return (I, kept, mean_abs) if detail else (I, kept)


def range_of(HS, centres=CENTRES, detail: bool = False):
    """The loudness range (float32, LU) from the histogram of 3 s windows; with ``detail`` also ``(mean, N, k10, k95)``."""
    HS = np.asarray(HS, np.int64)
    n = int(HS.sum())
    if n == 0:
        return (np.float32(0.0), None, 0, None, None) if detail else np.float32(0.0)
    mean = math.fsum(HS * centres) / n
    kept = np.where(100.0 * centres > mean, HS, 0)
    N = int(kept.sum())
    if N == 0:
        return (np.float32(0.0), mean, 0, None, None) if detail else np.float32(0.0)
    lo, hi = (N + 4) // 10, (95 * (N - 1) + 50) // 100
    cum = np.cumsum(kept)
    k10, k95 = int(np.argmax(cum > lo)), int(np.argmax(cum > hi))
    lra = np.float32(k95 - k10) / np.float32(10.0)
    return (lra, mean, N, k10, k95) if detail else lra


def advance(seg, first: int, count: int, fs: int, hist, tables=None):
    """The entries ``[first, first + count)`` of a row with the segment table ``seg`` (from segment 0), from the histograms
    ``hist`` ``[2, 1000]`` int32 -- the state after ``[0, first)``, taken as zero at ``first == 0`` --, which are advanced in
    place.  Returns ``dict(M, S, I, kept, I64, lra)`` over those entries (float32 tables, the levels before their rounding,
    and the range after the last entry)."""
    edges, centres = tables or (EDGES, CENTRES)
    if first == 0:
        hist[...] = 0
    F = first + count
    M, S, *_ = ms_tables(seg, F, fs)
    zB, zS = mean_squares(seg, F, fs)
    I64, kept = [], []
    for s in range(first, F):
        for row, z in ((0, zB[s]), (1, zS[s])):
            k = -1 if z is None else bin_of(z, edges)
            if k >= 0:
                hist[row, k] += 1
        i, n = level_of(hist[0], centres)
        I64.append(i)
        kept.append(n)
    return dict(M=M[first:], S=S[first:], I=np.array(I64, np.float64).astype(np.float32), kept=np.array(kept, np.int32), I64=I64,
                lra=range_of(hist[1], centres))


def whole(seg, n: int, fs: int, tables=None):
    """``advance`` over all F = n // h complete segments of a row from zero histograms, with the histograms: ``dict(M, S, I,
    kept, I64, lra, hist, i_hist)``."""
    F = int(n) // lr.segment_samples(fs)
    hist = np.zeros((2, NB), np.int32)
    r = advance(seg, 0, F, fs, hist, tables)
    r.update(hist=hist, i_hist=r["I"][-1] if F else np.float32(-np.inf))
    return r


def measure(x, n: int, fs: int, tables=None):
    """``whole`` of the fp64 restatement's segments of ``x[:n]``."""
    return whole(lr.segments(lr.kfilter(np.asarray(x)[:n], fs), n, fs), n, fs, tables)


# ---------------------------------------------------------------------------------------------- margins
def edge_distance(z: float, edges=EDGES) -> float:
    """The smallest relative distance of a mean square from any edge (1 for z = 0)."""
    return float(np.min(np.abs(z / edges - 1.0)))


def threshold_distance(mean: float, factor: float, centres=CENTRES) -> float:
    """The smallest relative distance of ``factor c_k`` from ``mean`` over the bins."""
    return float(np.min(np.abs(factor * centres / mean - 1.0)))


# ---------------------------------------------------------------------------------------------- the rows of the tests
def two_level(fs: int, half_s: float, db_a: float, db_b: float, f: float = 1000.0) -> np.ndarray:
    """A tone of ``f`` Hz in two equal halves of ``half_s`` seconds, at ``db_a`` then ``db_b`` dBFS (peak)."""
    n = int(round(half_s * fs))
    t = np.arange(2 * n, dtype=np.float64) / fs
    amp = np.where(np.arange(2 * n) < n, 10.0 ** (db_a / 20.0), 10.0 ** (db_b / 20.0))
    return (amp * np.sin(2 * np.pi * f * t)).astype(np.float32)


def edge_rows(edges=EDGES):
    """Double segment tables at ``loudness_ref.TABLE_FS`` for the operator alone, of F in {1, 3, 4, 29, 30, 31, 64, 65, 130}
    segments: mean squares between -45 and -20 LUFS, so that both relative gates cut.  The rows of 64 segments and more
    also hold ``plants``: each as a run of four equal segments q = z h, so that the block that ends the run has the mean
    square z in every bit (``planted_ok`` asserts that on the host) -- on an edge, the double below an edge, a zero and a
    value below e_0; the rows of 64 and 65 also a value above e_1000, which then is all their relative gates keep."""
    h = lr.segment_samples(lr.TABLE_FS)
    rng = np.random.default_rng(24)
    rows = []
    for F in (1, 3, 4, 29, 30, 31, 64, 65, 130):
        seg = h * np.power(10.0, rng.uniform(-4.5, -2.0, size=F))
        if F >= 64:
            for j, z in enumerate(plants(edges)):
                if z > edges[NB] and F == 130:
                    continue
                seg[8 + 5 * j: 12 + 5 * j] = z * h
        rows.append(seg)
    return rows


def plants(edges=EDGES):
    """Mean squares to plant: up to four on an edge and four one double below an edge (the first of the candidates k for which
    ``(((q + q) + q) + q) / (4 h) == z`` at q = z h, h = 800), then one above e_1000, a zero and one below e_0."""
    h = float(lr.segment_samples(lr.TABLE_FS))
    on, below = [], []
    for k in (0, 1000, 500, 999, 437, 1, 750, 250, 998, 2, 997, 3):
        z, y = float(edges[k]), float(np.nextafter(edges[k], 0.0))
        if roundtrips(z, h) and len(on) < 4:
            on.append(z)
        if roundtrips(y, h) and len(below) < 4:
            below.append(y)
    return on + below + [float(edges[NB]) * 8.0, 0.0, float(edges[0]) / 4.0]


def roundtrips(z: float, h: float) -> bool:
    q = z * h
    return (((q + q) + q) + q) / (4.0 * h) == z


def planted_ok(edges=EDGES) -> bool:
    h = float(lr.segment_samples(lr.TABLE_FS))
    p = plants(edges)
    on = [z for z in p if z in set(edges.tolist())]
    below = [z for z in p if float(np.nextafter(z, np.inf)) in set(edges.tolist())]
    return all(roundtrips(z, h) for z in p) and len(on) >= 2 and len(below) >= 2 and len(p) <= 11


# ---------------------------------------------------------------------------------------------- a numpy engine
class NumpyEngine(ltr.NumpyEngine):
    """``loudness_time_ref.NumpyEngine`` with the two methods a ``loudness.Stream(gate="histogram")`` drives."""

    def loudness_hist_state(self, B: int):
        return np.zeros((B, 2, NB), np.int32)

    def loudness_time_hist(self, seg, first, count, sample_rate, hist, tables=None):
        fs = int(sample_rate)
        self.calls.append(("time_hist", list(first), list(count)))
        M, S, I, kept = tables
        B = len(seg)
        m_max, s_max = np.full(B, -np.inf, np.float32), np.full(B, -np.inf, np.float32)
        lra = np.zeros(B, np.float32)
        for b in range(B):
            f, n = int(first[b]), int(first[b]) + int(count[b])
            r = advance(seg[b][:n], f, n - f, fs, hist[b])
            M[b][f:n], S[b][f:n], I[b][f:n], kept[b][f:n] = r["M"], r["S"], r["I"], r["kept"]
            lra[b] = r["lra"]
            if n > f:
                m_max[b], s_max[b] = r["M"].max(), r["S"].max()
        return M, S, I, kept, m_max, s_max, lra
