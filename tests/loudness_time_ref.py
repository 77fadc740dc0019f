"""Loudness over time and the leveller restated in numpy, on top of tests/loudness_ref.py (whose
K-weighting, segments, blocks and gates are section 4p's and are used as they are).  Nothing here is shared with the library.
Tables are fp64 until their last rounding to float32; the leveller's gain in dB is float32 adds, subtracts, mins and maxes,
which numpy's float32 scalars perform exactly as the device does, so ``level_gains`` and ``level_apply`` are bit-exact
references for the device's own inputs."""
from __future__ import annotations

import math

import numpy as np

import loudness_ref as lr

DEFAULTS = dict(target_lufs=-23.0, max_gain_db=12.0, max_cut_db=12.0, slew_db_per_s=3.0, initial_gain_db=0.0)


def lufs(E: float, D: float) -> float:
    return -0.691 + 10.0 * math.log10(E / D) if E > 0 else -math.inf


def time_tables(seg, n: int, fs: int):
    """``(M, S, I, kept, M64, S64, I64)`` over the F = n // h complete segments of a row with the segment table ``seg``:
    float32 tables and kept counts, then the same values before their rounding (python floats)."""
    h = lr.segment_samples(fs)
    F = int(n) // h
    seg = np.asarray(seg, np.float64)
    M64, S64, I64, kept = [], [], [], []
    for s in range(F):
        M64.append(lufs(((float(seg[s - 3]) + float(seg[s - 2])) + float(seg[s - 1])) + float(seg[s]), 4.0 * h) if s >= 3 else -math.inf)
        T = 0.0
        if s >= 29:
            for k in range(s - 29, s + 1):
                T = T + float(seg[k])
        S64.append(lufs(T, 30.0 * h) if s >= 29 else -math.inf)
        g = lr.gate(seg[: s + 1], (s + 1) * h, fs, detail=True)
        I64.append(g[-1])
        kept.append(g[2])
    f32 = lambda v: np.array(v, dtype=np.float64).astype(np.float32)
    return f32(M64), f32(S64), f32(I64), np.array(kept, dtype=np.int32), M64, S64, I64


def level_gains(I, target_lufs=-23.0, max_gain_db=12.0, max_cut_db=12.0, slew_db_per_s=3.0, initial_gain_db=0.0, c_db_prev=None):
    """``(c_dB, c)`` float32 for the running levels ``I`` (float32; -inf: no level yet), from ``c_db_prev`` (None: the
    initial gain).  Every operation on c_dB is a float32 add, subtract, min or max."""
    f = np.float32
    target, hi, lo = f(target_lufs), f(max_gain_db), -f(max_cut_db)
    d = f(slew_db_per_s) / f(10.0)
    prev = f(initial_gain_db) if c_db_prev is None else f(c_db_prev)
    out = np.empty(len(I), np.float32)
    for s, Is in enumerate(np.asarray(I, np.float32)):
        q = prev if Is == -np.inf else min(max(f(target - Is), lo), hi)
        prev = f(prev + min(max(f(q - prev), -d), d))
        out[s] = prev
    return out, linear(out)


def linear(c_db) -> np.ndarray:
    """fl32(10^(c_dB / 20)), the power in double."""
    return (10.0 ** (np.asarray(c_db, np.float32).astype(np.float64) / 20.0)).astype(np.float32)


def level_apply(x, c, c_init, fs: int, pos: int = 0) -> np.ndarray:
    """The stream's samples ``[pos, pos + len(x))`` against its gain table ``c`` (float32, entry s the gain reached at the
    end of segment s; ``c_init`` = c[-1]): every product and sum a float32 operation of its own."""
    f = np.float32
    h = lr.segment_samples(fs)
    rh = f(1.0) / f(h)
    x = np.asarray(x, np.float32)
    i = pos + np.arange(len(x), dtype=np.int64)
    s, k = i // h, i % h
    tab = np.concatenate([[f(c_init), f(c_init)], np.asarray(c, np.float32)])        # tab[s + 2] = c[s]
    c0, c1 = tab[s], tab[s + 1]                                                       # c[s - 2], c[s - 1]
    w = ((k + 1).astype(np.float32) * rh).astype(np.float32)
    a = (c0 + ((c1 - c0).astype(np.float32) * w).astype(np.float32)).astype(np.float32)
    return (a * x).astype(np.float32)


def level(x, n: int, fs: int, **params):
    """The whole restatement of a row in fp64: ``dict(M, S, I, kept, c_db, c, out, I_end)``."""
    p = dict(DEFAULTS, **params)
    seg = lr.segments(lr.kfilter(np.asarray(x)[:n], fs), n, fs)
    M, S, I, kept, *_ = time_tables(seg, n, fs)
    c_db, c = level_gains(I, **p)
    out = level_apply(np.asarray(x)[:n], c, linear([p["initial_gain_db"]])[0], fs)
    return dict(M=M, S=S, I=I, kept=kept, c_db=c_db, c=c, out=out, I_end=lr.gate(seg, n, fs)[0], seg=seg)


# ---------------------------------------------------------------------------------------------- the rows of the tests
def step_row(fs: int) -> np.ndarray:
    """220 Hz at amplitudes 0.1, 0.2 and 0.07 for 2 s each, plus 7 samples; DC 0.05 and 3 Hz of 0.02 as the main signal."""
    n = 6 * fs + 7
    t = np.arange(n, dtype=np.float64) / fs
    amp = np.select([t < 2.0, t < 4.0], [0.1, 0.2], 0.07)
    return (amp * np.sin(2 * np.pi * 220.0 * t) + 0.05 + 0.02 * np.sin(2 * np.pi * 3.0 * t)).astype(np.float32)


def audio_rows(fs: int):
    return lr.audio_rows(fs) + [("step", step_row(fs))]


_CACHE = {}


def measured_rows(fs: int):
    """``loudness_ref.measured_rows(fs)`` and the step row, each with the restatement's tables over time: dict(name, x, n,
    seg, gate_lu, M, S, I, kept, M64, S64, I64, L) -- ``gate_lu`` as there: 4 times the distance of the float32 recurrence
    from the fp64 one, at least 1e-5 LU, at most 0.1 LU."""
    if fs in _CACHE:
        return _CACHE[fs]
    rows = [dict(r) for r in lr.measured_rows(fs)]
    x = step_row(fs)
    n = len(x)
    seg = lr.segments(lr.kfilter(x, fs, np.float64), n, fs)
    L, NB, _, kept, _, _, _, L64 = lr.gate(seg, n, fs, detail=True)
    L32 = lr.gate(lr.segments(lr.kfilter(x, fs, np.float32), n, fs), n, fs, detail=True)[-1]
    err = abs(L64 - L32)
    rows.append(dict(name="step", x=x, n=n, seg=seg, L=L, L64=L64, NB=NB, kept=kept, peak=np.float32(np.max(np.abs(x))), yardstick=err,
                     gate_lu=min(max(4.0 * err, 1e-5), 0.1)))
    for r in rows:
        M, S, I, k, M64, S64, I64 = time_tables(r["seg"], r["n"], fs)
        r.update(M=M, S=S, I=I, kept_s=k, M64=M64, S64=S64, I64=I64)
    _CACHE[fs] = rows
    return rows


def prefix_margins(seg, n: int, fs: int):
    """The smallest ``loudness_ref.gate_margins`` over EVERY prefix of complete segments of a row: ``(absolute, relative)``."""
    h = lr.segment_samples(fs)
    fa = fr = math.inf
    for s in range(int(n) // h):
        a, r = lr.gate_margins(seg[: s + 1], (s + 1) * h, fs)
        fa, fr = min(fa, a), min(fr, r)
    return fa, fr


# ---------------------------------------------------------------------------------------------- constructed tables
def time_tables_rows():
    """Double tables for the table operator alone, ``[seg]`` at ``loudness_ref.TABLE_FS`` (a row of S segments is S h
    samples): ``loudness_ref.gate_tables()``'s rows that are whole segments, and rows of 29, 30, 31 (the short-term edge)
    and 64, 65, 130 segments.  Every value is a small multiple of a power of two: every sum is exact in any order."""
    h = lr.segment_samples(lr.TABLE_FS)
    rows = [seg for seg, n in lr.gate_tables() if n == len(seg) * h]
    rng = np.random.default_rng(23)
    for S in (29, 30, 31, 64, 65, 130):
        rows.append(rng.integers(1, 40, size=S).astype(np.float64) * 0.25)
    return rows


# ---------------------------------------------------------------------------------------------- a numpy engine
class NumpyEngine:
    """The engine of ``vispeech_amd.loudness`` in numpy: the methods ``loudness.Stream`` drives, on numpy arrays, computed by
    this file's restatement (so a stream over it, under any split, must give ``level`` of the whole row in every bit)."""

    def __init__(self):
        self.calls = []

    def loudness_state(self, B: int):
        return np.zeros((B, 4), np.float64)

    def loudness_table(self, n: int, dtype):
        return np.full(n, -1 if np.dtype(dtype).kind == "i" else np.nan, dtype=dtype)

    def loudness_segments_from(self, audio, n_samples, sample_rate, state=None, first=None):
        fs = int(sample_rate)
        h = lr.segment_samples(fs)
        c = [float(v) for v in lr.kweighting(fs)]
        B = len(n_samples)
        self.calls.append(("segments_from", [int(n) for n in n_samples]))
        seg = np.zeros((B, lr.segments_count(max(n_samples), fs)))
        peak = np.zeros(B, np.float32)
        out = np.zeros((B, 4))
        for b in range(B):
            assert first is None or int(first[b]) % h == 0
            st = [0.0] * 4 if state is None else [float(v) for v in state[b]]
            out[b] = st
            n = int(n_samples[b])
            acc = []
            for i in range(n):
                v = float(audio[b][i])
                u = c[0] * v + st[0]
                st[0] = c[1] * v - c[3] * u + st[1]
                st[1] = c[2] * v - c[4] * u
                y = c[5] * u + st[2]
                st[2] = c[6] * u - c[8] * y + st[3]
                st[3] = c[7] * u - c[9] * y
                acc.append(y * y)
                if (i + 1) % h == 0 or i + 1 == n:
                    seg[b, i // h] = math.fsum(acc)
                    acc = []
                    if (i + 1) % h == 0:
                        out[b] = st
            peak[b] = np.max(np.abs(np.asarray(audio[b][:n], np.float32)))
        return seg, peak, out

    def loudness_time(self, seg, first, count, sample_rate, tables=None):
        fs = int(sample_rate)
        h = lr.segment_samples(fs)
        self.calls.append(("time", list(first), list(count)))
        M, S, I, kept = tables
        m_max, s_max = np.full(len(seg), -np.inf, np.float32), np.full(len(seg), -np.inf, np.float32)
        for b in range(len(seg)):
            f, n = int(first[b]), int(first[b]) + int(count[b])
            m, s, i, k, *_ = time_tables(seg[b][:n], n * h, fs)
            M[b][f:n], S[b][f:n], I[b][f:n], kept[b][f:n] = m[f:], s[f:], i[f:], k[f:]
            if n > f:
                m_max[b], s_max[b] = m[f:].max(), s[f:].max()
        return M, S, I, kept, m_max, s_max

    def loudness_level_gains(self, I, first, count, params, tables=None):
        self.calls.append(("level_gains", list(first), list(count)))
        c_db, c = tables
        for b, p in enumerate(params):
            f, n = int(first[b]), int(first[b]) + int(count[b])
            if math.isnan(p["target_lufs"]):
                continue
            c_db[b][f:n], c[b][f:n] = level_gains(I[b][f:n], c_db_prev=c_db[b][f - 1] if f else None, **p)
        return c_db, c

    def loudness_level_apply(self, x, pos, c, entries, sample_rate, params, n_samples=None, out=None):
        self.calls.append(("level_apply", list(pos), [len(v) for v in x]))
        x = [v.numpy() if hasattr(v, "numpy") else v for v in x]
        out = [np.array(v, np.float32) for v in x]
        for b, p in enumerate(params):
            if not math.isnan(p["target_lufs"]):
                out[b] = level_apply(x[b], c[b][: int(entries[b])], linear([p["initial_gain_db"]])[0], int(sample_rate), int(pos[b]))
        return out
