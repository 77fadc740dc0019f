"""The loudness specification (ITU-R BS.1770-4 / EBU R 128 integrated loudness of a mono row) restated
in fp64 numpy, and the rows the tests measure.  Nothing here is shared with the library: the filter is the plain sequential
recurrence of the two biquads (transposed direct form II, as ``scipy.signal.lfilter`` runs it), a sample at a time.  The
same recurrence can be run in float32 (``dtype``): its distance from the fp64 run is the yardstick of the GPU tests."""
from __future__ import annotations

import math

import numpy as np

Z_ABS = 10.0 ** ((-70.0 + 0.691) / 10.0)

SHELF = dict(f0=1681.974450955533, G=3.999843853973347, Q=0.7071752369554196)
HIGHPASS = dict(f0=38.13547087602444, Q=0.5003270373238773)


def kweighting(fs: float) -> np.ndarray:
    """[b0, b1, b2, a1, a2] of the shelf, then of the high-pass (a0 = 1)."""
    K = math.tan(math.pi * SHELF["f0"] / fs)
    Q = SHELF["Q"]
    Vh = 10.0 ** (SHELF["G"] / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
             2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    K = math.tan(math.pi * HIGHPASS["f0"] / fs)
    Q = HIGHPASS["Q"]
    a0 = 1.0 + K / Q + K * K
    hp = [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    return np.array(shelf + hp, dtype=np.float64)


def segment_samples(fs: int) -> int:
    return (int(fs) + 5) // 10


def segments_count(n: int, fs: int) -> int:
    h = segment_samples(fs)
    return (int(n) + h - 1) // h


def kfilter(x, fs: int, dtype=np.float64) -> np.ndarray:
    """The K-weighted row, from zero state, every operation in ``dtype``."""
    c = kweighting(fs)
    if dtype == np.float64:                       # (python floats are IEEE doubles: the same arithmetic, much faster)
        b0, b1, b2, a1, a2, c0, c1, c2, d1, d2 = (float(v) for v in c)
        xs = [float(v) for v in np.asarray(x, np.float32)]
        zero = 0.0
    else:
        b0, b1, b2, a1, a2, c0, c1, c2, d1, d2 = (dtype(v) for v in c)
        xs = list(np.asarray(x, np.float32).astype(dtype))
        zero = dtype(0)
    s1 = s2 = t1 = t2 = zero
    out = np.empty(len(xs), dtype=dtype)
    for i, v in enumerate(xs):
        u = b0 * v + s1
        s1 = b1 * v - a1 * u + s2
        s2 = b2 * v - a2 * u
        y = c0 * u + t1
        t1 = c1 * u - d1 * y + t2
        t2 = c2 * u - d2 * y
        out[i] = y
    return out


def segments(y, n: int, fs: int) -> np.ndarray:
    """seg[s] = sum of y^2 over [s h, min((s + 1) h, n)), in double, for the first n samples of a filtered row."""
    h = segment_samples(fs)
    y = np.asarray(y[:n], np.float64)
    return np.array([math.fsum(y[s * h: min((s + 1) * h, n)] ** 2) for s in range(segments_count(n, fs))], dtype=np.float64)


def blocks(seg, n: int, fs: int):
    """``(E, D)``: the block energies of a row of n samples with the segment table ``seg``, and the samples of a block."""
    h = segment_samples(fs)
    seg = np.asarray(seg, np.float64)
    if n >= 4 * h:
        NB = n // h - 3
        return np.array([((seg[j] + seg[j + 1]) + seg[j + 2]) + seg[j + 3] for j in range(NB)], dtype=np.float64), 4 * h
    E = 0.0
    for s in range(segments_count(n, fs)):
        E = E + float(seg[s])
    return np.array([E], dtype=np.float64), n


def gate(seg, n: int, fs: int, detail: bool = False):
    """``(L float32, NB, kept count)`` -- with ``detail`` also the kept set, E, D and mean_abs (None where no block passes)."""
    E, D = blocks(seg, n, fs)
    passed = [j for j in range(len(E)) if E[j] / D > Z_ABS]
    mean_abs = None
    kept = []
    if passed:
        acc = 0.0
        for j in passed:
            acc = acc + float(E[j])
        mean_abs = acc / len(passed)
        kept = [j for j in passed if 10.0 * E[j] > mean_abs]
    if kept:
        acc = 0.0
        for j in kept:
            acc = acc + float(E[j])
        L64 = -0.691 + 10.0 * math.log10(acc / len(kept) / D)
    else:
        L64 = -math.inf
    out = (np.float32(L64), len(E), len(kept))
    return out + (kept, E, D, mean_abs, L64) if detail else out


def loudness(x, n: int, fs: int, dtype=np.float64) -> float:
    """The integrated loudness of ``x[:n]`` (a double; -inf where no block is kept)."""
    return gate(segments(kfilter(np.asarray(x)[:n], fs, dtype), n, fs), n, fs, detail=True)[-1]


def gain(L, peak, target, ceiling, max_gain_db) -> float:
    """The gain of a row with loudness ``L`` and sample peak ``peak`` (a double)."""
    if math.isnan(target) or L == -math.inf:
        return 1.0
    g = 10.0 ** ((float(target) - float(L)) / 20.0)
    g = min(g, 10.0 ** (float(max_gain_db) / 20.0))
    if peak > 0:
        g = min(g, float(ceiling) / float(peak))
    return g


def gate_margins(seg, n: int, fs: int):
    """How far a row's blocks are from either gate, as factors >= 1: ``(absolute, relative)``, the smallest over EVERY block
    (inf where a gate does not apply: E = 0 against the absolute gate; no block passed, so there is no relative gate)."""
    _, _, _, _, E, D, mean_abs, _ = gate(seg, n, fs, detail=True)
    fa = min((max(e / D / Z_ABS, Z_ABS / (e / D)) if e > 0 else math.inf) for e in E)
    fr = math.inf
    if mean_abs is not None:
        fr = min((max(10.0 * e / mean_abs, mean_abs / (10.0 * e)) if e > 0 else math.inf) for e in E)
    return fa, fr


# ---------------------------------------------------------------------------------------------- the rows of the tests
MAIN_LENGTHS = (1, 4409, 4410, 17639, 17640, 22049, 22050, 3 * 44100 + 7, 8 * 44100)


def main_signal(fs: int, n: int) -> np.ndarray:
    """A 220 Hz tone alternating every 2 s between amplitude 0.1 and 30 dB below it, plus DC 0.05, plus 3 Hz of 0.02."""
    t = np.arange(n, dtype=np.float64) / fs
    amp = np.where((np.floor(t / 2.0).astype(np.int64) % 2) == 0, 0.1, 0.1 * 10.0 ** (-30.0 / 20.0))
    return (amp * np.sin(2 * np.pi * 220.0 * t) + 0.05 + 0.02 * np.sin(2 * np.pi * 3.0 * t)).astype(np.float32)


def tone(fs: int, n: int, f: float, a: float) -> np.ndarray:
    return (a * np.sin(2 * np.pi * f * np.arange(n, dtype=np.float64) / fs)).astype(np.float32)


def drop_row(fs: int) -> np.ndarray:
    """440 Hz at 0.5 for 3 s, then 70 dB lower for 1.5 s: the quiet blocks fail the absolute gate."""
    x = tone(fs, int(4.5 * fs), 440.0, 0.5).astype(np.float64)
    x[3 * fs:] *= 10.0 ** (-70.0 / 20.0)
    return x.astype(np.float32)


def audio_rows(fs: int):
    """The rows of one batch at ``fs``: ``[(name, samples float32)]``.  At 44.1 kHz the issue's list; at the other rates
    prefixes of the main signal around the segment (h) and block (4 h) boundaries, and a tone (above 48 kHz shorter rows:
    the restatement filters a sample at a time)."""
    if fs == 44100:
        x = main_signal(fs, max(MAIN_LENGTHS))
        rows = [(f"main[:{n}]", x[:n]) for n in MAIN_LENGTHS]
        rows += [("zeros", np.zeros(30000, np.float32)), ("tone 1e-4", tone(fs, 2 * fs, 1000.0, 1e-4)), ("drop", drop_row(fs))]
        return rows
    h = segment_samples(fs)
    lengths = (h - 1, h, 4 * h - 1, 4 * h, 5 * h + 3, int(2.5 * fs) + 1 if fs <= 48000 else 9 * h + 5)
    x = main_signal(fs, max(lengths))
    return [(f"main[:{n}]", x[:n]) for n in lengths] + [("tone", tone(fs, min(fs, 44100) + 17, 997.0, 0.25))]


_CACHE = {}


def measured_rows(fs: int):
    """Per row of ``audio_rows(fs)``: dict(name, x, n, seg, L, L64, NB, kept, peak, gate_lu) -- the fp64 restatement's
    values, and the row's gate in LU: 4 times the distance of the float32 run of the same recurrence from the fp64 run,
    at least 1e-5, never above 0.1.  Computed once per process (prefixes of one signal share its filtered output)."""
    if fs in _CACHE:
        return _CACHE[fs]
    out, filt = [], {}
    for name, x in audio_rows(fs):
        key = name.split("[")[0]
        if key not in filt or len(filt[key][0]) < len(x):
            filt[key] = (kfilter(x, fs, np.float64), kfilter(x, fs, np.float32))
        y64, y32 = filt[key]
        n = len(x)
        seg = segments(y64, n, fs)
        L, NB, _, kept, _, _, _, L64 = gate(seg, n, fs, detail=True)
        L32 = gate(segments(y32, n, fs), n, fs, detail=True)[-1]
        err = 0.0 if L64 == L32 else abs(L64 - L32)
        out.append(dict(name=name, x=x, n=n, seg=seg, L=L, L64=L64, NB=NB, kept=kept, peak=np.float32(np.max(np.abs(x))),
                        yardstick=err, gate_lu=min(max(4.0 * err, 1e-5), 0.1)))
    _CACHE[fs] = out
    return out


def pack(rows, fill=np.nan):
    """``(audio [B][L_max] float32 with ``fill`` behind every row, n [B])``; one extra column so that every row has a tail."""
    n = [len(r) for r in rows]
    a = np.full((len(rows), max(n) + 1), fill, dtype=np.float32)
    for b, r in enumerate(rows):
        a[b, : n[b]] = r
    return a, n


# ---------------------------------------------------------------------------------------------- constructed segment tables
TABLE_FS = 8000                        # h = 800: a row of S segments is taken as n = S h samples (D = 4 h)
TABLE_SEGMENTS = (1, 3, 4, 5, 64, 65, 130)


def at_abs_gate(D: float) -> float:
    """The largest double E with E / D <= Z_abs: a block AT the absolute gate, which does not pass it."""
    e = Z_ABS * D
    while e / D > Z_ABS:
        e = float(np.nextafter(e, -np.inf))
    while float(np.nextafter(e, np.inf)) / D <= Z_ABS:
        e = float(np.nextafter(e, np.inf))
    return e


def gate_tables():
    """Ragged double tables for the gate operator alone: ``[(seg [S], n)]`` with exact ties at both gates.  Every value is a
    small multiple of a power of two, so every sum is exact whatever its order and the ties are ties in any arithmetic."""
    h = segment_samples(TABLE_FS)
    rng = np.random.default_rng(21)
    rows = []
    for S in TABLE_SEGMENTS:
        seg = rng.integers(1, 40, size=S).astype(np.float64) * 0.25
        if S >= 5:
            # blocks 0 and 1 are {1, 19} scaled: mean_abs of a two-block row would be 10; the tie is planted below
            seg[:5] = [0.25, 0.25, 0.25, 0.25, 18.25]
        rows.append((seg, S * h))
    # the hand-worked tie: two blocks E = {1, 19}, D = 4 h: mean_abs = 10, 10 * 1 == 10 is NOT kept
    rows.append((np.array([0.25, 0.25, 0.25, 0.25, 18.25]), 5 * h))
    # a block exactly AT the absolute gate (E / D == Z_abs is not > Z_abs) beside one that passes
    rows.append((np.array([at_abs_gate(4.0 * h), 0.0, 0.0, 0.0, 4.0 * at_abs_gate(4.0 * h)]), 5 * h))
    # a short row (n < 4 h): one block of all its segments over D = n
    rows.append((np.array([3.0, 5.0, 0.5]), 2 * h + 11))
    # nothing passes
    rows.append((np.zeros(6), 6 * h))
    return rows
