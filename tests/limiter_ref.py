"""The true-peak meter and the look-ahead limiter restated in numpy, and the rows the tests use.
Nothing here is shared with the library.  Every function takes ``dtype``: float64 is the restatement, float32 is the same
operation order in the library's number format -- its distance from the float64 run is the yardstick of the GPU tests.
(numpy has no fused multiply-add: the float32 chain rounds ``float64(h) * float64(x) + float64(acc)`` to float32, which is
the fused result except where the double's own rounding falls on a float32 tie.)

A row is ``x[0 .. N)``, zero outside.  The taps are rounded to float32 once and the reciprocal ``1 / (A + 1)`` is one
float32 constant, in both runs: they are part of the specification, not of the arithmetic under test."""
from __future__ import annotations

import numpy as np

FS = 44100
ZEROS, BETA, OVERSAMPLE = 12, 9.62, 4
HALF = ZEROS * OVERSAMPLE            # 48: taps h[-48 .. 48]
REACH = ZEROS                        # J: input samples a side
MAX_ATTACK, MAX_HOLD = 1024, 8192


def taps64() -> np.ndarray:
    """h[n], n = -48 .. 48, in double: the resampling core's formula at L = 4, M = 1."""
    rolloff = 1.0 - 3.065 / ZEROS
    fc = rolloff / OVERSAMPLE
    n = np.arange(-HALF, HALF + 1, dtype=np.float64)
    w = np.i0(BETA * np.sqrt(np.maximum(0.0, 1.0 - (n / HALF) ** 2))) / np.i0(BETA)
    return OVERSAMPLE * fc * np.sinc(fc * n) * w


def taps() -> np.ndarray:
    return taps64().astype(np.float32)


def history(A: int, H: int):
    return A + H + REACH, A + REACH


def peaks(x, dtype=np.float64) -> np.ndarray:
    """p[n] = max(|x[n]|, |y[4n]| .. |y[4n+3]|), y[m] = sum_k h[m - 4k] x[k] as a chain from 0 in ascending k."""
    x = np.asarray(x, np.float32)
    N = len(x)
    h = taps().astype(np.float64)
    xp = np.concatenate([np.zeros(REACH, np.float32), x, np.zeros(REACH, np.float32)]).astype(np.float64)
    p = np.abs(x).astype(dtype)
    for ph in range(OVERSAMPLE):
        acc = np.zeros(N, dtype)
        for d in range(-REACH, REACH + 1):                    # k = n + d ascending; tap h[4 (n - k) + ph]
            t = -4 * d + ph
            if abs(t) > HALF:
                continue
            acc = (h[t + HALF] * xp[REACH + d:REACH + d + N] + acc.astype(np.float64)).astype(dtype)
        p = np.maximum(p, np.abs(acc))
    return p


def true_peak(x, dtype=np.float64):
    return peaks(x, dtype).max() if len(x) else dtype(0)


def sliding_min(r, A: int, H: int, before: int = 0) -> np.ndarray:
    """m[n] = min r[n - H .. n + A] for n = -before .. N - 1, r = 1 outside the row (min is exact: any order of evaluation
    gives the same values, so this one doubles the span)."""
    N, W = len(r), A + H + 1
    a = np.concatenate([np.ones(before + H, r.dtype), r, np.ones(A, r.dtype)])
    span = 1
    while 2 * span <= W:
        a[:len(a) - span] = np.minimum(a[:len(a) - span], a[span:])
        span *= 2
    return np.minimum(a[:N + before], a[W - span:W - span + N + before])


def limit(x, g, c, A: int, H: int, dtype=np.float64) -> dict:
    """The limiter of a whole row: p, r, m, s, out and the row's true peak ``tp`` (of the INPUT) and ``min_gain``."""
    assert 0 <= A <= MAX_ATTACK and 0 <= H <= MAX_HOLD
    x = np.asarray(x, np.float32)
    N = len(x)
    g, c = dtype(np.float32(g)), dtype(np.float32(c))
    p = peaks(x, dtype)
    e = g * p
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(e > c, c / np.where(e > c, e, 1), dtype(1)).astype(dtype)
    mp = sliding_min(r, A, H, before=A)                       # m[-A .. N): the windows of the samples before the row reach it
    m = mp[A:]
    acc = np.zeros(N, dtype)
    for k in range(A + 1):                                    # m[n - A] first
        acc = (acc + mp[k:k + N]).astype(dtype)
    inv = dtype(np.float32(1.0) / np.float32(A + 1))
    s = (acc * inv).astype(dtype)
    out = np.clip(((g * x.astype(dtype)).astype(dtype) * s).astype(dtype), -c, c)
    return dict(p=p, r=r, m=m, s=s, out=out, tp=p.max() if N else dtype(0), min_gain=s.min() if N else dtype(1))


def db(v) -> float:
    return 20.0 * float(np.log10(max(float(v), 1e-300)))


# ------------------------------------------------------------------------------------------------------------ the rows
def fs4_sine(n: int, a: float = 1.0) -> np.ndarray:
    """A sine at fs / 4 with 45 degrees of phase (EBU Tech 3341's kind of signal): every sample is a / sqrt(2) in size."""
    return (a * np.sin(np.pi / 2 * np.arange(n) + np.pi / 4)).astype(np.float32)


def voiced(n: int, seed: int, burst: bool = True) -> np.ndarray:
    """A noisy voiced signal: harmonics of 140 Hz under a slow envelope, noise, a 9 kHz burst and a click."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / FS
    x = sum(a * np.sin(2 * np.pi * 140.0 * k * t + k) for k, a in ((1, 0.25), (2, 0.12), (3, 0.08), (5, 0.04)))
    x = x * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t)) + 0.02 * rng.standard_normal(n)
    if burst:
        b0, b1 = n // 3, n // 3 + min(400, n // 8)
        x[b0:b1] += 0.6 * np.sin(2 * np.pi * 9000.0 * t[b0:b1]) * np.hanning(b1 - b0)
        x[(2 * n) // 3] += 0.9
    return x.astype(np.float32)


def fixture_rows():
    """[(name, x, g, ceiling)]: the rows of the issue's list, 44.1 kHz, fixed seeds."""
    n = 4410
    click0 = np.zeros(700, np.float32); click0[0] = 1.0
    clickN = np.zeros(900, np.float32); clickN[-1] = -1.0
    near = (0.01 * np.random.default_rng(7).standard_normal(1500)).astype(np.float32)
    near[600] += 0.95; near[630] -= 0.8                       # two peaks closer than the default attack of 66
    t = np.arange(n) / FS
    return [
        ("silence", np.zeros(1000, np.float32), 1.0, 0.9),
        ("click_first", click0, 1.5, 0.9),
        ("click_last", clickN, 1.5, 0.9),
        ("fs4_45deg", fs4_sine(2000), 1.0, 0.9),
        ("sine_997", (0.8 * np.sin(2 * np.pi * 997.0 * t)).astype(np.float32), 2.0, 0.9),
        ("voiced_burst", voiced(n, 11), 3.0, 0.9),
        ("two_peaks", near, 2.0, 0.9),
        ("loud", voiced(n, 13), 8.0, 0.9),
        ("never_limited", voiced(n, 17, burst=False), 1.25, 0.9),
    ]


def pack(rows, fill=np.nan):
    """Rows of different lengths as [B, L] float32 with ``fill`` behind every row's end, and their lengths."""
    L = max(len(r) for r in rows)
    L = (L + 3) // 4 * 4 + 4
    out = np.full((len(rows), L), fill, np.float32)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out, [len(r) for r in rows]
