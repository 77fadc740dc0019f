"""The prosody specification restated in fp64 numpy: per-frame energy and F0 of one recording and
their per-phoneme means.  Nothing here is shared with the library: the energy goes through ``numpy.fft.rfft`` (the library
uses the Parseval form, so the identity is tested and not assumed), the autocorrelation through an FFT.  The one number
format the specification itself fixes is kept: the window's autocorrelation enters as float32 reciprocals."""
from __future__ import annotations

import numpy as np

FS, HOP, N_FFT = 44100, 512, 1280
DEFAULTS = dict(floor=80.0, ceiling=750.0, voicing_threshold=0.6, silence_threshold=0.03, octave_cost=0.01)


def frames(n: int, hop: int = HOP) -> int:
    return n // hop + 1


def window_samples(floor: float) -> int:
    W = int(np.floor(3.0 * FS / floor + 0.5))
    return W + (W & 1)


def energy_frames(x, hop: int = HOP, parseval: bool = False) -> np.ndarray:
    """e_k = sqrt(sum over the one-sided bins of |rfft(frame_k * hann)|^2); ``parseval``: the DFT-free form."""
    x = np.asarray(x, np.float64)
    assert x.ndim == 1 and len(x) >= N_FFT // 2 + 1
    xp = np.pad(x, N_FFT // 2, mode="reflect")
    hann = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT)
    F = frames(len(x), hop)
    S = np.stack([xp[hop * k: hop * k + N_FFT] for k in range(F)]) * hann
    if parseval:
        alt = np.where(np.arange(N_FFT) % 2 == 0, 1.0, -1.0)
        return np.sqrt((N_FFT * (S * S).sum(1) + S.sum(1) ** 2 + (S * alt).sum(1) ** 2) / 2.0)
    X = np.fft.rfft(S, axis=1)
    return np.sqrt((np.abs(X) ** 2).sum(1))


def _autocorr(a: np.ndarray, n_lags: int) -> np.ndarray:
    """r[..., t] = sum_n a[..., n] a[..., n + t], t < n_lags, for the rows of ``a``."""
    W = a.shape[-1]
    size = 1 << int(np.ceil(np.log2(2 * W)))
    A = np.fft.rfft(a, size, axis=-1)
    return np.fft.irfft(A * np.conj(A), size, axis=-1)[..., :n_lags]


def f0_frames(x, hop: int = HOP, floor=80.0, ceiling=750.0, voicing_threshold=0.6, silence_threshold=0.03,
              octave_cost=0.01, with_margin: bool = False):
    """F0 per frame (0: unvoiced).  ``with_margin``: also the decision margin of every frame -- the winning strength minus
    the next competitor's, the unvoiced strength U included (inf where nothing competes: no candidate, or r_a(0) = 0)."""
    x = np.asarray(x, np.float64)
    n = len(x)
    F = frames(n, hop)
    W = window_samples(floor)
    tmin, tmax = int(np.floor(FS / ceiling)), int(np.ceil(FS / floor))
    gpk = np.abs(x - x.mean()).max()
    xz = np.concatenate([np.zeros(W // 2), x, np.zeros(W // 2 + hop)])
    s = np.stack([xz[hop * k: hop * k + W] for k in range(F)])          # x[hop k - W/2 : hop k + W/2], zeros outside
    s = s - s.mean(1, keepdims=True)
    lpk = np.abs(s).max(1)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(W) + 0.5) / W)
    ra = _autocorr(s * w, tmax + 2)
    rw = np.array([np.dot(w[: W - t], w[t:]) for t in range(tmax + 2)])
    inv_rw = (rw[0] / rw).astype(np.float32).astype(np.float64)         # the specification's float32 table
    f0 = np.zeros(F)
    margin = np.full(F, np.inf)
    if not gpk > 0:
        return (f0, margin) if with_margin else f0
    t = np.arange(tmin, tmax + 1)
    for k in range(F):
        if not ra[k, 0] > 0:
            continue
        r = ra[k] / ra[k, 0] * inv_rw
        rm, r0, rp = r[t - 1], r[t], r[t + 1]
        c = (r0 > rm) & (r0 >= rp)
        U = voicing_threshold + max(0.0, 2.0 - (lpk[k] / gpk) / (silence_threshold / (1.0 + voicing_threshold)))
        if not c.any():
            continue
        rm, r0, rp, tc = rm[c], r0[c], rp[c], t[c]
        d = 0.5 * (rm - rp) / (rm - 2.0 * r0 + rp)
        R = r0 - 0.25 * (rm - rp) * d
        f = FS / (tc + d)
        S = R + octave_cost * np.log2(f / floor)
        i = int(np.argmax(S))                                           # (the lowest lag among equals)
        others = np.append(np.delete(S, i), U)
        if S[i] > U:
            f0[k] = f[i]
            margin[k] = S[i] - others.max()
        else:
            margin[k] = U - S[i]
    return (f0, margin) if with_margin else f0


def interpolate(f0) -> np.ndarray:
    """Linear interpolation across unvoiced frames; the ends take the first / last voiced value; fewer than two voiced
    frames: unchanged."""
    f0 = np.asarray(f0, np.float64).copy()
    v = np.nonzero(f0)[0]
    if len(v) < 2:
        return f0
    out = f0.copy()
    for i in range(len(f0)):
        if f0[i] != 0:
            continue
        if i < v[0]:
            out[i] = f0[v[0]]
        elif i > v[-1]:
            out[i] = f0[v[-1]]
        else:
            q = int(np.searchsorted(v, i))
            p, q = v[q - 1], v[q]
            out[i] = f0[p] + (f0[q] - f0[p]) * ((i - p) / (q - p))
    return out


def phoneme_means(contour, durations) -> np.ndarray:
    """Phoneme i gets the mean of its own frames [sum_{j<i} d_j, + d_i) of the untouched contour, 0 where d_i = 0."""
    c = np.asarray(contour, np.float64)
    d = np.asarray(durations, np.int64)
    assert d.sum() <= len(c)
    start = np.concatenate([[0], np.cumsum(d)[:-1]])
    return np.array([c[s: s + n].mean() if n > 0 else 0.0 for s, n in zip(start, d)])


def prosody(x, durations, hop: int = HOP, **params):
    """(f0 [Tp], energy [Tp]) of one recording."""
    return (phoneme_means(interpolate(f0_frames(x, hop, **params)), durations),
            phoneme_means(energy_frames(x, hop), durations))


# ---------------------------------------------------------------------------------------------- test signals
def harmonic(f, n, partials: int = 8, decay: float = 0.6, amp: float = 0.25) -> np.ndarray:
    """A complex of ``partials`` harmonics of ``f`` Hz (f a scalar or an array of n instantaneous frequencies)."""
    ph = 2.0 * np.pi * np.cumsum(np.broadcast_to(np.asarray(f, np.float64), (n,))) / FS
    return amp * sum(decay ** h * np.sin(h * ph) for h in range(1, partials + 1))
