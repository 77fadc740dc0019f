"""Double-precision restatement of the output stage (include/vispeech_hip.h, "output stage"), kept beside the tests
that use it.  Nothing here calls the library: the plan and the filter are evaluated from the published formula with
numpy, the resampling sum is written out term by term."""
from math import gcd

import numpy as np

RATES = (22050, 16000, 24000, 48000, 8000, 11025, 32000)          # from 44100
TABLE = {22050: (1, 2, 129), 16000: (160, 441, 28225), 24000: (80, 147, 9409), 48000: (160, 147, 10241),
         8000: (80, 441, 28225), 11025: (1, 4, 257), 32000: (320, 441, 28225)}      # out_rate: (L, M, taps)


def plan(in_rate, out_rate, zeros=32):
    g = gcd(in_rate, out_rate)
    L, M = out_rate // g, in_rate // g
    return L, M, zeros * max(L, M)


def filter_fp64(in_rate, out_rate, zeros=32, beta=9.62, rolloff=None):
    """h[n], n = -H .. H:  L fc sinc(fc n) kaiser(2 H + 1, beta)[n + H],  fc = rolloff / max(L, M)."""
    L, M, H = plan(in_rate, out_rate, zeros)
    rolloff = 1.0 - 3.065 / zeros if rolloff is None else rolloff
    fc = rolloff / max(L, M)
    n = np.arange(-H, H + 1, dtype=np.float64)
    return L * fc * np.sinc(fc * n) * np.kaiser(2 * H + 1, beta)


def out_len(n, L, M):
    return -((-n * L) // M)


def resample_fp64(x, h, L, M, m0=0, m1=None, with_bound=False):
    """y[m] = sum_k h[m M - k L] x[k], k in [0, len(x)) with |m M - k L| <= H, for m in [m0, m1) -- in float64, whatever
    the precision of ``h`` and ``x``.  ``with_bound``: also N[m], the number of terms, and A[m] = sum_k |h| |x|."""
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    H = (len(h) - 1) // 2
    n = len(x)
    m1 = out_len(n, L, M) if m1 is None else m1
    m = np.arange(m0, m1, dtype=np.int64)
    y = np.zeros(len(m))
    cnt = np.zeros(len(m), dtype=np.int64)
    mag = np.zeros(len(m))
    if len(m) == 0:
        return (y, cnt, mag) if with_bound else y
    k_lo = -((H - m * M) // L)                     # ceil((m M - H) / L)
    k_hi = (m * M + H) // L
    for j in range(int((k_hi - k_lo).max()) + 1):
        k = k_lo + j
        ok = (k <= k_hi) & (k >= 0) & (k < n)
        t = m * M - k * L
        hv = h[np.clip(t + H, 0, 2 * H)]
        xv = x[np.clip(k, 0, max(n - 1, 0))] if n else np.zeros(len(m))
        term = np.where(ok, hv * xv, 0.0)
        y += term
        cnt += ok
        mag += np.abs(term)
    return (y, cnt, mag) if with_bound else y


def pcm16(a):
    """The host rule of vispeech_amd.service.pcm16, restated."""
    return np.clip(np.rint(np.asarray(a, dtype=np.float32) * np.float32(32767.0)), -32768, 32767).astype("<i2")
