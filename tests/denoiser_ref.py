"""The denoiser and the inverse STFT restated: this project's own specification in fp64 numpy, with a
float32 mode in which every product, sum and quotient is rounded to float32 (the matrix products by numpy's float32
``matmul``; the overlap-add chain and the window sum exactly as specified: from 0 in ascending t).  Self-contained.

Geometry (the model's own): N = n_fft, hop, the periodic Hann window, pad = (N - hop) / 2 with reflection at the row's own
two ends, T(n) = 1 + (n + 2 pad - N) // hop frames.
  analysis     X[r][t] = sum_n hann[n] xp[t hop + n] e^{-2 pi i r n / N}, r = 0 .. N / 2
  subtraction  m = sqrt(re^2 + im^2); q = max(m - s beta[r], 0) / m (0 where m = 0); X' = q X
  synthesis    v_t[n] = hann[n] (1 / N) sum_r w_r Re(X'[r][t] e^{+2 pi i r n / N}), w_0 = w_{N/2} = 1, else 2
               yp[p] = (sum_t v_t[p - t hop]) / W[p], W[p] = sum_t hann^2[p - t hop] over the row's own frames covering p
               out[i] = yp[pad + i], 0 <= i < n
Every angle is reduced exactly, (r n) mod N, before the cosine is taken.  In float32 mode the window sum adds
fl32(hann^2), the table the library keeps."""
from functools import lru_cache

import numpy as np

N_FFT, HOP = 2048, 512
W_FLOOR = 0.02


def pad_of(N: int = N_FFT, hop: int = HOP) -> int:
    return (N - hop) // 2


def frames(n: int, N: int = N_FFT, hop: int = HOP) -> int:
    pad = pad_of(N, hop)
    if n <= pad or n + 2 * pad < N:
        return 0
    return 1 + (n + 2 * pad - N) // hop


@lru_cache(maxsize=None)
def hann(N: int = N_FFT) -> np.ndarray:
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)


@lru_cache(maxsize=None)
def _trig(N: int):
    """cos, sin of 2 pi (r n mod N) / N as [N/2 + 1][N] in double."""
    k = (np.arange(N // 2 + 1, dtype=np.int64)[:, None] * np.arange(N, dtype=np.int64)[None, :]) % N
    a = 2.0 * np.pi * k / N
    return np.cos(a), np.sin(a)


@lru_cache(maxsize=None)
def analysis_basis(N: int = N_FFT) -> np.ndarray:
    """[2 spec][N] in double: rows cos * hann, then -sin * hann (the spectrogram front end's operand)."""
    c, s = _trig(N)
    return np.concatenate([c * hann(N)[None, :], -s * hann(N)[None, :]])


@lru_cache(maxsize=None)
def synthesis_basis(N: int = N_FFT) -> np.ndarray:
    """[N][2 spec] in double: hann[n] (w_r / N) cos, then -hann[n] (w_r / N) sin."""
    c, s = _trig(N)
    w = np.full(N // 2 + 1, 2.0 / N)
    w[0] = w[-1] = 1.0 / N
    return np.concatenate([(c * w[:, None]).T, (-s * w[:, None]).T], axis=1) * hann(N)[:, None]


def reflect_pad(x: np.ndarray, pad: int) -> np.ndarray:
    assert len(x) > pad
    return np.concatenate([x[1:pad + 1][::-1], x, x[-pad - 1:-1][::-1]]) if pad else x


def analysis(x, N: int = N_FFT, hop: int = HOP, dtype=np.float64) -> np.ndarray:
    """RI [2 spec][T]: real rows, then imaginary rows."""
    x = np.asarray(x, np.float32)
    T = frames(len(x), N, hop)
    assert T > 0
    xp = reflect_pad(x, pad_of(N, hop)).astype(dtype)
    F = np.stack([xp[t * hop:t * hop + N] for t in range(T)], axis=1)          # [N][T]
    return analysis_basis(N).astype(dtype) @ F


def subtract(ri, beta, s, dtype=np.float64) -> np.ndarray:
    spec = ri.shape[0] // 2
    re, im = ri[:spec].astype(dtype), ri[spec:].astype(dtype)
    m = np.sqrt(re * re + im * im)
    thr = dtype(np.float32(s)) * np.asarray(beta).astype(dtype)[:, None]       # (the library's bias is float32; any here)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(m > 0, np.maximum(m - thr, dtype(0)) / np.where(m > 0, m, dtype(1)), dtype(0)).astype(dtype)
    return np.concatenate([q * re, q * im])


def window_sum(n: int, N: int = N_FFT, hop: int = HOP, dtype=np.float64) -> np.ndarray:
    """W over the row's true samples, summed in ascending t."""
    T, pad = frames(n, N, hop), pad_of(N, hop)
    w2 = hann(N) ** 2
    w2 = w2.astype(np.float32).astype(dtype) if dtype == np.float32 else w2
    W = np.zeros((T - 1) * hop + N, dtype)
    for t in range(T):
        W[t * hop:t * hop + N] += w2
    return W[pad:pad + n]


def synthesis(ri, n: int, N: int = N_FFT, hop: int = HOP, dtype=np.float64) -> np.ndarray:
    """out[0 .. n) from RI [2 spec][>= T(n)]; columns at or behind T(n) are not used."""
    T, pad = frames(n, N, hop), pad_of(N, hop)
    assert T > 0 and ri.shape[1] >= T
    v = synthesis_basis(N).astype(dtype) @ np.asarray(ri)[:, :T].astype(dtype)    # [N][T]
    y = np.zeros((T - 1) * hop + N, dtype)
    for t in range(T):                                                         # ascending t, a chain from 0
        y[t * hop:t * hop + N] += v[:, t]
    W = window_sum(n, N, hop, dtype)
    assert W.min() >= W_FLOOR, (n, W.min())
    return (y[pad:pad + n] / W).astype(dtype)


def denoise(x, beta, s, N: int = N_FFT, hop: int = HOP, dtype=np.float64) -> np.ndarray:
    ri = analysis(x, N, hop, dtype)
    return synthesis(subtract(ri, beta, s, dtype), len(x), N, hop, dtype)


def bias_of(period, N: int = N_FFT, hop: int = HOP, dtype=np.float64) -> np.ndarray:
    """beta[r] = |sum_n hann[n] c[n mod hop] e^{-2 pi i r n / N}|."""
    c = np.asarray(period, np.float32)
    assert len(c) == hop and N % hop == 0
    ri = analysis_basis(N).astype(dtype) @ np.tile(c, N // hop).astype(dtype)
    spec = N // 2 + 1
    return np.sqrt(ri[:spec] ** 2 + ri[spec:] ** 2)


# ------------------------------------------------------------------------------------------------------------ the rows
# the lengths at which the kernels change path (framing and overlap-add tiles of 16 frames); ROW_ALONE is left alone
LENGTHS = (769, 1023, 1024, 16 * HOP - 1, 5000, 16 * HOP, 17 * HOP + 300, 40 * HOP + 77)
ROW_ALONE = 4


def voiced(n: int, seed: int, fs: int = 44100) -> np.ndarray:
    """Harmonics of 140 Hz under a slow envelope (limiter_ref.voiced's kind, without the burst), a tiled random period of
    one hop -- the kind of component the denoiser removes -- and a little noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    x = sum(a * np.sin(2 * np.pi * 140.0 * k * t + k) for k, a in ((1, 0.25), (2, 0.12), (3, 0.08), (5, 0.04)))
    x = x * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t))
    c = 0.01 * rng.standard_normal(HOP)
    x = x + np.tile(c, n // HOP + 1)[:n] + 0.005 * rng.standard_normal(n)
    return x.astype(np.float32)


def fixture_rows():
    """[(x, beta)]: one row per entry of LENGTHS, fixed seeds; beta a random non-negative spectrum."""
    out = []
    for i, n in enumerate(LENGTHS):
        rng = np.random.default_rng(1000 + i)
        beta = np.abs(rng.standard_normal(N_FFT // 2 + 1)).astype(np.float32) * np.float32(2.0)
        out.append((voiced(n, 50 + i), beta))
    return out


def pack(rows, fill=np.nan):
    """Rows of different lengths as [B, L] float32 with ``fill`` behind every row's end, and their lengths."""
    L = max(len(r) for r in rows) + 5
    out = np.full((len(rows), L), fill, np.float32)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out, [len(r) for r in rows]


U32 = 2.0 ** -24


def floor_of(x, n: int) -> float:
    """The gate's floor for a row (the derivation: tests/test_denoiser_gpu.py): sqrt(2048) roundings of 2^-24 of the row's
    peak, divided by the row's smallest window sum."""
    return float(np.sqrt(2048.0) * U32 * np.abs(np.asarray(x, np.float64)).max() / window_sum(n).min())
