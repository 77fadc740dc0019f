"""The denoiser on an FFT, restated.  The specification does not change: an FFT computes the sums of
tests/denoiser_ref.py, so the fp64 side of every comparison is ``denoiser_ref.denoise / synthesis / bias_of``.  This file
adds the float32 mode of the FFT path, whose distance from fp64 sets the gate:

  frames times fl32(hann); a radix-2 transform in float32 -- real and imaginary parts apart, every product and sum rounded
  on its own, the twiddles a table rounded once from fp64 --; ``denoiser_ref.subtract(dtype=float32)``; the Hermitian
  extension (the imaginary parts of bins 0 and N / 2 dropped, as the specification's real part drops them), the inverse
  transform, 1 / N (exact) and fl32(hann); the project's overlap-add chain from 0 in ascending t and
  ``denoiser_ref.window_sum(dtype=float32)``.

The gate of a row is max(4 x |float32 FFT restatement - fp64|, floor), floor = sqrt(4 log2 N + 8) 2^-24 P / min W: an output
sample passes through an add and a multiply per pass each way (4 log2 N = 44), the two windows, the chain of four and the
quotient (8) -- 52 roundings of at most 2^-24 of the row's peak P that add as a random walk, divided by the row's smallest
window sum W.  Self-contained: numpy only, no ``np.fft``."""
from functools import lru_cache

import numpy as np

import denoiser_ref as dr

N_FFT, HOP, U32 = dr.N_FFT, dr.HOP, dr.U32
F32 = np.float32


@lru_cache(maxsize=None)
def _plan(N: int):
    """(bit reversal of 0 .. N - 1, fl32 cos and fl32 sin of 2 pi k / N for k < N / 2)."""
    bits = N.bit_length() - 1
    assert 1 << bits == N
    rev = np.zeros(N, np.int64)
    for b in range(bits):
        rev |= ((np.arange(N) >> b) & 1) << (bits - 1 - b)
    a = 2.0 * np.pi * np.arange(N // 2) / N
    return rev, np.cos(a).astype(F32), np.sin(a).astype(F32)


def fft32(re, im, sign: int):
    """sum_n (re + i im)[n] e^{sign 2 pi i k n / N} over axis 0 of [N][T] float32 arrays, in float32, not normalised."""
    N, T = re.shape
    rev, c, s = _plan(N)
    re, im = re[rev].astype(F32), im[rev].astype(F32)
    L = 2
    while L <= N:
        h, step = L // 2, N // L
        wr = c[::step][:h][None, :, None]
        wi = (F32(sign) * s[::step][:h])[None, :, None]
        R, I = re.reshape(N // L, L, T), im.reshape(N // L, L, T)
        ar, ai, br, bi = R[:, :h].copy(), I[:, :h].copy(), R[:, h:].copy(), I[:, h:].copy()
        tr, ti = br * wr - bi * wi, br * wi + bi * wr
        R[:, :h], I[:, :h], R[:, h:], I[:, h:] = ar + tr, ai + ti, ar - tr, ai - ti
        L *= 2
    assert re.dtype == F32 and im.dtype == F32
    return re, im


def analysis(x, N: int = N_FFT, hop: int = HOP) -> np.ndarray:
    """RI [2 spec][T] float32 of the FFT path: real rows, then imaginary rows."""
    x = np.asarray(x, F32)
    T = dr.frames(len(x), N, hop)
    assert T > 0
    xp = dr.reflect_pad(x, dr.pad_of(N, hop))
    F = np.stack([xp[t * hop:t * hop + N] for t in range(T)], axis=1) * dr.hann(N).astype(F32)[:, None]
    re, im = fft32(F, np.zeros_like(F), -1)
    spec = N // 2 + 1
    return np.concatenate([re[:spec], im[:spec]])


def synthesis(ri, n: int, N: int = N_FFT, hop: int = HOP) -> np.ndarray:
    """out[0 .. n) float32 from RI [2 spec][>= T(n)] on the FFT path."""
    T, pad, spec = dr.frames(n, N, hop), dr.pad_of(N, hop), N // 2 + 1
    assert T > 0 and ri.shape[1] >= T
    ri = np.asarray(ri)[:, :T].astype(F32)
    re, im = ri[:spec], ri[spec:].copy()
    im[0] = 0
    im[-1] = 0
    re = np.concatenate([re, re[-2:0:-1]])
    im = np.concatenate([im, -im[-2:0:-1]])
    v, _ = fft32(re, im, +1)
    v = (v * F32(1.0 / N)) * dr.hann(N).astype(F32)[:, None]
    y = np.zeros((T - 1) * hop + N, F32)
    for t in range(T):                                                         # ascending t, a chain from 0
        y[t * hop:t * hop + N] += v[:, t]
    W = dr.window_sum(n, N, hop, F32)
    out = y[pad:pad + n] / W
    assert out.dtype == F32
    return out


def denoise(x, beta, s, N: int = N_FFT, hop: int = HOP) -> np.ndarray:
    return synthesis(dr.subtract(analysis(x, N, hop), beta, s, F32), len(x), N, hop)


def bias_of(period, N: int = N_FFT, hop: int = HOP) -> np.ndarray:
    c = np.asarray(period, F32)
    assert len(c) == hop and N % hop == 0
    F = (np.tile(c, N // hop) * dr.hann(N).astype(F32))[:, None]
    re, im = fft32(F, np.zeros_like(F), -1)
    spec = N // 2 + 1
    return np.sqrt(re[:spec, 0] * re[:spec, 0] + im[:spec, 0] * im[:spec, 0])


ROUNDINGS = 4 * 11 + 8          # 4 log2 N + 8 for N = 2048


def floor_of(x, n: int) -> float:
    """sqrt(4 log2 N + 8) 2^-24 P / min W."""
    return float(np.sqrt(ROUNDINGS) * U32 * np.abs(np.asarray(x, np.float64)).max() / dr.window_sum(n).min())


def gate_of(f32, f64, floor: float) -> float:
    return max(4.0 * float(np.abs(np.asarray(f32, np.float64) - f64).max()), floor)


@lru_cache(maxsize=None)
def restated(strengths=(0.0, 0.01, 1.0, 50.0)):
    """{strength: [(fp64 output, float32 FFT output, gate) per fixture row]}, computed once per process."""
    out = {}
    for s in strengths:
        per = []
        for x, beta in dr.fixture_rows():
            d, f = dr.denoise(x, beta, s), denoise(x, beta, s)
            per.append((d, f, gate_of(f, d, floor_of(x, len(x)))))
        out[s] = per
    return out
