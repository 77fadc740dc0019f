"""One call of the denoiser for streams restated: the window of frames a call's outputs need and
those outputs only, in fp64 numpy or -- ``dtype=np.float32`` -- with every product, sum and quotient rounded to float32.
The arithmetic is that of tests/denoiser_ref.py; what is new is the bookkeeping: which frames, read from where, reflected
at which ends, summed into which outputs.

Every frame goes through the two DFT products ALONE, as a matrix-vector product of one fixed shape, so a frame's numbers do
not depend on the window it is computed in (numpy's matrix-matrix product makes no such promise); each output's sum is one
chain from 0 in ascending t, and so is its window sum.  A stream cut anywhere therefore gives the whole row's BITS here, as
the library promises for itself.  Frames are cached by their content -- the cuts of the tests compute the same frames many
times over.

``RefEngine`` is the numpy stand-in for ``vispeech_amd.engine.Engine`` that ``vispeech_amd.denoiser`` drives in the host
tests: it refuses a row whose buffer lacks a sample one of its frames reads."""
from functools import lru_cache

import numpy as np

import denoiser_ref as dr

N_FFT, HOP = dr.N_FFT, dr.HOP


def complete(n: int, N: int = N_FFT, hop: int = HOP) -> int:
    """E(n): the outputs that are final with n samples of an open stream."""
    pad = dr.pad_of(N, hop)
    room = n + pad - N
    Tc = 0 if room < 0 else room // hop + 1
    return max(0, Tc * hop - pad)


def window(out_first: int, out_count: int, total, N: int = N_FFT, hop: int = HOP):
    """(w0, w1, T_b): the frames [w0, w1) that cover the outputs, and the bound of the stream's frames (None: open)."""
    pad, R = dr.pad_of(N, hop), N // hop
    T_b = None if total is None or total < 0 else dr.frames(total, N, hop)
    w0 = max(0, (out_first + pad) // hop - (R - 1))
    w1 = (out_first + out_count - 1 + pad) // hop + 1
    return w0, (w1 if T_b is None else min(w1, T_b)), T_b


def frame_indices(t: int, total, N: int = N_FFT, hop: int = HOP) -> np.ndarray:
    """The samples frame t reads, reflected at 0 and -- ``total`` known -- at the stream's end."""
    j = t * hop - dr.pad_of(N, hop) + np.arange(N)
    j = np.abs(j)
    if total is not None and total >= 0:
        j = np.where(j >= total, 2 * (total - 1) - j, j)
    return j


@lru_cache(maxsize=None)
def _bases(N: int, dtype):
    return np.ascontiguousarray(dr.analysis_basis(N).astype(dtype)), np.ascontiguousarray(dr.synthesis_basis(N).astype(dtype))


_frames = {}


def synthesis_frame(fr: np.ndarray, beta: np.ndarray, s: float, N: int, dtype) -> np.ndarray:
    """v_t [N] of one frame's samples ``fr`` (float32): analysis, subtraction, synthesis, windowed."""
    beta = np.asarray(beta, np.float32)
    key = (fr.tobytes(), beta.tobytes(), float(np.float32(s)), N, np.dtype(dtype).name)
    v = _frames.get(key)
    if v is None:
        A, S = _bases(N, dtype)
        ri = A @ fr.astype(dtype)
        v = S @ dr.subtract(ri[:, None], beta, s, dtype)[:, 0]
        _frames[key] = v
    return v


def call(x, first: int, out_first: int, out_count: int, total, beta, s, N: int = N_FFT, hop: int = HOP, dtype=np.float64):
    """Outputs [out_first, out_first + out_count) of a stream whose samples [first, first + len(x)) are ``x``; ``total``:
    the stream's length, or None / -1 while its end is unknown.  ValueError where a frame reads a sample ``x`` lacks."""
    x = np.asarray(x, np.float32)
    pad = dr.pad_of(N, hop)
    w0, w1, T_b = window(out_first, out_count, total, N, hop)
    if total is not None and total >= 0 and (total <= pad or out_first + out_count > total or first + len(x) > total):
        raise ValueError("the stream is too short, or the row lies behind its end")
    known = total if total is not None and total >= 0 and first + len(x) == total else None
    w2 = dr.hann(N) ** 2
    w2 = w2.astype(np.float32).astype(dtype) if dtype == np.float32 else w2
    y, W = np.zeros(out_count, dtype), np.zeros(out_count, dtype)
    p0 = out_first + pad
    for t in range(w0, w1):                                # ascending t: every output's sum is a chain from 0
        j = frame_indices(t, known, N, hop)
        if j.min() < first or j.max() >= first + len(x):
            raise ValueError(f"frame {t} reads samples [{j.min()}, {j.max()}], the row holds [{first}, {first + len(x)})")
        v = synthesis_frame(x[j - first], beta, s, N, dtype)
        a, b = max(p0, t * hop), min(p0 + out_count, t * hop + N)     # the padded positions of this frame among the outputs
        if a < b:
            y[a - p0:b - p0] += v[a - t * hop:b - t * hop]
            W[a - p0:b - p0] += w2[a - t * hop:b - t * hop]
    assert W.min() >= dr.W_FLOOR, W.min()
    return (y / W).astype(dtype)


def whole(x, beta, s, N: int = N_FFT, hop: int = HOP, dtype=np.float64):
    return call(x, 0, 0, len(x), len(x), beta, s, N, hop, dtype)


class RefEngine:
    """What ``vispeech_amd.denoiser`` needs of an engine, on numpy; ``calls`` counts the ``denoise_rows`` calls and
    ``rows`` keeps every row's positions ``(first, count, out_first, out_count, total)``."""

    def __init__(self, dtype=np.float64, N: int = N_FFT, hop: int = HOP):
        self.dtype, self.N, self.hop = dtype, N, hop
        self.calls, self.rows = 0, []

    def denoise_history(self):
        return self.N - self.hop, self.N - 1

    def denoise_complete(self, n_seen: int, closed: bool = False) -> int:
        return int(n_seen) if closed else complete(int(n_seen), self.N, self.hop)

    def denoise_rows(self, rows, bias):
        self.calls += 1
        outs = []
        for b, (x, first, out_first, out_count, total, strength) in enumerate(rows):
            self.rows.append((first, len(x), out_first, out_count, total))
            if strength is None or strength != strength:
                outs.append(np.zeros(0, np.float32))
                continue
            outs.append(call(x, first, out_first, out_count, total, bias[b], strength, self.N, self.hop, self.dtype))
        return outs
