"""Double-precision restatement of the input stage (include/vispeech_hip.h, "input stage"), kept beside the tests that
use it.  Nothing here calls the library: the plan and its limits, the filter (the output stage's published formula, rates
swapped) and the two G.711 decoding rules are written out in numpy; the resampling sum is ``output_stage_ref.resample_fp64``."""
from math import gcd

import numpy as np

import output_stage_ref as out_ref

MODEL_RATE = 44100
F32, S16, ULAW, ALAW = 0, 1, 2, 3
DTYPES = {F32: np.float32, S16: np.int16, ULAW: np.uint8, ALAW: np.uint8}
MAX_L, MAX_M, MAX_ZEROS = 441, 640, 64
#        in_rate: (L, M)
TABLE = {16000: (441, 160), 8000: (441, 80), 32000: (441, 320), 48000: (147, 160), 96000: (147, 320),
         192000: (147, 640), 22050: (2, 1), 44100: (1, 1)}


def plan(in_rate, model_rate=MODEL_RATE, zeros=32):
    """(L, M, H), or None where the stage does not cover the pair."""
    g = gcd(in_rate, model_rate)
    L, M = model_rate // g, in_rate // g
    if L > MAX_L or M > MAX_M or not 1 <= zeros <= MAX_ZEROS:
        return None
    return L, M, (0 if L == M == 1 else zeros * max(L, M))


def filter_fp64(in_rate, model_rate=MODEL_RATE, zeros=32, beta=9.62, rolloff=None):
    """h[n], n = -H .. H:  L fc sinc(fc n) kaiser(2 H + 1, beta)[n + H],  fc = rolloff / max(L, M); one unit tap for L = M = 1."""
    L, M, H = plan(in_rate, model_rate, zeros)
    if H == 0:
        return np.ones(1)
    rolloff = 1.0 - 3.065 / zeros if rolloff is None else rolloff
    fc = rolloff / max(L, M)
    n = np.arange(-H, H + 1, dtype=np.float64)
    return L * fc * np.sinc(fc * n) * np.kaiser(2 * H + 1, beta)


def ulaw_linear(code):
    """ITU-T G.711 mu-law, the 16-bit linear value of a code byte: the complemented byte is sign | exponent | mantissa."""
    u = ~np.asarray(code, dtype=np.int64) & 0xFF
    t = ((((u & 15) << 3) + 0x84) << ((u >> 4) & 7)) - 0x84
    return np.where(u & 0x80, -t, t)


def alaw_linear(code):
    """ITU-T G.711 A-law: the byte with its even bits inverted is sign | exponent | mantissa; a set sign bit is positive."""
    a = (np.asarray(code, dtype=np.int64) ^ 0x55) & 0xFF
    e, t = (a >> 4) & 7, ((a & 15) << 4) + 8
    t = np.where(e >= 1, (t + 0x100) << np.maximum(e - 1, 0), t)
    return np.where(a & 0x80, t, -t)


def decode(raw, enc):
    """Raw samples -> the float32 the stage resamples (every rule is exact in float32)."""
    raw = np.asarray(raw)
    if enc == F32:
        assert raw.dtype == np.float32
        return raw
    assert raw.dtype == DTYPES[enc]
    v = raw.astype(np.int64) if enc == S16 else (ulaw_linear(raw) if enc == ULAW else alaw_linear(raw))
    x = (v / 32768.0).astype(np.float32)
    assert np.array_equal(x.astype(np.float64) * 32768.0, v)
    return x


def random_raw(rng, n, enc):
    """n raw samples of an encoding: a clipped signal for float32, every code equally likely for the integer encodings."""
    if enc == F32:
        return np.tanh(0.5 * rng.standard_normal(n)).astype(np.float32)
    if enc == S16:
        return rng.integers(-32768, 32768, n).astype(np.int16)
    return rng.integers(0, 256, n).astype(np.uint8)


def poison(enc):
    """What the tests put where nothing may be read: NaN, 0x7FFF, 0x80 (full scale in both laws)."""
    return {F32: np.float32(np.nan), S16: np.int16(0x7FFF), ULAW: np.uint8(0x80), ALAW: np.uint8(0x80)}[enc]


def resample_fp64(raw, enc, h, L, M, m0=0, m1=None, with_bound=False):
    """The fp64 sum over the taps ``h`` and the exactly decoded input (``output_stage_ref.resample_fp64``)."""
    return out_ref.resample_fp64(decode(raw, enc), h, L, M, m0, m1, with_bound)


out_len = out_ref.out_len
