"""Host logic of the output stage (include/vispeech_hip.h, "output stage"): the plan and taps of the resampling filter,
and the one place that decides which output samples a streamed window completes and which input samples the next window
still needs.  All arithmetic on audio runs in ``vsp_output_chunk``; the functions here drive an *engine* -- any object with

    output_plan                                                  (L, M, H) of the configured stage
    output_chunk(x, x_first, n_max, m0, m1, n_valid, pcm)        output samples [m0, m1) from the window x [B, n]
                                                                 that holds input samples [x_first, x_first + n)

-- which is ``vispeech_amd.engine.Engine`` in production and a double-precision stand-in in the host tests.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, Iterator, Optional, Tuple

import numpy as np

DEFAULT_ZEROS = 32
DEFAULT_BETA = 9.62          # Kaiser's formula for 96 dB, the floor of a 16-bit output


def default_rolloff(zeros: int = DEFAULT_ZEROS) -> float:
    """Puts the stop-band edge on the narrower Nyquist frequency."""
    return 1.0 - 3.065 / zeros


def plan(in_rate: int, out_rate: int, zeros: int = DEFAULT_ZEROS) -> Tuple[int, int, int]:
    """``vsp_resample_plan``: (L, M, H) -- resampling by L / M with a prototype of 2 H + 1 taps."""
    from . import _lib
    L, M, H = C.c_int(), C.c_int(), C.c_int()
    rc = _lib.lib().vsp_resample_plan(int(in_rate), int(out_rate), int(zeros), C.byref(L), C.byref(M), C.byref(H))
    _lib.check(rc, None, f"vsp_resample_plan({in_rate} -> {out_rate}, zeros = {zeros})")
    return L.value, M.value, H.value


def taps(in_rate: int, out_rate: int, zeros: int = DEFAULT_ZEROS, beta: float = DEFAULT_BETA,
         rolloff: Optional[float] = None) -> np.ndarray:
    """``vsp_resample_filter``: the library's own fp32 prototype h[-H .. H]."""
    from . import _lib
    _, _, H = plan(in_rate, out_rate, zeros)
    h = np.zeros(2 * H + 1, dtype=np.float32)
    rc = _lib.lib().vsp_resample_filter(int(in_rate), int(out_rate), int(zeros), float(beta),
                                        0.0 if rolloff is None else float(rolloff), h.ctypes.data_as(C.c_void_p))
    _lib.check(rc, None, "vsp_resample_filter")
    return h


def out_len(n: int, L: int, M: int) -> int:
    """ceil(n L / M): output samples of an utterance of n input samples."""
    return -((-int(n) * L) // M)


def complete_outputs(n_seen: int, L: int, M: int, H: int, ended: bool = False) -> int:
    """How many leading output samples are final once input samples [0, n_seen) are known: sample m is complete when its
    last tap lies inside them, m M + H < L n_seen, or when the input has ended."""
    total = out_len(n_seen, L, M)
    if ended:
        return total
    return min(total, max(0, -((H - L * int(n_seen)) // M)))          # ceil((L n_seen - H) / M)


def history_start(m_next: int, L: int, M: int, H: int) -> int:
    """First input sample that output sample ``m_next`` (the first incomplete one) depends on: ceil((m M - H) / L)."""
    return max(0, -((H - int(m_next) * M) // L))


def _cat(a, b):
    if isinstance(a, np.ndarray):
        return np.concatenate([a, b], axis=1)
    import torch
    return torch.cat([a, b], dim=1)


def one_shot(eng, x, n_valid=None, pcm: bool = True):
    """The whole of x [B, n] in one ``output_chunk`` call -> [B, ceil(n L / M)]."""
    L, M, _ = eng.output_plan
    n = int(x.shape[1])
    return eng.output_chunk(x, 0, n, 0, out_len(n, L, M), n_valid, pcm)


class Stream:
    """The streamed output stage, one window at a time: ``push`` takes the next window [B, n_i] of the input and returns
    the output samples it completes ([B, m_i]; None for a window too short to complete one), ``finish`` returns the tail
    once the input has ended (or None).  Between windows only the input samples that incomplete outputs still need are
    kept (``hist``, which starts at input sample ``first``: about 2 H / L of them, on the device for device windows).  The
    concatenation equals ``one_shot`` of the concatenated input exactly: the same samples go through the same
    ``output_chunk`` arithmetic, whose result depends on (x, m) alone."""

    def __init__(self, eng, n_valid=None, pcm: bool = True):
        self.eng, self.n_valid, self.pcm = eng, n_valid, pcm
        self.plan = eng.output_plan
        self.hist, self.first, self.seen, self.m_next = None, 0, 0, 0

    def push(self, window):
        x = window.reshape(window.shape[0], -1)
        win = x if self.hist is None or self.hist.shape[1] == 0 else _cat(self.hist, x)
        self.seen += int(x.shape[1])
        m_done = complete_outputs(self.seen, *self.plan)
        y = None
        if m_done > self.m_next:
            y = self.eng.output_chunk(win, self.first, self.seen, self.m_next, m_done, self.n_valid, self.pcm)
            self.m_next = m_done
        k = min(self.seen, history_start(self.m_next, *self.plan))
        self.hist, self.first = win[:, k - self.first:], k
        return y

    def finish(self):
        m_end = out_len(self.seen, *self.plan[:2])
        if self.hist is None or m_end <= self.m_next:
            return None
        return self.eng.output_chunk(self.hist, self.first, self.seen, self.m_next, m_end, self.n_valid, self.pcm)


def stream(eng, chunks: Iterable, n_valid=None, pcm: bool = True) -> Iterator:
    """``Stream`` over consecutive windows: yields, per window that completes output samples, those samples, then the
    tail once the windows have ended."""
    s = Stream(eng, n_valid, pcm)
    yield from (y for y in map(s.push, chunks) if y is not None)
    tail = s.finish()
    if tail is not None:
        yield tail


# ---------------------------------------------------------------------------------------------- output rows
# Rows with their own rate and encoding (include/vispeech_hip.h, "output rows").  The functions below drive an engine with
#
#     output_rate_plan(rate)                 (L, M, H) of a rate of the engine's set (``configure_output_rate``)
#     output_row_buffers(K)                  the two history buffers of one request: something indexable by 0 and 1
#     output_rows(rows)                      rows of (x, ended, rate, enc, state_or_None) -> (packed bytes, [(offset, count)])
F32, S16, ULAW, ALAW = 0, 1, 2, 3                                    # VSP_OUT_*, the numbers of VSP_IN_*
NAMES = {"f32": F32, "float32": F32, "s16": S16, "pcm16": S16, "int16": S16, "ulaw": ULAW, "mulaw": ULAW, "alaw": ALAW}
NUMPY_DTYPES = {F32: np.float32, S16: np.int16, ULAW: np.uint8, ALAW: np.uint8}
RATES_MAX = 8
ROWS_MAX = 64
ROW_ALIGN = 16                 # bytes: where a row of a packed result starts


def encoding(enc) -> int:
    """``VSP_OUT_*`` of an encoding given by number or by name (None: PCM16, what the services deliver)."""
    if enc is None:
        return S16
    if isinstance(enc, str):
        if enc.lower() not in NAMES:
            raise ValueError(f"unknown encoding {enc!r}: one of {sorted(NAMES)}")
        return NAMES[enc.lower()]
    if int(enc) not in NUMPY_DTYPES:
        raise ValueError(f"unknown encoding {enc!r}: 0 (float32), 1 (PCM16), 2 (mu-law), 3 (A-law)")
    return int(enc)


def element_size(enc) -> int:
    return np.dtype(NUMPY_DTYPES[encoding(enc)]).itemsize


def encode(pcm16, enc) -> np.ndarray:
    """``vsp_output_encode``: the G.711 compressor of the kernel on the host, int16 values -> code bytes (uint8); PCM16
    comes back as it is."""
    from . import _lib
    enc = encoding(enc)
    s = np.ascontiguousarray(pcm16)
    if s.dtype != np.int16:
        raise ValueError(f"encode wants int16 values, got {s.dtype}")
    if enc == S16:
        return s
    codes = np.zeros(s.shape, dtype=np.uint8)
    rc = _lib.lib().vsp_output_encode(enc, s.ctypes.data_as(C.c_void_p), s.size, codes.ctypes.data_as(C.c_void_p))
    _lib.check(rc, None, "vsp_output_encode")
    return codes


def silence(enc):
    """The encoding's code of 0: 0.0, 0, 0xFF, 0xD5."""
    enc = encoding(enc)
    return np.float32(0.0) if enc == F32 else encode(np.zeros(1, np.int16), enc)[0]


def rows_plan(L: int, M: int, H: int, x_first: int, n: int, ended: bool) -> Tuple[int, int, int, int]:
    """``vsp_output_rows_plan``: (m0, m1, k0, k1) of a call that brings input samples [x_first, x_first + n) -- it delivers
    output samples [m0, m1), reads the history from input sample k0 and leaves the history from k1."""
    from . import _lib
    res = [C.c_int64() for _ in range(4)]
    rc = _lib.lib().vsp_output_rows_plan(int(L), int(M), int(H), int(x_first), int(n), int(bool(ended)), *map(C.byref, res))
    _lib.check(rc, None, f"vsp_output_rows_plan(L = {L}, M = {M}, H = {H}, x_first = {x_first}, n = {n})")
    return tuple(r.value for r in res)


def history_samples(L: int, M: int, H: int) -> int:
    """``vsp_output_history_samples``: floor(2 H / L), the floats of one history buffer."""
    return (2 * int(H)) // int(L)


class RowState:
    """What one request keeps between two ``output_rows`` calls at ``rate``: its two history buffers (``buf[side]`` is read
    by the next call, ``buf[1 - side]`` written) and ``x_first``, the input samples it has brought so far."""

    def __init__(self, eng, rate: int):
        self.rate = int(rate)
        self.plan = tuple(eng.output_rate_plan(self.rate))
        self.K = history_samples(*self.plan)
        self.buf = eng.output_row_buffers(self.K)
        self.side, self.x_first = 0, 0

    def advance(self, n: int) -> None:
        """After a call that brought ``n`` samples: the written buffer becomes the one to read."""
        self.side, self.x_first = 1 - self.side, self.x_first + int(n)


def unpack(host_bytes, spans, encs):
    """The rows of a packed result copied to the host (a uint8 array or bytes) as arrays of their encodings' dtypes."""
    a = np.frombuffer(host_bytes, dtype=np.uint8) if not isinstance(host_bytes, np.ndarray) else host_bytes.reshape(-1).view(np.uint8)
    out = []
    for (off, cnt), enc in zip(spans, encs):
        dt = np.dtype(NUMPY_DTYPES[encoding(enc)])
        out.append(a[off:off + cnt * dt.itemsize].view(dt))
    return out
