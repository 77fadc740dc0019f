"""Host logic of the input stage (include/vispeech_hip.h, "input stage"): raw samples at the caller's rate -- float32,
PCM16 or G.711 -- to float32 at the model's rate.  The mirror of ``output_stage``: the plan, the taps and the G.711 tables
come from the library's host functions, all arithmetic on audio runs in ``vsp_input_rows``, and which outputs a piece of a
live feed completes (and which raw samples the next piece still needs) is decided by ``output_stage.complete_outputs`` /
``history_start``, which are generic in (L, M, H).  The functions here drive an *engine* -- any object with

    input_plan(rate)                       (L, M, H) of a configured input rate
    input_rows(rows, rate, enc)            rows of (raw, in_first, n_total, m0, m1): ``raw`` (1-D, the encoding's dtype) holds
                                           input samples [in_first, in_first + len(raw)) of a recording of n_total samples
                                           (-1 while it is open); returns one 1-D float32 result per row, output samples
                                           [m0, m1)

-- which is ``vispeech_amd.engine.Engine`` in production and a double-precision stand-in in the host tests.

The filter is ours by specification (the output stage's formula with the rates swapped); it is not librosa's ``resample``.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, Iterator, Optional, Tuple

import numpy as np

from .output_stage import DEFAULT_BETA, DEFAULT_ZEROS, complete_outputs, history_start, out_len

F32, S16, ULAW, ALAW = 0, 1, 2, 3                                    # VSP_IN_*
NAMES = {"f32": F32, "float32": F32, "s16": S16, "pcm16": S16, "int16": S16, "ulaw": ULAW, "mulaw": ULAW, "alaw": ALAW}
NUMPY_DTYPES = {F32: np.float32, S16: np.int16, ULAW: np.uint8, ALAW: np.uint8}
RATES_MAX = 8
ROWS_MAX = 64


def encoding(enc) -> int:
    """``VSP_IN_*`` of an encoding given by number or by name (None: float32)."""
    if enc is None:
        return F32
    if isinstance(enc, str):
        if enc.lower() not in NAMES:
            raise ValueError(f"unknown encoding {enc!r}: one of {sorted(NAMES)}")
        return NAMES[enc.lower()]
    if int(enc) not in NUMPY_DTYPES:
        raise ValueError(f"unknown encoding {enc!r}: 0 (float32), 1 (PCM16), 2 (mu-law), 3 (A-law)")
    return int(enc)


def as_raw(samples, enc: int) -> np.ndarray:
    """``bytes`` or an array -> a numpy array of the encoding's own dtype.  Nothing is converted: PCM16 wants int16, G.711
    wants uint8 (bytes are taken as little-endian samples); float input of any float dtype becomes float32."""
    dt = NUMPY_DTYPES[enc]
    if isinstance(samples, (bytes, bytearray, memoryview)):
        return np.frombuffer(samples, dtype=np.dtype(dt).newbyteorder("<")).astype(dt, copy=False)
    a = np.asarray(samples)
    if enc == F32:
        if a.dtype.kind != "f":
            raise ValueError(f"float32 input must be a float array, got {a.dtype}")
        return np.ascontiguousarray(a, dtype=np.float32)
    if a.dtype != dt:
        raise ValueError(f"encoding {enc} wants {np.dtype(dt).name} samples, got {a.dtype}")
    return np.ascontiguousarray(a)


def plan(in_rate: int, model_rate: int, zeros: int = DEFAULT_ZEROS) -> Tuple[int, int, int]:
    """``vsp_input_plan``: (L, M, H) -- resampling by L / M with a prototype of 2 H + 1 taps."""
    from . import _lib
    L, M, H = C.c_int(), C.c_int(), C.c_int()
    rc = _lib.lib().vsp_input_plan(int(in_rate), int(model_rate), int(zeros), C.byref(L), C.byref(M), C.byref(H))
    _lib.check(rc, None, f"vsp_input_plan({in_rate} -> {model_rate}, zeros = {zeros})")
    return L.value, M.value, H.value


def taps(in_rate: int, model_rate: int, zeros: int = DEFAULT_ZEROS, beta: float = DEFAULT_BETA,
         rolloff: Optional[float] = None) -> np.ndarray:
    """``vsp_input_filter``: the library's own fp32 prototype h[-H .. H]."""
    from . import _lib
    _, _, H = plan(in_rate, model_rate, zeros)
    h = np.zeros(2 * H + 1, dtype=np.float32)
    rc = _lib.lib().vsp_input_filter(int(in_rate), int(model_rate), int(zeros), float(beta),
                                     0.0 if rolloff is None else float(rolloff), h.ctypes.data_as(C.c_void_p))
    _lib.check(rc, None, "vsp_input_filter")
    return h


def decode_table(enc) -> np.ndarray:
    """``vsp_input_decode_table``: the 256 float32 values of a G.711 law, as the kernel decodes them."""
    from . import _lib
    t = np.zeros(256, dtype=np.float32)
    rc = _lib.lib().vsp_input_decode_table(encoding(enc), t.ctypes.data_as(C.c_void_p))
    _lib.check(rc, None, "vsp_input_decode_table")
    return t


def _cat(a, b):
    if isinstance(a, np.ndarray):
        return np.concatenate([a, b])
    import torch
    return torch.cat([a, b])


def one_shot(eng, raw, n: int, rate: int, enc):
    """The recording ``raw[:n]`` in one ``input_rows`` call -> its ceil(n L / M) samples at the model's rate."""
    L, M, _ = eng.input_plan(rate)
    n = int(n)
    return eng.input_rows([(raw[:n], 0, n, 0, out_len(n, L, M))], rate, encoding(enc))[0]


class Stream:
    """The input stage over a live feed, one piece at a time: ``push`` takes the next raw piece (1-D, in the stream's rate
    and encoding) and returns the model-rate samples it completes (None for a piece too short to complete one), ``finish``
    returns the tail once the recording has ended (or None).  Between pieces only the raw samples that incomplete outputs
    still need are kept (``hist``, which starts at input sample ``first``: at most floor(2 H / L) of them, on the device
    for device pieces).  The concatenation equals ``one_shot`` of the concatenated pieces exactly: the same samples go
    through the same ``input_rows`` arithmetic, whose result depends on (decoded x, m) alone.

    ``take`` / ``take_tail`` are the two halves for a caller that batches the rows of many streams into one
    ``input_rows`` call: they return the row (or None) and advance the stream."""

    def __init__(self, eng, rate: int, enc):
        self.eng, self.rate, self.enc = eng, int(rate), encoding(enc)
        self.plan = eng.input_plan(self.rate)
        self.hist, self.first, self.seen, self.m_next = None, 0, 0, 0

    def take(self, piece):
        x = piece.reshape(-1)
        win = x if self.hist is None or self.hist.shape[0] == 0 else _cat(self.hist, x)
        self.seen += int(x.shape[0])
        m_done = complete_outputs(self.seen, *self.plan)
        row = None
        if m_done > self.m_next:
            row = (win, self.first, -1, self.m_next, m_done)
            self.m_next = m_done
        k = min(self.seen, history_start(self.m_next, *self.plan))
        self.hist, self.first = win[k - self.first:], k
        return row

    def take_tail(self):
        m_end = out_len(self.seen, *self.plan[:2])
        if self.hist is None or m_end <= self.m_next:
            return None
        row = (self.hist, self.first, self.seen, self.m_next, m_end)
        self.m_next = m_end
        return row

    def _run(self, row):
        return None if row is None else self.eng.input_rows([row], self.rate, self.enc)[0]

    def push(self, piece):
        return self._run(self.take(piece))

    def finish(self):
        return self._run(self.take_tail())


def stream(eng, pieces: Iterable, rate: int, enc) -> Iterator:
    """``Stream`` over consecutive pieces: yields, per piece that completes output samples, those samples, then the tail."""
    s = Stream(eng, rate, enc)
    yield from (y for y in map(s.push, pieces) if y is not None)
    tail = s.finish()
    if tail is not None:
        yield tail
