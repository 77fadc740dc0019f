"""Host logic of the look-ahead limiter (include/vispeech_hip.h, "true peak and look-ahead limiter"):
the one rounding rule from milliseconds to samples, and the one place that decides which samples of a stream a push
completes and which it still has to keep.  All arithmetic on audio runs in ``vsp_limiter_rows``; the classes here drive an
*engine* -- any object with

    limiter_history(attack, hold)                  (behind, ahead): the samples before and after an output that reach it
    limiter_rows(rows, attack, hold, gains)        rows of (x, first, out_first, out_count, total or -1, ceiling), x holding
                                                   the stream's samples [first, first + len(x)) -> (outs, min_gain)

-- which is ``vispeech_amd.engine.Engine`` in production and a numpy stand-in in the host tests.

The limiter has no recurrence: output n is a function of x[n - behind .. n + ahead].  So a stream keeps ``behind`` samples
of history and the ``ahead`` samples it could not put out yet, and any split of it gives the bits of the whole."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

DEFAULT_ATTACK_MS, DEFAULT_HOLD_MS = 1.5, 20.0          # 66 and 882 samples at 44.1 kHz
MAX_ATTACK, MAX_HOLD = 1024, 8192                       # samples


def samples(ms: float, fs: int) -> int:
    """Milliseconds to samples at ``fs``: rounded to the nearest sample, halves up -- the one rule of this project."""
    ms = float(ms)
    if not ms >= 0.0:
        raise ValueError(f"limiter: {ms} ms: a duration must be at least 0")
    return int(np.floor(ms * int(fs) / 1000.0 + 0.5))


def window(fs: int, attack_ms: Optional[float] = None, hold_ms: Optional[float] = None) -> Tuple[int, int]:
    """``(attack, hold)`` in samples at ``fs`` (None: 1.5 ms and 20 ms), refused where the library would refuse them."""
    A = samples(DEFAULT_ATTACK_MS if attack_ms is None else attack_ms, fs)
    H = samples(DEFAULT_HOLD_MS if hold_ms is None else hold_ms, fs)
    if A > MAX_ATTACK or H > MAX_HOLD:
        raise ValueError(f"limiter: attack {A} and hold {H} samples at {fs} Hz: at most {MAX_ATTACK} and {MAX_HOLD}")
    return A, H


def _cat(a, b):
    if isinstance(a, np.ndarray):
        return np.concatenate([a, b])
    import torch
    return torch.cat([a, b])


class Stream:
    """One stream through the limiter at a fixed ``ceiling`` and static ``gain``: ``push(x)`` takes the next samples (1-D)
    and returns the limited samples they complete -- everything up to ``ahead`` samples before the newest one --,
    ``push(x, final=True)`` returns the rest up to the stream's end (x may be empty).  Between pushes the stream keeps
    ``behind`` samples of history and the pending ``ahead`` samples (``buf``, which starts at sample ``first``; on the device
    for device input).  The delay is ``ahead = attack + 12`` samples."""

    def __init__(self, engine, ceiling: float, gain: float = 1.0, attack: int = 66, hold: int = 882):
        self.eng, self.ceiling, self.gain = engine, float(ceiling), float(gain)
        self.attack, self.hold = int(attack), int(hold)
        self.behind, self.ahead = engine.limiter_history(self.attack, self.hold)
        self.buf, self.first, self.seen, self.out_next, self.ended = None, 0, 0, 0, False
        self.min_gain = None                            # this stream's entry of the last call's min_gain, or None

    def _take(self, x, final: bool):
        """Appends ``x``; the row of this push ``(x, first, out_first, out_count, total, ceiling)`` or None (nothing completes)."""
        if self.ended:
            raise ValueError("limiter.Stream: pushed after its final push")
        x = x.reshape(-1)
        self.buf = x if self.buf is None else _cat(self.buf, x)
        self.seen += int(x.shape[0])
        self.ended = bool(final)
        out_end = self.seen if final else max(self.out_next, self.seen - self.ahead)
        if out_end <= self.out_next:
            return None
        return (self.buf, self.first, self.out_next, out_end - self.out_next, self.seen if final else -1, self.ceiling)

    def _advance(self, row) -> None:
        if row is not None:
            self.out_next += row[3]
        k = max(self.first, min(self.seen, max(0, self.out_next - self.behind)))
        self.buf, self.first = self.buf[k - self.first:], k

    def push(self, x, final: bool = False):
        return push_rows(self.eng, [(self, x, final)])[0]


def push_rows(engine, pushes: Sequence[tuple]) -> List:
    """Several streams advance in ONE ``limiter_rows`` call: ``pushes`` is ``[(stream, x, final), ...]`` (streams of one
    attack and hold, each at its own position).  Returns, per push, the samples it completes (an empty array where it
    completes none).  No call is made when no push completes a sample."""
    if not pushes:
        return []
    A, H = pushes[0][0].attack, pushes[0][0].hold
    if any((s.attack, s.hold) != (A, H) for s, _, _ in pushes):
        raise ValueError("limiter.push_rows: the streams of one call share their attack and hold")
    if len({id(s) for s, _, _ in pushes}) != len(pushes):
        raise ValueError("limiter.push_rows: a stream advances once per call")
    rows = [s._take(x, final) for s, x, final in pushes]
    live = [i for i, r in enumerate(rows) if r is not None]
    res = [s.buf[:0] for s, _, _ in pushes]
    if live:
        outs, mg = engine.limiter_rows([rows[i] for i in live], A, H, [pushes[i][0].gain for i in live])
        for j, i in enumerate(live):
            res[i] = outs[j]
            pushes[i][0].min_gain = mg[j]
    for (s, _, _), r in zip(pushes, rows):
        s._advance(r)
    return res


def spec(value, fs: int, default_ceiling: float = 1.0):
    """``(attack, hold, ceiling, gain)`` -- samples, samples, linear, linear -- of a request or service that names a limiter:
    ``True``, or a mapping of ``attack_ms``, ``hold_ms``, ``ceiling`` and ``gain_db``; None / False: none."""
    if value is None or value is False:
        return None
    vals = dict(attack_ms=None, hold_ms=None, ceiling=None, gain_db=0.0)
    if hasattr(value, "keys"):
        unknown = set(value) - set(vals)
        if unknown:
            raise ValueError(f"limiter: unknown {sorted(unknown)}; the fields are {list(vals)}")
        vals.update(value)
    elif value is not True:
        raise ValueError("limiter: True, or a mapping of attack_ms, hold_ms, ceiling and gain_db")
    A, H = window(fs, vals["attack_ms"], vals["hold_ms"])
    c = float(default_ceiling if vals["ceiling"] is None else vals["ceiling"])
    g_db = float(vals["gain_db"])
    if not (c > 0.0 and np.isfinite(c)):
        raise ValueError("limiter: ceiling must be above 0")
    if not np.isfinite(g_db):
        raise ValueError("limiter: gain_db must be finite")
    return A, H, c, float(10.0 ** (g_db / 20.0))
