"""Host logic of loudness over time (include/vispeech_hip.h, "loudness over time"): a stream's meter
-- momentary, short-term and running integrated loudness per 100 ms -- and the causal leveller steered by the running
level.  All arithmetic on audio runs in the library; the classes here drive an *engine* -- any object with

    loudness_state(B)                               [B, 4] float64 zeros: the K-weighting's state of B new streams
    loudness_table(n, dtype)                        a 1-D table of n entries
    loudness_segments_from(audio, n, fs, state, first)          -> (seg, peak, state_out)
    loudness_time(seg, first, count, fs, tables)    the entries [first, first + count) of (M, S, I, kept), in place
    loudness_level_gains(I, first, count, params, tables)       likewise of (c_db, c)
    loudness_level_apply(x, pos, c, entries, fs, params)        -> the levelled samples, new arrays
    loudness_hist_state(B)                          [B, 2, 1000] int32 zeros: the histograms of B new streams      } streams with
    loudness_time_hist(seg, first, count, fs, hist, tables)     -> (M, S, I, kept, m_max, s_max, lra)              } gate="histogram"

-- which is ``vispeech_amd.engine.Engine`` in production and a numpy stand-in in the host tests (tests/loudness_time_ref.py).

A stream keeps, where the engine keeps its arrays (on the device in production): the samples of its open segment (fewer than
h), the 4-double filter state behind its last complete segment, its tables, which grow by doubling, and with them the gain
reached so far.  Entry s of a table depends on the stream's first (s + 1) h samples and on s alone, and the gain over
segment s on the samples before it, so ANY split of a stream gives the tables and the samples of the one call on the whole
row, bit for bit -- and every sample leaves in the push it arrives in: the leveller has no look-ahead and adds no delay.

``gate="histogram"``: the stream also keeps two histograms of block loudness, integer counts; its
running level I is read from them at a cost that does not grow with the stream (the exact gate walks the prefix), within
0.05 LU of the exact one, and it has a loudness range.  Every value is a function of the counts, so the rule above holds."""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np

MAX_SAMPLES = 1 << 30                 # of a stream: 6.7 hours at 44.1 kHz, 93 minutes (55 924 segments) at 192 kHz
FIRST_CAPACITY = 512                  # segments a new stream's tables hold (51 s); doubled when full

GATES = ("exact", "histogram")

LEVEL_FIELDS = dict(target_lufs=-23.0, max_gain_db=12.0, max_cut_db=12.0, slew_db_per_s=3.0, initial_gain_db=0.0)


def segment_samples(fs: int) -> int:
    return (int(fs) + 5) // 10


def max_segments(fs: int) -> int:
    """The segments a stream may have at ``fs``: its 2^30 samples (at least 55 924, above an hour and a half, at any rate)."""
    return MAX_SAMPLES // segment_samples(fs)


def spec(value):
    """What a request or service names as ``loudness=``: None / False: nothing (returns None); ``True``: a meter only
    (returns ``{}``); a number: the leveller's target; a mapping of ``target_lufs``, ``max_gain_db``, ``max_cut_db``,
    ``slew_db_per_s`` and ``initial_gain_db``.  Returns the five values as a dict, refused where the library would refuse."""
    if value is None or value is False:
        return None
    if value is True:
        return {}
    vals = dict(LEVEL_FIELDS)
    if hasattr(value, "keys"):
        unknown = set(value) - set(vals)
        if unknown:
            raise ValueError(f"loudness: unknown {sorted(unknown)}; the fields are {list(vals)}")
        if "target_lufs" not in value:
            raise ValueError("loudness: a mapping names its target_lufs")
        vals.update(value)
    else:
        vals["target_lufs"] = value
    vals = {k: float(v) for k, v in vals.items()}
    if not math.isfinite(vals["target_lufs"]):
        raise ValueError("loudness: target_lufs must be finite")
    if not vals["max_gain_db"] >= 0.0 or not vals["max_cut_db"] >= 0.0:
        raise ValueError("loudness: max_gain_db and max_cut_db must be at least 0")
    if not vals["slew_db_per_s"] > 0.0:
        raise ValueError("loudness: slew_db_per_s must be above 0")
    if not math.isfinite(vals["initial_gain_db"]):
        raise ValueError("loudness: initial_gain_db must be finite")
    return vals


def _cat(a, b):
    if isinstance(a, np.ndarray):
        return np.concatenate([a, b])
    import torch
    return torch.cat([a, b])


def _stack(rows, width: Optional[int] = None):
    """Rows of equal length (``width`` None) or the rows' first samples padded to ``width`` with zeros, as one 2-D array."""
    if isinstance(rows[0], np.ndarray):
        if width is None:
            return np.stack(rows)
        out = np.zeros((len(rows), width), rows[0].dtype)
    else:
        import torch
        if width is None:
            return torch.stack(rows)
        out = torch.zeros((len(rows), width), dtype=rows[0].dtype, device=rows[0].device)
    for b, r in enumerate(rows):
        out[b, : r.shape[0]] = r
    return out


class Stream:
    """One stream through the meter and, with ``level``, the leveller.  ``push(x)`` takes the next samples (1-D float32, where
    the engine works) and returns ALL of them levelled -- or ``x`` itself when only metering.  ``level``: None / True (meter),
    a target in LUFS, or a mapping (``spec``).  ``final`` only closes the stream: nothing is held back.  ``gate``: "exact"
    (section 4r's running level) or "histogram" (section 4s's, and a ``loudness_range``)."""

    def __init__(self, engine, fs: int, level=None, gate: str = "exact"):
        if gate not in GATES:
            raise ValueError(f"loudness.Stream: gate is one of {GATES}, not {gate!r}")
        self.eng, self.fs, self.h = engine, int(fs), segment_samples(fs)
        self.level = spec(level) or None
        self.gate = gate
        self.hist = engine.loudness_hist_state(1)[0] if gate == "histogram" else None
        self._lra = None
        self.open, self.seen, self.segments, self.ended = None, 0, 0, False
        self.state = engine.loudness_state(1)[0]
        self.capacity = 0
        self.seg = self.M = self.S = self.I = self.kept = self.c_db = self.c = None

    # -- what a meter shows
    @property
    def table(self):
        """``dict(M, S, I, kept)`` (and ``c_db``, ``c`` with a leveller): the entries of the complete segments so far."""
        F = self.segments
        names = ("M", "S", "I", "kept") + (("c_db", "c") if self.level else ())
        return {k: (getattr(self, k)[:F] if F else None) for k in names}

    @property
    def integrated(self) -> float:
        """The running integrated loudness: of all complete segments so far (-inf before the first, and while nothing is kept)."""
        return float(self.I[self.segments - 1]) if self.segments else -math.inf

    @property
    def momentary_max(self) -> float:
        return float(self.M[: self.segments].max()) if self.segments else -math.inf

    @property
    def short_term_max(self) -> float:
        return float(self.S[: self.segments].max()) if self.segments else -math.inf

    @property
    def gain_db(self) -> Optional[float]:
        """The gain the leveller has reached (dB), None for a meter."""
        if not self.level:
            return None
        return float(self.c_db[self.segments - 1]) if self.segments else self.level["initial_gain_db"]

    @property
    def loudness_range(self) -> Optional[float]:
        """The loudness range (LU) of the complete segments so far, from the histogram of 3 s windows; None for an exact stream."""
        if self.hist is None:
            return None
        return 0.0 if self._lra is None else float(self._lra)

    # -- one push, in the three steps of ``push_rows``
    def _take(self, x, final: bool):
        if self.ended:
            raise ValueError("loudness.Stream: pushed after its final push")
        x = x.reshape(-1)
        if self.seen + int(x.shape[0]) > MAX_SAMPLES:
            raise ValueError(f"loudness.Stream: a stream holds at most {MAX_SAMPLES} samples ({max_segments(self.fs)} segments at {self.fs} Hz)")
        self.ended = bool(final)
        piece = x if self.open is None else _cat(self.open, x)
        k = int(piece.shape[0]) // self.h
        self._grow(max(self.segments + k, 1))
        return x, piece, k

    def _grow(self, need: int) -> None:
        if need <= self.capacity:
            return
        cap = max(self.capacity, FIRST_CAPACITY)
        while cap < need:
            cap *= 2
        cap = min(cap, max_segments(self.fs))
        for name, dtype in (("seg", np.float64), ("M", np.float32), ("S", np.float32), ("I", np.float32), ("kept", np.int32),
                            ("c_db", np.float32), ("c", np.float32)):
            new = self.eng.loudness_table(cap, dtype)
            if self.capacity:
                new[: self.capacity] = getattr(self, name)
            setattr(self, name, new)
        self.capacity = cap

    def push(self, x, final: bool = False):
        return push_rows(self.eng, [(self, x, final)])[0]


def push_rows(engine, pushes: Sequence[tuple]) -> List:
    """Several streams of one sample rate advance, each at its own position, in ONE set of calls: ``pushes`` is ``[(stream, x,
    final), ...]``.  The streams that complete a segment share one ``loudness_segments_from`` (their complete segments, padded to a
    batch; the rest stays the stream's open segment) and one ``loudness_time`` -- those with the histogram gate one
    ``loudness_time_hist`` instead; a call may mix both --, the levelled ones among them one
    ``loudness_level_gains``, and every levelled stream that brought samples one ``loudness_level_apply``.  Returns, per push, its
    samples levelled (``x`` itself for a meter)."""
    if not pushes:
        return []
    fs = pushes[0][0].fs
    if any(s.fs != fs for s, _, _ in pushes):
        raise ValueError("loudness.push_rows: the streams of one call share their sample rate")
    if len({id(s) for s, _, _ in pushes}) != len(pushes):
        raise ValueError("loudness.push_rows: a stream advances once per call")
    h = segment_samples(fs)
    taken = [s._take(x, final) for s, x, final in pushes]
    grown = [i for i, (_, _, k) in enumerate(taken) if k]
    if grown:
        st = [pushes[i][0] for i in grown]
        ks = [taken[i][2] for i in grown]
        audio = _stack([taken[i][1][: k * h] for i, k in zip(grown, ks)], max(ks) * h)
        seg, _, state = engine.loudness_segments_from(audio, [k * h for k in ks], fs, state=_stack([s.state for s in st]),
                                                      first=[s.segments * h for s in st])
        first = [s.segments for s in st]
        for j, s in enumerate(st):
            s.seg[first[j]: first[j] + ks[j]] = seg[j, : ks[j]]
            s.state = state[j]
        exact = [j for j, s in enumerate(st) if s.hist is None]
        if exact:
            engine.loudness_time([st[j].seg for j in exact], [first[j] for j in exact], [ks[j] for j in exact], fs,
                                 tables=tuple([getattr(st[j], n) for j in exact] for n in ("M", "S", "I", "kept")))
        hg = [j for j, s in enumerate(st) if s.hist is not None]
        if hg:
            lra = engine.loudness_time_hist([st[j].seg for j in hg], [first[j] for j in hg], [ks[j] for j in hg], fs, [st[j].hist for j in hg],
                                            tables=tuple([getattr(st[j], n) for j in hg] for n in ("M", "S", "I", "kept")))[-1]
            for i, j in enumerate(hg):
                st[j]._lra = lra[i]
        lv = [j for j, s in enumerate(st) if s.level]
        if lv:
            engine.loudness_level_gains([st[j].I for j in lv], [first[j] for j in lv], [ks[j] for j in lv], [st[j].level for j in lv],
                                        tables=([st[j].c_db for j in lv], [st[j].c for j in lv]))
    res = [x for x, _, _ in taken]
    lv = [i for i, (x, _, _) in enumerate(taken) if pushes[i][0].level and int(x.shape[0])]
    if lv:
        st = [pushes[i][0] for i in lv]
        outs = engine.loudness_level_apply([taken[i][0] for i in lv], [s.seen for s in st], [s.c for s in st],
                                           [s.segments + taken[i][2] for i, s in zip(lv, st)], fs, [s.level for s in st])
        for j, i in enumerate(lv):
            res[i] = outs[j]
    for (s, _, _), (x, piece, k) in zip(pushes, taken):
        s.seen += int(x.shape[0])
        s.segments += k
        rest = piece[k * h:]
        s.open = _cat(rest[:0], rest) if int(rest.shape[0]) else None        # (a copy: the push's samples are the caller's)
    return res
