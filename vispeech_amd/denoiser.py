"""Host logic of the denoiser for streams (include/vispeech_hip.h, "denoiser for streams"): the one
place that decides which samples of a stream a push completes and which it still has to keep.  All arithmetic on audio
runs in ``vsp_denoise_rows``; the classes here drive an *engine* -- any object with

    denoise_history()                 (behind, ahead) = (n_fft - hop, n_fft - 1)
    denoise_complete(n_seen)          (optional) the outputs that are final once n_seen samples of an open stream are in
    denoise_rows(rows, bias)          rows of (x, first, out_first, out_count, total or -1, strength), x holding the
                                      stream's samples [first, first + len(x)); bias [B, spec] -> the rows' outputs;
                                      called with transform="fft" for streams that carry it, and
                                      with no keyword otherwise

-- which is ``vispeech_amd.engine.Engine`` in production and a numpy stand-in in the host tests.

The denoiser has no recurrence: output j sums the frames that cover it, and a frame is final once the samples it reads are
in.  So a stream keeps the ``behind`` samples before its next output and everything after it, and any split of it gives the
bits of the whole.  The delay is between ``n_fft - hop`` and ``n_fft - 1`` samples."""
from __future__ import annotations

from typing import List, Sequence

import numpy as np


def _cat(a, b):
    if isinstance(a, np.ndarray):
        return np.concatenate([a, b])
    import torch
    return torch.cat([a, b])


def _stack(rows):
    if isinstance(rows[0], np.ndarray):
        return np.stack(rows)
    import torch
    return torch.stack(rows)


class Stream:
    """One stream through the denoiser with the speaker's ``bias_row`` [spec] at a fixed ``strength``: ``push(x)`` takes the
    next samples (1-D) and returns the denoised samples they complete -- ``denoise_complete(seen)`` of them in all --,
    ``push(x, final=True)`` returns the rest up to the stream's end (x may be empty), reflected there as the one-shot call
    reflects.  Between pushes the stream keeps the ``behind`` samples before ``out_next`` and those after it (``buf``, which
    starts at sample ``first``; on the device for device input).  A stream that ends at ``pad`` samples or fewer, for which
    the reflection is undefined, returns its own samples.  ``transform``: ``"dft"`` or ``"fft"``, the transform of every call
    the stream makes (``bias_row`` should come from the same one)."""

    def __init__(self, engine, bias_row, strength: float = 0.01, transform: str = "dft"):
        self.eng, self.bias, self.strength = engine, bias_row, float(strength)
        if transform not in ("dft", "fft"):
            raise ValueError(f"denoiser.Stream: transform must be 'dft' or 'fft', not {transform!r}")
        self.transform = transform
        if not (self.strength >= 0.0 and np.isfinite(self.strength)):
            raise ValueError("denoiser.Stream: the strength is a finite number, at least 0")
        self.behind, self.ahead = engine.denoise_history()
        self.buf, self.first, self.seen, self.out_next, self.ended = None, 0, 0, 0, False

    def _complete(self, n: int) -> int:
        """The outputs that are final with ``n`` samples in: the engine's rule (``vsp_denoise_complete``); for an engine that
        has none, the same arithmetic from its history (n_fft = ahead + 1, hop = n_fft - behind, pad = behind / 2)."""
        rule = getattr(self.eng, "denoise_complete", None)
        if rule is not None:
            return rule(n)
        n_fft, pad = self.ahead + 1, self.behind // 2
        hop, room = n_fft - self.behind, n + pad - n_fft
        return max(0, (0 if room < 0 else room // hop + 1) * hop - pad)

    def _take(self, x, final: bool):
        """Appends ``x``; the row of this push ``(x, first, out_first, out_count, total, strength)`` or None (nothing
        completes, or the stream is too short to denoise: ``_advance`` then hands out its samples)."""
        if self.ended:
            raise ValueError("denoiser.Stream: pushed after its final push")
        x = x.reshape(-1)
        self.buf = x if self.buf is None else _cat(self.buf, x)
        self.seen += int(x.shape[0])
        self.ended = bool(final)
        out_end = self.seen if final else max(self.out_next, self._complete(self.seen))
        if out_end <= self.out_next or (final and self.seen <= self.behind // 2):      # (pad = (n_fft - hop) / 2 = behind / 2)
            return None
        return (self.buf, self.first, self.out_next, out_end - self.out_next, self.seen if final else -1, self.strength)

    def _advance(self, row, out):
        """The stream behind a call: ``out`` (the call's result for ``row``, or None) or what stands in for it, and the
        samples the next call no longer reads dropped."""
        if row is not None:
            self.out_next += row[3]
        elif self.ended and self.out_next < self.seen:      # (only a stream of at most pad samples ends so: left alone)
            out, self.out_next = self.buf[self.out_next - self.first:], self.seen
        k = max(self.first, min(self.seen, max(0, self.out_next - self.behind)))
        self.buf, self.first = self.buf[k - self.first:], k
        return self.buf[:0] if out is None else out

    def push(self, x, final: bool = False):
        return push_rows(self.eng, [(self, x, final)])[0]


def push_rows(engine, pushes: Sequence[tuple]) -> List:
    """Several streams advance in ONE ``denoise_rows`` call: ``pushes`` is ``[(stream, x, final), ...]``, each stream at its
    own position with its own bias and strength.  Returns, per push, the samples it completes (an empty array where it
    completes none).  No call is made when no push completes a sample.  The call runs under the streams' transform; streams
    that disagree are refused."""
    if not pushes:
        return []
    if len({id(s) for s, _, _ in pushes}) != len(pushes):
        raise ValueError("denoiser.push_rows: a stream advances once per call")
    if any(s.ended for s, _, _ in pushes):
        raise ValueError("denoiser.Stream: pushed after its final push")
    transforms = {s.transform for s, _, _ in pushes}
    if len(transforms) != 1:
        raise ValueError("denoiser.push_rows: the streams of one call share one transform, not " + " and ".join(sorted(transforms)))
    kw = {} if transforms == {"dft"} else {"transform": transforms.pop()}      # (the default makes the call it always made)
    rows = [s._take(x, final) for s, x, final in pushes]
    live = [i for i, r in enumerate(rows) if r is not None]
    outs = [None] * len(pushes)
    if live:
        done = engine.denoise_rows([rows[i] for i in live], _stack([pushes[i][0].bias for i in live]), **kw)
        for j, i in enumerate(live):
            outs[i] = done[j]
    return [s._advance(r, o) for (s, _, _), r, o in zip(pushes, rows, outs)]
