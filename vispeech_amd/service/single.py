"""The single-flight services: ``SynthesisService`` (one synthesis per model, one-shot and streamed) and one such slot per
context of a pool, ``PooledSynthesisService``."""
from __future__ import annotations

import io
import threading
import wave
from typing import Dict, Iterator, Optional

import numpy as np

from ._pcm import Busy, _check_numerics, _host_i16, _row_pcm16, pcm16


class _LockedStream:
    """Iterator over the chunks of one streamed synthesis that OWNS the service's single-flight lock."""

    def __init__(self, service: "SynthesisService", chunks: Iterator[bytes]):
        self._service = service
        self._chunks = chunks
        self._held = True

    def __iter__(self):
        return self

    def __next__(self) -> bytes:
        if not self._held:
            raise StopIteration
        try:
            return next(self._chunks)
        except BaseException:          # exhausted (StopIteration) or failed: either way the synthesis is over
            self.close()
            raise

    def close(self) -> None:
        if self._held:
            self._held = False
            try:
                self._chunks.close()
            finally:
                self._service.release()

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class SynthesisService:
    """One model, one synthesis at a time, never queueing (reference inference_api.py:13, 37)."""

    def __init__(self, net, sampling_rate: int = 44100, chunk_frames: int = 64, noise_scale: float = 0.667, stream=None,
                 *, output_rate: Optional[int] = None, device_pcm: bool = False, isolated: bool = False):
        """``isolated``: run every batch in isolated mode (``SynthesizerTrn.infer(isolated=True)``): an utterance's audio is
        what the reference returns for it alone, whatever it is batched with.
        ``output_rate``: deliver PCM16 at this rate instead of the model's -- the reference's service sends the
        22.05 kHz file that ``ffmpeg -ar 22050`` makes of the waveform (inference_api.py:51); here the engine's output
        stage resamples and quantises on the GPU, one-shot and per streamed chunk, and int16 is what crosses to the
        host.  ``device_pcm=True`` without a rate: the same stage as a pass-through (GPU quantisation at the model's
        rate).  Neither: the float32 copy and the host quantiser, exactly as before."""
        self.net = net
        self.sampling_rate = int(sampling_rate)
        self.chunk_frames = int(chunk_frames)
        self.noise_scale = float(noise_scale)
        self.isolated = bool(isolated)
        # (passed only when set: engine / net stand-ins of older callers and tests need not know the keyword)
        self._iso = {"isolated": True} if self.isolated else {}
        self._lock = threading.Lock()
        self._stream = stream          # a torch.cuda.Stream all of this service's GPU work runs on (None: the caller's)
        self.output_rate = None if output_rate is None else int(output_rate)
        self._output_stage = output_rate is not None or bool(device_pcm)
        if self._output_stage:
            with self._scope():
                net._engine.configure_output(self.delivered_rate, in_rate=self.sampling_rate)

    @property
    def delivered_rate(self) -> int:
        """Sampling rate of the PCM16 this service returns."""
        return self.sampling_rate if self.output_rate is None else self.output_rate

    def _output_engine(self):
        """The engine, checked: the output stage is state of the ENGINE, and another service on the same model may have
        configured another rate since this one was built."""
        eng = self.net._engine
        if eng.output_rate != self.delivered_rate:
            raise RuntimeError(f"the engine's output stage delivers {eng.output_rate} Hz, this service {self.delivered_rate} Hz: "
                               "one output rate per model context")
        return eng

    def _scope(self):
        """The stream scope of this service's GPU work (``PooledSynthesisService`` gives every slot its own stream)."""
        import contextlib
        if self._stream is None:
            return contextlib.nullcontext()
        import torch
        return torch.cuda.stream(self._stream)

    # ------------------------------------------------------------------ single-flight
    def try_acquire(self) -> bool:
        return self._lock.acquire(blocking=False)

    def release(self) -> None:
        self._lock.release()

    @property
    def busy(self) -> bool:
        return self._lock.locked()

    # ------------------------------------------------------------------ one-shot (what the reference's /tts does)
    def synthesize(self, batch: Dict[str, "np.ndarray"], utterance: int = 0, noise=None) -> Optional[np.ndarray]:
        """``batch`` = the arrays of ``vispeech_amd.text.collate_rows`` (phonemes, lengths, sid and optionally
        duration / f0 / energy).  Returns the PCM16 samples of ``utterance`` (valid part only), or ``None`` if
        another request is in flight (the reference returns None -> "busy")."""
        if not self.try_acquire():
            return None
        try:
            with self._scope():
                o, frames = self._infer(batch, noise)
                n = int(frames[utterance]) * self.net.dims.total_upsample
                # (device -> host: int16 at the output rate, or the float samples once the stream has drained)
                pcm = _row_pcm16(o[utterance:utterance + 1, 0, :n], self._output_engine() if self._output_stage else None)
            _check_numerics(self.net)
            return pcm
        finally:
            self.release()

    def wav_bytes(self, batch, utterance: int = 0, noise=None) -> Optional[bytes]:
        """The reference's response body: a mono PCM16 WAV (inference_api.py:50-52, 64) at the model's sampling rate or, with
        ``output_rate``, at that rate."""
        pcm = self.synthesize(batch, utterance, noise)
        if pcm is None:
            return None
        buf = io.BytesIO()
        with wave.open(buf, "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(self.delivered_rate)
            w.writeframes(pcm.tobytes())
        return buf.getvalue()

    # ------------------------------------------------------------------ streamed
    def stream(self, batch, utterance: int = 0, noise=None) -> Iterator[bytes]:
        """PCM16 bytes of ``utterance``, one vocoder chunk (``chunk_frames`` frames) at a time.  Raises ``Busy``
        at once when another synthesis is in flight.  The lock is owned by the returned ``_LockedStream`` and is
        released exactly once: when the stream is exhausted, fails, is ``close()``d, or is dropped -- also when it
        was never started (a plain generator that is never advanced would never run its ``finally``).  The
        concatenation equals ``synthesize`` byte for byte."""
        if not self.try_acquire():
            raise Busy("another synthesis is in flight")
        return _LockedStream(self, self._stream_chunks(batch, utterance, noise))

    def _stream_chunks(self, batch, utterance, noise) -> Iterator[bytes]:
        import torch
        net, eng = self.net, self.net._engine
        with self._scope():
            enc, frames, tf = self._encode(batch)
            z_noise = noise if noise is not None else torch.randn(
                enc["x_var"].shape[0], net.dims.inter_channels, tf, dtype=torch.float32, device=eng.device)
            dec = eng.decode(enc, tf, z_noise, self.noise_scale, max_len=0, **self._iso)     # everything but the vocoder
            left = int(frames[utterance]) * net.dims.total_upsample
            if self.isolated:
                # the utterance's own frames: a tensor that really ends where the isolated batch's ended artificially
                u, utterance = utterance, 0
                chunks = eng.generator_stream(dec["z"][u:u + 1, :, :int(frames[u])], enc["g"][u:u + 1], self.chunk_frames)
            else:
                chunks = eng.generator_stream(dec["z"], enc["g"], self.chunk_frames)
        if self._output_stage:
            yield from self._stream_output_stage(chunks, utterance, left)
            return
        while left > 0:
            # (the stream scope is entered per chunk, never held across a yield: the consumer's thread keeps its own stream)
            with self._scope():
                o = next(chunks, None)
                if o is None:
                    break
                piece = pcm16(o[utterance, 0, : min(left, o.shape[2])])
            _check_numerics(self.net)
            left -= piece.size
            yield piece.tobytes()

    def _stream_output_stage(self, chunks, utterance: int, left: int) -> Iterator[bytes]:
        """The streamed path through the output stage: each vocoder chunk's valid samples go through
        ``Engine.output_stream``, which returns the output samples that chunk completes; the tail follows the last one."""
        def valid_part():
            n = left
            for o in chunks:
                if n <= 0:
                    break
                take = min(n, o.shape[2])
                n -= take
                yield o[utterance:utterance + 1, 0, :take]
        pieces = self._output_engine().output_stream(valid_part(), None, pcm=True)
        while True:
            with self._scope():                      # (per chunk, as above: never held across a yield)
                y = next(pieces, None)
                if y is None:
                    break
                piece = _host_i16(y)
            _check_numerics(self.net)
            yield piece.tobytes()

    # ------------------------------------------------------------------ helpers
    def _controls(self, batch):
        return {k: batch.get(k) for k in ("duration", "f0", "energy")}

    def _encode(self, batch):
        import torch
        eng = self.net._engine
        c = self._controls(batch)
        t = lambda a: None if a is None else torch.as_tensor(np.asarray(a))
        enc = eng.encode(t(batch["phonemes"]), t(batch["lengths"]), t(batch["sid"]), t(c["duration"]), t(c["f0"]),
                         t(c["energy"]), **self._iso)
        frames, tf = eng.frame_lengths_host(enc["frame_lengths"])
        if tf <= 0:
            raise ValueError("all durations are zero: nothing to synthesise")
        return enc, frames, tf

    def _infer(self, batch, noise):
        import torch
        net = self.net
        c = self._controls(batch)
        t = lambda a: None if a is None else torch.as_tensor(np.asarray(a)).to(net.device)
        o, x_mask, *_ = net.infer(t(batch["phonemes"]), t(batch["lengths"]), sid=t(batch["sid"]),
                                  noise_scale=self.noise_scale, duration_control=t(c["duration"]),
                                  pitch_control=t(c["f0"]), energy_control=t(c["energy"]), noise=noise, **self._iso)
        return o, x_mask.sum(dim=(1, 2)).cpu().tolist()


class PooledSynthesisService:
    """Up to N syntheses in flight on one GPU (round 6): one single-flight ``SynthesisService`` per context of an
    ``InFlightPool``, each on its context's stream.  The reference's semantics generalised, not replaced: a request is
    served by the first FREE slot or refused at once (``None`` / ``Busy``) -- never queued (inference_api.py:13, 37 with
    N locks instead of one).  The frame-rate half of one request overlaps the vocoder of another: 3.1 -> 2.1 -> 1.7 ms per
    single-utterance request at 1 / 2 / 3 slots (profiles/r06_batches_in_flight.txt)."""

    def __init__(self, pool, sampling_rate: int = 44100, chunk_frames: int = 64, noise_scale: float = 0.667, *,
                 output_rate: Optional[int] = None, device_pcm: bool = False, isolated: bool = False):
        self.slots = [SynthesisService(net, sampling_rate, chunk_frames, noise_scale, stream=st, output_rate=output_rate,
                                       device_pcm=device_pcm, isolated=isolated)
                      for net, st in zip(pool.nets, pool.streams if pool.streams[0] is not None else [None] * len(pool.nets))]

    @property
    def busy(self) -> bool:
        return all(s.busy for s in self.slots)

    def _first_free(self, method: str, *args):
        """``method`` of the first slot that is free (a taken slot answers None or raises ``Busy``: try the next); None if
        every slot is taken."""
        for s in self.slots:
            try:
                result = getattr(s, method)(*args)
            except Busy:
                continue
            if result is not None:
                return result
        return None

    def synthesize(self, batch, utterance: int = 0, noise=None) -> Optional[np.ndarray]:
        return self._first_free("synthesize", batch, utterance, noise)

    def wav_bytes(self, batch, utterance: int = 0, noise=None) -> Optional[bytes]:
        return self._first_free("wav_bytes", batch, utterance, noise)

    def stream(self, batch, utterance: int = 0, noise=None) -> Iterator[bytes]:
        chunks = self._first_free("stream", batch, utterance, noise)
        if chunks is None:
            raise Busy("every synthesis slot is taken")
        return chunks
