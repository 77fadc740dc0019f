"""Service wrapper around the synthesis path.

The reference's web app (``inference_api.py:13, 35-65``) guards its one model with a NON-BLOCKING lock: a request
that arrives while another is being synthesised is answered "busy" at once (``mutex.acquire(blocking=False)``,
:37), otherwise ``infer`` runs and the waveform is written as a 44.1 kHz PCM16 WAV (:50).  ``SynthesisService``
keeps those semantics -- one synthesis in flight per model, callers are refused rather than queued -- and adds
what the MI355X path makes possible: the vocoder output is STREAMED, chunk by chunk, as PCM16 bytes
(``vsp_generator_stream_chunk``: the 13/14-frame-halo streamer, bit-identical to the one-shot waveform), so the
first audio leaves after one chunk instead of after the whole utterance.  Pure host logic; all arithmetic runs in
libvispeech_hip through ``vispeech_amd.models.SynthesizerTrn``.
"""
from __future__ import annotations

import collections
import io
import threading
import wave
import concurrent.futures
import queue
import time
from typing import Dict, Iterator, Optional, Sequence

import numpy as np


def pcm16(audio) -> np.ndarray:
    """float waveform in [-1, 1] -> little-endian int16 (the conversion of ``utils.write_wav``)."""
    a = audio.detach().cpu().numpy() if hasattr(audio, "detach") else np.asarray(audio)
    return np.clip(np.rint(np.asarray(a, dtype=np.float32).reshape(-1) * 32767.0), -32768, 32767).astype("<i2")


def _host_i16(y) -> np.ndarray:
    """int16 output of the engine's output stage -> little-endian int16 on the host."""
    a = y.detach().cpu().numpy() if hasattr(y, "detach") else np.asarray(y)
    return np.ascontiguousarray(a.reshape(-1), dtype="<i2")


class Busy(RuntimeError):
    """Another synthesis is in flight (the reference answers such a request with a 'server busy' text)."""


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
                hop = self.net.dims.total_upsample
                if self._output_stage:
                    y, _ = self._output_engine().output(o[utterance:utterance + 1, 0, : int(frames[utterance]) * hop], pcm=True)
                    pcm = _host_i16(y)                                            # (device -> host: int16 at the output rate)
                else:
                    pcm = pcm16(o[utterance, 0, : int(frames[utterance]) * hop])  # (device -> host: the stream has drained)
            self._check_numerics()
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
            self._check_numerics()
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
            self._check_numerics()
            yield piece.tobytes()

    # ------------------------------------------------------------------ helpers
    def _check_numerics(self) -> None:
        """After a device -> host copy: raise if a kernel reported values outside the range the split-f16 matrix kernels
        represent (Engine.check_numerics; the audio just copied would be inf / NaN garbage)."""
        eng = getattr(self.net, "_engine", None)
        if eng is not None and hasattr(eng, "check_numerics"):
            eng.check_numerics(sync=False)

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

    def synthesize(self, batch, utterance: int = 0, noise=None) -> Optional[np.ndarray]:
        for s in self.slots:
            pcm = s.synthesize(batch, utterance, noise)          # (None = this slot is taken: try the next)
            if pcm is not None:
                return pcm
        return None

    def wav_bytes(self, batch, utterance: int = 0, noise=None) -> Optional[bytes]:
        for s in self.slots:
            wav = s.wav_bytes(batch, utterance, noise)
            if wav is not None:
                return wav
        return None

    def stream(self, batch, utterance: int = 0, noise=None) -> Iterator[bytes]:
        for s in self.slots:
            try:
                return s.stream(batch, utterance, noise)
            except Busy:
                continue
        raise Busy("every synthesis slot is taken")


def _row_table(batch, scales, noise_scale: float):
    """The per-row table of a batch of requests (``models.RowControls``), or None where the batch needs none: no request
    named a scale and every row carries all three controls -- then the services make the calls they always made.
    ``scales``: per request ``(duration_scale, pitch_scale, energy_scale, noise_scale)``, None = 1.0 and the service's
    ``noise_scale``.  ``given`` is ``collate_rows``' array; a collate callable that returns none gives every row the
    controls its batch has."""
    B = len(scales)
    given = batch.get("given")
    if all(v is None for sc in scales for v in sc) and (given is None or bool(np.all(given))):
        return None
    if given is None:
        given = np.tile(np.array([[batch.get(k) is not None for k in ("duration", "f0", "energy")]], dtype=bool), (B, 1))
    from .models import RowControls
    col = lambda i, default: np.array([default if sc[i] is None else float(sc[i]) for sc in scales], dtype=np.float32)
    return RowControls(col(0, 1.0), col(1, 1.0), col(2, 1.0), col(3, noise_scale), np.asarray(given, dtype=bool))


def _table_controls(batch, rows_ctl):
    """duration / f0 / energy of a batch that runs with a table: a control no row is given is not passed."""
    return tuple(batch.get(k) if rows_ctl.given[:, i].any() else None for i, k in enumerate(("duration", "f0", "energy")))


def _text_latents(eng, collate, rows, seeds, scales, noise_scale: float):
    """The text requests of one batch or admitted group to their latent: ``collate``, the per-row table where the requests
    need one, then ONE isolated ``encode`` / ``frame_lengths_host`` / ``decode(max_len=0)``.  Returns per request
    ``(z row [inter, T], g row, frames)``; a request of no frames gives ``(None, None, 0)``."""
    import torch
    batch = collate(rows)
    t = lambda a: None if a is None else torch.as_tensor(np.asarray(a))
    ctl = (batch.get("duration"), batch.get("f0"), batch.get("energy"))
    table = _row_table(batch, scales, noise_scale)
    kw = {}
    if table is not None:                # (passed only when set: a group without one makes the calls it always made)
        ctl, kw = _table_controls(batch, table), {"row_controls": table}
    enc = eng.encode(t(batch["phonemes"]), t(batch["lengths"]), t(batch["sid"]), t(ctl[0]), t(ctl[1]), t(ctl[2]),
                     isolated=True, **kw)
    frames, tf = eng.frame_lengths_host(enc["frame_lengths"])
    z = None
    if tf > 0:
        z = eng.decode(enc, tf, None, noise_scale, max_len=0, noise_seed=list(seeds), isolated=True, **kw)["z"]
    return [(z[b], enc["g"][b], int(frames[b])) if int(frames[b]) > 0 else (None, None, 0) for b in range(len(rows))]


class _Conversion:
    """A conversion request of the batching services (``submit_conversion``): a recording at the model's rate, the speaker
    it was spoken by and the speaker to convert it to.  To the vocoder it is a row like any other -- a latent, a speaker
    vector and a length -- so it shares generator calls and ticks with text requests."""

    def __init__(self, audio, sid_src: int, sid_tgt: int, noise_scale):
        a = np.ascontiguousarray(np.asarray(audio, dtype=np.float32))
        if a.ndim != 1:
            raise ValueError("audio must be a 1-D float32 array at the model's sampling rate")
        self.audio, self.sid_src, self.sid_tgt = a, int(sid_src), int(sid_tgt)
        self.noise_scale = 1.0 if noise_scale is None else float(noise_scale)      # (1.0: the reference's posterior)


def _convert_latents(eng, jobs, seeds):
    """The conversion requests of one batch or admitted group through ``Engine.convert_latent``: ONE call (one per
    distinct ``noise_scale``, which is an argument of the call, where the requests name several).  Returns per request
    ``(z_hat row, g row, frames)``; a recording too short for a frame gives ``(None, None, 0)``.  The frame counts are
    host arithmetic (``frames_host``): nothing is read back from the device."""
    out = [(None, None, 0)] * len(jobs)
    for scale in sorted({j.noise_scale for j in jobs}):
        idx = [i for i, j in enumerate(jobs) if j.noise_scale == scale and eng.convert_frames(j.audio.size) > 0]
        if not idx:
            continue
        n = [jobs[i].audio.size for i in idx]
        audio = np.zeros((len(idx), max(n)), dtype=np.float32)
        for k, i in enumerate(idx):
            audio[k, : n[k]] = jobs[i].audio
        r = eng.convert_latent(audio, n, [jobs[i].sid_src for i in idx], [jobs[i].sid_tgt for i in idx], None,
                               noise_seed=[int(seeds[i]) for i in idx], noise_scale=scale)
        for k, i in enumerate(idx):
            out[i] = (r["z_hat"][k], r["g"][k], int(r["frames_host"][k]))
    return out


class BatchingSynthesisService:
    """Requests from many callers, synthesised together (round 10).  The services above refuse a request while another is in
    flight, because in the reference's padded batch an utterance's audio depends on its batch-mates; in ISOLATED mode it
    does not, so requests can share a batch: ``submit`` queues one ``collate_rows`` row with its own noise seed and
    returns a future of its PCM16; one worker thread collects up to ``max_batch`` requests -- waiting at most
    ``max_wait_s`` after the first -- collates them and runs ONE ``net.infer(..., isolated=True)`` with the requests' seeds.
    A failing batch fails its own futures and nothing else.  No retry, no priority.
    A request may leave any of durations / f0 / energy to the predictors (``text.request_row``) and name its own
    ``duration_scale`` / ``pitch_scale`` / ``energy_scale`` / ``noise_scale``: such a batch runs with the per-row table built
    from its requests (``infer(row_controls=...)``), and each request is still what the reference returns for it alone.
    ``submit_conversion`` queues a recording to convert from one speaker to another (``SynthesizerTrn.convert_audio``); a
    collected batch may hold both kinds: the text rows go to their latent (``encode`` / ``frame_lengths_host`` /
    ``decode(max_len=0)``), the conversions through one ``convert_latent``, and ONE ``generator_ragged`` call produces every
    waveform.  A batch without a conversion makes exactly the ``net.infer`` call above.
    ``table`` / ``spk2id``: what ``collate_rows`` needs to pad the rows (or ``collate``: any callable rows -> batch arrays)."""

    def __init__(self, net, max_batch: int = 16, max_wait_s: float = 0.005, noise_scale: float = 0.667, *, table=None,
                 spk2id=None, collate=None, output_rate: Optional[int] = None, sampling_rate: int = 44100):
        if max_batch < 1 or max_wait_s < 0:
            raise ValueError("max_batch >= 1 and max_wait_s >= 0")
        if collate is None:
            if table is None or spk2id is None:
                raise ValueError("pass table and spk2id (for collate_rows) or a collate callable")
            from .text import collate_rows
            collate = lambda rows: collate_rows(rows, table, spk2id)
        self._collate = collate
        self.net, self.max_batch, self.max_wait_s = net, int(max_batch), float(max_wait_s)
        self.noise_scale = float(noise_scale)
        self.output_rate = None if output_rate is None else int(output_rate)
        if self.output_rate is not None:
            net._engine.configure_output(self.output_rate, in_rate=int(sampling_rate))
        self._q: "queue.Queue" = queue.Queue()
        self._closed = False
        self._gate = threading.Lock()        # orders submit's check + put against close's sentinel: nothing queues behind it
        self._worker = threading.Thread(target=self._run, name="vispeech-batching", daemon=True)
        self._worker.start()

    def submit(self, row, noise_seed: int, *, duration_scale=None, pitch_scale=None, energy_scale=None,
               noise_scale=None) -> "concurrent.futures.Future":
        """``row``: one row as ``vispeech_amd.text.collate_rows`` takes it (a ``FilelistRow``).  The four scales are the
        request's own (None: 1.0, and the service's ``noise_scale``); a scale whose control the row carries is not read.
        The future's result is the request's PCM16 samples (numpy int16, valid part only)."""
        fut: "concurrent.futures.Future" = concurrent.futures.Future()
        with self._gate:
            if self._closed:
                raise RuntimeError("the service is closed")
            self._q.put((row, int(noise_seed), fut, (duration_scale, pitch_scale, energy_scale, noise_scale)))
        return fut

    def submit_conversion(self, audio, sid_src: int, sid_tgt: int, noise_seed: int, *,
                          noise_scale=None) -> "concurrent.futures.Future":
        """``audio``: a 1-D float32 recording at the model's rate, spoken by speaker ``sid_src``; the future's result is the
        PCM16 of the recording converted to ``sid_tgt`` (``T(n) * up`` samples at the model's rate, or at ``output_rate``).
        ``noise_scale`` multiplies the posterior's noise (None: 1.0, the reference -- NOT the service's text-to-speech
        ``noise_scale``); ``noise_seed`` keys that noise."""
        fut: "concurrent.futures.Future" = concurrent.futures.Future()
        job = _Conversion(audio, sid_src, sid_tgt, noise_scale)
        with self._gate:
            if self._closed:
                raise RuntimeError("the service is closed")
            self._q.put((job, int(noise_seed), fut, (None,) * 4))
        return fut

    def close(self) -> None:
        """Serve what is queued, then stop the worker and join it."""
        with self._gate:
            if not self._closed:
                self._closed = True
                self._q.put(None)
        self._worker.join()

    def _run(self) -> None:
        stop = False
        while not stop:
            first = self._q.get()
            if first is None:
                break
            reqs, deadline = [first], time.monotonic() + self.max_wait_s
            while len(reqs) < self.max_batch:
                try:
                    nxt = self._q.get(timeout=max(deadline - time.monotonic(), 0.0))
                except queue.Empty:
                    break
                if nxt is None:
                    stop = True
                    break
                reqs.append(nxt)
            reqs = [r for r in reqs if r[2].set_running_or_notify_cancel()]
            if not reqs:
                continue
            try:
                pcms = self._synthesize([r[0] for r in reqs], [r[1] for r in reqs], [r[3] for r in reqs])
                for r, pcm in zip(reqs, pcms):
                    r[2].set_result(pcm)
            except Exception as e:           # this batch's requests fail; the worker lives on
                for r in reqs:
                    if not r[2].done():
                        r[2].set_exception(e)

    def _synthesize(self, rows, seeds, scales=None):
        import torch
        net = self.net
        if any(isinstance(r, _Conversion) for r in rows):
            return self._synthesize_mixed(rows, seeds, scales)
        batch = self._collate(rows)
        t = lambda a: None if a is None else torch.as_tensor(np.asarray(a)).to(net.device)
        ctl = (batch.get("duration"), batch.get("f0"), batch.get("energy"))
        table = _row_table(batch, scales if scales is not None else [(None,) * 4] * len(rows), self.noise_scale)
        kw = {}
        if table is not None:            # (the keyword is passed only when set: a batch without one makes the call it always made)
            ctl, kw = _table_controls(batch, table), {"row_controls": table}
        o, x_mask, *_ = net.infer(t(batch["phonemes"]), t(batch["lengths"]), sid=t(batch["sid"]), noise_scale=self.noise_scale,
                                  duration_control=t(ctl[0]), pitch_control=t(ctl[1]),
                                  energy_control=t(ctl[2]), noise_seed=list(seeds), isolated=True, **kw)
        frames = x_mask.sum(dim=(1, 2)).cpu().tolist()
        hop = net.dims.total_upsample
        if self.output_rate is None:
            return [pcm16(o[b, 0, : int(frames[b]) * hop]) for b in range(len(rows))]
        eng = net._engine
        return [_host_i16(eng.output(o[b:b + 1, 0, : int(frames[b]) * hop], pcm=True)[0]) for b in range(len(rows))]

    def _latents(self, rows, seeds, scales):
        """Per request ``(z row [inter, T], g row, frames)``: the text rows of a mixed batch through ``_text_latents`` (the
        streaming service's admission), its conversions through ``_convert_latents``."""
        eng = self.net._engine
        out = [None] * len(rows)
        text = [i for i, r in enumerate(rows) if not isinstance(r, _Conversion)]
        conv = [i for i, r in enumerate(rows) if isinstance(r, _Conversion)]
        if text:
            lats = _text_latents(eng, self._collate, [rows[i] for i in text], [seeds[i] for i in text],
                                 [scales[i] for i in text], self.noise_scale)
            for i, lat in zip(text, lats):
                out[i] = lat
        for i, lat in zip(conv, _convert_latents(eng, [rows[i] for i in conv], [seeds[i] for i in conv])):
            out[i] = lat
        return out

    def _synthesize_mixed(self, rows, seeds, scales):
        """A batch with conversions: every request's latent, speaker vector and length packed into one ragged batch, ONE
        ``generator_ragged`` call, then the output stage as in ``_synthesize``."""
        import torch
        net, eng = self.net, self.net._engine
        scales = scales if scales is not None else [(None,) * 4] * len(rows)
        lat = self._latents(rows, seeds, scales)
        live = [i for i, (_, _, L) in enumerate(lat) if L > 0]
        pcms = [np.zeros(0, dtype="<i2") for _ in rows]
        if not live:
            return pcms
        T = max(lat[i][2] for i in live)
        z0 = torch.as_tensor(lat[live[0]][0])
        Z = torch.zeros((len(live), z0.shape[0], T), dtype=torch.float32, device=z0.device)
        for b, i in enumerate(live):
            Z[b, :, : lat[i][2]] = torch.as_tensor(lat[i][0])[:, : lat[i][2]]
        G = torch.stack([torch.as_tensor(lat[i][1]).reshape(-1) for i in live])
        o = eng.generator_ragged(Z, G, [lat[i][2] for i in live])
        hop = net.dims.total_upsample
        for b, i in enumerate(live):
            x = o[b:b + 1, 0, : lat[i][2] * hop]
            pcms[i] = pcm16(x) if self.output_rate is None else _host_i16(eng.output(x, pcm=True)[0])
        return pcms


class _RowStream:
    """Iterator over one request's PCM16 chunks of a ``StreamingBatchService``.  ``close()`` abandons the request: its row
    leaves the batch at the next tick."""

    _END = object()

    def __init__(self):
        self._q: "queue.Queue" = queue.Queue()
        self._closed = False
        self._done = False

    def __iter__(self):
        return self

    def __next__(self) -> bytes:
        if self._done or self._closed:
            raise StopIteration
        item = self._q.get()
        if item is self._END:
            self._done = True
            raise StopIteration
        if isinstance(item, BaseException):
            self._done = True
            raise item
        return item

    def close(self) -> None:
        self._closed = True

    @property
    def closed(self) -> bool:
        return self._closed

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class _StreamRequest:
    """One request of a ``StreamingBatchService``: queued (``z`` None), then active at frame ``pos`` of its ``L``."""

    def __init__(self, row, seed: int, scales=(None, None, None, None)):
        self.row, self.seed, self.stream = row, seed, _RowStream()       # (``row``: a collate row, or a ``_Conversion``)
        self.scales = scales          # the request's own (duration, pitch, energy, noise) scales; None: the defaults
        self.z = self.g = None
        self.L = self.pos = 0
        # output stage (``output_rate``): the request's own Engine.output_stream, fed one window per tick
        self.pieces = None
        self.window = None            # the window the feeder hands over next
        self.held = None              # float chunks that complete no output sample yet (merged into the next window)
        self.seen = self.m_next = 0
        self.last = False
        self.history = None           # ``fused_output``: the request's Engine.output_history(), from admission on


class LiveConversion(_RowStream):
    """A live conversion of a ``StreamingBatchService`` (``open_conversion``): the caller feeds the recording while it is
    being made and iterates over the converted PCM16 ``bytes`` -- exact chunks, what the finished recording converted
    alone gives.  ``feed`` and ``end`` may be called from any thread; ``close()`` abandons the session."""

    def __init__(self, cv: "threading.Condition"):
        super().__init__()
        self._cv = cv                 # the service's condition: guards _fed / _ended / _wake, wakes the worker
        self._fed: list = []          # pieces the worker has not taken yet
        self._ended = False
        self._wake = True             # something changed since the worker last looked at this session

    def feed(self, samples) -> None:
        """The next samples of the recording: 1-D float32 at the model's rate, a piece of any size (copied)."""
        a = np.array(samples, dtype=np.float32, copy=True)
        if a.ndim != 1:
            raise ValueError("samples must be a 1-D float32 array at the model's sampling rate")
        with self._cv:
            if self._ended:
                raise RuntimeError("the recording has ended")
            if a.size:
                self._fed.append(a)
                self._wake = True
                self._cv.notify_all()

    def end(self) -> None:
        """The recording is complete: what remains is converted, reflected at its true end, and the iterator ends."""
        with self._cv:
            if not self._ended:
                self._ended = self._wake = True
                self._cv.notify_all()

    def close(self) -> None:
        super().close()
        with self._cv:
            self._wake = True
            self._cv.notify_all()


class _LiveRequest(_StreamRequest):
    """The worker's side of a ``LiveConversion``.  ``n`` samples have reached the device, ``buf`` holds those from ``first``
    on, ``done`` frames are delivered.  For the tick it takes part in, the request is an ordinary row of the vocoder call:
    ``z`` is its window of ``z_hat`` -- frames ``[e0, e0 + L)`` of the recording -- and ``pos`` counts from ``e0``."""

    def __init__(self, stream: LiveConversion, sid_src: int, sid_tgt: int, seed: int, noise_scale: float):
        super().__init__(None, seed)
        self.stream = stream
        self.sid_src, self.sid_tgt, self.noise_scale = int(sid_src), int(sid_tgt), float(noise_scale)
        self.buf = None
        self.first = self.n = self.done = self.e0 = 0
        self.closed = False


class StreamingBatchService:
    """Streaming AND batching (round 11): a set of active requests, each at its own position of its own utterance; every
    tick advances all of them by one chunk in ONE set of generator launches (``Engine.generator_stream_rows``), requests join
    and leave between ticks, and each caller receives PCM16 bytes as its chunk completes.  ``submit`` returns an iterator
    of ``bytes`` (with ``close()``); one worker thread loops over ``step()`` -- one synchronous tick -- and with
    ``autostart=False`` the caller drives ``step()`` itself.  A tick, in order:

    1. admit    queued requests while fewer than ``max_batch`` are active: one isolated ``encode`` / ``frame_lengths_host`` /
                ``decode(max_len=0)`` with the requests' seeds -- and, where a request names a scale or leaves a control to
                the predictors, the group's per-row table -- for the admitted group; each keeps its z row, g row and L.  A
                zero-frame request ends at once with no bytes; a failing admission fails that group's streams only.
    2. generate one ``generator_stream_rows`` call for all active requests, each at its own ``f0`` (a request's first chunk
                has ``first_chunk_frames`` frames if that is given: earlier first audio).
    3. deliver  one device-to-host copy of the int16 block, ``check_numerics(sync=False)``, each request's bytes on its queue.
    4. retire   finished and closed requests.

    A request's audio is what the reference returns for it alone (isolated mode + the halo of the streamed vocoder), whoever
    shares its ticks.  ``output_rate``: each request's float chunk goes through its own ``Engine.output_stream`` (one small
    launch and one copy per request per tick); the bytes are those of the one-shot output stage.  With ``fused_output=True``
    the tick instead makes one ``Engine.generator_stream_rows_output`` call -- the ragged output stage in place of the
    collect launch -- and one device-to-host copy, as the plain path does; a request carries its filter history
    (``Engine.output_history``) from admission on, and the bytes are the same.  ``stats``: ticks, rows per tick and
    admitted groups.  No priorities, no retries, no backpressure.
    ``submit_conversion`` queues a recording to convert to another speaker: admission runs the group's conversions through
    one ``convert_latent`` and keeps each one's ``z_hat`` row, target speaker vector and ``L = T(n)``; from then on it is an
    ordinary row of the tick, next to text rows (a group without a conversion makes the calls it always made).
    ``open_conversion`` opens a LIVE conversion: the recording is fed while it is made (``LiveConversion.feed`` / ``end``).
    A session joins a tick when the samples its next chunk depends on have arrived -- the chunk, the vocoder's halo G and
    the conversion's halo H (``schema.convert_halo_frames``) behind it: an algorithmic delay of
    ``(G + H) * hop + n_fft - pad`` samples, about 1.3 s for the default configuration --; the tick then runs ONE
    ``Engine.convert_stream_rows`` for the ready sessions and hands each one's window of ``z_hat`` to the tick's vocoder call
    as one more row.  A session that is not ready sits the tick out; while only such sessions exist the worker sleeps.  The
    bytes are those of the finished recording converted alone, with the frame-major noise of ``vsp_convert_stream_rows``
    (not the layout ``submit_conversion`` draws).  A session keeps on the device the samples its next window reads and
    those behind them, nothing older.  No backpressure and no reduced-lookahead mode."""

    def __init__(self, net, max_batch: int = 16, chunk_frames: int = 64, first_chunk_frames: Optional[int] = None,
                 noise_scale: float = 0.667, *, table=None, spk2id=None, collate=None, output_rate: Optional[int] = None,
                 sampling_rate: int = 44100, autostart: bool = True, fused_output: bool = False):
        if not 1 <= max_batch <= 64 or chunk_frames < 1:
            raise ValueError("1 <= max_batch <= 64 and chunk_frames >= 1")
        if fused_output and output_rate is None:
            raise ValueError("fused_output needs an output_rate")
        if first_chunk_frames is not None and not 1 <= first_chunk_frames <= chunk_frames:
            raise ValueError("1 <= first_chunk_frames <= chunk_frames")
        if collate is None:
            if table is None or spk2id is None:
                raise ValueError("pass table and spk2id (for collate_rows) or a collate callable")
            from .text import collate_rows
            collate = lambda rows: collate_rows(rows, table, spk2id)
        self._collate = collate
        self.net, self.max_batch, self.chunk_frames = net, int(max_batch), int(chunk_frames)
        self.first_chunk_frames = None if first_chunk_frames is None else int(first_chunk_frames)
        self.noise_scale = float(noise_scale)
        self.output_rate = None if output_rate is None else int(output_rate)
        self.fused_output = bool(fused_output)
        if self.output_rate is not None:
            net._engine.configure_output(self.output_rate, in_rate=int(sampling_rate))
        self.stats = {"ticks": 0, "rows_per_tick": [], "groups": 0}
        self._pending: "collections.deque" = collections.deque()
        self._active: list = []
        self._live: list = []                # open live conversions (_LiveRequest); guarded by _cv
        self._cv = threading.Condition()     # guards _pending / _live / _closed; the worker sleeps on it while there is no work
        self._closed = False
        self._worker = None
        if autostart:
            self._worker = threading.Thread(target=self._run, name="vispeech-stream-batching", daemon=True)
            self._worker.start()

    # ------------------------------------------------------------------ callers' side
    def submit(self, row, noise_seed: int, *, duration_scale=None, pitch_scale=None, energy_scale=None,
               noise_scale=None) -> _RowStream:
        """``row``: one row as ``vispeech_amd.text.collate_rows`` takes it; the four scales are the request's own (None:
        1.0, and the service's ``noise_scale``), as in ``BatchingSynthesisService.submit``.  Returns the iterator of the
        request's PCM16 ``bytes``, one piece per tick the request takes part in."""
        req = _StreamRequest(row, int(noise_seed), (duration_scale, pitch_scale, energy_scale, noise_scale))
        with self._cv:
            if self._closed:
                raise RuntimeError("the service is closed")
            self._pending.append(req)
            self._cv.notify()
        return req.stream

    def submit_conversion(self, audio, sid_src: int, sid_tgt: int, noise_seed: int, *, noise_scale=None) -> _RowStream:
        """``audio``: a 1-D float32 recording at the model's rate, spoken by speaker ``sid_src``.  Returns the iterator of
        the PCM16 ``bytes`` of the recording converted to ``sid_tgt``, one piece per tick; a recording too short for one
        frame ends at once with no bytes.  ``noise_scale`` multiplies the posterior's noise (None: 1.0, the reference --
        NOT the service's text-to-speech ``noise_scale``)."""
        req = _StreamRequest(_Conversion(audio, sid_src, sid_tgt, noise_scale), int(noise_seed))
        with self._cv:
            if self._closed:
                raise RuntimeError("the service is closed")
            self._pending.append(req)
            self._cv.notify()
        return req.stream

    def open_conversion(self, sid_src: int, sid_tgt: int, noise_seed: int, *, noise_scale=None) -> LiveConversion:
        """Opens a live conversion from speaker ``sid_src`` to ``sid_tgt``: ``feed`` the recording to the returned
        ``LiveConversion`` as it arrives, ``end()`` it, and iterate over it for the PCM16 ``bytes``.  ``noise_scale`` as in
        ``submit_conversion`` (None: 1.0); ``noise_seed`` keys the noise, frame-major (``vsp_convert_stream_rows``)."""
        if self.fused_output:
            # the tick hands a live row to the fused output stage at a position counted from its window's first frame: the
            # filter's phase and its history must not see the shift
            eng = self.net._engine
            L, M, H = eng.output_plan
            shift = self.net.dims.total_upsample * L
            if shift % M or 2 * H + M > eng.generator_halo * shift:
                raise ValueError("fused_output cannot carry a live conversion at this output rate (one frame is not a whole "
                                 "number of output samples, or the filter is longer than the vocoder's halo): "
                                 "use fused_output=False")
        stream = LiveConversion(self._cv)
        req = _LiveRequest(stream, sid_src, sid_tgt, int(noise_seed), 1.0 if noise_scale is None else float(noise_scale))
        with self._cv:
            if self._closed:
                raise RuntimeError("the service is closed")
            if len(self._live) + len(self._active) >= self.max_batch:      # (a tick has at most max_batch rows)
                raise Busy(f"{self.max_batch} requests are active")
            self._live.append(req)
        return stream

    def close(self) -> None:
        """Serve what is queued and active, then stop the worker and join it (without a worker: run the ticks here).  Live
        conversions still open are ended: what they were fed is converted."""
        with self._cv:
            self._closed = True
            live = list(self._live)
            self._cv.notify()
        for r in live:
            r.stream.end()
        if self._worker is not None:
            self._worker.join()
        else:
            while self.step():
                pass

    def _run(self) -> None:
        while True:
            with self._cv:
                # (live sessions that wait for samples are no work: feed / end / close set their _wake and notify)
                while not self._pending and not self._active and not self._closed and not any(r.stream._wake for r in self._live):
                    self._cv.wait()
                if self._closed and not self._pending and not self._active and not self._live:
                    return
            self.step()

    # ------------------------------------------------------------------ one tick
    def step(self) -> bool:
        """One tick (admit, generate, deliver, retire).  Returns whether requests are still queued or active."""
        self._admit()
        self._active = [r for r in self._active if not r.stream.closed]      # (closed by its caller: the row leaves here)
        live = self._ready_live()
        if self._active or live:
            try:
                self._generate_and_deliver(self._active + live)
            except Exception as e:             # the tick's requests fail; the service lives on
                for r in self._active + live:
                    r.stream._q.put(e)
                self._active = []
                self._drop_live(live)
                live = []
        for r in self._active:
            if r.pos >= r.L:
                r.stream._q.put(_RowStream._END)
        self._active = [r for r in self._active if r.pos < r.L]
        for r in live:
            self._after_live_tick(r)
        with self._cv:
            return bool(self._pending or self._active or any(r.stream._wake for r in self._live))

    # ------------------------------------------------------------------ live conversions
    def _drop_live(self, reqs) -> None:
        with self._cv:
            self._live = [r for r in self._live if not any(r is x for x in reqs)]

    def _ready_live(self) -> list:
        """Takes what the live sessions were fed, and runs the conversion windows of those whose next chunk is ready: ONE
        ``convert_stream_rows`` call.  Returns them as rows of this tick's vocoder call; a session that must wait, and one
        that fails, is not among them."""
        import torch
        from . import schema
        with self._cv:
            if not self._live:
                return []
            taken = []
            for r in self._live:
                taken.append((r, r.stream._fed, r.stream._ended, r.stream.closed))
                r.stream._fed, r.stream._wake = [], False
        eng, dims = self.net._engine, self.net.dims
        hop, n_fft = dims.hop_length, 2 * (dims.spec_channels - 1)
        G, H = eng.generator_halo, schema.convert_halo_frames(dims)
        device = getattr(eng, "device", "cpu")
        ready, rows, gone = [], [], []
        for r, pieces, ended, closed in taken:
            if closed:                           # abandoned by its caller: the session leaves here
                gone.append(r)
                continue
            if pieces:
                new = torch.as_tensor(np.concatenate(pieces)).to(device)
                r.buf = new if r.buf is None else torch.cat([r.buf, new])
                r.n += int(new.numel())
            r.closed = ended
            n = self.first_chunk_frames if (r.done == 0 and self.first_chunk_frames is not None) else self.chunk_frames
            f1 = r.done + n
            if r.closed:
                T = schema.convert_frames(r.n, n_fft, hop)
                if r.done >= T:                  # (a recording too short for a frame: no bytes)
                    r.stream._q.put(_RowStream._END)
                    gone.append(r)
                    continue
                f1 = min(T, f1)
            e0 = max(0, r.done - G)
            e1 = min(f1 + G, T) if r.closed else f1 + G
            if not schema.convert_window_plan(n_fft, hop, H, r.n, r.closed, e0, e1)[0]:
                continue                         # the samples this chunk depends on have not arrived: sit the tick out
            r.e0, r.L, r.pos = e0, e1 - e0, r.done - e0
            ready.append(r)
            rows.append((r.buf, r.first, r.n, r.closed, e0, e1, r.sid_src, r.sid_tgt, r.seed, r.noise_scale))
        if ready:
            try:
                z, g = eng.convert_stream_rows(rows, self.chunk_frames + 2 * G)
                for b, r in enumerate(ready):
                    r.z, r.g = z[b], g[b]
                    if self.fused_output and r.history is None:
                        r.history = eng.output_history()
            except Exception as e:               # these sessions fail; the tick's other rows and the service live on
                for r in ready:
                    r.stream._q.put(e)
                gone += ready
                ready = []
        if gone:
            self._drop_live(gone)
        return ready

    def _after_live_tick(self, r: "_LiveRequest") -> None:
        """A live session after its tick: the end of the stream, or the samples its next window no longer reads dropped."""
        from . import schema
        dims = self.net.dims
        hop, pad = dims.hop_length, (2 * (dims.spec_channels - 1) - dims.hop_length) // 2
        finished = r.pos >= r.L                  # (the window ended at the recording's last frame, and so did the chunk)
        r.done = r.e0 + r.pos
        r.z = r.g = None
        if finished:
            r.stream._q.put(_RowStream._END)
            self._drop_live([r])
            return
        # the next window starts at frame done - G - H; a reflection at the end, whenever it comes, reaches back pad samples
        w0 = max(0, r.done - self.net._engine.generator_halo - schema.convert_halo_frames(dims))
        keep = max(0, min(w0 * hop - pad, r.n - 1 - pad))
        if keep > r.first:
            r.buf = r.buf[keep - r.first:].clone()
            r.first = keep
        with self._cv:
            r.stream._wake = True                # (it may be ready again at once: the next step looks)

    def _admit(self) -> None:
        group = []
        with self._cv:
            while self._pending and len(self._active) + len(self._live) + len(group) < self.max_batch:
                req = self._pending.popleft()
                if req.stream.closed:
                    req.stream._q.put(_RowStream._END)
                else:
                    group.append(req)
        if not group:
            return
        self.stats["groups"] += 1
        try:
            eng = self.net._engine
            text = [r for r in group if not isinstance(r.row, _Conversion)]
            conv = [r for r in group if isinstance(r.row, _Conversion)]
            lats = []
            if text:
                lats += zip(text, _text_latents(eng, self._collate, [r.row for r in text], [r.seed for r in text],
                                                [r.scales for r in text], self.noise_scale))
            if conv:                         # the group's conversions: their z_hat, target speaker vector and T(n)
                lats += zip(conv, _convert_latents(eng, [r.row for r in conv], [r.seed for r in conv]))
            for r, (z, g, L) in lats:
                r.z, r.g, r.L, r.pos = z, g, L, 0
            for r in group:
                if r.L <= 0:
                    r.stream._q.put(_RowStream._END)          # nothing to synthesise: no bytes
                    continue
                if self.fused_output:
                    r.history = eng.output_history()
                self._active.append(r)
        except Exception as e:                 # this group's requests fail; the active ones and the service live on
            for r in group:
                r.stream._q.put(e)

    def _generate_and_deliver(self, reqs) -> None:
        eng = self.net._engine
        hop = self.net.dims.total_upsample
        rows, counts = [], []
        for r in reqs:
            n = self.first_chunk_frames if (r.pos == 0 and self.first_chunk_frames is not None) else self.chunk_frames
            f1 = min(r.L, r.pos + n)
            rows.append((r.z, r.g, r.L, r.pos, f1))
            counts.append(f1 - r.pos)
        self.stats["ticks"] += 1
        self.stats["rows_per_tick"].append(len(rows))
        if self.fused_output:
            out, done = eng.generator_stream_rows_output([row + (r.history,) for row, r in zip(rows, reqs)],
                                                         self.chunk_frames, pcm=True)
            block = _host_i16_2d(out)                                        # the tick's one device-to-host copy
            self._check_numerics()
            for b, (r, n) in enumerate(zip(reqs, counts)):
                r.pos += n
                if done[b]:
                    r.stream._q.put(block[b, : done[b]].tobytes())
            return
        out = eng.generator_stream_rows(rows, self.chunk_frames, pcm=self.output_rate is None)
        if self.output_rate is None:
            block = _host_i16_2d(out)                                        # the tick's one device-to-host copy
            self._check_numerics()
            for b, (r, n) in enumerate(zip(reqs, counts)):
                r.pos += n
                r.stream._q.put(block[b, : n * hop].tobytes())
            return
        for b, (r, n) in enumerate(zip(reqs, counts)):
            r.pos += n
            piece = self._through_output_stage(r, out[b:b + 1, : n * hop])
            self._check_numerics()
            if piece:
                r.stream._q.put(piece)

    def _through_output_stage(self, r: _StreamRequest, x) -> bytes:
        """The request's float window through its own ``Engine.output_stream``; returns the PCM16 bytes it completes.  The
        stream pulls its windows, a tick pushes one: a window that completes no output sample yet (``complete_outputs``) is
        held back and handed over together with the next one -- consecutive windows of any lengths give the same bytes."""
        import torch
        from . import output_stage
        eng = self.net._engine
        if r.pieces is None:
            def feed():
                while r.window is not None:
                    w, r.window = r.window, None
                    yield w
            r.pieces = eng.output_stream(feed(), None, pcm=True)
        L, M, H = eng.output_plan
        r.held = x if r.held is None else torch.cat([r.held, x], dim=1)
        r.last = r.pos >= r.L
        seen = r.seen + int(r.held.shape[1])
        m_done = output_stage.complete_outputs(seen, L, M, H)
        if not r.last and m_done <= r.m_next:
            return b""
        r.window, r.held, r.seen = r.held, None, seen
        if not r.last:
            r.m_next = m_done
            return _host_i16(next(r.pieces)).tobytes()
        return b"".join(_host_i16(y).tobytes() for y in r.pieces)      # the last window and the filter's tail

    def _check_numerics(self) -> None:
        eng = getattr(self.net, "_engine", None)
        if eng is not None and hasattr(eng, "check_numerics"):
            eng.check_numerics(sync=False)


def _host_i16_2d(y) -> np.ndarray:
    """[B, n] int16 block of the engine -> little-endian int16 [B, n] on the host (one copy)."""
    a = y.detach().cpu().numpy() if hasattr(y, "detach") else np.asarray(y)
    return np.ascontiguousarray(a, dtype="<i2")
