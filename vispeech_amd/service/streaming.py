"""Streaming and batching at once: ``StreamingBatchService``, its callers' iterators (``_RowStream``, ``LiveConversion``)
and the worker's side of a request."""
from __future__ import annotations

import collections
import queue
import threading
from typing import Optional

import numpy as np

from .. import denoiser, input_stage, limiter, loudness, output_stage
from ._pcm import Busy, _check_numerics, _host_i16
from .batching import (_Conversion, _Request, _collate_from, _denoise_spec, _denoise_transform, _input_format, _limiter_spec, _output_format, _row_formats,
                       latents)


class _RowStream:
    """Iterator over one request's PCM16 chunks of a ``StreamingBatchService``.  ``close()`` abandons the request: its row
    leaves the batch at the next tick."""

    _END = object()

    def __init__(self):
        self._q: "queue.Queue" = queue.Queue()
        self._closed = False
        self._done = False
        self.loudness = None          # a request that named ``loudness=``, once finished: integrated, maxima, last gain

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


class _StreamRequest(_Request):
    """One request of a ``StreamingBatchService``: queued (``z`` None), then active at frame ``pos`` of its ``L``."""

    def __init__(self, row, seed: int, scales=(None, None, None, None), out_fmt=None, limiter=None, level=None, denoise=None):
        super().__init__(row, seed, scales, out_fmt, limiter=limiter, denoise=denoise)
        self.den = None               # a request with a denoiser: its ``denoiser.Stream``, from its first tick on
        self.lim = None               # a request with a limiter: its ``limiter.Stream``, from its first tick on
        self.level = level            # ``loudness.spec``: the leveller's five values, {} for a meter only, or None
        self.loud = None              # a request that names a loudness: its ``loudness.Stream``, from its first tick on
        self.stream = _RowStream()
        self.z = self.g = None
        self.L = self.pos = 0
        self.output = None            # ``output_rate``: the request's own ``output_stage.Stream``, one window per tick
        self.history = None           # ``fused_output``: the request's Engine.output_history(), from admission on
        self.row_state = None         # ticks with per-request formats: the request's ``output_stage.RowState``


class LiveConversion(_RowStream):
    """A live conversion of a ``StreamingBatchService`` (``open_conversion``): the caller feeds the recording while it is
    being made and iterates over the converted PCM16 ``bytes`` -- exact chunks, what the finished recording converted
    alone gives.  ``feed`` and ``end`` may be called from any thread; ``close()`` abandons the session."""

    def __init__(self, cv: "threading.Condition", fmt=None):
        super().__init__()
        self._cv = cv                 # the service's condition: guards _fed / _ended / _wake, wakes the worker
        self._fmt = fmt               # (rate, encoding) of what is fed; None: float32 at the model's rate
        self._fed: list = []          # pieces the worker has not taken yet
        self._ended = False
        self._wake = True             # something changed since the worker last looked at this session

    def feed(self, samples) -> None:
        """The next samples of the recording: 1-D float32 at the model's rate, a piece of any size (copied) -- or, for a
        session opened with a ``sample_rate`` / ``encoding``, raw samples in that format (an array of the encoding's dtype or
        ``bytes``)."""
        if self._fmt is None:
            a = np.array(samples, dtype=np.float32, copy=True)
        else:
            a = np.array(input_stage.as_raw(samples, self._fmt[1]), copy=True)
        if a.ndim != 1:
            raise ValueError("samples must be a 1-D array: float32 at the model's sampling rate, or raw samples in the "
                             "session's encoding")
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

    def __init__(self, stream: LiveConversion, sid_src: int, sid_tgt: int, seed: int, noise_scale, out_fmt=None, limiter=None, level=None,
                 denoise=None):
        super().__init__(None, seed, out_fmt=out_fmt, limiter=limiter, level=level, denoise=denoise)
        self.stream = stream
        self.fmt = stream._fmt        # (rate, encoding) of the feed: its pieces go through ``input`` before they reach ``buf``
        self.input = None             # the session's ``input_stage.Stream``, from its first piece on
        self.input_ended = False      # the input stage's tail has been flushed
        self.sid_src, self.sid_tgt = int(sid_src), int(sid_tgt)
        self.noise_scale = 1.0 if noise_scale is None else float(noise_scale)
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
    shares its ticks.  ``output_rate``: each request's float chunk goes through its own ``output_stage.Stream`` (one small
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
    those behind them, nothing older.  No backpressure and no reduced-lookahead mode.
    ``submit`` / ``submit_conversion`` / ``open_conversion`` take ``output_rate=`` / ``output_encoding=``: the request's own
    delivery format (float32, PCM16, G.711 mu-law or A-law at any rate of the output stage).  A tick in which an active
    request names one runs ``generator_stream_rows(pcm=False)`` and then ONE ``Engine.output_rows`` call over all its rows,
    each with its request's rate, encoding and ``output_stage.RowState``, and one device-to-host copy; a request that ends
    gets its filter's tail in the same call; requests that name nothing ride at (the service's rate, PCM16) and get the
    bytes of their own path.  A tick without such a request is the tick described above.  ``fused_output=True`` refuses
    a request's own format (``ValueError``).
    They also take ``limiter=`` (True or a mapping of attack_ms, hold_ms, ceiling, gain_db): a fixed gain held under a
    ceiling by the look-ahead limiter, the level control a stream can have.  A tick in which an
    active request has one runs on the same ``output_rows`` path, with ONE ``limiter.push_rows`` call for those rows between
    the generator and ``output_rows``; the request's last chunk flushes its limiter.  Its bytes are those of
    ``SynthesizerTrn.limit`` on its whole waveform, then the output stage; its delay grows by attack + 12 samples.
    ``fused_output=True`` refuses the keyword as well.
    And ``loudness=`` (round 23): a number -- the target in LUFS of the causal leveller, which follows
    the stream's running integrated loudness with no look-ahead and no delay --, a mapping of (target_lufs, max_gain_db,
    max_cut_db, slew_db_per_s, initial_gain_db), or True: a meter only.  Such a tick runs on the ``output_rows`` path too,
    with ONE ``loudness.push_rows`` call for those rows between the generator and the limiter / ``output_rows``; the request's
    samples are those of ``SynthesizerTrn.level`` on its whole waveform (then ``limit``, then the output stage).  When the
    request has finished, its stream carries ``.loudness``: ``dict(integrated, momentary_max, short_term_max, gain_db)``.
    ``fused_output=True`` refuses the keyword; a request that names nothing gets the bytes it always got.
    ``loudness_gate="histogram"`` (round 24; "exact" is the default) gives those streams the histogram
    gate: their running level costs the same at every tick, however long a request lasts -- what ``open_conversion`` needs
    --, stays within 0.05 LU of the exact one, and ``.loudness`` gains ``range_lu``, the loudness range.
    ``denoise=`` (round 26), on the service for every request or on ``submit`` / ``submit_conversion`` /
    ``open_conversion`` for one (None there: the service's; False: none): a strength, or True for 0.01 -- the denoiser of
    ``SynthesizerTrn.denoise`` with the speaker's own bias (a conversion's: ``sid_tgt``), on the generator's chunks as they
    come.  Such a tick runs on the ``output_rows`` path with ONE ``denoiser.push_rows`` call for those rows, in front of the
    loudness call and the limiter -- the order of ``BatchingSynthesisService`` --; the request's last chunk flushes its
    denoiser, and the stages behind are handed the positions of the denoiser's output.  Its samples are those of
    ``SynthesizerTrn.denoise`` on its whole waveform; its delay grows by ``n_fft - hop`` to ``n_fft - 1`` samples, and a tick
    in which its denoiser completes no sample delivers nothing for it.  ``fused_output=True`` refuses the keyword; a
    request that names nothing gets the bytes it always got, and a service in which nobody does makes the calls it always
    made.  ``denoise_transform="fft"`` (round 27): the requests' streams, their biases and so the one
    ``push_rows`` call per tick run on the in-LDS FFT; a service that names none makes the calls it always made."""

    def __init__(self, net, max_batch: int = 16, chunk_frames: int = 64, first_chunk_frames: Optional[int] = None,
                 noise_scale: float = 0.667, *, table=None, spk2id=None, collate=None, output_rate: Optional[int] = None,
                 sampling_rate: int = 44100, autostart: bool = True, fused_output: bool = False, loudness_gate: str = "exact",
                 denoise=None, denoise_transform=None):
        if not 1 <= max_batch <= 64 or chunk_frames < 1:
            raise ValueError("1 <= max_batch <= 64 and chunk_frames >= 1")
        self.denoise = _denoise_spec(denoise)
        self.denoise_transform = _denoise_transform(denoise_transform)
        if self.denoise is not None and fused_output:
            raise ValueError("fused_output delivers every row through its one launch: a denoiser needs fused_output=False")
        if loudness_gate not in loudness.GATES:
            raise ValueError(f"loudness_gate is one of {loudness.GATES}, not {loudness_gate!r}")
        self.loudness_gate = loudness_gate
        if fused_output and output_rate is None:
            raise ValueError("fused_output needs an output_rate")
        if first_chunk_frames is not None and not 1 <= first_chunk_frames <= chunk_frames:
            raise ValueError("1 <= first_chunk_frames <= chunk_frames")
        self._collate = _collate_from(table, spk2id, collate)
        self.net, self.max_batch, self.chunk_frames = net, int(max_batch), int(chunk_frames)
        self.first_chunk_frames = None if first_chunk_frames is None else int(first_chunk_frames)
        self.noise_scale = float(noise_scale)
        self.output_rate = None if output_rate is None else int(output_rate)
        self.fused_output = bool(fused_output)
        self.sampling_rate = int(sampling_rate)
        if self.output_rate is not None:
            net._engine.configure_output(self.output_rate, in_rate=int(sampling_rate))
        self.stats = {"ticks": 0, "rows_per_tick": [], "groups": 0}
        self._pending: "collections.deque" = collections.deque()
        self._active: list = []
        self._live: list = []                # open live conversions (_LiveRequest); guarded by _cv
        self._geometry = None                # (hop, n_fft, pad, G, H) of live conversions, from the first open_conversion on
        self._cv = threading.Condition()     # guards _pending / _live / _closed; the worker sleeps on it while there is no work
        self._closed = False
        self._worker = None
        if autostart:
            self._worker = threading.Thread(target=self._run, name="vispeech-stream-batching", daemon=True)
            self._worker.start()

    # ------------------------------------------------------------------ callers' side
    def _out_fmt(self, output_rate, output_encoding):
        fmt = _output_format(output_rate, output_encoding)
        if fmt is not None and self.fused_output:
            raise ValueError("fused_output delivers every row at the service's rate as PCM16: a request's own output_rate / "
                             "output_encoding needs fused_output=False")
        return fmt

    def _limiter(self, limiter):
        """A request's ``limiter=``: ``(attack, hold, ceiling, gain)`` or None (``batching._limiter_spec``)."""
        if limiter is None or limiter is False:
            return None
        if self.fused_output:
            raise ValueError("fused_output delivers every row through its one launch: a request's limiter needs fused_output=False")
        return _limiter_spec(limiter, None, self.sampling_rate)

    def _loudness(self, value):
        """A request's ``loudness=``: ``loudness.spec`` -- the leveller's values, {} for a meter -- or None."""
        if value is None or value is False:
            return None
        if self.fused_output:
            raise ValueError("fused_output delivers every row through its one launch: a request's loudness needs fused_output=False")
        return loudness.spec(value)

    def _denoise(self, value):
        """A request's ``denoise=``: its strength (``batching._denoise_spec``), the service's for None, or None."""
        strength = self.denoise if value is None else _denoise_spec(value)
        if strength is not None and self.fused_output:
            raise ValueError("fused_output delivers every row through its one launch: a request's denoiser needs fused_output=False")
        return strength

    def submit(self, row, noise_seed: int, *, duration_scale=None, pitch_scale=None, energy_scale=None,
               noise_scale=None, output_rate: Optional[int] = None, output_encoding=None, limiter=None, loudness=None,
               denoise=None) -> _RowStream:
        """``row``: one row as ``vispeech_amd.text.collate_rows`` takes it; the four scales are the request's own (None:
        1.0, and the service's ``noise_scale``), as in ``BatchingSynthesisService.submit``.  Returns the iterator of the
        request's PCM16 ``bytes``, one piece per tick the request takes part in.
        ``output_rate`` / ``output_encoding`` ("f32", "s16", "ulaw", "alaw"): the request's own delivery format; its
        ``bytes`` are then little-endian elements of that encoding at that rate (see the class text).
        ``limiter``: the look-ahead limiter in front of the request's output stage -- True or a
        mapping of (attack_ms, hold_ms, ceiling, gain_db): the level control a stream can have, a fixed gain held under a
        ceiling.  The request's bytes are those of ``SynthesizerTrn.limit`` on its whole waveform, then the output stage;
        its delay grows by attack + 12 samples.  A tick in which a request has one runs as a tick in which a request names
        a format does, with ONE ``limiter.push_rows`` call for those rows between the generator and ``output_rows``.
        ``loudness``: the leveller's target (LUFS), a mapping of its five values, or True for a meter only (see the class
        text); it runs in front of the limiter.
        ``denoise``: the strength of the denoiser on the request's waveform, or True for 0.01; None: the service's; False:
        none (see the class text); it runs in front of both."""
        return self._enqueue(_StreamRequest(row, noise_seed, (duration_scale, pitch_scale, energy_scale, noise_scale),
                                            self._out_fmt(output_rate, output_encoding), self._limiter(limiter), self._loudness(loudness),
                                            self._denoise(denoise)))

    def submit_conversion(self, audio, sid_src: int, sid_tgt: int, noise_seed: int, *, noise_scale=None,
                          sample_rate: Optional[int] = None, encoding=None, output_rate: Optional[int] = None,
                          output_encoding=None, limiter=None, loudness=None, denoise=None) -> _RowStream:
        """``audio``: a 1-D float32 recording at the model's rate, spoken by speaker ``sid_src``.  Returns the iterator of
        the PCM16 ``bytes`` of the recording converted to ``sid_tgt``, one piece per tick; a recording too short for one
        frame ends at once with no bytes.  ``noise_scale`` multiplies the posterior's noise (None: 1.0, the reference --
        NOT the service's text-to-speech ``noise_scale``).  ``sample_rate`` / ``encoding``: ``audio`` is raw samples in that
        format (an array of the encoding's dtype or ``bytes``); admission runs the group's raw recordings through the
        input stage, one call per distinct (rate, encoding), before its one ``convert_latent``.  ``output_rate`` /
        ``output_encoding`` / ``limiter`` / ``loudness``: as in ``submit``; ``denoise``: as in ``submit``, with the bias of
        ``sid_tgt``."""
        fmt = _input_format(sample_rate, encoding, self.sampling_rate)
        return self._enqueue(_StreamRequest(_Conversion(audio, sid_src, sid_tgt, noise_scale, fmt), noise_seed,
                                            out_fmt=self._out_fmt(output_rate, output_encoding), limiter=self._limiter(limiter),
                                            level=self._loudness(loudness), denoise=self._denoise(denoise)))

    def open_conversion(self, sid_src: int, sid_tgt: int, noise_seed: int, *, noise_scale=None,
                        sample_rate: Optional[int] = None, encoding=None, output_rate: Optional[int] = None,
                        output_encoding=None, limiter=None, loudness=None, denoise=None) -> LiveConversion:
        """Opens a live conversion from speaker ``sid_src`` to ``sid_tgt``: ``feed`` the recording to the returned
        ``LiveConversion`` as it arrives, ``end()`` it, and iterate over it for the PCM16 ``bytes``.  ``noise_scale`` as in
        ``submit_conversion`` (None: 1.0); ``noise_seed`` keys the noise, frame-major (``vsp_convert_stream_rows``).
        ``sample_rate`` / ``encoding``: ``feed`` takes raw pieces in that format; every tick the worker resamples what
        arrived -- one ``Engine.input_rows`` call per distinct (rate, encoding) among the sessions with new audio -- and
        appends the model-rate samples that are complete to the session's buffer; ``end()`` flushes the filter's tail.
        Readiness is decided on those samples, so the session's delay grows by the filter's half length: ``zeros`` = 32
        input periods (2 ms at 16 kHz).  ``output_rate`` / ``output_encoding``: as in ``submit``; on that path a frame
        need not be a whole number of output samples.  ``limiter`` / ``loudness``: as in ``submit`` -- the leveller is what
        keeps a call that lasts minutes, whose talker moves about the microphone, at its level.  ``denoise``: as in
        ``submit_conversion`` -- a call that lasts minutes is where the vocoder's steady buzz is heard longest."""
        out_fmt = self._out_fmt(output_rate, output_encoding)
        limiter = self._limiter(limiter)
        level = self._loudness(loudness)
        denoise = self._denoise(denoise)
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
        if self._geometry is None:
            # (not in the constructor: a net that serves text only need not have the front end's dimensions)
            from .. import schema
            dims = self.net.dims
            hop, n_fft = dims.hop_length, 2 * (dims.spec_channels - 1)
            self._geometry = (hop, n_fft, (n_fft - hop) // 2, self.net._engine.generator_halo, schema.convert_halo_frames(dims))
        fmt = _input_format(sample_rate, encoding, self.sampling_rate)
        if fmt is not None and fmt[0] not in self.net._engine.input_rates:
            self.net._engine.configure_input(fmt[0], model_rate=self.sampling_rate)      # (allocates: here, not in a tick)
        return self._enqueue(_LiveRequest(LiveConversion(self._cv, fmt), sid_src, sid_tgt, noise_seed, noise_scale, out_fmt, limiter, level,
                                          denoise))

    def _enqueue(self, req: _StreamRequest) -> _RowStream:
        """A text request or a conversion joins the queue, a live session the open sessions; the worker is woken."""
        with self._cv:
            if self._closed:
                raise RuntimeError("the service is closed")
            if isinstance(req, _LiveRequest):
                if len(self._live) + len(self._active) >= self.max_batch:      # (a tick has at most max_batch rows)
                    raise Busy(f"{self.max_batch} requests are active")
                self._live.append(req)
            else:
                self._pending.append(req)
            self._cv.notify()
        return req.stream

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

    def _chunk_len(self, first: bool) -> int:
        """Frames of a request's next chunk: ``first_chunk_frames`` for its first one, where that is given."""
        return self.first_chunk_frames if first and self.first_chunk_frames is not None else self.chunk_frames

    # ------------------------------------------------------------------ live conversions
    def _drop_live(self, reqs) -> None:
        with self._cv:
            self._live = [r for r in self._live if not any(r is x for x in reqs)]

    def _ready_live(self) -> list:
        """Takes what the live sessions were fed, and runs the conversion windows of those whose next chunk is ready: ONE
        ``convert_stream_rows`` call.  Returns them as rows of this tick's vocoder call; a session that must wait, and one
        that fails, is not among them."""
        import torch
        from .. import schema
        with self._cv:
            if not self._live:
                return []
            taken = []
            for r in self._live:
                taken.append((r, r.stream._fed, r.stream._ended, r.stream.closed))
                r.stream._fed, r.stream._wake = [], False
        eng = self.net._engine
        hop, n_fft, _, G, H = self._geometry
        device = getattr(eng, "device", "cpu")
        ready, rows, gone = [], [], []
        failed = self._live_input(taken, device)
        for r, pieces, ended, closed in taken:
            if closed or any(r is x for x in failed):   # abandoned by its caller, or its input stage failed: it leaves here
                gone.append(r)
                continue
            if pieces:
                new = torch.as_tensor(np.concatenate(pieces)).to(device) if r.fmt is None else torch.cat(pieces)
                r.buf = new if r.buf is None else torch.cat([r.buf, new])
                r.n += int(new.numel())
            r.closed = ended
            f1 = r.done + self._chunk_len(r.done == 0)
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

    def _live_input(self, taken, device) -> list:
        """The raw pieces of this tick's sessions through the input stage: ONE ``Engine.input_rows`` call per distinct
        (rate, encoding) among the sessions with new audio or a tail to flush.  Replaces each such session's pieces in
        ``taken`` by the model-rate samples they complete (device tensors); returns the sessions whose call failed."""
        import torch
        eng = self.net._engine
        jobs = {}                                # (rate, encoding) -> [(index into taken, row)]
        for i, (r, pieces, ended, closed) in enumerate(taken):
            if r.fmt is None or closed:
                continue
            taken[i] = (r, [], ended, closed)
            if r.input is None:
                r.input = input_stage.Stream(eng, *r.fmt)
            rows = []
            if pieces:
                rows.append(r.input.take(torch.as_tensor(np.concatenate(pieces)).to(device)))
            if ended and not r.input_ended:      # the recording has ended: the filter's tail, before the session is closed
                r.input_ended = True
                rows.append(r.input.take_tail())
            for row in rows:
                if row is not None:              # (a piece too short to complete an output sample gives none)
                    jobs.setdefault(r.fmt, []).append((i, row))
        failed = []
        for (rate, enc), job in sorted(jobs.items()):
            try:
                for (i, _), y in zip(job, eng.input_rows([row for _, row in job], rate, enc)):
                    taken[i][1].append(y)
            except Exception as e:               # these sessions fail; the others and the service live on
                for r in {id(taken[i][0]): taken[i][0] for i, _ in job}.values():
                    r.stream._q.put(e)
                    failed.append(r)
        return failed

    def _after_live_tick(self, r: "_LiveRequest") -> None:
        """A live session after its tick: the end of the stream, or the samples its next window no longer reads dropped."""
        hop, _, pad, G, H = self._geometry
        finished = r.pos >= r.L                  # (the window ended at the recording's last frame, and so did the chunk)
        r.done = r.e0 + r.pos
        r.z = r.g = None
        if finished:
            r.stream._q.put(_RowStream._END)
            self._drop_live([r])
            return
        # the next window starts at frame done - G - H; a reflection at the end, whenever it comes, reaches back pad samples
        w0 = max(0, r.done - G - H)
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
            for r, (z, g, L) in zip(group, latents(eng, self._collate, group, self.noise_scale, self.sampling_rate)):
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
            f1 = min(r.L, r.pos + self._chunk_len(r.pos == 0))
            rows.append((r.z, r.g, r.L, r.pos, f1))
            counts.append(f1 - r.pos)
        self.stats["ticks"] += 1
        self.stats["rows_per_tick"].append(len(rows))
        if any(r.out_fmt is not None or r.limiter is not None or r.level is not None or r.denoise is not None for r in reqs):
            return self._deliver_rows(reqs, rows, counts)
        for r in reqs:
            if r.row_state is not None:        # it shared earlier ticks with requests that name a format
                self._leave_rows_path(r)
        if self.fused_output:
            out, done = eng.generator_stream_rows_output([row + (r.history,) for row, r in zip(rows, reqs)],
                                                         self.chunk_frames, pcm=True)
        else:
            out = eng.generator_stream_rows(rows, self.chunk_frames, pcm=self.output_rate is None)
            done = [n * hop for n in counts]
        if self.output_rate is not None and not self.fused_output:
            for b, (r, n) in enumerate(zip(reqs, counts)):     # each float chunk through its request's own output stage
                r.pos += n
                piece = self._through_output_stage(r, out[b:b + 1, : done[b]])
                _check_numerics(self.net)
                if piece:
                    r.stream._q.put(piece)
            return
        block = _host_i16(out, flat=False)                                   # the tick's one device-to-host copy
        _check_numerics(self.net)
        for b, (r, n) in enumerate(zip(reqs, counts)):
            r.pos += n
            if done[b]:                        # (a fused tick may complete no output sample of a request)
                r.stream._q.put(block[b, : done[b]].tobytes())

    def _deliver_rows(self, reqs, rows, counts) -> None:
        """A tick in which a request names its own format: the float chunks of ``generator_stream_rows`` as rows of ONE
        ``Engine.output_rows`` call -- each with its request's rate, encoding and ``RowState``; a request that names nothing
        rides at (the service's rate, PCM16), the bytes of its own path -- then one device-to-host copy.  A request's last
        chunk carries ``ended``: its tail comes in the same call."""
        from ._pcm import _host
        eng = self.net._engine
        hop = self.net.dims.total_upsample
        base = self.sampling_rate if self.output_rate is None else self.output_rate
        fmts = _row_formats(eng, reqs, base, self.sampling_rate)
        out = eng.generator_stream_rows(rows, self.chunk_frames, pcm=False)
        pieces = [out[b, : n * hop] for b, n in enumerate(counts)]
        first = [(getattr(r, "e0", 0) + r.pos) * hop for r in reqs]
        last = [r.pos + n >= r.L for r, n in zip(reqs, counts)]
        denoised = [b for b, r in enumerate(reqs) if r.denoise is not None]
        if denoised:                                                    # in front of everything: the one-shot service's order
            for b in denoised:
                r = reqs[b]
                if r.den is None:
                    sid = r.sid_tgt if isinstance(r, _LiveRequest) else r.row.sid_tgt if r.is_conversion else r.sid
                    if self.denoise_transform == "dft":
                        r.den = denoiser.Stream(eng, self.net.denoiser_bias([sid])[0], r.denoise)
                    else:
                        r.den = denoiser.Stream(eng, self.net.denoiser_bias([sid], self.denoise_transform)[0], r.denoise,
                                                transform=self.denoise_transform)
                first[b] = r.den.out_next                               # the stages behind see the denoiser's samples
            for b, y in zip(denoised, denoiser.push_rows(eng, [(reqs[b].den, pieces[b], last[b]) for b in denoised])):
                pieces[b] = y
        named = [b for b, r in enumerate(reqs) if r.level is not None]
        if named:                                                       # the leveller (or meter): no delay, so `first` stands
            for b in named:
                if reqs[b].loud is None:
                    reqs[b].loud = loudness.Stream(eng, self.sampling_rate, level=reqs[b].level or True, gate=self.loudness_gate)
            for b, y in zip(named, loudness.push_rows(eng, [(reqs[b].loud, pieces[b], last[b]) for b in named])):
                pieces[b] = y
                if last[b]:
                    st = reqs[b].loud
                    reqs[b].stream.loudness = dict(integrated=st.integrated, momentary_max=st.momentary_max,
                                                   short_term_max=st.short_term_max, gain_db=st.gain_db)
                    if st.loudness_range is not None:
                        reqs[b].stream.loudness["range_lu"] = st.loudness_range
        limited = [b for b, r in enumerate(reqs) if r.limiter is not None]
        for b in limited:
            r = reqs[b]
            if r.lim is None:
                r.lim = limiter.Stream(eng, r.limiter[2], gain=r.limiter[3], attack=r.limiter[0], hold=r.limiter[1])
            first[b] = r.lim.out_next                                   # the output stage sees the limiter's samples
        for window in sorted({reqs[b].limiter[:2] for b in limited}):   # (one call: a tick's limiters share attack and hold as a rule)
            group = [b for b in limited if reqs[b].limiter[:2] == window]
            done = limiter.push_rows(eng, [(reqs[b].lim, pieces[b], last[b]) for b in group])
            for b, y in zip(group, done):
                pieces[b] = y
        job, rode = [], []
        for b, (r, n, (rate, enc)) in enumerate(zip(reqs, counts, fmts)):
            if r.row_state is None:
                self._enter_rows_path(r, rate, first[b])
            r.pos += n
            if pieces[b].shape[0] or r.pos >= r.L:                      # (a limiter's first short chunk may complete no sample)
                job.append((pieces[b], r.pos >= r.L, rate, enc, r.row_state))
                rode.append(b)
        buf, spans = eng.output_rows(job)
        host = _host(buf)                                               # the tick's one device-to-host copy
        _check_numerics(self.net)
        for b, (off, cnt) in zip(rode, spans):
            r, enc = reqs[b], fmts[b][1]
            if cnt:                            # (a short chunk at a low rate may complete no output sample)
                r.stream._q.put(host[off:off + cnt * output_stage.element_size(enc)].tobytes())

    def _enter_rows_path(self, r: _StreamRequest, rate: int, x_first: int) -> None:
        """The request's ``RowState`` at input sample ``x_first``; a request that came along on the service's own path
        brings the samples its ``output_stage.Stream`` kept -- they start at the k0 of its next call."""
        r.row_state = output_stage.RowState(self.net._engine, rate)
        r.row_state.x_first = int(x_first)
        s, r.output = r.output, None
        if s is not None and s.hist is not None and s.hist.shape[1]:
            r.row_state.buf[r.row_state.side][: s.hist.shape[1]] = s.hist[0]

    def _leave_rows_path(self, r: _StreamRequest) -> None:
        """Back to the service's own path (no request of the tick names a format): the ``output_stage.Stream`` of a service
        with an ``output_rate`` continues from what the request's ``RowState`` holds."""
        st, r.row_state = r.row_state, None
        if self.output_rate is None or self.fused_output:
            return
        s = output_stage.Stream(self.net._engine, None, pcm=True)
        L, M, H = s.plan
        s.seen = st.x_first
        s.m_next = output_stage.complete_outputs(s.seen, L, M, H)
        s.first = min(s.seen, output_stage.history_start(s.m_next, L, M, H))
        s.hist = st.buf[st.side][: s.seen - s.first].reshape(1, -1)
        r.output = s

    def _through_output_stage(self, r: _StreamRequest, x) -> bytes:
        """The request's float window through its own ``output_stage.Stream``; returns the PCM16 bytes it completes (none
        for a window too short to complete an output sample), with the filter's tail behind the request's last window."""
        if r.output is None:
            r.output = output_stage.Stream(self.net._engine, None, pcm=True)
        done = [r.output.push(x)] + ([r.output.finish()] if r.pos >= r.L else [])
        return b"".join(_host_i16(y).tobytes() for y in done if y is not None)
