"""Requests from many callers in one batch: the request the batching services queue, the one way from a group of requests
to their latents, and ``BatchingSynthesisService``."""
from __future__ import annotations

import concurrent.futures
import math
import queue
import threading
import time
from typing import Optional

import numpy as np

from ._pcm import _row_pcm16


def _input_format(sample_rate, encoding, model_rate: int):
    """``(rate, VSP_IN_*)`` of a request that names a sample rate or an encoding, None of one that names neither (its audio
    is float32 at the model's rate and takes the path it always took)."""
    if sample_rate is None and encoding is None:
        return None
    from .. import input_stage
    return (int(model_rate if sample_rate is None else sample_rate), input_stage.encoding(encoding))


def _output_format(output_rate, output_encoding):
    """``(rate or None, VSP_OUT_*)`` of a request that names an output rate or encoding (None: the service's rate; PCM16),
    None of one that names neither -- its bytes are the ones it always got."""
    if output_rate is None and output_encoding is None:
        return None
    from .. import output_stage
    if output_rate is not None and int(output_rate) <= 0:
        raise ValueError("output_rate must be positive")
    return (None if output_rate is None else int(output_rate), output_stage.encoding(output_encoding))


def _loudness_spec(loudness):
    """``(target_lufs, peak_ceiling, max_gain_db)`` of a request or service that names a loudness -- a target in LUFS, or a
    mapping of the three (``peak_ceiling`` 1.0 and ``max_gain_db`` 30.0 where it leaves them out) --, None of one that names
    none (None or False).  Refused here, not in the worker."""
    if loudness is None or loudness is False:
        return None
    vals = {"target_lufs": None, "peak_ceiling": 1.0, "max_gain_db": 30.0}
    if hasattr(loudness, "keys"):
        unknown = set(loudness) - set(vals)
        if unknown:
            raise ValueError(f"loudness: unknown {sorted(unknown)}; the fields are {list(vals)}")
        vals.update(loudness)
    else:
        vals["target_lufs"] = loudness
    if vals["target_lufs"] is None or isinstance(vals["target_lufs"], bool):
        raise ValueError("loudness: a target in LUFS, or a mapping with target_lufs")
    t, c, m = float(vals["target_lufs"]), float(vals["peak_ceiling"]), float(vals["max_gain_db"])
    if not (t == t and abs(t) != float("inf")):
        raise ValueError("loudness: target_lufs must be finite")
    if not c > 0.0:
        raise ValueError("loudness: peak_ceiling must be above 0")
    if not m >= 0.0:
        raise ValueError("loudness: max_gain_db must be at least 0")
    return (t, c, m)


def _denoise_transform(value) -> str:
    """A service's ``denoise_transform=``: None or ``"dft"`` -- the calls the service always made -- or ``"fft"`` (DESIGN.md
    section 4v)."""
    if value is None:
        return "dft"
    if value not in ("dft", "fft"):
        raise ValueError(f"denoise_transform is 'dft' or 'fft', not {value!r}")
    return value


def _denoise_spec(value):
    """The strength of a request or service that names a denoiser (``SynthesizerTrn.denoise``): a
    finite number >= 0, ``True`` for 0.01; None / False: none."""
    if value is None or value is False:
        return None
    if value is True:
        return 0.01
    if isinstance(value, (int, float, np.integer, np.floating)) and math.isfinite(float(value)) and float(value) >= 0.0:
        return float(value)
    raise ValueError("denoise: a strength (a finite number, at least 0), or True for 0.01")


def _limiter_spec(value, loudness, fs: int):
    """``(attack, hold, ceiling, gain)`` -- samples, samples, linear, linear -- of a request or service that names a limiter
    (``vispeech_amd.limiter.spec``): ``True`` or a mapping of ``attack_ms``, ``hold_ms``, ``ceiling`` and ``gain_db``.  The
    ceiling it does not name is its loudness's ``peak_ceiling`` (``loudness``: a ``_loudness_spec``), or 1."""
    from .. import limiter
    return limiter.spec(value, fs, default_ceiling=1.0 if loudness is None else loudness[1])


def level_rows(eng, reqs, waves, n, fs: int) -> None:
    """The level control of a batch in which a request names a limiter, on ``waves`` [B, L] in place (row b's first
    ``n[b]`` samples).  A request with a loudness and no limiter: the peak-cut normalisation it always got
    (``Engine.loudness_normalize``).  A request with a limiter: its gain -- the loudness gain NOT cut by the peak, or its
    ``gain_db`` -- and ONE limiter call for all of them (one per distinct attack and hold), the gains staying on the
    device.  Everybody else is neither read nor written."""
    from ..engine import Engine
    nan = float("nan")
    B = len(reqs)
    n_host = [max(int(v), 1) for v in n]
    live = [n[b] >= 1 for b in range(B)]
    plain = [live[b] and r.loudness is not None and r.limiter is None for b, r in enumerate(reqs)]
    if any(plain):
        spec = [r.loudness if plain[b] else (nan, 1.0, 0.0) for b, r in enumerate(reqs)]
        eng.loudness_normalize(waves, n_host, fs, Engine.loudness_params(B, *zip(*spec)))
    for A, H in sorted({r.limiter[:2] for b, r in enumerate(reqs) if live[b] and r.limiter is not None}):
        rows = [live[b] and r.limiter is not None and r.limiter[:2] == (A, H) for b, r in enumerate(reqs)]
        ceilings = [r.limiter[2] if rows[b] else nan for b, r in enumerate(reqs)]
        static = [r.limiter[3] if rows[b] and r.loudness is None else 1.0 for b, r in enumerate(reqs)]
        if any(rows[b] and r.loudness is not None for b, r in enumerate(reqs)):
            spec = [r.loudness if rows[b] and r.loudness is not None else (nan, 1.0, 0.0) for b, r in enumerate(reqs)]
            eng.loudness_limit(waves, n_host, fs, Engine.loudness_params(B, *zip(*spec)), attack=A, hold=H, ceilings=ceilings,
                               static_gains=None if all(g == 1.0 for g in static) else static)
        else:
            eng.limit(waves, n_host, ceilings, gains=static, attack=A, hold=H)


def _row_formats(eng, reqs, base_rate: int, model_rate: int):
    """Per request the ``(rate, VSP_OUT_*)`` of its row in an ``Engine.output_rows`` call: its own format, or -- for a
    request that names none -- (the service's rate, PCM16), the bytes it gets on the service's own path.  Rates the engine's
    set does not hold yet are configured here (allocates: configure them ahead where that matters)."""
    from .. import output_stage
    fmts = [(base_rate, output_stage.S16) if r.out_fmt is None else (base_rate if r.out_fmt[0] is None else r.out_fmt[0], r.out_fmt[1])
            for r in reqs]
    for rate in sorted({f[0] for f in fmts}):
        if rate not in eng.output_rates:
            eng.configure_output_rate(rate, in_rate=model_rate)
    return fmts


class _Conversion:
    """A conversion request of the batching services (``submit_conversion``): a recording at the model's rate, the speaker
    it was spoken by and the speaker to convert it to.  To the vocoder it is a row like any other -- a latent, a speaker
    vector and a length -- so it shares generator calls and ticks with text requests.  ``fmt`` = ``(rate, encoding)``: the
    recording is ``raw`` in that format (``audio`` None) until admission has run it through the input stage."""

    def __init__(self, audio, sid_src: int, sid_tgt: int, noise_scale, fmt=None):
        self.fmt, self.raw = fmt, None
        if fmt is None:
            a = np.ascontiguousarray(np.asarray(audio, dtype=np.float32))
        else:
            from .. import input_stage
            a, self.raw = None, input_stage.as_raw(audio, fmt[1])
        if (self.raw if a is None else a).ndim != 1:
            raise ValueError("audio must be a 1-D array: float32 at the model's sampling rate, or raw samples in the "
                             "encoding the request names")
        self.audio, self.sid_src, self.sid_tgt = a, int(sid_src), int(sid_tgt)
        self.noise_scale = 1.0 if noise_scale is None else float(noise_scale)      # (1.0: the reference's posterior)


class _Recording:
    """The recording a text request takes its melody and loudness from (``submit(prosody_audio=...)``): float32 at the
    model's rate in ``audio``, or -- ``fmt`` = ``(rate, encoding)`` -- ``raw`` until the worker has run it through the input
    stage (the attributes ``_through_input_stage`` reads and writes)."""

    def __init__(self, audio, fmt=None, sid=None):
        self.fmt, self.raw = fmt, None
        self.sid = None if sid is None else int(sid)      # who speaks the recording (alignment only); None: the row's speaker
        if fmt is None:
            a = np.ascontiguousarray(np.asarray(audio, dtype=np.float32))
        else:
            from .. import input_stage
            a, self.raw = None, input_stage.as_raw(audio, fmt[1])
        if (self.raw if a is None else a).ndim != 1:
            raise ValueError("prosody_audio must be a 1-D array: float32 at the model's sampling rate, or raw samples in the "
                             "encoding the request names")
        self.audio = a

    def samples(self, model_rate: int) -> int:
        """Samples at the model's rate, host arithmetic."""
        if self.fmt is None:
            return int(self.audio.size)
        from .. import input_stage
        L, M, _ = input_stage.plan(self.fmt[0], model_rate)
        return input_stage.out_len(int(self.raw.size), L, M)


class _Request:
    """One request of the batching services: ``row`` is a row as ``collate_rows`` takes it or a ``_Conversion``, ``seed``
    keys its noise, ``scales`` are its own (duration, pitch, energy, noise) scales -- None: 1.0 and the service's
    ``noise_scale``; a conversion's noise scale is its row's."""

    def __init__(self, row, seed: int, scales=(None, None, None, None), out_fmt=None, prosody=None, loudness=None, limiter=None,
                 denoise=None):
        self.row, self.seed, self.scales = row, int(seed), scales
        self.denoise = denoise        # ``_denoise_spec``: the strength of the denoiser on the request's waveform, or None
        self.sid = None               # a text request's speaker number, once its batch is collated (the denoiser's bias)
        self.limiter = limiter        # ``_limiter_spec``: (attack, hold, ceiling, gain) of the limiter behind the request's gain, or None
        self.loudness = loudness      # ``_loudness_spec``: the level the request's waveform is brought to, or None
        self.out_fmt = out_fmt        # ``_output_format``: the request's own output rate and encoding, or None
        self.prosody = prosody        # a ``_Recording``: the row's f0 / energy come from it (``_prosody_controls``), or None

    @property
    def is_conversion(self) -> bool:
        return isinstance(self.row, _Conversion)


def _collate_from(table, spk2id, collate):
    """The rows -> batch arrays callable of a batching service: ``collate``, or ``collate_rows`` with ``table`` / ``spk2id``."""
    if collate is not None:
        return collate
    if table is None or spk2id is None:
        raise ValueError("pass table and spk2id (for collate_rows) or a collate callable")
    from ..text import collate_rows
    return lambda rows: collate_rows(rows, table, spk2id)


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
    from ..models import RowControls
    col = lambda i, default: np.array([default if sc[i] is None else float(sc[i]) for sc in scales], dtype=np.float32)
    return RowControls(col(0, 1.0), col(1, 1.0), col(2, 1.0), col(3, noise_scale), np.asarray(given, dtype=bool))


def _table_controls(batch, rows_ctl):
    """duration / f0 / energy of a batch that runs with a table: a control no row is given is not passed."""
    return tuple(batch.get(k) if rows_ctl.given[:, i].any() else None for i, k in enumerate(("duration", "f0", "energy")))


def _aligned_durations(eng, batch, reqs, idx, audio, n, align):
    """The prosody requests whose rows brought no durations (a service with ``prosody_align``): ONE ``Engine.align_audio``
    call for all of them -- the row's text against its recording, spoken by the row's speaker unless the request named
    ``prosody_sid`` -- and the result in the batch's ``duration`` rows, marked ``given``.  A batch whose prosody rows all
    brought their durations is not touched."""
    need = [k for k, i in enumerate(idx) if getattr(reqs[i].row, "durations", None) is None]
    if not need:
        return batch
    if align is None:
        raise ValueError("prosody_audio: the row must bring its durations (the phonemes' frames in the recording)")
    B, Tp = np.asarray(batch["phonemes"]).shape
    given = batch.get("given")
    if given is None:                        # (a collate callable that returns none: every row has what its batch has,
        have = [batch.get(k) is not None for k in ("duration", "f0", "energy")]      # but for the rows aligned here)
        given = np.tile(np.array([have], dtype=bool), (B, 1))
        given[[idx[k] for k in need], 0] = False
    rows = [idx[k] for k in need]
    sid = np.asarray(batch["sid"])[rows]
    sid_audio = [int(sid[q]) if reqs[i].prosody.sid is None else reqs[i].prosody.sid for q, i in enumerate(rows)]
    d = eng.align_audio(_as_tensor(np.asarray(batch["phonemes"])[rows]), _as_tensor(np.asarray(batch["lengths"])[rows]),
                        _as_tensor(sid), audio[need], [n[k] for k in need], sid_audio=sid_audio, params=align)
    batch = dict(batch)
    dur = (np.zeros((B, Tp), dtype=np.float32) if batch.get("duration") is None
           else np.array(batch["duration"], dtype=np.float32))
    dur[rows] = d.cpu().numpy()
    given = np.array(given, dtype=bool)
    given[rows, 0] = True
    batch["duration"], batch["given"] = dur, given
    return batch


def _prosody_controls(eng, batch, reqs, model_rate, path=None, align=None):
    """The requests that name a recording (``submit(prosody_audio=...)``): their raw recordings through the input stage,
    then ONE ``Engine.prosody_contours`` and ONE ``Engine.prosody_phonemes`` call for all of them, with the durations their
    rows brought.  The results go into the batch's ``f0`` / ``energy`` control rows ON THE DEVICE (the two arrays become
    device tensors; nothing is read back) and the rows are marked ``given``.  A batch without such a request is not touched.
    ``path``: the service's ``prosody_path`` -- None: the contour call as it always was; else its ``path`` keyword (still ONE call).
    ``align``: the service's ``prosody_align`` -- rows that brought no durations are aligned to their recordings first
    (``_aligned_durations``); rows that brought them make the calls they always made."""
    idx = [i for i, r in enumerate(reqs) if r.prosody is not None]
    if not idx:
        return batch
    import torch
    jobs = [reqs[i].prosody for i in idx]
    if any(j.fmt is not None for j in jobs):
        _through_input_stage(eng, jobs, model_rate)
    n = [len(j.audio) for j in jobs]
    audio = torch.zeros((len(idx), max(n)), dtype=torch.float32, device=eng.device)
    for k, j in enumerate(jobs):
        audio[k, : n[k]] = torch.as_tensor(j.audio)
    batch = _aligned_durations(eng, batch, reqs, idx, audio, n, align)
    f0_frames, energy_frames, _, frames_host = (eng.prosody_contours(audio, n) if path is None
                                                else eng.prosody_contours(audio, n, path=path))
    dur = np.asarray(batch["duration"])
    B, Tp = dur.shape
    f0, energy = eng.prosody_phonemes(f0_frames, energy_frames, frames_host, dur[idx], np.asarray(batch["lengths"])[idx])
    batch = dict(batch)
    rows = torch.as_tensor(idx, device=eng.device)
    for key, val in (("f0", f0), ("energy", energy)):
        have = batch.get(key)
        ctl = (torch.zeros((B, Tp), dtype=torch.float32) if have is None else torch.as_tensor(np.asarray(have), dtype=torch.float32))
        ctl = ctl.to(eng.device)
        ctl[rows] = val
        batch[key] = ctl
    given = batch.get("given")
    if given is None:
        given = np.tile(np.array([[batch.get(k) is not None for k in ("duration", "f0", "energy")]], dtype=bool), (B, 1))
    given = np.array(given, dtype=bool)
    given[idx, 1:] = True
    batch["given"] = given
    return batch


def _collated(collate, reqs, noise_scale: float, eng=None, model_rate=None, prosody_path=None, prosody_align=None):
    """``(batch, (duration, f0, energy), keywords)`` of text requests: ``collate``, the controls of the requests that name a
    recording (``_prosody_controls``) and, where the requests need one, the per-row table -- the ``row_controls`` keyword is
    passed only then: a group without one makes the calls it always made."""
    batch = collate([r.row for r in reqs])
    if eng is not None:
        batch = _prosody_controls(eng, batch, reqs, model_rate, prosody_path, prosody_align)
    table = _row_table(batch, [r.scales for r in reqs], noise_scale)
    if table is None:
        return batch, (batch.get("duration"), batch.get("f0"), batch.get("energy")), {}
    return batch, _table_controls(batch, table), {"row_controls": table}


def _as_tensor(a):
    """A batch array as a tensor: numpy through ``torch.as_tensor``, a control that is on the device already as it is."""
    import torch
    return None if a is None else a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))


def _text_latents(eng, collate, reqs, noise_scale: float, model_rate=None, prosody_path=None, prosody_align=None):
    """The text requests of one batch or admitted group to their latent: ``collate``, the per-row table where the requests
    need one, then ONE isolated ``encode`` / ``frame_lengths_host`` / ``decode(max_len=0)``.  Returns per request
    ``(z row [inter, T], g row, frames)``; a request of no frames gives ``(None, None, 0)``."""
    prosody = any(getattr(r, "prosody", None) is not None for r in reqs)
    batch, ctl, kw = _collated(collate, reqs, noise_scale, *((eng, model_rate, prosody_path, prosody_align) if prosody else ()))
    t = _as_tensor
    for b, r in enumerate(reqs):
        r.sid = int(batch["sid"][b])
    enc = eng.encode(t(batch["phonemes"]), t(batch["lengths"]), t(batch["sid"]), t(ctl[0]), t(ctl[1]), t(ctl[2]),
                     isolated=True, **kw)
    frames, tf = eng.frame_lengths_host(enc["frame_lengths"])
    z = None
    if tf > 0:
        z = eng.decode(enc, tf, None, noise_scale, max_len=0, noise_seed=[r.seed for r in reqs], isolated=True, **kw)["z"]
    return [(z[b], enc["g"][b], int(frames[b])) if int(frames[b]) > 0 else (None, None, 0) for b in range(len(reqs))]


def _convert_latents(eng, reqs, model_rate=None):
    """The conversion requests of one batch or admitted group through ``Engine.convert_latent``: ONE call (one per
    distinct ``noise_scale``, which is an argument of the call, where the requests name several).  Returns per request
    ``(z_hat row, g row, frames)``; a recording too short for a frame gives ``(None, None, 0)``.  The frame counts are
    host arithmetic (``frames_host``): nothing is read back from the device."""
    jobs = [r.row for r in reqs]
    out = [(None, None, 0)] * len(jobs)
    raw = [j for j in jobs if j.fmt is not None]
    if raw:
        _through_input_stage(eng, raw, model_rate)
    for scale in sorted({j.noise_scale for j in jobs}):
        idx = [i for i, j in enumerate(jobs) if j.noise_scale == scale and eng.convert_frames(len(j.audio)) > 0]
        if not idx:
            continue
        n = [len(jobs[i].audio) for i in idx]
        if raw:                                  # (rows from the input stage are on the device: the batch is built there)
            import torch
            audio = torch.zeros((len(idx), max(n)), dtype=torch.float32, device=eng.device)
            for k, i in enumerate(idx):
                audio[k, : n[k]] = torch.as_tensor(jobs[i].audio)
        else:
            audio = np.zeros((len(idx), max(n)), dtype=np.float32)
            for k, i in enumerate(idx):
                audio[k, : n[k]] = jobs[i].audio
        r = eng.convert_latent(audio, n, [jobs[i].sid_src for i in idx], [jobs[i].sid_tgt for i in idx], None,
                               noise_seed=[reqs[i].seed for i in idx], noise_scale=scale)
        for k, i in enumerate(idx):
            out[i] = (r["z_hat"][k], r["g"][k], int(r["frames_host"][k]))
    return out


def _through_input_stage(eng, jobs, model_rate=None) -> None:
    """The raw recordings of a group to float32 at the model's rate: ONE ``Engine.input_batch`` call per distinct
    ``(rate, encoding)``; each job's ``audio`` becomes its row of the result (on the device, its own length)."""
    for fmt in sorted({j.fmt for j in jobs}):
        group = [j for j in jobs if j.fmt == fmt and j.audio is None]
        if not group:
            continue
        rate, enc = fmt
        if rate not in eng.input_rates:
            eng.configure_input(rate, model_rate=model_rate)      # (allocates: configure the rates ahead where that matters)
        n = [j.raw.size for j in group]
        batch = np.zeros((len(group), max(max(n), 1)), dtype=group[0].raw.dtype)
        for k, j in enumerate(group):
            batch[k, : n[k]] = j.raw
        audio, n_out = eng.input_batch(batch, n, rate, enc)
        for k, j in enumerate(group):
            j.audio = audio[k, : n_out[k]]


def latents(eng, collate, requests, noise_scale: float, model_rate=None, prosody_path=None, prosody_align=None):
    """Per request ``(z row [inter, T], g row, frames)``, in request order: the text rows of the group through
    ``_text_latents``, then its conversions through ``_convert_latents``."""
    text = [i for i, r in enumerate(requests) if not r.is_conversion]
    conv = [i for i, r in enumerate(requests) if r.is_conversion]
    done = []
    if text:
        done += zip(text, _text_latents(eng, collate, [requests[i] for i in text], noise_scale, model_rate, prosody_path, prosody_align))
    if conv:
        done += zip(conv, _convert_latents(eng, [requests[i] for i in conv], model_rate))
    out = [None] * len(requests)
    for i, lat in done:
        out[i] = lat
    return out


class BatchingSynthesisService:
    """Requests from many callers, synthesised together (round 10).  The single-flight services refuse a request while
    another is in flight, because in the reference's padded batch an utterance's audio depends on its batch-mates; in ISOLATED mode it
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
    ``table`` / ``spk2id``: what ``collate_rows`` needs to pad the rows (or ``collate``: any callable rows -> batch arrays).
    ``prosody_path``: how every ``prosody_audio`` request of this service gets its F0 -- None: each frame decides for itself;
    True or (octave_jump_cost, voiced_unvoiced_cost, max_candidates) / a dict of them: the path finder
    (``Engine.prosody_contours(path=...)``).  A batch still makes ONE contour call.
    ``prosody_align``: None -- a ``prosody_audio`` request must bring its durations, as always; True or (max_advance, stay_cost,
    skip_cost) / a dict of them (True: 2, 0, 0): a request whose row brings none gets them from its recording first
    (``Engine.align_audio``; needs the ``enc_q.*`` tensors), ONE call per batch.
    ``loudness``: the level every request of this service is brought to unless it names its own (``submit(loudness=)``;
    False there: none) -- a target in LUFS or a mapping of (target_lufs, peak_ceiling, max_gain_db); None: none.  A batch in
    which a request has one makes ONE ``Engine.loudness_normalize`` call on the generator's output, in place, before the
    output stage; a batch in which nobody has one makes exactly the calls it always made.
    ``limiter``: the look-ahead limiter behind every request's gain unless it names its own
    (``submit(limiter=)``; False there: none) -- True or a mapping of (attack_ms, hold_ms, ceiling, gain_db); None: none.  A
    request with a loudness and a limiter gets the gain of its target NOT cut by its peak and the limiter at its
    ``peak_ceiling`` (``normalize_loudness(limiter=)``); one with a limiter only gets ``gain_db`` (0) and the limiter at
    ``ceiling`` (1).  ONE limiter call per batch, before the output stage; a batch in which nobody names a limiter makes
    exactly the calls it made before.
    ``denoise``: the denoiser on every request's waveform unless it names its own
    (``submit(denoise=)``; False there: none) -- a strength, or True for 0.01; None: none.  A batch in which a request has
    one makes ONE ``net.denoise`` call on the generator's output, in place, with the speaker's own bias (a conversion's:
    ``sid_tgt``), BEFORE the loudness call, the limiter and the encoding: what is measured and limited is what is delivered.
    The other rows carry a NaN strength and are neither read nor written, and so does a row too short for the reflection
    at its ends (at most (n_fft - hop) / 2 samples); a batch in which nobody has one makes exactly the calls it made before.
    ``denoise_transform="fft"`` hands ``transform="fft"`` to that one call; a service that names none
    makes the call, and delivers the bytes, it always did."""

    def __init__(self, net, max_batch: int = 16, max_wait_s: float = 0.005, noise_scale: float = 0.667, *, table=None,
                 spk2id=None, collate=None, output_rate: Optional[int] = None, sampling_rate: int = 44100, prosody_path=None,
                 prosody_align=None, loudness=None, limiter=None, denoise=None, denoise_transform=None):
        if max_batch < 1 or max_wait_s < 0:
            raise ValueError("max_batch >= 1 and max_wait_s >= 0")
        self._collate = _collate_from(table, spk2id, collate)
        self.net, self.max_batch, self.max_wait_s = net, int(max_batch), float(max_wait_s)
        self.noise_scale = float(noise_scale)
        self.output_rate = None if output_rate is None else int(output_rate)
        self.sampling_rate = int(sampling_rate)
        if prosody_path is not None and prosody_path is not False:
            from ..engine import Engine
            prosody_path = Engine._prosody_path(prosody_path)         # (refused here, not in the worker)
        self.prosody_path = prosody_path or None
        if prosody_align is not None and prosody_align is not False:
            from ..engine import Engine
            prosody_align = Engine._align_params(prosody_align)      # (refused here, not in the worker)
        self.prosody_align = prosody_align or None
        self.loudness = _loudness_spec(loudness)
        self.limiter = limiter if limiter is not None and limiter is not False else None
        _limiter_spec(self.limiter, self.loudness, self.sampling_rate)             # (refused here, not in the worker)
        self.denoise = _denoise_spec(denoise)
        self.denoise_transform = _denoise_transform(denoise_transform)
        if self.output_rate is not None:
            net._engine.configure_output(self.output_rate, in_rate=int(sampling_rate))
        self._q: "queue.Queue" = queue.Queue()
        self._closed = False
        self._gate = threading.Lock()        # orders _enqueue's check + put against close's sentinel: nothing queues behind it
        self._worker = threading.Thread(target=self._run, name="vispeech-batching", daemon=True)
        self._worker.start()

    def submit(self, row, noise_seed: int, *, duration_scale=None, pitch_scale=None, energy_scale=None,
               noise_scale=None, output_rate: Optional[int] = None, output_encoding=None, prosody_audio=None,
               prosody_sample_rate: Optional[int] = None, prosody_encoding=None, prosody_sid=None,
               loudness=None, limiter=None, denoise=None) -> "concurrent.futures.Future":
        """``row``: one row as ``vispeech_amd.text.collate_rows`` takes it (a ``FilelistRow``).  The four scales are the
        request's own (None: 1.0, and the service's ``noise_scale``); a scale whose control the row carries is not read.
        The future's result is the request's PCM16 samples (numpy int16, valid part only).
        ``output_rate`` / ``output_encoding`` (``vispeech_amd.output_stage``: "f32", "s16", "ulaw", "alaw"): the request's own
        delivery format -- the result is then float32, int16 or uint8 (G.711 codes) at that rate.  When any request of a
        collected batch names one, all its waveforms leave through ONE ``Engine.output_rows`` call and one device-to-host
        copy; requests that name none ride as rows of (the service's rate, PCM16) and get the bytes they always got.
        ``prosody_audio`` (prosody transfer): a 1-D recording -- float32 at the model's rate, or raw at
        ``prosody_sample_rate`` / in ``prosody_encoding`` (``vispeech_amd.input_stage``) -- whose melody and loudness the
        request is spoken with.  The row brings phones and durations (refused here without them, and where the durations
        claim more frames than the recording has); the worker computes the recording's per-phoneme F0 and energy
        (``SynthesizerTrn.prosody_from_audio``: ONE contour call and ONE phoneme call for all such requests of a batch) and
        they take the place of whatever f0 / energy the row carries.  The request is then what
        ``infer(isolated=True, duration_control=.., pitch_control=f0, energy_control=energy)`` returns for it alone.
        On a service with ``prosody_align`` a row without durations is accepted: the worker aligns its text to the recording
        first (``prosody_sid``: the recording's speaker where it is not the row's).
        ``loudness``: the integrated loudness (BS.1770, LUFS) the request's waveform is brought to before it is encoded -- a
        target, or a mapping of (target_lufs, peak_ceiling, max_gain_db); None: the service's; False: none.
        ``limiter``: the limiter behind the request's gain -- True or a mapping of (attack_ms, hold_ms, ceiling, gain_db);
        None: the service's; False: none.
        ``denoise``: the strength of the denoiser on the request's waveform, or True for 0.01; None: the service's; False:
        none."""
        prosody = None
        if prosody_sid is not None:
            n_spk = getattr(self.net, "n_speakers", None)
            if int(prosody_sid) != prosody_sid or int(prosody_sid) < 0 or (n_spk is not None and int(prosody_sid) >= int(n_spk)):
                raise ValueError(f"prosody_sid must be a speaker number in [0, {n_spk if n_spk is not None else 'n_speakers'})")
        if prosody_audio is not None:
            prosody = _Recording(prosody_audio, _input_format(prosody_sample_rate, prosody_encoding, self.sampling_rate), prosody_sid)
            durations = getattr(row, "durations", None)
            if durations is None and self.prosody_align is None:
                raise ValueError("prosody_audio: the row must bring its durations (the phonemes' frames in the recording)")
            n, hop = prosody.samples(self.sampling_rate), int(self.net.dims.total_upsample)
            if durations is None:
                if n < 641:
                    raise ValueError(f"prosody_audio: {n} samples at the model's rate: it needs 641")
            elif n < 641 or int(np.sum(durations)) > n // hop + 1:
                raise ValueError(f"prosody_audio: {n} samples at the model's rate ({n // hop + 1} frames): it needs 641, and "
                                 f"the row's durations claim {int(np.sum(durations))} frames")
        elif prosody_sample_rate is not None or prosody_encoding is not None:
            raise ValueError("prosody_sample_rate / prosody_encoding describe prosody_audio: pass it")
        elif prosody_sid is not None:
            raise ValueError("prosody_sid names the speaker of prosody_audio: pass it")
        return self._enqueue(_Request(row, noise_seed, (duration_scale, pitch_scale, energy_scale, noise_scale),
                                      _output_format(output_rate, output_encoding), prosody, *self._level_of(loudness, limiter),
                                      denoise=self._denoise_of(denoise)))

    def submit_conversion(self, audio, sid_src: int, sid_tgt: int, noise_seed: int, *, noise_scale=None,
                          sample_rate: Optional[int] = None, encoding=None, output_rate: Optional[int] = None,
                          output_encoding=None, loudness=None, limiter=None, denoise=None) -> "concurrent.futures.Future":
        """``audio``: a 1-D float32 recording at the model's rate, spoken by speaker ``sid_src``; the future's result is the
        PCM16 of the recording converted to ``sid_tgt`` (``T(n) * up`` samples at the model's rate, or at ``output_rate``).
        ``noise_scale`` multiplies the posterior's noise (None: 1.0, the reference -- NOT the service's text-to-speech
        ``noise_scale``); ``noise_seed`` keys that noise.
        ``sample_rate`` / ``encoding`` (``vispeech_amd.input_stage``): ``audio`` is raw -- an array of the encoding's dtype or
        ``bytes`` -- at that rate; the batch's raw recordings go through the input stage on the GPU, one call per distinct
        (rate, encoding), before the one ``convert_latent``.  ``output_rate`` / ``output_encoding`` / ``loudness``: as in
        ``submit`` (the level is that of the converted waveform; the recording is not normalised before conversion);
        ``limiter``: as in ``submit``; ``denoise``: as in ``submit``, with the bias of ``sid_tgt``."""
        fmt = _input_format(sample_rate, encoding, self.sampling_rate)
        return self._enqueue(_Request(_Conversion(audio, sid_src, sid_tgt, noise_scale, fmt), noise_seed,
                                      out_fmt=_output_format(output_rate, output_encoding), denoise=self._denoise_of(denoise),
                                      **dict(zip(("loudness", "limiter"), self._level_of(loudness, limiter)))))

    def _denoise_of(self, denoise):
        return self.denoise if denoise is None else _denoise_spec(denoise)

    def _denoise(self, reqs, waves, n, sids) -> None:
        """The requests that have a denoiser: ONE ``net.denoise`` call over the batch's rows ``waves`` [B, L] (the generator's
        output, row b's first ``n[b]`` samples), in place, each row with the bias of its speaker ``sids[b]``.  A row that asks
        for nothing, or is too short for the reflection at its ends, carries a NaN strength and is neither read nor
        written; a batch in which nobody asks makes no call."""
        if waves.shape[-1] == 0 or all(r.denoise is None for r in reqs):
            return
        d = self.net.dims
        pad = (2 * (int(d.spec_channels) - 1) - int(d.total_upsample)) // 2
        nan = float("nan")
        strength = [nan if r.denoise is None or int(n[b]) <= pad else r.denoise for b, r in enumerate(reqs)]
        if all(s != s for s in strength):
            return
        kw = {} if self.denoise_transform == "dft" else {"transform": self.denoise_transform}
        self.net.denoise(waves, [max(int(v), 1) for v in n], [int(s) for s in sids], strength, **kw)

    def _loudness_of(self, loudness):
        return self.loudness if loudness is None else _loudness_spec(loudness)

    def _level_of(self, loudness, limiter):
        """``(loudness, limiter)`` specs of a request: its own, or the service's."""
        loud = self._loudness_of(loudness)
        return loud, _limiter_spec(self.limiter if limiter is None else limiter, loud, self.sampling_rate)

    def _normalize(self, reqs, waves, n) -> None:
        """The requests that have a loudness: ONE ``Engine.loudness_normalize`` call over the batch's rows ``waves`` [B, L]
        (the generator's output, row b's first ``n[b]`` samples), in place, at the model's rate.  A row that asks for nothing
        carries a NaN target and is neither read nor written by the apply; a batch in which nobody asks makes no call."""
        if waves.shape[-1] == 0:
            return
        if any(r.limiter is not None for r in reqs):
            return level_rows(self.net._engine, reqs, waves, n, self.sampling_rate)
        if all(r.loudness is None for r in reqs):
            return
        from ..engine import Engine
        nan = float("nan")
        spec = [(nan, 1.0, 0.0) if r.loudness is None or n[b] < 1 else r.loudness for b, r in enumerate(reqs)]
        params = Engine.loudness_params(len(reqs), *zip(*spec))
        self.net._engine.loudness_normalize(waves, [max(int(v), 1) for v in n], self.sampling_rate, params)

    def _enqueue(self, req: _Request) -> "concurrent.futures.Future":
        req.future = concurrent.futures.Future()
        with self._gate:
            if self._closed:
                raise RuntimeError("the service is closed")
            self._q.put(req)
        return req.future

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
            reqs = [r for r in reqs if r.future.set_running_or_notify_cancel()]
            if not reqs:
                continue
            try:
                for r, pcm in zip(reqs, self._synthesize(reqs)):
                    r.future.set_result(pcm)
            except Exception as e:           # this batch's requests fail; the worker lives on
                for r in reqs:
                    if not r.future.done():
                        r.future.set_exception(e)

    def _pcm16(self, x) -> np.ndarray:
        return _row_pcm16(x, None if self.output_rate is None else self.net._engine)

    def _synthesize(self, reqs):
        import torch
        net = self.net
        if any(r.is_conversion for r in reqs):
            return self._synthesize_mixed(reqs)
        hop = net.dims.total_upsample
        prosody = (net._engine, self.sampling_rate, self.prosody_path, self.prosody_align) if any(r.prosody is not None for r in reqs) else ()
        batch, ctl, kw = _collated(self._collate, reqs, self.noise_scale, *prosody)
        t = lambda a: None if a is None else _as_tensor(a).to(net.device)
        o, x_mask, *_ = net.infer(t(batch["phonemes"]), t(batch["lengths"]), sid=t(batch["sid"]), noise_scale=self.noise_scale,
                                  duration_control=t(ctl[0]), pitch_control=t(ctl[1]),
                                  energy_control=t(ctl[2]), noise_seed=[r.seed for r in reqs], isolated=True, **kw)
        frames = x_mask.sum(dim=(1, 2)).cpu().tolist()
        self._denoise(reqs, o[:, 0, :], [int(frames[b]) * hop for b in range(len(reqs))], np.asarray(batch["sid"]).reshape(-1))
        self._normalize(reqs, o[:, 0, :], [int(frames[b]) * hop for b in range(len(reqs))])
        if any(r.out_fmt is not None for r in reqs):
            return self._deliver_rows(reqs, [o[b, 0, : int(frames[b]) * hop] for b in range(len(reqs))])
        return [self._pcm16(o[b:b + 1, 0, : int(frames[b]) * hop]) for b in range(len(reqs))]

    def _deliver_rows(self, reqs, waves):
        """A batch in which a request names its own format: every request's valid samples (``waves``, 1-D float rows on the
        device; None: nothing to deliver) as a row of ONE ``Engine.output_rows`` call, ONE device-to-host copy, and each
        request's array in its encoding's dtype."""
        from .. import output_stage
        from ._pcm import _host
        eng = self.net._engine
        base = self.sampling_rate if self.output_rate is None else self.output_rate
        fmts = _row_formats(eng, reqs, base, self.sampling_rate)
        empty = lambda enc: np.zeros(0, dtype=np.dtype(output_stage.NUMPY_DTYPES[enc]).newbyteorder("<"))
        out = [empty(enc) for _, enc in fmts]
        live = [i for i, w in enumerate(waves) if w is not None and w.shape[-1] > 0]
        if live:
            buf, spans = eng.output_rows([(waves[i].reshape(-1), True, fmts[i][0], fmts[i][1], None) for i in live])
            host = _host(buf)                                           # the batch's one device-to-host copy
            for i, a in zip(live, output_stage.unpack(host, spans, [fmts[i][1] for i in live])):
                out[i] = a.copy()
        return out

    def _synthesize_mixed(self, reqs):
        """A batch with conversions: every request's latent, speaker vector and length packed into one ragged batch, ONE
        ``generator_ragged`` call, then the output stage as in ``_synthesize``."""
        import torch
        net, eng = self.net, self.net._engine
        lat = latents(eng, self._collate, reqs, self.noise_scale, self.sampling_rate, self.prosody_path, self.prosody_align)
        live = [i for i, (_, _, L) in enumerate(lat) if L > 0]
        pcms = [np.zeros(0, dtype="<i2") for _ in reqs]
        if not live:
            return self._deliver_rows(reqs, [None] * len(reqs)) if any(r.out_fmt is not None for r in reqs) else pcms
        T = max(lat[i][2] for i in live)
        z0 = torch.as_tensor(lat[live[0]][0])
        Z = torch.zeros((len(live), z0.shape[0], T), dtype=torch.float32, device=z0.device)
        for b, i in enumerate(live):
            Z[b, :, : lat[i][2]] = torch.as_tensor(lat[i][0])[:, : lat[i][2]]
        G = torch.stack([torch.as_tensor(lat[i][1]).reshape(-1) for i in live])
        o = eng.generator_ragged(Z, G, [lat[i][2] for i in live])
        hop = net.dims.total_upsample
        self._denoise([reqs[i] for i in live], o[:, 0, :], [lat[i][2] * hop for i in live],
                      [reqs[i].row.sid_tgt if reqs[i].is_conversion else reqs[i].sid for i in live])
        self._normalize([reqs[i] for i in live], o[:, 0, :], [lat[i][2] * hop for i in live])
        if any(r.out_fmt is not None for r in reqs):
            waves = [None] * len(reqs)
            for b, i in enumerate(live):
                waves[i] = o[b, 0, : lat[i][2] * hop]
            return self._deliver_rows(reqs, waves)
        for b, i in enumerate(live):
            pcms[i] = self._pcm16(o[b:b + 1, 0, : lat[i][2] * hop])
        return pcms
