"""Drop-in ``SynthesizerTrn`` for the inference path.

Mirrors the reference's class surface for ``infer`` and nothing else:
the constructor signature (reference models.py:537-561), ``infer`` with the same arguments and the
same 6-tuple result (reference models.py:672-722), ``load_state_dict`` accepting reference
checkpoints unchanged (753-tensor schema, weight_g/weight_v pairs included; 609 tensors for ``resblock`` "2", the
ResBlock2 generator), ``eval()``, ``to()``.
``voice_conversion`` (reference models.py:724-732) is served as well when the checkpoint carries the
``enc_q.*`` tensors.  Training-time members (``forward``, discriminators) are out of scope and raise.  All arithmetic runs in libvispeech_hip on the MI355X; if the extension is not
built, constructing the model raises ImportError.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Mapping, Optional

import numpy as np
import torch

from .engine import Engine
from .schema import ModelDims, dims_from_ctor, state_dict_schema, used_by_infer


@dataclass
class RowControls:
    """Per-row arguments of an isolated ``infer`` (``vsp_set_row_controls``): utterance b is synthesised as the reference's
    B = 1 call with ``duration_control`` = row b of the tensor if ``given[b, 0]`` else the scalar ``duration_scale[b]``,
    likewise pitch (``given[b, 1]``) and energy (``given[b, 2]``), and ``noise_scale[b]``.  Four ``[B]`` float arrays and
    a ``[B, 3]`` bool array; a scale whose control is given is not read."""
    duration_scale: np.ndarray
    pitch_scale: np.ndarray
    energy_scale: np.ndarray
    noise_scale: np.ndarray
    given: np.ndarray

    def __post_init__(self):
        for k in ("duration_scale", "pitch_scale", "energy_scale", "noise_scale"):
            setattr(self, k, np.asarray(getattr(self, k), dtype=np.float32).reshape(-1))
        self.given = np.asarray(self.given, dtype=bool)
        B = len(self.duration_scale)
        if any(len(getattr(self, k)) != B for k in ("pitch_scale", "energy_scale", "noise_scale")) or self.given.shape != (B, 3):
            raise ValueError("RowControls: four [B] scale arrays and a [B, 3] bool `given`")

    def __len__(self) -> int:
        return len(self.duration_scale)

    @classmethod
    def uniform(cls, B: int, duration_scale: float = 1.0, pitch_scale: float = 1.0, energy_scale: float = 1.0,
                noise_scale: float = 1.0, given=(False, False, False)) -> "RowControls":
        """Every row with the same scales and given bits: what the scalar arguments of a call say."""
        full = lambda v: np.full(int(B), v, dtype=np.float32)
        return cls(full(duration_scale), full(pitch_scale), full(energy_scale), full(noise_scale),
                   np.tile(np.asarray(given, dtype=bool).reshape(1, 3), (int(B), 1)))


class SynthesizerTrn:
    """Synthesizer for inference (reference models.py:532-722)."""

    def __init__(self, n_vocab, spec_channels, hop_length, sampling_rate, segment_size, inter_channels,
                 hidden_channels, filter_channels, n_heads, n_layers, kernel_size, p_dropout, resblock,
                 resblock_kernel_sizes, resblock_dilation_sizes, upsample_rates, upsample_initial_channel,
                 upsample_kernel_sizes, n_speakers=0, gin_channels=0, use_sdp=False, freeze_textencoder=False,
                 freeze_decoder=False, device="cuda:0", **kwargs):
        self.dims: ModelDims = dims_from_ctor(
            n_vocab, spec_channels, hop_length, sampling_rate, segment_size, inter_channels, hidden_channels,
            filter_channels, n_heads, n_layers, kernel_size, p_dropout, resblock, resblock_kernel_sizes,
            resblock_dilation_sizes, upsample_rates, upsample_initial_channel, upsample_kernel_sizes,
            n_speakers=n_speakers, gin_channels=gin_channels)
        self.n_speakers = n_speakers
        self.gin_channels = gin_channels
        self.use_sdp = use_sdp            # stored and ignored, as in the reference (models.py:583)
        self.hop_length = hop_length
        self.sampling_rate = sampling_rate
        self.training = False
        self._engine = Engine(self.dims, device)
        self._state: "dict[str, np.ndarray]" = {}

    # ---------------------------------------------------------------- nn.Module-like surface
    @property
    def device(self) -> torch.device:
        return self._engine.device

    def eval(self):
        self.training = False
        return self

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError("training is out of scope of the MI355X synthesis path")
        return self

    def to(self, device):
        if torch.device(device) != self._engine.device:
            eng = Engine(self.dims, device)
            if self._state:
                eng.set_weights(self._state, strict=False)
                eng.finalize()
            self._engine = eng
        return self

    def cuda(self, device=None):
        return self.to(f"cuda:{0 if device is None else device}")

    def state_dict(self):
        """Every tensor of the reference's 753-key schema, in the reference's order: the loaded value where one has been
        loaded, zeros of the schema's shape otherwise -- so that the reference's own loader (utils.py:29-46), which
        iterates ``model.state_dict()`` BEFORE the first load and keeps the model's value for keys the checkpoint
        lacks, runs against this class as written (inference.py:36).  (The reference keeps its random init there; this
        class has no init: a key the checkpoint lacks loads as zeros.)"""
        from collections import OrderedDict
        out = OrderedDict()
        for k, shape in state_dict_schema(self.dims).items():
            v = self._state.get(k)
            out[k] = torch.from_numpy(v.copy()) if v is not None else torch.zeros(shape, dtype=torch.float32)
        for k, v in self._state.items():
            if k not in out:
                out[k] = torch.from_numpy(v.copy())
        return out

    def load_state_dict(self, state_dict: Mapping[str, "torch.Tensor | np.ndarray"], strict: bool = True):
        """Accepts a reference ``net_g.state_dict()`` / ``checkpoint['model']`` unchanged."""
        schema = state_dict_schema(self.dims)
        host = {}
        for k, v in state_dict.items():
            # float32 host copy (what state_dict() / to() hand back); the engine itself receives the tensors as
            # they are, so a float16 / bfloat16 / float64 or device-resident checkpoint goes through the typed entry
            a = v.detach().to(torch.float32).cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
            host[k] = np.ascontiguousarray(a, dtype=np.float32)
        missing = [k for k in schema if used_by_infer(k) and k not in host]
        if strict and missing:
            raise RuntimeError(f"load_state_dict: {len(missing)} missing keys, e.g. {missing[:3]}")
        _, unexpected = self._engine.set_weights(state_dict, strict=strict)
        self._state = host
        self.__dict__.pop("_denoiser_bias", None)      # (the denoiser's bias is a function of the weights)
        self._engine.finalize()
        return missing, unexpected

    def forward(self, *a, **k):
        raise NotImplementedError("SynthesizerTrn.forward is the training path (reference models.py:624-670): out of scope")

    @torch.no_grad()
    def voice_conversion(self, y, y_lengths, sid_src, sid_tgt, *, noise: Optional[torch.Tensor] = None,
                         isolated: bool = False):
        """Reference models.py:724-732: posterior encoder on the linear spectrogram ``y``
        [B, spec_channels, T] with the source speaker, flow forward (source), flow reverse (target),
        generator (target).  ``noise`` (keyword-only, optional) replaces the ``torch.randn_like`` of
        the posterior encoder (models.py:240).  ``isolated``: as in ``infer`` -- the vocoder ends every utterance's tensors at
        its own length.  Returns ``(o_hat, y_mask, (z, z_p, z_hat))``; needs the
        ``enc_q.*`` tensors in the loaded state_dict."""
        eng = self._engine
        if not eng.ready:
            raise RuntimeError("weights not loaded: call load_state_dict first")
        assert self.n_speakers > 0, "n_speakers have to be larger than 0."      # models.py:725
        if not eng.has_voice_conversion:
            raise RuntimeError("voice_conversion needs the enc_q.* tensors: the loaded state_dict had none")
        B, _, T = y.shape
        if noise is None:
            noise = torch.randn(B, self.dims.inter_channels, T, dtype=torch.float32, device=eng.device)
        # (the keyword is passed only when set: engine stand-ins of older callers and tests need not know it)
        r = eng.voice_conversion(y, y_lengths, sid_src, sid_tgt, noise, **({"isolated": True} if isolated else {}))
        return r["o_hat"], r["y_mask"].to(torch.float32), (r["z"], r["z_p"], r["z_hat"])

    @torch.no_grad()
    def convert_audio(self, audio, n_samples, sid_src, sid_tgt, *, noise: Optional[torch.Tensor] = None, noise_seed=None,
                      noise_scale: float = 1.0, sample_rate: Optional[int] = None, encoding=None):
        """``voice_conversion`` from audio, for a batch of recordings of different lengths: ``audio`` [B, L] at the model's
        rate, row b the recording ``audio[b, :n_samples[b]]`` (what lies behind is never read).  Every recording is
        converted as the reference converts it alone -- ``voice_conversion`` on ``spectrogram_torch`` of that recording,
        B = 1 -- and every returned tensor is exactly 0 behind the row's ``T_b`` frames (``T_b * up`` samples).
        ``noise`` [B, inter, T_max] replaces the posterior's ``torch.randn_like`` (row b uses its first ``T_b`` columns);
        without it ``noise_seed`` is a list of B ints, one Philox key per recording (a plain int raises ``ValueError``, as in
        ``infer(isolated=True)``).  ``noise_scale`` multiplies that noise: 1.0 is the reference, 0 needs neither noise nor
        seeds.  Returns ``(o_hat, y_mask, (z, z_p, z_hat))`` like ``voice_conversion``.
        ``sample_rate`` / ``encoding`` (``vispeech_amd.input_stage``: float32, PCM16, mu-law or A-law, by name or number):
        ``audio`` [B, L] is then raw -- int16 or uint8 for the integer encodings -- at ``sample_rate`` (None: the model's),
        ``n_samples`` counts INPUT samples, and the batch goes through the input stage (``Engine.input_batch``) first; the
        rest is the path above on its result.  Without the two keywords nothing changes."""
        eng = self._engine
        if not eng.ready:
            raise RuntimeError("weights not loaded: call load_state_dict first")
        assert self.n_speakers > 0, "n_speakers have to be larger than 0."      # models.py:725
        if not eng.has_voice_conversion:
            raise RuntimeError("convert_audio needs the enc_q.* tensors: the loaded state_dict had none")
        if sample_rate is not None or encoding is not None:
            rate = int(self.dims.sampling_rate if sample_rate is None else sample_rate)
            if rate not in eng.input_rates:
                eng.configure_input(rate)
            audio, n_samples = eng.input_batch(audio, n_samples, rate, 0 if encoding is None else encoding)
        r = eng.convert(audio, n_samples, sid_src, sid_tgt, noise=noise, noise_seed=noise_seed, noise_scale=noise_scale)
        return r["o_hat"], r["y_mask"].to(torch.float32), (r["z"], r["z_p"], r["z_hat"])

    @torch.no_grad()
    def prosody_from_audio(self, audio, n_samples, durations, phonemes_lengths, *, sample_rate: Optional[int] = None,
                           encoding=None, params=None, path=None):
        """Per-phoneme F0 and energy of recordings -- what the reference's data preparation (f0energy.py) writes into a
        filelist row -- for a batch of recordings of different lengths: ``audio`` [B, L] at the model's rate, row b the
        recording ``audio[b, :n_samples[b]]`` (what lies behind is never read), ``durations`` [B, Tp] the frames of each of
        its ``phonemes_lengths[b]`` phonemes (whole numbers; ``sum <= n_samples[b] // hop + 1``).  Returns ``(f0, energy)``,
        both ``[B, Tp]`` float32 on the device, exact 0 for a phoneme of no frames and behind a row's phonemes: pass them
        straight to ``infer(..., isolated=True, duration_control=durations, pitch_control=f0, energy_control=energy)`` to
        speak a text with the melody and loudness of the recording.  F0 is Boersma's autocorrelation method as DESIGN.md
        section 4m states it (``params``: floor_hz, ceiling_hz, voicing_threshold, silence_threshold, octave_cost; None: 80,
        750, 0.6, 0.03, 0.01) -- NOT bit-compatible with parselmouth.  Works without the ``enc_q.*`` tensors.
        ``path``: None -- every frame decides for itself --, True or (octave_jump_cost, voiced_unvoiced_cost,
        max_candidates) / a dict of them (True: 0.35, 0.14, 15) -- F0 from the best path through every frame's candidates
        (section 4n), which neither jumps an octave for a frame nor drops a weak frame of a voiced stretch.
        ``sample_rate`` / ``encoding``: as in ``convert_audio`` -- ``audio`` is raw at that rate, ``n_samples`` counts input
        samples, and the batch goes through the input stage (``Engine.input_batch``) first."""
        eng = self._engine
        if sample_rate is not None or encoding is not None:
            rate = int(self.dims.sampling_rate if sample_rate is None else sample_rate)
            if rate not in eng.input_rates:
                eng.configure_input(rate)
            audio, n_samples = eng.input_batch(audio, n_samples, rate, 0 if encoding is None else encoding)
        if path is None:
            f0_frames, energy_frames, _, frames_host = eng.prosody_contours(audio, n_samples, params)
        else:
            f0_frames, energy_frames, _, frames_host = eng.prosody_contours(audio, n_samples, params, path=path)
        return eng.prosody_phonemes(f0_frames, energy_frames, frames_host, durations, phonemes_lengths)

    @torch.no_grad()
    def align_audio(self, phonemes, phonemes_lengths, sid, audio, n_samples, *, sid_audio=None,
                    sample_rate: Optional[int] = None, encoding=None, params=None, fit_length: bool = True):
        """The frames each phoneme of a text occupies in a recording of it -- the ``durations`` that ``prosody_from_audio``
        and ``infer(duration_control=)`` take, which the reference gets from an external forced aligner -- by monotonic
        alignment in the model's own prior space.  ``phonemes`` [B, Tp], ``phonemes_lengths`` [B],
        ``sid`` [B]: the texts; ``audio`` [B, L], ``n_samples`` [B]: their recordings as in ``convert_audio``
        (``sample_rate`` / ``encoding``: raw recordings through the input stage first); ``sid_audio`` [B]: who speaks the
        recordings (None: ``sid``).  The text is encoded in isolated mode with predicted durations, pitch and energy and
        decoded to its frame-level prior (``m_p``, ``logs_p``: a state per template frame, ``cum_dur`` maps states to
        phonemes); the recording goes through the posterior encoder and the forward flow without noise (``z_p``); every
        recording frame is scored under every state and the best left-to-right path is cut at the phoneme boundaries.
        ``fit_length``: encode a second time with each row's ``duration_scale = T_b / K_b`` (its recording's frames over its
        predicted frames), so that the template is about as long as the recording and the advance limit rarely binds.
        ``params``: (max_advance, stay_cost, skip_cost) or a dict of them (None: 2, 0, 0).  Returns ``durations`` [B, Tp]
        int64 on the device, ``sum(durations[b]) = vsp_convert_frames(n_samples[b]) <= n_samples[b] // hop + 1``, 0 behind a
        row's phonemes.  A recording too short for its text (fewer than (K_b - 1) / max_advance + 1 frames) is a
        ``ValueError`` naming the row.  Needs the ``enc_q.*`` tensors.  Alignment quality depends on the checkpoint."""
        eng = self._engine
        if not eng.ready:
            raise RuntimeError("weights not loaded: call load_state_dict first")
        assert self.n_speakers > 0, "n_speakers have to be larger than 0."
        if not eng.has_voice_conversion:
            raise RuntimeError("align_audio needs the enc_q.* tensors: the loaded state_dict had none")
        pp = eng._align_params(params)
        if sample_rate is not None or encoding is not None:
            rate = int(self.dims.sampling_rate if sample_rate is None else sample_rate)
            if rate not in eng.input_rates:
                eng.configure_input(rate)
            audio, n_samples = eng.input_batch(audio, n_samples, rate, 0 if encoding is None else encoding)
        return eng.align_audio(phonemes, phonemes_lengths, sid, audio, n_samples, sid_audio=sid_audio, params=pp,
                               fit_length=fit_length)

    @torch.no_grad()
    def loudness(self, audio, n_samples, sample_rate: Optional[int] = None):
        """The integrated loudness (ITU-R BS.1770-4 / EBU R 128, mono) of every row of a ragged batch:
        ``audio`` [B, L] float32 at ``sample_rate`` (None: the model's), row b ``audio[b, :n_samples[b]]`` (what lies behind
        is never read).  Returns ``(lufs, peak)``, both ``[B]`` float32 on the device: LUFS (-inf for a row all of whose
        blocks are gated out) and the SAMPLE peak (true peak is not computed).  Needs no weights."""
        fs = int(self.sampling_rate if sample_rate is None else sample_rate)
        lufs, peak, _ = self._engine.loudness(audio, n_samples, fs)
        return lufs, peak

    @torch.no_grad()
    def normalize_loudness(self, audio, n_samples, target_lufs=-23.0, peak_ceiling=1.0, max_gain_db=30.0,
                           sample_rate: Optional[int] = None, out=None, limiter=None):
        """Every row of ``audio`` [B, L] scaled to its target loudness, on the device in one call: ``g = 10^((target - L) /
        20)``, at most ``max_gain_db`` and at most ``peak_ceiling / peak``.  The three values are scalars or one per row; a row
        whose target is None or NaN, and a row of no loudness (-inf), is left as it is (gain exactly 1).  In place where
        ``audio`` is a float32 tensor on the model's device and ``out`` is None; samples at or behind ``n_samples[b]`` are not
        touched.  Returns ``(audio, gains)``.  ``infer(...)[0][:, 0]`` and ``convert_audio(...)[0][:, 0]`` are such batches.

        ``limiter``: ``True`` or ``dict(attack_ms=, hold_ms=)`` puts the look-ahead limiter (``limit``) behind the gain: a
        row's gain is ``min(target gain, max_gain_db)``, no longer cut by its sample peak -- one transient does not pull the
        whole row under its target --, and the limiter holds the row under ``peak_ceiling``.  Segments, gate and limiter run
        in this order with the gains staying on the device."""
        fs = int(self.sampling_rate if sample_rate is None else sample_rate)
        eng = self._engine
        B = len(n_samples)
        params = eng.loudness_params(B, target_lufs, peak_ceiling, max_gain_db)
        if limiter is None or limiter is False:
            res = eng.loudness_normalize(audio, n_samples, fs, params, out=out)
            return res[0], res[1]
        from . import limiter as _limiter
        if limiter is not True and set(limiter) - {"attack_ms", "hold_ms"}:
            raise ValueError("normalize_loudness: limiter is True or a mapping of attack_ms and hold_ms")
        A, H, _, _ = _limiter.spec(limiter, fs)
        res = eng.loudness_limit(audio, n_samples, fs, params, attack=A, hold=H, out=out)
        return res[0], res[1]

    @torch.no_grad()
    def true_peak(self, audio, n_samples):
        """The true peak (4x oversampled) of every row ``audio[b, :n_samples[b]]``: ``[B]`` float32 on the
        device, linear.  What lies behind a row's end is never read.  Needs no weights."""
        return self._engine.true_peak(audio, n_samples)

    @torch.no_grad()
    def limit(self, audio, n_samples, ceiling=1.0, gains=None, attack_ms: Optional[float] = None, hold_ms: Optional[float] = None,
              sample_rate: Optional[int] = None, out=None):
        """The look-ahead limiter over every row of a ragged batch: ``gains[b] * audio[b]`` held under
        ``ceiling`` (a scalar or one per row; None / NaN leaves the row alone) by a smoothed gain that looks ``attack_ms``
        (1.5) ahead and holds for ``hold_ms`` (20).  In place where ``audio`` is a float32 tensor on the model's device and
        ``out`` is None.  Returns ``(audio, min_gain)``: ``min_gain[b]`` is the smallest gain the limiter applied to the row."""
        from . import limiter as _limiter
        fs = int(self.sampling_rate if sample_rate is None else sample_rate)
        A, H = _limiter.window(fs, attack_ms, hold_ms)
        return self._engine.limit(audio, n_samples, ceiling, gains=gains, attack=A, hold=H, out=out)

    @torch.no_grad()
    def loudness_profile(self, audio, n_samples, sample_rate: Optional[int] = None, gate: str = "exact"):
        """Loudness over time (EBU Tech 3341's M, S and I) of every row of a ragged batch, one value per
        complete 100 ms segment: returns ``(M, S, I, M_max, S_max, I_end)`` -- momentary, short-term and running integrated
        loudness ``[B, F_max]`` float32 (NaN behind row b's ``n_samples[b] // h`` entries, -inf where a value does not exist
        yet), the rows' maxima and the integrated loudness of the whole row (``loudness``' value), all on the device.

        ``gate="histogram"`` (section 4s): ``I`` is the histogram gate's running level and ``I_end`` its value at the row's last
        complete segment (-inf where the row has none); ``M`` and ``S`` keep their bits."""
        fs = int(self.sampling_rate if sample_rate is None else sample_rate)
        if gate == "histogram":
            eng = self._engine
            seg, _ = eng.loudness_segments(audio, n_samples, fs)
            F = [int(n) // ((fs + 5) // 10) for n in n_samples]
            M, S, I, _, m_max, s_max, _ = eng.loudness_time_hist(seg, 0, F, fs, eng.loudness_hist_state(len(F)))
            i_end = torch.full((len(F),), float("-inf"), dtype=torch.float32, device=I.device)
            rows = [b for b, f in enumerate(F) if f]
            if rows:
                i_end[rows] = I[rows, [F[b] - 1 for b in rows]]
            return M, S, I, m_max, s_max, i_end
        if gate != "exact":
            raise ValueError(f'loudness_profile: gate is "exact" or "histogram", not {gate!r}')
        r = self._engine.loudness_level(audio, n_samples, fs)
        return r["M"], r["S"], r["I"], r["m_max"], r["s_max"], r["i_end"]

    @torch.no_grad()
    def loudness_range(self, audio, n_samples, sample_rate: Optional[int] = None):
        """The loudness range (EBU Tech 3342 from a histogram of 3 s windows in 0.1 LU bins) of every
        row of a ragged batch, in one call: returns ``(lra, I_h)``, both ``[B]`` float32 on the device -- the range in LU (0
        for a row with fewer than 3 s) and the histogram gate's integrated level over the row's complete 100 ms segments."""
        fs = int(self.sampling_rate if sample_rate is None else sample_rate)
        r = self._engine.loudness_range(audio, n_samples, fs)
        return r["lra"], r["i_hist"]

    @torch.no_grad()
    def level(self, audio, n_samples, target_lufs=-23.0, max_gain_db=12, max_cut_db=12, slew_db_per_s=3, initial_gain_db=0,
              sample_rate: Optional[int] = None, out=None):
        """The causal leveller: every row follows its own running integrated loudness towards
        ``target_lufs``, by at most ``slew_db_per_s``, between ``-max_cut_db`` and ``max_gain_db``, starting from
        ``initial_gain_db`` -- no look-ahead, no delay; the gain over a 100 ms segment depends on what came before it only.  The
        five values are scalars or one per row; a row whose target is None or NaN is left alone.  In place where ``audio`` is a
        float32 tensor on the model's device and ``out`` is None.  It does not clamp: put ``limit`` behind it.  Returns
        ``(wave, c_dB)``: ``c_dB`` ``[B, F_max]`` is the gain in dB reached at the end of every complete segment."""
        fs = int(self.sampling_rate if sample_rate is None else sample_rate)
        eng = self._engine
        params = eng.loudness_level_params(len(n_samples), target_lufs, max_gain_db, max_cut_db, slew_db_per_s, initial_gain_db)
        r = eng.loudness_level(audio, n_samples, fs, params, out=out)
        return r["out"], r["c_db"]

    @torch.no_grad()
    def denoiser_bias(self, sid, transform="dft"):
        """The denoiser's bias of speakers ``sid``, ``[len(sid), spec_channels]`` float32 on the device:
        the magnitude spectrum of the steady period the generator lays under its output for ``g = emb_g[sid]``.  Built on
        first use per speaker (one generator call on zeros for the speakers not seen yet), kept until ``load_state_dict``.
        ``transform``: ``"dft"`` or ``"fft"`` -- the table is keyed by ``(speaker, transform)``, so each
        path subtracts a bias made by its own transform."""
        if transform not in ("dft", "fft"):
            raise ValueError(f"denoiser_bias: transform must be 'dft' or 'fft', not {transform!r}")
        ids = [int(s) for s in (sid.tolist() if hasattr(sid, "tolist") else sid)]
        table = self.__dict__.setdefault("_denoiser_bias", {})
        new = sorted(s for s in set(ids) if (s, transform) not in table)
        kw = {} if transform == "dft" else {"transform": transform}      # (the default makes the call it always made)
        if new:
            if "emb_g.weight" not in self._state:
                raise RuntimeError("denoiser_bias: no weights loaded")
            rows = self._engine.denoise_bias(self._state["emb_g.weight"][new], **kw)
            for i, s in enumerate(new):
                table[(s, transform)] = rows[i]
        return torch.stack([table[(s, transform)] for s in ids])

    @torch.no_grad()
    def denoise(self, audio, n_samples, sid, strength=0.01, out=None, transform="dft"):
        """Subtract ``strength`` times the speaker's own bias (``denoiser_bias``) from the magnitude of every STFT frame of
        ``audio[b, :n_samples[b]]`` and return to audio: the post-filter of the denoisers shipped
        with WaveGlow and HiFi-GAN, with the steady state as the bias.  ``sid`` per row; ``strength`` a scalar or one per
        row, None / NaN leaves the row alone.  In place where ``audio`` is a float32 tensor on the model's device and ``out``
        is None.  Returns the audio.  ``transform="fft"``: both the call and the bias on the in-LDS FFT
        instead of the DFT products -- the same sums, other bits."""
        ids = [int(s) for s in (sid.tolist() if hasattr(sid, "tolist") else sid)]
        if transform == "dft":
            return self._engine.denoise(audio, n_samples, self.denoiser_bias(ids), strength, out=out)
        return self._engine.denoise(audio, n_samples, self.denoiser_bias(ids, transform), strength, out=out, transform=transform)

    @torch.no_grad()
    def denoise_stream(self, sid, strength=0.01, transform="dft"):
        """``denoise`` for audio that is still arriving: a ``vispeech_amd.denoiser.Stream`` with
        speaker ``sid``'s bias.  ``push(x)`` returns the denoised samples the pushes so far complete, ``push(x, final=True)``
        the rest; the pieces joined are the bits of ``denoise`` on the whole, at a delay of ``n_fft - hop`` to ``n_fft - 1``
        samples.  Several streams advance in one call through ``denoiser.push_rows``.  ``transform``: as in ``denoise``; the
        stream carries it and its bias is that transform's."""
        from . import denoiser
        return denoiser.Stream(self._engine, self.denoiser_bias([int(sid)], transform)[0], strength, transform=transform)

    def __call__(self, *a, **k):
        return self.forward(*a, **k)

    # ---------------------------------------------------------------- the hot path
    @torch.no_grad()
    def infer(self, phonemes, phonemes_lengths, sid=None, noise_scale=1, max_len=None, energy_control=None,
              pitch_control=None, duration_control=None, *, noise: Optional[torch.Tensor] = None,
              t_f: Optional[int] = None, noise_seed=None, noise_offset: int = 0, isolated: bool = False,
              row_controls: Optional[RowControls] = None):
        """Reference models.py:672-722.  ``noise`` (keyword-only, optional) replaces the
        ``torch.randn_like`` draw of models.py:718 so runs can be reproduced; without it the draw is
        ``torch.randn`` on the GPU (torch's generator, as in the reference) unless ``noise_seed`` is given: then the
        library draws it itself (``vsp_randn``, what a C caller gets) from stream element ``noise_offset`` on (a shard
        [lo, hi) of a global batch passes lo * inter_channels * t_f: same noise as unsharded).  ``t_f`` pads the frame
        axis to a global maximum for sharded batches (SURVEY gotcha G6).
        ``isolated`` (off by default: the reference's padded call, bit-compatible): every returned tensor, restricted to
        utterance b's own extent, is what the reference returns for a B = 1 call on that utterance's unpadded inputs --
        independent of the batch it shares -- and exactly 0 behind the extent.  ``noise_seed`` is then a sequence of B
        ints, one Philox key per utterance (a plain int raises: it would hand every utterance the same draw), and
        ``noise_offset`` is not read.
        ``row_controls`` (a ``RowControls``; needs ``isolated``, else ValueError): utterance b's own scales, noise scale and
        which of its controls are given.  ``duration_control`` / ``pitch_control`` / ``energy_control`` are then ``[B, Tp]``
        tensors read in the rows that are given them (None if no row is), the positional ``noise_scale`` is not read, and
        the returned ``duration`` is the one every row ended up with.  Returns
        ``(o, x_mask, (z, z_p, m_p, logs_p), duration, F0, energy)``."""
        eng = self._engine
        if not eng.ready:
            raise RuntimeError("weights not loaded: call load_state_dict first")
        if sid is None:
            raise ValueError("sid is required (the reference's EnergyPredictor needs g; n_speakers > 0)")
        B, Tp = phonemes.shape
        if row_controls is not None:
            if not isolated:
                raise ValueError("row_controls needs isolated=True: per-row values have no reference meaning in a padded batch")
            if len(row_controls) != B:
                raise ValueError(f"row_controls must have {B} rows, got {len(row_controls)}")
            for name, ctl, col in (("duration", duration_control, 0), ("pitch", pitch_control, 1), ("energy", energy_control, 2)):
                if ctl is not None and not isinstance(ctl, torch.Tensor):
                    raise ValueError(f"row_controls: {name}_control is a [B, Tp] tensor or None (the scales are in the table)")
                if ctl is None and bool(row_controls.given[:, col].any()):
                    raise ValueError(f"row_controls: a row is given {name} but {name}_control is None")

        def split(ctl):
            if isinstance(ctl, torch.Tensor):      # the reference's isinstance(.., torch.Tensor) branches
                return ctl, 1.0
            return None, 1.0 if ctl is None else float(ctl)

        d_t, d_s = split(duration_control)
        p_t, p_s = split(pitch_control)
        e_t, e_s = split(energy_control)
        # (the keyword is passed only when set: engine stand-ins of older callers and tests need not know it)
        iso = {"isolated": True} if isolated else {}
        if row_controls is not None:
            iso["row_controls"] = row_controls
        no_seed = noise_seed is None                     # the caller named no seed: torch draws the noise, in either mode
        noise_seed, seeds = eng._isolated_seeds(bool(isolated), noise, 0.0, noise_seed, B)
        enc = eng.encode(phonemes, phonemes_lengths, sid, d_t, p_t, e_t, d_s, p_s, e_s, **iso)
        # (a known padding: the second half's tensors are allocated while the GPU is still busy with the first)
        bufs = eng.decode_buffers(B, Tp, int(t_f), max_len) if t_f is not None and int(t_f) > 0 else None
        _, tf_local = eng.frame_lengths_host(enc["frame_lengths"])
        Tf = tf_local if t_f is None else max(int(t_f), tf_local)
        if Tf <= 0:
            raise ValueError("all durations are zero: nothing to synthesise")
        # (with a table: whether ANY row draws noise; the engine does not read the scalar then)
        ns = float(noise_scale) if row_controls is None else float(bool((row_controls.noise_scale != 0).any()))
        if noise is None and ns != 0.0 and no_seed:
            noise = torch.randn(B, self.dims.inter_channels, Tf, dtype=torch.float32, device=eng.device)
        dec = eng.decode(enc, Tf, noise, ns, max_len, noise_seed=seeds if isolated else (0 if noise_seed is None else int(noise_seed)),
                         bufs=bufs, noise_offset=int(noise_offset), **iso)
        duration = duration_control if d_t is not None and row_controls is None else enc["duration"].view(B, 1, Tp)
        return (dec["o"], dec["x_mask"], (dec["z"], dec["z_p"], dec["m_p"], dec["logs_p"]), duration, enc["F0"],
                enc["energy"])
