"""Thin torch-side driver of the C-ABI: owns a ``vsp_ctx``, hands torch CUDA tensors' pointers to
libvispeech_hip and keeps the caller-owned workspaces.  torch is plumbing here (device memory,
the current HIP stream); every arithmetic step runs in the library's kernels.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Mapping, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .schema import ModelDims


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _dev_f32(t, device) -> torch.Tensor:
    return torch.as_tensor(t).to(device=device, dtype=torch.float32).contiguous()


def _dev_i64(t, device) -> torch.Tensor:
    return torch.as_tensor(t).to(device=device, dtype=torch.int64).contiguous()


def _host_list(v, conv=int, n=None, name=None):
    """``v`` (a tensor, an array or any sequence) as a list on the host, every entry through ``conv``; with ``n`` a
    ``ValueError`` naming ``name`` unless it has ``n`` entries."""
    out = [conv(x) for x in (v.tolist() if hasattr(v, "tolist") else v)]
    if n is not None and len(out) != n:
        raise ValueError(f"{name} must be a scalar or have {n} entries")
    return out


def _nan_float(x) -> float:
    return float("nan") if x is None else float(x)


def _column(v, B: int, name: str, conv=_nan_float):
    """One value per row: a scalar (or None) for every row, or ``B`` values."""
    if v is None or np.ndim(v) == 0:
        return [conv(v)] * B
    return _host_list(v, conv, B, name)


class OutputHistory:
    """What a streamed request keeps between two ``Engine.generator_stream_rows_output`` calls: a [2, K] float32 device
    tensor -- the input samples the next outputs still need, K = ``vsp_output_history_samples`` -- and which side is
    current.  A call reads the current side, writes the other, then flips."""

    def __init__(self, K: int, device):
        self.buf = torch.empty((2, max(K, 0)), dtype=torch.float32, device=device)
        self.side = 0

    def pointers(self):
        """(hist_in, hist_out) as integers; None for both when K = 0 (the pass-through keeps nothing)."""
        if self.buf.shape[1] == 0:
            return None, None
        return self.buf[self.side].data_ptr(), self.buf[1 - self.side].data_ptr()

    def flip(self) -> None:
        self.side = 1 - self.side


class Engine:
    def __init__(self, dims: ModelDims, device: "torch.device | str | int" = "cuda:0"):
        self.lib = _lib.lib()                      # raises ImportError if the extension is absent
        self.dims = dims
        self.device = torch.device(device if not isinstance(device, int) else f"cuda:{device}")
        if self.device.type != "cuda":
            raise RuntimeError("vispeech_amd runs on an MI355X (torch device 'cuda'); there is no CPU path")
        self.cfg = _lib.make_config(dims)
        ctx = C.c_void_p()
        if dims.resblock_kind == 2:                 # (ResBlock1 contexts keep the plain vsp_create)
            rc = self.lib.vsp_create_ex(C.byref(self.cfg), 2, self.device.index or 0, C.byref(ctx))
        else:
            rc = self.lib.vsp_create(C.byref(self.cfg), self.device.index or 0, C.byref(ctx))
        self.ctx = ctx
        _lib.check(rc, ctx, "vsp_create")
        self._arena: Optional[torch.Tensor] = None
        self._ws: Dict[str, torch.Tensor] = {}
        self.ready = False

    def __del__(self):
        try:
            if getattr(self, "ctx", None):
                self.lib.vsp_destroy(self.ctx)
                self.ctx = None
        except Exception:  # pragma: no cover
            pass

    # ------------------------------------------------------------------ weights
    def set_weights(self, state_dict: Mapping[str, "np.ndarray | torch.Tensor"], strict: bool = True):
        """One ``vsp_set_weight[_typed]`` per tensor of a fresh load (``vsp_begin_weights`` first: nothing of an
        earlier load survives).  float16 / bfloat16 / float64 checkpoints and tensors that already live on the
        device are handed over as they are (``vsp_set_weight_typed``); everything else is float32 host data."""
        missing, unexpected = [], []
        _lib.check(self.lib.vsp_begin_weights(self.ctx), self.ctx, "vsp_begin_weights")
        self.ready = False
        for k, v in state_dict.items():
            if torch.is_tensor(v) and str(v.dtype).replace("torch.", "") in _lib.DTYPES and (v.is_cuda or v.dtype != torch.float32):
                t = v.detach().contiguous()
                if t.is_cuda:
                    # the library copies with a blocking hipMemcpy on the NULL stream, which does not order against
                    # torch's (possibly non-blocking) streams: whatever produced `t` must have finished first
                    torch.cuda.synchronize(t.device)
                shape = (C.c_int64 * max(t.dim(), 1))(*t.shape)
                rc = self.lib.vsp_set_weight_typed(self.ctx, k.encode(), C.c_void_p(t.data_ptr()), shape, t.dim(),
                                                   _lib.DTYPES[str(t.dtype).replace("torch.", "")], int(t.is_cuda))
                if rc == -4:
                    unexpected.append(k)
                    continue
                _lib.check(rc, self.ctx, f"vsp_set_weight_typed({k})")
                continue
            a = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
            a = np.ascontiguousarray(a, dtype=np.float32)
            shape = (C.c_int64 * max(a.ndim, 1))(*a.shape)
            rc = self.lib.vsp_set_weight(self.ctx, k.encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim)
            if rc == -4:
                unexpected.append(k)
                continue
            _lib.check(rc, self.ctx, f"vsp_set_weight({k})")
        n_missing = self.lib.vsp_missing_weights(self.ctx)
        if n_missing:
            missing.append(f"{n_missing} infer-path tensors")
        if strict and (unexpected or n_missing):
            raise RuntimeError(f"load_state_dict: unexpected keys {unexpected[:5]}..., missing {missing}")
        return missing, unexpected

    def arena_bytes(self) -> int:
        return int(self.lib.vsp_weight_arena_bytes(self.ctx))

    def _alloc_arena(self) -> torch.Tensor:
        if self._arena is None:
            self._arena = torch.empty(self.arena_bytes() // 4, dtype=torch.float32, device=self.device)
        return self._arena

    def finalize(self) -> torch.Tensor:
        """Fold, pack and upload; returns the packed arena as a flat float tensor (the object a
        multi-GPU run broadcasts from rank 0)."""
        arena = self._alloc_arena()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.vsp_finalize_weights(self.ctx, _ptr(arena)), self.ctx, "vsp_finalize_weights")
        self.ready = True
        return arena

    def adopt(self, arena: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Non-root rank: use an arena whose bytes arrive by broadcast.  The engine is NOT ready until
        ``commit_adopted()`` has checked the header of the received bytes."""
        if arena is None:
            arena = self._alloc_arena()
        assert arena.numel() * 4 == self.arena_bytes() and arena.is_cuda
        self._arena = arena
        _lib.check(self.lib.vsp_adopt_packed_weights(self.ctx, _ptr(arena)), self.ctx, "vsp_adopt_packed_weights")
        self.ready = False
        return arena

    def commit_adopted(self) -> None:
        """After the broadcast: read the arena header (magic, ABI, size, config hash, what rank 0 packed)."""
        with torch.cuda.device(self.device):
            _lib.check(self.lib.vsp_commit_adopted_weights(self.ctx, self._stream()), self.ctx,
                       "vsp_commit_adopted_weights")
        self.ready = True

    # ------------------------------------------------------------------ helpers
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _workspace(self, tag: str, nbytes: int) -> torch.Tensor:
        if nbytes < 0:
            _lib.check(int(nbytes), self.ctx, f"{tag} workspace size")
        w = self._ws.get(tag)
        if w is None or w.numel() < nbytes:
            self._ws[tag] = None
            w = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=self.device)
            self._ws[tag] = w
        return w

    def _f(self, *shape) -> torch.Tensor:
        return torch.empty(shape, dtype=torch.float32, device=self.device)

    # ------------------------------------------------------------------ isolated mode (vsp_set_isolated)
    def set_isolated(self, on: bool) -> None:
        """Sticky context state: every utterance of a batch as the reference computes it ALONE (include/vispeech_hip.h).
        ``encode`` / ``decode`` / ``infer_padded`` / ``voice_conversion`` set it from their ``isolated`` argument on every
        call, so a default call on a shared engine is never isolated by accident."""
        _lib.check(self.lib.vsp_set_isolated(self.ctx, int(bool(on))), self.ctx, "vsp_set_isolated")

    @property
    def isolated(self) -> bool:
        return bool(self.lib.vsp_get_isolated(self.ctx))

    def set_noise_seeds(self, seeds: Optional[Sequence[int]]) -> None:
        """``vsp_set_noise_seeds``: the Philox key of every utterance's own noise in isolated mode (None: forget them)."""
        seeds = [] if seeds is None else [int(x) & (2**64 - 1) for x in seeds]
        arr = (C.c_uint64 * max(len(seeds), 1))(*seeds)
        _lib.check(self.lib.vsp_set_noise_seeds(self.ctx, arr, len(seeds)), self.ctx, "vsp_set_noise_seeds")

    # ------------------------------------------------------------------ per-row controls (vsp_set_row_controls)
    def set_row_controls(self, rows) -> None:
        """``vsp_set_row_controls``: every utterance's own ``duration_scale`` / ``pitch_scale`` / ``energy_scale`` /
        ``noise_scale`` and which of its controls are given -- the arguments of the B = 1 reference call isolated mode
        reproduces for it (include/vispeech_hip.h).  ``rows``: an object with those four ``[B]`` float arrays and a
        ``[B, 3]`` bool ``given`` (duration, pitch, energy), e.g. ``models.RowControls``; None forgets the table.  Sticky
        context state: ``encode`` / ``decode`` / ``infer_padded`` set it from their ``row_controls`` argument on every
        call, so a call without one never runs with the table of an earlier call."""
        if rows is None:
            _lib.check(self.lib.vsp_set_row_controls(self.ctx, None, 0), self.ctx, "vsp_set_row_controls")
            return
        arr = self._row_control_array(rows)
        _lib.check(self.lib.vsp_set_row_controls(self.ctx, arr, len(arr)), self.ctx, "vsp_set_row_controls")

    @staticmethod
    def _row_control_array(rows):
        cols = [np.asarray(getattr(rows, k), dtype=np.float32).reshape(-1)
                for k in ("duration_scale", "pitch_scale", "energy_scale", "noise_scale")]
        given = np.asarray(rows.given, dtype=bool)
        B = len(cols[0])
        if B == 0 or any(len(c) != B for c in cols) or given.shape != (B, 3):
            raise ValueError("row controls: four [B] scale arrays and a [B, 3] bool `given`, B > 0")
        arr = (_lib.VspRowControl * B)()
        for b in range(B):
            bits = sum(bit for bit, on in zip((_lib.GIVEN_DURATION, _lib.GIVEN_PITCH, _lib.GIVEN_ENERGY), given[b]) if on)
            arr[b] = _lib.VspRowControl(float(cols[0][b]), float(cols[1][b]), float(cols[2][b]), float(cols[3][b]), bits)
        return arr

    @staticmethod
    def _check_row_controls(rows, isolated: bool, B: int, noise_scale):
        """The ``noise_scale`` the seed rules see: with a table, whether ANY row draws noise."""
        if rows is None:
            return noise_scale
        if not isolated:
            raise ValueError("row_controls needs isolated=True (per-row values have no reference meaning in a padded batch)")
        ns = np.asarray(rows.noise_scale, dtype=np.float32).reshape(-1)
        if len(ns) != B:
            raise ValueError(f"row_controls must have {B} rows, got {len(ns)}")
        return 1.0 if bool((ns != 0).any()) else 0.0

    @staticmethod
    def _isolated_seeds(isolated: bool, noise, noise_scale, noise_seed, B: int):
        """(scalar seed for the C call, per-utterance seeds or None).  Isolated mode keys the noise per utterance: a plain
        int would hand every utterance of the batch the same draw."""
        if not isolated:
            if noise_seed is not None and not isinstance(noise_seed, (int, np.integer)):
                raise ValueError("a sequence of noise seeds needs isolated=True")
            return noise_seed, None
        if noise_seed is None:
            if noise is None and float(noise_scale) != 0.0:
                raise ValueError("isolated=True: pass noise or one noise_seed per utterance (noise_scale != 0)")
            return 0, None
        if isinstance(noise_seed, (int, np.integer)):
            raise ValueError("isolated=True takes one noise_seed per utterance (a sequence of B ints), not a plain int")
        seeds = [int(x) for x in noise_seed]
        if len(seeds) != B:
            raise ValueError(f"noise_seed must have {B} entries, got {len(seeds)}")
        return 0, seeds

    def _noise_args(self, row_controls, isolated: bool, B: int, noise, noise_scale, noise_seed):
        """What ``decode`` and ``infer_padded`` check before anything else: the table against the batch, the seed rules, and
        that noise the library draws has a named seed.  Returns (noise_scale, scalar seed, per-utterance seeds or None)."""
        noise_scale = self._check_row_controls(row_controls, isolated, B, noise_scale)
        noise_seed, seeds = self._isolated_seeds(isolated, noise, noise_scale, noise_seed, B)
        if noise is None and float(noise_scale) != 0.0 and noise_seed is None:
            raise ValueError("pass noise or an explicit noise_seed (noise_scale != 0)")
        return noise_scale, 0 if noise_seed is None else noise_seed, seeds

    def _set_call_state(self, isolated: bool, seeds, row_controls, noise_offset: int) -> None:
        """The sticky context state ``vsp_decode`` / ``vsp_infer`` read, set from the call's own arguments."""
        self.set_isolated(isolated)
        if isolated:
            self.set_noise_seeds(seeds)
        self.set_row_controls(row_controls)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.vsp_set_noise_offset(self.ctx, int(noise_offset)), self.ctx, "vsp_set_noise_offset")

    def _hop(self, hop_length: Optional[int]) -> int:
        return int(self.dims.hop_length if hop_length is None else hop_length)

    def _need_output(self) -> None:
        if self.output_plan is None:
            raise RuntimeError("configure_output() first")

    # ------------------------------------------------------------------ the path
    def encode(self, phonemes, lengths, sid, duration_ctl=None, pitch_ctl=None, energy_ctl=None,
               duration_scale=1.0, pitch_scale=1.0, energy_scale=1.0, isolated: bool = False,
               row_controls=None) -> Dict[str, torch.Tensor]:
        """``row_controls`` (``set_row_controls``; needs ``isolated``): per-row scales and given bits; the three scalar
        scales are then not read, and a ``*_ctl`` tensor is read in the rows that are given it only."""
        d = self.dims
        ph = _dev_i64(phonemes, self.device)
        ln = _dev_i64(lengths, self.device)
        sd = _dev_i64(sid, self.device)
        B, Tp = ph.shape
        self._check_row_controls(row_controls, isolated, B, 0.0)
        dc = None if duration_ctl is None else _dev_f32(duration_ctl, self.device).reshape(B, -1)
        pc = None if pitch_ctl is None else _dev_f32(pitch_ctl, self.device).reshape(B, -1)
        ec = None if energy_ctl is None else _dev_f32(energy_ctl, self.device).reshape(B, -1)
        for name, t in (("duration", dc), ("pitch", pc), ("energy", ec)):
            if t is not None and t.shape[1] != Tp:
                raise ValueError(f"{name}_control must have {Tp} entries per utterance, got {t.shape[1]}")
        out = dict(x_var=self._f(B, d.hidden_channels, Tp), g=self._f(B, d.gin_channels),
                   duration=self._f(B, Tp), F0=self._f(B, Tp), energy=self._f(B, Tp),
                   frame_lengths=torch.empty(B, dtype=torch.int64, device=self.device),
                   cum_dur=torch.empty(B, Tp, dtype=torch.int32, device=self.device))
        ws = self._workspace("encode", self.lib.vsp_encode_workspace_bytes(self.ctx, B, Tp))
        self.set_isolated(isolated)
        self.set_row_controls(row_controls)
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_encode(self.ctx, self._stream(), B, Tp, _ptr(ph), _ptr(ln), _ptr(sd), _ptr(dc), _ptr(pc),
                                     _ptr(ec), float(duration_scale), float(pitch_scale), float(energy_scale),
                                     _ptr(out["x_var"]), _ptr(out["g"]), _ptr(out["duration"]), _ptr(out["F0"]),
                                     _ptr(out["energy"]), _ptr(out["frame_lengths"]), _ptr(out["cum_dur"]), _ptr(ws),
                                     ws.numel())
        _lib.check(rc, self.ctx, "vsp_encode")
        out["_keep"] = (ph, ln, sd, dc, pc, ec)
        return out

    def frame_lengths_host(self, frame_lengths: torch.Tensor):
        B = frame_lengths.numel()
        host = (C.c_int64 * B)()
        mx = C.c_int64()
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_frame_lengths_host(self.ctx, self._stream(), B, _ptr(frame_lengths), host, C.byref(mx))
        _lib.check(rc, self.ctx, "vsp_frame_lengths_host")
        self.check_numerics(sync=False)       # (free: a pinned word; reports what has completed, e.g. the previous call)
        return list(host), int(mx.value)

    # ------------------------------------------------------------------ numeric-range status (vsp_status)
    def status(self, clear: bool = False) -> int:
        """The context's sticky VSP_FLAG_* word (no synchronisation: launches that have completed)."""
        flags = C.c_uint(0)
        _lib.check(self.lib.vsp_status(self.ctx, C.byref(flags), int(clear)), self.ctx, "vsp_status")
        return int(flags.value)

    def check_numerics(self, sync: bool = True) -> None:
        """Raise ``VspError`` if a kernel has reported non-finite values since the last check -- an activation left the
        range the split-f16 matrix kernels represent (include/vispeech_hip.h, vsp_status) or an input was not finite.
        ``sync=True`` waits for the device first, so that the answer covers everything enqueued so far."""
        if sync:
            torch.cuda.synchronize(self.device)
        f = self.status(clear=True)
        if f:
            what = [n for b, n in ((_lib.FLAG_NONFINITE_LATENT, "z_p (phoneme- / frame-rate stages)"),
                                   (_lib.FLAG_NONFINITE_WAVE, "the waveform (flow / generator)")) if f & b]
            raise _lib.VspError("non-finite values in " + " and ".join(what) + ": an activation beyond the split-f16 range "
                                "(|x| > 65504; inside the generator 65504 / 2^VSP_ACT_SCALE_LOG2) or a non-finite input; "
                                "VSP_GENERATOR=f32 / VSP_FRAME=f32 select the f32 matrix kernels, which have no such limit")

    def decode_buffers(self, B: int, Tp: int, Tf: int, max_len: Optional[int] = None):
        """Output tensors and workspace of ``decode`` for a padded frame count ``Tf``.  A caller that knows ``Tf`` before
        the frame counts are read back (a sharded batch's global padding, ``t_f``) allocates them while the GPU is still
        busy with ``encode``: the host work between the two halves is then the read itself."""
        d = self.dims
        inter = d.inter_channels
        if max_len is not None and int(max_len) < 0:
            raise ValueError("max_len must be >= 0 (None = no truncation)")   # the C side reads < 0 as "no limit"
        Tdec = Tf if max_len is None else min(Tf, int(max_len))
        o_buf = self._f(B, 1, max(Tdec * d.total_upsample, 1))      # (never a null pointer: max_len = 0 skips the vocoder)
        out = dict(o=o_buf[:, :, :Tdec * d.total_upsample] if Tdec * d.total_upsample != o_buf.shape[2] else o_buf,
                   x_mask=torch.empty(B, 1, Tf, dtype=torch.uint8, device=self.device),
                   z=self._f(B, inter, Tf), z_p=self._f(B, inter, Tf), m_p=self._f(B, inter, Tf),
                   logs_p=self._f(B, inter, Tf))
        ws = self._workspace("decode", self.lib.vsp_decode_workspace_bytes(self.ctx, B, Tp, Tf))
        return dict(Tf=int(Tf), Tdec=Tdec, o_buf=o_buf, out=out, ws=ws, max_len=max_len)

    def decode(self, enc: Mapping[str, torch.Tensor], Tf: int, noise: Optional[torch.Tensor], noise_scale: float,
               max_len: Optional[int] = None, noise_seed=None, bufs=None,
               noise_offset: int = 0, isolated: bool = False, row_controls=None) -> Dict[str, torch.Tensor]:
        """``noise`` None with ``noise_scale`` != 0: the library draws it on the device -- elements ``noise_offset`` ..
        of ``vsp_randn(noise_seed)``; the caller must then name the seed (a silent default would hand out the same
        "random" sample on every call).  ``noise_offset``: a shard [lo, hi) of a global batch passes lo * inter * Tf so
        that its utterances get the noise they would get unsharded.
        ``bufs``: a ``decode_buffers`` result for the same ``Tf`` / ``max_len`` (else allocated here).
        ``isolated``: every utterance as the reference computes it alone; ``noise_seed`` is then a sequence of B ints, one
        key per utterance (``vsp_set_noise_seeds``), and ``noise_offset`` is not read.
        ``row_controls`` (``set_row_controls``; needs ``isolated``): row b's own ``noise_scale``; the argument is not read."""
        B, _, Tp = enc["x_var"].shape
        noise_scale, noise_seed, seeds = self._noise_args(row_controls, isolated, B, noise, noise_scale, noise_seed)
        d = self.dims
        inter = d.inter_channels
        if bufs is None or bufs["Tf"] != int(Tf) or bufs["max_len"] != max_len:
            bufs = self.decode_buffers(B, Tp, Tf, max_len)
        Tdec, o_buf, out, ws = bufs["Tdec"], bufs["o_buf"], bufs["out"], bufs["ws"]
        if noise is not None:
            noise = _dev_f32(noise, self.device)
            if tuple(noise.shape) != (B, inter, Tf):
                raise ValueError(f"noise must be [{B},{inter},{Tf}], got {tuple(noise.shape)}")
        self._set_call_state(isolated, seeds, row_controls, noise_offset)
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_decode(self.ctx, self._stream(), B, Tp, Tf, -1 if max_len is None else Tdec,
                                     _ptr(enc["x_var"]), _ptr(enc["g"]), _ptr(enc["cum_dur"]),
                                     _ptr(enc["frame_lengths"]), _ptr(noise), int(noise_seed) & (2**64 - 1),
                                     float(noise_scale), _ptr(o_buf),
                                     _ptr(out["x_mask"]), _ptr(out["z"]), _ptr(out["z_p"]), _ptr(out["m_p"]),
                                     _ptr(out["logs_p"]), _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_decode")
        out["x_mask"] = out["x_mask"].view(torch.bool) if hasattr(torch, "bool") else out["x_mask"]
        return out

    # ------------------------------------------------------------------ per-stage entry points
    def infer_padded(self, phonemes, lengths, sid, tf_pad: int, noise, noise_scale: float = 1.0, max_len=None,
                     duration_ctl=None, pitch_ctl=None, energy_ctl=None, duration_scale: float = 1.0,
                     pitch_scale: float = 1.0, energy_scale: float = 1.0, noise_seed=None,
                     noise_offset: int = 0, isolated: bool = False, row_controls=None) -> Dict[str, torch.Tensor]:
        """``vsp_infer``: the whole path in ONE call and without the host read of the frame counts, for
        callers that know an upper bound ``tf_pad`` of the frame count (supplied durations / fixed max_len).
        ``noise`` None with ``noise_scale`` != 0 needs an explicit ``noise_seed`` (see ``decode``, also for ``isolated``
        and ``row_controls``, which replaces the four scalar scales)."""
        ph = _dev_i64(phonemes, self.device)
        B, Tp = ph.shape
        noise_scale, noise_seed, seeds = self._noise_args(row_controls, isolated, B, noise, noise_scale, noise_seed)
        ln, sd = _dev_i64(lengths, self.device), _dev_i64(sid, self.device)
        ctl = [None if t is None else _dev_f32(t, self.device).reshape(B, Tp) for t in (duration_ctl, pitch_ctl, energy_ctl)]
        Tf = int(tf_pad)
        if max_len is not None and int(max_len) < 0:
            raise ValueError("max_len must be >= 0 (None = no truncation)")
        Tdec = Tf if max_len is None else min(Tf, int(max_len))
        inter = self.dims.inter_channels
        ns = float(noise_scale)
        nz = None if noise is None else _dev_f32(noise, self.device)
        if nz is not None and tuple(nz.shape) != (B, inter, Tf):
            raise ValueError("noise must be [B, inter_channels, tf_pad]")
        o = self._f(B, 1, max(Tdec, 0) * self.dims.total_upsample)
        z, z_p, m_p, logs_p = (self._f(B, inter, Tf) for _ in range(4))
        x_mask = torch.empty((B, 1, Tf), dtype=torch.uint8, device=self.device)
        dur, f0, en = (self._f(B, Tp) for _ in range(3))
        fl = torch.empty(B, dtype=torch.int64, device=self.device)
        ws = self._workspace("infer", self.lib.vsp_infer_workspace_bytes(self.ctx, B, Tp, Tf))
        self._set_call_state(isolated, seeds, row_controls, noise_offset)
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_infer(self.ctx, self._stream(), B, Tp, Tf, -1 if max_len is None else Tdec,
                                    _ptr(ph), _ptr(ln), _ptr(sd), _ptr(ctl[0]), _ptr(ctl[1]), _ptr(ctl[2]),
                                    float(duration_scale), float(pitch_scale), float(energy_scale), _ptr(nz),
                                    int(noise_seed) & (2**64 - 1), ns,
                                    _ptr(o), _ptr(x_mask), _ptr(z), _ptr(z_p), _ptr(m_p), _ptr(logs_p), _ptr(dur),
                                    _ptr(f0), _ptr(en), _ptr(fl), _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_infer")
        return dict(o=o, x_mask=x_mask.view(torch.bool), z=z, z_p=z_p, m_p=m_p, logs_p=logs_p, duration=dur, F0=f0,
                    energy=en, frame_lengths=fl)

    def attention(self, which: int, layer: int, qkv, lengths) -> torch.Tensor:
        """``vsp_attention``: relative-position attention of one encoder layer on ready q|k|v [B,3H,T]."""
        qkv = _dev_f32(qkv, self.device)
        ln = _dev_i64(lengths, self.device)
        B, C3, T = qkv.shape
        out = self._f(B, C3 // 3, T)
        ws = self._workspace("attention", self.lib.vsp_attention_workspace_bytes(self.ctx, B, T))
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_attention(self.ctx, self._stream(), which, layer, B, T, _ptr(qkv), _ptr(ln), _ptr(out),
                                        _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_attention")
        return out

    def wn_layer(self, which: int, layer: int, x, g, lengths, skip=None):
        """``vsp_wn_layer``: one layer of modules.WN.forward (reference modules.py:148-176) of flow ``which``
        (-1: the posterior encoder's WN).  Returns (x_new, skip_new); ``skip`` None starts the skip sum."""
        x = _dev_f32(x, self.device).clone()
        B, h, T = x.shape
        g = _dev_f32(g, self.device).reshape(B, -1)
        ln = _dev_i64(lengths, self.device)
        acc = skip is not None
        sk = _dev_f32(skip, self.device).clone() if acc else self._f(B, h, T)
        ws = self._workspace("wn_layer", self.lib.vsp_wn_layer_workspace_bytes(self.ctx, which, B, T))
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_wn_layer(self.ctx, self._stream(), which, layer, B, T, _ptr(x), _ptr(g), _ptr(ln), _ptr(sk),
                                       int(acc), _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_wn_layer")
        return x, sk

    def randn(self, seed: int, *shape, first: int = 0) -> torch.Tensor:
        """``vsp_randn_at``: elements ``first`` .. of the library's own standard-normal stream (Philox4x32-10 keyed by
        ``seed``)."""
        out = self._f(*shape)
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_randn_at(self._stream(), int(seed) & (2**64 - 1), int(first), out.numel(), _ptr(out))
        _lib.check(rc, self.ctx, "vsp_randn_at")
        return out

    def encoder(self, which: int, x, lengths) -> torch.Tensor:
        x = _dev_f32(x, self.device)
        ln = _dev_i64(lengths, self.device)
        B, h, T = x.shape
        y = self._f(B, h, T)
        ws = self._workspace("encoder", self.lib.vsp_encoder_workspace_bytes(self.ctx, B, T))
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_encoder(self.ctx, self._stream(), which, B, T, _ptr(x), _ptr(ln), _ptr(y), _ptr(ws),
                                      ws.numel())
        _lib.check(rc, self.ctx, "vsp_encoder")
        return y

    def length_regulate(self, x, cum_dur, Tf: int) -> torch.Tensor:
        x = _dev_f32(x, self.device)
        cum = torch.as_tensor(cum_dur).to(device=self.device, dtype=torch.int32).contiguous()
        B, Cc, Tp = x.shape
        y = self._f(B, Cc, Tf)
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_length_regulate(self.ctx, self._stream(), B, Cc, Tp, Tf, _ptr(x), _ptr(cum), _ptr(y))
        _lib.check(rc, self.ctx, "vsp_length_regulate")
        return y

    def flow_reverse(self, z_p, g, frame_lengths) -> torch.Tensor:
        z_p = _dev_f32(z_p, self.device)
        g = _dev_f32(g, self.device).reshape(z_p.shape[0], -1)
        fl = _dev_i64(frame_lengths, self.device)
        B, _, Tf = z_p.shape
        z = torch.empty_like(z_p)
        ws = self._workspace("flow", self.lib.vsp_flow_workspace_bytes(self.ctx, B, Tf))
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_flow_reverse(self.ctx, self._stream(), B, Tf, _ptr(z_p), _ptr(g), _ptr(fl), _ptr(z),
                                           _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_flow_reverse")
        return z

    def flow_forward(self, z, g, frame_lengths) -> torch.Tensor:
        """ResidualCouplingBlock.forward(reverse=False) (reference models.py:202-206)."""
        z = _dev_f32(z, self.device)
        g = _dev_f32(g, self.device).reshape(z.shape[0], -1)
        fl = _dev_i64(frame_lengths, self.device)
        B, _, Tf = z.shape
        z_p = torch.empty_like(z)
        ws = self._workspace("flow", self.lib.vsp_flow_workspace_bytes(self.ctx, B, Tf))
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_flow_forward(self.ctx, self._stream(), B, Tf, _ptr(z), _ptr(g), _ptr(fl), _ptr(z_p),
                                           _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_flow_forward")
        return z_p

    # ------------------------------------------------------------------ voice conversion
    @property
    def has_voice_conversion(self) -> bool:
        return bool(self.lib.vsp_has_voice_conversion(self.ctx))

    def spectrogram(self, audio, hop_length: Optional[int] = None) -> torch.Tensor:
        """``mel_processing.spectrogram_torch`` (reference mel_processing.py:50-69): audio [B, L] in [-1, 1] ->
        linear magnitude spectrogram [B, spec_channels, L // hop] (n_fft = win = 2 * (spec_channels - 1))."""
        a = _dev_f32(audio, self.device)
        if a.dim() != 2:
            raise ValueError("audio must be [B, L]")
        hop = self._hop(hop_length)
        B, L = a.shape
        T = int(self.lib.vsp_spectrogram_frames(self.ctx, L, hop))
        if T <= 0:
            raise ValueError("signal too short for the reflect padding of the spectrogram")
        spec = self._f(B, self.dims.spec_channels, T)
        ws = self._workspace("spectrogram", self.lib.vsp_spectrogram_workspace_bytes(self.ctx, B, L, hop))
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_spectrogram(self.ctx, self._stream(), B, L, hop, _ptr(a), _ptr(spec), _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_spectrogram")
        return spec

    def spec_to_mel(self, spec, n_mels: int, sampling_rate: int, fmin: float = 0.0, fmax: Optional[float] = None) -> torch.Tensor:
        """``mel_processing.spec_to_mel_torch`` (reference mel_processing.py:73-82): linear magnitude spectrogram
        [B, n_fft // 2 + 1, T] -> log-mel [B, n_mels, T] (Slaney basis as ``librosa.filters.mel``, log(clamp(x, 1e-5)))."""
        sp = _dev_f32(spec, self.device)
        if sp.dim() != 3 or sp.shape[1] < 2:
            raise ValueError("spec must be [B, n_fft // 2 + 1, T]")
        B, nf, T = sp.shape
        mel = self._f(B, int(n_mels), T)
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_spec_to_mel(self._stream(), B, T, 2 * (nf - 1), int(n_mels), int(sampling_rate), float(fmin),
                                          0.0 if fmax is None else float(fmax), _ptr(sp), _ptr(mel))
        _lib.check(rc, self.ctx, "vsp_spec_to_mel")
        return mel

    def mel_spectrogram(self, audio, n_mels: int, sampling_rate: int, fmin: float = 0.0, fmax: Optional[float] = None,
                        hop_length: Optional[int] = None) -> torch.Tensor:
        """``mel_processing.mel_spectrogram_torch`` (reference mel_processing.py:85-112) on the GPU: spectrogram, then
        the mel projection and dynamic range compression."""
        return self.spec_to_mel(self.spectrogram(audio, hop_length), n_mels, sampling_rate, fmin, fmax)

    def posterior_encoder(self, y, y_lengths, g, noise):
        """PosteriorEncoder.forward (reference models.py:233-241) -> (z, m, logs)."""
        y = _dev_f32(y, self.device)
        g = _dev_f32(g, self.device).reshape(y.shape[0], -1)
        yl = _dev_i64(y_lengths, self.device)
        B, _, T = y.shape
        noise = _dev_f32(noise, self.device)
        z, m, logs = (self._f(B, self.dims.inter_channels, T) for _ in range(3))
        ws = self._workspace("posterior", self.lib.vsp_posterior_workspace_bytes(self.ctx, B, T))
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_posterior_encoder(self.ctx, self._stream(), B, T, _ptr(y), _ptr(yl), _ptr(g), _ptr(noise),
                                                _ptr(z), _ptr(m), _ptr(logs), _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_posterior_encoder")
        return z, m, logs

    def voice_conversion(self, y, y_lengths, sid_src, sid_tgt, noise, isolated: bool = False) -> Dict[str, torch.Tensor]:
        """SynthesizerTrn.voice_conversion (reference models.py:724-732); ``noise`` [B,inter,T] is the
        ``torch.randn_like`` of the posterior encoder (models.py:240)."""
        y = _dev_f32(y, self.device)
        B, S, T = y.shape
        if S != self.dims.spec_channels:
            raise ValueError(f"y has {S} channels, the model's spec_channels is {self.dims.spec_channels}")
        yl, ss, st = (_dev_i64(t, self.device) for t in (y_lengths, sid_src, sid_tgt))
        noise = _dev_f32(noise, self.device)
        if tuple(noise.shape) != (B, self.dims.inter_channels, T):
            raise ValueError("noise must be [B, inter_channels, T]")
        inter = self.dims.inter_channels
        o = self._f(B, 1, T * self.dims.total_upsample)
        z, z_p, z_hat, m_q, logs_q = (self._f(B, inter, T) for _ in range(5))
        y_mask = torch.empty((B, 1, T), dtype=torch.uint8, device=self.device)
        ws = self._workspace("vc", self.lib.vsp_voice_conversion_workspace_bytes(self.ctx, B, T))
        self.set_isolated(isolated)
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_voice_conversion(self.ctx, self._stream(), B, T, _ptr(y), _ptr(yl), _ptr(ss), _ptr(st),
                                               _ptr(noise), _ptr(o), _ptr(y_mask), _ptr(z), _ptr(z_p), _ptr(z_hat),
                                               _ptr(m_q), _ptr(logs_q), _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_voice_conversion")
        return dict(o_hat=o, y_mask=y_mask, z=z, z_p=z_p, z_hat=z_hat, m_q=m_q, logs_q=logs_q)

    # ------------------------------------------------------------------ conversion from audio (ragged front end)
    def convert_frames(self, n_samples: int, hop_length: Optional[int] = None) -> int:
        """``vsp_convert_frames``: frames of a recording of ``n_samples`` samples (0: too short for a frame).  Host only."""
        hop = self._hop(hop_length)
        T = int(self.lib.vsp_convert_frames(self.ctx, int(n_samples), hop))
        if T < 0:
            _lib.check(T, self.ctx, "vsp_convert_frames")
        return T

    def _ragged_audio(self, audio, n_samples, hop_length):
        """(audio [B, stride] on the device, n_samples on the device and as host ints, L_max, hop, T_max, frames per row).
        The host knows every length: the frame counts come from ``vsp_convert_frames``, nothing is read back."""
        a = _dev_f32(audio, self.device)
        if a.dim() != 2:
            raise ValueError("audio must be [B, L] (rows padded to a common length)")
        B, stride = a.shape
        n_host = _host_list(n_samples)
        if len(n_host) != B:
            raise ValueError(f"n_samples must have {B} entries")
        if any(x < 0 or x > stride for x in n_host):
            raise ValueError("0 <= n_samples[b] <= audio.shape[1]")
        hop = self._hop(hop_length)
        frames = [self.convert_frames(x, hop) for x in n_host]
        L_max = max(n_host)
        T = max(frames)
        if T <= 0:
            raise ValueError("every recording is too short for one spectrogram frame")
        return a, _dev_i64(n_host, self.device), n_host, L_max, hop, T, frames

    def spectrogram_ragged(self, audio, n_samples, hop_length: Optional[int] = None):
        """``vsp_spectrogram_ragged``: recordings of different lengths in one padded ``audio`` [B, L]; row b is
        ``audio[b, :n_samples[b]]``.  Returns (spec [B, spec_channels, T_max], frames [B] int64 on the device): row b's first
        ``frames[b]`` columns are ``spectrogram(audio[b:b+1, :n_samples[b]])``, the rest is 0; samples behind a row's end
        are never read."""
        a, n_dev, _, L_max, hop, T, _ = self._ragged_audio(audio, n_samples, hop_length)
        B = a.shape[0]
        spec = self._f(B, self.dims.spec_channels, T)
        frames = torch.empty(B, dtype=torch.int64, device=self.device)
        ws = self._workspace("spectrogram", self.lib.vsp_spectrogram_ragged_workspace_bytes(self.ctx, B, L_max, hop))
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_spectrogram_ragged(self.ctx, self._stream(), B, L_max, hop, _ptr(a), a.shape[1], _ptr(n_dev),
                                                 _ptr(spec), _ptr(frames), _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_spectrogram_ragged")
        return spec, frames

    def convert_latent(self, audio, n_samples, sid_src, sid_tgt, noise=None, noise_seed=None, noise_scale: float = 1.0,
                       hop_length: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """``vsp_convert_latent``: audio to the converted latent -- ragged spectrogram, posterior encoder and forward flow
        with the source speaker, reverse flow with the target speaker; the generator does not run (the counterpart of
        ``decode(max_len=0)``).  Row b is what ``voice_conversion`` computes up to ``z_hat`` for the recording alone.
        ``noise`` [B, inter, T_max]: row b uses ``noise[b, :, :frames[b]]``; None: the library draws row b's tensor from the
        Philox stream keyed ``noise_seed[b]`` (a list of B ints).  ``noise_scale`` multiplies the posterior's noise (1.0: the
        reference; 0: nothing is drawn or read).  Returns ``z_hat, g, frames, y_mask, z, z_p`` (device) and ``frames_host``."""
        a, n_dev, _, L_max, hop, T, frames_host = self._ragged_audio(audio, n_samples, hop_length)
        B = a.shape[0]
        if isinstance(noise_seed, (int, np.integer)):
            raise ValueError("convert_latent takes one noise_seed per recording (a sequence of B ints), not a plain int")
        seeds = None if noise_seed is None else [int(x) for x in noise_seed]
        if seeds is not None and len(seeds) != B:
            raise ValueError(f"noise_seed must have {B} entries, got {len(seeds)}")
        ss, st = _dev_i64(sid_src, self.device).reshape(-1), _dev_i64(sid_tgt, self.device).reshape(-1)
        if ss.numel() != B or st.numel() != B:
            raise ValueError(f"sid_src and sid_tgt must have {B} entries")
        inter = self.dims.inter_channels
        if noise is not None:
            noise = _dev_f32(noise, self.device)
            if tuple(noise.shape) != (B, inter, T):
                raise ValueError(f"noise must be [{B},{inter},{T}], got {tuple(noise.shape)}")
        z, z_p, z_hat = (self._f(B, inter, T) for _ in range(3))
        g = self._f(B, self.dims.gin_channels)
        frames = torch.empty(B, dtype=torch.int64, device=self.device)
        y_mask = torch.empty((B, 1, T), dtype=torch.uint8, device=self.device)
        ws = self._workspace("convert", self.lib.vsp_convert_latent_workspace_bytes(self.ctx, B, L_max, hop))
        if noise is None and float(noise_scale) != 0.0:   # (scale 0 draws nothing: the context's seeds stay as they are)
            self.set_noise_seeds(seeds)      # (None forgets them: the library then refuses to draw, VSP_ERR_STATE)
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_convert_latent(self.ctx, self._stream(), B, L_max, hop, _ptr(a), a.shape[1], _ptr(n_dev),
                                             _ptr(ss), _ptr(st), _ptr(noise), float(noise_scale), _ptr(z_hat), _ptr(g),
                                             _ptr(frames), _ptr(y_mask), _ptr(z), _ptr(z_p), _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_convert_latent")
        return dict(z_hat=z_hat, g=g, frames=frames, y_mask=y_mask, z=z, z_p=z_p, frames_host=frames_host)

    def convert(self, audio, n_samples, sid_src, sid_tgt, noise=None, noise_seed=None, noise_scale: float = 1.0,
                hop_length: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """``convert_latent`` followed by ``generator_ragged``: ``o_hat`` [B, 1, T_max * up], row b the
        ``frames[b] * up`` samples of the recording converted alone and 0 behind; plus what ``convert_latent`` returns."""
        r = self.convert_latent(audio, n_samples, sid_src, sid_tgt, noise, noise_seed, noise_scale, hop_length)
        r["o_hat"] = self.generator_ragged(r["z_hat"], r["g"], r["frames"])
        return r

    @property
    def convert_halo(self) -> int:
        """``vsp_convert_halo_frames``: frames of spectrogram a frame of ``z_hat`` depends on, on each side."""
        return int(self.lib.vsp_convert_halo_frames(self.ctx))

    def convert_window_plan(self, n_known: int, closed: bool, e0: int, e1: int, hop_length: Optional[int] = None):
        """``vsp_convert_window_plan`` (host only) with this model's geometry and halo: ``(ready, w0, w1, s_lo, s_hi)`` of the
        window that delivers frames ``[e0, e1)`` (``vispeech_amd.schema.convert_window_plan`` is its pure-Python twin)."""
        hop = self._hop(hop_length)
        w0, w1, lo, hi = C.c_int(), C.c_int(), C.c_int64(), C.c_int64()
        rc = int(self.lib.vsp_convert_window_plan(2 * (self.dims.spec_channels - 1), hop, self.convert_halo, int(n_known),
                                                  int(bool(closed)), int(e0), int(e1), C.byref(w0), C.byref(w1), C.byref(lo),
                                                  C.byref(hi)))
        if rc < 0:
            _lib.check(rc, None, "vsp_convert_window_plan")
        return bool(rc), int(w0.value), int(w1.value), int(lo.value), int(hi.value)

    def convert_stream_rows(self, rows, span_frames: int, hop_length: Optional[int] = None):
        """``vsp_convert_stream_rows``: up to 64 windows of recordings that may still be arriving, in ONE set of launches.
        ``rows`` is a sequence of ``(audio, first_sample, n_known, closed, e0, e1, sid_src, sid_tgt, seed, noise_scale)``:
        ``audio`` a 1-D float32 tensor on the device that holds the samples ``[first_sample, n_known)`` of the recording,
        and the frames ``[e0, e1)`` to deliver, ``e1 - e0 <= span_frames``; every row must be ready
        (``convert_window_plan``).  Returns ``(z_hat [B, inter, span_frames], g [B, gin])``: row b's first ``e1 - e0``
        columns are those frames of ``z_hat`` of the WHOLE recording converted alone, zeros behind; ``g`` is
        ``emb_g(sid_tgt)``.  The noise of (channel c, frame t) is ``noise_scale`` times element ``t * inter + c`` of the
        Philox stream keyed ``seed`` -- ``randn(seed, T, inter).T``, NOT the ``[inter, T]`` layout of ``convert_latent``."""
        rows = list(rows)
        B = len(rows)
        if not 1 <= B <= _lib.STREAM_ROWS_MAX:
            raise ValueError(f"1 .. {_lib.STREAM_ROWS_MAX} rows per call, got {B}")
        hop = self._hop(hop_length)
        span_frames = int(span_frames)
        arr = (_lib.VspConvertRow * B)()
        keep = []
        for r, (audio, first, n_known, closed, e0, e1, sid_src, sid_tgt, seed, noise_scale) in zip(arr, rows):
            if (not torch.is_tensor(audio) or audio.dtype != torch.float32 or audio.device != self.device or audio.dim() != 1
                    or not audio.is_contiguous() or audio.numel() < int(n_known) - int(first)):
                raise ValueError("a row's audio must be a contiguous 1-D float32 tensor on the engine's device that holds "
                                 "the samples [first_sample, n_known)")
            keep.append(audio)
            r.audio, r.first_sample, r.n_known = audio.data_ptr(), int(first), int(n_known)
            r.closed, r.e0, r.e1 = int(bool(closed)), int(e0), int(e1)
            r.sid_src, r.sid_tgt, r.seed, r.noise_scale = int(sid_src), int(sid_tgt), int(seed), float(noise_scale)
        z_hat = self._f(B, self.dims.inter_channels, max(span_frames, 1))
        g = self._f(B, self.dims.gin_channels)
        ws = self._workspace("convert_stream_rows", self.lib.vsp_convert_stream_rows_workspace_bytes(self.ctx, B, span_frames))
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_convert_stream_rows(self.ctx, self._stream(), B, hop, arr, span_frames, _ptr(z_hat), _ptr(g),
                                                  _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_convert_stream_rows")
        return z_hat, g

    def generator(self, z, g) -> torch.Tensor:
        z = _dev_f32(z, self.device)
        g = _dev_f32(g, self.device).reshape(z.shape[0], -1)
        B, _, T = z.shape
        o = self._f(B, 1, T * self.dims.total_upsample)
        ws = self._workspace("generator", self.lib.vsp_generator_workspace_bytes(self.ctx, B, T))
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_generator(self.ctx, self._stream(), B, T, _ptr(z), _ptr(g), _ptr(o), _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_generator")
        return o

    def generator_ragged(self, z, g, lengths) -> torch.Tensor:
        """``vsp_generator_ragged``: the generator with per-utterance ends -- utterance b's first ``lengths[b]`` frames of
        waveform are what ``generator(z[b:b+1, :, :lengths[b]], g[b:b+1])`` returns, the rest of its row is 0."""
        z = _dev_f32(z, self.device)
        g = _dev_f32(g, self.device).reshape(z.shape[0], -1)
        ln = _dev_i64(lengths, self.device)
        B, _, T = z.shape
        if ln.numel() != B:
            raise ValueError(f"lengths must have {B} entries")
        o = self._f(B, 1, T * self.dims.total_upsample)
        ws = self._workspace("generator", self.lib.vsp_generator_workspace_bytes(self.ctx, B, T) + 4 * B)
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_generator_ragged(self.ctx, self._stream(), B, T, _ptr(z), _ptr(g), _ptr(ln), _ptr(o), _ptr(ws),
                                               ws.numel())
        _lib.check(rc, self.ctx, "vsp_generator_ragged")
        return o

    @property
    def generator_kind(self) -> int:
        """Which generator the context runs (``vsp_generator_kind``): 0 the channel-major f32 kernels (``VSP_GENERATOR=f32``
        or a configuration the channels-last kernels do not cover), 1 split-f16 channels-last, 2 the opt-in plain f16."""
        return int(self.lib.vsp_generator_kind(self.ctx))

    @property
    def generator_halo(self) -> int:
        """Frames of context the streamed vocoder adds on each side (``vsp_generator_halo_frames``)."""
        return int(self.lib.vsp_generator_halo_frames(self.ctx))

    def generator_frame_dependence(self):
        """(back, fwd): output frame F of the vocoder depends on input frames [F - back, F + fwd], sample-exact from the
        configuration (``vsp_generator_frame_dependence``; 13 / 13 for configs/config.json) -- what the trimmed tails of a
        ragged batch rest on: an utterance of L frames is computed to min(T, L + back + 1 + fwd) frames."""
        b, f = C.c_int(), C.c_int()
        _lib.check(self.lib.vsp_generator_frame_dependence(self.ctx, C.byref(b), C.byref(f)), self.ctx,
                   "vsp_generator_frame_dependence")
        return int(b.value), int(f.value)

    def generator_tail_extents(self):
        """(back, fwd, reach1) (``vsp_generator_tail_extents``; 13 / 13 / 2 for configs/config.json): an utterance served by
        the per-speaker silence table is computed to min(T, L + back + reach1) frames behind the first stage."""
        b, f, r = C.c_int(), C.c_int(), C.c_int()
        _lib.check(self.lib.vsp_generator_tail_extents(self.ctx, C.byref(b), C.byref(f), C.byref(r)), self.ctx,
                   "vsp_generator_tail_extents")
        return int(b.value), int(f.value), int(r.value)

    def generator_stream(self, z, g, chunk_frames: int = 256):
        """Streamed vocoder (BASELINE config 5): yields the waveform of ``z`` [B][C][T] chunk by chunk
        ([B,1,512*n] tensors) so that the first audio is available after one chunk instead of after
        the whole utterance.  Each chunk is one ``vsp_generator_stream_chunk`` call: the generator on its
        frames plus the halo on both sides (zero padding only at the true ends), so the concatenation is
        bit-identical to one ``generator(z, g)`` call."""
        z = _dev_f32(z, self.device)
        g = _dev_f32(g, self.device).reshape(z.shape[0], -1)
        B, _, T = z.shape
        up = self.dims.total_upsample
        ws = self._workspace("generator_stream", self.lib.vsp_generator_stream_workspace_bytes(self.ctx, B, chunk_frames))
        for f0 in range(0, T, chunk_frames):
            f1 = min(T, f0 + chunk_frames)
            o = self._f(B, 1, (f1 - f0) * up)
            with torch.cuda.device(self.device):
                rc = self.lib.vsp_generator_stream_chunk(self.ctx, self._stream(), B, T, _ptr(z), _ptr(g), f0, f1,
                                                         _ptr(o), _ptr(ws), ws.numel())
            _lib.check(rc, self.ctx, "vsp_generator_stream_chunk")
            yield o

    @staticmethod
    def _plan_rows(rows):
        """(L, f0, f1) triples as a ``VspStreamRow`` array (one unused element where there are no rows)."""
        arr = (_lib.VspStreamRow * max(len(rows), 1))()
        for r, (L, f0, f1) in zip(arr, rows):
            r.L, r.f0, r.f1 = int(L), int(f0), int(f1)
        return arr

    def stream_rows_plan(self, rows):
        """``vsp_stream_rows_plan`` (host only): ([lo], [hi], span_max) of rows given as (L, f0, f1) triples -- the window
        ``[max(0, f0 - halo), min(L, f1 + halo))`` each row's chunk is computed from."""
        rows = list(rows)
        arr = self._plan_rows(rows)
        lo, hi = (C.c_int32 * max(len(rows), 1))(), (C.c_int32 * max(len(rows), 1))()
        span = C.c_int32()
        _lib.check(self.lib.vsp_stream_rows_plan(self.ctx, len(rows), arr, lo, hi, C.byref(span)), None, "vsp_stream_rows_plan")
        return list(lo)[:len(rows)], list(hi)[:len(rows)], int(span.value)

    def generator_stream_rows(self, rows, chunk_frames: int, pcm: bool = True) -> torch.Tensor:
        """``vsp_generator_stream_rows``: one chunk of up to 64 requests in ONE set of generator launches.  ``rows`` is a
        sequence of ``(z, g, L, f0, f1)``: ``z`` [inter, >= L] float32 on the device with contiguous frames (any channel
        stride: a row of a batch's latent), ``g`` [gin], and the frames [f0, f1) of the utterance's L to deliver,
        ``f1 - f0 <= chunk_frames``.  Returns [B, chunk_frames * up], int16 if ``pcm`` else float32: row b holds its
        (f1 - f0) * up samples -- those of ``generator_ragged`` on the utterance alone -- and zeros behind them."""
        rows = list(rows)
        B, up = len(rows), self.dims.total_upsample
        if not 1 <= B <= _lib.STREAM_ROWS_MAX:
            raise ValueError(f"1 .. {_lib.STREAM_ROWS_MAX} rows per call, got {B}")
        arr = (_lib.VspStreamRow * B)()
        keep = [self._fill_stream_row(r, *row) for r, row in zip(arr, rows)]
        chunk_frames = int(chunk_frames)
        out = torch.empty((B, max(chunk_frames, 0) * up), dtype=torch.int16 if pcm else torch.float32, device=self.device)
        ws = self._workspace("generator_stream_rows",
                             self.lib.vsp_generator_stream_rows_workspace_bytes(self.ctx, B, chunk_frames))
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_generator_stream_rows(self.ctx, self._stream(), B, arr, _ptr(out), out.shape[1],
                                                    int(bool(pcm)), _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_generator_stream_rows")
        return out

    def _fill_stream_row(self, r, z, g, L, f0, f1):
        """Checks one row's latent and speaker vector and fills the ``VspStreamRow`` ``r``; returns (z, g) to keep alive."""
        d = self.dims
        if (not torch.is_tensor(z) or z.dtype != torch.float32 or z.device != self.device or z.dim() != 2
                or z.shape[0] != d.inter_channels or z.shape[1] < int(L) or (z.shape[1] > 1 and z.stride(1) != 1)):
            raise ValueError("a row's z must be a float32 [inter_channels, >= L] tensor on the engine's device with "
                             "contiguous frames")
        g = _dev_f32(g, self.device).reshape(-1)
        if g.numel() != d.gin_channels:
            raise ValueError(f"a row's g must have {d.gin_channels} entries")
        r.z, r.z_channel_stride, r.g = z.data_ptr(), max(int(z.stride(0)), int(L)), g.data_ptr()
        r.L, r.f0, r.f1 = int(L), int(f0), int(f1)
        return z, g

    def stream_rows_output_plan(self, rows):
        """``vsp_stream_rows_output_plan`` (host only) for the configured output stage: ([m0], [m1], [k0], [k1]) of rows
        given as (L, f0, f1) triples -- the tick delivers output samples [m0, m1), reads the history from input sample k0
        and leaves the history from k1 (``vispeech_amd.output_stage.complete_outputs`` / ``history_start``)."""
        self._need_output()
        rows = list(rows)
        arr = self._plan_rows(rows)
        res = [(C.c_int64 * len(arr))() for _ in range(4)]
        Lo, Mo, Ho = self.output_plan
        _lib.check(self.lib.vsp_stream_rows_output_plan(Lo, Mo, Ho, self.dims.total_upsample, len(rows), arr, *res), None,
                   "vsp_stream_rows_output_plan")
        return tuple(list(a)[:len(rows)] for a in res)

    def output_history(self) -> "OutputHistory":
        """The state one streamed request carries through ``generator_stream_rows_output``."""
        self._need_output()
        return OutputHistory(int(self.lib.vsp_output_history_samples(*self.output_plan)), self.device)

    def stream_rows_out_samples(self, chunk_frames: int) -> int:
        """``vsp_stream_rows_out_samples``: the row length of ``generator_stream_rows_output`` for chunks of up to
        ``chunk_frames`` frames."""
        self._need_output()
        n = int(self.lib.vsp_stream_rows_out_samples(*self.output_plan, self.dims.total_upsample, int(chunk_frames)))
        if n < 0:
            _lib.check(n, None, "vsp_stream_rows_out_samples")
        return n

    def generator_stream_rows_output(self, rows, chunk_frames: int, pcm: bool = True):
        """``vsp_generator_stream_rows_output``: ``generator_stream_rows`` with the ragged output stage instead of the
        collect -- one launch set per tick, delivered at the output rate.  ``rows`` is a sequence of
        ``(z, g, L, f0, f1, state)``, ``state`` the request's ``OutputHistory`` (``output_history()``; its sides are swapped
        here).  A request's ticks must be consecutive: f0 of a call is f1 of its previous one.  Returns
        ``(out [B, stream_rows_out_samples(chunk_frames)], counts)``: row b holds its ``counts[b]`` output samples --
        those ``output`` returns one-shot for the concatenated float chunks, bit for bit -- and zeros behind them."""
        rows = list(rows)
        B = len(rows)
        if not 1 <= B <= _lib.STREAM_ROWS_MAX:
            raise ValueError(f"1 .. {_lib.STREAM_ROWS_MAX} rows per call, got {B}")
        m0, m1, _, _ = self.stream_rows_output_plan([(L, f0, f1) for _, _, L, f0, f1, _ in rows])
        arr = (_lib.VspStreamRowOut * B)()
        keep = []
        for r, (*row, state) in zip(arr, rows):
            keep.append(self._fill_stream_row(r.row, *row))
            r.hist_in, r.hist_out = state.pointers()
        out = torch.empty((B, self.stream_rows_out_samples(chunk_frames)), dtype=torch.int16 if pcm else torch.float32,
                          device=self.device)
        ws = self._workspace("generator_stream_rows",
                             self.lib.vsp_generator_stream_rows_workspace_bytes(self.ctx, B, int(chunk_frames)))
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_generator_stream_rows_output(self.ctx, self._stream(), B, arr, _ptr(out), out.shape[1],
                                                           int(bool(pcm)), _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_generator_stream_rows_output")
        for row in rows:
            row[5].flip()
        return out, [int(b - a) for a, b in zip(m0, m1)]

    # ------------------------------------------------------------------ output stage
    def configure_output(self, out_rate: Optional[int], zeros: int = 32, beta: float = 9.62,
                         rolloff: Optional[float] = None, in_rate: Optional[int] = None) -> None:
        """``vsp_output_configure``: build and upload the filter that takes the waveform from ``in_rate`` (the model's
        sampling rate) to ``out_rate`` -- what the reference's service does with ffmpeg after synthesis
        (inference_api.py:51).  ``out_rate`` equal to ``in_rate`` is the pass-through (quantisation only), None turns the
        stage off.  Allocates: call it once, outside the request path."""
        from . import output_stage
        in_rate = int(self.dims.sampling_rate if in_rate is None else in_rate)
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_output_configure(self.ctx, in_rate, 0 if out_rate is None else int(out_rate), int(zeros),
                                               float(beta), 0.0 if rolloff is None else float(rolloff))
        _lib.check(rc, self.ctx, "vsp_output_configure")
        self.output_plan = None if out_rate is None else output_stage.plan(in_rate, int(out_rate), int(zeros))
        self.output_rate = None if out_rate is None else int(out_rate)

    output_plan = None        # (L, M, H) of the configured output stage
    output_rate = None

    def output_chunk(self, x: torch.Tensor, x_first: int, n_max: int, m0: int, m1: int, n_valid=None,
                     pcm: bool = True) -> torch.Tensor:
        """``vsp_output_chunk``: output samples [m0, m1) of every utterance from the window ``x`` [B, n] (float32 on the
        device, rows may be strided), which holds input samples [x_first, x_first + n).  ``n_valid``: None or the
        utterances' total valid lengths (int64 on the device).  Returns [B, m1 - m0], int16 if ``pcm`` else float32."""
        self._need_output()
        if x.dim() != 2 or x.dtype != torch.float32 or not x.is_cuda or (x.shape[1] > 1 and x.stride(1) != 1):
            raise ValueError("x must be a float32 [B, n] tensor on the engine's device with contiguous rows")
        B, n = x.shape
        nv = None if n_valid is None else _dev_i64(n_valid, self.device)
        if nv is not None and nv.numel() != B:
            raise ValueError(f"n_valid must have {B} entries")
        out = torch.empty((B, max(int(m1 - m0), 0)), dtype=torch.int16 if pcm else torch.float32, device=self.device)
        if out.numel() == 0:
            return out
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_output_chunk(self.ctx, self._stream(), B, _ptr(x), x.stride(0) if B > 1 else max(n, 1),
                                           int(x_first), n, _ptr(nv), int(n_max), int(m0), int(m1), _ptr(out),
                                           out.shape[1], int(bool(pcm)))
        _lib.check(rc, self.ctx, "vsp_output_chunk")
        return out

    def output(self, o: torch.Tensor, sample_lengths=None, pcm: bool = True):
        """One-shot output stage of a whole batch: ``o`` [B, 1, n] or [B, n] as ``infer`` returns it, ``sample_lengths``
        the valid samples per utterance (None: all n) -> (tensor [B, ceil(n L / M)], out_lengths).  What ``o`` holds
        behind an utterance's valid length is never read; the output behind ``out_lengths[b]`` is 0."""
        from . import output_stage
        self._need_output()
        x = o.reshape(o.shape[0], -1) if o.dim() == 3 else o
        L, M, _ = self.output_plan
        nv = None if sample_lengths is None else _dev_i64(sample_lengths, self.device).clamp(0, x.shape[1])
        y = output_stage.one_shot(self, x, nv, pcm)
        lens = torch.full((x.shape[0],), y.shape[1], dtype=torch.int64, device=self.device) if nv is None \
            else (nv * L + (M - 1)) // M
        return y, lens

    def output_stream(self, chunks, n_valid=None, pcm: bool = True):
        """Streamed output stage: consumes the [B, 1, n] chunks of ``generator_stream`` (or any consecutive windows of a
        waveform), keeps the history the filter still needs between chunks on the device, yields the output samples
        each chunk completes ([B, m] tensors) and flushes the tail when the chunks end.  The concatenation equals
        ``output`` of the concatenated waveform bit for bit (``vispeech_amd.output_stage.stream``)."""
        from . import output_stage
        self._need_output()
        nv = None if n_valid is None else _dev_i64(n_valid, self.device)
        return output_stage.stream(self, chunks, nv, pcm)

    # ------------------------------------------------------------------ output rows
    def configure_output_rate(self, rate: int, zeros: int = 32, beta: float = 9.62, rolloff: Optional[float] = None,
                              in_rate: Optional[int] = None) -> None:
        """``vsp_output_rate_configure``: build and upload the filter that takes waveforms from ``in_rate`` (the model's
        sampling rate) to ``rate`` into the context's SET of output rates, which ``output_rows`` reads -- beside the single
        stage of ``configure_output``, which it neither reads nor changes.  Idempotent per rate: the same arguments again
        do nothing, others replace the rate's table; a context holds up to 8 rates.  Allocates: call it outside the
        request path."""
        from . import output_stage
        rate = int(rate)
        in_rate = int(self.dims.sampling_rate if in_rate is None else in_rate)
        key = (in_rate, int(zeros), float(beta), None if rolloff is None else float(rolloff))
        if self._out_rates is None:
            self._out_rates = {}
        if rate in self._out_rates and self._out_rates[rate][0] == key:
            return
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_output_rate_configure(self.ctx, in_rate, rate, int(zeros), float(beta),
                                                    0.0 if rolloff is None else float(rolloff))
        _lib.check(rc, self.ctx, "vsp_output_rate_configure")
        self._out_rates[rate] = (key, output_stage.plan(in_rate, rate, int(zeros)))

    def drop_output_rate(self, rate: int) -> None:
        """Frees the table of an output rate (``vsp_output_rate_configure`` with model_rate 0)."""
        with torch.cuda.device(self.device):
            _lib.check(self.lib.vsp_output_rate_configure(self.ctx, 0, int(rate), 0, 0.0, 0.0), self.ctx,
                       "vsp_output_rate_configure")
        (self._out_rates or {}).pop(int(rate), None)

    _out_rates = None         # rate -> (configuration, (L, M, H)) of the configured output rates

    @property
    def output_rates(self):
        """The rates of the set ``output_rows`` reads."""
        return tuple(self._out_rates or ())

    def output_rate_plan(self, rate: int):
        """(L, M, H) of a rate of the set."""
        if not self._out_rates or int(rate) not in self._out_rates:
            raise RuntimeError(f"output rate {rate} Hz is not configured: call Engine.configure_output_rate({rate}) first")
        return self._out_rates[int(rate)][1]

    def output_row_buffers(self, K: int) -> torch.Tensor:
        """The two history buffers of one request ([2, K] float32 on the device; ``output_stage.RowState``)."""
        return torch.empty((2, max(int(K), 0)), dtype=torch.float32, device=self.device)

    def output_rows(self, rows, outs=None):
        """``vsp_output_rows``: rows of ``(x, ended, rate, enc, state)`` in ONE call per 64 rows, every row with its own
        configured rate and encoding (name or ``VSP_OUT_*``).  ``x``: the row's NEW samples at the model's rate, a 1-D
        contiguous float32 device tensor (None or empty: flush the tail, with ``ended``); ``state``: the request's
        ``output_stage.RowState`` (advanced here), or None for a whole utterance in one call (``ended`` must hold).
        Returns ``(buf, spans)``: one packed uint8 device buffer and per row ``(offset, count)`` -- its ``count`` output
        samples start ``offset`` bytes into ``buf`` (a multiple of 16), as elements of its encoding; the gap up to the next
        row holds the encoding's silence, so one device-to-host copy of ``buf`` delivers all rows.  ``outs``: per row a
        1-D contiguous device tensor of the encoding's dtype that receives the samples instead (all of it is written);
        ``buf`` is then None and the offsets are 0."""
        from . import output_stage
        rows = list(rows)
        B = len(rows)
        if B == 0:
            return torch.empty(0, dtype=torch.uint8, device=self.device), []
        if outs is not None and len(outs) != B:
            raise ValueError(f"outs must have {B} entries")
        arr = (_lib.VspOutputRow * B)()
        keep, counts, sizes = [], [], []
        for r, (x, ended, rate, enc, state) in zip(arr, rows):
            enc = output_stage.encoding(enc)
            L, M, H = self.output_rate_plan(rate)
            if state is None and not ended:
                raise ValueError("a row without a state is a whole utterance: ended must be true")
            if state is not None and state.rate != int(rate):
                raise ValueError(f"a row's state was made for {state.rate} Hz, the row asks for {rate} Hz")
            n = 0 if x is None else int(x.numel())
            if n and (x.dtype != torch.float32 or x.device != self.device or x.dim() != 1 or (n > 1 and x.stride(0) != 1)):
                raise ValueError("a row's x must be a contiguous 1-D float32 tensor on the engine's device")
            if n == 0 and not ended:
                raise ValueError("a row without new samples must end its utterance")
            first = 0 if state is None else state.x_first
            m0, m1, _, _ = output_stage.rows_plan(L, M, H, first, n, ended)
            keep.append(x)
            r.x, r.x_first, r.n, r.ended = (x.data_ptr() if n else None), first, n, int(bool(ended))
            r.out_rate, r.enc = int(rate), enc
            if state is not None and state.K:
                r.hist_in, r.hist_out = state.buf[state.side].data_ptr(), state.buf[1 - state.side].data_ptr()
            counts.append(m1 - m0)
            sizes.append(output_stage.element_size(enc))
        if outs is None:
            A = output_stage.ROW_ALIGN
            slots = [(c * es + A - 1) // A * A for c, es in zip(counts, sizes)]
            offs = [0]
            for s in slots:
                offs.append(offs[-1] + s)
            buf = torch.empty(max(offs[-1], 1), dtype=torch.uint8, device=self.device)
            for r, o, s, es in zip(arr, offs, slots, sizes):
                r.out, r.out_fill = (buf.data_ptr() + o if s else None), s // es
            spans = list(zip(offs[:-1], counts))
        else:
            buf = None
            dts = {0: torch.float32, 1: torch.int16, 2: torch.uint8, 3: torch.uint8}
            for r, out, c in zip(arr, outs, counts):
                if (out.dtype != dts[r.enc] or out.device != self.device or out.dim() != 1 or out.numel() < c
                        or (out.numel() > 1 and out.stride(0) != 1)):
                    raise ValueError("a row's out must be a contiguous 1-D device tensor of its encoding's dtype, at least "
                                     "as long as the row's output")
                r.out, r.out_fill = (out.data_ptr() if out.numel() else None), out.numel()
            spans = [(0, c) for c in counts]
        with torch.cuda.device(self.device):
            for b0 in range(0, B, _lib.STREAM_ROWS_MAX):
                nb = min(_lib.STREAM_ROWS_MAX, B - b0)
                sub = C.cast(C.byref(arr, b0 * C.sizeof(_lib.VspOutputRow)), C.POINTER(_lib.VspOutputRow))
                _lib.check(self.lib.vsp_output_rows(self.ctx, self._stream(), nb, sub), self.ctx, "vsp_output_rows")
        for (x, _, _, _, state), c in zip(rows, counts):
            if state is not None:
                state.advance(0 if x is None else int(x.numel()))
        return buf, spans

    def output_batch(self, o: torch.Tensor, sample_lengths, formats):
        """One-shot output of a whole batch with a format per row: ``o`` [B, 1, n] or [B, n] as ``infer`` returns it,
        ``sample_lengths`` the valid samples per utterance (host integers; None: all n), ``formats`` per row
        ``(rate, enc)``.  Returns ``(buf, spans)`` as ``output_rows`` does: what ``o`` holds behind an utterance's valid
        length is never read."""
        x = o.reshape(o.shape[0], -1) if o.dim() == 3 else o
        if x.dim() != 2 or x.dtype != torch.float32 or (x.shape[1] > 1 and x.stride(1) != 1):
            raise ValueError("o must be a float32 [B, 1, n] or [B, n] tensor with contiguous rows")
        B, n = x.shape
        lens = [n] * B if sample_lengths is None else \
            _host_list(sample_lengths)
        formats = list(formats)
        if len(lens) != B or len(formats) != B or any(v < 0 or v > n for v in lens):
            raise ValueError(f"sample_lengths and formats must have {B} entries, 0 <= sample_lengths[b] <= {n}")
        return self.output_rows([(x[b, :v], True, rate, enc, None) for b, (v, (rate, enc)) in enumerate(zip(lens, formats))])

    # ------------------------------------------------------------------ input stage
    def configure_input(self, rate: int, zeros: int = 32, beta: float = 9.62, rolloff: Optional[float] = None,
                        model_rate: Optional[int] = None) -> None:
        """``vsp_input_configure``: build and upload the filter that takes recordings from ``rate`` to ``model_rate`` (the
        model's sampling rate).  Idempotent per rate: the same arguments again do nothing, others replace the rate's table;
        a context holds up to 8 rates.  ``rate`` equal to the model's is the pass-through (decoding only).  Allocates:
        call it outside the request path."""
        from . import input_stage
        rate = int(rate)
        model_rate = int(self.dims.sampling_rate if model_rate is None else model_rate)
        key = (model_rate, int(zeros), float(beta), None if rolloff is None else float(rolloff))
        if self._input is None:
            self._input = {}
        if rate in self._input and self._input[rate][0] == key:
            return
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_input_configure(self.ctx, rate, model_rate, int(zeros), float(beta),
                                              0.0 if rolloff is None else float(rolloff))
        _lib.check(rc, self.ctx, "vsp_input_configure")
        self._input[rate] = (key, input_stage.plan(rate, model_rate, int(zeros)))

    def drop_input(self, rate: int) -> None:
        """Frees the table of an input rate (``vsp_input_configure`` with model_rate 0)."""
        with torch.cuda.device(self.device):
            _lib.check(self.lib.vsp_input_configure(self.ctx, int(rate), 0, 0, 0.0, 0.0), self.ctx, "vsp_input_configure")
        (self._input or {}).pop(int(rate), None)

    _input = None             # rate -> (configuration, (L, M, H)) of the configured input rates

    @property
    def input_rates(self):
        """The configured input rates."""
        return tuple(self._input or ())

    def input_plan(self, rate: int):
        """(L, M, H) of a configured input rate."""
        if not self._input or int(rate) not in self._input:
            raise RuntimeError(f"input rate {rate} Hz is not configured: call Engine.configure_input({rate}) first")
        return self._input[int(rate)][1]

    def _raw(self, raw, enc: int) -> torch.Tensor:
        """Raw samples (bytes, numpy or torch) as a device tensor of the encoding's own dtype."""
        from . import input_stage
        dt = {0: torch.float32, 1: torch.int16, 2: torch.uint8, 3: torch.uint8}[enc]
        if torch.is_tensor(raw):
            if raw.dtype != dt and not (enc == 0 and raw.dtype.is_floating_point):
                raise ValueError(f"encoding {enc} wants {dt} samples, got {raw.dtype}")
            return raw.to(device=self.device, dtype=dt)
        return torch.from_numpy(input_stage.as_raw(raw, enc)).to(self.device)

    def input_rows(self, rows, rate: int, enc: int = 0, outs=None):
        """``vsp_input_rows``: rows of ``(raw, in_first, n_total, m0, m1)`` in ONE call per 64 rows -- ``raw`` a 1-D tensor of
        the encoding's dtype that holds input samples ``[in_first, in_first + len(raw))`` of a recording of ``n_total`` samples
        (-1 while it is still open), ``[m0, m1)`` the output samples wanted.  ``outs``: per row a 1-D float32 device tensor that
        receives them (all of it is written: zeros behind ``m1 - m0``); None: one is allocated.  Returns the rows' results,
        each ``[m1 - m0]`` float32."""
        from . import input_stage
        enc = input_stage.encoding(enc)
        L, M, H = self.input_plan(rate)
        rows = list(rows)
        B = len(rows)
        if B == 0:
            return []
        raws = [self._raw(r[0], enc).reshape(-1) for r in rows]
        counts = [int(r[4]) - int(r[3]) for r in rows]
        if any(c < 0 for c in counts):
            raise ValueError("a row needs m0 <= m1")
        if outs is None:
            offs = np.concatenate([[0], np.cumsum([(c + 3) // 4 * 4 for c in counts])])
            flat = self._f(max(int(offs[-1]), 1))
            outs = [flat[int(o):int(o) + c] for o, c in zip(offs[:-1], counts)]
        elif len(outs) != B:
            raise ValueError(f"outs must have {B} entries")
        arr = (_lib.VspInputRow * B)()
        for r, raw, (_, first, n_total, m0, m1), out, c in zip(arr, raws, rows, outs, counts):
            if not raw.is_contiguous():
                raise ValueError("a row's raw samples must be contiguous")
            if (out.dtype != torch.float32 or out.device != self.device or out.dim() != 1 or out.numel() < c
                    or (out.numel() > 1 and out.stride(0) != 1)):
                raise ValueError("a row's out must be a contiguous 1-D float32 tensor on the engine's device of at least m1 - m0")
            r.in_ = raw.data_ptr() if raw.numel() else None
            r.in_first, r.in_len, r.n_total = int(first), raw.numel(), int(n_total)
            r.out = out.data_ptr() if out.numel() else None
            r.m0, r.m1, r.out_fill = int(m0), int(m1), out.numel()
        with torch.cuda.device(self.device):
            for b0 in range(0, B, _lib.STREAM_ROWS_MAX):
                n = min(_lib.STREAM_ROWS_MAX, B - b0)
                sub = C.cast(C.byref(arr, b0 * C.sizeof(_lib.VspInputRow)), C.POINTER(_lib.VspInputRow))
                _lib.check(self.lib.vsp_input_rows(self.ctx, self._stream(), int(rate), enc, n, sub), self.ctx, "vsp_input_rows")
        return [o[:c] for o, c in zip(outs, counts)]

    def input_batch(self, raw, n_in, rate: int, enc: int = 0):
        """Whole recordings of one (rate, encoding): ``raw`` [B, stride] (bytes are not accepted here: a 2-D array or tensor
        of the encoding's dtype), row b the recording ``raw[b, :n_in[b]]`` -- what lies behind is never read.  Returns
        ``(audio [B, ceil(max n L / M)] float32, n_out)``: row b holds its ``n_out[b] = ceil(n_in[b] L / M)`` samples at the
        model's rate and exact zeros behind.  The lengths are computed on the host; nothing is read back."""
        from . import input_stage
        enc = input_stage.encoding(enc)
        L, M, _ = self.input_plan(rate)
        a = self._raw(raw, enc)
        if a.dim() == 1:
            a = a.reshape(1, -1)
        if a.dim() != 2 or (a.shape[1] > 1 and a.stride(1) != 1):
            raise ValueError("raw must be [B, stride] with contiguous rows")
        B, stride = a.shape
        n_host = _host_list(n_in)
        if len(n_host) != B or any(x < 0 or x > stride for x in n_host):
            raise ValueError(f"n_in must have {B} entries with 0 <= n_in[b] <= raw.shape[1]")
        n_out = [input_stage.out_len(x, L, M) for x in n_host]
        audio = self._f(B, max(n_out) if B else 0)
        if B and audio.shape[1]:
            self.input_rows([(a[b, :n], 0, n, 0, m) for b, (n, m) in enumerate(zip(n_host, n_out))], rate, enc,
                            outs=[audio[b] for b in range(B)])
        return audio, n_out

    # ------------------------------------------------------------------ prosody from a recording
    @staticmethod
    def _prosody_params(params):
        """None, a ``VspProsodyParams``, or a mapping / sequence of (floor_hz, ceiling_hz, voicing_threshold,
        silence_threshold, octave_cost) -- missing keys take the defaults -- as a ``VspProsodyParams`` or None."""
        if params is None or isinstance(params, _lib.VspProsodyParams):
            return params
        names = [f[0] for f in _lib.VspProsodyParams._fields_]
        vals = dict(zip(names, (80.0, 750.0, 0.6, 0.03, 0.01)))
        if isinstance(params, Mapping):
            unknown = set(params) - set(names)
            if unknown:
                raise ValueError(f"prosody params: unknown {sorted(unknown)}; the fields are {names}")
            vals.update(params)
        else:
            params = list(params)
            if len(params) != len(names):
                raise ValueError(f"prosody params: {len(names)} values {names}")
            vals = dict(zip(names, params))
        return _lib.VspProsodyParams(*(float(vals[k]) for k in names))

    def prosody_frames(self, n_samples: int, hop_length: Optional[int] = None) -> int:
        """``vsp_prosody_frames``: ``n_samples // hop + 1``; a recording below 641 samples is refused.  Host only."""
        F = int(self.lib.vsp_prosody_frames(int(n_samples), self._hop(hop_length)))
        if F < 0:
            raise ValueError(f"prosody: a recording of {int(n_samples)} samples: it needs {_lib.PROSODY_NFFT // 2 + 1} to 2^30")
        return F

    @staticmethod
    def _prosody_path(path):
        """None (no path finder), True (Praat's costs: octave jump 0.35, voiced/unvoiced 0.14, 15 candidates), a
        ``VspProsodyPathParams``, or a mapping / sequence of (octave_jump_cost, voiced_unvoiced_cost, max_candidates) --
        missing keys take the defaults -- as a ``VspProsodyPathParams`` or None."""
        if path is None or path is False or isinstance(path, _lib.VspProsodyPathParams):
            return path or None
        names = [f[0] for f in _lib.VspProsodyPathParams._fields_]
        vals = dict(zip(names, (0.35, 0.14, _lib.PROSODY_MAX_CANDIDATES)))
        if path is True:
            pass
        elif isinstance(path, Mapping):
            unknown = set(path) - set(names)
            if unknown:
                raise ValueError(f"prosody path: unknown {sorted(unknown)}; the fields are {names}")
            vals.update(path)
        else:
            path = list(path)
            if len(path) != len(names):
                raise ValueError(f"prosody path: {len(names)} values {names}")
            vals = dict(zip(names, path))
        oj, vu, n = float(vals[names[0]]), float(vals[names[1]]), vals[names[2]]
        if not (oj >= 0.0 and vu >= 0.0):
            raise ValueError("prosody path: the octave-jump cost and the voiced/unvoiced cost must be at least 0")
        if int(n) != n or not 2 <= int(n) <= _lib.PROSODY_MAX_CANDIDATES:
            raise ValueError(f"prosody path: max_candidates must be a whole number in [2, {_lib.PROSODY_MAX_CANDIDATES}]")
        return _lib.VspProsodyPathParams(oj, vu, int(n))

    def _prosody_rows(self, audio, n_samples, hop_length):
        """The checks every contour call makes of its rows: ``(audio, B, stride, n_host, hop, L_max, frames_host)``."""
        a = _dev_f32(audio, self.device)
        if a.dim() != 2 or (a.shape[1] > 1 and a.stride(1) != 1):
            raise ValueError("audio must be [B, L] (rows padded to a common length, contiguous)")
        B, stride = a.shape[0], (a.stride(0) if a.shape[0] > 1 else a.shape[1])
        n_host = _host_list(n_samples)
        if len(n_host) != B or B == 0:
            raise ValueError(f"n_samples must have {B} entries (at least one row)")
        hop = self._hop(hop_length)
        frames_host = []
        for b, n in enumerate(n_host):
            if n > a.shape[1]:
                raise ValueError(f"row {b}: n_samples {n} > audio.shape[1] = {a.shape[1]}")
            F = int(self.lib.vsp_prosody_frames(n, hop))
            if F < 0:
                raise ValueError(f"row {b}: a recording of {n} samples: prosody needs {_lib.PROSODY_NFFT // 2 + 1} to 2^30")
            frames_host.append(F)
        return a, B, int(stride), n_host, hop, max(n_host), frames_host

    def prosody_candidates(self, audio, n_samples, params=None, max_candidates: int = _lib.PROSODY_MAX_CANDIDATES,
                           hop_length: Optional[int] = None):
        """``vsp_prosody_candidates``: the rows of ``prosody_contours``; instead of a decision, every frame's candidates for
        the path finder.  Returns ``(cand_f, cand_s, energy_frames, frames, frames_host)``: the two
        tables ``[B, F_max, 16]`` float32 -- slot 0 the unvoiced candidate (0, U), slots 1 .. ``max_candidates - 1`` the
        strongest voiced candidates (f, S) in descending S, unused slots (0, -inf), exact zeros behind a row's frames."""
        a, B, stride, n_host, hop, L_max, frames_host = self._prosody_rows(audio, n_samples, hop_length)
        if int(max_candidates) != max_candidates or not 2 <= int(max_candidates) <= _lib.PROSODY_MAX_CANDIDATES:
            raise ValueError(f"prosody path: max_candidates must be a whole number in [2, {_lib.PROSODY_MAX_CANDIDATES}]")
        F_max = max(frames_host)
        p = self._prosody_params(params)
        cand_f, cand_s = self._f(B, F_max, _lib.PROSODY_SLOTS), self._f(B, F_max, _lib.PROSODY_SLOTS)
        en = self._f(B, F_max)
        frames = torch.empty(B, dtype=torch.int64, device=self.device)
        ws = self._workspace("prosody", self.lib.vsp_prosody_workspace_bytes(B, L_max, hop, 1, p))
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_prosody_candidates(self.ctx, self._stream(), B, L_max, hop, _ptr(a), stride, (C.c_int64 * B)(*n_host),
                                                 p, int(max_candidates), _ptr(cand_f), _ptr(cand_s), _ptr(en), _ptr(frames),
                                                 _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_prosody_candidates")
        return cand_f, cand_s, en, frames, frames_host

    def prosody_path(self, cand_f, cand_s, frames_host, path=True, hop_length: Optional[int] = None):
        """``vsp_prosody_path``: the best path through candidate tables ``[B, F_max, 16]`` (``prosody_candidates``', or any:
        f = 0 marks an unvoiced candidate, delta is finite or -inf).  ``frames_host`` [B]: host ints, frames at or behind
        them are not read.  Returns ``f0_frames`` [B, F_max]: the chosen candidate's f in every bit, exact 0 behind a row's
        frames.  ``path``: ``_prosody_path`` (None is refused here: there is nothing to run without one)."""
        cf, cs = _dev_f32(cand_f, self.device), _dev_f32(cand_s, self.device)
        if cf.dim() != 3 or cf.shape[2] != _lib.PROSODY_SLOTS or cf.shape != cs.shape or not cf.is_contiguous() or not cs.is_contiguous():
            raise ValueError(f"cand_f and cand_s must be contiguous [B, F_max, {_lib.PROSODY_SLOTS}] tensors of one shape")
        pp = self._prosody_path(path)
        if pp is None:
            raise ValueError("prosody_path needs path parameters (True for the defaults)")
        B, F_max = int(cf.shape[0]), int(cf.shape[1])
        fh = [int(x) for x in frames_host]
        if len(fh) != B or B == 0 or F_max == 0:
            raise ValueError(f"frames_host must have {B} entries (at least one row of at least one frame)")
        for b, F in enumerate(fh):
            if not 1 <= F <= F_max:
                raise ValueError(f"row {b}: {F} frames: 1 <= frames <= F_max = {F_max}")
        hop = self._hop(hop_length)
        f0 = self._f(B, F_max)
        # (the size is monotone in the length: F_max frames cover any row of the batch)
        ws = self._workspace("prosody", self.lib.vsp_prosody_path_workspace_bytes(B, max((F_max - 1) * hop, 641), hop, None, pp))
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_prosody_path(self.ctx, self._stream(), B, F_max, hop, _ptr(cf), _ptr(cs), (C.c_int64 * B)(*fh), pp,
                                           _ptr(f0), _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_prosody_path")
        return f0

    def prosody_contours(self, audio, n_samples, params=None, hop_length: Optional[int] = None, path=None):
        """``vsp_prosody_contours``: recordings of different lengths in one padded ``audio`` [B, L] at the model's rate; row
        b is ``audio[b, :n_samples[b]]`` (what lies behind is never read).  Returns ``(f0_frames, energy_frames, frames,
        frames_host)``: two ``[B, F_max]`` float32 tensors -- per-frame F0 in Hz (0: unvoiced) and energy, row b's first
        ``frames[b] = n_samples[b] // hop + 1`` columns, exact zeros behind --, the frame counts on the device and as host
        ints (host arithmetic: nothing is read back).  ``params``: ``_prosody_params``.  ``path``: None -- every frame decides
        for itself --, or ``_prosody_path`` (True: Praat's costs): ``vsp_prosody_contours_path``, F0 from the best path through
        every frame's candidates."""
        pp = self._prosody_path(path)
        if pp is not None:
            a, B, stride, n_host, hop, L_max, frames_host = self._prosody_rows(audio, n_samples, hop_length)
            F_max = max(frames_host)
            p = self._prosody_params(params)
            f0, en = self._f(B, F_max), self._f(B, F_max)
            frames = torch.empty(B, dtype=torch.int64, device=self.device)
            ws = self._workspace("prosody", self.lib.vsp_prosody_path_workspace_bytes(B, L_max, hop, p, pp))
            with torch.cuda.device(self.device):
                rc = self.lib.vsp_prosody_contours_path(self.ctx, self._stream(), B, L_max, hop, _ptr(a), stride,
                                                        (C.c_int64 * B)(*n_host), p, pp, _ptr(f0), _ptr(en), _ptr(frames), _ptr(ws),
                                                        ws.numel())
            _lib.check(rc, self.ctx, "vsp_prosody_contours_path")
            return f0, en, frames, frames_host
        a = _dev_f32(audio, self.device)
        if a.dim() != 2 or (a.shape[1] > 1 and a.stride(1) != 1):
            raise ValueError("audio must be [B, L] (rows padded to a common length, contiguous)")
        B, stride = a.shape[0], (a.stride(0) if a.shape[0] > 1 else a.shape[1])
        n_host = _host_list(n_samples)
        if len(n_host) != B or B == 0:
            raise ValueError(f"n_samples must have {B} entries (at least one row)")
        hop = self._hop(hop_length)
        for b, n in enumerate(n_host):
            if n > a.shape[1]:
                raise ValueError(f"row {b}: n_samples {n} > audio.shape[1] = {a.shape[1]}")
        L_max = max(n_host)
        frames_host = []
        for b, n in enumerate(n_host):
            F = int(self.lib.vsp_prosody_frames(n, hop))
            if F < 0:
                raise ValueError(f"row {b}: a recording of {n} samples: prosody needs {_lib.PROSODY_NFFT // 2 + 1} to 2^30")
            frames_host.append(F)
        F_max = max(frames_host)
        p = self._prosody_params(params)
        f0 = self._f(B, F_max)
        en = self._f(B, F_max)
        frames = torch.empty(B, dtype=torch.int64, device=self.device)
        ws = self._workspace("prosody", self.lib.vsp_prosody_workspace_bytes(B, L_max, hop, 1, p))
        n_arr = (C.c_int64 * B)(*n_host)
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_prosody_contours(self.ctx, self._stream(), B, L_max, hop, _ptr(a), int(stride), n_arr, p, _ptr(f0),
                                               _ptr(en), _ptr(frames), _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_prosody_contours")
        return f0, en, frames, frames_host

    def prosody_phonemes(self, f0_frames, energy_frames, frames_host, durations, lengths):
        """``vsp_prosody_phonemes``: the contours of ``prosody_contours`` to per-phoneme means.  ``durations`` [B, Tp] (frames
        per phoneme, integers) and ``lengths`` [B] are read on the HOST (a device tensor is copied back: bring host arrays
        on the request path); row b needs ``sum(durations[b, :lengths[b]]) <= frames_host[b]``.  Returns ``(f0, energy)``,
        ``[B, Tp]`` float32 on the device: F0 interpolated across unvoiced frames, then both averaged over each phoneme's own
        frames; exact 0 for a phoneme of no frames and behind ``lengths[b]``."""
        f0f, enf = _dev_f32(f0_frames, self.device), _dev_f32(energy_frames, self.device)
        if f0f.dim() != 2 or f0f.shape != enf.shape or not f0f.is_contiguous() or not enf.is_contiguous():
            raise ValueError("f0_frames and energy_frames must be contiguous [B, F_max] tensors of one shape")
        B, F_max = f0f.shape
        d = durations.detach().cpu().numpy() if torch.is_tensor(durations) else np.asarray(durations)
        d = d.reshape(B, -1)
        di = np.ascontiguousarray(d, dtype=np.int64)
        if not np.array_equal(di, d):
            raise ValueError("durations must be whole numbers of frames")
        Tp = di.shape[1]
        ln = _host_list(lengths)
        fh = [int(x) for x in frames_host]
        if len(ln) != B or len(fh) != B or Tp < 1:
            raise ValueError(f"lengths and frames_host must have {B} entries, durations at least one column")
        f0, en = self._f(B, Tp), self._f(B, Tp)
        # (the size is monotone in every argument: F_max frames cover any row of the batch)
        ws = self._workspace("prosody", self.lib.vsp_prosody_workspace_bytes(B, max((F_max - 1) * self._hop(None), 641),
                                                                             self._hop(None), Tp, None))
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_prosody_phonemes(self.ctx, self._stream(), B, F_max, Tp, _ptr(f0f), _ptr(enf), (C.c_int64 * B)(*fh),
                                               di.ctypes.data_as(C.POINTER(C.c_int64)), (C.c_int64 * B)(*ln), _ptr(f0), _ptr(en),
                                               _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_prosody_phonemes")
        return f0, en

    # ------------------------------------------------------------------ align: durations from a recording (section 4o)
    @staticmethod
    def _align_params(params):
        """None or True (max_advance 2, both costs 0), a ``VspAlignParams``, or a mapping / sequence of (max_advance,
        stay_cost, skip_cost) -- missing keys take the defaults -- as a ``VspAlignParams``."""
        if isinstance(params, _lib.VspAlignParams):
            return params
        names = [f[0] for f in _lib.VspAlignParams._fields_]
        vals = dict(zip(names, (2, 0.0, 0.0)))
        if params is None or params is True:
            pass
        elif isinstance(params, Mapping):
            unknown = set(params) - set(names)
            if unknown:
                raise ValueError(f"align: unknown {sorted(unknown)}; the fields are {names}")
            vals.update(params)
        else:
            params = list(params)
            if len(params) != len(names):
                raise ValueError(f"align: {len(names)} values {names}")
            vals = dict(zip(names, params))
        A, stay, skip = vals[names[0]], float(vals[names[1]]), float(vals[names[2]])
        if A not in (1, 2):
            raise ValueError("align: max_advance must be 1 or 2")
        if not (stay >= 0.0 and skip >= 0.0):
            raise ValueError("align: the stay cost and the skip cost must be at least 0")
        return _lib.VspAlignParams(int(A), stay, skip)

    @property
    def align_max_states(self) -> int:
        return int(self.lib.vsp_align_max_states())

    @staticmethod
    def _align_rows(B, F_max, K_max, frames_host, states_host, pp=None, limit=None):
        """The rows of an align call as host ints, refused here as the library refuses them (a ``ValueError`` naming the row)."""
        fh, kh = [int(v) for v in frames_host], [int(v) for v in states_host]
        if len(fh) != B or len(kh) != B or B == 0:
            raise ValueError(f"frames_host and states_host must have {B} entries (at least one row)")
        for b, (F, K) in enumerate(zip(fh, kh)):
            if not 1 <= F <= F_max:
                raise ValueError(f"align: row {b} has {F} frames: 1 <= frames <= F_max = {F_max}")
            if not 1 <= K <= K_max:
                raise ValueError(f"align: row {b} has {K} states: 1 <= states <= K_max = {K_max}")
            if pp is not None:
                if K > limit:
                    raise ValueError(f"align: row {b} has {K} states: the limit is {limit}")
                if K > pp.max_advance * (F - 1) + 1:
                    raise ValueError(f"align: row {b} is infeasible: {F} frames cannot reach {K} states advancing at most "
                                     f"{pp.max_advance} a frame (the recording is too short for its text)")
        return fh, kh

    def _align_inputs(self, x, m, logs):
        x, m, logs = (_dev_f32(a, self.device).contiguous() for a in (x, m, logs))
        if x.dim() != 3 or m.dim() != 3 or m.shape != logs.shape or x.shape[:2] != m.shape[:2]:
            raise ValueError("align: x [B, C, F_max], m and logs [B, C, K_max]")
        return x, m, logs

    @staticmethod
    def _align_cum(cum_dur, lengths, B):
        """``cum_dur`` [B, Tp] and ``lengths`` [B] on the HOST (a device tensor is copied back)."""
        c = cum_dur.detach().cpu().numpy() if torch.is_tensor(cum_dur) else np.asarray(cum_dur)
        c = np.ascontiguousarray(c.reshape(B, -1), dtype=np.int32)
        ln = _host_list(lengths)
        if len(ln) != B or c.shape[1] < 1:
            raise ValueError(f"lengths must have {B} entries, cum_dur at least one column")
        return c, ln

    def align_scores(self, x, m, logs, frames_host, states_host):
        """``vsp_align_scores``: ``S`` [B, F_max, K_max] float32, row b's ``frames_host[b] x states_host[b]`` corner the
        Gaussian log-likelihood of every frame of ``x`` [B, C, F_max] under every state of ``m``, ``logs`` [B, C, K_max]
        (the direct form), exact 0 outside; nothing outside a row's extent is read."""
        x, m, logs = self._align_inputs(x, m, logs)
        B, Cc, F_max = x.shape
        K_max = m.shape[2]
        fh, kh = self._align_rows(B, F_max, K_max, frames_host, states_host)
        S = self._f(B, F_max, K_max)
        ws = self._workspace("align", self.lib.vsp_align_scores_workspace_bytes(B, F_max, K_max))
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_align_scores(self.ctx, self._stream(), B, Cc, F_max, K_max, _ptr(x), _ptr(m), _ptr(logs),
                                           (C.c_int64 * B)(*fh), (C.c_int64 * B)(*kh), _ptr(S), _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_align_scores")
        return S

    def align_path(self, scores, frames_host, states_host, params=None):
        """``vsp_align_path``: the best monotone path through score tables ``[B, F_max, K_max]`` (``align_scores``', or
        any finite ones): ``states`` [B, F_max] int32, frame j's state, from 0 to ``states_host[b] - 1`` advancing at most
        ``max_advance`` a frame; exact 0 behind a row's frames.  fp64 accumulation: the fp64 restatement's path on the same
        scores bit for bit.  ``params``: ``_align_params``."""
        S = _dev_f32(scores, self.device)
        if S.dim() != 3 or not S.is_contiguous():
            raise ValueError("scores must be a contiguous [B, F_max, K_max] tensor")
        pp = self._align_params(params)
        B, F_max, K_max = S.shape
        fh, kh = self._align_rows(B, F_max, K_max, frames_host, states_host, pp, self.align_max_states)
        states = torch.empty((B, F_max), dtype=torch.int32, device=self.device)
        ws = self._workspace("align", self.lib.vsp_align_path_workspace_bytes(B, F_max, K_max))
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_align_path(self.ctx, self._stream(), B, F_max, K_max, _ptr(S), (C.c_int64 * B)(*fh),
                                         (C.c_int64 * B)(*kh), pp, _ptr(states), _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_align_path")
        return states

    def align_durations(self, states, frames_host, cum_dur, lengths):
        """``vsp_align_durations``: ``states`` [B, F_max] int32 to per-phoneme frame counts ``[B, Tp]`` int32 (device):
        phoneme i of row b gets the frames whose state lies in ``[cum_dur[b, i - 1], cum_dur[b, i])`` -- ``cum_dur`` as
        ``encode`` returns it, read on the HOST --, 0 behind ``lengths[b]``."""
        st = torch.as_tensor(states).to(device=self.device, dtype=torch.int32).contiguous()
        if st.dim() != 2:
            raise ValueError("states must be [B, F_max]")
        B, F_max = st.shape
        cum, ln = self._align_cum(cum_dur, lengths, B)
        Tp = cum.shape[1]
        fh = [int(v) for v in frames_host]
        for b, F in enumerate(fh):
            if not 1 <= F <= F_max:
                raise ValueError(f"align: row {b} has {F} frames: 1 <= frames <= F_max = {F_max}")
        dur = torch.empty((B, Tp), dtype=torch.int32, device=self.device)
        ws = self._workspace("align", self.lib.vsp_align_workspace_bytes(B, F_max, 1, Tp))
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_align_durations(self.ctx, self._stream(), B, F_max, Tp, _ptr(st), (C.c_int64 * B)(*fh),
                                              cum.ctypes.data_as(C.POINTER(C.c_int32)), (C.c_int64 * B)(*ln), _ptr(dur), _ptr(ws),
                                              ws.numel())
        _lib.check(rc, self.ctx, "vsp_align_durations")
        return dur

    def align(self, x, m, logs, frames_host, states_host, cum_dur, lengths, params=None):
        """``vsp_align``: scores, path and durations in one call (three launches; the score matrix stays in the workspace).
        ``x`` [B, C, F_max]: the recordings' latent (``convert_latent(noise_scale=0)['z_p']``); ``m``, ``logs`` [B, C, K_max]
        and ``cum_dur`` [B, Tp]: the text's frame-level prior and phoneme map (``decode(max_len=0)``, ``encode``).  Returns
        ``(states [B, F_max], durations [B, Tp])`` int32 on the device; ``sum(durations[b]) == frames_host[b]``.  A row whose
        recording is too short for its template is a ``ValueError`` naming it."""
        x, m, logs = self._align_inputs(x, m, logs)
        pp = self._align_params(params)
        B, Cc, F_max = x.shape
        K_max = m.shape[2]
        fh, kh = self._align_rows(B, F_max, K_max, frames_host, states_host, pp, self.align_max_states)
        cum, ln = self._align_cum(cum_dur, lengths, B)
        Tp = cum.shape[1]
        for b in range(B):
            if not 1 <= ln[b] <= Tp or int(cum[b, ln[b] - 1]) != kh[b]:
                raise ValueError(f"align: row {b}: cum_dur must end at the row's {kh[b]} states (1 <= length <= Tp = {Tp})")
        states = torch.empty((B, F_max), dtype=torch.int32, device=self.device)
        dur = torch.empty((B, Tp), dtype=torch.int32, device=self.device)
        ws = self._workspace("align", self.lib.vsp_align_workspace_bytes(B, F_max, K_max, Tp))
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_align(self.ctx, self._stream(), B, Cc, F_max, K_max, Tp, _ptr(x), _ptr(m), _ptr(logs),
                                    (C.c_int64 * B)(*fh), (C.c_int64 * B)(*kh), cum.ctypes.data_as(C.POINTER(C.c_int32)),
                                    (C.c_int64 * B)(*ln), pp, _ptr(states), _ptr(dur), _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_align")
        return states, dur

    def align_audio(self, phonemes, lengths, sid, audio, n_samples, sid_audio=None, params=None, fit_length: bool = True):
        """What ``SynthesizerTrn.align_audio`` runs on recordings at the model's rate: the text through an isolated
        ``encode`` (twice with ``fit_length``: the second time with row b's ``duration_scale = T_b / K_b``) and
        ``decode(max_len=0)``, the recordings through ``convert_latent(noise_scale=0)``, then ``align``.  Returns
        ``durations`` [B, Tp] int64 on the device."""
        from types import SimpleNamespace
        pp = self._align_params(params)
        n_host = _host_list(n_samples)
        frames = [self.convert_frames(n) for n in n_host]
        for b, T in enumerate(frames):
            if T < 1:
                raise ValueError(f"align_audio: row {b}: a recording of {n_host[b]} samples is too short for one frame")
        B = len(frames)
        enc = self.encode(phonemes, lengths, sid, isolated=True)
        states, tf = self.frame_lengths_host(enc["frame_lengths"])
        kw = {}
        if fit_length:
            one, flat = np.ones(B, dtype=np.float32), np.zeros(B, dtype=np.float32)
            scale = np.array([frames[b] / states[b] if states[b] > 0 else 1.0 for b in range(B)], dtype=np.float32)
            kw["row_controls"] = SimpleNamespace(duration_scale=scale, pitch_scale=one, energy_scale=one, noise_scale=flat,
                                                 given=np.zeros((B, 3), dtype=bool))
            enc = self.encode(phonemes, lengths, sid, isolated=True, **kw)
            states, tf = self.frame_lengths_host(enc["frame_lengths"])
        for b, K in enumerate(states):
            if K < 1:
                raise ValueError(f"align_audio: row {b}: its text has no template frames")
        self._align_rows(B, max(frames), tf, frames, states, pp, self.align_max_states)     # (refused before the device works)
        dec = self.decode(enc, tf, None, 0.0, max_len=0, isolated=True, **kw)
        sid_a = sid if sid_audio is None else sid_audio
        lat = self.convert_latent(audio, n_host, sid_a, sid_a, noise_scale=0.0)
        _, dur = self.align(lat["z_p"], dec["m_p"], dec["logs_p"], lat["frames_host"], states, enc["cum_dur"], lengths, pp)
        return dur.to(torch.int64)

    # ------------------------------------------------------------------ loudness (section 4p)
    @staticmethod
    def loudness_params(B: int, target_lufs=-23.0, peak_ceiling=1.0, max_gain_db=30.0):
        """``vsp_loudness_params`` [B] from three values, each a scalar or one value per row.  A row's ``target_lufs`` may be
        None or NaN: the row is left alone.  Refused here as the library refuses them (a ``ValueError`` naming the row)."""
        t, c, m = (_column(v, B, f"loudness: {n}") for v, n in ((target_lufs, "target_lufs"), (peak_ceiling, "peak_ceiling"),
                                                                 (max_gain_db, "max_gain_db")))
        out = (_lib.VspLoudnessParams * B)()
        for b in range(B):
            if not c[b] > 0.0:
                raise ValueError(f"loudness: row {b}: peak_ceiling must be above 0")
            if not m[b] >= 0.0:
                raise ValueError(f"loudness: row {b}: max_gain_db must be at least 0")
            out[b] = _lib.VspLoudnessParams(t[b], c[b], m[b])
        return out

    def _loudness_rows(self, audio, n_samples, sample_rate, what: str = "audio"):
        """The checks every loudness call makes of its rows: ``(audio, B, stride, n_host, fs)``.  A float32 tensor on the
        device with contiguous rows is used as it is (so that ``loudness_apply`` can work in place)."""
        a = audio if (torch.is_tensor(audio) and audio.dtype == torch.float32 and audio.device == self.device) \
            else _dev_f32(audio, self.device)
        if a.dim() != 2 or (a.shape[1] > 1 and a.stride(1) != 1):
            raise ValueError(f"{what} must be [B, L] (rows padded to a common length, each contiguous)")
        B = a.shape[0]
        stride = a.stride(0) if B > 1 else a.shape[1]
        n_host = _host_list(n_samples)
        if len(n_host) != B or B == 0:
            raise ValueError(f"n_samples must have {B} entries (at least one row)")
        if stride < a.shape[1]:
            raise ValueError(f"{what}: rows overlap")
        for b, n in enumerate(n_host):
            if not 1 <= n <= a.shape[1]:
                raise ValueError(f"loudness: row {b} has {n} samples: 1 <= n_samples <= {what}.shape[1] = {a.shape[1]}")
        fs = None
        if sample_rate is not None:
            fs = int(sample_rate)
            if not _lib.LOUDNESS_FS_MIN <= fs <= _lib.LOUDNESS_FS_MAX:
                raise ValueError(f"loudness: sample_rate {fs}: {_lib.LOUDNESS_FS_MIN} <= sample_rate <= {_lib.LOUDNESS_FS_MAX}")
        return a, B, int(stride), n_host, fs

    def loudness_segments(self, audio, n_samples, sample_rate: int):
        """``vsp_loudness_segments``: ``audio`` [B, L] float32 at ``sample_rate``, row b ``audio[b, :n_samples[b]]`` (what lies
        behind is never read).  Returns ``(seg, peak)``: the K-weighted energy of every 100 ms segment, ``[B, S_max]`` float64
        with exact zeros behind a row's segments, and the rows' sample peaks ``[B]`` float32 (exact)."""
        a, B, stride, n_host, fs = self._loudness_rows(audio, n_samples, sample_rate)
        L_max = max(n_host)
        S_max = int(self.lib.vsp_loudness_segments_count(L_max, fs))
        seg = torch.empty((B, S_max), dtype=torch.float64, device=self.device)
        peak = self._f(B)
        ws = self._workspace("loudness", self.lib.vsp_loudness_workspace_bytes(B, L_max, fs))
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_loudness_segments(self.ctx, self._stream(), B, L_max, fs, _ptr(a), stride, (C.c_int64 * B)(*n_host),
                                                _ptr(seg), _ptr(peak), _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_loudness_segments")
        return seg, peak

    def loudness_gate(self, seg, n_samples, sample_rate: int, peak=None, params=None):
        """``vsp_loudness_gate``: any float64 segment table ``[B, S_max]`` (``loudness_segments``', or any) with the rows'
        ``n_samples`` to ``(lufs [B] float32, blocks [B, 2] int32)`` -- the integrated loudness (-inf where no block is
        kept) and (blocks, kept blocks) --; with ``params`` (``loudness_params``) and the rows' ``peak`` also ``gains`` [B]."""
        t = torch.as_tensor(seg).to(device=self.device, dtype=torch.float64).contiguous()
        if t.dim() != 2 or t.shape[1] < 1:
            raise ValueError("seg must be [B, S_max]")
        B, S_max = t.shape
        n_host = _host_list(n_samples)
        fs = int(sample_rate)
        if len(n_host) != B or B == 0:
            raise ValueError(f"n_samples must have {B} entries (at least one row)")
        h = (fs + 5) // 10
        for b, n in enumerate(n_host):
            if not 1 <= n <= S_max * h:
                raise ValueError(f"loudness: row {b} has {n} samples: 1 <= n_samples <= S_max h = {S_max * h}")
        lufs = self._f(B)
        blocks = torch.empty((B, 2), dtype=torch.int32, device=self.device)
        gains = pk = None
        if params is not None:
            if peak is None:
                raise ValueError("loudness_gate: gains need the rows' peak")
            pk = _dev_f32(peak, self.device)
            gains = self._f(B)
        ws = self._workspace("loudness", self.lib.vsp_loudness_workspace_bytes(B, 1, _lib.LOUDNESS_FS_MIN))
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_loudness_gate(self.ctx, self._stream(), B, S_max, fs, _ptr(t), (C.c_int64 * B)(*n_host), _ptr(pk),
                                            params, _ptr(lufs), _ptr(blocks), _ptr(gains), _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_loudness_gate")
        return (lufs, blocks) if params is None else (lufs, blocks, gains)

    def loudness(self, audio, n_samples, sample_rate: int):
        """The integrated loudness of every row: ``loudness_segments`` then ``loudness_gate``.  Returns ``(lufs, peak,
        blocks)``, all on the device."""
        seg, peak = self.loudness_segments(audio, n_samples, sample_rate)
        lufs, blocks = self.loudness_gate(seg, n_samples, sample_rate)
        return lufs, peak, blocks

    def loudness_apply(self, audio, n_samples, gains, params=None, out=None):
        """``vsp_loudness_apply``: ``out[b, :n_b] = gains[b] * audio[b, :n_b]``; ``out`` None: in place where ``audio`` is a
        float32 device tensor (a copy of it otherwise).  With ``params`` a row whose target is NaN is neither read nor
        written.  Nothing at or behind ``n_b`` is touched.  Returns ``out``."""
        a, B, stride, n_host, _ = self._loudness_rows(audio, n_samples, None)
        o, _, o_stride, _, _ = self._loudness_rows(a if out is None else out, n_samples, None, "out")
        if out is not None and o is not out:
            raise ValueError("out must be a float32 tensor on the engine's device")
        g = _dev_f32(gains, self.device)
        if g.shape != (B,):
            raise ValueError(f"gains must have {B} entries")
        L_max = max(n_host)
        ws = self._workspace("loudness", self.lib.vsp_loudness_workspace_bytes(B, 1, _lib.LOUDNESS_FS_MIN))
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_loudness_apply(self.ctx, self._stream(), B, L_max, _ptr(a), stride, _ptr(o), o_stride,
                                             (C.c_int64 * B)(*n_host), _ptr(g), params, _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_loudness_apply")
        return o

    def loudness_normalize(self, audio, n_samples, sample_rate: int, params, out=None):
        """``vsp_loudness_normalize``: measure, derive every row's gain from its ``params`` (``loudness_params``) and apply
        it, in ONE call (five launches behind one upload; nothing is read back in between).  ``out`` None: in place where
        ``audio`` is a float32 device tensor.  Returns ``(out, gains, lufs, peak, blocks)``, all on the device; a row whose
        target is NaN keeps its samples (gain exactly 1, neither read nor written by the apply)."""
        a, B, stride, n_host, fs = self._loudness_rows(audio, n_samples, sample_rate)
        o, _, o_stride, _, _ = self._loudness_rows(a if out is None else out, n_samples, None, "out")
        if out is not None and o is not out:
            raise ValueError("out must be a float32 tensor on the engine's device")
        if len(params) != B:
            raise ValueError(f"loudness: params must have {B} rows")
        L_max = max(n_host)
        lufs, peak, gains = self._f(B), self._f(B), self._f(B)
        blocks = torch.empty((B, 2), dtype=torch.int32, device=self.device)
        ws = self._workspace("loudness", self.lib.vsp_loudness_workspace_bytes(B, L_max, fs))
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_loudness_normalize(self.ctx, self._stream(), B, L_max, fs, _ptr(a), stride, _ptr(o), o_stride,
                                                 (C.c_int64 * B)(*n_host), params, _ptr(lufs), _ptr(peak), _ptr(gains),
                                                 _ptr(blocks), _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_loudness_normalize")
        return o, gains, lufs, peak, blocks

    # ------------------------------------------------------------------ loudness over time (section 4r)
    @staticmethod
    def loudness_level_params(B: int, target_lufs=-23.0, max_gain_db=12.0, max_cut_db=12.0, slew_db_per_s=3.0, initial_gain_db=0.0):
        """``vsp_loudness_level_params`` [B] from five values, each a scalar or one value per row.  A row's ``target_lufs`` may
        be None or NaN: the leveller leaves the row alone.  Refused here as the library refuses them, naming the row."""
        cols = [_column(v, B, f"loudness: {n}") for v, n in ((target_lufs, "target_lufs"), (max_gain_db, "max_gain_db"), (max_cut_db, "max_cut_db"),
                                       (slew_db_per_s, "slew_db_per_s"), (initial_gain_db, "initial_gain_db"))]
        out = (_lib.VspLoudnessLevelParams * B)()
        for b in range(B):
            t, g, c, s, i = (col[b] for col in cols)
            if not g >= 0.0:
                raise ValueError(f"loudness: row {b}: max_gain_db must be at least 0")
            if not c >= 0.0:
                raise ValueError(f"loudness: row {b}: max_cut_db must be at least 0")
            if not s > 0.0:
                raise ValueError(f"loudness: row {b}: slew_db_per_s must be above 0")
            if not np.isfinite(i):
                raise ValueError(f"loudness: row {b}: initial_gain_db must be finite")
            out[b] = _lib.VspLoudnessLevelParams(t, g, c, s, i)
        return out

    def _own_rows(self, t, dtype, what: str, B=None):
        """The rows of a table given as ``[B, T]`` or as B 1-D tensors allocated apart: each must already be a ``dtype`` tensor
        on the device with unit stride (the calls of this section write in place and read what earlier calls left)."""
        rows = list(t)
        if B is not None and len(rows) != B:
            raise ValueError(f"{what} must have {B} rows")
        for b, r in enumerate(rows):
            if not (torch.is_tensor(r) and r.dtype == dtype and r.device == self.device and r.dim() == 1 and (r.numel() < 2 or r.stride(0) == 1)):
                raise ValueError(f"{what}: row {b} must be a 1-D {dtype} tensor on the engine's device")
        return rows

    @staticmethod
    def _ints(v, B: int, what: str):
        return [int(v)] * B if np.ndim(v) == 0 else _host_list(v, int, B, what)

    def _level_params(self, params, B: int):
        """``params`` as ``loudness_level_params`` made them, or B mappings of the five fields (a missing one: its default)."""
        if isinstance(params, C.Array):
            if len(params) != B:
                raise ValueError(f"loudness: params must have {B} rows")
            return params
        rows = list(params)
        if len(rows) != B:
            raise ValueError(f"loudness: params must have {B} rows")
        names = ("target_lufs", "max_gain_db", "max_cut_db", "slew_db_per_s", "initial_gain_db")
        defaults = (-23.0, 12.0, 12.0, 3.0, 0.0)
        return self.loudness_level_params(B, *[[r.get(n, d) for r in rows] for n, d in zip(names, defaults)])

    def loudness_state(self, B: int):
        """The K-weighting's state of B new streams: ``[B, 4]`` float64 zeros on the device."""
        return torch.zeros((B, 4), dtype=torch.float64, device=self.device)

    def loudness_table(self, n: int, dtype):
        """A 1-D table of ``n`` entries of a numpy ``dtype`` on the device (NaN, or -1 for integers, until written)."""
        dt = {"float64": torch.float64, "float32": torch.float32, "int32": torch.int32}[np.dtype(dtype).name]
        return torch.full((int(n),), -1 if dt == torch.int32 else float("nan"), dtype=dt, device=self.device)

    def _tables(self, B: int, T: int, floats: int, ints: int = 0):
        """New ``[B, T]`` tables on the device: ``floats`` float32 ones of NaN, then ``ints`` int32 ones of -1."""
        return tuple(torch.full((B, T), float("nan"), dtype=torch.float32, device=self.device) for _ in range(floats)) + \
            tuple(torch.full((B, T), -1, dtype=torch.int32, device=self.device) for _ in range(ints))

    def _time_ws(self, B: int):
        return self._workspace("loudness", self.lib.vsp_loudness_time_workspace_bytes(B, 1, _lib.LOUDNESS_FS_MIN))

    def _time_rows(self, segs, first, count, tables):
        """What ``loudness_time`` and ``loudness_time_hist`` hand the library: ``(desc, M, S, I, kept)`` -- the rows'
        ``VspLoudnessRow`` over their segment tables ``segs`` and ``tables`` (None: new ones, to the last entry asked for)."""
        B = len(segs)
        if tables is None:
            tables = self._tables(B, max(1, max(f + c for f, c in zip(first, count))), 3, 1)
        M, S, I, kept = tables
        rows = [self._own_rows(t, torch.float32, n, B) for t, n in ((M, "M"), (S, "S"), (I, "I"))] + [self._own_rows(kept, torch.int32, "kept", B)]
        desc = (_lib.VspLoudnessRow * B)()
        for b in range(B):
            entries = min([segs[b].numel()] + [r[b].numel() for r in rows])
            desc[b] = _lib.VspLoudnessRow(seg=segs[b].data_ptr(), M=rows[0][b].data_ptr(), S=rows[1][b].data_ptr(), I=rows[2][b].data_ptr(),
                                          kept=rows[3][b].data_ptr(), first=first[b], count=count[b], entries=entries)
        return desc, M, S, I, kept

    def loudness_segments_from(self, audio, n_samples, sample_rate: int, state=None, first=None):
        """``vsp_loudness_segments_from``: ``loudness_segments`` of the pieces ``audio[b, :n_samples[b]]`` of B streams, each
        starting on a segment boundary of its stream (``first``: the streams' positions, checked; None: 0) with the
        K-weighting's ``state`` ``[B, 4]`` float64 on the device (None: zero).  Returns ``(seg, peak, state_out)``:
        ``state_out`` ``[B, 4]`` is the state behind each piece's last complete segment -- what the next piece starts from."""
        a, B, stride, n_host, fs = self._loudness_rows(audio, n_samples, sample_rate)
        L_max = max(n_host)
        S_max = int(self.lib.vsp_loudness_segments_count(L_max, fs))
        st = None
        if state is not None:
            st = torch.as_tensor(state).to(device=self.device, dtype=torch.float64).contiguous()
            if st.shape != (B, 4):
                raise ValueError(f"state must be [{B}, 4]")
        f = None if first is None else (C.c_int64 * B)(*self._ints(first, B, "first"))
        seg = torch.empty((B, S_max), dtype=torch.float64, device=self.device)
        peak = self._f(B)
        st_out = torch.empty((B, 4), dtype=torch.float64, device=self.device)
        ws = self._workspace("loudness", self.lib.vsp_loudness_workspace_bytes(B, L_max, fs))
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_loudness_segments_from(self.ctx, self._stream(), B, L_max, fs, _ptr(a), stride, (C.c_int64 * B)(*n_host), f,
                                                     _ptr(st), _ptr(st_out), _ptr(seg), _ptr(peak), _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_loudness_segments_from")
        return seg, peak, st_out

    def loudness_time(self, seg, first, count, sample_rate: int, tables=None):
        """``vsp_loudness_time``: the entries ``[first_b, first_b + count_b)`` of every row's ``M, S, I`` (float32) and ``kept``
        (int32) from its float64 segment table ``seg`` -- ``[B, T]`` or B 1-D tensors allocated apart, each from the row's
        segment 0.  ``tables``: ``(M, S, I, kept)`` to write into (likewise), or None: new ``[B, T]`` tensors, NaN (-1 for
        ``kept``) outside the entries computed.  Returns ``(M, S, I, kept, m_max, s_max)``; the maxima ``[B]`` are those of
        THIS call's entries."""
        segs = self._own_rows(seg, torch.float64, "seg")
        B = len(segs)
        if B == 0:
            raise ValueError("loudness_time: at least one row")
        first, count = self._ints(first, B, "first"), self._ints(count, B, "count")
        desc, M, S, I, kept = self._time_rows(segs, first, count, tables)
        m_max, s_max = self._f(B), self._f(B)
        ws = self._time_ws(B)
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_loudness_time(self.ctx, self._stream(), B, int(sample_rate), desc, _ptr(m_max), _ptr(s_max), _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_loudness_time")
        return M, S, I, kept, m_max, s_max

    def loudness_level_gains(self, I, first, count, params, tables=None):
        """``vsp_loudness_level_gains``: the leveller's gain in dB and linear, ``c_db`` and ``c``, entries ``[first_b, first_b +
        count_b)`` of every row from ANY table ``I`` (rows as ``loudness_time``), continuing from ``c_db[first_b - 1]`` of the
        row's own table (``initial_gain_db`` at 0).  ``tables``: ``(c_db, c)`` to write into, or None: new ``[B, T]`` tensors
        (NaN outside).  A NaN-target row is neither read nor written.  Returns ``(c_db, c)``."""
        Is = self._own_rows(I, torch.float32, "I")
        B = len(Is)
        if B == 0:
            raise ValueError("loudness_level_gains: at least one row")
        params = self._level_params(params, B)
        first, count = self._ints(first, B, "first"), self._ints(count, B, "count")
        if tables is None:
            tables = self._tables(B, max(1, max(f + c for f, c in zip(first, count))), 2)
        c_db, c = tables
        dbs, cs = self._own_rows(c_db, torch.float32, "c_db", B), self._own_rows(c, torch.float32, "c", B)
        desc = (_lib.VspLoudnessRow * B)()
        for b in range(B):
            desc[b] = _lib.VspLoudnessRow(I=Is[b].data_ptr(), c_db=dbs[b].data_ptr(), c=cs[b].data_ptr(), first=first[b], count=count[b],
                                          entries=min(Is[b].numel(), dbs[b].numel(), cs[b].numel()))
        ws = self._time_ws(B)
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_loudness_level_gains(self.ctx, self._stream(), B, desc, params, _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_loudness_level_gains")
        return c_db, c

    def loudness_level_apply(self, x, pos, c, entries, sample_rate: int, params, n_samples=None, out=None):
        """``vsp_loudness_level_apply``: row b's samples ``x[b][:n_b]`` (``n_samples`` None: all of the row) are its stream's
        ``[pos_b, pos_b + n_b)``; they are levelled against the row's gain table ``c``, of which ``entries[b]`` are valid
        (at least ``(pos_b + n_b - 1) // h``).  ``x``, ``c``, ``out``: ``[B, .]`` or B 1-D tensors allocated apart.  ``out``
        may be ``x`` (in place); None: new tensors (of ``n_b`` samples each for rows given apart, a copy of a 2-D ``x``
        otherwise).  Nothing at or behind ``n_b`` and no NaN-target row is read or written.  Returns ``out``."""
        xs = self._own_rows(x, torch.float32, "x")
        B = len(xs)
        if B == 0:
            raise ValueError("loudness_level_apply: at least one row")
        params = self._level_params(params, B)
        cs = self._own_rows(c, torch.float32, "c", B)
        pos, entries = self._ints(pos, B, "pos"), self._ints(entries, B, "entries")
        n = [r.numel() for r in xs] if n_samples is None else self._ints(n_samples, B, "n_samples")
        if out is None:
            out = x.clone() if torch.is_tensor(x) else [self._f(max(0, min(k, r.numel()))) for k, r in zip(n, xs)]
        os_ = self._own_rows(out, torch.float32, "out", B)
        desc = (_lib.VspLoudnessRow * B)()
        for b in range(B):
            if not 0 <= n[b] <= min(xs[b].numel(), os_[b].numel()):
                raise ValueError(f"loudness: row {b} has {n[b]} samples: its tensors hold {min(xs[b].numel(), os_[b].numel())}")
            if not 0 <= entries[b] <= cs[b].numel():
                raise ValueError(f"loudness: row {b}: {entries[b]} entries of a table of {cs[b].numel()}")
            desc[b] = _lib.VspLoudnessRow(c=cs[b].data_ptr(), entries=entries[b], inp=xs[b].data_ptr(), out=os_[b].data_ptr(), pos=pos[b],
                                          samples=n[b])
        ws = self._time_ws(B)
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_loudness_level_apply(self.ctx, self._stream(), B, int(sample_rate), desc, params, _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_loudness_level_apply")
        return out

    def loudness_level(self, audio, n_samples, sample_rate: int, params=None, out=None):
        """``vsp_loudness_level``: whole rows in ONE call -- segments, the loudness of the row, the tables over time and, with
        ``params`` (``loudness_level_params``), the leveller's gains and its output (``out`` None: in place where ``audio`` is a
        float32 device tensor).  Returns a dict: ``M, S, I`` ``[B, F_max]`` float32 and ``kept`` int32 (row b written for ``s <
        n_b // h``, NaN / -1 behind), ``m_max, s_max, i_end, peak`` ``[B]``, and with ``params`` ``c_db, c`` and ``out``."""
        a, B, stride, n_host, fs = self._loudness_rows(audio, n_samples, sample_rate)
        o = o_stride = None
        if params is not None:
            params = self._level_params(params, B)
            o, _, o_stride, _, _ = self._loudness_rows(a if out is None else out, n_samples, None, "out")
            if out is not None and o is not out:
                raise ValueError("out must be a float32 tensor on the engine's device")
        L_max = max(n_host)
        T = max(1, L_max // ((fs + 5) // 10))
        r = dict(zip(("M", "S", "I", "kept"), self._tables(B, T, 3, 1)), m_max=self._f(B), s_max=self._f(B), i_end=self._f(B), peak=self._f(B))
        if params is not None:
            r.update(zip(("c_db", "c"), self._tables(B, T, 2)), out=o)
        ws = self._workspace("loudness", self.lib.vsp_loudness_time_workspace_bytes(B, L_max, fs))
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_loudness_level(self.ctx, self._stream(), B, L_max, fs, _ptr(a), stride, _ptr(o), o_stride or 0,
                                             (C.c_int64 * B)(*n_host), params, _ptr(r["M"]), _ptr(r["S"]), _ptr(r["I"]), _ptr(r["kept"]),
                                             _ptr(r.get("c_db")), _ptr(r.get("c")), T, _ptr(r["m_max"]), _ptr(r["s_max"]), _ptr(r["i_end"]),
                                             _ptr(r["peak"]), _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_loudness_level")
        return r

    # ------------------------------------------------------------------ loudness range and the histogram gate (section 4s)
    def loudness_hist_tables(self):
        """``vsp_loudness_hist_tables``: ``(edges [1001], centres [1000])`` float64 numpy arrays, the bits the device gets."""
        e, c = np.empty(_lib.LOUDNESS_HIST_BINS + 1, np.float64), np.empty(_lib.LOUDNESS_HIST_BINS, np.float64)
        rc = self.lib.vsp_loudness_hist_tables(e.ctypes.data_as(C.POINTER(C.c_double)), c.ctypes.data_as(C.POINTER(C.c_double)))
        _lib.check(rc, None, "vsp_loudness_hist_tables")
        return e, c

    def loudness_hist_state(self, B: int):
        """The histograms of B new streams: ``[B, 2, 1000]`` int32 zeros on the device (the 400 ms blocks, the 3 s windows)."""
        return torch.zeros((B, 2, _lib.LOUDNESS_HIST_BINS), dtype=torch.int32, device=self.device)

    def loudness_time_hist(self, seg, first, count, sample_rate: int, hist, tables=None):
        """``vsp_loudness_time_hist``: ``loudness_time`` under the histogram gate.  ``hist``: ``[B, 2, 1000]`` int32 or B
        ``[2, 1000]`` tensors allocated apart, on the device: each row's state after its entries ``[0, first_b)`` (taken as
        zero at ``first_b == 0``), advanced IN PLACE to the state after ``first_b + count_b``.  Returns ``(M, S, I, kept, m_max,
        s_max, lra)``: ``M`` and ``S`` are ``loudness_time``'s, ``I`` and ``kept`` the histogram gate's, ``lra`` ``[B]`` the
        loudness range after this call's last entry.  The work of an entry does not depend on where the stream stands."""
        segs = self._own_rows(seg, torch.float64, "seg")
        B = len(segs)
        if B == 0:
            raise ValueError("loudness_time_hist: at least one row")
        first, count = self._ints(first, B, "first"), self._ints(count, B, "count")
        hs = list(hist)
        if len(hs) != B:
            raise ValueError(f"hist must have {B} rows")
        for b, t in enumerate(hs):
            if not (torch.is_tensor(t) and t.dtype == torch.int32 and t.device == self.device and t.is_contiguous()
                    and tuple(t.shape) == (2, _lib.LOUDNESS_HIST_BINS)):
                raise ValueError(f"hist: row {b} must be a contiguous [2, {_lib.LOUDNESS_HIST_BINS}] int32 tensor on the engine's device")
        desc, M, S, I, kept = self._time_rows(segs, first, count, tables)
        m_max, s_max, lra = self._f(B), self._f(B), self._f(B)
        ws = self._workspace("loudness", self.lib.vsp_loudness_hist_workspace_bytes(B, 1, _lib.LOUDNESS_FS_MIN))
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_loudness_time_hist(self.ctx, self._stream(), B, int(sample_rate), desc, (C.c_void_p * B)(*[t.data_ptr() for t in hs]),
                                                 _ptr(m_max), _ptr(s_max), _ptr(lra), _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_loudness_time_hist")
        return M, S, I, kept, m_max, s_max, lra

    def loudness_range(self, audio, n_samples, sample_rate: int):
        """``vsp_loudness_range``: whole rows in ONE call -- segments, then the histogram gate from zero histograms.  Returns a
        dict: ``lra`` ``[B]`` float32 (LU), ``i_hist`` ``[B]`` (the running level at the row's last complete segment, -inf
        where it has none), ``M, S, I`` ``[B, F_max]`` float32 and ``kept`` int32 (NaN / -1 behind a row's entries)."""
        a, B, stride, n_host, fs = self._loudness_rows(audio, n_samples, sample_rate)
        L_max = max(n_host)
        T = max(1, L_max // ((fs + 5) // 10))
        r = dict(lra=self._f(B), i_hist=self._f(B), **dict(zip(("M", "S", "I", "kept"), self._tables(B, T, 3, 1))))
        ws = self._workspace("loudness", self.lib.vsp_loudness_hist_workspace_bytes(B, L_max, fs))
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_loudness_range(self.ctx, self._stream(), B, L_max, fs, _ptr(a), stride, (C.c_int64 * B)(*n_host), _ptr(r["lra"]),
                                             _ptr(r["i_hist"]), _ptr(r["M"]), _ptr(r["S"]), _ptr(r["I"]), _ptr(r["kept"]), T, _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_loudness_range")
        return r

    # ------------------------------------------------------------------ true peak and limiter (section 4q)
    def limiter_history(self, attack: int, hold: int):
        """``vsp_limiter_history``: ``(behind, ahead)`` -- the samples before an output and after it that reach it."""
        behind, ahead = C.c_int64(), C.c_int64()
        rc = self.lib.vsp_limiter_history(int(attack), int(hold), C.byref(behind), C.byref(ahead))
        _lib.check(rc, None, f"vsp_limiter_history(attack = {attack}, hold = {hold})")
        return behind.value, ahead.value

    def true_peak(self, audio, n_samples):
        """``vsp_true_peak``: the true peak (4x oversampled) of every row ``audio[b, :n_samples[b]]``,
        ``[B]`` float32 on the device.  What lies behind a row's end is never read."""
        a, B, stride, n_host, _ = self._loudness_rows(audio, n_samples, None)
        tp = self._f(B)
        ws = self._workspace("limiter", self.lib.vsp_limiter_workspace_bytes(B, 1, 0, 0))
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_true_peak(self.ctx, self._stream(), B, max(n_host), _ptr(a), stride, (C.c_int64 * B)(*n_host),
                                        _ptr(tp), _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_true_peak")
        return tp

    def limiter_rows(self, rows, attack: int, hold: int, gains=None):
        """``vsp_limiter_rows``: ONE call over rows ``(x, first, out_first, out_count, total, ceiling)`` -- ``x`` a 1-D
        float32 device tensor holding the stream's samples ``[first, first + len(x))``, ``total`` the stream's length or -1,
        ``ceiling`` None / NaN for a row left alone -- each at its own position.  ``gains``: one per row (a device tensor
        stays on the device) or None for 1.  Returns ``(outs, min_gain)``: the rows' limited samples ``[out_first, out_first +
        out_count)`` as new 1-D tensors, and ``[B]`` float32."""
        B = len(rows)
        if B == 0:
            raise ValueError("limiter_rows: at least one row")
        A, H = int(attack), int(hold)
        desc = (_lib.VspLimiterRow * B)()
        keep, outs = [], []
        for b, (x, first, out_first, out_count, total, ceiling) in enumerate(rows):
            x = x if (torch.is_tensor(x) and x.dtype == torch.float32 and x.device == self.device and x.is_contiguous()) \
                else _dev_f32(x, self.device)
            if x.dim() != 1:
                raise ValueError(f"limiter_rows: row {b}: samples must be 1-D")
            o = self._f(max(int(out_count), 0))
            keep.append(x)
            outs.append(o)
            desc[b] = _lib.VspLimiterRow(x.data_ptr() if x.numel() else None, int(first), x.numel(),
                                         o.data_ptr() if o.numel() else None, int(out_first), int(out_count),
                                         -1 if total is None else int(total), float("nan") if ceiling is None else float(ceiling))
        g = None
        if gains is not None:
            g = _dev_f32(gains, self.device)
            if g.shape != (B,):
                raise ValueError(f"gains must have {B} entries")
        mg = self._f(B)
        L_max = max(1, max(int(r[3]) for r in rows))
        ws = self._workspace("limiter", self.lib.vsp_limiter_workspace_bytes(B, L_max, min(max(A, 0), _lib.LIMITER_MAX_ATTACK),
                                                                             min(max(H, 0), _lib.LIMITER_MAX_HOLD)))
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_limiter_rows(self.ctx, self._stream(), B, A, H, desc, _ptr(g), _ptr(mg), _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_limiter_rows")
        return outs, mg

    def limit(self, audio, n_samples, ceiling, gains=None, attack: int = 66, hold: int = 882, out=None):
        """The look-ahead limiter over whole rows ``audio[b, :n_samples[b]]``: ``out = clamp(g x s,
        -c, c)`` with the smoothed gain ``s`` that keeps ``g |x|`` -- and, up to the measured overshoot, its true peak --
        under the row's ``ceiling`` (a scalar or one per row; None / NaN: the row is neither read nor written).  ``gains``:
        the rows' static gains ``g`` (a device tensor stays there), None for 1.  ``attack`` (= look-ahead) and ``hold`` in
        samples.  ``out`` None: in place where ``audio`` is a float32 device tensor.  Returns ``(out, min_gain)``."""
        a, B, stride, n_host, _ = self._loudness_rows(audio, n_samples, None)
        o, _, o_stride, _, _ = self._loudness_rows(a if out is None else out, n_samples, None, "out")
        if out is not None and o is not out:
            raise ValueError("out must be a float32 tensor on the engine's device")
        c = _column(ceiling, B, "limiter: ceiling")
        A, H = int(attack), int(hold)
        desc = (_lib.VspLimiterRow * B)()
        for b, n in enumerate(n_host):
            desc[b] = _lib.VspLimiterRow(a.data_ptr() + 4 * b * stride, 0, n, o.data_ptr() + 4 * b * o_stride, 0, n, n, c[b])
        g = None
        if gains is not None:
            g = _dev_f32(gains, self.device)
            if g.shape != (B,):
                raise ValueError(f"gains must have {B} entries")
        mg = self._f(B)
        ws = self._workspace("limiter", self.lib.vsp_limiter_workspace_bytes(B, max(n_host), min(max(A, 0), _lib.LIMITER_MAX_ATTACK),
                                                                             min(max(H, 0), _lib.LIMITER_MAX_HOLD)))
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_limiter_rows(self.ctx, self._stream(), B, A, H, desc, _ptr(g), _ptr(mg), _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_limiter_rows")
        return o, mg

    def loudness_limit(self, audio, n_samples, sample_rate: int, params, attack: int = 66, hold: int = 882, ceilings=None,
                       static_gains=None, out=None):
        """Normalisation with the limiter behind the gain: ``loudness_segments``, ``loudness_gate`` with the rows' ``params``
        but an infinite ceiling -- so a row's gain is ``min(target gain, max_gain_db)``, not cut by its peak --, then ``limit``
        at the rows' ``peak_ceiling`` (or ``ceilings``: one per row, None / NaN for a row the limiter leaves alone).  The
        gains stay on the device.  ``static_gains`` (one per row) multiply the gate's, for rows that name a gain and no
        target (whose gate gain is exactly 1).  A row with a NaN target and no entry in ``ceilings`` is left as it is.
        Returns ``(out, gains, lufs, peak, blocks, min_gain)``."""
        B = len(params)
        inf = float("inf")
        free = (_lib.VspLoudnessParams * B)(*[_lib.VspLoudnessParams(p.target_lufs, inf, p.max_gain_db) for p in params])
        if ceilings is None:
            ceilings = [float("nan") if p.target_lufs != p.target_lufs else p.peak_ceiling for p in params]
        seg, peak = self.loudness_segments(audio, n_samples, sample_rate)
        lufs, blocks, gains = self.loudness_gate(seg, n_samples, sample_rate, peak=peak, params=free)
        if static_gains is not None:
            gains = gains * _dev_f32(static_gains, self.device)
        o, mg = self.limit(audio, n_samples, ceilings, gains=gains, attack=attack, hold=hold, out=out)
        return o, gains, lufs, peak, blocks, mg

    # ------------------------------------------------------------------ denoiser and inverse STFT (section 4t)
    def _set_transform(self, transform: str, what: str) -> None:
        """``vsp_set_stft_transform`` right before a call: ``"dft"``, the two products, or ``"fft"``.
        The workspace of the call is sized behind it, by the same switch."""
        if transform not in _lib.STFT_TRANSFORMS:
            raise ValueError(f"{what}: transform must be 'dft' or 'fft', not {transform!r}")
        _lib.check(self.lib.vsp_set_stft_transform(self.ctx, _lib.STFT_TRANSFORMS[transform]), self.ctx, "vsp_set_stft_transform")

    def _denoise_ws(self, B: int, L_max: int, what: str) -> torch.Tensor:
        if int(self.dims.hop_length) != int(self.dims.total_upsample):
            raise ValueError(f"{what}: hop_length {self.dims.hop_length} is not the generator's total upsampling "
                             f"{self.dims.total_upsample}: the bias would not be periodic in a frame")
        need =int(self.lib.vsp_denoise_workspace_bytes(self.ctx, int(B), int(L_max)))
        if need < 0:
            raise ValueError(f"{what}: the context has no denoiser geometry (spec_channels > 1, hop = the generator's total "
                             f"upsampling dividing n_fft at least four times), or B = {B} / L_max = {L_max} is out of range")
        return self._workspace("denoise", need)

    def denoise_bias(self, g, transform: str = "dft") -> torch.Tensor:
        """The denoiser's bias of conditioning vectors ``g`` [S, gin] (any: no row of ``emb_g`` is needed), [S, spec_channels]
        float32 on the device: the generator on ``back + 1 + fwd`` all-zero latent frames, its output frame ``back`` -- the
        steady period, without the start-up transient --, then ``vsp_denoise_bias``: the magnitude of the windowed DFT of
        that period tiled to ``n_fft`` samples."""
        g = _dev_f32(g, self.device)
        g = g.reshape(-1, g.shape[-1]) if g.dim() != 2 else g
        S = g.shape[0]
        back, fwd = self.generator_frame_dependence()
        up = self.dims.total_upsample
        z = torch.zeros((S, self.dims.inter_channels, back + 1 + fwd), dtype=torch.float32, device=self.device)
        o = self.generator(z, g)
        period = o[:, 0, back * up:(back + 1) * up].contiguous()
        return self.denoise_bias_of(period, transform=transform)

    def denoise_bias_of(self, period, transform: str = "dft") -> torch.Tensor:
        """``vsp_denoise_bias``: ``period`` [S, hop] float32 -> [S, spec_channels] on the device."""
        self._set_transform(transform, "denoise_bias")
        p = _dev_f32(period, self.device)
        if p.dim() != 2 or p.shape[1] != self.dims.total_upsample or p.shape[0] < 1:
            raise ValueError(f"period must be [S, {self.dims.total_upsample}]")
        S = p.shape[0]
        bias = self._f(S, self.dims.spec_channels)
        ws = self._denoise_ws(S, 2 * (self.dims.spec_channels - 1), "denoise_bias")
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_denoise_bias(self.ctx, self._stream(), S, _ptr(p), _ptr(bias), _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_denoise_bias")
        return bias

    def istft(self, ri, n_samples, transform: str = "dft") -> torch.Tensor:
        """``vsp_istft``: ``ri`` [B, 2 spec_channels, T_max] (real rows, then imaginary; T_max the frames of the longest row)
        to audio [B, max(n_samples)] by weighted overlap-add; row b's first ``n_samples[b]`` samples are written, the rest
        is 0."""
        x = _dev_f32(ri, self.device)
        n_host = _host_list(n_samples)
        B, L_max = len(n_host), max(n_host)
        self._set_transform(transform, "istft")
        ws = self._denoise_ws(B, L_max, "istft")
        T = self.convert_frames(L_max, self.dims.total_upsample)
        if x.dim() != 3 or tuple(x.shape) != (B, 2 * self.dims.spec_channels, T):
            raise ValueError(f"ri must be [{B}, {2 * self.dims.spec_channels}, {T}]")
        out = torch.zeros((B, L_max), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_istft(self.ctx, self._stream(), B, L_max, _ptr(x), (C.c_int64 * B)(*n_host), _ptr(out), L_max,
                                    _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_istft")
        return out

    def denoise(self, audio, n_samples, bias, strength, out=None, transform: str = "dft") -> torch.Tensor:
        """``vsp_denoise``: subtract ``strength[b] * bias[b]`` from the magnitude of every STFT frame of ``audio[b,
        :n_samples[b]]`` and return to audio.  ``bias`` [B, spec_channels] (row b's own); ``strength`` a scalar or one per
        row, None / NaN: the row is neither read nor written.  ``out`` None: in place where ``audio`` is a float32 device
        tensor.  Nothing at or behind ``n_samples[b]`` is touched.  Returns ``out``.  ``transform``: ``"dft"``, the two
        products, or ``"fft"``, the in-LDS FFT (``bias`` should come from the same transform) -- as in
        ``istft``, ``denoise_bias``, ``denoise_bias_of`` and ``denoise_rows``."""
        a, B, stride, n_host, _ = self._loudness_rows(audio, n_samples, None)
        o, _, o_stride, _, _ = self._loudness_rows(a if out is None else out, n_samples, None, "out")
        if out is not None and o is not out:
            raise ValueError("out must be a float32 tensor on the engine's device")
        s = _column(strength, B, "denoise: strength")
        bp = None
        if bias is not None:
            bp = _dev_f32(bias, self.device)
            if tuple(bp.shape) != (B, self.dims.spec_channels):
                raise ValueError(f"bias must be [{B}, {self.dims.spec_channels}]")
        L_max = max(n_host)
        self._set_transform(transform, "denoise")
        ws = self._denoise_ws(B, L_max, "denoise")
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_denoise(self.ctx, self._stream(), B, L_max, _ptr(a), stride, (C.c_int64 * B)(*n_host), _ptr(bp),
                                      (C.c_float * B)(*s), _ptr(o), o_stride, _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_denoise")
        return o

    def denoise_history(self):
        """``vsp_denoise_history``: ``(behind, ahead)`` = ``(n_fft - hop, n_fft - 1)`` -- the samples before an output and
        after it that can reach it."""
        behind, ahead = C.c_int64(), C.c_int64()
        _lib.check(self.lib.vsp_denoise_history(self.ctx, C.byref(behind), C.byref(ahead)), None,
                   "vsp_denoise_history (the context has no denoiser geometry)")
        return behind.value, ahead.value

    def denoise_complete(self, n_seen: int, closed: bool = False) -> int:
        """``vsp_denoise_complete``: the outputs of a stream that are final once ``n_seen`` samples are in (host arithmetic)."""
        e = int(self.lib.vsp_denoise_complete(self.ctx, int(n_seen), int(bool(closed))))
        if e < 0:
            raise ValueError(f"denoise_complete({n_seen}): negative, or the context has no denoiser geometry")
        return e

    def denoise_rows(self, rows, bias, transform: str = "dft"):
        """``vsp_denoise_rows``: ONE call over rows ``(x, first, out_first, out_count, total, strength)`` -- ``x`` a 1-D
        float32 device tensor holding the stream's samples ``[first, first + len(x))``, ``total`` the stream's length or -1 /
        None, ``strength`` None / NaN for a row left alone -- each at its own position.  ``bias`` [B, spec_channels] (row
        b's own), or None when every row is left alone.  Returns the rows' denoised samples ``[out_first, out_first +
        out_count)`` as new 1-D tensors."""
        B = len(rows)
        if B == 0:
            raise ValueError("denoise_rows: at least one row")
        if int(self.dims.hop_length) != int(self.dims.total_upsample):
            raise ValueError(f"denoise_rows: hop_length {self.dims.hop_length} is not the generator's total upsampling "
                             f"{self.dims.total_upsample}: the bias would not be periodic in a frame")
        bp = None
        if bias is not None:
            bp = _dev_f32(bias, self.device)
            if tuple(bp.shape) != (B, self.dims.spec_channels):
                raise ValueError(f"bias must be [{B}, {self.dims.spec_channels}]")
        desc = (_lib.VspDenoiseRow * B)()
        keep, outs = [], []
        for b, (x, first, out_first, out_count, total, strength) in enumerate(rows):
            x = x if (torch.is_tensor(x) and x.dtype == torch.float32 and x.device == self.device and x.is_contiguous()) \
                else _dev_f32(x, self.device)
            if x.dim() != 1:
                raise ValueError(f"denoise_rows: row {b}: samples must be 1-D")
            o = self._f(max(int(out_count), 0))
            keep.append(x)
            outs.append(o)
            desc[b] = _lib.VspDenoiseRow(x.data_ptr() if x.numel() else None, int(first), x.numel(),
                                         o.data_ptr() if o.numel() else None, int(out_first), int(out_count),
                                         -1 if total is None else int(total), float("nan") if strength is None else float(strength))
        L_max = max(1, max(int(r[3]) for r in rows))
        self._set_transform(transform, "denoise_rows")
        need = int(self.lib.vsp_denoise_rows_workspace_bytes(self.ctx, B, L_max))
        if need < 0:
            raise ValueError(f"denoise_rows: the context has no denoiser geometry (spec_channels > 1, hop = the generator's total "
                             f"upsampling dividing n_fft at least four times), or B = {B} / {L_max} outputs is out of range")
        ws = self._workspace("denoise", need)
        with torch.cuda.device(self.device):
            rc = self.lib.vsp_denoise_rows(self.ctx, self._stream(), B, desc, _ptr(bp), _ptr(ws), ws.numel())
        _lib.check(rc, self.ctx, "vsp_denoise_rows")
        return outs

    def profile(self, on: bool) -> None:
        _lib.check(self.lib.vsp_profile_enable(self.ctx, int(on)), self.ctx, "vsp_profile_enable")

    def profile_read(self, reset: bool = True, cls: int = _lib.PROF_GENERATOR):
        """(launches, ms, algorithmic FLOPs, SURVEY-8d bytes, bytes incl. residual / accumulate reads, bytes the launches
        move as fused) of one class."""
        n, ms, fl, by, bx, bm = C.c_int64(), C.c_double(), C.c_double(), C.c_double(), C.c_double(), C.c_double()
        _lib.check(self.lib.vsp_profile_read_class(self.ctx, int(cls), C.byref(n), C.byref(ms), C.byref(fl), C.byref(by),
                                                   C.byref(bx), C.byref(bm), int(reset)), self.ctx, "vsp_profile_read_class")
        return int(n.value), float(ms.value), float(fl.value), float(by.value), float(bx.value), float(bm.value)


    _FAMILY_KINDS = {0: "other", 1: "conv", 2: "ups", 3: "pair", 4: "chain", 5: "pre", 6: "rb2"}

    def profile_read_families(self, cls: int = _lib.PROF_GENERATOR, max_families: int = 64):
        """Per kernel family of one class since the last reset (call BEFORE profile_read(reset=True)):
        [{kind, channels, launches, ms, flops, bytes, moved}], largest total time first."""
        m = int(max_families)
        fam, n = (C.c_int * m)(), (C.c_int64 * m)()
        ms, fl, by, bm = (C.c_double * m)(), (C.c_double * m)(), (C.c_double * m)(), (C.c_double * m)()
        k = self.lib.vsp_profile_read_families(self.ctx, int(cls), m, fam, n, ms, fl, by, bm)
        _lib.check(min(k, 0), self.ctx, "vsp_profile_read_families")
        out = [dict(kind=self._FAMILY_KINDS.get(fam[i] & 7, "other"), channels=16 if (fam[i] >> 3) == 7 else 32 << (fam[i] >> 3), launches=int(n[i]),
                    ms=float(ms[i]), flops=float(fl[i]), bytes=float(by[i]), moved=float(bm[i])) for i in range(k)]
        return sorted(out, key=lambda d: -d["ms"])


def rq_spline(x, uw, uh, ud, inverse: bool = False, tail_bound: float = 5.0):
    """piecewise_rational_quadratic_transform(..., tails='linear') on the GPU (reference
    transforms.py:12-193).  x [...]; uw, uh [..., nb]; ud [..., nb-1]."""
    l = _lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device()) if not (torch.is_tensor(x) and x.is_cuda) else x.device
    x = _dev_f32(x, dev)
    uw, uh, ud = _dev_f32(uw, dev), _dev_f32(uh, dev), _dev_f32(ud, dev)
    nb = uw.shape[-1]
    n = x.numel()
    y, lad = torch.empty_like(x), torch.empty_like(x)
    with torch.cuda.device(dev):
        rc = l.vsp_rq_spline(C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), n, nb, _ptr(x), _ptr(uw), _ptr(uh),
                             _ptr(ud), int(inverse), float(tail_bound), _ptr(y), _ptr(lad))
    _lib.check(rc, None, "vsp_rq_spline")
    return y, lad
