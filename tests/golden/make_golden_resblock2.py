#!/usr/bin/env python3
"""Generate tests/golden/resblock2.npz from the REAL reference with ``resblock = "2"``.

Runs only where the reference checkout exists (VISPEECH_REFERENCE; imported read-only, nothing of it is copied), like
make_golden.py.  The reference ``SynthesizerTrn`` is built from its unchanged configs/config.json with the one
constructor argument ``resblock`` set to "2" (reference models.py:251 then builds modules.ResBlock2, modules.py:232-256,
which reads dilation[0] and dilation[1] of each [1, 3, 5] row), loaded with this repo's seeded synthetic weights, and run
on CPU with ``torch.randn_like`` patched to return the fixture noise:

  * ``infer`` (reference models.py:672-722) on a ragged batch of three utterances, given durations / pitch / energy, and
    the same batch again with ``max_len`` (its waveform only, ``ml_o``: every other output is the first run's);
  * ``voice_conversion`` (reference models.py:724-732) on a short ragged batch of synthetic spectrograms (prefix ``vc_``).

Every array written is data: inputs, noise, expected outputs, and the reference's state_dict key list with its shapes.

    python tests/golden/make_golden_resblock2.py        # rewrites tests/golden/resblock2.npz
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("VISPEECH_REFERENCE", "/root/reference")
sys.path.insert(0, REPO)
sys.path.insert(0, REF)

from vispeech_amd import config as vcfg                          # noqa: E402
from vispeech_amd.schema import dims_from_ctor, state_dict_schema  # noqa: E402
from vispeech_amd.synth import synth_batch, synth_state_dict      # noqa: E402

import models as ref_models                                       # noqa: E402  (reference)
import utils as ref_utils                                         # noqa: E402  (reference)
from text.symbols import symbols as ref_symbols                   # noqa: E402  (reference)

WEIGHT_SEED = 2718


def build_reference():
    hps = ref_utils.get_hparams_from_file(os.path.join(REF, "configs", "config.json"))
    mine = vcfg.default_hparams()
    for k, v in mine.model.items():
        assert hps.model[k] == v, ("config drift", k)
    assert len(ref_symbols) == vcfg.N_SYMBOLS
    mine.model["resblock"] = "2"
    args, kwargs = vcfg.synthesizer_args(mine, len(ref_symbols))
    net = ref_models.SynthesizerTrn(*args, **kwargs).eval()
    assert type(net.dec.resblocks[0]).__name__ == "ResBlock2"
    dims = dims_from_ctor(*args, **kwargs)
    ref_sd = net.state_dict()
    schema = state_dict_schema(dims)
    assert list(schema.keys()) == list(ref_sd.keys()), "schema key order/content differs from the reference"
    for k, s in schema.items():
        assert tuple(ref_sd[k].shape) == tuple(s), (k, ref_sd[k].shape, s)
    sd = synth_state_dict(dims, seed=WEIGHT_SEED)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    keys = list(ref_sd.keys())
    shapes = np.full((len(keys), 4), -1, dtype=np.int64)
    for i, k in enumerate(keys):
        shapes[i, :ref_sd[k].dim()] = tuple(ref_sd[k].shape)
    return net, dims, keys, shapes


class _Noise:
    """Patch ``torch.randn_like`` so the reference consumes the fixture noise (models.py:718, 231)."""

    def __init__(self, noise):
        self.noise = torch.from_numpy(noise)

    def __enter__(self):
        self._orig = torch.randn_like
        torch.randn_like = lambda t, *a, **k: self.noise[:, :, :t.shape[2]].to(t.dtype).clone()
        return self

    def __exit__(self, *exc):
        torch.randn_like = self._orig


def infer_case(net, batch, prefix, max_len=None):
    ph = torch.from_numpy(batch["phonemes"])
    with torch.no_grad(), _Noise(batch["noise"]):
        o, x_mask, (z, z_p, m_p, logs_p), _dur, _f0, _en = net.infer(
            ph, torch.from_numpy(batch["lengths"]), sid=torch.from_numpy(batch["sid"]), noise_scale=0.667,
            max_len=max_len, duration_control=torch.from_numpy(batch["duration"]),
            pitch_control=torch.from_numpy(batch["f0"]), energy_control=torch.from_numpy(batch["energy"]))
    tf = x_mask.shape[2]
    out = {"max_len": np.int64(-1 if max_len is None else max_len), "noise": np.ascontiguousarray(batch["noise"][:, :, :tf]),
           "o": o.numpy(), "x_mask": x_mask.numpy(), "z": z.numpy(), "z_p": z_p.numpy(), "m_p": m_p.numpy(),
           "logs_p": logs_p.numpy()}
    print(f"{prefix or 'infer'}: B={ph.shape[0]} Tf={tf} frames={x_mask.numpy().sum(axis=(1, 2)).astype(int).tolist()} "
          f"|o|max={np.abs(out['o']).max():.4f}")
    return {prefix + k: v for k, v in out.items()}


def vc_case(net, dims):
    r = np.random.Generator(np.random.PCG64(3141))
    lens = np.array([10, 5], dtype=np.int64)
    B, T = len(lens), int(lens.max())
    y = np.abs(r.standard_normal((B, dims.spec_channels, T))).astype(np.float32)
    for b, n in enumerate(lens):
        y[b, :, n:] = 0.0
    sid_src = np.array([5, 77], dtype=np.int64)
    sid_tgt = np.array([12, 3], dtype=np.int64)
    noise = r.standard_normal((B, dims.inter_channels, T)).astype(np.float32)
    with torch.no_grad(), _Noise(noise):
        o_hat, y_mask, (z, z_p, z_hat) = net.voice_conversion(
            torch.from_numpy(y), torch.from_numpy(lens), torch.from_numpy(sid_src), torch.from_numpy(sid_tgt))
    print(f"voice_conversion: B={B} T={T} |o|max={np.abs(o_hat.numpy()).max():.4f}")
    return dict(vc_y=y, vc_lengths=lens, vc_sid_src=sid_src, vc_sid_tgt=sid_tgt, vc_noise=noise, vc_o_hat=o_hat.numpy(),
                vc_y_mask=y_mask.numpy(), vc_z=z.numpy(), vc_z_p=z_p.numpy(), vc_z_hat=z_hat.numpy())


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    net, dims, keys, shapes = build_reference()
    # three utterances of different lengths (26 / 13 / 30 frames): the 13-frame one ends early enough for a trimmed tail
    batch = synth_batch(3, seed=11, mean_phonemes=8, std_phonemes=3, min_phonemes=4, max_phonemes=12,
                        mean_frames=26, jitter_frames=16)
    out = dict(weight_seed=np.int64(WEIGHT_SEED), ref_keys=np.array(keys), ref_shapes=shapes,
               in_phonemes=batch["phonemes"], in_lengths=batch["lengths"], in_sid=batch["sid"],
               in_duration=batch["duration"], in_f0=batch["f0"], in_energy=batch["energy"])
    out.update(infer_case(net, batch, ""))
    out["ml_max_len"] = np.int64(16)
    out["ml_o"] = infer_case(net, batch, "ml_", max_len=16)["ml_o"]
    out.update(vc_case(net, dims))
    path = os.path.join(HERE, "resblock2.npz")
    np.savez_compressed(path, **out)
    print(f"resblock2.npz: {len(keys)} keys -> {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
