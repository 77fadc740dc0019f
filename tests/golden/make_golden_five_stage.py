#!/usr/bin/env python3
"""Generate tests/golden/five_stage.npz from the REAL reference built as a FIVE-stage generator.

Runs only where the reference checkout exists (VISPEECH_REFERENCE; imported read-only, nothing of it is copied), like
make_golden_resblock2.py.  The reference ``SynthesizerTrn`` is built from its unchanged configs/config.json with three
constructor arguments replaced by HiFi-GAN's usual 44.1 kHz / hop 512 vocoder shape:

    upsample_rates [8, 8, 2, 2, 2], upsample_kernel_sizes [16, 16, 4, 4, 4], upsample_initial_channel 512

(stages of 256, 128, 64, 32 and 16 channels; the product of the rates is 512, the configuration's hop_length), loaded
with this repo's seeded synthetic weights and run on CPU with ``torch.randn_like`` patched to return the fixture noise:

  * ``infer`` (reference models.py:672-722) with ``resblock`` "1" on a ragged batch of three utterances with given
    durations / pitch / energy: o, x_mask, z, z_p, m_p, logs_p;
  * the same batch with ``resblock`` "2": the waveform only (``rb2_o``; the latents do not depend on the vocoder).

Every array written is data: inputs, noise, expected outputs, and the reference's state_dict key list with its shapes.

    python tests/golden/make_golden_five_stage.py        # rewrites tests/golden/five_stage.npz
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

WEIGHT_SEED = 1618
FIVE_STAGE = dict(upsample_rates=[8, 8, 2, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4, 4], upsample_initial_channel=512)


def build_reference(resblock):
    hps = ref_utils.get_hparams_from_file(os.path.join(REF, "configs", "config.json"))
    mine = vcfg.default_hparams()
    for k, v in mine.model.items():
        assert hps.model[k] == v, ("config drift", k)
    assert len(ref_symbols) == vcfg.N_SYMBOLS
    assert int(np.prod(FIVE_STAGE["upsample_rates"])) == hps.data.hop_length
    for k, v in FIVE_STAGE.items():
        mine.model[k] = v
    mine.model["resblock"] = resblock
    args, kwargs = vcfg.synthesizer_args(mine, len(ref_symbols))
    net = ref_models.SynthesizerTrn(*args, **kwargs).eval()
    assert type(net.dec.resblocks[0]).__name__ == "ResBlock" + resblock
    assert net.dec.conv_post.in_channels == 16 and len(net.dec.ups) == 5
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
    return net, keys, shapes


class _Noise:
    """Patch ``torch.randn_like`` so the reference consumes the fixture noise (models.py:718)."""

    def __init__(self, noise):
        self.noise = torch.from_numpy(noise)

    def __enter__(self):
        self._orig = torch.randn_like
        torch.randn_like = lambda t, *a, **k: self.noise[:, :, :t.shape[2]].to(t.dtype).clone()
        return self

    def __exit__(self, *exc):
        torch.randn_like = self._orig


def infer_case(net, batch, tag):
    ph = torch.from_numpy(batch["phonemes"])
    with torch.no_grad(), _Noise(batch["noise"]):
        o, x_mask, (z, z_p, m_p, logs_p), _dur, _f0, _en = net.infer(
            ph, torch.from_numpy(batch["lengths"]), sid=torch.from_numpy(batch["sid"]), noise_scale=0.667,
            duration_control=torch.from_numpy(batch["duration"]), pitch_control=torch.from_numpy(batch["f0"]),
            energy_control=torch.from_numpy(batch["energy"]))
    tf = x_mask.shape[2]
    out = {"noise": np.ascontiguousarray(batch["noise"][:, :, :tf]), "o": o.numpy(), "x_mask": x_mask.numpy(),
           "z": z.numpy(), "z_p": z_p.numpy(), "m_p": m_p.numpy(), "logs_p": logs_p.numpy()}
    print(f"resblock {tag}: B={ph.shape[0]} Tf={tf} frames={x_mask.numpy().sum(axis=(1, 2)).astype(int).tolist()} "
          f"o={tuple(out['o'].shape)} |o|max={np.abs(out['o']).max():.4f}")
    return out


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    # three utterances of different lengths (26 / 13 / 30 frames): the 13-frame one ends early enough for a trimmed tail
    batch = synth_batch(3, seed=11, mean_phonemes=8, std_phonemes=3, min_phonemes=4, max_phonemes=12,
                        mean_frames=26, jitter_frames=16)
    net1, keys, shapes = build_reference("1")
    out = dict(weight_seed=np.int64(WEIGHT_SEED), ref_keys=np.array(keys), ref_shapes=shapes,
               in_phonemes=batch["phonemes"], in_lengths=batch["lengths"], in_sid=batch["sid"],
               in_duration=batch["duration"], in_f0=batch["f0"], in_energy=batch["energy"])
    out.update(infer_case(net1, batch, "1"))
    net2, keys2, shapes2 = build_reference("2")
    out["rb2_ref_keys"] = np.array(keys2)
    out["rb2_ref_shapes"] = shapes2
    out["rb2_o"] = infer_case(net2, batch, "2")["o"]
    path = os.path.join(HERE, "five_stage.npz")
    np.savez_compressed(path, **out)
    print(f"five_stage.npz: {len(keys)} / {len(keys2)} keys -> {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
