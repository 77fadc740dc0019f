#!/usr/bin/env python3
"""Loudness measurement and normalisation, measured on the GPU (default configuration, synthetic weights; DESIGN.md section
4p): for 16 rows of 10 s at the model's rate

1. each call alone -- ``Engine.loudness_segments`` (three launches), ``Engine.loudness_gate``, ``Engine.loudness_apply`` --
   and the fused ``Engine.loudness_normalize`` (five launches behind one upload);
2. the ``Engine.generator_ragged`` call whose output the service normalises, beside it.

Device-event times per call (``torch.cuda.Event``) over a window of ``steps`` calls after a warm-up of the same shape; best /
median / spread of ``rounds`` rounds that alternate over the calls.  No gate is set on any of them.

usage: tools/loudness_measure.py [steps] [rounds] [out.txt]      (default out: profiles/r21_loudness.txt)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vispeech_amd import config as vcfg                 # noqa: E402
from vispeech_amd.models import SynthesizerTrn          # noqa: E402
from vispeech_amd.schema import dims_from_ctor          # noqa: E402
from vispeech_amd.synth import synth_state_dict         # noqa: E402

STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "r21_loudness.txt")
SECONDS, B = 10, 16


def timed(fn, steps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def fmt(v):
    return f"best {min(v):8.3f} ms  median {float(np.median(v)):8.3f} ms  spread {max(v) - min(v):6.3f} ms"


def main():
    a, kw0 = vcfg.synthesizer_args(vcfg.default_hparams())
    dims = dims_from_ctor(*a, **kw0)
    net = SynthesizerTrn(*a, device="cuda:0", **kw0).eval()
    net.load_state_dict(synth_state_dict(dims, seed=1234))
    eng, fs, up = net._engine, dims.sampling_rate, dims.total_upsample
    frames = SECONDS * fs // up
    n = frames * up
    r = np.random.default_rng(21)
    # the generator call that feeds the normalisation: 16 latents of 10 s
    sid = torch.arange(B, device="cuda:0") % dims.n_speakers
    enc = eng.encode(torch.ones((B, 2), dtype=torch.int64, device="cuda:0"), torch.full((B,), 2, dtype=torch.int64, device="cuda:0"),
                     sid, isolated=True)
    G = torch.stack([enc["g"][b].reshape(-1) for b in range(B)])
    Z = torch.from_numpy(0.5 * r.standard_normal((B, dims.inter_channels, frames)).astype(np.float32)).to("cuda:0")
    lengths = [frames] * B
    # the rows measured: voiced glides at different levels (the generator's output under synthetic weights is no speech)
    t = np.arange(n) / fs
    rows = np.stack([10.0 ** (-r.uniform(6.0, 30.0) / 20.0) * np.sin(2.0 * np.pi * np.cumsum(r.uniform(110.0, 260.0) + 40.0 *
                     np.sin(2.0 * np.pi * r.uniform(0.5, 2.0) * t)) / fs) for _ in range(B)]).astype(np.float32)
    audio = torch.from_numpy(rows).to("cuda:0")
    n_samples = [n] * B
    params = eng.loudness_params(B, -23.0, 1.0, 30.0)
    seg, peak = eng.loudness_segments(audio, n_samples, fs)
    lufs, blocks, gains = eng.loudness_gate(seg, n_samples, fs, peak=peak, params=params)
    out = torch.empty_like(audio)
    again, _, _ = eng.loudness(eng.loudness_normalize(audio, n_samples, fs, params, out=out)[0], n_samples, fs)
    before, after = lufs.cpu().numpy(), again.cpu().numpy()
    assert np.abs(after + 23.0).max() < 1e-3, after

    jobs = {
        "loudness_segments": lambda: eng.loudness_segments(audio, n_samples, fs),
        "loudness_gate": lambda: eng.loudness_gate(seg, n_samples, fs, peak=peak, params=params),
        "loudness_apply": lambda: eng.loudness_apply(audio, n_samples, gains, params=params, out=out),
        "loudness_normalize (fused)": lambda: eng.loudness_normalize(audio, n_samples, fs, params, out=out),
        "generator_ragged": lambda: eng.generator_ragged(Z, G, lengths),
    }
    ms = {k: [] for k in jobs}
    for _ in range(ROUNDS):
        for k, fn in jobs.items():
            ms[k].append(timed(fn, max(STEPS // 2, 2) if k == "generator_ragged" else STEPS))
    med = lambda k: float(np.median(ms[k]))
    props = torch.cuda.get_device_properties(0)
    h = (fs + 5) // 10
    lines = [f"loudness: {B} rows of {SECONDS} s at {fs} Hz ({n} samples, {-(-n // h)} segments of {h} samples each; lane runs of "
             f"{-(-h // 64)} samples); {ROUNDS} rounds, a window of {STEPS} calls ({max(STEPS // 2, 2)} for generator_ragged)",
             f"device {torch.cuda.get_device_name(0)} ({getattr(props, 'gcnArchName', 'arch not available')}, "
             f"{props.multi_processor_count} CUs)",
             "timer: device events around a window of calls, per call (the Engine calls include their host work and uploads)", ""]
    for k in jobs:
        lines.append(f"   {k:27s} {fmt(ms[k])}")
    lines += ["",
              f"   segments: {B * n / 1e6:.2f} M samples a call = {B * n / med('loudness_segments') / 1e6:.2f} G samples/s, three runs "
              f"of the recurrence a sample; audio read twice: {2 * 4 * B * n / med('loudness_segments') / 1e6:.1f} GB/s",
              f"   apply: {2 * 4 * B * n / med('loudness_apply') / 1e6:.1f} GB/s read + written",
              f"   loudness_normalize / generator_ragged = {med('loudness_normalize (fused)') / med('generator_ragged') * 100:.2f} %",
              f"   rows before {before.min():.2f} .. {before.max():.2f} LUFS; after, measured again: {after.min():.4f} .. {after.max():.4f} LUFS"]
    assert eng.status() == 0
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
