#!/usr/bin/env python3
"""The true-peak meter and the look-ahead limiter, measured on the GPU (default configuration, synthetic weights; DESIGN.md
section 4q): for 16 rows of 10 s at the model's rate

1. ``Engine.true_peak`` (one launch) and ``Engine.limit`` (two launches) at 1.5 ms attack and 20 ms hold, and at the
   largest window (1024, 8192);
2. ``normalize_loudness(limiter=True)`` -- ``Engine.loudness_limit``: segments, gate, limiter -- beside the peak-cut
   ``Engine.loudness_normalize`` on the same rows and the ``Engine.generator_ragged`` call that produces such rows.

Device-event times per call (``torch.cuda.Event``) over a window of ``steps`` calls after a warm-up of the same shape; best /
median / spread of ``rounds`` rounds that alternate over the calls.  No gate is set on any of them.  The bytes the two
launches of the limiter must move are 20 a sample (x in, r out; r in, x in, out); their rate is set against the 6.3 TB/s
a copy kernel reaches on this part.

usage: tools/limiter_measure.py [steps] [rounds] [out.txt]      (default out: profiles/r22_limiter.txt)"""
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
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "r22_limiter.txt")
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
    r = np.random.default_rng(22)
    # the generator call that feeds the normalisation: 16 latents of 10 s
    sid = torch.arange(B, device="cuda:0") % dims.n_speakers
    enc = eng.encode(torch.ones((B, 2), dtype=torch.int64, device="cuda:0"), torch.full((B,), 2, dtype=torch.int64, device="cuda:0"),
                     sid, isolated=True)
    G = torch.stack([enc["g"][b].reshape(-1) for b in range(B)])
    Z = torch.from_numpy(0.5 * r.standard_normal((B, dims.inter_channels, frames)).astype(np.float32)).to("cuda:0")
    lengths = [frames] * B
    # the rows measured: voiced glides at different levels with a click a second (the generator's output under synthetic
    # weights is no speech)
    t = np.arange(n) / fs
    rows = np.stack([10.0 ** (-r.uniform(6.0, 30.0) / 20.0) * np.sin(2.0 * np.pi * np.cumsum(r.uniform(110.0, 260.0) + 40.0 *
                     np.sin(2.0 * np.pi * r.uniform(0.5, 2.0) * t)) / fs) for _ in range(B)]).astype(np.float32)
    rows[:, fs // 2::fs] += np.float32(0.8)
    audio = torch.from_numpy(rows).to("cuda:0")
    n_samples = [n] * B
    params = eng.loudness_params(B, -23.0, 0.9, 30.0)
    A, H = 66, 882
    out = torch.empty_like(audio)
    tp = eng.true_peak(audio, n_samples).cpu().numpy()
    _, gains_cut, lufs, peak, _ = eng.loudness_normalize(audio, n_samples, fs, params, out=out)
    after_cut = eng.loudness(out, n_samples, fs)[0].cpu().numpy()
    _, gains, _, _, _, mg = eng.loudness_limit(audio, n_samples, fs, params, attack=A, hold=H, out=out)
    after_lim = eng.loudness(out, n_samples, fs)[0].cpu().numpy()
    tp_out = eng.true_peak(out, n_samples).cpu().numpy()
    assert float(out.abs().max()) <= np.float32(0.9)

    jobs = {
        "true_peak": lambda: eng.true_peak(audio, n_samples),
        "limit (66, 882)": lambda: eng.limit(audio, n_samples, 0.9, gains=gains, attack=A, hold=H, out=out),
        "limit (1024, 8192)": lambda: eng.limit(audio, n_samples, 0.9, gains=gains, attack=1024, hold=8192, out=out),
        "loudness_limit": lambda: eng.loudness_limit(audio, n_samples, fs, params, attack=A, hold=H, out=out),
        "loudness_normalize (peak cut)": lambda: eng.loudness_normalize(audio, n_samples, fs, params, out=out),
        "generator_ragged": lambda: eng.generator_ragged(Z, G, lengths),
    }
    ms = {k: [] for k in jobs}
    for _ in range(ROUNDS):
        for k, fn in jobs.items():
            ms[k].append(timed(fn, max(STEPS // 2, 2) if k == "generator_ragged" else STEPS))
    med = lambda k: float(np.median(ms[k]))
    props = torch.cuda.get_device_properties(0)
    HBM = 6.3e12
    lines = [f"limiter: {B} rows of {SECONDS} s at {fs} Hz ({n} samples); {ROUNDS} rounds, a window of {STEPS} calls "
             f"({max(STEPS // 2, 2)} for generator_ragged)",
             f"device {torch.cuda.get_device_name(0)} ({getattr(props, 'gcnArchName', 'arch not available')}, "
             f"{props.multi_processor_count} CUs)",
             "timer: device events around a window of calls, per call (the Engine calls include their host work and uploads)", ""]
    for k in jobs:
        lines.append(f"   {k:30s} {fmt(ms[k])}")
    rate = lambda k, bytes_per_sample: bytes_per_sample * B * n / (med(k) * 1e-3)
    lines += ["",
              f"   true_peak: 4 B a sample: {rate('true_peak', 4) / 1e9:.1f} GB/s = {rate('true_peak', 4) / HBM * 100:.2f} % of 6.3 TB/s; "
              f"{97 * 2 * B * n / med('true_peak') / 1e6:.0f} GFLOP/s of the four chains",
              f"   limit (66, 882): 20 B a sample: {rate('limit (66, 882)', 20) / 1e9:.1f} GB/s = {rate('limit (66, 882)', 20) / HBM * 100:.2f} % of 6.3 TB/s",
              f"   limit (1024, 8192): {rate('limit (1024, 8192)', 20) / 1e9:.1f} GB/s = {rate('limit (1024, 8192)', 20) / HBM * 100:.2f} % of 6.3 TB/s "
              f"(a tile of 2048 outputs reads 12288 values of r and sums 1025 values an output)",
              f"   loudness_limit / loudness_normalize = {med('loudness_limit') / med('loudness_normalize (peak cut)'):.2f}; "
              f"loudness_limit / generator_ragged = {med('loudness_limit') / med('generator_ragged') * 100:.2f} %",
              f"   rows before {lufs.cpu().numpy().min():.2f} .. {lufs.cpu().numpy().max():.2f} LUFS, true peak {tp.min():.3f} .. {tp.max():.3f}; target -23 LUFS, ceiling 0.9",
              f"   cut by the peak: gains {gains_cut.cpu().numpy().min():.3f} .. {gains_cut.cpu().numpy().max():.3f}, measured again "
              f"{after_cut.min():.3f} .. {after_cut.max():.3f} LUFS",
              f"   with the limiter: gains {gains.cpu().numpy().min():.3f} .. {gains.cpu().numpy().max():.3f}, smallest limiter gain "
              f"{mg.cpu().numpy().min():.3f}, measured again {after_lim.min():.3f} .. {after_lim.max():.3f} LUFS; true peak of the "
              f"output at most {20 * np.log10(tp_out.max() / 0.9):+.4f} dB re the ceiling"]
    assert eng.status() == 0
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
