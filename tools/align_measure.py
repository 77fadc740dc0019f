#!/usr/bin/env python3
"""Durations from a recording, measured on the GPU (default configuration, synthetic weights): for 16
recordings of 10 s and texts of 120 phonemes

1. the three launches on the tensors ``align_audio`` hands them -- ``Engine.align_scores``, ``Engine.align_path``,
   ``Engine.align_durations`` -- and the fused ``Engine.align``; the path kernel's time per frame;
2. ``SynthesizerTrn.align_audio`` as a whole (two encodes, ``decode(max_len=0)``, ``convert_latent``, ``align``);
3. ``SynthesizerTrn.convert_audio`` on the same recordings, beside it.

Device-event times per call (``torch.cuda.Event``) over a window of ``steps`` calls after a warm-up of the same shape; best /
median / spread of ``rounds`` rounds that alternate over the calls.  No gate is set on any of them.  The weights are
synthetic: the figures are times, not alignment quality.

usage: tools/align_measure.py [steps] [rounds] [out.txt]      (default out: profiles/r20_align.txt)"""
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
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "r20_align.txt")
SECONDS, B, TP = 10, 16, 120


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


def recordings(n, rate, seed=20):
    """Voiced glides under a slow envelope with a little noise."""
    r = np.random.default_rng(seed)
    t = np.arange(n) / rate
    rows = []
    for _ in range(B):
        f = r.uniform(110.0, 260.0) + 40.0 * np.sin(2.0 * np.pi * r.uniform(0.5, 2.0) * t)
        x = 0.4 * np.sin(2.0 * np.pi * np.cumsum(f) / rate) * (0.5 + 0.5 * np.sin(2.0 * np.pi * r.uniform(0.5, 3.0) * t) ** 2)
        rows.append(x + 0.01 * r.standard_normal(n))
    return np.stack(rows).astype(np.float32)


def fmt(v):
    return f"best {min(v):8.3f} ms  median {float(np.median(v)):8.3f} ms  spread {max(v) - min(v):6.3f} ms"


def main():
    a, kw0 = vcfg.synthesizer_args(vcfg.default_hparams())
    dims = dims_from_ctor(*a, **kw0)
    net = SynthesizerTrn(*a, device="cuda:0", **kw0).eval()
    net.load_state_dict(synth_state_dict(dims, seed=1234))
    eng = net._engine
    n = SECONDS * dims.sampling_rate
    audio = torch.from_numpy(recordings(n, dims.sampling_rate)).to("cuda:0")
    n_samples = [n] * B
    r = np.random.default_rng(21)
    ph = torch.from_numpy(r.integers(1, dims.n_vocab, (B, TP))).to("cuda:0")
    ln = torch.full((B,), TP, dtype=torch.int64, device="cuda:0")
    sid = torch.arange(B, device="cuda:0") % dims.n_speakers
    src, tgt = [b % dims.n_speakers for b in range(B)], [(b + 7) % dims.n_speakers for b in range(B)]
    seeds = list(range(100, 100 + B))

    # the tensors align_audio hands the three launches
    from types import SimpleNamespace
    frames = [eng.convert_frames(v) for v in n_samples]
    enc = eng.encode(ph, ln, sid, isolated=True)
    states, _ = eng.frame_lengths_host(enc["frame_lengths"])
    predicted = list(states)
    one, flat = np.ones(B, np.float32), np.zeros(B, np.float32)
    rows = SimpleNamespace(duration_scale=np.array([frames[b] / max(states[b], 1) for b in range(B)], np.float32), pitch_scale=one,
                           energy_scale=one, noise_scale=flat, given=np.zeros((B, 3), bool))
    enc = eng.encode(ph, ln, sid, isolated=True, row_controls=rows)
    states, tf = eng.frame_lengths_host(enc["frame_lengths"])
    dec = eng.decode(enc, tf, None, 0.0, max_len=0, isolated=True, row_controls=rows)
    lat = eng.convert_latent(audio, n_samples, sid, sid, noise_scale=0.0)
    x, m, logs, cum = lat["z_p"], dec["m_p"], dec["logs_p"], enc["cum_dur"].cpu().numpy()
    S = eng.align_scores(x, m, logs, frames, states)
    path = eng.align_path(S, frames, states)
    dur = net.align_audio(ph, ln, sid, audio, n_samples)
    assert torch.equal(dur, eng.align_durations(path, frames, cum, ln).to(torch.int64))
    assert [int(v) for v in dur.sum(dim=1)] == frames
    F, K, C = max(frames), max(states), x.shape[1]

    jobs = {
        "align_scores": lambda: eng.align_scores(x, m, logs, frames, states),
        "align_path": lambda: eng.align_path(S, frames, states),
        "align_durations": lambda: eng.align_durations(path, frames, cum, ln),
        "align (the three, fused)": lambda: eng.align(x, m, logs, frames, states, cum, ln),
        "align_audio": lambda: net.align_audio(ph, ln, sid, audio, n_samples),
        "convert_audio": lambda: net.convert_audio(audio, n_samples, src, tgt, noise_seed=seeds),
    }
    ms = {k: [] for k in jobs}
    for _ in range(ROUNDS):
        for k, fn in jobs.items():
            ms[k].append(timed(fn, max(STEPS // 2, 2) if k in ("convert_audio", "align_audio") else STEPS))
    med = lambda k: float(np.median(ms[k]))
    props = torch.cuda.get_device_properties(0)
    triples = sum(f * k for f, k in zip(frames, states)) * C
    lines = [f"align: default configuration ({dims.sampling_rate} Hz, hop {dims.hop_length}), {B} recordings of {SECONDS} s "
             f"({F} frames each), texts of {TP} phonemes (predicted {min(predicted)} .. {max(predicted)} template frames; with "
             f"fit_length {min(states)} .. {max(states)} states), {C} channels; max_advance 2, costs 0; {ROUNDS} rounds, a window of "
             f"{STEPS} calls ({max(STEPS // 2, 2)} for align_audio and convert_audio)",
             f"device {torch.cuda.get_device_name(0)} ({getattr(props, 'gcnArchName', 'arch not available')}, "
             f"{props.multi_processor_count} CUs)",
             "timer: device events around a window of calls, per call (the Engine calls include their host work and uploads)", ""]
    for k in jobs:
        lines.append(f"   {k:27s} {fmt(ms[k])}")
    lines += ["",
              f"   scores: {triples / 1e9:.2f} G difference-square-FMA triples per call = "
              f"{3 * triples / med('align_scores') / 1e9:.1f} TFLOP/s counting three operations a triple (fp32 vector pipe)",
              f"   path: {B} blocks, {F} frames each in sequence, forward and backward: {med('align_path') / F * 1e3:.2f} us per frame "
              f"({(K + 3) // 4} threads of 4 states)",
              f"   align_audio / convert_audio = {med('align_audio') / med('convert_audio') * 100:.1f} %; the three launches are "
              f"{med('align (the three, fused)') / med('align_audio') * 100:.1f} % of align_audio",
              "   synthetic weights: these are times; alignment quality on a trained checkpoint is not measured here"]
    assert eng.status() == 0
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
