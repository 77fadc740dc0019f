#!/usr/bin/env python3
"""Prosody from a recording, measured on the GPU (default configuration, synthetic weights): for 16 recordings of 10 s

1. ``Engine.prosody_contours`` and ``Engine.prosody_phonemes`` (31 phonemes per row), each call and the pair;
2. the ``SynthesizerTrn.convert_audio`` call on the same recordings, and the pair's share of it;
3. the fp64 numpy restatement (tests/prosody_ref.py) on the host for ONE of the recordings.

The GPU figures are device-event times per call (``torch.cuda.Event``) over a window of ``steps`` calls after a warm-up of
the same shape; best / median / spread of ``rounds`` rounds that alternate over the calls.  No gate is set on any of them.

``--path`` measures the path finder instead: the contour call without and with the path, the
candidate call and the path alone on its tables, the same recordings, timer and rounds.

usage: tools/prosody_measure.py [--path] [steps] [rounds] [out.txt]
       (default out: profiles/r18_prosody.txt, with --path profiles/r19_prosody_path.txt)"""
import os
import platform
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import prosody_ref as ref                               # noqa: E402
from vispeech_amd import config as vcfg                 # noqa: E402
from vispeech_amd.models import SynthesizerTrn          # noqa: E402
from vispeech_amd.schema import dims_from_ctor          # noqa: E402
from vispeech_amd.synth import synth_state_dict         # noqa: E402

PATH = "--path" in sys.argv[1:]
ARGS = [a for a in sys.argv[1:] if a != "--path"]
STEPS = int(ARGS[0]) if len(ARGS) > 0 else 10
ROUNDS = int(ARGS[1]) if len(ARGS) > 1 else 3
OUT = ARGS[2] if len(ARGS) > 2 else os.path.join(ROOT, "profiles", "r19_prosody_path.txt" if PATH else "r18_prosody.txt")
SECONDS, B, TP = 10, 16, 31


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


def recordings(n, seed=18):
    """Voiced glides with pauses and a little noise: every frame runs the whole analysis, as speech does."""
    r = np.random.default_rng(seed)
    t = np.arange(n) / ref.FS
    rows = []
    for b in range(B):
        f = r.uniform(110.0, 260.0) + 40.0 * np.sin(2.0 * np.pi * r.uniform(0.5, 2.0) * t)
        x = ref.harmonic(f, n, partials=10) + 0.01 * r.standard_normal(n)
        for _ in range(4):
            p = int(r.integers(0, n - 22050))
            x[p: p + int(r.integers(4410, 22050))] *= 0.0
        rows.append(x)
    return np.stack(rows).astype(np.float32)


def fmt(v):
    return f"best {min(v):8.3f} ms  median {float(np.median(v)):8.3f} ms  spread {max(v) - min(v):6.3f} ms"


def measure_path(net, dims, audio, n_samples):
    """The contour call without and with the path finder, and the two halves of the latter on their own."""
    eng = net._engine
    F = n_samples[0] // dims.hop_length + 1
    cand_f, cand_s, _, _, frames_host = eng.prosody_candidates(audio, n_samples)
    f0 = eng.prosody_contours(audio, n_samples)[0]
    p0 = eng.prosody_contours(audio, n_samples, path=True)[0]
    z0 = eng.prosody_contours(audio, n_samples, path=(0.0, 0.0, 15))[0]
    assert torch.equal(z0, f0), "with both costs 0 the path must be the per-frame decision"
    changed = int((p0 != f0).sum())
    jobs = {
        "prosody_contours": lambda: eng.prosody_contours(audio, n_samples),
        "prosody_contours(path=True)": lambda: eng.prosody_contours(audio, n_samples, path=True),
        "prosody_candidates": lambda: eng.prosody_candidates(audio, n_samples),
        "prosody_path (alone)": lambda: eng.prosody_path(cand_f, cand_s, frames_host),
    }
    ms = {k: [] for k in jobs}
    for _ in range(ROUNDS):
        for k, fn in jobs.items():
            ms[k].append(timed(fn, STEPS))
    med = lambda k: float(np.median(ms[k]))
    props = torch.cuda.get_device_properties(0)
    lines = [f"prosody path finder: default configuration ({dims.sampling_rate} Hz, hop {dims.hop_length}), {B} recordings of "
             f"{SECONDS} s ({F} frames each); defaults (octave jump 0.35, voiced/unvoiced 0.14, 15 candidates); {ROUNDS} rounds, "
             f"a window of {STEPS} calls",
             f"device {torch.cuda.get_device_name(0)} ({getattr(props, 'gcnArchName', 'arch not available')}, "
             f"{props.multi_processor_count} CUs), host {platform.node()}",
             "timer: device events around a window of calls, per call", ""]
    for k in jobs:
        lines.append(f"   {k:29s} {fmt(ms[k])}")
    lines += ["",
              f"   the path adds {med('prosody_contours(path=True)') - med('prosody_contours'):.3f} ms to the contour call (medians): "
              f"{med('prosody_candidates') - med('prosody_contours'):+.3f} ms in the candidate kernel's tail and its tables, "
              f"{med('prosody_path (alone)'):.3f} ms the path kernel ({B} waves, {F} frames each in sequence: "
              f"{med('prosody_path (alone)') / F * 1e3:.2f} us per frame, forward and backward)",
              f"   frames whose F0 the path changes: {changed} of {B * F}; with both costs 0: none, bit for bit"]
    assert eng.status() == 0
    return "\n".join(lines)


def main():
    a, kw0 = vcfg.synthesizer_args(vcfg.default_hparams())
    dims = dims_from_ctor(*a, **kw0)
    net = SynthesizerTrn(*a, device="cuda:0", **kw0).eval()
    net.load_state_dict(synth_state_dict(dims, seed=1234))
    eng = net._engine
    n = SECONDS * dims.sampling_rate
    host = recordings(n)
    audio = torch.from_numpy(host).to("cuda:0")
    n_samples = [n] * B
    if PATH:
        text = measure_path(net, dims, audio, n_samples)
        print(text)
        os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
        with open(OUT, "w") as f:
            f.write(text + "\n")
        return
    F = n // dims.hop_length + 1
    dur = np.full((B, TP), F // TP, np.int64)
    lengths = [TP] * B
    src, tgt = [b % dims.n_speakers for b in range(B)], [(b + 7) % dims.n_speakers for b in range(B)]
    seeds = list(range(100, 100 + B))
    f0f, enf, _, frames_host = eng.prosody_contours(audio, n_samples)
    voiced = float((f0f > 0).float().mean())

    jobs = {
        "prosody_contours": lambda: eng.prosody_contours(audio, n_samples),
        "prosody_phonemes": lambda: eng.prosody_phonemes(f0f, enf, frames_host, dur, lengths),
        "both (prosody_from_audio)": lambda: net.prosody_from_audio(audio, n_samples, dur, lengths),
        "convert_audio": lambda: net.convert_audio(audio, n_samples, src, tgt, noise_seed=seeds),
    }
    ms = {k: [] for k in jobs}
    for _ in range(ROUNDS):
        for k, fn in jobs.items():
            ms[k].append(timed(fn, max(STEPS // 2, 2) if k == "convert_audio" else STEPS))
    host_s = []
    for _ in range(3):
        t0 = time.perf_counter()
        ref.prosody(host[0], dur[0])
        host_s.append(time.perf_counter() - t0)

    med = lambda k: float(np.median(ms[k]))
    props = torch.cuda.get_device_properties(0)
    W = ref.window_samples(80.0)
    macs = F * (W * 497 + W)          # lags 57 .. 553 and lag 0, per frame
    lines = [f"prosody: default configuration ({dims.sampling_rate} Hz, hop {dims.hop_length}), {B} recordings of {SECONDS} s "
             f"({F} frames each, {voiced * 100:.0f} % voiced), {TP} phonemes per row; {ROUNDS} rounds, a window of {STEPS} calls "
             f"({max(STEPS // 2, 2)} for convert_audio)",
             f"device {torch.cuda.get_device_name(0)} ({getattr(props, 'gcnArchName', 'arch not available')}, "
             f"{props.multi_processor_count} CUs), host {platform.node()}",
             "timer: device events around a window of calls, per call", ""]
    for k in jobs:
        lines.append(f"   {k:27s} {fmt(ms[k])}")
    lines += ["",
              f"   the two calls / convert_audio = {med('both (prosody_from_audio)') / med('convert_audio') * 100:.2f} %",
              f"   autocorrelation work: {macs / 1e9:.2f} GMAC per row, {B * macs / 1e9:.1f} per call = "
              f"{2 * B * macs / med('prosody_contours') / 1e9:.1f} TFLOP/s (fp32 vector FMA) over the contour call",
              f"   fp64 numpy restatement on the host, ONE recording: best {min(host_s) * 1e3:.1f} ms, median "
              f"{float(np.median(host_s)) * 1e3:.1f} ms (FFT autocorrelation; {B} recordings cost {B} times that)"]
    assert eng.status() == 0
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
