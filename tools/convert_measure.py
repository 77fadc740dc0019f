#!/usr/bin/env python3
"""Conversion from audio, measured on the GPU: 16 recordings of about 5 s with mixed lengths (3.5 .. 6.5 s at 44.1 kHz).

1. one ``Engine.convert`` call (ragged front end, one posterior / flow pass, one ragged generator call) against 16 B = 1
   runs of the existing ``spectrogram`` + ``voice_conversion(isolated=True)``;
2. the ragged front end alone (``spectrogram_ragged``) against ``spectrogram`` at the same padded shape;
3. a streaming service with 8 text rows and 8 conversion rows sharing its ticks against two services of 8, one per kind:
   wall time from the first ``step()`` to the last, admission included.

Every timing is a host clock (``time.perf_counter``) around work that ends in a device synchronise; the two sides of a
comparison run in the SAME process in alternating rounds, each after its own warm-up, and the spread of the rounds is
printed beside the difference.  The file names the device (name, architecture, CUs, PCI bus id, uuid), the host, the
timer, the device's peak engine clock and the engine clock sampled (read-only ``rocm-smi --showclocks``) while the timed
loops ran; where a source is not available the file says "not available", never a guess.

usage: tools/convert_measure.py [steps] [rounds] [out.txt]     (default out: profiles/r14_convert.txt)"""
import ctypes
import os
import platform
import re
import subprocess
import sys
import threading
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vispeech_amd import config as vcfg                 # noqa: E402
from vispeech_amd.models import SynthesizerTrn          # noqa: E402
from vispeech_amd.schema import dims_from_ctor          # noqa: E402
from vispeech_amd.service import StreamingBatchService  # noqa: E402
from vispeech_amd.synth import synth_batch, synth_state_dict  # noqa: E402

STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "r14_convert.txt")
B, RATE = 16, 44100


class ClockSampler:
    """Engine clock (sclk, MHz) sampled while the body runs (as tools/five_stage_measure.py); no samples where rocm-smi is
    not available."""

    def __init__(self):
        self.samples, self._stop = [], threading.Event()

    def _run(self):
        while not self._stop.is_set():
            try:
                out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=5).stdout
                m = re.search(r"sclk clock level: \S+ \((\d+)Mhz\)", out)
                if m:
                    self.samples.append(int(m.group(1)))
            except Exception:
                return
            self._stop.wait(0.2)

    def __enter__(self):
        self._t = threading.Thread(target=self._run, daemon=True)
        self._t.start()
        return self

    def __exit__(self, *exc):
        self._stop.set()
        self._t.join(timeout=10)

    def line(self):
        if not self.samples:
            return "engine clock under load: not available (rocm-smi --showclocks gave no sclk)"
        return (f"engine clock under load (rocm-smi --showclocks, {len(self.samples)} samples over the timed loops): median "
                f"{float(np.median(self.samples)):.0f} MHz, min {min(self.samples)} MHz, max {max(self.samples)} MHz")


def peak_clock_mhz():
    """hipDeviceGetAttribute(hipDeviceAttributeClockRate) of device 0 in MHz, or None."""
    try:
        v = ctypes.c_int(0)
        rc = ctypes.CDLL("libamdhip64.so").hipDeviceGetAttribute(ctypes.byref(v), 5, 0)     # 5: hipDeviceAttributeClockRate, kHz
        return v.value / 1e3 if rc == 0 and v.value > 0 else None
    except Exception:
        return None


def recordings(r):
    n = r.integers(int(3.5 * RATE), int(6.5 * RATE), size=B)
    t = np.arange(int(n.max())) / RATE
    audio = (0.4 * np.sin(2 * np.pi * 220.0 * t)[None, :] * r.uniform(0.2, 1.0, (B, 1)) +
             0.1 * r.standard_normal((B, t.size))).astype(np.float32).clip(-1, 1)
    for b, k in enumerate(n):
        audio[b, k:] = 0.0
    return audio, [int(x) for x in n]


def timed(fn, steps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def ab(name_a, fn_a, name_b, fn_b, steps, rounds):
    ms = {name_a: [], name_b: []}
    for _ in range(rounds):
        for name, fn in ((name_a, fn_a), (name_b, fn_b)):
            ms[name].append(timed(fn, steps))
    lines = [f"  {name:58s} best {min(v):8.3f} ms   median {float(np.median(v)):8.3f} ms   spread {max(v) - min(v):6.3f} ms"
             for name, v in ms.items()]
    a, b = min(ms[name_a]), min(ms[name_b])
    lines.append(f"  {name_a} / {name_b} (best of rounds): {a / b:.3f}x ({a - b:+.3f} ms); run-to-run spread "
                 f"{max(max(v) - min(v) for v in ms.values()):.3f} ms")
    return lines


def main():
    a, kw0 = vcfg.synthesizer_args(vcfg.default_hparams())
    dims = dims_from_ctor(*a, **kw0)
    net = SynthesizerTrn(*a, device="cuda:0", **kw0).eval()
    net.load_state_dict(synth_state_dict(dims, seed=1234))
    eng = net._engine
    r = np.random.Generator(np.random.PCG64(14))
    audio, n = recordings(r)
    frames = [eng.convert_frames(x) for x in n]
    src, tgt = r.integers(0, dims.n_speakers, B), r.integers(0, dims.n_speakers, B)
    seeds = list(range(1000, 1000 + B))
    dev_audio = torch.from_numpy(audio).to("cuda:0")
    rows = [dev_audio[b:b + 1, : n[b]].contiguous() for b in range(B)]
    noise = [eng.randn(seeds[b], 1, dims.inter_channels, frames[b]) for b in range(B)]
    one = lambda v, b: torch.tensor([int(v[b])], device="cuda:0")
    ids = [(one(frames, b), one(src, b), one(tgt, b)) for b in range(B)]
    props = torch.cuda.get_device_properties(0)
    peak = peak_clock_mhz()
    lines = [f"conversion from audio: {B} recordings, {min(n) / RATE:.2f} .. {max(n) / RATE:.2f} s ({min(frames)} .. {max(frames)} frames, "
             f"{100 * (1 - sum(frames) / (B * max(frames))):.1f} % padding), {STEPS} steps x {ROUNDS} alternating rounds",
             f"device {torch.cuda.get_device_name(0)} ({getattr(props, 'gcnArchName', 'arch not available')}, "
             f"{props.multi_processor_count} CUs, PCI {getattr(props, 'pci_bus_id', 0):02x}, uuid {getattr(props, 'uuid', 'not available')}), "
             f"host {platform.node()}",
             "peak engine clock (hipDeviceAttributeClockRate): " + (f"{peak:.0f} MHz" if peak else "not available"),
             "timer: time.perf_counter around a synchronised window, per call", ""]
    sampler = ClockSampler()
    sampler.__enter__()

    def batched():
        eng.convert(dev_audio, n, src, tgt, noise_seed=seeds)

    def one_by_one():
        for b in range(B):
            y = eng.spectrogram(rows[b])
            eng.voice_conversion(y, ids[b][0], ids[b][1], ids[b][2], noise[b], isolated=True)

    lines.append("1. audio to audio")
    lines += ab("one convert call (B = 16, ragged)", batched, "16 x (spectrogram + voice_conversion(isolated), B = 1)",
                one_by_one, STEPS, ROUNDS)
    lines += ["", "2. front end alone, same padded shape"]
    lines += ab("spectrogram_ragged (LDS-staged framing)", lambda: eng.spectrogram_ragged(dev_audio, n),
                "spectrogram (vsp_spectrogram)", lambda: eng.spectrogram(dev_audio), 5 * STEPS, ROUNDS)

    # 3. streaming: 8 text rows + 8 conversion rows
    text = synth_batch(8, seed=15)
    collate = lambda rr: {k: text[k][rr] for k in ("phonemes", "lengths", "sid", "duration", "f0", "energy")}

    def serve(kinds):
        svcs = []
        for kind in kinds:
            svc = StreamingBatchService(net, max_batch=16, chunk_frames=64, collate=collate, autostart=False)
            streams = []
            if "text" in kind:
                streams += [svc.submit(b, 2000 + b) for b in range(8)]
            if "conv" in kind:
                streams += [svc.submit_conversion(audio[b, : n[b]], int(src[b]), int(tgt[b]), seeds[b]) for b in range(8)]
            svcs.append((svc, streams))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for svc, _ in svcs:
            while svc.step():
                pass
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        ticks = sum(svc.stats["ticks"] for svc, _ in svcs)
        assert all(sum(len(p) for p in s) > 0 for _, ss in svcs for s in ss)
        return ms, ticks

    res = {"mixed": [], "split": []}
    for k in range(ROUNDS + 1):
        for name, kinds in (("mixed", [("text", "conv")]), ("split", [("text",), ("conv",)])):
            v = serve(kinds)
            if k:                                    # (round 0 is the warm-up of both)
                res[name].append(v)
    lines += ["", "3. streaming, chunk_frames = 64, every request submitted before the first tick, first step() to last"]
    for name, label in (("mixed", "one service: 8 text + 8 conversion rows per tick"),
                        ("split", "two services of 8 (text, then conversion)")):
        ms = [v[0] for v in res[name]]
        lines.append(f"  {label:58s} best {min(ms):8.3f} ms   median {float(np.median(ms)):8.3f} ms   spread "
                     f"{max(ms) - min(ms):6.3f} ms   {res[name][0][1]} ticks ({min(ms) / res[name][0][1]:.3f} ms per tick)")
    m, s = min(v[0] for v in res["mixed"]), min(v[0] for v in res["split"])
    lines.append(f"  mixed / split (best of rounds): {m / s:.3f}x ({m - s:+.3f} ms)")
    sampler.__exit__()
    lines += ["", sampler.line()]
    assert eng.status() == 0
    text_out = "\n".join(lines)
    print(text_out)
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        f.write(text_out + "\n")


if __name__ == "__main__":
    main()
