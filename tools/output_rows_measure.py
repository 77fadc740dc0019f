#!/usr/bin/env python3
"""Output rows, measured on the GPU (default configuration, synthetic weights).

1. 16 waveforms of 10 s at the model's rate, delivered at 8000 Hz, both ways in the same process:
   (a) the single stage: ``configure_output(8000)`` once, then per request one ``output_chunk(pcm=True)`` launch and one
       device-to-host copy (PCM16: the single stage has no G.711 step, so none is charged);
   (b) ONE ``output_rows`` call of 16 mu-law rows and one copy.
   Both include their copies to the host and end in a synchronise; the bytes of (b) are checked against
   ``output_stage.encode`` of (a)'s.
2. ``output_rows`` beside the generator call that feeds it: ``generator_ragged`` of 16 utterances of 2 s (device time,
   no copy), and the ``output_rows`` call over its waveforms.
3. A mixed group of 64 short rows (0.1 s each, 5 rates x 4 encodings) in one call against 64 solo calls, copies included.

Every figure is a device-event time per call (``torch.cuda.Event``) over a window of ``steps`` calls after a warm-up of the
same shape; rounds alternate over the configurations, and best / median / spread of the rounds are printed.

usage: tools/output_rows_measure.py [steps] [rounds] [out.txt]     (default out: profiles/r17_output_rows.txt)"""
import os
import platform
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vispeech_amd import config as vcfg, output_stage   # noqa: E402
from vispeech_amd.models import SynthesizerTrn          # noqa: E402
from vispeech_amd.schema import dims_from_ctor          # noqa: E402
from vispeech_amd.synth import synth_state_dict         # noqa: E402

STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "r17_output_rows.txt")
SECONDS, B = 10, 16
RATES = (8000, 48000, 22050, 16000, 44100)
ENCS = ("f32", "s16", "ulaw", "alaw")


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


def waves(n, rows, seed):
    r = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n) / 44100.0
    x = 0.4 * np.sin(2 * np.pi * 220.0 * t)[None, :] * r.uniform(0.2, 1.0, (rows, 1)) + 0.1 * r.standard_normal((rows, n))
    return torch.from_numpy(x.clip(-1, 1).astype(np.float32)).to("cuda:0")


def clock():
    try:
        out = subprocess.run(["/opt/rocm/bin/rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        lines = [line.strip() for line in out.splitlines() if "sclk" in line or "mclk" in line]
        return "; ".join(lines[:2]) if lines else "not available"
    except Exception:
        return "not available"


def kernel_figures():
    try:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"),
                              os.path.join(ROOT, "vispeech_amd", "csrc", "output_rows.hip")], capture_output=True, text=True,
                             timeout=600).stdout.strip()
        return out or "not available (no compiler here)"
    except Exception:
        return "not available (no compiler here)"


def main():
    a, kw0 = vcfg.synthesizer_args(vcfg.default_hparams())
    dims = dims_from_ctor(*a, **kw0)
    net = SynthesizerTrn(*a, device="cuda:0", **kw0).eval()
    net.load_state_dict(synth_state_dict(dims, seed=1234))
    eng = net._engine
    rate, up = dims.sampling_rate, dims.total_upsample
    for r in RATES:
        eng.configure_output_rate(r)
    eng.configure_output(8000)
    props = torch.cuda.get_device_properties(0)
    lines = [f"output rows: default configuration ({rate} Hz); {ROUNDS} rounds per figure, a window of {STEPS} calls",
             f"device {torch.cuda.get_device_name(0)} ({getattr(props, 'gcnArchName', 'arch not available')}, "
             f"{props.multi_processor_count} CUs), host {platform.node()}",
             f"clocks: {clock()}",
             "timer: device events around a window of calls, per call; copies to the host are inside where the text says so",
             f"kernel (tools/kernel_regs.py; dynamic LDS: at most 8 KiB per block): {kernel_figures()}", ""]

    n = SECONDS * rate
    x = waves(n, B, 17)
    L, M, _ = eng.output_plan
    m1 = output_stage.out_len(n, L, M)

    def single_stage():
        return [eng.output_chunk(x[b:b + 1], 0, n, 0, m1, None, True).cpu() for b in range(B)]

    def rows_call():
        buf, spans = eng.output_rows([(x[b], True, 8000, "ulaw", None) for b in range(B)])
        return buf.cpu(), spans

    pcm = single_stage()
    buf, spans = rows_call()
    codes = output_stage.unpack(buf.numpy(), spans, ["ulaw"] * B)
    for b in range(B):
        assert codes[b].tobytes() == output_stage.encode(pcm[b].numpy().reshape(-1), "ulaw").tobytes(), b

    frames = 2 * rate // up
    r = np.random.Generator(np.random.PCG64(3))
    z = torch.from_numpy(r.standard_normal((B, dims.inter_channels, frames)).astype(np.float32)).to("cuda:0")
    g = torch.from_numpy(r.standard_normal((B, dims.gin_channels)).astype(np.float32)).to("cuda:0")
    o = eng.generator_ragged(z, g, [frames] * B)

    def generator():
        return eng.generator_ragged(z, g, [frames] * B)

    def rows_behind_generator():
        return eng.output_rows([(o[b, 0], True, 8000, "ulaw", None) for b in range(B)])

    short = waves(rate // 10, 64, 23)
    formats = [(RATES[b % 5], ENCS[(b // 5) % 4]) for b in range(64)]

    def mixed_one_call():
        return eng.output_rows([(short[b], True, *formats[b], None) for b in range(64)])[0].cpu()

    def mixed_solo_calls():
        return [eng.output_rows([(short[b], True, *formats[b], None)])[0].cpu() for b in range(64)]

    jobs = {"single stage, 16 launches + 16 copies (PCM16)": single_stage, "output_rows, 1 call + 1 copy (mu-law)": rows_call,
            "generator_ragged 16 x 2 s": generator, "output_rows behind it (no copy)": rows_behind_generator,
            "64 mixed rows, 1 call + 1 copy": mixed_one_call, "64 mixed rows, 64 calls + 64 copies": mixed_solo_calls}
    ms = {k: [] for k in jobs}
    for _ in range(ROUNDS):
        for k, fn in jobs.items():
            ms[k].append(timed(fn, max(STEPS // 2, 2) if k.startswith("generator") else STEPS))
    med = lambda k: float(np.median(ms[k]))
    keys = list(jobs)
    lines.append(f"1. {B} waveforms of {SECONDS} s ({n} samples) -> 8000 Hz ({m1} samples each)")
    for k in keys[:2]:
        lines.append(f"   {k:48s} {fmt(ms[k])}")
    lines.append(f"   one output_rows call / the single stage's way = {med(keys[1]) / med(keys[0]):.3f}")
    lines.append(f"2. beside the generator call that feeds it ({B} utterances of 2 s)")
    for k in keys[2:4]:
        lines.append(f"   {k:48s} {fmt(ms[k])}")
    lines.append(f"   output_rows / generator_ragged = {med(keys[3]) / med(keys[2]) * 100:.3f} %")
    lines.append("3. 64 rows of 0.1 s, 5 rates x 4 encodings")
    for k in keys[4:]:
        lines.append(f"   {k:48s} {fmt(ms[k])}")
    lines.append(f"   one call / 64 solo calls = {med(keys[4]) / med(keys[5]):.3f}")
    assert eng.status() == 0
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
