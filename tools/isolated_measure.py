#!/usr/bin/env python3
"""Step time of the C3 batch in isolated mode (infer(..., isolated=True)) next to the default mode, the way bench.py times
one batch start to end: a step = one full infer() with every input resident in HBM.  Both modes run in the SAME process
on the same context, each with its own warm-up, in alternating rounds (same box, same clocks: a same-box A/B); the
spread of the rounds is printed beside the difference so that the difference can be judged against it.

usage: tools/isolated_measure.py [steps] [rounds] [out.txt]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vispeech_amd import config as vcfg                 # noqa: E402
from vispeech_amd.models import SynthesizerTrn          # noqa: E402
from vispeech_amd.schema import dims_from_ctor          # noqa: E402
from vispeech_amd.synth import synth_state_dict, workload  # noqa: E402

STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
OUT = sys.argv[3] if len(sys.argv) > 3 else None


def main():
    a, kw0 = vcfg.synthesizer_args(vcfg.default_hparams())
    sd = synth_state_dict(dims_from_ctor(*a, **kw0), seed=1234, infer_only=True)
    net = SynthesizerTrn(*a, device="cuda:0", **kw0).eval()
    net.load_state_dict(sd)
    b = workload("C3")
    t = lambda x: torch.from_numpy(np.asarray(x)).to("cuda:0")
    args = (t(b["phonemes"]), t(b["lengths"]))
    kw = dict(sid=t(b["sid"]), noise_scale=0.667, noise=t(b["noise"]), t_f=int(b["frame_lengths"].max()),
              duration_control=t(b["duration"]), pitch_control=t(b["f0"]), energy_control=t(b["energy"]))

    def timed(isolated):
        for _ in range(3):
            net.infer(*args, isolated=isolated, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            net.infer(*args, isolated=isolated, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / STEPS * 1e3

    ms = {False: [], True: []}
    for _ in range(ROUNDS):
        for mode in (False, True):
            ms[mode].append(timed(mode))
    assert net._engine.status() == 0
    frames = b["frame_lengths"]
    lines = [f"C3 batch (64 utterances, {int(frames.max())} padded frames, {100 * (1 - frames.sum() / (64 * frames.max())):.1f} % padding), "
             f"one batch start to end, {STEPS} steps x {ROUNDS} alternating rounds, {torch.cuda.get_device_name(0)}"]
    for mode, name in ((False, "default (padded batch, trimmed tails)"), (True, "isolated")):
        v = ms[mode]
        lines.append(f"{name:40s} best {min(v):7.3f} ms   median {float(np.median(v)):7.3f} ms   spread {max(v) - min(v):6.3f} ms   {['%.3f' % x for x in v]}")
    d = min(ms[True]) - min(ms[False])
    lines.append(f"isolated - default (best of rounds): {d:+.3f} ms ({100 * d / min(ms[False]):+.2f} %); run-to-run spread of this file: "
                 f"{max(max(v) - min(v) for v in ms.values()):.3f} ms")
    text = "\n".join(lines)
    print(text)
    if OUT:
        os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
        with open(OUT, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
