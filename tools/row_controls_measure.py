#!/usr/bin/env python3
"""What a per-row table costs (infer(..., isolated=True, row_controls=...)): the same 4-row batch with C3's statistics,
one full infer() start to end with every input resident in HBM, timed in ONE process on one context in alternating rounds
(a same-box A/B; the spread of the rounds is printed beside the differences):

    scalar        every control a tensor, scalar noise_scale: the isolated call as it was
    uniform       the same arguments as a table (all rows given all three): the per-row kernels instead of the scalar ones
    mixed p+e     rows 2, 3 leave pitch and energy to the predictors (durations given: the SAME frame counts) -- the
                  pitch and energy predictors now run for the batch
    mixed all     rows 2, 3 leave all three to the predictors, duration_scale 0.5 -- the duration predictor runs too, no
                  early frame-count copy, and the batch has the frame counts those rows predict (printed)

The library draws the noise in all four (one seed per row), so that the last one needs no noise tensor of a size nobody
knows before the call.

usage: tools/row_controls_measure.py [steps] [rounds] [out.txt]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vispeech_amd import config as vcfg                    # noqa: E402
from vispeech_amd.models import RowControls, SynthesizerTrn   # noqa: E402
from vispeech_amd.schema import dims_from_ctor             # noqa: E402
from vispeech_amd.synth import synth_state_dict, workload  # noqa: E402

STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
OUT = sys.argv[3] if len(sys.argv) > 3 else None
B = 4


def main():
    a, kw0 = vcfg.synthesizer_args(vcfg.default_hparams())
    sd = synth_state_dict(dims_from_ctor(*a, **kw0), seed=1234, infer_only=True)
    net = SynthesizerTrn(*a, device="cuda:0", **kw0).eval()
    net.load_state_dict(sd)
    b = workload("C3", batch=B)
    t = lambda x: torch.from_numpy(np.asarray(x)).to("cuda:0")
    args = (t(b["phonemes"]), t(b["lengths"]))
    common = dict(sid=t(b["sid"]), duration_control=t(b["duration"]), pitch_control=t(b["f0"]), energy_control=t(b["energy"]),
                  noise_seed=[1, 2, 3, 4], isolated=True)
    half = lambda d, p, e: np.array([[True] * 3] * 2 + [[d, p, e]] * 2)
    cases = {
        "scalar": dict(noise_scale=0.667),
        "uniform": dict(row_controls=RowControls.uniform(B, noise_scale=0.667, given=(True, True, True))),
        "mixed p+e": dict(row_controls=RowControls(np.ones(B), np.ones(B), np.ones(B), np.full(B, 0.667), half(True, False, False))),
        "mixed all": dict(row_controls=RowControls([1, 1, 0.5, 0.5], np.ones(B), np.ones(B), np.full(B, 0.667), half(False, False, False))),
    }
    frames = {}

    def timed(name):
        kw = dict(common, **cases[name])
        for _ in range(3):
            res = net.infer(*args, **kw)
        frames[name] = res[1].sum(dim=(1, 2)).cpu().tolist()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            net.infer(*args, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / STEPS * 1e3

    ms = {k: [] for k in cases}
    for _ in range(ROUNDS):
        for name in cases:
            ms[name].append(timed(name))
    assert net._engine.status() == 0
    lines = [f"{B} rows with C3's statistics ({[int(x) for x in b['lengths']]} phonemes), isolated infer start to end, "
             f"{STEPS} steps x {ROUNDS} alternating rounds, {torch.cuda.get_device_name(0)}"]
    for name, v in ms.items():
        lines.append(f"{name:10s} best {min(v):7.3f} ms   median {float(np.median(v)):7.3f} ms   spread {max(v) - min(v):6.3f} ms   "
                     f"frames {[int(x) for x in frames[name]]}")
    base = min(ms["scalar"])
    for name in ("uniform", "mixed p+e", "mixed all"):
        d = min(ms[name]) - base
        lines.append(f"{name} - scalar (best of rounds): {d:+.3f} ms ({100 * d / base:+.2f} %)")
    lines.append(f"run-to-run spread of this file: {max(max(v) - min(v) for v in ms.values()):.3f} ms")
    text = "\n".join(lines)
    print(text)
    if OUT:
        os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
        with open(OUT, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
