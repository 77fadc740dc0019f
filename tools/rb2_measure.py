#!/usr/bin/env python3
"""Step time of a synthetic ResBlock2 model (resblock "2", configs/config.json otherwise) next to the ResBlock1 model on
the C3 batch, the way bench.py times it: a step = one full infer() with every input resident in HBM, two batches in
flight (InFlightPool, two contexts on two streams) and one batch start to end; then one profiled step per model
(Engine.profile_read_families: generator time per kernel family and channel count).  The ResBlock2 model runs twice,
fused (default) and VSP_RB2_FUSE=0 (one launch per convolution): a same-box A/B.  Rounds alternate the models.

usage: tools/rb2_measure.py [steps] [rounds] [out.json]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vispeech_amd import config as vcfg                 # noqa: E402
from vispeech_amd.models import SynthesizerTrn          # noqa: E402
from vispeech_amd.pipeline import InFlightPool          # noqa: E402
from vispeech_amd.schema import dims_from_ctor          # noqa: E402
from vispeech_amd.synth import synth_state_dict, workload  # noqa: E402

STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 2
OUT = sys.argv[3] if len(sys.argv) > 3 else None
MODELS = [("resblock1", "1", {}), ("resblock2", "2", {}), ("resblock2_per_conv", "2", {"VSP_RB2_FUSE": "0"})]


def build(resblock, env):
    hp = vcfg.default_hparams()
    hp.model["resblock"] = resblock
    a, kw = vcfg.synthesizer_args(hp)
    dims = dims_from_ctor(*a, **kw)
    sd = synth_state_dict(dims, seed=1234, infer_only=True)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        pool = InFlightPool(lambda: SynthesizerTrn(*a, device="cuda:0", **kw).eval(), lambda m: m.load_state_dict(sd), n=2)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return pool


def main():
    b = workload("C3")
    t = lambda x: torch.from_numpy(np.asarray(x)).to("cuda:0")
    args = (t(b["phonemes"]), t(b["lengths"]))
    kw = dict(sid=t(b["sid"]), noise_scale=0.667, noise=t(b["noise"]), t_f=int(b["frame_lengths"].max()),
              duration_control=t(b["duration"]), pitch_control=t(b["f0"]), energy_control=t(b["energy"]))
    pools = {name: build(rb, env) for name, rb, env in MODELS}
    res = {name: {"two_in_flight_ms": [], "one_batch_ms": []} for name, _, _ in MODELS}

    def timed(pool, n):
        for _ in range(3):
            pool.infer(*args, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            pool.infer(*args, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    for _ in range(ROUNDS):
        for name, _, _ in MODELS:
            res[name]["two_in_flight_ms"].append(timed(pools[name], STEPS))
            res[name]["one_batch_ms"].append(timed(pools[name].restrict(1), STEPS))
    for name, _, _ in MODELS:
        one = pools[name].restrict(1)
        eng = one.next_slot()[0]._engine
        one.infer(*args, **kw)
        torch.cuda.synchronize()
        eng.profile(True)
        one.infer(*args, **kw)
        torch.cuda.synchronize()
        fams = eng.profile_read_families()
        n, ms, *_ = eng.profile_read(reset=True)
        eng.profile(False)
        assert eng.status() == 0
        res[name]["generator_ms"] = ms
        res[name]["generator_launches"] = n
        res[name]["families"] = [dict(kind=f["kind"], channels=f["channels"], launches=f["launches"], ms=round(f["ms"], 4))
                                 for f in fams]
        res[name]["two_in_flight_ms_best"] = min(res[name]["two_in_flight_ms"])
        res[name]["one_batch_ms_best"] = min(res[name]["one_batch_ms"])
    out = {"workload": "C3 (64 utterances, durations / pitch / energy given)", "steps": STEPS, "rounds": ROUNDS,
           "device": torch.cuda.get_device_name(0), "models": res}
    text = json.dumps(out, indent=1)
    print(text)
    if OUT:
        os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
        with open(OUT, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
