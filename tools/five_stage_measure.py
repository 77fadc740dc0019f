#!/usr/bin/env python3
"""What the 16-channel kernel family (g16_c16, gen16_c16.hip) buys a FIVE-stage generator (upsample_rates [8, 8, 2, 2, 2],
512 initial channels: stages of 256 / 128 / 64 / 32 / 16 channels), measured on one box in one call:

  1. model: step time (one full infer() of the C3-shaped batch, inputs resident, HIP events around synchronised work) and
     the profiled generator time per kernel family, for the default split-f16 generator, for the SAME library under
     VSP_GENERATOR=f32 -- the channel-major f32 generator, which is what served this configuration before the 16-channel
     kernels existed -- and for VSP_CHAIN=0 (the 16-channel stage as one launch per convolution).  Rounds alternate.
  2. operator: the fused 16-channel ResBlock1 (vsp_cl_resblock, C = 16, mode 2) against (a) its own per-convolution form
     (mode 0) and (b) the existing 32-channel operator (C = 32, its best fused mode) fed the same weights zero-padded to 32
     channels -- the cheap alternative the 16-channel kernel has to beat.  The stand-alone operators pack and upload
     their weights inside the call; that host share is measured with a one-column call and reported next to the raw time.

The GPU clock is sampled (read-only rocm-smi --showclocks) while the timed loops run.

usage: tools/five_stage_measure.py [steps] [rounds] [out.json] [batch]"""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import threading

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vispeech_amd import _lib                            # noqa: E402
from vispeech_amd import config as vcfg                  # noqa: E402
from vispeech_amd.models import SynthesizerTrn           # noqa: E402
from vispeech_amd.schema import dims_from_ctor           # noqa: E402
from vispeech_amd.synth import synth_state_dict, workload  # noqa: E402

STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 2
OUT = sys.argv[3] if len(sys.argv) > 3 else None
BATCH = int(sys.argv[4]) if len(sys.argv) > 4 else 64
FIVE_STAGE = dict(upsample_rates=[8, 8, 2, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4, 4], upsample_initial_channel=512)
MODELS = [("split_f16", {}), ("f32_generator", {"VSP_GENERATOR": "f32"}), ("split_f16_per_conv", {"VSP_CHAIN": "0"})]


class ClockSampler:
    """Median sclk (MHz) while the body runs; None where rocm-smi is not available."""

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
        self._stop.clear()
        self._t = threading.Thread(target=self._run, daemon=True)
        self._t.start()
        return self

    def __exit__(self, *exc):
        self._stop.set()
        self._t.join(timeout=10)

    def median(self):
        return float(np.median(self.samples)) if self.samples else None


def build(env):
    hp = vcfg.default_hparams()
    for k, v in FIVE_STAGE.items():
        hp.model[k] = v
    a, kw = vcfg.synthesizer_args(hp)
    dims = dims_from_ctor(*a, **kw)
    sd = synth_state_dict(dims, seed=1234, infer_only=True)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        net = SynthesizerTrn(*a, device="cuda:0", **kw).eval()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    net.load_state_dict(sd)
    return net


def event_ms(fn, n, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def measure_models(clock):
    b = workload("C3", batch=BATCH)
    t = lambda x: torch.from_numpy(np.asarray(x)).to("cuda:0")
    args = (t(b["phonemes"]), t(b["lengths"]))
    kw = dict(sid=t(b["sid"]), noise_scale=0.667, noise=t(b["noise"]), duration_control=t(b["duration"]),
              pitch_control=t(b["f0"]), energy_control=t(b["energy"]))
    nets = {name: build(env) for name, env in MODELS}
    res = {name: {"generator_kind": nets[name]._engine.generator_kind, "step_ms": []} for name, _ in MODELS}
    with clock:
        for _ in range(ROUNDS):
            for name, _ in MODELS:
                res[name]["step_ms"].append(event_ms(lambda: nets[name].infer(*args, **kw), STEPS))
    for name, _ in MODELS:
        eng = nets[name]._engine
        eng.profile(True)
        nets[name].infer(*args, **kw)
        torch.cuda.synchronize()
        fams = eng.profile_read_families()
        n, ms, *_ = eng.profile_read(reset=True)
        eng.profile(False)
        assert eng.status() == 0
        res[name].update(step_ms_best=min(res[name]["step_ms"]), generator_ms=ms, generator_launches=n,
                         families=[dict(kind=f["kind"], channels=f["channels"], launches=f["launches"], ms=round(f["ms"], 4))
                                   for f in fams])
    frames = [int(v) for v in b["frame_lengths"]]
    return {"batch": BATCH, "frames_max": max(frames), "frames_sum": sum(frames), "models": res}


def measure_operator(clock, k, b, t):
    lib = _lib.lib()
    dils = (1, 3, 5)
    r = np.random.Generator(np.random.PCG64(k))
    w16 = [(r.standard_normal((16, 16, k)) / np.sqrt(16 * k)).astype(np.float32) for _ in range(6)]
    b16 = [r.standard_normal(16).astype(np.float32) * 0.1 for _ in range(6)]
    w32, b32 = [], []
    for w, bi in zip(w16, b16):
        wp = np.zeros((32, 32, k), dtype=np.float32)
        wp[:16, :16] = w
        bp = np.zeros(32, dtype=np.float32)
        bp[:16] = bi
        w32.append(wp)
        b32.append(bp)
    ptrs = lambda arrs: (C.c_void_p * len(arrs))(*[a.ctypes.data_as(C.c_void_p) for a in arrs])
    darr = (C.c_int * 3)(*dils)
    x16 = torch.randn(b, t, 16, device="cuda")
    x32 = torch.zeros(b, t, 32, device="cuda")
    x32[:, :, :16] = x16
    o16, o32 = torch.empty_like(x16), torch.empty_like(x32)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda v: C.c_void_p(v.data_ptr())

    def call(c, mode, bb, tt, x, o, ws, bs):
        rc = lib.vsp_cl_resblock(stream, bb, tt, c, k, 3, darr, P(x), ptrs(ws), ptrs(bs), mode, 3, P(o))
        assert rc == 0, (c, mode, rc)

    forms = {"c16_fused": (16, 2, x16, o16, w16, b16), "c16_per_conv": (16, 0, x16, o16, w16, b16),
             "c32_zero_padded_fused": (32, 2, x32, o32, w32, b32), "c32_zero_padded_pairs": (32, 1, x32, o32, w32, b32)}
    out = {name: {"raw_ms": [], "host_ms": []} for name in forms}
    with clock:
        for _ in range(ROUNDS):
            for name, (c, mode, x, o, ws, bs) in forms.items():
                out[name]["raw_ms"].append(event_ms(lambda: call(c, mode, b, t, x, o, ws, bs), 5))
                out[name]["host_ms"].append(event_ms(lambda: call(c, mode, 1, 1, x, o, ws, bs), 5))
    call(16, 2, b, t, x16, o16, w16, b16)
    call(32, 2, b, t, x32, o32, w32, b32)
    torch.cuda.synchronize()
    same = float((o32[:, :, :16] - o16).abs().max())
    for name in forms:
        out[name]["net_ms_best"] = min(out[name]["raw_ms"]) - min(out[name]["host_ms"])
    return {"kernel": k, "dilations": dils, "batch": b, "columns": t, "max_abs_diff_c16_vs_padded_c32": same, "forms": out}


def main():
    clock = ClockSampler()
    res = {"device": torch.cuda.get_device_name(0), "steps": STEPS, "rounds": ROUNDS}
    res["model"] = measure_models(clock)
    torch.cuda.empty_cache()
    res["operator"] = [measure_operator(clock, k, 16, 1 << 18) for k in (3, 7, 11)]
    res["sclk_mhz_median_under_load"] = clock.median()
    text = json.dumps(res, indent=1)
    print(text)
    if OUT:
        os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
        with open(OUT, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
