#!/usr/bin/env python3
"""Measurements of the output stage (resample.hip; DESIGN.md "Output stage").

  kernel   device time of one vsp_output_chunk launch per output rate (HIP events, warmed, median of 20) on the BASELINE
           config 3 batch (64 utterances, ~5 s each, ragged) and on the single 5.6 s / 60 s utterances of tools/ttfa.py,
           beside the bytes the launch must move (4 n_in + 2 n_out per utterance) and the device time of the infer call
           that produced the waveform: the stage's share of the step.
  service  latency of SynthesisService with output_rate=22050 against the plain 44.1 kHz float path of the same process,
           ALTERNATING request by request: call -> first streamed chunk on the host, and the one-shot call; median and
           min .. max of each, so that a difference can be read against the run-to-run spread of the same call.

usage (on the GPU box, each step under its own time limit):
  timeout 300 python tools/output_stage_measure.py kernel  >> profiles/<tag>.txt
  timeout 300 python tools/output_stage_measure.py service >> profiles/<tag>.txt"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from vispeech_amd import config as vcfg
from vispeech_amd.models import SynthesizerTrn
from vispeech_amd.schema import ModelDims
from vispeech_amd.service import SynthesisService
from vispeech_amd.synth import synth_state_dict, workload

RATES = (22050, 16000, 24000, 48000, 8000, 11025, 32000, 44100)
HBM_PEAK = 8.0e12          # bytes / s, MI355X data sheet


def make_net():
    a, kw = vcfg.synthesizer_args(vcfg.default_hparams())
    net = SynthesizerTrn(*a, **kw).eval()
    net.load_state_dict(synth_state_dict(ModelDims(), seed=1234, infer_only=True))
    return net


def event_ms(fn, warm=3, runs=20):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def infer(net, batch):
    t = lambda a: torch.from_numpy(np.asarray(a)).to(net.device)
    args = (t(batch["phonemes"]), t(batch["lengths"]))
    kw = dict(sid=t(batch["sid"]), noise_scale=0.667, duration_control=t(batch["duration"]), pitch_control=t(batch["f0"]),
              energy_control=t(batch["energy"]), noise=t(batch["noise"]))
    return lambda: net.infer(*args, **kw)


def kernel():
    net = make_net()
    eng = net._engine
    print("== output stage: device time of one launch (median of 20, HIP events), PCM16 out")
    print("   bytes = sum over utterances of 4 n_in + 2 n_out; share = launch / device time of the infer call before it")
    for name, batch in (("C3 (64 x ~5 s)", workload("C3")), ("one 5.6 s utterance", workload("C2", batch=1)),
                        ("one 60 s utterance (C5)", workload("C5"))):
        run = infer(net, batch)
        o, x_mask, *_ = run()
        step_ms = event_ms(run, warm=2, runs=5)
        n_valid = (x_mask.sum(dim=(1, 2)) * 512).to(torch.int64)
        n_in = n_valid.cpu().numpy().astype(np.float64)
        print(f"-- {name}: padded {o.shape[2]} samples, valid {int(n_in.sum())}, infer {step_ms:.3f} ms")
        for rate in RATES:
            eng.configure_output(rate)
            L, M, H = eng.output_plan
            x, n = o.reshape(o.shape[0], -1), o.shape[2]
            m1 = -((-n * L) // M)
            ms = event_ms(lambda: eng.output_chunk(x, 0, n, 0, m1, n_valid, True))
            moved = float((4 * n_in + 2 * np.ceil(n_in * L / M)).sum())
            fma = float((np.ceil(n_in * L / M) * (2 * H // L + 1)).sum())
            print(f"   {rate:6d} Hz  L/M {L:3d}/{M:3d}  taps/output {2 * H // L + 1:4d}  {ms * 1e3:8.1f} us  "
                  f"{moved / 1e6:8.2f} MB -> {moved / ms / 1e9 * 1e3:7.1f} GB/s ({100 * moved / ms * 1e3 / HBM_PEAK:4.1f} % of HBM peak)  "
                  f"{fma / ms / 1e6:7.1f} GFMA/s  share of the step {100 * ms / step_ms:5.2f} %")
        eng.configure_output(None)


def service(runs=15):
    net = make_net()
    plain = SynthesisService(net, chunk_frames=64)
    staged = SynthesisService(net, chunk_frames=64, output_rate=22050)
    print("== service latency, alternating plain (44.1 kHz float copy + host quantiser) / output_rate=22050 (GPU stage, int16 copy)")
    print(f"   ms on the host clock: median [min .. max] of {runs} after 3 warm-ups, chunk = 64 frames")
    for name, batch in (("one 5.6 s utterance", workload("C2", batch=1)), ("one 60 s utterance (C5)", workload("C5"))):
        noise = torch.from_numpy(batch["noise"]).to(net.device)
        res = {(k, w): [] for k in ("plain", "staged") for w in ("first", "stream", "one_shot")}
        for i in range(runs + 3):
            for key, svc in (("plain", plain), ("staged", staged)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                it = svc.stream(batch, 0, noise=noise)
                next(it)
                t1 = time.perf_counter()
                for _ in it:
                    pass
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                svc.synthesize(batch, 0, noise=noise)
                t3 = time.perf_counter()
                if i >= 3:
                    res[key, "first"].append(t1 - t0)
                    res[key, "stream"].append(t2 - t0)
                    res[key, "one_shot"].append(t3 - t2)
        print(f"-- {name}")
        for w in ("first", "stream", "one_shot"):
            line = f"   {w:9s}"
            for key in ("plain", "staged"):
                v = sorted(res[key, w])
                line += f"  {key} {v[len(v) // 2] * 1e3:8.3f} [{v[0] * 1e3:8.3f} .. {v[-1] * 1e3:8.3f}]"
            print(line)


if __name__ == "__main__":
    {"kernel": kernel, "service": service}[sys.argv[1] if len(sys.argv) > 1 else "kernel"]()
