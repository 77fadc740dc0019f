#!/usr/bin/env python3
"""What streaming for batched requests (StreamingBatchService, vsp_generator_stream_rows) costs and buys.

1. Time from submit to the first PCM16 chunk of a request that arrives while 1, 4 and 16 others are mid-utterance:
   StreamingBatchService (the request joins the next tick) against BatchingSynthesisService (it waits for the batch in
   flight, then for a whole batch of its own) and the single-flight SynthesisService.stream (idle service: with anybody
   in flight it answers Busy).  Utterances of ~430 frames (5 s).
2. Samples/s of ticking 16 utterances at chunk_frames 32, 64 and 128 against ONE vsp_generator_ragged call on the same
   utterances: the halo recompute alone predicts (chunk + 28) / chunk.
3. The largest deviation of the ticked chunks from generator_ragged B = 1 on each utterance alone (the tests' 1e-5 bound).

usage: tools/stream_batch_measure.py [repeats] [out.txt]

With --output-rate R the tool measures the service's output stage instead: 16 requests of ~5 s submitted to an idle
StreamingBatchService driven by step(), chunk_frames 32 and 64, in ONE process -- the plain service (output_rate=None), the
per-request output stage (output_rate=R) and, with --fused, the ragged output stage (fused_output=True), alternated
within every repeat after a warm-up run of each.  Per run: the median wall time of the ticks that advance all 16 requests,
delivered samples/s (first submit to last byte) and the time from submit to the first chunk in hand.

usage: tools/stream_batch_measure.py --output-rate R [--fused] [repeats] [out.txt]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vispeech_amd import config as vcfg                                   # noqa: E402
from vispeech_amd.models import SynthesizerTrn                            # noqa: E402
from vispeech_amd.schema import dims_from_ctor                            # noqa: E402
from vispeech_amd.service import (BatchingSynthesisService, StreamingBatchService,   # noqa: E402
                                  SynthesisService)
from vispeech_amd.synth import synth_batch, synth_state_dict             # noqa: E402

ARGS = list(sys.argv[1:])
FUSED = "--fused" in ARGS
if FUSED:
    ARGS.remove("--fused")
OUTPUT_RATE = None
if "--output-rate" in ARGS:
    i = ARGS.index("--output-rate")
    OUTPUT_RATE = int(ARGS[i + 1])
    del ARGS[i:i + 2]
if FUSED and OUTPUT_RATE is None:
    sys.exit("--fused needs --output-rate")
REPEATS = int(ARGS[0]) if len(ARGS) > 0 else 5
OUT = ARGS[1] if len(ARGS) > 1 else None
KEYS = ("phonemes", "lengths", "sid", "duration", "f0", "energy")


def med(v):
    return float(np.median(v))


def first_chunk_latency(net, batch, others, chunk):
    """ms from submit to the first chunk in hand, `others` requests two ticks into their utterances (driven by step():
    what the worker thread does, without its wake-up)."""
    collate = lambda rows: {k: batch[k][rows] for k in KEYS}
    out = []
    for rep in range(REPEATS + 1):                      # (the first repeat warms the workspaces up)
        svc = StreamingBatchService(net, max_batch=others + 1, chunk_frames=chunk, collate=collate, autostart=False)
        mates = [svc.submit(b, 1000 + b) for b in range(others)]
        svc.step(); svc.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        probe = svc.submit(others, 77)
        svc.step()
        first = next(probe)
        out.append((time.perf_counter() - t0) * 1e3)
        assert len(first) == 2 * chunk * net.dims.total_upsample and svc.stats["rows_per_tick"][-1] == others + 1
        for s in mates + [probe]:
            s.close()
        svc.close()
    return out[1:]


def batching_latency(net, batch, others):
    """ms from submit to the PCM16 of a request that arrives 1 ms after a batch of `others` started."""
    collate = lambda rows: {k: batch[k][rows] for k in KEYS}
    out = []
    for rep in range(REPEATS + 1):
        svc = BatchingSynthesisService(net, max_batch=others, max_wait_s=0.0, collate=collate)
        try:
            mates = [svc.submit(b, 1000 + b) for b in range(others)]
            time.sleep(0.001)
            t0 = time.perf_counter()
            probe = svc.submit(others, 77)
            probe.result(300)
            out.append((time.perf_counter() - t0) * 1e3)
            for m in mates:
                m.result(300)
        finally:
            svc.close()
    return out[1:]


def single_flight_latency(net, batch, chunk):
    svc = SynthesisService(net, chunk_frames=chunk, isolated=True)
    one = {k: batch[k][:1] for k in KEYS}
    out = []
    for rep in range(REPEATS + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = svc.stream(one, 0)
        next(st)
        out.append((time.perf_counter() - t0) * 1e3)
        st.close()
    return out[1:]


def ticking_throughput(net, n_utt, chunks):
    eng, d = net._engine, net.dims
    r = np.random.Generator(np.random.PCG64(5))
    lengths = [int(x) for x in r.integers(300, 520, size=n_utt)]
    T, up = max(lengths), d.total_upsample
    z = torch.from_numpy(r.standard_normal((n_utt, d.inter_channels, T)).astype(np.float32)).to(eng.device)
    g = torch.from_numpy(r.standard_normal((n_utt, d.gin_channels)).astype(np.float32) * 0.1).to(eng.device)
    samples = sum(lengths) * up

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return med(ts)

    def ticks(chunk, keep=None):
        pos = [0] * n_utt
        while any(p < L for p, L in zip(pos, lengths)):
            act = [b for b in range(n_utt) if pos[b] < lengths[b]]
            rows = [(z[b], g[b], lengths[b], pos[b], min(lengths[b], pos[b] + chunk)) for b in act]
            o = eng.generator_stream_rows(rows, chunk, pcm=keep is None)
            for k, b in enumerate(act):
                if keep is not None:
                    keep[b].append(o[k, : (rows[k][4] - pos[b]) * up].clone())
                pos[b] = rows[k][4]

    t_one = timed(lambda: eng.generator_ragged(z, g, lengths))
    lines = [f"{n_utt} utterances of {min(lengths)} .. {max(lengths)} frames ({samples} samples), median of {REPEATS}:",
             f"  one generator_ragged call                    {t_one * 1e3:8.2f} ms   {samples / t_one / 1e6:8.1f} Msamples/s"]
    for c in chunks:
        t = timed(lambda: ticks(c))
        lines.append(f"  ticking, chunk_frames {c:3d} ({-(-T // c):2d} ticks)          {t * 1e3:8.2f} ms   {samples / t / 1e6:8.1f} Msamples/s   "
                     f"{t / t_one:5.2f}x the one call (halo alone predicts {(c + 28) / c:.2f}x)")
    # deviation of the ticked chunks from each utterance's own run
    keep = [[] for _ in range(n_utt)]
    ticks(64, keep)
    worst = 0.0
    for b in range(min(n_utt, 4)):
        alone = eng.generator_ragged(z[b:b + 1, :, :lengths[b]].contiguous(), g[b:b + 1], [lengths[b]])[0, 0]
        got = torch.cat(keep[b])
        worst = max(worst, float((got - alone).abs().max() / alone.abs().max()))
    lines.append(f"  ticked chunks (64) vs generator_ragged B = 1 on the utterance alone: max |diff| / max |ref| = {worst:.2e}")
    return lines


def service_run(net, batch, n_req, chunk, **kw):
    """One idle service, `n_req` requests submitted at once, driven by step() until everything is delivered.  Returns
    (median ms of the ticks with all n_req rows, delivered samples per second, ms from submit to the first chunk, samples)."""
    collate = lambda rows: {k: batch[k][rows] for k in KEYS}
    svc = StreamingBatchService(net, max_batch=n_req, chunk_frames=chunk, collate=collate, autostart=False, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    streams = [svc.submit(b, 1000 + b) for b in range(n_req)]
    more = svc.step()                                   # admission + the first tick
    first = next(streams[0])
    t_first = time.perf_counter() - t0
    ticks = []
    while more:
        t1 = time.perf_counter()
        more = svc.step()                               # (synchronous: it ends with the tick's device-to-host copy)
        ticks.append(time.perf_counter() - t1)
    total = time.perf_counter() - t0
    samples = len(first) // 2 + sum(len(piece) // 2 for s in streams for piece in s)
    svc.close()
    full = [t for t, rows in zip(ticks, svc.stats["rows_per_tick"][1:]) if rows == n_req]
    return med(full) * 1e3, samples / total, t_first * 1e3, samples


def output_stage_mode(net, batch, n_req=16):
    kinds = [("plain, output_rate=None", {}), (f"output_rate={OUTPUT_RATE}, per request", {"output_rate": OUTPUT_RATE})]
    if FUSED:
        kinds.append((f"output_rate={OUTPUT_RATE}, fused_output", {"output_rate": OUTPUT_RATE, "fused_output": True}))
    frames = batch["frame_lengths"][:n_req]
    lines = [f"{torch.cuda.get_device_name(0)}; {n_req} requests of {int(frames.min())} .. {int(frames.max())} frames submitted to "
             f"an idle StreamingBatchService, step() driven; median [min .. max] of {REPEATS} runs, the kinds alternated "
             "within every repeat after one warm-up run of each; profiler off"]
    for chunk in (32, 64):
        res = {name: [] for name, _ in kinds}
        for rep in range(REPEATS + 1):
            for name, kw in kinds:
                r = service_run(net, batch, n_req, chunk, **kw)
                if rep:
                    res[name].append(r)
        net._engine.configure_output(None)
        lines.append(f"chunk_frames {chunk}:")
        for name, _ in kinds:
            t, sps, fc = ([r[i] for r in res[name]] for i in range(3))
            lines.append(f"  {name:42s} tick {med(t):7.3f} [{min(t):.3f} .. {max(t):.3f}] ms   delivered {med(sps) / 1e6:7.2f} "
                         f"[{min(sps) / 1e6:.2f} .. {max(sps) / 1e6:.2f}] Msamples/s ({res[name][0][3]} samples)   "
                         f"first chunk {med(fc):6.2f} [{min(fc):.2f} .. {max(fc):.2f}] ms")
    return lines


def main():
    a, kw0 = vcfg.synthesizer_args(vcfg.default_hparams())
    sd = synth_state_dict(dims_from_ctor(*a, **kw0), seed=1234, infer_only=True)
    net = SynthesizerTrn(*a, device="cuda:0", **kw0).eval()
    net.load_state_dict(sd)
    batch = synth_batch(17, seed=11)
    if OUTPUT_RATE is not None:
        lines = output_stage_mode(net, batch)
        assert net._engine.status() == 0
        return report(lines)
    chunk = 64
    lines = [f"{torch.cuda.get_device_name(0)}; utterances of {int(batch['frame_lengths'].min())} .. "
             f"{int(batch['frame_lengths'].max())} frames; chunk_frames {chunk} (0.74 s); median [min .. max] of {REPEATS}",
             "submit -> first PCM16 chunk of a request arriving while N others are mid-utterance, ms:"]
    v = single_flight_latency(net, batch, chunk)
    lines.append(f"  SynthesisService.stream, idle service (anybody in flight: Busy)   {med(v):8.2f} [{min(v):.2f} .. {max(v):.2f}]")
    for n in (1, 4, 16):
        s = first_chunk_latency(net, batch, n, chunk)
        w = batching_latency(net, batch, n)
        lines.append(f"  N = {n:2d}: StreamingBatchService {med(s):8.2f} [{min(s):.2f} .. {max(s):.2f}]   "
                     f"BatchingSynthesisService (whole utterance) {med(w):8.2f} [{min(w):.2f} .. {max(w):.2f}]")
    lines += ticking_throughput(net, 16, (32, 64, 128))
    assert net._engine.status() == 0
    report(lines)


def report(lines):
    text = "\n".join(lines)
    print(text)
    if OUT:
        os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
        with open(OUT, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
