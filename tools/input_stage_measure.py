#!/usr/bin/env python3
"""The input stage, measured on the GPU (default configuration, synthetic weights).

1. ``Engine.input_batch`` for 16 recordings of 10 s at 16000 Hz / PCM16, 48000 Hz / float32 and 8000 Hz / mu-law, beside the
   ``Engine.convert_latent`` and ``Engine.generator_ragged`` calls of the batch it produces: the stage's share of the
   conversion call it feeds.
2. The per-tick input call of 16 live sessions at chunks of 64 frames -- one ``Engine.input_rows`` call of 16 open rows, each
   the raw samples of one chunk behind the history its stream kept -- beside the tick it feeds (``convert_stream_rows`` +
   ``generator_stream_rows`` + the PCM16 copy, an interior tick).

Every figure is a device-event time per call (``torch.cuda.Event``) over a window of ``steps`` calls after a warm-up of the
same shape (50 x ``steps`` calls for the short input calls); rounds alternate over the configurations, and best / median /
spread of the rounds are printed.  A call of a tenth of a millisecond is bounded by the host's enqueue, not by its kernel:
the figures of the input calls are upper bounds of the stage's device time.

usage: tools/input_stage_measure.py [steps] [rounds] [out.txt]     (default out: profiles/r16_input_stage.txt)"""
import os
import platform
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vispeech_amd import config as vcfg, input_stage, output_stage   # noqa: E402
from vispeech_amd.models import SynthesizerTrn          # noqa: E402
from vispeech_amd.schema import convert_halo_frames, dims_from_ctor  # noqa: E402
from vispeech_amd.synth import synth_state_dict         # noqa: E402

STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "r16_input_stage.txt")
SECONDS, B, CHUNK = 10, 16, 64
FORMATS = ((16000, input_stage.S16, "PCM16"), (48000, input_stage.F32, "float32"), (8000, input_stage.ULAW, "mu-law"))


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


def raw_batch(rate, enc, seed):
    r = np.random.Generator(np.random.PCG64(seed))
    n = SECONDS * rate
    t = np.arange(n) / rate
    x = (0.4 * np.sin(2 * np.pi * 220.0 * t)[None, :] * r.uniform(0.2, 1.0, (B, 1)) + 0.1 * r.standard_normal((B, n))).clip(-1, 1)
    if enc == input_stage.F32:
        return x.astype(np.float32)
    if enc == input_stage.S16:
        return np.rint(x * 32767.0).astype(np.int16)
    return r.integers(0, 256, (B, n)).astype(np.uint8)      # (every code: the table look-ups are as scattered as they get)


def fmt(v):
    return f"best {min(v):8.3f} ms  median {float(np.median(v)):8.3f} ms  spread {max(v) - min(v):6.3f} ms"


def main():
    a, kw0 = vcfg.synthesizer_args(vcfg.default_hparams())
    dims = dims_from_ctor(*a, **kw0)
    net = SynthesizerTrn(*a, device="cuda:0", **kw0).eval()
    net.load_state_dict(synth_state_dict(dims, seed=1234))
    eng = net._engine
    model_rate, hop, n_fft = dims.sampling_rate, dims.hop_length, 2 * (dims.spec_channels - 1)
    pad = (n_fft - hop) // 2
    G, H = eng.generator_halo, convert_halo_frames(dims)
    props = torch.cuda.get_device_properties(0)
    lines = [f"input stage: default configuration ({model_rate} Hz), {B} recordings of {SECONDS} s; {ROUNDS} rounds per figure, a window of "
             f"{STEPS * 50} calls for the input calls, {STEPS} for the tick, {max(STEPS // 2, 2)} for convert_latent and the generator",
             f"device {torch.cuda.get_device_name(0)} ({getattr(props, 'gcnArchName', 'arch not available')}, "
             f"{props.multi_processor_count} CUs), host {platform.node()}",
             "timer: device events around a window of calls, per call", ""]
    src, tgt = [b % dims.n_speakers for b in range(B)], [(b + 7) % dims.n_speakers for b in range(B)]
    seeds = list(range(100, 100 + B))

    jobs, ms = {}, {}
    for rate, enc, name in FORMATS:
        eng.configure_input(rate)
        L, M, Hf = eng.input_plan(rate)
        raw = eng._raw(raw_batch(rate, enc, rate), enc)
        n_in = [SECONDS * rate] * B
        audio, n_out = eng.input_batch(raw, n_in, rate, enc)
        lat = eng.convert_latent(audio, n_out, src, tgt, noise_seed=seeds)
        jobs[("input_batch", name)] = lambda raw=raw, n_in=n_in, rate=rate, enc=enc: eng.input_batch(raw, n_in, rate, enc)
        jobs[("convert_latent", name)] = lambda audio=audio, n_out=n_out: eng.convert_latent(audio, n_out, src, tgt, noise_seed=seeds)
        jobs[("generator_ragged", name)] = lambda lat=lat: eng.generator_ragged(lat["z_hat"], lat["g"], lat["frames"])
        # the live tick: every session has one chunk of new raw samples behind its stream's history
        n_piece = -(-CHUNK * hop * M // L)
        hist = (2 * Hf) // L
        first = 5 * n_piece
        rows = []
        for b in range(B):
            win = raw[b, first - hist:first + n_piece]
            m0 = output_stage.complete_outputs(first, L, M, Hf)
            m1 = output_stage.complete_outputs(first + n_piece, L, M, Hf)
            assert output_stage.history_start(m0, L, M, Hf) >= first - hist
            rows.append((win, first - hist, -1, m0, m1))
        jobs[("input_rows tick", name)] = lambda rows=rows, rate=rate, enc=enc: eng.input_rows(rows, rate, enc)
        lines.append(f"{rate} Hz {name}: L / M = {L} / {M}, {2 * Hf + 1} taps ({(2 * Hf) // L + 1} per output), {n_in[0]} -> {n_out[0]} samples; "
                     f"a tick's piece: {n_piece} raw samples behind {hist} of history")
    dev = torch.from_numpy(raw_batch(model_rate, input_stage.F32, 7)[0]).to("cuda:0")
    f0 = G + H + 8
    f1 = f0 + CHUNK
    e0, e1 = f0 - G, f1 + G
    n_known = (e1 + H - 1) * hop - pad + n_fft
    assert eng.convert_window_plan(n_known, False, e0, e1)[0]
    live_rows = [(dev, 0, n_known, False, e0, e1, src[b], tgt[b], 100 + b, 1.0) for b in range(B)]

    def tick():
        z, g = eng.convert_stream_rows(live_rows, CHUNK + 2 * G)
        return eng.generator_stream_rows([(z[b], g[b], e1 - e0, f0 - e0, f1 - e0) for b in range(B)], CHUNK, pcm=True).cpu()
    jobs[("live tick", "")] = tick

    ms = {k: [] for k in jobs}
    for _ in range(ROUNDS):
        for k, fn in jobs.items():
            # (the input calls are short: their windows are 50 times as many calls, so that each lasts tens of milliseconds)
            ms[k].append(timed(fn, STEPS * 50 if k[0].startswith("input") else STEPS if k[0] == "live tick" else max(STEPS // 2, 2)))
    med = lambda k: float(np.median(ms[k]))
    lines += ["", f"1. one-shot: input_batch beside the conversion of its {B} x {SECONDS} s batch"]
    for _, _, name in FORMATS:
        conv = med(("convert_latent", name)) + med(("generator_ragged", name))
        for what in ("input_batch", "convert_latent", "generator_ragged"):
            lines.append(f"   {name:8s} {what:17s} {fmt(ms[(what, name)])}")
        lines.append(f"   {name:8s} input stage / (convert_latent + generator_ragged) = {med(('input_batch', name)) / conv * 100:.3f} %")
    lines += ["", f"2. live: the input call of a tick of {B} sessions at chunk {CHUNK} beside the tick it feeds"]
    lines.append(f"   {'':8s} {'live tick':17s} {fmt(ms[('live tick', '')])}   (the chunk lasts {CHUNK * hop / model_rate * 1e3:.1f} ms)")
    for _, _, name in FORMATS:
        lines.append(f"   {name:8s} {'input_rows':17s} {fmt(ms[('input_rows tick', name)])}   = "
                     f"{med(('input_rows tick', name)) / med(('live tick', '')) * 100:.3f} % of the tick")
    assert eng.status() == 0
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
