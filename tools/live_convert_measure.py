#!/usr/bin/env python3
"""Live voice conversion, measured on the GPU (default configuration, synthetic weights).

1. The time of one tick of 1 / 16 / 64 live rows at chunks of 16 / 32 / 64 frames, in steady state (interior windows: both
   halos full): one ``Engine.convert_stream_rows`` call, one ``Engine.generator_stream_rows`` call on its rows and the
   device-to-host copy of the PCM16 block -- what ``StreamingBatchService.step`` runs for them -- against the duration of
   the chunk, the only condition a live conversion has (a tick must take less than its chunk lasts).
2. The same recordings (10 s each) converted one-shot, ``Engine.convert`` (``convert_latent`` + ``generator_ragged``), against
   the ticks it takes to stream them: what recomputing the halo every tick costs, beside the arithmetic factor
   (chunk + 2 (G + H)) / chunk.
3. The workspace of a 10-minute recording, one-shot against live (sizing passes only; nothing that large is run).

Every timing is a host clock (``time.perf_counter``) around work that ends in a device synchronise, after a warm-up of the
same shape; rounds alternate over the configurations and the spread of the rounds is printed.

usage: tools/live_convert_measure.py [steps] [rounds] [out.txt]     (default out: profiles/r15_live_convert.txt)"""
import os
import platform
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vispeech_amd import config as vcfg                 # noqa: E402
from vispeech_amd.models import SynthesizerTrn          # noqa: E402
from vispeech_amd.schema import convert_halo_frames, dims_from_ctor  # noqa: E402
from vispeech_amd.synth import synth_state_dict         # noqa: E402

STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "r15_live_convert.txt")
RATE, SECONDS = 44100, 10
ROWS, CHUNKS = (1, 16, 64), (16, 32, 64)


def timed(fn, steps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    a, kw0 = vcfg.synthesizer_args(vcfg.default_hparams())
    dims = dims_from_ctor(*a, **kw0)
    net = SynthesizerTrn(*a, device="cuda:0", **kw0).eval()
    net.load_state_dict(synth_state_dict(dims, seed=1234))
    eng = net._engine
    hop, n_fft, up = dims.hop_length, 2 * (dims.spec_channels - 1), dims.total_upsample
    pad = (n_fft - hop) // 2
    G, H = eng.generator_halo, convert_halo_frames(dims)
    assert H == eng.convert_halo
    r = np.random.Generator(np.random.PCG64(15))
    n = SECONDS * RATE
    T = eng.convert_frames(n)
    t = np.arange(n) / RATE
    audio = (0.4 * np.sin(2 * np.pi * 220.0 * t) + 0.1 * r.standard_normal(n)).astype(np.float32).clip(-1, 1)
    dev = torch.from_numpy(audio).to("cuda:0")
    props = torch.cuda.get_device_properties(0)
    lines = [f"live voice conversion: default configuration, G = {G} (vocoder halo), H = {H} (conversion halo), hop {hop}, "
             f"n_fft {n_fft}; recordings of {SECONDS} s ({T} frames); {STEPS} steps x {ROUNDS} rounds per figure",
             f"device {torch.cuda.get_device_name(0)} ({getattr(props, 'gcnArchName', 'arch not available')}, "
             f"{props.multi_processor_count} CUs), host {platform.node()}",
             "timer: time.perf_counter around a synchronised window, per call",
             f"algorithmic delay: (G + H) * hop + n_fft - pad = {(G + H) * hop + n_fft - pad} samples = "
             f"{((G + H) * hop + n_fft - pad) / RATE:.3f} s, plus the chunk", ""]

    def tick_of(B, chunk):
        """An interior tick: frames [f0, f0 + chunk) of B open recordings, every sample the windows read arrived."""
        f0 = G + H + 8
        f1 = f0 + chunk
        e0, e1 = f0 - G, f1 + G
        n_known = (e1 + H - 1) * hop - pad + n_fft
        assert n_known <= n and eng.convert_window_plan(n_known, False, e0, e1)[0]
        rows = [(dev, 0, n_known, False, e0, e1, b % dims.n_speakers, (b + 7) % dims.n_speakers, 100 + b, 1.0) for b in range(B)]

        def tick():
            z, g = eng.convert_stream_rows(rows, chunk + 2 * G)
            out = eng.generator_stream_rows([(z[b], g[b], e1 - e0, f0 - e0, f1 - e0) for b in range(B)], chunk, pcm=True)
            return out.cpu()
        return tick

    ticks = {(B, c): tick_of(B, c) for B in ROWS for c in CHUNKS}
    ms = {k: [] for k in ticks}
    for _ in range(ROUNDS):
        for k, fn in ticks.items():
            ms[k].append(timed(fn, STEPS))
    lines.append("1. one tick in steady state: convert_stream_rows + generator_stream_rows + the PCM16 copy")
    lines.append(f"   {'rows':>4s} {'chunk':>5s} {'window':>6s} {'redundancy':>10s} {'best ms':>9s} {'median':>9s} {'spread':>8s} "
                 f"{'chunk ms':>9s} {'margin':>8s}")
    worst = None
    for (B, c), v in ms.items():
        dur = c * hop / RATE * 1e3
        margin = dur / float(np.median(v))
        worst = margin if worst is None else min(worst, margin)
        lines.append(f"   {B:4d} {c:5d} {c + 2 * (G + H):6d} {(c + 2 * (G + H)) / c:10.2f} {min(v):9.3f} {float(np.median(v)):9.3f} "
                     f"{max(v) - min(v):8.3f} {dur:9.1f} {margin:7.1f}x")
    lines.append(f"   margin = chunk duration / median tick; the smallest measured: {worst:.1f}x "
                 f"({'every tick takes less than its chunk lasts' if worst > 1 else 'A TICK TAKES LONGER THAN ITS CHUNK'})")

    lines += ["", f"2. {SECONDS} s recordings: one-shot Engine.convert (convert_latent + generator_ragged) against streaming them live"]
    for B in ROWS:
        batch = dev[None, :].expand(B, n).contiguous()
        src, tgt = [b % dims.n_speakers for b in range(B)], [(b + 7) % dims.n_speakers for b in range(B)]
        seeds = list(range(100, 100 + B))
        one = [timed(lambda: eng.convert(batch, [n] * B, src, tgt, noise_seed=seeds), max(STEPS // 2, 2)) for _ in range(ROUNDS)]
        del batch
        cols = []
        for c in CHUNKS:
            n_ticks = -(-T // c)
            live = n_ticks * float(np.median(ms[(B, c)]))
            cols.append(f"chunk {c}: {n_ticks} ticks = {live:8.1f} ms ({live / float(np.median(one)):5.2f}x)")
        lines.append(f"   {B:2d} rows: one-shot best {min(one):8.3f} ms median {float(np.median(one)):8.3f} ms spread "
                     f"{max(one) - min(one):6.3f} ms | live, every tick at the steady-state cost: " + "; ".join(cols))

    lines += ["", "3. workspace of one 10-minute recording (sizing passes; bytes)"]
    n10 = 600 * RATE
    T10 = eng.convert_frames(n10)
    lat = int(eng.lib.vsp_convert_latent_workspace_bytes(eng.ctx, 1, n10, hop))
    gen = int(eng.lib.vsp_generator_workspace_bytes(eng.ctx, 1, T10))
    held = 4 * (n10 + 3 * dims.inter_channels * T10 + T10 * up)        # the recording, z / z_p / z_hat and the waveform
    lines.append(f"   one-shot ({T10} frames): convert_latent {lat:,} + generator {gen:,} (one after the other: peak "
                 f"{max(lat, gen):,}), beside {held:,} of audio, latents and waveform")
    for c in CHUNKS:
        cw = int(eng.lib.vsp_convert_stream_rows_workspace_bytes(eng.ctx, 1, c + 2 * G))
        gw = int(eng.lib.vsp_generator_stream_rows_workspace_bytes(eng.ctx, 1, c))
        buf = 4 * ((c + 2 * (G + H) - 1) * hop + n_fft)
        lines.append(f"   live, chunk {c}: convert_stream_rows {cw:,} + generator_stream_rows {gw:,} (peak {max(cw, gw):,}), beside "
                     f"{buf:,} of window samples: one-shot peak / live peak = {max(lat, gen) / max(cw, gw):.0f}x")
    assert eng.status() == 0
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
