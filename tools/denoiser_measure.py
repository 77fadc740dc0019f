#!/usr/bin/env python3
"""The denoiser and the inverse STFT, measured on the GPU (default configuration, synthetic weights):
``Engine.denoise`` on 16 rows of 10 s at the model's rate beside the ``Engine.generator_ragged`` call that produces such
rows, ``Engine.istft`` (the inverse convolution and the overlap-add kernel) and ``Engine.spectrogram_ragged`` (framing, the
forward convolution on the form launch_conv picks, magnitude) on the same rows, in one session.

Device-event times per call (``torch.cuda.Event``) over a window of ``steps`` calls after a warm-up of the same shape; best /
median / spread of ``rounds`` rounds that alternate over the calls.  The two convolutions of a ``denoise`` call are then
read from the library's own per-launch events (``Engine.profile``, class FRAME: one event pair a launch), and so is the
one of an ``istft`` call; the three small kernels are what is left of the call, and the overlap-add kernel what is left of
``istft``.  Per kernel: run the tool under ``rocprofv3 --kernel-trace --stats --output-format csv`` (the table under the
tool's own lines in profiles/r25_denoiser.txt).  No gate is set on any of them.

``--stream`` measures the denoiser for streams instead: one tick of 16 streams, each pushing a piece of
64 frames through ``denoiser.push_rows`` (ONE ``vsp_denoise_rows`` call: 67 frames a row, 3 of them the overlap an earlier
tick computed too), beside that tick's ``Engine.generator_stream_rows`` call and beside ``Engine.denoise`` on the same 16
pieces as whole rows.  The streams run on (their pieces cycle over the 10 s rows), so every timed tick is a steady-state one.

``--transform fft``, alone or with ``--stream``: the same rows under both transforms, ``dft`` and
``fft`` alternating call by call's window in one session, each with the bias of its own transform; per launch, the two
products of the one and the fused launch of the other from the library's events.  The frames a block of the FFT kernels owns
is the process's (``VSP_FFT_TILE`` = 4 / 8 / 16, default 8): one run per tile size.

usage: tools/denoiser_measure.py [--stream] [--transform fft] [steps] [rounds] [out.txt]
       (default out: profiles/r25_denoiser.txt, with --stream profiles/r26_denoiser_stream.txt, with --transform fft
       profiles/r27_denoiser_fft.txt)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vispeech_amd import _lib                           # noqa: E402
from vispeech_amd import config as vcfg                 # noqa: E402
from vispeech_amd.models import SynthesizerTrn          # noqa: E402
from vispeech_amd.schema import dims_from_ctor          # noqa: E402
from vispeech_amd.synth import synth_state_dict         # noqa: E402

STREAM = "--stream" in sys.argv[1:]
ARGS = [a for a in sys.argv[1:] if a != "--stream"]
TRANSFORM = "dft"
if "--transform" in ARGS:
    i = ARGS.index("--transform")
    TRANSFORM = ARGS[i + 1] if i + 1 < len(ARGS) else ""
    if TRANSFORM not in ("dft", "fft"):
        sys.exit("--transform dft | fft")
    del ARGS[i:i + 2]
FFT = TRANSFORM == "fft"
TILE = os.environ.get("VSP_FFT_TILE", "8")
STEPS = int(ARGS[0]) if len(ARGS) > 0 else 10
ROUNDS = int(ARGS[1]) if len(ARGS) > 1 else 3
OUT = ARGS[2] if len(ARGS) > 2 else os.path.join(
    ROOT, "profiles", "r27_denoiser_fft.txt" if FFT else "r26_denoiser_stream.txt" if STREAM else "r25_denoiser.txt")
SECONDS, B = 10, 16
CHUNK = 64                                             # frames of a piece: the streaming service's default chunk


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


def convs(eng, fn, calls=5):
    """(launches per call, ms per call) of the frame-rate convolutions of ``fn``, from the library's per-launch events."""
    fn()
    torch.cuda.synchronize()
    eng.profile(True)
    eng.profile_read(True, _lib.PROF_FRAME)
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    n, ms = eng.profile_read(True, _lib.PROF_FRAME)[:2]
    eng.profile(False)
    return n / calls, ms / calls


def main():
    a, kw0 = vcfg.synthesizer_args(vcfg.default_hparams())
    dims = dims_from_ctor(*a, **kw0)
    net = SynthesizerTrn(*a, device="cuda:0", **kw0).eval()
    net.load_state_dict(synth_state_dict(dims, seed=1234))
    eng, fs, up = net._engine, dims.sampling_rate, dims.total_upsample
    spec, N = dims.spec_channels, 2 * (dims.spec_channels - 1)
    frames = SECONDS * fs // up
    n = frames * up
    r = np.random.default_rng(25)
    sid = [b % dims.n_speakers for b in range(B)]
    G = torch.from_numpy(net._state["emb_g.weight"][sid]).to("cuda:0")
    Z = torch.from_numpy(0.5 * r.standard_normal((B, dims.inter_channels, frames)).astype(np.float32)).to("cuda:0")
    lengths = [frames] * B
    audio = eng.generator_ragged(Z, G, lengths)[:, 0, :].contiguous()          # the rows measured: the generator's own
    n_samples = [n] * B
    bias = net.denoiser_bias(sid)
    if STREAM:
        return stream_main(net, dims, audio, Z, G, bias, frames, net.denoiser_bias(sid, "fft") if FFT else None)
    T = eng.convert_frames(n, up)
    if FFT:
        return fft_main(net, dims, audio, n_samples, Z, G, lengths, bias, net.denoiser_bias(sid, "fft"), T)
    out = torch.empty_like(audio)
    ri = torch.zeros((B, 2 * spec, T), dtype=torch.float32, device="cuda:0")
    jobs = {
        "denoise (strength 0.01)": lambda: eng.denoise(audio, n_samples, bias, 0.01, out=out),
        "istft": lambda: eng.istft(ri, n_samples),
        "spectrogram_ragged": lambda: eng.spectrogram_ragged(audio, n_samples),
        "generator_ragged": lambda: eng.generator_ragged(Z, G, lengths),
    }
    ms = {k: [] for k in jobs}
    for _ in range(ROUNDS):
        for k, fn in jobs.items():
            ms[k].append(timed(fn, max(STEPS // 2, 2) if k == "generator_ragged" else STEPS))
    med = lambda k: float(np.median(ms[k]))
    n_all, c_all = convs(eng, jobs["denoise (strength 0.01)"])
    n_inv, c_inv = convs(eng, jobs["istft"])
    flop = 2.0 * (2 * spec) * N * T * B                                        # one DFT product
    props = torch.cuda.get_device_properties(0)
    den, ist = med("denoise (strength 0.01)"), med("istft")
    lines = [f"denoiser: {B} rows of {SECONDS} s at {fs} Hz ({n} samples, {T} frames); {ROUNDS} rounds, a window of {STEPS} calls "
             f"({max(STEPS // 2, 2)} for generator_ragged)",
             f"device {torch.cuda.get_device_name(0)} ({getattr(props, 'gcnArchName', 'arch not available')}, "
             f"{props.multi_processor_count} CUs)",
             "timer: device events around a window of calls, per call (the Engine calls include their host work and uploads)", ""]
    for k in jobs:
        lines.append(f"   {k:30s} {fmt(ms[k])}")
    lines += ["",
              f"   denoise / generator_ragged = {den / med('generator_ragged') * 100:.2f} %",
              f"   the two DFT products: {2 * flop / 1e9:.1f} GFLOP a call ({flop / 1e9:.1f} each: {2 * spec} x {N} x {T} frames x {B} rows)",
              "   per launch, from the library's own events (profiling on):",
              f"      both convolutions of a denoise call ({n_all:.0f} launches)      {c_all:8.3f} ms  ({2 * flop / c_all / 1e9:.1f} TFLOP/s)",
              f"      framing, subtraction and overlap-add (what is left)  {den - c_all:8.3f} ms",
              f"      the convolution of an istft call ({n_inv:.0f} launch)           {c_inv:8.3f} ms  ({flop / c_inv / 1e9:.1f} TFLOP/s; its operand is the "
              f"caller's dense RI, rows of {T} floats: not 16-byte aligned unless T_max is a multiple of 4)",
              f"      overlap-add (istft less its convolution)             {ist - c_inv:8.3f} ms"]
    assert eng.status() == 0
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        f.write(text + "\n")


def fft_main(net, dims, audio, n_samples, Z, G, lengths, bias, bias_fft, T):
    """``denoise`` and ``istft`` under both transforms, alternating, and the per-launch split of each."""
    eng, fs = net._engine, dims.sampling_rate
    spec, N = dims.spec_channels, 2 * (dims.spec_channels - 1)
    out = torch.empty_like(audio)
    ri = torch.zeros((B, 2 * spec, T), dtype=torch.float32, device="cuda:0")
    jobs = {
        "denoise dft (strength 0.01)": lambda: eng.denoise(audio, n_samples, bias, 0.01, out=out),
        "denoise fft (strength 0.01)": lambda: eng.denoise(audio, n_samples, bias_fft, 0.01, out=out, transform="fft"),
        "istft dft": lambda: eng.istft(ri, n_samples),
        "istft fft": lambda: eng.istft(ri, n_samples, transform="fft"),
        "generator_ragged": lambda: eng.generator_ragged(Z, G, lengths),
    }
    ms = {k: [] for k in jobs}
    for _ in range(ROUNDS):
        for k, fn in jobs.items():
            ms[k].append(timed(fn, max(STEPS // 2, 2) if k == "generator_ragged" else STEPS))
    med = lambda k: float(np.median(ms[k]))
    split = {k: convs(eng, jobs[k]) for k in jobs if k != "generator_ragged"}
    d_dft, d_fft = med("denoise dft (strength 0.01)"), med("denoise fft (strength 0.01)")
    moved = 2.0 * 4.0 * B * N * T                                              # the frame tensor in, the synthesis frames out
    props = torch.cuda.get_device_properties(0)
    lines = [f"denoiser on the in-LDS FFT: {B} rows of {SECONDS} s at {fs} Hz ({n_samples[0]} samples, {T} frames); {ROUNDS} rounds that "
             f"alternate over the calls, a window of {STEPS} calls ({max(STEPS // 2, 2)} for generator_ragged)",
             f"device {torch.cuda.get_device_name(0)} ({getattr(props, 'gcnArchName', 'arch not available')}, "
             f"{props.multi_processor_count} CUs); frames a block of the FFT kernels: {TILE}",
             "timer: device events around a window of calls, per call (the Engine calls include their host work and uploads)", ""]
    for k in jobs:
        lines.append(f"   {k:30s} {fmt(ms[k])}")
    lines += ["",
              f"   denoise fft / denoise dft = {d_fft / d_dft:.3f};  of generator_ragged: dft {d_dft / med('generator_ragged') * 100:.2f} %, "
              f"fft {d_fft / med('generator_ragged') * 100:.2f} %",
              "   per launch, from the library's own events (profiling on):"]
    for k, (n_l, c) in split.items():
        what = "fused launch" if k.startswith("denoise fft") else "inverse launch" if k == "istft fft" else "product(s)"
        lines.append(f"      {k:30s} {n_l:.0f} {what:15s} {c:8.3f} ms   the rest of the call (framing, subtraction, overlap-add) {med(k) - c:8.3f} ms")
    c_fused, c_prod = split["denoise fft (strength 0.01)"][1], split["denoise dft (strength 0.01)"][1]
    lines += [f"   the fused launch moves {moved / 1e6:.0f} MB (frames in, synthesis frames out, in place): {moved / c_fused / 1e9:.2f} TB/s; "
              f"fused launch / the two products = {c_fused / c_prod:.3f}"]
    assert eng.status() == 0
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        f.write(text + "\n")


def stream_main(net, dims, audio, Z, G, bias, frames, bias_fft=None):
    from vispeech_amd import denoiser
    eng, fs, up = net._engine, dims.sampling_rate, dims.total_upsample
    N = 2 * (dims.spec_channels - 1)
    piece = CHUNK * up
    per_row = frames // CHUNK                              # whole pieces in a 10 s row
    streams = [denoiser.Stream(eng, bias[b], 0.01) for b in range(B)]
    state = {"k": 0, "out": 0}

    def tick(streams=streams, state=state):
        k = state["k"] % per_row
        state["k"] += 1
        outs = denoiser.push_rows(eng, [(streams[b], audio[b, k * piece:(k + 1) * piece], False) for b in range(B)])
        state["out"] = sum(int(o.shape[0]) for o in outs)

    f0 = frames // 2                                       # the generator's tick: every row mid-utterance
    rows = [(Z[b], G[b], frames, f0, f0 + CHUNK) for b in range(B)]
    whole = audio[:, :piece].contiguous()
    out = torch.empty_like(whole)
    jobs = {
        "denoiser.push_rows (a tick)": tick,
        "denoise (the pieces, whole)": lambda: eng.denoise(whole, [piece] * B, bias, 0.01, out=out),
        "generator_stream_rows (a tick)": lambda: eng.generator_stream_rows(rows, CHUNK, pcm=False),
    }
    if bias_fft is not None:                               # the same tick and the same pieces on the FFT, alternating with the above
        streams_fft = [denoiser.Stream(eng, bias_fft[b], 0.01, transform="fft") for b in range(B)]
        state_fft = {"k": 0, "out": 0}
        jobs["denoiser.push_rows fft (a tick)"] = lambda: tick(streams_fft, state_fft)
        jobs["denoise fft (the pieces, whole)"] = lambda: eng.denoise(whole, [piece] * B, bias_fft, 0.01, out=out, transform="fft")
    ms = {k: [] for k in jobs}
    for _ in range(ROUNDS):
        for k, fn in jobs.items():
            ms[k].append(timed(fn, STEPS))
    med = lambda k: float(np.median(ms[k]))
    assert state["out"] == B * piece                       # steady state: a tick puts out what it takes in
    T = CHUNK + N // up - 1
    props = torch.cuda.get_device_properties(0)
    lines = [f"denoiser for streams: a tick of {B} streams, each a piece of {CHUNK} frames ({piece} samples, {piece / fs * 1e3:.0f} ms at {fs} Hz); "
             f"{ROUNDS} rounds, a window of {STEPS} calls",
             f"device {torch.cuda.get_device_name(0)} ({getattr(props, 'gcnArchName', 'arch not available')}, "
             f"{props.multi_processor_count} CUs)",
             "timer: device events around a window of calls, per call (the calls include their host work: a tick's also the",
             "       streams' buffers -- one torch.cat and one slice a stream)", ""]
    for k in jobs:
        lines.append(f"   {k:32s} {fmt(ms[k])}")
    push, one, gen = med("denoiser.push_rows (a tick)"), med("denoise (the pieces, whole)"), med("generator_stream_rows (a tick)")
    lines += ["",
              f"   a tick's windows hold {T} frames a row, {T - CHUNK} of them computed by the tick before too ({(T - CHUNK) / T * 100:.1f} %)",
              f"   push_rows / denoise of the same pieces whole = {push / one:.2f}",
              f"   push_rows / generator_stream_rows            = {push / gen * 100:.2f} %",
              f"   algorithmic delay of the stream: {N - up} .. {N - 1} samples ({(N - up) / fs * 1e3:.1f} .. {(N - 1) / fs * 1e3:.1f} ms)"]
    if bias_fft is not None:
        assert state_fft["out"] == B * piece
        push_fft = med("denoiser.push_rows fft (a tick)")
        lines += [f"   frames a block of the FFT kernels: {TILE}",
                  f"   push_rows fft / push_rows dft                = {push_fft / push:.3f}",
                  f"   push_rows fft / generator_stream_rows        = {push_fft / gen * 100:.2f} %",
                  f"   denoise fft / denoise dft (the pieces whole) = {med('denoise fft (the pieces, whole)') / one:.3f}"]
    assert eng.status() == 0
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
