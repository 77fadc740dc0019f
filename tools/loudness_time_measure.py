#!/usr/bin/env python3
"""Loudness over time and the leveller, measured on the GPU (default configuration, synthetic weights).
Every figure stands beside a call of the SAME run:

1. ``Engine.loudness_level`` (segments, the row's loudness, the tables over time, gains, apply: eight launches) on 16 rows of
   10 s, beside ``Engine.loudness_normalize`` (five launches) on the same rows;
2. one tick of 16 streams with pieces of 64 frames (0.74 s) -- ``loudness.push_rows``: segments_from, time, level_gains,
   level_apply -- beside that tick's ``Engine.generator_stream_rows`` call;
3. the same tick with every stream's tables 36 000 segments long (an hour in): the cost of a table entry grows with its
   position, because both gate passes run over the blocks of the prefix.  The tables are built through the table operator
   on a constructed segment table, and the tick's ``loudness_time`` call is also timed alone at both positions.

``--gate histogram`` measures, in ONE session, the histogram gate beside the exact one:

4. the tick of 16 streams 100 segments in and 36 000 segments in, under both gates, and each tick's table call alone
   (``loudness_time`` / ``loudness_time_hist``): the histogram gate's work per entry does not depend on the position;
5. ``Engine.loudness_range`` on 16 rows of 10 s beside ``Engine.loudness_level`` as a meter (``loudness_profile``'s exact call)
   and the ``Engine.generator`` call that produces 16 such rows;
6. ``max |I_h - I|`` over those rows' entries from the fourth on, beside the derived 0.05 LU.

Device-event times per call (``torch.cuda.Event``) over a window of ``steps`` calls after a warm-up of the same shape; best /
median / spread of ``rounds`` rounds that alternate over the calls.  No gate is set on any of them.

usage: tools/loudness_time_measure.py [--gate {exact,histogram}] [steps] [rounds] [out.txt]
       (default out: profiles/r23_loudness_time.txt; with --gate histogram profiles/r24_loudness_hist.txt)"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vispeech_amd import config as vcfg                 # noqa: E402
from vispeech_amd import loudness                       # noqa: E402
from vispeech_amd.models import SynthesizerTrn          # noqa: E402
from vispeech_amd.schema import dims_from_ctor          # noqa: E402
from vispeech_amd.synth import synth_state_dict         # noqa: E402

_p = argparse.ArgumentParser(description="loudness over time, measured on the GPU")
_p.add_argument("--gate", choices=("exact", "histogram"), default="exact")
_p.add_argument("steps", nargs="?", type=int, default=10)
_p.add_argument("rounds", nargs="?", type=int, default=3)
_p.add_argument("out", nargs="?", default=None)
ARGS = _p.parse_args()
STEPS, ROUNDS, GATE = ARGS.steps, ARGS.rounds, ARGS.gate
OUT = ARGS.out or os.path.join(ROOT, "profiles", "r23_loudness_time.txt" if GATE == "exact" else "r24_loudness_hist.txt")
SECONDS, B, CHUNK, LONG, SHORT = 10, 16, 64, 36000, 100


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


def main():
    a, kw0 = vcfg.synthesizer_args(vcfg.default_hparams())
    dims = dims_from_ctor(*a, **kw0)
    net = SynthesizerTrn(*a, device="cuda:0", **kw0).eval()
    net.load_state_dict(synth_state_dict(dims, seed=1234))
    eng, fs, up = net._engine, dims.sampling_rate, dims.total_upsample
    h = loudness.segment_samples(fs)
    frames = SECONDS * fs // up
    n = frames * up
    r = np.random.default_rng(23)
    sid = torch.arange(B, device="cuda:0") % dims.n_speakers
    enc = eng.encode(torch.ones((B, 2), dtype=torch.int64, device="cuda:0"), torch.full((B,), 2, dtype=torch.int64, device="cuda:0"),
                     sid, isolated=True)
    G = [enc["g"][b].reshape(-1) for b in range(B)]
    Z = torch.from_numpy(0.5 * r.standard_normal((B, dims.inter_channels, frames)).astype(np.float32)).to("cuda:0")
    # the rows measured: voiced glides whose level steps every 2.5 s (the generator's output under synthetic weights is no speech)
    t = np.arange(n) / fs
    rows = np.stack([10.0 ** (-(r.uniform(6.0, 30.0) + 6.0 * (np.floor(t / 2.5) % 2)) / 20.0) *
                     np.sin(2.0 * np.pi * np.cumsum(r.uniform(110.0, 260.0) + 40.0 * np.sin(2.0 * np.pi * r.uniform(0.5, 2.0) * t)) / fs)
                     for _ in range(B)]).astype(np.float32)
    audio = torch.from_numpy(rows).to("cuda:0")
    n_samples = [n] * B
    out = torch.empty_like(audio)
    norm = eng.loudness_params(B, -23.0, 0.9, 30.0)
    level = eng.loudness_level_params(B, -23.0)
    res = eng.loudness_level(audio, n_samples, fs, level, out=out)
    after = eng.loudness(out, n_samples, fs)[0].cpu().numpy()
    before = res["i_end"].cpu().numpy()
    c_db = res["c_db"].cpu().numpy()

    # the tick: 16 streams, each fed the next 64 frames of its row (the rows wrap around)
    piece = CHUNK * up
    spec = dict(target_lufs=-23.0)
    if GATE == "histogram":
        return histogram_session(eng, dims, audio, n_samples, Z, enc["g"], spec, r)

    def streams_at(segments):
        sts = [loudness.Stream(eng, fs, level=spec) for _ in range(B)]
        if segments:
            table = torch.from_numpy(r.uniform(0.5, 50.0, size=(B, segments))).to("cuda:0")
            for b, s in enumerate(sts):
                s._grow(segments + 4096)
                s.seg[:segments] = table[b]
            eng.loudness_time([s.seg for s in sts], 0, segments, fs, tables=tuple([getattr(s, k) for s in sts] for k in ("M", "S", "I", "kept")))
            eng.loudness_level_gains([s.I for s in sts], 0, segments, [spec] * B, tables=([s.c_db for s in sts], [s.c for s in sts]))
            for s in sts:
                s.segments, s.seen = segments, segments * h
        return sts

    near, far = streams_at(0), streams_at(LONG)
    at = [0]

    def tick(sts):
        k = at[0] % (n // piece)
        at[0] += 1
        return loudness.push_rows(eng, [(s, audio[b, k * piece: (k + 1) * piece], False) for b, s in enumerate(sts)])

    def time_alone(sts, first):
        count = piece // h
        return eng.loudness_time([s.seg for s in sts], first, count, fs, tables=tuple([getattr(s, k) for s in sts] for k in ("M", "S", "I", "kept")))

    f0 = [0]

    def generator_tick():
        k = f0[0] % (frames // CHUNK)
        f0[0] += 1
        return eng.generator_stream_rows([(Z[b], G[b], frames, k * CHUNK, (k + 1) * CHUNK) for b in range(B)], CHUNK, pcm=False)

    jobs = {
        "loudness_level": lambda: eng.loudness_level(audio, n_samples, fs, level, out=out),
        "loudness_level (meter: no params)": lambda: eng.loudness_level(audio, n_samples, fs),
        "loudness_normalize": lambda: eng.loudness_normalize(audio, n_samples, fs, norm, out=out),
        "tick: push_rows, 16 streams": lambda: tick(near),
        f"tick: push_rows at {LONG} segments": lambda: tick(far),
        "loudness_time alone, entries 8 ..": lambda: time_alone(near, 8),
        f"loudness_time alone, entries {LONG - 8} ..": lambda: time_alone(far, LONG - 8),
        "tick: generator_stream_rows": generator_tick,
    }
    ms = {k: [] for k in jobs}
    for _ in range(ROUNDS):
        for k, fn in jobs.items():
            ms[k].append(timed(fn, STEPS))
    med = lambda k: float(np.median(ms[k]))
    props = torch.cuda.get_device_properties(0)
    keys = list(jobs)
    lines = [f"loudness over time: {B} rows of {SECONDS} s at {fs} Hz ({n} samples, {n // h} segments); a tick of {B} streams with pieces "
             f"of {CHUNK} frames ({piece} samples, {piece / fs:.2f} s); {ROUNDS} rounds, a window of {STEPS} calls",
             f"device {torch.cuda.get_device_name(0)} ({getattr(props, 'gcnArchName', 'arch not available')}, "
             f"{props.multi_processor_count} CUs)",
             "timer: device events around a window of calls, per call (the Engine calls include their host work and uploads; a tick of",
             "push_rows includes its per-stream torch copies)", ""]
    for k in jobs:
        lines.append(f"   {k:44s} {fmt(ms[k])}")
    lines += ["",
              f"   loudness_level / loudness_normalize = {med(keys[0]) / med(keys[2]):.2f}",
              f"   tick of the leveller / the tick's generator call = {med(keys[3]) / med(keys[7]) * 100:.2f} %; "
              f"an hour in ({LONG} segments) {med(keys[4]) / med(keys[7]) * 100:.2f} %",
              f"   loudness_time for the tick's {piece // h} entries a stream: {med(keys[5]):.3f} ms at the start, {med(keys[6]):.3f} ms at "
              f"{LONG} segments",
              f"   rows before {before.min():.2f} .. {before.max():.2f} LUFS; levelled (target -23 LUFS, 3 dB/s, +-12 dB) "
              f"{after.min():.2f} .. {after.max():.2f} LUFS; gain at the rows' ends {np.nanmin(c_db[:, -1]):+.2f} .. {np.nanmax(c_db[:, -1]):+.2f} dB"]
    assert eng.status() == 0
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        f.write(text + "\n")


def histogram_session(eng, dims, audio, n_samples, Z, g, spec, r):
    fs, up = dims.sampling_rate, dims.total_upsample
    h = loudness.segment_samples(fs)
    n = n_samples[0]
    piece = CHUNK * up
    count = piece // h
    names = ("M", "S", "I", "kept")

    def tables(sts):
        return tuple([getattr(s, k) for s in sts] for k in names)

    def streams_at(segments, gate):
        sts = [loudness.Stream(eng, fs, level=spec, gate=gate) for _ in range(B)]
        table = torch.from_numpy(r.uniform(0.5, 50.0, size=(B, segments))).to("cuda:0")
        for b, s in enumerate(sts):
            s._grow(segments + 4096)
            s.seg[:segments] = table[b]
        if gate == "exact":
            eng.loudness_time([s.seg for s in sts], 0, segments, fs, tables=tables(sts))
        else:
            eng.loudness_time_hist([s.seg for s in sts], 0, segments, fs, [s.hist for s in sts], tables=tables(sts))
        eng.loudness_level_gains([s.I for s in sts], 0, segments, [spec] * B, tables=([s.c_db for s in sts], [s.c for s in sts]))
        for s in sts:
            s.segments, s.seen = segments, segments * h
        return sts

    sets = {(gate, at): streams_at(at, gate) for gate in ("exact", "histogram") for at in (SHORT, LONG)}
    k0 = [0]

    def tick(sts):
        k = k0[0] % (n // piece)
        k0[0] += 1
        return loudness.push_rows(eng, [(s, audio[b, k * piece: (k + 1) * piece], False) for b, s in enumerate(sts)])

    def alone(sts, first, gate):
        # (into tables and histograms of its own: the streams' must stay what their ticks left)
        tabs = tuple([torch.empty_like(getattr(s, k)) for s in sts] for k in names)
        segs = [s.seg for s in sts]
        if gate == "exact":
            return lambda: eng.loudness_time(segs, first, count, fs, tables=tabs)
        hists = [torch.zeros_like(s.hist) for s in sts]
        return lambda: eng.loudness_time_hist(segs, first, count, fs, hists, tables=tabs)

    frames = Z.shape[2]
    f0 = [0]

    def generator_tick():
        k = f0[0] % (frames // CHUNK)
        f0[0] += 1
        return eng.generator_stream_rows([(Z[b], g[b].reshape(-1), frames, k * CHUNK, (k + 1) * CHUNK) for b in range(B)], CHUNK, pcm=False)

    jobs = {}
    for at in (SHORT, LONG):
        for gate in ("exact", "histogram"):
            jobs[f"tick: push_rows at {at} segments, {gate}"] = (lambda sts: lambda: tick(sts))(sets[(gate, at)])
    for at in (SHORT, LONG):
        jobs[f"loudness_time alone, entries {at - count} .."] = alone(sets[("exact", at)], at - count, "exact")
        jobs[f"loudness_time_hist alone, entries {at - count} .."] = alone(sets[("histogram", at)], at - count, "histogram")
    jobs["tick: generator_stream_rows"] = generator_tick
    jobs["loudness_range, 16 rows of 10 s"] = lambda: eng.loudness_range(audio, n_samples, fs)
    jobs["loudness_level (meter), 16 rows of 10 s"] = lambda: eng.loudness_level(audio, n_samples, fs)
    jobs["generator, 16 rows of 10 s"] = lambda: eng.generator(Z, g)
    ms = {k: [] for k in jobs}
    for _ in range(ROUNDS):
        for k, fn in jobs.items():
            ms[k].append(timed(fn, STEPS))
    med = lambda k: float(np.median(ms[k]))
    spread = lambda k: max(ms[k]) - min(ms[k])
    # the two gates on the rows measured
    hist, exact = eng.loudness_range(audio, n_samples, fs), eng.loudness_level(audio, n_samples, fs)
    F = n // h
    Ih, I = hist["I"][:, 3:F].double().cpu().numpy(), exact["I"][:, 3:F].double().cpu().numpy()
    both = np.isfinite(Ih) & np.isfinite(I)
    same_kept = bool((hist["kept"][:, 3:F] == exact["kept"][:, 3:F]).all())
    lra = hist["lra"].cpu().numpy()
    props = torch.cuda.get_device_properties(0)
    keys = list(jobs)
    lines = [f"loudness range and the histogram gate: a tick of {B} streams with pieces of {CHUNK} frames ({piece} samples, {piece / fs:.2f} s, "
             f"{count} entries a stream) at {fs} Hz; {B} rows of {SECONDS} s ({n} samples, {F} segments); {ROUNDS} rounds, a window of {STEPS} calls",
             f"device {torch.cuda.get_device_name(0)} ({getattr(props, 'gcnArchName', 'arch not available')}, "
             f"{props.multi_processor_count} CUs)",
             "timer: device events around a window of calls, per call (the Engine calls include their host work and uploads; a tick of",
             "push_rows includes its per-stream torch copies); the streams advance with every tick, so a window of ticks ends",
             f"{(2 + STEPS) * ROUNDS * count} segments behind the position named", ""]
    for k in jobs:
        lines.append(f"   {k:52s} {fmt(ms[k])}")
    t = {(gate, at): f"tick: push_rows at {at} segments, {gate}" for gate in ("exact", "histogram") for at in (SHORT, LONG)}
    gen = med("tick: generator_stream_rows")
    d = med(t[("histogram", LONG)]) - med(t[("histogram", SHORT)])
    lines += ["",
              f"   histogram tick at {LONG} - at {SHORT} segments = {d:+.3f} ms (spreads {spread(t[('histogram', SHORT)]):.3f} / "
              f"{spread(t[('histogram', LONG)]):.3f} ms); exact tick: {med(t[('exact', LONG)]) - med(t[('exact', SHORT)]):+.3f} ms",
              f"   histogram / exact tick at {SHORT} segments = {med(t[('histogram', SHORT)]) / med(t[('exact', SHORT)]):.2f}, at {LONG} = "
              f"{med(t[('histogram', LONG)]) / med(t[('exact', LONG)]):.2f}",
              f"   tick / the tick's generator call: exact {med(t[('exact', SHORT)]) / gen * 100:.1f} % and {med(t[('exact', LONG)]) / gen * 100:.1f} %; "
              f"histogram {med(t[('histogram', SHORT)]) / gen * 100:.1f} % and {med(t[('histogram', LONG)]) / gen * 100:.1f} %",
              f"   loudness_range / loudness_level (meter) = {med(keys[-3]) / med(keys[-2]):.2f}; / the generator call of the rows = "
              f"{med(keys[-3]) / med(keys[-1]) * 100:.2f} %",
              f"   max |I_h - I| over {int(both.sum())} entries of the rows = {float(np.abs(Ih - I)[both].max()):.4f} LU (derived: 0.05 where every "
              f"prefix stays 1.05 clear of both gates); kept equal at every entry: {same_kept}; LRA of the rows {lra.min():.1f} .. {lra.max():.1f} LU"]
    assert eng.status() == 0
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
