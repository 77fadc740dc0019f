"""The true-peak meter and the look-ahead limiter on the GPU against the restatement
(tests/limiter_ref.py): one ragged batch -- the fixture rows, rows of the lengths at which the kernels change path (1, 5,
A + H - 1, a tile of either kernel minus and plus one, several tiles and a ragged rest), NaN behind every row's end and a
NaN-ceiling row in the middle -- at (attack, hold) = (66, 882), (0, 0), (1, 0) and the maxima (1024, 8192); the exact
properties; the ragged contract; streams under any split against the whole, library against library; the limited
normalisation; the true peak of what the limiter puts out; and both services against the direct path.

The gate of a row is NOT taken from the library: it is 4 times the distance of the restatement's float32 run from its fp64
run on that row (measured on the CPU: 1e-7 .. 7e-7 at attack 66, up to 1.2e-5 at attack 1024, where 1025 values are
summed; exactly 0 on silence and on the clicks at attack 0), and at least FLOOR = 2^-21 = 4.8e-7.  The floor is the number
format's, not the code's: outputs, gains and peaks here are at most about 1, where a float32 rounding is up to 2^-25; the
path to an output has some sixteen of them that the two float32 runs need not share (numpy has no fused multiply-add, so
the float32 run's chains round twice; a quotient one place off moves the minimum, the sum and the product), and on rows
where the float32 run happens to agree with fp64 the measured distance alone would leave no room for them.

The restatement's OWN true-peak overshoot of the limited fixtures, measured on the CPU: at most +0.0003 dB over the ceiling
at (66, 882) and 0.0000 dB at (1024, 8192); with next to no attack the sample ceiling still holds but the true peak does
not: up to +2.0 dB at (0, 0) and +1.1 dB at (1, 0) (the loud row)."""
import numpy as np
import pytest
import torch

import limiter_ref as lr

pytestmark = pytest.mark.gpu

WINDOWS = ((66, 882), (0, 0), (1, 0), (1024, 8192))
FLOOR = 2.0 ** -21
NAN = float("nan")
T1, T2 = 1024, 2048                                       # the tiles of the two kernels


def to_np(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from vispeech_amd.engine import Engine
    from vispeech_amd.schema import ModelDims
    return Engine(ModelDims(), "cuda:0")                   # (the limiter needs no weights)


@pytest.fixture(scope="module")
def rows():
    """[(name, x, g, c)]: the fixture rows, then the rows of the lengths, with a NaN-ceiling row in the middle."""
    out = list(lr.fixture_rows())
    out.append(("left_alone", lr.voiced(1500, 23), 4.0, NAN))
    for i, n in enumerate((1, 5, 66 + 882 - 1, T1 - 1, T1 + 1, T2 - 1, T2 + 1, 3 * T2 + 777)):
        x = lr.voiced(max(n, 64), 40 + i)[:n]
        if n <= 5:
            x = (x + np.float32(0.5)).astype(np.float32)   # (so that the shortest rows are limited too)
        out.append((f"n{n}", x, 3.0, 0.9))
    return out


@pytest.fixture(scope="module")
def ref(rows):
    """Per window and row: the restatement's fp64 and float32 runs, computed once."""
    out = {}
    for A, H in WINDOWS:
        out[A, H] = [None if c != c else (lr.limit(x, g, c, A, H), lr.limit(x, g, c, A, H, np.float32)) for _, x, g, c in rows]
    return out


@pytest.fixture(scope="module")
def run(eng, rows):
    """Per window: the library's out-of-place and in-place runs of the batch."""
    audio, n = lr.pack([x for _, x, _, _ in rows])
    g = [r[2] for r in rows]
    c = [r[3] for r in rows]
    dev = torch.from_numpy(audio).to(eng.device)
    out = dict(audio=audio, n=n, g=g, c=c, dev=dev, tp=to_np(eng.true_peak(dev, n)))
    for A, H in WINDOWS:
        o = torch.full_like(dev, 7.0)
        o2, mg = eng.limit(dev, n, c, gains=g, attack=A, hold=H, out=o)
        assert o2 is o
        inplace = dev.clone()
        p2, mg2 = eng.limit(inplace, n, c, gains=g, attack=A, hold=H)
        assert p2 is inplace
        out[A, H] = dict(out=to_np(o), mg=to_np(mg), inplace=to_np(inplace), mg_inplace=to_np(mg2))
    assert np.array_equal(bits(to_np(dev)), bits(audio))   # out of place: the input is untouched
    return out


def test_true_peak_against_the_restatement(rows, run):
    for b, (name, x, _, _) in enumerate(rows):
        t64, t32 = float(lr.true_peak(x)), float(lr.true_peak(x, np.float32))
        gate = max(4.0 * abs(t32 - t64), FLOOR)
        got = float(run["tp"][b])
        print(f"{name}: tp {got:.7f} restated {t64:.7f} distance {abs(got - t64):.2e} gate {gate:.2e}")
        assert abs(got - t64) <= gate, name
        if name.startswith("click"):
            assert bits(run["tp"][b]) == bits(np.float32(1.0)), name       # the peak is a sample value: exact
    assert run["tp"][0] == 0.0                                              # silence


@pytest.mark.parametrize("A,H", WINDOWS)
def test_ragged_batch_against_the_restatement(rows, ref, run, A, H):
    r = run[A, H]
    for b, (name, x, g, c) in enumerate(rows):
        if c != c:
            continue
        d, f = ref[A, H][b]
        n = len(x)
        gate = max(4.0 * float(np.abs(f["out"].astype(np.float64) - d["out"]).max()), FLOOR)
        gate_mg = max(4.0 * abs(float(f["min_gain"]) - float(d["min_gain"])), FLOOR)
        dist = float(np.abs(r["out"][b, :n].astype(np.float64) - d["out"]).max())
        dist_mg = abs(float(r["mg"][b]) - float(d["min_gain"]))
        print(f"({A}, {H}) {name}: out {dist:.2e} (gate {gate:.2e})  min_gain {dist_mg:.2e} (gate {gate_mg:.2e})")
        assert dist <= gate, name
        assert dist_mg <= gate_mg, name


@pytest.mark.parametrize("A,H", WINDOWS)
def test_exact_properties(rows, run, A, H):
    r = run[A, H]
    audio, n = run["audio"], run["n"]
    names = [row[0] for row in rows]
    for b, (name, x, g, c) in enumerate(rows):
        if c != c:                                          # the row left alone: not written out of place, unchanged in place
            assert np.all(r["out"][b] == 7.0) and np.array_equal(bits(r["inplace"][b]), bits(audio[b]))
            assert r["mg"][b] == 1.0
            continue
        assert np.abs(r["out"][b, :n[b]]).max() <= np.float32(c), name
        assert np.all(r["out"][b, n[b]:] == 7.0), name                      # nothing behind the row's end is written
        assert np.array_equal(bits(r["inplace"][b, n[b]:]), bits(audio[b, n[b]:])), name
    b = names.index("never_limited")
    assert np.array_equal(bits(r["out"][b, :n[b]]), bits(np.float32(rows[b][2]) * rows[b][1])) and r["mg"][b] == 1.0
    for b, (name, _, _, c) in enumerate(rows):             # in place equals out of place
        if c == c:
            assert np.array_equal(bits(r["inplace"][b, :n[b]]), bits(r["out"][b, :n[b]])), name
    assert np.array_equal(bits(r["mg"]), bits(r["mg_inplace"]))


@pytest.mark.parametrize("A,H", ((66, 882), (1024, 8192)))
def test_a_row_alone_gives_the_bits_of_its_batch(eng, rows, run, A, H):
    r = run[A, H]
    for b, (name, x, g, c) in enumerate(rows):
        if c != c:
            continue
        one = torch.from_numpy(np.concatenate([x, np.full(3, np.nan, np.float32)])[None, :]).to(eng.device)
        assert bits(to_np(eng.true_peak(one, [len(x)])))[0] == bits(run["tp"])[b], name
        o, mg = eng.limit(one, [len(x)], c, gains=[g], attack=A, hold=H)      # (in place)
        assert np.array_equal(bits(to_np(o)[0, :len(x)]), bits(r["out"][b, :len(x)])), name
        assert bits(to_np(mg))[0] == bits(r["mg"])[b], name


def _stream_whole(eng, x, g, c, A, H, sizes):
    from vispeech_amd import limiter
    s = limiter.Stream(eng, c, gain=g, attack=A, hold=H)
    dev = torch.from_numpy(x).to(eng.device)
    got, k = [], 0
    for i, m in enumerate(sizes):
        got.append(s.push(dev[k:k + m], final=(k + m >= len(x))))
        k += m
    assert k >= len(x)
    return to_np(torch.cat(got))


@pytest.mark.parametrize("A,H,N,split", ((16, 100, 400, "ones"), (66, 882, 5000, "sevens"), (66, 882, 3 * T2 + 777, "tile"),
                                         (66, 882, 3 * T2 + 777, "random"), (1024, 8192, 3 * T2 + 777, "random"), (0, 0, 700, "random")))
def test_streams_under_any_split_equal_the_whole(eng, A, H, N, split):
    x = lr.voiced(N, 61)
    g, c = 3.0, 0.9
    whole, mg = eng.limit(torch.from_numpy(x[None, :].copy()).to(eng.device), [N], c, gains=[g], attack=A, hold=H)
    whole = to_np(whole)[0]
    assert to_np(mg)[0] < 1.0                              # (the row is limited)
    rng = np.random.default_rng(5)
    if split == "ones":
        sizes = [1] * N
    elif split == "sevens":
        sizes = [7] * (N // 7 + 1)
    elif split == "tile":
        sizes = [T2] * (N // T2 + 1)
    else:
        sizes = []
        while sum(sizes) < N:
            sizes.append(int(rng.integers(1, 1500)))
    sizes[-1] -= sum(sizes) - N
    got = _stream_whole(eng, x, g, c, A, H, [m for m in sizes if m > 0])
    assert got.shape == whole.shape and np.array_equal(bits(got), bits(whole))


def test_streams_at_different_positions_share_one_call(eng):
    from vispeech_amd import limiter
    A, H = 66, 882
    xs = [lr.voiced(5000, 71), lr.voiced(3000, 72), lr.voiced(900, 73)]
    gs, cs = [3.0, 8.0, 2.0], [0.9, 0.5, 0.9]
    steps = [700, 333, 450]
    streams = [limiter.Stream(eng, c, gain=g, attack=A, hold=H) for g, c in zip(gs, cs)]
    got, pos = [[] for _ in xs], [0, 0, 0]
    while any(p < len(x) for p, x in zip(pos, xs)):
        pushes = []
        for i, x in enumerate(xs):
            if pos[i] < len(x):
                seg = torch.from_numpy(x[pos[i]:pos[i] + steps[i]].copy()).to(eng.device)
                pos[i] += steps[i]
                pushes.append((i, (streams[i], seg, pos[i] >= len(x))))
        for (i, _), y in zip(pushes, limiter.push_rows(eng, [p for _, p in pushes])):
            got[i].append(y)
    for i, x in enumerate(xs):
        whole, _ = eng.limit(torch.from_numpy(x[None, :].copy()).to(eng.device), [len(x)], cs[i], gains=[gs[i]], attack=A, hold=H)
        assert np.array_equal(bits(to_np(torch.cat(got[i]))), bits(to_np(whole)[0])), i


def test_true_peak_of_the_limited_fixtures(eng, rows, ref, run):
    """The library's true peak of its own output stays within the restatement's own overshoot for the row plus the row's
    gate, carried through the meter: a sample moved by d moves an oversampled value by at most d times the largest phase's
    sum of |taps|."""
    h = lr.taps().astype(np.float64)
    l1 = max(np.abs(h[ph::4]).sum() for ph in range(4))
    for A, H in WINDOWS:
        r = run[A, H]
        o = torch.from_numpy(np.nan_to_num(r["out"], nan=0.0)).to(eng.device)
        tp = to_np(eng.true_peak(o, run["n"]))
        for b, (name, x, g, c) in enumerate(rows):
            if c != c:
                continue
            d, f = ref[A, H][b]
            own = float(lr.true_peak(d["out"].astype(np.float32)))
            gate = max(4.0 * float(np.abs(f["out"].astype(np.float64) - d["out"]).max()), FLOOR)
            print(f"({A}, {H}) {name}: true peak out {tp[b]:.6f} = {lr.db(tp[b] / c):+.4f} dB re ceiling; restated {own:.6f}")
            assert tp[b] <= own + l1 * gate, name
            if (A, H) == (66, 882) and name in [fr[0] for fr in lr.fixture_rows()]:
                assert lr.db(own / c) <= 0.011, name                       # what the documents state as measured


# ---------------------------------------------------------------------------------------------- the model
@pytest.fixture(scope="module")
def net():
    from vispeech_amd import config as vcfg
    from vispeech_amd.models import SynthesizerTrn
    from vispeech_amd.schema import dims_from_ctor
    from vispeech_amd.synth import synth_state_dict
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    ctor = vcfg.synthesizer_args(vcfg.default_hparams())
    m = SynthesizerTrn(*ctor[0], **ctor[1]).eval()
    m.load_state_dict(synth_state_dict(dims_from_ctor(*ctor[0], **ctor[1]), seed=1234), strict=True)
    return m


def test_the_models_calls_and_the_limited_normalisation(net, rows, run):
    eng = net._engine
    fs = net.sampling_rate
    assert fs == 44100
    tp = net.true_peak(run["dev"], run["n"])
    assert np.array_equal(bits(to_np(tp)), bits(run["tp"]))
    o, mg = net.limit(run["dev"].clone(), run["n"], run["c"], gains=run["g"])          # 1.5 ms, 20 ms: 66 and 882 samples
    assert np.array_equal(bits(np.nan_to_num(to_np(o))), bits(np.nan_to_num(run[66, 882]["inplace"])))
    # the burst row, half a second of it, and a quiet row that needs no limiting
    xs = [lr.voiced(22050, 11), (0.5 * lr.voiced(22050, 12, burst=False)).astype(np.float32)]
    audio, n = lr.pack(xs)
    dev = torch.from_numpy(audio).to(net.device)
    target, ceiling = -14.0, 0.9
    lim, gains = net.normalize_loudness(dev.clone(), n, target_lufs=target, peak_ceiling=ceiling, limiter=True)
    # ... is the composition of the three public calls
    seg, peak = eng.loudness_segments(dev, n, fs)
    _, _, g3 = eng.loudness_gate(seg, n, fs, peak=peak, params=eng.loudness_params(2, target, float("inf"), 30.0))
    want, _ = eng.limit(dev.clone(), n, ceiling, gains=g3, attack=66, hold=882)
    assert np.array_equal(bits(to_np(gains)), bits(to_np(g3)))
    assert np.array_equal(bits(np.nan_to_num(to_np(lim))), bits(np.nan_to_num(to_np(want))))
    assert np.abs(np.nan_to_num(to_np(lim))).max() <= np.float32(ceiling)
    # ... and lands nearer the target than the peak-cut normalisation of the same row
    cut, gains_cut = net.normalize_loudness(dev.clone(), n, target_lufs=target, peak_ceiling=ceiling)
    l_lim, _ = net.loudness(lim, n)
    l_cut, _ = net.loudness(cut, n)
    l_lim, l_cut = to_np(l_lim), to_np(l_cut)
    print(f"burst row: target {target} LUFS; with the limiter {l_lim[0]:.3f} LUFS (gain {to_np(gains)[0]:.3f}); "
          f"cut by the peak {l_cut[0]:.3f} LUFS (gain {to_np(gains_cut)[0]:.3f}); quiet row {l_lim[1]:.3f} / {l_cut[1]:.3f}")
    assert to_np(gains_cut)[0] < to_np(gains)[0]
    assert abs(l_lim[0] - target) < abs(l_cut[0] - target)
    with pytest.raises(ValueError):
        net.normalize_loudness(dev.clone(), n, limiter=dict(ceiling=0.5))


# ---------------------------------------------------------------------------------------------- the services
FRAMES, PHON, SEEDS = [33, 15, 5], [7, 5, 2], [411, 412, 413]
MODEL = 44100


def _collate(batch):
    return lambda rows: {k: batch[k][rows] for k in ("phonemes", "lengths", "sid", "duration", "f0", "energy")}


def _streamed(net, batch, kws):
    """The three requests join at ticks 0, 1 and 2; chunks of 8 frames; driven by step()."""
    from vispeech_amd.service import StreamingBatchService
    svc = StreamingBatchService(net, max_batch=3, chunk_frames=8, collate=_collate(batch), autostart=False)
    streams = []
    for b, kw in enumerate(kws):
        streams.append(svc.submit(b, SEEDS[b], **kw))
        svc.step()
    svc.close()
    return [b"".join(s) for s in streams]


def _batched(net, batch, kws):
    from vispeech_amd.service import BatchingSynthesisService
    svc = BatchingSynthesisService(net, max_batch=3, max_wait_s=30.0, collate=_collate(batch))
    try:
        return [f.result(120).tobytes() for f in [svc.submit(b, SEEDS[b], **kw) for b, kw in enumerate(kws)]]
    finally:
        svc.close()


def _row_bytes(eng, wave, fmt):
    from vispeech_amd import output_stage
    buf, spans = eng.output_batch(wave.reshape(1, -1), [wave.numel()], [fmt])
    return output_stage.unpack(to_np(buf), spans, [output_stage.encoding(fmt[1])])[0].tobytes()


def test_services_with_a_limiter_equal_the_direct_path(net):
    import isolated_ref as iso
    batch = iso.make_batch(FRAMES, PHON, seed=2170)
    eng, up = net._engine, net.dims.total_upsample
    f32 = dict(output_rate=MODEL, output_encoding="f32")
    dev = lambda raw: torch.from_numpy(np.frombuffer(raw, "<f4").copy()).to(net.device)
    # streaming: a limiter and a format; a neighbour that names nothing; a limiter alone
    plain = _streamed(net, batch, [{}, {}, {}])
    floats = [dev(b) for b in _streamed(net, batch, [f32] * 3)]
    assert [f.numel() for f in floats] == [n * up for n in FRAMES]
    c = [0.5 * float(f.abs().max()) for f in floats]
    assert min(c) > 1e-4
    g = 10.0 ** (3.0 / 20.0)
    lim = lambda b: dict(ceiling=c[b], gain_db=3.0)
    got = _streamed(net, batch, [dict(limiter=lim(0), output_rate=8000, output_encoding="ulaw"), {}, dict(limiter=lim(2))])

    def direct(b, fmt):
        y, mg = net.limit(floats[b].clone().reshape(1, -1), [floats[b].numel()], ceiling=c[b], gains=[g])
        assert float(mg[0]) < 0.6 and float(y.abs().max()) <= np.float32(c[b])
        return _row_bytes(eng, y[0], fmt)

    assert got[0] == direct(0, (8000, "ulaw")) and got[2] == direct(2, (MODEL, "s16"))
    assert got[1] == plain[1]                                # the neighbour: the bytes it always got
    assert got[2] != plain[2]
    # batching: a loudness and a limiter; a limiter alone; nothing
    b_plain = _batched(net, batch, [{}, {}, {}])
    b_floats = [dev(b) for b in _batched(net, batch, [f32] * 3)]
    cb = [0.5 * float(f.abs().max()) for f in b_floats]
    target = float(net.loudness(b_floats[0].reshape(1, -1), [b_floats[0].numel()])[0][0]) + 12.0      # 12 LU up: into the ceiling
    got = _batched(net, batch, [dict(loudness=dict(target_lufs=target, peak_ceiling=cb[0]), limiter=True, output_rate=8000, output_encoding="ulaw"),
                                dict(limiter=dict(ceiling=cb[1], gain_db=3.0)), {}])
    y, gains = net.normalize_loudness(b_floats[0].clone().reshape(1, -1), [b_floats[0].numel()], target_lufs=target, peak_ceiling=cb[0],
                                      limiter=True)
    assert abs(float(gains[0]) - 10.0 ** (12.0 / 20.0)) < 1e-3 and float(y.abs().max()) <= np.float32(cb[0])
    assert got[0] == _row_bytes(eng, y[0], (8000, "ulaw"))
    y, _ = net.limit(b_floats[1].clone().reshape(1, -1), [b_floats[1].numel()], ceiling=cb[1], gains=[g])
    assert got[1] == _row_bytes(eng, y[0], (MODEL, "s16")) and got[1] != b_plain[1]
    assert got[2] == b_plain[2]
    assert eng.status() == 0
