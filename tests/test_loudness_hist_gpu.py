"""Loudness range and the histogram gate on the device against tests/loudness_hist_ref.py.

The state is integer counts, so the comparisons are exact wherever the specification fixes the value: both histograms, ``kept``
and the range are compared EXACTLY (tests/test_loudness_hist_host.py shows that every audio fixture keeps 1e-6 from every bin
edge and gate, against 6.2e-9 between the device's segment energies and fp64); ``M`` and ``S`` have the bits of
``loudness_time``; ``I`` is within one float32 ulp of the restatement, because only the summation order is free; and any split
of a stream gives the bits of the one call, wherever the stream stands."""
import math

import numpy as np
import pytest
import torch

import loudness_hist_ref as hr
import loudness_ref as lr
import loudness_time_ref as ltr

pytestmark = pytest.mark.gpu

NAN = float("nan")
CUTS = ([1, 2, 63, 64, 65], [65, 64, 63, 2, 1], [64, 1, 65, 2, 63])        # segments a piece: 195 in all


def to_np(t):
    return t.detach().cpu().numpy()


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def within_one_ulp(got, ref):
    """float32 arrays: equal, or neighbours; -inf exactly where the reference has it."""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    return bool(((got == ref) | (got == np.nextafter(ref, np.float32(np.inf))) | (got == np.nextafter(ref, np.float32(-np.inf)))).all()
                and np.array_equal(np.isneginf(got), np.isneginf(ref)))


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from vispeech_amd.engine import Engine
    from vispeech_amd.schema import ModelDims
    return Engine(ModelDims(), "cuda:0")                   # (the loudness calls need no weights)


@pytest.fixture(scope="module")
def tables(eng):
    """The library's own tables: what the device bins against, and so what the restatement is given."""
    return eng.loudness_hist_tables()


def dev(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


# ---------------------------------------------------------------------------------------------- the tables
def test_tables(tables):
    e, c = tables
    assert e.shape == (1001,) and c.shape == (1000,)
    assert np.abs(e / hr.EDGES - 1.0).max() <= 4.5e-16 and np.abs(c / hr.CENTRES - 1.0).max() <= 4.5e-16
    assert abs(e[0] / lr.Z_ABS - 1.0) <= 4.5e-16
    assert (np.diff(e) > 0).all() and (np.diff(c) > 0).all()


# ---------------------------------------------------------------------------------------------- the operator alone
def packed(rows, width):
    t = np.full((len(rows), width), NAN)
    for b, seg in enumerate(rows):
        t[b, : len(seg)] = seg
    return t


@pytest.fixture(scope="module")
def constructed(eng, tables):
    """The constructed rows, the restatement of each (computed once), and the ONE call on all of them from zero histograms."""
    fs = lr.TABLE_FS
    h = lr.segment_samples(fs)
    assert hr.planted_ok(tables[0])                       # the plants sit on (and one double below) the library's own edges
    rows = hr.edge_rows(tables[0])
    assert [len(r) for r in rows] == [1, 3, 4, 29, 30, 31, 64, 65, 130]
    want = [hr.whole(seg, len(seg) * h, fs, tables) for seg in rows]
    t = dev(eng, packed(rows, 131))
    count = [len(r) for r in rows]
    hist = eng.loudness_hist_state(len(rows))
    got = eng.loudness_time_hist(t, 0, count, fs, hist)
    return dict(fs=fs, rows=rows, want=want, t=t, count=count, hist=to_np(hist), got=[to_np(v) for v in got])


def test_operator_on_constructed_tables(constructed, eng):
    c = constructed
    M, S, I, kept, m_max, s_max, lra = c["got"]
    Mx, Sx, _, _, mx, sx = (to_np(v) for v in eng.loudness_time(c["t"], 0, c["count"], c["fs"]))
    assert same(M, Mx) and same(S, Sx) and same(m_max, mx) and same(s_max, sx)          # the bits of the exact gate's call
    planted = 0
    for b, (seg, w) in enumerate(zip(c["rows"], c["want"])):
        F = len(seg)
        assert np.array_equal(c["hist"][b], w["hist"]), (F, "both histograms, exactly")
        assert np.array_equal(kept[b, :F], w["kept"]) and (kept[b, F:] == -1).all(), F
        assert within_one_ulp(I[b, :F], w["I"]), (F, I[b, :F], w["I"])
        assert np.isnan(I[b, F:]).all() and np.isneginf(I[b, : min(F, 3)]).all() and (kept[b, : min(F, 3)] == 0).all()
        assert lra[b] == w["lra"], (F, lra[b], w["lra"])
        planted += int(w["hist"][0, 999] > 0 and w["hist"][0, 0] > 0)
    assert planted == 3                                    # the rows with plants: counts in the first and in the last bin
    assert lra[-1] > 0.0 and (lra[:5] == 0.0).all()


def test_a_histogram_of_garbage_at_first_zero_is_taken_as_zero(constructed, eng):
    c = constructed
    hist = torch.full((len(c["rows"]), 2, hr.NB), 0x7FFFFFFF, dtype=torch.int32, device=eng.device)
    got = eng.loudness_time_hist(c["t"], 0, c["count"], c["fs"], hist)
    assert same(to_np(hist), c["hist"])
    for a, b in zip(got, c["got"]):
        assert same(to_np(a), b)


def test_a_call_for_some_entries_and_rows_given_apart(constructed, eng):
    """Rows as a stream keeps them (tensors of their own); count 0 leaves the histogram as it is and still gives the range."""
    c = constructed
    rows, fs = c["rows"], c["fs"]
    segs = [dev(eng, r) for r in rows]
    tabs = tuple([torch.full((len(r),), 7, dtype=dt, device=eng.device) for r in rows] for dt in (torch.float32,) * 3 + (torch.int32,))
    hist = [torch.zeros((2, hr.NB), dtype=torch.int32, device=eng.device) for _ in rows]
    first = [0, 0, 0, 0, 0, 0, 0, 0, 0]
    mid = [1, 2, 3, 20, 29, 30, 33, 64, 100]
    eng.loudness_time_hist(segs, first, mid, fs, hist, tables=tabs)
    rest = [len(r) - m for r, m in zip(rows, mid)]
    lra = to_np(eng.loudness_time_hist(segs, mid, rest, fs, hist, tables=tabs)[-1])
    M, S, I, kept, _, _, want_lra = c["got"]
    for b, r in enumerate(rows):
        for part, full in zip(tabs, (M, S, I, kept)):
            assert same(to_np(part[b]), full[b, : len(r)]), b
        assert same(to_np(hist[b]), c["hist"][b])
    assert same(lra, want_lra)
    again = to_np(eng.loudness_time_hist(segs, [len(r) for r in rows], 0, fs, hist, tables=tabs)[-1])
    assert same(again, want_lra) and all(same(to_np(hist[b]), c["hist"][b]) for b in range(len(rows)))


# ---------------------------------------------------------------------------------------------- audio
@pytest.mark.parametrize("fs", [44100, 8000])
def test_audio_rows_through_the_fused_call(eng, tables, fs):
    h = lr.segment_samples(fs)
    rows = ltr.measured_rows(fs)
    audio, n = lr.pack([r["x"] for r in rows])             # NaN behind every row
    d = dev(eng, audio)
    r = {k: to_np(v) for k, v in eng.loudness_range(d, n, fs).items()}
    exact = {k: to_np(v) for k, v in eng.loudness_level(d, n, fs).items()}
    assert same(to_np(d), audio)
    assert same(r["M"], exact["M"]) and same(r["S"], exact["S"])                         # M and S: the bits of section 4r
    worst = 0.0
    for b, row in enumerate(rows):
        F = row["n"] // h
        w = hr.whole(row["seg"], row["n"], fs, tables)
        assert np.array_equal(r["kept"][b, :F], w["kept"]) and (r["kept"][b, F:] == -1).all(), row["name"]
        assert within_one_ulp(r["I"][b, :F], w["I"]), row["name"]
        assert np.isnan(r["I"][b, F:]).all()
        assert r["lra"][b] == w["lra"], (row["name"], r["lra"][b], w["lra"])
        assert same(r["i_hist"][b: b + 1], r["I"][b, F - 1: F] if F else np.array([-np.inf], np.float32)), row["name"]
        both = np.isfinite(r["I"][b, 3:F]) & np.isfinite(exact["I"][b, 3:F])
        assert np.array_equal(np.isfinite(r["I"][b, 3:F]), np.isfinite(exact["I"][b, 3:F]))
        assert np.array_equal(r["kept"][b, 3:F], exact["kept"][b, 3:F]), row["name"]
        if both.any():
            worst = max(worst, float(np.abs(r["I"][b, 3:F][both].astype(np.float64) - exact["I"][b, 3:F][both]).max()))
    print(f"fs {fs}: max |I_h - I| on the device = {worst:.4f} LU (derived bound 0.05)")
    assert worst <= 0.05 + 1e-4
    # the operators give the fused call's bits, and the histograms the restatement's counts
    seg, _ = eng.loudness_segments(d, n, fs)
    F = [k // h for k in n]
    hist = eng.loudness_hist_state(len(rows))
    M, S, I, kept, _, _, lra = eng.loudness_time_hist(seg, 0, F, fs, hist)
    for k, t in (("M", M), ("S", S), ("I", I), ("kept", kept), ("lra", lra)):
        assert same(to_np(t), r[k]), k
    for b, row in enumerate(rows):
        assert np.array_equal(to_np(hist[b]), hr.whole(row["seg"], row["n"], fs, tables)["hist"]), row["name"]


def test_two_level_tone(eng, tables):
    fs = 8000
    x = hr.two_level(fs, 4.0, -20.0, -30.0)
    audio, n = lr.pack([x])
    r = eng.loudness_range(dev(eng, audio), n, fs)
    w = hr.measure(x, len(x), fs, tables)
    lra = float(r["lra"][0])
    print(f"two-level tone: LRA {lra!r} LU")
    assert abs(lra - 10.0) <= 0.1 + 1e-6 and lra == float(w["lra"])
    assert within_one_ulp(to_np(r["i_hist"]), np.array([w["i_hist"]]))


# ---------------------------------------------------------------------------------------------- any split, any position
def stream_table(F, seed):
    """A double table of F segments between -50 and -15 LUFS at TABLE_FS, loud and quiet stretches of a few seconds."""
    rng = np.random.default_rng(seed)
    slow = np.repeat(rng.uniform(-5.0, -2.3, size=F // 25 + 1), 25)[:F]
    return lr.segment_samples(lr.TABLE_FS) * np.power(10.0, slow + rng.uniform(-0.2, 0.2, size=F))


def in_rounds(eng, fs, segs, cuts):
    """Every stream advances by its next piece, all of them in ONE call per round, each at its own position."""
    F = [len(s) for s in segs]
    ds = [dev(eng, s) for s in segs]
    tabs = tuple([torch.full((f,), 7, dtype=dt, device=eng.device) for f in F] for dt in (torch.float32,) * 3 + (torch.int32,))
    hist = [torch.full((2, hr.NB), -5, dtype=torch.int32, device=eng.device) for _ in segs]       # (garbage: first == 0 clears it)
    pos = [0] * len(segs)
    todo = [list(c) for c in cuts]
    lra = [None] * len(segs)
    rounds = 0
    while any(p < f for p, f in zip(pos, F)):
        live = [i for i in range(len(segs)) if pos[i] < F[i]]
        cnt = [min(todo[i].pop(0) if todo[i] else F[i], F[i] - pos[i]) for i in live]
        out = eng.loudness_time_hist([ds[i] for i in live], [pos[i] for i in live], cnt, fs, [hist[i] for i in live],
                                     tables=tuple([t[i] for i in live] for t in tabs))[-1]
        for j, i in enumerate(live):
            pos[i] += cnt[j]
            lra[i] = out[j]
        rounds += 1
    return [[to_np(t[i]) for t in tabs] for i in range(len(segs))], [to_np(x) for x in hist], [float(v) for v in lra], rounds


def test_three_streams_at_their_own_positions_equal_the_one_call(eng):
    fs = lr.TABLE_FS
    segs = [stream_table(195, 1), stream_table(195, 2), stream_table(195, 3)]
    whole_t, whole_h, whole_lra, one = in_rounds(eng, fs, segs, [[195]] * 3)
    got_t, got_h, got_lra, rounds = in_rounds(eng, fs, segs, CUTS)
    assert one == 1 and rounds == 5
    for i in range(3):
        for a, b in zip(got_t[i], whole_t[i]):
            assert same(a, b), i
        assert same(got_h[i], whole_h[i]) and got_lra[i] == whole_lra[i] > 0.0, i


def test_a_far_position_in_pieces_of_seven_equals_the_one_call(eng, tables):
    """4096 segments: the entry at 4095 costs what the entry at 3 costs, and its bits do not depend on the split."""
    fs = lr.TABLE_FS
    seg = stream_table(4096, 4)
    whole_t, whole_h, whole_lra, _ = in_rounds(eng, fs, [seg], [[4096]])
    got_t, got_h, got_lra, rounds = in_rounds(eng, fs, [seg], [[7] * 586])
    assert rounds == 586
    for a, b in zip(got_t[0], whole_t[0]):
        assert same(a, b)
    assert same(got_h[0], whole_h[0]) and got_lra[0] == whole_lra[0]
    w = hr.whole(seg, 4096 * lr.segment_samples(fs), fs, tables)
    assert np.array_equal(whole_h[0], w["hist"]) and np.array_equal(whole_t[0][3], w["kept"]) and whole_lra[0] == float(w["lra"]) > 3.0
    assert within_one_ulp(whole_t[0][2], w["I"])


# ---------------------------------------------------------------------------------------------- streams and the leveller
def _split(n, cuts):
    edges = [0]
    for c in cuts:
        if edges[-1] >= n:
            break
        edges.append(min(n, edges[-1] + c))
    if edges[-1] < n:
        edges.append(n)
    return list(zip(edges[:-1], edges[1:]))


def test_the_leveller_under_the_histogram_gate(eng):
    from vispeech_amd import loudness
    fs = 8000
    h = lr.segment_samples(fs)
    x = ltr.step_row(fs)
    d = dev(eng, x)
    spec = dict(target_lufs=-16.0, slew_db_per_s=20.0, initial_gain_db=-2.0)
    runs = []
    for cuts in ([len(x)], [1, 7, h - 1, h, h + 1, 3 * h + 5] * 12):
        st = loudness.Stream(eng, fs, level=spec, gate="histogram")
        pieces = _split(len(x), cuts)
        outs = [st.push(d[a:b], final=(b == len(x))) for a, b in pieces]
        assert [o.numel() for o in outs] == [b - a for a, b in pieces]                    # every sample leaves in its own push
        runs.append((st, np.concatenate([to_np(o) for o in outs])))
    (a, out_a), (b, out_b) = runs
    F = len(x) // h
    assert a.segments == b.segments == F
    for k in ("M", "S", "I", "kept", "c_db", "c"):
        assert same(to_np(a.table[k]), to_np(b.table[k])), k
    assert same(out_a, out_b) and not same(out_a, x)                                      # levelled samples are split-invariant
    assert same(to_np(a.hist), to_np(b.hist)) and a.loudness_range == b.loudness_range > 0.0
    # the gain is the float32 restatement fed the device's own I_h, bit for bit
    want_db, _ = ltr.level_gains(to_np(a.table["I"]), **spec)
    assert same(to_np(a.table["c_db"]), want_db) and np.ptp(want_db) > 1.0
    assert same(out_a, ltr.level_apply(x, to_np(a.table["c"]), ltr.linear([spec["initial_gain_db"]])[0], fs))
    # and the tables are those of the fused call on the whole row
    r = eng.loudness_range(d[None, :].clone(), [len(x)], fs)
    assert same(to_np(r["I"])[0, :F], to_np(a.table["I"])) and float(r["lra"][0]) == a.loudness_range
    assert float(r["i_hist"][0]) == a.integrated


def test_both_gates_in_one_push_rows(eng):
    from vispeech_amd import loudness
    fs = 8000
    h = lr.segment_samples(fs)
    x = ltr.step_row(fs)
    d = dev(eng, x)
    spec = dict(target_lufs=-16.0, slew_db_per_s=20.0)
    alone = loudness.Stream(eng, fs, level=spec)
    exact, hist = loudness.Stream(eng, fs, level=spec), loudness.Stream(eng, fs, level=spec, gate="histogram")
    outs = [[], [], []]
    for lo, hi in _split(len(x), [3 * h + 5, 1, h - 1] * 40):
        last = hi == len(x)
        outs[0].append(alone.push(d[lo:hi], final=last))
        got = loudness.push_rows(eng, [(hist, d[lo:hi], last), (exact, d[lo:hi], last)])
        outs[1].append(got[1])
        outs[2].append(got[0])
    cat = lambda v: np.concatenate([to_np(o) for o in v])
    for k in ("M", "S", "I", "kept", "c_db", "c"):
        assert same(to_np(exact.table[k]), to_np(alone.table[k])), k                      # as without its histogram neighbour
    assert same(cat(outs[1]), cat(outs[0])) and not same(cat(outs[2]), cat(outs[0]))
    assert same(to_np(hist.table["M"]), to_np(exact.table["M"])) and same(to_np(hist.table["S"]), to_np(exact.table["S"]))
    assert exact.loudness_range is None and hist.loudness_range > 0.0
    F = len(x) // h
    assert np.abs(to_np(hist.table["I"])[3:F] - to_np(exact.table["I"])[3:F]).max() <= 0.05 + 1e-4


# ---------------------------------------------------------------------------------------------- the model and the service
TEXT_FRAMES, TEXT_PHONEMES, TEXT_SEED = [60, 48], [9, 7], 512
MODEL = 44100


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


def test_the_models_calls(net):
    eng = net._engine
    fs = 8000
    h = lr.segment_samples(fs)
    rows = [ltr.step_row(fs), hr.two_level(fs, 4.0, -20.0, -30.0)[: 37 * h + 5], lr.tone(fs, h - 1, 997.0, 0.25)]
    audio, n = lr.pack(rows)
    d = dev(eng, audio)
    r = eng.loudness_range(d, n, fs)
    lra, i_h = net.loudness_range(d, n, sample_rate=fs)
    assert same(to_np(lra), to_np(r["lra"])) and same(to_np(i_h), to_np(r["i_hist"])) and float(i_h[2]) == -math.inf and float(lra[2]) == 0.0
    M, S, I, m_max, s_max, i_end = net.loudness_profile(d, n, sample_rate=fs, gate="histogram")
    Mx, Sx, Ix, mx, sx, _ = net.loudness_profile(d, n, sample_rate=fs)
    for got, want in ((M, r["M"]), (S, r["S"]), (I, r["I"]), (i_end, r["i_hist"]), (M, Mx), (S, Sx), (m_max, mx), (s_max, sx)):
        assert same(to_np(got), to_np(want))
    assert not same(to_np(I), to_np(Ix))
    with pytest.raises(ValueError):
        net.loudness_profile(d, n, sample_rate=fs, gate="hist")


def _streamed(net, batch, kw, **svc_kw):
    from vispeech_amd.service import StreamingBatchService
    collate = lambda rows: {k: batch[k][rows] for k in ("phonemes", "lengths", "sid", "duration", "f0", "energy")}
    svc = StreamingBatchService(net, max_batch=3, chunk_frames=8, collate=collate, autostart=False, **svc_kw)
    stream = svc.submit(1, TEXT_SEED, **kw)                # the smaller utterance: 48 frames
    svc.close()
    return stream, b"".join(stream)


def test_streaming_service_with_the_histogram_gate(net):
    import isolated_ref as iso
    from vispeech_amd import loudness
    batch = iso.make_batch(TEXT_FRAMES, TEXT_PHONEMES, seed=2230)
    _, plain = _streamed(net, batch, {})
    stream, got = _streamed(net, batch, dict(loudness=True), loudness_gate="histogram")
    assert got == plain and len(got) == 2 * 48 * net.dims.total_upsample                  # a meter: the bytes of a request without it
    _, raw = _streamed(net, batch, dict(output_rate=MODEL, output_encoding="f32"))
    wave = torch.from_numpy(np.frombuffer(raw, "<f4").copy()).to(net.device)
    st = loudness.Stream(net._engine, MODEL, gate="histogram")
    st.push(wave, final=True)
    info = stream.loudness
    assert info["range_lu"] == st.loudness_range and info["integrated"] == st.integrated and math.isfinite(info["integrated"])
    assert info["gain_db"] is None and info["momentary_max"] == st.momentary_max
    exact, _ = _streamed(net, batch, dict(loudness=True))
    assert "range_lu" not in exact.loudness and exact.loudness["momentary_max"] == info["momentary_max"]
