"""Loudness on the GPU against the fp64 restatement (tests/loudness_ref.py): the K-weighted segment
energies, the sample peak, the blocks and the integrated loudness of ragged batches at 44.1, 22.05 and 8 kHz (h = 4410, 2205
and 800: no multiple of 64) and at 192 kHz (h = 19200: 64 full lanes, the largest LDS image) with NaN behind every row; the
gate operator alone on constructed double tables with exact ties; gains and their two limits; apply in place and out of place; the ragged contract (a row alone gives the bits of its batch;
the fused call gives the bits of the three calls); and the batching service, bit for bit against the direct path.

The gate of a row (``gate_lu``) is NOT taken from the library: it is 4 times the distance of a float32 run of the
restatement's own sequential recurrence from its fp64 run (2.8e-4 LU on the rows with DC, a few 1e-6 elsewhere), at least
1e-5 LU and never above 0.1 LU (EBU Tech 3341's meter tolerance).  tests/test_loudness_host.py asserts that every block of
every row here stays a factor 1.05 clear of both gates, so no block is left out of any comparison."""
import math

import numpy as np
import pytest
import torch

import isolated_ref as iso
import loudness_ref as lr

pytestmark = pytest.mark.gpu

RATES = (44100, 22050, 8000, 192000)        # 192 kHz: h = 19200 = 64 runs of 300, no partial lane; 75 KiB of LDS a wave
NAN = float("nan")


def to_np(t):
    return t.detach().cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from vispeech_amd.engine import Engine
    from vispeech_amd.schema import ModelDims
    return Engine(ModelDims(), "cuda:0")                   # (the loudness calls need no weights)


@pytest.fixture(scope="module")
def measured(eng):
    """Per rate: the restatement's rows and the library's (seg, peak, lufs, blocks) of them as ONE ragged batch."""
    out = {}
    for fs in RATES:
        rows = lr.measured_rows(fs)
        audio, n = lr.pack([r["x"] for r in rows])
        dev = torch.from_numpy(audio).to(eng.device)
        seg, peak = eng.loudness_segments(dev, n, fs)
        lufs, blocks = eng.loudness_gate(seg, n, fs)
        out[fs] = dict(rows=rows, audio=audio, n=n, dev=dev, seg=to_np(seg), peak=to_np(peak), lufs=to_np(lufs), blocks=to_np(blocks))
    return out


# ---------------------------------------------------------------------------------------------- segments, peak, blocks, L
@pytest.mark.parametrize("fs", RATES)
def test_segments_peak_blocks_and_loudness(measured, fs):
    m = measured[fs]
    h = lr.segment_samples(fs)
    assert m["seg"].dtype == np.float64 and m["seg"].shape == (len(m["rows"]), lr.segments_count(max(m["n"]), fs))
    worst_seg = worst_lu = worst_ratio = 0.0
    for b, r in enumerate(m["rows"]):
        S = lr.segments_count(r["n"], fs)
        got, want = m["seg"][b, :S], r["seg"]
        assert not m["seg"][b, S:].any() and not np.signbit(m["seg"][b, S:]).any(), (r["name"], "zeros behind the row's segments")
        tol = 10.0 ** (r["gate_lu"] / 10.0) - 1.0
        err = np.where(want > 0, np.abs(got - want) / np.where(want > 0, want, 1.0), np.where(got == 0, 0.0, np.inf))
        worst_seg = max(worst_seg, float(err.max()))
        assert err.max() <= tol, (r["name"], "segment", int(err.argmax()), float(err.max()), tol)
        assert bits(m["peak"][b: b + 1])[0] == bits(np.array([r["peak"]], np.float32))[0], (r["name"], "peak")
        assert tuple(m["blocks"][b]) == (r["NB"], len(r["kept"])), (r["name"], tuple(m["blocks"][b]), r["NB"], len(r["kept"]))
        if r["L64"] == -math.inf:
            assert m["lufs"][b] == -np.inf, r["name"]
            continue
        d = abs(float(m["lufs"][b]) - r["L64"])
        worst_lu, worst_ratio = max(worst_lu, d), max(worst_ratio, d / r["gate_lu"])
        assert d <= r["gate_lu"] <= 0.1, (r["name"], d, r["gate_lu"])
    print(f"fs {fs} (h = {h}): worst segment error {worst_seg:.3g} relative, worst |L - L64| {worst_lu:.3g} LU "
          f"= {worst_ratio:.3g} of the row's gate; yardsticks {min(r['yardstick'] for r in m['rows']):.3g} .. "
          f"{max(r['yardstick'] for r in m['rows']):.3g} LU")


def test_silence_and_a_tone_below_the_absolute_gate(measured, eng):
    m = measured[44100]
    names = [r["name"] for r in m["rows"]]
    idx = [names.index("zeros"), names.index("tone 1e-4")]
    for b in idx:
        assert m["lufs"][b] == -np.inf and m["blocks"][b][1] == 0
    assert not m["seg"][idx[0]].any() and m["peak"][idx[0]] == 0.0
    rows = [m["rows"][b]["x"] for b in idx]
    audio, n = lr.pack(rows)
    _, gains, lufs, _, _ = eng.loudness_normalize(torch.from_numpy(audio).to(eng.device), n, 44100, eng.loudness_params(2, -16.0))
    assert to_np(gains).tolist() == [1.0, 1.0] and (to_np(lufs) == -np.inf).all()


# ---------------------------------------------------------------------------------------------- the gate operator alone
def test_gate_operator_on_constructed_tables(eng):
    fs = lr.TABLE_FS
    rows = lr.gate_tables()
    table, _ = lr.pack([r[0] for r in rows])
    table = table.astype(np.float64)
    for b, (seg, _) in enumerate(rows):                    # (lr.pack is float32: put the doubles back, NaN stays behind)
        table[b, : len(seg)] = seg
    n = [r[1] for r in rows]
    lufs, blocks = eng.loudness_gate(torch.from_numpy(table).to(eng.device), n, fs)
    lufs, blocks = to_np(lufs), to_np(blocks)
    worst = 0.0
    for b, (seg, nb) in enumerate(rows):
        L, NB, kept = lr.gate(seg, nb, fs)
        assert tuple(blocks[b]) == (NB, kept), (b, tuple(blocks[b]), NB, kept)
        if L == -np.inf:
            assert lufs[b] == -np.inf
        else:
            worst = max(worst, abs(float(lufs[b]) - float(L)))
            assert abs(float(lufs[b]) - float(L)) <= 1e-6, (b, lufs[b], L)
    print(f"gate operator: {len(rows)} tables, worst |L - restatement| {worst:.3g} LU")


# ---------------------------------------------------------------------------------------------- gains and apply
def gain_rows():
    """(samples, (target, ceiling, max_gain_db), what binds)."""
    x = lr.main_signal(44100, 22050)
    return [(x, (-16.0, 1.0, 30.0), None), (x[:17640], (-23.0, 1.0, 30.0), None), (x[:4410], (NAN, 1.0, 30.0), "alone"),
            (lr.tone(44100, 30000, 997.0, 0.25), (-6.0, 0.5, 30.0), "ceiling"), (lr.tone(44100, 26461, 997.0, 1e-3), (-23.0, 1.0, 20.0), "max_gain"),
            (lr.tone(44100, 20000, 1000.0, 1e-4), (-23.0, 1.0, 30.0), "silent")]


@pytest.fixture(scope="module")
def gained(eng):
    rows = gain_rows()
    audio, n = lr.pack([r[0] for r in rows])               # (an odd stride: rows that are not 16-byte aligned)
    B = len(rows)
    params = eng.loudness_params(B, *zip(*[r[1] for r in rows]))
    dev = torch.from_numpy(audio).to(eng.device)
    out, gains, lufs, peak, blocks = eng.loudness_normalize(dev, n, 44100, params)          # in place
    assert out is dev
    return dict(rows=rows, audio=audio, n=n, params=params, out=to_np(out), gains=to_np(gains), lufs=to_np(lufs), peak=to_np(peak),
                blocks=to_np(blocks))


def test_gains_follow_the_formula_on_the_devices_own_measurement(gained):
    g = gained
    for b, (x, (target, ceiling, max_db), binds) in enumerate(g["rows"]):
        want = lr.gain(float(g["lufs"][b]), float(g["peak"][b]), target, ceiling, max_db)
        assert abs(float(g["gains"][b]) - want) <= 1e-6 * want, (b, g["gains"][b], want)
        assert bits(g["peak"][b: b + 1])[0] == bits(np.array([np.abs(x).max()], np.float32))[0]
        if binds in ("alone", "silent"):
            assert g["gains"][b] == 1.0
        elif binds == "ceiling":
            assert abs(float(g["gains"][b]) * float(g["peak"][b]) - ceiling) <= 1e-6 and want < 10 ** ((target - float(g["lufs"][b])) / 20)
        elif binds == "max_gain":
            assert abs(float(g["gains"][b]) - 10.0) <= 1e-5 and 10 ** ((target - float(g["lufs"][b])) / 20) > 10.0
        else:
            assert abs(want - 10 ** ((target - float(g["lufs"][b])) / 20)) <= 1e-12 * want
    assert g["lufs"][5] == -np.inf and g["lufs"][4] < -60.0


def test_apply_in_place_is_the_float32_product_and_touches_nothing_else(gained):
    g = gained
    for b, (x, _, binds) in enumerate(g["rows"]):
        n = g["n"][b]
        want = np.float32(g["gains"][b]) * x
        assert np.array_equal(bits(g["out"][b, :n]), bits(want)), b
        assert np.array_equal(bits(g["out"][b, n:]), bits(g["audio"][b, n:])), (b, "behind the row")      # the NaN it held
    assert np.array_equal(bits(g["out"][2]), bits(g["audio"][2]))                                        # the NaN-target row


def test_apply_out_of_place_on_aligned_rows(gained, eng):
    g = gained
    B, L = g["audio"].shape
    stride = (L + 3) // 4 * 4 + 4
    src = torch.full((B, stride), NAN, dtype=torch.float32, device=eng.device)
    src[:, :L] = torch.from_numpy(g["audio"]).to(eng.device)
    dst = torch.full((B, stride), 7.0, dtype=torch.float32, device=eng.device)
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    out, gains, *_ = eng.loudness_normalize(src, g["n"], 44100, g["params"], out=dst)
    assert out is dst and np.array_equal(bits(to_np(gains)), bits(g["gains"]))
    out = to_np(out)
    for b in range(B):
        n = g["n"][b]
        if b == 2:
            assert (out[b] == 7.0).all()                                                                 # never written
            continue
        assert np.array_equal(bits(out[b, :n]), bits(g["out"][b, :n])), b
        assert (out[b, n:] == 7.0).all(), (b, "behind the row")
    assert np.array_equal(bits(to_np(src)[:, :L]), bits(g["audio"]))                                     # the source is read only


def test_measuring_the_result_again_gives_the_target(gained, eng):
    g = gained
    yard = {r["n"]: r["gate_lu"] for r in lr.measured_rows(44100)}
    lufs, _, _ = eng.loudness(torch.from_numpy(g["out"]).to(eng.device), g["n"], 44100)
    lufs = to_np(lufs)
    for b in (0, 1):
        target, gate = g["rows"][b][1][0], yard[g["n"][b]]
        print(f"row {b}: measured again {lufs[b]:.6f} LUFS, target {target}, gate {gate:.3g} LU")
        assert abs(float(lufs[b]) - target) <= gate


# ---------------------------------------------------------------------------------------------- the ragged contract
def test_every_row_alone_gives_the_bits_of_the_batch(measured, gained, eng):
    for fs in RATES:
        m = measured[fs]
        for b, r in enumerate(m["rows"]):
            x = np.concatenate([r["x"], np.full(3, NAN, np.float32)])[None, :]
            seg, peak = eng.loudness_segments(torch.from_numpy(x).to(eng.device), [r["n"]], fs)
            lufs, blocks = eng.loudness_gate(seg, [r["n"]], fs)
            S = seg.shape[1]
            assert np.array_equal(bits(to_np(seg)[0]), bits(m["seg"][b, :S])), (fs, r["name"])
            assert bits(to_np(lufs))[0] == bits(m["lufs"][b: b + 1])[0] and bits(to_np(peak))[0] == bits(m["peak"][b: b + 1])[0]
            assert tuple(to_np(blocks)[0]) == tuple(m["blocks"][b])
    g = gained
    for b, (x, spec, _) in enumerate(g["rows"]):
        dev = torch.from_numpy(np.concatenate([x, np.full(2, NAN, np.float32)])[None, :]).to(eng.device)
        out, gains, lufs, _, _ = eng.loudness_normalize(dev, [len(x)], 44100, eng.loudness_params(1, *spec))
        assert bits(to_np(gains))[0] == bits(g["gains"][b: b + 1])[0] and bits(to_np(lufs))[0] == bits(g["lufs"][b: b + 1])[0], b
        assert np.array_equal(bits(to_np(out)[0, : len(x)]), bits(g["out"][b, : len(x)])), b


def test_the_fused_call_gives_the_bits_of_the_three_calls(gained, eng):
    g = gained
    dev = torch.from_numpy(g["audio"]).to(eng.device)
    seg, peak = eng.loudness_segments(dev, g["n"], 44100)
    lufs, blocks, gains = eng.loudness_gate(seg, g["n"], 44100, peak=peak, params=g["params"])
    out = eng.loudness_apply(dev, g["n"], gains, params=g["params"])
    assert out is dev
    for a, b in ((lufs, g["lufs"]), (peak, g["peak"]), (gains, g["gains"]), (out, g["out"])):
        assert np.array_equal(bits(to_np(a)), bits(b))
    assert np.array_equal(to_np(blocks), g["blocks"])
    lufs2, blocks2 = eng.loudness_gate(seg, g["n"], 44100)                                               # without params: the same L
    assert np.array_equal(bits(to_np(lufs2)), bits(g["lufs"])) and np.array_equal(to_np(blocks2), g["blocks"])


# ---------------------------------------------------------------------------------------------- the model and the service
TEXT_FRAMES, TEXT_PHONEMES, TEXT_SEEDS = [60, 48], [9, 7], [501, 502]
N_REC, SRC, TGT, CONV_SEED = 4708, 5, 20, 601             # a recording of 9 frames


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


def test_the_models_two_calls(net, measured):
    m = measured[44100]
    lufs, peak = net.loudness(m["dev"], m["n"])
    assert np.array_equal(bits(to_np(lufs)), bits(m["lufs"])) and np.array_equal(bits(to_np(peak)), bits(m["peak"]))
    x = m["rows"][6]["x"]                                  # main[:22050]
    out, gains = net.normalize_loudness(torch.from_numpy(x[None, :].copy()).to(net.device), [len(x)], target_lufs=[-20.0])
    want = lr.gain(float(m["lufs"][6]), float(m["peak"][6]), -20.0, 1.0, 30.0)
    assert abs(float(to_np(gains)[0]) - want) <= 1e-6 * want
    assert np.array_equal(bits(to_np(out)[0]), bits(np.float32(to_np(gains)[0]) * x))


@pytest.fixture(scope="module")
def served(net):
    """One batch of three requests -- a text request (60 frames) at -16 LUFS delivered as mu-law at 8 kHz, a conversion at -16
    LUFS, a text request (48 frames) that names nothing -- through ``BatchingSynthesisService``; the same three through the
    service with nobody naming a loudness; and the direct path of the first two.  (60 and 48 frames: lengths that agree in
    what the frame-rate kernels' selection reads of a frame count, as tests/test_prosody_gpu.py explains.)"""
    from vispeech_amd.service import BatchingSynthesisService
    batch = iso.make_batch(TEXT_FRAMES, TEXT_PHONEMES, seed=2210)
    collate = lambda rows: {k: batch[k][rows] for k in ("phonemes", "lengths", "sid", "duration", "f0", "energy")}
    t = np.arange(N_REC) / 44100.0
    rec = (0.4 * np.sin(2 * np.pi * 220.0 * t) + 0.1 * np.random.default_rng(31).standard_normal(N_REC)).astype(np.float32).clip(-1, 1)
    eng, up = net._engine, net.dims.total_upsample
    dev = lambda a: torch.as_tensor(np.asarray(a)).to(net.device)

    def serve(loud):
        kw = {"loudness": -16} if loud else {}
        svc = BatchingSynthesisService(net, max_batch=3, max_wait_s=30.0, noise_scale=0.667, collate=collate)
        try:
            futs = [svc.submit(0, TEXT_SEEDS[0], output_rate=8000, output_encoding="ulaw", **kw),
                    svc.submit_conversion(rec, SRC, TGT, CONV_SEED, **kw), svc.submit(1, TEXT_SEEDS[1])]
            return [f.result(120) for f in futs]
        finally:
            svc.close()

    out = dict(loud=serve(True), plain=serve(False), up=up)
    # the direct path: the isolated infer of the text request alone, normalize_loudness, the output rows
    n0 = TEXT_PHONEMES[0]
    o, x_mask, *_ = net.infer(dev(batch["phonemes"][:1, :n0]), dev([n0]), sid=dev(batch["sid"][:1]), noise_scale=0.667,
                              duration_control=dev(batch["duration"][:1, :n0]), pitch_control=dev(batch["f0"][:1, :n0]),
                              energy_control=dev(batch["energy"][:1, :n0]), noise_seed=[TEXT_SEEDS[0]], isolated=True)
    n = int(x_mask[0].sum()) * up
    assert n == TEXT_FRAMES[0] * up
    out["text_before"] = to_np(o[0, 0, :n]).copy()
    wave, gains = net.normalize_loudness(o[:, 0, :], [n], target_lufs=-16.0)
    out["text_gain"] = float(to_np(gains)[0])
    out["text_wave"] = to_np(wave[0, :n]).copy()
    out["text_direct"] = _rows(eng, wave[:, :n], [n], [(8000, "ulaw")])[0]
    o_hat, y_mask, _ = net.convert_audio(rec[None, :], [N_REC], [SRC], [TGT], noise_seed=[CONV_SEED])
    n = int(y_mask[0].sum()) * up
    assert n == 9 * up
    wave, gains = net.normalize_loudness(o_hat[:, 0, :], [n], target_lufs=-16.0)
    out["conv_gain"] = float(to_np(gains)[0])
    out["conv_direct"] = _rows(eng, wave[:, :n], [n], [(44100, "s16")])[0]
    return out


def _rows(eng, x, n, formats):
    from vispeech_amd import output_stage
    buf, spans = eng.output_batch(x, n, formats)
    return [a.copy() for a in output_stage.unpack(to_np(buf), spans, [output_stage.encoding(e) for _, e in formats])]


def test_service_requests_equal_the_direct_path(served):
    s = served
    assert s["loud"][0].dtype == np.uint8 and s["loud"][1].dtype == np.dtype("<i2")
    assert s["text_gain"] != 1.0 and s["conv_gain"] != 1.0 and np.abs(s["text_before"]).max() > 1e-3
    assert np.array_equal(bits(s["text_wave"]), bits(np.float32(s["text_gain"]) * s["text_before"]))
    assert s["loud"][0].shape == s["text_direct"].shape and np.array_equal(s["loud"][0], s["text_direct"])
    assert s["loud"][1].shape == s["conv_direct"].shape == (9 * s["up"],) and np.array_equal(s["loud"][1], s["conv_direct"])
    assert not np.array_equal(s["loud"][0], s["plain"][0]) and not np.array_equal(s["loud"][1], s["plain"][1])


def test_service_request_that_names_nothing_gets_the_bytes_it_always_got(served):
    s = served
    assert s["loud"][2].dtype == np.dtype("<i2") and s["loud"][2].size == TEXT_FRAMES[1] * s["up"] and s["loud"][2].any()
    assert np.array_equal(s["loud"][2], s["plain"][2])
