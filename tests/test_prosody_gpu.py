"""Prosody from a recording on the MI355X (``vsp_prosody_contours`` / ``vsp_prosody_phonemes``, ``Engine.prosody_*``,
``SynthesizerTrn.prosody_from_audio``, ``BatchingSynthesisService.submit(prosody_audio=...)``) against the fp64 restatement
of the specification (tests/prosody_ref.py, judged on its own by tests/test_prosody_host.py).

Gates: energy within 1e-5 of the row's largest frame energy (the project's stage gate); the set of voiced frames identical;
F0 within 1e-4 relative on them (the waveform gate; fp32 arithmetic noise measured at 4.2e-6).  A frame whose fp64 decision
margin -- the winning strength minus the next competitor's, the unvoiced strength included -- is below 1e-3 is left out of
the F0 comparison: there fp32 may rightly decide otherwise; at most 2 % of a case's frames may be left out.  Per-phoneme
means: the same two gates.  Raggedness, the input stage and the service are compared bit for bit.
Needs an MI355X: `pytest -m gpu`."""
import os

import numpy as np
import pytest
import torch

import prosody_ref as ref
from prosody_ref import FS, HOP

pytestmark = pytest.mark.gpu

ENERGY_TOL, F0_TOL, MARGIN, LEFT_OUT = 1e-5, 1e-4, 1e-3, 0.02
TONES = (90.0, 100.0, 220.5, 333.0, 441.0, 700.0)
LENGTHS = (61 * HOP, 61 * HOP - 1, 20 * HOP + 300, 641)     # tones, glide, noise, silence (the minimum: 2 frames)


def to_np(t):
    return t.detach().cpu().numpy()


def tones_row(n):
    """The six harmonic complexes spliced into one row."""
    cuts = np.linspace(0, n, len(TONES) + 1).astype(int)
    return np.concatenate([ref.harmonic(f, b - a) for f, a, b in zip(TONES, cuts[:-1], cuts[1:])])


def glide_row(n, seed=2):
    """180 + 60 sin(2 pi 1.5 t) Hz with 10 partials; hops 15-25 zeroed, hops 40-48 replaced by noise."""
    t = np.arange(n) / FS
    x = ref.harmonic(180.0 + 60.0 * np.sin(2.0 * np.pi * 1.5 * t), n, partials=10)
    x[15 * HOP: 26 * HOP] = 0.0
    x[40 * HOP: 49 * HOP] = np.random.default_rng(seed).standard_normal(9 * HOP) * 0.1
    return x


def main_rows():
    rng = np.random.default_rng(1)
    return [tones_row(LENGTHS[0]), glide_row(LENGTHS[1]), rng.standard_normal(LENGTHS[2]) * 0.1, np.zeros(LENGTHS[3])]


def pad(rows, fill=0.0):
    a = np.full((len(rows), max(len(r) for r in rows)), fill, np.float32)
    for b, r in enumerate(rows):
        a[b, : len(r)] = r
    return a


@pytest.fixture(scope="module")
def net():
    from vispeech_amd import config as vcfg
    from vispeech_amd.models import SynthesizerTrn
    from vispeech_amd.schema import dims_from_ctor
    from vispeech_amd.synth import synth_state_dict
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    ctor = vcfg.synthesizer_args(vcfg.default_hparams())
    m = SynthesizerTrn(*ctor[0], **ctor[1]).eval()
    m.load_state_dict(synth_state_dict(dims_from_ctor(*ctor[0], **ctor[1]), seed=1234, infer_only=True), strict=True)
    return m


@pytest.fixture(scope="module")
def eng(net):
    return net._engine


@pytest.fixture(scope="module")
def main():
    """The main batch: float32 rows (what the GPU gets) and the restatement of exactly those samples, computed once."""
    rows = [r.astype(np.float32) for r in main_rows()]
    want = [(*ref.f0_frames(r, with_margin=True), ref.energy_frames(r)) for r in rows]
    return rows, want


@pytest.fixture(scope="module")
def main_gpu(eng, main):
    rows, _ = main
    f0, en, frames, frames_host = eng.prosody_contours(pad(rows), [len(r) for r in rows])
    torch.cuda.synchronize()
    return to_np(f0), to_np(en), to_np(frames), frames_host


def check_contours(f0, en, want, tag):
    w_f0, margin, w_en = want
    F = len(w_f0)
    peak = w_en.max()
    err_e = np.abs(en[:F] - w_en).max() / peak if peak > 0 else np.abs(en[:F]).max()
    keep = margin >= MARGIN
    left_out = int((~keep).sum())
    voiced = w_f0 > 0
    same = np.array_equal((f0[:F] > 0)[keep], voiced[keep])
    k = keep & voiced & (f0[:F] > 0)
    err_f = np.abs(f0[:F][k] / w_f0[k] - 1.0).max() if k.any() else 0.0
    print(f"{tag}: frames {F}, voiced {int(voiced.sum())}, left out {left_out}, smallest margin {margin.min():.4g}, "
          f"energy err {err_e:.3g}, f0 err {err_f:.3g}")
    assert err_e <= ENERGY_TOL, (tag, err_e)
    assert left_out <= LEFT_OUT * F, (tag, left_out, F)
    assert same, (tag, np.nonzero((f0[:F] > 0) != voiced)[0])
    assert err_f <= F0_TOL, (tag, err_f)


# ---------------------------------------------------------------------------------------------- contours
def test_contours_against_the_restatement(main, main_gpu):
    rows, want = main
    f0, en, frames, frames_host = main_gpu
    assert list(frames) == frames_host == [len(r) // HOP + 1 for r in rows] == [62, 61, 21, 2]
    assert f0.shape == en.shape == (4, 62)
    assert (want[0][0] > 0).sum() >= 50 and 20 <= (want[1][0] > 0).sum() <= 45       # the inputs do what they are for
    assert not want[2][0].any() and not want[3][0].any()
    for b, tag in enumerate(("tones", "glide", "noise", "silence")):
        check_contours(f0[b], en[b], want[b], tag)


def test_outputs_behind_a_rows_frames_are_zero(main_gpu):
    f0, en, frames, _ = main_gpu
    for b, F in enumerate(frames):
        assert not f0[b, F:].any() and not en[b, F:].any()
    assert (en[0, : frames[0]] > 0).all() and (en[2, : frames[2]] > 0).all()         # (so that zeros behind are not by accident)


def test_nan_behind_every_rows_end_changes_no_bit(eng, main, main_gpu):
    rows, _ = main
    a = pad(rows, fill=np.nan)
    a = np.concatenate([a, np.full((4, 777), np.nan, np.float32)], axis=1)           # and a stride beyond L_max
    f0, en, frames, _ = eng.prosody_contours(a, [len(r) for r in rows])
    np.testing.assert_array_equal(to_np(f0).view(np.uint32), main_gpu[0].view(np.uint32))
    np.testing.assert_array_equal(to_np(en).view(np.uint32), main_gpu[1].view(np.uint32))
    np.testing.assert_array_equal(to_np(frames), main_gpu[2])


def test_every_row_alone_gives_the_bits_of_the_batch(eng, main, main_gpu):
    rows, _ = main
    for b, r in enumerate(rows):
        f0, en, frames, fh = eng.prosody_contours(r[None, :], [len(r)])
        F = fh[0]
        assert f0.shape == (1, F) and int(frames[0]) == F
        np.testing.assert_array_equal(to_np(f0)[0].view(np.uint32), main_gpu[0][b, :F].view(np.uint32))
        np.testing.assert_array_equal(to_np(en)[0].view(np.uint32), main_gpu[1][b, :F].view(np.uint32))


def test_other_parameters(eng):
    """Floor 60 Hz, ceiling 500 Hz: another window (2206 samples), another lag range and three lag blocks."""
    x = glide_row(52 * HOP + 77).astype(np.float32)
    p = dict(floor=60.0, ceiling=500.0, voicing_threshold=0.5, silence_threshold=0.05, octave_cost=0.02)
    want = (*ref.f0_frames(x, with_margin=True, **p), ref.energy_frames(x))
    f0, en, _, _ = eng.prosody_contours(x[None, :], [len(x)], params=dict(
        floor_hz=60.0, ceiling_hz=500.0, voicing_threshold=0.5, silence_threshold=0.05, octave_cost=0.02))
    check_contours(to_np(f0)[0], to_np(en)[0], want, "floor 60, ceiling 500")


def test_low_floors_in_a_row(eng):
    """Floor 50 Hz, then floor 40 Hz (the lowest accepted), in this order in one process: the block's LDS grows from 76 KiB to
    112 KiB -- both above the 64 KiB a kernel gets without asking, the second above the first -- and at floor 40 the five lag
    blocks no longer fit over the raw span, so the lag buffers lie behind the frame buffers."""
    n = 52 * HOP + 77
    x = ref.harmonic(70.0 + 12.0 * np.sin(2.0 * np.pi * 1.2 * np.arange(n) / FS), n, partials=12)     # a glide 58 ... 82 Hz
    x[14 * HOP: 22 * HOP] = 0.0
    x[38 * HOP: 45 * HOP] = np.random.default_rng(4).standard_normal(7 * HOP) * 0.1
    x = x.astype(np.float32)
    for floor, ceiling in ((50.0, 600.0), (40.0, 750.0)):
        want = (*ref.f0_frames(x, with_margin=True, floor=floor, ceiling=ceiling), ref.energy_frames(x))
        assert 25 <= (want[0] > 0).sum() <= 40                                       # (below the default floor of 80 Hz)
        f0, en, _, _ = eng.prosody_contours(x[None, :], [len(x)], params=dict(floor_hz=floor, ceiling_hz=ceiling))
        check_contours(to_np(f0)[0], to_np(en)[0], want, f"floor {floor:g}, ceiling {ceiling:g}")


# ---------------------------------------------------------------------------------------------- phonemes
@pytest.fixture(scope="module")
def filelist(golden_dir):
    g = np.load(os.path.join(golden_dir, "val_filelist.npz"))
    return {k: g[k] for k in ("in_phonemes", "in_lengths", "in_sid", "in_duration")}


def phoneme_rows(dur):
    """Synthetic recordings of exactly sum(d) frames for the two duration rows: voiced stretches, pauses and noise."""
    rows = []
    for b, d in enumerate(dur):
        n = (int(d.sum()) - 1) * HOP + 5 + 200 * b
        t = np.arange(n) / FS
        x = ref.harmonic(200.0 + 40.0 * b + 50.0 * np.sin(2.0 * np.pi * 0.7 * t), n, partials=6)
        for lo, hi in ((30, 55), (120, 131), (250, 262)):
            x[lo * HOP: hi * HOP] = 0.0
        x[180 * HOP: 200 * HOP] = np.random.default_rng(b).standard_normal(20 * HOP) * 0.05
        x *= 0.6 + 0.4 * np.sin(2.0 * np.pi * 0.3 * t) ** 2
        rows.append(x.astype(np.float32))
    return rows


def test_phoneme_means(net, filelist):
    dur = filelist["in_duration"].astype(np.int64)
    rows = phoneme_rows(dur)
    assert [len(r) // HOP + 1 for r in rows] == [310, 479]
    lengths = [31, 31]                       # row 0: its 11 phonemes and 20 of no frames
    f0, en = net.prosody_from_audio(pad(rows), [len(r) for r in rows], filelist["in_duration"], lengths)
    f0, en = to_np(f0), to_np(en)
    assert f0.shape == en.shape == (2, 31)
    for b, x in enumerate(rows):
        c, margin = ref.f0_frames(x, with_margin=True)
        e = ref.energy_frames(x)
        # a condition on the inputs: a mean cannot leave a frame out, so no frame may be one fp32 may decide otherwise
        assert (margin >= MARGIN).all() and 0 < (c > 0).sum() < len(c)
        w_f0, w_en = ref.phoneme_means(ref.interpolate(c), dur[b]), ref.phoneme_means(e, dur[b])
        live = dur[b] > 0
        err_f = np.abs(f0[b][live] / w_f0[live] - 1.0).max()
        err_e = np.abs(en[b] - w_en).max() / e.max()
        print(f"row {b}: f0 mean err {err_f:.3g}, energy mean err {err_e:.3g}")
        assert err_f <= F0_TOL and err_e <= ENERGY_TOL
        assert not f0[b][~live].any() and not en[b][~live].any()                     # exact 0 for a phoneme of no frames
    # behind lengths[b]: row 0 cut to its 11 phonemes gives the same 11 and exact zeros behind
    f0c, enc = net.prosody_from_audio(pad(rows), [len(r) for r in rows], filelist["in_duration"], [11, 31])
    np.testing.assert_array_equal(to_np(f0c)[0, :11].view(np.uint32), f0[0, :11].view(np.uint32))
    assert not to_np(f0c)[0, 11:].any() and not to_np(enc)[0, 11:].any()
    np.testing.assert_array_equal(to_np(f0c)[1].view(np.uint32), f0[1].view(np.uint32))


def test_interpolation_edges_on_the_gpu(eng):
    """No voiced frame, exactly one, voiced frames only at the ends: constructed contours through the phoneme call.
    Tolerance: fp32 against fp64 -- four roundings in an interpolated value, then a sequential sum of up to 30 terms (at
    most half an ulp of the running sum each) and a division: under 20 ulp = 1.2e-6; 2e-6."""
    F = 70                                                    # two chunks of the wave's scan
    c = np.zeros((4, F), np.float32)
    c[1, 66] = 210.0
    c[2, 0], c[2, F - 1] = 100.0, 169.0
    c[3, 5], c[3, 20], c[3, 64] = 120.0, 150.0, 90.0
    e = np.tile(np.arange(F, dtype=np.float32), (4, 1))
    d = np.tile(np.array([[1, 0, 9, 30, 30]], np.int64), (4, 1))
    f0, en = eng.prosody_phonemes(c, e, [F, F, F, 66], d, [5, 5, 5, 4])
    f0, en = to_np(f0), to_np(en)
    for b, (n, Tl) in enumerate(zip((F, F, F, 66), (5, 5, 5, 4))):
        w = ref.phoneme_means(ref.interpolate(c[b, :n].astype(np.float64)), d[b, :Tl])
        np.testing.assert_allclose(f0[b, :Tl], w, rtol=2e-6, atol=0)
        np.testing.assert_allclose(en[b, :Tl], ref.phoneme_means(e[b, :n], d[b, :Tl]), rtol=2e-6)
        assert not f0[b, Tl:].any() and not en[b, Tl:].any()


# ---------------------------------------------------------------------------------------------- the input stage
def test_raw_recordings_go_through_the_input_stage(net, eng):
    rate = 16000
    n_in = [16000, 9000]
    t = np.arange(max(n_in)) / rate
    x = 0.25 * sum(0.6 ** h * np.sin(2.0 * np.pi * 150.0 * h * t) for h in range(1, 6))
    raw = np.stack([np.rint(x * 32767.0).astype(np.int16), np.rint(x[::-1] * 20000.0).astype(np.int16)])
    dur = np.array([[20, 0, 30, 25], [10, 12, 0, 0]], np.int64)
    got = net.prosody_from_audio(raw, n_in, dur, [4, 2], sample_rate=rate, encoding="s16")
    audio, n_out = eng.input_batch(raw, n_in, rate, 1)
    assert n_out == [44100, 24807]
    want = net.prosody_from_audio(audio, n_out, dur, [4, 2])
    for g, w in zip(got, want):
        assert g.shape == (2, 4) and to_np(w).any()
        np.testing.assert_array_equal(to_np(g).view(np.uint32), to_np(w).view(np.uint32))


# ---------------------------------------------------------------------------------------------- the service
@pytest.fixture(scope="module")
def served(net, filelist):
    """One request with a recording (11 phonemes, 60 frames) and one plain request (14 phonemes, durations predicted: 48
    frames) through ``BatchingSynthesisService`` in one batch; the plain one again in a batch of its own; and the direct calls.

    The lengths are chosen on the library's stated guarantee ("shard-size independence", and 4e): runs of
    different shapes are bit-equal where both select the same frame-rate kernels -- ``launch_conv`` picks the channel-split /
    latency / throughput form from the size of the launch, and a split-k sum adds in another order -- and within the 1e-4
    waveform gate otherwise.  The decision tree (conv_mfma.hip, ``conv_form``) reads the frame count T through
    ceil(T / 32), ceil(T / 64), ceil(T / 128), T <= 96 and T >= 1024; 48 frames alone and 60 frames as a batch agree in
    all five.  That is a precondition on the inputs, not a proof: the tree also multiplies its block counts by the batch
    size, so a batch of two can still take another form than a run alone.  Whether it did is what the bit-for-bit
    assertions decide: the plain request, padded beside a longer one, is held to its alone run in every bit.  (Measured beside a
    request of 103 frames, which crosses T <= 96: the reverse flow's ``z`` differs by 4.8e-7, the waveform by 1.2e-7, 10 of
    24576 PCM16 samples by one step; encoder, predictors and the vocoder itself agree in every bit.)"""
    from vispeech_amd.models import RowControls
    from vispeech_amd.service import BatchingSynthesisService, pcm16
    from vispeech_amd.text import SymbolTable, request_row
    table = SymbolTable([str(i) for i in range(519)])
    spk = {str(i): i for i in range(67)}
    n0, n1 = 11, 14
    phones = lambda b, n: [str(int(v)) for v in filelist["in_phonemes"][b, :n]]
    dur = filelist["in_duration"][0, :n0].astype(np.int64).copy()
    dur[6], dur[9], dur[10] = 5, 4, 0                          # 60 frames, the last phoneme of none
    rec = glide_row(int(dur.sum()) * HOP - 100).astype(np.float32)
    up = net.dims.total_upsample
    dev = lambda a: torch.as_tensor(np.asarray(a)).to(net.device)
    cut = lambda o, x_mask, b: pcm16(o[b, 0, : int(x_mask[b].sum()) * up])

    def direct(b, n, seed, **ctl):
        o, x_mask, *_ = net.infer(dev(filelist["in_phonemes"][b:b + 1, :n]), dev([n]), sid=dev(filelist["in_sid"][b:b + 1]),
                                  noise_scale=0.667, noise_seed=[seed], isolated=True, **ctl)
        return cut(o, x_mask, 0)

    f0, en = net.prosody_from_audio(rec[None, :], [len(rec)], dur[None, :], [n0])
    out = dict(frames0=int(dur.sum()), up=up)
    assert out["frames0"] == 60
    out["direct0"] = direct(0, n0, 41, duration_control=dev(dur[None, :].astype(np.float32)), pitch_control=f0, energy_control=en)
    out["direct1"] = direct(1, n1, 42)
    # the batch the service builds, called directly: both rows, the table, the prosody tensors in row 0
    ph = np.zeros((2, n1), np.int64)
    ph[0, :n0], ph[1] = filelist["in_phonemes"][0, :n0], filelist["in_phonemes"][1, :n1]
    ctl = [torch.zeros((2, n1), dtype=torch.float32, device=net.device) for _ in range(3)]
    ctl[0][0, :n0], ctl[1][0, :n0], ctl[2][0, :n0] = dev(dur.astype(np.float32)), f0[0], en[0]
    rows = RowControls([1.0, 1.0], [1.0, 1.0], [1.0, 1.0], [0.667, 0.667], [[True] * 3, [False] * 3])
    o, x_mask, *_ = net.infer(dev(ph), dev([n0, n1]), sid=dev(filelist["in_sid"]), duration_control=ctl[0], pitch_control=ctl[1],
                              energy_control=ctl[2], noise_seed=[41, 42], isolated=True, row_controls=rows)
    out["direct_batch"] = [cut(o, x_mask, 0), cut(o, x_mask, 1)]

    def serve(reqs):
        svc = BatchingSynthesisService(net, max_batch=len(reqs), max_wait_s=30.0, noise_scale=0.667, table=table, spk2id=spk)
        try:
            return [f.result(120) for f in [svc.submit(r, s, **kw) for r, s, kw in reqs]]
        finally:
            svc.close()

    sid = lambda b: str(int(filelist["in_sid"][b]))
    with_rec = (request_row(sid(0), phones(0, n0), durations=dur), 41, dict(prosody_audio=rec))
    plain = (request_row(sid(1), phones(1, n1)), 42, {})
    out["together"] = serve([with_rec, plain])
    out["plain_alone"] = serve([plain])[0]
    return out


def test_service_prosody_request_is_the_direct_infer(served):
    """The request with a recording: bit for bit the direct isolated ``infer`` of that utterance alone with
    ``prosody_from_audio``'s tensors."""
    assert served["direct0"].shape == (served["frames0"] * served["up"],)
    np.testing.assert_array_equal(served["together"][0], served["direct0"])


def test_service_batch_is_the_direct_infer_of_its_rows(served):
    """Both requests: bit for bit the ONE direct isolated ``infer`` of the two rows with the table the service builds -- the
    service adds nothing to the model's call."""
    for b in range(2):
        assert served["together"][b].size > 0
        np.testing.assert_array_equal(served["together"][b], served["direct_batch"][b])


def conv_form_class(T):
    """What ``conv_form`` reads of a launch's FRAME COUNT.  (It also reads the batch size, through block counts: equal
    classes are a precondition this test puts on its inputs, not a guarantee that two runs select the same kernels.)"""
    return (-(-T // 32), -(-T // 64), -(-T // 128), T <= 96, T >= 1024)


def test_service_plain_request_beside_a_prosody_request(served):
    """The plain request beside the prosody request: bit for bit the direct isolated ``infer`` of it alone, and the bytes it
    gets in a batch of its own (``served``: at lengths where both runs select the same frame-rate kernels)."""
    frames1 = served["direct1"].size // served["up"]
    assert 0 < frames1 < served["frames0"], "the plain request is to be the shorter row of its batch"
    assert conv_form_class(frames1) == conv_form_class(served["frames0"]), (frames1, served["frames0"])
    np.testing.assert_array_equal(served["plain_alone"], served["direct1"])
    np.testing.assert_array_equal(served["together"][1], served["direct1"])
    np.testing.assert_array_equal(served["together"][1], served["plain_alone"])
