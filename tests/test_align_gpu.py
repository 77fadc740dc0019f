"""Durations from a recording on the GPU against the fp64 restatement (tests/align_ref.py): the
score kernel within a bound derived from fp32 (no measured tolerance), the path kernel EXACTLY -- every frame of every row,
ties included, because it accumulates in fp64 what the restatement accumulates in fp64 on the same fp32 scores --, the
durations against numpy, then ``align_audio`` and the batching service on the test model.  The inputs' preconditions (the
planted path is the restatement's, the ties table has ties, the constructed rows are feasible) are asserted on the CPU in
tests/test_align_host.py.  What these tests cannot show is alignment QUALITY: the fixtures' weights are no trained voice."""
import os

import numpy as np
import pytest
import torch

import align_ref as ar

pytestmark = pytest.mark.gpu

HOP = 512


def to_np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def net():
    from vispeech_amd import config as vcfg
    from vispeech_amd.models import SynthesizerTrn
    from vispeech_amd.schema import ModelDims
    from vispeech_amd.synth import synth_state_dict
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    args, kwargs = vcfg.synthesizer_args(vcfg.default_hparams())
    m = SynthesizerTrn(*args, **kwargs).eval()
    m.load_state_dict(synth_state_dict(ModelDims(), seed=1234), strict=True)          # (with the enc_q.* tensors)
    return m


@pytest.fixture(scope="module")
def eng(net):
    return net._engine


# ---------------------------------------------------------------------------------------------- scores
@pytest.fixture(scope="module", params=[192, 7])
def scored(request, eng):
    """The ragged batch of 25 rows -- every (F, K) of {1, 63, 64, 65, 130}^2 -- with NaN behind every extent of all three
    inputs: the device's matrix and, computed once, the restatement's with the two sums of its error bound."""
    C = request.param
    rows = ar.score_rows(C, seed=100 + C)
    x, m, logs, F, K = ar.pack_inputs(rows, fill=np.nan)
    S = to_np(eng.align_scores(x, m, logs, F, K))
    want = [ar.scores(*r, with_sums=True) for r in rows]
    return C, rows, (x, m, logs, F, K), S, want


def test_scores_within_the_fp32_bound(scored):
    """|S_gpu - S_fp64| <= (C + 8) 2^-24 (sum_c |term_c| + sum_c |logs_c|): C roundings of the accumulation in any order,
    plus the exponential's, the difference's, the square's and the final subtraction's on every term."""
    C, rows, (_, _, _, F, K), S, want = scored
    worst = 0.0
    for b, (w, t, l) in enumerate(want):
        got = S[b, : F[b], : K[b]].astype(np.float64)
        assert np.isfinite(got).all()
        bound = (C + 8) * 2.0 ** -24 * (t + l[None, :])
        ratio = float((np.abs(got - w) / bound).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (b, F[b], K[b], ratio)
    print(f"C = {C}: the largest error is {worst:.3f} of the bound")


def test_scores_are_exact_zeros_outside_a_rows_extent(scored):
    _, _, (_, _, _, F, K), S, _ = scored
    assert S.shape == (25, 130, 130)
    for b in range(25):
        assert not S[b, F[b]:, :].view(np.uint32).any() and not S[b, :, K[b]:].view(np.uint32).any()


def test_every_row_alone_gives_the_scores_of_the_batch(scored, eng):
    _, rows, (_, _, _, F, K), S, _ = scored
    for b in range(len(rows)):
        x, m, logs, f, k = ar.pack_inputs(rows[b:b + 1], fill=np.nan)
        alone = to_np(eng.align_scores(x, m, logs, f, k))
        np.testing.assert_array_equal(alone[0].view(np.uint32), S[b, : F[b], : K[b]].view(np.uint32))


# ---------------------------------------------------------------------------------------------- path
def check_paths(eng, tables, params, fill=0.0):
    S, F, K = ar.pack(tables, fill=fill)
    got = to_np(eng.align_path(S, F, K, params))
    assert got.dtype == np.int32 and got.shape == (len(tables), max(F))
    for b, t in enumerate(tables):
        want = ar.best_path(t, *params)
        np.testing.assert_array_equal(got[b, : F[b]], want, err_msg=f"row {b} ({F[b]} x {K[b]})")      # every frame
        assert not got[b, F[b]:].any()
    return got


@pytest.mark.parametrize("costs", ar.COSTS)
def test_paths_on_constructed_tables(eng, costs):
    got = check_paths(eng, ar.random_tables(ar.PATH_ROWS_A2, seed=21), (2, *costs))
    np.testing.assert_array_equal(got[5, :63], 2 * np.arange(63))                                  # all skips
    got = check_paths(eng, ar.random_tables(ar.PATH_ROWS_A1, seed=22), (1, *costs))
    np.testing.assert_array_equal(got[0], np.arange(130))                                          # the diagonal
    assert not got[1].any()


def test_exact_ties_take_the_lowest_advance(eng):
    check_paths(eng, [ar.ties_table()], (2, 0.5, 1.0))
    check_paths(eng, [ar.ties_table(seed=6)], (1, 0.5, 1.0))


def test_a_row_that_crosses_every_ownership_boundary(eng):
    """K = 1025: one state more than 256 threads of four states hold, so the block is five waves and states pass from
    thread to thread and wave to wave; F = 545 = 17 back-pointer chunks of 32 frames and one frame (and 68 prefetch groups
    of 8 and one frame)."""
    tables = ar.random_tables([(545, 1025), (33, 5), (130, 257)], seed=23)
    check_paths(eng, tables, (2, 0.3, 0.7))
    check_paths(eng, tables[:1], (2, 0.0, 0.0))


def test_the_state_limit_runs_and_one_more_is_refused(eng):
    kmax = eng.align_max_states
    assert kmax >= 4096
    F = kmax // 2 + 1
    (t,) = ar.random_tables([(F, kmax)], seed=24)
    check_paths(eng, [t], (2, 0.3, 0.7))
    S = torch.zeros((1, F + 1, kmax + 1), device=eng.device)
    with pytest.raises(ValueError, match="row 0.*limit"):
        eng.align_path(S, [F + 1], [kmax + 1])


def test_nan_behind_every_extent_changes_no_path(eng):
    tables = ar.random_tables(ar.PATH_ROWS_A2, seed=21)
    check_paths(eng, tables, (2, 0.3, 0.7), fill=np.nan)


# ---------------------------------------------------------------------------------------------- planted path
def test_the_fused_call_returns_the_planted_path(eng):
    x, m, logs, k = ar.planted()
    cum = np.array([[0, 3, 3, 10, 25, 40, 40]], np.int32)                      # phonemes of no template frames at both ends
    states, dur = eng.align(x[None], m[None], logs[None], [55], [40], cum, [7])
    np.testing.assert_array_equal(to_np(states)[0], k)
    np.testing.assert_array_equal(to_np(dur)[0], ar.durations(k, cum[0], 7, 7))
    assert int(to_np(dur).sum()) == 55


# ---------------------------------------------------------------------------------------------- durations
def test_durations_against_numpy(eng):
    rng = np.random.default_rng(31)
    F, K = [70, 300, 1], [40, 200, 1]
    states = np.zeros((3, 300), np.int32)
    for b in range(3):
        adv = rng.integers(0, 3, F[b] - 1)
        states[b, : F[b]] = np.minimum(np.concatenate(([0], np.cumsum(adv))), K[b] - 1)
    Tp = 300
    cum = np.zeros((3, Tp), np.int32)
    cum[0, :8] = [0, 0, 5, 5, 5, 17, 40, 40]                                   # none at the start, in the middle, at the end
    cum[1, :290] = np.sort(rng.integers(0, 201, 290))
    cum[1, 289] = 200
    cum[2, :2] = [0, 1]
    lengths = [8, 290, 2]
    got = to_np(eng.align_durations(states, F, cum, lengths))
    assert got.shape == (3, Tp) and got.dtype == np.int32
    for b in range(3):
        np.testing.assert_array_equal(got[b], ar.durations(states[b, : F[b]], cum[b], lengths[b], Tp))
        assert int(got[b].sum()) == F[b] and not got[b, lengths[b]:].any()
    assert got[0, 0] == 0 and got[0, 3] == 0 and got[0, 7] == 0


# ---------------------------------------------------------------------------------------------- the model
@pytest.fixture(scope="module")
def filelist(golden_dir):
    g = np.load(os.path.join(golden_dir, "val_filelist.npz"))
    return {k: g[k] for k in ("in_phonemes", "in_lengths", "in_sid")}


def recording(n, seed):
    r = np.random.default_rng(seed)
    t = np.arange(n) / 44100.0
    f = 180.0 + 60.0 * np.sin(2.0 * np.pi * 0.9 * t + seed)
    x = 0.4 * np.sin(2.0 * np.pi * np.cumsum(f) / 44100.0) * (0.5 + 0.5 * np.sin(2.0 * np.pi * 1.7 * t) ** 2)
    return (x + 0.02 * r.standard_normal(n)).astype(np.float32)


N0, N1 = 11, 14                            # phonemes of the two texts


def text_batch(filelist, device):
    ph = np.zeros((2, N1), np.int64)
    ph[0, :N0], ph[1] = filelist["in_phonemes"][0, :N0], filelist["in_phonemes"][1, :N1]
    dev = lambda a: torch.as_tensor(np.asarray(a)).to(device)
    return dev(ph), dev([N0, N1]), dev(filelist["in_sid"][:2])


@pytest.mark.parametrize("fit_length", [True, False])
def test_align_audio_is_the_engine_calls_and_the_restatement(net, eng, filelist, fit_length):
    from vispeech_amd.models import RowControls
    ph, ln, sid = text_batch(filelist, net.device)
    n = [70 * HOP + 17, 52 * HOP]
    audio = np.zeros((2, max(n)), np.float32)
    for b in range(2):
        audio[b, : n[b]] = recording(n[b], 40 + b)
    dur = net.align_audio(ph, ln, sid, audio, n, fit_length=fit_length)
    assert dur.shape == (2, N1) and dur.dtype == torch.int64
    # the same calls, by hand
    frames = [eng.convert_frames(v) for v in n]
    enc = eng.encode(ph, ln, sid, isolated=True)
    states, tf = eng.frame_lengths_host(enc["frame_lengths"])
    kw = {}
    if fit_length:
        scale = [frames[b] / states[b] for b in range(2)]
        kw["row_controls"] = RowControls(scale, [1, 1], [1, 1], [0, 0], np.zeros((2, 3), bool))
        enc = eng.encode(ph, ln, sid, isolated=True, **kw)
        states, tf = eng.frame_lengths_host(enc["frame_lengths"])
        print(f"fit_length: recordings of {frames} frames, templates of {states} states")
    dec = eng.decode(enc, tf, None, 0.0, max_len=0, isolated=True, **kw)
    lat = eng.convert_latent(audio, n, sid, sid, noise_scale=0.0)
    assert lat["frames_host"] == frames and all(f <= v // HOP + 1 for f, v in zip(frames, n))
    path, d2 = eng.align(lat["z_p"], dec["m_p"], dec["logs_p"], frames, states, enc["cum_dur"], ln)
    assert torch.equal(dur, d2.to(torch.int64))
    # the fp64 path on the device's own fp32 scores for those tensors
    S = to_np(eng.align_scores(lat["z_p"], dec["m_p"], dec["logs_p"], frames, states))
    cum = to_np(enc["cum_dur"])
    for b in range(2):
        want = ar.best_path(S[b, : frames[b], : states[b]], 2)
        np.testing.assert_array_equal(to_np(path)[b, : frames[b]], want)
        np.testing.assert_array_equal(to_np(dur)[b], ar.durations(want, cum[b], int(ln[b]), N1))
        assert int(dur[b].sum()) == frames[b]
    # the result goes where durations go
    f0, en = net.prosody_from_audio(audio, n, dur, ln)
    o, x_mask, *_ = net.infer(ph, ln, sid=sid, noise_scale=0.667, noise_seed=[5, 6], isolated=True,
                              duration_control=dur.to(torch.float32), pitch_control=f0, energy_control=en)
    assert [int(x_mask[b].sum()) for b in range(2)] == frames and bool(torch.isfinite(o).all())


def test_a_recording_too_short_for_its_text_names_its_row(net, filelist):
    ph, ln, sid = text_batch(filelist, net.device)
    n = [70 * HOP, 6 * HOP]
    audio = np.zeros((2, max(n)), np.float32)
    for b in range(2):
        audio[b, : n[b]] = recording(n[b], 40 + b)
    with pytest.raises(ValueError, match="row 1"):
        net.align_audio(ph, ln, sid, audio, n, fit_length=False)
    with pytest.raises(ValueError, match="row 1"):
        net.align_audio(ph, ln, sid, audio, n, params=(1, 0.0, 0.0), fit_length=False)


# ---------------------------------------------------------------------------------------------- the service
def test_service_aligns_a_request_without_durations(net, filelist):
    """A ``prosody_audio`` request whose row brings no durations, on a service with ``prosody_align``: bit for bit the direct
    isolated ``infer`` with ``align_audio``'s durations and ``prosody_from_audio``'s tensors.  Without the keyword it raises."""
    from vispeech_amd.service import BatchingSynthesisService, pcm16
    from vispeech_amd.text import SymbolTable, request_row
    table = SymbolTable([str(i) for i in range(519)])
    spk = {str(i): i for i in range(67)}
    dev = lambda a: torch.as_tensor(np.asarray(a)).to(net.device)
    rec = recording(60 * HOP - 100, 44)
    ph, ln, sid = dev(filelist["in_phonemes"][0:1, :N0]), dev([N0]), dev(filelist["in_sid"][0:1])
    dur = net.align_audio(ph, ln, sid, rec[None, :], [len(rec)])
    f0, en = net.prosody_from_audio(rec[None, :], [len(rec)], dur, [N0])
    o, x_mask, *_ = net.infer(ph, ln, sid=sid, noise_scale=0.667, noise_seed=[41], isolated=True,
                              duration_control=dur.to(torch.float32), pitch_control=f0, energy_control=en)
    want = pcm16(o[0, 0, : int(x_mask[0].sum()) * net.dims.total_upsample])
    row = request_row(str(int(filelist["in_sid"][0])), [str(int(v)) for v in filelist["in_phonemes"][0, :N0]])
    svc = BatchingSynthesisService(net, max_batch=1, max_wait_s=30.0, noise_scale=0.667, table=table, spk2id=spk, prosody_align=True)
    try:
        got = svc.submit(row, 41, prosody_audio=rec).result(120)
    finally:
        svc.close()
    assert got.size == int(dur.sum()) * net.dims.total_upsample > 0
    np.testing.assert_array_equal(got, want)
    svc = BatchingSynthesisService(net, max_batch=1, max_wait_s=30.0, noise_scale=0.667, table=table, spk2id=spk)
    try:
        with pytest.raises(ValueError, match="durations"):
            svc.submit(row, 41, prosody_audio=rec)
    finally:
        svc.close()
