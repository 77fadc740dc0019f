"""The prosody path finder on the MI355X (``vsp_prosody_candidates`` / ``vsp_prosody_path`` / ``vsp_prosody_contours_path``,
``Engine.prosody_candidates`` / ``prosody_path`` / ``prosody_contours(path=)``, ``SynthesizerTrn.prosody_from_audio(path=)``,
``BatchingSynthesisService(prosody_path=)``) against the fp64 restatement of the specification (tests/prosody_path_ref.py,
judged on its own by tests/test_prosody_path_host.py, which also asserts what these inputs must be).

Gates: a frame whose fp64 max-marginal -- the best total through its chosen candidate minus the best through any other -- is
below 1e-3 (tests/test_prosody_gpu.py's MARGIN) is left out: there fp32 may rightly choose otherwise; at most 1 % of a
constructed table's frames and 2 % of a recording's may be.  On every other frame the F0 of a table is the table's f bit
for bit, and that of a recording within 1e-4 relative with the same voiced frames.  Candidates: f within 1e-4 relative, strengths
within 1e-5, the same lags wherever the last strength kept and the first left out differ by 1e-3 or more.  Tie rules, zero
costs, raggedness and the service are compared bit for bit.

Measured (MI355X): no frame left out anywhere -- the smallest margin kept is 1.4e-3 on the random tables,
3.5e-3 on the recordings --; candidates f 1.6e-5, strengths 1.8e-6 (8.6e-6 at floor 60), U 9.5e-8; path F0 5.0e-6; the phoneme
over the octave frames 2.1e-7 from the steady value with the path, an octave off without.
Needs an MI355X: `pytest -m gpu`."""
import os

import numpy as np
import pytest
import torch

import prosody_path_ref as pr
import prosody_ref as ref
from prosody_ref import HOP

pytestmark = pytest.mark.gpu

F0_TOL, STRENGTH_TOL, MARGIN, LEFT_OUT_TABLE, LEFT_OUT = 1e-4, 1e-5, 1e-3, 0.01, 0.02


def to_np(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


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


# ---------------------------------------------------------------------------------------------- 1. the path alone
def check_tables(eng, cand_f, cand_s, tag, hop=HOP, exact=False, **path):
    """The path through constructed tables against ``best_path``: bit for bit on every frame kept (``exact``: on every frame)."""
    frames = list(pr.TABLE_FRAMES)
    f0 = eng.prosody_path(cand_f, cand_s, frames, path=path or True, hop_length=hop)
    torch.cuda.synchronize()
    f0 = to_np(f0)
    assert f0.shape == cand_f.shape[:2]
    out = total = 0
    smallest = np.inf
    for b, F in enumerate(frames):
        want, _ = pr.best_path(cand_f[b], cand_s[b], F, hop, **path)
        margin = pr.path_margins(cand_f[b], cand_s[b], F, hop, **path)
        keep = np.ones(F, bool) if exact else margin >= MARGIN
        out, total = out + int((~keep).sum()), total + F
        smallest = min(smallest, margin[keep].min())
        np.testing.assert_array_equal(bits(f0[b, :F][keep]), bits(want[:F][keep]), err_msg=f"{tag}: row {b} ({F} frames)")
        assert not f0[b, F:].any(), (tag, b)                                   # exact zeros behind the row (its table there is NaN)
    print(f"{tag}: {total} frames, left out {out}, smallest margin kept {smallest:.4g}")
    assert out <= LEFT_OUT_TABLE * total, (tag, out, total)


@pytest.mark.parametrize("n_used", (2, 15))
def test_path_on_random_tables(eng, n_used):
    cand_f, cand_s = pr.random_tables(n_used)
    check_tables(eng, cand_f, cand_s, f"random, {n_used} candidates")


def test_path_tie_rules_bit_for_bit(eng):
    """Integers and powers of two at kappa = 1: every score is exact in fp32, so every tie is one on the device too, and the
    lowest previous candidate / the lowest last candidate must come out, frame for frame."""
    cand_f, cand_s = pr.tie_tables()
    check_tables(eng, cand_f, cand_s, "ties", hop=pr.TIE_HOP, exact=True, **pr.TIE_PATH)


def test_path_with_fewer_candidates_allowed_reads_the_table_as_it_is(eng):
    """``max_candidates`` bounds what the candidate kernel emits; the path operator takes any table."""
    cand_f, cand_s = pr.random_tables(15)
    a = eng.prosody_path(cand_f, cand_s, list(pr.TABLE_FRAMES), path=dict(max_candidates=2))
    b = eng.prosody_path(cand_f, cand_s, list(pr.TABLE_FRAMES), path=True)
    np.testing.assert_array_equal(bits(to_np(a)), bits(to_np(b)))


# ---------------------------------------------------------------------------------------------- 2. candidates
@pytest.fixture(scope="module")
def main():
    rows = pr.main_rows()
    return rows, [pr.candidates(r) for r in rows]


@pytest.fixture(scope="module")
def main_candidates(eng, main):
    rows, _ = main
    cand_f, cand_s, en, frames, frames_host = eng.prosody_candidates(pr.pad(rows), [len(r) for r in rows])
    torch.cuda.synchronize()
    return to_np(cand_f), to_np(cand_s), to_np(en), to_np(frames), frames_host


# A maximum's refined lag is t + 0.5 (rm - rp) / (rm - 2 r0 + rp): an error eps in r moves it by about eps / curvature, and f
# by that over t.  r(t) is a sum of W (1654 .. 2206) fp32 products, normalised to r(0) = 1 and scaled by r_w(0) / r_w(t) <= 2.5:
# eps is about 2.5 sqrt(W) 2^-24 = 7e-6, at most 1e-5.  So f can be held to 1e-4 only where curvature * t >= 1e-5 / 1e-4 = 0.1; a
# flatter maximum (they sit at the edges of silence, where r is nearly constant) is compared in its strength and its being
# there, not in its f.  The four main rows are compared without this allowance.
FLAT = 0.1


def check_candidates(cand_f, cand_s, want, tag, n_max=15, flat=None):
    w_f, w_s, lags, gap = want[:4]
    F = len(w_f)
    err_f = err_s = err_u = 0.0
    compared = n_flat = 0
    for k in range(F):
        assert cand_f[k, 0] == 0.0 and not cand_f[k, n_max:].any() and np.isneginf(cand_s[k, n_max:]).all(), (tag, k)
        err_u = max(err_u, abs(cand_s[k, 0] - w_s[k, 0]))
        used = np.isfinite(cand_s[k, 1:])
        assert ((cand_f[k, 1:] > 0) == used).all(), (tag, k)
        s = cand_s[k, 1:][used]
        assert (s[1:] <= s[:-1]).all() and not used[len(s):].any(), (tag, k)   # descending, the unused slots last
        if gap[k] < MARGIN:
            continue                                                           # fp32 may rightly keep the other maximum
        n = int((lags[k] > 0).sum())
        assert len(s) == n, (tag, k, len(s), n)
        if n == 0:
            continue
        # the same lags: maxima lie two lags or more apart, 3.6e-3 of f at the longest lag -- sorted by f they pair off
        i, j = np.argsort(cand_f[k, 1: 1 + n]), np.argsort(w_f[k, 1: 1 + n])
        sharp = np.ones(n, bool) if flat is None else (want[4][k, 1: 1 + n] * lags[k, 1: 1 + n])[j] >= flat
        n_flat += int((~sharp).sum())
        # (a flat maximum still pairs off: its f may move by the lag's own spacing at most, or it would be another maximum)
        err_f = max(err_f, np.abs(cand_f[k, 1: 1 + n][i] / w_f[k, 1: 1 + n][j] - 1.0)[sharp].max(initial=0.0))
        err_s = max(err_s, np.abs(cand_s[k, 1: 1 + n][i] - w_s[k, 1: 1 + n][j]).max())
        compared += 1
    print(f"{tag}: frames {F}, compared as sets {compared}, f err {err_f:.3g}, strength err {err_s:.3g}, U err {err_u:.3g}, "
          f"flat maxima not compared in f {n_flat}")
    assert err_u <= STRENGTH_TOL, (tag, err_u)
    assert err_f <= F0_TOL and err_s <= STRENGTH_TOL, (tag, err_f, err_s)


def test_candidates_against_the_restatement(main, main_candidates):
    rows, want = main
    cand_f, cand_s, en, frames, frames_host = main_candidates
    assert list(frames) == frames_host == [62, 61, 21, 2] and cand_f.shape == cand_s.shape == (4, 62, 16)
    for b, tag in enumerate(("tones", "glide", "noise", "silence")):
        F = frames_host[b]
        check_candidates(cand_f[b, :F], cand_s[b, :F], want[b], tag)
        assert not cand_f[b, F:].any() and not cand_s[b, F:].any()            # exact zeros behind a row's frames
        e = ref.energy_frames(rows[b])
        assert np.abs(en[b, :F] - e).max() <= 1e-5 * max(e.max(), 1e-30) and not en[b, F:].any()
    # a dead frame has the unvoiced candidate alone, at voicing_threshold + 2
    assert (cand_s[3, :2, 0] == np.float32(2.6)).all() and np.isneginf(cand_s[3, :2, 1:]).all()


# ---------------------------------------------------------------------------------------------- 3. zero costs
def test_zero_costs_give_the_bits_of_the_per_frame_call(eng, main):
    rows, _ = main
    rows = rows + [pr.octave_signal().astype(np.float32), pr.dip_signal().astype(np.float32)]
    a, n = pr.pad(rows), [len(r) for r in rows]
    f0, en, frames, _ = eng.prosody_contours(a, n)
    z0, zen, zframes, _ = eng.prosody_contours(a, n, path=(0.0, 0.0, 15))
    p0, pen, _, _ = eng.prosody_contours(a, n, path=True)
    f0, z0, p0 = to_np(f0), to_np(z0), to_np(p0)
    assert (f0 > 0).sum() > 100
    np.testing.assert_array_equal(bits(z0), bits(f0))
    np.testing.assert_array_equal(to_np(zframes), to_np(frames))
    for e in (zen, pen):                                                       # the energy: the same bits with any costs
        np.testing.assert_array_equal(bits(to_np(e)), bits(to_np(en)))
    assert not np.array_equal(p0, f0)                                          # (and the costs do something)


# ---------------------------------------------------------------------------------------------- 4. where the decisions differ
def check_path_contour(f0, x, tag, n_max=15, params=None, **path):
    """A recording's path F0 against the path restatement of the same samples."""
    cand_f, cand_s, _, _ = pr.candidates(x, max_candidates=n_max, **(params or {}))
    want, _ = pr.best_path(cand_f, cand_s, **path)
    margin = pr.path_margins(cand_f, cand_s, **path)
    F = len(want)
    keep = margin >= MARGIN
    left_out = int((~keep).sum())
    voiced = want > 0
    k = keep & voiced & (f0[:F] > 0)
    err_f = np.abs(f0[:F][k] / want[k] - 1.0).max() if k.any() else 0.0
    print(f"{tag}: frames {F}, voiced {int(voiced.sum())}, left out {left_out}, smallest margin {margin.min():.4g}, f0 err {err_f:.3g}")
    assert left_out <= LEFT_OUT * F, (tag, left_out, F)
    assert np.array_equal((f0[:F] > 0)[keep], voiced[keep]), (tag, np.nonzero((f0[:F] > 0) != voiced)[0])
    assert err_f <= F0_TOL, (tag, err_f)
    return want


def test_the_path_neither_jumps_an_octave_nor_flickers(net, eng):
    octave, dip = pr.octave_signal().astype(np.float32), pr.dip_signal().astype(np.float32)
    rows = [octave, dip]
    a, n = pr.pad(rows), [len(r) for r in rows]
    per_frame = to_np(eng.prosody_contours(a, n)[0])
    path = to_np(eng.prosody_contours(a, n, path=True)[0])
    for b, (x, tag) in enumerate(zip(rows, ("octave signal", "dip signal"))):
        check_path_contour(path[b], x, tag)
    ko, kd = list(pr.OCTAVE_FRAMES), list(pr.DIP_FRAMES)
    assert np.abs(per_frame[0, ko] / (2 * pr.F_STEADY) - 1).max() < 1e-4       # each frame for itself: an octave up ...
    assert np.abs(path[0, ko] / pr.F_STEADY - 1).max() < 1e-4                  # ... the path: where its neighbours are
    assert not per_frame[1, kd].any() and (path[1, kd] > 0).all()              # a weak frame dropped / kept
    # a phoneme over exactly the octave signal's frames
    dur = np.array([[ko[0], len(ko), 31 - ko[-1] - 1]], np.int64)
    with_path, _ = net.prosody_from_audio(octave[None, :], [len(octave)], dur, [3], path=True)
    without, _ = net.prosody_from_audio(octave[None, :], [len(octave)], dur, [3])
    steady = pr.F_STEADY                                                       # (a period of 200 samples: the parabola adds nothing)
    err_with, err_without = abs(float(with_path[0, 1]) / steady - 1), abs(float(without[0, 1]) / steady - 1)
    print(f"phoneme over the octave frames: {err_with:.3g} off with the path, {err_without:.3g} without")
    assert err_with <= 1e-4 and err_without > 0.1


# ---------------------------------------------------------------------------------------------- 5. the ragged contract
@pytest.fixture(scope="module")
def main_path(eng, main):
    rows, _ = main
    f0, en, frames, frames_host = eng.prosody_contours(pr.pad(rows), [len(r) for r in rows], path=True)
    torch.cuda.synchronize()
    return to_np(f0), to_np(en), to_np(frames), frames_host


def test_path_contours_against_the_restatement(main, main_path):
    rows, _ = main
    f0, en, frames, frames_host = main_path
    assert list(frames) == frames_host == [62, 61, 21, 2] and f0.shape == en.shape == (4, 62)
    for b, tag in enumerate(("tones", "glide", "noise", "silence")):
        check_path_contour(f0[b], rows[b], tag)
        assert not f0[b, frames_host[b]:].any() and not en[b, frames_host[b]:].any()     # zeros behind a row's frames
    assert (f0[0] > 0).sum() >= 50 and not f0[2].any() and not f0[3].any()


def test_nan_behind_every_rows_end_changes_no_bit(eng, main, main_path, main_candidates):
    rows, _ = main
    a = np.concatenate([pr.pad(rows, fill=np.nan), np.full((4, 777), np.nan, np.float32)], axis=1)     # and a stride beyond L_max
    n = [len(r) for r in rows]
    f0, en, frames, _ = eng.prosody_contours(a, n, path=True)
    np.testing.assert_array_equal(bits(to_np(f0)), bits(main_path[0]))
    np.testing.assert_array_equal(bits(to_np(en)), bits(main_path[1]))
    np.testing.assert_array_equal(to_np(frames), main_path[2])
    cand_f, cand_s, en, _, _ = eng.prosody_candidates(a, n)
    np.testing.assert_array_equal(bits(to_np(cand_f)), bits(main_candidates[0]))
    np.testing.assert_array_equal(bits(to_np(cand_s)), bits(main_candidates[1]))
    np.testing.assert_array_equal(bits(to_np(en)), bits(main_candidates[2]))


def test_every_row_alone_gives_the_bits_of_the_batch(eng, main, main_path, main_candidates):
    rows, _ = main
    for b, r in enumerate(rows):
        f0, en, frames, fh = eng.prosody_contours(r[None, :], [len(r)], path=True)
        F = fh[0]
        assert f0.shape == (1, F) and int(frames[0]) == F
        np.testing.assert_array_equal(bits(to_np(f0)[0]), bits(main_path[0][b, :F]))
        np.testing.assert_array_equal(bits(to_np(en)[0]), bits(main_path[1][b, :F]))
        cand_f, cand_s, _, _, _ = eng.prosody_candidates(r[None, :], [len(r)])
        np.testing.assert_array_equal(bits(to_np(cand_f)[0]), bits(main_candidates[0][b, :F]))
        np.testing.assert_array_equal(bits(to_np(cand_s)[0]), bits(main_candidates[1][b, :F]))
        # the path alone on the batch's tables is the fused call
        p0 = eng.prosody_path(main_candidates[0][b: b + 1, :F], main_candidates[1][b: b + 1, :F], [F])
        np.testing.assert_array_equal(bits(to_np(p0)[0]), bits(main_path[0][b, :F]))


def test_other_parameters(eng):
    """Floor 60 Hz, ceiling 500 Hz (another window, three lag blocks), four candidates, other costs."""
    x = pr.glide_row(52 * HOP + 77).astype(np.float32)
    p = dict(floor=60.0, ceiling=500.0, voicing_threshold=0.5, silence_threshold=0.05, octave_cost=0.02)
    lib_p = dict(floor_hz=60.0, ceiling_hz=500.0, voicing_threshold=0.5, silence_threshold=0.05, octave_cost=0.02)
    cand_f, cand_s, _, _, _ = eng.prosody_candidates(x[None, :], [len(x)], params=lib_p, max_candidates=4)
    check_candidates(to_np(cand_f)[0], to_np(cand_s)[0], pr.candidates(x, max_candidates=4, with_curvature=True, **p),
                     "floor 60, 4 candidates", n_max=4, flat=FLAT)
    f0, _, _, _ = eng.prosody_contours(x[None, :], [len(x)], params=lib_p, path=(0.2, 0.3, 4))
    check_path_contour(to_np(f0)[0], x, "floor 60, 4 candidates, costs 0.2 / 0.3", n_max=4, params=p, octave_jump_cost=0.2,
                       voiced_unvoiced_cost=0.3)


# ---------------------------------------------------------------------------------------------- 6. the service
def test_service_with_a_path_is_the_direct_infer(net, golden_dir):
    """A ``prosody_audio`` request through ``BatchingSynthesisService(prosody_path=True)``: bit for bit the direct isolated
    ``infer`` with ``prosody_from_audio(..., path=True)``'s tensors -- and not that of the tensors without the path."""
    from vispeech_amd.service import BatchingSynthesisService, pcm16
    from vispeech_amd.text import SymbolTable, request_row
    g = np.load(os.path.join(golden_dir, "val_filelist.npz"))
    n0 = 5
    ko = list(pr.OCTAVE_FRAMES)
    dur = np.array([ko[0] - 6, 6, len(ko), 5, 31 - ko[-1] - 6], np.int64)      # 31 frames, the third phoneme on the octave frames
    rec = pr.octave_signal().astype(np.float32)
    assert int(dur.sum()) == len(rec) // HOP + 1 == 31
    dev = lambda a: torch.as_tensor(np.asarray(a)).to(net.device)
    up = net.dims.total_upsample

    def direct(**kw):
        f0, en = net.prosody_from_audio(rec[None, :], [len(rec)], dur[None, :], [n0], **kw)
        o, x_mask, *_ = net.infer(dev(g["in_phonemes"][0:1, :n0]), dev([n0]), sid=dev(g["in_sid"][0:1]), noise_scale=0.667,
                                  noise_seed=[41], isolated=True, duration_control=dev(dur[None, :].astype(np.float32)),
                                  pitch_control=f0, energy_control=en)
        return pcm16(o[0, 0, : int(x_mask[0].sum()) * up])

    table = SymbolTable([str(i) for i in range(519)])
    svc = BatchingSynthesisService(net, max_batch=1, max_wait_s=30.0, noise_scale=0.667, table=table,
                                   spk2id={str(i): i for i in range(67)}, prosody_path=True)
    try:
        row = request_row(str(int(g["in_sid"][0])), [str(int(v)) for v in g["in_phonemes"][0, :n0]], durations=dur)
        got = svc.submit(row, 41, prosody_audio=rec).result(120)
    finally:
        svc.close()
    want = direct(path=True)
    assert want.shape == (31 * up,)
    np.testing.assert_array_equal(got, want)
    assert not np.array_equal(got, direct())
