"""The prosody path finder, everything a CPU can check (no kernel is launched): the four entry points
exist and refuse what they must before a device is needed; the fp64 restatement (tests/prosody_path_ref.py) judged on its own
-- with both costs 0 it is the per-frame restatement, small tables against every path enumerated, one frame, no voiced
candidate --; the properties the GPU tests' inputs must have (tests/test_prosody_path_gpu.py rests on them); and the batching
service's calls with and without ``prosody_path``."""
import ctypes as C
import itertools

import numpy as np
import pytest

import prosody_path_ref as pr
import prosody_ref as ref
import test_abi
from prosody_ref import FS, HOP
from vispeech_amd import _lib
from vispeech_amd.schema import ModelDims

MARGIN = 1e-3                           # tests/test_prosody_gpu.py's: below it fp32 may rightly decide otherwise
NEW = ("vsp_prosody_path_workspace_bytes", "vsp_prosody_candidates", "vsp_prosody_path", "vsp_prosody_contours_path")


# ---------------------------------------------------------------------------------------------- symbols and ABI
def test_symbols_and_abi():
    lib = _lib.lib()
    for s in NEW:
        assert hasattr(lib, s) and s in _lib.SIGNATURES, s
    assert lib.vsp_abi_version() == 7
    assert sorted(_lib.SIGNATURES) == test_abi.header_symbols()
    assert _lib.PROSODY_MAX_CANDIDATES == 15 and C.sizeof(_lib.VspProsodyPathParams) == 12


# ---------------------------------------------------------------------------------------------- refusals
@pytest.fixture()
def ctx():
    lib = _lib.lib()
    cfg = _lib.make_config(ModelDims())
    h = C.c_void_p()
    assert lib.vsp_create(C.byref(cfg), 0, C.byref(h)) == 0
    yield lib, h
    lib.vsp_destroy(h)


BAD = C.c_void_p(8)                     # a pointer no kernel may ever see: every refusal is decided before a device is needed


def _contours_path(lib, h, n_samples, path=None, params=None):
    B = len(n_samples)
    p = None if params is None else C.byref(_lib.VspProsodyParams(*params))
    pp = None if path is None else C.byref(_lib.VspProsodyPathParams(*path))
    L = max(n_samples)
    return lib.vsp_prosody_contours_path(h, None, B, L, HOP, BAD, L, (C.c_int64 * B)(*n_samples), p, pp, BAD, BAD, BAD, BAD, 1 << 40)


def _candidates(lib, h, n_samples, max_candidates=15, params=None):
    B = len(n_samples)
    p = None if params is None else C.byref(_lib.VspProsodyParams(*params))
    L = max(n_samples)
    return lib.vsp_prosody_candidates(h, None, B, L, HOP, BAD, L, (C.c_int64 * B)(*n_samples), p, max_candidates, BAD, BAD, BAD,
                                      BAD, BAD, 1 << 40)


def _path(lib, h, frames, F_max, path=None, hop=HOP):
    B = len(frames)
    pp = None if path is None else C.byref(_lib.VspProsodyPathParams(*path))
    return lib.vsp_prosody_path(h, None, B, F_max, hop, BAD, BAD, (C.c_int64 * B)(*frames), pp, BAD, BAD, 1 << 40)


def test_refusals_before_a_device_is_needed(ctx):
    lib, h = ctx
    err = lambda: lib.vsp_last_error(h)
    # the path's own parameters, in all three calls
    for path, word in (((-0.01, 0.14, 15), b"cost"), ((0.35, -1.0, 15), b"cost"), ((float("nan"), 0.14, 15), b"cost"),
                       ((0.35, 0.14, 1), b"max_candidates"), ((0.35, 0.14, 16), b"max_candidates")):
        assert _contours_path(lib, h, [4096], path) == -1 and word in err() and b"vsp_prosody_contours_path" in err()
        assert _path(lib, h, [9], 9, path) == -1 and word in err() and b"vsp_prosody_path" in err()
        assert lib.vsp_prosody_path_workspace_bytes(1, 4096, HOP, None, C.byref(_lib.VspProsodyPathParams(*path))) == -1
    for n in (1, 16, 0, -3):
        assert _candidates(lib, h, [4096], n) == -1 and b"max_candidates" in err()
    # everything vsp_prosody_contours refuses, naming the row
    for call in (_contours_path, _candidates):
        assert call(lib, h, [4096, 640, 4096]) == -1 and b"row 1" in err()
        assert call(lib, h, [4096], params=(39.9, 750, 0.6, 0.03, 0.01)) == -1 and b"floor" in err()
        assert call(lib, h, [4096], params=(80, FS / 4 + 1, 0.6, 0.03, 0.01)) == -1 and b"ceiling" in err()
        assert call(lib, h, [4096], params=(80, 80, 0.6, 0.03, 0.01)) == -1
    # the path alone: a row of no frames, or of more than the table has
    assert _path(lib, h, [9, 0, 9], 9) == -1 and b"row 1" in err()
    assert _path(lib, h, [9, 9, 10], 9) == -1 and b"row 2" in err()
    assert _path(lib, h, [9], 9, hop=0) == -1
    # a workspace too small is a refusal of its own (-6), and the size covers all three calls
    need = lib.vsp_prosody_path_workspace_bytes(2, 44100, HOP, None, None)
    assert need > lib.vsp_prosody_workspace_bytes(2, 44100, HOP, 1, None) > 0
    assert need >= 2 * 87 * 16 * (4 + 4 + 1)                                  # the two tables and a byte per back-pointer
    assert lib.vsp_prosody_contours_path(h, None, 1, 4096, HOP, BAD, 4096, (C.c_int64 * 1)(4096), None, None, BAD, BAD, BAD, BAD,
                                         1024) == -6
    assert lib.vsp_prosody_path_workspace_bytes(1, 640, HOP, None, None) == -1
    assert lib.vsp_prosody_path_workspace_bytes(1, 4096, HOP, C.byref(_lib.VspProsodyParams(39.0, 750, 0.6, 0.03, 0.01)), None) == -1


def test_the_engine_validates_path_parameters_like_its_others():
    from vispeech_amd.engine import Engine
    P = Engine._prosody_path
    assert P(None) is None
    d = P(True)
    assert (round(d.octave_jump_cost, 6), round(d.voiced_unvoiced_cost, 6), d.max_candidates) == (0.35, 0.14, 15)
    assert P(dict(max_candidates=4)).max_candidates == 4 and round(P(dict(max_candidates=4)).octave_jump_cost, 6) == 0.35
    assert P((0.0, 0.0, 2)).max_candidates == 2
    for bad in (dict(octave=1.0), (0.35, 0.14), (-1.0, 0.14, 15), (0.35, 0.14, 16), (0.35, 0.14, 1), (0.35, 0.14, 2.5)):
        with pytest.raises(ValueError):
            P(bad)


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.fixture(scope="module")
def rows():
    return pr.main_rows()


def test_with_costs_zero_the_path_is_the_per_frame_decision(rows):
    for x in rows + [pr.octave_signal().astype(np.float32), pr.dip_signal().astype(np.float32)]:
        cand_f, cand_s, _, _ = pr.candidates(x)
        f0, choice = pr.best_path(cand_f, cand_s, octave_jump_cost=0.0, voiced_unvoiced_cost=0.0)
        np.testing.assert_array_equal(f0, ref.f0_frames(x))
        assert set(choice) <= {0, 1}                                           # the unvoiced candidate or the strongest


def test_candidate_tables_are_what_the_specification_says(rows):
    for x, n_max in zip(rows, (15, 4, 15, 15)):
        cand_f, cand_s, lags, _ = pr.candidates(x, max_candidates=n_max)
        assert cand_f.shape == cand_s.shape == (len(x) // HOP + 1, 16)
        assert not cand_f[:, 0].any() and np.isfinite(cand_s[:, 0]).all()      # slot 0: unvoiced, always there
        assert not cand_f[:, n_max:].any() and np.isneginf(cand_s[:, n_max:]).all()
        used = np.isfinite(cand_s[:, 1:])
        assert ((cand_f[:, 1:] > 0) == used).all() and ((lags[:, 1:] > 0) == used).all()
        s = np.where(used, cand_s[:, 1:], -np.inf)
        assert (s[:, 1:] <= s[:, :-1]).all()                                   # descending, the unused slots last
    cand_f, cand_s, _, _ = pr.candidates(rows[3])                              # silence: dead frames
    assert np.array_equal(cand_s[:, 0], [2.6, 2.6]) and np.isneginf(cand_s[:, 1:]).all()


def _small_table(rng, F, N, ties):
    cand_f = np.zeros((F, 16))
    cand_s = np.full((F, 16), -np.inf)
    if ties:
        cand_f[:, 1:N] = 2.0 ** rng.integers(7, 10, (F, N - 1))
        cand_s[:, :N] = rng.integers(0, 3, (F, N))
    else:
        cand_f[:, 1:N] = rng.uniform(80.0, 750.0, (F, N - 1))
        cand_s[:, :N] = rng.uniform(0.0, 1.5, (F, N))
    return cand_f, cand_s


@pytest.mark.parametrize("ties", (False, True))
def test_small_tables_against_every_path(ties):
    rng = np.random.default_rng(17)
    path = pr.TIE_PATH if ties else pr.PATH_DEFAULTS
    hop = pr.TIE_HOP if ties else HOP
    for F, N in itertools.product((1, 2, 3, 6), (2, 3, 4)):
        cand_f, cand_s = _small_table(rng, F, N, ties)
        best, first = pr.brute_force(cand_f[:, :N], cand_s[:, :N], hop, **path)
        f0, choice = pr.best_path(cand_f, cand_s, None, hop, **path)
        assert abs(pr.path_total(cand_f, cand_s, choice, hop, **path) - best) <= 1e-12 * max(1.0, abs(best)), (F, N)
        np.testing.assert_array_equal(f0, cand_f[np.arange(F), choice])
        # the margins: the best total minus the best total of a path that takes another candidate in frame k
        margin = pr.path_margins(cand_f, cand_s, None, hop, **path)
        for k in range(F):
            other = max(pr.path_total(cand_f, cand_s, c, hop, **path) for c in itertools.product(range(N), repeat=F)
                        if c[k] != choice[k])
            assert abs(margin[k] - (best - other)) <= 1e-12, (F, N, k)
        if not ties:
            assert tuple(choice) == first and margin.min() > 0


def test_tie_rules():
    """Two frames, everything equal: the lowest candidate at the end, the lowest previous candidate behind it."""
    cand_f = np.zeros((2, 16))
    cand_s = np.full((2, 16), -np.inf)
    cand_f[:, 1:4] = 256.0
    cand_s[:, :4] = 1.0
    f0, choice = pr.best_path(cand_f, cand_s, None, pr.TIE_HOP, **pr.TIE_PATH)
    assert list(choice) == [0, 0]                                              # unvoiced -> unvoiced costs nothing, slot 0 first
    cand_s[:, 0] = 0.0
    f0, choice = pr.best_path(cand_f, cand_s, None, pr.TIE_HOP, **pr.TIE_PATH)
    assert list(choice) == [1, 1] and list(f0) == [256.0, 256.0]


def test_one_frame_and_no_voiced_candidate():
    cand_f, cand_s = _small_table(np.random.default_rng(2), 1, 4, False)
    f0, choice = pr.best_path(cand_f, cand_s)
    assert choice[0] == np.argmax(cand_s[0]) and f0[0] == cand_f[0, choice[0]]
    cand_f, cand_s = _small_table(np.random.default_rng(3), 9, 4, False)
    cand_f[:] = 0.0                                                            # every candidate unvoiced: no cost anywhere
    f0, choice = pr.best_path(cand_f, cand_s)
    assert not f0.any() and list(choice) == list(np.argmax(cand_s, axis=1))
    f0, choice = pr.best_path(cand_f, cand_s, frames=4)                        # a ragged row: zeros behind its frames
    assert len(choice) == 4 and len(f0) == 9 and not f0[4:].any()


# ---------------------------------------------------------------------------------------------- the GPU tests' inputs
@pytest.mark.parametrize("n_used", (2, 15))
def test_the_random_tables_leave_out_at_most_one_frame_in_a_hundred(n_used):
    cand_f, cand_s = pr.random_tables(n_used)
    assert cand_f.dtype == np.float32 and cand_f.shape == (6, 130, 16)
    out = total = 0
    for b, F in enumerate(pr.TABLE_FRAMES):
        assert np.isnan(cand_f[b, F:]).all() and np.isnan(cand_s[b, F:]).all()
        assert np.isneginf(cand_s[b, :F, n_used:]).all() and np.isfinite(cand_s[b, :F, :n_used]).all()
        margin = pr.path_margins(cand_f[b], cand_s[b], F)
        f0, _ = pr.best_path(cand_f[b], cand_s[b], F)
        out, total = out + int((margin < MARGIN).sum()), total + F
        if F > 2:
            assert 0 < (f0[:F] > 0).sum() and len(np.unique(f0[:F])) > F // 4   # (a path that moves)
    print(f"random tables, {n_used} candidates: {out} of {total} frames below the margin")
    assert out <= 0.01 * total


def test_the_tie_tables_are_exact_and_full_of_ties():
    cand_f, cand_s = pr.tie_tables()
    ties = 0
    for b, F in enumerate(pr.TABLE_FRAMES):
        T = pr.transition(cand_f[b, 0], cand_f[b, 0], pr.TIE_HOP, **pr.TIE_PATH)
        assert set(np.unique(T)) <= {0.0, 0.5, 1.0}                              # kappa = 1: multiples of one half
        margin = pr.path_margins(cand_f[b], cand_s[b], F, pr.TIE_HOP, **pr.TIE_PATH)
        assert (margin == np.round(2 * margin) / 2).all()
        ties += int((margin == 0).sum())
    assert pr.kappa(pr.TIE_HOP) == 1.0 and ties >= 100


def test_the_octave_signal_misleads_the_per_frame_decision_and_not_the_path():
    x = pr.octave_signal().astype(np.float32)
    f0, margin = ref.f0_frames(x, with_margin=True)
    k = list(pr.OCTAVE_FRAMES)
    assert np.abs(f0[k] / (2 * pr.F_STEADY) - 1).max() < 1e-4 and margin[k].min() >= MARGIN        # an octave up, and sure of it
    steady = np.r_[4:12, 19:27]
    assert np.abs(f0[steady] / pr.F_STEADY - 1).max() < 1e-4
    cand_f, cand_s, _, _ = pr.candidates(x)
    p0, _ = pr.best_path(cand_f, cand_s)
    pm = pr.path_margins(cand_f, cand_s)
    assert np.abs(p0[k] / pr.F_STEADY - 1).max() < 1e-5 and pm[k].min() >= MARGIN
    assert pm.min() >= MARGIN and (np.abs(p0[2:-2] / pr.F_STEADY - 1) < 5e-3).all()                # no jump anywhere
    # a phoneme over exactly those frames: an octave (100 %) off without the path, the steady value with it
    dur = [k[0], len(k), len(f0) - k[-1] - 1]
    assert abs(ref.phoneme_means(ref.interpolate(p0), dur)[1] / pr.F_STEADY - 1) < 1e-5
    assert abs(ref.phoneme_means(ref.interpolate(f0), dur)[1] / pr.F_STEADY - 1) > 0.1


def test_the_dip_signal_flickers_per_frame_and_not_on_the_path():
    x = pr.dip_signal().astype(np.float32)
    f0, margin = ref.f0_frames(x, with_margin=True)
    unvoiced = np.nonzero(f0[2:-2] == 0)[0] + 2
    assert list(unvoiced) == list(pr.DIP_FRAMES) and margin[unvoiced].min() >= MARGIN
    cand_f, cand_s, _, _ = pr.candidates(x)
    p0, _ = pr.best_path(cand_f, cand_s)
    pm = pr.path_margins(cand_f, cand_s)
    assert (p0[2:-2] > 0).all() and pm.min() >= MARGIN
    assert np.abs(p0[2:-2] / pr.F_STEADY - 1).max() < 0.02                     # (the dip's frames are noisy, not an octave off)


def test_the_recordings_exercise_the_selection(rows):
    """Noise: every frame has more maxima than slots.  The other parameters of the GPU test (floor 60, four candidates)."""
    _, _, lags, gap = pr.candidates(rows[2])
    assert ((lags > 0).sum(1) == 14).all() and np.isfinite(gap).all()
    assert 0 < (gap >= MARGIN).sum() < len(gap)                               # frames compared as sets, and frames left out
    for x in rows[:2]:
        cand_f, cand_s, lags, gap = pr.candidates(x)
        assert (pr.path_margins(cand_f, cand_s) >= MARGIN).all()
    x = pr.glide_row(52 * HOP + 77).astype(np.float32)
    p = dict(floor=60.0, ceiling=500.0, voicing_threshold=0.5, silence_threshold=0.05, octave_cost=0.02)
    cand_f, cand_s, lags, gap, curvature = pr.candidates(x, max_candidates=4, with_curvature=True, **p)
    assert (lags > 0).sum(1).max() == 3
    # maxima too flat for fp32 to place to 1e-4 (tests/test_prosody_path_gpu.py, FLAT): a few, at the edges of the pause
    kept = (lags > 0) & (gap >= MARGIN)[:, None]
    flat = kept & (np.where(lags > 0, curvature, np.inf) * np.maximum(lags, 1) < 0.1)
    assert 0 < flat.sum() <= 0.05 * kept.sum()
    pm = pr.path_margins(cand_f, cand_s, octave_jump_cost=0.2, voiced_unvoiced_cost=0.3)
    assert (pm < MARGIN).sum() <= 0.02 * len(pm)


# ---------------------------------------------------------------------------------------------- the service's calls
from test_prosody_host import SVC_HOP, InferNet, ProsodyEngine  # noqa: E402


class PathEngine(ProsodyEngine):
    """The recording engine of tests/test_prosody_host.py with the ``path`` keyword: the call is recorded with it."""

    def prosody_contours(self, audio, n_samples, params=None, hop_length=None, path=None):
        out = super().prosody_contours(audio, n_samples, params, hop_length)
        if path is not None:
            self.calls[-1] = self.calls[-1] + ((round(path.octave_jump_cost, 6), round(path.voiced_unvoiced_cost, 6),
                                                path.max_candidates),)
        return out


def _serve(**kw):
    from vispeech_amd.service import BatchingSynthesisService
    from vispeech_amd.text import SymbolTable, request_row
    net = InferNet()
    net._engine = PathEngine()
    rec_a = np.arange(1, 3 * SVC_HOP + 1, dtype=np.float32)
    rec_b = 100.0 + np.arange(2 * SVC_HOP, dtype=np.float32)
    svc = BatchingSynthesisService(net, max_batch=3, max_wait_s=30.0, table=SymbolTable(["a", "b", "c"]), spk2id={"s": 0, "t": 1}, **kw)
    try:
        futs = [svc.submit(request_row("s", ["a", "b", "c"], durations=[1, 0, 2]), 7, prosody_audio=rec_a),
                svc.submit(request_row("t", ["a", "b"]), 8),
                svc.submit(request_row("s", ["c", "a"], durations=[2, 1]), 9, prosody_audio=rec_b)]
        for f in futs:
            assert f.result(60).shape == (3 * SVC_HOP,)
    finally:
        svc.close()
    return net


def test_service_calls_with_and_without_a_path():
    contour = ("prosody_contours", [3 * SVC_HOP, 2 * SVC_HOP])
    phoneme = ("prosody_phonemes", [4, 3], [[1, 0, 2], [2, 1, 0]], [3, 2])
    assert _serve()._engine.calls == [contour, phoneme]                        # the calls it always made
    assert _serve(prosody_path=None)._engine.calls == [contour, phoneme]
    assert _serve(prosody_path=True)._engine.calls == [contour + ((0.35, 0.14, 15),), phoneme]     # still ONE contour call
    net = _serve(prosody_path=dict(octave_jump_cost=0.2, max_candidates=6))
    assert net._engine.calls == [contour + ((0.2, 0.14, 6),), phoneme]
    assert len(net.infers) == 1


def test_service_refuses_bad_path_parameters_in_its_constructor():
    from vispeech_amd.service import BatchingSynthesisService
    from vispeech_amd.text import SymbolTable
    for bad in (dict(max_candidates=1), (-1.0, 0.14, 15), dict(nope=1)):
        with pytest.raises(ValueError):
            BatchingSynthesisService(InferNet(), table=SymbolTable(["a"]), spk2id={"s": 0}, prosody_path=bad)
