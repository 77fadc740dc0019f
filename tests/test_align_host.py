"""Durations from a recording, everything a CPU can check (no kernel is launched): the eight entry
points exist and refuse what they must before a device is needed, naming the row; the workspace sizes are monotone; the fp64
restatement (tests/align_ref.py) judged on its own -- every path of every small table enumerated, feasibility exactly
K <= A (F - 1) + 1, the tie rule on tables worked by hand --; the properties the GPU tests' inputs must have
(tests/test_align_gpu.py rests on them); and the batching service's calls with and without ``prosody_align``."""
import ctypes as C
import itertools

import numpy as np
import pytest

import align_ref as ar
import test_abi
from vispeech_amd import _lib
from vispeech_amd.schema import ModelDims

NEW = ("vsp_align_max_states", "vsp_align_scores_workspace_bytes", "vsp_align_scores", "vsp_align_path_workspace_bytes",
       "vsp_align_path", "vsp_align_durations", "vsp_align_workspace_bytes", "vsp_align")


# ---------------------------------------------------------------------------------------------- symbols and ABI
def test_symbols_and_abi():
    lib = _lib.lib()
    for s in NEW:
        assert hasattr(lib, s) and s in _lib.SIGNATURES, s
    assert lib.vsp_abi_version() == 7
    assert sorted(_lib.SIGNATURES) == test_abi.header_symbols()
    assert C.sizeof(_lib.VspAlignParams) == 12
    assert lib.vsp_align_max_states() >= 4096


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
BIG = 1 << 40


def _i64(v):
    return (C.c_int64 * len(v))(*v)


def _params(p):
    return None if p is None else C.byref(_lib.VspAlignParams(*p))


def _scores(lib, h, frames, states, F_max, K_max, Cc=4):
    return lib.vsp_align_scores(h, None, len(frames), Cc, F_max, K_max, BAD, BAD, BAD, _i64(frames), _i64(states), BAD, BAD, BIG)


def _path(lib, h, frames, states, F_max, K_max, params=None):
    return lib.vsp_align_path(h, None, len(frames), F_max, K_max, BAD, _i64(frames), _i64(states), _params(params), BAD, BAD, BIG)


def _align(lib, h, frames, states, F_max, K_max, cum, lengths, params=None):
    B, Tp = len(frames), len(cum[0])
    flat = (C.c_int32 * (B * Tp))(*[v for row in cum for v in row])
    return lib.vsp_align(h, None, B, 4, F_max, K_max, Tp, BAD, BAD, BAD, _i64(frames), _i64(states), flat, _i64(lengths),
                         _params(params), BAD, BAD, BAD, BIG)


def _durations(lib, h, frames, F_max, cum, lengths):
    B, Tp = len(frames), len(cum[0])
    flat = (C.c_int32 * (B * Tp))(*[v for row in cum for v in row])
    return lib.vsp_align_durations(h, None, B, F_max, Tp, BAD, _i64(frames), flat, _i64(lengths), BAD, BAD, BIG)


def test_refusals_before_a_device_is_needed(ctx):
    lib, h = ctx
    err = lambda: lib.vsp_last_error(h)
    kmax = lib.vsp_align_max_states()
    cum3 = [[3, 5, 9], [3, 5, 9], [3, 5, 9]]
    # the parameters, in both calls that take them
    for p, word in (((0, 0.0, 0.0), b"max_advance"), ((3, 0.0, 0.0), b"max_advance"), ((2, -0.1, 0.0), b"cost"),
                    ((1, 0.0, -1.0), b"cost"), ((2, float("nan"), 0.0), b"cost")):
        assert _path(lib, h, [9], [9], 9, 9, p) == -1 and word in err() and b"vsp_align_path" in err()
        assert _align(lib, h, [9], [9], 9, 9, [[3, 5, 9]], [3], p) == -1 and word in err()
    # an infeasible row, naming it: K <= A (F - 1) + 1 exactly
    assert _path(lib, h, [9, 5, 9], [9, 10, 9], 9, 10) == -1 and b"row 1" in err() and b"infeasible" in err()
    assert _path(lib, h, [9, 9, 5], [9, 9, 6], 9, 9, (1, 0.0, 0.0)) == -1 and b"row 2" in err() and b"infeasible" in err()
    assert _align(lib, h, [9, 9, 4], [9, 9, 9], 9, 9, cum3, [3, 3, 3]) == -1 and b"row 2" in err() and b"infeasible" in err()
    # the state limit
    assert _path(lib, h, [5000, 5000], [9, kmax + 1], 5000, kmax + 1) == -1 and b"row 1" in err() and b"limit" in err()
    # a row of no frames, of more frames or states than the tables have, of no states
    for call in (lambda f, k: _path(lib, h, f, k, 9, 9), lambda f, k: _scores(lib, h, f, k, 9, 9),
                 lambda f, k: _align(lib, h, f, k, 9, 9, cum3, [3, 3, 3])):
        assert call([9, 0, 9], [9, 9, 9]) == -1 and b"row 1" in err() and b"frames" in err()
        assert call([9, 9, 10], [9, 9, 9]) == -1 and b"row 2" in err()
        assert call([9, 9, 9], [0, 9, 9]) == -1 and b"row 0" in err() and b"states" in err()
        assert call([9, 9, 9], [9, 10, 9]) == -1 and b"row 1" in err()
    # cum_dur must end at the row's states
    assert _align(lib, h, [9, 9], [9, 9], 9, 9, [[3, 5, 9], [3, 5, 8]], [3, 3]) == -1 and b"row 1" in err() and b"cum_dur" in err()
    assert _align(lib, h, [9, 9], [9, 9], 9, 9, [[3, 5, 9], [5, 3, 9]], [3, 3]) == -1 and b"row 1" in err() and b"decreases" in err()
    assert _durations(lib, h, [9, 0], 9, [[3, 5, 9], [3, 5, 9]], [3, 3]) == -1 and b"row 1" in err()
    assert _durations(lib, h, [9, 9], 9, [[3, 5, 9], [3, 5, 9]], [3, 4]) == -1 and b"row 1" in err()
    assert _durations(lib, h, [9, 9], 9, [[3, 5, 9], [3, 5, 9]], [3, 0]) == -1 and b"row 1" in err() and b"phonemes" in err()
    # a workspace too small is a refusal of its own (-6)
    assert lib.vsp_align_path(h, None, 1, 9, 9, BAD, _i64([9]), _i64([9]), None, BAD, BAD, 16) == -6
    assert lib.vsp_align_scores(h, None, 1, 4, 9, 9, BAD, BAD, BAD, _i64([9]), _i64([9]), BAD, BAD, 16) == -6


def test_null_pointers_are_refused_after_the_rows(ctx):
    lib, h = ctx
    assert lib.vsp_align_path(h, None, 1, 9, 9, None, _i64([9]), _i64([9]), None, BAD, BAD, BIG) == -1
    assert lib.vsp_align_scores(h, None, 1, 4, 9, 9, BAD, None, BAD, _i64([9]), _i64([9]), BAD, BAD, BIG) == -1


def test_workspace_sizes_are_monotone():
    lib = _lib.lib()
    fns = ((lambda B, F, K: lib.vsp_align_scores_workspace_bytes(B, F, K)), (lambda B, F, K: lib.vsp_align_path_workspace_bytes(B, F, K)),
           (lambda B, F, K: lib.vsp_align_workspace_bytes(B, F, K, 50)))
    grid = [(B, F, K) for B in (1, 2, 16) for F in (1, 64, 65, 900) for K in (1, 255, 256, 257, 1025, 4096, 5000)]
    for fn in fns:
        for B, F, K in grid:
            v = fn(B, F, K)
            assert v > 0
            assert fn(B + 1, F, K) >= v and fn(B, F + 1, K) >= v and fn(B, F, K + 1) >= v
        assert fn(0, 9, 9) == -1 and fn(1, 0, 9) == -1 and fn(1, 9, 0) == -1
    # the fused call holds the score matrix, 2 bits a back-pointer, and covers each part
    assert lib.vsp_align_workspace_bytes(2, 100, 300, 50) >= 2 * 100 * 300 * 4 + 2 * 100 * 300 // 4
    assert lib.vsp_align_workspace_bytes(2, 100, 300, 50) > lib.vsp_align_path_workspace_bytes(2, 100, 300) > \
        lib.vsp_align_scores_workspace_bytes(2, 100, 300)
    assert lib.vsp_align_workspace_bytes(2, 100, 300, 51) >= lib.vsp_align_workspace_bytes(2, 100, 300, 50)


def test_the_engine_validates_align_parameters_like_its_others():
    from vispeech_amd.engine import Engine
    P = Engine._align_params
    d = P(None)
    assert (d.max_advance, d.stay_cost, d.skip_cost) == (2, 0.0, 0.0)
    assert P(True).max_advance == 2 and P(dict(max_advance=1)).max_advance == 1
    assert round(P((2, 0.3, 0.7)).skip_cost, 6) == 0.7
    for bad in (dict(advance=1), (2, 0.0), (0, 0.0, 0.0), (3, 0.0, 0.0), (2, -1.0, 0.0), (2, 0.0, float("nan"))):
        with pytest.raises(ValueError):
            P(bad)
    R = Engine._align_rows
    assert R(2, 9, 9, [9, 5], [9, 9], P(None), 4096) == ([9, 5], [9, 9])
    with pytest.raises(ValueError, match="row 1.*infeasible"):
        R(2, 9, 9, [9, 4], [9, 9], P(None), 4096)
    with pytest.raises(ValueError, match="row 0.*limit"):
        R(1, 9000, 5000, [9000], [4097], P(None), 4096)


# ---------------------------------------------------------------------------------------------- the restatement
def test_the_path_against_every_path_enumerated():
    rng = np.random.default_rng(0)
    checked = 0
    for A, F, K in itertools.product((1, 2), range(1, 7), range(1, 8)):
        paths = ar.all_paths(F, K, A)
        assert (len(paths) > 0) == ar.feasible(F, K, A) == (K <= A * (F - 1) + 1)
        S = rng.standard_normal((F, K)).astype(np.float32)
        if not paths:
            with pytest.raises(ValueError):
                ar.best_path(S, A, 0.3, 0.7)
            continue
        states, value = ar.best_path(S, A, 0.3, 0.7, with_value=True)
        values = [ar.path_value(S, p, 0.3, 0.7) for p in paths]
        assert value == ar.path_value(S, states, 0.3, 0.7)
        assert abs(value - max(values)) <= 1e-12 * max(1.0, abs(value))
        assert any(np.array_equal(states, p) for p in paths)
        assert states[0] == 0 and states[-1] == K - 1 and set(np.diff(states)) <= set(range(A + 1))
        checked += 1
    assert checked > 40


def test_the_tie_rule_on_tables_worked_by_hand():
    # F = 3, K = 2, all scores 0, no costs: [0, 0, 1] and [0, 1, 1] are equal.  At the last cell staying (from state 1) and
    # advancing (from state 0) both give 0: the lowest advance wins, so frame 1 is already in state 1.
    np.testing.assert_array_equal(ar.best_path(np.zeros((3, 2), np.float32), 1), [0, 1, 1])
    np.testing.assert_array_equal(ar.best_path(np.zeros((3, 2), np.float32), 2), [0, 1, 1])
    # F = 3, K = 3, A = 2: [0, 1, 2], [0, 2, 2] and [0, 0, 2] are equal; the last cell stays, so frame 1 took the skip
    np.testing.assert_array_equal(ar.best_path(np.zeros((3, 3), np.float32), 2), [0, 2, 2])
    # with costs 0.5 / 1: stay-then-step and step-then-stay both cost 0.5; again the last cell stays
    np.testing.assert_array_equal(ar.best_path(np.zeros((3, 2), np.float32), 2, 0.5, 1.0), [0, 1, 1])
    # ... and where the costs decide, they do: one step a frame is free, the skip and the stay are not
    np.testing.assert_array_equal(ar.best_path(np.zeros((3, 3), np.float32), 2, 0.5, 1.0), [0, 1, 2])


def test_scores_are_the_gaussian_log_likelihood_without_its_constant():
    rng = np.random.default_rng(3)
    x, m, logs = rng.standard_normal((5, 4)), rng.standard_normal((5, 3)), rng.uniform(-2, 1, (5, 3))
    S, t, l = ar.scores(x, m, logs, with_sums=True)
    for j in range(4):
        for k in range(3):
            sd = np.exp(logs[:, k])
            full = np.sum(-0.5 * np.log(2 * np.pi) - logs[:, k] - 0.5 * ((x[:, j] - m[:, k]) / sd) ** 2)
            assert abs(S[j, k] - (full + 0.5 * 5 * np.log(2 * np.pi))) < 1e-9
    assert t.shape == (4, 3) and l.shape == (3,) and (t >= 0).all()


def test_durations_count_the_frames_of_each_phoneme():
    states = np.array([0, 0, 1, 3, 3, 4, 6], dtype=np.int32)
    np.testing.assert_array_equal(ar.durations(states, [0, 2, 2, 5, 7, 7], 6, 8), [0, 3, 0, 3, 1, 0, 0, 0])


# ---------------------------------------------------------------------------------------------- the GPU tests' inputs
def test_the_planted_path_is_recovered_by_the_restatement():
    x, m, logs, k = ar.planted()
    adv = np.diff(k)
    assert x.shape == (192, 55) and m.shape == (192, 40)
    assert (np.count_nonzero(adv == 1), np.count_nonzero(adv == 2), np.count_nonzero(adv == 0)) == (31, 4, 19)
    S = ar.scores(x, m, logs)
    np.testing.assert_array_equal(ar.best_path(S.astype(np.float32), 2), k)
    # what the test is there to catch would not pass: a minimiser, a transposed matrix, a reversed walk
    assert not np.array_equal(ar.best_path((-S).astype(np.float32), 2), k)
    assert not np.array_equal(k, (39 - k)[::-1])


def test_the_ties_table_really_has_ties():
    S = ar.ties_table()
    assert S.shape == (65, 40) and set(np.unique(S)) == {0.0, 1.0, 2.0}
    assert ar.count_ties(S, 2, 0.5, 1.0) > 100
    # ... on the best path too: another path of the same value exists
    states, value = ar.best_path(S, 2, 0.5, 1.0, with_value=True)
    assert value == ar.path_value(S, states, 0.5, 1.0) and float(value * 2).is_integer()


def test_the_constructed_rows_are_what_the_gpu_tests_say():
    for (F, K) in ar.PATH_ROWS_A2:
        assert ar.feasible(F, K, 2)
    for (F, K) in ar.PATH_ROWS_A1:
        assert ar.feasible(F, K, 1)
    assert 125 == 2 * (63 - 1) + 1 and not ar.feasible(63, 126, 2)          # the only path is all skips
    np.testing.assert_array_equal(ar.best_path(ar.random_tables([(63, 125)], 1)[0], 2), 2 * np.arange(63))
    np.testing.assert_array_equal(ar.best_path(ar.random_tables([(130, 130)], 1)[0], 1), np.arange(130))
    np.testing.assert_array_equal(ar.best_path(ar.random_tables([(130, 1)], 1)[0], 1), np.zeros(130))
    rows = ar.score_rows(7, 1)
    assert len(rows) == 25 and {(r[0].shape[1], r[1].shape[1]) for r in rows} == set(itertools.product(ar.SCORE_SIZES, repeat=2))
    x, m, logs, F, K = ar.pack_inputs(rows)
    assert np.isnan(x[0, :, 1:]).all() and np.isnan(m[0, :, 1:]).all() and np.isnan(logs[0, :, 1:]).all()
    assert all(np.isfinite(x[b, :, :F[b]]).all() and np.isfinite(logs[b, :, :K[b]]).all() for b in range(25))


# ---------------------------------------------------------------------------------------------- the service's calls
from test_prosody_host import SVC_HOP, InferNet, ProsodyEngine  # noqa: E402


class AlignEngine(ProsodyEngine):
    """The recording engine with ``align_audio``: every phoneme of a row gets one frame, its first the rest."""

    def align_audio(self, phonemes, lengths, sid, audio, n_samples, sid_audio=None, params=None, fit_length=True):
        import torch
        n = [int(v) for v in n_samples]
        self.calls.append(("align_audio", phonemes.tolist(), [int(v) for v in lengths], [int(v) for v in sid], n, list(sid_audio),
                           (params.max_advance, params.stay_cost, params.skip_cost)))
        assert tuple(audio.shape[:1]) == (len(n),) and fit_length
        d = torch.zeros(phonemes.shape, dtype=torch.int64)
        for b, L in enumerate(lengths):
            d[b, : int(L)] = 1
            d[b, 0] = n[b] // SVC_HOP + 1 - (int(L) - 1)
        return d


def _service(net, **kw):
    from vispeech_amd.service import BatchingSynthesisService
    from vispeech_amd.text import SymbolTable
    return BatchingSynthesisService(net, max_batch=3, max_wait_s=30.0, table=SymbolTable(["a", "b", "c"]), spk2id={"s": 0, "t": 1}, **kw)


def test_service_aligns_the_rows_that_bring_no_durations_in_one_call():
    from vispeech_amd.text import request_row
    net = InferNet()
    net._engine = AlignEngine()
    rec_a = np.arange(1, 3 * SVC_HOP + 1, dtype=np.float32)                   # 4 frames
    rec_b = 100.0 + np.arange(2 * SVC_HOP, dtype=np.float32)                  # 3 frames
    rec_c = 200.0 + np.arange(4 * SVC_HOP, dtype=np.float32)                  # 5 frames
    svc = _service(net, prosody_align=dict(stay_cost=0.25))
    try:
        futs = [svc.submit(request_row("s", ["a", "b", "c"]), 7, prosody_audio=rec_a),
                svc.submit(request_row("t", ["c", "a"], durations=[2, 1]), 8, prosody_audio=rec_b),
                svc.submit(request_row("t", ["b", "a"]), 9, prosody_audio=rec_c, prosody_sid=0)]
        for f in futs:
            assert f.result(60).shape == (3 * SVC_HOP,)
    finally:
        svc.close()
    assert net._engine.calls == [
        ("align_audio", [[0, 1, 2], [1, 0, 0]], [3, 2], [0, 1], [3 * SVC_HOP, 4 * SVC_HOP], [0, 0], (2, 0.25, 0.0)),
        ("prosody_contours", [3 * SVC_HOP, 2 * SVC_HOP, 4 * SVC_HOP]),
        ("prosody_phonemes", [4, 3, 5], [[2, 1, 1], [2, 1, 0], [4, 1, 0]], [3, 2, 2])]
    (call,) = net.infers
    np.testing.assert_array_equal(np.asarray(call["duration"]), [[2, 1, 1], [2, 1, 0], [4, 1, 0]])
    assert call["rows"] is None                                               # every row ended up with all three controls
    assert call["seeds"] == [7, 8, 9]


def test_service_with_align_leaves_rows_that_bring_durations_alone():
    from vispeech_amd.text import request_row
    net = InferNet()
    net._engine = AlignEngine()
    svc = _service(net, prosody_align=True)
    try:
        f = svc.submit(request_row("s", ["a", "b", "c"], durations=[1, 0, 2]), 7, prosody_audio=np.arange(1, 3 * SVC_HOP + 1, dtype=np.float32))
        assert f.result(60).shape == (3 * SVC_HOP,)
    finally:
        svc.close()
    assert [c[0] for c in net._engine.calls] == ["prosody_contours", "prosody_phonemes"]


def test_service_without_align_refuses_as_it_always_did():
    from vispeech_amd.text import request_row
    net = InferNet()
    net._engine = AlignEngine()
    svc = _service(net)
    try:
        with pytest.raises(ValueError, match="durations"):
            svc.submit(request_row("s", ["a"]), 1, prosody_audio=np.zeros(4096, np.float32))
        with pytest.raises(ValueError):
            svc.submit(request_row("s", ["a"], durations=[1]), 1, prosody_sid=0)
    finally:
        svc.close()
    with pytest.raises(ValueError):
        _service(net, prosody_align=(3, 0.0, 0.0))
    svc = _service(net, prosody_align=True)
    try:
        with pytest.raises(ValueError, match="641"):
            svc.submit(request_row("s", ["a"]), 1, prosody_audio=np.zeros(100, np.float32))
    finally:
        svc.close()
    assert net._engine.calls == [] and net.infers == []


def test_service_with_a_collate_that_returns_no_given_array():
    """A collate callable need not say which controls a row carries: the rows aligned here are marked by the service."""
    from vispeech_amd.service import BatchingSynthesisService
    from vispeech_amd.text import SymbolTable, collate_rows, request_row
    table, spk = SymbolTable(["a", "b", "c"]), {"s": 0, "t": 1}

    def collate(rows):
        out = collate_rows(rows, table, spk)
        return {k: v for k, v in out.items() if k in ("phonemes", "lengths", "sid")}

    net = InferNet()
    net._engine = AlignEngine()
    svc = BatchingSynthesisService(net, max_batch=1, max_wait_s=30.0, collate=collate, prosody_align=True)
    try:
        f = svc.submit(request_row("t", ["b", "a"]), 9, prosody_audio=200.0 + np.arange(4 * SVC_HOP, dtype=np.float32))
        assert f.result(60).shape == (3 * SVC_HOP,)
    finally:
        svc.close()
    assert [c[0] for c in net._engine.calls] == ["align_audio", "prosody_contours", "prosody_phonemes"]
    assert net._engine.calls[2][2] == [[4, 1]]
    (call,) = net.infers
    np.testing.assert_array_equal(np.asarray(call["duration"]), [[4, 1]])


def test_submit_checks_the_recordings_speaker():
    from vispeech_amd.text import request_row
    net = InferNet()
    net._engine = AlignEngine()
    net.n_speakers = 2
    svc = _service(net, prosody_align=True)
    rec = np.zeros(4096, np.float32)
    try:
        for bad in (-1, 2, 0.5):
            with pytest.raises(ValueError, match="prosody_sid"):
                svc.submit(request_row("s", ["a"]), 1, prosody_audio=rec, prosody_sid=bad)
        with pytest.raises(ValueError, match="prosody_sid"):
            svc.submit(request_row("s", ["a"], durations=[1]), 1, prosody_sid=1)
        with pytest.raises(ValueError, match="prosody_sample_rate / prosody_encoding describe prosody_audio"):
            svc.submit(request_row("s", ["a"], durations=[1]), 1, prosody_sample_rate=16000)
    finally:
        svc.close()
    assert net._engine.calls == [] and net.infers == []


# ---------------------------------------------------------------------------------------------- align_audio without enc_q
def test_align_audio_needs_the_posterior_encoder():
    """A checkpoint without the ``enc_q.*`` tensors: the error of ``convert_audio`` and ``voice_conversion``, before any call."""
    from vispeech_amd.models import SynthesizerTrn

    class Eng:
        ready, has_voice_conversion, calls = True, False, []

        def __getattr__(self, name):
            raise AssertionError(f"the engine was asked for {name}")

    class Net:
        n_speakers = 2
        _engine = Eng()

    with pytest.raises(RuntimeError, match=r"align_audio needs the enc_q\.\* tensors: the loaded state_dict had none"):
        SynthesizerTrn.align_audio(Net(), np.zeros((1, 2), np.int64), [2], [0], np.zeros((1, 4096), np.float32), [4096])
    Net._engine = type("NotReady", (Eng,), dict(ready=False))()
    with pytest.raises(RuntimeError, match="weights not loaded"):
        SynthesizerTrn.align_audio(Net(), np.zeros((1, 2), np.int64), [2], [0], np.zeros((1, 4096), np.float32), [4096])
