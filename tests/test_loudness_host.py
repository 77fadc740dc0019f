"""Loudness, everything a CPU can check (no kernel is launched): the entry points exist and refuse what
they must before a device is needed, naming the row; the workspace sizes are monotone; the K-weighting coefficients at 48 kHz
are BS.1770's tables; the fp64 restatement (tests/loudness_ref.py) judged on its own -- BS.1770's -3.01 LKFS sine, the values
measured with an fp64 scipy run of the specification, the gates on tables worked by hand --; the properties the GPU tests'
inputs must have (tests/test_loudness_gpu.py rests on them); and the batching service's calls with and without ``loudness=``."""
import ctypes as C
import math

import numpy as np
import pytest

import loudness_ref as lr
import test_abi
from vispeech_amd import _lib
from vispeech_amd.schema import ModelDims

NEW = ("vsp_loudness_kweighting", "vsp_loudness_segments_count", "vsp_loudness_workspace_bytes", "vsp_loudness_segments",
       "vsp_loudness_gate", "vsp_loudness_apply", "vsp_loudness_normalize")


# ---------------------------------------------------------------------------------------------- symbols and ABI
def test_symbols_and_abi():
    lib = _lib.lib()
    for s in NEW:
        assert hasattr(lib, s) and s in _lib.SIGNATURES, s
    assert lib.vsp_abi_version() == 7
    assert sorted(_lib.SIGNATURES) == test_abi.header_symbols()
    assert C.sizeof(_lib.VspLoudnessParams) == 12


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
NAN = float("nan")


def _i64(v):
    return (C.c_int64 * len(v))(*v)


def _params(rows):
    return None if rows is None else (_lib.VspLoudnessParams * len(rows))(*[_lib.VspLoudnessParams(*r) for r in rows])


def _segments(lib, h, n, L_max, fs=44100, ws=BIG):
    return lib.vsp_loudness_segments(h, None, len(n), L_max, fs, BAD, L_max, _i64(n), BAD, BAD, BAD, ws)


def _gate(lib, h, n, S_max, fs=44100, params=None, ws=BIG):
    return lib.vsp_loudness_gate(h, None, len(n), S_max, fs, BAD, _i64(n), BAD, _params(params), BAD, BAD, BAD, BAD, ws)


def _apply(lib, h, n, L_max, params=None, ws=BIG):
    return lib.vsp_loudness_apply(h, None, len(n), L_max, BAD, L_max, BAD, L_max, _i64(n), BAD, _params(params), BAD, ws)


def _normalize(lib, h, n, L_max, params, fs=44100, ws=BIG):
    return lib.vsp_loudness_normalize(h, None, len(n), L_max, fs, BAD, L_max, BAD, L_max, _i64(n), _params(params), BAD, BAD, BAD,
                                      BAD, BAD, ws)


def test_refusals_before_a_device_is_needed(ctx):
    lib, h = ctx
    err = lambda: lib.vsp_last_error(h)
    ok = (-23.0, 1.0, 30.0)
    # a row of no samples, a row longer than L_max: every call, naming the row
    for call in (lambda n: _segments(lib, h, n, 9000), lambda n: _apply(lib, h, n, 9000),
                 lambda n: _normalize(lib, h, n, 9000, [ok] * len(n)), lambda n: _gate(lib, h, n, 2, fs=45000)):     # S_max h = 9000
        assert call([9000, 0, 5]) == -1 and b"row 1" in err() and b"samples" in err()
        assert call([9000, 5, 9001]) == -1 and b"row 2" in err()
        assert call([9000, -3]) == -1 and b"row 1" in err()
    # the sample rate
    for fs in (7999, 192001, 0, -44100):
        assert _segments(lib, h, [5], 9, fs=fs) == -1 and b"sample_rate" in err()
        assert _gate(lib, h, [5], 1, fs=fs) == -1 and b"sample_rate" in err()
        assert _normalize(lib, h, [5], 9, [ok], fs=fs) == -1 and b"sample_rate" in err()
        assert lib.vsp_loudness_workspace_bytes(1, 9, fs) == -1 and lib.vsp_loudness_segments_count(9, fs) == -1
        assert lib.vsp_loudness_kweighting(fs, (C.c_double * 10)()) == -1
    assert _segments(lib, h, [5], 9, fs=8000, ws=16) == -6 and _segments(lib, h, [5], 9, fs=192000, ws=16) == -6      # (the ends are fine)
    # the params, in every call that takes them
    for bad, word in (((-23.0, 0.0, 30.0), b"peak_ceiling"), ((-23.0, -1.0, 30.0), b"peak_ceiling"), ((-23.0, NAN, 30.0), b"peak_ceiling"),
                      ((-23.0, 1.0, -0.5), b"max_gain_db"), ((-23.0, 1.0, NAN), b"max_gain_db"), ((NAN, 1.0, -1.0), b"max_gain_db")):
        for call in (lambda p: _normalize(lib, h, [9, 9, 9], 9, p), lambda p: _gate(lib, h, [9, 9, 9], 1, params=p),
                     lambda p: _apply(lib, h, [9, 9, 9], 9, params=p)):
            assert call([ok, ok, bad]) == -1 and b"row 2" in err() and word in err()
    # a NaN target is no refusal: the row is left alone (the next thing refused is the workspace)
    assert _normalize(lib, h, [9], 9, [(NAN, 1.0, 0.0)], ws=16) == -6
    # a workspace too small is a refusal of its own (-6)
    assert _segments(lib, h, [9000], 9000, ws=16) == -6 and _gate(lib, h, [9], 1, ws=16) == -6
    assert _apply(lib, h, [9], 9, ws=16) == -6 and _normalize(lib, h, [9000], 9000, [ok], ws=16) == -6
    need = lib.vsp_loudness_workspace_bytes(1, 9000, 44100)
    assert _normalize(lib, h, [9000], 9000, [ok], ws=need - 1) == -6


def test_null_pointers_are_refused_after_the_rows(ctx):
    lib, h = ctx
    assert lib.vsp_loudness_segments(h, None, 1, 9, 44100, None, 9, _i64([9]), BAD, BAD, BAD, BIG) == -1
    assert lib.vsp_loudness_apply(h, None, 1, 9, BAD, 9, None, 9, _i64([9]), BAD, None, BAD, BIG) == -1
    assert lib.vsp_loudness_gate(h, None, 1, 1, 44100, BAD, _i64([9]), None, _params([(-23.0, 1.0, 30.0)]), BAD, BAD, BAD, BAD, BIG) == -1
    assert lib.vsp_loudness_normalize(h, None, 1, 9, 44100, BAD, 9, BAD, 9, _i64([9]), None, BAD, BAD, BAD, BAD, BAD, BIG) == -1
    assert lib.vsp_loudness_segments(None, None, 1, 9, 44100, BAD, 9, _i64([9]), BAD, BAD, BAD, BIG) == -1


def test_workspace_sizes_are_monotone():
    lib = _lib.lib()
    for fs in (8000, 22050, 44100, 48000, 192000):
        for B in (1, 2, 16, 17):
            for L in (1, 799, 800, 4410, 4411, 44100, 441000, 1 << 24):
                v = lib.vsp_loudness_workspace_bytes(B, L, fs)
                assert v > 0
                assert lib.vsp_loudness_workspace_bytes(B + 1, L, fs) >= v and lib.vsp_loudness_workspace_bytes(B, L + 1, fs) >= v
                assert lib.vsp_loudness_workspace_bytes(B, L + 64 * lr.segment_samples(fs), fs) > v
                S = lib.vsp_loudness_segments_count(L, fs)
                assert S == lr.segments_count(L, fs) and v >= B * S * (4 + 4 + 1) * 8          # two state tables and seg
    assert lib.vsp_loudness_workspace_bytes(0, 9, 44100) == -1 and lib.vsp_loudness_workspace_bytes(1, 0, 44100) == -1
    assert lib.vsp_loudness_segments_count(0, 44100) == -1
    assert [lr.segment_samples(fs) for fs in (44100, 22050, 8000, 48000)] == [4410, 2205, 800, 4800]


# ---------------------------------------------------------------------------------------------- K-weighting
TABLE_48K = (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
             1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621)


def test_kweighting_at_48k_is_the_standards_table():
    lib = _lib.lib()
    c = (C.c_double * 10)()
    assert lib.vsp_loudness_kweighting(48000, c) == 0
    np.testing.assert_allclose(list(c), TABLE_48K, rtol=0, atol=1e-12)
    np.testing.assert_allclose(lr.kweighting(48000), TABLE_48K, rtol=0, atol=1e-12)
    for fs in (8000, 22050, 44100, 96000, 192000):
        assert lib.vsp_loudness_kweighting(fs, c) == 0
        np.testing.assert_allclose(list(c), lr.kweighting(fs), rtol=1e-14, atol=0)


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("fs, f, a, want, tol", [(48000, 997.0, 1.0, -3.01, 0.005), (48000, 997.0, 1.0, -3.0103, 1e-4),
                                                 (44100, 997.0, 1.0, -3.0075, 1e-4), (22050, 997.0, 1.0, -2.981, 1e-3),
                                                 (44100, 1000.0, 0.1, -23.0008, 1e-4)])
def test_the_restatement_reproduces_the_measured_values(fs, f, a, want, tol):
    x = lr.tone(fs, 5 * fs, f, a)
    assert abs(lr.loudness(x, len(x), fs) - want) <= tol


def test_the_restatements_filter_is_scipys():
    signal = pytest.importorskip("scipy.signal")
    for fs in (8000, 44100):
        x = lr.main_signal(fs, 3 * fs // 2)
        c = lr.kweighting(fs)
        y = signal.lfilter(c[5:8], [1.0, c[8], c[9]], signal.lfilter(c[:3], [1.0, c[3], c[4]], x.astype(np.float64)))
        np.testing.assert_allclose(lr.kfilter(x, fs), y, rtol=0, atol=1e-12)


H = lr.segment_samples(lr.TABLE_FS)


def _blocks_table(E):
    """A segment table whose blocks are E[0], then four of each further E: seg = [E0, 0, 0, 0, E1, 0, 0, 0, ...]."""
    seg = np.zeros(4 * len(E))
    seg[::4] = E
    return seg, 4 * len(E) * H


def test_gating_on_tables_worked_by_hand():
    fs, D = lr.TABLE_FS, 4.0 * H
    # E = {1, 19} (over D = 1 in the issue's words; the gates see E / D, so scale by D): mean_abs = 10, 10 * 1 == 10: NOT kept
    seg = np.array([0.25, 0.25, 0.25, 0.25, 18.25]) * D
    L, NB, kept, which, E, Dg, mean_abs, L64 = lr.gate(seg, 5 * H, fs, detail=True)
    assert (NB, kept, which) == (2, 1, [1]) and list(E) == [D, 19 * D] and Dg == D and mean_abs == 10 * D
    assert L64 == -0.691 + 10 * math.log10(19.0)
    # just above the tie the block is kept
    seg[0] = 0.25 * D * (1 + 1e-9)
    assert lr.gate(seg, 5 * H, fs)[1:] == (2, 2)
    # the absolute gate is strict too: E / D == Z_abs does not pass
    at = lr.at_abs_gate(D)
    assert not at / D > lr.Z_ABS and np.nextafter(at, np.inf) / D > lr.Z_ABS
    assert lr.gate(np.array([at, 0, 0, 0, 4.0 * at]), 5 * H, fs, detail=True)[3] == [1]
    assert lr.gate(np.array([np.nextafter(at, np.inf), 0, 0, 0, 4.0 * at]), 5 * H, fs, detail=True)[3] == [0, 1]
    # a short row: one block of all its segments over D = n
    L, NB, kept = lr.gate(np.array([3.0, 5.0, 0.5]), 2 * H + 11, fs)
    assert (NB, kept) == (1, 1) and L == np.float32(-0.691 + 10 * math.log10(8.5 / (2 * H + 11)))
    # only complete blocks count: 5 h + (h - 1) samples are still two blocks
    assert lr.gate(np.ones(6), 6 * H - 1, fs)[1] == 2 and lr.gate(np.ones(6), 6 * H, fs)[1] == 3
    # nothing passes: -inf
    L, NB, kept = lr.gate(np.zeros(6), 6 * H, fs)
    assert L == -np.inf and (NB, kept) == (3, 0)


def test_the_absolute_gate_changes_what_the_relative_gate_keeps():
    fs, D = lr.TABLE_FS, 4.0 * H
    z = lr.Z_ABS * D
    # one block of 1000, then blocks of 15, then many of 0.5 (in units of the absolute gate): with the quiet blocks gated out
    # mean_abs = (1000 + 4 * 15) / 5 = 212 > 150, so the blocks of 15 go; had the quiet blocks counted, the mean over all 45
    # blocks would be (1060 + 40 * 0.5) / 45 = 24 < 150 and they would stay
    E = [1000 * z, 15 * z] + [0.5 * z] * 10
    seg, n = _blocks_table(E)
    L, NB, kept, which, Eb, _, mean_abs, _ = lr.gate(seg, n, fs, detail=True)
    assert NB == 4 * len(E) - 3 and which == [0] and math.isclose(mean_abs, 212 * z, rel_tol=1e-12)
    assert 10 * 15 * z > np.mean(Eb)
    assert L == np.float32(-0.691 + 10 * math.log10(1000 * lr.Z_ABS))


def test_gain_formula_and_its_limits():
    assert lr.gain(-30.0, 0.1, -23.0, 1.0, 30.0) == 10 ** (7 / 20)
    assert lr.gain(-30.0, 0.5, -23.0, 1.0, 30.0) == 2.0                     # the ceiling binds
    assert lr.gain(-60.0, 0.001, -23.0, 1.0, 20.0) == 10.0                  # the gain limit binds
    assert lr.gain(-30.0, 0.1, NAN, 1.0, 30.0) == 1.0 and lr.gain(-math.inf, 0.1, -23.0, 1.0, 30.0) == 1.0
    assert lr.gain(-30.0, 0.0, -23.0, 1.0, 30.0) == 10 ** (7 / 20)          # no peak, no ceiling


# ---------------------------------------------------------------------------------------------- the GPU tests' inputs
@pytest.mark.parametrize("fs", [44100, 22050, 8000, 192000])
def test_the_audio_rows_stay_clear_of_both_gates(fs):
    """A condition on the inputs, every block of every row: E_j / D is a factor 1.05 from Z_abs and 10 E_j from mean_abs, so
    that no rounding of a correct implementation can move a block across a gate."""
    rows = lr.measured_rows(fs)
    fa, fr = zip(*(lr.gate_margins(r["seg"], r["n"], fs) for r in rows))
    assert min(fa) >= 1.05 and min(fr) >= 1.05, (min(fa), min(fr))
    if fs == 44100:
        assert [r["n"] for r in rows[:9]] == list(lr.MAIN_LENGTHS)
        by = {r["name"]: r for r in rows}
        assert by["zeros"]["L"] == -np.inf and by["tone 1e-4"]["L"] == -np.inf and by["tone 1e-4"]["NB"] == 17
        assert by["drop"]["NB"] == 42 and 0 < len(by["drop"]["kept"]) < 42                   # the quiet end is gated out
        assert len(by["main[:352800]"]["kept"]) < by["main[:352800]"]["NB"] == 77            # the relative gate works here
        assert max(r["yardstick"] for r in rows[:9]) > 1e-4 > by["drop"]["yardstick"]        # DC: float32 is 2.8e-4 LU off
    h = lr.segment_samples(fs)
    # uneven lane runs at the common rates; 192 kHz is the rate whose segment IS 64 runs of 300 (and needs the most LDS)
    assert (h % 64 == 0) == (fs == 192000) and {r["n"] for r in rows} >= ({1, 4409, 4410, 17639, 17640} if fs == 44100 else {h - 1, h, 4 * h - 1, 4 * h})
    for r in rows:
        assert 1e-5 <= r["gate_lu"] <= 0.1


def test_the_gate_tables_have_exact_ties():
    fs = lr.TABLE_FS
    rows = lr.gate_tables()
    assert [len(seg) for seg, _ in rows[:7]] == list(lr.TABLE_SEGMENTS)
    ties = 0
    for seg, n in rows:
        _, _, _, kept, E, D, mean_abs, _ = lr.gate(seg, n, fs, detail=True)
        if mean_abs is not None:
            ties += sum(1 for e in E if 10.0 * e == mean_abs)
    assert ties >= 2
    a, n = lr.pack([r[0] for r in rows])
    assert a.shape[1] == 131 and np.isnan(a[0, 1:]).all()


# ---------------------------------------------------------------------------------------------- parameters in Python
def test_the_engine_and_the_service_validate_loudness_parameters():
    from vispeech_amd.engine import Engine
    from vispeech_amd.service.batching import _loudness_spec
    p = Engine.loudness_params(3, [-16.0, None, NAN], 0.9, [30.0, 0.0, 6.0])
    assert p[0].target_lufs == -16.0 and math.isnan(p[1].target_lufs) and math.isnan(p[2].target_lufs)
    assert round(p[1].peak_ceiling, 6) == 0.9 and p[2].max_gain_db == 6.0
    assert Engine.loudness_params(2)[1].target_lufs == -23.0
    with pytest.raises(ValueError, match="row 1.*peak_ceiling"):
        Engine.loudness_params(2, -23.0, [1.0, 0.0])
    with pytest.raises(ValueError, match="row 0.*max_gain_db"):
        Engine.loudness_params(1, -23.0, 1.0, -3.0)
    with pytest.raises(ValueError, match="2 entries"):
        Engine.loudness_params(2, [-23.0])
    assert _loudness_spec(None) is None and _loudness_spec(False) is None
    assert _loudness_spec(-16) == (-16.0, 1.0, 30.0)
    assert _loudness_spec(dict(target_lufs=-20, max_gain_db=6)) == (-20.0, 1.0, 6.0)
    for bad in (NAN, float("inf"), dict(peak_ceiling=1.0), dict(target_lufs=-16, gain=3), dict(target_lufs=-16, peak_ceiling=0),
                dict(target_lufs=-16, max_gain_db=-1), True):
        with pytest.raises(ValueError):
            _loudness_spec(bad)


# ---------------------------------------------------------------------------------------------- the service's calls
from test_prosody_host import SVC_HOP, InferNet, ProsodyEngine  # noqa: E402
from test_service_paths_host import PAD, UP, RecordingEngine, RecordingNet, _audio, _collate  # noqa: E402


def _record_normalize(self, waves, n, sample_rate, params):
    """The stand-in's ``loudness_normalize``: records its rows and doubles, in place, every row that has a target."""
    assert waves.dim() == 2 and waves.shape[0] == len(n) == len(params)
    rows = [(None if math.isnan(p.target_lufs) else round(p.target_lufs, 3), round(p.peak_ceiling, 3), round(p.max_gain_db, 3))
            for p in params]
    self.calls.append(("loudness_normalize", [int(v) for v in n], int(sample_rate), rows))
    for b, p in enumerate(params):
        if not math.isnan(p.target_lufs):
            waves[b, : int(n[b])] *= 2.0


class LoudInferEngine(ProsodyEngine):
    loudness_normalize = _record_normalize


class LoudInferNet(InferNet):
    """``InferNet`` whose waveform is 0.25 everywhere, so that a doubled row shows in its PCM16."""

    def __init__(self):
        super().__init__()
        self._engine = LoudInferEngine()

    def infer(self, *a, **k):
        o, x_mask = super().infer(*a, **k)
        return o + 0.25, x_mask


def _text_service(net, max_batch=3, **kw):
    from vispeech_amd.service import BatchingSynthesisService
    from vispeech_amd.text import SymbolTable
    return BatchingSynthesisService(net, max_batch=max_batch, max_wait_s=30.0, table=SymbolTable(["a", "b", "c"]), spk2id={"s": 0, "t": 1}, **kw)


def test_service_makes_one_normalize_call_for_a_text_batch():
    from vispeech_amd.text import request_row
    net = LoudInferNet()
    svc = _text_service(net)
    row = lambda: request_row("s", ["a", "b"], durations=[1, 2], f0=[5.0, 6.0], energy=[1.0, 2.0])
    try:
        futs = [svc.submit(row(), 1, loudness=-16), svc.submit(row(), 2),
                svc.submit(row(), 3, loudness=dict(target_lufs=-20.0, peak_ceiling=0.5, max_gain_db=6.0))]
        got = [f.result(60) for f in futs]
    finally:
        svc.close()
    n = 3 * SVC_HOP
    assert net._engine.calls == [("loudness_normalize", [n, n, n], 44100, [(-16.0, 1.0, 30.0), (None, 1.0, 0.0), (-20.0, 0.5, 6.0)])]
    assert len(net.infers) == 1
    q = lambda v: int(np.rint(np.float32(v) * 32767.0))
    assert [set(g.tolist()) for g in got] == [{q(0.5)}, {q(0.25)}, {q(0.5)}] and all(g.shape == (n,) for g in got)


def test_service_default_loudness_and_opting_out():
    from vispeech_amd.text import request_row
    net = LoudInferNet()
    svc = _text_service(net, loudness=dict(target_lufs=-18.0, max_gain_db=12.0))
    row = lambda: request_row("s", ["a"], durations=[3], f0=[5.0], energy=[1.0])
    try:
        futs = [svc.submit(row(), 1), svc.submit(row(), 2, loudness=False), svc.submit(row(), 3, loudness=-30.0)]
        [f.result(60) for f in futs]
    finally:
        svc.close()
    assert net._engine.calls[0][3] == [(-18.0, 1.0, 12.0), (None, 1.0, 0.0), (-30.0, 1.0, 30.0)]
    with pytest.raises(ValueError):
        _text_service(net, loudness=dict(target_lufs=-18.0, peak_ceiling=-1.0))


def test_service_without_loudness_makes_the_calls_it_always_made():
    from vispeech_amd.text import request_row
    net = LoudInferNet()
    svc = _text_service(net, max_batch=2)
    try:
        futs = [svc.submit(request_row("s", ["a"], durations=[3], f0=[5.0], energy=[1.0]), 1),
                svc.submit(request_row("t", ["b"], durations=[3], f0=[5.0], energy=[1.0]), 2)]
        got = [f.result(60) for f in futs]
        with pytest.raises(ValueError):
            svc.submit(request_row("s", ["a"], durations=[3], f0=[5.0], energy=[1.0]), 3, loudness=NAN)
    finally:
        svc.close()
    assert net._engine.calls == [] and len(net.infers) == 1
    assert all(set(g.tolist()) == {int(np.rint(np.float32(0.25) * 32767.0))} for g in got)


class LoudRecordingEngine(RecordingEngine):
    loudness_normalize = _record_normalize


def _mixed(loud):
    from vispeech_amd.service import BatchingSynthesisService
    net = RecordingNet()
    net._engine = eng = LoudRecordingEngine()
    svc = BatchingSynthesisService(net, max_batch=4, max_wait_s=30.0, collate=_collate, output_rate=22050)
    kw = lambda v: {"loudness": v} if loud else {}
    try:
        futs = [svc.submit({"id": 1, "frames": 6}, 7, **kw(-16)),
                svc.submit_conversion(_audio(93), 3, 5, 21, **kw(dict(target_lufs=-23.0, peak_ceiling=0.8))),
                svc.submit_conversion(_audio(PAD), 3, 9, 23, **kw(-16)),                # too short for one frame: no row
                svc.submit({"id": 2, "frames": 3}, 8)]
        got = [f.result(60) for f in futs]
    finally:
        svc.close()
    return eng.calls, got


def test_service_mixed_batch_normalizes_between_the_generator_and_the_output_stage():
    plain, got_plain = _mixed(False)
    calls, got = _mixed(True)
    assert "loudness_normalize" not in [c[0] for c in plain]
    k = [c[0] for c in calls].index("loudness_normalize")
    assert calls[k - 1][0] == "generator_ragged" and calls[k + 1][0] == "output"
    assert calls[k] == ("loudness_normalize", [6 * UP, 9 * UP, 3 * UP], 44100, [(-16.0, 1.0, 30.0), (-23.0, 0.8, 30.0), (None, 1.0, 0.0)])
    rest = calls[:k] + calls[k + 1:]                                         # but for it, the calls of the plain batch
    assert [c for c in rest if c[0] != "output"] == [c for c in plain if c[0] != "output"]
    assert [(c[0], c[-1]) for c in rest] == [(c[0], c[-1]) for c in plain]
    np.testing.assert_array_equal(got[0], 2 * got_plain[0])
    np.testing.assert_array_equal(got[1], 2 * got_plain[1])
    assert got[2].size == 0
    np.testing.assert_array_equal(got[3], got_plain[3])                      # the request that names nothing: its bytes
