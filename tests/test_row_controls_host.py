"""Per-row controls, host side (no GPU): vsp_set_row_controls' validation and state rules on a device-less context,
collate_rows with requests that leave controls to the predictors, the table the two batching services build from their
requests (on recording stand-ins), the argument checks of infer / infer_sharded / InFlightPool, and the checker of the GPU
tests -- the CPU oracle run alone with a row's own arguments -- against the REAL reference (tests/golden/row_controls.npz)."""
import ctypes as C

import numpy as np
import pytest

import row_controls_ref as rcr
from vispeech_amd import _lib
from vispeech_amd.schema import ModelDims

OK, ERR_ARG, ERR_STATE = 0, -1, -2


# ------------------------------------------------------------------ the C ABI on a context without a device
@pytest.fixture()
def ctx():
    lib = _lib.lib()
    cfg = _lib.make_config(ModelDims())
    h = C.c_void_p()
    assert lib.vsp_create(C.byref(cfg), 0, C.byref(h)) == 0
    yield lib, h
    lib.vsp_destroy(h)


def _rows(*rows):
    arr = (_lib.VspRowControl * len(rows))()
    for b, r in enumerate(rows):
        arr[b] = _lib.VspRowControl(*r)
    return arr


def _encode(lib, h, B, ctl=(None, None, None)):
    return lib.vsp_encode(h, None, B, 4, None, None, None, ctl[0], ctl[1], ctl[2], 1.0, 1.0, 1.0, None, None, None, None, None,
                          None, None, None, 0)


def _decode(lib, h, B):
    return lib.vsp_decode(h, None, B, 4, 8, -1, None, None, None, None, None, 0, 1.0, None, None, None, None, None, None,
                          None, 0)


def _infer(lib, h, B, ctl=(None, None, None)):
    return lib.vsp_infer(h, None, B, 4, 8, -1, None, None, None, ctl[0], ctl[1], ctl[2], 1.0, 1.0, 1.0, None, 0, 1.0,
                         None, None, None, None, None, None, None, None, None, None, None, 0)


def test_layout_matches_the_header():
    assert C.sizeof(_lib.VspRowControl) == 20       # four floats and the bits: what the kernels index by row
    assert (_lib.GIVEN_DURATION, _lib.GIVEN_PITCH, _lib.GIVEN_ENERGY) == (1, 2, 4)


def test_validation_needs_no_device(ctx):
    lib, h = ctx
    good = (1.0, 1.0, 1.0, 0.667, 0)
    assert lib.vsp_set_row_controls(h, _rows(good, (0.5, 2.0, 1.5, 0.0, 7)), 2) == OK
    assert lib.vsp_set_row_controls(h, _rows(good, (1.0, 1.0, 1.0, 1.0, 8)), 2) == ERR_ARG          # unknown bit
    assert b"given bits" in lib.vsp_last_error(h)
    for k in range(4):
        for bad in (float("nan"), float("inf"), -float("inf")):
            r = list(good)
            r[k] = bad
            assert lib.vsp_set_row_controls(h, _rows(good, tuple(r)), 2) == ERR_ARG, (k, bad)
            assert b"not finite" in lib.vsp_last_error(h)
    assert lib.vsp_set_row_controls(h, _rows(good), -1) == ERR_ARG
    assert lib.vsp_set_row_controls(h, None, 1) == ERR_ARG
    assert lib.vsp_set_row_controls(None, _rows(good), 1) == ERR_ARG


def test_a_table_needs_isolated_mode_and_its_own_batch_size(ctx):
    lib, h = ctx
    assert lib.vsp_set_row_controls(h, _rows((1.0, 1.0, 1.0, 1.0, 0), (1.0, 1.0, 1.0, 1.0, 0)), 2) == OK
    for call in (_encode, _decode, _infer):                     # not isolated: per-row values have no reference meaning
        assert call(lib, h, 2) == ERR_STATE
        assert b"not isolated" in lib.vsp_last_error(h), lib.vsp_last_error(h)
    assert lib.vsp_set_isolated(h, 1) == OK
    for call in (_encode, _decode, _infer):                     # a call of another batch size
        assert call(lib, h, 3) == ERR_STATE
        assert b"B = 2" in lib.vsp_last_error(h) and b"B = 3" in lib.vsp_last_error(h)
    # the right size passes these checks: what refuses the call now is that nothing is loaded
    for call in (_encode, _decode, _infer):
        assert call(lib, h, 2) == ERR_STATE and b"not finalised" in lib.vsp_last_error(h)
    # a refused table changes nothing; B = 0 forgets the table
    assert lib.vsp_set_row_controls(h, _rows((1.0, 1.0, 1.0, 1.0, 8)), 1) == ERR_ARG
    assert _encode(lib, h, 3) == ERR_STATE and b"B = 2" in lib.vsp_last_error(h)
    assert lib.vsp_set_row_controls(h, None, 0) == OK
    assert _encode(lib, h, 3) == ERR_STATE and b"not finalised" in lib.vsp_last_error(h)
    assert lib.vsp_set_isolated(h, 0) == OK
    assert _encode(lib, h, 3) == ERR_STATE and b"not finalised" in lib.vsp_last_error(h)


def test_a_given_control_must_be_there(ctx):
    lib, h = ctx
    assert lib.vsp_set_isolated(h, 1) == OK
    p = C.c_void_p(256)                   # (never dereferenced: the call is refused, or stops at "not finalised")
    for bit, slot in ((_lib.GIVEN_DURATION, 0), (_lib.GIVEN_PITCH, 1), (_lib.GIVEN_ENERGY, 2)):
        assert lib.vsp_set_row_controls(h, _rows((1.0, 1.0, 1.0, 1.0, 0), (1.0, 1.0, 1.0, 1.0, bit)), 2) == OK
        for call in (_encode, _infer):
            assert call(lib, h, 2) == ERR_ARG and b"NULL" in lib.vsp_last_error(h)
            ctl = [None, None, None]
            ctl[slot] = p
            assert call(lib, h, 2, ctl) == ERR_STATE and b"not finalised" in lib.vsp_last_error(h)
        assert _decode(lib, h, 2) == ERR_STATE and b"not finalised" in lib.vsp_last_error(h)   # (decode reads no control)


def test_workspace_sizes_do_not_depend_on_the_table(ctx):
    lib, h = ctx
    before = (lib.vsp_encode_workspace_bytes(h, 3, 40), lib.vsp_decode_workspace_bytes(h, 3, 40, 100),
              lib.vsp_infer_workspace_bytes(h, 3, 40, 100))
    assert lib.vsp_set_isolated(h, 1) == OK
    assert lib.vsp_set_row_controls(h, _rows(*[(1.0, 1.0, 1.0, 0.0, 7)] * 3), 3) == OK      # (every predictor and the draw skipped)
    after = (lib.vsp_encode_workspace_bytes(h, 3, 40), lib.vsp_decode_workspace_bytes(h, 3, 40, 100),
             lib.vsp_infer_workspace_bytes(h, 3, 40, 100))
    assert before == after and min(before) > 0


# ------------------------------------------------------------------ requests without prosody
def test_collate_rows_with_mixed_rows():
    from vispeech_amd.text import FilelistRow, SymbolTable, collate_rows, parse_filelist_row, request_row
    table = SymbolTable(["_", "a", "b", "c"])
    spk = {"x": 3, "y": 5}
    full = parse_filelist_row("x|u0|a b c|1 2 3|100.0 0.0 120.5|10.0 20.0 30.0")
    plain = request_row("y", ["b", "a"])
    dur_only = request_row("x", ["c"], durations=[4])
    pitch_energy = FilelistRow("y", "", ["a", "b"], None, np.array([1.0, 2.0], np.float32), np.array([3.0, 4.0], np.float32))
    assert plain.durations is None and plain.f0 is None and plain.energy is None
    out = collate_rows([full, plain, dur_only, pitch_energy], table, spk)
    np.testing.assert_array_equal(out["given"], [[1, 1, 1], [0, 0, 0], [1, 0, 0], [0, 1, 1]])
    assert out["given"].dtype == bool
    np.testing.assert_array_equal(out["phonemes"], [[1, 2, 3], [2, 1, 0], [3, 0, 0], [1, 2, 0]])
    np.testing.assert_array_equal(out["lengths"], [3, 2, 1, 2])
    np.testing.assert_array_equal(out["sid"], [3, 5, 3, 5])
    np.testing.assert_array_equal(out["duration"], [[1, 2, 3], [0, 0, 0], [4, 0, 0], [0, 0, 0]])
    np.testing.assert_array_equal(out["f0"], np.array([[100.0, 0.0, 120.5], [0, 0, 0], [0, 0, 0], [1, 2, 0]], np.float32))
    np.testing.assert_array_equal(out["energy"], np.array([[10, 20, 30], [0, 0, 0], [0, 0, 0], [3, 4, 0]], np.float32))
    # fully controlled rows: the arrays they always gave (and every bit set)
    two = collate_rows([full, parse_filelist_row("y|u1|b|7|50.0|5.0")], table, spk)
    assert two["given"].all()
    np.testing.assert_array_equal(two["duration"], np.array([[1, 2, 3], [7, 0, 0]], np.float32))
    np.testing.assert_array_equal(two["f0"], np.array([[100.0, 0.0, 120.5], [50.0, 0, 0]], np.float32))
    np.testing.assert_array_equal(two["energy"], np.array([[10, 20, 30], [5, 0, 0]], np.float32))
    assert {k: v.dtype for k, v in two.items() if k != "given"} == dict(
        phonemes=np.int64, lengths=np.int64, sid=np.int64, duration=np.float32, f0=np.float32, energy=np.float32)
    with pytest.raises(ValueError):
        request_row("x", ["a", "b"], durations=[1])


# ------------------------------------------------------------------ the services on recording stand-ins
class _Dims:
    total_upsample = 4
    inter_channels = 2


def _snapshot(rc):
    if rc is None:
        return None
    return dict(duration_scale=rc.duration_scale.tolist(), pitch_scale=rc.pitch_scale.tolist(),
                energy_scale=rc.energy_scale.tolist(), noise_scale=rc.noise_scale.tolist(), given=rc.given.tolist())


class _RecordingNet:
    """Records every infer call's keywords; every utterance gets two frames of its first phoneme id / 1000."""
    device = "cpu"
    dims = _Dims()

    def __init__(self):
        self.calls = []

    def infer(self, phonemes, lengths, **kw):
        import torch
        self.calls.append(dict(keys=sorted(kw), table=_snapshot(kw.get("row_controls")), noise_scale=kw["noise_scale"],
                               controls=[kw[k] is not None for k in ("duration_control", "pitch_control", "energy_control")],
                               seeds=kw["noise_seed"], ids=phonemes[:, 0].tolist()))
        B = phonemes.shape[0]
        o = (phonemes[:, :1].to(torch.float32) / 1000.0).reshape(B, 1, 1).repeat(1, 1, 8)
        return o, torch.ones(B, 1, 2, dtype=torch.bool), (None,) * 4, None, None, None


def _text():
    from vispeech_amd.text import SymbolTable
    return SymbolTable(["_"] + [f"p{i}" for i in range(1, 40)]), {"x": 1}


def _filelist(i):
    from vispeech_amd.text import parse_filelist_row
    return parse_filelist_row(f"x|u|p{i} p1|1 1|100.0 110.0|10.0 20.0")


def _plain(i, **kw):
    from vispeech_amd.text import request_row
    return request_row("x", [f"p{i}", "p1"], **kw)


F32 = lambda *v: np.asarray(v, np.float32).tolist()


def test_batching_service_builds_the_table_in_request_order():
    from vispeech_amd.service import BatchingSynthesisService
    table, spk = _text()
    net = _RecordingNet()
    svc = BatchingSynthesisService(net, max_batch=4, max_wait_s=30.0, noise_scale=0.5, table=table, spk2id=spk)
    try:
        futs = [svc.submit(_plain(11), 101, duration_scale=1.25, noise_scale=0.25),
                svc.submit(_filelist(12), 102),
                svc.submit(_plain(13, durations=[2, 3]), 103, pitch_scale=0.9, energy_scale=1.5),
                svc.submit(_plain(14), 104),
                # second batch: nobody names a scale and every row carries its controls -> the call the service always made
                svc.submit(_filelist(15), 105), svc.submit(_filelist(16), 106)]
    finally:
        svc.close()
    for i, f in enumerate(futs):
        np.testing.assert_array_equal(f.result(0), np.full(8, round((11 + i) / 1000.0 * 32767.0), dtype="<i2"))
    first, second = net.calls
    assert first["ids"] == [11, 12, 13, 14] and first["seeds"] == [101, 102, 103, 104]
    assert first["table"] == dict(duration_scale=F32(1.25, 1, 1, 1), pitch_scale=F32(1, 1, 0.9, 1), energy_scale=F32(1, 1, 1.5, 1),
                                  noise_scale=F32(0.25, 0.5, 0.5, 0.5),                 # None: the service's noise_scale
                                  given=[[False] * 3, [True] * 3, [True, False, False], [False] * 3])
    assert first["controls"] == [True, True, True]
    assert second["ids"] == [15, 16] and second["table"] is None
    assert second["keys"] == ["duration_control", "energy_control", "isolated", "noise_scale", "noise_seed", "pitch_control", "sid"]
    assert second["controls"] == [True, True, True] and second["noise_scale"] == 0.5


def test_batching_service_passes_no_control_that_no_row_is_given():
    from vispeech_amd.service import BatchingSynthesisService
    table, spk = _text()
    net = _RecordingNet()
    svc = BatchingSynthesisService(net, max_batch=2, max_wait_s=30.0, table=table, spk2id=spk)
    try:
        svc.submit(_plain(21), 1)
        svc.submit(_plain(22, durations=[1, 1]), 2)
    finally:
        svc.close()
    (call,) = net.calls
    assert call["controls"] == [True, False, False]
    assert call["table"]["given"] == [[False] * 3, [True, False, False]] and call["table"]["noise_scale"] == F32(0.667, 0.667)


class _RecordingEngine:
    def __init__(self):
        self.encodes, self.decodes = [], []

    def encode(self, phonemes, lengths, sid, duration, f0, energy, **kw):
        self.encodes.append(dict(keys=sorted(kw), table=_snapshot(kw.get("row_controls")),
                                 controls=[c is not None for c in (duration, f0, energy)], ids=phonemes[:, 0].tolist()))
        B = phonemes.shape[0]
        return {"frame_lengths": [2] * B, "g": np.zeros((B, 1), np.float32)}

    def frame_lengths_host(self, fl):
        return list(fl), max(fl)

    def decode(self, enc, tf, noise, noise_scale, **kw):
        self.decodes.append(dict(keys=sorted(kw), table=_snapshot(kw.get("row_controls")), noise_scale=noise_scale,
                                 seeds=kw["noise_seed"]))
        return {"z": np.zeros((len(enc["frame_lengths"]), 1, tf), np.float32)}

    def generator_stream_rows(self, rows, chunk_frames, pcm=True):
        return np.zeros((len(rows), chunk_frames * 4), np.int16)


class _EngineNet:
    dims = _Dims()

    def __init__(self):
        self._engine = _RecordingEngine()


def test_streaming_service_builds_the_table_per_admitted_group():
    from vispeech_amd.service import StreamingBatchService
    table, spk = _text()
    net = _EngineNet()
    svc = StreamingBatchService(net, max_batch=8, chunk_frames=8, noise_scale=0.5, table=table, spk2id=spk, autostart=False)
    a = svc.submit(_filelist(31), 1, noise_scale=0.0)
    b = svc.submit(_plain(32), 2, duration_scale=2.0)
    svc.step()                                       # one admitted group: the two requests above
    c, d = svc.submit(_filelist(33), 3), svc.submit(_filelist(34), 4)
    svc.close()                                      # ... and the next: no keyword, fully controlled rows
    assert all(len(b"".join(s)) == 2 * 4 * 2 for s in (a, b, c, d))
    eng = net._engine
    want = dict(duration_scale=F32(1, 2), pitch_scale=F32(1, 1), energy_scale=F32(1, 1), noise_scale=F32(0, 0.5),
                given=[[True] * 3, [False] * 3])
    assert eng.encodes[0] == dict(keys=["isolated", "row_controls"], table=want, controls=[True, True, True], ids=[31, 32])
    assert eng.decodes[0] == dict(keys=["isolated", "max_len", "noise_seed", "row_controls"], table=want, noise_scale=0.5, seeds=[1, 2])
    # today's calls, to the keyword
    assert eng.encodes[1] == dict(keys=["isolated"], table=None, controls=[True, True, True], ids=[33, 34])
    assert eng.decodes[1] == dict(keys=["isolated", "max_len", "noise_seed"], table=None, noise_scale=0.5, seeds=[3, 4])


# ------------------------------------------------------------------ argument checks
def test_row_controls_dataclass():
    from vispeech_amd.models import RowControls
    u = RowControls.uniform(3, duration_scale=0.5, noise_scale=0.667, given=(True, False, False))
    assert len(u) == 3 and u.duration_scale.dtype == np.float32 and u.given.dtype == bool
    assert u.duration_scale.tolist() == F32(0.5, 0.5, 0.5) and u.pitch_scale.tolist() == [1.0] * 3
    assert u.noise_scale.tolist() == F32(0.667, 0.667, 0.667) and u.given.tolist() == [[True, False, False]] * 3
    with pytest.raises(ValueError):
        RowControls([1.0, 1.0], [1.0], [1.0, 1.0], [1.0, 1.0], np.zeros((2, 3), bool))
    with pytest.raises(ValueError):
        RowControls([1.0], [1.0], [1.0], [1.0], np.zeros((1, 2), bool))


class _ReadyEngine:
    ready = True


def test_infer_with_a_table_needs_isolated_mode():
    """The check comes before anything touches the device: a model object without a context shows it."""
    import torch
    from vispeech_amd.models import RowControls, SynthesizerTrn
    net = SynthesizerTrn.__new__(SynthesizerTrn)
    net._engine = _ReadyEngine()
    ph, ln, sid = torch.zeros(2, 3, dtype=torch.int64), torch.tensor([3, 2]), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ValueError, match="isolated"):
        net.infer(ph, ln, sid=sid, row_controls=RowControls.uniform(2))
    with pytest.raises(ValueError, match="2 rows"):
        net.infer(ph, ln, sid=sid, row_controls=RowControls.uniform(3), isolated=True)
    with pytest.raises(ValueError, match="duration_control is None"):
        net.infer(ph, ln, sid=sid, row_controls=RowControls.uniform(2, given=(True, False, False)), isolated=True)
    with pytest.raises(ValueError, match="tensor or None"):
        net.infer(ph, ln, sid=sid, pitch_control=1.1, row_controls=RowControls.uniform(2), isolated=True)


def test_engine_refuses_a_table_without_isolated_mode():
    from vispeech_amd.engine import Engine
    from vispeech_amd.models import RowControls
    with pytest.raises(ValueError, match="isolated"):
        Engine._check_row_controls(RowControls.uniform(2), False, 2, 1.0)
    with pytest.raises(ValueError, match="2 rows"):
        Engine._check_row_controls(RowControls.uniform(3), True, 2, 1.0)
    assert Engine._check_row_controls(None, False, 2, 0.3) == 0.3
    assert Engine._check_row_controls(RowControls.uniform(2, noise_scale=0.0), True, 2, 0.3) == 0.0     # nobody draws
    arr = Engine._row_control_array(RowControls([0.5, 1.0], [1.0, 2.0], [1.0, 1.0], [0.0, 0.25], [[1, 0, 1], [0, 1, 0]]))
    assert [(r.duration_scale, r.pitch_scale, r.energy_scale, r.noise_scale, r.given) for r in arr] == [
        (0.5, 1.0, 1.0, 0.0, 5), (1.0, 2.0, 1.0, 0.25, 2)]


def test_sharded_and_pooled_callers_refuse_the_keyword():
    import torch
    from vispeech_amd.models import RowControls
    from vispeech_amd.pipeline import InFlightPool
    from vispeech_amd.sharding import infer_sharded
    ph = torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(ValueError, match="row_controls"):
        infer_sharded(object(), ph, torch.tensor([3, 2]), torch.zeros(2, dtype=torch.int64), frame_counts=[1, 1],
                      isolated=True, row_controls=RowControls.uniform(2))
    pool = InFlightPool.__new__(InFlightPool)
    with pytest.raises(ValueError, match="row_controls"):
        pool.infer(ph, torch.tensor([3, 2]), isolated=True, row_controls=RowControls.uniform(2))


# ------------------------------------------------------------------ the GPU tests' checker against the real reference
def test_oracle_alone_with_row_arguments_matches_the_reference(golden_dir):
    """tests/golden/make_golden_row_controls.py: each utterance run alone by the REAL reference with its own arguments.
    The fixture's margin holds for the oracle's logw too, and the predicted frame counts agree exactly."""
    from oracle.vispeech_oracle import Oracle
    from vispeech_amd.synth import synth_state_dict
    dims = ModelDims()
    oracle = Oracle(synth_state_dict(dims, seed=1234, infer_only=True), dims)
    batch, rows, want = rcr.load_golden(golden_dir)
    assert list(batch["lengths"]) == [2, 5, 9, 9]
    assert rows.given.tolist() == [[True] * 3, [False] * 3, [True, False, False], [False] * 3]
    assert float(rows.noise_scale[0]) == np.float32(0.667) and float(rows.noise_scale[2]) == 1.0 and float(rows.noise_scale[3]) == 0.0
    assert all(float(s[1]) != 1.0 for s in (rows.duration_scale, rows.pitch_scale, rows.energy_scale))
    assert (want["duration"][[1, 3]] <= 0).any() and (want["logw"][[1, 3]] < 0).any()      # the ceil of a negative
    for b in range(4):
        ref, n, L = rcr.alone(oracle, batch, rows, b)
        assert L == int(batch["frame_lengths"][b]) and 1 <= L <= 64
        if not rows.given[b, 0]:
            rcr.assert_margin(want["logw"][b, :n], float(rows.duration_scale[b]))
            rcr.assert_margin(ref["logw"].reshape(-1), float(rows.duration_scale[b]))
        np.testing.assert_array_equal(ref["duration"].reshape(-1), want["duration"][b, :n])
        for k in ("F0", "energy"):
            assert rcr.iso.rel_err(ref[k].reshape(-1), want[k][b, :n]) <= rcr.STAGE_TOL, (b, k)
        for k in ("m_p", "logs_p", "z_p", "z"):
            assert rcr.iso.rel_err(ref[k][0], want[k][b, :, :L]) <= rcr.STAGE_TOL, (b, k)
        assert rcr.iso.rel_err(ref["o"][0], want["o"][b, :, :L * 512]) <= rcr.WAVE_TOL, b
    np.testing.assert_array_equal(want["z_p"][3], want["m_p"][3])                          # noise_scale 0: z_p = m_p exactly
