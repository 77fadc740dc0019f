"""Isolated mode, host side (no GPU): the effect it removes is large enough for the project's gate to see; the CPU oracle
run one utterance at a time agrees with the REAL reference run that way (tests/golden/isolated.npz); the batching
service groups requests, keeps their order and their failures apart; the argument checks."""
import os
import numpy as np
import pytest

import isolated_ref as iso

WAVE_TOL, STAGE_TOL = 1e-4, 1e-5      # the project's gates (tests/test_hip_parity.py)


@pytest.fixture(scope="module")
def dims():
    from vispeech_amd.schema import ModelDims
    return ModelDims()


@pytest.fixture(scope="module")
def oracle(dims):
    from oracle.vispeech_oracle import Oracle
    from vispeech_amd.synth import synth_state_dict
    return Oracle(synth_state_dict(dims, seed=1234, infer_only=True), dims)


def test_padded_batch_differs_from_alone_runs_far_beyond_the_gate(oracle):
    """SURVEY gotcha G5, measured: in the reference's padded batch a shorter utterance's waveform differs from its alone
    run by 0.3-0.5 of the peak -- more than 100x the 1e-4 * max gate the GPU tests hold isolated mode to."""
    from vispeech_amd.synth import synth_batch
    b = synth_batch(3, seed=7, mean_phonemes=10, std_phonemes=2, min_phonemes=6, max_phonemes=14, mean_frames=24,
                    jitter_frames=10)
    assert list(b["lengths"]) == [10, 11, 9] and list(b["frame_lengths"]) == [23, 19, 24]
    pad = iso.padded(oracle, b, "controls")["o"].numpy()
    worst = 0.0
    for u in range(3):
        ref, n, L = iso.alone(oracle, b, u, "controls")
        ratio = np.abs(pad[u, 0, :L * 512] - ref["o"][0, 0]).max() / np.abs(ref["o"]).max()
        print(f"utterance {u}: padded vs alone = {ratio:.3f} of the peak")
        worst = max(worst, ratio)
    assert worst > 100 * WAVE_TOL


@pytest.mark.parametrize("mode", ["controls", "predictors"])
def test_oracle_alone_matches_the_reference_alone(oracle, golden_dir, mode):
    """The checker of the GPU tests against the real reference, B = 1 per utterance (tests/golden/make_golden_isolated.py),
    with tests/test_oracle_golden.py's tolerances."""
    g = np.load(os.path.join(golden_dir, "isolated.npz"))
    batch = {k[3:]: g[k] for k in g.files if k.startswith("in_")}
    assert list(batch["frame_lengths"]) == [1, 14, 40, 41] and list(batch["lengths"]) == [2, 5, 9, 9]
    for b in range(4):
        ref, n, L = iso.alone(oracle, batch, b, mode, noise_scale=float(g["in_noise_scale"]))
        assert L == int(batch["frame_lengths"][b])
        np.testing.assert_array_equal(ref["duration"].reshape(-1), g[f"{mode}_duration"][b, :n])
        for k in ("F0", "energy"):
            assert iso.rel_err(ref[k].reshape(-1), g[f"{mode}_{k}"][b, :n]) <= STAGE_TOL, (b, k)
        for k in ("m_p", "logs_p", "z"):
            assert iso.rel_err(ref[k][0], g[f"{mode}_{k}"][b, :, :L]) <= STAGE_TOL, (b, k)
        assert iso.rel_err(ref["o"][0], g[f"{mode}_o"][b, :, :L * 512]) <= WAVE_TOL, b


# ------------------------------------------------------------------ BatchingSynthesisService on a recording fake net
class _Dims:
    total_upsample = 4
    inter_channels = 2


class _FakeNet:
    """Records every infer call; utterance b's waveform is its first phoneme id repeated over its frames / 1000."""
    device = "cpu"
    dims = _Dims()

    def __init__(self, fail_on=None):
        self.calls, self.fail_on = [], fail_on

    def infer(self, phonemes, lengths, sid=None, noise_scale=1, duration_control=None, pitch_control=None,
              energy_control=None, noise_seed=None, isolated=False, **kw):
        import torch
        self.calls.append(dict(B=int(phonemes.shape[0]), seeds=noise_seed, isolated=isolated, ids=phonemes[:, 0].tolist()))
        if self.fail_on is not None and self.fail_on in phonemes[:, 0].tolist():
            raise RuntimeError("boom")
        frames = duration_control.sum(dim=1).to(torch.int64)
        tf = int(frames.max())
        o = torch.zeros(phonemes.shape[0], 1, tf * 4)
        mask = torch.zeros(phonemes.shape[0], 1, tf, dtype=torch.bool)
        for b in range(phonemes.shape[0]):
            o[b, 0, : int(frames[b]) * 4] = float(phonemes[b, 0]) / 1000.0
            mask[b, 0, : int(frames[b])] = True
        return o, mask, (None,) * 4, duration_control, None, None


def _collate(rows):
    tp = max(len(r["ph"]) for r in rows)
    out = dict(phonemes=np.zeros((len(rows), tp), np.int64), lengths=np.zeros(len(rows), np.int64),
               sid=np.zeros(len(rows), np.int64), duration=np.zeros((len(rows), tp), np.float32))
    for b, r in enumerate(rows):
        out["phonemes"][b, : len(r["ph"])] = r["ph"]
        out["lengths"][b] = len(r["ph"])
        out["duration"][b, : len(r["ph"])] = r["dur"]
    return out


def _row(first_id, frames):
    return dict(ph=[first_id, 5], dur=[frames, 0])


def _expected(first_id, frames):
    return np.full(frames * 4, round(first_id / 1000.0 * 32767.0), dtype="<i2")


def test_batching_service_groups_requests_and_keeps_order():
    """max_wait_s is long here: a batch closes when it is full, the last one when close() drains the queue."""
    from vispeech_amd.service import BatchingSynthesisService
    net = _FakeNet()
    svc = BatchingSynthesisService(net, max_batch=3, max_wait_s=30.0, collate=_collate)
    try:
        futs = [svc.submit(_row(20 + i, 2 + i), noise_seed=200 + i) for i in range(5)]
    finally:
        svc.close()
    assert not svc._worker.is_alive()
    for i, f in enumerate(futs):
        np.testing.assert_array_equal(f.result(0), _expected(20 + i, 2 + i))           # each its own utterance's samples
    assert all(c["isolated"] is True for c in net.calls)
    assert [c["B"] for c in net.calls] == [3, 2]                                       # grouped up to max_batch, in order
    assert [c["seeds"] for c in net.calls] == [[200, 201, 202], [203, 204]]           # per-utterance seeds, as a sequence
    assert [c["ids"] for c in net.calls] == [[20, 21, 22], [23, 24]]


def test_batching_service_lone_request_leaves_after_max_wait():
    from vispeech_amd.service import BatchingSynthesisService
    net = _FakeNet()
    svc = BatchingSynthesisService(net, max_batch=8, max_wait_s=0.02, collate=_collate)
    try:
        np.testing.assert_array_equal(svc.submit(_row(7, 3), noise_seed=1).result(10), _expected(7, 3))
    finally:
        svc.close()
    assert net.calls == [dict(B=1, seeds=[1], isolated=True, ids=[7])]


def test_batching_service_failure_stays_in_its_batch():
    from vispeech_amd.service import BatchingSynthesisService
    net = _FakeNet(fail_on=66)
    svc = BatchingSynthesisService(net, max_batch=1, max_wait_s=0.0, collate=_collate)
    try:
        bad, good = svc.submit(_row(66, 2), noise_seed=1), svc.submit(_row(8, 2), noise_seed=2)
        with pytest.raises(RuntimeError, match="boom"):
            bad.result(10)
        np.testing.assert_array_equal(good.result(10), _expected(8, 2))
    finally:
        svc.close()
    with pytest.raises(RuntimeError, match="closed"):
        svc.submit(_row(1, 1), noise_seed=0)
    svc.close()                                                                        # (idempotent)


# ------------------------------------------------------------------ argument checks
def test_isolated_needs_one_seed_per_utterance():
    from vispeech_amd.engine import Engine
    with pytest.raises(ValueError, match="one noise_seed per utterance"):
        Engine._isolated_seeds(True, None, 0.667, 5, 3)
    with pytest.raises(ValueError, match="3 entries"):
        Engine._isolated_seeds(True, None, 0.667, [1, 2], 3)
    with pytest.raises(ValueError, match="isolated=True"):
        Engine._isolated_seeds(False, None, 0.667, [1, 2, 3], 3)
    assert Engine._isolated_seeds(True, None, 0.667, [1, 2, 3], 3) == (0, [1, 2, 3])
    assert Engine._isolated_seeds(False, None, 0.667, 9, 3) == (9, None)


def test_infer_refuses_a_plain_int_seed_in_isolated_mode():
    """Through SynthesizerTrn.infer itself (an engine stub: the check runs before anything is launched)."""
    import torch
    from vispeech_amd.engine import Engine
    from vispeech_amd.models import SynthesizerTrn

    class Stub:
        ready = True
        _isolated_seeds = staticmethod(Engine._isolated_seeds)

        def encode(self, *a, **k):
            raise AssertionError("nothing may run before the argument check")

    net = SynthesizerTrn.__new__(SynthesizerTrn)
    net._engine = Stub()
    with pytest.raises(ValueError, match="one noise_seed per utterance"):
        net.infer(torch.zeros(2, 3, dtype=torch.int64), torch.tensor([3, 2]), sid=torch.tensor([0, 1]), noise_seed=4, isolated=True)


def test_isolated_without_noise_or_seeds_draws_with_torch_as_the_default_mode_does():
    """No `noise`, no `noise_seed`: the draw is torch.randn in either mode -- decode receives a [B, inter, T_f] tensor."""
    import torch
    from vispeech_amd.engine import Engine
    from vispeech_amd.models import SynthesizerTrn
    seen = {}

    class Dims:
        inter_channels = 6

    class Stub:
        ready, device = True, "cpu"
        _isolated_seeds = staticmethod(Engine._isolated_seeds)

        def encode(self, ph, *a, **k):
            seen.setdefault("encode", []).append(k.get("isolated", False))
            return dict(frame_lengths=None, duration=torch.zeros(2, 3), F0=None, energy=None)

        def decode_buffers(self, *a):
            return None

        def frame_lengths_host(self, fl):
            return [4, 5], 5

        def decode(self, enc, Tf, noise, ns, max_len, noise_seed=None, bufs=None, noise_offset=0, isolated=False):
            Engine._isolated_seeds(isolated, noise, ns, noise_seed, 2)        # (what the real decode checks first)
            seen.setdefault("decode", []).append((isolated, None if noise is None else tuple(noise.shape), noise_seed))
            return dict(o=None, x_mask=None, z=None, z_p=None, m_p=None, logs_p=None)

    net = SynthesizerTrn.__new__(SynthesizerTrn)
    net._engine, net.dims = Stub(), Dims()
    for isolated in (False, True):
        net.infer(torch.zeros(2, 3, dtype=torch.int64), torch.tensor([3, 2]), sid=torch.tensor([0, 1]), noise_scale=0.667,
                  isolated=isolated)
    assert seen["encode"] == [False, True]
    assert seen["decode"] == [(False, (2, 6, 5), 0), (True, (2, 6, 5), None)]
    # ... and seeds, when given, go to the library instead of a torch draw
    net.infer(torch.zeros(2, 3, dtype=torch.int64), torch.tensor([3, 2]), sid=torch.tensor([0, 1]), noise_seed=[8, 9], isolated=True)
    assert seen["decode"][-1] == (True, None, [8, 9])


def test_infer_sharded_slices_per_utterance_seeds_once(monkeypatch):
    """Rank 1 of 2 gets ITS utterances' seeds, whether the global sequence is a list or a [B] tensor."""
    import types
    import torch
    from vispeech_amd import sharding
    monkeypatch.setattr(sharding, "_active", lambda: True)
    monkeypatch.setattr(sharding, "dist", types.SimpleNamespace(get_rank=lambda g=None: 1, get_world_size=lambda g=None: 2))
    monkeypatch.setattr(sharding, "global_max", lambda v, *a, **k: int(v))
    monkeypatch.setattr(sharding, "gather_batch", lambda *a, **k: None)
    calls = []

    class Net:
        dims = types.SimpleNamespace(inter_channels=2)

        def infer(self, ph, ln, **kw):
            calls.append(dict(B=ph.shape[0], seeds=kw["noise_seed"], isolated=kw["isolated"], offset=kw.get("noise_offset")))
            return (torch.zeros(ph.shape[0], 1, 4),)
    ph, ln, sid = torch.zeros(5, 3, dtype=torch.int64), torch.full((5,), 3), torch.zeros(5, dtype=torch.int64)
    for seeds in ([10, 11, 12, 13, 14], torch.tensor([10, 11, 12, 13, 14])):
        sharding.infer_sharded(Net(), ph, ln, sid, frame_counts=[4] * 5, noise_seed=seeds, isolated=True)
    assert calls == [dict(B=2, seeds=[13, 14], isolated=True, offset=None)] * 2


def test_library_exports_the_isolated_entry_points():
    import ctypes as C
    from vispeech_amd import _lib
    lib = _lib.lib()
    for name in ("vsp_set_isolated", "vsp_get_isolated", "vsp_set_noise_seeds", "vsp_generator_ragged"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    cfg = _lib.make_config(__import__("vispeech_amd.schema", fromlist=["ModelDims"]).ModelDims())
    h = C.c_void_p()
    assert lib.vsp_create(C.byref(cfg), 0, C.byref(h)) == 0
    try:
        assert lib.vsp_get_isolated(h) == 0                          # off on a fresh context
        assert lib.vsp_set_isolated(h, 1) == 0 and lib.vsp_get_isolated(h) == 1
        assert lib.vsp_set_isolated(h, 0) == 0 and lib.vsp_get_isolated(h) == 0
        seeds = (C.c_uint64 * 2)(1, 2)
        assert lib.vsp_set_noise_seeds(h, seeds, 2) == 0 and lib.vsp_set_noise_seeds(h, None, 0) == 0
        assert lib.vsp_set_noise_seeds(h, None, 2) == -1 and lib.vsp_set_noise_seeds(h, seeds, -1) == -1
        assert lib.vsp_set_isolated(None, 1) == -1 and lib.vsp_get_isolated(None) == -1
        rc = lib.vsp_generator_ragged(h, None, 1, 8, C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), 1 << 20)
        assert rc == -2 and b"not finalised" in lib.vsp_last_error(h)
    finally:
        lib.vsp_destroy(h)
