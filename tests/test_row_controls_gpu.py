"""Per-row controls on the MI355X (``SynthesizerTrn.infer(..., isolated=True, row_controls=...)``, include/vispeech_hip.h
vsp_set_row_controls): every utterance of a batch comes out as the reference computes it ALONE with ITS OWN arguments --
which controls are given, the scales of those that are predicted, its noise scale -- whatever it is batched with.  Checked
against the real reference's alone runs (tests/golden/row_controls.npz) and the CPU oracle run alone per row
(tests/row_controls_ref.py; pinned to the reference by tests/test_row_controls_host.py) at the project's isolated-mode
gates: integers exact, 1e-5 relative per stage, 1e-4 on waveforms, exact zeros behind every extent.
Needs an MI355X: `pytest -m gpu`."""
import numpy as np
import pytest
import torch

import row_controls_ref as rcr
from row_controls_ref import STAGE_TOL, WAVE_TOL, iso

pytestmark = pytest.mark.gpu

UP = 512


def to_np(t):
    return t.detach().cpu().numpy()


def dev(net, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(net.device)


@pytest.fixture(scope="module")
def dims_weights():
    from vispeech_amd import config as vcfg
    from vispeech_amd.schema import dims_from_ctor
    from vispeech_amd.synth import synth_state_dict
    ctor = vcfg.synthesizer_args(vcfg.default_hparams())
    d = dims_from_ctor(*ctor[0], **ctor[1])
    return ctor, d, synth_state_dict(d, seed=1234, infer_only=True)


@pytest.fixture(scope="module")
def net(dims_weights):
    from vispeech_amd.models import SynthesizerTrn
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    ctor, _, sd = dims_weights
    m = SynthesizerTrn(*ctor[0], **ctor[1]).eval()
    m.load_state_dict(sd, strict=True)
    return m


@pytest.fixture(scope="module")
def oracle(dims_weights):
    from oracle.vispeech_oracle import Oracle
    return Oracle(dims_weights[2], dims_weights[1])


@pytest.fixture(scope="module")
def golden(golden_dir):
    return rcr.load_golden(golden_dir)


def controls_for(batch, rows, idx=slice(None)):
    """The three control tensors of a call with a table: None where no row is given one."""
    return [batch[k][idx] if rows.given[:, i].any() else None for i, k in enumerate(("duration", "f0", "energy"))]


def infer(net, batch, rows, idx=slice(None), **kw):
    d, p, e = controls_for(batch, rows, idx)
    return net.infer(dev(net, batch["phonemes"][idx]), dev(net, batch["lengths"][idx]), sid=dev(net, batch["sid"][idx]),
                     duration_control=dev(net, d), pitch_control=dev(net, p), energy_control=dev(net, e), isolated=True,
                     row_controls=rows, **kw)


def check_row(res, b, want, n, L, tag):
    """Row ``b`` of an infer result against ``want`` (duration / F0 / energy [n]; z, z_p, m_p, logs_p [inter, L];
    o [1, L * UP]) on its extent, at the gates; exact zeros behind it."""
    o, x_mask, (z, z_p, m_p, logs_p), duration, f0, energy = res
    B = z.shape[0]
    d = to_np(duration).reshape(B, -1)[b]
    np.testing.assert_array_equal(d[:n], want["duration"])                       # exact: the ceil did not flip
    assert not d[n:].any(), (tag, b, "duration not zero behind the extent")
    np.testing.assert_array_equal(to_np(x_mask)[b, 0], np.arange(x_mask.shape[2]) < L)       # the frame count, exact
    errs = {}
    for k, v in (("z", z), ("z_p", z_p), ("m_p", m_p), ("logs_p", logs_p)):
        a = to_np(v)[b]
        errs[k] = iso.rel_err(a[:, :L], want[k])
        assert not a[:, L:].any(), (tag, b, k, "not zero behind the extent")
    for k, v in (("F0", f0), ("energy", energy)):
        a = to_np(v).reshape(B, -1)[b]
        errs[k] = iso.rel_err(a[:n], want[k])
        assert not a[n:].any(), (tag, b, k, "not zero behind the extent")
    w = to_np(o)[b, 0]
    errs["o"] = iso.rel_err(w[:L * UP], want["o"].reshape(-1))
    assert not w[L * UP:].any(), (tag, b, "o not zero behind the extent")
    print(tag, b, f"n={n} L={L}", {k: f"{v:.1e}" for k, v in errs.items()})
    for k in ("z", "z_p", "m_p", "logs_p", "F0", "energy"):
        assert errs[k] <= STAGE_TOL, (tag, b, k, errs[k])
    assert errs["o"] <= WAVE_TOL, (tag, b, errs["o"])


def golden_row(want, batch, b):
    n, L = int(batch["lengths"][b]), int(batch["frame_lengths"][b])
    w = {k: want[k][b, :n] for k in ("duration", "F0", "energy")}
    w.update({k: want[k][b, :, :L] for k in ("z", "z_p", "m_p", "logs_p")})
    w["o"] = want["o"][b, :, :L * UP]
    return w, n, L


def oracle_row(ref):
    w = {k: ref[k].reshape(-1) for k in ("duration", "F0", "energy")}
    w.update({k: ref[k][0] for k in ("z", "z_p", "m_p", "logs_p")})
    w["o"] = ref["o"][0]
    return w


# ------------------------------------------------------------------ 1. the mixed table against the real reference
def test_mixed_table_equals_the_reference_alone_runs(net, golden):
    """Row 0 all given, row 1 all predicted with its own scales, row 2 durations given, row 3 predicted with noise_scale 0
    (and a predicted duration that is the ceil of a negative): one call, the caller's noise."""
    batch, rows, want = golden
    tf = int(batch["frame_lengths"].max())
    res = infer(net, batch, rows, noise=dev(net, batch["noise"][:, :, :tf]))
    assert res[0].shape == (4, 1, tf * UP) and res[2][0].shape == (4, 192, tf)
    for b in range(4):
        check_row(res, b, *golden_row(want, batch, b), "golden")
    np.testing.assert_array_equal(to_np(res[2][1])[3], to_np(res[2][2])[3])      # noise_scale 0: z_p = m_p exactly
    assert net._engine.status() == 0


# ------------------------------------------------------------------ 2. position and company
def test_rows_do_not_depend_on_position_or_company(net, golden, oracle):
    """The fixture's rows permuted, and a fifth utterance (12 phonemes: another T_p; 30 frames: another T_f) appended."""
    batch, rows, want = golden
    perm = [2, 0, 3, 1]
    extra = iso.make_batch([30], [12], seed=77)
    tp, tf = 12, 30
    pad = lambda a, fill: np.concatenate([a, np.full((a.shape[0], tp - a.shape[1]), fill, a.dtype)], axis=1)
    b5 = dict(phonemes=np.concatenate([pad(batch["phonemes"][perm], 3), extra["phonemes"]]),
              lengths=np.concatenate([batch["lengths"][perm], extra["lengths"]]),
              sid=np.concatenate([batch["sid"][perm], extra["sid"]]),
              duration=np.concatenate([pad(batch["duration"][perm], 7.0), extra["duration"]]),
              f0=np.concatenate([pad(batch["f0"][perm], 333.0), extra["f0"]]),
              energy=np.concatenate([pad(batch["energy"][perm], 77.0), extra["energy"]]),
              noise=np.concatenate([batch["noise"][perm][:, :, :tf], extra["noise"][:, :, :tf]]))
    r5 = rcr.table(*[np.concatenate([getattr(rows, k)[perm], [v]]) for k, v in
                     (("duration_scale", 1.0), ("pitch_scale", 1.3), ("energy_scale", 1.0), ("noise_scale", 0.8))],
                   np.concatenate([rows.given[perm], [[True, False, True]]]))
    res = infer(net, b5, r5, noise=dev(net, b5["noise"]))
    assert res[0].shape == (5, 1, tf * UP)
    for pos, b in enumerate(perm):
        check_row(res, pos, *golden_row(want, batch, b), f"permuted (row {b})")
    ref, n, L = rcr.alone(oracle, b5, r5, 4)
    assert (n, L) == (12, 30)
    check_row(res, 4, oracle_row(ref), n, L, "fifth")


# ------------------------------------------------------------------ 3. a uniform table is the scalar call, bit for bit
@pytest.mark.parametrize("given", [(False, False, False), (True, False, False), (True, True, True)])
def test_uniform_table_equals_the_scalar_call_bit_for_bit(net, golden, given):
    from vispeech_amd.models import RowControls
    batch, _, _ = golden
    scales = dict(duration_scale=0.6, pitch_scale=1.15, energy_scale=0.85, noise_scale=0.4)
    seeds = [11, 12, 13, 14]
    t = lambda k: dev(net, batch[k])
    scalar = net.infer(t("phonemes"), t("lengths"), sid=t("sid"), noise_scale=scales["noise_scale"],
                       duration_control=t("duration") if given[0] else scales["duration_scale"],
                       pitch_control=t("f0") if given[1] else scales["pitch_scale"],
                       energy_control=t("energy") if given[2] else scales["energy_scale"], isolated=True, noise_seed=seeds)
    table = infer(net, batch, RowControls.uniform(4, given=given, **scales), noise_seed=seeds)
    flat = lambda r: [r[0], r[1], *r[2], r[4], r[5]]
    names = ["o", "x_mask", "z", "z_p", "m_p", "logs_p", "F0", "energy"]
    for k, a, b in zip(names, flat(scalar), flat(table)):
        assert a.shape == b.shape and torch.equal(a, b), k
    # (the scalar call hands a duration TENSOR back as it came, garbage behind `lengths` included: the extents compare)
    ds, dt = to_np(scalar[3]).reshape(4, -1), to_np(table[3]).reshape(4, -1)
    for b, n in enumerate(batch["lengths"]):
        np.testing.assert_array_equal(ds[b, :n], dt[b, :n])
    assert float(to_np(scalar[0]).std()) > 1e-4


# ------------------------------------------------------------------ 4. more than one 64-wide block per row
TP70 = dict(lengths=[70, 33, 65], duration_scale=[0.05, 0.1, 0.03], pitch_scale=[0.9, 1.0, 1.2], energy_scale=[1.1, 1.0, 0.8],
            noise_scale=[0.667, 0.3, 1.0], given=[[False, False, False], [False, False, True], [False, True, False]], seed=7001)


def test_predicted_durations_with_a_scale_per_row_tp70(net, oracle):
    """B = 3, T_p = 70: every row's durations predicted with its own duration_scale, against the oracle alone per row.
    The margin of the golden fixture is asserted on the oracle's logw first: a condition on the inputs."""
    c = TP70
    r = np.random.Generator(np.random.PCG64(c["seed"]))
    B, tp = 3, 70
    batch = dict(phonemes=r.integers(1, 200, size=(B, tp)).astype(np.int64), lengths=np.asarray(c["lengths"], np.int64),
                 sid=r.integers(0, 67, size=B).astype(np.int64), f0=r.uniform(150.0, 400.0, size=(B, tp)).astype(np.float32),
                 energy=r.uniform(0.0, 100.0, size=(B, tp)).astype(np.float32),
                 noise=r.standard_normal((B, 192, 256), dtype=np.float32))
    rows = rcr.table(c["duration_scale"], c["pitch_scale"], c["energy_scale"], c["noise_scale"], c["given"])
    refs = [rcr.alone(oracle, batch, rows, b) for b in range(B)]
    for b, (ref, n, L) in enumerate(refs):
        rcr.assert_margin(ref["logw"].reshape(-1), c["duration_scale"][b])
        assert 1 <= L <= 256 and n == c["lengths"][b]
        print(f"tp70 row {b}: {L} frames, durations {int(ref['duration'].min())} .. {int(ref['duration'].max())}")
    tf = max(L for _, _, L in refs)
    res = infer(net, batch, rows, noise=dev(net, batch["noise"][:, :, :tf]))
    np.testing.assert_array_equal(to_np(res[1]).sum(axis=(1, 2)), [L for _, _, L in refs])
    for b, (ref, n, L) in enumerate(refs):
        check_row(res, b, oracle_row(ref), n, L, "tp70")


# ------------------------------------------------------------------ 5. the one-call form
def test_one_call_form_equals_encode_plus_decode(net, golden):
    batch, rows, _ = golden
    idx = [1, 2]
    r2 = rcr.take(rows, idx)
    eng = net._engine
    ph, ln, sid = (dev(net, batch[k][idx]) for k in ("phonemes", "lengths", "sid"))
    d, p, e = (dev(net, c) for c in controls_for(batch, r2, idx))
    enc = eng.encode(ph, ln, sid, d, p, e, isolated=True, row_controls=r2)
    frames, tf = eng.frame_lengths_host(enc["frame_lengths"])
    assert frames == [int(batch["frame_lengths"][b]) for b in idx]
    noise = dev(net, batch["noise"][idx][:, :, :tf])
    dec = eng.decode(enc, tf, noise, 123.0, isolated=True, row_controls=r2)       # (the scalar is not read)
    one = eng.infer_padded(ph, ln, sid, tf, noise, noise_scale=456.0, duration_ctl=d, pitch_ctl=p, energy_ctl=e,
                           duration_scale=9.0, pitch_scale=9.0, energy_scale=9.0, isolated=True, row_controls=r2)
    for k in ("o", "x_mask", "z", "z_p", "m_p", "logs_p"):
        assert torch.equal(one[k], dec[k]), k
    for k in ("duration", "F0", "energy", "frame_lengths"):
        assert torch.equal(one[k], enc[k]), k
    # ... and a table the next call does not pass is forgotten: the scalar call after it is the scalar call
    plain = eng.encode(ph, ln, sid, d, None, None, 1.0, float(r2.pitch_scale[0]), float(r2.energy_scale[0]), isolated=True)
    assert torch.equal(plain["duration"], d * (torch.arange(d.shape[1], device=d.device)[None, :] < ln[:, None]))


# ------------------------------------------------------------------ 6. noise the library draws
def test_library_drawn_noise_per_row(net, golden):
    batch, rows, _ = golden
    seeds = [901, 902, 903, 904]
    res = infer(net, batch, rows, noise_seed=seeds)
    z_p, m_p = to_np(res[2][1]), to_np(res[2][2])
    np.testing.assert_array_equal(z_p[3], m_p[3])                                 # noise_scale 0
    assert np.abs(z_p[1] - m_p[1]).max() > 1e-3                                   # ... and a row that draws
    for b in (0, 1):          # all given, noise_scale 0.667; all predicted, its own scales and noise_scale
        n = int(batch["lengths"][b])
        sl = slice(b, b + 1)
        d, p, e, ns = rcr.row_arguments(batch, rows, b, n)
        ctl = lambda c: dev(net, c) if isinstance(c, np.ndarray) else c
        alone = net.infer(dev(net, batch["phonemes"][sl, :n]), dev(net, batch["lengths"][sl]), sid=dev(net, batch["sid"][sl]),
                          noise_scale=ns, duration_control=ctl(d), pitch_control=ctl(p), energy_control=ctl(e),
                          isolated=True, noise_seed=[seeds[b]])
        L = int(to_np(alone[1]).sum())
        assert L == int(batch["frame_lengths"][b])
        want = dict(duration=to_np(alone[3]).reshape(-1), F0=to_np(alone[4]).reshape(-1), energy=to_np(alone[5]).reshape(-1),
                    o=to_np(alone[0])[0], **{k: to_np(v)[0] for k, v in zip(("z", "z_p", "m_p", "logs_p"), alone[2])})
        check_row(res, b, want, n, L, "drawn")


# ------------------------------------------------------------------ 7. the services
def _requests(batch):
    """The fixture's utterances as service requests (phones named by their ids): 0 a filelist row, 1 and 3 plain, 2 with
    durations, and 4 = request 1 again with another duration_scale."""
    from vispeech_amd.text import SymbolTable, request_row
    table = SymbolTable([str(i) for i in range(519)])
    spk = {str(i): i for i in range(67)}

    def row(b, dur=False, rest=False):
        n = int(batch["lengths"][b])
        return request_row(str(int(batch["sid"][b])), [str(int(x)) for x in batch["phonemes"][b, :n]],
                           durations=batch["duration"][b, :n] if dur else None, f0=batch["f0"][b, :n] if rest else None,
                           energy=batch["energy"][b, :n] if rest else None)
    reqs = [(row(0, True, True), 501, {}),
            (row(1), 502, dict(duration_scale=0.6, pitch_scale=1.15, energy_scale=0.85, noise_scale=0.4)),
            (row(2, True), 503, dict(pitch_scale=0.9, energy_scale=1.2, noise_scale=1.0)),
            (row(3), 504, dict(noise_scale=0.0)),
            (row(1), 502, dict(duration_scale=1.2, pitch_scale=1.15, energy_scale=0.85, noise_scale=0.4))]
    return table, spk, reqs


def _one_infer(net, table, spk, reqs, service_noise_scale):
    """pcm16 per request of the ONE isolated infer with the same rows, seeds and table."""
    from vispeech_amd.service import pcm16
    from vispeech_amd.text import collate_rows
    batch = collate_rows([r for r, _, _ in reqs], table, spk)
    sc = lambda k, default: [kw.get(k, default) for _, _, kw in reqs]
    rows = rcr.table(sc("duration_scale", 1.0), sc("pitch_scale", 1.0), sc("energy_scale", 1.0),
                     sc("noise_scale", service_noise_scale), batch["given"])
    res = infer(net, batch, rows, noise_seed=[s for _, s, _ in reqs])
    frames = to_np(res[1]).sum(axis=(1, 2))
    return [pcm16(res[0][b, 0, : int(frames[b]) * UP]) for b in range(len(reqs))]


def test_batching_service_serves_mixed_requests(net, golden):
    from vispeech_amd.service import BatchingSynthesisService
    table, spk, reqs = _requests(golden[0])
    want = _one_infer(net, table, spk, reqs, 0.667)
    svc = BatchingSynthesisService(net, max_batch=len(reqs), max_wait_s=30.0, noise_scale=0.667, table=table, spk2id=spk)
    try:
        got = [f.result(120) for f in [svc.submit(r, s, **kw) for r, s, kw in reqs]]
    finally:
        svc.close()
    for b in range(len(reqs)):
        np.testing.assert_array_equal(got[b], want[b])
    assert got[0].shape == (14 * UP,) and got[1].shape == (16 * UP,) and got[2].shape == (24 * UP,) and got[3].shape == (19 * UP,)
    assert got[4].shape != got[1].shape and got[4].size > 0          # the same request, another duration_scale


def test_streaming_service_serves_mixed_requests(net, golden):
    from vispeech_amd.service import StreamingBatchService
    table, spk, reqs = _requests(golden[0])
    want = _one_infer(net, table, spk, reqs, 0.667)
    svc = StreamingBatchService(net, max_batch=8, chunk_frames=8, noise_scale=0.667, table=table, spk2id=spk, autostart=False)
    streams = [svc.submit(r, s, **kw) for r, s, kw in reqs]           # one admitted group: the rows of the one infer
    svc.close()
    got = [np.frombuffer(b"".join(s), dtype="<i2") for s in streams]
    assert svc.stats["groups"] == 1 and svc.stats["rows_per_tick"][0] == len(reqs)
    for b in range(len(reqs)):
        assert got[b].shape == want[b].shape, b
        print(f"request {b}: worst {int(np.abs(got[b].astype(np.int64) - want[b].astype(np.int64)).max())} PCM16 steps from the one infer")
    for b in range(len(reqs)):
        np.testing.assert_array_equal(got[b], want[b])
    assert got[4].shape != got[1].shape
