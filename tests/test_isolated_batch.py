"""Isolated mode on the MI355X (``SynthesizerTrn.infer(..., isolated=True)``, include/vispeech_hip.h vsp_set_isolated):
every utterance of a padded batch comes out as the reference computes it ALONE -- B = 1, its unpadded inputs -- whatever
it is batched with, and every float output is exactly 0 behind the utterance's extent.  The checker is the CPU oracle run
one utterance at a time (tests/isolated_ref.py; pinned to the real reference by tests/test_isolated_host.py), at the
project's gates: 1e-4 * max|ref| on waveforms, 1e-5 relative per stage, integers exact.  Needs an MI355X: `pytest -m gpu`."""
import os

import numpy as np
import pytest
import torch

import isolated_ref as iso

pytestmark = pytest.mark.gpu

STAGE_TOL, WAVE_TOL = 1e-5, 1e-4
# 28 = the smallest per-utterance extent the generator kernels met before this mode (0 + 13 + 1 + 13), 64 / 65 sit either side
# of the 64-column tile, 150 = the padded length (one utterance untrimmed)
FRAMES = [1, 2, 13, 14, 27, 28, 63, 64, 65, 150]
PHONEMES = [2, 5, 9, 12, 2, 5, 9, 12, 5, 12]           # T_p = 12


def to_np(t):
    return t.detach().cpu().numpy()


def dev(net, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(net.device) if isinstance(a, np.ndarray) else a


def ctor_for(**model):
    from vispeech_amd import config as vcfg
    hp = vcfg.default_hparams()
    for k, v in model.items():
        hp.model[k] = v
    return vcfg.synthesizer_args(hp)


def make_net(ctor, weights, **env):
    from vispeech_amd.models import SynthesizerTrn
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    mp = pytest.MonkeyPatch()
    for k, v in env.items():
        mp.setenv(k, v)
    try:
        m = SynthesizerTrn(*ctor[0], **ctor[1]).eval()     # (the VSP_* switches are read when the context is created)
    finally:
        mp.undo()
    m.load_state_dict(weights, strict=True)
    return m


def weights_of(ctor):
    from vispeech_amd.schema import dims_from_ctor
    from vispeech_amd.synth import synth_state_dict
    d = dims_from_ctor(*ctor[0], **ctor[1])
    return d, synth_state_dict(d, seed=1234)               # (with the posterior encoder: voice conversion)


@pytest.fixture(scope="module")
def ctor():
    return ctor_for()


@pytest.fixture(scope="module")
def dims_weights(ctor):
    return weights_of(ctor)


@pytest.fixture(scope="module")
def net(ctor, dims_weights):
    return make_net(ctor, dims_weights[1])


@pytest.fixture(scope="module")
def oracle(dims_weights):
    from oracle.vispeech_oracle import Oracle
    return Oracle(dims_weights[1], dims_weights[0])


def run(net, batch, mode, sl=slice(None), isolated=True, noise_scale=0.667, **kw):
    d, p, e = iso.controls(batch, mode, sl)
    if "noise" not in kw and "noise_seed" not in kw:
        kw["noise"] = dev(net, batch["noise"][sl])
    return net.infer(dev(net, batch["phonemes"][sl]), dev(net, batch["lengths"][sl]), sid=dev(net, batch["sid"][sl]),
                     noise_scale=noise_scale, duration_control=dev(net, d), pitch_control=dev(net, p),
                     energy_control=dev(net, e), isolated=isolated, **kw)


def check_utterance(res, b, ref, n, L, up, tag, max_len=None):
    """Utterance ``b`` of an infer result against its alone reference on its extent; exact zeros behind it."""
    o, x_mask, (z, z_p, m_p, logs_p), duration, f0, energy = res
    Lw = L if max_len is None else min(L, max_len)
    errs = {}
    for k, v in (("z", z), ("z_p", z_p), ("m_p", m_p), ("logs_p", logs_p)):
        a = to_np(v)[b]
        errs[k] = iso.rel_err(a[:, :L], ref[k][0])
        assert not a[:, L:].any(), (tag, b, k, "not zero behind the extent")
    for k, v in (("F0", f0), ("energy", energy)):
        a = to_np(v).reshape(z.shape[0], -1)[b]
        errs[k] = iso.rel_err(a[:n], ref[k].reshape(-1))
        assert not a[n:].any(), (tag, b, k, "not zero behind the extent")
    w = to_np(o)[b, 0]
    errs["o"] = iso.rel_err(w[:Lw * up], ref["o"][0, 0])
    assert not w[Lw * up:].any(), (tag, b, "o not zero behind the extent")
    np.testing.assert_array_equal(to_np(x_mask)[b, 0], np.arange(x_mask.shape[2]) < L)
    print(tag, b, f"n={n} L={L}", {k: f"{v:.1e}" for k, v in errs.items()})
    for k in ("z", "z_p", "m_p", "logs_p", "F0", "energy"):
        assert errs[k] <= STAGE_TOL, (tag, b, k, errs[k])
    assert errs["o"] <= WAVE_TOL, (tag, b, errs["o"])
    return errs


# ------------------------------------------------------------------ 1. end to end
@pytest.fixture(scope="module")
def e2e_batch():
    return iso.make_batch(FRAMES, PHONEMES, seed=2001)


@pytest.fixture(scope="module")
def e2e_refs(oracle, e2e_batch):
    """The alone runs, computed once per (mode, utterance) and shared."""
    cache = {}

    def get(mode, b):
        if (mode, b) not in cache:
            cache[(mode, b)] = iso.alone(oracle, e2e_batch, b, mode)
        return cache[(mode, b)]
    return get


@pytest.mark.parametrize("mode", ["controls", "predictors"])
def test_every_utterance_equals_its_alone_run(net, e2e_batch, e2e_refs, mode):
    """"controls": every control a tensor; "predictors": pitch and energy PREDICTED (scalar controls), durations given --
    they are what fixes the frame counts.  Control tensors hold non-zero garbage behind `lengths`."""
    up = net.dims.total_upsample
    res = run(net, e2e_batch, mode)
    assert res[0].shape == (len(FRAMES), 1, 150 * up) and res[2][0].shape[2] == 150
    dur = to_np(res[3]).reshape(len(FRAMES), -1) if mode != "controls" else None
    for b in range(len(FRAMES)):
        ref, n, L = e2e_refs(mode, b)
        assert L == FRAMES[b]
        check_utterance(res, b, ref, n, L, up, mode)
    # the engine's own duration output (the shim hands a duration TENSOR back as it came)
    enc = net._engine.encode(dev(net, e2e_batch["phonemes"]), dev(net, e2e_batch["lengths"]), dev(net, e2e_batch["sid"]),
                             dev(net, e2e_batch["duration"]), isolated=True)
    d = to_np(enc["duration"])
    for b, n in enumerate(PHONEMES):
        np.testing.assert_array_equal(d[b, :n], e2e_batch["duration"][b, :n])
        assert not d[b, n:].any() and not to_np(enc["x_var"])[b, :, n:].any()
    np.testing.assert_array_equal(to_np(enc["frame_lengths"]), FRAMES)
    assert dur is None or dur.shape == (len(FRAMES), 12)


@pytest.mark.parametrize("mode", ["controls", "predictors"])
def test_default_mode_is_the_padded_batch_not_the_alone_run(net, e2e_batch, e2e_refs, mode):
    """The same inputs with isolated=False: the reference's padded call, which differs from the alone runs beyond the gate
    (here also because the garbage durations behind `lengths` count as frames there)."""
    up = net.dims.total_upsample
    tf = int((e2e_batch["duration"].sum(axis=1)).max())                 # (the padded call's own frame count)
    noise = np.pad(e2e_batch["noise"], ((0, 0), (0, 0), (0, tf - 150)))  # every utterance keeps its own noise columns
    o = to_np(run(net, e2e_batch, mode, isolated=False, noise=dev(net, noise))[0])
    worst = 0.0
    for b in range(len(FRAMES)):
        ref, n, L = e2e_refs(mode, b)
        m = min(L * up, o.shape[2])
        worst = max(worst, iso.rel_err(o[b, 0, :m], ref["o"][0, 0, :m]))
    assert worst > WAVE_TOL, worst


def test_predicted_durations(net, oracle):
    """Every predictor on: the frame counts are the duration predictor's (masked like the alone call's), so T_f is the
    library's; noise_scale 0."""
    batch = iso.make_batch([4, 4, 4, 4], [3, 7, 12, 5], seed=2002, t_f=200)
    res = run(net, batch, "all_predicted", noise_scale=0.0, noise=None)
    dur = to_np(res[3]).reshape(4, -1)
    for b in range(4):
        ref, n, L = iso.alone(oracle, batch, b, "all_predicted", noise_scale=0.0)
        np.testing.assert_array_equal(dur[b, :n], ref["duration"].reshape(-1))
        assert not dur[b, n:].any()
        check_utterance(res, b, ref, n, L, net.dims.total_upsample, "all_predicted")


# ------------------------------------------------------------------ 2. batch-mate independence
def place(frames, phonemes, pos, utt, seed, t_f=None):
    """A batch with other utterances around ``utt`` (a one-utterance batch) at position ``pos``."""
    b = iso.make_batch(frames, phonemes, seed, t_f=t_f)
    n, L = int(utt["lengths"][0]), int(utt["frame_lengths"][0])
    assert phonemes[pos] == n and frames[pos] == L
    for k in ("phonemes", "duration", "f0", "energy"):
        b[k][pos, :n] = utt[k][0, :n]
    b["sid"][pos] = utt["sid"][0]
    b["noise"][pos, :, :L] = utt["noise"][0, :, :L]
    return b


def test_an_utterance_does_not_depend_on_its_batch(net, oracle):
    utt = iso.make_batch([27], [5], seed=2003)
    ref, n, L = iso.alone(oracle, utt, 0, "controls")
    up = net.dims.total_upsample
    a = place([27, 90, 61], [5, 14, 8], 0, utt, seed=2004)                                  # B = 3, T_f = 90, first
    c = place([40, 3, 33, 12, 27], [6, 2, 9, 4, 5], 4, utt, seed=2005)                      # B = 5, T_f = 40, last
    d = place([27, 90, 61], [5, 14, 8], 0, utt, seed=2004, t_f=90 + 37)                     # a global padding beyond T_f
    check_utterance(run(net, a, "controls"), 0, ref, n, L, up, "B=3")
    check_utterance(run(net, c, "controls"), 4, ref, n, L, up, "B=5")
    res = run(net, d, "controls", t_f=90 + 37)
    assert res[0].shape[2] == (90 + 37) * up
    check_utterance(res, 0, ref, n, L, up, "t_f=T_f+37")


# ------------------------------------------------------------------ 3. the real reference, one utterance per call
@pytest.mark.parametrize("mode", ["controls", "predictors"])
def test_isolated_batch_matches_the_reference_golden(net, golden_dir, mode):
    g = np.load(os.path.join(golden_dir, "isolated.npz"))
    batch = {k[3:]: g[k] for k in g.files if k.startswith("in_")}
    res = run(net, batch, mode, noise_scale=float(g["in_noise_scale"]))
    o, _, (z, z_p, m_p, logs_p), _, f0, energy = res
    for b in range(4):
        n, L = int(batch["lengths"][b]), int(batch["frame_lengths"][b])
        for k, v in (("z", z), ("m_p", m_p), ("logs_p", logs_p)):
            assert iso.rel_err(to_np(v)[b, :, :L], g[f"{mode}_{k}"][b, :, :L]) <= STAGE_TOL, (b, k)
            assert not to_np(v)[b, :, L:].any()
        for k, v in (("F0", f0), ("energy", energy)):
            assert iso.rel_err(to_np(v).reshape(4, -1)[b, :n], g[f"{mode}_{k}"][b, :n]) <= STAGE_TOL, (b, k)
        assert iso.rel_err(to_np(o)[b, :, :L * 512], g[f"{mode}_o"][b, :, :L * 512]) <= WAVE_TOL, b
        assert not to_np(o)[b, :, L * 512:].any()


# ------------------------------------------------------------------ 4. the generator alone
RAGGED = [1, 3, 28, 65]


def check_generator_ragged(net, d, w):
    from oracle.vispeech_oracle import Oracle, generator
    orc = Oracle(w, d)
    r = np.random.Generator(np.random.PCG64(2006))
    z = r.standard_normal((4, d.inter_channels, 65)).astype(np.float32)      # (also behind the lengths: never read)
    sid = np.array([3, 40, 11, 62])
    gv = orc.w["emb_g.weight"][torch.from_numpy(sid)]
    o = to_np(net._engine.generator_ragged(z, gv.numpy(), RAGGED))
    up = d.total_upsample
    assert o.shape == (4, 1, 65 * up)
    for b, L in enumerate(RAGGED):
        ref = generator(orc.w, torch.from_numpy(z[b:b + 1, :, :L]), gv[b:b + 1, :, None], d).numpy()
        e = iso.rel_err(o[b, :, :L * up], ref[0])
        print(f"generator_ragged kind={net._engine.generator_kind} L={L}: {e:.1e}")
        assert e <= WAVE_TOL, (b, L, e)
        assert not o[b, :, L * up:].any(), (b, L)
    assert net._engine.status() == 0


def test_generator_ragged_default(net, dims_weights):
    assert net._engine.generator_kind == 1
    check_generator_ragged(net, *dims_weights)


@pytest.mark.parametrize("model", [dict(resblock="2"),
                                   dict(upsample_rates=[8, 8, 2, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4, 4],
                                        upsample_initial_channel=512)], ids=["resblock2", "five_stage"])
def test_generator_ragged_other_generators(model):
    c = ctor_for(**model)
    d, w = weights_of(c)
    m = make_net(c, w)
    assert m._engine.generator_kind == 1
    check_generator_ragged(m, d, w)


def test_generator_ragged_f32_fallback(ctor, dims_weights):
    """VSP_GENERATOR=f32: the channel-major kernels have no per-utterance extent; every convolution masks its staged input
    with the utterance's length at its stage's rate instead."""
    m = make_net(ctor, dims_weights[1], VSP_GENERATOR="f32")
    assert m._engine.generator_kind == 0
    check_generator_ragged(m, *dims_weights)


def test_max_len_truncates_only_the_longer_utterances(net, oracle):
    batch = iso.make_batch(RAGGED, [2, 3, 6, 9], seed=2007)
    res = run(net, batch, "controls", max_len=20)
    assert res[0].shape[2] == 20 * net.dims.total_upsample
    for b in range(4):
        ref, n, L = iso.alone(oracle, batch, b, "controls", max_len=20)
        assert ref["o"].shape[2] == min(L, 20) * net.dims.total_upsample
        check_utterance(res, b, ref, n, L, net.dims.total_upsample, "max_len=20", max_len=20)


# ------------------------------------------------------------------ 5. noise
def noise_of(res, scale):
    _, _, (z, z_p, m_p, logs_p), *_ = res
    return to_np(z_p), to_np(m_p), to_np(logs_p)


def check_noise(res, frames, seeds, scale, inter):
    from oracle.vispeech_oracle import philox_randn
    z_p, m_p, logs_p = noise_of(res, scale)
    for b, (L, s) in enumerate(zip(frames, seeds)):
        want = philox_randn(int(s), inter * L).reshape(inter, L) * np.exp(logs_p[b, :, :L]) * scale
        # the draw: same words, logf / sincosf differ in the last ulps (2e-5, tests/test_hip_parity.py); z_p: fp32 rounding
        tol = 2e-5 * float(np.exp(logs_p[b, :, :L]).max()) * scale + 4 * 2.0 ** -24 * float(np.abs(z_p[b]).max())
        assert np.abs((z_p[b, :, :L] - m_p[b, :, :L]) - want).max() <= tol, (b, L, s)
        assert not z_p[b, :, L:].any()


def test_per_utterance_noise_seeds(net):
    frames, phon, seeds = [9, 31, 17], [3, 6, 4], [11, 2 ** 40 + 5, 12]
    batch = iso.make_batch(frames, phon, seed=2008)
    inter = net.dims.inter_channels
    # two calls back to back, no synchronisation between them: each keeps the seeds it was called with
    other = [s + 1000 for s in seeds]
    first, second = run(net, batch, "controls", noise_seed=seeds), run(net, batch, "controls", noise_seed=other)
    check_noise(first, frames, seeds, 0.667, inter)
    check_noise(second, frames, other, 0.667, inter)
    # the same utterances in another order, each with its own seed: the same noise
    order = [2, 0, 1]
    moved = {k: v[order] for k, v in batch.items()}
    check_noise(run(net, moved, "controls", noise_seed=[seeds[i] for i in order]), [frames[i] for i in order],
                [seeds[i] for i in order], 0.667, inter)


def test_drawing_without_seeds_is_an_error(net, monkeypatch):
    from vispeech_amd._lib import VspError
    batch = iso.make_batch([9, 12], [3, 4], seed=2009)
    eng = net._engine
    eng.set_noise_seeds(None)
    monkeypatch.setattr(eng, "set_noise_seeds", lambda seeds: None)       # (the shim would set them: reach the library's check)
    with pytest.raises(VspError, match="VSP_ERR_STATE"):
        run(net, batch, "controls", noise_seed=[1, 2])
    with pytest.raises(ValueError):
        run(net, batch, "controls", noise_seed=7)                          # a plain int: every utterance the same draw


# ------------------------------------------------------------------ 6. voice conversion
def test_voice_conversion_isolated(net, oracle, dims_weights):
    d = dims_weights[0]
    r = np.random.Generator(np.random.PCG64(2010))
    lens = np.array([21, 9], dtype=np.int64)
    y = np.abs(r.standard_normal((2, d.spec_channels, 21))).astype(np.float32)       # (garbage behind the lengths)
    src, tgt = np.array([3, 40]), np.array([8, 2])
    noise = r.standard_normal((2, d.inter_channels, 21)).astype(np.float32)
    o_hat, y_mask, (z, z_p, z_hat) = net.voice_conversion(dev(net, y), dev(net, lens), dev(net, src), dev(net, tgt),
                                                          noise=dev(net, noise), isolated=True)
    up = d.total_upsample
    for b, L in enumerate(lens):
        ref = oracle.voice_conversion(y[b:b + 1, :, :L], lens[b:b + 1], src[b:b + 1], tgt[b:b + 1], noise[b:b + 1, :, :L])
        for k, v in (("z", z), ("z_p", z_p), ("z_hat", z_hat)):
            assert iso.rel_err(to_np(v)[b, :, :L], ref[k][0].numpy()) <= STAGE_TOL, (b, k)
        assert iso.rel_err(to_np(o_hat)[b, :, :L * up], ref["o_hat"][0].numpy()) <= WAVE_TOL, b
        assert not to_np(o_hat)[b, :, L * up:].any()


# ------------------------------------------------------------------ 7. services
@pytest.mark.parametrize("chunk", [7, 64])
def test_stream_equals_synthesize_byte_for_byte(net, chunk):
    from vispeech_amd.service import SynthesisService
    batch = iso.make_batch([5, 70, 33], [2, 9, 6], seed=2011)
    noise = dev(net, batch["noise"])
    svc = SynthesisService(net, chunk_frames=chunk, isolated=True)
    for u in range(3):
        whole = svc.synthesize(batch, u, noise).tobytes()
        assert len(whole) == 2 * int(batch["frame_lengths"][u]) * net.dims.total_upsample
        assert b"".join(svc.stream(batch, u, noise)) == whole, (chunk, u)


def test_synthesize_without_noise_draws_its_own(net):
    """The services' default call (noise=None) in isolated mode: torch draws the noise, as in the default mode."""
    from vispeech_amd.service import SynthesisService
    batch = iso.make_batch([5, 33], [2, 6], seed=2014)
    svc = SynthesisService(net, chunk_frames=16, isolated=True)
    for u in range(2):
        pcm = svc.synthesize(batch, u)
        assert pcm is not None and pcm.size == int(batch["frame_lengths"][u]) * net.dims.total_upsample and pcm.any()
        assert len(svc.wav_bytes(batch, u)) == 44 + 2 * pcm.size
        assert sum(len(c) for c in svc.stream(batch, u)) == 2 * pcm.size


def test_batching_service_on_the_real_net(net, oracle):
    """Four concurrent submits, one isolated batch: every request's PCM16 against pcm16(oracle alone) with its own noise
    (the library's draw for its seed).  Two values within the waveform gate round to PCM16 values at most
    1 + floor(gate in steps) apart: one step where the gate is under half a step (printed)."""
    from oracle.vispeech_oracle import philox_randn
    from vispeech_amd.service import BatchingSynthesisService, pcm16
    frames, phon, seeds = [6, 40, 23, 1], [2, 7, 5, 2], [101, 102, 103, 104]
    batch = iso.make_batch(frames, phon, seed=2012)
    inter = net.dims.inter_channels

    def collate(rows):
        return {k: batch[k][rows] for k in ("phonemes", "lengths", "sid", "duration", "f0", "energy")}
    svc = BatchingSynthesisService(net, max_batch=4, max_wait_s=30.0, collate=collate)
    try:
        futs = [svc.submit(b, seeds[b]) for b in range(4)]
        got = [f.result(120) for f in futs]
    finally:
        svc.close()
    for b in range(4):
        nz = np.zeros_like(batch["noise"])
        nz[b, :, :frames[b]] = philox_randn(seeds[b], inter * frames[b]).reshape(inter, frames[b])
        ref, n, L = iso.alone(oracle, batch, b, "controls", noise=nz)
        gate_steps = WAVE_TOL * float(np.abs(ref["o"]).max()) * 32767.0
        allowed = 1 + int(np.floor(gate_steps))
        assert allowed == 1, (b, gate_steps)      # (this fixture's gate is under one step: the bound must not loosen silently)
        want = pcm16(ref["o"][0, 0]).astype(np.int64)
        assert got[b].shape == want.shape
        worst = int(np.abs(got[b].astype(np.int64) - want).max())
        print(f"request {b}: gate = {gate_steps:.2f} PCM16 steps, allowed {allowed}, worst {worst}")
        assert worst <= allowed, (b, worst, allowed)


# ------------------------------------------------------------------ 8. the default mode is untouched
def test_default_calls_are_bit_identical_after_the_mode_was_used(ctor, dims_weights, net):
    fresh = make_net(ctor, dims_weights[1])
    assert fresh._engine.lib.vsp_get_isolated(fresh._engine.ctx) == 0 and not fresh._engine.isolated
    batch = iso.make_batch([20, 55, 31], [4, 8, 6], seed=2013)
    for k in ("duration", "f0", "energy"):                  # (a well-formed padded batch: zeros behind the lengths)
        for b, n in enumerate(batch["lengths"]):
            batch[k][b, n:] = 0
    want = run(fresh, batch, "controls", isolated=False)
    run(net, batch, "controls")                            # set(1) ...
    net._engine.set_isolated(True)
    net._engine.set_isolated(False)                        # ... then set(0)
    assert net._engine.lib.vsp_get_isolated(net._engine.ctx) == 0
    got = run(net, batch, "controls", isolated=False)
    assert torch.equal(got[0], want[0]) and torch.equal(got[2][0], want[2][0]) and torch.equal(got[2][1], want[2][1])
