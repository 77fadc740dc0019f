"""SynthesizerTrn with resblock "2" (reference models.py:251, modules.py:232-256) end to end on the MI355X: infer and
voice_conversion against the real reference's outputs (tests/golden/resblock2.npz, make_golden_resblock2.py) at the gates
of tests/test_hip_parity.py, the f32 generator, the per-convolution second implementation (VSP_RB2_FUSE=0), trimmed
tails, the streamed vocoder, the frame dependence, and the arena hash that keeps ResBlock1 and ResBlock2 arenas apart."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

STAGE_TOL = 1e-5
WAVE_TOL = 1e-4


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def to_np(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "resblock2.npz"))


@pytest.fixture(scope="module")
def ctor():
    from vispeech_amd import config as vcfg
    hp = vcfg.default_hparams()
    hp.model["resblock"] = "2"
    return vcfg.synthesizer_args(hp)


@pytest.fixture(scope="module")
def dims(ctor):
    from vispeech_amd.schema import dims_from_ctor
    return dims_from_ctor(*ctor[0], **ctor[1])


@pytest.fixture(scope="module")
def weights(dims, g):
    from vispeech_amd.synth import synth_state_dict
    return synth_state_dict(dims, seed=int(g["weight_seed"]))


def make_net(ctor, weights, **env):
    from vispeech_amd.models import SynthesizerTrn
    mp = pytest.MonkeyPatch()
    for k, v in env.items():
        mp.setenv(k, v)
    try:
        m = SynthesizerTrn(*ctor[0], **ctor[1]).eval()     # (the VSP_* switches are read when the context is created)
    finally:
        mp.undo()
    m.load_state_dict(weights, strict=True)
    return m


@pytest.fixture(scope="module")
def net(ctor, weights):
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return make_net(ctor, weights)


def infer(net, g, max_len=None):
    t = lambda a: torch.from_numpy(np.asarray(a)).to(net.device)
    return net.infer(t(g["in_phonemes"]), t(g["in_lengths"]), sid=t(g["in_sid"]), noise_scale=0.667, max_len=max_len,
                     duration_control=t(g["in_duration"]), pitch_control=t(g["in_f0"]), energy_control=t(g["in_energy"]),
                     noise=t(g["noise"]))


def vc(net, g):
    t = lambda a: torch.from_numpy(np.asarray(a)).to(net.device)
    return net.voice_conversion(t(g["vc_y"]), t(g["vc_lengths"]), t(g["vc_sid_src"]), t(g["vc_sid_tgt"]), noise=t(g["vc_noise"]))


def check_infer(net, g):
    o, x_mask, (z, z_p, m_p, logs_p), *_ = infer(net, g)
    np.testing.assert_array_equal(to_np(x_mask), g["x_mask"])
    errs = {n: rel_err(to_np(v), g[n]) for n, v in (("z", z), ("z_p", z_p), ("m_p", m_p), ("logs_p", logs_p))}
    errs["o"] = rel_err(to_np(o), g["o"])
    print({k: f"{v:.2e}" for k, v in errs.items()})
    assert all(errs[n] <= STAGE_TOL for n in ("z", "z_p", "m_p", "logs_p")), errs
    assert errs["o"] <= WAVE_TOL, errs
    o_ml = infer(net, g, max_len=int(g["ml_max_len"]))[0]
    assert rel_err(to_np(o_ml), g["ml_o"]) <= WAVE_TOL
    assert net._engine.status() == 0
    return o


def check_vc(net, g):
    o_hat, y_mask, (z, z_p, z_hat) = vc(net, g)
    np.testing.assert_array_equal(to_np(y_mask).astype(g["vc_y_mask"].dtype), g["vc_y_mask"])
    for n, v in (("vc_z", z), ("vc_z_p", z_p), ("vc_z_hat", z_hat)):
        assert rel_err(to_np(v), g[n]) <= STAGE_TOL, n
    assert rel_err(to_np(o_hat), g["vc_o_hat"]) <= WAVE_TOL
    assert net._engine.status() == 0


def test_infer_matches_the_reference(net, g):
    check_infer(net, g)


def test_voice_conversion_matches_the_reference(net, g):
    check_vc(net, g)


def test_f32_generator_matches_the_reference(ctor, weights, g):
    m = make_net(ctor, weights, VSP_GENERATOR="f32")
    check_infer(m, g)
    check_vc(m, g)


def test_per_convolution_form_is_bit_identical(net, ctor, weights, g):
    m = make_net(ctor, weights, VSP_RB2_FUSE="0")
    assert same_bits(infer(net, g)[0], infer(m, g)[0])
    assert same_bits(vc(net, g)[0], vc(m, g)[0])
    assert m._engine.status() == 0


def test_generator_schedule(net, ctor, weights, dims):
    """one g16_rb2 launch per block on the 32 / 64-channel stages, two g16_conv launches per block
    on the 128 / 256-channel ones and, under VSP_RB2_FUSE=0, everywhere (3 blocks per stage; conv_pre, 4 up-convolutions)."""
    common = {("pre", 512): 1, ("ups", 256): 1, ("ups", 128): 1, ("ups", 64): 1, ("ups", 32): 1}
    gen = torch.Generator().manual_seed(3)
    z = torch.randn(2, dims.inter_channels, 37, generator=gen)
    gv = torch.randn(2, dims.gin_channels, generator=gen)
    for m, launches in ((net, {("conv", 256): 6, ("conv", 128): 6, ("rb2", 64): 3, ("rb2", 32): 3}),
                        (make_net(ctor, weights, VSP_RB2_FUSE="0"), {("conv", c): 6 for c in (256, 128, 64, 32)})):
        e = m._engine
        e.profile(True)
        e.generator(z, gv)
        fam = e.profile_read_families()
        e.profile_read(reset=True)
        e.profile(False)
        assert {(f["kind"], f["channels"]): f["launches"] for f in fam} == {**common, **launches}


def test_trimmed_tails_are_bit_identical(net, ctor, weights, g):
    m = make_net(ctor, weights, VSP_TRIM_TAILS="0")
    back, fwd = net._engine.generator_frame_dependence()
    assert int(np.asarray(g["x_mask"]).sum(axis=(1, 2)).min()) + back + 1 + fwd < g["x_mask"].shape[2]   # (a tail is trimmed)
    assert same_bits(infer(net, g)[0], infer(m, g)[0])
    assert m._engine.status() == 0


def test_frame_dependence(net):
    assert net._engine.generator_frame_dependence() == (7, 7)
    assert net._engine.generator_halo >= 7


@pytest.mark.parametrize("chunk", [1, 37, 256])
def test_streamed_vocoder_is_bit_identical(net, dims, chunk):
    gen = torch.Generator().manual_seed(chunk)
    T = 300 if chunk > 1 else 40
    z = torch.randn(2, dims.inter_channels, T, generator=gen).to(net.device)
    gv = torch.randn(2, dims.gin_channels, generator=gen).to(net.device)
    eng = net._engine
    whole = eng.generator(z, gv)
    streamed = torch.cat(list(eng.generator_stream(z, gv, chunk_frames=chunk)), dim=-1)
    assert same_bits(streamed, whole)
    assert eng.status() == 0


def test_adopted_arena_and_the_kind_in_its_hash(dims, weights):
    from vispeech_amd._lib import VspError
    from vispeech_amd.engine import Engine
    from vispeech_amd.schema import ModelDims
    from vispeech_amd.synth import synth_state_dict
    root = Engine(dims, "cuda:0")
    root.set_weights(weights)
    arena = root.finalize()
    peer = Engine(dims, "cuda:0")
    mine = peer.adopt()
    mine.copy_(arena)
    torch.cuda.synchronize()
    peer.commit_adopted()
    z = torch.randn(2, dims.inter_channels, 50, device="cuda")
    gv = torch.randn(2, dims.gin_channels, device="cuda")
    assert same_bits(peer.generator(z, gv), root.generator(z, gv))
    # a ResBlock1 context refuses the ResBlock2 arena, and the other way round
    rb1 = Engine(ModelDims(), "cuda:0")
    a1 = rb1.adopt()
    n = min(a1.numel(), arena.numel())
    a1.zero_()
    a1.view(-1)[:n].copy_(arena.view(-1)[:n])
    torch.cuda.synchronize()
    with pytest.raises(VspError):
        rb1.commit_adopted()
    root1 = Engine(ModelDims(), "cuda:0")
    root1.set_weights(synth_state_dict(ModelDims(), seed=1234, infer_only=True))
    arena1 = root1.finalize()
    peer2 = Engine(dims, "cuda:0")
    a2 = peer2.adopt()
    n = min(a2.numel(), arena1.numel())
    a2.zero_()
    a2.view(-1)[:n].copy_(arena1.view(-1)[:n])
    torch.cuda.synchronize()
    with pytest.raises(VspError):
        peer2.commit_adopted()


def test_load_checkpoint_serves_a_resblock2_checkpoint(ctor, weights, g, tmp_path):
    """utils.load_checkpoint (the reference's loader, utils.py:21-51) on a resblock "2" checkpoint."""
    from vispeech_amd import utils
    from vispeech_amd.models import SynthesizerTrn
    p = tmp_path / "G_rb2.pth"
    torch.save({"model": {k: torch.from_numpy(v) for k, v in weights.items()}, "iteration": 1, "optimizer": None,
                "learning_rate": 2e-4}, str(p))
    m = SynthesizerTrn(*ctor[0], **ctor[1]).eval()
    utils.load_checkpoint(str(p), m, None)
    o = infer(m, g)[0]
    assert rel_err(to_np(o), g["o"]) <= WAVE_TOL
