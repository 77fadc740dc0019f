"""SynthesizerTrn as a FIVE-stage generator (upsample_rates [8, 8, 2, 2, 2], 512 initial channels: a 16-channel last
stage) end to end on the MI355X: the split-f16 channels-last generator serves it (vsp_generator_kind), infer against the
real reference's outputs (tests/golden/five_stage.npz, make_golden_five_stage.py) at the gates of
tests/test_hip_parity.py for both generator kinds and both ResBlock kinds, trimmed tails, the per-convolution second
implementation, and the streamed vocoder."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

STAGE_TOL = 1e-5
WAVE_TOL = 1e-4
FIVE_STAGE = dict(upsample_rates=[8, 8, 2, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4, 4], upsample_initial_channel=512)


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def to_np(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def ctor_for(resblock="1", **model):
    from vispeech_amd import config as vcfg
    hp = vcfg.default_hparams()
    for k, v in dict(FIVE_STAGE, **model).items():
        hp.model[k] = v
    hp.model["resblock"] = resblock
    return vcfg.synthesizer_args(hp)


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "five_stage.npz"))


def weights_for(ctor, g):
    from vispeech_amd.schema import dims_from_ctor
    from vispeech_amd.synth import synth_state_dict
    return synth_state_dict(dims_from_ctor(*ctor[0], **ctor[1]), seed=int(g["weight_seed"]))


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


@pytest.fixture(scope="module")
def ctor1():
    return ctor_for("1")


@pytest.fixture(scope="module")
def ctor2():
    return ctor_for("2")


@pytest.fixture(scope="module")
def w1(ctor1, g):
    return weights_for(ctor1, g)


@pytest.fixture(scope="module")
def w2(ctor2, g):
    return weights_for(ctor2, g)


@pytest.fixture(scope="module")
def net(ctor1, w1):
    return make_net(ctor1, w1)


@pytest.fixture(scope="module")
def net2(ctor2, w2):
    return make_net(ctor2, w2)


def infer(net, g):
    t = lambda a: torch.from_numpy(np.asarray(a)).to(net.device)
    return net.infer(t(g["in_phonemes"]), t(g["in_lengths"]), sid=t(g["in_sid"]), noise_scale=0.667,
                     duration_control=t(g["in_duration"]), pitch_control=t(g["in_f0"]), energy_control=t(g["in_energy"]),
                     noise=t(g["noise"]))


def check_infer(net, g, wave="o"):
    o, x_mask, (z, z_p, m_p, logs_p), *_ = infer(net, g)
    np.testing.assert_array_equal(to_np(x_mask), g["x_mask"])
    errs = {n: rel_err(to_np(v), g[n]) for n, v in (("z", z), ("z_p", z_p), ("m_p", m_p), ("logs_p", logs_p))}
    errs["o"] = rel_err(to_np(o), g[wave])
    print({k: f"{v:.2e}" for k, v in errs.items()})
    assert all(errs[n] <= STAGE_TOL for n in ("z", "z_p", "m_p", "logs_p")), errs
    assert errs["o"] <= WAVE_TOL, errs
    assert net._engine.status() == 0


def test_the_split_f16_generator_serves_five_stages(net, net2, ctor1, w1):
    assert net._engine.generator_kind == 1 and net2._engine.generator_kind == 1
    assert make_net(ctor1, w1, VSP_GENERATOR="f32")._engine.generator_kind == 0
    assert make_net(ctor1, w1, VSP_GENERATOR="f16")._engine.generator_kind == 2


def test_other_configurations_keep_their_generator(g):
    from vispeech_amd.engine import Engine
    from vispeech_amd.schema import ModelDims, dims_from_ctor
    assert Engine(ModelDims(), "cuda:0").generator_kind == 1                           # configs/config.json
    c384 = ctor_for("1", upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4], upsample_initial_channel=384)
    assert Engine(dims_from_ctor(*c384[0], **c384[1]), "cuda:0").generator_kind == 0    # 192 / 96 / 48 / 24 channels
    # 16 channels anywhere but last, and a last stage of 16 not reached from 32 by a covered up-convolution
    c_mid = ctor_for("1", upsample_rates=[8, 8, 2, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4, 4], upsample_initial_channel=256)
    assert Engine(dims_from_ctor(*c_mid[0], **c_mid[1]), "cuda:0").generator_kind == 0  # 128 / 64 / 32 / 16 / 8
    c_odd = ctor_for("1", upsample_rates=[8, 8, 8, 1, 1], upsample_kernel_sizes=[16, 16, 16, 3, 3], upsample_initial_channel=512)
    assert Engine(dims_from_ctor(*c_odd[0], **c_odd[1]), "cuda:0").generator_kind == 0  # stride 1 into 16 channels


def test_infer_matches_the_reference(net, g):
    check_infer(net, g)


def test_f32_generator_matches_the_reference(ctor1, w1, g):
    check_infer(make_net(ctor1, w1, VSP_GENERATOR="f32"), g)


def test_resblock2_waveform_matches_the_reference(net2, ctor2, w2, g):
    check_infer(net2, g, wave="rb2_o")
    check_infer(make_net(ctor2, w2, VSP_GENERATOR="f32"), g, wave="rb2_o")


def ragged_batch(frames=(8, 48, 21), seed=23):
    """A synthetic batch whose utterances have exactly `frames` frames (durations rewritten, noise redrawn)."""
    from vispeech_amd.synth import synth_batch
    frames = np.asarray(frames, dtype=np.int64)
    b = synth_batch(len(frames), seed=seed, mean_phonemes=8, std_phonemes=3, min_phonemes=4, max_phonemes=12,
                    mean_frames=26, jitter_frames=5)
    r = np.random.Generator(np.random.PCG64(seed + 1))
    for i, L in enumerate(frames):
        n = int(b["lengths"][i])
        cut = np.sort(r.integers(0, L + 1, size=n - 1))
        b["duration"][i, :] = 0
        b["duration"][i, :n] = np.diff(np.concatenate([[0], cut, [L]]))
    b["frame_lengths"] = frames
    b["noise"] = r.standard_normal((len(frames), 192, int(frames.max())), dtype=np.float32)
    return b


def infer_batch(net, b):
    t = lambda a: torch.from_numpy(np.asarray(a)).to(net.device)
    return net.infer(t(b["phonemes"]), t(b["lengths"]), sid=t(b["sid"]), noise_scale=0.667, duration_control=t(b["duration"]),
                     pitch_control=t(b["f0"]), energy_control=t(b["energy"]), noise=t(b["noise"]))[0]


@pytest.mark.parametrize("kind", ["1", "2"])
def test_trimmed_tails_are_bit_identical(kind, net, net2, ctor1, ctor2, w1, w2):
    a, ctor, w = (net, ctor1, w1) if kind == "1" else (net2, ctor2, w2)
    m = make_net(ctor, w, VSP_TRIM_TAILS="0")
    b = ragged_batch()
    fl = [int(v) for v in b["frame_lengths"]]
    back, fwd = a._engine.generator_frame_dependence()
    assert fl == [8, 48, 21], fl
    assert min(fl) + back + 1 + fwd < max(fl)                       # (a tail is trimmed)
    assert same_bits(infer_batch(a, b), infer_batch(m, b))
    assert a._engine.status() == 0 and m._engine.status() == 0


def test_per_convolution_forms_are_bit_identical(net, net2, ctor1, ctor2, w1, w2, g):
    o = infer(net, g)[0]
    for env in ({"VSP_CHAIN": "0"}, {"VSP_FUSE_PAIRS": "0"}):
        m = make_net(ctor1, w1, **env)
        assert m._engine.generator_kind == 1
        assert same_bits(o, infer(m, g)[0]), env
        assert m._engine.status() == 0
    m2 = make_net(ctor2, w2, VSP_RB2_FUSE="0")
    assert same_bits(infer(net2, g)[0], infer(m2, g)[0])
    assert m2._engine.status() == 0


def test_generator_schedule(net, ctor1, w1):
    """the four wide stages as in configs/config.json, each ResBlock of the 16-channel stage one
    g16_c16 launch charged to the chain family; VSP_CHAIN=0: pairs on the 32-channel stage, one launch per convolution on
    the 16-channel one (3 blocks x 3 pairs x 2 convolutions)."""
    common = {("pre", 512): 1, ("ups", 256): 1, ("ups", 128): 1, ("ups", 64): 1, ("ups", 32): 1, ("ups", 16): 1,
              ("conv", 256): 18, ("conv", 128): 6, ("pair", 128): 6, ("pair", 64): 9}
    gen = torch.Generator().manual_seed(3)
    z = torch.randn(2, net.dims.inter_channels, 37, generator=gen)
    gv = torch.randn(2, net.dims.gin_channels, generator=gen)
    for m, launches in ((net, {("pair", 32): 6, ("chain", 32): 1, ("chain", 16): 3}),
                        (make_net(ctor1, w1, VSP_CHAIN="0"), {("pair", 32): 9, ("conv", 16): 18})):
        e = m._engine
        e.profile(True)
        e.generator(z, gv)
        fam = e.profile_read_families()
        e.profile_read(reset=True)
        e.profile(False)
        assert {(f["kind"], f["channels"]): f["launches"] for f in fam} == {**common, **launches}


@pytest.mark.parametrize("kind", ["1", "2"])
@pytest.mark.parametrize("chunk", [5, 64])
def test_streamed_vocoder_is_bit_identical(kind, chunk, net, net2):
    m = net if kind == "1" else net2
    gen = torch.Generator().manual_seed(chunk)
    T = 70
    z = torch.randn(2, m.dims.inter_channels, T, generator=gen).to(m.device)
    gv = torch.randn(2, m.dims.gin_channels, generator=gen).to(m.device)
    eng = m._engine
    whole = eng.generator(z, gv)
    assert whole.shape == (2, 1, T * 512)
    streamed = torch.cat(list(eng.generator_stream(z, gv, chunk_frames=chunk)), dim=-1)
    assert same_bits(streamed, whole)
    assert eng.status() == 0
