"""The f32 generator as the FALLBACK: plan_model switches a context to the channel-major f32 generator (gen_mode 0) when a
stage's channel count is neither 32 nor a multiple of 64 (weights.cpp).  configs/config.json with upsample_initial_channel
384 has stages of 192, 96, 48 and 24 channels, none of them covered; it runs for ResBlock1 and ResBlock2 against the fp64
oracle generator, as one ragged infer, and streamed.  Then the last stage wider than 32 channels on the f32 generator
(conv_post's kernel, misc.hip): such configurations run and match the oracle, or are refused when the context is created
-- never a context that loads and then fails its first generator call."""
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


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def ctor(resblock="1", c0=384, rates=None, kernels=None):
    from vispeech_amd import config as vcfg
    hp = vcfg.default_hparams()
    hp.model["resblock"] = resblock
    hp.model["upsample_initial_channel"] = c0
    if rates is not None:
        hp.model["upsample_rates"] = list(rates)
        hp.model["upsample_kernel_sizes"] = list(kernels)
        hp.data["hop_length"] = int(np.prod(rates))
    return vcfg.synthesizer_args(hp)


def dims_of(args):
    from vispeech_amd.schema import dims_from_ctor
    return dims_from_ctor(*args[0], **args[1])


def engine(dims, sd, **env):
    from vispeech_amd.engine import Engine
    mp = pytest.MonkeyPatch()
    for k, v in env.items():
        mp.setenv(k, v)
    try:
        e = Engine(dims, "cuda:0")                          # (the VSP_* switches are read when the context is created)
    finally:
        mp.undo()
    e.set_weights(sd)
    e.finalize()
    return e


def oracle_wave(sd, dims, z, g):
    from oracle.vispeech_oracle import Oracle, generator
    w = Oracle(sd, dims, dtype=torch.float64).w
    with torch.no_grad():
        return generator(w, z.double().cpu(), g.double().cpu()[:, :, None], dims).numpy()


def latent(dims, b, t, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(b, dims.inter_channels, t, generator=gen), torch.randn(b, dims.gin_channels, generator=gen)


@pytest.fixture(scope="module", params=["1", "2"], ids=["resblock1", "resblock2"])
def fallback(request):
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from vispeech_amd.synth import synth_state_dict
    args = ctor(request.param)
    dims = dims_of(args)
    assert [dims.upsample_initial_channel >> (i + 1) for i in range(4)] == [192, 96, 48, 24]
    sd = synth_state_dict(dims, seed=21)
    return args, dims, sd, engine(dims, sd)


@pytest.mark.parametrize("frames", [1, 13, 33, 257])
def test_fallback_generator_matches_the_fp64_oracle(fallback, frames):
    _, dims, sd, eng = fallback
    z, g = latent(dims, 2, frames, seed=frames)
    o = eng.generator(z.cuda(), g.cuda())
    assert rel_err(o.cpu().numpy(), oracle_wave(sd, dims, z, g)) <= WAVE_TOL
    assert eng.status() == 0


def test_fallback_is_the_f32_generator(fallback):
    """The default context gives the same bits as a VSP_GENERATOR=f32 context: the evidence that the fallback ran (the
    split-f16 generator's arithmetic differs in its last bits)."""
    _, dims, sd, eng = fallback
    f32 = engine(dims, sd, VSP_GENERATOR="f32")
    z, g = latent(dims, 2, 45, seed=3)
    assert same_bits(eng.generator(z.cuda(), g.cuda()), f32.generator(z.cuda(), g.cuda()))


def test_fallback_ragged_infer_matches_the_oracle(fallback):
    from oracle.vispeech_oracle import Oracle
    from vispeech_amd.models import SynthesizerTrn
    args, dims, sd, _ = fallback
    net = SynthesizerTrn(*args[0], **args[1]).eval()
    net.load_state_dict(sd, strict=True)
    r = np.random.Generator(np.random.PCG64(17))
    B, Tp = 3, 9
    lens = np.array([9, 6, 3], dtype=np.int64)
    ph = r.integers(1, dims.n_vocab, (B, Tp)).astype(np.int64)
    dur = r.integers(1, 6, (B, Tp)).astype(np.float32)
    f0 = r.uniform(100, 400, (B, Tp)).astype(np.float32)
    en = r.uniform(0, 100, (B, Tp)).astype(np.float32)
    for b, n in enumerate(lens):
        ph[b, n:] = 0; dur[b, n:] = 0; f0[b, n:] = 0; en[b, n:] = 0
    sid = np.array([0, 5, 11], dtype=np.int64)
    tf = int(dur.sum(axis=1).max())
    noise = r.standard_normal((B, dims.inter_channels, tf)).astype(np.float32)
    ref = Oracle(sd, dims).infer(ph, lens, sid, noise=noise, noise_scale=0.667, duration_control=dur, pitch_control=f0,
                                 energy_control=en)
    t = lambda x: torch.from_numpy(x).to(net.device)
    o, x_mask, (z, z_p, m_p, logs_p), *_ = net.infer(t(ph), t(lens), sid=t(sid), noise_scale=0.667, duration_control=t(dur),
                                                      pitch_control=t(f0), energy_control=t(en), noise=t(noise))
    for name, v in (("m_p", m_p), ("z_p", z_p), ("z", z)):
        assert rel_err(v.cpu().numpy(), ref[name].numpy()) <= STAGE_TOL, name
    assert rel_err(o.cpu().numpy(), ref["o"].numpy()) <= WAVE_TOL
    assert net._engine.status() == 0


def test_fallback_streamed_vocoder_is_bit_identical(fallback):
    _, dims, _, eng = fallback
    z, g = latent(dims, 2, 90, seed=5)
    whole = eng.generator(z.cuda(), g.cuda())
    streamed = torch.cat(list(eng.generator_stream(z.cuda(), g.cuda(), chunk_frames=37)), dim=-1)
    assert same_bits(streamed, whole)
    assert eng.status() == 0


# the last stage wider than 32 channels: (c0, rates, kernels, env, last stage's channels)
WIDE = [(384, [8, 8, 4], [16, 16, 8], {}, 48),                         # outside the split-f16 cover: the fallback
        (512, [8, 8, 4], [16, 16, 8], {"VSP_GENERATOR": "f32"}, 64),   # configs/config.json's channels on the f32 generator
        (512, [8, 8, 4], [16, 16, 8], {}, 64)]                          # ... and on the split-f16 one


@pytest.mark.parametrize("c0,rates,kernels,env,last", WIDE, ids=["384-fallback", "512-f32", "512-default"])
def test_last_stage_wider_than_32_channels_runs_and_matches_the_oracle(c0, rates, kernels, env, last):
    from vispeech_amd.synth import synth_state_dict
    dims = dims_of(ctor("1", c0, rates, kernels))
    assert dims.upsample_initial_channel >> len(rates) == last and dims.total_upsample == 256
    sd = synth_state_dict(dims, seed=c0)
    eng = engine(dims, sd, **env)                             # (loads: the planner accepts the configuration)
    z, g = latent(dims, 2, 21, seed=c0)
    o = eng.generator(z.cuda(), g.cuda())                     # ... and its first generator call runs
    assert o.shape[-1] == 21 * 256
    assert rel_err(o.cpu().numpy(), oracle_wave(sd, dims, z, g)) <= WAVE_TOL
    assert eng.status() == 0


@pytest.mark.parametrize("env", [{}, {"VSP_GENERATOR": "f32"}], ids=["default", "f32"])
def test_last_stage_wider_than_64_channels_is_refused_when_the_context_is_created(env):
    from vispeech_amd._lib import VspError
    dims = dims_of(ctor("1", 512, [16, 16], [32, 32]))        # 512 -> 256 -> 128: conv_post would read 128 channels
    assert dims.upsample_initial_channel >> 2 == 128 and dims.total_upsample == 256
    mp = pytest.MonkeyPatch()
    for k, v in env.items():
        mp.setenv(k, v)
    try:
        from vispeech_amd.engine import Engine
        with pytest.raises(VspError, match="VSP_ERR_UNSUPPORTED.*conv_post"):
            Engine(dims, "cuda:0")
    finally:
        mp.undo()
