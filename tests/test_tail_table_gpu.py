"""The per-speaker silence table (vispeech_amd/csrc/model.h, kernels.h): behind an utterance the vocoder's input is zero, so
the steady-state frame and the frames at the tensor's end depend on the weights and the speaker vector only.  A context
keeps them per row of emb_g; an utterance whose g is such a row (compared bit for bit on the device) and whose
length + back + fwd <= T takes its padded tail from the table, and the stages behind the first compute it to
length + back + reach1 frames.  The FULL padded waveform must stay what the to-the-padded-length run gives
(VSP_TRIM_TAILS=0), bit for bit: here on both sides of the eligibility edge, with speakers shared between rows, with a g
that is no row of the table, after a reload, on the other generator configurations, and on the callers that pass lengths
but end every utterance at its own length.  VSP_TAIL_TABLE=0 is the path without the table.  Needs an MI355X."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BACK, FWD, REACH1 = 13, 13, 2          # configs/config.json (tests/test_tail_extents_host.py derives them)


def to_np(t):
    return t.detach().cpu().numpy()


def default_ctor():
    from vispeech_amd import config as vcfg
    return vcfg.synthesizer_args(vcfg.default_hparams())


def ctor_for(**model):
    from vispeech_amd import config as vcfg
    hp = vcfg.default_hparams()
    for k, v in model.items():
        hp.model[k] = v
    return vcfg.synthesizer_args(hp)


def weights_for(ctor, seed=1234):
    from vispeech_amd.schema import dims_from_ctor
    from vispeech_amd.synth import synth_state_dict
    return synth_state_dict(dims_from_ctor(*ctor[0], **ctor[1]), seed=seed, infer_only=True)


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
def ctor():
    return default_ctor()


@pytest.fixture(scope="module")
def weights(ctor):
    return weights_for(ctor)


@pytest.fixture(scope="module")
def net(ctor, weights):
    return make_net(ctor, weights)


@pytest.fixture(scope="module")
def net_untrimmed(ctor, weights):
    return make_net(ctor, weights, VSP_TRIM_TAILS="0")


@pytest.fixture(scope="module")
def net_no_table(ctor, weights):
    return make_net(ctor, weights, VSP_TAIL_TABLE="0")


def batch_with_frames(frames, seed, shared_sid=True):
    """A synthetic batch whose utterances have exactly `frames` frames (durations rewritten, noise redrawn); rows 0 and 1
    speak with the same speaker."""
    from vispeech_amd.synth import synth_batch
    frames = np.asarray(frames, dtype=np.int64)
    b = synth_batch(len(frames), seed=seed, mean_phonemes=10, std_phonemes=3, min_phonemes=6, max_phonemes=16,
                    mean_frames=30, jitter_frames=5)
    r = np.random.Generator(np.random.PCG64(seed + 1))
    for i, L in enumerate(frames):
        n = int(b["lengths"][i])
        cut = np.sort(r.integers(0, L + 1, size=n - 1))
        b["duration"][i, :] = 0
        b["duration"][i, :n] = np.diff(np.concatenate([[0], cut, [L]]))
    b["frame_lengths"] = frames
    b["noise"] = r.standard_normal((len(frames), 192, int(frames.max())), dtype=np.float32)
    if shared_sid and len(frames) > 1:
        b["sid"][1] = b["sid"][0]
    return b


def run(net, b):
    t = lambda a: torch.from_numpy(np.asarray(a)).to(net.device)
    o, _, (z, *_), *_ = net.infer(t(b["phonemes"]), t(b["lengths"]), sid=t(b["sid"]), noise_scale=0.667,
                                  duration_control=t(b["duration"]), pitch_control=t(b["f0"]),
                                  energy_control=t(b["energy"]), noise=t(b["noise"]))
    return o, z


def assert_same(a, c, frames, what):
    assert a.shape == c.shape
    a, c = to_np(a), to_np(c)
    for i, L in enumerate(frames):       # per utterance, so that a failure names the case
        np.testing.assert_array_equal(a[i], c[i], err_msg=f"{what}: utterance {i} ({L} of {max(frames)} frames)")


def edge_frames(T):
    """Both sides of length + back + fwd <= T (T - 25 is not eligible, T - 26 is the last that is and runs stage 0 to the
    tensor's true end, T - 27 the first whose stage 0 ends early too), the full length, one below `back`, and one frame."""
    return [T, T - 25, T - 26, T - 27, 5, 1]


def test_extents(net):
    assert net._engine.generator_tail_extents() == (BACK, FWD, REACH1)


# T = 41: a second padded length, where the three edge lengths (16, 15, 14) sit right above `back`
@pytest.mark.parametrize("T", [64, 41])
def test_table_equals_the_padded_run_bit_for_bit(net, net_untrimmed, net_no_table, T):
    frames = edge_frames(T)
    b = batch_with_frames(frames, seed=700 + T)
    o1, z1 = run(net, b)
    o0, z0 = run(net_untrimmed, b)
    o2, z2 = run(net_no_table, b)
    assert o1.shape == (6, 1, 512 * T)
    assert torch.equal(z1, z0) and torch.equal(z2, z0)
    assert_same(o1, o0, frames, "table vs untrimmed")
    assert_same(o2, o1, frames, "VSP_TAIL_TABLE=0 vs default")
    # the padded tails are not zero: the fill is doing real work
    assert np.abs(to_np(o1)[4, 0, 512 * (5 + BACK):]).max() > 0
    assert net._engine.status() == 0


def test_second_call_and_repeated_speaker(net, net_untrimmed):
    """Every row the same speaker, and the same context called again: the table is read, not rebuilt, not consumed."""
    frames = [50, 9, 24, 17]
    b = batch_with_frames(frames, seed=711)
    b["sid"][:] = b["sid"][0]
    o0, _ = run(net_untrimmed, b)
    for _ in range(2):
        assert_same(run(net, b)[0], o0, frames, "one speaker")


def decode_with_g(net, b, g_edit=None):
    """encode / decode as two calls, so that the speaker vectors can be edited in between."""
    e = net._engine
    t = lambda a: torch.from_numpy(np.asarray(a)).to(net.device)
    enc = e.encode(t(b["phonemes"]), t(b["lengths"]), t(b["sid"]), duration_ctl=t(b["duration"]), pitch_ctl=t(b["f0"]),
                   energy_ctl=t(b["energy"]))
    _, tf = e.frame_lengths_host(enc["frame_lengths"])
    if g_edit is not None:
        g_edit(enc["g"])
    return e.decode(enc, tf, t(b["noise"]), 0.667)["o"].clone()


def test_custom_g_is_not_served_by_the_table(net, net_untrimmed, weights):
    """A g one ulp away from its row of emb_g is no row of the table: that utterance runs as it did without one, next to
    rows that are served -- through vsp_decode (the padded batch) and through vsp_generator_ragged (own ends)."""
    frames = [56, 20, 11, 30]
    b = batch_with_frames(frames, seed=712)

    def one_ulp(g):
        bits = g[2].view(torch.int32)
        bits[7] += 1                       # one ulp up in magnitude, one word of the row

    o1 = decode_with_g(net, b, one_ulp)
    o0 = decode_with_g(net_untrimmed, b, one_ulp)
    assert_same(o1, o0, frames, "custom g, vsp_decode")

    r = np.random.Generator(np.random.PCG64(713))
    z = torch.from_numpy(r.standard_normal((4, 192, 56)).astype(np.float32))
    g = torch.from_numpy(np.asarray(weights["emb_g.weight"], dtype=np.float32)[[3, 3, 5, 8]].copy())
    g[2].view(torch.int32)[0] += 1
    a = net._engine.generator_ragged(z, g, frames)
    c = net_untrimmed._engine.generator_ragged(z, g, frames)
    assert torch.equal(a, c)


def test_reload_invalidates_the_table(ctor, weights):
    """Load, run, load a state dict with another emb_g, run: the second result is the untrimmed one of the NEW weights."""
    frames = [60, 12, 30]
    b = batch_with_frames(frames, seed=714)
    m = make_net(ctor, weights)
    first = run(m, b)[0].clone()
    w2 = dict(weights)
    r = np.random.Generator(np.random.PCG64(715))
    w2["emb_g.weight"] = r.standard_normal(weights["emb_g.weight"].shape).astype(np.float32)
    m.load_state_dict(w2, strict=True)
    second = run(m, b)[0]
    o0 = run(make_net(ctor, w2, VSP_TRIM_TAILS="0"), b)[0]
    assert_same(second, o0, frames, "after the reload")
    assert not torch.equal(first, second)


FIVE_STAGE = dict(upsample_rates=[8, 8, 2, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4, 4], upsample_initial_channel=512)


@pytest.mark.parametrize("model", [FIVE_STAGE, dict(resblock="2")], ids=["five-stage", "resblock2"])
def test_other_configurations(model):
    """The support arithmetic is general: B = 3, T = 48 with the last eligible length, whatever back / fwd are there."""
    c = ctor_for(**model)
    w = weights_for(c)
    a = make_net(c, w)
    back, fwd, reach1 = a._engine.generator_tail_extents()
    T = 48
    assert a._engine.generator_kind == 1 and T > back + fwd + 1 and reach1 <= fwd
    frames = [T, T - back - fwd, 3]
    b = batch_with_frames(frames, seed=716)
    o1 = run(a, b)[0]
    o0 = run(make_net(c, w, VSP_TRIM_TAILS="0"), b)[0]
    assert o1.shape[2] == T * a._engine.dims.total_upsample
    assert_same(o1, o0, frames, str(model))
    assert a._engine.status() == 0


def test_streaming_rows_keep_their_own_ends(net, net_untrimmed, weights):
    """The batched streaming call passes lengths but ends every row at its own window (isolated extents): the table does
    not apply, and speakers that ARE rows of the table change nothing."""
    r = np.random.Generator(np.random.PCG64(717))
    emb = torch.from_numpy(np.asarray(weights["emb_g.weight"], dtype=np.float32))
    rows = []
    for L, f0, f1, sid in ((40, 0, 16, 3), (23, 7, 23, 3), (9, 0, 9, 11)):
        z = torch.from_numpy(r.standard_normal((192, L)).astype(np.float32)).to(net.device)
        rows.append((z, emb[sid].float().to(net.device), L, f0, f1))
    a = net._engine.generator_stream_rows(rows, 16, pcm=False)
    c = net_untrimmed._engine.generator_stream_rows(rows, 16, pcm=False)
    assert torch.equal(a, c)


def profiled(net, b):
    e = net._engine
    e.profile(True)
    run(net, b)
    torch.cuda.synchronize()
    fam = e.profile_read_families()
    n, _, flops, *_ = e.profile_read(reset=True)
    e.profile(False)
    return {(f["kind"], f["channels"]): f["launches"] for f in fam}, n, flops


def test_schedule_is_the_same_with_and_without_the_table(ctor, weights, net_no_table):
    """A profiled call books the same launches per kernel family on its first call, on a later one and without the table
    (the build is no part of any call's profile; 51 launches: tests/test_hip_parity.py) -- and fewer flops with the table:
    the stages behind the first are charged the frames they compute."""
    frames = [64, 30, 12, 5]
    b = batch_with_frames(frames, seed=718)
    m = make_net(ctor, weights)
    first = profiled(m, b)
    later = profiled(m, b)
    plain = profiled(net_no_table, b)
    assert first == later
    assert first[0] == plain[0] and first[1] == plain[1] == 51
    assert first[2] < plain[2]
    assert m._engine.status() == 0
