"""Streaming for batched requests on the MI355X (``vsp_generator_stream_rows``, ``StreamingBatchService``): ragged chunks
of several utterances, each at its own offset, computed in one set of generator launches, are the utterance's ALONE run --
within 1e-4 * max|ref| of the CPU oracle's generator (the WAVE_TOL of tests/test_isolated_batch.py) and within
1e-5 * max|ref| of ``Engine.generator_ragged`` B = 1 on the same utterance (the bound between two launch shapes of this
library, sharded against unsharded) -- and exactly 0 behind a row's samples.  Needs an MI355X: `pytest -m gpu`."""
import numpy as np
import pytest
import torch

import isolated_ref as iso

pytestmark = pytest.mark.gpu

WAVE_TOL, SHAPE_TOL = 1e-4, 1e-5
# one frame; shorter than a chunk; either side of the halo (14); a last chunk of one frame (33 = 2 * 16 + 1 = 4 * 8 + 1);
# several chunks
LENGTHS = [1, 5, 14, 15, 33, 97]
START = {97: 0, 33: 1, 15: 2, 14: 3, 5: 3, 1: 4}       # the tick an utterance joins at: rows of a tick sit at different offsets


def to_np(t):
    return t.detach().cpu().numpy()


def ctor_for(**model):
    from vispeech_amd import config as vcfg
    hp = vcfg.default_hparams()
    for k, v in model.items():
        hp.model[k] = v
    return vcfg.synthesizer_args(hp)


def weights_of(ctor):
    from vispeech_amd.schema import dims_from_ctor
    from vispeech_amd.synth import synth_state_dict
    d = dims_from_ctor(*ctor[0], **ctor[1])
    return d, synth_state_dict(d, seed=1234)


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
    return ctor_for()


@pytest.fixture(scope="module")
def dims_weights(ctor):
    return weights_of(ctor)


@pytest.fixture(scope="module")
def net(ctor, dims_weights):
    return make_net(ctor, dims_weights[1])


class Utterances:
    """Random latents of the given lengths on the device, each with its speaker vector, and their alone references
    (computed once, shared, never changed): the CPU oracle's generator and ``generator_ragged`` B = 1.  Even utterances are
    rows of ONE padded tensor (channel stride = the padded length), odd ones tensors of their own of exactly L frames."""

    def __init__(self, net, d, w, lengths, seed):
        from oracle.vispeech_oracle import Oracle, generator
        eng = net._engine
        orc = Oracle(w, d)
        r = np.random.Generator(np.random.PCG64(seed))
        n, T = len(lengths), max(lengths)
        z = r.standard_normal((n, d.inter_channels, T)).astype(np.float32)      # (also behind the lengths: never read)
        gv = orc.w["emb_g.weight"][torch.from_numpy(r.integers(0, 67, size=n))]
        self.lengths, self.up = list(lengths), d.total_upsample
        zd, gd = torch.from_numpy(z).to(eng.device), gv.to(eng.device)
        self.z = [zd[b] if b % 2 == 0 else zd[b, :, :L].contiguous() for b, L in enumerate(lengths)]
        self.g = [gd[b] for b in range(n)]
        self.oracle = [generator(orc.w, torch.from_numpy(z[b:b + 1, :, :L]), gv[b:b + 1, :, None], d).numpy()[0, 0]
                       for b, L in enumerate(lengths)]
        self.alone = [to_np(eng.generator_ragged(zd[b:b + 1, :, :L].contiguous(), gd[b:b + 1], [L]))[0, 0]
                      for b, L in enumerate(lengths)]
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def utts(net, dims_weights):
    return Utterances(net, *dims_weights, LENGTHS, seed=2101)


def drive(eng, u, chunk, start=None, pcm=False):
    """Ticks until every utterance is delivered: utterance b joins at tick start[L_b] and advances by ``chunk`` frames per
    tick.  Returns (per-utterance concatenated samples, the ticks' plans [(b, f0, f1, lo, hi)])."""
    up, n = u.up, len(u.lengths)
    pos, got, plans = [0] * n, [[] for _ in range(n)], []
    tick = 0
    while any(p < L for p, L in zip(pos, u.lengths)):
        act = [b for b in range(n) if pos[b] < u.lengths[b] and (start is None or start[u.lengths[b]] <= tick)]
        tick += 1
        if not act:
            continue
        rows = [(u.z[b], u.g[b], u.lengths[b], pos[b], min(u.lengths[b], pos[b] + chunk)) for b in act]
        out = to_np(eng.generator_stream_rows(rows, chunk, pcm=pcm))
        assert out.shape == (len(act), chunk * up) and out.dtype == (np.int16 if pcm else np.float32)
        lo, hi, span = eng.stream_rows_plan([(L, f0, f1) for _, _, L, f0, f1 in rows])
        assert span <= chunk + 2 * eng.generator_halo
        plans.append([(b, f0, f1, l, h) for b, (_, _, _, f0, f1), l, h in zip(act, rows, lo, hi)])
        for k, (b, (_, _, L, f0, f1)) in enumerate(zip(act, rows)):
            m = (f1 - f0) * up
            assert not out[k, m:].any(), (b, f0, f1, "not zero behind the row's samples")
            got[b].append(out[k, :m])
            pos[b] = f1
    return [np.concatenate(x) for x in got], plans


def check_against_alone(got, u, tag):
    worst = 0.0
    for b, L in enumerate(u.lengths):
        assert got[b].shape == (L * u.up,)
        e_or, e_al = iso.rel_err(got[b], u.oracle[b]), iso.rel_err(got[b], u.alone[b])
        print(f"{tag} L={L}: vs oracle {e_or:.2e}, vs generator_ragged B=1 {e_al:.2e}")
        assert e_or <= WAVE_TOL, (tag, L, e_or)
        assert e_al <= SHAPE_TOL, (tag, L, e_al)
        worst = max(worst, e_al)
    print(f"{tag}: worst vs generator_ragged B=1 = {worst:.2e}")


@pytest.mark.parametrize("chunk", [8, 16])
def test_ragged_chunks_equal_the_alone_run(net, utts, chunk):
    eng = net._engine
    assert eng.generator_kind == 1 and eng.generator_halo == 14
    got, plans = drive(eng, utts, chunk, START)
    L_of = dict(enumerate(utts.lengths))
    # the case this is about: single calls whose rows differ in both edges
    assert any(any(l == 0 for _, _, _, l, _ in p) and any(l > 0 for _, _, _, l, _ in p) for p in plans)
    assert any(any(h == L_of[b] for b, _, _, _, h in p) and any(h < L_of[b] for b, _, _, _, h in p) for p in plans)
    assert max(len(p) for p in plans) >= 4
    check_against_alone(got, utts, f"chunk={chunk}")
    assert eng.status() == 0


@pytest.mark.parametrize("model,env,kind", [
    (dict(resblock="2"), {}, 1),
    (dict(upsample_rates=[8, 8, 2, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4, 4], upsample_initial_channel=512), {}, 1),
    ({}, {"VSP_GENERATOR": "f32"}, 0)], ids=["resblock2", "five_stage", "f32"])
def test_other_generators(model, env, kind):
    c = ctor_for(**model)
    d, w = weights_of(c)
    m = make_net(c, w, **env)
    assert m._engine.generator_kind == kind
    u = Utterances(m, d, w, [5, 33, 97], seed=2102)
    got, _ = drive(m._engine, u, 16, {97: 0, 33: 1, 5: 2})
    check_against_alone(got, u, f"kind={kind} {'/'.join(model) or 'f32'}")
    assert m._engine.status() == 0


def rows_at(u, picks):
    return [(u.z[b], u.g[b], u.lengths[b], f0, f1) for b, f0, f1 in picks]


def test_pcm_is_pcm16_of_the_float_output(net, utts):
    from vispeech_amd.service import pcm16
    eng = net._engine
    rows = rows_at(utts, [(5, 32, 48), (4, 32, 33), (1, 0, 5), (0, 0, 1)])        # L = 97, 33, 5, 1
    f = to_np(eng.generator_stream_rows(rows, 16, pcm=False))
    q = to_np(eng.generator_stream_rows(rows, 16, pcm=True))
    assert q.dtype == np.int16 and q.shape == f.shape and np.abs(f).max() > 1e-3
    np.testing.assert_array_equal(q.reshape(-1), pcm16(f))


def test_a_row_does_not_depend_on_its_neighbours(net, utts):
    eng = net._engine
    me = (5, 40, 56)                                                             # L = 97: an inner window
    ref = utts.alone[5][40 * utts.up: 56 * utts.up]
    alone = to_np(eng.generator_stream_rows(rows_at(utts, [me]), 16, pcm=False))[0]
    beside = to_np(eng.generator_stream_rows(rows_at(utts, [(1, 0, 5), me, (4, 16, 32)]), 16, pcm=False))
    again = to_np(eng.generator_stream_rows(rows_at(utts, [(1, 0, 5), me, (4, 16, 32)]), 16, pcm=False))
    np.testing.assert_array_equal(beside, again)                                 # two identical calls: identical bytes
    scale = float(np.abs(ref).max())
    for name, x in (("alone", alone), ("beside", beside[1])):
        e = float(np.abs(x - ref).max()) / scale
        print(f"row {name}: {e:.2e} of the utterance's own run")
        assert e <= SHAPE_TOL, (name, e)
    assert float(np.abs(alone - beside[1]).max()) / scale <= SHAPE_TOL


def test_bad_rows_are_refused(net, utts):
    from vispeech_amd._lib import VspError
    eng = net._engine
    for picks in ([(5, 0, 17)], [(1, 0, 6)], [(1, 3, 3)], [(5, 0, 16), (1, -1, 4)]):     # chunk too long, f1 > L, empty, f0 < 0
        with pytest.raises(VspError, match="VSP_ERR_ARG"):
            eng.generator_stream_rows(rows_at(utts, picks), 16)
    with pytest.raises(ValueError):
        eng.generator_stream_rows([], 16)


# ------------------------------------------------------------------ the service on the real net
FRAMES, PHON, SEEDS = [6, 40, 23], [2, 7, 5], [201, 202, 203]


def run_service(net, batch, monkeypatch, **kw):
    """Rows 0 and 1 submitted while idle, row 2 after tick 2; driven by step().  Returns (per-request bytes, per-request
    float samples of the same generator calls, stats)."""
    from vispeech_amd.service import StreamingBatchService
    eng, up = net._engine, net.dims.total_upsample
    floats = {}
    real = eng.generator_stream_rows

    def recording(rows, chunk_frames, pcm=True):
        f = to_np(real(rows, chunk_frames, pcm=False))
        for k, (z, g, L, f0, f1) in enumerate(rows):
            floats.setdefault(z.data_ptr(), []).append(f[k, : (f1 - f0) * up])
        return real(rows, chunk_frames, pcm=pcm)
    monkeypatch.setattr(eng, "generator_stream_rows", recording)

    def collate(rows):
        return {k: batch[k][rows] for k in ("phonemes", "lengths", "sid", "duration", "f0", "energy")}
    svc = StreamingBatchService(net, max_batch=4, chunk_frames=16, collate=collate, autostart=False, **kw)
    streams = [svc.submit(0, SEEDS[0]), svc.submit(1, SEEDS[1])]
    svc.step(); svc.step()
    streams.append(svc.submit(2, SEEDS[2]))
    svc.close()
    monkeypatch.undo()
    assert svc.stats["rows_per_tick"] == [2, 1, 2, 1] and svc.stats["groups"] == 2
    order = sorted(floats, key=lambda p: -sum(len(c) for c in floats[p]))         # by length: rows 1, 2, 0
    by_row = {1: order[0], 2: order[1], 0: order[2]}
    return [b"".join(s) for s in streams], [np.concatenate(floats[by_row[b]]) for b in range(3)], svc.stats


def test_service_on_the_real_net(net, monkeypatch):
    from vispeech_amd.service import BatchingSynthesisService, pcm16
    batch = iso.make_batch(FRAMES, PHON, seed=2103)
    up = net.dims.total_upsample
    got, floats, _ = run_service(net, batch, monkeypatch)

    def collate(rows):
        return {k: batch[k][rows] for k in ("phonemes", "lengths", "sid", "duration", "f0", "energy")}
    ref_svc = BatchingSynthesisService(net, max_batch=3, max_wait_s=30.0, collate=collate)
    try:
        want = [f.result(120) for f in [ref_svc.submit(b, SEEDS[b]) for b in range(3)]]
    finally:
        ref_svc.close()
    for b in range(3):
        mine = np.frombuffer(got[b], dtype="<i2")
        assert mine.shape == want[b].shape == (FRAMES[b] * up,)
        np.testing.assert_array_equal(mine, pcm16(floats[b]))                    # exactly pcm16 of its own float path
        worst = int(np.abs(mine.astype(np.int64) - want[b].astype(np.int64)).max())
        print(f"request {b}: worst {worst} PCM16 steps from BatchingSynthesisService")
        assert worst <= 1, (b, worst)


def test_service_with_an_output_rate(net, monkeypatch):
    batch = iso.make_batch(FRAMES, PHON, seed=2103)
    eng, up = net._engine, net.dims.total_upsample
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(net.device)
    try:
        got, _, _ = run_service(net, batch, monkeypatch, output_rate=22050)
        o, *_ = net.infer(dev(batch["phonemes"]), dev(batch["lengths"]), sid=dev(batch["sid"]), noise_scale=0.667,
                          duration_control=dev(batch["duration"]), pitch_control=dev(batch["f0"]),
                          energy_control=dev(batch["energy"]), noise_seed=list(SEEDS), isolated=True)
        for b in range(3):
            want = to_np(eng.output(o[b:b + 1, 0, : FRAMES[b] * up], pcm=True)[0]).reshape(-1)
            mine = np.frombuffer(got[b], dtype="<i2")
            assert mine.shape == want.shape == (FRAMES[b] * up // 2,)
            worst = int(np.abs(mine.astype(np.int64) - want.astype(np.int64)).max())
            print(f"request {b} at 22050 Hz: worst {worst} PCM16 steps from Engine.output of the one-shot waveform")
            assert worst <= 1, (b, worst)
    finally:
        eng.configure_output(None)
