"""The ragged output stage of streamed batches on the MI355X (``vsp_generator_stream_rows_output``,
``StreamingBatchService(fused_output=True)``).  The yardstick is the library's own one-shot output stage, EXACTLY: the
same tick schedule is driven through ``generator_stream_rows(pcm=False)`` and through the new call; the floats,
concatenated per utterance and passed through ``Engine.output`` in one shot, must equal the concatenated ticked output bit
for bit, as float32 and as int16 -- same taps, same FMA order, same input samples.  Needs an MI355X: `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest
import torch

import isolated_ref as iso
from vispeech_amd import output_stage

pytestmark = pytest.mark.gpu

# one frame (ends in its first tick: no history, the whole tail); shorter than a chunk of 8; two chunks; a last chunk of one
# frame (33 = 4 * 8 + 1)
LENGTHS = [1, 5, 15, 33]
START = {33: 0, 15: 1, 5: 2, 1: 3}          # the tick an utterance joins at: the rows of a tick sit at different positions
# (out_rate, zeros): L = 1; more outputs than inputs; a 705-sample history, longer than a one-frame chunk of 512; pass-through
STAGES = [(22050, 32), (48000, 32), (8000, 64), (44100, 32)]


def to_np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def net():
    from vispeech_amd import config as vcfg
    from vispeech_amd.models import SynthesizerTrn
    from vispeech_amd.schema import dims_from_ctor
    from vispeech_amd.synth import synth_state_dict
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    ctor = vcfg.synthesizer_args(vcfg.default_hparams())
    m = SynthesizerTrn(*ctor[0], **ctor[1]).eval()
    m.load_state_dict(synth_state_dict(dims_from_ctor(*ctor[0], **ctor[1]), seed=1234), strict=True)
    yield m
    m._engine.configure_output(None)


class Utterances:
    """Random latents of the given lengths on the device, each with its speaker vector.  Even utterances are rows of ONE
    padded tensor (channel stride = the padded length), odd ones tensors of their own of exactly L frames."""

    def __init__(self, net, lengths, seed):
        eng, d = net._engine, net.dims
        r = np.random.Generator(np.random.PCG64(seed))
        n, T = len(lengths), max(lengths)
        zd = torch.from_numpy(r.standard_normal((n, d.inter_channels, T)).astype(np.float32)).to(eng.device)
        gd = torch.from_numpy(r.standard_normal((n, d.gin_channels)).astype(np.float32)).to(eng.device)
        self.lengths, self.up = list(lengths), d.total_upsample
        self.z = [zd[b] if b % 2 == 0 else zd[b, :, :L].contiguous() for b, L in enumerate(lengths)]
        self.g = [gd[b] for b in range(n)]


@pytest.fixture(scope="module")
def utts(net):
    return Utterances(net, LENGTHS, seed=2201)


def schedule(u, chunk, start):
    """The ticks until every utterance is delivered: a list of [(b, f0, f1)] per tick with at least one row."""
    pos, ticks, tick = [0] * len(u.lengths), [], 0
    while any(p < L for p, L in zip(pos, u.lengths)):
        act = [b for b, L in enumerate(u.lengths) if pos[b] < L and start[L] <= tick]
        tick += 1
        if act:
            ticks.append([(b, pos[b], min(u.lengths[b], pos[b] + chunk)) for b in act])
            for b, _, f1 in ticks[-1]:
                pos[b] = f1
    return ticks


@pytest.fixture(scope="module")
def float_runs(net, utts):
    """Per chunk size, the concatenated float chunks of every utterance from ``generator_stream_rows(pcm=False)`` on the
    schedule below -- computed once, shared by every stage and format, never changed."""
    eng, runs = net._engine, {}
    for chunk in (1, 8):
        got = [[] for _ in utts.lengths]
        for tick in schedule(utts, chunk, START):
            out = to_np(eng.generator_stream_rows([(utts.z[b], utts.g[b], utts.lengths[b], f0, f1) for b, f0, f1 in tick],
                                                  chunk, pcm=False))
            for k, (b, f0, f1) in enumerate(tick):
                got[b].append(out[k, : (f1 - f0) * utts.up])
        runs[chunk] = [np.concatenate(x) for x in got]
    return runs


def one_shot(eng, x, pcm):
    """``Engine.output`` of one utterance's whole float waveform (a numpy vector)."""
    y, _ = eng.output(torch.from_numpy(x).to(eng.device)[None, :], pcm=pcm)
    return to_np(y)[0]


@pytest.mark.parametrize("pcm", [False, True], ids=["f32", "pcm16"])
@pytest.mark.parametrize("chunk", [1, 8])
@pytest.mark.parametrize("stage", STAGES, ids=lambda s: f"{s[0]}z{s[1]}")
def test_ticked_output_is_the_one_shot_output_stage(net, utts, float_runs, stage, chunk, pcm):
    eng = net._engine
    eng.configure_output(stage[0], zeros=stage[1])
    L, M, H = eng.output_plan
    width = eng.stream_rows_out_samples(chunk)
    states = [eng.output_history() for _ in utts.lengths]
    if stage == (8000, 64):
        assert states[0].buf.shape == (2, 705) and 705 > utts.up
    if stage[0] == 44100:
        assert states[0].buf.shape == (2, 0)
    got, ticks = [[] for _ in utts.lengths], schedule(utts, chunk, START)
    assert max(len(t) for t in ticks) >= 3 and len({f0 for t in ticks for _, f0, _ in t if len(t) > 1}) > 1
    for tick in ticks:
        rows = [(utts.z[b], utts.g[b], utts.lengths[b], f0, f1, states[b]) for b, f0, f1 in tick]
        sides = [s.side for _, _, _, _, _, s in rows]
        out, counts = eng.generator_stream_rows_output(rows, chunk, pcm=pcm)
        assert [s.side for _, _, _, _, _, s in rows] == [1 - s for s in sides]
        out = to_np(out)
        assert out.shape == (len(tick), width) and out.dtype == (np.int16 if pcm else np.float32)
        m0, m1, _, _ = eng.stream_rows_output_plan([(utts.lengths[b], f0, f1) for b, f0, f1 in tick])
        assert counts == [b - a for a, b in zip(m0, m1)]
        for k, (b, f0, f1) in enumerate(tick):
            assert not out[k, counts[k]:].any(), (b, f0, f1, "not zero behind the row's samples")
            got[b].append(out[k, : counts[k]])
    for b, Lf in enumerate(utts.lengths):
        mine = np.concatenate(got[b])
        assert mine.shape == (-(-Lf * utts.up * L // M),)
        want = one_shot(eng, float_runs[chunk][b], pcm)
        assert np.abs(want.astype(np.float64)).max() > (10 if pcm else 1e-3)
        np.testing.assert_array_equal(mine, want, err_msg=f"utterance of {Lf} frames")
    assert eng.status() == 0


def test_sixty_four_rows_of_one_frame(net):
    eng = net._engine
    eng.configure_output(22050)
    u = Utterances(net, [1] * 64, seed=2202)
    plain = [(u.z[b], u.g[b], 1, 0, 1) for b in range(64)]
    f = eng.generator_stream_rows(plain, 1, pcm=False)
    want, _ = eng.output(f, pcm=True)
    out, counts = eng.generator_stream_rows_output([r + (eng.output_history(),) for r in plain], 1, pcm=True)
    out = to_np(out)
    assert counts == [u.up // 2] * 64 and out.shape == (64, eng.stream_rows_out_samples(1))
    np.testing.assert_array_equal(out[:, : u.up // 2], to_np(want))
    assert not out[:, u.up // 2:].any() and np.abs(out).max() > 10
    assert len({out[b, : u.up // 2].tobytes() for b in range(64)}) == 64          # every row its own utterance


def raw_call(eng, row, hist_in, hist_out, out_stride, chunk=8):
    """One row through the C function itself, with history pointers as given."""
    z, g, Lf, f0, f1 = row
    arr = (eng_lib().VspStreamRowOut * 1)()
    arr[0].row.z, arr[0].row.z_channel_stride, arr[0].row.g = z.data_ptr(), max(int(z.stride(0)), Lf), g.data_ptr()
    arr[0].row.L, arr[0].row.f0, arr[0].row.f1 = Lf, f0, f1
    arr[0].hist_in, arr[0].hist_out = hist_in, hist_out
    out = torch.zeros((1, max(out_stride, 1)), dtype=torch.int16, device=eng.device)
    ws = eng._workspace("generator_stream_rows", eng.lib.vsp_generator_stream_rows_workspace_bytes(eng.ctx, 1, chunk))
    with torch.cuda.device(eng.device):
        return eng.lib.vsp_generator_stream_rows_output(eng.ctx, eng._stream(), 1, arr, C.c_void_p(out.data_ptr()), out_stride,
                                                        1, C.c_void_p(ws.data_ptr()), ws.numel())


def eng_lib():
    from vispeech_amd import _lib
    return _lib


def test_bad_calls_are_refused_before_any_launch(net, utts):
    eng = net._engine
    row0, row1 = (utts.z[3], utts.g[3], 33, 0, 8), (utts.z[3], utts.g[3], 33, 8, 16)
    eng.configure_output(None)
    assert raw_call(eng, row0, None, None, 4096) == -2                        # VSP_ERR_STATE: no output stage
    with pytest.raises(RuntimeError):
        eng.generator_stream_rows_output([row0 + (None,)], 8)
    eng.configure_output(22050)
    h = eng.output_history()
    a, b = h.buf[0].data_ptr(), h.buf[1].data_ptr()
    width = eng.stream_rows_out_samples(8)
    assert raw_call(eng, row1, a, a, width) == -1                             # hist_in == hist_out
    assert raw_call(eng, row1, a, None, width) == -1                          # no hist_out, K > 0
    assert raw_call(eng, row1, None, b, width) == -1                          # no hist_in, f0 > 0
    assert raw_call(eng, row0, None, b, width) == 0                           # f0 == 0: hist_in is ignored
    L, M, H = eng.output_plan
    done = output_stage.complete_outputs(8 * utts.up, L, M, H)
    assert raw_call(eng, row0, None, b, done - 1) == -5                       # VSP_ERR_SHAPE: the row completes `done` samples
    assert raw_call(eng, row0, None, b, done) == 0
    assert raw_call(eng, (utts.z[3], utts.g[3], 33, 8, 34), a, b, width) == -1
    torch.cuda.synchronize()
    assert eng.status() == 0


# ------------------------------------------------------------------ the service on the real net
FRAMES, PHON, SEEDS = [6, 40, 23], [2, 7, 5], [201, 202, 203]


def run_service(net, batch, **kw):
    """Rows 0 and 1 submitted while idle, row 2 after tick 2; driven by step().  Returns the per-request bytes."""
    from vispeech_amd.service import StreamingBatchService

    def collate(rows):
        return {k: batch[k][rows] for k in ("phonemes", "lengths", "sid", "duration", "f0", "energy")}
    svc = StreamingBatchService(net, max_batch=4, chunk_frames=16, collate=collate, autostart=False, output_rate=22050, **kw)
    streams = [svc.submit(0, SEEDS[0]), svc.submit(1, SEEDS[1])]
    svc.step(); svc.step()
    streams.append(svc.submit(2, SEEDS[2]))
    svc.close()
    assert svc.stats["rows_per_tick"] == [2, 1, 2, 1] and svc.stats["groups"] == 2
    return [b"".join(s) for s in streams]


def test_service_with_the_fused_output_stage(net, monkeypatch):
    batch = iso.make_batch(FRAMES, PHON, seed=2103)
    eng, up = net._engine, net.dims.total_upsample
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(net.device)
    calls = []
    real = eng.generator_stream_rows_output
    monkeypatch.setattr(eng, "generator_stream_rows_output", lambda *a, **k: (calls.append(len(a[0])), real(*a, **k))[1])
    fused = run_service(net, batch, fused_output=True)
    monkeypatch.undo()
    assert calls == [2, 1, 2, 1]                                               # one call per tick
    default = run_service(net, batch)
    o, *_ = net.infer(dev(batch["phonemes"]), dev(batch["lengths"]), sid=dev(batch["sid"]), noise_scale=0.667,
                      duration_control=dev(batch["duration"]), pitch_control=dev(batch["f0"]),
                      energy_control=dev(batch["energy"]), noise_seed=list(SEEDS), isolated=True)
    for b in range(3):
        want = to_np(eng.output(o[b:b + 1, 0, : FRAMES[b] * up], pcm=True)[0]).reshape(-1)
        mine = np.frombuffer(fused[b], dtype="<i2")
        assert mine.shape == want.shape == (FRAMES[b] * up // 2,)
        worst = int(np.abs(mine.astype(np.int64) - want.astype(np.int64)).max())
        print(f"request {b} at 22050 Hz, fused: worst {worst} PCM16 steps from Engine.output of the one-shot waveform")
        assert worst <= 1, (b, worst)
        assert fused[b] == default[b], f"request {b}: fused and per-request output stages differ"
