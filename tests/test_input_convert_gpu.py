"""Voice conversion from raw recordings on the GPU: ``convert_audio``, ``BatchingSynthesisService`` and live sessions of
``StreamingBatchService`` fed PCM16 / G.711 / float32 at the caller's rate, against the same calls fed the input stage's
one-shot result as float32 at the model's rate -- bit for bit: the code behind the input stage is unchanged (and pinned to
the oracle by tests/test_convert_gpu.py and tests/test_live_convert_gpu.py), so the input stage is the sole difference.
The small configuration of ``live_convert_ref``.

Where two runs differ in MORE than the input stage -- a request alone against the same request in a group, a feed cut in
another way, so that its ticks hold other windows -- the code behind the stage does not promise the same bits (its tests pin
it to the oracle within ``WAVE_TOL``), and two results that each lie within that bound of the oracle's lie within
``pcm_steps`` of each other; measured on the MI355X: at most 1 step."""
import numpy as np
import pytest
import torch

import input_stage_ref as isr
import isolated_ref as iso
import live_convert_ref as ref
from input_stage_ref import F32, S16, ULAW
from live_convert_ref import HOP, UP
from test_convert_gpu import WAVE_TOL
from vispeech_amd import input_stage, output_stage

pytestmark = pytest.mark.gpu

SRC, TGT = 5, 9
MODEL = 22050                           # the small configuration's sampling rate


def to_np(t):
    return t.detach().cpu().numpy()


class Net:
    """What ``convert_audio`` and the services need of a model: the engine, its dimensions and the speaker count."""
    device = "cuda:0"

    def __init__(self, eng, dims):
        self._engine, self.dims, self.n_speakers = eng, dims, dims.n_speakers

    def convert_audio(self, *a, **k):
        from vispeech_amd.models import SynthesizerTrn
        return SynthesizerTrn.convert_audio(self, *a, **k)


@pytest.fixture(scope="module")
def dims():
    d = ref.small_dims()
    assert d.sampling_rate == MODEL
    return d


@pytest.fixture(scope="module")
def eng(dims):
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from vispeech_amd.engine import Engine
    e = Engine(dims)
    e.set_weights(ref.small_weights(dims), strict=True)
    e.finalize()
    for rate in (16000, 48000, 8000):
        e.configure_input(rate)
    return e


@pytest.fixture(scope="module")
def net(eng, dims):
    return Net(eng, dims)


def speech(n, seed, rate):
    """``live_convert_ref.recording`` sampled at ``rate``: float32 in [-1, 1]."""
    return ref.recording(n, seed, rate=float(rate))


def as_s16(x):
    return np.clip(np.rint(x * 32767.0), -32768, 32767).astype(np.int16)


def as_ulaw(x):
    """The nearest mu-law code of every sample (by the decoding table: no encoder is under test)."""
    table = input_stage.decode_table(ULAW).astype(np.float64)
    return np.abs(x.astype(np.float64)[:, None] - table[None, :]).argmin(axis=1).astype(np.uint8)


def pcm_steps(pcm):
    """How far apart two PCM16 results may lie that are both within ``check_pcm``'s bound of the same reference."""
    return 2 * (int(np.ceil(WAVE_TOL * float(np.abs(pcm).max()))) + 1)


def resampled(eng, raw, rate, enc):
    """The input stage's one-shot result of one recording, on the host."""
    return to_np(input_stage.one_shot(eng, eng._raw(raw, enc), len(raw), rate, enc))


# ---------------------------------------------------------------------------------------------- convert_audio
def test_convert_audio_from_pcm16_is_convert_audio_of_the_resampled_batch(net, eng):
    n_in = [5000, 7111, 12000]
    raw = np.full((3, max(n_in) + 13), 0x7FFF, np.int16)
    for b, n in enumerate(n_in):
        raw[b, :n] = as_s16(speech(n, 60 + b, 16000))
    seeds = [11, 12, 13]
    got = net.convert_audio(raw, n_in, [SRC] * 3, [TGT, TGT + 1, TGT], noise_seed=seeds, sample_rate=16000, encoding="s16")
    audio, n_out = eng.input_batch(raw, n_in, 16000, S16)
    assert eng.input_plan(16000) == (441, 320, 32 * 441) and n_out == [isr.out_len(n, 441, 320) for n in n_in] and audio.shape == (3, max(n_out))
    want = net.convert_audio(audio, n_out, [SRC] * 3, [TGT, TGT + 1, TGT], noise_seed=seeds)
    frames = [ref.frames_of(n) for n in n_out]
    assert got[0].shape == (3, 1, max(frames) * UP) and min(frames) > 20
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    for a, b in zip(got[2], want[2]):
        assert torch.equal(a, b)
    o = to_np(got[0])
    assert np.isfinite(o).all() and all(np.abs(o[b, 0, : frames[b] * UP]).max() > 1e-3 for b in range(3))


# ---------------------------------------------------------------------------------------------- the batching service
def test_batching_service_mixes_formats(net, eng):
    from vispeech_amd.service import BatchingSynthesisService
    jobs = [(as_s16(speech(4000, 70, 16000)), dict(sample_rate=16000, encoding="s16"), 16000, S16),
            (speech(9000, 71, 48000), dict(sample_rate=48000), 48000, F32),
            (speech(7000, 72, MODEL), {}, None, None)]
    floats = [x if rate is None else resampled(eng, x, rate, enc) for x, _, rate, enc in jobs]

    def run(max_batch, items):
        svc = BatchingSynthesisService(net, max_batch=max_batch, max_wait_s=30.0, collate=lambda rows: None, sampling_rate=MODEL)
        try:
            return [f.result(120) for f in [svc.submit_conversion(x, SRC, TGT, 21 + i, **kw) for i, x, kw in items]]
        finally:
            svc.close()

    got = run(3, [(i, x, kw) for i, (x, kw, _, _) in enumerate(jobs)])
    # the same group fed what each request's own B = 1 input call returns: the input stage is the sole difference
    same_group = run(3, [(i, x, {}) for i, x in enumerate(floats)])
    for i, (g, w, x) in enumerate(zip(got, same_group, floats)):
        assert g.dtype == np.dtype("<i2") and g.size == ref.frames_of(len(x)) * UP and g.size > 10 * UP
        assert np.abs(g).max() > 30
        np.testing.assert_array_equal(g, w)
        (alone,) = run(1, [(i, jobs[i][0], jobs[i][1])])                          # ... and the request served alone
        worst = int(np.abs(g.astype(np.int32) - alone).max())
        print(f"request {i}: max |group - alone| = {worst} of {np.abs(g).max()}, bound {pcm_steps(alone)}")
        assert alone.shape == g.shape and worst <= pcm_steps(alone)


# ---------------------------------------------------------------------------------------------- live sessions
N_MODEL = 100 * HOP + 77                # about 100 frames at the model's rate


TEXT_AT = 3                             # the step at which the text request joins: both sessions have had their first 4097 samples


def live_run(net, plan, text=None, **service):
    """One ``StreamingBatchService`` driven by hand: ``plan`` is per session (seed, open_conversion keywords, the pieces of
    every step, a last piece fed together with the end); a step follows every round of pieces, the sessions are ended, and
    the service runs dry.  ``text``: (collate, seed) of a text request that joins at step TEXT_AT."""
    from vispeech_amd.service import StreamingBatchService
    collate = (lambda rows: None) if text is None else text[0]
    svc = StreamingBatchService(net, chunk_frames=16, first_chunk_frames=4, collate=collate, autostart=False, sampling_rate=MODEL,
                                **service)
    sessions = [svc.open_conversion(SRC, TGT, seed, **kw) for seed, kw, _, _ in plan]
    streams = []
    for k in range(max(len(pieces) for _, _, pieces, _ in plan)):
        if text is not None and k == TEXT_AT:
            streams.append(svc.submit(0, text[1]))
        for s, (_, _, pieces, _) in zip(sessions, plan):
            if k < len(pieces) and len(pieces[k]):
                s.feed(pieces[k])
        svc.step()
    for s, (_, _, _, last) in zip(sessions, plan):
        if last is not None and len(last):
            s.feed(last)
        s.end()
    while svc.step():
        pass
    assert svc._live == []
    return [b"".join(s) for s in sessions + streams], svc.stats


def cut(x, sizes):
    out, at, k = [], 0, 0
    while at < len(x):
        out.append(x[at:at + sizes[k % len(sizes)]])
        at, k = at + sizes[k % len(sizes)], k + 1
    return out


def float_pieces(eng, raw_pieces, rate, whole):
    """The one-shot resampled recording cut where the raw feed's pieces complete it: the float session then knows, at
    every tick, exactly the samples the raw session knows, and its tail arrives with the last piece."""
    L, M, H = eng.input_plan(rate)
    out, seen, m = [], 0, 0
    for p in raw_pieces:
        seen += len(p)
        m1 = output_stage.complete_outputs(seen, L, M, H)
        out.append(whole[m:m1])
        m = m1
    return out, whole[m:]


@pytest.fixture(scope="module")
def live_inputs(eng):
    """(raw, rate, encoding, one-shot float) of the two recordings: 16 kHz PCM16 and 8 kHz mu-law, about 100 frames each."""
    a = as_s16(speech(N_MODEL * 320 // 441, 80, 16000))
    b = as_ulaw(speech(N_MODEL * 160 // 441, 81, 8000))
    out = [(a, 16000, S16, resampled(eng, a, 16000, S16)), (b, 8000, ULAW, resampled(eng, b, 8000, ULAW))]
    assert [ref.frames_of(len(w)) for _, _, _, w in out] == [100, 100]
    return out


def text_request(eng, dims):
    batch = iso.make_batch([40], [8], seed=2150)
    batch["phonemes"] = batch["phonemes"] % (dims.n_vocab - 1) + 1
    batch["sid"] = batch["sid"] % dims.n_speakers
    return (lambda rows: {k: batch[k][rows] for k in ("phonemes", "lengths", "sid", "duration", "f0", "energy")}), 301


def test_live_sessions_fed_raw_pieces_deliver_the_bytes_of_the_resampled_recording(net, eng, dims, live_inputs):
    kws = [dict(sample_rate=16000, encoding="s16"), dict(sample_rate=8000, encoding="ulaw")]
    raw_plan, float_plan = [], []
    for i, ((raw, rate, enc, whole), kw) in enumerate(zip(live_inputs, kws)):
        pieces = cut(raw, (1, 255, 4097))
        raw_plan.append((31 + i, kw, pieces, None))
        fp, tail = float_pieces(eng, pieces, rate, whole)
        # the tail is complete only once the recording has ended: the float session gets it as its last piece, which the
        # worker takes together with the end -- as the raw session's flush arrives
        float_plan.append((31 + i, {}, fp, tail))
    text = text_request(eng, dims)
    got, stats = live_run(net, raw_plan, text)
    want, stats_f = live_run(net, float_plan, text)
    assert len(raw_plan[1][2]) > TEXT_AT and max(stats["rows_per_tick"]) == 3       # both sessions share a tick with the text
    assert stats["rows_per_tick"] == stats_f["rows_per_tick"]
    for g, w, (_, _, _, whole) in zip(got[:2], want[:2], live_inputs):
        assert len(g) == 2 * 100 * UP
        assert g == w
    assert got[2] == want[2] and len(got[2]) == 2 * 40 * UP
    # however the feed is cut: two pieces give the bytes of the float session cut alike ...
    halves = [[raw[:3000], raw[3000:]] for raw, _, _, _ in live_inputs]
    other, _ = live_run(net, [(31 + i, kw, h, None) for i, (h, kw) in enumerate(zip(halves, kws))])
    plan = []
    for i, (h, (_, rate, _, whole)) in enumerate(zip(halves, live_inputs)):
        fp, tail = float_pieces(eng, h, rate, whole)
        plan.append((31 + i, {}, fp, tail))
    other_f, _ = live_run(net, plan)
    for i, (g, o, f) in enumerate(zip(got[:2], other, other_f)):
        assert o == f
        # ... and, their ticks holding other windows, the bytes of the first cut within the bound of the code behind the stage
        a, b = np.frombuffer(g, "<i2").astype(np.int32), np.frombuffer(o, "<i2").astype(np.int32)
        print(f"session {i}: max |pieces - two halves| = {np.abs(a - b).max()} of {np.abs(a).max()}, bound {pcm_steps(a)}")
        assert a.shape == b.shape and np.abs(a - b).max() <= pcm_steps(a)


def test_live_session_fed_raw_pieces_at_an_output_rate(net, eng, live_inputs):
    raw, rate, enc, whole = live_inputs[0]
    pieces = cut(raw, (1, 255, 4097))
    fp, tail = float_pieces(eng, pieces, rate, whole)
    try:
        got, _ = live_run(net, [(41, dict(sample_rate=16000, encoding="s16"), pieces, None)], output_rate=11025, fused_output=True)
        want, _ = live_run(net, [(41, {}, fp, tail)], output_rate=11025, fused_output=True)
    finally:
        eng.configure_output(None)
    assert len(got[0]) == 2 * output_stage.out_len(100 * UP, 1, 2) and got[0] == want[0]
