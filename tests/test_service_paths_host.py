"""Paths of the batching services that no other host test drives (no GPU): the streaming service's per-request output stage
(``output_rate`` without ``fused_output``) and a mixed batch of ``BatchingSynthesisService`` with an ``output_rate``, each
over a stand-in for the engine that records what it is asked for and computes in integers, so that bytes compare exactly."""
import numpy as np
import torch

from vispeech_amd import output_stage

UP = 4
LMH = (1, 2, 5)                                          # the stand-in stage: decimation by 2, eleven integer taps
TAPS = np.asarray([1, 2, 3, 4, 5, 6, 5, 4, 3, 2, 1], np.int64)       # h[-5 .. 5]


def resample_ref(x, m0, m1, sample_first=0):
    """y[m] = sum_k h[m M - k L] x[k] for m in [m0, m1), x holding samples [sample_first, ...), zero outside."""
    L, M, H = LMH
    y = np.zeros(m1 - m0, np.int64)
    for m in range(m0, m1):
        for k in range(-(-(m * M - H) // L), (m * M + H) // L + 1):
            if sample_first <= k < sample_first + len(x):
                y[m - m0] += TAPS[m * M - k * L + H] * int(x[k - sample_first])
    return y


def _collate(rows):
    return {"phonemes": np.zeros((len(rows), 1), np.int64), "lengths": np.asarray([r["frames"] for r in rows]),
            "sid": np.asarray([r["id"] for r in rows])}


# ---------------------------------------------------------------------------------------------- streaming, per request
class StreamEngine:
    """A request is a dict(id, frames); its latent holds 10 * id + frame and the 'waveform' of a frame is UP copies of that
    number.  ``generator_stream_rows`` returns the float frames, ``output_chunk`` filters a window with ``resample_ref``:
    a window that lacks a sample its outputs need gives other bytes than the one-shot filter."""

    output_plan = LMH

    def __init__(self):
        self.ticks, self.chunks = [], []

    def configure_output(self, out_rate, in_rate=None):
        self.configured = (out_rate, in_rate)

    def encode(self, phonemes, lengths, sid, duration, f0, energy, isolated=False):
        ids = [int(x) for x in np.asarray(sid)]
        return {"frame_lengths": [int(x) for x in np.asarray(lengths)], "g": np.asarray(ids, np.float32).reshape(-1, 1),
                "ids": ids}

    def frame_lengths_host(self, fl):
        return list(fl), max(fl)

    def decode(self, enc, tf, noise, noise_scale, max_len=None, noise_seed=None, isolated=False):
        return {"z": np.stack([10 * i + np.arange(tf, dtype=np.float32)[None, :] for i in enc["ids"]])}

    def generator_stream_rows(self, rows, chunk_frames, pcm=True):
        assert not pcm                                    # the output stage takes the float chunk
        out = torch.zeros((len(rows), chunk_frames * UP), dtype=torch.float32)
        for b, (z, g, L, f0, f1) in enumerate(rows):
            assert 0 <= f0 < f1 <= L and f1 - f0 <= chunk_frames
            out[b, : (f1 - f0) * UP] = torch.from_numpy(np.repeat(z[0, f0:f1], UP))
        self.ticks.append([(int(g[0]), L, f0, f1) for _, g, L, f0, f1 in rows])
        return out

    def output_chunk(self, x, x_first, n_max, m0, m1, n_valid=None, pcm=True):
        assert pcm and n_valid is None and x.shape[0] == 1 and x_first + x.shape[1] == n_max and m1 > m0
        self.chunks.append((x_first, int(x.shape[1]), m0, m1))
        return resample_ref(np.asarray(x[0]).astype(np.int64), m0, m1, x_first).astype(np.int16)[None, :]

    def output_stream(self, chunks, n_valid=None, pcm=True):
        return output_stage.stream(self, chunks, n_valid, pcm)

    def generator_stream_rows_output(self, *a, **k):
        raise AssertionError("without fused_output the tick must not run the fused stage")


class StreamNet:
    class dims:
        total_upsample = UP

    def __init__(self):
        self._engine = StreamEngine()


def _streaming(**kw):
    from vispeech_amd.service import StreamingBatchService
    net = StreamNet()
    svc = StreamingBatchService(net, collate=_collate, autostart=False, output_rate=22050, **kw)
    assert net._engine.configured == (22050, 44100) and not svc.fused_output
    return svc, net._engine


def _one_shot(rid, frames):
    """The one-shot filter of the request's own waveform."""
    x = np.repeat(10 * rid + np.arange(frames), UP)
    return resample_ref(x, 0, -(-len(x) * LMH[0] // LMH[1])).astype("<i2").tobytes()


def _pieces(stream):
    pieces = list(stream)
    assert all(len(p) > 0 for p in pieces), "an empty piece reached the queue"
    return pieces


def test_streaming_output_stage_first_window_completes_nothing():
    svc, eng = _streaming(chunk_frames=1)
    assert output_stage.complete_outputs(UP, *LMH) == 0               # H = 5: the first frame's 4 samples complete nothing
    a = svc.submit({"id": 4, "frames": 3}, 1)
    svc.close()
    pieces = _pieces(a)
    assert svc.stats["ticks"] == len(eng.ticks) == 3 and len(pieces) == 2      # three ticks, two pieces
    assert b"".join(pieces) == _one_shot(4, 3)
    # the held-back window went out together with the second one; the third call is the last window and the tail
    assert [c[:2] for c in eng.chunks[:1]] == [(0, 2 * UP)]


def test_streaming_output_stage_requests_join_and_leave():
    svc, eng = _streaming(chunk_frames=4)
    a = svc.submit({"id": 1, "frames": 18}, 7)
    svc.step(); svc.step()
    b = svc.submit({"id": 2, "frames": 5}, 8)
    c = svc.submit({"id": 3, "frames": 1}, 9)                          # ends in its first tick: the whole of it is tail
    svc.close()
    assert eng.ticks == [
        [(1, 18, 0, 4)], [(1, 18, 4, 8)], [(1, 18, 8, 12), (2, 5, 0, 4), (3, 1, 0, 1)], [(1, 18, 12, 16), (2, 5, 4, 5)],
        [(1, 18, 16, 18)]]
    assert svc.stats["rows_per_tick"] == [1, 1, 3, 2, 1]
    for s, (rid, frames) in ((a, (1, 18)), (b, (2, 5)), (c, (3, 1))):
        assert b"".join(_pieces(s)) == _one_shot(rid, frames), rid


def test_streaming_output_stage_short_first_chunk():
    svc, eng = _streaming(chunk_frames=4, first_chunk_frames=1)
    a, b = svc.submit({"id": 5, "frames": 11}, 1), svc.submit({"id": 6, "frames": 2}, 2)
    svc.close()
    assert eng.ticks[:2] == [[(5, 11, 0, 1), (6, 2, 0, 1)], [(5, 11, 1, 5), (6, 2, 1, 2)]]
    assert [t[0][2:] for t in eng.ticks] == [(0, 1), (1, 5), (5, 9), (9, 11)]
    pa, pb = _pieces(a), _pieces(b)
    assert len(pa) == 3 and len(pb) == 1                              # the one-frame first window completes nothing
    assert b"".join(pa) == _one_shot(5, 11) and b"".join(pb) == _one_shot(6, 2)


# ---------------------------------------------------------------------------------------------- batching, mixed batch
HOP, PAD = 10, 15             # the stand-in's front end: T(n) = 0 up to PAD samples, n // HOP behind


class RecordingEngine:
    """Records what the service asks for.  A text request is a dict(id, frames), a conversion a recording of n samples to
    speaker tgt; a request's latent holds (100 * id + frame) / 32767 with id = the text request's id or the target speaker,
    and the 'output stage' keeps every second sample: the PCM16 names the request, the frame and the stage."""

    def __init__(self):
        self.calls = []

    def configure_output(self, out_rate, in_rate=None):
        self.calls.append(("configure_output", out_rate, in_rate))

    def encode(self, phonemes, lengths, sid, duration, f0, energy, isolated=False):
        assert isolated
        ids = [int(x) for x in np.asarray(sid)]
        self.calls.append(("encode", ids))
        return {"frame_lengths": [int(x) for x in np.asarray(lengths)],
                "g": torch.tensor(ids, dtype=torch.float32).reshape(-1, 1), "ids": ids}

    def frame_lengths_host(self, fl):
        return list(fl), max(fl)

    def decode(self, enc, tf, noise, noise_scale, max_len=None, noise_seed=None, isolated=False):
        assert isolated and noise is None
        self.calls.append(("decode", max_len, list(noise_seed)))
        return {"z": torch.stack([(100 * i + torch.arange(tf, dtype=torch.float32))[None, :] / 32767.0 for i in enc["ids"]])}

    def convert_frames(self, n):
        return 0 if n <= PAD else n // HOP

    def convert_latent(self, audio, n_samples, sid_src, sid_tgt, noise=None, noise_seed=None, noise_scale=1.0):
        n = [int(x) for x in n_samples]
        assert noise is None and audio.shape == (len(n), max(n)) and audio.dtype == np.float32
        self.calls.append(("convert_latent", n, list(sid_tgt), list(noise_seed), float(noise_scale)))
        frames = [self.convert_frames(x) for x in n]
        z = torch.stack([(100 * t + torch.arange(max(frames), dtype=torch.float32))[None, :] / 32767.0 for t in sid_tgt])
        return {"z_hat": z, "g": torch.tensor(list(sid_tgt), dtype=torch.float32).reshape(-1, 1), "frames_host": frames}

    def generator_ragged(self, z, g, lengths):
        self.calls.append(("generator_ragged", [int(x) for x in g.reshape(-1)], list(lengths), tuple(z.shape)))
        return torch.repeat_interleave(z[:, :1, :], UP, dim=2)

    def output(self, x, sample_lengths=None, pcm=True):
        assert pcm and sample_lengths is None and x.dim() == 2 and x.shape[0] == 1
        self.calls.append(("output", int(round(float(x[0, 0]) * 32767.0)) // 100, int(x.shape[1])))
        return torch.round(x[:, ::2] * 32767.0).to(torch.int16), None


class RecordingNet:
    class dims:
        total_upsample = UP

    device = "cpu"

    def __init__(self):
        self._engine = RecordingEngine()

    def infer(self, *a, **k):
        raise AssertionError("a batch with conversions does not go through net.infer")


def _audio(n):
    return np.linspace(-0.5, 0.5, n, dtype=np.float32)


def test_batching_mixed_batch_with_an_output_rate():
    from vispeech_amd.service import BatchingSynthesisService
    net = RecordingNet()
    eng = net._engine
    svc = BatchingSynthesisService(net, max_batch=6, max_wait_s=30.0, collate=_collate, output_rate=22050)
    try:
        futs = [svc.submit({"id": 1, "frames": 6}, 7),
                svc.submit_conversion(_audio(93), 3, 5, 21, noise_scale=0.5),       # 9 frames, to speaker 5
                svc.submit_conversion(_audio(PAD), 3, 9, 23),                       # too short for one frame
                svc.submit({"id": 2, "frames": 3}, 8),
                svc.submit_conversion(_audio(50), 4, 6, 22),                        # 5 frames; the default scale, 1.0
                svc.submit_conversion(_audio(40), 4, 7, 24, noise_scale=0.5)]       # 4 frames; shares the call of the first
        got = [f.result(60) for f in futs]
    finally:
        svc.close()
    assert eng.calls == [
        ("configure_output", 22050, 44100),
        ("encode", [1, 2]), ("decode", 0, [7, 8]),                                  # one pair for the text rows
        ("convert_latent", [93, 40], [5, 7], [21, 24], 0.5),                        # one call per scale, ascending
        ("convert_latent", [50], [6], [22], 1.0),
        ("generator_ragged", [1, 5, 2, 6, 7], [6, 9, 3, 5, 4], (5, 1, 9)),          # one call, request order
        ("output", 1, 6 * UP), ("output", 5, 9 * UP), ("output", 2, 3 * UP), ("output", 6, 5 * UP), ("output", 7, 4 * UP),
    ]
    expect = lambda rid, frames: np.repeat(100 * rid + np.arange(frames), UP)[::2].astype("<i2")
    want = [expect(1, 6), expect(5, 9), np.zeros(0, "<i2"), expect(2, 3), expect(6, 5), expect(7, 4)]
    assert all(g.dtype == np.dtype("<i2") and g.ndim == 1 for g in got)
    assert got[2].size == 0
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
