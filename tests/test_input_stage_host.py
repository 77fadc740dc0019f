"""Input stage, host side (no GPU): the plan, the taps and the G.711 tables of the library against the restatement in
``input_stage_ref``; ``input_stage.Stream`` against an engine whose arithmetic is the fp64 sum; what ``vsp_input_rows``
refuses without a configured rate; and the host logic of the services -- which calls a request with a sample rate or an
encoding adds, and that a request without them makes the calls it always made."""
import ctypes as C

import numpy as np
import pytest
import torch

import input_stage_ref as ref
import test_live_convert_host as live_host
import test_service_paths_host as paths_host
from live_convert_ref import HOP, frames_of
from vispeech_amd import _lib, input_stage, output_stage

MODEL = ref.MODEL_RATE


def _plan(in_rate, model_rate, zeros):
    L, M, H = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    rc = _lib.lib().vsp_input_plan(in_rate, model_rate, zeros, C.byref(L), C.byref(M), C.byref(H))
    return rc, L.value, M.value, H.value


def test_plan_matches_the_table_and_refuses_what_is_not_covered():
    lib = _lib.lib()
    for rate, (L, M) in ref.TABLE.items():
        H = 0 if rate == MODEL else 32 * max(L, M)
        assert _plan(rate, MODEL, 32) == (0, L, M, H), rate
        assert ref.plan(rate) == (L, M, H) == input_stage.plan(rate, MODEL)
    assert _plan(16000, MODEL, 0) == (0, 441, 160, 32 * 441)                 # zeros == 0: the default
    assert _plan(16000, MODEL, 64)[0] == 0 and _plan(16000, MODEL, 1) == (0, 441, 160, 441)
    assert _plan(MODEL, 44200, 32)[0] == -7 and ref.plan(MODEL, 44200) is None          # L = 442 (M = 441)
    assert _plan(44200, MODEL, 32) == (0, 441, 442, 32 * 442)                # (the other way round both are covered)
    assert _plan(641, 1, 32)[0] == -7 and ref.plan(641, 1) is None           # M = 641
    assert _plan(640, 1, 32) == (0, 1, 640, 32 * 640)
    assert _plan(16000, MODEL, 65)[0] == -7 and ref.plan(16000, MODEL, 65) is None
    # the output stage's own limits are where they were
    assert lib.vsp_resample_plan(MODEL, 44000, 32, C.byref(C.c_int()), C.byref(C.c_int()), C.byref(C.c_int())) == -7
    for bad in ((0, MODEL, 32), (16000, 0, 32), (-1, MODEL, 32), (16000, -5, 32), (16000, MODEL, -3)):
        assert _plan(*bad)[0] == -1, bad
    L, M, H = C.c_int(), C.c_int(), C.c_int()
    assert lib.vsp_input_plan(16000, MODEL, 32, None, C.byref(M), C.byref(H)) == -1
    assert lib.vsp_input_plan(16000, MODEL, 32, C.byref(L), C.byref(M), None) == -1
    one = np.zeros(1, np.float32)
    p = one.ctypes.data_as(C.c_void_p)
    assert lib.vsp_input_filter(MODEL, MODEL, 32, 9.62, 0.0, p) == 0 and one[0] == 1.0      # the pass-through: one unit tap
    assert lib.vsp_input_filter(16000, MODEL, 32, 9.62, 0.0, None) == -1
    assert lib.vsp_input_filter(16000, MODEL, 32, -1.0, 0.0, p) == -1
    assert lib.vsp_input_filter(16000, MODEL, 32, 9.62, 1.5, p) == -1
    assert lib.vsp_input_filter(MODEL, 44200, 32, 9.62, 0.0, p) == -7


@pytest.mark.parametrize("rate,zeros", [(16000, 32), (8000, 32), (32000, 32), (48000, 32), (96000, 32), (192000, 16), (22050, 32)])
def test_taps_are_the_formula(rate, zeros):
    L, M, H = ref.plan(rate, MODEL, zeros)
    h = input_stage.taps(rate, MODEL, zeros)
    want = ref.filter_fp64(rate, MODEL, zeros)
    assert h.dtype == np.float32 and h.shape == want.shape == (2 * H + 1,)
    assert np.all(np.abs(h.astype(np.float64) - want) <= 2.0 ** -23 * np.abs(want) + 1e-12)
    np.testing.assert_array_equal(h, h[::-1])
    np.testing.assert_array_equal(input_stage.taps(rate, MODEL, zeros, 9.62, 1.0 - 3.065 / zeros), h)
    # unity gain: every phase of an up-sampler sums to about 1 (DC gain L of the prototype)
    assert abs(h.astype(np.float64).sum() / L - 1.0) <= 1e-3


def test_decode_tables_are_g711():
    lib = _lib.lib()
    codes = np.arange(256)
    for enc, rule in ((ref.ULAW, ref.ulaw_linear), (ref.ALAW, ref.alaw_linear)):
        t = input_stage.decode_table(enc)
        assert t.dtype == np.float32 and t.shape == (256,)
        np.testing.assert_array_equal(t.astype(np.float64) * 32768.0, rule(codes))
        np.testing.assert_array_equal(t, ref.decode(codes.astype(np.uint8), enc))
        assert len(set(np.abs(rule(codes)).tolist())) == 128 and np.array_equal(np.sort(rule(codes)), np.sort(-rule(codes)))
    u, a = input_stage.decode_table("ulaw") * 32768.0, input_stage.decode_table("alaw") * 32768.0
    assert (u[0xFF], u[0x7F], u[0x80], u[0x00]) == (0, 0, 32124, -32124)
    assert (a[0xD5], a[0x55], a[0xAA], a[0x2A]) == (8, -8, 32256, -32256)
    t = np.zeros(256, np.float32)
    for enc in (ref.F32, ref.S16, 4, -1):
        assert lib.vsp_input_decode_table(enc, t.ctypes.data_as(C.c_void_p)) == -1
    assert lib.vsp_input_decode_table(ref.ULAW, None) == -1
    with pytest.raises(ValueError):
        input_stage.encoding("opus")
    assert [input_stage.encoding(e) for e in (None, "f32", "s16", "PCM16", "ulaw", "alaw", 3)] == [0, 0, 1, 1, 2, 3, 3]
    assert input_stage.as_raw(np.int16([1, -2]).tobytes(), ref.S16).tolist() == [1, -2]
    with pytest.raises(ValueError):
        input_stage.as_raw(np.zeros(3, np.float32), ref.S16)


def test_rows_are_refused_without_a_configured_rate():
    lib = _lib.lib()
    cfg = _lib.make_config(__import__("vispeech_amd.schema", fromlist=["ModelDims"]).ModelDims())
    h = C.c_void_p()
    assert lib.vsp_create(C.byref(cfg), 0, C.byref(h)) == 0
    row = (_lib.VspInputRow * 1)()
    row[0].in_, row[0].in_len, row[0].n_total, row[0].out, row[0].m1, row[0].out_fill = 16, 8, 8, 16, 4, 4
    assert lib.vsp_input_rows(None, None, 16000, ref.S16, 1, row) == -1
    assert lib.vsp_input_rows(h, None, 16000, ref.S16, 1, row) == -2
    assert b"not configured" in lib.vsp_last_error(h)
    assert lib.vsp_input_configure(h, MODEL, 44200, 32, 9.62, 0.0) == -7           # refused before any device call
    assert lib.vsp_input_configure(h, 16000, MODEL, 65, 9.62, 0.0) == -7
    assert lib.vsp_input_configure(h, 0, MODEL, 32, 9.62, 0.0) == -1
    assert lib.vsp_input_configure(h, 16000, MODEL, 32, -1.0, 0.0) == -1
    assert lib.vsp_input_configure(h, 16000, 0, 32, 9.62, 0.0) == 0                # dropping a rate that is not there
    assert lib.vsp_input_configure(None, 16000, MODEL, 32, 9.62, 0.0) == -1
    lib.vsp_destroy(h)


# ---------------------------------------------------------------------------------------------- Stream
class RefEngine:
    """An engine whose input stage is the fp64 sum over the library's own taps (numpy in, numpy out).  What lies outside a
    row's window is NaN to it: a window that lacks a needed sample shows."""

    def __init__(self, rate, zeros=32):
        self.rate, self.plan = rate, ref.plan(rate, MODEL, zeros)
        self.h = input_stage.taps(rate, MODEL, zeros).astype(np.float64)
        self.calls = []

    def input_plan(self, rate):
        assert rate == self.rate
        return self.plan

    def input_rows(self, rows, rate, enc):
        L, M, H = self.input_plan(rate)
        out = []
        for raw, first, n_total, m0, m1 in rows:
            n = first + len(raw) if n_total < 0 else n_total
            assert first + len(raw) <= n and m1 <= output_stage.complete_outputs(first + len(raw), L, M, H, ended=n_total >= 0)
            self.calls.append((first, len(raw), n_total, m0, m1))
            x = np.full(n, np.nan)
            x[first:first + len(raw)] = ref.decode(raw, enc)
            y = ref.out_ref.resample_fp64(x, self.h, L, M, m0, m1)
            assert np.isfinite(y).all()
            out.append(y)
        return out


SPLITS = [(1,), (7,), (159, 160, 161), (1, 2, 159, 160, 161, 1024, 3), (4000,), (93, 1, 1, 3000)]


@pytest.mark.parametrize("rate,enc", [(16000, ref.S16), (48000, ref.F32), (8000, ref.ALAW), (22050, ref.ULAW), (44100, ref.S16)])
def test_stream_equals_one_shot_under_any_split(rate, enc):
    eng = RefEngine(rate)
    L, M, H = eng.plan
    rng = np.random.default_rng(rate + enc)
    for n in (0, 1, 93, 1601):
        raw = ref.random_raw(rng, n, enc)
        whole = input_stage.one_shot(eng, raw, n, rate, enc)
        assert whole.shape == (ref.out_len(n, L, M),)
        if rate == MODEL:
            np.testing.assert_array_equal(whole, ref.decode(raw, enc))
        for sizes in SPLITS if n < 1000 else SPLITS[2:]:       # (sample by sample: the short recordings only)
            s = input_stage.Stream(eng, rate, enc)
            got, at, k = [], 0, 0
            while at < n:
                y = s.push(raw[at:at + sizes[k % len(sizes)]])
                at, k = at + sizes[k % len(sizes)], k + 1
                assert len(s.hist) <= (2 * H) // L and s.first + len(s.hist) == min(at, n)
                got += [] if y is None else [y]
            tail = s.finish()
            got += [] if tail is None else [tail]
            assert s.finish() is None
            np.testing.assert_array_equal(np.concatenate(got) if got else np.zeros(0), whole)
    assert list(input_stage.stream(eng, [raw[:100], raw[100:]], rate, enc))[0].shape[0] > 0


# ---------------------------------------------------------------------------------------------- the services' calls
class InputRecordingEngine(paths_host.RecordingEngine):
    """``RecordingEngine`` with an input stage that doubles the sample count and records its calls."""
    device = "cpu"

    def __init__(self):
        super().__init__()
        self.input_rates = ()

    def configure_input(self, rate, model_rate=None):
        assert model_rate == MODEL
        self.calls.append(("configure_input", rate))
        self.input_rates += (rate,)

    def input_batch(self, raw, n_in, rate, enc):
        assert raw.dtype == ref.DTYPES[enc] and raw.shape[0] == len(n_in)
        self.calls.append(("input_batch", rate, enc, list(n_in)))
        n_out = [2 * n for n in n_in]
        return torch.zeros((len(n_in), max(n_out))), n_out

    def convert_latent(self, audio, n_samples, *a, **k):
        return super().convert_latent(np.asarray(audio), n_samples, *a, **k)


def _mixed_batch(eng_cls, formats):
    from vispeech_amd.service import BatchingSynthesisService
    net = paths_host.RecordingNet()
    net._engine = eng = eng_cls()
    svc = BatchingSynthesisService(net, max_batch=5, max_wait_s=30.0, collate=paths_host._collate, output_rate=22050)
    try:
        futs = [svc.submit({"id": 1, "frames": 6}, 7)]
        for (n, src, tgt, seed), fmt in zip(((93, 3, 5, 21), (50, 4, 6, 22), (40, 4, 7, 24), (60, 4, 8, 25)), formats):
            audio = paths_host._audio(n) if fmt is None or fmt.get("encoding") in (None, "f32") else np.zeros(n, np.int16)
            futs.append(svc.submit_conversion(audio, src, tgt, seed, **(fmt or {})))
        got = [f.result(60) for f in futs]
    finally:
        svc.close()
    return eng.calls, got


def test_batching_service_without_the_keywords_makes_the_calls_it_always_made():
    calls, _ = _mixed_batch(paths_host.RecordingEngine, [None] * 4)        # (an engine without an input stage at all)
    UP = paths_host.UP
    assert calls == [
        ("configure_output", 22050, 44100),
        ("encode", [1]), ("decode", 0, [7]),
        ("convert_latent", [93, 50, 40, 60], [5, 6, 7, 8], [21, 22, 24, 25], 1.0),
        ("generator_ragged", [1, 5, 6, 7, 8], [6, 9, 5, 4, 6], (5, 1, 9)),
        ("output", 1, 6 * UP), ("output", 5, 9 * UP), ("output", 6, 5 * UP), ("output", 7, 4 * UP), ("output", 8, 6 * UP),
    ]
    again, _ = _mixed_batch(InputRecordingEngine, [None] * 4)
    assert again == calls


def test_batching_service_groups_raw_recordings_by_rate_and_encoding():
    s16 = {"sample_rate": 16000, "encoding": "s16"}
    calls, _ = _mixed_batch(InputRecordingEngine, [s16, {"sample_rate": 48000}, s16, None])
    assert calls[3:7] == [
        ("configure_input", 16000), ("input_batch", 16000, ref.S16, [93, 40]),           # one call per distinct pair
        ("configure_input", 48000), ("input_batch", 48000, ref.F32, [50]),
    ]
    assert calls[7] == ("convert_latent", [186, 100, 80, 60], [5, 6, 7, 8], [21, 22, 24, 25], 1.0)    # then the ONE call


class LiveInputEngine(live_host.FakeEngine):
    """``FakeEngine`` of the live-conversion host tests with an input stage: 22050 Hz doubles (L, M, H) = (2, 1, 64), the
    model's rate passes through; raw sample k must hold k, output sample m is m -- so the session's buffer is the ramp the
    stand-in's conversion checks -- and every row must hold the raw samples its outputs need."""
    device = "cpu"
    plans = {22050: (2, 1, 64), MODEL: (1, 1, 0)}

    def __init__(self):
        super().__init__()
        self.input_rates, self.input_calls = (22050, MODEL), []

    def input_plan(self, rate):
        return self.plans[rate]

    def input_rows(self, rows, rate, enc):
        L, M, H = self.plans[rate]
        self.input_calls.append((rate, enc, len(rows)))
        out = []
        for raw, first, n_total, m0, m1 in rows:
            assert raw.dtype == torch.int16
            assert torch.equal(raw, torch.arange(first, first + len(raw), dtype=torch.int16))
            end = first + len(raw)
            assert m1 <= output_stage.complete_outputs(end, L, M, H, ended=n_total >= 0) and (n_total < 0 or end == n_total)
            assert m0 == m1 or first <= output_stage.history_start(m0, L, M, H)
            out.append(torch.arange(m0, m1, dtype=torch.float32))
        return out


def _live(fmts, n_model, sizes):
    from vispeech_amd.service import StreamingBatchService
    net = live_host.FakeNet()
    net._engine = eng = LiveInputEngine()
    svc = StreamingBatchService(net, collate=lambda rows: None, autostart=False, chunk_frames=4)
    sessions = [svc.open_conversion(1, 2, 9, **fmt) for fmt in fmts]
    feeds = []
    for fmt in fmts:
        rate = fmt.get("sample_rate", MODEL)
        n = n_model * rate // MODEL
        feeds.append(np.arange(n, dtype=np.float32 if not fmt else np.int16))
    at, k = 0, 0
    while at < n_model:
        size = sizes[k % len(sizes)]
        for s, f in zip(sessions, feeds):
            lo, hi = at * len(f) // n_model, min(at + size, n_model) * len(f) // n_model
            s.feed(f[lo:hi] if f.dtype == np.float32 else f[lo:hi].tobytes())
        at, k = at + size, k + 1
        while svc.step():
            pass
    for s in sessions:
        s.end()
    while svc.step():
        pass
    return eng, [b"".join(s) for s in sessions]


def test_live_sessions_resample_per_tick_and_deliver_the_same_bytes():
    n = 30 * HOP + 100
    assert frames_of(n) == 30
    plain, a = _live([{}], n, [1, 255, 4097])
    assert plain.input_calls == []                                          # no keyword: no input call, the calls it always made
    fmts = [{"sample_rate": 22050, "encoding": "s16"}, {}, {"encoding": "s16"}, {"sample_rate": 22050, "encoding": "s16"}]
    eng, b = _live(fmts, n, [1, 255, 4097])
    assert b[0] == b[1] == b[2] == b[3] == a[0] == live_host.expect(0, 30)
    # one call per distinct (rate, encoding) and tick: the two 22050 Hz sessions share theirs
    assert {c[:2] for c in eng.input_calls} == {(22050, ref.S16), (MODEL, ref.S16)}
    assert max(c[2] for c in eng.input_calls if c[0] == 22050) == 2 and all(c[2] == 1 for c in eng.input_calls if c[0] == MODEL)


class _Fake:
    pass


def test_convert_audio_without_the_keywords_calls_convert_alone():
    from vispeech_amd.models import SynthesizerTrn
    calls = []

    class Eng:
        ready = has_voice_conversion = True
        input_rates = ()

        def convert(self, audio, n, src, tgt, noise=None, noise_seed=None, noise_scale=1.0):
            calls.append(("convert", audio, tuple(n)))
            return {k: torch.zeros(1) for k in ("o_hat", "z", "z_p", "z_hat")} | {"y_mask": torch.ones(1)}

        def configure_input(self, rate):
            calls.append(("configure_input", rate))
            self.input_rates += (rate,)

        def input_batch(self, raw, n, rate, enc):
            calls.append(("input_batch", raw, tuple(n), rate, enc))
            return "resampled", [2 * x for x in n]

    net = _Fake()
    net._engine, net.n_speakers, net.dims = Eng(), 4, _Fake()
    net.dims.sampling_rate = MODEL
    SynthesizerTrn.convert_audio(net, "audio", [5, 7], [0, 1], [2, 3], noise_seed=[1, 2])
    assert calls == [("convert", "audio", (5, 7))]
    del calls[:]
    SynthesizerTrn.convert_audio(net, "raw", [5, 7], [0, 1], [2, 3], noise_seed=[1, 2], sample_rate=16000, encoding="s16")
    SynthesizerTrn.convert_audio(net, "raw", [5], [0], [2], noise_seed=[1], encoding="ulaw")
    assert calls == [("configure_input", 16000), ("input_batch", "raw", (5, 7), 16000, "s16"), ("convert", "resampled", (10, 14)),
                     ("configure_input", MODEL), ("input_batch", "raw", (5,), MODEL, "ulaw"), ("convert", "resampled", (10,))]
