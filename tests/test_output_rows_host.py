"""Output rows, host side (no GPU): the new symbols, the G.711 compressor against its two formulas restated in numpy, the
plan of ``vsp_output_rows_plan`` against a brute-force enumeration, what ``vsp_output_rows`` refuses before it needs a
device, and the host logic of the services over an engine whose output stage is the fp64 sum over the library's own taps
-- which calls a request with its own output format adds, and that a group without one makes the calls it always made.
(The refusals that need a configured rate -- and so a device -- are in ``test_output_rows_gpu.py``.)"""
import ctypes as C

import numpy as np
import pytest
import torch

import output_stage_ref as ref
import test_abi
import test_service_paths_host as paths_host
from vispeech_amd import _lib, input_stage, output_stage

MODEL = 44100
F32, S16, ULAW, ALAW = 0, 1, 2, 3


# ---------------------------------------------------------------------------------------------- the two formulas, in numpy
def ulaw_ref(s):
    s = np.asarray(s).astype(np.int64)
    neg = s < 0
    mag = np.minimum(np.abs(s), 32635) + 0x84
    e = np.floor(np.log2(mag)).astype(np.int64) - 7
    q = (mag >> (e + 3)) & 15
    return (~(np.where(neg, 0x80, 0) | (e << 4) | q) & 0xFF).astype(np.uint8)


def alaw_ref(s):
    s = np.asarray(s).astype(np.int64)
    neg = s < 0
    mag = np.where(neg, ~s, s) >> 3
    e = np.where(mag > 0, np.maximum(np.floor(np.log2(np.maximum(mag, 1))).astype(np.int64) - 4, 0), 0)
    q = np.where(e == 0, (mag >> 1) & 15, (mag >> e) & 15)
    return ((np.where(neg, 0, 0x80) | (e << 4) | q) ^ 0x55).astype(np.uint8)


LAW_REF = {ULAW: ulaw_ref, ALAW: alaw_ref}


def encode_ref(y32, enc):
    """A float32 row in encoding ``enc``, by the published rules."""
    if enc == F32:
        return np.asarray(y32, np.float32)
    s = ref.pcm16(y32)
    return s if enc == S16 else LAW_REF[enc](s)


# ---------------------------------------------------------------------------------------------- symbols and ABI
def test_symbols_abi_and_struct_size():
    lib = _lib.lib()
    for name in ("vsp_output_encode", "vsp_output_rate_configure", "vsp_output_rows_plan", "vsp_output_rows"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.vsp_abi_version() == 7
    assert sorted(_lib.SIGNATURES) == test_abi.header_symbols()
    # x, x_first, n | ended, out_rate, enc, (pad) | hist_in, hist_out, out, out_fill
    assert C.sizeof(_lib.VspOutputRow) == 72 and _lib.VspOutputRow.hist_in.offset == 40 and _lib.VspOutputRow.out_fill.offset == 64
    assert (_lib.OUT_F32, _lib.OUT_S16, _lib.OUT_ULAW, _lib.OUT_ALAW) == (_lib.IN_F32, _lib.IN_S16, _lib.IN_ULAW, _lib.IN_ALAW)
    assert _lib.OUTPUT_RATES_MAX == output_stage.RATES_MAX == 8
    assert [output_stage.encoding(e) for e in ("f32", "s16", "ulaw", "alaw", 0, 3, None)] == [0, 1, 2, 3, 0, 3, 1]
    with pytest.raises(ValueError):
        output_stage.encoding("opus")
    with pytest.raises(ValueError):
        output_stage.encoding(4)


# ---------------------------------------------------------------------------------------------- compressor
@pytest.mark.parametrize("enc", [ULAW, ALAW])
def test_compressor_is_the_formula_for_every_value(enc):
    s = np.arange(-32768, 32768).astype(np.int16)
    c = output_stage.encode(s, enc)
    assert c.dtype == np.uint8 and c.shape == s.shape
    np.testing.assert_array_equal(c, LAW_REF[enc](s))
    table = input_stage.decode_table(enc)
    # every code's own value encodes back to the code (mu-law's negative zero comes back as the positive one)
    own = np.round(table.astype(np.float64) * 32768.0).astype(np.int16)
    want = np.arange(256, dtype=np.uint8)
    if enc == ULAW:
        want[0x7F] = 0xFF
    np.testing.assert_array_equal(output_stage.encode(own, enc), want)
    assert np.all(np.diff(table[c]) >= 0)                            # decode(encode(s)) is monotone in s
    assert output_stage.silence(enc) == output_stage.encode(np.zeros(1, np.int16), enc)[0] == (0xFF if enc == ULAW else 0xD5)


def test_compressor_edges_and_refusals():
    lib = _lib.lib()
    assert output_stage.silence("f32") == 0.0 and output_stage.silence("s16") == 0
    np.testing.assert_array_equal(output_stage.encode(np.int16([3, -4]), "s16"), [3, -4])
    assert output_stage.encode(np.zeros(0, np.int16), "ulaw").shape == (0,)
    with pytest.raises(ValueError):
        output_stage.encode(np.zeros(3, np.float32), "ulaw")
    s, c = np.zeros(4, np.int16), np.zeros(4, np.uint8)
    ps, pc = s.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p)
    for enc in (F32, S16, 4, -1):
        assert lib.vsp_output_encode(enc, ps, 4, pc) == -1
    assert lib.vsp_output_encode(ULAW, None, 4, pc) == -1 and lib.vsp_output_encode(ULAW, ps, 4, None) == -1
    assert lib.vsp_output_encode(ULAW, ps, -1, pc) == -1 and lib.vsp_output_encode(ALAW, None, 0, None) == 0


# ---------------------------------------------------------------------------------------------- plan
def _brute(L, M, H, x_first, n, ended):
    """(m0, m1, k0, k1) by enumeration: output m is complete once every tap of it lies below the samples seen."""
    def complete(s, end):
        total = -(-s * L // M)
        if end:
            return total
        m = 0
        while m < total and m * M + H < L * s:
            m += 1
        return m

    def start(m):
        k = 0
        while k * L < m * M - H:
            k += 1
        return k
    m0, m1 = complete(x_first, False), complete(x_first + n, ended)
    return m0, m1, min(x_first, start(m0)), min(x_first + n, start(m1))


SPLITS = [(1,), (7,), (159, 160, 161), (1, 2, 159, 160, 161, 1024, 3), (4000,), (93, 1, 1, 3000)]


@pytest.mark.parametrize("rate", sorted(ref.TABLE) + [MODEL])
def test_plan_is_the_enumeration_and_calls_tile_the_output(rate):
    L, M, H = output_stage.plan(MODEL, rate)
    K = _lib.lib().vsp_output_history_samples(L, M, H)
    assert K == output_stage.history_samples(L, M, H)
    rng = np.random.default_rng(rate)
    for total in (1, 93, 1601):
        for sizes in SPLITS + [tuple(int(v) for v in rng.integers(1, 400, 9))]:
            for flush in (False, True):                              # the end comes with the last piece, or as n = 0 behind it
                at, k, m_next, k_prev = 0, 0, 0, 0
                while True:
                    n = min(sizes[k % len(sizes)], total - at)
                    ended = (at + n == total and not flush) or n == 0
                    got = output_stage.rows_plan(L, M, H, at, n, ended)
                    if total <= 93 or k < 3:
                        assert got == _brute(L, M, H, at, n, ended), (at, n, ended)
                    m0, m1, k0, k1 = got
                    assert m0 == m_next and m1 >= m0 and k0 == k_prev          # the calls tile the outputs; k0 is the last k1
                    assert 0 <= at - k0 <= K and 0 <= at + n - k1 <= K
                    m_next, k_prev, at, k = m1, k1, at + n, k + 1
                    if ended:
                        break
                assert m_next == -(-total * L // M)
    lib = _lib.lib()
    for bad in ((0, M, H, 0, 1, 0), (L, 0, H, 0, 1, 0), (L, M, -1, 0, 1, 0), (L, M, H, -1, 1, 0), (L, M, H, 0, -1, 1)):
        assert lib.vsp_output_rows_plan(*bad, None, None, None, None) == -1, bad
    assert lib.vsp_output_rows_plan(L, M, H, 0, 5, 1, None, None, None, None) == 0


def test_plan_equals_the_stream_rows_plan_for_frame_aligned_input():
    lib = _lib.lib()
    up = 512
    for rate in (22050, 8000, 48000):
        L, M, H = output_stage.plan(MODEL, rate)
        frames = 23
        rows = (_lib.VspStreamRow * 1)()
        for f0, f1 in ((0, 1), (1, 9), (9, 22), (22, 23)):
            rows[0].L, rows[0].f0, rows[0].f1 = frames, f0, f1
            res = [(C.c_int64 * 1)() for _ in range(4)]
            assert lib.vsp_stream_rows_output_plan(L, M, H, up, 1, rows, *res) == 0
            assert tuple(r[0] for r in res) == output_stage.rows_plan(L, M, H, f0 * up, (f1 - f0) * up, f1 == frames)


# ---------------------------------------------------------------------------------------------- refusals without a device
def test_rows_are_refused_before_a_device_is_needed():
    from vispeech_amd.schema import ModelDims
    lib = _lib.lib()
    cfg = _lib.make_config(ModelDims())
    h = C.c_void_p()
    assert lib.vsp_create(C.byref(cfg), 0, C.byref(h)) == 0
    row = (_lib.VspOutputRow * 1)()
    r = row[0]
    r.x, r.n, r.ended, r.out_rate, r.enc, r.out, r.out_fill = 16, 8, 1, 8000, ULAW, 16, 8
    assert lib.vsp_output_rows(None, None, 1, row) == -1
    assert lib.vsp_output_rows(h, None, 1, row) == -2 and b"not configured" in lib.vsp_last_error(h)
    for B in (0, 65, -1):
        assert lib.vsp_output_rows(h, None, B, row) == -1 and b"rows" in lib.vsp_last_error(h)
    assert lib.vsp_output_rows(h, None, 1, None) == -1
    for enc in (4, -1):
        r.enc = enc
        assert lib.vsp_output_rows(h, None, 1, row) == -1 and b"VSP_OUT_" in lib.vsp_last_error(h)
    r.enc, r.n = ULAW, -1
    assert lib.vsp_output_rows(h, None, 1, row) == -1 and b"negative" in lib.vsp_last_error(h)
    r.n, r.ended = 0, 0
    assert lib.vsp_output_rows(h, None, 1, row) == -1 and b"n == 0" in lib.vsp_last_error(h)
    r.ended = 1
    assert lib.vsp_output_rows(h, None, 1, row) == -2                          # n == 0 with ended gets as far as the rate
    # the set of rates and the single stage do not see each other: neither is configured by refusing the other
    assert lib.vsp_output_rate_configure(h, MODEL, 44000, 32, 9.62, 0.0) == -7     # L = 440: refused before any device call
    assert lib.vsp_output_rate_configure(h, MODEL, 16000, 65, 9.62, 0.0) == -7
    assert lib.vsp_output_rate_configure(h, MODEL, 0, 32, 9.62, 0.0) == -1
    assert lib.vsp_output_rate_configure(h, MODEL, -8000, 32, 9.62, 0.0) == -1
    assert lib.vsp_output_rate_configure(h, MODEL, 16000, 32, -1.0, 0.0) == -1
    assert lib.vsp_output_rate_configure(h, MODEL, 16000, 32, 9.62, 1.5) == -1
    assert lib.vsp_output_rate_configure(h, 0, 16000, 32, 9.62, 0.0) == 0         # dropping a rate that is not there
    assert lib.vsp_output_rate_configure(None, MODEL, 16000, 32, 9.62, 0.0) == -1
    assert lib.vsp_output_configure(h, MODEL, 0, 32, 9.62, 0.0) == 0              # the single stage: off, as it was
    lib.vsp_destroy(h)


# ---------------------------------------------------------------------------------------------- the services
class RowsEngine:
    """The output-rows half of an engine in double precision: a row's float value is the fp64 sum over the library's own
    taps, rounded to float32 once; PCM16 and G.711 follow by the published rules.  What lies outside a row's two segments
    is NaN to it, so a history that lacks a needed sample shows.  Records its calls in ``calls``."""

    def __init__(self):
        self.output_rates, self._taps = (), {}
        if not hasattr(self, "calls"):
            self.calls = []

    def configure_output_rate(self, rate, in_rate=None):
        assert in_rate == MODEL and rate not in self.output_rates
        self.calls.append(("configure_output_rate", rate))
        self.output_rates += (rate,)
        self._taps[rate] = output_stage.taps(MODEL, rate).astype(np.float64)

    def output_rate_plan(self, rate):
        assert rate in self.output_rates
        return output_stage.plan(MODEL, rate)

    def output_row_buffers(self, K):
        return np.full((2, K), np.nan, np.float32)

    def output_rows(self, rows):
        self.calls.append(("output_rows", [(int(0 if x is None else len(x)), bool(ended), rate, enc) for x, ended, rate, enc, _ in rows]))
        parts, spans, at = [], [], 0
        for x, ended, rate, enc, state in rows:
            L, M, H = self.output_rate_plan(rate)
            x = np.zeros(0, np.float32) if x is None else np.asarray(x, np.float32)
            first = 0 if state is None else state.x_first
            m0, m1, k0, k1 = output_stage.rows_plan(L, M, H, first, len(x), ended)
            full = np.full(first + len(x), np.nan)
            if first > k0:
                full[k0:first] = state.buf[state.side][: first - k0]
            full[first:] = x
            y = ref.resample_fp64(full, self._taps[rate], L, M, m0, m1)
            assert np.isfinite(y).all() and (ended or m1 == output_stage.complete_outputs(len(full), L, M, H))
            if state is not None:
                state.buf[1 - state.side][:] = np.nan
                state.buf[1 - state.side][: len(full) - k1] = full[k1:]
                state.advance(len(x))
            raw = encode_ref(y.astype(np.float32), enc).tobytes()
            spans.append((at, m1 - m0))
            raw += b"\xee" * (-len(raw) % 16)
            parts.append(raw)
            at += len(raw)
        return np.frombuffer(b"".join(parts), np.uint8), spans


class BatchEngine(paths_host.RecordingEngine, RowsEngine):
    def __init__(self):
        paths_host.RecordingEngine.__init__(self)
        RowsEngine.__init__(self)


FORMATS = [(8000, "ulaw"), (8000, "alaw"), (48000, "s16"), None, (22050, "f32")]


def _kw(fmt):
    return {} if fmt is None else {"output_rate": fmt[0], "output_encoding": fmt[1]}


def _batch(formats, eng_cls=BatchEngine):
    from vispeech_amd.service import BatchingSynthesisService
    net = paths_host.RecordingNet()
    net._engine = eng = eng_cls()
    svc = BatchingSynthesisService(net, max_batch=5, max_wait_s=30.0, collate=paths_host._collate, output_rate=22050)
    try:
        futs = [svc.submit({"id": 1, "frames": 6}, 7, **_kw(formats[0]))]
        for (n, src, tgt, seed), fmt in zip(((93, 3, 5, 21), (50, 4, 6, 22), (40, 4, 7, 24), (60, 4, 8, 25)), formats[1:]):
            futs.append(svc.submit_conversion(paths_host._audio(n), src, tgt, seed, **_kw(fmt)))
        got = [f.result(60) for f in futs]
    finally:
        svc.close()
    return eng, got


HEAD = [("configure_output", 22050, 44100), ("encode", [1]), ("decode", 0, [7]),
        ("convert_latent", [93, 50, 40, 60], [5, 6, 7, 8], [21, 22, 24, 25], 1.0),
        ("generator_ragged", [1, 5, 6, 7, 8], [6, 9, 5, 4, 6], (5, 1, 9))]


def test_batching_group_with_formats_makes_one_output_rows_call():
    UP = paths_host.UP
    eng, got = _batch(FORMATS)
    assert eng.calls[:5] == HEAD
    assert sorted(eng.calls[5:-1]) == [("configure_output_rate", r) for r in (8000, 22050, 48000)]
    assert eng.calls[-1] == ("output_rows", [(6 * UP, True, 8000, ULAW), (9 * UP, True, 8000, ALAW), (5 * UP, True, 48000, S16),
                                             (4 * UP, True, 22050, S16), (6 * UP, True, 22050, F32)])
    assert [g.dtype for g in got] == [np.uint8, np.uint8, np.dtype("<i2"), np.dtype("<i2"), np.float32]
    for g, (rid, frames), fmt in zip(got, ((1, 6), (5, 9), (6, 5), (7, 4), (8, 6)), FORMATS):
        rate, enc = (22050, "s16") if fmt is None else fmt
        x = (np.repeat(100 * rid + np.arange(frames), UP) / 32767.0).astype(np.float32)
        L, M, _ = output_stage.plan(MODEL, rate)
        y = ref.resample_fp64(x, output_stage.taps(MODEL, rate), L, M).astype(np.float32)
        np.testing.assert_array_equal(g, encode_ref(y, output_stage.encoding(enc)))


def test_batching_group_without_formats_makes_the_calls_it_always_made():
    UP = paths_host.UP
    want = HEAD + [("output", 1, 6 * UP), ("output", 5, 9 * UP), ("output", 6, 5 * UP), ("output", 7, 4 * UP), ("output", 8, 6 * UP)]
    eng, got = _batch([None] * 5)
    assert eng.calls == want
    plain, again = _batch([None] * 5, paths_host.RecordingEngine)             # (an engine without output rows at all)
    assert plain.calls == want and all(np.array_equal(a, b) for a, b in zip(got, again))


class StreamRowsEngine(paths_host.StreamEngine, RowsEngine):
    """``StreamEngine`` (integer frames, its own integer single stage at 22050 Hz) with output rows in double precision."""

    def __init__(self):
        paths_host.StreamEngine.__init__(self)
        self.calls = []
        RowsEngine.__init__(self)


REQUESTS = [(1, 18, (8000, "ulaw")), (2, 5, (48000, "s16")), (3, 1, None), (4, 9, (22050, "f32")), (5, 7, (8000, "alaw"))]


def _one_shot_bytes(rid, frames, fmt, base):
    rate, enc = base if fmt is None else fmt
    x = np.repeat(10 * rid + np.arange(frames), paths_host.UP).astype(np.float32)
    L, M, _ = output_stage.plan(MODEL, rate)
    y = ref.resample_fp64(x, output_stage.taps(MODEL, rate), L, M).astype(np.float32)
    return encode_ref(y, output_stage.encoding(enc)).tobytes()


@pytest.mark.parametrize("chunk", [4, 3])
def test_streaming_requests_join_and_leave_and_get_their_one_shot_bytes(chunk):
    from vispeech_amd.service import StreamingBatchService
    net = paths_host.StreamNet()
    net._engine = eng = StreamRowsEngine()
    svc = StreamingBatchService(net, collate=paths_host._collate, autostart=False, chunk_frames=chunk)
    sub = lambda rid, frames, fmt: svc.submit({"id": rid, "frames": frames}, rid, **_kw(fmt))
    streams = [sub(*REQUESTS[0])]
    svc.step(); svc.step()
    streams += [sub(*REQUESTS[1]), sub(*REQUESTS[2])]                          # the third names nothing and ends in one tick
    svc.step()
    streams += [sub(*REQUESTS[3]), sub(*REQUESTS[4])]
    svc.close()
    for s, (rid, frames, fmt) in zip(streams, REQUESTS):
        assert b"".join(paths_host._pieces(s)) == _one_shot_bytes(rid, frames, fmt, (MODEL, "s16")), rid
    calls = [c for c in eng.calls if c[0] == "output_rows"]
    assert len(calls) == svc.stats["ticks"] == len(eng.ticks)                 # ONE call per tick, over all its rows
    assert [len(c[1]) for c in calls] == svc.stats["rows_per_tick"]
    assert max(svc.stats["rows_per_tick"]) >= 3
    assert all(row[1] == (t[3] == t[1]) for c, tick in zip(calls, eng.ticks) for row, t in zip(c[1], tick))   # ended with the last frame


class OneStageEngine(StreamRowsEngine):
    """``StreamRowsEngine`` whose single stage and whose 22050 Hz rows are ONE filter -- the eleven taps of
    ``test_service_paths_host`` scaled by 2^-15, summed in double precision -- so that a request may change between the two
    paths; a window or a history that lacks a needed sample is NaN to both."""
    H22 = paths_host.TAPS.astype(np.float64) / 2.0 ** 15

    def output_rate_plan(self, rate):
        return paths_host.LMH if rate == 22050 else super().output_rate_plan(rate)

    def configure_output_rate(self, rate, in_rate=None):
        super().configure_output_rate(rate, in_rate)
        if rate == 22050:
            self._taps[rate] = self.H22

    def output_chunk(self, x, x_first, n_max, m0, m1, n_valid=None, pcm=True):
        assert pcm and n_valid is None and x.shape[0] == 1 and x_first + x.shape[1] == n_max and m1 > m0
        self.chunks.append((x_first, int(x.shape[1]), m0, m1))
        full = np.full(n_max, np.nan)
        full[x_first:] = np.asarray(x[0])
        y = ref.resample_fp64(full, self.H22, *paths_host.LMH[:2], m0, m1)
        assert np.isfinite(y).all()
        return torch.from_numpy(ref.pcm16(y.astype(np.float32)).astype(np.int16))[None, :]


def test_streaming_unformatted_request_changes_path_and_keeps_its_bytes():
    """A service with an output rate: a request that names nothing runs alone on the service's own per-request stage, shares
    two ticks with a request that names a format -- as a row of ``output_rows`` -- and finishes alone again; the samples
    its filter still needs change hands both times."""
    from vispeech_amd.service import StreamingBatchService
    UP = paths_host.UP
    net = paths_host.StreamNet()
    net._engine = eng = OneStageEngine()
    svc = StreamingBatchService(net, collate=paths_host._collate, autostart=False, chunk_frames=4, output_rate=22050)
    a = svc.submit({"id": 1, "frames": 40}, 7)
    svc.step(); svc.step()
    b = svc.submit({"id": 2, "frames": 8}, 8, output_rate=8000, output_encoding="ulaw")
    svc.close()
    assert b"".join(paths_host._pieces(b)) == _one_shot_bytes(2, 8, (8000, "ulaw"), None)
    calls = [c for c in eng.calls if c[0] == "output_rows"]
    assert [[row[2:] for row in c[1]] for c in calls] == [[(22050, S16), (8000, ULAW)]] * 2
    x = np.repeat(10 * 1 + np.arange(40), UP).astype(np.float32)
    whole = ref.pcm16(ref.resample_fp64(x, eng.H22, *paths_host.LMH[:2]).astype(np.float32))
    assert b"".join(paths_host._pieces(a)) == whole.tobytes()
    ends = [c[0] + c[1] for c in eng.chunks]                                  # its own stage ran before and behind the shared ticks
    assert min(ends) <= 2 * 4 * UP and max(ends) == 40 * UP and not any(2 * 4 * UP < e <= 4 * 4 * UP for e in ends)


def test_fused_output_refuses_a_request_format():
    from vispeech_amd.service import StreamingBatchService
    net = paths_host.StreamNet()
    svc = StreamingBatchService(net, collate=paths_host._collate, autostart=False, output_rate=22050, fused_output=True)
    with pytest.raises(ValueError, match="fused_output"):
        svc.submit({"id": 1, "frames": 3}, 1, output_rate=8000)
    with pytest.raises(ValueError, match="fused_output"):
        svc.submit_conversion(paths_host._audio(50), 1, 2, 3, output_encoding="ulaw")
    with pytest.raises(ValueError, match="fused_output"):
        svc.open_conversion(1, 2, 3, output_encoding="alaw")
    svc.submit({"id": 1, "frames": 3}, 1).close()                             # without a format it is accepted as before
