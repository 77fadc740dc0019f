"""The denoiser for streams without a GPU: the symbols, ``vsp_denoise_complete`` against a brute-force
count over frames, every refusal of ``vsp_denoise_rows`` (decided on the host before a device is touched),
``denoiser.Stream``'s bookkeeping on a numpy stand-in engine built on the restatement of one call
(tests/denoiser_stream_ref.py) -- every row of the fixture, cut four ways, gives the whole row's result bit for bit --, the
refusals of the host layer, and ``StreamingBatchService`` with stand-ins: the order denoiser, limiter, output rows, the
positions handed on, and that a request naming no denoiser gets the bytes it always got."""
import ctypes as C

import numpy as np
import pytest

import denoiser_ref as dr
import denoiser_stream_ref as sr
import test_abi
from vispeech_amd import _lib, denoiser
from vispeech_amd.schema import ModelDims

NEW = ("vsp_denoise_history", "vsp_denoise_complete", "vsp_denoise_rows_workspace_bytes", "vsp_denoise_rows")
N, HOP, PAD = dr.N_FFT, dr.HOP, dr.pad_of()
NAN = float("nan")
BAD = 8                                 # a pointer no kernel may ever see: every refusal is decided before a device is needed
BIG = 1 << 40
CUTS = {
    "one": lambda n: [n],
    "hop": lambda n: [HOP] * (n // HOP + 1),
    "odd": lambda n: [1279, 1, 512, 511, 513] + [997] * (n // 997 + 1),
    "100": lambda n: [100] * (n // 100 + 1),
}


def test_symbols_and_abi():
    lib = _lib.lib()
    for s in NEW:
        assert hasattr(lib, s) and s in _lib.SIGNATURES, s
    assert lib.vsp_abi_version() == 7
    assert sorted(_lib.SIGNATURES) == test_abi.header_symbols()
    assert C.sizeof(_lib.VspDenoiseRow) == 64


@pytest.fixture()
def ctx():
    lib = _lib.lib()
    cfg = _lib.make_config(ModelDims())
    h = C.c_void_p()
    assert lib.vsp_create(C.byref(cfg), 0, C.byref(h)) == 0
    yield lib, h
    lib.vsp_destroy(h)


# ---------------------------------------------------------------------------------------------- the one rule
def _brute_complete(n):
    """Frames that read no sample at or behind n, counted one by one; the outputs all of whose frames are among them."""
    Tc = 0
    while Tc * HOP - PAD + N <= n:
        Tc += 1
    j = 0
    while (j + PAD) // HOP <= Tc - 1:        # output j's last frame is floor((j + pad) / hop)
        j += 1
    return j


def test_complete_is_the_brute_force_count(ctx):
    lib, h = ctx
    behind, ahead = C.c_int64(), C.c_int64()
    assert lib.vsp_denoise_history(h, C.byref(behind), C.byref(ahead)) == 0 and (behind.value, ahead.value) == (N - HOP, N - 1)
    for n in range(0, 3 * N + 1):
        e = _brute_complete(n)
        assert lib.vsp_denoise_complete(h, n, 0) == e == sr.complete(n), n
        assert lib.vsp_denoise_complete(h, n, 1) == n
        assert e == 0 or N - HOP <= n - e <= N - 1, n                    # the delay
    assert lib.vsp_denoise_complete(h, -1, 0) == -1 and lib.vsp_denoise_complete(None, 5, 0) == -1
    assert lib.vsp_denoise_history(h, None, C.byref(ahead)) == -1


def test_a_context_without_the_geometry_has_no_stream_calls():
    lib = _lib.lib()
    cfg = _lib.make_config(ModelDims(spec_channels=1001))
    h = C.c_void_p()
    assert lib.vsp_create(C.byref(cfg), 0, C.byref(h)) == 0
    try:
        a = C.c_int64()
        assert lib.vsp_denoise_history(h, C.byref(a), C.byref(a)) == -1 and lib.vsp_denoise_complete(h, 5000, 0) == -1
        assert lib.vsp_denoise_rows_workspace_bytes(h, 1, 5000) == -1
        row = (_lib.VspDenoiseRow * 1)(_lib.VspDenoiseRow(BAD, 0, 5000, BAD, 0, 5000, 5000, 1.0))
        assert lib.vsp_denoise_rows(h, None, 1, row, BAD, BAD, BIG) == -1 and b"does not divide" in lib.vsp_last_error(h)
    finally:
        lib.vsp_destroy(h)


# ---------------------------------------------------------------------------------------------- refusals of the C call
def _rows(lib, h, rows, bias=BAD, ws=BIG, wsp=BAD, B=None):
    desc = (_lib.VspDenoiseRow * max(len(rows), B or 1))(*[_lib.VspDenoiseRow(*r) for r in rows])
    return lib.vsp_denoise_rows(h, None, len(rows) if B is None else B, desc, bias, wsp, ws)


def test_rows_are_refused_before_a_device_is_needed(ctx):
    lib, h = ctx
    err = lambda: lib.vsp_last_error(h)
    whole = (BAD, 0, 5000, BAD, 0, 5000, 5000, 1.0)
    # E(4000) = 2304 and E(6000) = 4352: the frames 3 .. 9, which read the samples [768, 5888)
    mid = (BAD, 768, 6000 - 768, BAD, 2304, 4352 - 2304, -1, 0.5)
    # rows that pass every check: the next thing refused is the workspace, then the missing weights
    need = lib.vsp_denoise_rows_workspace_bytes(h, 2, 5000)
    assert need >= 2 * (2048 + 2050 + 2048) * (10 + 4) * 4
    assert _rows(lib, h, [whole, mid], ws=need - 1) == -6 and _rows(lib, h, [whole, mid], wsp=None) == -6
    assert _rows(lib, h, [whole, mid], ws=need) == -2 and _rows(lib, h, [whole, mid]) == -2
    assert _rows(lib, h, [whole, (BAD, 768, 5888 - 768, BAD, 2304, 4352 - 2304, -1, 0.5)]) == -2      # exactly what the frames read
    # history, look-ahead
    assert _rows(lib, h, [whole, (BAD, 769, 6000 - 769, BAD, 2304, 2048, -1, 0.5)]) == -1 and b"row 1" in err() and b"history" in err()
    assert _rows(lib, h, [whole, (BAD, 768, 5887 - 768, BAD, 2304, 2048, -1, 0.5)]) == -1 and b"row 1" in err() and b"look-ahead" in err()
    # ... also where the end is known and not reached; reached, the frames reflect there and nothing is missing
    assert _rows(lib, h, [(BAD, 768, 5887 - 768, BAD, 2304, 2048, 7000, 0.5)]) == -1 and b"row 0" in err() and b"look-ahead" in err()
    assert _rows(lib, h, [(BAD, 768, 5887 - 768, BAD, 2304, 5887 - 2304, 5887, 0.5)]) == -2
    # the end reflection reads back to total - 1 - pad at most: a closing row may start there when it puts out the tail only
    assert _rows(lib, h, [(BAD, 3000, 2000, BAD, 4990, 10, 5000, 0.5)]) == -2
    assert _rows(lib, h, [(BAD, 3700, 1300, BAD, 4990, 10, 5000, 0.5)]) == -1 and b"history" in err()
    # total <= pad; outputs or samples behind the end; outputs the samples do not hold
    for total in (PAD, 1, 0):
        assert _rows(lib, h, [whole, (BAD, 0, total, BAD, 0, total, total, 1.0)]) == -1 and b"row 1" in err(), total
    assert _rows(lib, h, [(BAD, 0, 5000, BAD, 0, 5001, 5000, 1.0)]) == -1 and b"row 0" in err()
    assert _rows(lib, h, [(BAD, 0, 5001, BAD, 0, 5000, 5000, 1.0)]) == -1 and b"row 0" in err()
    # negative or too large positions and counts
    for bad in ((BAD, -1, 5000, BAD, 0, 100, -1, 1.0), (BAD, 0, -5, BAD, 0, 100, -1, 1.0), (BAD, 0, 5000, BAD, -1, 100, -1, 1.0),
                (BAD, 0, 5000, BAD, 0, -1, -1, 1.0), (BAD, 0, 5000, BAD, 0, 100, -2, 1.0), (BAD, 0, (1 << 30) + 1, BAD, 0, 100, -1, 1.0),
                (BAD, (1 << 30) + 1, 5000, BAD, (1 << 30) + 1, 100, -1, 1.0)):
        assert _rows(lib, h, [whole, whole, bad]) == -1 and b"row 2" in err(), bad
    # null pointers on a live row; a strength; the bias
    assert _rows(lib, h, [(None, 0, 5000, BAD, 0, 5000, 5000, 1.0)]) == -1 and b"row 0" in err() and b"null" in err()
    assert _rows(lib, h, [(BAD, 0, 5000, None, 0, 5000, 5000, 1.0)]) == -1 and b"row 0" in err()
    for s in (-0.5, float("inf"), -float("inf")):
        assert _rows(lib, h, [whole, (BAD, 0, 5000, BAD, 0, 5000, 5000, s)]) == -1 and b"row 1" in err() and b"strength" in err(), s
    assert _rows(lib, h, [(BAD, 0, 5000, BAD, 0, 5000, 5000, NAN), whole], bias=None) == -1 and b"row 1" in err() and b"bias" in err()
    # a NaN row is left alone whatever it holds, and a row without outputs is not read: no refusal of theirs
    assert _rows(lib, h, [(None, -7, 1 << 40, None, -1, -1, -9, NAN), (None, 0, 0, None, 0, 0, -1, 1.0)], ws=16) == -6
    assert _rows(lib, h, [(None, -7, 1 << 40, None, -1, -1, -9, NAN)], bias=None) == -2
    # B
    assert _rows(lib, h, [whole], B=65) == -1 and b"64" in err() and _rows(lib, h, [whole], B=0) == -1
    assert lib.vsp_denoise_rows(h, None, 1, None, BAD, BAD, BIG) == -1 and lib.vsp_denoise_rows(None, None, 1, None, BAD, BAD, BIG) == -1
    # the workspace: monotone in both arguments, refused outside them
    size = lambda B, L: lib.vsp_denoise_rows_workspace_bytes(h, B, L)
    assert size(1, 1) <= size(1, 2) <= size(1, HOP + 2) <= size(2, HOP + 2) <= size(2, 40 * HOP) <= size(64, 40 * HOP)
    assert size(1, 5000) < size(2, 5000) and size(1, 5000) < size(1, 5000 + 64 * HOP)
    for B, L in ((0, 5000), (65, 5000), (1, 0), (1, (1 << 30) + 1)):
        assert size(B, L) == -1
    assert lib.vsp_denoise_rows_workspace_bytes(None, 1, 5000) == -1


# ---------------------------------------------------------------------------------------------- the stream's bookkeeping
@pytest.fixture(scope="module")
def rows():
    return dr.fixture_rows()


@pytest.fixture(scope="module")
def wholes(rows):
    """The restatement's whole-row result per row (a row of at most pad samples: its own samples), computed once."""
    return [sr.whole(x, beta, 1.0) if len(x) > PAD else x.copy() for x, beta in rows]


def test_the_restated_call_is_the_restated_denoiser(rows, wholes):
    """One frame at a time against the matrix product of tests/denoiser_ref.py: the same numbers but for the order of the
    DFT sums."""
    for (x, beta), w in zip(rows, wholes):
        d = dr.denoise(x, beta, 1.0)
        assert w.dtype == np.float64 and np.abs(w - d).max() <= 1e-12 * np.abs(x).max(), len(x)


def _stream(eng, x, beta, cut, s=1.0):
    """Streams ``x`` in pieces of ``cut``; checks the bookkeeping after every push.  Returns the joined output."""
    st = denoiser.Stream(eng, beta, s)
    behind, _ = eng.denoise_history()
    outs, pos = [], 0
    for c in cut:
        if pos >= len(x):
            break
        piece = x[pos:pos + c]
        pos += len(piece)
        final = pos >= len(x)
        calls = eng.calls
        y = st.push(piece, final=final)
        outs.append(y)
        assert st.seen == pos and st.out_next == (pos if final else sr.complete(pos))
        assert (eng.calls - calls) == int(len(y) > 0 and not (final and len(x) <= PAD))     # no call where nothing completes
        # what is kept starts at the first sample the next call can read, and never behind it
        assert st.first == max(0, min(pos, st.out_next - behind)) and st.first + len(st.buf) == pos
    return np.concatenate(outs)


@pytest.mark.parametrize("cut", list(CUTS))
def test_every_row_under_every_cut_has_the_bits_of_the_whole(rows, wholes, cut):
    for (x, beta), want in zip(rows, wholes):
        eng = sr.RefEngine()
        got = _stream(eng, x, beta, CUTS[cut](len(x)))
        assert got.shape == want.shape and np.array_equal(got, want), (cut, len(x))
        # every call held what its frames read (the stand-in refuses a row that lacks a sample), and nothing older than
        # `behind` before its first output
        assert all(first == max(0, out_first - (N - HOP)) for first, _, out_first, _, _ in eng.rows)


def test_a_final_push_of_no_samples_flushes_the_stream(rows, wholes):
    for b in (1, 3, 5, 7):
        x, beta = rows[b]
        eng = sr.RefEngine()
        st = denoiser.Stream(eng, beta, 1.0)
        outs = [st.push(x[:len(x) // 2]), st.push(x[len(x) // 2:]), st.push(x[:0], final=True)]
        assert len(outs[2]) == len(x) - sr.complete(len(x)) > 0
        assert np.array_equal(np.concatenate(outs), wholes[b]), b
        assert eng.rows[-1][4] == len(x) and eng.rows[-1][0] == max(0, sr.complete(len(x)) - (N - HOP))


def test_a_stream_that_ends_at_pad_samples_or_fewer_is_left_alone(rows):
    x, beta = rows[7]
    for n, cut in ((PAD, [PAD]), (PAD, [500, 268]), (1, [1]), (300, [100, 100, 100])):
        eng = sr.RefEngine()
        got = _stream(eng, x[:n], beta, cut)
        assert eng.calls == 0 and np.array_equal(got, x[:n]), n
    eng = sr.RefEngine()
    assert np.array_equal(_stream(eng, x[:PAD + 1], beta, [400, 369]), sr.whole(x[:PAD + 1], beta, 1.0)) and eng.calls == 1


def test_several_streams_advance_in_one_call(rows, wholes):
    eng = sr.RefEngine()
    idx = (7, 6, 3)
    st = [denoiser.Stream(eng, rows[b][1], 1.0) for b in idx]
    pos, outs = [0, 0, 0], [[], [], []]
    steps = [(3000, 100, 2500), (700, 2000, 5691), (16 * HOP + 1, 3000, 0), (10 ** 6, 10 ** 6, 0)]
    for k, step in enumerate(steps):
        pushes = []
        for i, (b, n) in enumerate(zip(idx, step)):
            x = rows[b][0]
            if pos[i] >= len(x):
                continue
            piece = x[pos[i]:pos[i] + n]
            pos[i] += len(piece)
            pushes.append((i, (st[i], piece, pos[i] >= len(x))))
        calls = eng.calls
        for (i, _), y in zip(pushes, denoiser.push_rows(eng, [p for _, p in pushes])):
            outs[i].append(y)
        assert eng.calls == calls + 1, k                                      # ONE call for all of them
    for i, b in enumerate(idx):
        assert np.array_equal(np.concatenate(outs[i]), wholes[b]), b
    assert denoiser.push_rows(eng, []) == []


def test_an_engine_with_history_and_rows_alone_is_enough(rows, wholes):
    """Without ``denoise_complete`` the stream takes the same rule from the history: the same calls, the same bits."""
    class TwoMethods:
        def __init__(self):
            self.ref = sr.RefEngine()
            self.denoise_history, self.denoise_rows = self.ref.denoise_history, self.ref.denoise_rows

    x, beta = rows[6]
    eng, full = TwoMethods(), sr.RefEngine()
    a, b = denoiser.Stream(eng, beta, 1.0), denoiser.Stream(full, beta, 1.0)
    for n in range(0, 3 * N + 1, 7):
        assert a._complete(n) == b._complete(n) == sr.complete(n), n
    got = np.concatenate([a.push(x[:3000]), a.push(x[3000:3001]), a.push(x[3001:], final=True)])
    assert np.array_equal(got, wholes[6]) and eng.ref.calls == 2


def test_refusals_of_the_host_layer(rows):
    x, beta = rows[5]
    eng = sr.RefEngine()
    st = denoiser.Stream(eng, beta, 1.0)
    st.push(x, final=True)
    with pytest.raises(ValueError, match="final"):
        st.push(x[:10])
    a, b = denoiser.Stream(eng, beta, 1.0), denoiser.Stream(eng, beta, 1.0)
    with pytest.raises(ValueError, match="once per call"):
        denoiser.push_rows(eng, [(a, x[:3000], False), (b, x[:3000], False), (a, x[3000:4000], False)])
    assert a.seen == 0 and b.seen == 0                                        # refused before anything was taken
    for s in (-1.0, NAN, float("inf")):
        with pytest.raises(ValueError, match="strength"):
            denoiser.Stream(eng, beta, s)


# ---------------------------------------------------------------------------------------------- the streaming service
import limiter_ref as lr  # noqa: E402
import output_stage_ref as oref  # noqa: E402
import test_output_rows_host as rows_host  # noqa: E402
import test_service_paths_host as paths_host  # noqa: E402
from test_limiter_host import LIMITED, StreamLimiterEngine  # noqa: E402
from vispeech_amd import limiter, output_stage  # noqa: E402

SN, SHOP = 4 * paths_host.UP, paths_host.UP               # the stand-in's geometry: n_fft 16, hop 4, pad 6, a delay of 12 .. 15
SBETA = np.abs(np.random.default_rng(7).standard_normal((8, SN // 2 + 1))).astype(np.float32) * np.float32(40.0)


class StreamDenoiseEngine(StreamLimiterEngine):
    """The streaming stand-in with the restated denoiser in float32 (n_fft 16, hop 4), its calls recorded."""

    def __init__(self):
        super().__init__()
        self.ref = sr.RefEngine(np.float32, SN, SHOP)

    def denoise_history(self):
        return self.ref.denoise_history()

    def denoise_complete(self, n_seen, closed=False):
        return self.ref.denoise_complete(n_seen, closed)

    def denoise_rows(self, rows, bias):
        import torch
        self.calls.append(("denoise_rows", [(r[1], len(r[0]), r[2], r[3], r[4], r[5]) for r in rows]))
        return [torch.from_numpy(y) for y in self.ref.denoise_rows(rows, bias)]      # (tensors, as the generator's chunks are)


class StreamDenoiseNet(paths_host.StreamNet):
    def __init__(self):
        self._engine = StreamDenoiseEngine()
        self.bias_of = []

    def denoiser_bias(self, sid):
        self.bias_of.append(list(sid))
        return SBETA[list(sid)]


def _wave(rid, frames):
    return np.repeat(10 * rid + np.arange(frames), paths_host.UP).astype(np.float32)


def _denoised(rid, frames, s, sid=None):
    x = _wave(rid, frames)
    return x if len(x) <= (SN - SHOP) // 2 else sr.whole(x, SBETA[rid if sid is None else sid], s, SN, SHOP, np.float32)


def _bytes(y, fmt):
    L, M, _ = output_stage.plan(rows_host.MODEL, fmt[0])
    z = oref.resample_fp64(y, output_stage.taps(rows_host.MODEL, fmt[0]), L, M).astype(np.float32)
    return rows_host.encode_ref(z, output_stage.encoding(fmt[1])).tobytes()


@pytest.mark.parametrize("chunk", [4, 3])
def test_streaming_service_denoises_in_front_of_the_limiter_and_the_output_rows(chunk):
    from vispeech_amd.service import StreamingBatchService
    net = StreamDenoiseNet()
    eng = net._engine
    svc = StreamingBatchService(net, collate=paths_host._collate, autostart=False, chunk_frames=chunk)
    a = svc.submit({"id": 1, "frames": 30}, 1, denoise=0.5, limiter=LIMITED)         # a denoiser and a limiter behind it
    b = svc.submit({"id": 2, "frames": 9}, 2)                                        # a neighbour that names nothing
    svc.step(); svc.step()
    c = svc.submit({"id": 3, "frames": 14}, 3, denoise=True, output_rate=8000, output_encoding="ulaw")
    d = svc.submit({"id": 4, "frames": 1}, 4, denoise=2.0)                           # 4 samples <= pad: left alone
    svc.close()
    base = (rows_host.MODEL, "s16")
    A, H, ceil, g = limiter.spec(LIMITED, rows_host.MODEL)
    want_a = lr.limit(_denoised(1, 30, 0.5), g, ceil, A, H, np.float32)["out"]
    assert not np.array_equal(_denoised(1, 30, 0.5), _wave(1, 30))
    assert b"".join(paths_host._pieces(a)) == _bytes(want_a, base)
    assert b"".join(paths_host._pieces(c)) == _bytes(_denoised(3, 14, 0.01), (8000, "ulaw"))
    assert b"".join(paths_host._pieces(d)) == _bytes(_wave(4, 1), base)
    assert b"".join(paths_host._pieces(b)) == rows_host._one_shot_bytes(2, 9, None, base)      # the bytes of its own path
    assert sorted(s for call in net.bias_of for s in call) == [1, 3, 4]              # each request's own speaker, once
    # every tick: at most ONE denoiser call, in front of at most one limiter call, in front of the tick's output rows
    names = [k[0] for k in eng.calls if k[0] in ("denoise_rows", "limiter_rows", "output_rows")]
    ticks = "".join(n[0] for n in names).split("o")[:-1]
    assert len(ticks) == svc.stats["ticks"] and set(ticks) <= {"", "d", "dl", "l"} and "dl" in ticks
    den = [k[1] for k in eng.calls if k[0] == "denoise_rows"]
    assert max(len(k) for k in den) == 2
    # the denoiser's rows: each stream's outputs tile [0, total), the last chunk carries the end, the strengths are the requests'
    for rid, frames, s in ((1, 30, 0.5), (3, 14, 0.01)):
        mine = [r for k in den for r in k if r[5] == s]
        assert [r[2] for r in mine] == list(np.cumsum([0] + [r[3] for r in mine])[:-1]) and sum(r[3] for r in mine) == frames * SHOP
        assert [r[4] for r in mine[:-1]] == [-1] * (len(mine) - 1) and mine[-1][4] == frames * SHOP
    # the limiter behind it is handed the denoiser's samples at the denoiser's positions: its samples end where they end
    lim = [k[1][0] for k in eng.calls if k[0] == "limiter_rows"]
    assert lim[0][0] == 0 and lim[-1][4] == 30 * SHOP and all(r[0] + r[1] <= 30 * SHOP for r in lim)
    # the first tick: 16 samples complete 2 (too few for the limiter behind), 12 complete none -- no call, and only the
    # neighbour rides in the tick's output rows
    assert ticks[0] == ("d" if chunk == 4 else "")
    assert len([k for k in eng.calls if k[0] == "output_rows"][0][1]) == 1


def test_streaming_service_default_denoiser_and_opting_out():
    from vispeech_amd.service import StreamingBatchService
    net = StreamDenoiseNet()
    svc = StreamingBatchService(net, collate=paths_host._collate, autostart=False, chunk_frames=4, denoise=0.5)
    assert svc.denoise == 0.5
    a = svc.submit({"id": 1, "frames": 11}, 1)
    b = svc.submit({"id": 2, "frames": 6}, 2, denoise=False)
    svc.close()
    base = (rows_host.MODEL, "s16")
    assert b"".join(paths_host._pieces(a)) == _bytes(_denoised(1, 11, 0.5), base)
    assert b"".join(paths_host._pieces(b)) == rows_host._one_shot_bytes(2, 6, None, base)
    for bad in (-0.1, NAN, float("inf"), "strong", dict(strength=1.0)):
        with pytest.raises(ValueError):
            svc.submit({"id": 1, "frames": 3}, 3, denoise=bad)
    with pytest.raises(ValueError):
        StreamingBatchService(net, collate=paths_host._collate, autostart=False, denoise=-1.0)


def test_a_service_in_which_nobody_names_a_denoiser_makes_the_old_calls():
    from vispeech_amd.service import StreamingBatchService

    def run(**kw):
        net = paths_host.StreamNet()
        net._engine = eng = rows_host.StreamRowsEngine()
        svc = StreamingBatchService(net, collate=paths_host._collate, autostart=False, chunk_frames=4)
        s = [svc.submit({"id": 1, "frames": 11}, 1, output_rate=8000, output_encoding="ulaw", **kw), svc.submit({"id": 2, "frames": 6}, 2, **kw)]
        svc.close()
        return eng.calls, [b"".join(paths_host._pieces(x)) for x in s]

    assert run() == run(denoise=False) == run(denoise=None)                  # (an engine without a denoiser at all)


def test_fused_output_refuses_a_denoiser():
    from vispeech_amd.service import StreamingBatchService
    net = paths_host.StreamNet()
    svc = StreamingBatchService(net, collate=paths_host._collate, autostart=False, output_rate=22050, fused_output=True)
    with pytest.raises(ValueError, match="fused_output"):
        svc.submit({"id": 1, "frames": 3}, 1, denoise=True)
    with pytest.raises(ValueError, match="fused_output"):
        svc.submit_conversion(paths_host._audio(50), 1, 2, 3, denoise=0.5)
    with pytest.raises(ValueError, match="fused_output"):
        svc.open_conversion(1, 2, 3, denoise=True)
    svc.submit({"id": 1, "frames": 3}, 1, denoise=False).close()
    with pytest.raises(ValueError, match="fused_output"):
        StreamingBatchService(net, collate=paths_host._collate, autostart=False, output_rate=22050, fused_output=True, denoise=True)
