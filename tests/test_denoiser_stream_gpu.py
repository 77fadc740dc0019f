"""The denoiser for streams on the GPU: ``vsp_denoise_rows`` and ``vispeech_amd.denoiser`` against
``Engine.denoise`` on the whole row -- bit for bit: a whole row as one row of the call, a row streamed under five cuts, five
streams at different positions in one call --, against the fp64 restatement of one call (tests/denoiser_stream_ref.py)
under the gate rule of tests/test_denoiser_gpu.py, the refusals, the workspace and ``StreamingBatchService(denoise=)``.

The cuts: one push; hop-sized pushes; 1279, 1, 512, 511, 513 and then 997s (a first push that completes nothing, a push of
one sample, pushes on, below and above the hop, then pieces that are no multiple of anything); pieces of 100 (most pushes
complete nothing); pieces of 16 hop + 1 (a call then spans more than one overlap-add tile of 16 frames and its window
starts off a tile boundary of the one-shot call)."""
import ctypes as C

import numpy as np
import pytest
import torch

import denoiser_ref as dr
import denoiser_stream_ref as sr

pytestmark = pytest.mark.gpu

HOP, N_FFT, PAD = dr.HOP, dr.N_FFT, dr.pad_of()
BEHIND = N_FFT - HOP
ALONE = dr.ROW_ALONE
LIVE = [b for b in range(len(dr.LENGTHS)) if b != ALONE]
STREAMED = [1, 3, 5, 6, 7]                                # 1023, 16 hop - 1, 16 hop, 17 hop + 300, 40 hop + 77
CUTS = {
    "one": lambda n: [n],
    "hop": lambda n: [HOP] * (n // HOP + 1),
    "odd": lambda n: [1279, 1, 512, 511, 513] + [997] * (n // 997 + 1),
    "100": lambda n: [100] * (n // 100 + 1),
    "16hop+1": lambda n: [16 * HOP + 1] * (n // (16 * HOP + 1) + 1),
}
S_CUT = 1.0


def to_np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def net():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from vispeech_amd import config as vcfg
    from vispeech_amd.models import SynthesizerTrn
    from vispeech_amd.schema import ModelDims
    from vispeech_amd.synth import synth_state_dict
    args, kwargs = vcfg.synthesizer_args(vcfg.default_hparams())
    m = SynthesizerTrn(*args, **kwargs).eval()
    m.load_state_dict(synth_state_dict(ModelDims(), seed=1234), strict=True)
    return m


@pytest.fixture(scope="module")
def rows():
    return dr.fixture_rows()


@pytest.fixture(scope="module")
def one_shot(net, rows):
    """Per strength: ``Engine.denoise`` on the fixture's batch of eight (row ALONE at a NaN strength), computed once."""
    audio, n = dr.pack([x for x, _ in rows])
    bias = np.stack([b for _, b in rows])
    out = {}
    for s in (0.01, 1.0, 50.0):
        strength = [float("nan") if b == ALONE else s for b in range(len(rows))]
        got = to_np(net._engine.denoise(torch.from_numpy(audio.copy()).to(net.device), n, bias, strength))
        out[s] = [got[b, :n[b]].copy() for b in range(len(rows))]
    return out


class Counting:
    """The engine with its ``denoise_rows`` calls counted."""

    def __init__(self, eng):
        self.eng, self.calls = eng, 0

    def denoise_history(self):
        return self.eng.denoise_history()

    def denoise_complete(self, n_seen, closed=False):
        return self.eng.denoise_complete(n_seen, closed)

    def denoise_rows(self, rows, bias):
        self.calls += 1
        return self.eng.denoise_rows(rows, bias)


def test_history_and_complete_are_the_restatements(net):
    eng = net._engine
    assert eng.denoise_history() == (BEHIND, N_FFT - 1)
    for n in list(range(0, 3 * N_FFT + 1, 37)) + [N_FFT - PAD - 1, N_FFT - PAD, N_FFT - PAD + HOP - 1, N_FFT - PAD + HOP]:
        assert eng.denoise_complete(n) == sr.complete(n), n
        assert eng.denoise_complete(n, True) == n


@pytest.mark.parametrize("s", (0.01, 1.0, 50.0))
def test_whole_rows_have_the_bits_of_denoise(net, rows, one_shot, s):
    dev = net.device
    call = [(torch.from_numpy(rows[b][0]).to(dev), 0, 0, len(rows[b][0]), len(rows[b][0]), s) for b in LIVE]
    got = net._engine.denoise_rows(call, np.stack([rows[b][1] for b in LIVE]))
    for b, y in zip(LIVE, got):
        assert np.array_equal(to_np(y), one_shot[s][b]), (s, b)


@pytest.mark.parametrize("cut", list(CUTS))
def test_any_split_has_the_bits_of_the_whole(net, rows, one_shot, cut):
    from vispeech_amd import denoiser
    dev = net.device
    for b in STREAMED:
        x, beta = rows[b]
        eng = Counting(net._engine)
        st = denoiser.Stream(eng, torch.from_numpy(beta).to(dev), S_CUT)
        xd = torch.from_numpy(x).to(dev)
        outs, pos, completing = [], 0, 0
        for c in CUTS[cut](len(x)):
            if pos >= len(x):
                break
            piece = xd[pos:pos + c]
            pos += int(piece.shape[0])
            y = st.push(piece, final=pos >= len(x))
            completing += int(y.shape[0] > 0)
            outs.append(y)
            assert st.out_next == (len(x) if pos >= len(x) else sr.complete(pos)) and st.seen == pos
        got = to_np(torch.cat(outs))
        assert got.shape == (len(x),) and np.array_equal(got, one_shot[S_CUT][b]), (cut, b)
        assert eng.calls == completing, (cut, b, eng.calls, completing)


# ---- the C call itself, on buffers with guards ---------------------------------------------------------------------
GUARD = 64


class Raw:
    """``vsp_denoise_rows`` on caller-made buffers: row b's samples sit in a NaN-filled buffer at offset GUARD, its outputs
    in another (or, in place, in the same buffer at the same positions)."""

    def __init__(self, net):
        from vispeech_amd import _lib
        self.net, self.eng, self._lib = net, net._engine, _lib

    def run(self, rows, bias, in_place=False, ws_bytes=None, B=None, sentinel=float("nan")):
        """rows: (samples np, first, out_first, out_count, total, strength).  Returns (rc, message, ins, outs) with the
        buffers read back whole."""
        dev, eng = self.net.device, self.eng
        n_rows = len(rows)
        desc = (self._lib.VspDenoiseRow * max(n_rows, B or 0))()
        ins, outs = [], []
        for b, (x, first, out_first, out_count, total, s) in enumerate(rows):
            buf = np.full(len(x) + 2 * GUARD, np.nan, np.float32)
            buf[GUARD:GUARD + len(x)] = x
            i = torch.from_numpy(buf).to(dev)
            o = i if in_place else torch.full((max(out_count, 0) + 2 * GUARD,), sentinel, dtype=torch.float32, device=dev)
            off = GUARD + (out_first - first if in_place else 0)
            ins.append(i)
            outs.append(o)
            desc[b] = self._lib.VspDenoiseRow(i.data_ptr() + 4 * GUARD, first, len(x), o.data_ptr() + 4 * off, out_first, out_count,
                                              total, s)
        bp = None if bias is None else torch.from_numpy(np.ascontiguousarray(bias, np.float32)).to(dev)
        L_max = max(1, max(r[3] for r in rows))
        need = int(eng.lib.vsp_denoise_rows_workspace_bytes(eng.ctx, min(max(B or n_rows, 1), 64), L_max))
        assert need > 0
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            rc = eng.lib.vsp_denoise_rows(eng.ctx, eng._stream(), B or n_rows, desc, None if bp is None else C.c_void_p(bp.data_ptr()),
                                          C.c_void_p(ws.data_ptr()), need if ws_bytes is None else ws_bytes(need))
        torch.cuda.synchronize(dev)
        msg = eng.lib.vsp_last_error(eng.ctx)
        return rc, (msg.decode("utf-8", "replace") if msg else ""), [to_np(t) for t in ins], [to_np(t) for t in outs]


@pytest.fixture(scope="module")
def raw(net):
    return Raw(net)


def _piece(x, n0, n1, final=False):
    """The row of a stream of samples ``x`` that had seen n0 samples and now has n1 (all of them, ``final``)."""
    o0 = sr.complete(n0)
    o1 = len(x) if final else sr.complete(n1)
    first = max(0, o0 - BEHIND)
    return (x[first:n1], first, o0, o1 - o0, len(x) if final else -1)


@pytest.mark.parametrize("in_place", (False, True))
def test_five_streams_in_one_call(raw, rows, one_shot, in_place):
    s = 1.0
    x7, x6, x5, x3 = rows[7][0], rows[6][0], rows[5][0], rows[3][0]
    pieces = [
        (6, _piece(x6, 0, 3000)),                            # its first call
        (7, _piece(x7, 4000, 4000 + 16 * HOP + 1)),          # mid-stream, more than one tile
        (5, _piece(x5, 2500, 3777)),                         # mid-stream at another offset
        (3, _piece(x3, 6000, len(x3), final=True)),          # ends in this call, under the smallest window sum
    ]
    call = [p + (s,) for _, p in pieces] + [(x7[:1000].copy(), 0, 0, 500, -1, float("nan"))]
    bias = np.stack([rows[b][1] for b, _ in pieces] + [rows[0][1]])
    rc, msg, ins, outs = raw.run(call, bias, in_place=in_place)
    assert rc == 0, msg
    for (b, (x, first, o0, cnt, _)), i, o in zip(pieces, ins, outs):
        assert cnt > 0
        want = one_shot[s][b][o0:o0 + cnt]
        if in_place:
            off = GUARD + o0 - first
            assert np.array_equal(o[off:off + cnt], want), b
            assert np.array_equal(o[GUARD:off], x[:o0 - first]) and np.array_equal(o[off + cnt:GUARD + len(x)], x[o0 - first + cnt:]), b
            assert np.all(np.isnan(o[:GUARD])) and np.all(np.isnan(o[GUARD + len(x):])), b
        else:
            assert np.array_equal(o[GUARD:GUARD + cnt], want), b
            assert np.all(np.isnan(o[:GUARD])) and np.all(np.isnan(o[GUARD + cnt:])), b      # nothing else is written
            assert np.array_equal(i[GUARD:GUARD + len(x)], x), b
    # the NaN-strength row: neither read nor written
    assert np.array_equal(ins[4][GUARD:GUARD + 1000], x7[:1000])
    assert np.all(np.isnan(outs[4][:GUARD])) and np.all(np.isnan(outs[4][GUARD + (1000 if in_place else 500):]))
    if not in_place:
        assert np.all(np.isnan(outs[4]))


def test_one_call_against_fp64(raw, rows):
    """A mid-stream call (first > 0, open, five frames of output) and a closing call under the smallest window sum (row 16
    hop - 1), each against the fp64 restatement of that call: the gate is 4 times the float32 restatement's distance
    from fp64 on those samples, and at least ``floor_of`` of the row."""
    s = 1.0
    x7, b7 = rows[7]
    x3, b3 = rows[3]
    n0 = N_FFT - PAD + 10 * HOP
    mid = _piece(x7, n0, n0 + 5 * HOP)
    end = _piece(x3, 6000, len(x3), final=True)
    assert mid[1] > 0 and mid[3] == 5 * HOP and end[4] == 16 * HOP - 1
    rc, msg, _, outs = raw.run([mid + (s,), end + (s,)], np.stack([b7, b3]))
    assert rc == 0, msg
    for name, (x, first, o0, cnt, total), beta, full, o in (("mid-stream", mid, b7, x7, outs[0]), ("closing", end, b3, x3, outs[1])):
        d = sr.call(x, first, o0, cnt, total, beta, s)
        f = sr.call(x, first, o0, cnt, total, beta, s, dtype=np.float32)
        gate = max(4.0 * float(np.abs(f.astype(np.float64) - d).max()), dr.floor_of(full, len(full)))
        dist = float(np.abs(o[GUARD:GUARD + cnt] - d).max())
        print(f"{name}: outputs [{o0}, {o0 + cnt}) distance {dist:.2e} gate {gate:.2e}")
        assert dist <= gate, (name, dist, gate)


def test_refusals_name_the_row_and_launch_nothing(raw, rows):
    x, beta = rows[7]
    good = _piece(x, 4000, 6000) + (1.0,)
    bias = np.stack([beta, beta])
    xs, first, o0, cnt, total = good[:5]
    cases = {
        "history": (xs[HOP:], first + HOP, o0, cnt, total, 1.0),
        "look-ahead": (xs[:-HOP], first, o0, cnt, total, 1.0),
        "total <= pad": (x[:PAD], 0, 0, PAD, PAD, 1.0),
        "strength": (xs, first, o0, cnt, total, -1.0),
    }
    for name, bad in cases.items():
        rc, msg, _, outs = raw.run([good, bad], bias, sentinel=7.0)
        print(f"{name}: {msg}")
        assert rc == -1 and "row 1" in msg, (name, rc, msg)
        assert all(np.all(o == 7.0) for o in outs), name                      # refused before any launch
    rc, msg, _, outs = raw.run([good], np.stack([beta] * 65), B=65, sentinel=7.0)
    assert rc == -1 and "64" in msg and np.all(outs[0] == 7.0), (rc, msg)
    rc, msg, _, outs = raw.run([good], None, sentinel=7.0)
    assert rc == -1 and "row 0" in msg and np.all(outs[0] == 7.0), (rc, msg)


def test_workspace(raw, rows, one_shot):
    x, beta = rows[6]
    row = (x, 0, 0, len(x), len(x), 1.0)
    rc, msg, _, outs = raw.run([row], beta[None, :], ws_bytes=lambda need: need - 1, sentinel=7.0)
    assert rc == -6 and np.all(outs[0] == 7.0), (rc, msg)
    rc, msg, _, outs = raw.run([row], beta[None, :])
    assert rc == 0 and np.array_equal(outs[0][GUARD:GUARD + len(x)], one_shot[1.0][6]), (rc, msg)
    eng = raw.eng
    size = lambda B, L: int(eng.lib.vsp_denoise_rows_workspace_bytes(eng.ctx, B, L))
    assert size(1, 1) <= size(1, HOP + 2) <= size(2, HOP + 2) <= size(2, 20 * HOP) and size(0, 1) < 0 and size(65, 1) < 0


# ---------------------------------------------------------------------------------------------- the streaming service
def test_streaming_service_denoises_the_request_that_asks(net):
    """Two text requests of 11 and 6 frames in ticks of 4 frames, float32 at the model's rate (the pass-through: the
    waveform's bits).  The request with ``denoise=0.5``: the bits of ``net.denoise`` on its plain waveform, whose pieces
    come out at the denoiser's delay; with a limiter behind it, ``net.limit`` of that.  The neighbour: its own bytes."""
    from vispeech_amd.service import StreamingBatchService
    import isolated_ref as iso
    batch = iso.make_batch([11, 6], [4, 2], seed=2140)
    collate = lambda rows: {k: batch[k][rows] for k in ("phonemes", "lengths", "sid", "duration", "f0", "energy")}

    def serve(**kw):
        svc = StreamingBatchService(net, max_batch=2, chunk_frames=4, collate=collate, autostart=False)
        streams = [svc.submit(0, 11, output_encoding="f32", **kw), svc.submit(1, 12, output_encoding="f32")]
        svc.close()
        pieces = [list(s) for s in streams]
        return [np.frombuffer(b"".join(p), "<f4") for p in pieces], [[len(x) // 4 for x in p] for p in pieces]

    plain, _ = serve()
    got, sizes = serve(denoise=0.5)
    n = plain[0].shape[0]
    assert n == 11 * HOP and got[0].shape == (n,) and plain[1].shape == (6 * HOP,)
    assert plain[1].tobytes() == got[1].tobytes()                            # the request that names none: its bytes
    sid = int(batch["sid"][0])
    wave = lambda a: torch.from_numpy(a.copy())[None, :].to(net.device)
    want = to_np(net.denoise(wave(plain[0]), [n], [sid], strength=0.5))[0]
    assert np.array_equal(got[0], want) and not np.array_equal(got[0], plain[0])
    # three ticks of 4, 4 and 3 frames: what each completes, the last with the flush (no piece is empty)
    assert sizes[0] == [sr.complete(4 * HOP), sr.complete(8 * HOP) - sr.complete(4 * HOP), n - sr.complete(8 * HOP)]
    # a limiter behind the denoiser: the one-shot calls in the one-shot service's order
    lim, _ = serve(denoise=0.5, limiter=True)
    y, _ = net.limit(wave(want), [n], ceiling=1.0)
    assert np.array_equal(lim[0], to_np(y)[0]) and lim[1].tobytes() == plain[1].tobytes()
    # ... and one that has work to do: half the denoised peak under 3 dB of gain
    c = 0.5 * float(np.abs(want).max())
    hard, _ = serve(denoise=0.5, limiter=dict(ceiling=c, gain_db=3.0))
    y, mg = net.limit(wave(want), [n], ceiling=c, gains=[10.0 ** (3.0 / 20.0)])
    assert float(mg[0]) < 0.8 and np.array_equal(hard[0], to_np(y)[0])
    # the service's own setting, and a request that opts out of it
    svc = StreamingBatchService(net, max_batch=2, chunk_frames=4, collate=collate, autostart=False, denoise=0.5)
    streams = [svc.submit(0, 11, output_encoding="f32"), svc.submit(1, 12, output_encoding="f32", denoise=False)]
    svc.close()
    both = [np.frombuffer(b"".join(s), "<f4") for s in streams]
    assert np.array_equal(both[0], want) and both[1].tobytes() == plain[1].tobytes()
    assert net._engine.status() == 0


def test_denoise_stream_of_the_model(net):
    """``SynthesizerTrn.denoise_stream``: the speaker's own bias, the bits of ``SynthesizerTrn.denoise``."""
    x = dr.voiced(7 * HOP + 123, 77)
    xd = torch.from_numpy(x).to(net.device)
    want = to_np(net.denoise(xd.clone()[None, :], [len(x)], [17], strength=0.3))[0]
    st = net.denoise_stream(17, strength=0.3)
    got = torch.cat([st.push(xd[:3000]), st.push(xd[3000:3001]), st.push(xd[3001:], final=True)])
    assert st.out_next == st.seen == len(x) and np.array_equal(to_np(got), want)
