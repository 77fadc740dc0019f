"""The denoiser for streams on the in-LDS FFT (DESIGN.md sections 4u and 4v): under ``transform="fft"`` a stream cut anywhere
gives the BITS of ``Engine.denoise(..., transform="fft")`` on the whole row -- every frame is transformed on its own, by one
template of the fused kernel in the one-shot and the rows form, so the property holds by construction; the overlap-add chain
is the product path's.  The split patterns are those of tests/test_denoiser_stream_gpu.py: one push; hop-sized pushes;
1279, 1, 512, 511, 513 and then 997s; pieces of 100; pieces of 16 hop + 1 (a window then starts off the tile boundaries of
the one-shot call, and spans more than two tiles of 8 frames)."""
import numpy as np
import pytest
import torch

import denoiser_ref as dr
import denoiser_stream_ref as sr
from test_denoiser_stream_gpu import ALONE, BEHIND, CUTS, HOP, LIVE, STREAMED, S_CUT, to_np

pytestmark = pytest.mark.gpu


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
    """``Engine.denoise(..., transform="fft")`` on the fixture's batch of eight (row ALONE at a NaN strength), computed once."""
    audio, n = dr.pack([x for x, _ in rows])
    bias = np.stack([b for _, b in rows])
    strength = [float("nan") if b == ALONE else S_CUT for b in range(len(rows))]
    got = to_np(net._engine.denoise(torch.from_numpy(audio.copy()).to(net.device), n, bias, strength, transform="fft"))
    return [got[b, :n[b]].copy() for b in range(len(rows))]


class Counting:
    """The engine with its ``denoise_rows`` calls counted and their keyword recorded."""

    def __init__(self, eng):
        self.eng, self.calls, self.kw = eng, 0, set()
        self.denoise_history, self.denoise_complete = eng.denoise_history, eng.denoise_complete

    def denoise_rows(self, rows, bias, **kw):
        self.calls += 1
        self.kw.add(tuple(sorted(kw.items())))
        return self.eng.denoise_rows(rows, bias, **kw)


def test_whole_rows_have_the_bits_of_denoise(net, rows, one_shot):
    dev = net.device
    call = [(torch.from_numpy(rows[b][0]).to(dev), 0, 0, len(rows[b][0]), len(rows[b][0]), S_CUT) for b in LIVE]
    got = net._engine.denoise_rows(call, np.stack([rows[b][1] for b in LIVE]), transform="fft")
    for b, y in zip(LIVE, got):
        assert np.array_equal(to_np(y), one_shot[b]), b
    plain = net._engine.denoise_rows(call[:1], rows[LIVE[0]][1][None, :])
    assert not np.array_equal(to_np(plain[0]), one_shot[LIVE[0]])            # (the default is still the product: other bits)


@pytest.mark.parametrize("cut", list(CUTS))
def test_any_split_has_the_bits_of_the_whole(net, rows, one_shot, cut):
    from vispeech_amd import denoiser
    dev = net.device
    for b in STREAMED:
        x, beta = rows[b]
        eng = Counting(net._engine)
        st = denoiser.Stream(eng, torch.from_numpy(beta).to(dev), S_CUT, transform="fft")
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
        assert got.shape == (len(x),) and np.array_equal(got, one_shot[b]), (cut, b)
        assert eng.calls == completing and eng.kw == {(("transform", "fft"),)}, (cut, b, eng.calls, completing)


def test_five_streams_at_different_positions_in_one_call(net, rows, one_shot):
    """Each stream's piece -- its first call, mid-stream over more than one tile, mid-stream at another offset, one that ends
    in this call under the smallest window sum, one pushed whole -- has the bits it has alone, which are the whole row's."""
    dev, eng = net.device, net._engine

    def piece(b, n0, n1, final=False):
        x = rows[b][0]
        o0, o1 = sr.complete(n0), len(x) if final else sr.complete(n1)
        first = max(0, o0 - BEHIND)
        return b, (torch.from_numpy(x[first:n1].copy()).to(dev), first, o0, o1 - o0, len(x) if final else -1, S_CUT)

    pieces = [piece(6, 0, 3000), piece(7, 4000, 4000 + 16 * HOP + 1), piece(5, 2500, 3777),
              piece(3, 6000, len(rows[3][0]), final=True), piece(1, 0, len(rows[1][0]), final=True)]
    bias = np.stack([rows[b][1] for b, _ in pieces])
    together = eng.denoise_rows([p for _, p in pieces], bias, transform="fft")
    for i, ((b, p), y) in enumerate(zip(pieces, together)):
        assert p[3] > 0
        alone = eng.denoise_rows([p], bias[i:i + 1], transform="fft")[0]
        assert np.array_equal(to_np(y), to_np(alone)), b
        assert np.array_equal(to_np(y), one_shot[b][p[2]:p[2] + p[3]]), b


def test_streaming_service_delivers_the_bytes_of_the_one_shot_fft_path(net):
    """Two text requests of 11 and 6 frames in ticks of 4 frames, float32 at the model's rate (the pass-through: the
    waveform's bits).  The request with ``denoise=0.5`` in a service with ``denoise_transform="fft"``: the bits of
    ``net.denoise(..., transform="fft")`` on its plain waveform.  The neighbour: its own bytes."""
    from vispeech_amd.service import StreamingBatchService
    import isolated_ref as iso
    batch = iso.make_batch([11, 6], [4, 2], seed=2140)
    collate = lambda rows: {k: batch[k][rows] for k in ("phonemes", "lengths", "sid", "duration", "f0", "energy")}

    def serve(denoise=None, **svc_kw):
        svc = StreamingBatchService(net, max_batch=2, chunk_frames=4, collate=collate, autostart=False, **svc_kw)
        streams = [svc.submit(0, 11, output_encoding="f32", denoise=denoise), svc.submit(1, 12, output_encoding="f32")]
        svc.close()
        return [np.frombuffer(b"".join(list(s)), "<f4") for s in streams]

    plain = serve()
    got = serve(denoise=0.5, denoise_transform="fft")
    n = plain[0].shape[0]
    assert n == 11 * HOP and got[0].shape == (n,) and plain[1].tobytes() == got[1].tobytes()
    sid = int(batch["sid"][0])
    wave = lambda a: torch.from_numpy(a.copy())[None, :].to(net.device)
    want = to_np(net.denoise(wave(plain[0]), [n], [sid], strength=0.5, transform="fft"))[0]
    assert np.array_equal(got[0], want) and not np.array_equal(got[0], plain[0])
    # a service that names no transform: the bytes of the product path, as before
    dft = serve(denoise=0.5)
    assert np.array_equal(dft[0], to_np(net.denoise(wave(plain[0]), [n], [sid], strength=0.5))[0]) and not np.array_equal(dft[0], got[0])
    assert net._engine.status() == 0
