"""The denoiser and the inverse STFT on the GPU against tests/denoiser_ref.py: ``vsp_istft`` alone,
``vsp_denoise_bias``, ``vsp_denoise`` at four strengths, the identity at strength 0, the ragged contract, the generator's own
zero-input output denoised with its own bias, and a ``denoise`` request in ``BatchingSynthesisService``.

One ragged batch of eight rows (``denoiser_ref.LENGTHS``) holds the lengths at which the kernels change path -- one frame
(``pad + 1``), one frame with 511 samples of slack (the smallest window sum, 0.022), two frames, either side of the tile of
16 frames the framing and the overlap-add kernel share, just past it, several tiles and a ragged rest -- and in its middle
a row whose strength is NaN.  NaN lies behind every row's end.

The gate of a row is NOT taken from the library: it is 4 times the distance of the restatement's float32 run from its fp64
run on that row, and at least a floor derived from the number format.  The floor: an output sample is a DFT sum of 2 spec
= 2050 products accumulated in float32, every partial sum rounded by up to 2^-24 of its size; the partial sums are of the
size of the result, at most the row's peak P, and roundings of either sign add as a random walk, so the sum carries about
sqrt(2048) 2^-24 P -- before it is divided by the window sum W, which multiplies it by at most 1 / min W of the row:
floor = sqrt(2048) 2^-24 P / min W (2.7e-6 P / min W: 1.8e-6 P where four frames overlap, 1.2e-4 P on the 0.022 rows).

The distances of the float32 run from the fp64 run on the fixture rows (CPU, max over the row, peak about 0.5), the first
term of the gate before its factor 4:
    strength     769      1023     1024     8191     8192     9004     20557
    0            2.2e-7   4.2e-7   3.9e-7   3.3e-7   4.5e-7   4.2e-7   3.9e-7
    0.01         2.3e-7   3.9e-7   3.3e-7   4.0e-7   3.3e-7   4.3e-7   3.7e-7
    1            1.2e-7   2.5e-7   1.3e-7   2.4e-7   1.9e-7   1.7e-7   1.8e-7
    50           3.1e-8   4.8e-8   1.9e-8   4.9e-8   3.5e-8   4.1e-8   2.1e-8
so the floor decides on the rows that end under a small window sum and at the large strength, the distance elsewhere.
Measured on the MI355X, the library's largest distance from the fp64 run per row at strength 0 / 1 / 50: 4.2e-7 / 3.0e-7 /
1.1e-7 (769), 9.2e-7 / 8.7e-7 / 4.1e-7 (1023), 3.7e-7 / 2.1e-7 / 1.9e-8 (1024), 6.3e-7 / 5.9e-7 / 1.4e-7 (8191), 5.4e-7 / 4.4e-7 /
6.6e-8 (8192), 5.1e-7 / 6.1e-7 / 1.1e-7 (9004), 5.7e-7 / 3.4e-7 / 7.8e-8 (20557), under gates of 9.7e-7 .. 4.4e-5.

A row's bits do not depend on the rows it is batched with: the two DFT products run on ONE form of the frame-rate
convolution whatever B and T_max (``ConvArgs::fixed_form``), which the ragged test crosses on purpose -- a row alone (one
column), in the batch of eight (41 columns) and beside a row of 103 frames."""
import numpy as np
import pytest
import torch

import denoiser_ref as dr

pytestmark = pytest.mark.gpu

STRENGTHS = (0.0, 0.01, 1.0, 50.0)
ALONE = dr.ROW_ALONE
SPEC = dr.N_FFT // 2 + 1


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
def packed(rows):
    """(audio [B, L] with NaN behind every row, lengths, bias [B, spec])."""
    audio, n = dr.pack([x for x, _ in rows])
    return audio, n, np.stack([b for _, b in rows])


@pytest.fixture(scope="module")
def restated(rows):
    """Per strength and row: (fp64 output, gate), computed once."""
    out = {}
    for s in STRENGTHS:
        per = []
        for x, beta in rows:
            d = dr.denoise(x, beta, s)
            f = dr.denoise(x, beta, s, dtype=np.float32)
            per.append((d, max(4.0 * float(np.abs(f.astype(np.float64) - d).max()), dr.floor_of(x, len(x)))))
        out[s] = per
    return out


def _strengths(s):
    return [float("nan") if b == ALONE else s for b in range(len(dr.LENGTHS))]


def _run(net, packed, s, **kw):
    audio, n, bias = packed
    return to_np(net._engine.denoise(torch.from_numpy(audio.copy()).to(net.device), n, bias, _strengths(s), **kw))


def test_istft_alone(net, rows, packed):
    """RI from the fp64 restatement (the subtracted spectrum at strength 1, rounded to float32), NaN in the columns behind
    every row's frames; the output against the restatement's synthesis of the same float32 RI."""
    _, n, _ = packed
    T_max = max(dr.frames(v) for v in n)
    ri = np.full((len(rows), 2 * SPEC, T_max), np.nan, np.float32)
    for b, (x, beta) in enumerate(rows):
        ri[b, :, :dr.frames(len(x))] = dr.subtract(dr.analysis(x), beta, 1.0)
    got = to_np(net._engine.istft(ri, n))
    assert got.shape == (len(rows), max(n))
    for b, (x, _) in enumerate(rows):
        r = ri[b, :, :dr.frames(n[b])]
        d, f = dr.synthesis(r.astype(np.float64), n[b]), dr.synthesis(r, n[b], dtype=np.float32)
        gate = max(4.0 * float(np.abs(f.astype(np.float64) - d).max()), dr.floor_of(x, n[b]))
        dist = float(np.abs(got[b, :n[b]] - d).max())
        print(f"istft row {b} ({n[b]}): distance {dist:.2e} gate {gate:.2e}")
        assert dist <= gate, (b, dist, gate)
        assert np.all(got[b, n[b]:] == 0)                           # nothing behind the row's end is written


def _steady_periods(net, sids):
    eng = net._engine
    back, fwd = eng.generator_frame_dependence()
    g = torch.from_numpy(net._state["emb_g.weight"][sids]).to(net.device)
    z = torch.zeros((len(sids), net.dims.inter_channels, back + 1 + fwd), dtype=torch.float32, device=net.device)
    o = eng.generator(z, g)
    return o[:, 0, back * dr.HOP:(back + 1) * dr.HOP].contiguous(), g


def test_denoise_bias_is_the_dft_of_the_period(net):
    """The period fed in is the library's own steady frame, so the gate judges the transform and not the generator.  The
    floor is that of the file's text with the result's own size in the place of P: sqrt(2048) 2^-24 max(beta)."""
    sids = [3, 17, 199]
    period, g = _steady_periods(net, sids)
    got = to_np(net._engine.denoise_bias_of(period))
    assert got.shape == (3, SPEC) and np.all(got >= 0)
    assert np.array_equal(got, to_np(net._engine.denoise_bias(g)))          # the engine's own way to the same rows
    assert np.array_equal(got, to_np(net.denoiser_bias(sids)))              # ... and the model's table
    assert np.array_equal(got[[2, 0]], to_np(net.denoiser_bias([199, 3])))  # (cached: any order, same rows)
    for i, c in enumerate(to_np(period)):
        d, f = dr.bias_of(c), dr.bias_of(c, dtype=np.float32)
        gate = max(4.0 * float(np.abs(f.astype(np.float64) - d).max()), float(np.sqrt(2048.0) * dr.U32 * d.max()))
        dist = float(np.abs(got[i] - d).max())
        print(f"bias speaker {sids[i]}: max {d.max():.3e} distance {dist:.2e} gate {gate:.2e}")
        assert d.max() > 0 and dist <= gate, (i, dist, gate)


@pytest.mark.parametrize("s", STRENGTHS)
def test_denoise_against_the_restatement(net, packed, restated, s):
    audio, n, _ = packed
    got = _run(net, packed, s)
    for b, (d, gate) in enumerate(restated[s]):
        if b == ALONE:
            continue
        dist = float(np.abs(got[b, :n[b]] - d).max())
        print(f"strength {s} row {b} ({n[b]}): distance {dist:.2e} gate {gate:.2e}")
        assert dist <= gate, (s, b, dist, gate)
    assert np.array_equal(got[ALONE], audio[ALONE], equal_nan=True)         # the NaN-strength row: its own bits
    if s == 50.0:                                                           # (the large one zeroes most bins)
        x, beta = dr.fixture_rows()[7]
        ri = dr.analysis(x)
        m = np.sqrt(ri[:SPEC] ** 2 + ri[SPEC:] ** 2)
        assert np.mean(m <= s * beta[:, None]) > 0.9


def test_strength_zero_is_the_identity(net, packed, restated):
    audio, n, _ = packed
    got = _run(net, packed, 0.0)
    for b, (_, gate) in enumerate(restated[0.0]):
        dist = float(np.abs(got[b, :n[b]] - audio[b, :n[b]]).max())
        print(f"identity row {b} ({n[b]}): distance {dist:.2e} gate {gate:.2e}")
        assert dist <= gate, (b, dist, gate)


def test_the_ragged_contract(net, packed):
    audio, n, bias = packed
    eng, dev = net._engine, net.device
    B, L = audio.shape
    got = _run(net, packed, 1.0)
    # nothing behind n_b is written (the NaN put there is still there), the NaN-strength row is untouched
    for b in range(B):
        assert np.all(np.isnan(got[b, n[b]:])) and not np.any(np.isnan(got[b, :n[b]])), b
    assert np.array_equal(got[ALONE], audio[ALONE], equal_nan=True)
    # NaN behind the ends changes nothing: the same rows with zeros behind them
    clean = np.where(np.isnan(audio), np.float32(0), audio)
    again = to_np(eng.denoise(torch.from_numpy(clean).to(dev), n, bias, _strengths(1.0)))
    for b in range(B):
        assert np.array_equal(again[b, :n[b]], got[b, :n[b]]) and np.all(again[b, n[b]:] == 0), b
    # every row alone gives the batch's bits
    for b in range(B):
        if b == ALONE:
            continue
        one = to_np(eng.denoise(torch.from_numpy(audio[b:b + 1, :n[b]].copy()).to(dev), [n[b]], bias[b:b + 1], 1.0))
        assert np.array_equal(one[0], got[b, :n[b]]), b
    # ... and so does a row beside a much longer one (the sizes at which launch_conv would otherwise change its kernel)
    long_row = dr.voiced(103 * dr.HOP + 5, 99)
    two, n2 = dr.pack([audio[6, :n[6]], long_row])
    pair = to_np(eng.denoise(torch.from_numpy(two).to(dev), n2, np.stack([bias[6], bias[0]]), 1.0))
    assert dr.frames(n2[1]) == 103 and np.array_equal(pair[0, :n[6]], got[6, :n[6]])
    # out of place: the input keeps its bits, the output has the in-place bits in the rows and is not written elsewhere
    a = torch.from_numpy(audio.copy()).to(dev)
    o = torch.full((B, L + 3), 7.0, dtype=torch.float32, device=dev)
    assert eng.denoise(a, n, bias, _strengths(1.0), out=o) is o
    o = to_np(o)
    assert np.array_equal(to_np(a), audio, equal_nan=True)
    for b in range(B):
        if b == ALONE:
            assert np.all(o[b] == 7.0)
        else:
            assert np.array_equal(o[b, :n[b]], got[b, :n[b]]) and np.all(o[b, n[b]:] == 7.0), b


def test_the_generators_own_buzz_is_removed(net):
    """60 all-zero latent frames of one speaker, denoised at strength 1 with that speaker's bias.  Interior: back + 4 frames
    from either end (the STFT frames that see only the steady state end four frames further in than the generator's own
    transients).  There the restatement says what is left, and the library is held to it under the file's gate."""
    sid, frames = 17, 60
    eng = net._engine
    back, fwd = eng.generator_frame_dependence()
    g = torch.from_numpy(net._state["emb_g.weight"][[sid]]).to(net.device)
    z = torch.zeros((1, net.dims.inter_channels, frames), dtype=torch.float32, device=net.device)
    wave = eng.generator(z, g)[:, 0, :].contiguous()
    n = frames * dr.HOP
    x = to_np(wave)[0]
    beta = to_np(net.denoiser_bias([sid]))[0]
    got = to_np(net.denoise(wave.clone(), [n], [sid], strength=1.0))[0]
    lo, hi = (back + 4) * dr.HOP, n - (max(back, fwd) + 4) * dr.HOP
    assert hi - lo >= 16 * dr.HOP
    d, f = dr.denoise(x, beta, 1.0), dr.denoise(x, beta, 1.0, dtype=np.float32)
    gate = max(4.0 * float(np.abs(f.astype(np.float64) - d)[lo:hi].max()), dr.floor_of(x, n))
    dist = float(np.abs(got - d)[lo:hi].max())
    rms = float(np.sqrt(np.mean(x[lo:hi].astype(np.float64) ** 2)))
    res = float(np.sqrt(np.mean(got[lo:hi].astype(np.float64) ** 2)))
    print(f"buzz: input rms {rms:.3e} residual rms {res:.3e} ({res / rms:.2e} of it; restated "
          f"{np.sqrt(np.mean(d[lo:hi] ** 2)) / rms:.2e}) distance {dist:.2e} gate {gate:.2e}")
    assert rms > 0 and dist <= gate, (dist, gate)
    # the interior of the input IS periodic in a frame (what the bias rests on), and the residual is small beside it
    assert np.array_equal(x[lo:lo + dr.HOP], x[lo + dr.HOP:lo + 2 * dr.HOP])
    assert float(np.abs(got[lo:hi]).max()) <= float(np.abs(d[lo:hi]).max()) + gate


def test_batching_service_denoises_the_request_that_asks(net):
    from vispeech_amd.service import BatchingSynthesisService
    import isolated_ref as iso
    batch = iso.make_batch([11, 6], [4, 2], seed=2140)
    collate = lambda rows: {k: batch[k][rows] for k in ("phonemes", "lengths", "sid", "duration", "f0", "energy")}

    def serve(**kw):
        """(the float32 rows at the model's own rate are the pass-through: the waveform's bits)"""
        svc = BatchingSynthesisService(net, max_batch=2, max_wait_s=30.0, collate=collate)
        try:
            futs = [svc.submit(0, 11, output_encoding="f32", **kw), svc.submit(1, 12, output_encoding="f32")]
            return [f.result(120) for f in futs]
        finally:
            svc.close()

    plain = serve()
    got = serve(denoise=0.5)
    assert plain[1].tobytes() == got[1].tobytes()                            # the request that names none: its bytes
    n = plain[0].shape[0]
    assert n == 11 * dr.HOP and got[0].shape == (n,) and plain[1].shape == (6 * dr.HOP,)
    want = to_np(net.denoise(torch.from_numpy(plain[0].copy())[None, :].to(net.device), [n], [int(batch["sid"][0])], strength=0.5))[0]
    assert np.array_equal(got[0], want) and not np.array_equal(got[0], plain[0])
