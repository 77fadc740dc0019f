"""The denoiser and the inverse STFT on the in-LDS FFT (``transform="fft"``) against the fp64
restatement of tests/denoiser_ref.py -- the specification is the product path's: an FFT computes the same sums -- under the
gate of tests/denoiser_fft_ref.py.  The file mirrors tests/test_denoiser_gpu.py: the same ragged batch of eight rows
(``denoiser_ref.LENGTHS``: 1, 1, 2, 15, 9, 16, 17 and 40 frames, partial and full tiles of 4, 8 and 16 frames) with the
NaN-strength row in its middle and NaN behind every row's end.

The gate of a row is max(4 x |float32 FFT restatement - fp64|, floor), floor = sqrt(4 log2 N + 8) 2^-24 P / min W (52
roundings as a random walk: tests/denoiser_fft_ref.py), several times tighter than the product path's gate: twiddles that
are off by 1e-6 pass that one and fail this one.

Measured on the MI355X (profiles/r27_denoiser_fft.txt), the library's largest distance from fp64 per row at strength 0 / 1 /
50: 7.1e-8 / 4.9e-8 / 3.4e-8 (769), 2.2e-7 / 1.2e-7 / 9.1e-8 (1023), 7.5e-8 / 8.0e-8 / 8.0e-9 (1024), 1.9e-7 / 1.4e-7 / 2.2e-8
(8191), 8.9e-8 / 8.2e-8 / 2.4e-8 (8192), 8.9e-8 / 8.8e-8 / 2.4e-8 (9004), 1.2e-7 / 1.0e-7 / 1.5e-8 (20557), under gates of 1.5e-7 ..
7.1e-6: at most 0.3 of the gate.

The switch test runs ``dft``, ``fft``, ``dft`` on one engine: the two ``dft`` outputs are bit-equal (the switch leaves
nothing behind), the ``fft`` output differs from them in bits and lies within the sum of the two paths' gates."""
import numpy as np
import pytest
import torch

import denoiser_fft_ref as fr
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
def restated():
    """Per strength and row: (fp64 output, float32 FFT output, gate), computed once."""
    return fr.restated(STRENGTHS)


def _strengths(s):
    return [float("nan") if b == ALONE else s for b in range(len(dr.LENGTHS))]


def _run(net, packed, s, transform="fft", **kw):
    audio, n, bias = packed
    return to_np(net._engine.denoise(torch.from_numpy(audio.copy()).to(net.device), n, bias, _strengths(s), transform=transform, **kw))


def test_istft_alone(net, rows, packed):
    """RI from the restatement's float32 FFT analysis, subtracted at strength 1, NaN in the columns behind every row's
    frames and garbage in the imaginary parts of bins 0 and N / 2 (the specification's real part drops them); the output
    against the fp64 synthesis of the same float32 RI."""
    _, n, _ = packed
    T_max = max(dr.frames(v) for v in n)
    ri = np.full((len(rows), 2 * SPEC, T_max), np.nan, np.float32)
    for b, (x, beta) in enumerate(rows):
        ri[b, :, :dr.frames(len(x))] = dr.subtract(fr.analysis(x), beta, 1.0, np.float32)
    clean = ri.copy()
    clean[:, SPEC] = 0                                              # (the fp64 side: those two rows as the specification reads them)
    clean[:, 2 * SPEC - 1] = 0
    ri[:, SPEC, :] = np.where(np.isnan(ri[:, SPEC, :]), np.nan, np.float32(3.0))
    ri[:, 2 * SPEC - 1, :] = np.where(np.isnan(ri[:, 2 * SPEC - 1, :]), np.nan, np.float32(-2.0))
    got = to_np(net._engine.istft(ri, n, transform="fft"))
    assert got.shape == (len(rows), max(n))
    for b, (x, _) in enumerate(rows):
        r = clean[b, :, :dr.frames(n[b])]
        d, f = dr.synthesis(r.astype(np.float64), n[b]), fr.synthesis(r, n[b])
        gate = fr.gate_of(f, d, fr.floor_of(x, n[b]))
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
    """The library's own steady periods; the floor with the result's size in the place of P: sqrt(52) 2^-24 max(beta).  Nine
    speakers: a full tile of 8 columns and one more."""
    sids = [3, 17, 199, 0, 5, 42, 77, 100, 150]
    period, g = _steady_periods(net, sids)
    got = to_np(net._engine.denoise_bias_of(period, transform="fft"))
    assert got.shape == (len(sids), SPEC) and np.all(got >= 0)
    assert np.array_equal(got, to_np(net._engine.denoise_bias(g, transform="fft")))    # the engine's own way to the same rows
    assert np.array_equal(got[:3], to_np(net.denoiser_bias(sids[:3], "fft")))           # ... and the model's table, by transform
    assert np.array_equal(got[[2, 0]], to_np(net.denoiser_bias([199, 3], transform="fft")))
    plain = to_np(net.denoiser_bias(sids[:3]))
    assert not np.array_equal(plain, got[:3]) and np.array_equal(plain, to_np(net._engine.denoise_bias_of(period[:3])))
    for i, c in enumerate(to_np(period)):
        d, f = dr.bias_of(c), fr.bias_of(c)
        gate = fr.gate_of(f, d, float(np.sqrt(fr.ROUNDINGS) * dr.U32 * d.max()))
        dist = float(np.abs(got[i] - d).max())
        print(f"bias speaker {sids[i]}: max {d.max():.3e} distance {dist:.2e} gate {gate:.2e}")
        assert d.max() > 0 and dist <= gate, (i, dist, gate)


@pytest.mark.parametrize("s", STRENGTHS)
def test_denoise_against_the_restatement(net, packed, restated, s):
    audio, n, _ = packed
    got = _run(net, packed, s)
    for b, (d, _, gate) in enumerate(restated[s]):
        if b == ALONE:
            continue
        dist = float(np.abs(got[b, :n[b]] - d).max())
        print(f"strength {s} row {b} ({n[b]}): distance {dist:.2e} gate {gate:.2e}")
        assert dist <= gate, (s, b, dist, gate)
    assert np.array_equal(got[ALONE], audio[ALONE], equal_nan=True)         # the NaN-strength row: its own bits


def test_strength_zero_is_the_identity(net, packed, restated):
    audio, n, _ = packed
    got = _run(net, packed, 0.0)
    for b, (_, _, gate) in enumerate(restated[0.0]):
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
    again = to_np(eng.denoise(torch.from_numpy(clean).to(dev), n, bias, _strengths(1.0), transform="fft"))
    for b in range(B):
        assert np.array_equal(again[b, :n[b]], got[b, :n[b]]) and np.all(again[b, n[b]:] == 0), b
    # every row alone gives the batch's bits
    for b in range(B):
        if b == ALONE:
            continue
        one = to_np(eng.denoise(torch.from_numpy(audio[b:b + 1, :n[b]].copy()).to(dev), [n[b]], bias[b:b + 1], 1.0, transform="fft"))
        assert np.array_equal(one[0], got[b, :n[b]]), b
    # ... and so does a row beside a much longer one
    long_row = dr.voiced(103 * dr.HOP + 5, 99)
    two, n2 = dr.pack([audio[6, :n[6]], long_row])
    pair = to_np(eng.denoise(torch.from_numpy(two).to(dev), n2, np.stack([bias[6], bias[0]]), 1.0, transform="fft"))
    assert dr.frames(n2[1]) == 103 and np.array_equal(pair[0, :n[6]], got[6, :n[6]])
    # out of place: the input keeps its bits, the output has the in-place bits in the rows and is not written elsewhere
    a = torch.from_numpy(audio.copy()).to(dev)
    o = torch.full((B, L + 3), 7.0, dtype=torch.float32, device=dev)
    assert eng.denoise(a, n, bias, _strengths(1.0), out=o, transform="fft") is o
    o = to_np(o)
    assert np.array_equal(to_np(a), audio, equal_nan=True)
    for b in range(B):
        if b == ALONE:
            assert np.all(o[b] == 7.0)
        else:
            assert np.array_equal(o[b, :n[b]], got[b, :n[b]]) and np.all(o[b, n[b]:] == 7.0), b


def test_the_switch_does_what_it_says_and_nothing_else(net, packed, restated):
    audio, n, _ = packed
    eng = net._engine
    first = _run(net, packed, 1.0, transform="dft")
    assert eng.lib.vsp_stft_transform(eng.ctx) == 0
    fft = _run(net, packed, 1.0, transform="fft")
    assert eng.lib.vsp_stft_transform(eng.ctx) == 1
    again = _run(net, packed, 1.0, transform="dft")
    default = to_np(eng.denoise(torch.from_numpy(audio.copy()).to(net.device), n, packed[2], _strengths(1.0)))      # no keyword at all
    assert eng.lib.vsp_stft_transform(eng.ctx) == 0
    assert np.array_equal(first, again, equal_nan=True) and np.array_equal(first, default, equal_nan=True)
    rows = dr.fixture_rows()
    for b, (d, _, gate) in enumerate(restated[1.0]):
        if b == ALONE:
            assert np.array_equal(fft[b], first[b], equal_nan=True)
            continue
        x, beta = rows[b]
        dft_gate = max(4.0 * float(np.abs(dr.denoise(x, beta, 1.0, dtype=np.float32).astype(np.float64) - d).max()), dr.floor_of(x, n[b]))
        dist = float(np.abs(fft[b, :n[b]].astype(np.float64) - first[b, :n[b]]).max())
        print(f"row {b} ({n[b]}): fft - dft {dist:.2e}, gates {gate:.2e} + {dft_gate:.2e}")
        assert not np.array_equal(fft[b, :n[b]], first[b, :n[b]]), b          # other bits ...
        assert dist <= gate + dft_gate, (b, dist, gate, dft_gate)            # ... of the same sums
    # the workspace the FFT call was sized with is the smaller one
    eng._set_transform("fft", "test")
    small = int(eng.lib.vsp_denoise_workspace_bytes(eng.ctx, len(n), max(n)))
    eng._set_transform("dft", "test")
    assert 0 < small < int(eng.lib.vsp_denoise_workspace_bytes(eng.ctx, len(n), max(n)))


def test_the_model_passes_the_transform_through(net):
    """``SynthesizerTrn.denoise(transform="fft")``: the FFT call with the FFT's bias of the speaker."""
    x = dr.voiced(9 * dr.HOP + 31, 78)
    xd = torch.from_numpy(x).to(net.device)
    got = to_np(net.denoise(xd.clone()[None, :], [len(x)], [17], strength=0.3, transform="fft"))[0]
    want = to_np(net._engine.denoise(xd.clone()[None, :], [len(x)], net.denoiser_bias([17], "fft"), 0.3, transform="fft"))[0]
    plain = to_np(net.denoise(xd.clone()[None, :], [len(x)], [17], strength=0.3))[0]
    assert np.array_equal(got, want) and not np.array_equal(got, plain)
    assert net._engine.status() == 0
