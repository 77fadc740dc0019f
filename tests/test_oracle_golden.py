"""Pin the oracle: the CPU restatement must reproduce every stage boundary the real reference
produced for the golden cases (tests/golden/make_golden.py generated them from /root/reference)."""
import os

import numpy as np
import pytest
import torch

from oracle.vispeech_oracle import Oracle, rq_spline
from vispeech_amd.schema import ModelDims
from vispeech_amd.synth import synth_state_dict

CASES = ["ragged_controls", "ragged_predictors", "maxlen_dur3d", "c1_filelist", "evaluate_caller"]


@pytest.fixture(scope="module")
def oracle():
    dims = ModelDims()
    return Oracle(synth_state_dict(dims, seed=1234, infer_only=True), dims)


def run_oracle_on_case(oracle, g):
    use = g["in_use"]
    sc = g["in_scalar"]
    max_len = int(g["in_max_len"])
    return oracle.infer(
        g["in_phonemes"], g["in_lengths"], g["in_sid"], noise=g["in_noise"],
        noise_scale=float(g["in_noise_scale"]), max_len=None if max_len < 0 else max_len,
        duration_control=g["in_duration"] if use[0] else float(sc[0]),
        pitch_control=g["in_f0"] if use[1] else float(sc[1]),
        energy_control=g["in_energy"] if use[2] else float(sc[2]))


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


@pytest.mark.parametrize("case", CASES)
def test_oracle_matches_reference_outputs(oracle, golden_dir, case):
    g = np.load(os.path.join(golden_dir, f"{case}.npz"))
    out = run_oracle_on_case(oracle, g)
    # integer-valued / boolean outputs are exact
    np.testing.assert_array_equal(out["duration"].reshape(g["duration"].shape).numpy(), g["duration"])
    np.testing.assert_array_equal(out["x_mask"].numpy(), g["x_mask"])
    assert out["x_mask"].dtype == torch.bool
    # floating-point stage boundaries: <= 1e-5 relative to the tensor's max
    for name in ["x_enc", "x_frame", "h_frame", "m_p", "logs_p", "z_p", "z", "F0", "energy"]:
        e = rel_err(out[name].numpy(), g[name])
        assert e <= 1e-5, (case, name, e)
    # waveform: <= 1e-4 * max|ref|
    assert out["o"].shape == g["o"].shape
    assert rel_err(out["o"].numpy(), g["o"]) <= 1e-4, case


def test_spline_matches_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, "spline.npz"))
    for inv, yk, lk in ((False, "y_fwd", "lad_fwd"), (True, "y_inv", "lad_inv")):
        y, lad = rq_spline(g["x"], g["uw"], g["uh"], g["ud"], inverse=inv, tail_bound=5.0)
        assert np.abs(y.numpy() - g[yk]).max() <= 1e-5
        assert np.abs(lad.numpy() - g[lk]).max() <= 1e-4
    # round trip
    y, _ = rq_spline(g["x"], g["uw"], g["uh"], g["ud"], inverse=False)
    x2, _ = rq_spline(y, g["uw"], g["uh"], g["ud"], inverse=True)
    assert np.abs(x2.numpy() - g["x"]).max() <= 1e-3   # fp32 round trip (SURVEY: 3.6e-5 typical)


def test_oracle_voice_conversion_matches_reference(golden_dir):
    """SynthesizerTrn.voice_conversion (reference models.py:724-732): posterior encoder, flow forward
    with the source speaker, flow reverse with the target speaker, generator."""
    dims = ModelDims()
    orc = Oracle(synth_state_dict(dims, seed=1234), dims)          # full checkpoint: enc_q.* included
    g = np.load(os.path.join(golden_dir, "voice_conversion.npz"))
    out = orc.voice_conversion(g["in_y"], g["in_lengths"], g["in_sid_src"], g["in_sid_tgt"], g["in_noise"])
    np.testing.assert_array_equal(out["y_mask"].numpy(), g["y_mask"])
    for name in ["m_q", "logs_q", "z", "z_p", "z_hat"]:
        e = rel_err(out[name].numpy(), g[name])
        assert e <= 1e-5, (name, e)
    assert rel_err(out["o_hat"].numpy(), g["o_hat"]) <= 1e-4
    # same speaker on both sides: the two flow passes cancel (row 1 has sid_src == sid_tgt)
    assert np.abs(out["z_hat"][1].numpy() - out["z"][1].numpy()).max() <= 1e-4 * np.abs(g["z"][1]).max()


def test_oracle_spectrogram_matches_direct_dft():
    """oracle.spectrogram (torch.stft restatement of reference mel_processing.py:50-69) against a direct
    float64 DFT of the reflect-padded, Hann-windowed frames."""
    from oracle.vispeech_oracle import spectrogram
    r = np.random.Generator(np.random.PCG64(1))
    n_fft, hop, L = 64, 16, 16 * 9
    y = r.uniform(-1, 1, (2, L)).astype(np.float32)
    got = spectrogram(y, n_fft, hop).numpy()
    pad = (n_fft - hop) // 2
    yp = np.pad(y.astype(np.float64), ((0, 0), (pad, pad)), mode="reflect")
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / n_fft)
    T = 1 + (yp.shape[1] - n_fft) // hop
    assert got.shape == (2, n_fft // 2 + 1, T) and T == L // hop
    frames = np.stack([yp[:, t * hop:t * hop + n_fft] * win for t in range(T)], axis=2)      # [B, n_fft, T]
    X = np.fft.rfft(frames, axis=1)
    ref = np.sqrt(X.real ** 2 + X.imag ** 2 + 1e-6)
    assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max()


def test_oracle_mel_filterbank_properties():
    """Slaney mel filterbank restated from librosa's published algorithm: shape, non-negativity, triangles that
    cover the band with area normalisation (each filter integrates to ~1 Hz^-1 * Hz), monotone centre frequencies."""
    from oracle.vispeech_oracle import mel_filterbank, mel_spectrogram
    fb = mel_filterbank(44100, 2048, 80)
    assert fb.shape == (80, 1025) and fb.min() >= 0.0
    centres = fb.argmax(axis=1)
    assert np.all(np.diff(centres) > 0)
    df = 44100 / 2048
    area = fb.sum(axis=1) * df
    assert np.allclose(area[5:], 1.0, atol=0.05)           # slaney norm: unit area once a triangle spans several bins
    lin = fb[:10].argmax(axis=1) * df                        # below 1 kHz the centres are 200/3 Hz * k apart (+ grid rounding)
    assert np.all(np.abs(np.diff(lin) - np.diff(lin).mean()) <= df)
    y = np.sin(2 * np.pi * 440.0 * np.arange(8192) / 44100.0)[None, :].astype(np.float32) * 0.5
    m = mel_spectrogram(y, 44100, 2048, 512, 80).numpy()
    assert m.shape == (1, 80, 16) and np.isfinite(m).all()
    assert abs(int(m[0, :, 8].argmax()) - int(np.abs(fb[:, round(440.0 / df)]).argmax())) <= 1


MEL_CASES = [(44100, 2048, 80, 0.0, None), (22050, 1024, 80, 0.0, 8000.0), (22050, 2048, 128, 0.0, None), (16000, 400, 80, 20.0, 7600.0)]


@pytest.mark.parametrize("sr,n_fft,n_mels,fmin,fmax", MEL_CASES)
def test_mel_basis_is_pinned_to_a_third_party_implementation_of_librosa_s_algorithm(sr, n_fft, n_mels, fmin, fmax):
    """Round 5: the pin for the mel half (reference mel_processing.py:14, 78-79, 96-99:
    `librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax)` with its defaults = Slaney scale + Slaney norm).  librosa and
    torchaudio are not in the image, but `transformers` is: `transformers.audio_utils.mel_filter_bank(norm="slaney",
    mel_scale="slaney")` -- "adapted from torchaudio and librosa ... librosa uses the 'slaney' implementation" (its
    docstring), the basis behind HF's Whisper features -- is a third party's implementation of the same routine.  The
    oracle's restatement AND the library's host function (`vsp_mel_filterbank`, no GPU involved) agree with it to fp32
    rounding for the reference's configuration (44.1 kHz, n_fft 2048, 80 mels, 0 .. Nyquist: configs/config.json:27-33)
    and three other shapes."""
    from transformers.audio_utils import mel_filter_bank
    from oracle.vispeech_oracle import mel_filterbank
    from vispeech_amd.mel_processing import mel_filterbank as lib_filterbank
    ref = mel_filter_bank(num_frequency_bins=n_fft // 2 + 1, num_mel_filters=n_mels, min_frequency=float(fmin),
                          max_frequency=float(sr / 2 if fmax is None else fmax), sampling_rate=sr, norm="slaney",
                          mel_scale="slaney").T
    tol = 2e-7 * float(np.abs(ref).max()) + 1e-9
    assert np.abs(np.asarray(mel_filterbank(sr, n_fft, n_mels, fmin, fmax), dtype=np.float64) - ref).max() <= tol
    assert np.abs(np.asarray(lib_filterbank(sr, n_fft, n_mels, fmin, fmax), dtype=np.float64) - ref).max() <= tol


def test_philox_restatement_known_answers():
    """The oracle's restatement of the library's noise stream (vsp_randn) is pinned on the Random123 known-answer
    vectors of Philox4x32-10 (kat_vectors: counter / key all zero, all ones)."""
    from oracle.vispeech_oracle import philox4x32_10, philox_randn
    z = philox4x32_10(np.zeros((1, 4), np.uint32), 0, 0)[0]
    assert [int(x) for x in z] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = philox4x32_10(np.full((1, 4), 0xFFFFFFFF, np.uint32), 0xFFFFFFFF, 0xFFFFFFFF)[0]
    assert [int(x) for x in f] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    x = philox_randn(99, 200001)
    assert x.shape == (200001,) and abs(float(x.mean())) < 1e-2 and abs(float(x.std()) - 1) < 1e-2
    np.testing.assert_array_equal(x[:1000], philox_randn(99, 1000))      # a function of (seed, index) only
    np.testing.assert_array_equal(x[1003:1500], philox_randn(99, 497, first=1003))   # ... from any stream offset
    assert float(np.abs(x).max()) < 6.0                                   # uniforms strictly inside (0, 1): no inf


def test_spectrogram_restatement_is_pinned_to_torch_stft():
    """the reference's linear spectrogram (mel_processing.py:50-69) is torch.stft on a reflect-padded
    signal + sqrt(re^2 + im^2 + 1e-6).  Its call form (no ``return_complex``) is rejected by the installed torch, so no
    reference RUN can pin it; what can be pinned is the third-party routine it names: the oracle must equal
    (a) ``torch.stft(..., return_complex=True)`` post-processed exactly as the reference does on the real view
    (``.pow(2).sum(-1)``), argument for argument (mel_processing.py:63-66), and (b) an independent framing + numpy FFT of
    the same definition (periodic Hann window, center=False, one-sided).  The mel BASIS: librosa is absent; its pin is the
    transformers implementation of the same routine (test_mel_basis_is_pinned_to_a_third_party_implementation_... above)."""
    import torch.nn.functional as F
    from oracle.vispeech_oracle import spectrogram
    r = np.random.Generator(np.random.PCG64(5))
    for n_fft, hop, L in ((2048, 512, 2048 * 3 + 100), (1024, 256, 5000), (512, 128, 700)):
        y = (r.standard_normal((2, L)) * 0.3).astype(np.float32)
        got = spectrogram(y, n_fft, hop).numpy()
        yt = torch.from_numpy(y)
        pad = int((n_fft - hop) / 2)
        yp = F.pad(yt.unsqueeze(1), (pad, pad), mode="reflect").squeeze(1)
        st = torch.stft(yp, n_fft, hop_length=hop, win_length=n_fft, window=torch.hann_window(n_fft), center=False,
                        pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
        ref = torch.sqrt(torch.view_as_real(st).pow(2).sum(-1) + 1e-6).numpy()
        np.testing.assert_array_equal(got, ref)
        ypn = np.pad(y.astype(np.float64), ((0, 0), (pad, pad)), mode="reflect")
        n_frames = 1 + (ypn.shape[1] - n_fft) // hop
        win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)          # periodic Hann
        fr = np.stack([ypn[:, i * hop:i * hop + n_fft] * win for i in range(n_frames)], axis=2)   # [B, n_fft, frames]
        spec = np.fft.rfft(fr, axis=1)
        ind = np.sqrt(spec.real ** 2 + spec.imag ** 2 + 1e-6)
        assert got.shape == ind.shape == (2, n_fft // 2 + 1, n_frames)
        assert np.abs(got - ind).max() <= 2e-4 * ind.max()                        # fp32 FFT vs float64


def test_oracle_generator_resblock2_matches_reference_outputs(golden_dir):
    """The oracle's ResBlock2 branch (reference modules.py:245-249) against the real reference's waveform of
    tests/golden/resblock2.npz: the generator on the golden's z * x_mask with the same weights, within 1e-5 of peak."""
    from oracle.vispeech_oracle import generator
    from vispeech_amd import config as vcfg
    from vispeech_amd.schema import dims_from_ctor
    g = np.load(os.path.join(golden_dir, "resblock2.npz"))
    hp = vcfg.default_hparams()
    hp.model["resblock"] = "2"
    args, kwargs = vcfg.synthesizer_args(hp)
    dims = dims_from_ctor(*args, **kwargs)
    assert dims.resblock_kind == 2
    o = Oracle(synth_state_dict(dims, seed=int(g["weight_seed"])), dims, dtype=torch.float64)
    w = o.w
    gv = w["emb_g.weight"][torch.from_numpy(g["in_sid"])][:, :, None]
    z = torch.from_numpy(g["z"]).double() * torch.from_numpy(g["x_mask"]).double()
    with torch.no_grad():
        wave = generator(w, z, gv, dims)
    assert wave.shape == g["o"].shape
    assert rel_err(wave.numpy(), g["o"]) <= 1e-5
