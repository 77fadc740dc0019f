"""Conversion from audio on the GPU: the ragged spectrogram front end, ``SynthesizerTrn.convert_audio`` (caller's noise,
per-row seeds, ``noise_scale``) and conversion requests in the two batching services -- every row against the CPU oracle
run on that recording ALONE (``oracle.spectrogram`` of ``audio[b, :n_b]``, then ``Oracle.voice_conversion`` with B = 1).
The padded buffer holds NaN behind every recording's end: nothing there may reach an output."""
import numpy as np
import pytest
import torch

import isolated_ref as iso

pytestmark = pytest.mark.gpu

SPEC_TOL = 2e-5              # ragged spectrogram vs torch.stft: the bound of the existing front-end test
Z_TOL, WAVE_TOL = 5e-5, 2e-4  # spectrogram error riding on the stage error (test_wav_to_wav_voice_conversion)
TEXT_WAVE_TOL = 1e-4         # WAVE_TOL of tests/test_isolated_batch.py
HOP, N_FFT, UP = 512, 2048, 512

N_SPEC = [4708, 769, 2560, 300, 768, 1023, 1024]
T_SPEC = [9, 1, 5, 0, 0, 1, 2]
N_VC = [4708, 2560, 769, 300]
T_VC = [9, 5, 1, 0]
SRC, TGT = [5, 6, 40, 7], [20, 3, 2, 9]


def to_np(t):
    return t.detach().cpu().numpy()


def recordings(lengths, seed, stride=None):
    """Sine plus noise, clipped to [-1, 1] (the signal of the existing front-end test); NaN behind each row's end."""
    r = np.random.Generator(np.random.PCG64(seed))
    B, L = len(lengths), int(stride or max(lengths))
    t = np.arange(L) / 44100.0
    audio = (0.4 * np.sin(2 * np.pi * 220.0 * t)[None, :] * r.uniform(0.2, 1.0, (B, 1)) +
             0.1 * r.standard_normal((B, L))).astype(np.float32).clip(-1, 1)
    for b, n in enumerate(lengths):
        audio[b, n:] = np.nan
    return audio


@pytest.fixture(scope="module")
def dims():
    from vispeech_amd.schema import ModelDims
    return ModelDims()


@pytest.fixture(scope="module")
def weights(dims):
    from vispeech_amd.synth import synth_state_dict
    return synth_state_dict(dims, seed=1234)


@pytest.fixture(scope="module")
def net(weights):
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from vispeech_amd import config as vcfg
    from vispeech_amd.models import SynthesizerTrn
    args, kwargs = vcfg.synthesizer_args(vcfg.default_hparams())
    m = SynthesizerTrn(*args, **kwargs).eval()
    m.load_state_dict(weights, strict=True)
    return m


@pytest.fixture(scope="module")
def oracle(dims, weights):
    from oracle.vispeech_oracle import Oracle
    return Oracle(weights, dims)


@pytest.fixture(scope="module")
def vc_audio():
    return recordings(N_VC, seed=31)


@pytest.fixture(scope="module")
def vc_noise(dims):
    r = np.random.Generator(np.random.PCG64(32))
    return r.standard_normal((len(N_VC), dims.inter_channels, max(T_VC))).astype(np.float32)


@pytest.fixture(scope="module")
def vc_specs(vc_audio):
    """The oracle's spectrogram of every recording alone, computed once (None: no frame)."""
    from oracle.vispeech_oracle import spectrogram
    return [spectrogram(vc_audio[b:b + 1, :n], N_FFT, HOP).numpy() if T > 0 else None
            for b, (n, T) in enumerate(zip(N_VC, T_VC))]


def alone(oracle, spec, src, tgt, noise):
    """``Oracle.voice_conversion`` on one recording's spectrogram, B = 1, noise [inter, T]."""
    T = spec.shape[2]
    ref = oracle.voice_conversion(spec, np.array([T]), np.array([src]), np.array([tgt]), noise[None, :, :T])
    return {k: v[0].numpy() for k, v in ref.items()}


def row_err(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(float(np.abs(ref).max()), 1e-30))


def check_rows(result, refs, frames, tag):
    """Rows of a ``convert_audio`` result against the recordings' alone runs: the bounds of test 2 and exact zeros behind."""
    o_hat, y_mask, (z, z_p, z_hat) = (result[0], result[1], result[2])
    o_hat, y_mask, z, z_p, z_hat = (to_np(v) for v in (o_hat, y_mask, z, z_p, z_hat))
    assert o_hat.shape == (len(frames), 1, max(frames) * UP) and z.shape[2] == max(frames)
    for b, T in enumerate(frames):
        assert y_mask[b, 0].tolist() == [1.0] * T + [0.0] * (max(frames) - T)
        for name, v in (("z", z), ("z_p", z_p), ("z_hat", z_hat)):
            assert not v[b, :, T:].any(), (tag, b, name)
        assert not o_hat[b, 0, T * UP:].any(), (tag, b)
        if T == 0:
            continue
        errs = {name: row_err(v[b, :, :T], refs[b][name]) for name, v in (("z", z), ("z_p", z_p), ("z_hat", z_hat))}
        errs["o_hat"] = row_err(o_hat[b, :, : T * UP], refs[b]["o_hat"])
        print(f"{tag} row {b} (T = {T}): " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()))
        assert errs["z"] <= Z_TOL and errs["z_p"] <= Z_TOL and errs["z_hat"] <= Z_TOL, (tag, b, errs)
        assert errs["o_hat"] <= WAVE_TOL, (tag, b, errs)
    assert np.isfinite(o_hat).all()


# ---------------------------------------------------------------------------------------------- 1. ragged spectrogram
@pytest.mark.parametrize("lengths,want,stride", [(N_SPEC, T_SPEC, 4708), ([512 * 37], [37], None)])
def test_ragged_spectrogram(net, dims, lengths, want, stride):
    from oracle.vispeech_oracle import spectrogram
    eng = net._engine
    audio = recordings(lengths, seed=30, stride=stride)
    assert [eng.convert_frames(n) for n in lengths] == want
    spec, frames = eng.spectrogram_ragged(audio, lengths)
    spec, frames = to_np(spec), to_np(frames)
    assert spec.shape == (len(lengths), dims.spec_channels, max(want)) and frames.dtype == np.int64
    assert frames.tolist() == want
    assert np.isfinite(spec).all()
    for b, (n, T) in enumerate(zip(lengths, want)):
        assert not spec[b, :, T:].any(), b                     # exactly 0.0, not sqrt(1e-6)
        if T == 0:
            continue
        ref = spectrogram(audio[b:b + 1, :n], N_FFT, HOP).numpy()[0]
        assert ref.shape == (dims.spec_channels, T)
        err = float(np.abs(spec[b, :, :T] - ref).max())
        print(f"row {b} (n = {n}, T = {T}): err {err:.3e}, bound {SPEC_TOL * float(np.abs(ref).max()):.3e}")
        assert err <= SPEC_TOL * float(np.abs(ref).max()), (b, n, err)


def test_ragged_spectrogram_is_the_padded_one_where_the_rows_are_full(net):
    """Two rows of the full length: the ragged front end runs the DFT convolution of ``vsp_spectrogram`` on the same
    operand -- the same bits."""
    eng = net._engine
    audio = recordings([512 * 11, 512 * 11], seed=33)
    spec, frames = eng.spectrogram_ragged(audio, [512 * 11] * 2)
    assert frames.tolist() == [11, 11]
    assert torch.equal(spec, eng.spectrogram(audio))


# ---------------------------------------------------------------------------------------------- 2. caller's noise
@pytest.fixture(scope="module")
def vc_refs(oracle, vc_specs, vc_noise):
    return [alone(oracle, s, SRC[b], TGT[b], vc_noise[b]) if s is not None else None for b, s in enumerate(vc_specs)]


def test_convert_audio_with_the_callers_noise(net, vc_audio, vc_noise, vc_refs):
    noise = vc_noise.copy()
    for b, T in enumerate(T_VC):
        noise[b, :, T:] = np.nan                                 # row b uses noise[b][:, :T_b] only
    res = net.convert_audio(vc_audio, N_VC, SRC, TGT, noise=noise)
    check_rows(res, vc_refs, T_VC, "noise")
    assert not to_np(res[0])[3].any()                            # the 300-sample recording: all zero


# ---------------------------------------------------------------------------------------------- 3. seeds
SEEDS = [11, 2 ** 40 + 5, 12, 13]


def seeded_noise(eng, seeds, frames, inter):
    N = torch.zeros((len(seeds), inter, max(frames)), dtype=torch.float32, device=eng.device)
    for b, (s, T) in enumerate(zip(seeds, frames)):
        if T > 0:
            N[b, :, :T] = eng.randn(s, inter, T)
    return N


def test_seeds_draw_what_randn_draws(net, dims, vc_audio):
    N = seeded_noise(net._engine, SEEDS, T_VC, dims.inter_channels)
    a = net.convert_audio(vc_audio, N_VC, SRC, TGT, noise_seed=SEEDS)
    b = net.convert_audio(vc_audio, N_VC, SRC, TGT, noise=N)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for x, y in zip(a[2], b[2]):
        assert torch.equal(x, y)


def test_seeds_move_with_their_recordings(net, oracle, dims, vc_audio, vc_specs):
    order = [2, 3, 0, 1]
    N = to_np(seeded_noise(net._engine, SEEDS, T_VC, dims.inter_channels))
    refs = [alone(oracle, vc_specs[i], SRC[i], TGT[i], N[i]) if vc_specs[i] is not None else None for i in order]
    pick = lambda v: [v[i] for i in order]
    res = net.convert_audio(vc_audio[order], pick(N_VC), pick(SRC), pick(TGT), noise_seed=pick(SEEDS))
    check_rows(res, refs, pick(T_VC), "moved")


def test_drawing_needs_seeds(net, vc_audio):
    from vispeech_amd._lib import VspError
    with pytest.raises(VspError, match="VSP_ERR_STATE"):
        net.convert_audio(vc_audio, N_VC, SRC, TGT)              # no noise, no seeds: the library's own check
    with pytest.raises(ValueError):
        net.convert_audio(vc_audio, N_VC, SRC, TGT, noise_seed=7)
    with pytest.raises(ValueError):
        net.convert_audio(vc_audio, N_VC, SRC, TGT, noise_seed=[1, 2])


# ---------------------------------------------------------------------------------------------- 4. noise_scale
def test_noise_scale_zero_needs_no_noise(net, oracle, vc_audio, vc_specs, vc_noise):
    zero = np.zeros_like(vc_noise)
    refs = [alone(oracle, s, SRC[b], TGT[b], zero[b]) if s is not None else None for b, s in enumerate(vc_specs)]
    net._engine.set_noise_seeds(None)
    res = net.convert_audio(vc_audio, N_VC, SRC, TGT, noise_scale=0.0)
    check_rows(res, refs, T_VC, "scale 0")
    nan = np.full_like(vc_noise, np.nan)                         # ... and a given tensor is not read
    res2 = net.convert_audio(vc_audio, N_VC, SRC, TGT, noise=nan, noise_scale=0.0)
    assert torch.equal(res[0], res2[0]) and torch.equal(res[2][0], res2[2][0])


def test_noise_scale_half(net, oracle, vc_audio, vc_specs, vc_noise):
    refs = [alone(oracle, s, SRC[b], TGT[b], 0.5 * vc_noise[b]) if s is not None else None for b, s in enumerate(vc_specs)]
    check_rows(net.convert_audio(vc_audio, N_VC, SRC, TGT, noise=vc_noise, noise_scale=0.5), refs, T_VC, "scale 0.5")


# ---------------------------------------------------------------------------------------------- 5. / 6. services
TEXT_FRAMES, TEXT_PHONEMES, TEXT_SEEDS = [6, 11], [2, 4], [101, 102]
CONV = [0, 1]                # the 9- and the 5-frame recording of the fixtures above
CONV_SEEDS = [201, 202]


@pytest.fixture(scope="module")
def text_batch():
    return iso.make_batch(TEXT_FRAMES, TEXT_PHONEMES, seed=2140)


def collate_of(batch):
    return lambda rows: {k: batch[k][rows] for k in ("phonemes", "lengths", "sid", "duration", "f0", "energy")}


@pytest.fixture(scope="module")
def service_refs(net, oracle, dims, text_batch, vc_specs):
    """The oracle's waveform of every request alone, with the noise the library draws for its seed."""
    eng, inter = net._engine, dims.inter_channels
    text = []
    for b, (L, s) in enumerate(zip(TEXT_FRAMES, TEXT_SEEDS)):
        nz = np.zeros_like(text_batch["noise"])
        nz[b, :, :L] = to_np(eng.randn(s, inter, L))
        ref, _, L_ref = iso.alone(oracle, text_batch, b, "controls", noise=nz)
        assert L_ref == L
        text.append(ref["o"][0, 0])
    conv = [alone(oracle, vc_specs[i], SRC[i], TGT[i], to_np(eng.randn(s, inter, T_VC[i])))["o_hat"][0]
            for i, s in zip(CONV, CONV_SEEDS)]
    return text, conv


def check_pcm(got, ref, tol, tag):
    """PCM16 within ceil(tol * max|ref| * 32767) + 1 of rint(ref * 32767): the float bound in steps, plus the quantiser's own."""
    got = np.frombuffer(got, dtype="<i2") if isinstance(got, (bytes, bytearray)) else np.asarray(got)
    want = np.rint(np.asarray(ref, np.float64) * 32767.0)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    allowed = int(np.ceil(tol * float(np.abs(ref).max()) * 32767.0)) + 1
    worst = int(np.abs(got.astype(np.int64) - want).max())
    print(f"{tag}: worst {worst} PCM16 steps, allowed {allowed}")
    assert worst <= allowed, (tag, worst, allowed)


def submit_mixed(svc, vc_audio):
    """text 0, conversion 0, text 1, conversion 1 -- in that order."""
    out = []
    for k in range(2):
        out.append(svc.submit(k, TEXT_SEEDS[k]))
        i = CONV[k]
        out.append(svc.submit_conversion(vc_audio[i, :N_VC[i]], SRC[i], TGT[i], CONV_SEEDS[k]))
    return out


def test_batching_service_mixed(net, text_batch, vc_audio, service_refs):
    from vispeech_amd.service import BatchingSynthesisService
    text_ref, conv_ref = service_refs
    svc = BatchingSynthesisService(net, max_batch=4, max_wait_s=30.0, collate=collate_of(text_batch))
    try:
        got = [f.result(120) for f in submit_mixed(svc, vc_audio)]
    finally:
        svc.close()
    for k in range(2):
        assert got[2 * k].size == TEXT_FRAMES[k] * UP and got[2 * k + 1].size == T_VC[CONV[k]] * UP
        check_pcm(got[2 * k], text_ref[k], TEXT_WAVE_TOL, f"text {k}")
        check_pcm(got[2 * k + 1], conv_ref[k], WAVE_TOL, f"conversion {k}")


def test_batching_service_mixed_at_an_output_rate(net, dims, text_batch, vc_audio):
    """``output_rate``: every request's bytes are ``Engine.output`` of its float row of the same mixed batch (the latents
    of the text rows and of the conversions, packed, through one ``generator_ragged`` call)."""
    from vispeech_amd.service import BatchingSynthesisService, _host_i16
    eng = net._engine
    svc = BatchingSynthesisService(net, max_batch=4, max_wait_s=30.0, collate=collate_of(text_batch), output_rate=22050)
    try:
        got = [f.result(120) for f in submit_mixed(svc, vc_audio)]
    finally:
        svc.close()
    t = lambda a: torch.as_tensor(np.asarray(a))
    enc = eng.encode(t(text_batch["phonemes"]), t(text_batch["lengths"]), t(text_batch["sid"]), t(text_batch["duration"]),
                     t(text_batch["f0"]), t(text_batch["energy"]), isolated=True)
    frames, tf = eng.frame_lengths_host(enc["frame_lengths"])
    assert [int(x) for x in frames] == TEXT_FRAMES and tf == max(TEXT_FRAMES)
    z_text = eng.decode(enc, tf, None, 0.667, max_len=0, noise_seed=TEXT_SEEDS, isolated=True)["z"]
    n = [N_VC[i] for i in CONV]
    lat = eng.convert_latent(np.nan_to_num(vc_audio[CONV]), n, [SRC[i] for i in CONV], [TGT[i] for i in CONV],
                             noise_seed=CONV_SEEDS)
    lengths = [TEXT_FRAMES[0], T_VC[CONV[0]], TEXT_FRAMES[1], T_VC[CONV[1]]]
    Z = torch.zeros((4, dims.inter_channels, max(lengths)), dtype=torch.float32, device=eng.device)
    for b, (src, k) in enumerate(((z_text, 0), (lat["z_hat"], 0), (z_text, 1), (lat["z_hat"], 1))):
        Z[b, :, : lengths[b]] = src[k, :, : lengths[b]]
    G = torch.stack([enc["g"][0].reshape(-1), lat["g"][0], enc["g"][1].reshape(-1), lat["g"][1]])
    o = eng.generator_ragged(Z, G, lengths)
    for b, L in enumerate(lengths):
        want = _host_i16(eng.output(o[b:b + 1, 0, : L * UP], pcm=True)[0])
        assert want.size == -(-L * UP // 2) and np.array_equal(got[b], want), b


def run_streaming(net, text_batch, vc_audio, **kw):
    from vispeech_amd.service import StreamingBatchService
    svc = StreamingBatchService(net, chunk_frames=4, first_chunk_frames=2, collate=collate_of(text_batch), autostart=False,
                                **kw)
    streams = [svc.submit(0, TEXT_SEEDS[0])] + [
        svc.submit_conversion(vc_audio[i, :N_VC[i]], SRC[i], TGT[i], s) for i, s in zip(CONV, CONV_SEEDS)]
    while svc.step():
        pass
    return svc, [list(s) for s in streams]


def test_streaming_service_mixed(net, text_batch, vc_audio, service_refs):
    text_ref, conv_ref = service_refs
    svc, pieces = run_streaming(net, text_batch, vc_audio)
    assert svc.stats == {"ticks": 3, "rows_per_tick": [3, 3, 1], "groups": 1}            # 6, 9 and 5 frames: shared ticks
    bytes_of = lambda frames: [2 * UP * f for f in frames]
    assert [len(p) for p in pieces[0]] == bytes_of([2, 4])
    assert [len(p) for p in pieces[1]] == bytes_of([2, 4, 3]) and [len(p) for p in pieces[2]] == bytes_of([2, 3])
    check_pcm(b"".join(pieces[0]), text_ref[0], TEXT_WAVE_TOL, "text 0")
    for k in range(2):
        check_pcm(b"".join(pieces[1 + k]), conv_ref[k], WAVE_TOL, f"conversion {k}")


def test_streaming_service_mixed_fused_output(net, text_batch, vc_audio):
    plain, a = run_streaming(net, text_batch, vc_audio, output_rate=22050)
    fused, b = run_streaming(net, text_batch, vc_audio, output_rate=22050, fused_output=True)
    assert plain.stats["rows_per_tick"] == fused.stats["rows_per_tick"] == [3, 3, 1]
    for k, (x, y) in enumerate(zip(a, b)):
        assert b"".join(x) == b"".join(y) and len(b"".join(y)) == 2 * (-(-[6, 9, 5][k] * UP // 2)), k
