"""Live voice conversion on the GPU: windows of recordings that are still arriving (``Engine.convert_stream_rows``) and
whole live sessions of ``StreamingBatchService`` -- every frame and every byte against the CPU oracle run on the WHOLE
recording alone (``oracle.spectrogram`` of it, then ``Oracle.voice_conversion`` with B = 1), with the frame-major noise
``randn(seed, T, inter).T``.  The small configuration of ``live_convert_ref`` unless said; the device buffers hold NaN
outside the samples a window may read."""
import numpy as np
import pytest
import torch

import isolated_ref as iso
import live_convert_ref as ref
import output_stage_ref as osr
from live_convert_ref import HOP, H_SMALL, N_FFT, PAD, UP
from test_convert_gpu import TEXT_WAVE_TOL, WAVE_TOL, Z_TOL, check_pcm

pytestmark = pytest.mark.gpu

SRC, TGT, SEED = 5, 9, 2 ** 40 + 77
N100 = 100 * HOP + 77                 # 100 frames
N5, N0, N20 = 5 * HOP + 200, 100, 20 * HOP          # 5 frames; no frame; 20 frames, the end exactly on a frame boundary
N9 = 9 * HOP + 50


def to_np(t):
    return t.detach().cpu().numpy()


class Net:
    """What the services need of a model: the engine and its dimensions."""

    def __init__(self, eng, dims):
        self._engine, self.dims = eng, dims


@pytest.fixture(scope="module")
def dims():
    return ref.small_dims()


@pytest.fixture(scope="module")
def weights(dims):
    return ref.small_weights(dims)


@pytest.fixture(scope="module")
def eng(dims, weights):
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from vispeech_amd.engine import Engine
    e = Engine(dims)
    e.set_weights(weights, strict=True)
    e.finalize()
    assert e.convert_halo == H_SMALL and e.generator_halo >= 1
    return e


@pytest.fixture(scope="module")
def oracle(dims, weights):
    from oracle.vispeech_oracle import Oracle
    return Oracle(weights, dims)


def z_hat_alone(oracle, audio, n_fft, hop, src, tgt, noise):
    """z_hat of ``Oracle.voice_conversion`` for one whole recording (its stages up to z_hat; the generator is not run)."""
    from oracle import vispeech_oracle as vo
    with torch.no_grad():
        spec = vo.spectrogram(audio[None], n_fft, hop)
        w, d = oracle.w, oracle.dims
        g_src, g_tgt = (w["emb_g.weight"][torch.tensor([s])][:, :, None] for s in (src, tgt))
        m = torch.ones((1, 1, spec.shape[2]))
        z, _, _ = vo.posterior_encoder(w, spec, m, g_src, torch.as_tensor(noise)[None], d)
        return vo.flow_reverse(w, vo.flow_forward(w, z, m, g_src, d), m, g_tgt, d)[0].numpy()


def wave_alone(oracle, audio, src, tgt, noise):
    """The oracle's waveform of one whole recording, B = 1, noise [inter, T]."""
    from oracle.vispeech_oracle import spectrogram
    spec = spectrogram(audio[None], N_FFT, HOP).numpy()
    T = spec.shape[2]
    assert noise.shape[1] == T
    return oracle.voice_conversion(spec, np.array([T]), np.array([src]), np.array([tgt]), noise[None])["o_hat"][0, 0].numpy()


def live_noise(eng, seed, T, inter):
    """The noise a live conversion draws for a recording of T frames: element t * inter + c of the seed's stream."""
    return to_np(eng.randn(seed, T, inter)).T.copy()


@pytest.fixture(scope="module")
def rec100():
    return ref.recording(N100, seed=41)


@pytest.fixture(scope="module")
def z100(eng, oracle, dims, rec100):
    assert eng.convert_frames(N100) == ref.frames_of(N100) == 100
    return z_hat_alone(oracle, rec100, N_FFT, HOP, SRC, TGT, live_noise(eng, SEED, 100, dims.inter_channels))


def row_of(eng, audio, n_known, closed, e0, e1, first=None, seed=SEED, scale=1.0, slack=(5, 7)):
    """A row of ``convert_stream_rows`` whose device buffer holds the recording's samples inside the window's
    [s_lo, s_hi) and NaN everywhere else; it starts ``slack[0]`` samples before s_lo unless ``first`` says where."""
    ready, w0, w1, lo, hi = eng.convert_window_plan(n_known, closed, e0, e1)
    assert ready
    first = max(0, lo - slack[0]) if first is None else first
    buf = np.full(n_known - first + slack[1], np.nan, np.float32)
    buf[lo - first:hi - first] = audio[lo:hi]
    return (torch.from_numpy(buf).to(eng.device), first, n_known, closed, e0, e1, SRC, TGT, seed, scale), (w0, w1, lo, hi)


def frame_err(got, want, scale):
    return float(np.abs(np.asarray(got, np.float64) - want).max() / scale)


# ---------------------------------------------------------------------------------------------- 4. one call, three windows
def test_three_windows_of_one_recording(eng, dims, weights, rec100, z100):
    span = 8
    open_at = lambda e1: (e1 + H_SMALL - 1) * HOP - PAD + N_FFT       # the samples an open window ending at e1 needs
    specs = [(open_at(6), False, 0, 6, 0),                            # the first window: w0 = 0, open
             (open_at(48), False, 40, 48, None),                      # interior: both ends artificial
             (N100, True, 93, 100, None)]                             # the last window: closed, w1 = T
    rows, plans = zip(*(row_of(eng, rec100, n, c, e0, e1, first=f) for n, c, e0, e1, f in specs))
    assert plans[0][:2] == (0, 6 + H_SMALL) and plans[1][:2] == (40 - H_SMALL, 48 + H_SMALL) and plans[2][:2] == (93 - H_SMALL, 100)
    assert plans[1][2] > 0 and plans[2][3] == N100 and rows[1][1] == plans[1][2] - 5
    z, g = eng.convert_stream_rows(rows, span)
    z, g = to_np(z), to_np(g)
    assert z.shape == (3, dims.inter_channels, span) and np.isfinite(z).all()
    assert np.array_equal(g, np.repeat(np.asarray(weights["emb_g.weight"], np.float32)[TGT][None], 3, 0))
    scale = float(np.abs(z100).max())
    for b, (_, _, e0, e1, _) in enumerate(specs):
        err = frame_err(z[b, :, : e1 - e0], z100[:, e0:e1], scale)
        print(f"row {b} frames [{e0}, {e1}): err {err:.2e}, bound {Z_TOL:.0e}")
        assert err <= Z_TOL, (b, err)
        assert not z[b, :, e1 - e0:].any(), b                         # exactly 0.0 behind the delivered frames


def test_noise_scale_zero_draws_nothing_and_rows_keep_their_own(eng, oracle, dims, rec100, z100):
    """Rows of one call with different noise scales: each is its own recording's z_hat (scale 0: z = m_q)."""
    zero = z_hat_alone(oracle, rec100, N_FFT, HOP, SRC, TGT, np.zeros((dims.inter_channels, 100), np.float32))
    rows = [row_of(eng, rec100, N100, True, 30, 38, scale=s)[0] for s in (0.0, 1.0)]
    z, _ = eng.convert_stream_rows(rows, 8)
    both, _ = eng.convert_stream_rows(rows[:1], 8)
    z, both = to_np(z), to_np(both)
    assert frame_err(z[0], zero[:, 30:38], float(np.abs(zero).max())) <= Z_TOL
    assert frame_err(z[1], z100[:, 30:38], float(np.abs(z100).max())) <= Z_TOL
    assert frame_err(both[0], zero[:, 30:38], float(np.abs(zero).max())) <= Z_TOL      # no row draws: no noise launch


# ---------------------------------------------------------------------------------------------- 5. open == closed
def test_a_frame_delivered_early_does_not_change(eng, rec100, z100):
    n_open = (76 + H_SMALL - 1) * HOP - PAD + N_FFT
    assert n_open < N100
    early, pa = row_of(eng, rec100, n_open, False, 70, 76)
    late, pb = row_of(eng, rec100, N100, True, 72, 80)
    assert pa[:2] == (70 - H_SMALL, 76 + H_SMALL) and pb[:2] == (72 - H_SMALL, 100)     # two different windows
    a = to_np(eng.convert_stream_rows([early], 8)[0])[0]
    b = to_np(eng.convert_stream_rows([late], 8)[0])[0]
    err = frame_err(a[:, 2:6], b[:, 0:4], float(np.abs(z100).max()))
    print(f"frames [72, 76) open vs closed: {err:.2e}, bound {2 * Z_TOL:.0e}")
    assert err <= 2 * Z_TOL


# ---------------------------------------------------------------------------------------------- 6. whole sessions
def drive(svc, sessions, pieces=(1, 255, 4097)):
    """Feeds every recording piece by piece -- a step after each piece --, ends it, and runs the service dry."""
    at = [0] * len(sessions)
    k = 0
    while any(a < len(x) for a, (_, x) in zip(at, sessions)):
        size = pieces[k % len(pieces)]
        k += 1
        for i, (s, x) in enumerate(sessions):
            if at[i] < len(x):
                s.feed(x[at[i]:at[i] + size])
                at[i] += size
                if at[i] >= len(x):
                    s.end()
        svc.step()
    for s, x in sessions:
        s.end()
    while svc.step():
        pass
    return [b"".join(s) for s, _ in sessions]


@pytest.fixture(scope="module")
def recs(rec100):
    return {N100: rec100, N5: ref.recording(N5, seed=42), N0: ref.recording(N0, seed=43), N20: ref.recording(N20, seed=44),
            N9: ref.recording(N9, seed=45)}


@pytest.fixture(scope="module")
def quiet_waves(oracle, dims, recs):
    """The oracle's waveform of every recording with noise_scale 0 (z = m_q)."""
    return {n: wave_alone(oracle, x, SRC, TGT, np.zeros((dims.inter_channels, ref.frames_of(n)), np.float32))
            for n, x in recs.items() if ref.frames_of(n) > 0}


def test_whole_sessions_fed_in_pieces(eng, dims, recs, quiet_waves):
    from vispeech_amd.service import StreamingBatchService
    svc = StreamingBatchService(Net(eng, dims), chunk_frames=16, first_chunk_frames=4, collate=lambda rows: None, autostart=False)
    lengths = [N100, N5, N0, N20]
    assert [ref.frames_of(n) for n in lengths] == [100, 5, 0, 20] and (N20 + 2 * PAD - N_FFT) % HOP == 0
    sessions = [(svc.open_conversion(SRC, TGT, 7 + i, noise_scale=0.0), recs[n]) for i, n in enumerate(lengths)]
    got = drive(svc, sessions, pieces=(1, 255, 4097, 2048))
    assert svc._live == []
    for n, pcm in zip(lengths, got):
        T = ref.frames_of(n)
        assert len(pcm) == 2 * T * UP, n                                 # exactly T(n) * up samples
        if T:
            check_pcm(pcm, quiet_waves[n], WAVE_TOL, f"live session of {T} frames")


# ---------------------------------------------------------------------------------------------- 7. a mixed tick
def test_a_live_session_shares_ticks_with_text_and_one_shot_conversions(eng, oracle, dims, recs):
    from vispeech_amd.service import StreamingBatchService
    inter = dims.inter_channels
    batch = iso.make_batch([6], [2], seed=2150)
    batch["phonemes"] = batch["phonemes"] % (dims.n_vocab - 1) + 1
    batch["sid"] = batch["sid"] % dims.n_speakers
    collate = lambda rows: {k: batch[k][rows] for k in ("phonemes", "lengths", "sid", "duration", "f0", "energy")}
    text_noise = np.zeros((1, inter, 6), np.float32)
    text_noise[0] = to_np(eng.randn(301, inter, 6))
    batch["noise"] = text_noise
    text_ref, _, L = iso.alone(oracle, batch, 0, "controls", noise=text_noise)
    assert L == 6
    conv_ref = wave_alone(oracle, recs[N9], SRC, TGT, to_np(eng.randn(302, inter, 9)))            # [inter][T]: the one-shot layout
    live_ref = wave_alone(oracle, recs[N20], SRC, TGT, live_noise(eng, 303, 20, inter))          # frame-major: the live layout
    svc = StreamingBatchService(Net(eng, dims), chunk_frames=4, collate=collate, autostart=False)
    live = svc.open_conversion(SRC, TGT, 303)
    live.feed(recs[N20])
    live.end()
    text, conv = svc.submit(0, 301), svc.submit_conversion(recs[N9], SRC, TGT, 302)
    while svc.step():
        pass
    assert svc.stats["rows_per_tick"] == [3, 3, 2, 1, 1] and svc.stats["groups"] == 1      # 6, 9 and 20 frames share ticks
    check_pcm(b"".join(text), text_ref["o"][0, 0], TEXT_WAVE_TOL, "text")
    check_pcm(b"".join(conv), conv_ref, WAVE_TOL, "one-shot conversion")
    check_pcm(b"".join(live), live_ref, WAVE_TOL, "live conversion")


# ---------------------------------------------------------------------------------------------- 8. the fused output stage
def test_a_live_session_at_an_output_rate(eng, dims, recs, quiet_waves):
    from vispeech_amd.service import StreamingBatchService
    try:
        svc = StreamingBatchService(Net(eng, dims), chunk_frames=8, first_chunk_frames=3, collate=lambda rows: None,
                                    autostart=False, output_rate=22050, fused_output=True)
        (got,) = drive(svc, [(svc.open_conversion(SRC, TGT, 1, noise_scale=0.0), recs[N20])])
    finally:
        eng.configure_output(None)
    L, M, _ = osr.plan(44100, 22050)
    want = osr.resample_fp64(quiet_waves[N20], osr.filter_fp64(44100, 22050), L, M)
    assert len(got) == 2 * osr.out_len(20 * UP, L, M)
    check_pcm(got, want, WAVE_TOL, "live session at 22050 Hz")


# ---------------------------------------------------------------------------------------------- 9. the default configuration
def test_default_configuration_interior_window():
    from oracle.vispeech_oracle import Oracle
    from vispeech_amd.engine import Engine
    from vispeech_amd.schema import ModelDims
    from vispeech_amd.synth import synth_state_dict
    d = ModelDims()
    sd = synth_state_dict(d, seed=1234)
    e = Engine(d)
    e.set_weights(sd, strict=True)
    e.finalize()
    assert e.convert_halo == 96
    hop, n_fft = d.hop_length, 2 * (d.spec_channels - 1)
    n = 230 * hop + 100
    assert e.convert_frames(n) == 230
    r = np.random.Generator(np.random.PCG64(46))
    audio = (0.4 * np.sin(2 * np.pi * 220.0 * np.arange(n) / 44100.0) * 0.7 + 0.1 * r.standard_normal(n)).astype(np.float32).clip(-1, 1)
    want = z_hat_alone(Oracle(sd, d), audio, n_fft, hop, 5, 20, live_noise(e, 11, 230, d.inter_channels))
    hi_n = (116 + 96 - 1) * hop - (n_fft - hop) // 2 + n_fft          # what an open window that ends at frame 116 + H needs
    ready, w0, w1, lo, hi = e.convert_window_plan(hi_n, False, 100, 116)
    assert ready and (w0, w1, hi) == (4, 212, hi_n) and lo > 0
    buf = np.full(hi_n - lo + 3, np.nan, np.float32)
    buf[: hi - lo] = audio[lo:hi]
    z, _ = e.convert_stream_rows([(torch.from_numpy(buf).to(e.device), lo, hi_n, False, 100, 116, 5, 20, 11, 1.0)], 16)
    z = to_np(z)[0]
    err = frame_err(z, want[:, 100:116], float(np.abs(want).max()))
    print(f"default configuration, frames [100, 116) of 230: err {err:.2e}, bound {Z_TOL:.0e}")
    assert np.isfinite(z).all() and err <= Z_TOL
