// Voice conversion (api_common.h): the linear spectrogram, padded and ragged, the posterior encoder's entry point,
// SynthesizerTrn.voice_conversion from spectrograms (vsp_voice_conversion) and from audio (vsp_convert_latent).
#include "api_common.h"

using namespace vsp;

namespace {

// The tensors of a sequence as its entry point receives them; the sizing pass hands in an empty one.
struct SpecIO {
  const float* audio; float* spec;
  // the ragged form (n_samples != NULL): row b holds n_samples[b] samples of audio_stride, and frames[b] is written
  int64_t audio_stride; const int64_t* n_samples; int64_t* frames;
};
struct VcIO {
  const float* y; const int64_t *y_lengths, *sid_src, *sid_tgt; const float* noise;
  float* o_hat; uint8_t* y_mask; float *z, *z_p, *z_hat, *m_q, *logs_q;
};
struct ConvertIO {
  SpecIO audio;
  const int64_t *sid_src, *sid_tgt; const float* noise; float noise_scale;
  float *z_hat, *g_tgt; uint8_t* y_mask; float *z, *z_p;
};
// ... and of the chain the two conversions share; every tensor dense, [B][C][T]
struct ChainIO {
  T3 y; const int64_t *lengths, *sid_src, *sid_tgt;
  const float* noise; float noise_scale;
  // the rows' own noise is drawn here if noise is NULL and noise_scale is not 0, from this copy of their seeds (draw_noise_rows)
  float* drawn; uint64_t* seeds_dev;
  float *g_src, *g_tgt; uint8_t* y_mask; float *z, *m_q, *logs_q, *z_p, *z_hat;
};

// audio [B][L] -> |STFT| [B][spec][T]: frames, the windowed DFT as one convolution, magnitude.  The ragged form frames
// every row by its own length (kernels.h, stft_ragged_frames); same convolution, same plan.
void spectrogram_impl(Run& r, int B, int L, int hop, int T, const SpecIO& io) {
  vsp_ctx* const ctx = r.ctx; const hipStream_t s = r.s; Ws& ws = r.ws;
  const vsp_config& c = ctx->cfg;
  const int n_fft = 2 * (c.spec_channels - 1);
  T3 F = ws.t3(B, n_fft, T), RI = ws.t3(B, 2 * c.spec_channels, T);
  if (ws.dry || ws.overflow) return;
  if (io.n_samples)
    r.chk(launch_stft_frames_ragged(io.audio, (long)io.audio_stride, io.n_samples, F.p, F.bs, F.cs, B, L, n_fft, hop, T, s),
          "stft frames ragged");
  else r.chk(launch_stft_frames(io.audio, L, F.p, F.bs, F.cs, B, L, n_fft, hop, T, s), "stft frames");
  ConvArgs a = r.args(ctx->model.stft, F, RI, T, T);
  r.conv(a, B);
  if (r.ok() && io.n_samples)
    r.chk(launch_stft_magnitude_ragged(RI.p, RI.bs, RI.cs, io.n_samples, io.spec, io.frames, B, L, n_fft, hop, c.spec_channels, T, s),
          "stft magnitude ragged");
  else if (r.ok()) r.chk(launch_stft_magnitude(RI.p, RI.bs, RI.cs, io.spec, B, c.spec_channels, T, s), "stft magnitude");
}

// SynthesizerTrn.voice_conversion (reference models.py:724-732) up to z_hat, under the caller's overlay: the two speaker
// rows, the mask, z = enc_q(y, g_src), z_p = flow(z, g_src), z_hat = flow(z_p, g_tgt, reverse).  Allocates scratch only.
void run_conversion(Run& r, Overlay& stages, int B, int T, const ChainIO& io) {
  const vsp_config& c = r.ctx->cfg;
  const Model& m = r.ctx->model;
  const int inter = c.inter_channels, gin = c.gin_channels;
  const long n = (long)B * inter * T;
  const bool live = !r.dry() && !r.ws.overflow;
  const float* noise = io.noise;
  if (live) {
    r.chk(launch_gather_rows(io.sid_src, r.A(m.emb_g), c.n_speakers, io.g_src, B, gin, r.s), "emb_g");
    r.chk(launch_gather_rows(io.sid_tgt, r.A(m.emb_g), c.n_speakers, io.g_tgt, B, gin, r.s), "emb_g");
    r.chk(launch_mask_u8(io.lengths, io.y_mask, B, T, r.s), "y_mask");
    if (io.noise_scale == 0.f) {
      noise = nullptr;                       // z = m_q: nothing is drawn, nothing is read
    } else if (!noise) {
      draw_noise_rows(r, io.seeds_dev, io.lengths, B, inter, T, io.drawn);
      noise = io.drawn;
    }
  }
  run_posterior(r, B, T, io.y, io.lengths, io.g_src, noise, ext(io.z, inter, T), ext(io.m_q, inter, T), ext(io.logs_q, inter, T),
                io.noise_scale);
  stages.next();
  if (live && r.ok()) r.chk(hipMemcpyAsync(io.z_p, io.z, n * sizeof(float), hipMemcpyDeviceToDevice, r.s), "z_p copy");
  run_flow(r, B, T, ext(io.z_p, inter, T), io.g_src, io.lengths, false);
  if (live && r.ok()) r.chk(hipMemcpyAsync(io.z_hat, io.z_p, n * sizeof(float), hipMemcpyDeviceToDevice, r.s), "z_hat copy");
  stages.next();
  run_flow(r, B, T, ext(io.z_hat, inter, T), io.g_tgt, io.lengths, true);
}

// SynthesizerTrn.voice_conversion (reference models.py:724-732)
void vc_impl(Run& r, int B, int T, const VcIO& io) {
  const vsp_config& c = r.ctx->cfg;
  const int inter = c.inter_channels, gin = c.gin_channels;
  Ws& ws = r.ws;
  r.iso = r.ctx->isolated;     // (the posterior encoder and both flows mask already: the generator call is the difference)
  float* g_src = ws.f((size_t)B * gin);
  float* g_tgt = ws.f((size_t)B * gin);
  // (scratch where the caller wants no m_q / logs_q; dense like theirs: launch_reparam walks contiguous tensors)
  float* m_q = io.m_q ? io.m_q : ws.t3(B, inter, T).p;
  float* logs_q = io.logs_q ? io.logs_q : ws.t3(B, inter, T).p;
  Overlay stages(ws);
  run_conversion(r, stages, B, T, ChainIO{ext(io.y, c.spec_channels, T), io.y_lengths, io.sid_src, io.sid_tgt, io.noise, 1.f, {}, {},
                                          g_src, g_tgt, io.y_mask, io.z, m_q, logs_q, io.z_p, io.z_hat});
  stages.next();
  // dec(z_hat * y_mask, g_tgt): z_hat is already masked by the flow's last update on x1 ... but x0
  // passes through unmasked only if the input was unmasked; z is masked, so z_hat * mask == z_hat.
  run_gen(r, B, T, ext(io.z_hat, inter, T), io.y_lengths, g_tgt, io.o_hat);
}

int convert_geometry(const vsp_ctx* ctx, int hop, int* n_fft) {
  if (!ctx || ctx->cfg.spec_channels <= 1 || hop <= 0) return VSP_ERR_ARG;
  *n_fft = 2 * (ctx->cfg.spec_channels - 1);
  return *n_fft < hop ? VSP_ERR_ARG : VSP_OK;
}

// frames of the padded shape, or <= 0: the shape the grids and the tensors of a ragged call are sized by
int convert_t_max(const vsp_ctx* ctx, int B, int L_max, int hop) {
  int n_fft = 0;
  if (convert_geometry(ctx, hop, &n_fft) != VSP_OK || B <= 0 || L_max <= 0 || stft_ragged_tile(n_fft, hop) <= 0) return VSP_ERR_ARG;
  return vsp_convert_frames(ctx, L_max, hop);
}

// Audio to the converted latent: ragged spectrogram -> enc_q(g_src) -> flow(g_src) -> flow(g_tgt, reverse), every stage
// with the rows' own frame counts as lengths (voice_conversion, reference models.py:724-732, up to z_hat).
void convert_latent_impl(Run& r, int B, int L_max, int hop, int T, const ConvertIO& io) {
  const vsp_config& c = r.ctx->cfg;
  const long n = (long)B * c.inter_channels * T;
  Ws& ws = r.ws;
  float* g_src = ws.f((size_t)B * c.gin_channels);
  float* spec = ws.f((size_t)B * c.spec_channels * T);
  float* z = io.z ? io.z : ws.f((size_t)n);
  float* z_p = io.z_p ? io.z_p : ws.f((size_t)n);
  float* m_q = ws.f((size_t)n);              // (launch_reparam walks contiguous tensors)
  float* logs_q = ws.f((size_t)n);
  float* drawn = ws.f((size_t)n);
  uint64_t* seeds_dev = reinterpret_cast<uint64_t*>(ws.bytes((size_t)B * sizeof(uint64_t)));
  Overlay stages(ws);
  SpecIO audio = io.audio;
  audio.spec = spec;
  spectrogram_impl(r, B, L_max, hop, T, audio);
  if (r.rc) return;
  stages.next();
  run_conversion(r, stages, B, T, ChainIO{ext(spec, c.spec_channels, T), io.audio.frames, io.sid_src, io.sid_tgt, io.noise,
                                          io.noise_scale, drawn, seeds_dev, g_src, io.g_tgt, io.y_mask, z, m_q, logs_q, z_p, io.z_hat});
}

// The rows of a vsp_convert_stream_rows call as its kernels take them (kernels.h), built and checked on the host.
struct WindowRows {
  ConvWinFrameRows frame; ConvWinNoiseRows noise; StreamCollectRows cut;
  bool draws = false;          // some row has a noise_scale other than 0
};
struct WindowIO {
  const WindowRows* rows;      // NULL in the sizing pass
  int span_frames; float *z_hat, *g_tgt;
};

// Windows of live recordings to their z_hat: window framing -> DFT -> magnitude, then the chain of vsp_convert_latent on
// the windows as utterances of w1 - w0 frames (their lengths and speakers written by the framing launch), then the cut.
// T: the longest window of the call (the sizing pass: span_frames + 2 halo).
void convert_window_impl(Run& r, int B, int hop, int T, const WindowIO& io) {
  vsp_ctx* const ctx = r.ctx;
  const vsp_config& c = ctx->cfg;
  const int n_fft = 2 * (c.spec_channels - 1), inter = c.inter_channels;
  const long n = (long)B * inter * T;
  Ws& ws = r.ws;
  int64_t* len = reinterpret_cast<int64_t*>(ws.bytes((size_t)B * sizeof(int64_t)));
  int64_t* sid_src = reinterpret_cast<int64_t*>(ws.bytes((size_t)B * sizeof(int64_t)));
  int64_t* sid_tgt = reinterpret_cast<int64_t*>(ws.bytes((size_t)B * sizeof(int64_t)));
  uint8_t* y_mask = reinterpret_cast<uint8_t*>(ws.bytes((size_t)B * T));
  float* g_src = ws.f((size_t)B * c.gin_channels);
  float* spec = ws.f((size_t)B * c.spec_channels * T);
  float *z = ws.f((size_t)n), *z_p = ws.f((size_t)n), *z_hat = ws.f((size_t)n);
  float *m_q = ws.f((size_t)n), *logs_q = ws.f((size_t)n);      // (launch_reparam walks contiguous tensors)
  float* drawn = ws.f((size_t)n);
  Overlay stages(ws);
  {
    T3 F = ws.t3(B, n_fft, T), RI = ws.t3(B, 2 * c.spec_channels, T);
    if (!ws.dry && !ws.overflow) {
      r.chk(launch_window_frames(io.rows->frame, F.p, F.bs, F.cs, len, sid_src, sid_tgt, B, n_fft, hop, T, r.s), "window frames");
      ConvArgs a = r.args(ctx->model.stft, F, RI, T, T);
      r.conv(a, B);
      if (r.ok()) r.chk(launch_window_magnitude(RI.p, RI.bs, RI.cs, len, spec, B, c.spec_channels, T, r.s), "window magnitude");
      if (r.ok() && io.rows->draws) r.chk(launch_window_noise(io.rows->noise, B, inter, T, drawn, r.s), "window noise");
    }
  }
  if (r.rc) return;
  stages.next();
  // (the rows' noise arrives scaled: noise_scale is each row's own; with no row drawing, nothing is read)
  const bool draws = io.rows && io.rows->draws;
  run_conversion(r, stages, B, T, ChainIO{ext(spec, c.spec_channels, T), len, sid_src, sid_tgt, draws ? drawn : nullptr,
                                          draws ? 1.f : 0.f, nullptr, nullptr, g_src, io.g_tgt, y_mask, z, m_q, logs_q, z_p, z_hat});
  if (!ws.dry && !ws.overflow && r.ok())
    r.chk(launch_window_cut(z_hat, io.rows->cut, B, inter, T, io.z_hat, io.span_frames, r.s), "window cut");
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------------------------- spectrogram
int vsp_spectrogram_frames(const vsp_ctx* ctx, int L, int hop) {
  if (!ctx || ctx->cfg.spec_channels <= 1 || hop <= 0) return VSP_ERR_ARG;
  const int n_fft = 2 * (ctx->cfg.spec_channels - 1), pad = (n_fft - hop) / 2;
  if (L <= pad || n_fft < hop) return VSP_ERR_ARG;      // reflect padding needs pad < L
  return 1 + (L + 2 * pad - n_fft) / hop;
}

int64_t vsp_spectrogram_workspace_bytes(const vsp_ctx* ctx, int B, int L, int hop) {
  const int T = vsp_spectrogram_frames(ctx, L, hop);
  if (T <= 0 || B <= 0) return VSP_ERR_ARG;
  return dry_bytes(ctx, [&](Run& r) { spectrogram_impl(r, B, L, hop, T, SpecIO{}); });
}

int vsp_spectrogram(vsp_ctx* ctx, void* stream, int B, int L, int hop, const float* audio, float* spec, void* workspace,
                    int64_t workspace_bytes) {
  int rc = check_ready(ctx);
  if (rc) return rc;
  if (ctx->cfg.spec_channels <= 1) return ctx->fail(VSP_ERR_STATE, "context was created without spec_channels");
  const int T = vsp_spectrogram_frames(ctx, L, hop);
  if (T <= 0 || B <= 0 || !audio || !spec || !workspace)
    return ctx->fail(VSP_ERR_ARG, "vsp_spectrogram: bad argument (the signal must be longer than (n_fft - hop) / 2)");
  return run_sized(ctx, stream, "spectrogram", vsp_spectrogram_workspace_bytes(ctx, B, L, hop), workspace, workspace_bytes,
                   [&](Run& r) { spectrogram_impl(r, B, L, hop, T, SpecIO{audio, spec}); });
}

// Frames of a recording of n samples: host arithmetic (kernels.h, stft_ragged_frames), 0 where there is no frame.
int vsp_convert_frames(const vsp_ctx* ctx, int64_t n_samples, int hop) {
  int n_fft = 0;
  if (convert_geometry(ctx, hop, &n_fft) != VSP_OK || n_samples < 0) return VSP_ERR_ARG;
  const long T = stft_ragged_frames((long)n_samples, n_fft, hop);
  return T > 0x7fffffffL ? VSP_ERR_ARG : (int)T;
}

int64_t vsp_spectrogram_ragged_workspace_bytes(const vsp_ctx* ctx, int B, int L_max, int hop) {
  const int T = convert_t_max(ctx, B, L_max, hop);
  if (T <= 0) return VSP_ERR_ARG;
  return dry_bytes(ctx, [&](Run& r) { spectrogram_impl(r, B, L_max, hop, T, SpecIO{}); });
}

int vsp_spectrogram_ragged(vsp_ctx* ctx, void* stream, int B, int L_max, int hop, const float* audio, int64_t audio_stride,
                           const int64_t* n_samples, float* spec, int64_t* frames, void* workspace, int64_t workspace_bytes) {
  if (!ctx) return VSP_ERR_ARG;
  const int T = convert_t_max(ctx, B, L_max, hop);
  if (T <= 0 || !audio || audio_stride < L_max || !n_samples || !spec || !frames || !workspace)
    return ctx->fail(VSP_ERR_ARG, "vsp_spectrogram_ragged: bad argument (needs spec_channels, B > 0, hop > 0, a padded length "
                                  "with at least one frame, audio_stride >= L_max and no null pointer)");
  int rc = check_ready(ctx);
  if (rc) return rc;
  const SpecIO io{audio, spec, audio_stride, n_samples, frames};
  return run_sized(ctx, stream, "ragged spectrogram", vsp_spectrogram_ragged_workspace_bytes(ctx, B, L_max, hop), workspace,
                   workspace_bytes, [&](Run& r) { spectrogram_impl(r, B, L_max, hop, T, io); });
}

// ---------------------------------------------------------------------------------- voice conversion
int64_t vsp_posterior_workspace_bytes(const vsp_ctx* ctx, int B, int T) {
  if (!ctx || B <= 0 || T <= 0) return VSP_ERR_ARG;
  return dry_bytes(ctx, [&](Run& r) { run_posterior(r, B, T, T3{}, nullptr, nullptr, nullptr, T3{}, T3{}, T3{}); });
}

int vsp_posterior_encoder(vsp_ctx* ctx, void* stream, int B, int T, const float* y, const int64_t* y_lengths,
                          const float* g, const float* noise, float* z, float* m, float* logs, void* workspace,
                          int64_t workspace_bytes) {
  int rc = check_vc(ctx);
  if (rc) return rc;
  if (B <= 0 || T <= 0 || !y || !y_lengths || !g || !noise || !z || !m || !logs || !workspace)
    return ctx->fail(VSP_ERR_ARG, "vsp_posterior_encoder: bad argument");
  return run_sized(ctx, stream, "posterior", vsp_posterior_workspace_bytes(ctx, B, T), workspace, workspace_bytes, [&](Run& r) {
    const int inter = ctx->cfg.inter_channels;
    run_posterior(r, B, T, ext(y, ctx->cfg.spec_channels, T), y_lengths, g, noise, ext(z, inter, T), ext(m, inter, T),
                  ext(logs, inter, T));
  });
}

int64_t vsp_voice_conversion_workspace_bytes(const vsp_ctx* ctx, int B, int T) {
  if (!ctx || B <= 0 || T <= 0) return VSP_ERR_ARG;
  return dry_bytes(ctx, [&](Run& r) { vc_impl(r, B, T, VcIO{}); });
}

int vsp_voice_conversion(vsp_ctx* ctx, void* stream, int B, int T, const float* y, const int64_t* y_lengths,
                         const int64_t* sid_src, const int64_t* sid_tgt, const float* noise, float* o_hat,
                         uint8_t* y_mask, float* z, float* z_p, float* z_hat, float* m_q, float* logs_q,
                         void* workspace, int64_t workspace_bytes) {
  int rc = check_vc(ctx);
  if (rc) return rc;
  if (B <= 0 || T <= 0 || !y || !y_lengths || !sid_src || !sid_tgt || !noise || !o_hat || !y_mask || !z || !z_p ||
      !z_hat || !workspace)
    return ctx->fail(VSP_ERR_ARG, "vsp_voice_conversion: null or non-positive argument");
  const VcIO io{y, y_lengths, sid_src, sid_tgt, noise, o_hat, y_mask, z, z_p, z_hat, m_q, logs_q};
  return run_sized(ctx, stream, "voice conversion", vsp_voice_conversion_workspace_bytes(ctx, B, T), workspace, workspace_bytes,
                   [&](Run& r) { vc_impl(r, B, T, io); });
}

// ---------------------------------------------------------------------------------- conversion from audio
int64_t vsp_convert_latent_workspace_bytes(const vsp_ctx* ctx, int B, int L_max, int hop) {
  const int T = convert_t_max(ctx, B, L_max, hop);
  if (T <= 0) return VSP_ERR_ARG;
  return dry_bytes(ctx, [&](Run& r) { convert_latent_impl(r, B, L_max, hop, T, ConvertIO{}); });
}

int vsp_convert_latent(vsp_ctx* ctx, void* stream, int B, int L_max, int hop, const float* audio, int64_t audio_stride,
                       const int64_t* n_samples, const int64_t* sid_src, const int64_t* sid_tgt, const float* noise,
                       float noise_scale, float* z_hat, float* g_tgt, int64_t* frames, uint8_t* y_mask, float* z, float* z_p,
                       void* workspace, int64_t workspace_bytes) {
  if (!ctx) return VSP_ERR_ARG;
  const int T = convert_t_max(ctx, B, L_max, hop);
  if (T <= 0 || !audio || audio_stride < L_max || !n_samples || !sid_src || !sid_tgt || !z_hat || !g_tgt || !frames ||
      !y_mask || !workspace || !std::isfinite(noise_scale))
    return ctx->fail(VSP_ERR_ARG, "vsp_convert_latent: bad argument (needs spec_channels, B > 0, hop > 0, a padded length with "
                                  "at least one frame, audio_stride >= L_max, a finite noise_scale and no null pointer)");
  int rc = check_vc(ctx);
  if (rc) return rc;
  if (!noise && noise_scale != 0.f && (int)ctx->noise_seeds.size() != B)
    return ctx->fail(VSP_ERR_STATE, "vsp_convert_latent draws per-row noise: vsp_set_noise_seeds for B = %d first (%d set)", B,
                     (int)ctx->noise_seeds.size());
  const ConvertIO io{{audio, nullptr, audio_stride, n_samples, frames}, sid_src, sid_tgt, noise, noise_scale, z_hat, g_tgt, y_mask, z, z_p};
  return run_sized(ctx, stream, "convert_latent", vsp_convert_latent_workspace_bytes(ctx, B, L_max, hop), workspace, workspace_bytes,
                   [&](Run& r) { convert_latent_impl(r, B, L_max, hop, T, io); });
}

// ---------------------------------------------------------------------------------- live conversion
int vsp_convert_halo_frames(const vsp_ctx* ctx) {
  if (!ctx) return VSP_ERR_ARG;
  const vsp_config& c = ctx->cfg;
  const int side = (c.flow_kernel - 1) / 2;
  if (c.flow_kernel < 1 || c.posterior_layers < 0 || c.n_flows < 0 || c.flow_layers < 0) return VSP_ERR_ARG;
  // enc_q's WN, then the flow forward and the flow in reverse: every WN layer widens the dependence by (k - 1) / 2 a side
  return c.posterior_layers * side + 2 * c.n_flows * c.flow_layers * side;
}

int vsp_convert_window_plan(int n_fft, int hop, int halo, int64_t n_known, int closed, int e0, int e1, int* w0, int* w1,
                            int64_t* s_lo, int64_t* s_hi) {
  long lo = 0, hi = 0;
  const int rc = convert_window_plan(n_fft, hop, halo, (long)n_known, closed, e0, e1, w0, w1, &lo, &hi);
  if (rc < 0) return VSP_ERR_ARG;
  if (s_lo) *s_lo = lo;
  if (s_hi) *s_hi = hi;
  return rc;
}

int64_t vsp_convert_stream_rows_workspace_bytes(const vsp_ctx* ctx, int B, int span_frames) {
  if (!ctx || ctx->cfg.spec_channels <= 1 || B < 1 || B > STREAM_ROWS_MAX || span_frames < 1) return VSP_ERR_ARG;
  const int halo = vsp_convert_halo_frames(ctx);
  if (halo < 0 || span_frames > INT32_MAX / 2 - 2 * halo) return VSP_ERR_ARG;
  return dry_bytes(ctx, [&](Run& r) { convert_window_impl(r, B, 1, span_frames + 2 * halo, WindowIO{}); });
}

int vsp_convert_stream_rows(vsp_ctx* ctx, void* stream, int B, int hop, const vsp_convert_row* rows, int span_frames,
                            float* z_hat, float* g_tgt, void* workspace, int64_t workspace_bytes) {
  if (!ctx) return VSP_ERR_ARG;
  int n_fft = 0;
  const int halo = vsp_convert_halo_frames(ctx);
  if (convert_geometry(ctx, hop, &n_fft) != VSP_OK || stft_ragged_tile(n_fft, hop) <= 0 || halo < 0 || B < 1 ||
      B > STREAM_ROWS_MAX || !rows || span_frames < 1 || !z_hat || !g_tgt || !workspace)
    return ctx->fail(VSP_ERR_ARG, "vsp_convert_stream_rows: bad argument (needs spec_channels, 1 <= B <= %d, hop > 0, "
                                  "span_frames >= 1 and no null pointer)", STREAM_ROWS_MAX);
  WindowRows w;
  int T = 0;
  for (int b = 0; b < B; ++b) {
    const vsp_convert_row& r = rows[b];
    if (!r.audio || r.first_sample < 0 || r.n_known < r.first_sample || r.e1 - (int64_t)r.e0 > span_frames ||
        !std::isfinite(r.noise_scale) || r.sid_src < 0 || r.sid_src >= ctx->cfg.n_speakers || r.sid_tgt < 0 ||
        r.sid_tgt >= ctx->cfg.n_speakers)
      return ctx->fail(VSP_ERR_ARG, "vsp_convert_stream_rows: row %d: null audio, first_sample outside [0, n_known], more than "
                                    "span_frames = %d frames, a noise_scale that is not finite or a speaker outside [0, %d)",
                       b, span_frames, ctx->cfg.n_speakers);
    int w0 = 0, w1 = 0;
    long s_lo = 0, s_hi = 0;
    const int ready = convert_window_plan(n_fft, hop, halo, (long)r.n_known, r.closed != 0, r.e0, r.e1, &w0, &w1, &s_lo, &s_hi);
    if (ready < 0)
      return ctx->fail(VSP_ERR_ARG, "vsp_convert_stream_rows: row %d: frames [%d, %d) are not 0 <= e0 < e1%s", b, r.e0, r.e1,
                       r.closed ? " <= T(n_known)" : "");
    if (ready == 0 || s_lo < r.first_sample)
      return ctx->fail(VSP_ERR_ARG, "vsp_convert_stream_rows: row %d: frames [%d, %d) read samples [%lld, %lld), the buffer holds "
                                    "[%lld, %lld) (vsp_convert_window_plan)", b, r.e0, r.e1, (long long)s_lo, (long long)s_hi,
                       (long long)r.first_sample, (long long)r.n_known);
    w.frame.r[b] = ConvWinFrameRow{r.audio, (long)r.first_sample, (long)r.n_known, w0, w1 - w0, r.closed != 0, (int)r.sid_src,
                                   (int)r.sid_tgt, 0};
    w.noise.r[b] = ConvWinNoiseRow{r.seed, w0, w1 - w0, r.noise_scale, 0};
    w.cut.r[b] = StreamCollectRow{r.e0 - w0, r.e1 - r.e0};
    w.draws = w.draws || r.noise_scale != 0.f;
    T = std::max(T, w1 - w0);
  }
  int rc = check_vc(ctx);
  if (rc) return rc;
  const WindowIO io{&w, span_frames, z_hat, g_tgt};
  return run_sized(ctx, stream, "convert_stream_rows", vsp_convert_stream_rows_workspace_bytes(ctx, B, span_frames), workspace,
                   workspace_bytes, [&](Run& r) { convert_window_impl(r, B, hop, T, io); });
}

}  // extern "C"
