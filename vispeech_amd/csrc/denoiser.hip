// Denoiser and inverse STFT (include/vispeech_hip.h, "denoiser and inverse STFT"): the generator's
// zero-input spectrum subtracted from every STFT frame of a ragged batch, and the way back to audio by weighted
// overlap-add.  Framing and both DFT products are the launchers of the spectrogram front end (spectrogram_ragged.hip,
// conv_mfma.hip); the kernels here are the subtraction, the overlap-add and the two small ones of the bias.
// For streams ("denoiser for streams") every row is a window of frames of its own stream: the window
// framing of the live conversion (convert_window.hip), the same two products, and the rows forms of the two kernels.
#include "api_common.h"
#include "fft_plan.h"       // (the n_fft the in-LDS FFT transforms, the layout of its tables)
#include "stft_framing.h"   // (the LDS budget and the bank skew of the framing kernels: overlap-add is framing run backwards)

using namespace vsp;

namespace vsp {

// One thread per element of the row's [spec_ch][T_max] plane, flat, as stft_magnitude_ragged_kernel: columns at or behind
// T_b stay what the framing and the convolution made them (zeros).  s = 0 gives q = m / m = 1: the spectrum's own bits.
__global__ void __launch_bounds__(256) denoise_subtract_kernel(float* __restrict__ ri, long r_bs, long r_cs,
                                                               const int64_t* __restrict__ n_samples,
                                                               const float* __restrict__ bias, const float* __restrict__ strength,
                                                               int L_max, int n_fft, int hop, int spec_ch, int T_max) {
  const int b = blockIdx.y;
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;      // r * T_max + t
  long n = n_samples[b];
  n = n < 0 ? 0 : (n > L_max ? (long)L_max : n);
  const long Tb = stft_ragged_frames(n, n_fft, hop);
  if (e >= (long)spec_ch * T_max) return;
  const int r = (int)(e / T_max), t = (int)(e - (long)r * T_max);
  if (t >= Tb) return;
  float* re_p = ri + (size_t)b * r_bs + (size_t)r * r_cs + t;
  float* im_p = ri + (size_t)b * r_bs + (size_t)(spec_ch + r) * r_cs + t;
  const float re = *re_p, im = *im_p;
  const float m = sqrtf(re * re + im * im);
  const float q = m > 0.f ? fmaxf(m - strength[b] * bias[(size_t)b * spec_ch + r], 0.f) / m : 0.f;
  *re_p = q * re;
  *im_p = q * im;
}

// The rows form: the same expressions on the same operands, so a bin has the bits denoise_subtract_kernel gives it.
__global__ void __launch_bounds__(256) denoise_subtract_rows_kernel(float* __restrict__ ri, long r_bs, long r_cs,
                                                                    const DenoiseSubRows rows, int spec_ch, int T_max) {
  const int b = blockIdx.y;
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;      // r * T_max + t
  if (e >= (long)spec_ch * T_max) return;
  const DenoiseSubRow row = rows.r[b];
  const int r = (int)(e / T_max), t = (int)(e - (long)r * T_max);
  if (t >= row.Tw) return;
  float* re_p = ri + (size_t)b * r_bs + (size_t)r * r_cs + t;
  float* im_p = ri + (size_t)b * r_bs + (size_t)(spec_ch + r) * r_cs + t;
  const float re = *re_p, im = *im_p;
  const float m = sqrtf(re * re + im * im);
  const float q = m > 0.f ? fmaxf(m - row.strength * row.bias[r], 0.f) / m : 0.f;
  *re_p = q * re;
  *im_p = q * im;
}

hipError_t launch_denoise_subtract_rows(float* ri, long r_bs, long r_cs, const DenoiseSubRows& rows, int B, int spec_ch,
                                        int T_max, hipStream_t s) {
  if (!ri || B <= 0 || B > STREAM_ROWS_MAX || T_max <= 0 || spec_ch <= 0 || r_cs < T_max) return hipErrorInvalidValue;
  for (int b = 0; b < B; ++b)
    if (!rows.r[b].bias || rows.r[b].Tw <= 0 || rows.r[b].Tw > T_max) return hipErrorInvalidValue;
  const long blocks = ((long)spec_ch * T_max + 255) / 256;
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(denoise_subtract_rows_kernel, dim3((unsigned)blocks, B), dim3(256), 0, s, ri, r_bs, r_cs, rows, spec_ch, T_max);
  return hipGetLastError();
}

hipError_t launch_denoise_subtract(float* ri, long r_bs, long r_cs, const int64_t* n_samples, const float* bias,
                                   const float* strength, int B, int L_max, int n_fft, int hop, int spec_ch, int T_max,
                                   hipStream_t s) {
  if (!ri || !n_samples || !bias || !strength || B <= 0 || B > 65535 || T_max <= 0 || spec_ch <= 0 || hop <= 0 || n_fft < hop)
    return hipErrorInvalidValue;
  const long blocks = ((long)spec_ch * T_max + 255) / 256;
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(denoise_subtract_kernel, dim3((unsigned)blocks, B), dim3(256), 0, s, ri, r_bs, r_cs, n_samples, bias,
                     strength, L_max, n_fft, hop, spec_ch, T_max);
  return hipGetLastError();
}

int istft_ola_tile(int n_fft, int hop) {
  if (hop <= 0 || n_fft < hop) return 0;
  for (int tile = FR_MAX_TILE; tile >= 1; tile >>= 1) {
    const long span = (long)tile * hop;
    if (span < (1L << 30) && (long)(fr_slot((int)span) + 1) * (long)sizeof(float) <= FR_LDS_BYTES) return tile;
  }
  return 0;
}

// One block = the `tile * hop` samples [t0 hop, (t0 + tile) hop) of one row's PADDED signal.  Sample p = (t0 + tl) hop + kk
// is covered by the frames t0 + tl - (R - 1) .. t0 + tl (R = n_fft / hop), frame t at its slot p - t hop; in pass q the
// block reads the [hop][tile] piece of the synthesis frames whose rows are the slots [(R - 1 - q) hop, (R - q) hop) and
// whose columns are the frames t0 - (R - 1) + q .. -- rows of `tile` contiguous floats, the pattern the framing kernel
// stores.  A thread owns the same samples in every pass, so each sum is ONE chain from 0 in ascending t whatever the tile;
// frames outside [0, T_b) are skipped, in the sum and in W alike.  The quotients pass through LDS (the framing kernel's
// skewed slots) to leave coalesced, clipped to the row's own [0, n_b).
__global__ void __launch_bounds__(FR_THREADS) istft_ola_kernel(const float* __restrict__ v, long v_bs, long v_cs,
                                                               const int64_t* __restrict__ n_samples,
                                                               const float* __restrict__ w2, float* __restrict__ out, long o_bs,
                                                               int L_max, int n_fft, int hop, int tile) {
  extern __shared__ float span[];
  const int b = blockIdx.y, t0 = blockIdx.x * tile;
  long n = n_samples[b];
  n = n < 0 ? 0 : (n > L_max ? (long)L_max : n);
  const long Tb = stft_ragged_frames(n, n_fft, hop);
  const int pad = (n_fft - hop) / 2, R = n_fft / hop;
  const long p0 = (long)t0 * hop;
  const int total = tile * hop;
  // (uniform over the block) nothing of the row falls into this span
  if (Tb <= 0 || p0 >= pad + n || p0 + total <= pad) return;
  const float* row = v + (size_t)b * v_bs;
  for (int e = threadIdx.x; e < total; e += FR_THREADS) {
    const int tl = e % tile, kk = e / tile;      // (tile is a power of two)
    float sum = 0.f, w = 0.f;
    for (int q = 0; q < R; ++q) {
      const long t = (long)t0 + tl - (R - 1) + q;
      const int k = kk + (R - 1 - q) * hop;
      if (t < 0 || t >= Tb) continue;
      sum += row[(size_t)k * v_cs + t];
      w += w2[k];
    }
    span[fr_slot(tl * hop + kk)] = w > 0.f ? sum / w : 0.f;
  }
  __syncthreads();
  float* o = out + (size_t)b * o_bs;
  for (int i = threadIdx.x; i < total; i += FR_THREADS) {
    const long j = p0 + i - pad;
    if (j >= 0 && j < n) o[j] = span[fr_slot(i)];
  }
}

hipError_t launch_istft_ola(const float* v, long v_bs, long v_cs, const int64_t* n_samples, const float* w2, float* out,
                            long o_bs, int B, int L_max, int n_fft, int hop, int T_max, hipStream_t s) {
  const int tile = istft_ola_tile(n_fft, hop);
  if (!v || !n_samples || !w2 || !out || B <= 0 || B > 65535 || L_max <= 0 || T_max <= 0 || tile <= 0 || n_fft % hop ||
      (n_fft - hop) % 2 || o_bs < L_max || v_cs < T_max)
    return hipErrorInvalidValue;
  // the padded signal of the longest row ends behind frame T_max - 1: (T_max - 1) hop + n_fft = (T_max + R - 1) hop samples
  const int R = n_fft / hop;
  const int tiles = (T_max + R - 1 + tile - 1) / tile;
  const size_t lds = (size_t)(fr_slot(tile * hop) + 1) * sizeof(float);
  hipLaunchKernelGGL(istft_ola_kernel, dim3(tiles, B), dim3(FR_THREADS), lds, s, v, v_bs, v_cs, n_samples, w2, out, o_bs, L_max,
                     n_fft, hop, tile);
  return hipGetLastError();
}

// The rows form.  One block = the `tile * hop` padded positions [(w0 + c0) hop, (w0 + c0 + tile) hop) of one row, c0 =
// blockIdx.x * tile a column of the row's window: the walk starts at the window's first position, so the tiles are not
// those of istft_ola_kernel -- and need not be, because a thread's chain is the sample's own: the frames floor(p / hop) -
// (R - 1) .. floor(p / hop), ascending, from 0, those outside [0, T_b) skipped.  Frame t is column t - w0; a column
// outside the window is skipped for memory's sake only (the host's windows hold every frame of every REQUESTED output, and
// the quotient of any other position is not stored).  The same two loops and the same skewed slots as above.
__global__ void __launch_bounds__(FR_THREADS) istft_ola_rows_kernel(const float* __restrict__ v, long v_bs, long v_cs,
                                                                    const DenoiseOlaRows rows, const float* __restrict__ w2,
                                                                    int n_fft, int hop, int tile) {
  extern __shared__ float span[];
  const int b = blockIdx.y, c0 = blockIdx.x * tile;
  const DenoiseOlaRow r = rows.r[b];
  const int pad = (n_fft - hop) / 2, R = n_fft / hop;
  const long p0 = ((long)r.w0 + c0) * hop;
  const int total = tile * hop;
  const long j0 = r.out_first + pad, j1 = j0 + r.out_count;       // the requested outputs as padded positions
  // (uniform over the block) none of the row's outputs falls into this span
  if (p0 >= j1 || p0 + total <= j0) return;
  const float* row = v + (size_t)b * v_bs;
  for (int e = threadIdx.x; e < total; e += FR_THREADS) {
    const int tl = e % tile, kk = e / tile;      // (tile is a power of two)
    float sum = 0.f, w = 0.f;
    for (int q = 0; q < R; ++q) {
      const int c = c0 + tl - (R - 1) + q;
      const int k = kk + (R - 1 - q) * hop;
      if (c < 0 || c >= r.Tw || (long)r.w0 + c >= r.T_b) continue;
      sum += row[(size_t)k * v_cs + c];
      w += w2[k];
    }
    span[fr_slot(tl * hop + kk)] = w > 0.f ? sum / w : 0.f;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < total; i += FR_THREADS) {
    const long p = p0 + i;
    if (p >= j0 && p < j1) r.out[p - j0] = span[fr_slot(i)];
  }
}

hipError_t launch_istft_ola_rows(const float* v, long v_bs, long v_cs, const DenoiseOlaRows& rows, const float* w2, int B,
                                 int n_fft, int hop, int T_max, hipStream_t s) {
  const int tile = istft_ola_tile(n_fft, hop);
  if (!v || !w2 || B <= 0 || B > STREAM_ROWS_MAX || T_max <= 0 || tile <= 0 || n_fft % hop || (n_fft - hop) % 2 || v_cs < T_max)
    return hipErrorInvalidValue;
  const int R = n_fft / hop, pad = (n_fft - hop) / 2;
  for (int b = 0; b < B; ++b) {
    const DenoiseOlaRow& r = rows.r[b];
    // every output lies under the window: [w0 hop, (w0 + Tw + R - 1) hop) in padded positions
    if (!r.out || r.out_count <= 0 || r.out_first < 0 || r.w0 < 0 || r.Tw <= 0 || r.Tw > T_max || r.T_b <= r.w0 ||
        r.out_first + pad < (long)r.w0 * hop || r.out_first + pad + r.out_count > ((long)r.w0 + r.Tw + R - 1) * hop)
      return hipErrorInvalidValue;
  }
  const int tiles = (T_max + R - 1 + tile - 1) / tile;
  const size_t lds = (size_t)(fr_slot(tile * hop) + 1) * sizeof(float);
  hipLaunchKernelGGL(istft_ola_rows_kernel, dim3(tiles, B), dim3(FR_THREADS), lds, s, v, v_bs, v_cs, rows, w2, n_fft, hop, tile);
  return hipGetLastError();
}

__global__ void __launch_bounds__(256) denoise_bias_frames_kernel(const float* __restrict__ period, float* __restrict__ f,
                                                                  long f_cs, int S, int n_fft, int hop) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;      // n * S + s
  if (e >= (long)n_fft * S) return;
  const int n = (int)(e / S), s = (int)(e - (long)n * S);
  f[(size_t)n * f_cs + s] = period[(size_t)s * hop + n % hop];
}

hipError_t launch_denoise_bias_frames(const float* period, float* f, long f_cs, int S, int n_fft, int hop, hipStream_t s) {
  if (!period || !f || S <= 0 || hop <= 0 || n_fft < hop || f_cs < S) return hipErrorInvalidValue;
  const long blocks = ((long)n_fft * S + 255) / 256;
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(denoise_bias_frames_kernel, dim3((unsigned)blocks), dim3(256), 0, s, period, f, f_cs, S, n_fft, hop);
  return hipGetLastError();
}

__global__ void __launch_bounds__(256) denoise_bias_magnitude_kernel(const float* __restrict__ ri, long r_cs,
                                                                     float* __restrict__ bias, int S, int spec_ch) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;      // s * spec_ch + r
  if (e >= (long)S * spec_ch) return;
  const int s = (int)(e / spec_ch), r = (int)(e - (long)s * spec_ch);
  const float re = ri[(size_t)r * r_cs + s], im = ri[(size_t)(spec_ch + r) * r_cs + s];
  bias[e] = sqrtf(re * re + im * im);
}

hipError_t launch_denoise_bias_magnitude(const float* ri, long r_cs, float* bias, int S, int spec_ch, hipStream_t s) {
  if (!ri || !bias || S <= 0 || spec_ch <= 0 || r_cs < S) return hipErrorInvalidValue;
  const long blocks = ((long)S * spec_ch + 255) / 256;
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(denoise_bias_magnitude_kernel, dim3((unsigned)blocks), dim3(256), 0, s, ri, r_cs, bias, S, spec_ch);
  return hipGetLastError();
}

}  // namespace vsp

namespace {

struct Geometry { int n_fft, hop, spec; };

// The context's own geometry, or why it has none.
const char* denoise_geometry(const vsp_ctx* ctx, Geometry* g) {
  const vsp_config& c = ctx->cfg;
  if (c.spec_channels <= 1) return "the context has no spectrogram (spec_channels <= 1)";
  long up = 1;
  for (int i = 0; i < c.n_upsamples && i < VSP_MAX_LIST; ++i) {
    if (c.upsample_rates[i] < 1 || up > (1L << 24)) return "the generator's upsampling rates are not positive";
    up *= c.upsample_rates[i];
  }
  const int N = 2 * (c.spec_channels - 1);
  if (up > N || N % (int)up) return "the hop (the generator's total upsampling) does not divide n_fft";
  const int hop = (int)up;
  // fewer than four frames over a sample leave the last samples of some rows uncovered or under a vanishing window sum
  if (N / hop < 4 || (N - hop) % 2) return "n_fft / hop < 4, or n_fft - hop is odd: the window sum does not cover every sample";
  if (stft_ragged_tile(N, hop) <= 0 || istft_ola_tile(N, hop) <= 0 || ctx->model.istft.M != N)
    return "n_fft exceeds what a block of the framing and overlap-add kernels stages";
  *g = Geometry{N, hop, c.spec_channels};
  return nullptr;
}

// The transform the context's switch asks for (vsp_set_stft_transform refuses VSP_STFT_FFT where it cannot run).
bool use_fft(const vsp_ctx* ctx) { return ctx->stft_transform == VSP_STFT_FFT && ctx->model.has_fft; }

// One launch of fft.hip under the library's per-launch events (class FRAME, as the products it stands in for): `passes`
// transforms of B x T frames -- 5 N log2 N flops each, the textbook count --, the frame tensor read and written once.
template <class Launch>
void fft_launch(Run& r, const Geometry& g, int B, int T, int passes, const char* what, Launch launch) {
  if (!r.ok()) return;
  const bool prof = r.prof_begin(VSP_PROF_FRAME);
  r.chk(launch(), what);
  if (prof) {
    const double frames = (double)B * T, bytes = 2.0 * 4.0 * frames * g.n_fft;
    r.prof_end(VSP_PROF_FRAME, passes * 5.0 * g.n_fft * std::log2((double)g.n_fft) * frames, bytes, bytes, bytes);
  }
}

struct Rows { const int64_t* n; const float* strength; };      // the upload: the head of the workspace
size_t rows_bytes(int B) { return ((size_t)B * (sizeof(int64_t) + sizeof(float)) + 255) / 256 * 256; }

struct DenoiseIO {
  const float* audio; int64_t audio_stride; const float* ri; const float* bias; float* out; int64_t out_stride; Rows rows;
};

// framing -> DFT -> subtraction in place -> inverse DFT -> overlap-add; with io.ri the synthesis half alone
void denoise_impl(Run& r, const Geometry& g, int B, int L_max, int T, const DenoiseIO& io, bool synthesis_only) {
  vsp_ctx* const ctx = r.ctx;
  Ws& ws = r.ws;
  if (use_fft(ctx)) {
    // framing -> ONE launch, frames to synthesis frames in place (RI stays in LDS) -> overlap-add; the synthesis half
    // alone: the inverse transform of io.ri into the same tensor
    T3 F = ws.t3(B, g.n_fft, T);
    if (ws.dry || ws.overflow) return;
    const float* tab = r.A(ctx->model.fft_tab);
    if (synthesis_only) {
      fft_launch(r, g, B, T, 1, "fft inverse", [&] {
        return launch_fft_inverse(io.ri, (long)2 * g.spec * T, T, F.p, F.bs, F.cs, tab, io.rows.n, B, L_max, g.n_fft, g.hop, T, r.s);
      });
    } else {
      r.chk(launch_stft_frames_ragged(io.audio, (long)io.audio_stride, io.rows.n, F.p, F.bs, F.cs, B, L_max, g.n_fft, g.hop, T, r.s),
            "stft frames ragged");
      fft_launch(r, g, B, T, 2, "fft denoise", [&] {
        return launch_fft_denoise(F.p, F.bs, F.cs, F.p, F.bs, F.cs, tab, io.rows.n, io.bias, io.rows.strength, B, L_max, g.n_fft, g.hop,
                                  g.spec, T, r.s);
      });
    }
    if (r.ok())
      r.chk(launch_istft_ola(F.p, F.bs, F.cs, io.rows.n, r.A(ctx->model.istft_w2), io.out, (long)io.out_stride, B, L_max, g.n_fft, g.hop,
                             T, r.s),
            "istft overlap-add");
    return;
  }
  T3 F = ws.t3(B, g.n_fft, T), RI = ws.t3(B, 2 * g.spec, T), V = ws.t3(B, g.n_fft, T);
  if (ws.dry || ws.overflow) return;
  if (synthesis_only) {
    RI = ext(io.ri, 2 * g.spec, T);
  } else {
    r.chk(launch_stft_frames_ragged(io.audio, (long)io.audio_stride, io.rows.n, F.p, F.bs, F.cs, B, L_max, g.n_fft, g.hop, T, r.s),
          "stft frames ragged");
    ConvArgs a = r.args(ctx->model.stft, F, RI, T, T);
    a.fixed_form = 1;      // (a row's bits must not depend on B or T_max: no grid-size threshold picks the kernel)
    r.conv(a, B);
    if (r.ok())
      r.chk(launch_denoise_subtract(RI.p, RI.bs, RI.cs, io.rows.n, io.bias, io.rows.strength, B, L_max, g.n_fft, g.hop, g.spec, T, r.s),
            "denoise subtract");
  }
  ConvArgs a = r.args(ctx->model.istft, RI, V, T, T);
  a.fixed_form = 1;
  r.conv(a, B);
  if (r.ok())
    r.chk(launch_istft_ola(V.p, V.bs, V.cs, io.rows.n, r.A(ctx->model.istft_w2), io.out, (long)io.out_stride, B, L_max, g.n_fft, g.hop,
                           T, r.s),
          "istft overlap-add");
}

void bias_impl(Run& r, const Geometry& g, int S, const float* period, float* bias) {
  Ws& ws = r.ws;
  T3 F = ws.t3(1, g.n_fft, S), RI = ws.t3(1, 2 * g.spec, S);
  if (ws.dry || ws.overflow) return;
  r.chk(launch_denoise_bias_frames(period, F.p, F.cs, S, g.n_fft, g.hop, r.s), "denoise bias frames");
  if (use_fft(r.ctx)) {      // (every column a speaker: all S of them live)
    fft_launch(r, g, 1, S, 1, "fft forward", [&] {
      return launch_fft_forward(F.p, F.bs, F.cs, RI.p, RI.bs, RI.cs, r.A(r.ctx->model.fft_tab), nullptr, 1, 0, g.n_fft, g.hop, S, r.s);
    });
    if (r.ok()) r.chk(launch_denoise_bias_magnitude(RI.p, RI.cs, bias, S, g.spec, r.s), "denoise bias magnitude");
    return;
  }
  ConvArgs a = r.args(r.ctx->model.stft, F, RI, S, S);
  a.fixed_form = 1;        // (a speaker's bias does not depend on the speakers it is computed with)
  r.conv(a, 1);
  if (r.ok()) r.chk(launch_denoise_bias_magnitude(RI.p, RI.cs, bias, S, g.spec, r.s), "denoise bias magnitude");
}

int frames_of(const Geometry& g, int64_t n) {
  const long T = stft_ragged_frames((long)n, g.n_fft, g.hop);
  return T > 0x7fffffffL ? 0 : (int)T;
}

// What vsp_istft and vsp_denoise share: the rows checked on the host naming the row, the workspace, the ONE upload, the run.
int denoise_call(vsp_ctx* ctx, const char* who, void* stream, int B, int L_max, const int64_t* n_host, const float* strength_host,
                 DenoiseIO io, bool synthesis_only, void* workspace, int64_t workspace_bytes) {
  if (!ctx) return VSP_ERR_ARG;
  Geometry g;
  if (const char* why = denoise_geometry(ctx, &g)) return ctx->fail(VSP_ERR_ARG, "%s: %s", who, why);
  const int pad = (g.n_fft - g.hop) / 2;
  if (B <= 0 || B > 65535 || L_max <= pad || L_max > (1 << 30) || !n_host || (!synthesis_only && !strength_host) ||
      (synthesis_only ? !io.ri : !io.audio || io.audio_stride < L_max) || !io.out || io.out_stride < L_max)
    return ctx->fail(VSP_ERR_ARG, "%s: bad argument (needs 1 <= B <= 65535, (n_fft - hop) / 2 = %d < L_max <= 2^30, strides >= L_max "
                                  "and no null pointer)", who, pad);
  const int T = frames_of(g, L_max);
  std::vector<char> up(rows_bytes(B), 0);
  int64_t* n_up = reinterpret_cast<int64_t*>(up.data());
  float* s_up = reinterpret_cast<float*>(up.data() + (size_t)B * sizeof(int64_t));
  bool any = false;
  for (int b = 0; b < B; ++b) {
    const float s = synthesis_only ? 0.f : strength_host[b];
    if (std::isnan(s)) { n_up[b] = 0; s_up[b] = 0.f; continue; }      // left alone: a row of no samples to every kernel
    if (n_host[b] <= pad || n_host[b] > L_max)
      return ctx->fail(VSP_ERR_ARG, "%s: row %d: %lld samples are not in ((n_fft - hop) / 2 = %d, L_max = %d]", who, b,
                       (long long)n_host[b], pad, L_max);
    if (s < 0.f || std::isinf(s)) return ctx->fail(VSP_ERR_ARG, "%s: row %d: the strength %g is negative or infinite", who, b, (double)s);
    if (!synthesis_only && !io.bias) return ctx->fail(VSP_ERR_ARG, "%s: row %d: a finite strength and no bias", who, b);
    n_up[b] = n_host[b];
    s_up[b] = s;
    any = true;
  }
  const int64_t need = vsp_denoise_workspace_bytes(ctx, B, L_max);
  if (need < 0) return ctx->fail(VSP_ERR_ARG, "%s: bad argument", who);
  if (!workspace || workspace_bytes < need)
    return ctx->fail(VSP_ERR_WORKSPACE, "%s workspace too small: %lld < %lld bytes", who, (long long)(workspace ? workspace_bytes : 0),
                     (long long)need);
  if (const int rc = check_ready(ctx)) return rc;
  if (!any) return VSP_OK;
  if (const int rc = vsp::Call{ctx, who, (hipStream_t)stream}.upload(workspace, up.data(), up.size())) return rc;
  io.rows.n = reinterpret_cast<const int64_t*>(workspace);
  io.rows.strength = reinterpret_cast<const float*>(static_cast<char*>(workspace) + (size_t)B * sizeof(int64_t));
  if (!io.bias) io.bias = io.rows.strength;      // (never read: the subtraction does not run without a bias)
  return run_sized(ctx, stream, who, need, workspace, workspace_bytes,
                   [&](Run& r) { denoise_impl(r, g, B, L_max, T, io, synthesis_only); }, (int64_t)rows_bytes(B));
}

// ---- rows: every row a window of frames of its own stream ------------------------------------
constexpr int64_t DN_MAX_SAMPLES = (int64_t)1 << 30;
constexpr long DN_NO_BOUND = 1L << 40;      // T_b of a stream whose end is unknown

// The largest window a row of L outputs has: its first output's frame, R - 1 before it, and one per hop started behind it.
int rows_window_max(const Geometry& g, int64_t L) { return (int)((L - 1 + g.hop - 1) / g.hop) + g.n_fft / g.hop; }

struct RowsIO { ConvWinFrameRows frame; DenoiseSubRows sub; DenoiseOlaRows ola; };

// launch_window_frames -> DFT -> subtraction in place -> inverse DFT -> overlap-add over the windows; B live rows
void denoise_rows_impl(Run& r, const Geometry& g, int B, int T, const RowsIO* io) {
  vsp_ctx* const ctx = r.ctx;
  Ws& ws = r.ws;
  int64_t* scal = static_cast<int64_t*>(ws.bytes((size_t)3 * B * sizeof(int64_t)));      // what the framing kernel leaves for others
  if (use_fft(ctx)) {        // (as denoise_impl: the same template of the fused kernel, so a frame has the one-shot call's bits)
    T3 F = ws.t3(B, g.n_fft, T);
    if (ws.dry || ws.overflow) return;
    r.chk(launch_window_frames(io->frame, F.p, F.bs, F.cs, scal, scal + B, scal + 2 * B, B, g.n_fft, g.hop, T, r.s), "window frames");
    fft_launch(r, g, B, T, 2, "fft denoise rows", [&] {
      return launch_fft_denoise_rows(F.p, F.bs, F.cs, F.p, F.bs, F.cs, r.A(ctx->model.fft_tab), io->sub, B, g.n_fft, g.spec, T, r.s);
    });
    if (r.ok())
      r.chk(launch_istft_ola_rows(F.p, F.bs, F.cs, io->ola, r.A(ctx->model.istft_w2), B, g.n_fft, g.hop, T, r.s), "istft overlap-add rows");
    return;
  }
  T3 F = ws.t3(B, g.n_fft, T), RI = ws.t3(B, 2 * g.spec, T), V = ws.t3(B, g.n_fft, T);
  if (ws.dry || ws.overflow) return;
  r.chk(launch_window_frames(io->frame, F.p, F.bs, F.cs, scal, scal + B, scal + 2 * B, B, g.n_fft, g.hop, T, r.s), "window frames");
  ConvArgs a = r.args(ctx->model.stft, F, RI, T, T);
  a.fixed_form = 1;        // (as denoise_impl: the form of the product is the one-shot call's whatever B and T)
  r.conv(a, B);
  if (r.ok()) r.chk(launch_denoise_subtract_rows(RI.p, RI.bs, RI.cs, io->sub, B, g.spec, T, r.s), "denoise subtract rows");
  a = r.args(ctx->model.istft, RI, V, T, T);
  a.fixed_form = 1;
  r.conv(a, B);
  if (r.ok())
    r.chk(launch_istft_ola_rows(V.p, V.bs, V.cs, io->ola, r.A(ctx->model.istft_w2), B, g.n_fft, g.hop, T, r.s), "istft overlap-add rows");
}

}  // namespace

extern "C" {

int vsp_set_stft_transform(vsp_ctx* ctx, int kind) {
  if (!ctx) return VSP_ERR_ARG;
  if (kind != VSP_STFT_DFT && kind != VSP_STFT_FFT)
    return ctx->fail(VSP_ERR_ARG, "vsp_set_stft_transform: unknown kind %d (VSP_STFT_DFT = 0, VSP_STFT_FFT = 1)", kind);
  if (kind == VSP_STFT_FFT) {
    Geometry g;
    if (const char* why = denoise_geometry(ctx, &g)) return ctx->fail(VSP_ERR_ARG, "vsp_set_stft_transform: %s", why);
    if (g.n_fft != FFT_N || !ctx->model.has_fft)
      return ctx->fail(VSP_ERR_ARG, "vsp_set_stft_transform: the FFT transforms n_fft = %d only, the context has n_fft = %d", FFT_N, g.n_fft);
  }
  ctx->stft_transform = kind;
  return VSP_OK;
}

int vsp_stft_transform(const vsp_ctx* ctx) { return ctx ? ctx->stft_transform : VSP_ERR_ARG; }

int vsp_denoise_history(const vsp_ctx* ctx, int64_t* behind, int64_t* ahead) {
  Geometry g;
  if (!ctx || !behind || !ahead || denoise_geometry(ctx, &g)) return VSP_ERR_ARG;
  *behind = g.n_fft - g.hop;
  *ahead = g.n_fft - 1;
  return VSP_OK;
}

int64_t vsp_denoise_complete(const vsp_ctx* ctx, int64_t n_seen, int closed) {
  Geometry g;
  if (!ctx || n_seen < 0 || denoise_geometry(ctx, &g)) return VSP_ERR_ARG;
  if (closed) return n_seen;
  const int64_t pad = (g.n_fft - g.hop) / 2, room = n_seen + pad - g.n_fft;
  const int64_t Tc = room < 0 ? 0 : room / g.hop + 1;      // frames t with t hop - pad + n_fft <= n_seen
  return std::max<int64_t>(0, Tc * g.hop - pad);
}

int64_t vsp_denoise_rows_workspace_bytes(const vsp_ctx* ctx, int B, int64_t L_max) {
  Geometry g;
  if (!ctx || denoise_geometry(ctx, &g) || B < 1 || B > STREAM_ROWS_MAX || L_max < 1 || L_max > DN_MAX_SAMPLES) return VSP_ERR_ARG;
  const int T = rows_window_max(g, L_max);
  return dry_bytes(ctx, [&](Run& r) { denoise_rows_impl(r, g, B, T, nullptr); });
}

int vsp_denoise_rows(vsp_ctx* ctx, void* stream, int B, const vsp_denoise_row* rows_host, const float* bias, void* workspace,
                     int64_t workspace_bytes) {
  if (!ctx) return VSP_ERR_ARG;
  const char* who = "vsp_denoise_rows";
  Geometry g;
  if (const char* why = denoise_geometry(ctx, &g)) return ctx->fail(VSP_ERR_ARG, "%s: %s", who, why);
  if (B < 1 || B > STREAM_ROWS_MAX || !rows_host) return ctx->fail(VSP_ERR_ARG, "%s: 1 <= B <= %d rows", who, STREAM_ROWS_MAX);
  const int64_t pad = (g.n_fft - g.hop) / 2, R = g.n_fft / g.hop;
  RowsIO io;
  std::memset(&io, 0, sizeof io);
  int live = 0, T = 0;
  int64_t out_max = 1;
  for (int b = 0; b < B; ++b) {
    const vsp_denoise_row& h = rows_host[b];
    if (std::isnan(h.strength)) continue;                  // left alone, whatever else it holds
    if (h.strength < 0.f || std::isinf(h.strength))
      return ctx->fail(VSP_ERR_ARG, "%s: row %d: the strength %g is negative or infinite", who, b, (double)h.strength);
    if (!bias) return ctx->fail(VSP_ERR_ARG, "%s: row %d: a finite strength and no bias", who, b);
    if (h.first < 0 || h.count < 0 || h.out_first < 0 || h.out_count < 0 || h.total < -1 || h.first > DN_MAX_SAMPLES ||
        h.count > DN_MAX_SAMPLES || h.out_first > DN_MAX_SAMPLES || h.out_count > DN_MAX_SAMPLES || h.total > DN_MAX_SAMPLES)
      return ctx->fail(VSP_ERR_ARG, "%s: row %d: negative position or count, or more than 2^30 samples", who, b);
    const int64_t end = h.first + h.count, out_end = h.out_first + h.out_count;
    if (h.total >= 0 && h.total <= pad)
      return ctx->fail(VSP_ERR_ARG, "%s: row %d: a stream of %lld samples is not above (n_fft - hop) / 2 = %lld: the reflection at its ends "
                                    "is undefined", who, b, (long long)h.total, (long long)pad);
    if (h.total >= 0 && (end > h.total || out_end > h.total))
      return ctx->fail(VSP_ERR_ARG, "%s: row %d: samples [%lld, %lld) or outputs [%lld, %lld) lie behind the stream's end %lld", who, b,
                       (long long)h.first, (long long)end, (long long)h.out_first, (long long)out_end, (long long)h.total);
    if ((h.count > 0 && !h.in) || (h.out_count > 0 && !h.out)) return ctx->fail(VSP_ERR_ARG, "%s: row %d: null pointer", who, b);
    out_max = std::max(out_max, h.out_count);
    if (h.out_count == 0) continue;                        // nothing to put out: nothing is read either
    // the frames that cover the outputs, and the samples those frames read (convert_window_plan without a halo)
    const bool closed = h.total >= 0 && end == h.total;
    const long T_b = h.total >= 0 ? stft_ragged_frames((long)h.total, g.n_fft, g.hop) : DN_NO_BOUND;
    const int64_t w0 = std::max<int64_t>(0, (h.out_first + pad) / g.hop - (R - 1));
    const int64_t w1 = std::min<int64_t>(T_b, (out_end - 1 + pad) / g.hop + 1);
    long lo = 0, hi = 0;
    // (an open row's frames must end inside its samples; a closed one's reflect at `total`)
    if (w1 <= w0 || convert_window_plan(g.n_fft, g.hop, 0, (long)end, closed ? 1 : 0, (int)w0, (int)w1, nullptr, nullptr, &lo, &hi) < 0)
      return ctx->fail(VSP_ERR_ARG, "%s: row %d: no frame covers the outputs [%lld, %lld)", who, b, (long long)h.out_first,
                       (long long)out_end);
    if (hi > end)
      return ctx->fail(VSP_ERR_ARG, "%s: row %d: outputs up to %lld need the samples up to %lld (look-ahead n_fft - 1 at most), the row ends "
                                    "at %lld before the stream does", who, b, (long long)out_end, (long long)hi, (long long)end);
    if (lo < h.first)
      return ctx->fail(VSP_ERR_ARG, "%s: row %d: output %lld needs the samples from %lld on (history n_fft - hop at most), the row starts at %lld",
                       who, b, (long long)h.out_first, (long long)lo, (long long)h.first);
    const int Tw = (int)(w1 - w0);
    ConvWinFrameRow& f = io.frame.r[live];
    f.audio = h.in; f.first = (long)h.first; f.n = (long)end; f.w0 = (int)w0; f.Tw = Tw; f.closed = closed ? 1 : 0;
    io.sub.r[live] = DenoiseSubRow{bias + (size_t)b * g.spec, h.strength, Tw};
    io.ola.r[live] = DenoiseOlaRow{h.out, (long)h.out_first, T_b, (int)h.out_count, (int)w0, Tw, 0};
    T = std::max(T, Tw);
    ++live;
  }
  const int64_t need = vsp_denoise_rows_workspace_bytes(ctx, B, out_max);
  if (need < 0) return ctx->fail(VSP_ERR_ARG, "%s: bad argument", who);
  if (!workspace || workspace_bytes < need)
    return ctx->fail(VSP_ERR_WORKSPACE, "%s workspace too small: %lld < %lld bytes", who, (long long)(workspace ? workspace_bytes : 0),
                     (long long)need);
  if (const int rc = check_ready(ctx)) return rc;
  if (!live) return VSP_OK;
  // (live <= B and T <= the window of out_max outputs: the run fits what `need` measured)
  return run_sized(ctx, stream, who, need, workspace, workspace_bytes, [&](Run& r) { denoise_rows_impl(r, g, live, T, &io); });
}

int64_t vsp_denoise_workspace_bytes(const vsp_ctx* ctx, int B, int L_max) {
  Geometry g;
  if (!ctx || denoise_geometry(ctx, &g) || B <= 0 || B > 65535 || L_max <= (g.n_fft - g.hop) / 2 || L_max > (1 << 30)) return VSP_ERR_ARG;
  const int T = frames_of(g, L_max);
  if (T <= 0) return VSP_ERR_ARG;
  return (int64_t)rows_bytes(B) + dry_bytes(ctx, [&](Run& r) { denoise_impl(r, g, B, L_max, T, DenoiseIO{}, false); });
}

int vsp_denoise_bias(vsp_ctx* ctx, void* stream, int S, const float* period, float* bias, void* workspace,
                     int64_t workspace_bytes) {
  if (!ctx) return VSP_ERR_ARG;
  Geometry g;
  if (const char* why = denoise_geometry(ctx, &g)) return ctx->fail(VSP_ERR_ARG, "vsp_denoise_bias: %s", why);
  if (S <= 0 || S > 65535 || !period || !bias) return ctx->fail(VSP_ERR_ARG, "vsp_denoise_bias: bad argument (needs 1 <= S <= 65535 and no null pointer)");
  const int64_t need = dry_bytes(ctx, [&](Run& r) { bias_impl(r, g, S, nullptr, nullptr); });
  if (!workspace || workspace_bytes < need)
    return ctx->fail(VSP_ERR_WORKSPACE, "vsp_denoise_bias workspace too small: %lld < %lld bytes", (long long)(workspace ? workspace_bytes : 0),
                     (long long)need);
  if (const int rc = check_ready(ctx)) return rc;
  return run_sized(ctx, stream, "vsp_denoise_bias", need, workspace, workspace_bytes, [&](Run& r) { bias_impl(r, g, S, period, bias); });
}

int vsp_istft(vsp_ctx* ctx, void* stream, int B, int L_max, const float* ri, const int64_t* n_samples_host, float* out,
              int64_t out_stride, void* workspace, int64_t workspace_bytes) {
  DenoiseIO io{};
  io.ri = ri; io.out = out; io.out_stride = out_stride;
  return denoise_call(ctx, "vsp_istft", stream, B, L_max, n_samples_host, nullptr, io, true, workspace, workspace_bytes);
}

int vsp_denoise(vsp_ctx* ctx, void* stream, int B, int L_max, const float* audio, int64_t audio_stride,
                const int64_t* n_samples_host, const float* bias, const float* strength_host, float* out, int64_t out_stride,
                void* workspace, int64_t workspace_bytes) {
  DenoiseIO io{};
  io.audio = audio; io.audio_stride = audio_stride; io.bias = bias; io.out = out; io.out_stride = out_stride;
  return denoise_call(ctx, "vsp_denoise", stream, B, L_max, n_samples_host, strength_host, io, false, workspace, workspace_bytes);
}

}  // extern "C"
