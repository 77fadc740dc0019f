// Live voice conversion (vsp_convert_stream_rows): every row of the call is a WINDOW of frames [w0, w0 + Tw) of a
// recording that may still be arriving.  z_hat of a frame depends on a bounded span of spectrogram columns
// (vsp_convert_halo_frames), so the window's frames -- framed here from the samples they read, reflected at the
// recording's true ends only -- run through the posterior encoder and the flows as an utterance of Tw frames, and the
// frames a full halo away from the window's artificial ends are those of the whole recording.  The kernels around that
// chain: the window framing and its magnitude, the frame-major noise, the cut.  The DFT between the first two is the
// model.stft convolution of vsp_spectrogram.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>

#include "kernels.h"
#include "philox.h"
#include "stft_framing.h"

namespace vsp {

// Host arithmetic only.  A window's frames [w0, w1) read the samples [w0 hop - pad, (w1 - 1) hop - pad + n_fft) of the
// reflect-padded recording.  Reflected at sample 0 (j -> -j) that range becomes [max(0, w0 hop - pad), ...): the mirrored
// samples 1 .. pad lie inside the first window, which reaches hop + pad - 1 >= pad.  At the end (j -> 2 (n - 1) - j, a
// closed recording only) the samples at and behind n fold back below n - 1.
int convert_window_plan(int n_fft, int hop, int halo, long n_known, int closed, int e0, int e1, int* w0, int* w1, long* s_lo,
                        long* s_hi) {
  if (hop <= 0 || n_fft < hop || halo < 0 || n_known < 0 || e0 < 0 || e1 <= e0 || e1 > INT_MAX - halo) return -1;
  const long pad = (n_fft - hop) / 2;
  const long T = stft_ragged_frames(n_known, n_fft, hop);
  if (closed && e1 > T) return -1;
  const int a = std::max(0, e0 - halo);
  int b = e1 + halo;
  if (closed && b > T) b = (int)T;
  long lo = std::max(0L, (long)a * hop - pad), hi = (long)(b - 1) * hop - pad + n_fft;      // [lo, hi) after |j|
  if (closed && hi > n_known) {
    lo = std::min(lo, 2 * (n_known - 1) - (hi - 1));
    hi = n_known;
  }
  if (w0) *w0 = a;
  if (w1) *w1 = b;
  if (s_lo) *s_lo = lo;
  if (s_hi) *s_hi = hi;
  return lo >= 0 && hi <= n_known ? 1 : 0;
}

// One block = `tile` consecutive columns of one row's window: stft_frames_ragged_kernel's scheme (the span of the live
// columns once through LDS, coalesced, then the [n_fft][tile] piece of the operand with the column on the lanes), for a
// window that starts at frame w0 of a buffer that starts at sample `first`.
__global__ void __launch_bounds__(FR_THREADS) window_frames_kernel(ConvWinFrameRows rows, float* __restrict__ f, long f_bs,
                                                                   long f_cs, int64_t* __restrict__ len,
                                                                   int64_t* __restrict__ sid_src, int64_t* __restrict__ sid_tgt,
                                                                   int n_fft, int hop, int T_max, int tile) {
  extern __shared__ float span[];
  const int b = blockIdx.y, t0 = blockIdx.x * tile;
  const ConvWinFrameRow r = rows.r[b];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    len[b] = r.Tw;
    sid_src[b] = r.sid_src;
    sid_tgt[b] = r.sid_tgt;
  }
  const int cols = T_max - t0 < tile ? T_max - t0 : tile;                 // columns of the operand this block owns
  const int left = r.Tw - t0;
  const int live = left <= 0 ? 0 : (left < cols ? left : cols);           // ... of which these are frames of the window
  const int pad = (n_fft - hop) / 2;
  if (live > 0) {
    const int n_span = (live - 1) * hop + n_fft;
    const long first = (long)(r.w0 + t0) * hop - pad;
    for (int i = threadIdx.x; i < n_span; i += FR_THREADS) {
      long j = first + i;
      if (j < 0) j = -j;                                  // torch reflect padding (edge sample not repeated)
      if (r.closed && j >= r.n) j = 2 * (r.n - 1) - j;    // (an open row reads nothing at or behind n: convert_window_plan)
      span[fr_slot(i)] = r.audio[j - r.first];
    }
  }
  __syncthreads();
  float* out = f + (size_t)b * f_bs + t0;
  const int total = n_fft * tile;
  for (int e = threadIdx.x; e < total; e += FR_THREADS) {
    const int tl = e % tile, k = e / tile;     // (tile is a power of two)
    if (tl >= cols) continue;
    out[(size_t)k * f_cs + tl] = tl < live ? span[fr_slot(tl * hop + k)] : 0.f;
  }
}

hipError_t launch_window_frames(const ConvWinFrameRows& rows, float* f, long f_bs, long f_cs, int64_t* len, int64_t* sid_src,
                                int64_t* sid_tgt, int B, int n_fft, int hop, int T_max, hipStream_t s) {
  const int tile = stft_ragged_tile(n_fft, hop);
  if (!f || !len || !sid_src || !sid_tgt || B <= 0 || B > STREAM_ROWS_MAX || T_max <= 0 || hop <= 0 || n_fft < hop || tile <= 0)
    return hipErrorInvalidValue;
  for (int b = 0; b < B; ++b)
    if (!rows.r[b].audio || rows.r[b].Tw <= 0 || rows.r[b].Tw > T_max || rows.r[b].w0 < 0) return hipErrorInvalidValue;
  const int tiles = (T_max + tile - 1) / tile;
  const int span = (tile - 1) * hop + n_fft;
  const size_t lds = (size_t)(fr_slot(span) + 1) * sizeof(float);
  hipLaunchKernelGGL(window_frames_kernel, dim3(tiles, B), dim3(FR_THREADS), lds, s, rows, f, f_bs, f_cs, len, sid_src, sid_tgt,
                     n_fft, hop, T_max, tile);
  return hipGetLastError();
}

// stft_magnitude_ragged_kernel with the window's length in place of the recording's frame count
__global__ void __launch_bounds__(256) window_magnitude_kernel(const float* __restrict__ ri, long r_bs, long r_cs,
                                                               const int64_t* __restrict__ len, float* __restrict__ spec,
                                                               int spec_ch, int T_max) {
  const int b = blockIdx.y;
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;      // r * T_max + t
  if (e >= (long)spec_ch * T_max) return;
  const long Tw = len[b];                                          // (uniform over the block: one scalar load)
  const int r = (int)(e / T_max), t = (int)(e - (long)r * T_max);
  float v = 0.f;
  if (t < Tw) {
    const float re = ri[(size_t)b * r_bs + (size_t)r * r_cs + t];
    const float im = ri[(size_t)b * r_bs + (size_t)(spec_ch + r) * r_cs + t];
    v = sqrtf(re * re + im * im + 1e-6f);
  }
  spec[(size_t)b * spec_ch * T_max + e] = v;
}

hipError_t launch_window_magnitude(const float* ri, long r_bs, long r_cs, const int64_t* len, float* spec, int B, int spec_ch,
                                   int T_max, hipStream_t s) {
  if (!ri || !len || !spec || B <= 0 || T_max <= 0 || spec_ch <= 0 || B > 65535) return hipErrorInvalidValue;
  const long blocks = ((long)spec_ch * T_max + 255) / 256;
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(window_magnitude_kernel, dim3((unsigned)blocks, B), dim3(256), 0, s, ri, r_bs, r_cs, len, spec, spec_ch,
                     T_max);
  return hipGetLastError();
}

// One element per thread, the column on the lanes (the store is contiguous); the four words of a counter are computed by
// the four threads that share it, as in randn_ragged_kernel.
__global__ void __launch_bounds__(256) window_noise_kernel(ConvWinNoiseRows rows, int C, int T_max, float* __restrict__ out) {
  const int b = blockIdx.y;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;      // c * T_max + j
  if (i >= (long)C * T_max) return;
  const ConvWinNoiseRow r = rows.r[b];
  const int c = (int)(i / T_max), j = (int)(i - (long)c * T_max);
  float v = 0.f;
  if (j < r.Tw && r.scale != 0.f) v = r.scale * philox_randn_element(r.seed, ((long)r.w0 + j) * C + c);
  out[(size_t)b * C * T_max + i] = v;
}

hipError_t launch_window_noise(const ConvWinNoiseRows& rows, int B, int C, int T_max, float* out, hipStream_t s) {
  if (!out || B <= 0 || B > STREAM_ROWS_MAX || C <= 0 || T_max <= 0) return hipErrorInvalidValue;
  const long blocks = ((long)C * T_max + 255) / 256;
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(window_noise_kernel, dim3((unsigned)blocks, B), dim3(256), 0, s, rows, C, T_max, out);
  return hipGetLastError();
}

__global__ void __launch_bounds__(256) window_cut_kernel(const float* __restrict__ z, StreamCollectRows rows, int C, int T_max,
                                                         float* __restrict__ out, int span) {
  const int b = blockIdx.y;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;      // c * span + j
  if (i >= (long)C * span) return;
  const StreamCollectRow r = rows.r[b];
  const int c = (int)(i / span), j = (int)(i - (long)c * span);
  out[(size_t)b * C * span + i] = j < r.n ? z[((size_t)b * C + c) * T_max + r.off + j] : 0.f;
}

hipError_t launch_window_cut(const float* z, const StreamCollectRows& rows, int B, int C, int T_max, float* out, int span,
                             hipStream_t s) {
  if (!z || !out || B <= 0 || B > STREAM_ROWS_MAX || C <= 0 || T_max <= 0 || span <= 0) return hipErrorInvalidValue;
  for (int b = 0; b < B; ++b) {
    const StreamCollectRow& r = rows.r[b];
    if (r.off < 0 || r.n < 0 || r.n > span || (long)r.off + r.n > T_max) return hipErrorInvalidValue;
  }
  const long blocks = ((long)C * span + 255) / 256;
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(window_cut_kernel, dim3((unsigned)blocks, B), dim3(256), 0, s, z, rows, C, T_max, out, span);
  return hipGetLastError();
}

}  // namespace vsp
