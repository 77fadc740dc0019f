// Ragged spectrogram front end (vsp_spectrogram_ragged, vsp_convert_latent): every row of the batch is a recording of
// its own length n_b inside a padded [B][stride] buffer.  Row b gets the frames of ITS reflect-padded signal
// (reference mel_processing.py:51-70 on audio[b][:n_b] alone) and exact zeros behind its T_b frames; nothing at or behind
// n_b is read.  The DFT between the two kernels is the model.stft convolution of vsp_spectrogram.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"
#include "stft_framing.h"   // (the LDS budget and the bank skew, shared with the window framing of convert_window.hip)

namespace vsp {

int stft_ragged_tile(int n_fft, int hop) {
  for (int tile = FR_MAX_TILE; tile >= 1; tile >>= 1) {
    const long span = (long)(tile - 1) * hop + n_fft;
    if (span < (1L << 30) && (long)(fr_slot((int)span) + 1) * (long)sizeof(float) <= FR_LDS_BYTES) return tile;
  }
  return 0;
}

// One block = `tile` consecutive frames of one row.  The frames overlap (n_fft > hop), so the row's span of
// (live - 1) * hop + n_fft samples is read ONCE, coalesced, reflected at the row's own two ends, into LDS; then the
// [n_fft][tile] piece of the operand is written with the frame index on the lanes (t contiguous in memory).
// (stft_frames_kernel reads audio[t * hop + n - pad] with t on the lanes: every load is its own cache line.)
__global__ void __launch_bounds__(FR_THREADS) stft_frames_ragged_kernel(const float* __restrict__ audio, long a_bs,
                                                                        const int64_t* __restrict__ n_samples,
                                                                        float* __restrict__ f, long f_bs, long f_cs, int L_max,
                                                                        int n_fft, int hop, int T_max, int tile) {
  extern __shared__ float span[];
  const int b = blockIdx.y, t0 = blockIdx.x * tile;
  long n = n_samples[b];
  n = n < 0 ? 0 : (n > L_max ? (long)L_max : n);
  const long Tb = stft_ragged_frames(n, n_fft, hop);
  const int cols = T_max - t0 < tile ? T_max - t0 : tile;                 // columns of the operand this block owns
  const long left = Tb - (long)t0;
  const int live = left <= 0 ? 0 : (left < cols ? (int)left : cols);      // ... of which these are frames of the row
  const int pad = (n_fft - hop) / 2;
  if (live > 0) {
    // Tb > 0 means n > pad, and t < Tb means t * hop + n_fft <= n + 2 pad: every index below reflects into [0, n)
    const int len = (live - 1) * hop + n_fft;
    const float* row = audio + (size_t)b * a_bs;
    const long first = (long)t0 * hop - pad;
    for (int i = threadIdx.x; i < len; i += FR_THREADS) {
      long j = first + i;
      if (j < 0) j = -j;                       // torch reflect padding (edge sample not repeated)
      if (j >= n) j = 2 * (n - 1) - j;
      span[fr_slot(i)] = row[j];
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

hipError_t launch_stft_frames_ragged(const float* audio, long a_bs, const int64_t* n_samples, float* f, long f_bs, long f_cs,
                                     int B, int L_max, int n_fft, int hop, int T_max, hipStream_t s) {
  const int tile = stft_ragged_tile(n_fft, hop);
  if (!audio || !n_samples || !f || B <= 0 || L_max <= 0 || T_max <= 0 || hop <= 0 || n_fft < hop || tile <= 0 || a_bs < L_max)
    return hipErrorInvalidValue;
  const int tiles = (T_max + tile - 1) / tile;
  if (B > 65535) return hipErrorInvalidValue;
  const int span = (tile - 1) * hop + n_fft;
  const size_t lds = (size_t)(fr_slot(span) + 1) * sizeof(float);
  hipLaunchKernelGGL(stft_frames_ragged_kernel, dim3(tiles, B), dim3(FR_THREADS), lds, s, audio, a_bs, n_samples, f, f_bs, f_cs,
                     L_max, n_fft, hop, T_max, tile);
  return hipGetLastError();
}

// The magnitude of vsp_spectrogram's kernel for the row's own frames; a column at or behind T_b is 0.0 (NOT sqrt(1e-6),
// what the magnitude of a zero frame gives).  frames[b] = T_b, written by the row's first thread.  One thread per element
// of the row's [spec_ch][T_max] plane, flat: a batch of short recordings (T_max of a few frames) fills its waves too,
// and the store is contiguous across the whole plane.
__global__ void __launch_bounds__(256) stft_magnitude_ragged_kernel(const float* __restrict__ ri, long r_bs, long r_cs,
                                                                    const int64_t* __restrict__ n_samples,
                                                                    float* __restrict__ spec, int64_t* __restrict__ frames,
                                                                    int L_max, int n_fft, int hop, int spec_ch, int T_max) {
  const int b = blockIdx.y;
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;      // r * T_max + t
  long n = n_samples[b];                                           // (uniform over the block: one scalar load)
  n = n < 0 ? 0 : (n > L_max ? (long)L_max : n);
  const long Tb = stft_ragged_frames(n, n_fft, hop);
  if (e == 0) frames[b] = Tb;
  if (e >= (long)spec_ch * T_max) return;
  const int r = (int)(e / T_max), t = (int)(e - (long)r * T_max);
  float v = 0.f;
  if (t < Tb) {
    const float re = ri[(size_t)b * r_bs + (size_t)r * r_cs + t];
    const float im = ri[(size_t)b * r_bs + (size_t)(spec_ch + r) * r_cs + t];
    v = sqrtf(re * re + im * im + 1e-6f);
  }
  spec[(size_t)b * spec_ch * T_max + e] = v;
}

hipError_t launch_stft_magnitude_ragged(const float* ri, long r_bs, long r_cs, const int64_t* n_samples, float* spec,
                                        int64_t* frames, int B, int L_max, int n_fft, int hop, int spec_ch, int T_max,
                                        hipStream_t s) {
  if (!ri || !n_samples || !spec || !frames || B <= 0 || T_max <= 0 || spec_ch <= 0 || B > 65535)
    return hipErrorInvalidValue;
  const long blocks = ((long)spec_ch * T_max + 255) / 256;
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(stft_magnitude_ragged_kernel, dim3((unsigned)blocks, B), dim3(256), 0, s, ri, r_bs, r_cs, n_samples, spec,
                     frames, L_max, n_fft, hop, spec_ch, T_max);
  return hipGetLastError();
}

}  // namespace vsp
