// The STFT of the denoiser as an in-LDS real FFT (include/vispeech_hip.h, vsp_set_stft_transform):
// the three kernels that stand in for the two DFT products and the subtraction between them when a call asks for
// VSP_STFT_FFT.  They work on the operands of the product path -- F [B][n_fft][T] from the framing kernels, RI [B][2 spec][T],
// V [B][n_fft][T] for the overlap-add kernels --, so framing and overlap-add stay what they are.
//
// A block owns `TILE` consecutive frames of one row.  Each frame has an image of M = 1024 complex slots in LDS (fft_plan.h:
// the index math and the arithmetic, shared with tools/micro/fft_plan_main.cpp); the block's 256 threads do one butterfly a
// pass and frame, frame after frame, with the pass's three factors loaded once for the tile.  A frame's arithmetic is a
// function of its own samples only: its place in the tile, the tile's size, B and T do not enter, and the one-shot and the
// rows form of the fused kernel are one template.  Global accesses are rows of TILE contiguous floats, as the framing
// kernel's stores; columns at or behind the row's live count are neither read nor written, and a tile of none returns.
#include <cstdlib>

#include "fft_plan.h"
#include "kernels.h"
#include "stft_framing.h"

namespace vsp {

namespace {

__device__ inline cf ld_cf(const float* tab, int off, int i) { return *reinterpret_cast<const cf*>(tab + off + 2 * i); }

__device__ inline cf* frame_image(cf* img, int tl) { return img + (size_t)tl * FFT_M; }

// x[b][n][t0 + tl] * win[n] -> sample n of frame tl, for the tile's `nf` live frames
template <int TILE>
__device__ inline void stage_frames(cf* img, const float* __restrict__ x, long cs, int t0, int nf, const float* __restrict__ win) {
  float* f = reinterpret_cast<float*>(img);
  for (int e = threadIdx.x; e < FFT_N * TILE; e += FFT_THREADS) {
    const int tl = e % TILE, n = e / TILE;
    if (tl < nf) f[(size_t)tl * (2 * FFT_M) + fft_sample_slot(fft_frame_skew(tl, TILE), n)] = x[(size_t)n * cs + t0 + tl] * win[n];
  }
}

template <int TILE>
__device__ inline void store_frames(const cf* img, float* __restrict__ v, long cs, int t0, int nf, const float* __restrict__ win) {
  const float* f = reinterpret_cast<const float*>(img);
  for (int e = threadIdx.x; e < FFT_N * TILE; e += FFT_THREADS) {
    const int tl = e % TILE, n = e / TILE;
    if (tl < nf) v[(size_t)n * cs + t0 + tl] = f[(size_t)tl * (2 * FFT_M) + fft_sample_slot(fft_frame_skew(tl, TILE), n)] * win[n];
  }
}

template <int TILE>
__device__ inline void forward_passes(cf* img, int nf, const float* __restrict__ tab) {
  for (int p = 0; p < FFT_PASSES; ++p) {
    const FftBfly b = fft_bfly(p, threadIdx.x);
    const cf w1 = ld_cf(tab, FFT_TAB_TW, b.twi), w2 = ld_cf(tab, FFT_TAB_TW, 2 * b.twi), w3 = ld_cf(tab, FFT_TAB_TW, 3 * b.twi);
    for (int tl = 0; tl < nf; ++tl) fft_fwd_bfly(frame_image(img, tl), fft_frame_skew(tl, TILE), b, w1, w2, w3);
    __syncthreads();
  }
}

template <int TILE>
__device__ inline void inverse_passes(cf* img, int nf, const float* __restrict__ tab) {
  for (int p = FFT_PASSES - 1; p >= 0; --p) {
    const FftBfly b = fft_bfly(p, threadIdx.x);
    const cf w1 = ld_cf(tab, FFT_TAB_TW, b.twi), w2 = ld_cf(tab, FFT_TAB_TW, 2 * b.twi), w3 = ld_cf(tab, FFT_TAB_TW, 3 * b.twi);
    for (int tl = 0; tl < nf; ++tl) fft_inv_bfly(frame_image(img, tl), fft_frame_skew(tl, TILE), b, w1, w2, w3);
    __syncthreads();
  }
}

// Where a row's live column count, strength and bias come from: n_samples and arrays (vsp_denoise) ...
struct OneShotRows {
  const int64_t* n_samples; const float* bias; const float* strength; int L_max, hop, spec;
  __device__ long live(int b) const {
    long n = n_samples[b];
    n = n < 0 ? 0 : (n > L_max ? (long)L_max : n);
    return stft_ragged_frames(n, FFT_N, hop);
  }
  __device__ float strength_of(int b) const { return strength[b]; }
  __device__ const float* bias_of(int b) const { return bias + (size_t)b * spec; }
};
// ... or descriptors by value (vsp_denoise_rows)
struct WindowRows {
  DenoiseSubRows rows;
  __device__ long live(int b) const { return rows.r[b].Tw; }
  __device__ float strength_of(int b) const { return rows.r[b].strength; }
  __device__ const float* bias_of(int b) const { return rows.r[b].bias; }
};

// F -> V: window, forward, split, subtraction with strength * bias[r], inverse split, inverse, window.  RI stays in LDS.
// f == v is allowed: a block reads its tile's columns before it writes them, and no other block touches them.
template <int TILE, class Rows>
__global__ void __launch_bounds__(FFT_THREADS) fft_denoise_kernel(const float* f, long f_bs, long f_cs, float* v, long v_bs,
                                                                  long v_cs, const float* __restrict__ tab, const Rows rows) {
  extern __shared__ cf img[];
  const int b = blockIdx.y, t0 = blockIdx.x * TILE;
  const long live = rows.live(b);
  if (t0 >= live) return;      // (uniform over the block) a dead tile, or a row of no samples
  const int nf = live - t0 < TILE ? (int)(live - t0) : TILE;
  stage_frames<TILE>(img, f + (size_t)b * f_bs, f_cs, t0, nf, tab + FFT_TAB_WA);
  __syncthreads();
  forward_passes<TILE>(img, nf, tab);
  const float s = rows.strength_of(b);
  const float* bias = rows.bias_of(b);
  for (int j = threadIdx.x; j < FFT_SPLIT_ITEMS; j += FFT_THREADS) {
    const int k = fft_split_bin(j), pk = fft_split_pos(k), pm = fft_split_pair(k);
    const cf w = ld_cf(tab, FFT_TAB_SPLIT, k);
    const float thr_k = s * bias[k], thr_m = s * bias[FFT_M - k];
    for (int tl = 0; tl < nf; ++tl) {
      cf* z = frame_image(img, tl);
      const int skew = fft_frame_skew(tl, TILE), sk = fft_slot(skew, pk), sm = fft_slot(skew, pm);
      cf xk, xm, za, zb;
      fft_split_fwd(z[sk], z[sm], w, &xk, &xm);
      fft_split_inv(fft_subtract(xk, thr_k), fft_subtract(xm, thr_m), w, &za, &zb);
      z[sk] = za;
      if (k != 0 && k != FFT_M / 2) z[sm] = zb;
    }
  }
  __syncthreads();
  inverse_passes<TILE>(img, nf, tab);
  store_frames<TILE>(img, v + (size_t)b * v_bs, v_cs, t0, nf, tab + FFT_TAB_WS);
}

// The live columns of row b where the caller's n_samples say so, else all T_max of them (the bias: every column a speaker).
__device__ inline long live_columns(const int64_t* n_samples, int b, int L_max, int hop, int T_max) {
  if (!n_samples) return T_max;
  long n = n_samples[b];
  n = n < 0 ? 0 : (n > L_max ? (long)L_max : n);
  return stft_ragged_frames(n, FFT_N, hop);
}

// F -> RI [B][2 spec][T]: rows 0 .. M real, then imaginary; bins 0 and M are real (their imaginary rows are 0).
template <int TILE>
__global__ void __launch_bounds__(FFT_THREADS) fft_forward_kernel(const float* __restrict__ f, long f_bs, long f_cs,
                                                                  float* __restrict__ ri, long r_bs, long r_cs,
                                                                  const int64_t* __restrict__ n_samples,
                                                                  const float* __restrict__ tab, int L_max, int hop, int T_max) {
  extern __shared__ cf img[];
  const int b = blockIdx.y, t0 = blockIdx.x * TILE;
  const long live = live_columns(n_samples, b, L_max, hop, T_max);
  if (t0 >= live) return;
  const int nf = live - t0 < TILE ? (int)(live - t0) : TILE;
  stage_frames<TILE>(img, f + (size_t)b * f_bs, f_cs, t0, nf, tab + FFT_TAB_WA);
  __syncthreads();
  forward_passes<TILE>(img, nf, tab);
  // X[k] and X[M - k] take the slots of Z[k] and Z[M - k]; slot 0 holds (X[0], X[M])
  for (int j = threadIdx.x; j < FFT_SPLIT_ITEMS; j += FFT_THREADS) {
    const int k = fft_split_bin(j), pk = fft_split_pos(k), pm = fft_split_pair(k);
    const cf w = ld_cf(tab, FFT_TAB_SPLIT, k);
    for (int tl = 0; tl < nf; ++tl) {
      cf* z = frame_image(img, tl);
      const int skew = fft_frame_skew(tl, TILE), sk = fft_slot(skew, pk), sm = fft_slot(skew, pm);
      cf xk, xm;
      fft_split_fwd(z[sk], z[sm], w, &xk, &xm);
      if (k == 0) {
        z[sk] = cf{xk.x, xm.x};
      } else {
        z[sk] = xk;
        if (k != FFT_M / 2) z[sm] = xm;
      }
    }
  }
  __syncthreads();
  float* o = ri + (size_t)b * r_bs;
  for (int e = threadIdx.x; e < (FFT_M + 1) * TILE; e += FFT_THREADS) {
    const int tl = e % TILE, r = e / TILE;
    if (tl >= nf) continue;
    const cf x = frame_image(img, tl)[fft_slot(fft_frame_skew(tl, TILE), fft_rev(r & (FFT_M - 1)))];
    o[(size_t)r * r_cs + t0 + tl] = r == FFT_M ? x.y : x.x;
    o[(size_t)(FFT_M + 1 + r) * r_cs + t0 + tl] = (r == 0 || r == FFT_M) ? 0.f : x.y;
  }
}

// RI -> V.  The imaginary parts of bins 0 and M are not used (the specification takes the real part of every term).
template <int TILE>
__global__ void __launch_bounds__(FFT_THREADS) fft_inverse_kernel(const float* __restrict__ ri, long r_bs, long r_cs,
                                                                  float* __restrict__ v, long v_bs, long v_cs,
                                                                  const int64_t* __restrict__ n_samples,
                                                                  const float* __restrict__ tab, int L_max, int hop, int T_max) {
  extern __shared__ cf img[];
  const int b = blockIdx.y, t0 = blockIdx.x * TILE;
  const long live = live_columns(n_samples, b, L_max, hop, T_max);
  if (t0 >= live) return;
  const int nf = live - t0 < TILE ? (int)(live - t0) : TILE;
  const float* x = ri + (size_t)b * r_bs;
  for (int e = threadIdx.x; e < (FFT_M + 1) * TILE; e += FFT_THREADS) {
    const int tl = e % TILE, r = e / TILE;
    if (tl >= nf) continue;
    const float re = x[(size_t)r * r_cs + t0 + tl];
    cf* z = frame_image(img, tl);
    const int skew = fft_frame_skew(tl, TILE);
    if (r == 0) {
      z[fft_slot(skew, 0)].x = re;
    } else if (r == FFT_M) {
      z[fft_slot(skew, 0)].y = re;
    } else {
      z[fft_slot(skew, fft_rev(r))] = cf{re, x[(size_t)(FFT_M + 1 + r) * r_cs + t0 + tl]};
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < FFT_SPLIT_ITEMS; j += FFT_THREADS) {
    const int k = fft_split_bin(j), pk = fft_split_pos(k), pm = fft_split_pair(k);
    const cf w = ld_cf(tab, FFT_TAB_SPLIT, k);
    for (int tl = 0; tl < nf; ++tl) {
      cf* z = frame_image(img, tl);
      const int skew = fft_frame_skew(tl, TILE), sk = fft_slot(skew, pk), sm = fft_slot(skew, pm);
      const cf a = z[sk], c = z[sm];
      cf za, zb;
      fft_split_inv(k ? a : cf{a.x, 0.f}, k ? c : cf{a.y, 0.f}, w, &za, &zb);
      z[sk] = za;
      if (k != 0 && k != FFT_M / 2) z[sm] = zb;
    }
  }
  __syncthreads();
  inverse_passes<TILE>(img, nf, tab);
  store_frames<TILE>(img, v + (size_t)b * v_bs, v_cs, t0, nf, tab + FFT_TAB_WS);
}

// Frames a block: 8 fit the 64 KiB of a framing block (stft_framing.h) and leave two blocks a CU; 16 need the opt-in above
// 64 KiB and leave one.  Measured (profiles/r27_denoiser_fft.txt); VSP_FFT_TILE = 4 / 8 / 16 is the experiment's switch.
int fft_tile() {
  static const int tile = [] {
    const char* e = std::getenv("VSP_FFT_TILE");
    const int t = e ? std::atoi(e) : 0;
    return t == 4 || t == 8 || t == 16 ? t : 8;
  }();
  return tile;
}

template <class Kern, class... Args>
hipError_t launch_tiled(Kern kern, std::atomic<uint64_t>& done, int tile, int B, int T_max, hipStream_t s, Args... args) {
  const int lds = tile * FFT_M * (int)sizeof(cf);
  if (lds > FR_LDS_BYTES) {
    const hipError_t e = set_max_dynamic_lds(reinterpret_cast<const void*>(kern), lds, done);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kern, dim3((T_max + tile - 1) / tile, B), dim3(FFT_THREADS), lds, s, args...);
  return hipGetLastError();
}

bool bad_operand(const void* p, long bs, long cs, int rows, int T_max) { return !p || cs < T_max || bs < (long)rows * cs; }

template <class Rows>
hipError_t launch_denoise(const float* f, long f_bs, long f_cs, float* v, long v_bs, long v_cs, const float* tab, const Rows& rows,
                          int B, int T_max, hipStream_t s) {
  static std::atomic<uint64_t> done{0};
  switch (fft_tile()) {
    case 4: return launch_tiled(fft_denoise_kernel<4, Rows>, done, 4, B, T_max, s, f, f_bs, f_cs, v, v_bs, v_cs, tab, rows);
    case 16: return launch_tiled(fft_denoise_kernel<16, Rows>, done, 16, B, T_max, s, f, f_bs, f_cs, v, v_bs, v_cs, tab, rows);
    default: return launch_tiled(fft_denoise_kernel<8, Rows>, done, 8, B, T_max, s, f, f_bs, f_cs, v, v_bs, v_cs, tab, rows);
  }
}

}  // namespace

hipError_t launch_fft_denoise(const float* f, long f_bs, long f_cs, float* v, long v_bs, long v_cs, const float* tab,
                              const int64_t* n_samples, const float* bias, const float* strength, int B, int L_max, int n_fft,
                              int hop, int spec_ch, int T_max, hipStream_t s) {
  if (n_fft != FFT_N || spec_ch != FFT_M + 1 || hop <= 0 || hop > n_fft || !tab || !n_samples || !bias || !strength || B <= 0 ||
      B > 65535 || T_max <= 0 || L_max <= 0 || bad_operand(f, f_bs, f_cs, n_fft, T_max) || bad_operand(v, v_bs, v_cs, n_fft, T_max) ||
      stft_ragged_frames(L_max, n_fft, hop) > T_max)      // (a row's live count is T(min(n_b, L_max)) <= T_max: no column outside)
    return hipErrorInvalidValue;
  return launch_denoise(f, f_bs, f_cs, v, v_bs, v_cs, tab, OneShotRows{n_samples, bias, strength, L_max, hop, spec_ch}, B, T_max, s);
}

hipError_t launch_fft_denoise_rows(const float* f, long f_bs, long f_cs, float* v, long v_bs, long v_cs, const float* tab,
                                   const DenoiseSubRows& rows, int B, int n_fft, int spec_ch, int T_max, hipStream_t s) {
  if (n_fft != FFT_N || spec_ch != FFT_M + 1 || !tab || B <= 0 || B > STREAM_ROWS_MAX || T_max <= 0 ||
      bad_operand(f, f_bs, f_cs, n_fft, T_max) || bad_operand(v, v_bs, v_cs, n_fft, T_max))
    return hipErrorInvalidValue;
  for (int b = 0; b < B; ++b)
    if (!rows.r[b].bias || rows.r[b].Tw <= 0 || rows.r[b].Tw > T_max) return hipErrorInvalidValue;
  WindowRows w;
  w.rows = rows;
  return launch_denoise(f, f_bs, f_cs, v, v_bs, v_cs, tab, w, B, T_max, s);
}

hipError_t launch_fft_forward(const float* f, long f_bs, long f_cs, float* ri, long r_bs, long r_cs, const float* tab,
                              const int64_t* n_samples, int B, int L_max, int n_fft, int hop, int T_max, hipStream_t s) {
  if (n_fft != FFT_N || hop <= 0 || hop > n_fft || !tab || B <= 0 || B > 65535 || T_max <= 0 ||
      bad_operand(f, f_bs, f_cs, n_fft, T_max) || bad_operand(ri, r_bs, r_cs, 2 * (FFT_M + 1), T_max) ||
      (n_samples && (L_max <= 0 || stft_ragged_frames(L_max, n_fft, hop) > T_max)))
    return hipErrorInvalidValue;
  static std::atomic<uint64_t> done{0};
  switch (fft_tile()) {
    case 4: return launch_tiled(fft_forward_kernel<4>, done, 4, B, T_max, s, f, f_bs, f_cs, ri, r_bs, r_cs, n_samples, tab, L_max, hop, T_max);
    case 16: return launch_tiled(fft_forward_kernel<16>, done, 16, B, T_max, s, f, f_bs, f_cs, ri, r_bs, r_cs, n_samples, tab, L_max, hop, T_max);
    default: return launch_tiled(fft_forward_kernel<8>, done, 8, B, T_max, s, f, f_bs, f_cs, ri, r_bs, r_cs, n_samples, tab, L_max, hop, T_max);
  }
}

hipError_t launch_fft_inverse(const float* ri, long r_bs, long r_cs, float* v, long v_bs, long v_cs, const float* tab,
                              const int64_t* n_samples, int B, int L_max, int n_fft, int hop, int T_max, hipStream_t s) {
  if (n_fft != FFT_N || hop <= 0 || hop > n_fft || !tab || B <= 0 || B > 65535 || T_max <= 0 ||
      bad_operand(ri, r_bs, r_cs, 2 * (FFT_M + 1), T_max) || bad_operand(v, v_bs, v_cs, n_fft, T_max) ||
      (n_samples && (L_max <= 0 || stft_ragged_frames(L_max, n_fft, hop) > T_max)))
    return hipErrorInvalidValue;
  static std::atomic<uint64_t> done{0};
  switch (fft_tile()) {
    case 4: return launch_tiled(fft_inverse_kernel<4>, done, 4, B, T_max, s, ri, r_bs, r_cs, v, v_bs, v_cs, n_samples, tab, L_max, hop, T_max);
    case 16: return launch_tiled(fft_inverse_kernel<16>, done, 16, B, T_max, s, ri, r_bs, r_cs, v, v_bs, v_cs, n_samples, tab, L_max, hop, T_max);
    default: return launch_tiled(fft_inverse_kernel<8>, done, 8, B, T_max, s, ri, r_bs, r_cs, v, v_bs, v_cs, n_samples, tab, L_max, hop, T_max);
  }
}

}  // namespace vsp
