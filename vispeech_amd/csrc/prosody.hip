// Prosody from a recording (include/vispeech_hip.h, "prosody"): per-frame F0 by Boersma's 1993
// autocorrelation method and per-frame energy (the L2 norm of a 1280-point one-sided STFT column), then both averaged over
// each phoneme's frames -- what the reference's data preparation (f0energy.py) computes with parselmouth and librosa on the
// CPU, restated as three launches.  Everything is ragged over the batch: row b is audio[b][0 .. n_b), nothing at or behind
// n_b is read (loads are predicated, not selected after the fact), outputs behind a row's frames or phonemes are exact
// zeros, and a row's result is a function of the row alone.
//
//   row_peak_kernel   one block per row, ONE pass: sum (double), min and max -> mean and gpk = max |x - mean|
//                     (= max(fl(max - mean), fl(mean - min)): fl(x - mean) is monotone in x, so this IS the maximum of the
//                     rounded differences).
//   contour_kernel    one block = PR_FPB consecutive frames of a row, one wave per frame.  The block stages the raw span of
//                     its frames once (consecutive frames share W - hop samples); each wave builds its mean-free windowed
//                     frame a[] in LDS, zero padded behind W, and runs r_a(t) = sum_n a[n] a[n + t] for the lags
//                     t0 + 4 lane + {0..3} (+ 256 per further lag block): per step of four n, ONE ds_read_b128 of a[n .. n+4)
//                     at the same address in every lane (a broadcast), ONE ds_read_b128 of the next four a[n + t ..]
//                     (consecutive across lanes, conflict free) and 16 FMAs; the sliding operand stays in registers.
//                     Lag 0 is the frame's sum of squares.  Candidates, parabola, strengths and the argmax are a wave
//                     reduction.  The three energy sums of the same frame (Parseval: no DFT) ride in the same launch.
//                     Bound: the vector FMA pipe, the LDS close behind -- two lag blocks share each broadcast quad, 3 LDS
//                     reads (12 LDS cycles) per 32 FMAs (64 SIMD cycles), three quarters of the LDS's cycles with four
//                     SIMDs issuing -- and nothing here is a matrix product an MFMA could take in fp32 faster.
//                     A second instantiation (CAND) writes every frame's strongest candidates instead of its decision, for
//   path_kernel       one wave per row (section 4n): the best path through the frames' candidates, Boersma's step 4 -- forward
//                     with back-pointers through the workspace, backward in LDS.  No sinc interpolation of the peaks.
//   phoneme_kernel    one wave per row: previous voiced frame by a forward wave64 max-scan, next voiced frame by a backward
//                     min-scan, linear interpolation in between, then one lane per phoneme sums its OWN frames (no
//                     prefix-sum differences: they would lose the digits the 1e-4 gate needs).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "kernels.h"
#include "model.h"
#include "op_host.h"

namespace {

constexpr int PR_FS = VSP_PROSODY_FS, PR_NFFT = VSP_PROSODY_NFFT, PR_MIN_SAMPLES = PR_NFFT / 2 + 1;
constexpr int PR_FPB = 4;               // frames (= waves) per block of the contour kernel
constexpr int PR_LAGS_PER_WAVE = 256;   // four consecutive lags per lane
constexpr int PR_MAX_HOP = 2048;
constexpr int PR_MAX_B = 65535;
constexpr int64_t PR_MAX_SAMPLES = (int64_t)1 << 30;
constexpr int PR_SLOTS = VSP_PROSODY_MAX_CANDIDATES + 1;   // floats of a frame in the candidate tables: 64 bytes

struct Plan {
  int W;      // samples of an analysis frame: round(3 fs / floor), made even
  int W4;     // ... rounded up to a multiple of 4 (the zero padding starts at W)
  int tmin, tmax;   // candidate lags [tmin, tmax] = [floor(fs / ceiling), ceil(fs / floor)]
  int t0;     // first lag of lane 0: (tmin - 1) rounded down to a multiple of 4
  int LB;     // lag blocks of 256: the lags t0 .. t0 + 256 LB - 1 cover tmin - 1 .. tmax + 1
  int NA;     // floats of one wave's frame buffer: W4 + t0 + 256 LB + 4
  vsp_prosody_params p;
};

const vsp_prosody_params kDefaults = {80.f, 750.f, 0.6f, 0.03f, 0.01f};

// 0: ok; else the refused field (1 floor, 2 ceiling, 3 the thresholds)
int make_plan(const vsp_prosody_params* params, Plan& pl) {
  const vsp_prosody_params p = params ? *params : kDefaults;
  if (!(p.floor_hz >= 40.f)) return 1;
  if (!(p.ceiling_hz <= (float)PR_FS / 4) || !(p.ceiling_hz > p.floor_hz)) return 2;
  if (!(p.voicing_threshold > -1.f && p.voicing_threshold < 1e6f) || !(p.silence_threshold > 0.f && p.silence_threshold < 1e6f) ||
      !(std::fabs(p.octave_cost) < 1e6f))
    return 3;
  pl.p = p;
  int W = (int)std::floor(3.0 * PR_FS / (double)p.floor_hz + 0.5);
  W += W & 1;
  pl.W = W;
  pl.W4 = (W + 3) & ~3;
  pl.tmin = (int)std::floor((double)PR_FS / (double)p.ceiling_hz);
  pl.tmax = (int)std::ceil((double)PR_FS / (double)p.floor_hz);
  pl.t0 = (pl.tmin - 1) & ~3;
  pl.LB = (pl.tmax + 2 - pl.t0 + PR_LAGS_PER_WAVE - 1) / PR_LAGS_PER_WAVE;
  pl.NA = pl.W4 + pl.t0 + PR_LAGS_PER_WAVE * pl.LB + 4;
  return 0;
}

// ------------------------------------------------------------------------------------------------------------ row peak
struct RowStat { float mean, gpk; };

__global__ void __launch_bounds__(1024) row_peak_kernel(const float* __restrict__ audio, int64_t a_bs,
                                                        const int64_t* __restrict__ n_samples, RowStat* __restrict__ stat) {
  __shared__ double s_sum[16];
  __shared__ float s_min[16], s_max[16];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t n = n_samples[b];
  const float* row = audio + (size_t)b * a_bs;
  double sum = 0.0;
  float mn = INFINITY, mx = -INFINITY;
#pragma unroll 8
  for (int64_t i = tid; i < n; i += 1024) {                        // (unrolled: eight loads in flight; the order of the adds stays)
    const float v = row[i];
    sum += (double)v;
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    sum += __shfl_xor(sum, off);
    mn = fminf(mn, __shfl_xor(mn, off));
    mx = fmaxf(mx, __shfl_xor(mx, off));
  }
  if (lane == 0) { s_sum[wave] = sum; s_min[wave] = mn; s_max[wave] = mx; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 16; ++w) { sum += s_sum[w]; mn = fminf(mn, s_min[w]); mx = fmaxf(mx, s_max[w]); }
    const float mean = n > 0 ? (float)(sum / (double)n) : 0.f;
    // (a NaN sample makes gpk NaN or 0: every comparison below then says "unvoiced")
    stat[b] = RowStat{mean, n > 0 ? fmaxf(mx - mean, mean - mn) : 0.f};
  }
}

// ------------------------------------------------------------------------------------------------------------ contours
struct ContourArgs {
  const float* audio; int64_t a_bs;
  const int64_t* n_samples;      // [B] (device copy of the host's array)
  const RowStat* stat;           // [B]
  const float* hann;             // [PR_NFFT] periodic Hann
  const float* win;              // [W] the analysis window w_n = 0.5 - 0.5 cos(2 pi (n + 0.5) / W)
  const float* inv_rw;           // [256 LB] r_w(0) / r_w(t0 + i), 0 where the lag is not used
  float* f0; float* energy;      // [B][F_max]
  int64_t* frames;               // [B]
  int F_max, hop;
  int W, W4, tmin, tmax, t0, LB, NA;
  int rbuf_off;                  // first float of the lag buffers in the block's LDS
  float fs, floor_hz, vt, st_scale, oc;     // st_scale = silence_threshold / (1 + voicing_threshold)
  // the candidate instantiation only (appended: the fields above keep their places)
  float* cand_f; float* cand_s;  // [B][F_max][PR_SLOTS]
  int n_voiced;                  // voiced slots to fill: max_candidates - 1
};

// Four floats as one value: the hot loop works on whole vectors (shuffles of the two loaded quads, element-wise FMA), so
// that each LDS read stays ONE ds_read_b128 -- written element by element, the compiler takes the vector loads apart into the
// elements each unrolled step uses and puts them together again as 8-byte pairs, a quarter of the LDS rate per byte.
typedef float pr_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ pr_f4 pr_lds128(const float* p) { return *reinterpret_cast<const pr_f4*>(p); }

// acc[j][e] = sum_n a[n] a[n + t], t = the lag sp points at + 256 j + e, for NB lag blocks: per step of four n one
// broadcast quad a[n .. n+4) and, per block, the next quad of the sliding operand (lo | hi = a[n + t .. n + t + 8)).
template <int NB>
__device__ __forceinline__ void pr_autocorr(const float* abuf, const float* sp, int W4, pr_f4 (&acc)[2]) {
  pr_f4 lo[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    lo[j] = pr_lds128(sp + PR_LAGS_PER_WAVE * j);
    acc[j] = pr_f4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll 2
  for (int i = 0; i < W4; i += 4) {
    const pr_f4 c = pr_lds128(abuf + i);                                     // the same address in every lane
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const pr_f4 hi = pr_lds128(sp + PR_LAGS_PER_WAVE * j + i + 4);
      acc[j] = __builtin_elementwise_fma(pr_f4(c.x), lo[j], acc[j]);
      acc[j] = __builtin_elementwise_fma(pr_f4(c.y), __builtin_shufflevector(lo[j], hi, 1, 2, 3, 4), acc[j]);
      acc[j] = __builtin_elementwise_fma(pr_f4(c.z), __builtin_shufflevector(lo[j], hi, 2, 3, 4, 5), acc[j]);
      acc[j] = __builtin_elementwise_fma(pr_f4(c.w), __builtin_shufflevector(lo[j], hi, 3, 4, 5, 6), acc[j]);
      lo[j] = hi;
    }
  }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  return v;
}

// grid (ceil(F_max / PR_FPB), B), 64 PR_FPB threads.  Dynamic LDS (floats): [raw span: W + (PR_FPB - 1) hop, to a multiple
// of 4] [PR_FPB frame buffers of NA] and PR_FPB lag buffers of 256 LB + 4, over the raw span or behind.  Control flow is uniform over the block: a wave
// whose frame lies behind the row's frames computes on the zeros the staging selected and stores 0.
// CAND: instead of the frame's decision, its PR_SLOTS (f, delta) pairs for the path finder (section 4n): slot 0 the
// unvoiced candidate (0, U), slots 1 .. n_voiced the strongest maxima in descending (S, then ascending lag), the rest
// (0, -inf); exact zeros in both tables behind the row's frames.
template <bool CAND>
__global__ void __launch_bounds__(64 * PR_FPB) contour_kernel(const ContourArgs g) {
  extern __shared__ __align__(16) float pr_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y, k0 = blockIdx.x * PR_FPB, k = k0 + wave;
  const int64_t n = g.n_samples[b];
  const int64_t F = n / g.hop + 1;
  if (tid == 0 && blockIdx.x == 0) g.frames[b] = F;
  float* f0_out = g.f0 + (size_t)b * g.F_max;
  float* en_out = g.energy + (size_t)b * g.F_max;
  if (k0 >= F) {                                                   // (uniform) the whole block lies behind the row's frames
    if constexpr (CAND) {
      if (lane < PR_SLOTS && k < g.F_max) {
        const size_t e = ((size_t)b * g.F_max + k) * PR_SLOTS + lane;
        g.cand_f[e] = 0.f;
        g.cand_s[e] = 0.f;
      }
      if (lane == 0 && k < g.F_max) en_out[k] = 0.f;
    } else {
      if (lane == 0 && k < g.F_max) { f0_out[k] = 0.f; en_out[k] = 0.f; }
    }
    return;
  }
  const int span = g.W + (PR_FPB - 1) * g.hop, span4 = (span + 3) & ~3;
  float* raw = pr_smem;
  float* abuf = pr_smem + span4 + (size_t)wave * g.NA;
  // (the lag buffers lie over the raw span where they fit: the span is dead once the frames are built, a barrier before)
  float* rbuf = pr_smem + g.rbuf_off + (size_t)wave * (PR_LAGS_PER_WAVE * g.LB + 4);
  const float* __restrict__ row = g.audio + (size_t)b * g.a_bs;
  const bool live = k < F;                                         // (uniform over the wave)

  // the raw span of the block's frames, zeros outside the row
  const int64_t first = (int64_t)k0 * g.hop - g.W / 2;
  for (int i = tid; i < span; i += 64 * PR_FPB) {
    const int64_t j = first + i;
    float v = 0.f;
    if (j >= 0 && j < n) v = row[j];
    raw[i] = v;
  }

  // energy of frame k: the frame's 1280 samples around hop k, reflected at the row's own two ends (n >= 641: one reflection
  // reaches every index), times the periodic Hann window; sum s^2, sum s, sum (-1)^j s_j
  float energy = 0.f;
  if (live) {
    float q = 0.f, s0 = 0.f, s1 = 0.f;
    const int64_t e_first = (int64_t)k * g.hop - PR_NFFT / 2;
    for (int j = lane; j < PR_NFFT; j += 64) {                     // (64 is even: a lane's samples all have the parity of the lane)
      int64_t i = e_first + j;
      if (i < 0) i = -i;
      if (i >= n) i = 2 * (n - 1) - i;
      const float s = row[i] * g.hann[j];
      q = fmaf(s, s, q);
      s0 += s;
      s1 += s;
    }
    if (lane & 1) s1 = -s1;
    q = wave_sum(q); s0 = wave_sum(s0); s1 = wave_sum(s1);
    energy = sqrtf(0.5f * fmaf((float)PR_NFFT, q, fmaf(s0, s0, s1 * s1)));
  }
  __syncthreads();

  // the frame: mean over its W samples (zeros outside the row included), local peak, window, zero padding
  const float* x = raw + wave * g.hop;
  float m = 0.f;
  for (int i = lane; i < g.W; i += 64) m += x[i];
  const float mean = wave_sum(m) / (float)g.W;
  float lpk = 0.f, ra0 = 0.f;
  for (int i = lane; i < g.NA; i += 64) {
    float a = 0.f;
    if (i < g.W) {
      const float s = x[i] - mean;
      lpk = fmaxf(lpk, fabsf(s));
      a = s * g.win[i];
      ra0 = fmaf(a, a, ra0);
    }
    abuf[i] = a;
  }
  lpk = wave_max(lpk);
  ra0 = wave_sum(ra0);
  __syncthreads();

  // autocorrelation: lane l of lag block lb owns the lags t0 + 256 lb + 4 l + {0, 1, 2, 3}
  // and, two lag blocks at a time, the same four of the next block: one broadcast read then feeds 32 FMAs (3 LDS reads per
  // 32 FMAs instead of 4: with every SIMD of the CU issuing FMAs at its rate, 4 would ask the LDS for all of its cycles)
  const float inv0 = ra0 > 0.f ? 1.f / ra0 : 0.f;
  for (int lb = 0; lb < g.LB; lb += 2) {
    const float* sp = abuf + g.t0 + PR_LAGS_PER_WAVE * lb + 4 * lane;
    const int li = PR_LAGS_PER_WAVE * lb + 4 * lane;
    pr_f4 acc[2];
    if (lb + 1 < g.LB) pr_autocorr<2>(abuf, sp, g.W4, acc);                  // (uniform over the block)
    else pr_autocorr<1>(abuf, sp, g.W4, acc);
    // r(t) = (r_a(t) / r_a(0)) * (r_w(0) / r_w(t)); the table holds 0 for lags outside [tmin - 1, tmax + 1]
    for (int j = 0; j < 2 && lb + j < g.LB; ++j) {
      const float4 iw = *reinterpret_cast<const float4*>(g.inv_rw + li + PR_LAGS_PER_WAVE * j);
      *reinterpret_cast<float4*>(rbuf + li + PR_LAGS_PER_WAVE * j) =
          make_float4(acc[j].x * inv0 * iw.x, acc[j].y * inv0 * iw.y, acc[j].z * inv0 * iw.z, acc[j].w * inv0 * iw.w);
    }
  }
  __syncthreads();

  // candidates: local maxima of r at the integer lags of [tmin, tmax], refined by a parabola; the strongest wins, the
  // lowest lag among equals
  float best_s = -INFINITY, best_f = 0.f;
  int best_t = 0x7fffffff;
  if constexpr (!CAND) {
    for (int t = g.tmin + lane; t <= g.tmax; t += 64) {
      const int i = t - g.t0;
      const float rm = rbuf[i - 1], r0 = rbuf[i], rp = rbuf[i + 1];
      if (r0 > rm && r0 >= rp) {
        const float d = 0.5f * (rm - rp) / (rm - 2.f * r0 + rp);
        const float R = r0 - 0.25f * (rm - rp) * d;
        const float f = g.fs / ((float)t + d);
        const float S = R + g.oc * log2f(f / g.floor_hz);
        if (S > best_s) { best_s = S; best_f = f; best_t = t; }    // (t ascends within a lane: the first of equals stays)
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const float os = __shfl_xor(best_s, off), of = __shfl_xor(best_f, off);
      const int ot = __shfl_xor(best_t, off);
      if (os > best_s || (os == best_s && ot < best_t)) { best_s = os; best_f = of; best_t = ot; }
    }
    if (lane == 0 && k < g.F_max) {
      const float gpk = g.stat[b].gpk;
      float f0 = 0.f;
      if (live && ra0 > 0.f && gpk > 0.f && best_t != 0x7fffffff) {
        const float U = g.vt + fmaxf(0.f, 2.f - (lpk / gpk) / g.st_scale);
        if (best_s > U) f0 = best_f;
      }
      f0_out[k] = f0;
      en_out[k] = live ? energy : 0.f;
    }
  } else {
    // The strongest n_voiced maxima, in order.  Every lane evaluates its lags ONCE and keeps (S, f) in the wave's own frame
    // buffer -- dead since the barrier above, and 2 (tmax - tmin + 1) < W floats always fit -- where it reads back only
    // what it wrote itself.  Then one round of the wave arg-max per slot, each restricted to the maxima behind the last
    // winner in (S descending, lag ascending): lane r keeps the winner of round r.
    const float gpk = g.stat[b].gpk;
    const bool alive = live && ra0 > 0.f && gpk > 0.f;             // (uniform over the wave)
    const int nl = g.tmax - g.tmin + 1;
    float* cs = abuf;
    float* cf = abuf + nl;
    float my_f = 0.f, my_s = -INFINITY;
    if (alive) {
      for (int t = g.tmin + lane; t <= g.tmax; t += 64) {
        // (the expressions of the decision above, letter for letter: with both path costs 0 the two are held to the same bits)
        const int i = t - g.t0;
        const float rm = rbuf[i - 1], r0 = rbuf[i], rp = rbuf[i + 1];
        float cand_f = 0.f, cand_S = -INFINITY;
        if (r0 > rm && r0 >= rp) {
          const float d = 0.5f * (rm - rp) / (rm - 2.f * r0 + rp);
          const float R = r0 - 0.25f * (rm - rp) * d;
          const float f = g.fs / ((float)t + d);
          const float S = R + g.oc * log2f(f / g.floor_hz);
          cand_f = f;
          cand_S = S;
        }
        cs[t - g.tmin] = cand_S;
        cf[t - g.tmin] = cand_f;
      }
      float last_s = INFINITY;
      int last_t = -1;
      for (int r = 1; r <= g.n_voiced; ++r) {
        best_s = -INFINITY; best_f = 0.f; best_t = 0x7fffffff;
        for (int t = g.tmin + lane; t <= g.tmax; t += 64) {
          const float S = cs[t - g.tmin];
          if ((S < last_s || (S == last_s && t > last_t)) && S > best_s) { best_s = S; best_f = cf[t - g.tmin]; best_t = t; }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
          const float os = __shfl_xor(best_s, off), of = __shfl_xor(best_f, off);
          const int ot = __shfl_xor(best_t, off);
          if (os > best_s || (os == best_s && ot < best_t)) { best_s = os; best_f = of; best_t = ot; }
        }
        if (best_t == 0x7fffffff) break;                           // (uniform) no maximum is left
        if (lane == r) { my_f = best_f; my_s = best_s; }
        last_s = best_s;
        last_t = best_t;
      }
    }
    if (lane == 0) {
      // (a dead frame -- r_a(0) = 0 or gpk = 0 -- has the unvoiced candidate alone, at the formula's value for lpk = 0)
      my_s = g.vt + (alive ? fmaxf(0.f, 2.f - (lpk / gpk) / g.st_scale) : 2.f);
    }
    if (lane < PR_SLOTS && k < g.F_max) {
      const size_t e = ((size_t)b * g.F_max + k) * PR_SLOTS + lane;
      g.cand_f[e] = live ? my_f : 0.f;
      g.cand_s[e] = live ? my_s : 0.f;
    }
    if (lane == 0 && k < g.F_max) en_out[k] = live ? energy : 0.f;
  }
}

// ------------------------------------------------------------------------------------------------------------ the path
// Section 4n.  One wave per row, grid B.  Lane = candidate c (lane & 15) x group g (lane >> 4) of the four previous
// candidates 4 g .. 4 g + 3: a lane takes the best of its four in registers, two cross-lane steps (xor 16, 32) finish
// max_p (s(p) - T(p, c)), the lowest p among equals.  A chunk of PR_CH frames is staged in LDS as (log2 f, delta) -- the next
// chunk's loads are in flight while this one runs -- so a voiced transition is |difference| times a constant, computed from
// LDS alone and so ahead of the chain; serial per frame are the subtract, the max steps, the add, the max over the 16
// candidates that normalises the frame (the best score is exactly 0.0f) and the four shuffles that hand every lane its
// group's new scores.  Back-pointers: one byte per (frame, candidate), collected in LDS and flushed per chunk as 16 bytes
// per lane.  Backward: the chunks come back the same way (every lane reads the 16 bytes it wrote) and the 64 frames are
// walked in LDS, by every lane alike (broadcast reads), so the walk costs an LDS read per frame, not a trip to memory.
// Frames at or behind frames[b] are neither read nor written, but for the zeros behind the row in f0.
constexpr int PR_CH = 64;

struct PathArgs {
  const float* cand_f; const float* cand_s;   // [B][F_max][PR_SLOTS]
  const int32_t* frames;                      // [B]
  uint8_t* bp;                                // [B][F_max][PR_SLOTS] scratch: the best previous candidate
  float* f0;                                  // [B][F_max]
  int F_max;
  float c_oct, c_vuv;                         // octave_jump_cost kappa, voiced_unvoiced_cost kappa
};

__device__ __forceinline__ float pr_log2_or_unvoiced(float f) { return f > 0.f ? log2f(f) : -INFINITY; }

__global__ void __launch_bounds__(64) path_kernel(const PathArgs g) {
  __shared__ __align__(16) float s_lf[PR_CH][PR_SLOTS];
  __shared__ __align__(16) float s_d[PR_CH][PR_SLOTS];
  __shared__ __align__(16) uint8_t s_bp[PR_CH][PR_SLOTS];
  const int b = blockIdx.x, lane = threadIdx.x, c = lane & 15, grp = lane >> 4;
  const int F = g.frames[b];
  const size_t row = (size_t)b * g.F_max;
  const float* __restrict__ cand_f = g.cand_f + row * PR_SLOTS;
  const float* __restrict__ cand_s = g.cand_s + row * PR_SLOTS;
  uint8_t* bp = g.bp + row * PR_SLOTS;
  float* f0 = g.f0 + row;
  for (int k = F + lane; k < g.F_max; k += 64) f0[k] = 0.f;

  // a chunk is 1024 (f, delta) pairs: lane l holds the quads (64 i + l), frame 16 i + l / 4, slots 4 (l & 3) ..
  pr_f4 nf[4], ns[4];
  auto fetch = [&](int base) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int fr = base + 16 * i + (lane >> 2);
      nf[i] = pr_f4{0.f, 0.f, 0.f, 0.f};
      ns[i] = nf[i];
      if (fr < F) {
        const size_t e = (size_t)fr * PR_SLOTS + 4 * (lane & 3);
        nf[i] = *reinterpret_cast<const pr_f4*>(cand_f + e);
        ns[i] = *reinterpret_cast<const pr_f4*>(cand_s + e);
      }
    }
  };
  fetch(0);
  float sp[4] = {0.f, 0.f, 0.f, 0.f};       // the previous frame's scores of this lane's group
  pr_f4 lfq = {0.f, 0.f, 0.f, 0.f};         // ... and their log2 f
  float s = 0.f;
  for (int base = 0; base < F; base += PR_CH) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int fr = 16 * i + (lane >> 2), sl = 4 * (lane & 3);
      *reinterpret_cast<pr_f4*>(&s_lf[fr][sl]) = pr_f4{pr_log2_or_unvoiced(nf[i].x), pr_log2_or_unvoiced(nf[i].y),
                                                       pr_log2_or_unvoiced(nf[i].z), pr_log2_or_unvoiced(nf[i].w)};
      *reinterpret_cast<pr_f4*>(&s_d[fr][sl]) = ns[i];
    }
    __syncthreads();
    if (base + PR_CH < F) fetch(base + PR_CH);
    const int n = min(PR_CH, F - base);
    for (int i = 0; i < n; ++i) {
      const float my_lf = s_lf[i][c], my_d = s_d[i][c];
      float bv = 0.f;
      int bi = 0;
      if (base + i > 0) {                                          // (uniform)
        const bool uc = my_lf == -INFINITY;
        const float lq[4] = {lfq.x, lfq.y, lfq.z, lfq.w};
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool up = lq[j] == -INFINITY;
          const float cost = (up && uc) ? 0.f : (up || uc) ? g.c_vuv : g.c_oct * fabsf(lq[j] - my_lf);
          v[j] = sp[j] - cost;
        }
        bv = v[0];
        bi = 4 * grp;
#pragma unroll
        for (int j = 1; j < 4; ++j)
          if (v[j] > bv) { bv = v[j]; bi = 4 * grp + j; }
#pragma unroll
        for (int off = 16; off <= 32; off <<= 1) {
          const float ov = __shfl_xor(bv, off);
          const int oi = __shfl_xor(bi, off);
          if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
      }
      s = my_d + bv;
      float m = s;
#pragma unroll
      for (int off = 1; off <= 8; off <<= 1) m = fmaxf(m, __shfl_xor(m, off));
      if (m > -INFINITY) s -= m;                                   // (a frame of -inf alone stays -inf, not NaN)
      if (grp == 0) s_bp[i][c] = (uint8_t)bi;
#pragma unroll
      for (int j = 0; j < 4; ++j) sp[j] = __shfl(s, 4 * grp + j);
      lfq = *reinterpret_cast<const pr_f4*>(&s_lf[i][4 * grp]);
    }
    __syncthreads();
    if (lane < n) *reinterpret_cast<uint4*>(bp + (size_t)(base + lane) * PR_SLOTS) = *reinterpret_cast<const uint4*>(s_bp[lane]);
    __syncthreads();
  }
  // the end: the best candidate of the last frame, the lowest among equals
  int cur = c;
#pragma unroll
  for (int off = 1; off <= 8; off <<= 1) {
    const float os = __shfl_xor(s, off);
    const int oc = __shfl_xor(cur, off);
    if (os > s || (os == s && oc < cur)) { s = os; cur = oc; }
  }
  for (int base = ((F - 1) / PR_CH) * PR_CH; base >= 0; base -= PR_CH) {
    const int n = min(PR_CH, F - base);
    // (lane l wrote these 16 bytes itself: no other thread's store is read)
    if (lane < n) *reinterpret_cast<uint4*>(s_bp[lane]) = *reinterpret_cast<const uint4*>(bp + (size_t)(base + lane) * PR_SLOTS);
    __syncthreads();
    int mine = 0;
    for (int i = n - 1; i >= 0; --i) {
      if (lane == i) mine = cur;
      cur = s_bp[i][cur];
    }
    if (lane < n) f0[base + lane] = cand_f[(size_t)(base + lane) * PR_SLOTS + mine];
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------------------ phonemes
struct PhonemeArgs {
  const float* f0_frames; const float* energy_frames;   // [B][F_max]
  const int32_t* start; const int32_t* dur;             // [B][Tp] first frame and frame count of every phoneme
  const int32_t* frames; const int32_t* lengths;        // [B]
  float* interp;                                        // [B][F_max] scratch: the interpolated contour
  int32_t* prev;                                        // [B][F_max] scratch: previous voiced frame (-1: none)
  float* f0; float* energy;                             // [B][Tp]
  int F_max, Tp;
};

// grid B, one wave.  Frames at or behind frames[b] are not read.
__global__ void __launch_bounds__(64) phoneme_kernel(const PhonemeArgs g) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int F = g.frames[b], Tl = g.lengths[b];
  const float* __restrict__ f0 = g.f0_frames + (size_t)b * g.F_max;
  const float* __restrict__ en = g.energy_frames + (size_t)b * g.F_max;
  float* ip = g.interp + (size_t)b * g.F_max;
  int32_t* pv = g.prev + (size_t)b * g.F_max;

  // forward: the last voiced frame at or before i (inclusive max-scan of voiced ? i : -1, carried across the chunks)
  int carry = -1, first_voiced = 0x7fffffff;
  for (int base = 0; base < F; base += 64) {
    const int i = base + lane;
    int v = (i < F && f0[i] != 0.f) ? i : -1;
    if (v >= 0) first_voiced = min(first_voiced, v);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int o = __shfl_up(v, off);
      if (lane >= off) v = max(v, o);
    }
    v = max(v, carry);
    if (i < F) pv[i] = v;
    carry = __shfl(v, 63);
  }
  const int last_voiced = carry;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) first_voiced = min(first_voiced, __shfl_xor(first_voiced, off));
  const bool interpolate = last_voiced >= 0 && first_voiced != last_voiced;     // two voiced frames or more
  __syncthreads();
  // backward: the first voiced frame at or behind i (inclusive min-scan from the end), then the interpolation
  carry = 0x7fffffff;
  for (int base = ((F - 1) / 64) * 64; base >= 0; base -= 64) {
    const int i = base + lane;
    const float fi = i < F ? f0[i] : 0.f;
    int v = (i < F && fi != 0.f) ? i : 0x7fffffff;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int o = __shfl_down(v, off);
      if (lane + off < 64) v = min(v, o);
    }
    v = min(v, carry);
    if (i < F) {
      float r = fi;
      if (interpolate && fi == 0.f) {
        const int p = pv[i], q = v;
        if (p < 0) r = f0[q];                                       // before the first voiced frame
        else if (q == 0x7fffffff) r = f0[p];                        // behind the last
        else r = f0[p] + (f0[q] - f0[p]) * ((float)(i - p) / (float)(q - p));
      }
      ip[i] = r;
    }
    carry = __shfl(v, 0);
  }
  __syncthreads();
  // one lane per phoneme: the mean of its own frames, summed directly
  for (int j = lane; j < g.Tp; j += 64) {
    float mf = 0.f, me = 0.f;
    if (j < Tl) {
      const int s = g.start[(size_t)b * g.Tp + j], d = g.dur[(size_t)b * g.Tp + j];
      if (d > 0) {
        float af = 0.f, ae = 0.f;
        for (int i = s; i < s + d; ++i) { af += ip[i]; ae += en[i]; }
        mf = af / (float)d;
        me = ae / (float)d;
      }
    }
    g.f0[(size_t)b * g.Tp + j] = mf;
    g.energy[(size_t)b * g.Tp + j] = me;
  }
}

// ------------------------------------------------------------------------------------------------------------ host
// The tables of a plan, in double on the host, stored as float32: the periodic Hann window of the energy frame, the
// analysis window and the reciprocals of its normalised autocorrelation.  One entry is kept (a service uses one plan).
struct Tables {
  int W = 0, t0 = 0, LB = 0, tmin = 0, tmax = 0;
  std::vector<float> host;       // [hann PR_NFFT][win W4][inv_rw 256 LB]
};
std::mutex g_tables_mu;
Tables g_tables;

void build_tables(const Plan& pl, Tables& t) {
  t.W = pl.W; t.t0 = pl.t0; t.LB = pl.LB; t.tmin = pl.tmin; t.tmax = pl.tmax;
  const int nl = PR_LAGS_PER_WAVE * pl.LB;
  t.host.assign((size_t)PR_NFFT + pl.W4 + nl, 0.f);
  const double two_pi = 6.283185307179586476925286766559;
  for (int j = 0; j < PR_NFFT; ++j) t.host[j] = (float)(0.5 - 0.5 * std::cos(two_pi * j / PR_NFFT));
  std::vector<double> w(pl.W);
  for (int i = 0; i < pl.W; ++i) {
    w[i] = 0.5 - 0.5 * std::cos(two_pi * (i + 0.5) / pl.W);
    t.host[PR_NFFT + i] = (float)w[i];
  }
  double r0 = 0.0;
  for (int i = 0; i < pl.W; ++i) r0 += w[i] * w[i];
  for (int lag = pl.tmin - 1; lag <= pl.tmax + 1; ++lag) {
    double r = 0.0;
    for (int i = 0; i + lag < pl.W; ++i) r += w[i] * w[i + lag];
    t.host[(size_t)PR_NFFT + pl.W4 + (lag - pl.t0)] = (float)(r0 / r);
  }
}

using vsp::Call;
using vsp::Ws;

// What each call carves from its workspace (op_host.h); the sizes are the dry passes of these.
struct ContourWs { int64_t* n_samples; RowStat* stat; float* tables; };
ContourWs carve_contour(Ws& ws, int B, const Plan& pl) {      // (a braced list is evaluated in order: so is every carve below)
  return {static_cast<int64_t*>(ws.bytes((size_t)B * sizeof(int64_t))), static_cast<RowStat*>(ws.bytes((size_t)B * sizeof(RowStat))),
          ws.f((size_t)PR_NFFT + pl.W4 + (size_t)PR_LAGS_PER_WAVE * pl.LB)};
}

struct PhonemeWs { int32_t* ints; float* interp; int32_t* prev; };
PhonemeWs carve_phoneme(Ws& ws, int B, int64_t F_max, int Tp) {      // ints: start, dur, frames, lengths
  return {static_cast<int32_t*>(ws.bytes(((size_t)2 * B * Tp + 2 * (size_t)B) * sizeof(int32_t))), ws.f((size_t)B * F_max),
          static_cast<int32_t*>(ws.bytes((size_t)B * F_max * sizeof(int32_t)))};
}

std::atomic<uint64_t> g_contour_lds_done{0}, g_candidate_lds_done{0};

// ---- the path finder's host side
const vsp_prosody_path_params kPathDefaults = {0.35f, 0.14f, VSP_PROSODY_MAX_CANDIDATES};

// 0: ok; else the refused field (1 the costs, 2 max_candidates)
int check_path(const vsp_prosody_path_params* path, vsp_prosody_path_params& pp) {
  pp = path ? *path : kPathDefaults;
  if (!(pp.octave_jump_cost >= 0.f && pp.octave_jump_cost < 1e6f) || !(pp.voiced_unvoiced_cost >= 0.f && pp.voiced_unvoiced_cost < 1e6f))
    return 1;
  if (pp.max_candidates < 2 || pp.max_candidates > VSP_PROSODY_MAX_CANDIDATES) return 2;
  return 0;
}

int refuse_path(vsp_ctx* ctx, const char* who, int bad) {
  if (bad == 1) return ctx->fail(VSP_ERR_ARG, "%s: the octave-jump cost and the voiced/unvoiced cost must be at least 0", who);
  return ctx->fail(VSP_ERR_ARG, "%s: max_candidates must lie in [2, %d] (the unvoiced candidate and at least one voiced one)", who,
                   VSP_PROSODY_MAX_CANDIDATES);
}

struct PathWs { int32_t* frames; uint8_t* bp; };
PathWs carve_path(Ws& ws, int B, int64_t F_max) {
  return {static_cast<int32_t*>(ws.bytes((size_t)B * sizeof(int32_t))), static_cast<uint8_t*>(ws.bytes((size_t)B * F_max * PR_SLOTS))};
}

// vsp_prosody_contours_path: [the contour call's] [cand_f] [cand_s] [the path's]
struct ContourPathWs { ContourWs contour; float* cand_f; float* cand_s; PathWs path; };
ContourPathWs carve_contour_path(Ws& ws, int B, int64_t F_max, const Plan& pl) {
  return {carve_contour(ws, B, pl), ws.f((size_t)B * F_max * PR_SLOTS), ws.f((size_t)B * F_max * PR_SLOTS), carve_path(ws, B, F_max)};
}

// The launch of the path kernel behind the upload of the rows' frame counts (already checked).
int launch_path(const Call& call, int B, int F_max, int hop, const float* cand_f, const float* cand_s,
                const std::vector<int32_t>& frames, const vsp_prosody_path_params& pp, float* f0_frames, const PathWs& w) {
  if (const int rc = call.upload(w.frames, frames.data(), (size_t)B * sizeof(int32_t), "frames")) return rc;
  // kappa = 0.01 fs / hop, Praat's time-step correction, written so that it is exactly 1 where fs = 100 hop
  const double kappa = (double)PR_FS / (100.0 * (double)hop);
  PathArgs a;
  a.cand_f = cand_f; a.cand_s = cand_s;
  a.frames = w.frames;
  a.bp = w.bp;
  a.f0 = f0_frames; a.F_max = F_max;
  a.c_oct = (float)((double)pp.octave_jump_cost * kappa);
  a.c_vuv = (float)((double)pp.voiced_unvoiced_cost * kappa);
  hipLaunchKernelGGL(path_kernel, dim3(B), dim3(64), 0, call.s, a);
  return call.launched("path_kernel");
}

}  // namespace

int vsp_prosody_frames(int64_t n_samples, int hop) {
  if (hop < 1 || hop > PR_MAX_HOP || n_samples < PR_MIN_SAMPLES || n_samples > PR_MAX_SAMPLES) return VSP_ERR_ARG;
  return (int)(n_samples / hop) + 1;
}

int64_t vsp_prosody_workspace_bytes(int B, int64_t L_max, int hop, int Tp, const vsp_prosody_params* params) {
  Plan pl;
  if (B < 1 || B > PR_MAX_B || Tp < 0 || make_plan(params, pl)) return VSP_ERR_ARG;
  const int F_max = vsp_prosody_frames(L_max, hop);
  if (F_max < 0) return VSP_ERR_ARG;
  Ws contour = vsp::dry_ws(), phoneme = vsp::dry_ws();
  carve_contour(contour, B, pl);
  carve_phoneme(phoneme, B, F_max, std::max(Tp, 1));
  return (int64_t)std::max(contour.cur, phoneme.cur);
}

// The contour call of all three entry points; `who` names the one in every message.  n_voiced = 0: the per-frame decision
// into f0_frames (vsp_prosody_contours).  n_voiced >= 1: the candidate tables instead -- the caller's (cand_f, cand_s), or,
// with `fused`, the workspace's, for the path that follows (vsp_prosody_contours_path: f0_frames is the path's output and
// is not touched here; the workspace must then hold that call's whole layout, which comes back in *fused).
static int contours_impl(const Call& call, int B, int64_t L_max, int hop, const float* audio, int64_t audio_stride,
                         const int64_t* n_samples_host, const vsp_prosody_params* params, int n_voiced, float* f0_frames, float* cand_f,
                         float* cand_s, float* energy_frames, int64_t* frames, void* workspace, int64_t workspace_bytes,
                         ContourPathWs* fused = nullptr) {
  vsp_ctx* const ctx = call.ctx;
  const char* const who = call.who;
  const bool own_tables = fused != nullptr;
  Plan pl;
  if (const int bad = make_plan(params, pl)) {
    if (bad == 1) return ctx->fail(VSP_ERR_ARG, "%s: the pitch floor must be at least 40 Hz (the analysis window must fit in LDS)", who);
    if (bad == 2) return ctx->fail(VSP_ERR_ARG, "%s: the pitch ceiling must be above the floor and at most fs / 4 = %d Hz", who, PR_FS / 4);
    return ctx->fail(VSP_ERR_ARG, "%s: thresholds out of range (the silence threshold must be positive)", who);
  }
  if (B < 1 || B > PR_MAX_B || !n_samples_host) return ctx->fail(VSP_ERR_ARG, "%s: 1 <= B <= %d rows and their lengths", who, PR_MAX_B);
  const int F_max = vsp_prosody_frames(L_max, hop);
  if (F_max < 0)
    return ctx->fail(VSP_ERR_ARG, "%s: 1 <= hop <= %d and %d <= L_max <= 2^30 samples", who, PR_MAX_HOP, PR_MIN_SAMPLES);
  for (int b = 0; b < B; ++b)
    if (n_samples_host[b] < PR_MIN_SAMPLES || n_samples_host[b] > L_max)
      return ctx->fail(VSP_ERR_ARG, "%s: row %d has %lld samples: a row needs %d (n_fft / 2 + 1, for the reflection) "
                       "to L_max = %lld", who, b, (long long)n_samples_host[b], PR_MIN_SAMPLES, (long long)L_max);
  if (!audio || (!f0_frames && (n_voiced == 0 || own_tables)) || (n_voiced > 0 && !own_tables && (!cand_f || !cand_s)) ||
      !energy_frames || !frames || audio_stride < L_max)
    return ctx->fail(VSP_ERR_ARG, "%s: null pointer, or audio_stride < L_max", who);
  Ws ws = call.open(workspace, workspace_bytes);
  if (own_tables) *fused = carve_contour_path(ws, B, F_max, pl);
  const ContourWs w = own_tables ? fused->contour : carve_contour(ws, B, pl);
  if (const int rc = call.need_ws(workspace, workspace_bytes, ws.cur)) return rc;
  const int span4 = (pl.W + (PR_FPB - 1) * hop + 3) & ~3;
  // the lag buffers share the raw span's floats where they fit (48 KiB per block at the defaults: three blocks per CU)
  const int rbuf_floats = PR_FPB * (PR_LAGS_PER_WAVE * pl.LB + 4);
  const bool rbuf_over_span = rbuf_floats <= span4;
  const int rbuf_off = rbuf_over_span ? 0 : span4 + PR_FPB * pl.NA;
  const size_t lds = ((size_t)span4 + (size_t)PR_FPB * pl.NA + (rbuf_over_span ? 0 : (size_t)rbuf_floats)) * sizeof(float);
  if (lds > 160 * 1024) return ctx->fail(VSP_ERR_UNSUPPORTED, "%s: %zu bytes of LDS", who, lds);

  const hipStream_t s = call.s;
  if (const int rc = call.upload(w.n_samples, n_samples_host, (size_t)B * sizeof(int64_t), "tables")) return rc;
  {
    std::lock_guard<std::mutex> lock(g_tables_mu);      // (dropped right after the call: the runtime has staged the table by then)
    Tables& t = g_tables;
    if (t.W != pl.W || t.t0 != pl.t0 || t.LB != pl.LB || t.tmin != pl.tmin || t.tmax != pl.tmax) build_tables(pl, t);
    if (const int rc = call.upload(w.tables, t.host.data(), t.host.size() * sizeof(float), "tables")) return rc;
  }
  const float* tab = w.tables;
  hipLaunchKernelGGL(row_peak_kernel, dim3(B), dim3(1024), 0, s, audio, audio_stride, w.n_samples, w.stat);
  if (const int rc = call.launched("row_peak_kernel")) return rc;
  if (lds > 64 * 1024) {
    // (the size follows the caller's floor and hop; the attribute is set ONCE per device and instantiation, so it is the cap
    // checked above, the largest request the kernel can get -- a later call with a lower floor must not find a smaller one)
    const hipError_t e =
        n_voiced > 0 ? vsp::set_max_dynamic_lds(reinterpret_cast<const void*>(contour_kernel<true>), 160 * 1024, g_candidate_lds_done)
                     : vsp::set_max_dynamic_lds(reinterpret_cast<const void*>(contour_kernel<false>), 160 * 1024, g_contour_lds_done);
    if (e != hipSuccess) return ctx->fail(VSP_ERR_HIP, "contour_kernel (LDS): %s", hipGetErrorString(e));
  }
  ContourArgs a;
  a.audio = audio; a.a_bs = audio_stride; a.n_samples = w.n_samples; a.stat = w.stat;
  a.hann = tab; a.win = tab + PR_NFFT; a.inv_rw = tab + PR_NFFT + pl.W4;
  a.f0 = f0_frames; a.energy = energy_frames; a.frames = frames;
  a.F_max = F_max; a.hop = hop;
  a.W = pl.W; a.W4 = pl.W4; a.tmin = pl.tmin; a.tmax = pl.tmax; a.t0 = pl.t0; a.LB = pl.LB; a.NA = pl.NA; a.rbuf_off = rbuf_off;
  a.fs = (float)PR_FS; a.floor_hz = pl.p.floor_hz; a.vt = pl.p.voicing_threshold;
  a.st_scale = pl.p.silence_threshold / (1.f + pl.p.voicing_threshold); a.oc = pl.p.octave_cost;
  a.cand_f = cand_f; a.cand_s = cand_s; a.n_voiced = n_voiced;
  if (own_tables) { a.cand_f = fused->cand_f; a.cand_s = fused->cand_s; }
  const dim3 grid((F_max + PR_FPB - 1) / PR_FPB, B), block(64 * PR_FPB);
  if (n_voiced > 0) hipLaunchKernelGGL(contour_kernel<true>, grid, block, lds, s, a);
  else hipLaunchKernelGGL(contour_kernel<false>, grid, block, lds, s, a);
  return call.launched("contour_kernel");
}

int vsp_prosody_contours(vsp_ctx* ctx, void* stream, int B, int64_t L_max, int hop, const float* audio, int64_t audio_stride,
                         const int64_t* n_samples_host, const vsp_prosody_params* params, float* f0_frames,
                         float* energy_frames, int64_t* frames, void* workspace, int64_t workspace_bytes) {
  if (!ctx) return VSP_ERR_ARG;
  return contours_impl(Call{ctx, "vsp_prosody_contours", (hipStream_t)stream}, B, L_max, hop, audio, audio_stride, n_samples_host, params,
                       0, f0_frames, nullptr, nullptr, energy_frames, frames, workspace, workspace_bytes);
}

int64_t vsp_prosody_path_workspace_bytes(int B, int64_t L_max, int hop, const vsp_prosody_params* params,
                                         const vsp_prosody_path_params* path) {
  Plan pl;
  vsp_prosody_path_params pp;
  if (B < 1 || B > PR_MAX_B || make_plan(params, pl) || check_path(path, pp)) return VSP_ERR_ARG;
  const int F_max = vsp_prosody_frames(L_max, hop);
  if (F_max < 0) return VSP_ERR_ARG;
  Ws ws = vsp::dry_ws();
  carve_contour_path(ws, B, F_max, pl);                   // (the candidate call and the path alone each need a part of it)
  return (int64_t)ws.cur;
}

int vsp_prosody_candidates(vsp_ctx* ctx, void* stream, int B, int64_t L_max, int hop, const float* audio, int64_t audio_stride,
                           const int64_t* n_samples_host, const vsp_prosody_params* params, int max_candidates, float* cand_f,
                           float* cand_s, float* energy_frames, int64_t* frames, void* workspace, int64_t workspace_bytes) {
  if (!ctx) return VSP_ERR_ARG;
  if (max_candidates < 2 || max_candidates > VSP_PROSODY_MAX_CANDIDATES) return refuse_path(ctx, "vsp_prosody_candidates", 2);
  if (!cand_f || !cand_s) return ctx->fail(VSP_ERR_ARG, "vsp_prosody_candidates: null pointer, or audio_stride < L_max");
  return contours_impl(Call{ctx, "vsp_prosody_candidates", (hipStream_t)stream}, B, L_max, hop, audio, audio_stride, n_samples_host,
                       params, max_candidates - 1, nullptr, cand_f, cand_s, energy_frames, frames, workspace, workspace_bytes);
}

int vsp_prosody_path(vsp_ctx* ctx, void* stream, int B, int F_max, int hop, const float* cand_f, const float* cand_s,
                     const int64_t* frames_host, const vsp_prosody_path_params* path, float* f0_frames, void* workspace,
                     int64_t workspace_bytes) {
  if (!ctx) return VSP_ERR_ARG;
  vsp_prosody_path_params pp;
  if (const int bad = check_path(path, pp)) return refuse_path(ctx, "vsp_prosody_path", bad);
  if (B < 1 || B > PR_MAX_B || F_max < 1 || hop < 1 || hop > PR_MAX_HOP || !frames_host)
    return ctx->fail(VSP_ERR_ARG, "vsp_prosody_path: 1 <= B <= %d rows, F_max >= 1, 1 <= hop <= %d, and the rows' frame counts", PR_MAX_B,
                     PR_MAX_HOP);
  std::vector<int32_t> fr(B);
  for (int b = 0; b < B; ++b) {
    if (frames_host[b] < 1 || frames_host[b] > F_max)
      return ctx->fail(VSP_ERR_ARG, "vsp_prosody_path: row %d: 1 <= frames <= F_max = %d", b, F_max);
    fr[b] = (int32_t)frames_host[b];
  }
  if (!cand_f || !cand_s || !f0_frames) return ctx->fail(VSP_ERR_ARG, "vsp_prosody_path: null pointer");
  const Call call{ctx, "vsp_prosody_path", (hipStream_t)stream};
  Ws ws = call.open(workspace, workspace_bytes);
  const PathWs w = carve_path(ws, B, F_max);
  if (const int rc = call.need_ws(workspace, workspace_bytes, ws.cur)) return rc;
  return launch_path(call, B, F_max, hop, cand_f, cand_s, fr, pp, f0_frames, w);
}

int vsp_prosody_contours_path(vsp_ctx* ctx, void* stream, int B, int64_t L_max, int hop, const float* audio, int64_t audio_stride,
                              const int64_t* n_samples_host, const vsp_prosody_params* params, const vsp_prosody_path_params* path,
                              float* f0_frames, float* energy_frames, int64_t* frames, void* workspace, int64_t workspace_bytes) {
  if (!ctx) return VSP_ERR_ARG;
  const char* who = "vsp_prosody_contours_path";
  vsp_prosody_path_params pp;
  if (const int bad = check_path(path, pp)) return refuse_path(ctx, who, bad);
  // (everything else is refused in there, before its first launch: the rows, the pointers, the whole layout's size)
  const Call call{ctx, who, (hipStream_t)stream};
  ContourPathWs w;
  const int rc = contours_impl(call, B, L_max, hop, audio, audio_stride, n_samples_host, params, pp.max_candidates - 1, f0_frames,
                               nullptr, nullptr, energy_frames, frames, workspace, workspace_bytes, &w);
  if (rc != VSP_OK) return rc;
  std::vector<int32_t> fr(B);
  for (int b = 0; b < B; ++b) fr[b] = (int32_t)(n_samples_host[b] / hop) + 1;
  return launch_path(call, B, vsp_prosody_frames(L_max, hop), hop, w.cand_f, w.cand_s, fr, pp, f0_frames, w.path);
}

int vsp_prosody_phonemes(vsp_ctx* ctx, void* stream, int B, int F_max, int Tp, const float* f0_frames, const float* energy_frames,
                         const int64_t* frames_host, const int64_t* durations_host, const int64_t* lengths_host, float* f0,
                         float* energy, void* workspace, int64_t workspace_bytes) {
  if (!ctx) return VSP_ERR_ARG;
  if (B < 1 || B > PR_MAX_B || F_max < 1 || Tp < 1 || (int64_t)B * Tp > ((int64_t)1 << 28) || !frames_host || !durations_host ||
      !lengths_host)
    return ctx->fail(VSP_ERR_ARG, "vsp_prosody_phonemes: 1 <= B <= %d rows, F_max >= 1, Tp >= 1, and the host arrays", PR_MAX_B);
  std::vector<int32_t> ints((size_t)2 * B * Tp + 2 * (size_t)B, 0);
  int32_t* start = ints.data();
  int32_t* dur = start + (size_t)B * Tp;
  int32_t* fr = dur + (size_t)B * Tp;
  int32_t* len = fr + B;
  for (int b = 0; b < B; ++b) {
    if (frames_host[b] < 1 || frames_host[b] > F_max || lengths_host[b] < 0 || lengths_host[b] > Tp)
      return ctx->fail(VSP_ERR_ARG, "vsp_prosody_phonemes: row %d: 1 <= frames <= F_max and 0 <= length <= Tp", b);
    int64_t pos = 0;
    for (int j = 0; j < (int)lengths_host[b]; ++j) {
      const int64_t d = durations_host[(size_t)b * Tp + j];
      if (d < 0 || d > frames_host[b] || pos + d > frames_host[b])
        return ctx->fail(VSP_ERR_ARG, "vsp_prosody_phonemes: row %d: its durations sum to more than its %lld frames (or one is "
                         "negative) at phoneme %d", b, (long long)frames_host[b], j);
      start[(size_t)b * Tp + j] = (int32_t)pos;
      dur[(size_t)b * Tp + j] = (int32_t)d;
      pos += d;
    }
    fr[b] = (int32_t)frames_host[b];
    len[b] = (int32_t)lengths_host[b];
  }
  if (!f0_frames || !energy_frames || !f0 || !energy) return ctx->fail(VSP_ERR_ARG, "vsp_prosody_phonemes: null pointer");
  const Call call{ctx, "vsp_prosody_phonemes", (hipStream_t)stream};
  Ws ws = call.open(workspace, workspace_bytes);
  const PhonemeWs w = carve_phoneme(ws, B, F_max, Tp);
  if (const int rc = call.need_ws(workspace, workspace_bytes, ws.cur)) return rc;
  if (const int rc = call.upload(w.ints, ints.data(), ints.size() * sizeof(int32_t), "durations")) return rc;
  PhonemeArgs a;
  a.f0_frames = f0_frames; a.energy_frames = energy_frames;
  a.start = w.ints;
  a.dur = a.start + (size_t)B * Tp;
  a.frames = a.dur + (size_t)B * Tp;
  a.lengths = a.frames + B;
  a.interp = w.interp;
  a.prev = w.prev;
  a.f0 = f0; a.energy = energy; a.F_max = F_max; a.Tp = Tp;
  hipLaunchKernelGGL(phoneme_kernel, dim3(B), dim3(64), 0, call.s, a);
  return call.launched("phoneme_kernel");
}
