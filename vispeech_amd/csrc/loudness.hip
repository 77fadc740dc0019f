// Loudness (include/vispeech_hip.h, "loudness"): the integrated loudness of ITU-R BS.1770-4 / EBU R 128
// per row of a ragged batch of mono float32 recordings, a gain per row from it, and the gain applied -- all on the device,
// nothing read back between measuring and applying.  The specification is this project's own (fp64 restatement in
// tests/loudness_ref.py).  Row b is audio[b][0 .. n_b); nothing at or behind n_b is read, and a row's result is a function of
// the row alone: every partition below follows the row's own n_b and the rate's segment h, never L_max.
//
// K-weighting is two cascaded biquads, a linear recurrence over the whole row with a 4-value state s (transposed direct
// form II: two values a biquad): s' = M s + x v.  Its poles sit at radius 0.9946 at 44.1 kHz, so nothing may be truncated;
// instead the row is cut into its 100 ms segments and a segment into 64 lane runs of r = ceil(h / 64) samples, and states are
// carried across the cuts exactly: the end state of a chunk of k samples is M^k s_in + e, e its end state from zero.  The
// powers needed -- M^r 2^i for the lane scan, M^(h mod r) for a segment's partial lane, M^h for the row -- are host constants
// in double and travel as kernel arguments.  States and sums are double throughout (as align.hip's scores are).
//
//   lk_ends_kernel    one wave per (row, full segment but the row's last).  The segment is staged into LDS (16-byte loads
//                     where a quad lies inside it), lane l's run at pitch r | 1 words: the run loop's ds_read_b32 has the
//                     lanes r | 1 words apart, odd, so a 32-lane half covers 32 banks.  Every lane runs its run from zero
//                     state; a Hillis-Steele scan v_l += M^(r 2^i) v_(l - 2^i) gives the end state of every FULL lane; the
//                     partial lane (h is no multiple of 64 at 44.1, 22.05 or 8 kHz, and a padded sample is no no-op) ends
//                     the segment with M^(h mod r) v + its own e; where r divides h the last full lane ends it.
//   lk_carry_kernel   one wave per row: 64 segment ends a load, then state <- M^h state + e through the wave in order; lane i
//                     keeps the state its segment starts from.  Also zeroes the row's peak.
//   lk_energy_kernel  one wave per (row, segment), the same lane split: lane 0 now runs from the segment's true start state,
//                     the same scan gives every lane its true start state, and a second run sums y^2 in double; a butterfly
//                     reduces the wave into seg[b][s].  The staging pass keeps max |x|: one unsigned atomic max per wave on
//                     the float's bits (exact, and independent of the order).  Segments behind the row: exact 0.
//   lk_gate_kernel    one wave per row: block energies, both gates, L, (NB, kept), and the gain.  Sums run over ascending j
//                     (the passing lanes are walked in order through the wave), so they are the restatement's in every bit.
//   lk_apply_kernel   out = g x over each row's own samples, 16 bytes a lane where both rows are aligned.
// What bounds the first three is the dependent chain of a lane's run (two fp64 FMAs deep per biquad and sample, r samples,
// three runs a sample in all) and the scan's shuffles, not a pipe: 7 M samples for 16 rows of 10 s is no load on HBM or the
// vector unit.
// The one-pass closed form (zero-state energy + cross term + Gram term of the incoming state) is NOT used: under DC the
// high-pass's output is about 0 and the three terms cancel catastrophically.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <vector>

#include "kernels.h"
#include "model.h"
#include "op_host.h"

namespace {

constexpr int LK_MAX_B = 65535;
constexpr int64_t LK_MAX_SAMPLES = (int64_t)1 << 30;
constexpr int LK_FS_MIN = 8000, LK_FS_MAX = 192000;
constexpr int LK_APPLY_SPAN = 4096;      // samples of a row per block of the apply kernel (256 threads, four quads each)

struct KW {                              // the constants of one sample rate
  double c[10];                          // shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2
  double P[6][16];                       // M^(r 2^i), row-major
  double T[16];                          // M^(h mod r)
  double H[16];                          // M^h
  int h, r, pitch, nf, p;                // segment; lane run; its pitch in LDS (words); full lanes of a full segment; h mod r
};

struct Rows {                            // uploaded with every call: the head of the workspace
  const int32_t* n;                      // [B] samples
  const int32_t* n_apply;                // [B] samples the apply kernel touches (0: a row left alone)
  const float* params;                   // [B][3] target_lufs, peak_ceiling, max_gain_db
};

__device__ __forceinline__ double kstep(const double (&c)[10], double x, double (&s)[4]) {
  const double u = fma(c[0], x, s[0]);
  s[0] = fma(-c[3], u, fma(c[1], x, s[1]));
  s[1] = fma(-c[4], u, c[2] * x);
  const double y = fma(c[5], u, s[2]);
  s[2] = fma(-c[8], y, fma(c[6], u, s[3]));
  s[3] = fma(-c[9], y, c[7] * u);
  return y;
}

__device__ __forceinline__ void matvec_add(const double (&A)[16], const double (&v)[4], double (&acc)[4]) {   // acc += A v
#pragma unroll
  for (int i = 0; i < 4; ++i)
    acc[i] = fma(A[4 * i + 3], v[3], fma(A[4 * i + 2], v[2], fma(A[4 * i + 1], v[1], fma(A[4 * i], v[0], acc[i]))));
}

// The segment row[0 .. len) into LDS, sample i at (i / r) * pitch + i % r; returns this lane's max |x|.  Quads that lie inside
// the segment are 16-byte loads; the samples before the first aligned quad and behind the last are single loads, so nothing
// outside [0, len) is touched.
__device__ __forceinline__ float stage_segment(const float* __restrict__ row, int len, float* lds, int r, int pitch, int lane) {
  const int head = min(len, (int)((4u - (unsigned)(((uintptr_t)row >> 2) & 3u)) & 3u));
  const int nquads = (len - head) >> 2;
  float pk = 0.f;
  auto put = [&](int i, float v) {
    const int q = i / r;
    lds[q * pitch + (i - q * r)] = v;
    pk = fmaxf(pk, fabsf(v));
  };
  if (lane < head) put(lane, row[lane]);
  const float4* __restrict__ quads = reinterpret_cast<const float4*>(row + head);
  for (int q = lane; q < nquads; q += 64) {
    const float4 v = quads[q];
    const int i = head + 4 * q;
    put(i, v.x); put(i + 1, v.y); put(i + 2, v.z); put(i + 3, v.w);
  }
  const int tail = head + 4 * nquads + lane;      // (fewer than 4 samples are left)
  if (tail < len) put(tail, row[tail]);
  return pk;
}

// Lane `lane` runs its samples from `s` (in: the state it starts from; out: the state it ends in); with SUM the sum of y^2.
template <bool SUM>
__device__ __forceinline__ double run_lane(const KW& kw, const float* lds, int lane, int len, double (&s)[4]) {
  const int mine = max(0, min(kw.r, len - lane * kw.r));
  const float* x = lds + lane * kw.pitch;
  double acc = 0.0;
  for (int i = 0; i < kw.r; ++i)                   // (uniform trip count; only the row's ragged end predicates)
    if (i < mine) {
      const double y = kstep(kw.c, (double)x[i], s);
      if (SUM) acc = fma(y, y, acc);
    }
  return acc;
}

// v_l <- sum_{k <= l} M^(r (l - k)) v_k: the end state of lane l where the lanes 0 .. l all ran r samples.
__device__ __forceinline__ void scan_lanes(const KW& kw, int lane, double (&v)[4]) {
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    double o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = __shfl_up(v[i], 1 << k);
    if (lane >= (1 << k)) matvec_add(kw.P[k], o, v);
  }
}

struct SegArgs {
  const float* audio;      // [B][stride]
  int64_t stride;
  Rows rows;
  double* ends;            // [B][S_max][4]   zero-state end states (lk_ends) ...
  double* starts;          // [B][S_max][4]   ... and the states the segments start from (lk_carry)
  double* seg;             // [B][S_max]
  unsigned* peak_bits;     // [B]
  int S_max;
  const double* state_in;  // [B][4] the state every row starts from (NULL: zero)
  double* state_out;       // [B][4] the state behind every row's last COMPLETE segment (NULL: not wanted); may be state_in
};

__global__ void __launch_bounds__(64) lk_ends_kernel(const SegArgs g, const KW kw) {
  extern __shared__ __align__(16) float lk_lds[];
  const int b = blockIdx.y, s = blockIdx.x, lane = threadIdx.x;
  const int n = g.rows.n[b];
  const int S = (n + kw.h - 1) / kw.h;
  // (uniform) the row's last segment hands its state to nobody -- unless the state behind the last complete one is wanted
  if (s >= (g.state_out ? n / kw.h : S - 1)) return;
  stage_segment(g.audio + (size_t)b * g.stride + (size_t)s * kw.h, kw.h, lk_lds, kw.r, kw.pitch, lane);
  __syncthreads();
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  run_lane<false>(kw, lk_lds, lane, kw.h, v);
  const double e[4] = {v[0], v[1], v[2], v[3]};
  scan_lanes(kw, lane, v);
  double prev[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) prev[i] = __shfl_up(v[i], 1);
  double* out = g.ends + ((size_t)b * g.S_max + s) * 4;
  if (kw.p == 0) {                                 // every lane that ran is full: lane nf - 1 ends the segment
    if (lane == kw.nf - 1)
      for (int i = 0; i < 4; ++i) out[i] = v[i];
  } else if (lane == kw.nf) {                      // the partial lane: M^p (the state it starts from) + its own end from zero
    double end[4] = {e[0], e[1], e[2], e[3]};
    if (lane == 0) prev[0] = prev[1] = prev[2] = prev[3] = 0.0;
    matvec_add(kw.T, prev, end);
    for (int i = 0; i < 4; ++i) out[i] = end[i];
  }
}

__global__ void __launch_bounds__(64) lk_carry_kernel(const SegArgs g, const KW kw) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int n = g.rows.n[b];
  const int S = (n + kw.h - 1) / kw.h;
  const int F = n / kw.h, have = g.state_out ? F : S - 1;      // complete segments; segments whose end state lk_ends left
  if (lane == 0) g.peak_bits[b] = 0u;
  double st[4] = {0.0, 0.0, 0.0, 0.0};
  if (g.state_in)
    for (int i = 0; i < 4; ++i) st[i] = g.state_in[4 * (size_t)b + i];
  double fin[4] = {st[0], st[1], st[2], st[3]};                // the state behind F segments (F = 0: the one it started from)
  for (int s0 = 0; s0 < S; s0 += 64) {
    const int s = s0 + lane;
    double e[4] = {0.0, 0.0, 0.0, 0.0};
    if (s < have) {
      const double* p = g.ends + ((size_t)b * g.S_max + s) * 4;
      for (int i = 0; i < 4; ++i) e[i] = p[i];
    }
    double mine[4] = {0.0, 0.0, 0.0, 0.0};
    const int cnt = min(64, S - s0);
    for (int j = 0; j < cnt; ++j) {                // (every lane walks alike)
      double ej[4], nx[4];
      for (int i = 0; i < 4; ++i) {
        ej[i] = __shfl(e[i], j);
        if (lane == j) mine[i] = st[i];
        nx[i] = ej[i];
      }
      matvec_add(kw.H, st, nx);
      for (int i = 0; i < 4; ++i) {
        st[i] = nx[i];
        if (s0 + j + 1 == F) fin[i] = nx[i];
      }
    }
    if (s < S) {
      double* p = g.starts + ((size_t)b * g.S_max + s) * 4;
      for (int i = 0; i < 4; ++i) p[i] = mine[i];
    }
  }
  if (g.state_out && lane == 0)
    for (int i = 0; i < 4; ++i) g.state_out[4 * (size_t)b + i] = fin[i];
}

__global__ void __launch_bounds__(64) lk_energy_kernel(const SegArgs g, const KW kw) {
  extern __shared__ __align__(16) float lk_lds[];
  const int b = blockIdx.y, s = blockIdx.x, lane = threadIdx.x;
  const int n = g.rows.n[b];
  const int S = (n + kw.h - 1) / kw.h;
  if (s >= S) {                                    // (uniform) behind the row: an exact zero, nothing read
    if (lane == 0) g.seg[(size_t)b * g.S_max + s] = 0.0;
    return;
  }
  const int len = min(kw.h, n - s * kw.h);
  float pk = stage_segment(g.audio + (size_t)b * g.stride + (size_t)s * kw.h, len, lk_lds, kw.r, kw.pitch, lane);
  __syncthreads();
  const double* sp = g.starts + ((size_t)b * g.S_max + s) * 4;
  const double in[4] = {sp[0], sp[1], sp[2], sp[3]};
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  if (lane == 0)
    for (int i = 0; i < 4; ++i) v[i] = in[i];
  run_lane<false>(kw, lk_lds, lane, len, v);       // lane 0 from the true state: the scan then carries it to every lane
  scan_lanes(kw, lane, v);
  double st[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    st[i] = __shfl_up(v[i], 1);
    if (lane == 0) st[i] = in[i];
  }
  double acc = run_lane<true>(kw, lk_lds, lane, len, st);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    acc += __shfl_xor(acc, d);
    pk = fmaxf(pk, __shfl_xor(pk, d));
  }
  if (lane == 0) {
    g.seg[(size_t)b * g.S_max + s] = acc;
    atomicMax(g.peak_bits + b, __float_as_uint(pk));     // (|x| >= 0: its bits order as the floats do)
  }
}

struct GateArgs {
  const double* seg;       // [B][S_max]
  Rows rows;
  const float* peak;       // [B] (read with params)
  float* lufs;             // [B]
  int32_t* blocks;         // [B][2]
  float* gains;            // [B] (written with params)
  int S_max, h, with_params;
  double z_abs;
};

struct Gated { float L; int NB, kept; };

// Both gates over the blocks of seg's first n samples, by one wave: the row of lk_gate_kernel, and every prefix of a row in
// lk_time_kernel -- ONE body, so that the running level of a prefix is the integrated loudness of that prefix in every bit.
__device__ __forceinline__ Gated gate_wave(const double* __restrict__ seg, int n, int h, double z_abs, int lane) {
  const bool four = n >= 4 * h;
  const int NB = four ? n / h - 3 : 1;
  const double D = four ? 4.0 * (double)h : (double)n;
  auto energy = [&](int j) {
    if (four) return ((seg[j] + seg[j + 1]) + seg[j + 2]) + seg[j + 3];
    double E = 0.0;
    const int S = (n + h - 1) / h;
    for (int s = 0; s < S; ++s) E += seg[s];
    return E;
  };
  // the sum of E_j over the blocks that `keep` accepts, ascending j, and their number
  auto gated = [&](auto keep, double& sum, int& cnt) {
    sum = 0.0;
    cnt = 0;
    for (int j0 = 0; j0 < NB; j0 += 64) {
      const int j = j0 + lane;
      const double E = j < NB ? energy(j) : 0.0;
      unsigned long long m = __ballot(j < NB && keep(E));
      cnt += __popcll(m);
      while (m) {                                  // (uniform: every lane adds the same values in the same order)
        const int i = __ffsll((long long)m) - 1;
        sum += __shfl(E, i);
        m &= m - 1;
      }
    }
  };
  double sum_abs, sum_kept;
  int n_abs, n_kept;
  gated([&](double E) { return E / D > z_abs; }, sum_abs, n_abs);
  const double mean_abs = n_abs ? sum_abs / (double)n_abs : 0.0;
  gated([&](double E) { return E / D > z_abs && 10.0 * E > mean_abs; }, sum_kept, n_kept);
  const float L = n_kept ? (float)(-0.691 + 10.0 * log10(sum_kept / (double)n_kept / D)) : -INFINITY;
  return {L, NB, n_kept};
}

__global__ void __launch_bounds__(64) lk_gate_kernel(const GateArgs g) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int n = g.rows.n[b];
  const Gated r = gate_wave(g.seg + (size_t)b * g.S_max, n, g.h, g.z_abs, lane);
  const float L = r.L;
  const int NB = r.NB, n_kept = r.kept;
  if (lane != 0) return;
  g.lufs[b] = L;
  g.blocks[2 * b] = NB;
  g.blocks[2 * b + 1] = n_kept;
  if (!g.with_params) return;
  const float target = g.rows.params[3 * b], ceiling = g.rows.params[3 * b + 1], max_db = g.rows.params[3 * b + 2];
  float gain = 1.f;
  if (!(target != target) && n_kept) {
    double gd = pow(10.0, ((double)target - (double)L) / 20.0);
    gd = fmin(gd, pow(10.0, (double)max_db / 20.0));
    const float pk = g.peak[b];
    if (pk > 0.f) gd = fmin(gd, (double)ceiling / (double)pk);
    gain = (float)gd;
  }
  g.gains[b] = gain;
}

struct ApplyArgs {
  const float* in;
  float* out;
  int64_t in_stride, out_stride;
  const int32_t* n_apply;  // [B]
  const float* gains;      // [B]
};

__global__ void __launch_bounds__(256) lk_apply_kernel(const ApplyArgs a) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const int n = a.n_apply[b];
  const int i0 = blockIdx.x * LK_APPLY_SPAN;
  if (i0 >= n) return;                             // (a row left alone has n = 0: neither read nor written)
  const float g = a.gains[b];
  const float* __restrict__ x = a.in + (size_t)b * a.in_stride;
  float* o = a.out + (size_t)b * a.out_stride;
  if ((((uintptr_t)x | (uintptr_t)o) & 15u) == 0) {
#pragma unroll
    for (int k = 0; k < LK_APPLY_SPAN / 1024; ++k) {
      const int i = i0 + (k * 256 + tid) * 4;
      if (i + 3 < n) {
        float4 v = *reinterpret_cast<const float4*>(x + i);
        v.x *= g; v.y *= g; v.z *= g; v.w *= g;
        *reinterpret_cast<float4*>(o + i) = v;
      } else {
        for (int j = i; j < min(i + 4, n); ++j) o[j] = g * x[j];
      }
    }
  } else {
#pragma unroll 4
    for (int k = 0; k < LK_APPLY_SPAN / 256; ++k) {
      const int i = i0 + k * 256 + tid;
      if (i < n) o[i] = g * x[i];
    }
  }
}

// ---------------------------------------------------------------------------------- loudness over time
// A row here is a stream or a whole recording, described by pointers of its own (its tables start at segment 0), so that
// streams that were allocated apart advance in one launch.  Entry s of every table is computed from seg[0 .. s] in an order
// that depends on s alone: the call, the batch and the split of a stream change no bit.
//   lk_time_kernel         one wave per (row, segment s of the call): M[s] from four segments, S[s] from thirty, and I[s],
//                          kept[s] = gate_wave over the prefix of (s + 1) h samples -- the body of lk_gate_kernel, so the cost
//                          of an entry grows with s (two passes over s - 2 blocks).
//   lk_time_max_kernel     one wave per row: the largest M and S among the call's entries (a maximum: exact in any order).
//   lk_level_gains_kernel  one lane per row: the slewed gain in dB, float32 adds, subtracts, mins and maxes only, and its
//                          linear value; it starts from c_dB[first - 1] in the row's own table (initial_gain_db at first = 0).
//   lk_level_apply_kernel  out[i] = (c[s-2] + (c[s-1] - c[s-2]) w) x[i], every product and sum rounded on its own (no FMA).
struct LRow {                            // uploaded with every call of this section
  const double* seg;
  float *M, *S, *I;
  int32_t* kept;
  float *c_db, *c;
  const float* in;
  float* out;
  int32_t first, count;                  // time, gains: the entries [first, first + count)
  int32_t pos, samples;                  // apply: the stream's samples [pos, pos + samples); 0 samples for a NaN target
  float target, max_gain, max_cut, slew, init;
  int32_t pad;
};

__device__ __forceinline__ float db_to_linear(float db) { return (float)pow(10.0, (double)db / 20.0); }

// M[s] and S[s] of one entry, with the energies they are the logarithms of: E of the 400 ms block and T of the 3 s window
// that end at segment s (0 where there is none yet).  The one body of lk_time_kernel and lk_hist_kernel.
struct Levels { float M, S; double E, T; };

__device__ __forceinline__ Levels time_levels(const double* __restrict__ seg, int s, int h) {
  Levels v = {-INFINITY, -INFINITY, 0.0, 0.0};
  if (s >= 3) {
    const double E = ((seg[s - 3] + seg[s - 2]) + seg[s - 1]) + seg[s];
    if (E > 0.0) v.M = (float)(-0.691 + 10.0 * log10(E / (4.0 * (double)h)));
    v.E = E;
  }
  if (s >= 29) {
    double T = 0.0;
    for (int k = s - 29; k <= s; ++k) T += seg[k];
    if (T > 0.0) v.S = (float)(-0.691 + 10.0 * log10(T / (30.0 * (double)h)));
    v.T = T;
  }
  return v;
}

__global__ void __launch_bounds__(64) lk_time_kernel(const LRow* __restrict__ rows, int h, double z_abs) {
  const int b = blockIdx.y, lane = threadIdx.x;
  const LRow r = rows[b];
  if ((int)blockIdx.x >= r.count) return;          // (uniform)
  const int s = r.first + blockIdx.x;
  const double* __restrict__ seg = r.seg;
  const Gated g = gate_wave(seg, (s + 1) * h, h, z_abs, lane);
  if (lane != 0) return;
  const Levels v = time_levels(seg, s, h);
  r.M[s] = v.M;
  r.S[s] = v.S;
  r.I[s] = g.L;
  r.kept[s] = g.kept;
}

// ------------------------------------------------------------------- the histogram gate and loudness range
// lk_hist_kernel: one wave per row, no atomics, and no block waits for another.  The wave keeps the row's two histograms in
// registers -- bin k in lane k & 63, slot k >> 6: 16 bins a lane -- with the bins' centres beside them, and the 1001 edges
// in LDS.  64 entries at a time, lane i computes M, S (time_levels) and the two bin indices of entry first + i0 + i (a 10-step
// binary search over the edges: comparisons only); then the wave walks those entries in order: it bumps the two counts and
// makes the two gated passes over its 16 bins a lane, each followed by a butterfly, so that every sum runs in an order
// that depends on k alone and I[s] is a function of the counts.  The quotient of entry i is parked in lane i; its
// logarithm is taken lane-parallel behind the walk.  The work of an entry does not depend on s: no loop runs over the prefix.
constexpr int LK_HIST_BINS = VSP_LOUDNESS_HIST_BINS, LK_HIST_SLOTS = 16;
static_assert(LK_HIST_SLOTS * 64 >= LK_HIST_BINS && LK_HIST_BINS <= 1023, "16 bins a lane; a 10-step search");

struct HistArgs {
  const LRow* rows;
  int32_t* const* hist;    // [B] -> [2][1000]
  const double* edges;     // [1001]
  const double* centres;   // [1000]
  float* lra;              // [B] or NULL
  float* i_last;           // [B] or NULL: I of the call's last entry (-inf where it has none)
  int h;
};

// The largest k <= 999 with e[k] <= z, or -1 where !(z >= e[0]).  e holds 1024 doubles, +inf behind the edges.
__device__ __forceinline__ int hist_bin(const double* e, double z) {
  if (!(z >= e[0])) return -1;
  int k = 0;
#pragma unroll
  for (int step = 512; step >= 1; step >>= 1) {
    const int t = k + step;
    if (t < LK_HIST_BINS && e[t] <= z) k = t;
  }
  return k;
}

// sum = the sum of n[k] c[k] and cnt = the sum of n[k] over the bins with factor c[k] > above: a lane's bins in ascending slot,
// then a butterfly (the same bits in every lane).
__device__ __forceinline__ void hist_sum(const int (&n)[LK_HIST_SLOTS], const double (&c)[LK_HIST_SLOTS], double factor, double above,
                                         double& sum, int& cnt) {
  sum = 0.0;
  cnt = 0;
#pragma unroll
  for (int j = 0; j < LK_HIST_SLOTS; ++j)
    if (factor * c[j] > above) {
      sum += (double)n[j] * c[j];
      cnt += n[j];
    }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    sum += __shfl_xor(sum, d);
    cnt += __shfl_xor(cnt, d);
  }
}

__global__ void __launch_bounds__(64) lk_hist_kernel(const HistArgs a) {
  __shared__ double e[1024];
  const int b = blockIdx.x, lane = threadIdx.x;
  const LRow r = a.rows[b];
  int32_t* hist = a.hist[b];
  for (int k = lane; k < 1024; k += 64) e[k] = k <= LK_HIST_BINS ? a.edges[k] : INFINITY;
  double c[LK_HIST_SLOTS];
  int hb[LK_HIST_SLOTS], hs[LK_HIST_SLOTS];
#pragma unroll
  for (int j = 0; j < LK_HIST_SLOTS; ++j) {
    const int k = j * 64 + lane;
    const bool in = k < LK_HIST_BINS;
    c[j] = in ? a.centres[k] : 0.0;                // (a bin behind the last: count 0, never kept)
    hb[j] = in && r.first ? hist[k] : 0;           // at first == 0 the histograms start from zero, whatever they hold
    hs[j] = in && r.first ? hist[LK_HIST_BINS + k] : 0;
  }
  __syncthreads();
  const double DB = 4.0 * (double)a.h, DS = 30.0 * (double)a.h;
  if (r.count == 0 && a.i_last && lane == 0) a.i_last[b] = -INFINITY;
  for (int i0 = 0; i0 < r.count; i0 += 64) {
    const int s = r.first + i0 + lane;
    const bool mine = i0 + lane < r.count;
    Levels v = {-INFINITY, -INFINITY, 0.0, 0.0};
    int kb = -1, ks = -1;
    if (mine) {
      v = time_levels(r.seg, s, a.h);
      if (s >= 3) kb = hist_bin(e, v.E / DB);
      if (s >= 29) ks = hist_bin(e, v.T / DS);
    }
    double q = 0.0;
    int kept = 0;
    const int cnt = min(64, r.count - i0);
    for (int i = 0; i < cnt; ++i) {                // (every lane walks alike)
      const int kbi = __shfl(kb, i), ksi = __shfl(ks, i);
#pragma unroll
      for (int j = 0; j < LK_HIST_SLOTS; ++j) {
        hb[j] += kbi == j * 64 + lane ? 1 : 0;
        hs[j] += ksi == j * 64 + lane ? 1 : 0;
      }
      double sum_abs, sum_kept;
      int n_abs, n_kept;
      hist_sum(hb, c, 1.0, -1.0, sum_abs, n_abs);
      const double mean_abs = n_abs ? sum_abs / (double)n_abs : 0.0;
      hist_sum(hb, c, 10.0, mean_abs, sum_kept, n_kept);
      if (lane == i) {
        q = n_kept ? sum_kept / (double)n_kept : 0.0;
        kept = n_kept;
      }
    }
    if (mine) {
      const float I = kept ? (float)(-0.691 + 10.0 * log10(q)) : -INFINITY;
      if (r.M) {
        r.M[s] = v.M;
        r.S[s] = v.S;
        r.I[s] = I;
        r.kept[s] = kept;
      }
      if (a.i_last && i0 + lane == r.count - 1) a.i_last[b] = I;
    }
  }
  if (a.lra) {                                     // the range: percentiles of the kept 3 s windows, by their bins
    double sum;
    int n_all;
    hist_sum(hs, c, 1.0, -1.0, sum, n_all);
    const double mean = n_all ? sum / (double)n_all : 0.0;
    int N = 0;
    int keptj[LK_HIST_SLOTS];
#pragma unroll
    for (int j = 0; j < LK_HIST_SLOTS; ++j) {
      keptj[j] = 100.0 * c[j] > mean ? hs[j] : 0;
      N += keptj[j];
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) N += __shfl_xor(N, d);
    const int lo = (N + 4) / 10, hi = N ? (int)((95ll * (N - 1) + 50) / 100) : 0;
    int k10 = -1, k95 = -1, base = 0;
#pragma unroll
    for (int j = 0; j < LK_HIST_SLOTS; ++j) {      // cumulative kept counts in ascending k: a scan through the wave per slot
      int cum = keptj[j];
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(cum, d);
        if (lane >= d) cum += t;
      }
      cum += base;
      const unsigned long long m10 = __ballot(cum > lo), m95 = __ballot(cum > hi);
      if (k10 < 0 && m10) k10 = j * 64 + __ffsll((long long)m10) - 1;
      if (k95 < 0 && m95) k95 = j * 64 + __ffsll((long long)m95) - 1;
      base = __shfl(cum, 63);
    }
    if (lane == 0) a.lra[b] = N ? (float)(k95 - k10) / 10.f : 0.f;
  }
#pragma unroll
  for (int j = 0; j < LK_HIST_SLOTS; ++j) {
    const int k = j * 64 + lane;
    if (k < LK_HIST_BINS) {
      hist[k] = hb[j];
      hist[LK_HIST_BINS + k] = hs[j];
    }
  }
}

__global__ void __launch_bounds__(64) lk_time_max_kernel(const LRow* __restrict__ rows, float* m_max, float* s_max) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const LRow r = rows[b];
  float m = -INFINITY, s = -INFINITY;
  for (int k = lane; k < r.count; k += 64) {
    m = fmaxf(m, r.M[r.first + k]);
    s = fmaxf(s, r.S[r.first + k]);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    m = fmaxf(m, __shfl_xor(m, d));
    s = fmaxf(s, __shfl_xor(s, d));
  }
  if (lane == 0) {
    m_max[b] = m;
    s_max[b] = s;
  }
}

__global__ void __launch_bounds__(64) lk_level_gains_kernel(const LRow* __restrict__ rows, int B) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const LRow r = rows[b];
  if (r.target != r.target) return;                // a NaN target: neither read nor written
  const float d = __fdiv_rn(r.slew, 10.f);
  float prev = r.first == 0 ? r.init : r.c_db[r.first - 1];
  for (int s = r.first; s < r.first + r.count; ++s) {
    const float I = r.I[s];
    float q = prev;
    if (I != -INFINITY) q = fminf(fmaxf(__fsub_rn(r.target, I), -r.max_cut), r.max_gain);
    prev = __fadd_rn(prev, fminf(fmaxf(__fsub_rn(q, prev), -d), d));
    r.c_db[s] = prev;
    r.c[s] = db_to_linear(prev);
  }
}

__global__ void __launch_bounds__(256) lk_level_apply_kernel(const LRow* __restrict__ rows, int h, float rh) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const LRow r = rows[b];
  const int n = r.samples;
  const int i0 = blockIdx.x * LK_APPLY_SPAN;
  if (i0 >= n) return;                             // (a NaN target has 0 samples: neither read nor written)
  const float c_init = db_to_linear(r.init);
  const float* __restrict__ c = r.c;
  const float* x = r.in;                           // (may be r.out)
  float* o = r.out;
  // out = fl32(a x), a = the line from c[s - 2] to c[s - 1] at sample k of segment s.  Every product and sum is rounded on
  // its own: hipcc contracts a * b + c into an FMA by default, and its __fmul_rn / __fadd_rn are plain operators that it
  // contracts just the same, so contraction is switched off for this body.
  auto levelled = [&](int s, int k, float v) {
#pragma clang fp contract(off)
    const float c0 = s >= 2 ? c[s - 2] : c_init, c1 = s >= 1 ? c[s - 1] : c_init;
    const float w = (float)(k + 1) * rh;
    const float t = (c1 - c0) * w;
    const float a = c0 + t;
    return a * v;
  };
  if ((((uintptr_t)x | (uintptr_t)o) & 15u) == 0) {
#pragma unroll
    for (int q = 0; q < LK_APPLY_SPAN / 1024; ++q) {
      const int i = i0 + (q * 256 + tid) * 4;
      if (i >= n) continue;
      int s = (r.pos + i) / h, k = (r.pos + i) - s * h;
      auto step = [&](float v) {
        const float y = levelled(s, k, v);
        if (++k == h) { k = 0; ++s; }
        return y;
      };
      if (i + 3 < n) {
        float4 v = *reinterpret_cast<const float4*>(x + i);
        v.x = step(v.x); v.y = step(v.y); v.z = step(v.z); v.w = step(v.w);
        *reinterpret_cast<float4*>(o + i) = v;
      } else {
        for (int j = i; j < n; ++j) o[j] = step(x[j]);
      }
    }
  } else {
#pragma unroll 4
    for (int q = 0; q < LK_APPLY_SPAN / 256; ++q) {
      const int i = i0 + q * 256 + tid;
      if (i < n) {
        const int s = (r.pos + i) / h;
        o[i] = levelled(s, (r.pos + i) - s * h, x[i]);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ host
using vsp::Call;
using vsp::Ws;

bool fs_ok(int fs) { return fs >= LK_FS_MIN && fs <= LK_FS_MAX; }
int segment_samples(int fs) { return (fs + 5) / 10; }
int64_t segments_of(int64_t n, int fs) { const int h = segment_samples(fs); return (n + h - 1) / h; }

void kweighting(int fs, double (&c)[10]) {
  const double pi = 3.14159265358979323846;
  {
    const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
    const double K = std::tan(pi * f0 / fs), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
    const double a0 = 1.0 + K / Q + K * K;
    c[0] = (Vh + Vb * K / Q + K * K) / a0;
    c[1] = 2.0 * (K * K - Vh) / a0;
    c[2] = (Vh - Vb * K / Q + K * K) / a0;
    c[3] = 2.0 * (K * K - 1.0) / a0;
    c[4] = (1.0 - K / Q + K * K) / a0;
  }
  {
    const double f0 = 38.13547087602444, Q = 0.5003270373238773;
    const double K = std::tan(pi * f0 / fs), a0 = 1.0 + K / Q + K * K;
    c[5] = 1.0; c[6] = -2.0; c[7] = 1.0;
    c[8] = 2.0 * (K * K - 1.0) / a0;
    c[9] = (1.0 - K / Q + K * K) / a0;
  }
}

void mat_mul(const double* A, const double* B, double* C) {
  double t[16];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      double s = 0.0;
      for (int k = 0; k < 4; ++k) s += A[4 * i + k] * B[4 * k + j];
      t[4 * i + j] = s;
    }
  std::memcpy(C, t, sizeof t);
}

void mat_pow(const double* M, int64_t k, double* out) {          // M^k by squaring (M^0 = I)
  double base[16], acc[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  std::memcpy(base, M, sizeof base);
  for (; k > 0; k >>= 1) {
    if (k & 1) mat_mul(base, acc, acc);
    mat_mul(base, base, base);
  }
  std::memcpy(out, acc, sizeof acc);
}

KW make_kw(int fs) {
  KW kw;
  kweighting(fs, kw.c);
  const double* c = kw.c;
  // the state's transition: kstep() with x = 0
  const double M[16] = {-c[3], 1, 0, 0,
                        -c[4], 0, 0, 0,
                        c[6] - c[8] * c[5], 0, -c[8], 1,
                        c[7] - c[9] * c[5], 0, -c[9], 0};
  kw.h = segment_samples(fs);
  kw.r = (kw.h + 63) / 64;
  kw.pitch = kw.r | 1;
  kw.nf = kw.h / kw.r;
  kw.p = kw.h - kw.nf * kw.r;
  mat_pow(M, kw.r, kw.P[0]);
  for (int k = 1; k < 6; ++k) mat_mul(kw.P[k - 1], kw.P[k - 1], kw.P[k]);
  mat_pow(M, kw.p, kw.T);
  mat_pow(M, kw.h, kw.H);
  return kw;
}

// What the calls carve from their workspace (op_host.h); the sizes are the dry passes of these.  Every call's workspace
// begins with its rows, so a call that needs the rows alone is covered by any of the sizes.
//   measuring calls:  [rows: n, n_apply (int32 [B] each), params (float [B][3])] [ends] [starts] [seg] [blocks]
Rows carve_rows(Ws& ws, int B) {
  const int32_t* n = static_cast<const int32_t*>(ws.bytes((size_t)5 * B * sizeof(int32_t)));
  return n ? Rows{n, n + B, reinterpret_cast<const float*>(n + (size_t)2 * B)} : Rows{};
}

struct SegWs { double* ends; double* starts; double* seg; int32_t* blocks; };
SegWs carve_segments(Ws& ws, int B, int64_t S_max) {      // (a braced list is evaluated in order: so is every carve below)
  const size_t cells = (size_t)B * S_max;
  return {static_cast<double*>(ws.bytes(cells * 4 * sizeof(double))), static_cast<double*>(ws.bytes(cells * 4 * sizeof(double))),
          static_cast<double*>(ws.bytes(cells * sizeof(double))), static_cast<int32_t*>(ws.bytes((size_t)2 * B * sizeof(int32_t)))};
}

struct MeasureWs { Rows rows; SegWs seg; };
MeasureWs carve_measure(Ws& ws, int B, int64_t S_max) { return {carve_rows(ws, B), carve_segments(ws, B, S_max)}; }

bool sizes_ok(int B, int64_t L_max) { return B >= 1 && B <= LK_MAX_B && L_max >= 1 && L_max <= LK_MAX_SAMPLES; }

double z_abs() { return std::pow(10.0, (-70.0 + 0.691) / 10.0); }      // the absolute gate, -70 LUFS, as an energy

const vsp_loudness_params kLeaveAlone = {NAN, 1.f, 0.f};

// The rows of a call, refused on the host naming the row; fills the upload: n, n_apply, params.
int check_rows(vsp_ctx* ctx, const char* who, int B, int64_t L_max, const int64_t* n_host, const vsp_loudness_params* params,
               std::vector<int32_t>& up) {
  up.assign((size_t)5 * B, 0);
  for (int b = 0; b < B; ++b) {
    const int64_t n = n_host[b];
    if (n < 1 || n > L_max)
      return ctx->fail(VSP_ERR_ARG, "%s: row %d has %lld samples: 1 <= n_samples <= %lld", who, b, (long long)n, (long long)L_max);
    const vsp_loudness_params p = params ? params[b] : kLeaveAlone;
    if (params) {
      if (!(p.peak_ceiling > 0.f))
        return ctx->fail(VSP_ERR_ARG, "%s: row %d: peak_ceiling must be above 0", who, b);
      if (!(p.max_gain_db >= 0.f))
        return ctx->fail(VSP_ERR_ARG, "%s: row %d: max_gain_db must be at least 0", who, b);
    }
    up[b] = (int32_t)n;
    up[(size_t)B + b] = (params && p.target_lufs != p.target_lufs) ? 0 : (int32_t)n;      // a NaN target: the row is left alone
    const float f[3] = {p.target_lufs, p.peak_ceiling, p.max_gain_db};
    std::memcpy(&up[(size_t)2 * B + (size_t)3 * b], f, sizeof f);
  }
  return VSP_OK;
}

int check_fs(const Call& call, int fs) {
  if (fs_ok(fs)) return VSP_OK;
  return call.ctx->fail(VSP_ERR_ARG, "%s: sample_rate %d: %d <= sample_rate <= %d", call.who, fs, LK_FS_MIN, LK_FS_MAX);
}

// What every call over a batch of rows begins with: its own conditions on the batch (`ok`; `wants` says them behind the
// rows' count), then the rows.  The sample rate, where the call has one, is checked before (`ok` may divide by a segment).
int check_batch(const Call& call, bool ok, const char* wants, int B, int64_t L_max, const int64_t* n_host,
                const vsp_loudness_params* params, std::vector<int32_t>& up) {
  if (!ok) return call.ctx->fail(VSP_ERR_ARG, "%s: 1 <= B <= %d rows, %s", call.who, LK_MAX_B, wants);
  return check_rows(call.ctx, call.who, B, L_max, n_host, params, up);
}

int null_pointer(const Call& call) { return call.ctx->fail(VSP_ERR_ARG, "%s: null pointer", call.who); }

int send_rows(const Call& call, const Rows& rows, const std::vector<int32_t>& up) {      // (check_rows' upload to carve_rows' place)
  return call.upload(const_cast<int32_t*>(rows.n), up.data(), up.size() * sizeof(int32_t));
}

int launch_segments(const Call& call, int B, int S_max, const KW& kw, const float* audio, int64_t stride, const Rows& rows,
                    const SegWs& w, double* seg, float* peak, const double* state_in, double* state_out) {
  vsp_ctx* const ctx = call.ctx;
  const hipStream_t s = call.s;
  SegArgs a;
  a.state_in = state_in; a.state_out = state_out;
  a.audio = audio; a.stride = stride; a.rows = rows;
  a.ends = w.ends;
  a.starts = w.starts;
  a.seg = seg;
  a.peak_bits = reinterpret_cast<unsigned*>(peak);
  a.S_max = S_max;
  const size_t lds = (size_t)64 * kw.pitch * sizeof(float);      // (77 KiB at 192 kHz)
  static std::atomic<uint64_t> done_e{0}, done_c{0};
  if (lds > 48 * 1024) {
    hipError_t e = vsp::set_max_dynamic_lds(reinterpret_cast<const void*>(lk_ends_kernel), 96 * 1024, done_e);
    if (e == hipSuccess) e = vsp::set_max_dynamic_lds(reinterpret_cast<const void*>(lk_energy_kernel), 96 * 1024, done_c);
    if (e != hipSuccess) return ctx->fail(VSP_ERR_HIP, "loudness (LDS): %s", hipGetErrorString(e));
  }
  const dim3 grid(S_max, B);
  if (S_max > 1 || state_out) hipLaunchKernelGGL(lk_ends_kernel, grid, dim3(64), lds, s, a, kw);
  hipLaunchKernelGGL(lk_carry_kernel, dim3(B), dim3(64), 0, s, a, kw);
  hipLaunchKernelGGL(lk_energy_kernel, grid, dim3(64), lds, s, a, kw);
  return call.launched("loudness segments");
}

int launch_gate(const Call& call, int B, int S_max, int h, const double* seg, const Rows& rows, bool with_params,
                const float* peak, float* lufs, int32_t* blocks, float* gains) {
  GateArgs a;
  a.seg = seg; a.rows = rows; a.peak = peak; a.lufs = lufs; a.blocks = blocks; a.gains = gains;
  a.S_max = S_max; a.h = h; a.with_params = with_params ? 1 : 0;
  a.z_abs = z_abs();
  hipLaunchKernelGGL(lk_gate_kernel, dim3(B), dim3(64), 0, call.s, a);
  return call.launched("lk_gate_kernel");
}

int launch_apply(const Call& call, int B, int64_t L_max, const float* in, int64_t in_stride, float* out, int64_t out_stride,
                 const Rows& rows, const float* gains) {
  ApplyArgs a;
  a.in = in; a.out = out; a.in_stride = in_stride; a.out_stride = out_stride; a.n_apply = rows.n_apply; a.gains = gains;
  hipLaunchKernelGGL(lk_apply_kernel, dim3((unsigned)((L_max + LK_APPLY_SPAN - 1) / LK_APPLY_SPAN), B), dim3(256), 0, call.s, a);
  return call.launched("lk_apply_kernel");
}

}  // namespace

int vsp_loudness_kweighting(int sample_rate, double* coef) {
  if (!fs_ok(sample_rate) || !coef) return VSP_ERR_ARG;
  double c[10];
  kweighting(sample_rate, c);
  std::memcpy(coef, c, sizeof c);
  return VSP_OK;
}

int64_t vsp_loudness_segments_count(int64_t n_samples, int sample_rate) {
  if (!fs_ok(sample_rate) || n_samples < 1 || n_samples > LK_MAX_SAMPLES) return VSP_ERR_ARG;
  return segments_of(n_samples, sample_rate);
}

int64_t vsp_loudness_workspace_bytes(int B, int64_t L_max, int sample_rate) {
  if (!sizes_ok(B, L_max) || !fs_ok(sample_rate)) return VSP_ERR_ARG;
  Ws ws = vsp::dry_ws();
  carve_measure(ws, B, segments_of(L_max, sample_rate));
  return (int64_t)ws.cur;
}

// vsp_loudness_segments, and vsp_loudness_segments_from (a piece of a stream: first_host, state_in, state_out)
static int segments_call(const Call& call, int B, int64_t L_max, int sample_rate, const float* audio, int64_t audio_stride,
                         const int64_t* n_samples_host, const int64_t* first_host, const double* state_in, double* state_out, double* seg,
                         float* peak, void* workspace, int64_t workspace_bytes) {
  if (const int rc = check_fs(call, sample_rate)) return rc;
  std::vector<int32_t> up;
  if (const int rc = check_batch(call, sizes_ok(B, L_max) && audio_stride >= L_max && n_samples_host,
                                 "1 <= L_max <= 2^30 <= audio_stride, and the rows' samples", B, L_max, n_samples_host, nullptr, up))
    return rc;
  const int h = segment_samples(sample_rate);
  for (int b = 0; first_host && b < B; ++b)
    if (first_host[b] < 0 || first_host[b] % h || first_host[b] + n_samples_host[b] > LK_MAX_SAMPLES)
      return call.ctx->fail(VSP_ERR_ARG, "%s: row %d: the piece starts at sample %lld: a segment boundary (a multiple of %d), the stream at most 2^30 samples",
                            call.who, b, (long long)first_host[b], h);
  if (!audio || !seg || !peak) return null_pointer(call);
  const int S_max = (int)segments_of(L_max, sample_rate);
  Ws ws = call.open(workspace, workspace_bytes);
  const MeasureWs w = carve_measure(ws, B, S_max);
  if (const int rc = call.need_ws(workspace, workspace_bytes, ws.cur)) return rc;
  if (const int rc = send_rows(call, w.rows, up)) return rc;
  return launch_segments(call, B, S_max, make_kw(sample_rate), audio, audio_stride, w.rows, w.seg, seg, peak, state_in, state_out);
}

int vsp_loudness_segments(vsp_ctx* ctx, void* stream, int B, int64_t L_max, int sample_rate, const float* audio, int64_t audio_stride,
                          const int64_t* n_samples_host, double* seg, float* peak, void* workspace, int64_t workspace_bytes) {
  if (!ctx) return VSP_ERR_ARG;
  return segments_call(Call{ctx, "vsp_loudness_segments", (hipStream_t)stream}, B, L_max, sample_rate, audio, audio_stride, n_samples_host,
                       nullptr, nullptr, nullptr, seg, peak, workspace, workspace_bytes);
}

int vsp_loudness_gate(vsp_ctx* ctx, void* stream, int B, int S_max, int sample_rate, const double* seg, const int64_t* n_samples_host,
                      const float* peak, const vsp_loudness_params* params_host, float* lufs, int32_t* blocks, float* gains,
                      void* workspace, int64_t workspace_bytes) {
  if (!ctx) return VSP_ERR_ARG;
  const Call call{ctx, "vsp_loudness_gate", (hipStream_t)stream};
  if (const int rc = check_fs(call, sample_rate)) return rc;
  const int h = segment_samples(sample_rate);
  std::vector<int32_t> up;
  if (const int rc = check_batch(call, B >= 1 && B <= LK_MAX_B && S_max >= 1 && (int64_t)S_max * h <= LK_MAX_SAMPLES + h && n_samples_host,
                                 "S_max >= 1 segments (at most 2^30 samples), and the rows' samples", B,
                                 std::min((int64_t)S_max * h, LK_MAX_SAMPLES), n_samples_host, params_host, up))
    return rc;
  if (!seg || !lufs || !blocks || (params_host && (!peak || !gains))) return null_pointer(call);
  Ws ws = call.open(workspace, workspace_bytes);
  const Rows rows = carve_rows(ws, B);
  if (const int rc = call.need_ws(workspace, workspace_bytes, ws.cur)) return rc;
  if (const int rc = send_rows(call, rows, up)) return rc;
  return launch_gate(call, B, S_max, h, seg, rows, params_host != nullptr, peak, lufs, blocks, gains);
}

int vsp_loudness_apply(vsp_ctx* ctx, void* stream, int B, int64_t L_max, const float* in, int64_t in_stride, float* out,
                       int64_t out_stride, const int64_t* n_samples_host, const float* gains, const vsp_loudness_params* params_host,
                       void* workspace, int64_t workspace_bytes) {
  if (!ctx) return VSP_ERR_ARG;
  const Call call{ctx, "vsp_loudness_apply", (hipStream_t)stream};
  std::vector<int32_t> up;
  if (const int rc = check_batch(call, sizes_ok(B, L_max) && in_stride >= L_max && out_stride >= L_max && n_samples_host,
                                 "1 <= L_max <= 2^30 <= both strides, and the rows' samples", B, L_max, n_samples_host, params_host, up))
    return rc;
  if (!in || !out || !gains) return null_pointer(call);
  Ws ws = call.open(workspace, workspace_bytes);
  const Rows rows = carve_rows(ws, B);
  if (const int rc = call.need_ws(workspace, workspace_bytes, ws.cur)) return rc;
  if (const int rc = send_rows(call, rows, up)) return rc;
  return launch_apply(call, B, L_max, in, in_stride, out, out_stride, rows, gains);
}

int vsp_loudness_normalize(vsp_ctx* ctx, void* stream, int B, int64_t L_max, int sample_rate, const float* audio, int64_t audio_stride,
                           float* out, int64_t out_stride, const int64_t* n_samples_host, const vsp_loudness_params* params_host,
                           float* lufs, float* peak, float* gains, int32_t* blocks, void* workspace, int64_t workspace_bytes) {
  if (!ctx) return VSP_ERR_ARG;
  const Call call{ctx, "vsp_loudness_normalize", (hipStream_t)stream};
  if (const int rc = check_fs(call, sample_rate)) return rc;
  std::vector<int32_t> up;
  if (const int rc = check_batch(call, sizes_ok(B, L_max) && audio_stride >= L_max && out_stride >= L_max && n_samples_host && params_host,
                                 "1 <= L_max <= 2^30 <= both strides, the rows' samples and their params", B, L_max, n_samples_host,
                                 params_host, up))
    return rc;
  if (!audio || !out || !lufs || !peak || !gains) return null_pointer(call);
  const int S_max = (int)segments_of(L_max, sample_rate);
  Ws ws = call.open(workspace, workspace_bytes);
  const MeasureWs w = carve_measure(ws, B, S_max);
  if (const int rc = call.need_ws(workspace, workspace_bytes, ws.cur)) return rc;
  if (const int rc = send_rows(call, w.rows, up)) return rc;
  const KW kw = make_kw(sample_rate);
  if (const int rc = launch_segments(call, B, S_max, kw, audio, audio_stride, w.rows, w.seg, w.seg.seg, peak, nullptr, nullptr)) return rc;
  if (!blocks) blocks = w.seg.blocks;
  if (const int rc = launch_gate(call, B, S_max, kw.h, w.seg.seg, w.rows, true, peak, lufs, blocks, gains)) return rc;
  return launch_apply(call, B, L_max, audio, audio_stride, out, out_stride, w.rows, gains);
}

// ---------------------------------------------------------------------------------- loudness over time: entry points
namespace {

constexpr int64_t LK_MAX_ENTRIES = LK_MAX_SAMPLES / 800 + 1;      // (h >= 800; every call checks entries h itself)

//   calls over time:  [rows (as every loudness call)] [LRow [B]] and, for the fused call, [ends] [starts] [seg] [blocks]
struct TimeWs { Rows rows; LRow* lrows; };
TimeWs carve_time(Ws& ws, int B) { return {carve_rows(ws, B), static_cast<LRow*>(ws.bytes((size_t)B * sizeof(LRow)))}; }

struct LevelWs { TimeWs head; SegWs seg; };
LevelWs carve_level(Ws& ws, int B, int64_t S_max) { return {carve_time(ws, B), carve_segments(ws, B, S_max)}; }

int check_level(vsp_ctx* ctx, const char* who, int b, const vsp_loudness_level_params& p) {
  if (!(p.max_gain_db >= 0.f)) return ctx->fail(VSP_ERR_ARG, "%s: row %d: max_gain_db must be at least 0", who, b);
  if (!(p.max_cut_db >= 0.f)) return ctx->fail(VSP_ERR_ARG, "%s: row %d: max_cut_db must be at least 0", who, b);
  if (!(p.slew_db_per_s > 0.f)) return ctx->fail(VSP_ERR_ARG, "%s: row %d: slew_db_per_s must be above 0", who, b);
  if (!std::isfinite(p.initial_gain_db)) return ctx->fail(VSP_ERR_ARG, "%s: row %d: initial_gain_db must be finite", who, b);
  return VSP_OK;
}

void set_level(LRow& r, const vsp_loudness_level_params& p) {
  r.target = p.target_lufs; r.max_gain = p.max_gain_db; r.max_cut = p.max_cut_db; r.slew = p.slew_db_per_s; r.init = p.initial_gain_db;
}

// The entries [first, first + count) of a row whose tables hold `entries`: refused naming the row.
int check_entries(vsp_ctx* ctx, const char* who, int b, const vsp_loudness_row& r, int h) {
  if (r.entries < 0 || r.entries > LK_MAX_ENTRIES || r.entries * h > LK_MAX_SAMPLES + h)
    return ctx->fail(VSP_ERR_ARG, "%s: row %d: a table of %lld entries: at most 2^30 samples", who, b, (long long)r.entries);
  if (r.first < 0 || r.count < 0 || r.first + r.count > r.entries)
    return ctx->fail(VSP_ERR_ARG, "%s: row %d: entries [%lld, %lld + %lld) of a table of %lld", who, b, (long long)r.first,
                     (long long)r.first, (long long)r.count, (long long)r.entries);
  return VSP_OK;
}

// The entries of a row that the time kernels read and write (vsp_loudness_time, vsp_loudness_time_hist).
int set_entries(const Call& call, int b, const vsp_loudness_row& r, int h, LRow& d) {
  if (const int rc = check_entries(call.ctx, call.who, b, r, h)) return rc;
  if (r.count && (!r.seg || !r.M || !r.S || !r.I || !r.kept)) return call.ctx->fail(VSP_ERR_ARG, "%s: row %d: null pointer", call.who, b);
  std::memset(&d, 0, sizeof d);
  d.seg = r.seg; d.M = r.M; d.S = r.S; d.I = r.I; d.kept = r.kept;
  d.first = (int32_t)r.first; d.count = (int32_t)r.count;
  return VSP_OK;
}

// What the three calls over a set of streams end their checks with: the workspace's head, and the LRows into it.
int send_lrows(const Call& call, int B, const std::vector<LRow>& up, void* workspace, int64_t workspace_bytes, const LRow*& dev) {
  Ws ws = call.open(workspace, workspace_bytes);
  const TimeWs w = carve_time(ws, B);
  if (const int rc = call.need_ws(workspace, workspace_bytes, ws.cur)) return rc;
  dev = w.lrows;
  return call.upload(w.lrows, up.data(), up.size() * sizeof(LRow));
}

int launch_time(const Call& call, int B, int count_max, int h, const LRow* rows, float* m_max, float* s_max) {
  if (count_max > 0) hipLaunchKernelGGL(lk_time_kernel, dim3(count_max, B), dim3(64), 0, call.s, rows, h, z_abs());
  if (m_max) hipLaunchKernelGGL(lk_time_max_kernel, dim3(B), dim3(64), 0, call.s, rows, m_max, s_max);
  return call.launched("loudness time");
}

int launch_level_gains(const Call& call, int B, const LRow* rows) {
  hipLaunchKernelGGL(lk_level_gains_kernel, dim3((B + 63) / 64), dim3(64), 0, call.s, rows, B);
  return call.launched("lk_level_gains_kernel");
}

int launch_level_apply(const Call& call, int B, int64_t samples_max, int h, const LRow* rows) {
  if (samples_max < 1) return VSP_OK;
  hipLaunchKernelGGL(lk_level_apply_kernel, dim3((unsigned)((samples_max + LK_APPLY_SPAN - 1) / LK_APPLY_SPAN), B), dim3(256), 0, call.s, rows,
                     h, 1.f / (float)h);
  return call.launched("lk_level_apply_kernel");
}

}  // namespace

int64_t vsp_loudness_time_workspace_bytes(int B, int64_t L_max, int sample_rate) {
  if (!sizes_ok(B, L_max) || !fs_ok(sample_rate)) return VSP_ERR_ARG;
  Ws ws = vsp::dry_ws();
  carve_level(ws, B, segments_of(L_max, sample_rate));
  return (int64_t)ws.cur;
}

int vsp_loudness_segments_from(vsp_ctx* ctx, void* stream, int B, int64_t L_max, int sample_rate, const float* audio, int64_t audio_stride,
                               const int64_t* n_samples_host, const int64_t* first_host, const double* state_in, double* state_out,
                               double* seg, float* peak, void* workspace, int64_t workspace_bytes) {
  if (!ctx) return VSP_ERR_ARG;
  return segments_call(Call{ctx, "vsp_loudness_segments_from", (hipStream_t)stream}, B, L_max, sample_rate, audio, audio_stride,
                       n_samples_host, first_host, state_in, state_out, seg, peak, workspace, workspace_bytes);
}

int vsp_loudness_time(vsp_ctx* ctx, void* stream, int B, int sample_rate, const vsp_loudness_row* rows_host, float* m_max, float* s_max,
                      void* workspace, int64_t workspace_bytes) {
  if (!ctx) return VSP_ERR_ARG;
  const char* who = "vsp_loudness_time";
  const Call call{ctx, who, (hipStream_t)stream};
  if (const int rc = check_fs(call, sample_rate)) return rc;
  if (B < 1 || B > LK_MAX_B || !rows_host) return ctx->fail(VSP_ERR_ARG, "%s: 1 <= B <= %d rows", who, LK_MAX_B);
  const int h = segment_samples(sample_rate);
  std::vector<LRow> up((size_t)B);
  int64_t count_max = 0;
  for (int b = 0; b < B; ++b) {
    if (const int rc = set_entries(call, b, rows_host[b], h, up[b])) return rc;
    count_max = std::max(count_max, rows_host[b].count);
  }
  if (!m_max != !s_max) return ctx->fail(VSP_ERR_ARG, "%s: m_max and s_max come together", who);
  const LRow* dev;
  if (const int rc = send_lrows(call, B, up, workspace, workspace_bytes, dev)) return rc;
  return launch_time(call, B, (int)count_max, h, dev, m_max, s_max);
}

int vsp_loudness_level_gains(vsp_ctx* ctx, void* stream, int B, const vsp_loudness_row* rows_host,
                             const vsp_loudness_level_params* params_host, void* workspace, int64_t workspace_bytes) {
  if (!ctx) return VSP_ERR_ARG;
  const char* who = "vsp_loudness_level_gains";
  const Call call{ctx, who, (hipStream_t)stream};
  if (B < 1 || B > LK_MAX_B || !rows_host || !params_host) return ctx->fail(VSP_ERR_ARG, "%s: 1 <= B <= %d rows and their params", who, LK_MAX_B);
  std::vector<LRow> up((size_t)B);
  for (int b = 0; b < B; ++b) {
    const vsp_loudness_row& r = rows_host[b];
    if (const int rc = check_entries(ctx, who, b, r, LK_FS_MIN / 10)) return rc;
    if (const int rc = check_level(ctx, who, b, params_host[b])) return rc;
    const bool alone = params_host[b].target_lufs != params_host[b].target_lufs;
    if (r.count && !alone && (!r.I || !r.c_db || !r.c)) return ctx->fail(VSP_ERR_ARG, "%s: row %d: null pointer", who, b);
    LRow& d = up[b];
    std::memset(&d, 0, sizeof d);
    d.I = r.I; d.c_db = r.c_db; d.c = r.c;
    d.first = (int32_t)r.first; d.count = (int32_t)r.count;
    set_level(d, params_host[b]);
  }
  const LRow* dev;
  if (const int rc = send_lrows(call, B, up, workspace, workspace_bytes, dev)) return rc;
  return launch_level_gains(call, B, dev);
}

int vsp_loudness_level_apply(vsp_ctx* ctx, void* stream, int B, int sample_rate, const vsp_loudness_row* rows_host,
                             const vsp_loudness_level_params* params_host, void* workspace, int64_t workspace_bytes) {
  if (!ctx) return VSP_ERR_ARG;
  const char* who = "vsp_loudness_level_apply";
  const Call call{ctx, who, (hipStream_t)stream};
  if (const int rc = check_fs(call, sample_rate)) return rc;
  if (B < 1 || B > LK_MAX_B || !rows_host || !params_host) return ctx->fail(VSP_ERR_ARG, "%s: 1 <= B <= %d rows and their params", who, LK_MAX_B);
  const int h = segment_samples(sample_rate);
  std::vector<LRow> up((size_t)B);
  int64_t samples_max = 0;
  for (int b = 0; b < B; ++b) {
    const vsp_loudness_row& r = rows_host[b];
    if (r.pos < 0 || r.samples < 0 || r.pos + r.samples > LK_MAX_SAMPLES)
      return ctx->fail(VSP_ERR_ARG, "%s: row %d: samples [%lld, %lld + %lld): inside [0, 2^30]", who, b, (long long)r.pos, (long long)r.pos,
                       (long long)r.samples);
    if (r.entries < 0 || r.entries > LK_MAX_ENTRIES || (r.samples && (r.pos + r.samples - 1) / h > r.entries))
      return ctx->fail(VSP_ERR_ARG, "%s: row %d: samples up to %lld need %lld entries of c, the table holds %lld", who, b,
                       (long long)(r.pos + r.samples), (long long)((r.pos + r.samples - 1) / h), (long long)r.entries);
    if (const int rc = check_level(ctx, who, b, params_host[b])) return rc;
    const bool alone = params_host[b].target_lufs != params_host[b].target_lufs;
    if (r.samples && !alone && (!r.in || !r.out || (r.entries && !r.c))) return ctx->fail(VSP_ERR_ARG, "%s: row %d: null pointer", who, b);
    LRow& d = up[b];
    std::memset(&d, 0, sizeof d);
    d.c = r.c; d.in = r.in; d.out = r.out;
    d.pos = (int32_t)r.pos; d.samples = alone ? 0 : (int32_t)r.samples;
    set_level(d, params_host[b]);
    samples_max = std::max(samples_max, (int64_t)d.samples);
  }
  const LRow* dev;
  if (const int rc = send_lrows(call, B, up, workspace, workspace_bytes, dev)) return rc;
  return launch_level_apply(call, B, samples_max, h, dev);
}

int vsp_loudness_level(vsp_ctx* ctx, void* stream, int B, int64_t L_max, int sample_rate, const float* audio, int64_t audio_stride, float* out,
                       int64_t out_stride, const int64_t* n_samples_host, const vsp_loudness_level_params* params_host, float* M, float* S,
                       float* I, int32_t* kept, float* c_db, float* c, int64_t table_stride, float* m_max, float* s_max, float* i_end,
                       float* peak, void* workspace, int64_t workspace_bytes) {
  if (!ctx) return VSP_ERR_ARG;
  const Call call{ctx, "vsp_loudness_level", (hipStream_t)stream};
  if (const int rc = check_fs(call, sample_rate)) return rc;
  const int h = segment_samples(sample_rate);
  std::vector<int32_t> up;
  if (const int rc = check_batch(call, sizes_ok(B, L_max) && audio_stride >= L_max && !(params_host && out_stride < L_max) && n_samples_host &&
                                           table_stride >= L_max / h,
                                 "1 <= L_max <= 2^30 <= both strides, table_stride >= L_max / h, and the rows' samples", B, L_max, n_samples_host,
                                 nullptr, up))
    return rc;
  for (int b = 0; params_host && b < B; ++b)
    if (const int rc = check_level(ctx, call.who, b, params_host[b])) return rc;
  if (!audio || !M || !S || !I || !kept || !m_max || !s_max || !i_end || !peak || (params_host && (!out || !c_db || !c))) return null_pointer(call);
  const int S_max = (int)segments_of(L_max, sample_rate);
  Ws ws = call.open(workspace, workspace_bytes);
  const LevelWs w = carve_level(ws, B, S_max);
  if (const int rc = call.need_ws(workspace, workspace_bytes, ws.cur)) return rc;
  // ONE upload: the rows of the segment kernels, then the rows of this section -- a host copy of the head, carved as the head is
  Ws head = vsp::dry_ws();
  carve_time(head, B);
  std::vector<char> both(head.cur, 0);
  Ws mirror(both.data(), both.size(), false);
  const TimeWs host = carve_time(mirror, B);
  std::memcpy(const_cast<int32_t*>(host.rows.n), up.data(), up.size() * sizeof(int32_t));
  for (int b = 0; b < B; ++b) {
    LRow& d = host.lrows[b];
    const size_t t = (size_t)b * table_stride;
    d.seg = w.seg.seg + (size_t)b * S_max;
    d.M = M + t; d.S = S + t; d.I = I + t; d.kept = kept + t;
    d.first = 0; d.count = (int32_t)(n_samples_host[b] / h);
    if (!params_host) continue;
    d.c_db = c_db + t; d.c = c + t;
    d.in = audio + (size_t)b * audio_stride; d.out = out + (size_t)b * out_stride;
    d.pos = 0; d.samples = params_host[b].target_lufs != params_host[b].target_lufs ? 0 : (int32_t)n_samples_host[b];
    set_level(d, params_host[b]);
  }
  if (const int rc = call.upload(workspace, both.data(), both.size())) return rc;
  const Rows& rows = w.head.rows;
  const LRow* dev = w.head.lrows;
  const KW kw = make_kw(sample_rate);
  if (const int rc = launch_segments(call, B, S_max, kw, audio, audio_stride, rows, w.seg, w.seg.seg, peak, nullptr, nullptr)) return rc;
  if (const int rc = launch_gate(call, B, S_max, h, w.seg.seg, rows, false, peak, i_end, w.seg.blocks, nullptr)) return rc;
  if (const int rc = launch_time(call, B, (int)(L_max / h), h, dev, m_max, s_max)) return rc;
  if (!params_host) return VSP_OK;
  if (const int rc = launch_level_gains(call, B, dev)) return rc;
  return launch_level_apply(call, B, L_max, h, dev);
}

// --------------------------------------------------------------- loudness range and the histogram gate: entry points
namespace {

constexpr size_t LK_HIST_TABLE_DOUBLES = 2 * LK_HIST_BINS + 1;      // the edges, then the centres

void hist_tables(double* edges, double* centres) {
  for (int k = 0; k <= LK_HIST_BINS; ++k) edges[k] = std::pow(10.0, ((double)k - 693.09) / 100.0);
  edges[0] = z_abs();                                    // by the exact gate's own expression (the line above is 2e-15 off it)
  for (int k = 0; k < LK_HIST_BINS; ++k) centres[k] = std::pow(10.0, ((double)k - 692.59) / 100.0);
}

//   histogram calls:  [rows (as every loudness call)] [LRow [B]] [histogram pointers [B]] [edges, centres] and, for the fused
//                     call, [a measuring call's: rows (not used: the head's serve), ends, starts, seg, blocks] [peak [B]]
//                     [histograms [B][2][1000]]
struct HistWs { TimeWs head; int32_t** hist; double* tables; };
HistWs carve_hist(Ws& ws, int B) {
  return {carve_time(ws, B), static_cast<int32_t**>(ws.bytes((size_t)B * sizeof(int32_t*))),
          static_cast<double*>(ws.bytes(LK_HIST_TABLE_DOUBLES * sizeof(double)))};
}

struct RangeWs { HistWs head; SegWs seg; float* peak; int32_t* hists; };
RangeWs carve_range(Ws& ws, int B, int64_t S_max) {
  return {carve_hist(ws, B), carve_measure(ws, B, S_max).seg, ws.f((size_t)B),
          static_cast<int32_t*>(ws.bytes((size_t)B * 2 * LK_HIST_BINS * sizeof(int32_t)))};
}

size_t hist_head_bytes(int B) {
  Ws ws = vsp::dry_ws();
  carve_hist(ws, B);
  return ws.cur;
}

// What a call of this section uploads: a host copy of the workspace's head, carved as the head is -- behind the rows of the
// segment kernels the LRows, the histogram pointers, the tables.
struct HistUpload {
  std::vector<char> bytes;
  Ws mirror;
  const HistWs host;
  explicit HistUpload(int B) : bytes(hist_head_bytes(B), 0), mirror(bytes.data(), bytes.size(), false), host(carve_hist(mirror, B)) {
    hist_tables(host.tables, host.tables + LK_HIST_BINS + 1);
  }
  // One copy, of the whole head or of what lies behind its first rows; the kernel's arguments point into the workspace.
  int send(const Call& call, const HistWs& dev, bool with_rows, float* lra, float* i_last, int h, HistArgs& a) const {
    const char* from = with_rows ? bytes.data() : reinterpret_cast<const char*>(host.head.lrows);
    void* to = with_rows ? (void*)dev.head.rows.n : (void*)dev.head.lrows;
    if (const int rc = call.upload(to, from, (size_t)(bytes.data() + bytes.size() - from))) return rc;
    a.rows = dev.head.lrows;
    a.hist = dev.hist;
    a.edges = dev.tables;
    a.centres = a.edges + LK_HIST_BINS + 1;
    a.lra = lra; a.i_last = i_last; a.h = h;
    return VSP_OK;
  }
};

int launch_hist(const Call& call, int B, const HistArgs& a, float* m_max, float* s_max) {
  hipLaunchKernelGGL(lk_hist_kernel, dim3(B), dim3(64), 0, call.s, a);
  if (m_max) hipLaunchKernelGGL(lk_time_max_kernel, dim3(B), dim3(64), 0, call.s, a.rows, m_max, s_max);
  return call.launched("loudness histogram");
}

}  // namespace

int vsp_loudness_hist_tables(double* edges, double* centres) {
  if (!edges || !centres) return VSP_ERR_ARG;
  hist_tables(edges, centres);
  return VSP_OK;
}

int64_t vsp_loudness_hist_workspace_bytes(int B, int64_t L_max, int sample_rate) {
  if (!sizes_ok(B, L_max) || !fs_ok(sample_rate)) return VSP_ERR_ARG;
  Ws ws = vsp::dry_ws();
  carve_range(ws, B, segments_of(L_max, sample_rate));
  return (int64_t)ws.cur;
}

int vsp_loudness_time_hist(vsp_ctx* ctx, void* stream, int B, int sample_rate, const vsp_loudness_row* rows_host, int32_t* const* hist_host,
                           float* m_max, float* s_max, float* lra, void* workspace, int64_t workspace_bytes) {
  if (!ctx) return VSP_ERR_ARG;
  const char* who = "vsp_loudness_time_hist";
  const Call call{ctx, who, (hipStream_t)stream};
  if (const int rc = check_fs(call, sample_rate)) return rc;
  if (B < 1 || B > LK_MAX_B || !rows_host || !hist_host) return ctx->fail(VSP_ERR_ARG, "%s: 1 <= B <= %d rows and their histograms", who, LK_MAX_B);
  const int h = segment_samples(sample_rate);
  HistUpload up(B);
  for (int b = 0; b < B; ++b) {
    if (const int rc = set_entries(call, b, rows_host[b], h, up.host.head.lrows[b])) return rc;
    if (!hist_host[b]) return ctx->fail(VSP_ERR_ARG, "%s: row %d: null histogram", who, b);
    up.host.hist[b] = hist_host[b];
  }
  if (!m_max != !s_max) return ctx->fail(VSP_ERR_ARG, "%s: m_max and s_max come together", who);
  Ws ws = call.open(workspace, workspace_bytes);
  const HistWs w = carve_hist(ws, B);
  if (const int rc = call.need_ws(workspace, workspace_bytes, ws.cur)) return rc;
  HistArgs a;
  if (const int rc = up.send(call, w, false, lra, nullptr, h, a)) return rc;
  return launch_hist(call, B, a, m_max, s_max);
}

int vsp_loudness_range(vsp_ctx* ctx, void* stream, int B, int64_t L_max, int sample_rate, const float* audio, int64_t audio_stride,
                       const int64_t* n_samples_host, float* lra, float* i_hist, float* M, float* S, float* I, int32_t* kept,
                       int64_t table_stride, void* workspace, int64_t workspace_bytes) {
  if (!ctx) return VSP_ERR_ARG;
  const Call call{ctx, "vsp_loudness_range", (hipStream_t)stream};
  if (const int rc = check_fs(call, sample_rate)) return rc;
  const int h = segment_samples(sample_rate);
  const bool tables = M || S || I || kept;
  if (tables && (!M || !S || !I || !kept)) return ctx->fail(VSP_ERR_ARG, "%s: M, S, I and kept come together", call.who);
  std::vector<int32_t> rows_up;
  if (const int rc = check_batch(call, sizes_ok(B, L_max) && audio_stride >= L_max && n_samples_host && !(tables && table_stride < L_max / h),
                                 "1 <= L_max <= 2^30 <= audio_stride, table_stride >= L_max / h, and the rows' samples", B, L_max,
                                 n_samples_host, nullptr, rows_up))
    return rc;
  if (!audio || !lra) return null_pointer(call);
  const int S_max = (int)segments_of(L_max, sample_rate);
  Ws ws = call.open(workspace, workspace_bytes);
  const RangeWs w = carve_range(ws, B, S_max);
  if (const int rc = call.need_ws(workspace, workspace_bytes, ws.cur)) return rc;
  HistUpload up(B);                                     // ONE upload: the rows of the segment kernels, then the rows of this section
  std::memcpy(const_cast<int32_t*>(up.host.head.rows.n), rows_up.data(), rows_up.size() * sizeof(int32_t));
  for (int b = 0; b < B; ++b) {
    LRow& d = up.host.head.lrows[b];
    const size_t t = (size_t)b * table_stride;
    d.seg = w.seg.seg + (size_t)b * S_max;
    if (tables) { d.M = M + t; d.S = S + t; d.I = I + t; d.kept = kept + t; }
    d.first = 0; d.count = (int32_t)(n_samples_host[b] / h);
    up.host.hist[b] = w.hists + (size_t)b * 2 * LK_HIST_BINS;
  }
  HistArgs a;
  if (const int rc = up.send(call, w.head, true, lra, i_hist, h, a)) return rc;
  if (const int rc = launch_segments(call, B, S_max, make_kw(sample_rate), audio, audio_stride, w.head.head.rows, w.seg, w.seg.seg, w.peak,
                                     nullptr, nullptr))
    return rc;
  return launch_hist(call, B, a, nullptr, nullptr);
}
