// Durations from a recording (include/vispeech_hip.h, "align"): monotonic alignment of a recording's
// latent frames x [B][C][F] to the frames of a text's prior (m, logs) [B][C][K] -- what VITS calls monotonic alignment
// search, with a skip allowed -- restated as three launches.  The specification is this project's own (fp64 restatement in
// tests/align_ref.py).  Everything is ragged over the batch: row b is F_b frames by K_b states, nothing outside a row's
// extent is read (loads are predicated, not selected after the fact), outputs outside it are exact zeros, and a row's result
// is a function of the row alone.
//
//   align_scores_kernel     S[j][k] = sum_c -0.5 (x[c][j] - m[c][k])^2 exp(-2 logs[c][k]) - sum_c logs[c][k], the DIRECT form
//                           (difference first, then the square).  One block = a 64 x 64 tile of (j, k), 256 threads, a 4 x 4
//                           register tile each; channels in slabs of AL_CS through LDS.  While a slab of logs is staged the
//                           staging thread forms w = -0.5 exp(-2 logs) and keeps its share of sum logs, so the prologue costs
//                           no pass of its own.  Per channel and thread: three ds_read_b128 (x is a broadcast within a
//                           16-lane group), 16 subtract / multiply / FMA triples.  Bound: the fp32 vector pipe (it is no
//                           matrix product: the weight sits between the two operands).  The order of a cell's sum is c
//                           ascending, whatever the batch.
//   align_path_kernel       one block per row, thread t owns the states 4t .. 4t + 3 and keeps their fp64 scores in registers;
//                           the two states left of them come through a double-buffered LDS array, ONE barrier per frame.
//                           Scores are fetched AL_PF frames ahead of the dependent chain.  Back-pointers: 2 bits a cell, so a
//                           thread's four states are one byte; AL_CH frames are collected in LDS and flushed with 16-byte
//                           stores.  Backward, a chunk of n frames moves at most A n states: only that band (<= 24 bytes a
//                           frame) comes back into LDS and one wave walks it.
//   align_durations_kernel  one thread per phoneme: the difference of two lower bounds over the row's (monotone) states.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "kernels.h"
#include "model.h"
#include "op_host.h"

namespace {

constexpr int AL_MAX_B = 65535;
constexpr int AL_MAX_STATES = 4096;      // vsp_align_max_states(): 1024 threads of AL_SPT states
constexpr int AL_MAX_FRAMES = 1 << 20;
constexpr int AL_MAX_C = 4096;
constexpr int AL_SPT = 4;                // states per thread of the path kernel: their back-pointers are one byte
constexpr int AL_CH = 32;                // frames per back-pointer chunk
constexpr int AL_PF = 8;                 // frames of scores in flight ahead of the chain
constexpr int AL_BAND = 24;              // bytes of a frame's back-pointers the walk back can touch in a chunk (A AL_CH / 4 + 2,
                                         // the start rounded down to a word)
constexpr int AL_TJ = 64, AL_TK = 64;    // the score tile
constexpr int AL_CS = 16;                // channels per LDS slab

const vsp_align_params kAlignDefaults = {2, 0.f, 0.f};

// ------------------------------------------------------------------------------------------------------------ scores
struct ScoreArgs {
  const float* x;        // [B][C][F_max]
  const float* m;        // [B][C][K_max]
  const float* logs;     // [B][C][K_max]
  const int32_t* frames; // [B]
  const int32_t* states; // [B]
  float* S;              // [B][F_max][K_max]
  int C, F_max, K_max;
};

__global__ void __launch_bounds__(256) align_scores_kernel(const ScoreArgs g) {
  __shared__ __align__(16) float s_x[AL_CS][AL_TJ];
  __shared__ __align__(16) float s_m[AL_CS][AL_TK];
  __shared__ __align__(16) float s_w[AL_CS][AL_TK];
  __shared__ float s_c[4][AL_TK];
  const int b = blockIdx.z, j0 = blockIdx.y * AL_TJ, k0 = blockIdx.x * AL_TK, tid = threadIdx.x;
  const int F = g.frames[b], K = g.states[b];
  const int tk = tid & 15, tj = tid >> 4;          // this thread's cells: j0 + 4 tj + {0..3}, k0 + 4 tk + {0..3}
  float* __restrict__ S = g.S + (size_t)b * g.F_max * g.K_max;
  if (j0 >= F || k0 >= K) {                        // (uniform) a tile outside the row's extent: zeros, nothing read
    for (int a = 0; a < 4; ++a)
      for (int c = 0; c < 4; ++c) {
        const int j = j0 + 4 * tj + a, k = k0 + 4 * tk + c;
        if (j < g.F_max && k < g.K_max) S[(size_t)j * g.K_max + k] = 0.f;
      }
    return;
  }
  const float* __restrict__ x = g.x + (size_t)b * g.C * g.F_max;
  const float* __restrict__ m = g.m + (size_t)b * g.C * g.K_max;
  const float* __restrict__ logs = g.logs + (size_t)b * g.C * g.K_max;
  // staging: thread -> column (tid & 63) of the channels (tid >> 6) + 4 i of a slab
  const int sc = tid & 63, sr = tid >> 6;
  const bool jin = j0 + sc < F, kin = k0 + sc < K;
  float acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[a][c] = 0.f;
  float lsum = 0.f;                                // sum of logs of column sc over the channels == sr (mod 4), ascending
  for (int c0 = 0; c0 < g.C; c0 += AL_CS) {
#pragma unroll
    for (int i = 0; i < AL_CS / 4; ++i) {
      const int cl = sr + 4 * i, c = c0 + cl;
      float xv = 0.f, mv = 0.f, wv = 0.f;
      if (c < g.C) {
        if (jin) xv = x[(size_t)c * g.F_max + j0 + sc];
        if (kin) {
          mv = m[(size_t)c * g.K_max + k0 + sc];
          const float lv = logs[(size_t)c * g.K_max + k0 + sc];
          wv = -0.5f * expf(-2.f * lv);
          lsum += lv;
        }
      }
      s_x[cl][sc] = xv;
      s_m[cl][sc] = mv;
      s_w[cl][sc] = wv;
    }
    __syncthreads();
#pragma unroll
    for (int cl = 0; cl < AL_CS; ++cl) {
      const float4 xv = *reinterpret_cast<const float4*>(&s_x[cl][4 * tj]);
      const float4 mv = *reinterpret_cast<const float4*>(&s_m[cl][4 * tk]);
      const float4 wv = *reinterpret_cast<const float4*>(&s_w[cl][4 * tk]);
      const float xa[4] = {xv.x, xv.y, xv.z, xv.w}, ma[4] = {mv.x, mv.y, mv.z, mv.w}, wa[4] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float d = xa[a] - ma[c];
          acc[a][c] = fmaf(wa[c], d * d, acc[a][c]);
        }
    }
    __syncthreads();
  }
  s_c[sr][sc] = lsum;
  __syncthreads();
  float ck[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int col = 4 * tk + c;
    ck[c] = ((s_c[0][col] + s_c[1][col]) + s_c[2][col]) + s_c[3][col];
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = j0 + 4 * tj + a, k = k0 + 4 * tk + c;
      if (j < g.F_max && k < g.K_max) S[(size_t)j * g.K_max + k] = (j < F && k < K) ? acc[a][c] - ck[c] : 0.f;
    }
}

// ------------------------------------------------------------------------------------------------------------ path
struct PathArgs {
  const float* S;          // [B][F_max][K_max]
  const int32_t* frames;   // [B]
  const int32_t* states;   // [B]
  uint8_t* bp;             // [B][F_max][RB] scratch: a byte = the advances (2 bits each) into the states 4t .. 4t + 3
  int32_t* path;           // [B][F_max]
  int F_max, K_max, RB;    // RB = blockDim.x, a multiple of 64
  int A;
  float stay_cost, skip_cost;
};

__global__ void __launch_bounds__(1024) align_path_kernel(const PathArgs g) {
  extern __shared__ __align__(16) uint8_t al_lds[];
  // [edge: 2 buffers x RB x 2 doubles][bp chunk: AL_CH x RB bytes] ; the walk back reuses the chunk's bytes
  double2* s_edge = reinterpret_cast<double2*>(al_lds);
  uint8_t* s_bp = al_lds + (size_t)2 * g.RB * sizeof(double2);
  const int b = blockIdx.x, t = threadIdx.x, RB = g.RB;
  const int F = g.frames[b], K = g.states[b];
  const float* __restrict__ S = g.S + (size_t)b * g.F_max * g.K_max;
  uint8_t* bp = g.bp + (size_t)b * g.F_max * RB;
  int32_t* path = g.path + (size_t)b * g.F_max;
  for (int j = F + t; j < g.F_max; j += RB) path[j] = 0;

  const int k0 = AL_SPT * t;
  const double NEG = -INFINITY;
  const double stay = (double)g.stay_cost, skip = (double)g.skip_cost;
  const bool two = g.A == 2;
  // scores in flight: frame j lives in ring slot j % AL_PF
  float ring[AL_PF][AL_SPT];
  auto fetch = [&](int j, float (&dst)[AL_SPT]) {
#pragma unroll
    for (int i = 0; i < AL_SPT; ++i) {
      dst[i] = 0.f;
      if (j < F && k0 + i < K) dst[i] = S[(size_t)j * g.K_max + k0 + i];
    }
  };
#pragma unroll
  for (int p = 0; p < AL_PF; ++p) fetch(p, ring[p]);

  double q[AL_SPT];
  for (int base = 0; base < F; base += AL_PF) {          // AL_CH is a multiple of AL_PF: a chunk ends on a group's end
#pragma unroll
    for (int p = 0; p < AL_PF; ++p) {
      const int j = base + p;
      if (j < F) {                                       // (uniform)
        float sc[AL_SPT];
#pragma unroll
        for (int i = 0; i < AL_SPT; ++i) sc[i] = ring[p][i];
        fetch(j + AL_PF, ring[p]);                       // the slot's next frame, issued ahead of the chain below
        unsigned byte = 0;
        if (j == 0) {
#pragma unroll
          for (int i = 0; i < AL_SPT; ++i) q[i] = (k0 + i == 0) ? (double)sc[i] : NEG;
        } else {
          double2 left = make_double2(NEG, NEG);         // Q_{j-1}(k0 - 2), Q_{j-1}(k0 - 1)
          if (t > 0) left = s_edge[(size_t)((j - 1) & 1) * RB + t - 1];
          const double prev[AL_SPT + 2] = {left.x, left.y, q[0], q[1], q[2], q[3]};
#pragma unroll
          for (int i = 0; i < AL_SPT; ++i) {
            double best = prev[i + 2] - stay;
            unsigned adv = 0;
            if (prev[i + 1] > best) { best = prev[i + 1]; adv = 1; }
            if (two) {
              const double p2 = prev[i] - skip;
              if (p2 > best) { best = p2; adv = 2; }
            }
            q[i] = (double)sc[i] + best;
            byte |= adv << (2 * i);
          }
        }
        s_edge[(size_t)(j & 1) * RB + t] = make_double2(q[2], q[3]);
        s_bp[(size_t)(j % AL_CH) * RB + t] = (uint8_t)byte;
        __syncthreads();
      }
    }
    const int done = min(base + AL_PF, F);
    if (done % AL_CH == 0 || done == F) {                // (uniform) flush the chunk: its frames' rows are contiguous
      const int first = ((done - 1) / AL_CH) * AL_CH, n = done - first;
      const uint4* src = reinterpret_cast<const uint4*>(s_bp);
      uint4* dst = reinterpret_cast<uint4*>(bp + (size_t)first * RB);
      for (int i = t; i < n * (RB / 16); i += RB) dst[i] = src[i];
      __syncthreads();
    }
  }
  // the flushes above were written by this block: make them visible to its own loads below
  __threadfence();
  __syncthreads();

  // backward: frame F - 1 is in state K - 1; a chunk's band comes into LDS, wave 0 walks it
  uint32_t* s_band = reinterpret_cast<uint32_t*>(s_bp);       // [AL_CH][AL_BAND / 4]
  int32_t* s_next = reinterpret_cast<int32_t*>(s_bp + AL_CH * AL_BAND);
  int k = K - 1;
  for (int first = ((F - 1) / AL_CH) * AL_CH; first >= 0; first -= AL_CH) {
    const int n = min(AL_CH, F - first);
    const int lo = max(0, k - g.A * n);
    const int byte0 = (lo >> 2) & ~3;                    // (a word's start; k / 4 - byte0 < AL_BAND)
    constexpr int WPF = AL_BAND / 4;
    for (int e = t; e < n * WPF; e += RB) {
      const int fr = e / WPF, w = e - fr * WPF, off = byte0 + 4 * w;
      s_band[e] = off < RB ? *reinterpret_cast<const uint32_t*>(bp + (size_t)(first + fr) * RB + off) : 0u;
    }
    __syncthreads();
    if (t < 64) {
      int mine = 0;
      for (int i = n - 1; i >= 0; --i) {                 // every lane walks alike: the reads are broadcasts
        if (t == i) mine = k;
        const int rel = (k >> 2) - byte0;
        const unsigned word = s_band[i * WPF + (rel >> 2)];
        const unsigned adv = (word >> (8 * (rel & 3) + 2 * (k & 3))) & 3u;
        k -= (first + i > 0) ? (int)adv : 0;
      }
      if (t < n) path[first + t] = mine;
      if (t == 0) *s_next = k;                           // (the other waves get the chunk's last state through LDS)
    }
    __syncthreads();
    k = *s_next;
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------------------ durations
struct DurArgs {
  const int32_t* path;     // [B][F_max]
  const int32_t* frames;   // [B]
  const int32_t* cum;      // [B][Tp] inclusive
  const int32_t* lengths;  // [B]
  int32_t* dur;            // [B][Tp]
  int F_max, Tp;
};

__device__ __forceinline__ int al_lower_bound(const int32_t* __restrict__ p, int n, int v) {   // first j with p[j] >= v
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (p[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(256) align_durations_kernel(const DurArgs g) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= g.Tp) return;
  int d = 0;
  if (i < g.lengths[b]) {
    const int32_t* __restrict__ p = g.path + (size_t)b * g.F_max;
    const int F = g.frames[b];
    const int c0 = i > 0 ? g.cum[(size_t)b * g.Tp + i - 1] : 0, c1 = g.cum[(size_t)b * g.Tp + i];
    if (c1 > c0) d = al_lower_bound(p, F, c1) - al_lower_bound(p, F, c0);
  }
  g.dur[(size_t)b * g.Tp + i] = d;
}

// ------------------------------------------------------------------------------------------------------------ host
using vsp::Call;
using vsp::Ws;

int path_threads(int K_max) { return std::max(64, ((K_max + AL_SPT - 1) / AL_SPT + 63) / 64 * 64); }

// What each call carves from its workspace (op_host.h); the sizes are the dry passes of these.
int32_t* carve_rows(Ws& ws, int B) { return static_cast<int32_t*>(ws.bytes((size_t)2 * B * sizeof(int32_t))); }   // frames [B], states [B]

struct PathWs { int32_t* rows; uint8_t* bp; };
PathWs carve_path(Ws& ws, int B, int F_max, int K_max) {   // (a braced list is evaluated in order)
  return {carve_rows(ws, B), static_cast<uint8_t*>(ws.bytes((size_t)B * F_max * path_threads(std::min(K_max, AL_MAX_STATES))))};
}

int32_t* carve_dur(Ws& ws, int B, int Tp) {                // frames [B], lengths [B], cum [B][Tp]
  return static_cast<int32_t*>(ws.bytes(((size_t)2 * B + (size_t)B * Tp) * sizeof(int32_t)));
}

// vsp_align: [the path's (its rows serve the scores too)] [S] [the durations']
struct AlignWs { PathWs path; float* S; int32_t* dur; };
AlignWs carve_align(Ws& ws, int B, int F_max, int K_max, int Tp) {
  return {carve_path(ws, B, F_max, K_max), ws.f((size_t)B * F_max * K_max), carve_dur(ws, B, Tp)};
}

bool sizes_ok(int B, int F_max, int K_max) {
  return B >= 1 && B <= AL_MAX_B && F_max >= 1 && F_max <= AL_MAX_FRAMES && K_max >= 1 && K_max <= AL_MAX_FRAMES &&
         (int64_t)B * F_max * K_max <= ((int64_t)1 << 40);
}

// The rows of a call: 1 <= F_b <= F_max, 1 <= K_b <= K_max; with `pp` also the path's own conditions.  Fills fk = frames, states.
int check_rows(vsp_ctx* ctx, const char* who, int B, int F_max, int K_max, const int64_t* frames_host, const int64_t* states_host,
               const vsp_align_params* pp, std::vector<int32_t>& fk) {
  fk.resize((size_t)2 * B);
  for (int b = 0; b < B; ++b) {
    const int64_t F = frames_host[b], K = states_host[b];
    if (F < 1 || F > F_max) return ctx->fail(VSP_ERR_ARG, "%s: row %d has %lld frames: 1 <= frames <= F_max = %d", who, b, (long long)F, F_max);
    if (K < 1 || K > K_max) return ctx->fail(VSP_ERR_ARG, "%s: row %d has %lld states: 1 <= states <= K_max = %d", who, b, (long long)K, K_max);
    if (pp) {
      if (K > AL_MAX_STATES)
        return ctx->fail(VSP_ERR_ARG, "%s: row %d has %lld states: the limit is %d (vsp_align_max_states)", who, b, (long long)K, AL_MAX_STATES);
      if (K > (int64_t)pp->max_advance * (F - 1) + 1)
        return ctx->fail(VSP_ERR_ARG, "%s: row %d is infeasible: %lld frames cannot reach %lld states advancing at most %d a frame "
                         "(states <= max_advance (frames - 1) + 1)", who, b, (long long)F, (long long)K, pp->max_advance);
    }
    fk[b] = (int32_t)F;
    fk[(size_t)B + b] = (int32_t)K;
  }
  return VSP_OK;
}

int check_params(vsp_ctx* ctx, const char* who, const vsp_align_params* params, vsp_align_params& pp) {
  pp = params ? *params : kAlignDefaults;
  if (pp.max_advance != 1 && pp.max_advance != 2) return ctx->fail(VSP_ERR_ARG, "%s: max_advance must be 1 or 2", who);
  if (!(pp.stay_cost >= 0.f && pp.stay_cost < 1e30f) || !(pp.skip_cost >= 0.f && pp.skip_cost < 1e30f))
    return ctx->fail(VSP_ERR_ARG, "%s: the stay cost and the skip cost must be at least 0", who);
  return VSP_OK;
}

// The phoneme side of a row: 1 <= length <= Tp (a row of no phonemes is refused), cum_dur non-decreasing from >= 0, and --
// where states_host is given (vsp_align) -- its last entry the row's states.
int check_cum(vsp_ctx* ctx, const char* who, int B, int Tp, const int32_t* cum_host, const int64_t* lengths_host,
              const int64_t* states_host) {
  for (int b = 0; b < B; ++b) {
    const int64_t L = lengths_host[b];
    if (L < 1 || L > Tp) return ctx->fail(VSP_ERR_ARG, "%s: row %d has %lld phonemes: 1 <= length <= Tp = %d", who, b, (long long)L, Tp);
    int32_t prev = 0;
    for (int i = 0; i < (int)L; ++i) {
      const int32_t c = cum_host[(size_t)b * Tp + i];
      if (c < prev) return ctx->fail(VSP_ERR_ARG, "%s: row %d: cum_dur decreases at phoneme %d", who, b, i);
      prev = c;
    }
    if (states_host && prev != states_host[b])
      return ctx->fail(VSP_ERR_ARG, "%s: row %d: cum_dur ends at %d, the row has %lld states", who, b, (int)prev, (long long)states_host[b]);
  }
  return VSP_OK;
}

int launch_scores(const Call& call, int B, int C, int F_max, int K_max, const float* x, const float* m, const float* logs,
                  const int32_t* rows_dev, float* S) {
  ScoreArgs a;
  a.x = x; a.m = m; a.logs = logs; a.frames = rows_dev; a.states = rows_dev + B; a.S = S;
  a.C = C; a.F_max = F_max; a.K_max = K_max;
  const dim3 grid((K_max + AL_TK - 1) / AL_TK, (F_max + AL_TJ - 1) / AL_TJ, B);
  hipLaunchKernelGGL(align_scores_kernel, grid, dim3(256), 0, call.s, a);
  return call.launched("align_scores_kernel");
}

int launch_path(const Call& call, int B, int F_max, int K_max, int K_top, const float* S, const int32_t* rows_dev,
                const vsp_align_params& pp, int32_t* states, uint8_t* bp) {
  PathArgs a;
  a.S = S; a.frames = rows_dev; a.states = rows_dev + B; a.bp = bp; a.path = states;
  a.F_max = F_max; a.K_max = K_max; a.RB = path_threads(K_top);
  a.A = pp.max_advance; a.stay_cost = pp.stay_cost; a.skip_cost = pp.skip_cost;
  const size_t lds = (size_t)2 * a.RB * sizeof(double2) + std::max((size_t)AL_CH * a.RB, (size_t)AL_CH * AL_BAND + sizeof(int32_t));
  hipLaunchKernelGGL(align_path_kernel, dim3(B), dim3(a.RB), lds, call.s, a);      // (at most 64 KiB: no attribute to raise)
  return call.launched("align_path_kernel");
}

int launch_durations(const Call& call, int B, int F_max, int Tp, const int32_t* states, const int64_t* frames_host,
                     const int32_t* cum_host, const int64_t* lengths_host, int32_t* durations, int32_t* dev) {
  std::vector<int32_t> ints((size_t)2 * B + (size_t)B * Tp, 0);
  for (int b = 0; b < B; ++b) {
    ints[b] = (int32_t)frames_host[b];
    ints[(size_t)B + b] = (int32_t)lengths_host[b];
    std::memcpy(&ints[(size_t)2 * B + (size_t)b * Tp], cum_host + (size_t)b * Tp, (size_t)lengths_host[b] * sizeof(int32_t));
  }
  if (const int rc = call.upload(dev, ints.data(), ints.size() * sizeof(int32_t))) return rc;
  DurArgs a;
  a.path = states;
  a.frames = dev;
  a.lengths = a.frames + B;
  a.cum = a.lengths + B;
  a.dur = durations; a.F_max = F_max; a.Tp = Tp;
  hipLaunchKernelGGL(align_durations_kernel, dim3((Tp + 255) / 256, B), dim3(256), 0, call.s, a);
  return call.launched("align_durations_kernel");
}

}  // namespace

int vsp_align_max_states(void) { return AL_MAX_STATES; }

int64_t vsp_align_scores_workspace_bytes(int B, int F_max, int K_max) {
  if (!sizes_ok(B, F_max, K_max)) return VSP_ERR_ARG;
  Ws ws = vsp::dry_ws();
  carve_rows(ws, B);
  return (int64_t)ws.cur;
}

int64_t vsp_align_path_workspace_bytes(int B, int F_max, int K_max) {
  if (!sizes_ok(B, F_max, K_max)) return VSP_ERR_ARG;
  Ws ws = vsp::dry_ws();
  carve_path(ws, B, F_max, K_max);
  return (int64_t)ws.cur;
}

int64_t vsp_align_workspace_bytes(int B, int F_max, int K_max, int Tp) {
  if (!sizes_ok(B, F_max, K_max) || Tp < 1 || (int64_t)B * Tp > ((int64_t)1 << 28)) return VSP_ERR_ARG;
  Ws ws = vsp::dry_ws();
  carve_align(ws, B, F_max, K_max, Tp);
  return (int64_t)ws.cur;
}

int vsp_align_scores(vsp_ctx* ctx, void* stream, int B, int C, int F_max, int K_max, const float* x, const float* m, const float* logs,
                     const int64_t* frames_host, const int64_t* states_host, float* scores, void* workspace, int64_t workspace_bytes) {
  if (!ctx) return VSP_ERR_ARG;
  const char* who = "vsp_align_scores";
  if (!sizes_ok(B, F_max, K_max) || C < 1 || C > AL_MAX_C || !frames_host || !states_host)
    return ctx->fail(VSP_ERR_ARG, "%s: 1 <= B <= %d rows, 1 <= C <= %d, F_max, K_max >= 1, and the rows' frames and states", who, AL_MAX_B,
                     AL_MAX_C);
  std::vector<int32_t> fk;
  if (const int rc = check_rows(ctx, who, B, F_max, K_max, frames_host, states_host, nullptr, fk)) return rc;
  if (!x || !m || !logs || !scores) return ctx->fail(VSP_ERR_ARG, "%s: null pointer", who);
  const Call call{ctx, who, (hipStream_t)stream};
  Ws ws = call.open(workspace, workspace_bytes);
  int32_t* rows = carve_rows(ws, B);
  if (const int rc = call.need_ws(workspace, workspace_bytes, ws.cur)) return rc;
  if (const int rc = call.upload(rows, fk.data(), fk.size() * sizeof(int32_t))) return rc;
  return launch_scores(call, B, C, F_max, K_max, x, m, logs, rows, scores);
}

int vsp_align_path(vsp_ctx* ctx, void* stream, int B, int F_max, int K_max, const float* scores, const int64_t* frames_host,
                   const int64_t* states_host, const vsp_align_params* params, int32_t* states, void* workspace,
                   int64_t workspace_bytes) {
  if (!ctx) return VSP_ERR_ARG;
  const char* who = "vsp_align_path";
  vsp_align_params pp;
  if (const int rc = check_params(ctx, who, params, pp)) return rc;
  if (!sizes_ok(B, F_max, K_max) || !frames_host || !states_host)
    return ctx->fail(VSP_ERR_ARG, "%s: 1 <= B <= %d rows, F_max, K_max >= 1, and the rows' frames and states", who, AL_MAX_B);
  std::vector<int32_t> fk;
  if (const int rc = check_rows(ctx, who, B, F_max, K_max, frames_host, states_host, &pp, fk)) return rc;
  if (!scores || !states) return ctx->fail(VSP_ERR_ARG, "%s: null pointer", who);
  const Call call{ctx, who, (hipStream_t)stream};
  Ws ws = call.open(workspace, workspace_bytes);
  const PathWs w = carve_path(ws, B, F_max, K_max);
  if (const int rc = call.need_ws(workspace, workspace_bytes, ws.cur)) return rc;
  if (const int rc = call.upload(w.rows, fk.data(), fk.size() * sizeof(int32_t))) return rc;
  const int K_top = *std::max_element(fk.begin() + B, fk.end());
  return launch_path(call, B, F_max, K_max, K_top, scores, w.rows, pp, states, w.bp);
}

int vsp_align_durations(vsp_ctx* ctx, void* stream, int B, int F_max, int Tp, const int32_t* states, const int64_t* frames_host,
                        const int32_t* cum_dur_host, const int64_t* lengths_host, int32_t* durations, void* workspace,
                        int64_t workspace_bytes) {
  if (!ctx) return VSP_ERR_ARG;
  const char* who = "vsp_align_durations";
  if (B < 1 || B > AL_MAX_B || F_max < 1 || F_max > AL_MAX_FRAMES || Tp < 1 || (int64_t)B * Tp > ((int64_t)1 << 28) || !frames_host ||
      !cum_dur_host || !lengths_host)
    return ctx->fail(VSP_ERR_ARG, "%s: 1 <= B <= %d rows, F_max >= 1, Tp >= 1, and the host arrays", who, AL_MAX_B);
  for (int b = 0; b < B; ++b)
    if (frames_host[b] < 1 || frames_host[b] > F_max)
      return ctx->fail(VSP_ERR_ARG, "%s: row %d has %lld frames: 1 <= frames <= F_max = %d", who, b, (long long)frames_host[b], F_max);
  if (const int rc = check_cum(ctx, who, B, Tp, cum_dur_host, lengths_host, nullptr)) return rc;
  if (!states || !durations) return ctx->fail(VSP_ERR_ARG, "%s: null pointer", who);
  const Call call{ctx, who, (hipStream_t)stream};
  Ws ws = call.open(workspace, workspace_bytes);
  int32_t* dev = carve_dur(ws, B, Tp);
  if (const int rc = call.need_ws(workspace, workspace_bytes, ws.cur)) return rc;
  return launch_durations(call, B, F_max, Tp, states, frames_host, cum_dur_host, lengths_host, durations, dev);
}

int vsp_align(vsp_ctx* ctx, void* stream, int B, int C, int F_max, int K_max, int Tp, const float* x, const float* m, const float* logs,
              const int64_t* frames_host, const int64_t* states_host, const int32_t* cum_dur_host, const int64_t* lengths_host,
              const vsp_align_params* params, int32_t* states, int32_t* durations, void* workspace, int64_t workspace_bytes) {
  if (!ctx) return VSP_ERR_ARG;
  const char* who = "vsp_align";
  vsp_align_params pp;
  if (const int rc = check_params(ctx, who, params, pp)) return rc;
  if (!sizes_ok(B, F_max, K_max) || C < 1 || C > AL_MAX_C || Tp < 1 || (int64_t)B * Tp > ((int64_t)1 << 28) || !frames_host ||
      !states_host || !cum_dur_host || !lengths_host)
    return ctx->fail(VSP_ERR_ARG, "%s: 1 <= B <= %d rows, 1 <= C <= %d, F_max, K_max, Tp >= 1, and the host arrays", who, AL_MAX_B, AL_MAX_C);
  std::vector<int32_t> fk;
  if (const int rc = check_rows(ctx, who, B, F_max, K_max, frames_host, states_host, &pp, fk)) return rc;
  if (const int rc = check_cum(ctx, who, B, Tp, cum_dur_host, lengths_host, states_host)) return rc;
  if (!x || !m || !logs || !states || !durations) return ctx->fail(VSP_ERR_ARG, "%s: null pointer", who);
  const Call call{ctx, who, (hipStream_t)stream};
  Ws ws = call.open(workspace, workspace_bytes);
  const AlignWs w = carve_align(ws, B, F_max, K_max, Tp);
  if (const int rc = call.need_ws(workspace, workspace_bytes, ws.cur)) return rc;
  if (const int rc = call.upload(w.path.rows, fk.data(), fk.size() * sizeof(int32_t))) return rc;
  if (const int rc = launch_scores(call, B, C, F_max, K_max, x, m, logs, w.path.rows, w.S)) return rc;
  const int K_top = *std::max_element(fk.begin() + B, fk.end());
  if (const int rc = launch_path(call, B, F_max, K_max, K_top, w.S, w.path.rows, pp, states, w.path.bp)) return rc;
  return launch_durations(call, B, F_max, Tp, states, frames_host, cum_dur_host, lengths_host, durations, w.dur);
}
