// The one resampling core of the output stage (resample.hip), the input stage (input_stage.hip) and the output rows
// (output_rows.hip): the plan and the Kaiser-windowed sinc of include/vispeech_hip.h ("output stage" / "input stage": one
// formula, the rates swapped), the polyphase table [P][L] all kernels read, and
//   device  rs_one_output  one output sample from global memory (mode 2 of all three kernels, stream_output_kernel)
//           rs_tile_output the same FMA chain from a tile staged in LDS (mode 0 of all three): geometry, staging passes, FMAs
//           out_store      an output sample in its encoding (float32, PCM16, G.711), packed stores where the row allows
//   host    stage_plan     how a kernel stages a rate: taps per pass, mode, LDS words
//           configure_rate a rate's table built, uploaded and swapped into a slot of the context; find_rate, drop_rate
//           plan_api, filter_api   the bodies of vsp_resample_plan / vsp_input_plan and vsp_resample_filter / vsp_input_filter
// The three kernels keep what is theirs: how a sample is fetched and what a 16-byte load of their rows decodes to.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

#include "model.h"

namespace vsp {
namespace rs {

constexpr int RS_TILE = 256;      // output samples (= threads) per block, in every kernel of this header
constexpr int RS_MIN_PASS = 32;   // fewer taps per staging pass than this: read x from global memory instead
constexpr int OUT_MAX_L = 320, OUT_MAX_M = 441;   // what the output stage and the output rows cover

// One output sample from global memory: acc = fmaf(tab[i][m mod L], x[ks + i], acc), i = 0 .. P - 1 ascending, ks =
// floor(m M / L) - J; `sample(k)` is input sample k of the utterance, 0 where it is not readable.  rs_tile_output runs this
// very chain.
template <class Sample>
__device__ __forceinline__ float rs_one_output(const float* __restrict__ tab, int L, int M, int J, int P, int64_t m, Sample sample) {
  const float* __restrict__ tcol = tab + (int)(m % L);
  const int64_t ks = (m * M) / L - J;
  float acc = 0.f;
#pragma unroll 4
  for (int i = 0; i < P; ++i) acc = fmaf(tcol[(size_t)i * L], sample(ks + i), acc);   // (loads in flight; the order stays)
  return acc;
}

// The lane's output sample of the tile [m_first, m_last] (lane t: m_first + t; lanes behind m_last shadow m_last, so their
// offsets stay in the tile) from a staged tile: the block writes the tile's input span to xs `pass` taps at a time (pass a
// multiple of 4 and of E when there is more than one) and every lane runs the chain of rs_one_output on it.  E = the
// elements of an aligned 16-byte load of the row; `load(k, v)` decodes the load that starts at sample k into v[0 .. E),
// called for kb <= k with [k, k + E) inside [vlo, vhi) only; everywhere else `sample(k)` is selected per element.  The
// tile's first staged sample kb is moved down to a 16-byte boundary: a0 + k is sample k's element index in memory (mod E).
// E = 1: no vector loads.  All RS_TILE threads call it (barriers); xs holds stage_plan's xs_words.
template <int E, class Load, class Sample>
__device__ __forceinline__ float rs_tile_output(float* xs, const float* __restrict__ tab, int L, int M, int J, int P, int pass,
                                                int64_t m_first, int64_t m_last, int64_t a0, int64_t vlo, int64_t vhi,
                                                Load load, Sample sample) {
  const int tid = threadIdx.x;
  const int64_t mm = min(m_first + tid, m_last);
  const int64_t ks = (mm * M) / L - J;                             // first input sample of this output
  const unsigned col = (unsigned)(mm % L);
  int64_t kb = (m_first * M) / L - J;                              // first input sample of the tile
  kb -= (a0 + kb) & (E - 1);
  const int off = (int)(ks - kb);
  const int span = (int)((m_last * M) / L - J - kb) + 1;           // tile words before the pass's taps are added
  float acc = 0.f;
  for (int i0 = 0; i0 < P; i0 += pass) {
    const int n_i = min(pass, P - i0);
    const int need = span + n_i - 1;
    const int64_t k_base = kb + i0;
    if (i0) __syncthreads();
    for (int o = tid * E; o < need; o += RS_TILE * E) {
      const int64_t k = k_base + o;
      float v[E];
      if (E > 1 && k >= vlo && k + E <= vhi) {
        load(k, v);
      } else {
#pragma unroll
        for (int q = 0; q < E; ++q) v[q] = sample(k + q);
      }
      if (E == 1) xs[o] = v[0];
#pragma unroll
      for (int q = 0; q + 4 <= E; q += 4) *reinterpret_cast<float4*>(xs + o + q) = make_float4(v[q], v[q + 1], v[q + 2], v[q + 3]);
    }
    __syncthreads();
    // tab[i0 + i][col] at byte offset tb from the (uniform) table: a 32-bit offset per load (the table is < 1 MiB), which
    // keeps the address arithmetic of this latency-bound loop to one add per load.  The loop is unrolled by four here and
    // no further (unroll 1): unrolled again it holds 16 loads and 20 more registers.
    const unsigned row = 4u * (unsigned)L;
    unsigned tb = 4u * (col + (unsigned)i0 * (unsigned)L);
    auto tap = [&](unsigned byte) { return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(tab) + byte); };
    const float* xo = xs + off;
    int i = 0;
#pragma unroll 1
    for (; i + 4 <= n_i; i += 4, tb += 4 * row) {                  // (four table loads in flight; the FMA order stays ascending)
      const float t0 = tap(tb), t1 = tap(tb + row), t2 = tap(tb + 2 * row), t3 = tap(tb + 3 * row);
      acc = fmaf(t0, xo[i], acc);
      acc = fmaf(t1, xo[i + 1], acc);
      acc = fmaf(t2, xo[i + 2], acc);
      acc = fmaf(t3, xo[i + 3], acc);
    }
    for (; i < n_i; ++i, tb += row) acc = fmaf(tap(tb), xo[i], acc);
  }
  return acc;
}

// The PCM16 value of an output sample
__device__ __forceinline__ int rs_pcm16(float y) {
  // service.pcm16: clip(rint(y * 32767.0f), -32768, 32767), product in fp32, round half to even
  const float r = rintf(y * 32767.0f);
  return (int)fminf(fmaxf(r, -32768.f), 32767.f);
}

// Stores element j of a row in its encoding VSP_OUT_*.  Every lane of the block calls it (the shuffles take all of them)
// with a valid y; lanes with j < fill store.  j - threadIdx.x is a multiple of RS_TILE, so j and the lane agree modulo 2 and
// 4.  Where the row's `out` is 4-byte aligned, PCM16 goes as packed pairs from even lanes and G.711 four codes to a 32-bit
// store; single elements only at a row's ragged end.
__device__ __forceinline__ void out_store(void* out, int enc, int64_t j, float y, int64_t fill) {
  const bool active = j < fill;
  if (enc == VSP_OUT_F32) {
    if (active) static_cast<float*>(out)[j] = y;
    return;
  }
  const int q = rs_pcm16(y);
  const bool word_ok = ((uintptr_t)out & 3) == 0;
  if (enc == VSP_OUT_S16) {
    const int q_next = __shfl_down(q, 1);
    int16_t* o = static_cast<int16_t*>(out) + j;
    if (word_ok) {
      if (!(threadIdx.x & 1) && active) {
        if (j + 1 < fill) *reinterpret_cast<uint32_t*>(o) = (uint32_t)(q & 0xffff) | ((uint32_t)q_next << 16);
        else *o = (int16_t)q;
      }
    } else if (active) {
      *o = (int16_t)q;
    }
    return;
  }
  const uint32_t c = (uint32_t)(enc == VSP_OUT_ULAW ? g711_ulaw_code(q) : g711_alaw_code(q));
  const uint32_t c1 = __shfl_down(c, 1), c2 = __shfl_down(c, 2), c3 = __shfl_down(c, 3);
  uint8_t* o = static_cast<uint8_t*>(out) + j;
  if (word_ok && (j | 3) < fill) {                                  // the lane's whole group of four is stored
    if (!(threadIdx.x & 3)) *reinterpret_cast<uint32_t*>(o) = c | (c1 << 8) | (c2 << 16) | (c3 << 24);
  } else if (active) {
    *o = (uint8_t)c;
  }
}

// ------------------------------------------------------------------------------------------------------------- host
static_assert(VSP_IN_F32 == VSP_OUT_F32 && VSP_IN_S16 == VSP_OUT_S16 && VSP_IN_ULAW == VSP_OUT_ULAW && VSP_IN_ALAW == VSP_OUT_ALAW,
              "one encoding numbering on the way in and out");
inline int enc_bytes(int enc) { return enc == VSP_OUT_F32 ? 4 : enc == VSP_OUT_S16 ? 2 : 1; }

// How a kernel stages a rate.  mode 0: the tile's span in LDS, `pass` taps per staging pass (P, or a multiple of `gran`);
// mode 2: samples from global memory (the span leaves no room for RS_MIN_PASS taps).  Tile words: the outputs of a tile
// start within (TILE - 1) M / L + 1 samples of each other, + `slack` for the alignment of the first; `overhang`: what the
// last 16-byte store of a pass may write behind the words it needs.
struct StagePlan { int pass, mode, xs_words; };
inline StagePlan stage_plan(int lds_floats, int slack, int overhang, int gran, int L, int M, int P) {
  const int64_t span = ((int64_t)(RS_TILE - 1) * M) / L + 2 + slack;
  const int64_t room = lds_floats - span - overhang;
  if (room < std::min<int64_t>(P, RS_MIN_PASS)) return {P, 2, 0};
  const int pass = room >= P ? P : (int)(room & ~(int64_t)(gran - 1));
  return {pass, 0, (int)((span + pass + overhang + 3) & ~(int64_t)3)};
}

inline double bessel_i0(double x) {
  const double q = x * x / 4.0;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 500; ++k) {
    term *= q / ((double)k * k);
    sum += term;
    if (term < sum * 1e-18) break;
  }
  return sum;
}

struct Plan { int L = 0, M = 0, H = 0; };

// from_rate -> to_rate by L / M; the stages differ only in the largest L and M their kernels cover
inline int make_plan(int from_rate, int to_rate, int zeros, int max_L, int max_M, Plan& p) {
  if (from_rate <= 0 || to_rate <= 0 || zeros < 1) return VSP_ERR_ARG;
  const int g = std::gcd(from_rate, to_rate);
  p.L = to_rate / g;
  p.M = from_rate / g;
  if (p.L > max_L || p.M > max_M || zeros > 64) return VSP_ERR_UNSUPPORTED;
  p.H = (p.L == 1 && p.M == 1) ? 0 : zeros * std::max(p.L, p.M);    // L = M = 1: the pass-through, one unit tap
  return VSP_OK;
}

// h[n], n = -H .. H, in double precision (numpy's sinc and kaiser conventions)
inline void make_filter(const Plan& p, int zeros, double beta, double rolloff, std::vector<double>& h) {
  const int H = p.H;
  h.assign((size_t)2 * H + 1, 0.0);
  if (H == 0) { h[0] = 1.0; return; }
  const double fc = rolloff / std::max(p.L, p.M);
  const double i0b = bessel_i0(beta);
  const double pi = 3.14159265358979323846;
  for (int n = -H; n <= H; ++n) {
    const double r = (double)n / H;
    const double w = bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
    const double a = pi * fc * n;
    const double s = n == 0 ? 1.0 : std::sin(a) / a;
    h[(size_t)(n + H)] = p.L * fc * s * w;
  }
}

inline double default_rolloff(int zeros) { return 1.0 - 3.065 / zeros; }

// The polyphase table of resample.hip's header comment: tab[i][m mod L] = h[p(m) + (J - i) L], i = 0 .. P - 1, J = H / L,
// p(m) = m M mod L, zero where the tap lies outside [-H, H]; input sample k = floor(m M / L) - J + i.
inline void make_table(const Plan& p, const std::vector<double>& h, int& J, int& P, std::vector<float>& tab) {
  const int L = p.L, M = p.M, H = p.H;
  J = H / L;
  P = J + (H + L - 1) / L + 1;
  tab.assign((size_t)P * L, 0.f);
  for (int c = 0; c < L; ++c) {
    const int64_t ph = ((int64_t)c * M) % L;
    for (int i = 0; i < P; ++i) {
      const int64_t t = ph + (int64_t)(J - i) * L;
      if (t >= -H && t <= H) tab[(size_t)i * L + c] = (float)h[(size_t)(t + H)];
    }
  }
}

// vsp_resample_plan / vsp_input_plan (which maps zeros == 0 to 32 first)
inline int plan_api(int from_rate, int to_rate, int zeros, int max_L, int max_M, int* L, int* M, int* half_len) {
  Plan p;
  if (!L || !M || !half_len) return VSP_ERR_ARG;
  if (int rc = make_plan(from_rate, to_rate, zeros, max_L, max_M, p)) return rc;
  *L = p.L; *M = p.M; *half_len = p.H;
  return VSP_OK;
}

// vsp_resample_filter / vsp_input_filter (which maps zeros == 0 to 32 first)
inline int filter_api(int from_rate, int to_rate, int zeros, double beta, double rolloff, int max_L, int max_M, float* taps_host) {
  Plan p;
  if (!taps_host || !(beta >= 0.0) || !(rolloff <= 1.0)) return VSP_ERR_ARG;
  if (int rc = make_plan(from_rate, to_rate, zeros, max_L, max_M, p)) return rc;
  if (!(rolloff > 0.0)) rolloff = default_rolloff(zeros);
  std::vector<double> h;
  make_filter(p, zeros, beta, rolloff, h);
  for (size_t i = 0; i < h.size(); ++i) taps_host[i] = (float)h[i];
  return VSP_OK;
}

// The configured slot of `rate` in a set of tables; with take_free, failing that, a free slot.  nullptr: neither.
inline vsp_ctx::RateTable* find_rate(vsp_ctx::RateTable* set, int n, int rate, bool take_free = false) {
  for (int i = 0; i < n; ++i)
    if (set[i].tab && set[i].rate == rate) return set + i;
  for (int i = 0; take_free && i < n; ++i)
    if (!set[i].tab) return set + i;
  return nullptr;
}

inline void drop_rate(vsp_ctx* ctx, vsp_ctx::RateTable* slot) {
  if (!slot || !slot->tab) return;
  (void)hipSetDevice(ctx->device);
  (void)hipFree(slot->tab);
  *slot = vsp_ctx::RateTable();
}

// Configures from_rate -> to_rate under the key `rate` in a set of n slots of the context: the table is built, uploaded and swapped
// into the key's slot or a free one.  `stage` names the stage in messages, `what` its rates ("input" / "output") where the
// set can be full.  On any failure the set is as it was.
inline int configure_rate(vsp_ctx* ctx, const char* stage, const char* what, vsp_ctx::RateTable* set, int n, int rate,
                          int from_rate, int to_rate, int zeros, double beta, double rolloff, int max_L, int max_M) {
  if (zeros == 0) zeros = 32;
  if (!(beta >= 0.0)) return ctx->fail(VSP_ERR_ARG, "%s: beta must be >= 0", stage);
  if (!(rolloff <= 1.0)) return ctx->fail(VSP_ERR_ARG, "%s: rolloff must be in (0, 1] (<= 0: 1 - 3.065 / zeros)", stage);
  Plan p;
  if (int rc = make_plan(from_rate, to_rate, zeros, max_L, max_M, p))
    return ctx->fail(rc, "%s %d -> %d Hz, %d zeros: rates must be positive, L <= %d, M <= %d, 1 <= zeros <= 64", stage, from_rate,
                     to_rate, zeros, max_L, max_M);
  vsp_ctx::RateTable* slot = find_rate(set, n, rate, true);
  if (!slot) return ctx->fail(VSP_ERR_STATE, "%s: %d %s rates are configured already", stage, n, what);
  if (!(rolloff > 0.0)) rolloff = default_rolloff(zeros);
  std::vector<double> h;
  make_filter(p, zeros, beta, rolloff, h);
  int J, P;
  std::vector<float> tab;
  make_table(p, h, J, P, tab);
  void* d = nullptr;
  hipError_t e = hipSetDevice(ctx->device);
  if (e == hipSuccess) e = hipMalloc(&d, tab.size() * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(d, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (d) (void)hipFree(d);
    return ctx->fail(VSP_ERR_HIP, "%s table: %s", stage, hipGetErrorString(e));
  }
  float* old = slot->tab;
  slot->rate = rate;
  slot->L = p.L; slot->M = p.M; slot->H = p.H; slot->J = J; slot->P = P;
  slot->tab = static_cast<float*>(d);                     // (last: a slot counts as configured once it has a table)
  if (old) (void)hipFree(old);
  return VSP_OK;
}

inline int64_t floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
inline int64_t ceil_div(int64_t a, int64_t b) { return -floor_div(-a, b); }

}  // namespace rs
}  // namespace vsp
