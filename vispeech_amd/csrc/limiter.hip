// True-peak meter and look-ahead limiter (include/vispeech_hip.h, "limiter") per row of a ragged
// batch of mono float32 rows, or of a set of streams each at its own position.  The specification is this project's own
// (fp64 restatement in tests/limiter_ref.py).  There is no recurrence in it: the gain at sample n is a function of
// x[n - (A + H + J) .. n + A + J], so a row is cut into tiles freely, and a stream needs that much history and look-ahead.
//
// All positions of a row are relative to its first PROVIDED sample (stream sample `first`): x(k) = in[k] for 0 <= k < count
// and 0 elsewhere; nothing outside [0, count) is read.  vsp_limiter_rows refuses every row for which a value that reaches an
// output would depend on a sample the caller did not provide, so "outside the provided samples" and "outside the row" agree
// wherever it matters.
//
//   lm_peak_kernel    tiles of LM_T1 samples x rows.  The tile's x with J samples of halo a side is staged into LDS (16-byte
//                     loads where a quad lies inside the provided samples, zeros outside them).  Thread t takes samples t,
//                     t + 256, ...: the lanes of a wave read consecutive words (no bank conflict) and the 97 taps are kernel
//                     arguments, uniform per instruction.  Four FMA chains a sample, ascending k: phase 0 has 25 taps, phases
//                     1 .. 3 have 24.  p = max(|x|, |y0|, |y1|, |y2|, |y3|).
//                       meter:   the block's max p, one unsigned atomic max per block on the float's bits into tp[b].
//                       limiter: r = c / (g p) where g p > c, else 1, written to the row's r buffer in the workspace, which
//                                covers [out_first - A - H, out_first + out_count + A): 1 outside the row.
//   lm_apply_kernel   tiles of LM_T2 outputs x rows.  The tile's r, T + 2 A + H values, is read into LDS and registers; the
//                     sliding minimum over W = A + H + 1 values is log-step doubling in place -- after step i, word j holds
//                     min r[j .. j + 2^i) -- and m = min(word[j], word[j + W - 2^k]), 2^k <= W < 2^(k+1): min is exact, so this
//                     is the specification's m in every bit.  The boxcar is the direct ascending fp32 sum of A + 1 values of
//                     m from LDS, times fl32(1 / (A + 1)); out = clamp((g x) s, -c, c).  x is read at the output's own
//                     position only, so in == out is allowed: the halo lives in r, which is why there are two launches.
//                     min_gain[b] = min s by an unsigned atomic min on the float's bits (s >= 0).
// Per sample: 4 B of x in and 4 B of r out, then 4 B of r and 4 B of x in and 4 B out, against 97 FMAs and A + 1 LDS adds.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <vector>

#include "kernels.h"
#include "model.h"
#include "op_host.h"
#include "resample_common.h"

namespace {

constexpr int LM_J = 12, LM_TAPS = 97, LM_HALF = 48;     // zeros = 12 at L = 4: H = 48, 97 taps, 12 samples a side
constexpr int LM_ZEROS = 12;
constexpr double LM_BETA = 9.62;
constexpr int LM_MAX_A = 1024, LM_MAX_H = 8192;
constexpr int LM_MAX_B = 65535;
constexpr int64_t LM_MAX_SAMPLES = (int64_t)1 << 30;
constexpr int LM_T1 = 1024;                              // samples of a row per block of lm_peak_kernel (256 threads, four each)
constexpr int LM_T2 = 2048;                              // outputs of a row per block of lm_apply_kernel
constexpr int LM_XS = LM_T1 + 2 * LM_J + 8;              // staged words: the tile, its halo, and the alignment of both ends
constexpr int LM_RMAX = LM_T2 + 2 * LM_MAX_A + LM_MAX_H; // r values of a tile at the largest A and H
constexpr int LM_RK = LM_RMAX / 256;                     // ... per thread
static_assert(LM_RMAX % 256 == 0, "r values per thread");

struct Taps { float h[LM_TAPS]; };                       // h[n + 48], n = -48 .. 48

struct Row {                     // uploaded with every call: the head of the workspace
  const float* in;               // in[k]: the row's provided sample k
  float* out;                    // out[o]: output o (the sample at relative position out_off + o)
  float* r;                      // r[i]: the gain wanted at relative position r0 + i
  int32_t count;                 // provided samples
  int32_t r0, r_count;
  int32_t out_off, out_count;
  float ceiling;                 // NaN: the row is neither read nor written
};

template <bool METER>
__global__ void __launch_bounds__(256) lm_peak_kernel(const Row* __restrict__ rows, const float* __restrict__ gains,
                                                      unsigned* tp_bits, unsigned* min_gain_bits, const Taps taps) {
  __shared__ __align__(16) float xs[LM_XS];
  const int b = blockIdx.y, tid = threadIdx.x;
  const Row row = rows[b];
  if (!METER && min_gain_bits && blockIdx.x == 0 && tid == 0) min_gain_bits[b] = __float_as_uint(1.f);
  if (row.ceiling != row.ceiling) return;
  const int i0 = blockIdx.x * LM_T1;
  if (i0 >= row.r_count) return;
  const int t0 = row.r0 + i0;                            // relative position of the tile's first value
  // the first staged sample, moved down to a 16-byte boundary of the row's memory
  int kb = t0 - LM_J;
  kb -= ((int)(((uintptr_t)row.in >> 2) & 3u) + kb) & 3;
  const int off = t0 - LM_J - kb;                        // 0 .. 3
  const int nq = (LM_T1 + 2 * LM_J + off + 3) >> 2;      // at most (1024 + 24 + 3 + 3) / 4 = 263 quads <= LM_XS / 4
  for (int q = tid; q < nq; q += 256) {
    const int k = kb + 4 * q;
    float4 v;
    if (k >= 0 && k + 4 <= row.count) {
      v = *reinterpret_cast<const float4*>(row.in + k);
    } else {
      v.x = (k >= 0 && k < row.count) ? row.in[k] : 0.f;
      v.y = (k + 1 >= 0 && k + 1 < row.count) ? row.in[k + 1] : 0.f;
      v.z = (k + 2 >= 0 && k + 2 < row.count) ? row.in[k + 2] : 0.f;
      v.w = (k + 3 >= 0 && k + 3 < row.count) ? row.in[k + 3] : 0.f;
    }
    *reinterpret_cast<float4*>(xs + 4 * q) = v;
  }
  __syncthreads();
  const float g = (!METER && gains) ? gains[b] : 1.f;
  const float c = row.ceiling;
  float pk = 0.f;
#pragma unroll 1
  for (int j = 0; j < LM_T1 / 256; ++j) {
    const int i = tid + 256 * j;
    const int n = t0 + i;
    const bool live = i0 + i < row.r_count;
    float rv = 1.f;
    if (live && n >= 0 && n < row.count) {
      const float* x = xs + off + i;                     // x[d + J]: the sample at n + d
      float y0 = 0.f, y1 = 0.f, y2 = 0.f, y3 = 0.f;
      y0 = fmaf(taps.h[LM_HALF + 4 * LM_J], x[0], y0);   // phase 0 alone reaches k = n - 12
#pragma unroll
      for (int d = -LM_J + 1; d <= LM_J; ++d) {          // y[4 n + ph] = sum_k h[4 (n - k) + ph] x[k], ascending k = n + d
        const float xv = x[d + LM_J];
        y0 = fmaf(taps.h[LM_HALF - 4 * d], xv, y0);
        y1 = fmaf(taps.h[LM_HALF - 4 * d + 1], xv, y1);
        y2 = fmaf(taps.h[LM_HALF - 4 * d + 2], xv, y2);
        y3 = fmaf(taps.h[LM_HALF - 4 * d + 3], xv, y3);
      }
      const float p = fmaxf(fmaxf(fmaxf(fabsf(x[LM_J]), fabsf(y0)), fmaxf(fabsf(y1), fabsf(y2))), fabsf(y3));
      if (METER) {
        pk = fmaxf(pk, p);
      } else {
        const float e = g * p;
        rv = e > c ? c / e : 1.f;
      }
    }
    if (!METER && live) row.r[i0 + i] = rv;
  }
  if (METER) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) pk = fmaxf(pk, __shfl_xor(pk, d));
    __syncthreads();                                     // (the tile is read: its first words carry the waves' maxima)
    if ((tid & 63) == 0) xs[tid >> 6] = pk;
    __syncthreads();
    // one atomic a block: the blocks of a row all meet at one address (p >= 0: its bits order as the floats do)
    if (tid == 0) atomicMax(tp_bits + b, __float_as_uint(fmaxf(fmaxf(xs[0], xs[1]), fmaxf(xs[2], xs[3]))));
  }
}

__global__ void __launch_bounds__(256) lm_apply_kernel(const Row* __restrict__ rows, const float* __restrict__ gains,
                                                       unsigned* min_gain_bits, int A, int H, float inv) {
  extern __shared__ __align__(16) float lm_lds[];
  const int b = blockIdx.y, tid = threadIdx.x;
  const Row row = rows[b];
  if (row.ceiling != row.ceiling) return;
  const int o0 = blockIdx.x * LM_T2;
  if (o0 >= row.out_count) return;
  const int T = min(LM_T2, row.out_count - o0);
  const int W = A + H + 1;
  const int nr = T + 2 * A + H;                          // word i: r[o0 + i]; o0 + nr <= out_count + 2 A + H = r_count
  const int nm = T + A;                                  // m word u: the sample of output o0 - A + u = min r words [u, u + W)
  float* rl = lm_lds;
  float* ml = lm_lds + ((nr + 3) & ~3);
  const float* __restrict__ rg = row.r + o0;
  float v[LM_RK];
#pragma unroll
  for (int q = 0; q < LM_RK; ++q) {
    const int i = tid + 256 * q;
    v[q] = INFINITY;
    if (i < nr) rl[i] = v[q] = rg[i];
  }
  __syncthreads();
  int span = 1;                                          // word i = min r[i .. i + span), cut at nr
  while (2 * span <= W) {
#pragma unroll
    for (int q = 0; q < LM_RK; ++q) {
      const int i = tid + 256 * q;
      if (i + span < nr) v[q] = fminf(v[q], rl[i + span]);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < LM_RK; ++q) {
      const int i = tid + 256 * q;
      if (i < nr) rl[i] = v[q];
    }
    __syncthreads();
    span *= 2;
  }
  for (int u = tid; u < nm; u += 256) ml[u] = fminf(rl[u], rl[u + W - span]);      // (u + W - 1 <= nr - 1)
  __syncthreads();
  const float g = gains ? gains[b] : 1.f;
  const float c = row.ceiling;
  const float* __restrict__ x = row.in + row.out_off + o0;
  float* o = row.out + o0;
  float smin = INFINITY;
  for (int t = tid; t < T; t += 256) {
    const float* mp = ml + t;                            // m of the samples n - A .. n
    float acc = 0.f;
    for (int k = 0; k <= A; ++k) acc += mp[k];
    const float s = acc * inv;
    const float y = (g * x[t]) * s;
    o[t] = fminf(fmaxf(y, -c), c);
    smin = fminf(smin, s);
  }
  if (!min_gain_bits) return;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) smin = fminf(smin, __shfl_xor(smin, d));
  __syncthreads();                                       // (m is read: its first words carry the waves' minima)
  if ((tid & 63) == 0) ml[tid >> 6] = smin;
  __syncthreads();
  if (tid != 0) return;
  smin = fminf(fminf(ml[0], ml[1]), fminf(ml[2], ml[3]));
  // one atomic a block at most: min_gain starts at 1, so a tile that was not limited has nothing to say (s >= 0: its bits
  // order as the floats do)
  if (smin < 1.f) atomicMin(min_gain_bits + b, __float_as_uint(smin));
}

// ------------------------------------------------------------------------------------------------------------ host
using vsp::Call;
using vsp::Ws;

// The workspace: [Row [B]], then one r buffer per row that has outputs, in row order.
Row* carve_rows(Ws& ws, int B) { return static_cast<Row*>(ws.bytes((size_t)B * sizeof(Row))); }
float* carve_r(Ws& ws, int64_t out_count, int A, int H) { return ws.f((size_t)(out_count + 2 * (int64_t)A + H)); }

bool window_ok(int A, int H) { return A >= 0 && A <= LM_MAX_A && H >= 0 && H <= LM_MAX_H; }

Taps make_taps() {
  vsp::rs::Plan p;
  p.L = 4; p.M = 1; p.H = LM_HALF;
  std::vector<double> h;
  vsp::rs::make_filter(p, LM_ZEROS, LM_BETA, vsp::rs::default_rolloff(LM_ZEROS), h);
  Taps t;
  for (int i = 0; i < LM_TAPS; ++i) t.h[i] = (float)h[(size_t)i];
  return t;
}

const Taps& the_taps() {
  static const Taps t = make_taps();
  return t;
}

}  // namespace

int vsp_true_peak_filter(float* taps97_host) {
  if (!taps97_host) return VSP_ERR_ARG;
  std::memcpy(taps97_host, the_taps().h, sizeof(float) * LM_TAPS);
  return VSP_OK;
}

int vsp_limiter_history(int A, int H, int64_t* behind, int64_t* ahead) {
  if (!window_ok(A, H) || !behind || !ahead) return VSP_ERR_ARG;
  *behind = (int64_t)A + H + LM_J;
  *ahead = (int64_t)A + LM_J;
  return VSP_OK;
}

int64_t vsp_limiter_workspace_bytes(int B, int64_t L_max, int A, int H) {
  if (B < 1 || B > LM_MAX_B || L_max < 1 || L_max > LM_MAX_SAMPLES || !window_ok(A, H)) return VSP_ERR_ARG;
  Ws ws = vsp::dry_ws();                                 // every row at L_max outputs
  carve_rows(ws, B);
  for (int b = 0; b < B; ++b) carve_r(ws, L_max, A, H);
  return (int64_t)ws.cur;
}

int vsp_true_peak(vsp_ctx* ctx, void* stream, int B, int64_t L_max, const float* audio, int64_t audio_stride,
                  const int64_t* n_samples_host, float* tp, void* workspace, int64_t workspace_bytes) {
  if (!ctx) return VSP_ERR_ARG;
  const char* who = "vsp_true_peak";
  if (B < 1 || B > LM_MAX_B || L_max < 1 || L_max > LM_MAX_SAMPLES || audio_stride < L_max || !n_samples_host)
    return ctx->fail(VSP_ERR_ARG, "%s: 1 <= B <= %d rows, 1 <= L_max <= 2^30 <= audio_stride, and the rows' samples", who, LM_MAX_B);
  std::vector<Row> up((size_t)B);
  int64_t n_max = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t n = n_samples_host[b];
    if (n < 1 || n > L_max)
      return ctx->fail(VSP_ERR_ARG, "%s: row %d has %lld samples: 1 <= n_samples <= %lld", who, b, (long long)n, (long long)L_max);
    Row& r = up[(size_t)b];
    r.in = audio + (size_t)b * (size_t)audio_stride;
    r.out = nullptr; r.r = nullptr;
    r.count = (int32_t)n; r.r0 = 0; r.r_count = (int32_t)n; r.out_off = 0; r.out_count = 0;
    r.ceiling = 1.f;
    n_max = std::max(n_max, n);
  }
  if (!audio || !tp) return ctx->fail(VSP_ERR_ARG, "%s: null pointer", who);
  hipStream_t s = (hipStream_t)stream;
  const Call call{ctx, who, s};
  Ws ws = call.open(workspace, workspace_bytes);
  Row* rows = carve_rows(ws, B);
  if (const int rc = call.need_ws(workspace, workspace_bytes, ws.cur)) return rc;
  if (const int rc = call.upload(rows, up.data(), up.size() * sizeof(Row))) return rc;
  const hipError_t e = hipMemsetAsync(tp, 0, (size_t)B * sizeof(float), s);
  if (e != hipSuccess) return ctx->fail(VSP_ERR_HIP, "%s (tp): %s", who, hipGetErrorString(e));
  hipLaunchKernelGGL(lm_peak_kernel<true>, dim3((unsigned)((n_max + LM_T1 - 1) / LM_T1), B), dim3(256), 0, s, rows,
                     (const float*)nullptr, reinterpret_cast<unsigned*>(tp), (unsigned*)nullptr, the_taps());
  return call.launched("lm_peak_kernel");
}

int vsp_limiter_rows(vsp_ctx* ctx, void* stream, int B, int A, int H, const vsp_limiter_row* rows_host, const float* gains,
                     float* min_gain, void* workspace, int64_t workspace_bytes) {
  if (!ctx) return VSP_ERR_ARG;
  const char* who = "vsp_limiter_rows";
  if (B < 1 || B > LM_MAX_B || !rows_host) return ctx->fail(VSP_ERR_ARG, "%s: 1 <= B <= %d rows", who, LM_MAX_B);
  if (!window_ok(A, H))
    return ctx->fail(VSP_ERR_ARG, "%s: attack %d, hold %d: 0 <= attack <= %d, 0 <= hold <= %d samples", who, A, H, LM_MAX_A, LM_MAX_H);
  const int64_t behind = (int64_t)A + H + LM_J, ahead = (int64_t)A + LM_J;
  hipStream_t s = (hipStream_t)stream;
  const Call call{ctx, who, s};
  Ws ws = call.open(workspace, workspace_bytes);
  Row* rows = carve_rows(ws, B);
  std::vector<Row> up((size_t)B);
  int64_t r_max = 0, out_max = 0;
  for (int b = 0; b < B; ++b) {
    const vsp_limiter_row& h = rows_host[b];
    Row& r = up[(size_t)b];
    std::memset(&r, 0, sizeof r);
    r.ceiling = h.ceiling;
    if (h.ceiling != h.ceiling) continue;                // a NaN ceiling: the row is left alone, whatever else it holds
    if (!(h.ceiling > 0.f)) return ctx->fail(VSP_ERR_ARG, "%s: row %d: ceiling must be above 0", who, b);
    if (h.first < 0 || h.count < 0 || h.count > LM_MAX_SAMPLES || h.out_count < 0 || h.out_first < 0 || h.total < -1)
      return ctx->fail(VSP_ERR_ARG, "%s: row %d: negative position or count, or more than 2^30 samples", who, b);
    const int64_t end = h.first + h.count, out_end = h.out_first + h.out_count;
    if (h.total >= 0 && end > h.total)
      return ctx->fail(VSP_ERR_ARG, "%s: row %d: samples [%lld, %lld) lie behind the stream's end %lld", who, b, (long long)h.first,
                       (long long)end, (long long)h.total);
    if (h.out_first < h.first || out_end > end)
      return ctx->fail(VSP_ERR_ARG, "%s: row %d: outputs [%lld, %lld) are not among the samples [%lld, %lld)", who, b,
                       (long long)h.out_first, (long long)out_end, (long long)h.first, (long long)end);
    if (h.first > std::max<int64_t>(0, h.out_first - behind))
      return ctx->fail(VSP_ERR_ARG, "%s: row %d: output %lld needs the %lld samples before it, the row starts at %lld", who, b,
                       (long long)h.out_first, (long long)behind, (long long)h.first);
    if (end < out_end + ahead && (h.total < 0 || h.total > end))
      return ctx->fail(VSP_ERR_ARG, "%s: row %d: outputs up to %lld need %lld samples of look-ahead, the row ends at %lld before the stream does",
                       who, b, (long long)out_end, (long long)ahead, (long long)end);
    if ((h.count > 0 && !h.in) || (h.out_count > 0 && !h.out)) return ctx->fail(VSP_ERR_ARG, "%s: row %d: null pointer", who, b);
    if (h.out_count == 0) {                              // nothing to put out: nothing is read either
      r.ceiling = NAN;
      continue;
    }
    r.in = h.in;
    r.out = h.out;
    r.count = (int32_t)h.count;
    r.out_off = (int32_t)(h.out_first - h.first);
    r.out_count = (int32_t)h.out_count;
    r.r0 = r.out_off - A - H;
    r.r_count = (int32_t)(h.out_count + 2 * (int64_t)A + H);
    r.r = carve_r(ws, h.out_count, A, H);
    r_max = std::max<int64_t>(r_max, r.r_count);
    out_max = std::max<int64_t>(out_max, h.out_count);
  }
  if (const int rc = call.need_ws(workspace, workspace_bytes, ws.cur)) return rc;
  if (const int rc = call.upload(rows, up.data(), up.size() * sizeof(Row))) return rc;
  unsigned* mg = reinterpret_cast<unsigned*>(min_gain);
  // (one tile at least: the launch also sets min_gain to 1)
  hipLaunchKernelGGL(lm_peak_kernel<false>, dim3((unsigned)std::max<int64_t>(1, (r_max + LM_T1 - 1) / LM_T1), B), dim3(256), 0, s, rows,
                     gains, (unsigned*)nullptr, mg, the_taps());
  if (const int rc = call.launched("lm_peak_kernel")) return rc;
  if (out_max == 0) return VSP_OK;
  const size_t lds = (size_t)(((LM_T2 + 2 * A + H + 3) & ~3) + LM_T2 + A) * sizeof(float);        // (at most 60 KiB)
  static std::atomic<uint64_t> done{0};
  if (lds > 48 * 1024) {
    const hipError_t e = vsp::set_max_dynamic_lds(reinterpret_cast<const void*>(lm_apply_kernel), 64 * 1024, done);
    if (e != hipSuccess) return ctx->fail(VSP_ERR_HIP, "limiter (LDS): %s", hipGetErrorString(e));
  }
  const float inv = 1.f / (float)(A + 1);
  hipLaunchKernelGGL(lm_apply_kernel, dim3((unsigned)((out_max + LM_T2 - 1) / LM_T2), B), dim3(256), lds, s, rows, gains, mg, A, H, inv);
  return call.launched("lm_apply_kernel");
}
