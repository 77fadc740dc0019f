// Output stage of the service path (include/vispeech_hip.h, "output stage"): waveform float32 at the model's rate ->
// rational polyphase FIR resampling by L / M -> float32 or PCM16 at the output rate.  What the reference does with
// `ffmpeg -i c.wav -ar 22050` after synthesis (inference_api.py:50-52), on the GPU and chunk by chunk.
//
//   y[m] = sum_k h[m M - k L] x[k],  |m M - k L| <= H,  k in [0, n_valid)        h: Kaiser-windowed sinc, 2 H + 1 taps
//
// With m M = k0 L + p (p = the sample's phase) the taps of one output are h[p + j L]; the table holds them per phase in
// ASCENDING k, all phases padded with zeros to the same count P and aligned to the same first input sample k0 - J
// (J = H / L):   tab[i][m mod L] = h[p(m) + (J - i) L],  i = 0 .. P - 1,  input sample k = k0 - J + i.
// The column index is m mod L, not p: m -> p is a bijection of [0, L) (gcd(L, M) = 1), and neighbouring lanes (consecutive
// m) then read neighbouring words of a table row -- a coalesced read of an L2-resident table (113 KB at most for the
// default filters) where a phase-major table would cost one cache line per lane.
//
// One thread per output sample, fp32 FMAs in ascending k: a sample's value is a function of (x, m) alone -- not of the tile,
// the window a streaming caller passes or the batch layout -- which is what makes the streamed output byte-identical to
// the one-shot one.  Samples outside [0, n_valid[b]) and outside the passed window are never read (selected to zero while
// the tile is staged), so whatever a padded batch holds behind an utterance's end cannot reach the output.
//
// What this file shares with input_stage.hip and output_rows.hip lives in resample_common.h: the staged tile of mode 0
// (rs_tile_output, with 16-byte loads of four floats where the rows are aligned, element by element where not), the
// global-memory chain of mode 2 (rs_one_output), the store (out_store), the staging plan (stage_plan) and the way a rate is
// configured (configure_rate into vsp_ctx::out_stage).  Its own: the [lo, hi) window of resample_kernel (x_first, x_len,
// n_valid), the one-phase tile of mode 1 and its sizing, and stream_output_kernel.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

#include "model.h"
#include "resample_common.h"

namespace {

using namespace vsp::rs;

constexpr int RS_X_LDS_FLOATS = 12288;  // input staging area per block (48 KiB)
constexpr int RS_TAB_LDS_FLOATS = 4096; // a one-phase table (L = 1) up to this size is held in LDS (16 KiB)

struct ResampleArgs {
  const float* x;
  int64_t x_stride, x_first, x_len;
  const int64_t* n_valid;
  int64_t n_max, m0, m1;
  void* out;
  int64_t out_stride;
  const float* tab;       // [P][L]
  int L, M, J, P;
  int pass;               // taps per staging pass (multiple of 4, or P)
  int xs_words;           // LDS words of the input tile (the one-phase table follows it)
  int seg;                // mode 1: words per polyphase segment of the de-interleaved tile
  int mode;               // 0: x tile in LDS, table from global / L2 (rs_tile_output);  1: L = 1, de-interleaved x tile +
                          // table in LDS;  2: x and table from global memory (spans too long for LDS; rs_one_output)
  int enc;                // VSP_OUT_F32 or VSP_OUT_S16
  int vec_ok;             // x rows are 16-byte aligned: the tile is staged with 16-byte loads
};

// Mode 1 of resample_kernel, L = 1: the tile is staged DE-INTERLEAVED (word o at (o mod M) seg + o / M) beside the table.
// Lane t reads tile word off + i = (off0 + t M) + i, so the lanes of a wave read consecutive words of one segment: no bank
// conflict where the linear tile would be read at stride M; the tap is the same for all lanes (a broadcast LDS read).
// Taps are fetched four at a time (one 16-byte broadcast read): 1.25 LDS reads per FMA instead of 2.  Geometry, passes and
// FMA order are rs_tile_output's.
template <class Sample>
__device__ __forceinline__ float one_phase_output(const ResampleArgs& a, float* smem, int64_t m_first, int64_t m_last, int64_t a0,
                                                  int64_t lo, int64_t hi, const float* __restrict__ xb, Sample sample) {
  const int tid = threadIdx.x;
  float* xs = smem;
  float* ts = smem + a.xs_words;
  for (int i = tid; i < a.P; i += RS_TILE) ts[i] = a.tab[i];
  const int64_t ks = min(m_first + tid, m_last) * a.M - a.J;        // first input sample of this output
  int64_t kb = m_first * a.M - a.J;                                 // first input sample of the tile
  if (a.vec_ok) kb -= (a0 + kb) & 3;                                // ... moved down to a 16-byte boundary of x
  const int off = (int)(ks - kb);
  const int span = (int)(m_last * a.M - a.J - kb) + 1;              // tile words before the pass's taps are added
  float acc = 0.f;
  for (int i0 = 0; i0 < a.P; i0 += a.pass) {
    const int n_i = min(a.pass, a.P - i0);
    const int need = span + n_i - 1;
    const int64_t k_base = kb + i0;
    if (i0) __syncthreads();
    if (a.vec_ok) {
      for (int o = tid * 4; o < need; o += RS_TILE * 4) {
        const int64_t k = k_base + o;
        float4 v;
        if (k >= lo && k + 3 < hi) v = *reinterpret_cast<const float4*>(xb + k);
        else v = make_float4(sample(k), sample(k + 1), sample(k + 2), sample(k + 3));
        const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) xs[((o + q) % a.M) * a.seg + (o + q) / a.M] = e[q];
      }
    } else {
      for (int o = tid; o < need; o += RS_TILE) xs[(o % a.M) * a.seg + o / a.M] = sample(k_base + o);
    }
    __syncthreads();
    int r = off % a.M;
    const float* xp = xs + r * a.seg + off / a.M;
    const int wrap = a.M * a.seg - 1;
    auto step = [&]() { xp += a.seg; if (++r == a.M) { r = 0; xp -= wrap; } };
    int i = 0;
    for (; i + 4 <= n_i; i += 4) {
      const float4 t = *reinterpret_cast<const float4*>(ts + i0 + i);
      acc = fmaf(t.x, *xp, acc); step();
      acc = fmaf(t.y, *xp, acc); step();
      acc = fmaf(t.z, *xp, acc); step();
      acc = fmaf(t.w, *xp, acc); step();
    }
    for (; i < n_i; ++i) { acc = fmaf(ts[i0 + i], *xp, acc); step(); }
  }
  return acc;
}

__global__ __launch_bounds__(RS_TILE) void resample_kernel(const ResampleArgs a) {
  extern __shared__ float smem[];
  const int b = blockIdx.y;
  const int64_t m_first = a.m0 + (int64_t)blockIdx.x * RS_TILE;
  const int64_t m_last = min(m_first + RS_TILE, a.m1) - 1;         // (the grid covers [m0, m1): m_first <= m_last)
  const int64_t m = m_first + threadIdx.x;
  int64_t nv = a.n_valid ? a.n_valid[b] : a.n_max;
  nv = min(max(nv, (int64_t)0), a.n_max);
  const int64_t lo = max(a.x_first, (int64_t)0), hi = min(nv, a.x_first + a.x_len);   // readable samples [lo, hi)
  const int64_t out_len = (nv * a.L + a.M - 1) / a.M;
  const int64_t a0 = (int64_t)b * a.x_stride - a.x_first;                               // (x itself is 16-byte aligned where it matters)
  const float* __restrict__ xb = a.x + a0;                                              // xb[k] = sample k of utterance b
  auto sample = [&](int64_t k) { return (k >= lo && k < hi) ? xb[k] : 0.f; };
  auto load = [&](int64_t k, float* v) {
    const float4 w = *reinterpret_cast<const float4*>(xb + k);
    v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
  };
  float acc;
  if (a.mode == 2) acc = rs_one_output(a.tab, a.L, a.M, a.J, a.P, min(m, m_last), sample);
  else if (a.mode == 1) acc = one_phase_output(a, smem, m_first, m_last, a0, lo, hi, xb, sample);
  else if (a.vec_ok) acc = rs_tile_output<4>(smem, a.tab, a.L, a.M, a.J, a.P, a.pass, m_first, m_last, a0, lo, hi, load, sample);
  else acc = rs_tile_output<1>(smem, a.tab, a.L, a.M, a.J, a.P, a.pass, m_first, m_last, a0, lo, hi, load, sample);

  // behind the utterance's own output: silence  (all lanes take part in the store's shuffle; idle lanes hold a valid shadow)
  out_store(static_cast<char*>(a.out) + (int64_t)b * a.out_stride * (a.enc == VSP_OUT_S16 ? 2 : 4), a.enc, m - a.m0,
            m < out_len ? acc : 0.f, a.m1 - a.m0);
}

// The ragged output stage (kernels.h, launch_stream_output).  grid (out_blocks + hist_blocks, B), RS_TILE threads; a block
// serves one row (blockIdx.y), whose descriptor is read through the constant kernel arguments.  Sample k of the row's
// utterance is its new segment for k in [x_first, x_first + n), hist_in for k in [k0, x_first) and 0 elsewhere: before k0 no
// output of [m0, m1) reads it, behind x_first + n it is the filter's tail.  The span's halo samples are never read.  Samples
// come from global memory (L1 / L2: a tile's window is a few KB) -- the chain of resample_kernel, so the same bits.
__global__ __launch_bounds__(RS_TILE) void stream_output_kernel(const vsp::StreamOutRows rows, const float* __restrict__ o_span,
                                                                long o_bs, const vsp::StreamOutFilter f, int K, int out_blocks,
                                                                void* __restrict__ out, long out_stride, int enc) {
  const int b = blockIdx.y;
  const vsp::StreamOutRow& r = rows.r[b];
  const int64_t x_first = r.x_first, x_end = x_first + r.n;
  const vsp::StreamOutPlan p = vsp::stream_output_plan(x_first, r.n, r.ended != 0, f.L, f.M, f.H);
  const float* __restrict__ xn = o_span + (size_t)b * o_bs + r.off - x_first;      // xn[k], k in [x_first, x_end)
  const float* __restrict__ xh = r.hist_in - p.k0;                                  // xh[k], k in [k0, x_first)
  auto sample = [&](int64_t k) { return k >= x_first ? (k < x_end ? xn[k] : 0.f) : (k >= p.k0 ? xh[k] : 0.f); };
  if ((int)blockIdx.x >= out_blocks) {
    const int64_t j = (int64_t)((int)blockIdx.x - out_blocks) * RS_TILE + threadIdx.x, k = p.k1 + j;
    if (j < K && k < x_end) r.hist_out[j] = sample(k);
    return;
  }
  const int64_t j = (int64_t)blockIdx.x * RS_TILE + threadIdx.x;
  const int64_t m = p.m0 + j;
  float y = 0.f;
  if (m < p.m1) y = rs_one_output(f.tab, f.L, f.M, f.J, f.P, m, sample);
  out_store(static_cast<char*>(out) + (int64_t)b * out_stride * (enc == VSP_OUT_S16 ? 2 : 4), enc, j, y, out_stride);
}

}  // namespace

int vsp_resample_plan(int in_rate, int out_rate, int zeros, int* L, int* M, int* half_len) {
  return plan_api(in_rate, out_rate, zeros, OUT_MAX_L, OUT_MAX_M, L, M, half_len);
}

int vsp_resample_filter(int in_rate, int out_rate, int zeros, double beta, double rolloff, float* taps_host) {
  return filter_api(in_rate, out_rate, zeros, beta, rolloff, OUT_MAX_L, OUT_MAX_M, taps_host);
}

int64_t vsp_resample_out_len(int64_t n, int L, int M) {
  if (n < 0 || L < 1 || M < 1) return VSP_ERR_ARG;
  return (n * L + M - 1) / M;
}

int vsp_output_history_samples(int L, int M, int H) {
  if (L < 1 || M < 1 || H < 0) return VSP_ERR_ARG;
  // Between windows the first incomplete output is m = ceil((L n_seen - H) / M) (or 0 while L n_seen <= H), so its first
  // input sample ceil((m M - H) / L) >= n_seen - 2 H / L: at most floor(2 H / L) samples are kept.
  return (int)(((int64_t)2 * H) / L);
}

int64_t vsp_stream_rows_out_samples(int L, int M, int H, int up, int chunk_frames) {
  if (L < 1 || M < 1 || H < 0 || up < 1 || chunk_frames < 1) return VSP_ERR_ARG;
  // m1 - m0 <= ceil((n L + H) / M) for the final tick (its m0 >= (L x_first - H) / M, its m1 = ceil(L (x_first + n) / M)),
  // ceil(n L / M) for any other
  const int64_t n = (int64_t)chunk_frames * up;
  return ((n * L + M - 1) / M + (H + M - 1) / M + 3) / 4 * 4;
}

int vsp_stream_rows_output_plan(int L, int M, int H, int up, int B, const vsp_stream_row* rows, int64_t* m0, int64_t* m1,
                                int64_t* k0, int64_t* k1) {
  if (L < 1 || M < 1 || H < 0 || up < 1 || !rows || B < 1 || B > vsp::STREAM_ROWS_MAX) return VSP_ERR_ARG;
  for (int b = 0; b < B; ++b)
    if (rows[b].f0 < 0 || rows[b].f1 <= rows[b].f0 || rows[b].f1 > rows[b].L) return VSP_ERR_ARG;
  for (int b = 0; b < B; ++b) {
    const vsp_stream_row& r = rows[b];
    const vsp::StreamOutPlan p = vsp::stream_output_plan((int64_t)r.f0 * up, (int64_t)(r.f1 - r.f0) * up, r.f1 == r.L, L, M, H);
    if (m0) m0[b] = p.m0;
    if (m1) m1[b] = p.m1;
    if (k0) k0[b] = p.k0;
    if (k1) k1[b] = p.k1;
  }
  return VSP_OK;
}

namespace vsp {
hipError_t launch_stream_output(const float* o_span, long o_bs, const StreamOutRows& rows, int B, const StreamOutFilter& f,
                                int K, void* out, long out_stride, int pcm, hipStream_t s) {
  if (B <= 0 || B > STREAM_ROWS_MAX || !o_span || !out || out_stride <= 0 || o_bs <= 0 || !f.tab || f.L < 1 || f.M < 1 ||
      f.H < 0 || f.P < 1 || K < 0)
    return hipErrorInvalidValue;
  for (int b = 0; b < B; ++b) {
    const StreamOutRow& r = rows.r[b];
    if (r.x_first < 0 || r.off < 0 || r.n <= 0 || (long)r.off + r.n > o_bs) return hipErrorInvalidValue;
    const StreamOutPlan p = stream_output_plan(r.x_first, r.n, r.ended != 0, f.L, f.M, f.H);
    const int64_t h_in = r.x_first - p.k0, h_out = r.x_first + r.n - p.k1;
    if (p.m1 - p.m0 > out_stride || h_in > K || h_out > K || (h_in > 0 && !r.hist_in) || (h_out > 0 && !r.hist_out) ||
        (r.hist_out && r.hist_in == r.hist_out))
      return hipErrorInvalidValue;
  }
  const int out_blocks = (int)((out_stride + RS_TILE - 1) / RS_TILE), hist_blocks = (K + RS_TILE - 1) / RS_TILE;
  hipLaunchKernelGGL(stream_output_kernel, dim3(out_blocks + hist_blocks, B), dim3(RS_TILE), 0, s, rows, o_span, o_bs, f, K,
                     out_blocks, out, out_stride, pcm ? VSP_OUT_S16 : VSP_OUT_F32);
  return hipGetLastError();
}
}  // namespace vsp

int vsp_output_configure(vsp_ctx* ctx, int in_rate, int out_rate, int zeros, double beta, double rolloff) {
  if (!ctx) return VSP_ERR_ARG;
  if (out_rate == 0) {                                   // off
    drop_rate(ctx, &ctx->out_stage);
    return VSP_OK;
  }
  return configure_rate(ctx, "output stage", "output", &ctx->out_stage, 1, 0, in_rate, out_rate, zeros, beta, rolloff, OUT_MAX_L,
                        OUT_MAX_M);
}

int vsp_output_chunk(vsp_ctx* ctx, void* stream, int B, const float* x, int64_t x_stride, int64_t x_first, int64_t x_len,
                     const int64_t* n_valid, int64_t n_max, int64_t m0, int64_t m1, void* out, int64_t out_stride,
                     int pcm) {
  if (!ctx) return VSP_ERR_ARG;
  const vsp_ctx::RateTable& t = ctx->out_stage;
  if (!t.tab) return ctx->fail(VSP_ERR_STATE, "output stage not configured (vsp_output_configure)");
  if (B < 0 || B > 65535 || !x || !out || (pcm != 0 && pcm != 1)) return ctx->fail(VSP_ERR_ARG, "vsp_output_chunk: null or bad argument");
  const int64_t L = t.L, M = t.M, H = t.H;
  if (n_max < 0 || n_max > ((int64_t)1 << 40) || x_first < 0 || x_len < 0 || x_first + x_len > n_max || x_len > x_stride)
    return ctx->fail(VSP_ERR_SHAPE, "vsp_output_chunk: window [%lld, +%lld) outside [0, n_max = %lld) or longer than its row",
                     (long long)x_first, (long long)x_len, (long long)n_max);
  if (m0 < 0 || m1 < m0 || m1 > (n_max * L + M - 1) / M || m1 - m0 > out_stride)
    return ctx->fail(VSP_ERR_SHAPE, "vsp_output_chunk: outputs [%lld, %lld) outside [0, ceil(n_max L / M)) or longer than their row",
                     (long long)m0, (long long)m1);
  if (B == 0 || m1 == m0) return VSP_OK;
  // every input sample of [0, n_max) that a requested output depends on must be in the window
  const int64_t k_lo = std::max<int64_t>(0, ceil_div(m0 * M - H, L));
  const int64_t k_hi = std::min<int64_t>(n_max - 1, floor_div((m1 - 1) * M + H, L));
  if (k_lo <= k_hi && (k_lo < x_first || k_hi >= x_first + x_len))
    return ctx->fail(VSP_ERR_SHAPE, "vsp_output_chunk: outputs [%lld, %lld) need input samples [%lld, %lld], the window holds [%lld, %lld)",
                     (long long)m0, (long long)m1, (long long)k_lo, (long long)k_hi, (long long)x_first,
                     (long long)(x_first + x_len));
  ResampleArgs a;
  a.x = x; a.x_stride = x_stride; a.x_first = x_first; a.x_len = x_len;
  a.n_valid = n_valid; a.n_max = n_max; a.m0 = m0; a.m1 = m1;
  a.out = out; a.out_stride = out_stride;
  a.tab = t.tab;
  a.L = t.L; a.M = t.M; a.J = t.J; a.P = t.P;
  a.enc = pcm ? VSP_OUT_S16 : VSP_OUT_F32;
  a.vec_ok = ((uintptr_t)x % 16 == 0) && (x_stride % 4 == 0);
  const StagePlan sp = stage_plan(RS_X_LDS_FLOATS, 3, 8, 4, t.L, t.M, t.P);
  a.pass = sp.pass; a.mode = sp.mode; a.xs_words = sp.xs_words; a.seg = 0;
  if (L == 1 && a.P <= RS_TAB_LDS_FLOATS) {
    // one phase: the de-interleaved tile of mode 1 (stage_plan's span, 2 M words of headroom), or global memory
    const int64_t span = ((int64_t)(RS_TILE - 1) * M) / L + 2 + 3;
    const int64_t room = RS_X_LDS_FLOATS - span - 2 * M - 8;
    a.pass = a.P; a.mode = 2; a.xs_words = 0;
    if (room >= std::min<int64_t>(a.P, RS_MIN_PASS)) {
      a.pass = room >= a.P ? a.P : (int)(room & ~(int64_t)3);
      a.mode = 1;
      a.seg = (int)((span + a.pass + 3) / M + 2);                        // (every tile word, the 16-byte loads' overhang included)
      a.xs_words = (int)(M * a.seg + 3) & ~3;
    }
  }
  const size_t lds = (size_t)(a.xs_words + (a.mode == 1 ? a.P : 0)) * sizeof(float);   // <= 48 KiB + 16 KiB
  const dim3 grid((unsigned)((m1 - m0 + RS_TILE - 1) / RS_TILE), (unsigned)B);
  hipLaunchKernelGGL(resample_kernel, grid, dim3(RS_TILE), lds, (hipStream_t)stream, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return ctx->fail(VSP_ERR_HIP, "resample_kernel: %s", hipGetErrorString(e));
  return VSP_OK;
}
