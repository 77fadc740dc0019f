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
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

#include "model.h"
#include "resample_common.h"

namespace {

using namespace vsp::rs;

constexpr int RS_TILE = 256;            // output samples (= threads) per block
constexpr int RS_X_LDS_FLOATS = 12288;  // input staging area per block (48 KiB)
constexpr int RS_TAB_LDS_FLOATS = 4096; // a one-phase table (L = 1) up to this size is held in LDS (16 KiB)
constexpr int RS_MIN_PASS = 32;         // fewer taps per staging pass than this: read x from global memory instead

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
  int seg;                // L = 1 staging: words per polyphase segment of the de-interleaved tile (0: linear tile)
  int mode;               // 0: x tile in LDS, table from global / L2;  1: L = 1, de-interleaved x tile + table in LDS;
                          // 2: x and table from global memory (spans too long for LDS)
  int pcm;                // 0: float32 out, 1: int16 out
  int pair_ok;            // int16 rows are 4-byte aligned: even lanes store packed pairs
  int vec_ok;             // x rows are 16-byte aligned: the tile is staged with 16-byte loads
};

// Stores sample j of a row (float32, or PCM16 with even lanes storing packed pairs where the row allows it).  Every lane
// of the wave calls it with a valid y (the shuffle takes all of them); `active` lanes store, `has_next`: lane + 1 is active.
__device__ __forceinline__ void rs_store(void* row, int64_t j, float y, bool active, bool has_next, int pcm, int pair_ok) {
  if (!pcm) {
    if (active) static_cast<float*>(row)[j] = y;
    return;
  }
  const int q = rs_pcm16(y);
  const int q_next = __shfl_down(q, 1);
  int16_t* o16 = static_cast<int16_t*>(row) + j;
  if (pair_ok) {
    if (!(threadIdx.x & 1) && active) {
      if (has_next) *reinterpret_cast<uint32_t*>(o16) = (uint32_t)(q & 0xffff) | ((uint32_t)q_next << 16);
      else *o16 = (int16_t)q;
    }
  } else if (active) {
    *o16 = (int16_t)q;
  }
}

__global__ __launch_bounds__(RS_TILE) void resample_kernel(const ResampleArgs a) {
  extern __shared__ float smem[];
  const int tid = threadIdx.x;
  const int b = blockIdx.y;
  const int64_t m_first = a.m0 + (int64_t)blockIdx.x * RS_TILE;
  const int64_t m_last = min(m_first + RS_TILE, a.m1) - 1;         // (the grid covers [m0, m1): m_first <= m_last)
  const int64_t m = m_first + tid;
  const bool active = m <= m_last;
  const int64_t mm = active ? m : m_last;                            // idle lanes shadow the last sample: offsets stay in the tile
  int64_t nv = a.n_valid ? a.n_valid[b] : a.n_max;
  nv = min(max(nv, (int64_t)0), a.n_max);
  const int64_t lo = max(a.x_first, (int64_t)0), hi = min(nv, a.x_first + a.x_len);   // readable samples [lo, hi)
  const int64_t out_len = (nv * a.L + a.M - 1) / a.M;
  const float* __restrict__ xb = a.x + (int64_t)b * a.x_stride - a.x_first;             // xb[k] = sample k of utterance b
  const int64_t ks = (mm * a.M) / a.L - a.J;                                             // first input sample of this output
  const int col = (int)(mm % a.L);
  const float* __restrict__ tcol = a.tab + col;
  float acc = 0.f;

  if (a.mode == 2) {
    acc = rs_one_output(tcol, a.L, a.P, ks, [&](int64_t k) { return (k >= lo && k < hi) ? xb[k] : 0.f; });
  } else {
    float* xs = smem;
    float* ts = smem + a.xs_words;
    if (a.mode == 1) {
      for (int i = tid; i < a.P; i += RS_TILE) ts[i] = a.tab[i];
    }
    int64_t kb = (m_first * a.M) / a.L - a.J;                        // first input sample of the tile
    if (a.vec_ok) kb -= (((int64_t)b * a.x_stride - a.x_first + kb) & 3);   // ... moved down to a 16-byte boundary of x
    const int off = (int)(ks - kb);
    const int span = (int)((m_last * a.M) / a.L - a.J - kb) + 1;    // tile words before the pass's taps are added
    for (int i0 = 0; i0 < a.P; i0 += a.pass) {
      const int n_i = min(a.pass, a.P - i0);
      const int need = span + n_i - 1;
      const int64_t k_base = kb + i0;
      if (i0) __syncthreads();
      if (a.vec_ok) {
        for (int o = tid * 4; o < need; o += RS_TILE * 4) {
          const int64_t k = k_base + o;
          float4 v;
          if (k >= lo && k + 3 < hi) {
            v = *reinterpret_cast<const float4*>(xb + k);
          } else {
            v.x = (k >= lo && k < hi) ? xb[k] : 0.f;
            v.y = (k + 1 >= lo && k + 1 < hi) ? xb[k + 1] : 0.f;
            v.z = (k + 2 >= lo && k + 2 < hi) ? xb[k + 2] : 0.f;
            v.w = (k + 3 >= lo && k + 3 < hi) ? xb[k + 3] : 0.f;
          }
          if (a.seg) {
            const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) xs[((o + q) % a.M) * a.seg + (o + q) / a.M] = e[q];
          } else {
            *reinterpret_cast<float4*>(xs + o) = v;
          }
        }
      } else {
        for (int o = tid; o < need; o += RS_TILE) {
          const int64_t k = k_base + o;
          const float v = (k >= lo && k < hi) ? xb[k] : 0.f;
          xs[a.seg ? (o % a.M) * a.seg + o / a.M : o] = v;
        }
      }
      __syncthreads();
      if (a.mode == 1) {
        // L = 1: lane t reads tile word off + i = (off0 + t M) + i.  In the de-interleaved tile (word o at
        // (o mod M) seg + o / M) the lanes of a wave read consecutive words of one segment: no bank conflict where the
        // linear tile would be read at stride M; the tap is the same for all lanes (a broadcast LDS read).
        // Taps are fetched four at a time (one 16-byte broadcast read): 1.25 LDS reads per FMA instead of 2.
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
      } else {
        const float* __restrict__ tp = tcol + (size_t)i0 * a.L;
        const float* xo = xs + off;
        int i = 0;
        for (; i + 4 <= n_i; i += 4) {                               // (four table loads in flight; the FMA order stays ascending)
          const float t0 = tp[(size_t)i * a.L], t1 = tp[(size_t)(i + 1) * a.L], t2 = tp[(size_t)(i + 2) * a.L],
                      t3 = tp[(size_t)(i + 3) * a.L];
          acc = fmaf(t0, xo[i], acc);
          acc = fmaf(t1, xo[i + 1], acc);
          acc = fmaf(t2, xo[i + 2], acc);
          acc = fmaf(t3, xo[i + 3], acc);
        }
        for (; i < n_i; ++i) acc = fmaf(tp[(size_t)i * a.L], xo[i], acc);
      }
    }
  }

  const float y = m < out_len ? acc : 0.f;                           // behind the utterance's own output: silence
  // (all lanes take part in the store's shuffle; idle lanes hold a valid shadow)
  rs_store(static_cast<char*>(a.out) + (int64_t)b * a.out_stride * (a.pcm ? 2 : 4), m - a.m0, y, active, m + 1 <= m_last, a.pcm,
           a.pair_ok);
}

// The ragged output stage (kernels.h, launch_stream_output).  grid (out_blocks + hist_blocks, B), RS_TILE threads; a block
// serves one row (blockIdx.y), whose descriptor is read through the constant kernel arguments.  Sample k of the row's
// utterance is its new segment for k in [x_first, x_first + n), hist_in for k in [k0, x_first) and 0 elsewhere: before k0 no
// output of [m0, m1) reads it, behind x_first + n it is the filter's tail.  The span's halo samples are never read.  Samples
// come from global memory (L1 / L2: a tile's window is a few KB) -- the chain of resample_kernel, so the same bits.
__global__ __launch_bounds__(RS_TILE) void stream_output_kernel(const vsp::StreamOutRows rows, const float* __restrict__ o_span,
                                                                long o_bs, const vsp::StreamOutFilter f, int K, int out_blocks,
                                                                void* __restrict__ out, long out_stride, int pcm, int pair_ok) {
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
  if (m < p.m1) y = rs_one_output(f.tab + (int)(m % f.L), f.L, f.P, (m * f.M) / f.L - f.J, sample);
  rs_store(static_cast<char*>(out) + (int64_t)b * out_stride * (pcm ? 2 : 4), j, y, j < out_stride, j + 1 < out_stride, pcm,
           pair_ok);
}

// ---------------------------------------------------------------------------------------------- host: plan and filter
constexpr int RS_MAX_L = 320, RS_MAX_M = 441;   // what resample_kernel's staging covers

int make_plan(int in_rate, int out_rate, int zeros, Plan& p) { return vsp::rs::make_plan(in_rate, out_rate, zeros, RS_MAX_L, RS_MAX_M, p); }

}  // namespace

int vsp_resample_plan(int in_rate, int out_rate, int zeros, int* L, int* M, int* half_len) {
  Plan p;
  if (!L || !M || !half_len) return VSP_ERR_ARG;
  if (int rc = make_plan(in_rate, out_rate, zeros, p)) return rc;
  *L = p.L; *M = p.M; *half_len = p.H;
  return VSP_OK;
}

int vsp_resample_filter(int in_rate, int out_rate, int zeros, double beta, double rolloff, float* taps_host) {
  Plan p;
  if (!taps_host || !(beta >= 0.0) || !(rolloff <= 1.0)) return VSP_ERR_ARG;
  if (int rc = make_plan(in_rate, out_rate, zeros, p)) return rc;
  if (!(rolloff > 0.0)) rolloff = default_rolloff(zeros);
  std::vector<double> h;
  make_filter(p, zeros, beta, rolloff, h);
  for (size_t i = 0; i < h.size(); ++i) taps_host[i] = (float)h[i];
  return VSP_OK;
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
  const int pair_ok = pcm && ((uintptr_t)out % 4 == 0) && (out_stride % 2 == 0);
  hipLaunchKernelGGL(stream_output_kernel, dim3(out_blocks + hist_blocks, B), dim3(RS_TILE), 0, s, rows, o_span, o_bs, f, K,
                     out_blocks, out, out_stride, pcm, pair_ok);
  return hipGetLastError();
}
}  // namespace vsp

int vsp_output_configure(vsp_ctx* ctx, int in_rate, int out_rate, int zeros, double beta, double rolloff) {
  if (!ctx) return VSP_ERR_ARG;
  if (out_rate == 0) {                                   // off
    if (ctx->out_tab) (void)hipFree(ctx->out_tab);
    ctx->out_tab = nullptr;
    ctx->out_L = ctx->out_M = ctx->out_H = ctx->out_J = ctx->out_P = 0;
    return VSP_OK;
  }
  if (zeros == 0) zeros = 32;
  if (!(beta >= 0.0)) return ctx->fail(VSP_ERR_ARG, "output stage: beta must be >= 0");
  if (!(rolloff <= 1.0)) return ctx->fail(VSP_ERR_ARG, "output stage: rolloff must be in (0, 1] (<= 0: 1 - 3.065 / zeros)");
  Plan p;
  if (int rc = make_plan(in_rate, out_rate, zeros, p))
    return ctx->fail(rc, "output stage %d -> %d Hz, %d zeros: rates must be positive, L <= 320, M <= 441, 1 <= zeros <= 64",
                     in_rate, out_rate, zeros);
  if (!(rolloff > 0.0)) rolloff = default_rolloff(zeros);
  std::vector<double> h;
  make_filter(p, zeros, beta, rolloff, h);
  const int L = p.L, M = p.M, H = p.H;
  int J, P;
  std::vector<float> tab;
  make_table(p, h, J, P, tab);
  void* d = nullptr;
  hipError_t e = hipSetDevice(ctx->device);
  if (e == hipSuccess) e = hipMalloc(&d, tab.size() * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(d, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (d) (void)hipFree(d);
    return ctx->fail(VSP_ERR_HIP, "output stage table: %s", hipGetErrorString(e));
  }
  if (ctx->out_tab) (void)hipFree(ctx->out_tab);
  ctx->out_tab = static_cast<float*>(d);
  ctx->out_L = L; ctx->out_M = M; ctx->out_H = H; ctx->out_J = J; ctx->out_P = P;
  return VSP_OK;
}

int vsp_output_chunk(vsp_ctx* ctx, void* stream, int B, const float* x, int64_t x_stride, int64_t x_first, int64_t x_len,
                     const int64_t* n_valid, int64_t n_max, int64_t m0, int64_t m1, void* out, int64_t out_stride,
                     int pcm) {
  if (!ctx) return VSP_ERR_ARG;
  if (!ctx->out_tab) return ctx->fail(VSP_ERR_STATE, "output stage not configured (vsp_output_configure)");
  if (B < 0 || B > 65535 || !x || !out || (pcm != 0 && pcm != 1)) return ctx->fail(VSP_ERR_ARG, "vsp_output_chunk: null or bad argument");
  const int64_t L = ctx->out_L, M = ctx->out_M, H = ctx->out_H;
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
  a.tab = ctx->out_tab;
  a.L = (int)L; a.M = (int)M; a.J = ctx->out_J; a.P = ctx->out_P;
  a.pcm = pcm;
  a.pair_ok = pcm && ((uintptr_t)out % 4 == 0) && (out_stride % 2 == 0);
  a.vec_ok = ((uintptr_t)x % 16 == 0) && (x_stride % 4 == 0);
  // tile words: the outputs of a tile start within (TILE - 1) M / L + 1 samples of each other, + 3 for the alignment
  const int64_t span = ((int64_t)(RS_TILE - 1) * M) / L + 2 + 3;
  const bool one_phase = L == 1 && a.P <= RS_TAB_LDS_FLOATS;
  const int64_t room = one_phase ? RS_X_LDS_FLOATS - span - 2 * M - 8 : RS_X_LDS_FLOATS - span - 8;
  a.seg = 0;
  if (room >= std::min<int64_t>(a.P, RS_MIN_PASS)) {
    a.pass = room >= a.P ? a.P : (int)(room & ~(int64_t)3);
    a.mode = one_phase ? 1 : 0;
    if (one_phase) a.seg = (int)((span + a.pass + 3) / M + 2);          // (every tile word, the 16-byte loads' overhang included)
    a.xs_words = one_phase ? (int)(M * a.seg) : (int)(span + a.pass + 8);
    a.xs_words = (a.xs_words + 3) & ~3;
  } else {
    a.pass = a.P;
    a.mode = 2;
    a.xs_words = 0;
  }
  const size_t lds = (size_t)(a.xs_words + (a.mode == 1 ? a.P : 0)) * sizeof(float);   // <= 48 KiB + 16 KiB
  const dim3 grid((unsigned)((m1 - m0 + RS_TILE - 1) / RS_TILE), (unsigned)B);
  hipLaunchKernelGGL(resample_kernel, grid, dim3(RS_TILE), lds, (hipStream_t)stream, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return ctx->fail(VSP_ERR_HIP, "resample_kernel: %s", hipGetErrorString(e));
  return VSP_OK;
}
