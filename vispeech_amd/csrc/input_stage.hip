// Input stage of voice conversion (include/vispeech_hip.h, "input stage"): raw samples at the caller's rate, float32 / PCM16 /
// G.711 -> rational polyphase FIR resampling by L / M -> float32 at the model's rate.  The mirror of resample.hip: the same
// filter formula with the rates swapped, the same table [P][L] (tab[i][m mod L], taps in ascending input sample, all phases
// aligned to input sample floor(m M / L) - J), the same FMA chain per output sample.
//
// A block is (row, tile of 256 outputs); one thread per output sample.  The block decodes the input span of its tile ONCE
// into LDS as float32 -- about 256 M / L + P samples, 16 bytes of raw samples per load wherever the window holds all of
// them (every row can: the tile's first staged sample is moved down to a 16-byte boundary of the row's own memory), G.711
// through a 256-entry table in LDS -- and every lane then runs acc = fmaf(tab[i][m mod L], x[ks + i], acc), i ascending:
// neighbouring lanes read neighbouring words of a table row (coalesced, the table stays in L2) and LDS words at most
// ceil(M / L) apart.  Taps that do not fit the staging area beside the span take several passes; a span that does not fit
// at all (M / L above 7) reads and decodes from global memory, the same chain.  Both are the routines of resample_common.h
// (rs_tile_output with E = 4, 8 or 16 raw samples per 16-byte load, rs_one_output), sized by its stage_plan; this file
// passes its decoders (in_decode_vec, in_decode_one) and owns the G.711 table in LDS.  The set of rates is configured by
// resample_common.h's configure_rate into vsp_ctx::in_rates.
//
// A sample's value is a function of (decoded x, m) alone -- not of the tile, the window or the batch -- so a recording fed
// piece by piece gives the bytes of the one-shot call.  Samples outside a row's window are never read (selected to zero
// while the tile is staged), and the host has checked that the window ends at or before the recording's end.
#include <algorithm>
#include <cstring>
#include <vector>

#include "model.h"
#include "resample_common.h"

namespace {

using namespace vsp::rs;

constexpr int IN_TILE = RS_TILE;        // output samples (= threads) per block; also the entries of a G.711 table
constexpr int IN_X_LDS_FLOATS = 2048;   // input staging area per block (8 KiB: eight blocks per CU keep their LDS)
constexpr int IN_VEC = 16;              // raw samples of the widest 16-byte load (G.711); passes are multiples of it
constexpr int IN_MAX_L = 441, IN_MAX_M = 640;

static_assert(sizeof(vsp::InputRows) + sizeof(vsp::InputFilter) + 16 <= 4096, "kernel arguments must fit 4 KiB");

template <int ENC> struct InEnc;
template <> struct InEnc<VSP_IN_F32> { static constexpr int ES = 4; };
template <> struct InEnc<VSP_IN_S16> { static constexpr int ES = 2; };
template <> struct InEnc<VSP_IN_ULAW> { static constexpr int ES = 1; };
template <> struct InEnc<VSP_IN_ALAW> { static constexpr int ES = 1; };

// element i of a row's window, decoded
template <int ENC>
__device__ __forceinline__ float in_decode_one(const void* __restrict__ in, int64_t i, const float* g711) {
  if (ENC == VSP_IN_F32) return static_cast<const float*>(in)[i];
  if (ENC == VSP_IN_S16) return (float)static_cast<const int16_t*>(in)[i] * (1.0f / 32768.0f);
  return g711[static_cast<const uint8_t*>(in)[i]];
}

// the 16 / ES elements of one aligned 16-byte load, decoded to v[]
template <int ENC>
__device__ __forceinline__ void in_decode_vec(const void* __restrict__ p, float* v, const float* g711) {
  const uint4 w = *static_cast<const uint4*>(p);
  const uint32_t q[4] = {w.x, w.y, w.z, w.w};
  if (ENC == VSP_IN_F32) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = __uint_as_float(q[i]);
  } else if (ENC == VSP_IN_S16) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] = (float)(int16_t)(q[i] & 0xffffu) * (1.0f / 32768.0f);
      v[2 * i + 1] = (float)(int16_t)(q[i] >> 16) * (1.0f / 32768.0f);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int b = 0; b < 4; ++b) v[4 * i + b] = g711[(q[i] >> (8 * b)) & 0xffu];
    }
  }
}

// grid (tiles of the longest out_fill, rows), IN_TILE threads.  mode 0: the tile's span staged in LDS, `pass` taps at a time;
// mode 2: samples decoded from global memory.  Dynamic LDS: [256 floats G.711 table, encodings 2 and 3] [staging area].
template <int ENC>
__global__ __launch_bounds__(IN_TILE) void input_kernel(const vsp::InputRows rows, const vsp::InputFilter f, int pass, int mode) {
  extern __shared__ __align__(16) float in_smem[];
  constexpr int ES = InEnc<ENC>::ES, E = 16 / ES;
  constexpr bool G711 = ENC == VSP_IN_ULAW || ENC == VSP_IN_ALAW;
  float* g711 = in_smem;
  float* xs = in_smem + (G711 ? IN_TILE : 0);
  const int tid = threadIdx.x;
  const vsp::InputRow& r = rows.r[blockIdx.y];
  const int64_t j0 = (int64_t)blockIdx.x * IN_TILE, j = j0 + tid;
  const int64_t cnt = r.m1 - r.m0;
  if (j0 >= r.out_fill) return;                                     // (uniform over the block, like the next one)
  if (j0 >= cnt) {                                                  // behind the row's outputs: silence
    if (j < r.out_fill) r.out[j] = 0.f;
    return;
  }
  const int64_t m_first = r.m0 + j0, m_last = min(m_first + IN_TILE, r.m1) - 1;
  const int64_t lo = r.in_first, hi = r.in_first + r.in_len;        // readable samples [lo, hi); sample k is element k - lo
  if (G711) {
    g711[tid] = (float)(ENC == VSP_IN_ULAW ? vsp::g711_ulaw_linear(tid) : vsp::g711_alaw_linear(tid)) * (1.0f / 32768.0f);
    __syncthreads();
  }
  auto sample = [&](int64_t k) { return (k >= lo && k < hi) ? in_decode_one<ENC>(r.in, k - lo, g711) : 0.f; };
  auto load = [&](int64_t k, float* v) { in_decode_vec<ENC>(static_cast<const char*>(r.in) + (k - lo) * ES, v, g711); };
  float acc;
  if (mode == 2) acc = rs_one_output(f.tab, f.L, f.M, f.J, f.P, min(m_first + tid, m_last), sample);
  else acc = rs_tile_output<E>(xs, f.tab, f.L, f.M, f.J, f.P, pass, m_first, m_last, (int64_t)((uintptr_t)r.in / ES) - lo, lo, hi,
                               load, sample);
  const bool active = m_first + tid <= m_last;
  if (active) r.out[j] = acc;
  else if (j < r.out_fill) r.out[j] = 0.f;
}

}  // namespace

int vsp_input_plan(int in_rate, int model_rate, int zeros, int* L, int* M, int* half_len) {
  return plan_api(in_rate, model_rate, zeros ? zeros : 32, IN_MAX_L, IN_MAX_M, L, M, half_len);
}

int vsp_input_filter(int in_rate, int model_rate, int zeros, double beta, double rolloff, float* taps_host) {
  return filter_api(in_rate, model_rate, zeros ? zeros : 32, beta, rolloff, IN_MAX_L, IN_MAX_M, taps_host);
}

int vsp_input_decode_table(int enc, float* table256) {
  if (!table256 || (enc != VSP_IN_ULAW && enc != VSP_IN_ALAW)) return VSP_ERR_ARG;
  for (int c = 0; c < 256; ++c)
    table256[c] = (float)(enc == VSP_IN_ULAW ? vsp::g711_ulaw_linear(c) : vsp::g711_alaw_linear(c)) * (1.0f / 32768.0f);
  return VSP_OK;
}

namespace vsp {
hipError_t launch_input_rows(const InputRows& rows, int B, const InputFilter& f, int enc, hipStream_t s) {
  if (B <= 0 || B > STREAM_ROWS_MAX || enc < VSP_IN_F32 || enc > VSP_IN_ALAW || !f.tab || f.L < 1 || f.M < 1 || f.J < 0 || f.P < 1)
    return hipErrorInvalidValue;
  int64_t fill = 0;
  for (int b = 0; b < B; ++b) {
    const InputRow& r = rows.r[b];
    if (r.in_first < 0 || r.in_len < 0 || r.m0 < 0 || r.m1 < r.m0 || r.out_fill < r.m1 - r.m0 || (r.in_len > 0 && !r.in) ||
        (r.out_fill > 0 && !r.out) || (uintptr_t)r.in % enc_bytes(enc) || (uintptr_t)r.out % 4)
      return hipErrorInvalidValue;
    fill = std::max(fill, r.out_fill);
  }
  if (fill == 0) return hipSuccess;
  const StagePlan sp = stage_plan(IN_X_LDS_FLOATS, IN_VEC - 1, IN_VEC, IN_VEC, f.L, f.M, f.P);
  const int pass = sp.pass, mode = sp.mode;
  const size_t lds = (size_t)(sp.xs_words + (enc >= VSP_IN_ULAW ? IN_TILE : 0)) * sizeof(float);
  const dim3 grid((unsigned)((fill + IN_TILE - 1) / IN_TILE), (unsigned)B);
  switch (enc) {
    case VSP_IN_F32: hipLaunchKernelGGL(input_kernel<VSP_IN_F32>, grid, dim3(IN_TILE), lds, s, rows, f, pass, mode); break;
    case VSP_IN_S16: hipLaunchKernelGGL(input_kernel<VSP_IN_S16>, grid, dim3(IN_TILE), lds, s, rows, f, pass, mode); break;
    case VSP_IN_ULAW: hipLaunchKernelGGL(input_kernel<VSP_IN_ULAW>, grid, dim3(IN_TILE), lds, s, rows, f, pass, mode); break;
    default: hipLaunchKernelGGL(input_kernel<VSP_IN_ALAW>, grid, dim3(IN_TILE), lds, s, rows, f, pass, mode); break;
  }
  return hipGetLastError();
}
}  // namespace vsp

int vsp_input_configure(vsp_ctx* ctx, int in_rate, int model_rate, int zeros, double beta, double rolloff) {
  if (!ctx) return VSP_ERR_ARG;
  if (in_rate <= 0) return ctx->fail(VSP_ERR_ARG, "input stage: in_rate must be positive");
  if (model_rate == 0) {                                  // drop the rate
    drop_rate(ctx, find_rate(ctx->in_rates, VSP_INPUT_RATES_MAX, in_rate));
    return VSP_OK;
  }
  return configure_rate(ctx, "input stage", "input", ctx->in_rates, VSP_INPUT_RATES_MAX, in_rate, in_rate, model_rate, zeros, beta,
                        rolloff, IN_MAX_L, IN_MAX_M);
}

int vsp_input_rows(vsp_ctx* ctx, void* stream, int in_rate, int enc, int B, const vsp_input_row* rows) {
  if (!ctx) return VSP_ERR_ARG;
  const vsp_ctx::RateTable* t = find_rate(ctx->in_rates, VSP_INPUT_RATES_MAX, in_rate);
  if (!t) return ctx->fail(VSP_ERR_STATE, "input stage: rate %d Hz is not configured (vsp_input_configure)", in_rate);
  if (!rows || B < 1 || B > vsp::STREAM_ROWS_MAX || enc < VSP_IN_F32 || enc > VSP_IN_ALAW)
    return ctx->fail(VSP_ERR_ARG, "vsp_input_rows: 1 <= B <= %d rows, enc one of VSP_IN_*", vsp::STREAM_ROWS_MAX);
  const int64_t L = t->L, M = t->M, H = t->H, big = (int64_t)1 << 40;
  vsp::InputRows dev = {};
  for (int b = 0; b < B; ++b) {
    const vsp_input_row& r = rows[b];
    if (r.in_len < 0 || r.n_total < -1 || (r.in_len > 0 && !r.in) || (r.out_fill > 0 && !r.out) ||
        (uintptr_t)r.in % enc_bytes(enc) || (uintptr_t)r.out % 4)
      return ctx->fail(VSP_ERR_ARG, "vsp_input_rows: row %d has a null or misaligned pointer, or a negative length", b);
    const bool closed = r.n_total >= 0;
    const int64_t end = r.in_first + r.in_len;
    if (r.in_first < 0 || r.in_first > big || r.in_len > big || r.n_total > big || r.m0 < 0 || r.m1 < r.m0 || r.out_fill < r.m1 - r.m0 ||
        r.m1 > big * 512 || (closed && end > r.n_total))
      return ctx->fail(VSP_ERR_SHAPE, "vsp_input_rows: row %d: need 0 <= in_first, in_first + in_len <= n_total, 0 <= m0 <= m1, "
                       "m1 - m0 <= out_fill", b);
    const int64_t m_max = closed ? (r.n_total * L + M - 1) / M : vsp::stream_output_complete(end, false, L, M, H);
    if (r.m1 > m_max)
      return ctx->fail(VSP_ERR_SHAPE, "vsp_input_rows: row %d asks for outputs up to %lld, its %s completes %lld", b, (long long)r.m1,
                       closed ? "recording" : "window", (long long)m_max);
    if (r.m1 > r.m0) {
      // every input sample of the recording that a requested output depends on must be in the window
      const int64_t k_lo = std::max<int64_t>(0, ceil_div(r.m0 * M - H, L));
      int64_t k_hi = floor_div((r.m1 - 1) * M + H, L);
      if (closed) k_hi = std::min(k_hi, r.n_total - 1);
      if (k_lo <= k_hi && (k_lo < r.in_first || k_hi >= end))
        return ctx->fail(VSP_ERR_SHAPE, "vsp_input_rows: row %d: outputs [%lld, %lld) need input samples [%lld, %lld], the window "
                         "holds [%lld, %lld)", b, (long long)r.m0, (long long)r.m1, (long long)k_lo, (long long)k_hi,
                         (long long)r.in_first, (long long)end);
    }
    dev.r[b] = vsp::InputRow{r.in, r.in_first, r.in_len, r.out, r.m0, r.m1, r.out_fill};
  }
  const vsp::InputFilter f{t->tab, t->L, t->M, t->J, t->P};
  const hipError_t e = vsp::launch_input_rows(dev, B, f, enc, (hipStream_t)stream);
  if (e != hipSuccess) return ctx->fail(VSP_ERR_HIP, "input_kernel: %s", hipGetErrorString(e));
  return VSP_OK;
}
