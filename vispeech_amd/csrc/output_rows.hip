// Output rows (include/vispeech_hip.h, "output rows"): the ragged output stage with every row's own rate and encoding.
// The counterpart of input_stage.hip on the way out: waveform float32 at the model's rate -> rational polyphase FIR
// resampling by the ROW's L / M -> float32, PCM16, G.711 mu-law or A-law.  The filter formula, the table [P][L]
// (tab[i][m mod L], taps in ascending input sample, all phases aligned to input sample floor(m M / L) - J) and the FMA
// chain per output sample are resample.hip's, so a float row is vsp_output_chunk's bit for bit.
//
// A block is (row, tile of 256 outputs); one thread per output sample.  The row's descriptor and its rate's filter entry
// come through the constant kernel arguments, so rows of different rates and encodings sit in one grid.  The block stages
// the input span of its tile ONCE in LDS -- about 256 M / L + P samples from the row's two segments: hist_in serves
// [k0, x_first), x serves [x_first, x_first + n), everything outside is zero; 16 bytes per load inside x (the tile's first
// staged sample is moved down to a 16-byte boundary of the row's own memory) -- and every lane then runs
// acc = fmaf(tab[i][m mod L], xs[off + i], acc), i ascending.  Taps that do not fit the staging area beside the span take
// several passes; a span that does not fit at all (M / L above 7) reads from global memory, the same chain.  Both are the
// routines of resample_common.h (rs_tile_output with E = 4, rs_one_output), sized by its stage_plan; this file passes its
// two-segment `sample` and the 16-byte load of x.
//
// The epilogue is the row's (out_store, resample_common.h): PCM16 as packed pairs from even lanes, G.711 codes four to a
// 32-bit store (wave shuffles) where the row's `out` is 4-byte aligned and the four lie inside out_fill; single elements
// only at a row's ragged end.  Behind m1 - m0 a lane encodes y = 0: the encoding's silence.  Extra blocks of the same grid
// write hist_out.  The set of rates is configured by resample_common.h's configure_rate into vsp_ctx::out_rates.
#include <algorithm>
#include <vector>

#include "model.h"
#include "resample_common.h"

namespace {

using namespace vsp::rs;

constexpr int OUT_TILE = RS_TILE;        // output samples (= threads) per block
constexpr int OUT_X_LDS_FLOATS = 2048;  // input staging area per block (8 KiB: eight blocks per CU keep their LDS)

static_assert(sizeof(vsp::OutRow) == 96 && sizeof(vsp::OutFilter) == 40, "descriptor layout");
static_assert(sizeof(vsp::OutRowsArgs) <= 4096, "kernel arguments must fit 4 KiB");
static_assert(vsp::OUT_FILTERS_MAX == VSP_OUTPUT_RATES_MAX, "one filter entry per configured rate");
static_assert(2 * vsp::OUT_ROWS_PER_LAUNCH >= vsp::STREAM_ROWS_MAX, "64 rows take at most two launches");

// grid (out_tiles + hist blocks, rows), OUT_TILE threads.  Dynamic LDS: the staging area of the launch's widest filter.
__global__ __launch_bounds__(OUT_TILE) void output_rows_kernel(const vsp::OutRowsArgs a) {
  extern __shared__ __align__(16) float out_xs[];
  const int tid = threadIdx.x;
  const vsp::OutRow& r = a.r[blockIdx.y];
  const vsp::OutFilter& f = a.f[r.filt];
  const int64_t x_first = r.x_first, x_end = x_first + r.n, k0 = r.k0;
  // sample k of the row's utterance: its new segment, its history, 0 elsewhere (before k0 no output of [m0, m1) has a
  // tap on it, behind x_end it is the filter's tail)
  auto sample = [&](int64_t k) {
    return k >= x_first ? (k < x_end ? r.x[k - x_first] : 0.f) : (k >= k0 ? r.hist_in[k - k0] : 0.f);
  };
  if ((int)blockIdx.x >= a.out_tiles) {                             // the history the row's next call reads
    const int64_t j = (int64_t)((int)blockIdx.x - a.out_tiles) * OUT_TILE + tid, k = r.k1 + j;
    if (r.hist_out && k < x_end) r.hist_out[j] = sample(k);
    return;
  }
  const int64_t j0 = (int64_t)blockIdx.x * OUT_TILE, j = j0 + tid;
  const int64_t cnt = r.m1 - r.m0;
  if (j0 >= r.out_fill) return;                                     // (uniform over the block, like the next branch)
  float acc = 0.f;
  if (j0 < cnt) {
    const int64_t m_first = r.m0 + j0, m_last = min(m_first + OUT_TILE, r.m1) - 1;
    if (f.mode == 2) {
      acc = rs_one_output(f.tab, f.L, f.M, f.J, f.P, min(m_first + tid, m_last), sample);
    } else {
      auto load = [&](int64_t k, float* v) {
        const float4 w = *reinterpret_cast<const float4*>(r.x + (k - x_first));
        v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
      };
      acc = rs_tile_output<4>(out_xs, f.tab, f.L, f.M, f.J, f.P, f.pass, m_first, m_last, (int64_t)((uintptr_t)r.x / 4) - x_first,
                              x_first, x_end, load, sample);
    }
  }
  out_store(r.out, r.enc, j, j < cnt ? acc : 0.f, r.out_fill);     // behind the row's outputs: the code of 0
}

// how output_rows_kernel stages a rate
vsp::OutFilter make_filter_entry(const vsp_ctx::RateTable& t) {
  const StagePlan sp = stage_plan(OUT_X_LDS_FLOATS, 3, 8, 4, t.L, t.M, t.P);
  return vsp::OutFilter{t.tab, t.L, t.M, t.H, t.J, t.P, sp.pass, sp.mode, sp.xs_words};
}

}  // namespace

int vsp_output_encode(int enc, const int16_t* pcm, int64_t n, uint8_t* codes) {
  if ((enc != VSP_OUT_ULAW && enc != VSP_OUT_ALAW) || n < 0 || (n > 0 && (!pcm || !codes))) return VSP_ERR_ARG;
  for (int64_t i = 0; i < n; ++i)
    codes[i] = (uint8_t)(enc == VSP_OUT_ULAW ? vsp::g711_ulaw_code(pcm[i]) : vsp::g711_alaw_code(pcm[i]));
  return VSP_OK;
}

int vsp_output_rows_plan(int L, int M, int H, int64_t x_first, int64_t n, int ended, int64_t* m0, int64_t* m1, int64_t* k0,
                         int64_t* k1) {
  const int64_t big = (int64_t)1 << 40;
  if (L < 1 || M < 1 || H < 0 || x_first < 0 || n < 0 || x_first > big || n > big) return VSP_ERR_ARG;
  const vsp::StreamOutPlan p = vsp::stream_output_plan(x_first, n, ended != 0, L, M, H);
  if (m0) *m0 = p.m0;
  if (m1) *m1 = p.m1;
  if (k0) *k0 = p.k0;
  if (k1) *k1 = p.k1;
  return VSP_OK;
}

namespace vsp {
hipError_t launch_output_rows(OutRowsArgs& a, int B, hipStream_t s) {
  if (B <= 0 || B > OUT_ROWS_PER_LAUNCH) return hipErrorInvalidValue;
  int64_t fill = 0, hist = 0;
  int xs_words = 0;
  for (int b = 0; b < B; ++b) {
    const OutRow& r = a.r[b];
    if (r.filt < 0 || r.filt >= OUT_FILTERS_MAX || !a.f[r.filt].tab || r.enc < VSP_OUT_F32 || r.enc > VSP_OUT_ALAW ||
        r.out_fill < r.m1 - r.m0 || r.m1 < r.m0 || r.n < 0 || r.k0 > r.x_first || r.k1 > r.x_first + r.n || r.k1 < r.k0)
      return hipErrorInvalidValue;
    fill = std::max(fill, r.out_fill);
    if (r.hist_out) hist = std::max(hist, r.x_first + r.n - r.k1);
    xs_words = std::max(xs_words, a.f[r.filt].xs_words);
  }
  a.out_tiles = (int)((fill + OUT_TILE - 1) / OUT_TILE);
  a.pad = 0;
  const int hist_blocks = (int)((hist + OUT_TILE - 1) / OUT_TILE);
  if (a.out_tiles + hist_blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(output_rows_kernel, dim3((unsigned)(a.out_tiles + hist_blocks), (unsigned)B), dim3(OUT_TILE),
                     (size_t)xs_words * sizeof(float), s, a);
  return hipGetLastError();
}
}  // namespace vsp

int vsp_output_rate_configure(vsp_ctx* ctx, int model_rate, int out_rate, int zeros, double beta, double rolloff) {
  if (!ctx) return VSP_ERR_ARG;
  if (out_rate <= 0) return ctx->fail(VSP_ERR_ARG, "output rows: out_rate must be positive");
  if (model_rate == 0) {                                  // drop the rate
    drop_rate(ctx, find_rate(ctx->out_rates, VSP_OUTPUT_RATES_MAX, out_rate));
    return VSP_OK;
  }
  return configure_rate(ctx, "output rows", "output", ctx->out_rates, VSP_OUTPUT_RATES_MAX, out_rate, model_rate, out_rate, zeros,
                        beta, rolloff, OUT_MAX_L, OUT_MAX_M);
}

int vsp_output_rows(vsp_ctx* ctx, void* stream, int B, const vsp_output_row* rows) {
  if (!ctx) return VSP_ERR_ARG;
  if (!rows || B < 1 || B > vsp::STREAM_ROWS_MAX)
    return ctx->fail(VSP_ERR_ARG, "vsp_output_rows: 1 <= B <= %d rows", vsp::STREAM_ROWS_MAX);
  const int64_t big = (int64_t)1 << 40;
  vsp::OutRow dev[vsp::STREAM_ROWS_MAX];
  for (int b = 0; b < B; ++b) {
    const vsp_output_row& r = rows[b];
    if (r.enc < VSP_OUT_F32 || r.enc > VSP_OUT_ALAW)
      return ctx->fail(VSP_ERR_ARG, "vsp_output_rows: row %d: enc must be one of VSP_OUT_*", b);
    if (r.n < 0 || r.n > big || r.x_first < 0 || r.x_first > big || r.out_fill < 0 || r.out_fill > big * 512)
      return ctx->fail(VSP_ERR_ARG, "vsp_output_rows: row %d has a negative x_first, n or out_fill", b);
    if (r.n == 0 && !r.ended) return ctx->fail(VSP_ERR_ARG, "vsp_output_rows: row %d: n == 0 is legal only with ended == 1", b);
    const vsp_ctx::RateTable* t = find_rate(ctx->out_rates, VSP_OUTPUT_RATES_MAX, r.out_rate);
    if (!t)
      return ctx->fail(VSP_ERR_STATE, "vsp_output_rows: row %d: rate %d Hz is not configured (vsp_output_rate_configure)", b,
                       r.out_rate);
    const vsp::StreamOutPlan p = vsp::stream_output_plan(r.x_first, r.n, r.ended != 0, t->L, t->M, t->H);
    const bool need_in = r.x_first > p.k0, need_out = !r.ended && r.x_first + r.n > p.k1;
    if ((r.n > 0 && !r.x) || (r.out_fill > 0 && !r.out) || (need_in && !r.hist_in) || (need_out && !r.hist_out))
      return ctx->fail(VSP_ERR_ARG, "vsp_output_rows: row %d lacks a pointer it needs (x, out, hist_in or hist_out)", b);
    if ((uintptr_t)r.x % 4 || (uintptr_t)r.hist_in % 4 || (uintptr_t)r.hist_out % 4 || (uintptr_t)r.out % enc_bytes(r.enc))
      return ctx->fail(VSP_ERR_ARG, "vsp_output_rows: row %d has a pointer misaligned to its element", b);
    if (r.hist_out && r.hist_in == r.hist_out)
      return ctx->fail(VSP_ERR_ARG, "vsp_output_rows: row %d: hist_in and hist_out must differ", b);
    if (p.m1 - p.m0 > r.out_fill)
      return ctx->fail(VSP_ERR_SHAPE, "vsp_output_rows: row %d delivers %lld output samples, out_fill is %lld", b,
                       (long long)(p.m1 - p.m0), (long long)r.out_fill);
    dev[b] = vsp::OutRow{r.x, need_in ? r.hist_in : nullptr, r.hist_out, r.out, r.x_first, r.n, p.m0, p.m1,
                         need_in ? p.k0 : r.x_first, p.k1, r.out_fill, r.enc, (int)(t - ctx->out_rates)};
  }
  // as few launches as the kernel-argument space allows, of about equal size
  const int launches = (B + vsp::OUT_ROWS_PER_LAUNCH - 1) / vsp::OUT_ROWS_PER_LAUNCH;
  for (int l = 0, b0 = 0; l < launches; ++l) {
    const int nb = (B - b0) / (launches - l);
    vsp::OutRowsArgs a = {};
    for (int i = 0; i < VSP_OUTPUT_RATES_MAX; ++i)
      if (ctx->out_rates[i].tab) a.f[i] = make_filter_entry(ctx->out_rates[i]);
    std::copy(dev + b0, dev + b0 + nb, a.r);
    const hipError_t e = vsp::launch_output_rows(a, nb, (hipStream_t)stream);
    if (e != hipSuccess) return ctx->fail(VSP_ERR_HIP, "output_rows_kernel: %s", hipGetErrorString(e));
    b0 += nb;
  }
  return VSP_OK;
}
