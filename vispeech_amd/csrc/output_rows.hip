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
// several passes; a span that does not fit at all (M / L above 7) reads from global memory, the same chain.
//
// The epilogue is the row's: PCM16 as packed pairs from even lanes, G.711 codes four to a 32-bit store (wave shuffles)
// where the row's `out` is 4-byte aligned and the four lie inside out_fill; single elements only at a row's ragged end.
// Behind m1 - m0 a lane encodes y = 0: the encoding's silence.  Extra blocks of the same grid write hist_out.
#include <algorithm>
#include <vector>

#include "model.h"
#include "resample_common.h"

namespace {

using namespace vsp::rs;

constexpr int OUT_TILE = 256;           // output samples (= threads) per block
constexpr int OUT_X_LDS_FLOATS = 2048;  // input staging area per block (8 KiB: eight blocks per CU keep their LDS)
constexpr int OUT_MIN_PASS = 32;        // fewer taps per staging pass than this: read x from global memory instead
constexpr int OUT_MAX_L = 320, OUT_MAX_M = 441;   // the output stage's own limits (resample.hip)

static_assert(sizeof(vsp::OutRow) == 96 && sizeof(vsp::OutFilter) == 40, "descriptor layout");
static_assert(sizeof(vsp::OutRowsArgs) <= 4096, "kernel arguments must fit 4 KiB");
static_assert(vsp::OUT_FILTERS_MAX == VSP_OUTPUT_RATES_MAX, "one filter entry per configured rate");
static_assert(2 * vsp::OUT_ROWS_PER_LAUNCH >= vsp::STREAM_ROWS_MAX, "64 rows take at most two launches");

// Stores element j of a row in its encoding.  Every lane of the block calls it (the shuffles take all of them) with a valid
// y; lanes with j < fill store.  j - threadIdx.x is a multiple of OUT_TILE, so j and the lane agree modulo 2 and 4.
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
  const uint32_t c = (uint32_t)(enc == VSP_OUT_ULAW ? vsp::g711_ulaw_code(q) : vsp::g711_alaw_code(q));
  const uint32_t c1 = __shfl_down(c, 1), c2 = __shfl_down(c, 2), c3 = __shfl_down(c, 3);
  uint8_t* o = static_cast<uint8_t*>(out) + j;
  if (word_ok && (j | 3) < fill) {                                  // the lane's whole group of four is stored
    if (!(threadIdx.x & 3)) *reinterpret_cast<uint32_t*>(o) = c | (c1 << 8) | (c2 << 16) | (c3 << 24);
  } else if (active) {
    *o = (uint8_t)c;
  }
}

// grid (out_tiles + hist blocks, rows), OUT_TILE threads.  Dynamic LDS: the staging area of the launch's widest filter.
__global__ __launch_bounds__(OUT_TILE) void output_rows_kernel(const vsp::OutRowsArgs a) {
  extern __shared__ __align__(16) float out_xs[];
  float* xs = out_xs;
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
    const int64_t m_first = r.m0 + j0;
    const int64_t m_last = min(m_first + OUT_TILE, r.m1) - 1;
    const int64_t m = m_first + tid;
    const int64_t mm = m <= m_last ? m : m_last;                    // idle lanes shadow the last sample: offsets stay in the tile
    const int64_t ks = (mm * f.M) / f.L - f.J;                      // first input sample of this output
    const float* __restrict__ tcol = f.tab + (int)(mm % f.L);
    if (f.mode == 2) {
      acc = rs_one_output(tcol, f.L, f.P, ks, sample);
    } else {
      int64_t kb = (m_first * f.M) / f.L - f.J;                     // first input sample of the tile
      kb -= ((int64_t)((uintptr_t)r.x / 4) + (kb - x_first)) & 3;   // ... moved down to a 16-byte boundary of x's memory
      const int off = (int)(ks - kb);
      const int span = (int)((m_last * f.M) / f.L - f.J - kb) + 1;  // tile words before the pass's taps are added
      for (int i0 = 0; i0 < f.P; i0 += f.pass) {                    // (pass % 4 == 0 when there is more than one)
        const int n_i = min(f.pass, f.P - i0);
        const int need = span + n_i - 1;
        const int64_t k_base = kb + i0;
        if (i0) __syncthreads();
        for (int o = tid * 4; o < need; o += OUT_TILE * 4) {
          const int64_t k = k_base + o;
          float4 v;
          if (k >= x_first && k + 4 <= x_end) {
            v = *reinterpret_cast<const float4*>(r.x + (k - x_first));
          } else {
            v.x = sample(k);
            v.y = sample(k + 1);
            v.z = sample(k + 2);
            v.w = sample(k + 3);
          }
          *reinterpret_cast<float4*>(xs + o) = v;
        }
        __syncthreads();
        const float* __restrict__ tp = tcol + (size_t)i0 * f.L;
        const float* xo = xs + off;
        int i = 0;
        for (; i + 4 <= n_i; i += 4) {                              // (four table loads in flight; the FMA order stays ascending)
          const float t0 = tp[(size_t)i * f.L], t1 = tp[(size_t)(i + 1) * f.L], t2 = tp[(size_t)(i + 2) * f.L],
                      t3 = tp[(size_t)(i + 3) * f.L];
          acc = fmaf(t0, xo[i], acc);
          acc = fmaf(t1, xo[i + 1], acc);
          acc = fmaf(t2, xo[i + 2], acc);
          acc = fmaf(t3, xo[i + 3], acc);
        }
        for (; i < n_i; ++i) acc = fmaf(tp[(size_t)i * f.L], xo[i], acc);
      }
    }
  }
  out_store(r.out, r.enc, j, j < cnt ? acc : 0.f, r.out_fill);     // behind the row's outputs: the code of 0
}

int make_plan(int model_rate, int out_rate, int zeros, Plan& p) {
  return vsp::rs::make_plan(model_rate, out_rate, zeros, OUT_MAX_L, OUT_MAX_M, p);
}

int enc_bytes(int enc) { return enc == VSP_OUT_F32 ? 4 : enc == VSP_OUT_S16 ? 2 : 1; }

vsp_ctx::InputRate* find_rate(vsp_ctx* ctx, int rate) {
  for (auto& r : ctx->out_rates)
    if (r.tab && r.rate == rate) return &r;
  return nullptr;
}

// how output_rows_kernel stages a rate: the arithmetic of vsp_output_chunk's launch with this kernel's staging area
vsp::OutFilter make_filter_entry(const vsp_ctx::InputRate& t) {
  vsp::OutFilter f{t.tab, t.L, t.M, t.H, t.J, t.P, t.P, 2, 0};
  // tile words: the outputs of a tile start within (TILE - 1) M / L + 1 samples of each other, + 3 for the alignment
  const int64_t span = ((int64_t)(OUT_TILE - 1) * t.M) / t.L + 2 + 3;
  const int64_t room = OUT_X_LDS_FLOATS - span - 8;                 // (the last 16-byte store's overhang)
  if (room >= std::min<int64_t>(t.P, OUT_MIN_PASS)) {
    f.pass = room >= t.P ? t.P : (int)(room & ~(int64_t)3);
    f.mode = 0;
    f.xs_words = (int)((span + f.pass + 8 + 3) & ~(int64_t)3);
  }
  return f;
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
  vsp_ctx::InputRate* slot = find_rate(ctx, out_rate);
  if (model_rate == 0) {                                  // drop the rate
    if (slot) {
      (void)hipSetDevice(ctx->device);
      (void)hipFree(slot->tab);
      *slot = vsp_ctx::InputRate();
    }
    return VSP_OK;
  }
  if (zeros == 0) zeros = 32;
  if (!(beta >= 0.0)) return ctx->fail(VSP_ERR_ARG, "output rows: beta must be >= 0");
  if (!(rolloff <= 1.0)) return ctx->fail(VSP_ERR_ARG, "output rows: rolloff must be in (0, 1] (<= 0: 1 - 3.065 / zeros)");
  Plan p;
  if (int rc = make_plan(model_rate, out_rate, zeros, p))
    return ctx->fail(rc, "output rows %d -> %d Hz, %d zeros: rates must be positive, L <= %d, M <= %d, 1 <= zeros <= 64", model_rate,
                     out_rate, zeros, OUT_MAX_L, OUT_MAX_M);
  if (!slot) {
    for (auto& r : ctx->out_rates)
      if (!r.tab) { slot = &r; break; }
    if (!slot) return ctx->fail(VSP_ERR_STATE, "output rows: %d output rates are configured already", VSP_OUTPUT_RATES_MAX);
  }
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
    return ctx->fail(VSP_ERR_HIP, "output rows table: %s", hipGetErrorString(e));
  }
  float* old = slot->tab;
  slot->rate = out_rate;
  slot->L = p.L; slot->M = p.M; slot->H = p.H; slot->J = J; slot->P = P;
  slot->tab = static_cast<float*>(d);                     // (last: a slot counts as configured once it has a table)
  if (old) (void)hipFree(old);
  return VSP_OK;
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
    const vsp_ctx::InputRate* t = find_rate(ctx, r.out_rate);
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
