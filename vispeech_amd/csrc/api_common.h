// What the launch sequences of the C-ABI (include/vispeech_hip.h) share: the workspace allocator and the tensor view
// (op_host.h, which the stand-alone operators use too), the Run that carries one call's stream, error state and profiling, and the declarations of the run_* sequences.  The sequences
// restate SynthesizerTrn.infer (reference models.py:672-722) as HIP kernel launches on the caller's stream; no allocation
// and no host synchronisation happens on these paths except vsp_frame_lengths_host.
//   api_context.hip    context, weights, setters, stand-alone operators, profile readers
//   api_frame.hip      encoder, WN, flow, posterior encoder; encode / decode / infer and the per-stage entries
//   api_generator.hip  both generator schedules, plan_resblock, the streamed vocoder
//   api_convert.hip    spectrograms and voice conversion
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "model.h"
#include "op_host.h"
#include "row_controls.h"

namespace vsp {

// Stages that run one after another on one stream share scratch: every stage starts at the scope's mark -- next()
// between two of them --, and the scope leaves `cur` behind the largest.  The only place that moves `cur` back.
struct Overlay {
  Ws& ws;
  const size_t mark;
  size_t peak;
  explicit Overlay(Ws& w) : ws(w), mark(w.cur), peak(w.cur) {}
  void next() { peak = std::max(peak, ws.cur); ws.cur = mark; }
  ~Overlay() { ws.cur = std::max(peak, ws.cur); }
};

inline T3 ext(const float* p, int C, int T) { return T3{const_cast<float*>(p), (long)C * T, (long)T}; }

struct Run {
  vsp_ctx* ctx;
  hipStream_t s;
  Ws& ws;
  int rc = VSP_OK;
  // ragged batch of the channels-last generator (kernels.h, ClConvArgs::glen): frames per utterance of the batch chunk
  // being launched, and the columns per frame of the current stage's input / output tensors
  const int64_t* host_lengths = nullptr;   // the batch's frame counts where the host knows them (vsp_ctx::fl_known), else NULL
  const int* glen = nullptr;
  int grate_in = 0, grate_out = 0;
  bool iso = false;                        // isolated mode (model.h): the generator ends utterance b's tensors at in_lengths[b]
  // share of the padded frames the launches of the current generator chunk compute (trimmed tails): the profiled work
  // of a launch is charged for the frames it processes, not for the padded tensor (set while profiling only)
  double work_frac = 1.0;
  bool dry() const { return ws.dry; }
  const float* A(size_t off) const { return ctx->arena + off; }
  bool ok() const { return rc == VSP_OK && !ws.overflow; }
  void chk(hipError_t e, const char* what) {
    if (e != hipSuccess && rc == VSP_OK) rc = ctx->fail(VSP_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
  }

  static int fam(int kind, int channels) {
    if (channels <= 16) return kind | (7 << 3);   // (the 16-channel last stage of a five-stage generator: level 7)
    int l = 0;
    while ((32 << l) < channels && l < 7) ++l;
    return kind | (l << 3);
  }
  ConvArgs args(const Conv& L, T3 x, T3 out, int T_in, int Nq) const {
    ConvArgs a;
    std::memset(&a, 0, sizeof a);
    a.x = x.p; a.x_bs = x.bs; a.x_cs = x.cs;
    a.wp = A(L.w);
    a.bias = L.b >= 0 ? A((size_t)L.b) : nullptr;
    a.out = out.p; a.o_bs = out.bs; a.o_cs = out.cs;
    a.Cin = L.Cin; a.M = L.M; a.K = L.K; a.dil = L.dil; a.pad = L.pad;
    a.T_in = T_in; a.Nq = Nq;
    a.nchunks = (L.Cin + CONV_CK - 1) / CONV_CK;
    a.alpha = 1.f; a.div = 1.f;
    a.ups_s = L.ups_s; a.ups_p = L.ups_p;
    a.f16s = L.f16s ? 1 : 0;
    a.wg = (L.has_wg && ctx->cols) ? reinterpret_cast<const uint16_t*>(A(L.wg)) : nullptr;
    a.wg_max_blocks = ctx->cols_blocks;
    a.wg_min_blocks = ctx->cols_min_blocks;
    return a;
  }
  // event pair around one launch of a profiled class; end() books the launch's algorithmic work
  bool prof_begin(int cls, int fam = VSP_FAM_OTHER) {
    if (!ctx->prof_on) return false;
    while (ctx->ev_pool.size() < ctx->ev_used + 2) {
      hipEvent_t e;
      if (hipEventCreate(&e) != hipSuccess) { rc = ctx->fail(VSP_ERR_HIP, "hipEventCreate"); return false; }
      ctx->ev_pool.push_back(e);
    }
    if (ctx->ev_cls.size() < ctx->ev_pool.size() / 2) {
      ctx->ev_cls.resize(ctx->ev_pool.size() / 2, 0);
      ctx->ev_fam.resize(ctx->ev_pool.size() / 2, 0);
      ctx->ev_flops.resize(ctx->ev_pool.size() / 2, 0.0);
      ctx->ev_bytes.resize(ctx->ev_pool.size() / 2, 0.0);
      ctx->ev_moved.resize(ctx->ev_pool.size() / 2, 0.0);
    }
    ctx->ev_cls[ctx->ev_used / 2] = cls;
    ctx->ev_fam[ctx->ev_used / 2] = fam;
    (void)hipEventRecord(ctx->ev_pool[ctx->ev_used], s);
    return true;
  }
  // bytes: SURVEY 8d's layer-boundary model (input + output of every CONVOLUTION the launch replaces); bytes_ext: the same
  // plus residual / accumulate reads; bytes_moved: what the launch moves through HBM as fused (each operand once)
  void prof_end(int cls, double flops, double bytes, double bytes_ext, double bytes_moved) {
    (void)hipEventRecord(ctx->ev_pool[ctx->ev_used + 1], s);
    const double f = cls == VSP_PROF_GENERATOR ? work_frac : 1.0;
    ctx->ev_flops[ctx->ev_used / 2] = flops * f;
    ctx->ev_bytes[ctx->ev_used / 2] = bytes * f;
    ctx->ev_moved[ctx->ev_used / 2] = bytes_moved * f;
    ctx->ev_used += 2;
    ctx->prof_launches[cls] += 1;
    ctx->prof_flops[cls] += flops * f;
    ctx->prof_bytes[cls] += bytes * f;
    ctx->prof_bytes_ext[cls] += bytes_ext * f;
    ctx->prof_bytes_moved[cls] += bytes_moved * f;
  }
  int terms() const { return ctx->gen_mode == 2 ? 1 : 3; }
  ClW cw(const ClConv& L) const { return ClW{reinterpret_cast<const uint16_t*>(A(L.wg)), A((size_t)L.b)}; }
  // convolution i of a ResBlock in execution order (cl_args.h): ResBlock1 conv1, conv2 of pair 0, 1, ..; ResBlock2 conv_a, conv_b
  ClW cw(const ResBlockW& rb, int i) const { return cw(rb.kind == 2 ? rb.h1[i] : ((i & 1) ? rb.h2 : rb.h1)[i / 2]); }
  // Books a fused launch that replaces n convolutions C -> C (kernel K) on B x T columns and reads r residuals: each
  // convolution is charged its input and its output -> bytes; the residual reads and the accumulate read
  // (acc_prev) -> bytes_ext; as fused the launch moves input, output and the previous sum once each -> bytes_moved.
  // (pair: n 2, r 1; chain of np pairs: n 2 np, r np; ResBlock2: n 2, r 2)
  void prof_end_fused(int n, int r, int C, int K, int T, int B, bool acc_prev) {
    const double el = (double)T * C, acc = acc_prev ? 1.0 : 0.0;
    prof_end(VSP_PROF_GENERATOR, n * 2.0 * C * C * K * (double)T * B, 4.0 * B * el * (2.0 * n), 4.0 * B * el * (2.0 * n + r + acc),
             4.0 * B * el * (2.0 + acc));
  }
  // the tail every fused launch shares: what the schedule alone knows, the launch, the booking
  template <class Args>
  void launch_fused(Args a, hipError_t (*launch)(const Args&, int, hipStream_t), const char* what, int family, int n, int r, int C,
                    int K, bool acc_prev, float div, int B) {
    a.acc_prev = acc_prev ? 1 : 0; a.div = div;
    a.glen = glen; a.grate = grate_out;
    const bool prof = prof_begin(VSP_PROF_GENERATOR, fam(family, C));
    chk(launch(a, B, s), what);
    if (prof) prof_end_fused(n, r, C, K, a.T, B, acc_prev);
  }
  // Pairs [p0, p0 + np) of a ResBlock1, or a whole ResBlock2, as ONE launch: out = block(x) [+ out] [/ div], x != out.
  //   as_pair: g16_pair (gen16.hip; np = 1), which routes to g16_rw / g16_rw64 / g16_pp itself;
  //   else 16 channels: g16_c16 (gen16_c16.hip), charged to the family of the kernel it stands in for;
  //        ResBlock2: g16_rb2 (gen16_rb2.hip);  ResBlock1: g16_chain (gen16.hip), which routes to g16_rc itself.
  void clfused(const ResBlockW& rb, int ch, int p0, int np, bool as_pair, const float* x, float* out, int T, bool acc_prev,
               float div, int B) {
    if (dry() || !ok()) return;
    const int n = rb.kind == 2 ? 2 : 2 * np, nres = rb.kind == 2 ? 2 : np;   // convolutions replaced, residual reads
    ClW w[6];
    for (int i = 0; i < n; ++i) w[i] = cw(rb, 2 * p0 + i);
    const int* dil = rb.dil.data() + p0;
    const int family = rb.kind == 2 ? VSP_FAM_RB2 : as_pair ? VSP_FAM_PAIR : VSP_FAM_CHAIN;
    if (as_pair) {
      ClPairArgs a = cl_pair_args(w, ch, rb.k, dil[0], x, out, T, terms());
      a.ring = ctx->pair_ring ? 1 : 0;
      a.rw64 = ctx->rw64 ? 1 : 0;
      launch_fused(a, launch_g16_pair, "g16_pair", family, n, nres, ch, rb.k, acc_prev, div, B);
    } else if (ch == 16) {
      launch_fused(cl_c16_args(rb.kind, w, rb.k, dil, np, x, out, T, terms()), launch_g16_c16, "g16_c16", family, n, nres, ch, rb.k,
                   acc_prev, div, B);
    } else if (rb.kind == 2) {
      launch_fused(cl_rb2_args(w, ch, rb.k, dil, x, out, T, terms()), launch_g16_rb2, "g16_rb2", family, n, nres, ch, rb.k, acc_prev,
                   div, B);
    } else {
      ClChainArgs a = cl_chain_args(w, ch, rb.k, dil, np, x, out, T, terms());
      a.ring = ctx->chain_ring ? 1 : 0;
      launch_fused(a, launch_g16_chain, "g16_chain", family, n, nres, ch, rb.k, acc_prev, div, B);
    }
  }
  void conv(const ConvArgs& a, int B, bool generator = false) {
    if (dry() || !ok()) return;
    const int cls = generator ? VSP_PROF_GENERATOR : VSP_PROF_FRAME;
    const bool prof = prof_begin(cls, generator ? (a.ups_s > 0 ? fam(VSP_FAM_UPS, a.M / a.ups_s) : fam(VSP_FAM_PRE, a.M)) : VSP_FAM_OTHER);
    chk(launch_conv(a, B, s), "conv1d_f32_mfma");
    if (prof) {
      const double in_el = (double)a.T_in * a.Cin, out_el = (double)(a.ups_s > 0 ? a.T_store * (a.M / a.ups_s) : a.Nq * a.M);
      const double ext = 4.0 * B * (in_el + out_el * (1.0 + (a.res ? 1.0 : 0.0) + (a.acc_prev ? 1.0 : 0.0)));
      prof_end(cls, 2.0 * a.M * a.Cin * a.K * (double)a.Nq * B, 4.0 * B * (in_el + out_el), ext, ext);
    }
  }
  // One channels-last split-f16 convolution of the generator (g16_conv): a ResBlock convolution x [B][T][C] -> out [+ res],
  // or an up-convolution (L.phases > 1) x [B][T][Cin] -> out [B][T phases][Cout].
  // x_img / o_img (round 4): the input read from / the result (also, or with out == NULL only) written as an OPERAND
  // IMAGE (kernels.h ClConvArgs): a ResBlock's intermediate lives in HBM as the next convolution's split, activated
  // window planes and reaches its LDS by LDS-DMA, without conversion arithmetic in the consumer.
  void clconv(const ClConv& L, const float* x, float* out, const float* res, int T, bool acc_prev, float div, int B,
              const uint16_t* x_img = nullptr, uint16_t* o_img = nullptr) {
    if (dry() || !ok()) return;
    ClConvArgs a = L.phases > 1 ? cl_ups_args(cw(L), L.Cin, L.Cout, L.K, L.phases, x, T, CL_LRELU_SLOPE, out, terms())
                                : cl_conv_args(cw(L), L.Cin, L.Cout, L.K, L.dil, x, T, CL_LRELU_SLOPE, res, out, terms());
    a.x_img = x_img; a.o_img = o_img;
    a.acc_prev = acc_prev ? 1 : 0; a.div = div;
    a.glen = glen; a.g_in = L.phases > 1 ? grate_in : grate_out; a.g_store = grate_out;
    const bool prof = prof_begin(VSP_PROF_GENERATOR, fam(L.phases > 1 ? VSP_FAM_UPS : VSP_FAM_CONV, L.Cout));
    chk(launch_g16_conv(a, B, s), "g16_conv");
    if (prof) {
      // input once + output once; the residual / accumulate reads go to bytes_ext
      const double in_el = (double)a.T_in * L.Cin, out_el = (double)a.T_store * L.Cout;
      const double ext = 4.0 * B * (in_el + out_el * (1.0 + (res ? 1.0 : 0.0) + (acc_prev ? 1.0 : 0.0)));
      prof_end(VSP_PROF_GENERATOR, 2.0 * L.Cout * L.Cin * L.K * L.phases * (double)a.Nq * B, 4.0 * B * (in_el + out_el), ext,
               ext + (out && o_img ? 4.0 * B * out_el : 0.0));
    }
  }
  // cond(g): 1x1 conv on g [B][gin] (T = 1) -> out [B][M]
  void cond(const Conv& L, const float* g, float* out, int B) {
    const int gin = L.Cin;
    ConvArgs a = args(L, T3{const_cast<float*>(g), (long)gin, 1}, T3{out, (long)L.M, 1}, 1, 1);
    conv(a, B);
  }
  void ln(T3 x, T3 res, size_t gamma, size_t beta, T3 y, int B, int C, int T) {
    if (dry() || !ok()) return;
    chk(launch_layernorm(x.p, x.bs, x.cs, res.p, res.bs, res.cs, A(gamma), A(beta), y.p, y.bs, y.cs, B, C, T, s),
        "layernorm");
  }
};

// The bytes a sequence needs: its dry pass.  seq(Run&) allocates and launches; its error, if any, stays in the Run.
template <class Seq>
int64_t dry_bytes(const vsp_ctx* ctx, Seq seq) {
  Ws ws(nullptr, 0, true);
  Run r{const_cast<vsp_ctx*>(ctx), nullptr, ws};
  seq(r);
  return (int64_t)ws.cur;
}

// What every entry point does once its arguments are checked: refuse a workspace shorter than `need` (the dry pass of the
// same sequence, vsp_*_workspace_bytes), run the sequence on the workspace behind its first `head` bytes, and report a
// sequence that still ran out (a sizing pass that disagrees with its run).
template <class Seq>
int run_sized(vsp_ctx* ctx, void* stream, const char* what, int64_t need, void* workspace, int64_t workspace_bytes, Seq seq,
              int64_t head = 0) {
  if (need >= 0 && workspace_bytes >= need) {
    Ws ws(static_cast<char*>(workspace) + head, (size_t)(workspace_bytes - head), false);
    Run r{ctx, (hipStream_t)stream, ws};
    seq(r);
    if (!ws.overflow) return r.rc;
    need = head + (int64_t)ws.cur;
  }
  return ctx->fail(VSP_ERR_WORKSPACE, "%s workspace too small: %lld < %lld bytes", what, (long long)workspace_bytes, (long long)need);
}

int check_ready(vsp_ctx* ctx);
int check_vc(vsp_ctx* ctx);      // ... and the posterior encoder's weights are there (voice conversion)

// api_frame.hip
void run_encoder_masked(Run& r, const EncoderW& E, int B, int T, T3 x_in, const int64_t* lengths, T3 y_out);
void mask3(Run& r, T3 x, const int64_t* lengths, int B, int C, int T);
void run_wn(Run& r, const Conv* cond, const std::vector<Conv>& in, const std::vector<Conv>& res, const std::vector<Conv>& skip,
            int nl, int B, int T, T3 H, T3 ACT, T3 OUT, float* gc, long gc_bs, const float* g, const int64_t* lengths);
void run_flow(Run& r, int B, int T, T3 z, const float* g, const int64_t* lengths, bool reverse = true);
void run_posterior(Run& r, int B, int T, T3 y, const int64_t* lengths, const float* g, const float* noise, T3 Z, T3 M, T3 LOGS,
                   float noise_scale = 1.f);
void draw_noise_rows(Run& r, uint64_t* seeds_dev, const int64_t* lengths, int B, int C, int T, float* drawn);
// api_generator.hip
void run_gen(Run& r, int B, int T, T3 z, const int64_t* in_lengths, const float* g, float* o);
// the context's silence table (model.h): built, synchronously on s, when weights are committed; dropped when they change
void tail_table_build(vsp_ctx* ctx, hipStream_t s);
void tail_table_drop(vsp_ctx* ctx);

}  // namespace vsp
