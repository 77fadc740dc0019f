// C-ABI of libvispeech_hip (include/vispeech_hip.h): context, weights, and the launch sequences
// that restate SynthesizerTrn.infer (reference models.py:672-722) as HIP kernel launches on the
// caller's stream.  No allocation and no host synchronisation happens on these paths except
// vsp_frame_lengths_host.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "model.h"
#include "row_controls.h"

using namespace vsp;

namespace {

void generator_frame_dependence(const vsp_config& c, int resblock, int pre_k, int post_k, int& back, int& fwd);   // (defined below)
long total_upsample(const vsp_config& c);

struct T3 {
  float* p = nullptr;
  long bs = 0, cs = 0;
  T3 chan(int c) const { return T3{p ? p + (size_t)c * cs : nullptr, bs, cs}; }
};

// Bump allocator over the caller's workspace; in dry mode it only measures.
struct Ws {
  char* base;
  size_t cap;
  size_t cur = 0;
  bool dry;
  bool overflow = false;
  Ws(void* b, size_t c, bool d) : base((char*)b), cap(c), dry(d) {}
  void* bytes(size_t n) {
    const size_t o = cur;
    cur += (n + 255) / 256 * 256;
    if (dry) return nullptr;
    if (cur > cap) { overflow = true; return nullptr; }
    return base + o;
  }
  float* f(size_t n) { return (float*)bytes(n * sizeof(float)); }
  T3 t3(int B, int C, int T) {
    const long ts = (T + 63) / 64 * 64;
    T3 t;
    t.p = f((size_t)B * C * ts);
    t.cs = ts;
    t.bs = (long)C * ts;
    return t;
  }
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

// attentions.Encoder.forward (reference attentions.py:35-47) including the x * x_mask the reference applies at its exit
// (:46).  x_in must already be masked by the caller's semantics (every reference call site passes x * x_mask); it is
// read, never written: layer 0 takes it as its input and residual directly (round 5: no entry copy), and the last
// layer's second LayerNorm writes y_out, masked in place behind it (no exit copy; a mask folded into the LayerNorm
// kernel's store was measured: its scalar spills made EVERY LayerNorm launch 9 us slower).
void run_encoder_masked(Run& r, const EncoderW& E, int B, int T, T3 x_in, const int64_t* lengths, T3 y_out) {
  const vsp_config& c = r.ctx->cfg;
  const int h = c.hidden_channels, f = c.filter_channels;
  T3 X = r.ws.t3(B, h, T), S = r.ws.t3(B, h, T), QKV = r.ws.t3(B, 3 * h, T), AT = r.ws.t3(B, h, T),
     FF = r.ws.t3(B, f, T);
  void* AP = r.ctx->att_f16s ? r.ws.bytes(3 * attn_pack_bytes(B, c.n_heads, h / c.n_heads, T)) : nullptr;   // packed q | k | v images
  if (E.layers.empty()) {                       // (no layer: y = x * mask)
    if (!r.dry() && r.ok()) {
      r.chk(launch_copy3(x_in.p, x_in.bs, x_in.cs, y_out.p, y_out.bs, y_out.cs, B, h, T, r.s), "copy");
      if (lengths) r.chk(launch_mask3(y_out.p, y_out.bs, y_out.cs, lengths, B, h, T, r.s), "mask");
    }
    return;
  }
  // round 6, the column-tile kernels (conv_cols.h): the projections write the packed attention operands themselves
  // (no [B][3h][T] tensor, no pack launch) and conv_o normalises in its own launch (no LayerNorm launch): 8 -> 6 launches
  // per layer.  VSP_COLS=0: the separate launches (second implementation, tests/test_hip_parity.py).
  // (not for a handful of column tiles -- one utterance --: a column-tile block is one chain of round trips of 10+ us, the
  // row-tiled kernels' blocks are shorter than the launch they save: measured 3.12 against 3.14 ms for one utterance)
  const long col_tiles = (long)B * ((T + 63) / 64);
  const bool cols_size = col_tiles >= r.ctx->cols_min_blocks;
  const bool fuse_qkv = r.ctx->cols && cols_size && r.ctx->att_f16s && r.ctx->frame_f16s && E.layers[0].qkv.has_wg &&
                        E.layers[0].qkv.Cin == h && attn_qkv_pack_supported(h, c.n_heads);
  const bool fuse_ln = r.ctx->cols && cols_size && r.ctx->frame_f16s && E.layers[0].o.has_wg && h == 192;
  for (size_t i = 0; i < E.layers.size(); ++i) {
    const EncLayer& L = E.layers[i];
    const T3 Xi = i == 0 ? x_in : X;            // this layer's input
    const bool last = i + 1 == E.layers.size();
    ConvArgs a = r.args(L.qkv, Xi, QKV, T, T);
    a.lengths = lengths; a.in_mask = 1;  // x * x_mask feeds the attention (attentions.py:38)
    if (!fuse_qkv) r.conv(a, B);
    else if (!r.dry() && r.ok()) {
      const bool prof = r.prof_begin(VSP_PROF_FRAME);
      r.chk(launch_attn_qkv_pack_f16s(Xi.p, Xi.bs, Xi.cs, a.wg, a.bias, lengths, B, h, c.n_heads, T, AP, r.s), "q | k | v + pack");
      if (prof) {
        const double in_el = (double)T * h, out_el = (double)T * 3 * h;
        r.prof_end(VSP_PROF_FRAME, 2.0 * 3 * h * h * (double)T * B, 4.0 * B * (in_el + out_el), 4.0 * B * (in_el + out_el),
                   4.0 * B * (in_el + out_el));
      }
    }
    if (!r.dry() && r.ok()) {
      const bool prof = r.prof_begin(VSP_PROF_ATTENTION);
      if (r.ctx->att_f16s)
        r.chk(launch_attention_f16s(fuse_qkv ? nullptr : QKV.p, QKV.bs, QKV.cs, r.A(L.ek), r.A(L.ev), lengths, AT.p, AT.bs, AT.cs, B, h,
                                    c.n_heads, T, c.window_size, AP, r.s), "attention (split f16)");
      else
        r.chk(launch_attention(QKV.p, QKV.bs, QKV.cs, r.A(L.ek), r.A(L.ev), lengths, AT.p, AT.bs, AT.cs, B, h,
                               c.n_heads, T, c.window_size, r.ctx->att_ksplit, r.s), "attention");
      // QK^T and PV: 2 * h * T^2 MAC per utterance; banded relative logits and values: 2 * h * T * (2w+1) MAC
      if (prof) r.prof_end(VSP_PROF_ATTENTION, (double)B * (4.0 * h * (double)T * T + 4.0 * h * (double)T * (2 * c.window_size + 1)),
                           4.0 * B * 4.0 * h * (double)T, 4.0 * B * 4.0 * h * (double)T, 4.0 * B * 4.0 * h * (double)T);
    }
    // S = x + conv_o(att);  X = LayerNorm(S)
    a = r.args(L.o, AT, S, T, T);
    a.res = Xi.p; a.r_bs = Xi.bs; a.r_cs = Xi.cs;
    if (fuse_ln && a.wg) {
      // one launch: the block holds every channel of its columns (Xi may be X: a block reads and writes its own columns only)
      a.out = X.p; a.o_bs = X.bs; a.o_cs = X.cs;
      if (!r.dry() && r.ok()) {
        const bool prof = r.prof_begin(VSP_PROF_FRAME);
        r.chk(launch_conv_cols(a, B, r.s, r.A(L.g1), r.A(L.b1)), "conv_o + LayerNorm");
        if (prof) {
          const double el = (double)T * h;
          r.prof_end(VSP_PROF_FRAME, 2.0 * h * h * (double)T * B, 4.0 * B * 2.0 * el, 4.0 * B * 3.0 * el, 4.0 * B * 3.0 * el);
        }
      }
    } else {
      r.conv(a, B);
      r.ln(S, T3{}, L.g1, L.b1, X, B, h, T);
    }
    // FFN (attentions.py:277-285)
    a = r.args(L.f1, X, FF, T, T);
    a.lengths = lengths; a.in_mask = 1; a.act = 1;
    r.conv(a, B);
    a = r.args(L.f2, FF, S, T, T);
    a.lengths = lengths; a.in_mask = 1; a.mask_pre = 1;
    a.res = X.p; a.r_bs = X.bs; a.r_cs = X.cs;
    r.conv(a, B);
    r.ln(S, T3{}, L.g2, L.b2, last ? y_out : X, B, h, T);
  }
  // y = x * mask (attentions.py:46)
  if (lengths && !r.dry() && r.ok()) r.chk(launch_mask3(y_out.p, y_out.bs, y_out.cs, lengths, B, h, T, r.s), "mask");
}

void mask3(Run& r, T3 x, const int64_t* lengths, int B, int C, int T) {
  if (r.dry() || !r.ok() || !lengths) return;
  r.chk(launch_mask3(x.p, x.bs, x.cs, lengths, B, C, T, r.s), "mask");
}

// modules.WN.forward (reference modules.py:148-176; dilation_rate 1) on H [B][h][T]: H is the running
// residual stream (destroyed), OUT receives the masked skip sum.  gc: nl * 2h conditioning rows.
// cond != null: cond_layer(g) is evaluated here into gc [B][nl * 2h]; null: gc already holds it, batch stride gc_bs.
void run_wn(Run& r, const Conv* cond, const std::vector<Conv>& in, const std::vector<Conv>& res,
            const std::vector<Conv>& skip, int nl, int B, int T, T3 H, T3 ACT, T3 OUT, float* gc, long gc_bs, const float* g,
            const int64_t* lengths) {
  const int h = r.ctx->cfg.hidden_channels;
  if (cond) r.cond(*cond, g, gc, B);
  for (int l = 0; l < nl; ++l) {
    ConvArgs a = r.args(in[l], H, ACT, T, T);
    a.act = 2; a.cond = gc ? gc + (size_t)l * 2 * h : nullptr; a.cond_bs = gc_bs;
    r.conv(a, B);
    if (l < nl - 1) {
      // res_skip_layers[l] (modules.py:165-172) as one launch with two destinations: rows [0, h) are the in-place
      // residual update H = (H + res) * mask, rows [h, 2 h) accumulate into the skip sum
      a = r.args(res[l], ACT, H, T, T);
      a.res = H.p; a.r_bs = H.bs; a.r_cs = H.cs;
      a.lengths = lengths; a.mask_post = 1;
      a.split_row = h; a.out2 = OUT.p; a.o2_bs = OUT.bs; a.o2_cs = OUT.cs; a.acc_prev2 = l > 0;
      r.conv(a, B);
    } else {
      a = r.args(skip[l], ACT, OUT, T, T);
      a.acc_prev = l > 0;
      a.lengths = lengths; a.mask_post = 1;
      r.conv(a, B);
    }
  }
}

// ResidualCouplingBlock.forward in place on z [B][inter][T] (reference models.py:202-209,
// modules.py:324-343, 148-176).  reverse: x1 = (x1 - m) * mask, layers n-1 .. 0 (infer);
// forward: x1 = m + x1 * mask, layers 0 .. n-1 (voice conversion).  With an even number of flows
// layer i sees the same channel flip in both directions (i and n - i flips).
void run_flow(Run& r, int B, int T, T3 z, const float* g, const int64_t* lengths, bool reverse = true) {
  const vsp_config& c = r.ctx->cfg;
  const Model& m = r.ctx->model;
  const int h = c.hidden_channels, half = c.inter_channels / 2, fl = c.flow_layers;
  T3 H = r.ws.t3(B, h, T), ACT = r.ws.t3(B, h, T), OUT = r.ws.t3(B, h, T);
  // cond_layer(g) of all coupling layers: one launch (reference modules.py:153-155, once per WN.forward)
  const long gcs = (long)c.n_flows * 2 * h * fl;
  float* gc = r.ws.f((size_t)B * gcs);
  r.cond(m.flow_cond_all, g, gc, B);
  for (int n = 0; n < c.n_flows; ++n) {
    const int i = reverse ? c.n_flows - 1 - n : n;
    const FlowW& F = m.flows[i];
    const T3 x0 = F.flipped ? z.chan(half) : z;
    const T3 x1 = F.flipped ? z : z.chan(half);
    ConvArgs a = r.args(F.pre, x0, H, T, T);
    a.lengths = lengths; a.mask_post = 1;
    r.conv(a, B);
    run_wn(r, nullptr, F.in, F.res, F.skip, fl, B, T, H, ACT, OUT, gc ? gc + (size_t)i * 2 * h * fl : nullptr, gcs, g, lengths);
    // m = post(out) * mask ; x1 = (x1 -/+ m) * mask
    a = r.args(F.post, OUT, x1, T, T);
    a.lengths = lengths; a.mask_pre = 1; a.alpha = reverse ? -1.f : 1.f;
    a.res = x1.p; a.r_bs = x1.bs; a.r_cs = x1.cs;
    a.mask_post = 1;
    r.conv(a, B);
  }
}

// PosteriorEncoder.forward (reference models.py:233-241): y [B][spec][T] -> m, logs, z [B][inter][T].
void run_posterior(Run& r, int B, int T, T3 y, const int64_t* lengths, const float* g, const float* noise, T3 Z,
                   T3 M, T3 LOGS, float noise_scale = 1.f) {
  const vsp_config& c = r.ctx->cfg;
  const PosteriorW& Q = r.ctx->model.enc_q;
  const int h = c.hidden_channels, ql = c.posterior_layers;
  T3 H = r.ws.t3(B, h, T), ACT = r.ws.t3(B, h, T), OUT = r.ws.t3(B, h, T);
  float* gc = r.ws.f((size_t)B * 2 * h * ql);
  if (r.dry()) return;
  ConvArgs a = r.args(Q.pre, y, H, T, T);
  a.lengths = lengths; a.mask_post = 1;
  r.conv(a, B);
  run_wn(r, &Q.cond, Q.in, Q.res, Q.skip, ql, B, T, H, ACT, OUT, gc, 2L * h * ql, g, lengths);
  // proj: m and logs rows in one launch, two destinations (reference models.py:238-239: stats = proj(x) * mask, split)
  a = r.args(Q.proj, OUT, M, T, T);
  a.lengths = lengths; a.mask_post = 1;
  a.split_row = c.inter_channels; a.out2 = LOGS.p; a.o2_bs = LOGS.bs; a.o2_cs = LOGS.cs; a.mask_post2 = 1;
  r.conv(a, B);
  if (r.ok()) {
    // z = (m + eps * exp(logs)) * mask   (contiguous [B][inter][T] outputs)
    r.chk(launch_reparam(M.p, LOGS.p, noise, noise_scale, Z.p, (long)B * c.inter_channels * T, r.s), "reparam");
    r.chk(launch_mask3(Z.p, Z.bs, Z.cs, lengths, B, c.inter_channels, T, r.s), "mask");
  }
}

// max over the generator's stages of f(channels, columns): stage i has upsample_initial_channel >> (i + 1) channels and
// T * upsample_rates[0] * .. * upsample_rates[i] columns per utterance
template <class F>
size_t max_over_stages(const vsp_config& c, int T, size_t mx, F f) {
  long t = T;
  for (int i = 0; i < c.n_upsamples; ++i) {
    t *= c.upsample_rates[i];
    mx = std::max(mx, (size_t)f(c.upsample_initial_channel >> (i + 1), t));
  }
  return mx;
}

// Generator.forward (reference models.py:271-290).  z [B][inter][T]; in_lengths != null applies
// the (z * x_mask) of models.py:720 while staging conv_pre's input.
void run_generator(Run& r, int B, int T, T3 z, const int64_t* in_lengths, const float* g, float* o) {
  const vsp_config& c = r.ctx->cfg;
  const Model& m = r.ctx->model;
  const int c0 = c.upsample_initial_channel, nk = c.n_resblock_kernels;
  float* gc = r.ws.f((size_t)B * c0);
  r.cond(m.g_cond, g, gc, B);
  // buffer sizes: max over stages of C * T
  const size_t mx = max_over_stages(c, T, (size_t)c0 * ((T + 63) / 64 * 64),
                                    [](int ch, long t) { return (size_t)ch * (size_t)((t + 63) / 64 * 64); });
  float* buf[5];
  for (auto& b : buf) b = r.ws.f((size_t)B * mx);
  auto view = [&](int k, int C, long Tn) {
    const long ts = (Tn + 63) / 64 * 64;
    return T3{buf[k], (long)C * ts, ts};
  };
  int cur = 0;  // buffer holding the stage input
  T3 X = view(cur, c0, T);
  // Isolated mode: these kernels have no per-utterance extent, but every convolution can mask its staged input
  // (ConvArgs::lengths + in_mask): with utterance b's length at every stage's rate, whatever a launch writes behind an
  // utterance's end is never read by the next one -- each convolution sees the zero padding of a tensor that ends there.
  // (the array is part of the workspace in either mode: its size does not depend on the context's state)
  int64_t* const stage_len = reinterpret_cast<int64_t*>(r.ws.bytes((size_t)(VSP_MAX_LIST + 1) * B * sizeof(int64_t)));
  const bool iso = r.iso && in_lengths;
  if (iso && !r.dry() && r.ok()) {
    long rate[VSP_MAX_LIST + 1] = {1};
    for (int i = 0; i < c.n_upsamples; ++i) rate[i + 1] = rate[i] * m.ups[i].ups_s;
    r.chk(launch_stage_lengths(in_lengths, B, rate, c.n_upsamples + 1, stage_len, r.s), "stage_lengths");
  }
  auto own_end = [&](ConvArgs& ca, int stage) {
    if (iso) { ca.lengths = stage_len + (size_t)stage * B; ca.in_mask = 1; }
  };
  ConvArgs a = r.args(m.g_pre, z, X, T, T);
  a.lengths = in_lengths; a.in_mask = in_lengths ? 1 : 0;
  a.cond = gc; a.cond_bs = c0;
  r.conv(a, B, true);
  long Tn = T;
  int ch = c0;
  for (int i = 0; i < c.n_upsamples; ++i) {
    const Conv& U = m.ups[i];
    const long Tout = Tn * U.ups_s;
    ch = c0 >> (i + 1);
    // free buffers: all but `cur`
    int fb[4], nf = 0;
    for (int k = 0; k < 5; ++k) if (k != cur) fb[nf++] = k;
    T3 XU = view(fb[0], ch, Tout), T1 = view(fb[1], ch, Tout), YA = view(fb[2], ch, Tout), XS = view(fb[3], ch, Tout);
    a = r.args(U, X, XU, (int)Tn, (int)Tn + 1);
    a.in_act = 1; a.in_slope = 0.1f;
    a.T_store = (int)Tout;
    own_end(a, i);
    r.conv(a, B, true);
    for (int j = 0; j < nk; ++j) {
      const ResBlockW& rb = m.rbs[i * nk + j];
      const int nd = (int)rb.dil.size();
      if (rb.kind == 2) {
        // ResBlock2 (reference modules.py:245-249): x = x + conv_d(lrelu(x)) per convolution, ping-pong XU -> YA -> XS
        for (int d = 0; d < nd; ++d) {
          const bool last = d == nd - 1;
          const T3 yin = d == 0 ? XU : ((d & 1) ? YA : T1);
          const T3 yout = last ? XS : ((d & 1) ? T1 : YA);
          a = r.args(rb.c1[d], yin, yout, (int)Tout, (int)Tout);
          a.in_act = 1; a.in_slope = 0.1f;
          a.res = yin.p; a.r_bs = yin.bs; a.r_cs = yin.cs;
          if (last) {
            a.acc_prev = j > 0;
            if (j == nk - 1) a.div = (float)nk;
          }
          own_end(a, i + 1);
          r.conv(a, B, true);
        }
        continue;
      }
      for (int d = 0; d < nd; ++d) {
        const T3 yin = d == 0 ? XU : YA;
        a = r.args(rb.c1[d], yin, T1, (int)Tout, (int)Tout);
        a.in_act = 1; a.in_slope = 0.1f;
        own_end(a, i + 1);
        r.conv(a, B, true);
        const bool last = d == nd - 1;
        a = r.args(rb.c2[d], T1, last ? XS : YA, (int)Tout, (int)Tout);
        a.in_act = 1; a.in_slope = 0.1f;
        a.res = yin.p; a.r_bs = yin.bs; a.r_cs = yin.cs;
        if (last) {
          a.acc_prev = j > 0;
          if (j == nk - 1) a.div = (float)nk;
        }
        own_end(a, i + 1);
        r.conv(a, B, true);
      }
    }
    cur = fb[3];
    X = XS;
    Tn = Tout;
  }
  if (!r.dry() && r.ok()) {
    r.chk(launch_conv_post(X.p, X.bs, X.cs, r.A(m.post_w), m.post_c, m.post_k, 0.01f, o, Tn, B, (int)Tn, r.s, r.ctx->flags_dev,
                           iso ? stage_len + (size_t)c.n_upsamples * B : nullptr), "conv_post");
    if (iso) r.chk(launch_gen_tail_zero(o, Tn, in_lengths, B, T, (int)(Tn / T), r.s), "gen_tail_zero");
  }
}

// The context's two side streams and n fork / join events (created on first use, on the device the caller's stream
// belongs to; destroyed with the context).
bool ensure_side_streams(Run& r, size_t n_events) {
  vsp_ctx* ctx = r.ctx;
  // side[0]: the device's greatest stream priority, side[1]: its least (the caller's stream is assumed to sit between)
  int least = 0, greatest = 0;
  (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
  for (int k = 0; k < 2; ++k)
    if (!ctx->side[k] &&
        hipStreamCreateWithPriority(&ctx->side[k], hipStreamNonBlocking, k == 0 ? greatest : least) != hipSuccess) {
      ctx->side[k] = nullptr;
      return false;
    }
  while (ctx->sync_ev.size() < n_events) {
    hipEvent_t e;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventDisableSystemFence) != hipSuccess) return false;
    ctx->sync_ev.push_back(e);
  }
  return true;
}

// stages that run one launch per convolution (>= 128 channels) hand a ResBlock1 pair's intermediate over as an operand image
// (VSP_TIMG=0, the plain-f16 generator and ResBlock2: fp32 tensors)
bool cl_stage_img(const vsp_ctx& c, int ch) {
  return c.t_img && c.gen_mode == 1 && c.resblock == 1 && ch >= 128 && ch % 32 == 0;
}

// The launches that serve one ResBlock of a channels-last stage, decided from the context's switches (model.h) and the
// kernels' predicates before anything runs.  Every choice computes the same bits (tests/test_hip_parity.py:
// test_fused_resblock_paths_are_bit_identical); what each one launches is pinned by test_generator_schedule.
enum class RbLaunch {
  Fused,          // pairs [p0, p0 + np) of a ResBlock1, or a whole ResBlock2, in one launch: g16_chain / g16_rc, g16_rb2, g16_c16
  Pair,           // one ResBlock1 pair: g16_pair, which routes to g16_rw / g16_rw64 / g16_pp
  TwoConvs,       // one ResBlock1 pair as two g16_conv launches, fp32 intermediate
  TwoConvsImage,  // ... the intermediate as an operand image
  Conv            // one ResBlock2 convolution: g16_conv with the residual
};
struct RbUnit {
  RbLaunch kind;
  int p0, np;
};
struct RbPlan {
  int n = 0;
  RbUnit u[VSP_MAX_LIST];           // (a block has at most VSP_MAX_LIST dilations: vsp_config)
  void add(RbLaunch kind, int p0, int np) { u[n++] = RbUnit{kind, p0, np}; }
};
RbPlan plan_resblock(const vsp_ctx& c, const ResBlockW& rb, int ch) {
  RbPlan p;
  const int nd = (int)rb.dil.size(), terms = c.gen_mode == 2 ? 1 : 3;
  const int* dil = rb.dil.data();
  if (rb.kind == 2) {
    // ResBlock2 (reference modules.py:245-249): one fused launch on the 16/32/64-channel stages, else one g16_conv per
    // convolution with in_act + res.  VSP_RB2_FUSE=0: per convolution everywhere.
    const bool fused = c.rb2_fuse && nd == 2 && (ch == 16 ? g16_c16_rb2_supported(rb.k, dil) : g16_rb2_supported(ch, rb.k, dil));
    if (fused) p.add(RbLaunch::Fused, 0, 2);
    for (int d = 0; d < nd && !fused; ++d) p.add(RbLaunch::Conv, d, 1);
    return p;
  }
  // the 16-channel last stage (gen16_c16.hip): the whole ResBlock as one launch for every kernel size -- its cost is
  // traffic, not arithmetic; VSP_CHAIN=0 / VSP_FUSE_PAIRS=0, or a halo the block cannot hold: one launch per
  // convolution below (launch_g16_conv routes 16 -> 16 to the same kernel: bit-identical)
  if (ch == 16 && c.fuse_pairs && c.chain_mask && g16_c16_rb1_supported(rb.k, dil, nd)) {
    p.add(RbLaunch::Fused, 0, nd);
    return p;
  }
  bool fuse = c.fuse_pairs;
  for (int d = 0; d < nd; ++d)
    fuse = fuse && (g16_pair_supported(ch, rb.k, dil[d]) || (c.pp_pairs && g16_pp_supported(ch, rb.k, dil[d], terms)));
  const int kbit = rb.k <= 3 ? 1 : rb.k <= 7 ? 2 : 4;
  if (fuse && (c.chain_mask & kbit) && ch <= c.chain_ch && nd <= 3 && g16_chain_supported(ch, rb.k, dil, nd)) {
    p.add(RbLaunch::Fused, 0, nd);
    return p;
  }
  for (int d = 0; d < nd; ++d) {
    if (fuse) p.add(RbLaunch::Pair, d, 1);
    // 128-channel pair as ONE launch (g16_chain, 128-column blocks; VSP_CHAIN128): the intermediate never reaches HBM
    else if (ch == 128 && (c.chain128_mask & kbit) && g16_chain_supported(ch, rb.k, dil + d, 1)) p.add(RbLaunch::Fused, d, 1);
    else p.add(cl_stage_img(c, ch) && rb.k >= 3 ? RbLaunch::TwoConvsImage : RbLaunch::TwoConvs, d, 1);
  }
  return p;
}

// Generator.forward on the split-f16 channels-last kernels (gen16.hip): conv_pre stays on the
// f32 kernel (input z is channel-major and tiny), its output is transposed once to [B][T][C].
void run_generator_cl(Run& r, int B, int T, T3 z, const int64_t* in_lengths, const float* g, float* o) {
  const vsp_config& c = r.ctx->cfg;
  const Model& m = r.ctx->model;
  const int c0 = c.upsample_initial_channel, nk = c.n_resblock_kernels;
  float* gc = r.ws.f((size_t)B * c0);
  r.cond(m.g_cond, g, gc, B);
  T3 X0 = r.ws.t3(B, c0, T);
  const size_t mx = max_over_stages(c, T, (size_t)c0 * T, [](int ch, long t) { return (size_t)ch * (size_t)t; });
  float* buf[5];
  for (auto& bptr : buf) bptr = r.ws.f((size_t)B * mx);
  // ResBlocks 1 .. nk-1 of a stage on side streams (vsp_ctx::rb_streams): their own ping-pong tensors (and operand image)
  std::vector<float*> side_buf;
  if (r.ctx->rb_streams)
    for (int j = 1; j < nk; ++j)
      for (int u = 0; u < 2; ++u) side_buf.push_back(r.ws.f((size_t)B * mx));
  // the operand image of a ResBlock intermediate on the stages that hand one over (cl_stage_img)
  const size_t mx_img = max_over_stages(
      c, T, 0, [&](int ch, long t) { return cl_stage_img(*r.ctx, ch) ? cl_img_halfs(ch, (int)t) / 2 : (size_t)0; });
  const bool want_img = mx_img != 0;
  uint16_t* timg = want_img ? reinterpret_cast<uint16_t*>(r.ws.f((size_t)B * mx_img)) : nullptr;
  std::vector<uint16_t*> side_img;
  if (want_img && r.ctx->rb_streams)
    for (int j = 1; j < nk; ++j) side_img.push_back(reinterpret_cast<uint16_t*>(r.ws.f((size_t)B * mx_img)));
  // Trimmed tails (round 5; VSP_TRIM_TAILS=0: off, second implementation, bit-identical).  Behind an utterance's last frame
  // the input is exactly zero (z * x_mask, reference models.py:720), so the output there depends on the distance to the
  // utterance's end and to the tensor's end only: every kernel below treats utterance b's tensor as ENDING after
  // len_b + back + 1 + fwd frames (kernels.h, ClConvArgs::glen) -- frames [0, len + back) come out as in the padded run,
  // frame len + back is the steady state (periodic in one frame), the last fwd frames are the tensor end's -- and
  // gen_tail_fill writes the rest of the padded tensor from those.  The reference's full padded output, bit for bit.
  // (back / fwd: output frame F depends on input frames [F - back, F + fwd], sample-exact: 13 / 13 for configs/config.json.
  // A tensor that ends after E frames is exact up to frame E - 1 - fwd; frame len + back is the first steady one.)
  int back = 0, fwd = 0;
  generator_frame_dependence(c, r.ctx->resblock, m.g_pre.K, m.post_k, back, fwd);
  // Isolated mode (model.h): the same per-utterance extent with glen[b] = the utterance's own length -- its tensors END where
  // a B = 1 call's would, nothing behind the end is computed, and gen_tail_zero writes the padded rest of the waveform.
  // Neither of the tail fill's preconditions below applies to it.
  const bool iso = r.iso && in_lengths;
  // (the plan is part of the workspace whatever the context's switches: its size does not depend on the context's state)
  int* glen_all = reinterpret_cast<int*>(r.ws.bytes((size_t)B * sizeof(int)));
  // (gen_tail_fill keeps the computed tensor end -- fwd frames of the waveform -- in 64 KB of LDS: other configurations run untrimmed)
  bool trim = in_lengths && (iso || (r.ctx->trim_tails && T > back + fwd + 1 &&
                                                 (size_t)fwd * total_upsample(c) * sizeof(float) <= 64 * 1024));
  if (trim && r.host_lengths) {
    // the host knows the frame counts (vsp_frame_lengths_host of this batch): when no utterance ends early enough to be
    // trimmed (a uniform batch, one long utterance) the kernels run WITHOUT per-utterance extents -- same output, and
    // the persistent pipelined g16_convp serves the uniform tiles again
    bool any = false;
    for (int b = 0; b < B; ++b) any = any || std::max<int64_t>(r.host_lengths[b], 0) + (iso ? 0 : back + 1 + fwd) < T;
    trim = any;
  }
  if (trim && !r.dry() && r.ok())
    r.chk(iso ? launch_gen_plan_isolated(in_lengths, B, T, glen_all, r.s) : launch_gen_plan(in_lengths, B, T, back, fwd, glen_all, r.s),
          "gen_plan");
  // profiled (untimed) passes charge every launch the frames it COMPUTES: read the plan back (a host wait -- profiling only)
  std::vector<int> glen_host;
  if (trim && r.ctx->prof_on && !r.dry() && r.ok()) {
    glen_host.resize(B);
    hipError_t e = hipMemcpyAsync(glen_host.data(), glen_all, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, r.s);
    if (e == hipSuccess) e = hipStreamSynchronize(r.s);
    r.chk(e, "gen_plan read-back (profiling)");
  }
  // the channels-last kernels address one utterance's tensor with 32-bit byte offsets (buffer descriptors)
  // (the operand images -- C * 4 * (T + 384) bytes per utterance -- are addressed the same way)
  if (mx * sizeof(float) >= (size_t)1 << 31 || (timg && mx_img * sizeof(float) >= (size_t)1 << 31)) {
    if (r.rc == VSP_OK)
      r.rc = r.ctx->fail(VSP_ERR_UNSUPPORTED, "generator: %d frames per call exceed the 2 GiB per-utterance activation "
                                              "limit; synthesise in chunks (Engine.generator_stream)", T);
    return;
  }
  ConvArgs a = r.args(m.g_pre, z, X0, T, T);
  a.lengths = in_lengths; a.in_mask = in_lengths ? 1 : 0;
  a.cond = gc; a.cond_bs = c0;
  r.conv(a, B, true);
  int cur = 0;
  if (!r.dry() && r.ok())
    r.chk(launch_transpose_ct(X0.p, X0.bs, X0.cs, buf[cur], (long)T * c0, c0, B, c0, T, r.s, r.ctx->act_scale), "transpose");
  long Tn = T;
  int ch = c0;
  for (int i = 0; i < c.n_upsamples; ++i) {
    const ClConv& U = m.ups_h[i];
    const long Tout = Tn * U.phases;
    const int cin = ch;
    ch = c0 >> (i + 1);
    int fb[4], nf = 0;
    for (int k = 0; k < 5; ++k) if (k != cur) fb[nf++] = k;
    float *XU = buf[fb[0]], *T1 = buf[fb[1]], *YA = buf[fb[2]], *XS = buf[fb[3]];
    const long bs = Tout * ch, xbs = Tn * cin;
    // Optional cache blocking over the batch (VSP_CHUNK_MB, default off): a stage runs chunk by chunk
    // so that the tensors two consecutive launches exchange are <= chunk_mb and could be served by the
    // 256 MiB Infinity Cache.  Measured on MI355X (profiles/r01_tile_experiments.txt): 32-192 MiB
    // chunks are 3-10 % SLOWER than whole-batch launches (more launches and tails, no shorter kernels),
    // so the product runs whole-batch; the knob stays for experiments.
    int Bc = B;
    if (r.ctx->chunk_mb > 0) {
      const double per_utt_mb = (double)bs * 4.0 / (1024.0 * 1024.0);
      Bc = (int)std::max(1.0, std::floor(r.ctx->chunk_mb / per_utt_mb));
      const long tiles_per_utt = (Tout + 255) / 256 * std::max(1, ch / 128);
      const int min_b = (int)((2 * 256 * (ch >= 128 ? 1 : 2) + tiles_per_utt - 1) / tiles_per_utt);
      Bc = std::min(B, std::max(Bc, min_b));
    }
    for (int b0 = 0; b0 < B; b0 += Bc) {
      const int nb = std::min(Bc, B - b0);
      r.glen = trim ? glen_all + b0 : nullptr;
      r.grate_in = (int)(Tn / T); r.grate_out = (int)(Tout / T);
      r.work_frac = 1.0;
      if (!glen_host.empty() && r.ok()) {
        double fr = 0.0;
        for (int b = b0; b < b0 + nb; ++b) fr += glen_host[b];
        r.work_frac = fr / ((double)nb * T);
      }
      const float* xin = buf[cur] + (size_t)b0 * xbs;
      float *xu = XU + (size_t)b0 * bs, *xs = XS + (size_t)b0 * bs;
      r.clconv(U, xin, xu, nullptr, (int)Tn, false, 1.f, nb);
      // The stage's ResBlocks are independent chains until their sum (reference models.py:276-285): chain 0 runs on the
      // caller's stream, chains 1 .. on the context's side streams with their own intermediates, forked after the
      // up-convolution; a chain's LAST launch accumulates into xs and therefore waits for the previous chain's last
      // launch (the reference's order of the sum, bit for bit), the caller's stream joins after the last chain.
      const bool conc = ((r.ctx->rb_streams >> i) & 1) && !r.ctx->prof_on && !r.dry() && r.ok() && Bc == B && nk > 1 &&
                        (int)side_buf.size() == 2 * (nk - 1) && ensure_side_streams(r, (size_t)c.n_upsamples * (nk + 1));
      hipStream_t const main_s = r.s;
      hipEvent_t* const ev = conc ? r.ctx->sync_ev.data() + (size_t)i * (nk + 1) : nullptr;   // [0] fork, [1 + j] chain j's last launch
      const bool use_img = timg && cl_stage_img(*r.ctx, ch);
      auto chain_img = [&](int j) -> uint16_t* {
        if (!use_img) return nullptr;
        uint16_t* base = (conc && j != 1 && (int)side_img.size() == nk - 1) ? side_img[j == 0 ? 0 : j - 1] : timg;
        return base + (size_t)b0 * cl_img_halfs(ch, (int)Tout);
      };
      if (use_img && !r.dry() && r.ok())
        for (int j = (conc && !side_img.empty()) ? 0 : 1; j < ((conc && !side_img.empty()) ? nk : 2); ++j)
          r.chk(launch_cl_img_zero_pads(chain_img(j), nb, ch, (int)Tout, r.s, r.glen, r.grate_out), "cl_img_zero_pads");
      if (conc) r.chk(hipEventRecord(ev[0], main_s), "fork event");
      for (int j = 0; j < nk; ++j) {
        const ResBlockW& rb = m.rbs[i * nk + j];
        // chain j's stream and intermediates: chain 0 on the high-priority side stream, chain 1 on the caller's, the rest
        // on the low-priority one -- the hardware then dispatches a chain's blocks into the slots the chains before it
        // leave free (ramps, partial last rounds) instead of sharing the CUs launch by launch in lockstep, and a chain's
        // last launch finds the previous chain's long finished
        float *t1 = T1 + (size_t)b0 * bs, *ya = YA + (size_t)b0 * bs;
        const int side_set = j == 0 ? 0 : j - 1;           // (chain 1 keeps the caller-stream tensors)
        if (conc && j != 1) {
          r.s = r.ctx->side[j == 0 ? 0 : 1];
          t1 = side_buf[2 * side_set] + (size_t)b0 * bs;
          ya = side_buf[2 * side_set + 1] + (size_t)b0 * bs;
          r.chk(hipStreamWaitEvent(r.s, ev[0], 0), "fork wait");
        }
        uint16_t* const ti = chain_img(j);
        // The block's launches in order (plan_resblock).  A launch reads the running tensor from `yin` and writes it to
        // another buffer (a tile reads halo rows that a neighbour writes) -- ping-pong between ya and t1; the two-launch
        // pair updates it in place (in ya from the first pair on), with the other of the two or the image as its intermediate.
        // The block's last launch adds its result to the stage's sum in xs (and the stage's last block divides by nk: the
        // reference's order of the sum).
        const RbPlan plan = plan_resblock(*r.ctx, rb, ch);
        const float* yin = xu;
        for (int k = 0; k < plan.n; ++k) {
          const RbUnit& u = plan.u[k];
          const bool last = k == plan.n - 1, acc = last && j > 0;
          const bool two = u.kind == RbLaunch::TwoConvs || u.kind == RbLaunch::TwoConvsImage;
          const float div = (last && j == nk - 1) ? (float)nk : 1.f;
          float* const mid = yin == t1 ? ya : t1;
          float* const yout = last ? xs : two ? (yin == xu ? ya : const_cast<float*>(yin)) : (yin == ya ? t1 : ya);
          uint16_t* const img = u.kind == RbLaunch::TwoConvsImage ? ti : nullptr;
          if (two) r.clconv(rb.h1[u.p0], yin, img ? nullptr : mid, nullptr, (int)Tout, false, 1.f, nb, nullptr, img);
          if (last && conc && j > 0) r.chk(hipStreamWaitEvent(r.s, ev[j], 0), "sum order wait");
          if (two) r.clconv(rb.h2[u.p0], mid, yout, yin, (int)Tout, acc, div, nb, img, nullptr);
          else if (u.kind == RbLaunch::Conv) r.clconv(rb.h1[u.p0], yin, yout, yin, (int)Tout, acc, div, nb);
          else r.clfused(rb, ch, u.p0, u.np, u.kind == RbLaunch::Pair, yin, yout, (int)Tout, acc, div, nb);
          yin = yout;
        }
        if (conc) r.chk(hipEventRecord(ev[1 + j], r.s), "chain end event");
        r.s = main_s;
      }
      if (conc) r.chk(hipStreamWaitEvent(main_s, ev[nk], 0), "join wait");
    }
    cur = fb[3];
    Tn = Tout;
  }
  r.glen = nullptr;
  r.work_frac = 1.0;
  if (!r.dry() && r.ok()) {
    r.chk(launch_conv_post_cl(buf[cur], Tn * ch, ch, r.A(m.post_wt), m.post_c, m.post_k, 0.01f, o, Tn, B, (int)Tn, r.s,
                              trim ? glen_all : nullptr, (int)(Tn / T), 1.f / r.ctx->act_scale, r.ctx->flags_dev), "conv_post_cl");
    if (trim && iso) r.chk(launch_gen_tail_zero(o, Tn, in_lengths, B, T, (int)(Tn / T), r.s), "gen_tail_zero");
    else if (trim) r.chk(launch_gen_tail_fill(o, Tn, in_lengths, glen_all, B, T, back, fwd, (int)(Tn / T), r.s), "gen_tail_fill");
  }
}

void run_gen(Run& r, int B, int T, T3 z, const int64_t* in_lengths, const float* g, float* o) {
  if (r.ctx->gen_mode >= 1 && r.ctx->model.has_cl) run_generator_cl(r, B, T, z, in_lengths, g, o);
  else run_generator(r, B, T, z, in_lengths, g, o);
}

int check_ready(vsp_ctx* ctx) {
  if (!ctx) return VSP_ERR_ARG;
  if (!ctx->ready) return ctx->fail(VSP_ERR_STATE, "weights not finalised");
  return VSP_OK;
}

// One-sided support of ResBlock j of a stage, in samples at the stage's rate: ResBlock1 (reference modules.py:210-223)
// sum over its dilations of (k - 1) d / 2 + (k - 1) / 2 (a dilated and an undilated convolution per step); ResBlock2
// (modules.py:245-249) (k - 1) d / 2 for dilation[0] and dilation[1] only (one convolution per step, the rest unused).
long resblock_support(const vsp_config& c, int resblock, int j) {
  const long kk = c.resblock_kernel_sizes[j];
  long acc = 0;
  if (resblock == 2) {
    for (int d = 0; d < 2 && d < c.n_resblock_dilations; ++d) acc += (kk - 1) * c.resblock_dilation_sizes[j][d] / 2;
    return acc;
  }
  for (int d = 0; d < c.n_resblock_dilations; ++d) acc += (kk - 1) * c.resblock_dilation_sizes[j][d] / 2 + (kk - 1) / 2;
  return acc;
}

// Exact dependence of the generator's output FRAMES on its input frames, from the configuration (sample-exact supports;
// vsp_generator_halo_frames below is the coarser per-stage bound the streamed vocoder uses): output frame F depends on
// input frames [F - back, F + fwd].  An impulse at input position 0 reaches output samples [lo, hi]: conv_pre widens the
// support by its padding, a transposed convolution (k, s, p) maps [lo, hi] to [lo s - p, hi s - p + k - 1], a stage's
// ResBlocks widen it by max_k of the block's support (resblock_support), conv_post by its padding.
void generator_frame_dependence(const vsp_config& c, int resblock, int pre_k, int post_k, int& back, int& fwd) {
  long lo = -(pre_k - 1) / 2, hi = (pre_k - 1) / 2, up = 1;
  for (int i = 0; i < c.n_upsamples; ++i) {
    const long s = c.upsample_rates[i], k = c.upsample_kernel_sizes[i], p = (k - s) / 2;
    lo = lo * s - p; hi = hi * s - p + k - 1; up *= s;
    long rb = 0;
    for (int j = 0; j < c.n_resblock_kernels; ++j) rb = std::max(rb, resblock_support(c, resblock, j));
    lo -= rb; hi += rb;
  }
  lo -= (post_k - 1) / 2; hi += (post_k - 1) / 2;
  // output frame F = samples [up F, up F + up - 1] depends on input frames f with up f + lo <= n <= up f + hi
  back = (int)(hi / up);                     // F - floor(hi / up)
  fwd = (int)((up - 1 - lo) / up);           // F + floor((up - 1 - lo) / up)
}

long total_upsample(const vsp_config& c) {
  long u = 1;
  for (int i = 0; i < c.n_upsamples; ++i) u *= c.upsample_rates[i];
  return u;
}

}  // namespace

// ============================================================================================
extern "C" {

int vsp_abi_version(void) { return VSP_ABI_VERSION; }

int vsp_create(const vsp_config* cfg, int device, vsp_ctx** out) { return vsp_create_ex(cfg, 1, device, out); }

int vsp_create_ex(const vsp_config* cfg, int32_t resblock, int device, vsp_ctx** out) {
  if (!cfg || !out || (resblock != 1 && resblock != 2)) return VSP_ERR_ARG;
  vsp_ctx* ctx = new (std::nothrow) vsp_ctx();
  if (!ctx) return VSP_ERR_ARG;
  ctx->cfg = *cfg;
  ctx->resblock = resblock;
  ctx->device = device;
  // Second implementations kept under test (tests/test_hip_parity.py): VSP_FRAME=f32 / VSP_ATT=f32 / VSP_GENERATOR=f32
  // (f32 matrix core), VSP_FUSE_PAIRS=0 (one launch per convolution), VSP_CHAIN=<mask> (whole-ResBlock launches:
  // bit 0 = k3, 1 = k7, 2 = k11), and the opt-in reduced precision VSP_GENERATOR=f16.  Everything else that was a
  // knob while the kernels were being tuned is compiled out of the product build (-DVSP_EXPERIMENTS brings it back).
  if (const char* e = getenv("VSP_FRAME")) ctx->frame_f16s = strcmp(e, "f32") != 0;
  if (const char* e = getenv("VSP_ATT")) ctx->att_f16s = strcmp(e, "f32") != 0;
  // the generator mode is part of the plan (conv_pre / cond packing): parse it BEFORE plan_model
  bool want_f16 = false;
  if (const char* e = getenv("VSP_GENERATOR")) {
    if (!strcmp(e, "f32")) ctx->gen_mode = 0;
    want_f16 = !strcmp(e, "f16");
  }
  if (const char* e = getenv("VSP_FUSE_PAIRS")) ctx->fuse_pairs = atoi(e) != 0;
  if (const char* e = getenv("VSP_RB2_FUSE")) ctx->rb2_fuse = atoi(e) != 0;      // 0: ResBlock2 one launch per convolution (second implementation)
  if (const char* e = getenv("VSP_TIMG")) ctx->t_img = atoi(e) != 0;   // 0: ResBlock intermediates as fp32 tensors (second implementation)
  if (const char* e = getenv("VSP_PP")) ctx->pp_pairs = atoi(e) != 0;  // 0: the 128-channel stage's k3 / k7 pairs as two launches
  if (const char* e = getenv("VSP_PAIR")) ctx->pair_ring = !strcmp(e, "ring");
  if (const char* e = getenv("VSP_CHAIN_RING")) ctx->chain_ring = atoi(e) != 0;
  if (const char* e = getenv("VSP_CHAIN")) ctx->chain_mask = atoi(e);
  if (const char* e = getenv("VSP_RW64")) ctx->rw64 = atoi(e) != 0;               // 1: g16_rw64 for the 64-channel k3 pairs (opt-in)
  if (const char* e = getenv("VSP_TRIM_TAILS")) ctx->trim_tails = atoi(e) != 0;   // 0: every utterance runs to the padded length
  if (const char* e = getenv("VSP_COLS")) ctx->cols = atoi(e) != 0;               // 0: no column-tile kernels (second implementation)
  if (const char* e = getenv("VSP_COLS_BLOCKS")) ctx->cols_blocks = atol(e);      // size limits of launch_conv's routing to them
  if (const char* e = getenv("VSP_COLS_MIN_BLOCKS")) ctx->cols_min_blocks = atol(e);
  if (const char* e = getenv("VSP_ACT_SCALE_LOG2")) {                             // model.h: the generator's activation scale
    const int l = atoi(e);
    ctx->act_scale = std::ldexp(1.f, l < 0 ? 0 : l > 8 ? 8 : l);
  }
  if (const char* e = getenv("VSP_EARLY_FL")) ctx->early_fl = atoi(e) != 0;
  if (const char* e = getenv("VSP_RB_STREAMS")) ctx->rb_streams = atoi(e);   // stage mask: ResBlock chains on side streams (opt-in, measured slower)
#ifdef VSP_EXPERIMENTS
  if (const char* e = getenv("VSP_ATT_KSPLIT")) ctx->att_ksplit = atoi(e);
  if (const char* e = getenv("VSP_CHUNK_MB")) ctx->chunk_mb = atof(e);
  if (const char* e = getenv("VSP_CHAIN_CH")) ctx->chain_ch = atoi(e);
  if (const char* e = getenv("VSP_CHAIN128")) ctx->chain128_mask = atoi(e);
#endif
  build_schema(ctx->cfg, ctx->schema, ctx->resblock);
  const int rc = plan_model(ctx);            // (falls back to gen_mode 0 when the channels-last kernels do not cover the config)
  if (want_f16 && ctx->gen_mode == 1) ctx->gen_mode = 2;   // opt-in reduced precision: same packing as mode 1
  *out = ctx;  // returned even on failure so that vsp_last_error can be read; caller destroys it
  return rc;
}

int vsp_destroy(vsp_ctx* ctx) {
  if (!ctx) return VSP_ERR_ARG;
  for (auto e : ctx->ev_pool) (void)hipEventDestroy(e);
  for (auto e : ctx->sync_ev) (void)hipEventDestroy(e);
  if (ctx->fl_ev) (void)hipEventDestroy(ctx->fl_ev);
  if (ctx->fl_pinned) (void)hipHostFree(ctx->fl_pinned);
  if (ctx->flags_host) (void)hipHostFree(ctx->flags_host);
  for (auto st : ctx->side) if (st) (void)hipStreamDestroy(st);
  if (ctx->arena && ctx->arena_owned) (void)hipFree(ctx->arena);
  if (ctx->out_tab) (void)hipFree(ctx->out_tab);
  delete ctx;
  return VSP_OK;
}

const char* vsp_last_error(const vsp_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int vsp_status(vsp_ctx* ctx, unsigned* flags, int clear) {
  if (!ctx || !flags) return VSP_ERR_ARG;
  *flags = 0u;
  if (!ctx->flags_host) return VSP_OK;                 // (nothing has run on this context yet)
  volatile unsigned* w = ctx->flags_host;
  *flags = clear ? __atomic_exchange_n(ctx->flags_host, 0u, __ATOMIC_ACQ_REL) : *w;
  return VSP_OK;
}

int vsp_begin_weights(vsp_ctx* ctx) {
  if (!ctx) return VSP_ERR_ARG;
  ctx->raw.clear();
  ctx->ready = false;
  ctx->adopted_pending = false;
  return VSP_OK;
}

int vsp_set_weight(vsp_ctx* ctx, const char* key, const float* host_data, const int64_t* shape, int ndim) {
  if (!ctx || !key || !host_data || !shape || ndim < 0 || ndim > 8) return ctx ? ctx->fail(VSP_ERR_ARG, "null argument") : VSP_ERR_ARG;
  const std::string k(key);
  // posterior encoder: voice conversion only; ignored by a context built without spec_channels
  if (k.rfind("enc_q.", 0) == 0 && ctx->cfg.spec_channels <= 0) return VSP_OK;
  auto it = ctx->schema.find(k);
  bool folded_form = false;
  if (it == ctx->schema.end()) {
    // accept a pre-folded "<x>.weight" where the schema has "<x>.weight_v" (remove_weight_norm'ed checkpoint)
    auto iv = ctx->schema.find(k + "_v");
    if (iv == ctx->schema.end()) return ctx->fail(VSP_ERR_KEY, "unknown state_dict key '%s'", key);
    it = iv;
    folded_form = true;
  }
  const SchemaEntry& e = it->second;
  bool same = (int)e.shape.size() == ndim;
  for (int i = 0; same && i < ndim; ++i) same = e.shape[i] == shape[i];
  if (!same) return ctx->fail(VSP_ERR_SHAPE, "shape mismatch for '%s'", key);
  if (!e.used) return VSP_OK;
  HostTensor t;
  t.shape.assign(shape, shape + ndim);
  t.data.assign(host_data, host_data + t.numel());
  // one form per layer: a folded "<x>.weight" replaces an earlier weight_g / weight_v pair and vice versa (a second
  // load on the same context must not keep the other form's tensors)
  if (folded_form) {
    ctx->raw.erase(k + "_v");
    ctx->raw.erase(k + "_g");
  } else if (k.size() > 9 && (k.compare(k.size() - 9, 9, ".weight_v") == 0 || k.compare(k.size() - 9, 9, ".weight_g") == 0)) {
    ctx->raw.erase(k.substr(0, k.size() - 2));
  }
  ctx->raw[k] = std::move(t);
  ctx->ready = false;
  return VSP_OK;
}

// f16 / bf16 bit patterns -> float (host)
static float half_bits_to_float(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, exp = (h >> 10) & 0x1fu, man = h & 0x3ffu;
  uint32_t bits;
  if (exp == 0) {
    if (man == 0) bits = sign;
    else {  // subnormal
      int e = -1;
      uint32_t m = man;
      do { ++e; m <<= 1; } while (!(m & 0x400u));
      bits = sign | ((uint32_t)(127 - 15 - e) << 23) | ((m & 0x3ffu) << 13);
    }
  } else if (exp == 31) bits = sign | 0x7f800000u | (man << 13);
  else bits = sign | ((exp + 112u) << 23) | (man << 13);
  float f;
  std::memcpy(&f, &bits, 4);
  return f;
}

int vsp_set_weight_typed(vsp_ctx* ctx, const char* key, const void* data, const int64_t* shape, int ndim, int dtype,
                         int on_device) {
  if (!ctx || !key || !data || !shape || ndim < 0 || ndim > 8) return ctx ? ctx->fail(VSP_ERR_ARG, "null argument") : VSP_ERR_ARG;
  size_t n = 1;
  for (int i = 0; i < ndim; ++i) {
    if (shape[i] < 0) return ctx->fail(VSP_ERR_ARG, "negative dimension");
    n *= (size_t)shape[i];
  }
  size_t esz = 0;
  switch (dtype) {
    case VSP_DTYPE_F32: esz = 4; break;
    case VSP_DTYPE_F16: case VSP_DTYPE_BF16: esz = 2; break;
    case VSP_DTYPE_F64: esz = 8; break;
    default: return ctx->fail(VSP_ERR_ARG, "vsp_set_weight_typed: unknown dtype %d", dtype);
  }
  std::vector<unsigned char> staged;
  const unsigned char* src = static_cast<const unsigned char*>(data);
  if (on_device) {
    staged.resize(n * esz);
    hipError_t e = hipMemcpy(staged.data(), data, n * esz, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return ctx->fail(VSP_ERR_HIP, "vsp_set_weight_typed(%s): %s", key, hipGetErrorString(e));
    src = staged.data();
  }
  if (dtype == VSP_DTYPE_F32) return vsp_set_weight(ctx, key, reinterpret_cast<const float*>(src), shape, ndim);
  std::vector<float> f(n);
  for (size_t i = 0; i < n; ++i) {
    if (dtype == VSP_DTYPE_F64) { double d; std::memcpy(&d, src + 8 * i, 8); f[i] = (float)d; }
    else {
      uint16_t h; std::memcpy(&h, src + 2 * i, 2);
      if (dtype == VSP_DTYPE_BF16) { const uint32_t b = (uint32_t)h << 16; std::memcpy(&f[i], &b, 4); }
      else f[i] = half_bits_to_float(h);
    }
  }
  return vsp_set_weight(ctx, key, f.data(), shape, ndim);
}

int vsp_missing_weights(const vsp_ctx* ctx) {
  if (!ctx) return VSP_ERR_ARG;
  int n = 0;
  for (const auto& kv : ctx->schema) {
    if (!kv.second.used || kv.second.optional) continue;
    if (ctx->raw.count(kv.first)) continue;
    const std::string& k = kv.first;
    // weight_g / weight_v are satisfied by a pre-folded weight
    if (k.size() > 2 && (k.compare(k.size() - 2, 2, "_v") == 0 || k.compare(k.size() - 2, 2, "_g") == 0) &&
        ctx->raw.count(k.substr(0, k.size() - 2)))
      continue;
    ++n;
  }
  return n;
}

int64_t vsp_weight_arena_bytes(const vsp_ctx* ctx) {
  return ctx ? (int64_t)(ctx->model.total_floats * sizeof(float)) : VSP_ERR_ARG;
}

// The status word (vsp_status): pinned host memory mapped into the device's address space, so that reading it costs no
// stream synchronisation; the kernels touch it only when they have something to report.
static int ensure_flags(vsp_ctx* ctx) {
  if (ctx->flags_host) return VSP_OK;
  void* h = nullptr;
  void* d = nullptr;
  hipError_t e = hipHostMalloc(&h, 64, hipHostMallocMapped | hipHostMallocPortable);
  if (e == hipSuccess) { *static_cast<unsigned*>(h) = 0u; e = hipHostGetDevicePointer(&d, h, 0); }
  if (e != hipSuccess) {
    if (h) (void)hipHostFree(h);
    return ctx->fail(VSP_ERR_HIP, "status word (hipHostMalloc): %s", hipGetErrorString(e));
  }
  ctx->flags_host = static_cast<unsigned*>(h);
  ctx->flags_dev = static_cast<unsigned*>(d);
  return VSP_OK;
}

static int set_arena(vsp_ctx* ctx, void* dev_arena) {
  if (int rc = ensure_flags(ctx)) return rc;
  if (ctx->arena && ctx->arena_owned && ctx->arena != dev_arena) (void)hipFree(ctx->arena);
  if (dev_arena) {
    ctx->arena = (float*)dev_arena;
    ctx->arena_owned = false;
  } else if (!ctx->arena || !ctx->arena_owned) {
    void* p = nullptr;
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipMalloc(&p, ctx->model.total_floats * sizeof(float));
    if (e != hipSuccess) return ctx->fail(VSP_ERR_HIP, "hipMalloc(weight arena): %s", hipGetErrorString(e));
    ctx->arena = (float*)p;
    ctx->arena_owned = true;
  }
  return VSP_OK;
}

static uint32_t config_hash(const vsp_ctx* ctx) {
  // FNV-1a over the config bytes and the switches that change the packing
  uint32_t h = 2166136261u;
  auto mix = [&](const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 16777619u; }
  };
  mix(&ctx->cfg, sizeof ctx->cfg);
  const int sw[3] = {ctx->frame_f16s ? 1 : 0, ctx->model.has_cl ? 1 : 0, ctx->gen_mode != 0 ? 1 : 0};
  mix(sw, sizeof sw);
  mix(&ctx->act_scale, sizeof ctx->act_scale);   // (the packed generator biases carry it)
  if (ctx->resblock == 2) mix(&ctx->resblock, sizeof ctx->resblock);   // (ResBlock1 arenas hash as they always did)
  return h;
}

int vsp_finalize_weights(vsp_ctx* ctx, void* dev_arena) {
  if (!ctx) return VSP_ERR_ARG;
  if (ctx->model.total_floats == 0) return ctx->fail(VSP_ERR_STATE, "context was not planned (vsp_create failed)");
  const int miss = vsp_missing_weights(ctx);
  if (miss) return ctx->fail(VSP_ERR_STATE, "%d infer-path tensors missing", miss);
  std::vector<float> host;
  int rc = fill_model(ctx, host);
  if (rc) return rc;
  {
    const uint64_t tf = ctx->model.total_floats;
    const uint32_t hdr[6] = {ARENA_MAGIC, (uint32_t)VSP_ABI_VERSION, (uint32_t)(tf & 0xffffffffu), (uint32_t)(tf >> 32),
                             ctx->model.has_vc ? ARENA_FLAG_VC : 0u, config_hash(ctx)};
    std::memcpy(host.data(), hdr, sizeof hdr);
  }
  rc = set_arena(ctx, dev_arena);
  if (rc) return rc;
  hipError_t e = hipMemcpy(ctx->arena, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) return ctx->fail(VSP_ERR_HIP, "hipMemcpy(weight arena): %s", hipGetErrorString(e));
  ctx->adopted_pending = false;
  ctx->ready = true;
  return VSP_OK;
}

int vsp_adopt_packed_weights(vsp_ctx* ctx, void* dev_arena) {
  if (!ctx || !dev_arena) return ctx ? ctx->fail(VSP_ERR_ARG, "null arena") : VSP_ERR_ARG;
  if (ctx->model.total_floats == 0) return ctx->fail(VSP_ERR_STATE, "context was not planned");
  const int rc = set_arena(ctx, dev_arena);
  if (rc) return rc;
  // the bytes may not have arrived yet (the broadcast follows): nothing is known about them until
  // vsp_commit_adopted_weights has read the header -- fail closed until then
  ctx->model.has_vc = false;
  ctx->ready = false;
  ctx->adopted_pending = true;
  return VSP_OK;
}

int vsp_commit_adopted_weights(vsp_ctx* ctx, void* stream) {
  if (!ctx) return VSP_ERR_ARG;
  if (!ctx->adopted_pending || !ctx->arena) return ctx->fail(VSP_ERR_STATE, "no adopted arena to commit");
  uint32_t hdr[6] = {0, 0, 0, 0, 0, 0};
  hipError_t e = hipMemcpyAsync(hdr, ctx->arena, sizeof hdr, hipMemcpyDeviceToHost, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  if (e != hipSuccess) return ctx->fail(VSP_ERR_HIP, "arena header read: %s", hipGetErrorString(e));
  const uint64_t tf = (uint64_t)hdr[2] | ((uint64_t)hdr[3] << 32);
  if (hdr[0] != ARENA_MAGIC) return ctx->fail(VSP_ERR_STATE, "adopted arena has no header (bytes not broadcast yet, or not a packed arena)");
  if (hdr[1] != (uint32_t)VSP_ABI_VERSION) return ctx->fail(VSP_ERR_STATE, "adopted arena was packed by ABI %u, this library is ABI %d", hdr[1], VSP_ABI_VERSION);
  if (tf != ctx->model.total_floats || hdr[5] != config_hash(ctx))
    return ctx->fail(VSP_ERR_STATE, "adopted arena was packed for a different configuration");
  ctx->model.has_vc = (hdr[4] & ARENA_FLAG_VC) != 0;
  ctx->adopted_pending = false;
  ctx->ready = true;
  return VSP_OK;
}

int vsp_has_voice_conversion(const vsp_ctx* ctx) { return ctx && ctx->ready && ctx->model.has_vc ? 1 : 0; }

int vsp_weight_arena(const vsp_ctx* ctx, void** dev_arena, int64_t* bytes) {
  if (!ctx || !dev_arena || !bytes) return VSP_ERR_ARG;
  *dev_arena = ctx->arena;
  *bytes = (int64_t)(ctx->model.total_floats * sizeof(float));
  return VSP_OK;
}

// -------------------------------------------------------------------------------------------- encode
// pinned host buffer + event of the early frame-count copy (created on first use, grown by doubling; kept with the context)
static bool early_frame_lengths_ready(vsp_ctx* ctx, int B) {
  if (!ctx->fl_ev && hipEventCreateWithFlags(&ctx->fl_ev, hipEventDisableTiming) != hipSuccess) {
    ctx->fl_ev = nullptr;
    return false;
  }
  if (ctx->fl_cap < B) {
    if (ctx->fl_pinned) (void)hipHostFree(ctx->fl_pinned);
    ctx->fl_pinned = nullptr;
    int cap = std::max(64, ctx->fl_cap);
    while (cap < B) cap *= 2;
    if (hipHostMalloc(reinterpret_cast<void**>(&ctx->fl_pinned), (size_t)cap * sizeof(int64_t), hipHostMallocDefault) != hipSuccess) {
      ctx->fl_pinned = nullptr;
      ctx->fl_cap = 0;
      return false;
    }
    ctx->fl_cap = cap;
  }
  return true;
}

static int encode_impl(vsp_ctx* ctx, hipStream_t s, Ws& ws, int B, int Tp, const int64_t* phonemes,
                       const int64_t* lengths, const int64_t* sid, const float* dctl, const float* pctl,
                       const float* ectl, float dscale, float pscale, float escale, float* x_var, float* g,
                       float* duration, float* f0, float* energy, int64_t* frame_lengths, int32_t* cum_dur,
                       bool early_copy = true) {
  const vsp_config& c = ctx->cfg;
  const Model& m = ctx->model;
  const int h = c.hidden_channels, gin = c.gin_channels;
  Run r{ctx, s, ws};
  // Isolated mode (model.h): the controls are read at t < lengths[b] only, the signals the two prenets convolve are zero
  // behind an utterance's end (what a B = 1 call's zero padding is), the EnergyPredictor masks like the duration
  // predictor, and every output is zero behind its extent.
  const bool iso = ctx->isolated;
  // Per-row controls (vsp_set_row_controls; the entry points have checked B, the mode and the *_ctl pointers): a control's
  // given path runs alone iff EVERY row has it, its predictor runs iff some row lacks it, and the per-row kernels select
  // the source and the scale by row.  No table: the *_ctl pointers decide for the whole batch, as they always did.
  const std::vector<vsp_row_control>& rows = ctx->row_controls;
  const bool per_row = !rows.empty() && !ws.dry;   // (sizing: the largest launch set, whatever the context holds)
  auto all_given = [&](uint32_t bit, const float* ctl) {
    if (!per_row) return ctl != nullptr;
    return std::all_of(rows.begin(), rows.end(), [bit](const vsp_row_control& r) { return (r.given & bit) != 0; });
  };
  const bool dur_given = all_given(VSP_GIVEN_DURATION, dctl), pit_given = all_given(VSP_GIVEN_PITCH, pctl),
             en_given = all_given(VSP_GIVEN_ENERGY, ectl);
  const T3 XV = ext(x_var, h, Tp);
  T3 XE = ws.t3(B, h, Tp), TMP = ws.t3(B, h, Tp);
  float* cvec = ws.f((size_t)B * h);
  float* lf0 = ws.f((size_t)B * Tp);
  float* pred = ws.f((size_t)B * Tp);
  float* norm_e = ws.f((size_t)B * Tp);
  // duration-predictor / energy-predictor activations
  const int fmax_ = std::max(c.dur_filter, c.energy_filter);
  T3 P1 = ws.t3(B, fmax_, Tp), P2 = ws.t3(B, fmax_, Tp);
  // the row table of THIS call (counted in every state: workspace sizes do not depend on context state)
  vsp_row_control* rows_dev = reinterpret_cast<vsp_row_control*>(ws.bytes((size_t)B * sizeof(vsp_row_control)));
  const bool live = !ws.dry && !ws.overflow;
  // (pageable source, like the noise seeds of vsp_decode: staged before this call returns, so a later
  // vsp_set_row_controls may replace the vector while the copy is still queued)
  if (live && per_row)
    r.chk(hipMemcpyAsync(rows_dev, rows.data(), (size_t)B * sizeof(vsp_row_control), hipMemcpyHostToDevice, s), "row controls");
  if (live) {
    r.chk(launch_gather_rows(sid, r.A(m.emb_g), c.n_speakers, g, B, gin, s), "emb_g");
    r.chk(launch_embed(phonemes, r.A(m.emb_sym), c.n_vocab, sqrtf((float)h), XE.p, XE.bs, XE.cs, B, h, Tp, s),
          "symbol_emb");
  }
  // ---- given durations (models.py:681): the frame counts need nothing computed here -- derive them FIRST and start their
  // copy to the host, so that vsp_frame_lengths_host returns while the text encoder runs (vsp_ctx::fl_pinned)
  if (live) { ctx->fl_src = nullptr; ctx->fl_known_src = nullptr; }
  if (dur_given && live) {
    r.chk(hipMemcpyAsync(duration, dctl, (size_t)B * Tp * sizeof(float), hipMemcpyDeviceToDevice, s), "dur copy");
    // (a caller's pad values would count as frames: the reference's regulator loops over all Tp)
    if (iso) r.chk(launch_mask_rows(lengths, B, Tp, duration, nullptr, nullptr, nullptr, s), "duration mask");
    r.chk(launch_duration_cumsum(duration, cum_dur, frame_lengths, B, Tp, s, ctx->flags_dev), "duration cumsum");
    // (early_copy == false: the one-call form vsp_infer never reads the counts back -- nothing would consume the copy)
    if (r.ok() && early_copy && ctx->early_fl && early_frame_lengths_ready(ctx, B)) {
      hipError_t e = hipMemcpyAsync(ctx->fl_pinned, frame_lengths, (size_t)B * sizeof(int64_t), hipMemcpyDeviceToHost, s);
      if (e == hipSuccess) e = hipEventRecord(ctx->fl_ev, s);
      if (e == hipSuccess) { ctx->fl_src = frame_lengths; ctx->fl_n = B; }
    }
  }
  mask3(r, XE, lengths, B, h, Tp);  // TextEncoder passes x * x_mask (models.py:173)
  run_encoder_masked(r, m.enc[0], B, Tp, XE, lengths, XV);   // XV = x_enc
  // ---- duration (models.py:681-688, 119-133)
  if (!dur_given) {
    const int f = c.dur_filter;
    T3 A1 = P1, A2 = P2;
    r.cond(m.dur_cond, g, cvec, B);
    if (live) r.chk(launch_add_cond(XV.p, XV.bs, XV.cs, cvec, h, TMP.p, TMP.bs, TMP.cs, B, h, Tp, s), "add_cond");
    ConvArgs a = r.args(m.dur_c1, TMP, A1, Tp, Tp);
    a.lengths = lengths; a.in_mask = 1; a.act = 1;
    r.conv(a, B);
    r.ln(A1, T3{}, m.dur_g1, m.dur_b1, A1, B, f, Tp);
    a = r.args(m.dur_c2, A1, A2, Tp, Tp);
    a.lengths = lengths; a.in_mask = 1; a.act = 1;
    r.conv(a, B);
    r.ln(A2, T3{}, m.dur_g2, m.dur_b2, A2, B, f, Tp);
    if (live) {
      r.chk(launch_chan_dot(A2.p, A2.bs, A2.cs, r.A(m.dur_pw), r.A(m.dur_pb), lengths, 1, 1, pred, B, f, Tp, s), "dur proj");
      if (per_row) r.chk(launch_duration_rows(pred, dctl, lengths, rows_dev, duration, B, Tp, s), "duration rows");
      else r.chk(launch_duration_from_logw(pred, lengths, dscale, duration, B, Tp, s), "duration");
      if (iso) r.chk(launch_mask_rows(lengths, B, Tp, duration, nullptr, nullptr, nullptr, s), "duration mask");   // (ceil(-scale) at the pad)
    }
  }
  // ---- pitch (models.py:691-698, 505-514)
  if (!pit_given) {
    T3 PI = ws.t3(B, h, Tp);
    r.cond(m.pit_cond, g, cvec, B);
    if (live) r.chk(launch_add_cond(XV.p, XV.bs, XV.cs, cvec, h, TMP.p, TMP.bs, TMP.cs, B, h, Tp, s), "add_cond");
    mask3(r, TMP, lengths, B, h, Tp);
    run_encoder_masked(r, m.enc[1], B, Tp, TMP, lengths, PI);
    if (live) r.chk(launch_chan_dot(PI.p, PI.bs, PI.cs, r.A(m.pit_pw), r.A(m.pit_pb), lengths, 1, 0, pred, B, h, Tp, s), "proj_f0");
  }
  if (live) {
    if (per_row) r.chk(launch_pitch_rows(pctl, pred, rows_dev, lf0, f0, B, Tp, s), "pitch rows");
    else r.chk(launch_pitch(pctl, pred, pscale, lf0, f0, B * Tp, s), "pitch");
    // (the predicted lf0 carries proj_f0's bias at the pad, a control whatever the caller left there)
    if (iso) r.chk(launch_mask_rows(lengths, B, Tp, lf0, f0, nullptr, nullptr, s), "pitch mask");
    r.chk(launch_prenet_add(XV.p, XV.bs, XV.cs, r.A(m.ppre_w), r.A(m.ppre_b), lf0, B, h, Tp, s), "pitch_prenet");
  }
  // ---- energy (models.py:701-708; frame_prior_network.py:104-124: no mask anywhere)
  if (!en_given) {
    const int e = c.energy_filter;
    T3 A1 = P1, A2 = P2;
    r.cond(m.en_cond, g, cvec, B);
    if (live) r.chk(launch_add_cond(XV.p, XV.bs, XV.cs, cvec, h, TMP.p, TMP.bs, TMP.cs, B, h, Tp, s), "add_cond");
    ConvArgs a = r.args(m.en_c1, TMP, A1, Tp, Tp);
    a.act = 1;
    if (iso) { a.lengths = lengths; a.in_mask = 1; }   // x + cond(g) is not zero at the pad
    r.conv(a, B);
    r.ln(A1, T3{}, m.en_g1, m.en_b1, A1, B, e, Tp);
    a = r.args(m.en_c2, A1, A2, Tp, Tp);
    a.act = 1;
    if (iso) { a.lengths = lengths; a.in_mask = 1; }   // ... nor what conv 1 + LayerNorm put there
    r.conv(a, B);
    r.ln(A2, T3{}, m.en_g2, m.en_b2, A2, B, e, Tp);
    if (live) r.chk(launch_chan_dot(A2.p, A2.bs, A2.cs, r.A(m.en_lw), r.A(m.en_lb), nullptr, 0, 0, pred, B, e, Tp, s), "energy linear");
  }
  if (live) {
    if (per_row) r.chk(launch_energy_rows(ectl, pred, rows_dev, norm_e, energy, B, Tp, s), "energy rows");
    else r.chk(launch_energy(ectl, pred, escale, norm_e, energy, B * Tp, s), "energy");
    // (norm_energy, not the control: a zero energy control is norm_energy = -60 / 36 at the pad)
    if (iso) r.chk(launch_mask_rows(lengths, B, Tp, norm_e, energy, nullptr, nullptr, s), "energy mask");
    r.chk(launch_prenet_add(XV.p, XV.bs, XV.cs, r.A(m.epre_w), r.A(m.epre_b), norm_e, B, h, Tp, s), "energy_prenet");
    // (the regulator never reads x_var behind an utterance's end; zero all the same: the stage's output contract)
    if (iso) r.chk(launch_mask3(XV.p, XV.bs, XV.cs, lengths, B, h, Tp, s), "x_var mask");
    if (!dur_given) r.chk(launch_duration_cumsum(duration, cum_dur, frame_lengths, B, Tp, s, ctx->flags_dev), "duration cumsum");
  }
  if (ws.overflow) return ctx->fail(VSP_ERR_WORKSPACE, "encode workspace too small (need %zu bytes)", ws.cur);
  return r.rc;
}

// Per-row controls at an entry point.  Host state only, so it runs before anything that needs the device or the weights:
// a table has a meaning in isolated mode only, holds for one batch size, and a control some row is given must be there.
static int check_row_controls(vsp_ctx* ctx, int B, const char* fn, bool encodes, const float* dctl, const float* pctl,
                              const float* ectl) {
  if (!ctx || ctx->row_controls.empty()) return VSP_OK;
  if (!ctx->isolated)
    return ctx->fail(VSP_ERR_STATE, "%s: row controls are set but the context is not isolated (vsp_set_isolated)", fn);
  if ((int)ctx->row_controls.size() != B)
    return ctx->fail(VSP_ERR_STATE, "%s: row controls are set for B = %d, the call has B = %d", fn, (int)ctx->row_controls.size(), B);
  if (!encodes) return VSP_OK;
  uint32_t any = 0;
  for (const vsp_row_control& rc : ctx->row_controls) any |= rc.given;
  if (((any & VSP_GIVEN_DURATION) && !dctl) || ((any & VSP_GIVEN_PITCH) && !pctl) || ((any & VSP_GIVEN_ENERGY) && !ectl))
    return ctx->fail(VSP_ERR_ARG, "%s: a row is given a control whose tensor is NULL", fn);
  return VSP_OK;
}

int64_t vsp_encode_workspace_bytes(const vsp_ctx* ctx, int B, int Tp) {
  if (!ctx || B <= 0 || Tp <= 0) return VSP_ERR_ARG;
  Ws ws(nullptr, 0, true);
  encode_impl(const_cast<vsp_ctx*>(ctx), nullptr, ws, B, Tp, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 1,
              1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  return (int64_t)ws.cur;
}

int vsp_encode(vsp_ctx* ctx, void* stream, int B, int Tp, const int64_t* phonemes, const int64_t* lengths,
               const int64_t* sid, const float* duration_ctl, const float* pitch_ctl, const float* energy_ctl,
               float duration_scale, float pitch_scale, float energy_scale, float* x_var, float* g, float* duration,
               float* f0, float* energy, int64_t* frame_lengths, int32_t* cum_dur, void* workspace,
               int64_t workspace_bytes) {
  int rc = check_row_controls(ctx, B, "vsp_encode", true, duration_ctl, pitch_ctl, energy_ctl);
  if (rc == VSP_OK) rc = check_ready(ctx);
  if (rc) return rc;
  if (B <= 0 || Tp <= 0 || !phonemes || !lengths || !sid || !x_var || !g || !duration || !f0 || !energy ||
      !frame_lengths || !cum_dur || !workspace)
    return ctx->fail(VSP_ERR_ARG, "vsp_encode: null or non-positive argument");
  const int64_t need = vsp_encode_workspace_bytes(ctx, B, Tp);
  if (workspace_bytes < need)
    return ctx->fail(VSP_ERR_WORKSPACE, "encode workspace too small: %lld < %lld bytes", (long long)workspace_bytes, (long long)need);
  Ws ws(workspace, (size_t)workspace_bytes, false);
  return encode_impl(ctx, (hipStream_t)stream, ws, B, Tp, phonemes, lengths, sid, duration_ctl, pitch_ctl, energy_ctl,
                     duration_scale, pitch_scale, energy_scale, x_var, g, duration, f0, energy, frame_lengths, cum_dur);
}

int vsp_frame_lengths_host(vsp_ctx* ctx, void* stream, int B, const int64_t* frame_lengths_dev,
                           int64_t* frame_lengths_host, int64_t* max_frames) {
  if (!ctx || B <= 0 || !frame_lengths_dev || !frame_lengths_host || !max_frames)
    return ctx ? ctx->fail(VSP_ERR_ARG, "vsp_frame_lengths_host: bad argument") : VSP_ERR_ARG;
  hipError_t e;
  if (ctx->fl_src == frame_lengths_dev && ctx->fl_n == B) {
    // vsp_encode already started this copy (given durations): wait for IT, not for the rest of the stream
    e = hipEventSynchronize(ctx->fl_ev);
    if (e == hipSuccess) std::memcpy(frame_lengths_host, ctx->fl_pinned, (size_t)B * sizeof(int64_t));
    ctx->fl_src = nullptr;
  } else {
    e = hipMemcpyAsync(frame_lengths_host, frame_lengths_dev, (size_t)B * sizeof(int64_t), hipMemcpyDeviceToHost,
                       (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  }
  if (e != hipSuccess) return ctx->fail(VSP_ERR_HIP, "frame length read: %s", hipGetErrorString(e));
  int64_t mx = 0;
  for (int b = 0; b < B; ++b) mx = std::max(mx, frame_lengths_host[b]);
  *max_frames = mx;
  ctx->fl_known.assign(frame_lengths_host, frame_lengths_host + B);   // (model.h: until the next vsp_encode)
  ctx->fl_known_src = frame_lengths_dev;
  return VSP_OK;
}

// -------------------------------------------------------------------------------------------- decode
static int decode_impl(vsp_ctx* ctx, hipStream_t s, Ws& ws, int B, int Tp, int Tf, int max_len, const float* x_var,
                       const float* g, const int32_t* cum_dur, const int64_t* frame_lengths, const float* noise,
                       uint64_t noise_seed, float noise_scale, float* o, uint8_t* x_mask, float* z, float* z_p, float* m_p,
                       float* logs_p) {
  const vsp_config& c = ctx->cfg;
  const Model& m = ctx->model;
  const int h = c.hidden_channels, inter = c.inter_channels;
  Run r{ctx, s, ws};
  r.iso = ctx->isolated;
  if (frame_lengths && ctx->fl_known_src == frame_lengths && (int)ctx->fl_known.size() == B) r.host_lengths = ctx->fl_known.data();
  T3 XF = ws.t3(B, h, Tf), HF = ws.t3(B, h, Tf);
  // noise == NULL: the library draws it (Philox4x32-10 keyed by noise_seed) -- the torch.randn_like of models.py:718
  float* drawn = ws.f((size_t)B * inter * Tf);
  uint64_t* seeds_dev = reinterpret_cast<uint64_t*>(ws.bytes((size_t)B * sizeof(uint64_t)));
  vsp_row_control* rows_dev = reinterpret_cast<vsp_row_control*>(ws.bytes((size_t)B * sizeof(vsp_row_control)));
  const bool live = !ws.dry && !ws.overflow;
  // per-row controls (vsp_set_row_controls): noise_scale[b] replaces the argument -- noise is drawn iff some row's is
  // non-zero -- and the table is copied into THIS call's workspace, as the seeds are
  const std::vector<vsp_row_control>& rows = ctx->row_controls;
  const bool per_row = !rows.empty();
  const bool want_noise = per_row ? std::any_of(rows.begin(), rows.end(), [](const vsp_row_control& rc) { return rc.noise_scale != 0.f; })
                                  : noise_scale != 0.f;
  if (live && per_row)
    r.chk(hipMemcpyAsync(rows_dev, rows.data(), (size_t)B * sizeof(vsp_row_control), hipMemcpyHostToDevice, s), "row controls");
  if (live && !noise && want_noise && r.iso) {
    // isolated mode: utterance b's own draw, keyed seeds[b], laid out [inter][L_b] -- what a B = 1 call with Tf = L_b and
    // noise_seed = seeds[b] draws (vsp_set_noise_seeds; noise_seed and the noise offset are not read)
    if ((int)ctx->noise_seeds.size() != B)
      return ctx->fail(VSP_ERR_STATE, "isolated mode draws per-utterance noise: vsp_set_noise_seeds for B = %d first (%d set)",
                       B, (int)ctx->noise_seeds.size());
    // (pageable source: the runtime reads it into its own staging memory before this call returns -- hipMemcpyAsync is
    // asynchronous only for pinned host memory -- so a later vsp_set_noise_seeds may replace the vector while the copy is
    // still queued on the stream; the seeds land in THIS call's workspace, not in context memory the next call overwrites)
    r.chk(hipMemcpyAsync(seeds_dev, ctx->noise_seeds.data(), (size_t)B * sizeof(uint64_t), hipMemcpyHostToDevice, s), "noise seeds");
    if (r.ok()) r.chk(launch_randn_ragged(seeds_dev, frame_lengths, B, inter, Tf, drawn, s), "randn_ragged");
    noise = drawn;
  } else if (live && !noise && want_noise) {
    r.chk(launch_randn(noise_seed, (long)ctx->noise_first, (long)B * inter * Tf, drawn, s), "randn");
    noise = drawn;
  }
  if (live) {
    r.chk(launch_length_regulate(x_var, (long)h * Tp, Tp, cum_dur, XF.p, XF.bs, XF.cs, B, h, Tp, Tf, s), "length_regulate");
    r.chk(launch_mask_u8(frame_lengths, x_mask, B, Tf, s), "x_mask");
  }
  run_encoder_masked(r, m.enc[2], B, Tf, XF, frame_lengths, HF);
  const T3 MP = ext(m_p, inter, Tf), LP = ext(logs_p, inter, Tf), Z = ext(z, inter, Tf);
  // Projection (reference models.py:526-529): one 1x1 convolution, m_p and logs_p rows to their own tensors
  ConvArgs a = r.args(m.proj, HF, MP, Tf, Tf);
  a.lengths = frame_lengths; a.mask_post = 1;
  a.split_row = inter; a.out2 = LP.p; a.o2_bs = LP.bs; a.o2_cs = LP.cs; a.mask_post2 = 1;
  r.conv(a, B);
  if (live) {
    const long n = (long)B * inter * Tf;
    // (z = z_p: the flow transforms z in place)
    if (per_row) r.chk(launch_reparam_rows(m_p, logs_p, noise, rows_dev, z_p, B, (long)inter * Tf, s, z, ctx->flags_dev), "reparam rows");
    else r.chk(launch_reparam(m_p, logs_p, noise, noise_scale, z_p, n, s, z, ctx->flags_dev), "reparam");
    if (r.iso) {   // m_p = logs_p = 0 at the pad: z_p is noise * noise_scale there
      r.chk(launch_mask3(z_p, (long)inter * Tf, Tf, frame_lengths, B, inter, Tf, s), "z_p mask");
      r.chk(launch_mask3(z, (long)inter * Tf, Tf, frame_lengths, B, inter, Tf, s), "z mask");
    }
  }
  run_flow(r, B, Tf, Z, g, frame_lengths);
  const int Tdec = max_len < 0 ? Tf : std::min(Tf, max_len);
  if (Tdec > 0) run_gen(r, B, Tdec, Z, frame_lengths, g, o);
  if (ws.overflow) return ctx->fail(VSP_ERR_WORKSPACE, "decode workspace too small (need %zu bytes)", ws.cur);
  return r.rc;
}

int64_t vsp_decode_workspace_bytes(const vsp_ctx* ctx, int B, int Tp, int Tf) {
  if (!ctx || B <= 0 || Tp <= 0 || Tf <= 0) return VSP_ERR_ARG;
  Ws ws(nullptr, 0, true);
  decode_impl(const_cast<vsp_ctx*>(ctx), nullptr, ws, B, Tp, Tf, -1, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0.f,
              nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  return (int64_t)ws.cur;
}

int vsp_decode(vsp_ctx* ctx, void* stream, int B, int Tp, int Tf, int max_len, const float* x_var, const float* g,
               const int32_t* cum_dur, const int64_t* frame_lengths, const float* noise, uint64_t noise_seed,
               float noise_scale, float* o, uint8_t* x_mask, float* z, float* z_p, float* m_p, float* logs_p,
               void* workspace, int64_t workspace_bytes) {
  int rc = check_row_controls(ctx, B, "vsp_decode", false, nullptr, nullptr, nullptr);
  if (rc == VSP_OK) rc = check_ready(ctx);
  if (rc) return rc;
  if (B <= 0 || Tp <= 0 || Tf <= 0 || !x_var || !g || !cum_dur || !frame_lengths || !o || !x_mask || !z || !z_p ||
      !m_p || !logs_p || !workspace)
    return ctx->fail(VSP_ERR_ARG, "vsp_decode: null or non-positive argument");
  const int64_t need = vsp_decode_workspace_bytes(ctx, B, Tp, Tf);
  if (workspace_bytes < need)
    return ctx->fail(VSP_ERR_WORKSPACE, "decode workspace too small: %lld < %lld bytes", (long long)workspace_bytes, (long long)need);
  Ws ws(workspace, (size_t)workspace_bytes, false);
  return decode_impl(ctx, (hipStream_t)stream, ws, B, Tp, Tf, max_len, x_var, g, cum_dur, frame_lengths, noise,
                     noise_seed, noise_scale, o, x_mask, z, z_p, m_p, logs_p);
}

// one-call form: encode + decode with a caller-supplied frame padding, no host synchronisation
static int infer_impl(vsp_ctx* ctx, hipStream_t s, Ws& ws, int B, int Tp, int Tf, int max_len, const int64_t* phonemes,
                      const int64_t* lengths, const int64_t* sid, const float* dctl, const float* pctl, const float* ectl,
                      float dsc, float psc, float esc, const float* noise, uint64_t noise_seed, float noise_scale, float* o,
                      uint8_t* x_mask, float* z, float* z_p, float* m_p, float* logs_p, float* duration, float* f0,
                      float* energy, int64_t* frame_lengths) {
  const vsp_config& c = ctx->cfg;
  float* x_var = ws.f((size_t)B * c.hidden_channels * Tp);
  float* g = ws.f((size_t)B * c.gin_channels);
  int32_t* cum = (int32_t*)ws.bytes((size_t)B * Tp * sizeof(int32_t));
  const size_t mark = ws.cur;
  int rc = encode_impl(ctx, s, ws, B, Tp, phonemes, lengths, sid, dctl, pctl, ectl, dsc, psc, esc, x_var, g, duration,
                       f0, energy, frame_lengths, cum, /*early_copy=*/false);
  const size_t after_enc = ws.cur;
  ws.cur = mark;                 // the two halves run one after the other on one stream: shared scratch
  if (rc == VSP_OK)
    rc = decode_impl(ctx, s, ws, B, Tp, Tf, max_len, x_var, g, cum, frame_lengths, noise, noise_seed, noise_scale, o, x_mask,
                     z, z_p, m_p, logs_p);
  ws.cur = std::max(ws.cur, after_enc);
  return rc;
}

int64_t vsp_infer_workspace_bytes(const vsp_ctx* ctx, int B, int Tp, int tf_pad) {
  if (!ctx || B <= 0 || Tp <= 0 || tf_pad <= 0) return VSP_ERR_ARG;
  Ws ws(nullptr, 0, true);
  infer_impl(const_cast<vsp_ctx*>(ctx), nullptr, ws, B, Tp, tf_pad, -1, nullptr, nullptr, nullptr, nullptr, nullptr,
             nullptr, 1.f, 1.f, 1.f, nullptr, 0, 0.f, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
             nullptr, nullptr);
  return (int64_t)ws.cur;
}

int vsp_infer(vsp_ctx* ctx, void* stream, int B, int Tp, int tf_pad, int max_len, const int64_t* phonemes,
              const int64_t* lengths, const int64_t* sid, const float* duration_ctl, const float* pitch_ctl,
              const float* energy_ctl, float duration_scale, float pitch_scale, float energy_scale, const float* noise,
              uint64_t noise_seed, float noise_scale, float* o, uint8_t* x_mask, float* z, float* z_p, float* m_p, float* logs_p,
              float* duration, float* f0, float* energy, int64_t* frame_lengths, void* workspace,
              int64_t workspace_bytes) {
  int rc = check_row_controls(ctx, B, "vsp_infer", true, duration_ctl, pitch_ctl, energy_ctl);
  if (rc == VSP_OK) rc = check_ready(ctx);
  if (rc) return rc;
  if (B <= 0 || Tp <= 0 || tf_pad <= 0 || !phonemes || !lengths || !sid || !o || !x_mask || !z || !z_p || !m_p ||
      !logs_p || !duration || !f0 || !energy || !frame_lengths || !workspace)
    return ctx->fail(VSP_ERR_ARG, "vsp_infer: null or non-positive argument");
  const int64_t need = vsp_infer_workspace_bytes(ctx, B, Tp, tf_pad);
  if (workspace_bytes < need)
    return ctx->fail(VSP_ERR_WORKSPACE, "infer workspace too small: %lld < %lld bytes", (long long)workspace_bytes,
                     (long long)need);
  Ws ws(workspace, (size_t)workspace_bytes, false);
  return infer_impl(ctx, (hipStream_t)stream, ws, B, Tp, tf_pad, max_len, phonemes, lengths, sid, duration_ctl, pitch_ctl,
                    energy_ctl, duration_scale, pitch_scale, energy_scale, noise, noise_seed, noise_scale, o, x_mask, z, z_p,
                    m_p, logs_p, duration, f0, energy, frame_lengths);
}

// -------------------------------------------------------------------------------------------- stages
int64_t vsp_attention_workspace_bytes(const vsp_ctx* ctx, int B, int T) {
  if (!ctx || B <= 0 || T <= 0) return VSP_ERR_ARG;
  const vsp_config& c = ctx->cfg;
  // the packed q | k | v operand images of the split-f16 kernel; the f32 kernel (VSP_ATT=f32) needs none
  return ctx->att_f16s ? (int64_t)(3 * attn_pack_bytes(B, c.n_heads, c.hidden_channels / c.n_heads, T)) : 256;
}

int vsp_attention(vsp_ctx* ctx, void* stream, int which, int layer, int B, int T, const float* qkv, const int64_t* lengths,
                  float* out, void* workspace, int64_t workspace_bytes) {
  int rc = check_ready(ctx);
  if (rc) return rc;
  if (which < 0 || which > 2 || B <= 0 || T <= 0 || !qkv || !lengths || !out || !workspace)
    return ctx->fail(VSP_ERR_ARG, "vsp_attention: bad argument");
  const EncoderW& E = ctx->model.enc[which];
  if (layer < 0 || layer >= (int)E.layers.size()) return ctx->fail(VSP_ERR_ARG, "vsp_attention: no such layer");
  if (workspace_bytes < vsp_attention_workspace_bytes(ctx, B, T))
    return ctx->fail(VSP_ERR_WORKSPACE, "attention workspace too small (need %lld bytes)",
                     (long long)vsp_attention_workspace_bytes(ctx, B, T));
  const vsp_config& c = ctx->cfg;
  const int h = c.hidden_channels;
  const EncLayer& L = E.layers[layer];
  hipError_t e;
  if (ctx->att_f16s)
    e = launch_attention_f16s(qkv, 3L * h * T, T, ctx->arena + L.ek, ctx->arena + L.ev, lengths, out, (long)h * T, T, B, h,
                              c.n_heads, T, c.window_size, workspace, (hipStream_t)stream);
  else
    e = launch_attention(qkv, 3L * h * T, T, ctx->arena + L.ek, ctx->arena + L.ev, lengths, out, (long)h * T, T,
                         B, h, c.n_heads, T, c.window_size, ctx->att_ksplit, (hipStream_t)stream);
  return e == hipSuccess ? VSP_OK : ctx->fail(VSP_ERR_HIP, "attention: %s", hipGetErrorString(e));
}

int64_t vsp_encoder_workspace_bytes(const vsp_ctx* ctx, int B, int T) {
  if (!ctx || B <= 0 || T <= 0) return VSP_ERR_ARG;
  Ws ws(nullptr, 0, true);
  Run r{const_cast<vsp_ctx*>(ctx), nullptr, ws};
  ws.t3(B, ctx->cfg.hidden_channels, T);
  run_encoder_masked(r, ctx->model.enc[0], B, T, T3{}, nullptr, T3{});
  return (int64_t)ws.cur;
}

int vsp_encoder(vsp_ctx* ctx, void* stream, int which, int B, int T, const float* x, const int64_t* lengths, float* y,
                void* workspace, int64_t workspace_bytes) {
  int rc = check_ready(ctx);
  if (rc) return rc;
  if (which < 0 || which > 2 || B <= 0 || T <= 0 || !x || !lengths || !y || !workspace)
    return ctx->fail(VSP_ERR_ARG, "vsp_encoder: bad argument");
  if (workspace_bytes < vsp_encoder_workspace_bytes(ctx, B, T))
    return ctx->fail(VSP_ERR_WORKSPACE, "encoder workspace too small");
  Ws ws(workspace, (size_t)workspace_bytes, false);
  Run r{ctx, (hipStream_t)stream, ws};
  const int h = ctx->cfg.hidden_channels;
  // the reference call sites pass x * x_mask (models.py:173, 469, 511): mask a private copy
  T3 XI = ws.t3(B, h, T);
  if (ws.overflow) return ctx->fail(VSP_ERR_WORKSPACE, "encoder workspace too small");
  r.chk(launch_copy3(x, (long)h * T, T, XI.p, XI.bs, XI.cs, B, h, T, r.s), "copy");
  mask3(r, XI, lengths, B, h, T);
  run_encoder_masked(r, ctx->model.enc[which], B, T, XI, lengths, ext(y, h, T));
  if (ws.overflow) return ctx->fail(VSP_ERR_WORKSPACE, "encoder workspace too small (need %zu bytes)", ws.cur);
  return r.rc;
}

int vsp_length_regulate(vsp_ctx* ctx, void* stream, int B, int C, int Tp, int Tf, const float* x, const int32_t* cum_dur,
                        float* x_frame) {
  if (!ctx || B <= 0 || C <= 0 || Tp <= 0 || Tf <= 0 || !x || !cum_dur || !x_frame)
    return ctx ? ctx->fail(VSP_ERR_ARG, "vsp_length_regulate: bad argument") : VSP_ERR_ARG;
  hipError_t e = launch_length_regulate(x, (long)C * Tp, Tp, cum_dur, x_frame, (long)C * Tf, Tf, B, C, Tp, Tf,
                                        (hipStream_t)stream);
  return e == hipSuccess ? VSP_OK : ctx->fail(VSP_ERR_HIP, "length_regulate: %s", hipGetErrorString(e));
}

int64_t vsp_flow_workspace_bytes(const vsp_ctx* ctx, int B, int Tf) {
  if (!ctx || B <= 0 || Tf <= 0) return VSP_ERR_ARG;
  Ws ws(nullptr, 0, true);
  Run r{const_cast<vsp_ctx*>(ctx), nullptr, ws};
  run_flow(r, B, Tf, T3{}, nullptr, nullptr);
  return (int64_t)ws.cur;
}

int vsp_flow_reverse(vsp_ctx* ctx, void* stream, int B, int Tf, const float* z_p, const float* g,
                     const int64_t* frame_lengths, float* z, void* workspace, int64_t workspace_bytes) {
  int rc = check_ready(ctx);
  if (rc) return rc;
  if (B <= 0 || Tf <= 0 || !z_p || !g || !frame_lengths || !z || !workspace)
    return ctx->fail(VSP_ERR_ARG, "vsp_flow_reverse: bad argument");
  if (workspace_bytes < vsp_flow_workspace_bytes(ctx, B, Tf))
    return ctx->fail(VSP_ERR_WORKSPACE, "flow workspace too small");
  Ws ws(workspace, (size_t)workspace_bytes, false);
  Run r{ctx, (hipStream_t)stream, ws};
  const long n = (long)B * ctx->cfg.inter_channels * Tf;
  r.chk(hipMemcpyAsync(z, z_p, n * sizeof(float), hipMemcpyDeviceToDevice, r.s), "z copy");
  run_flow(r, B, Tf, ext(z, ctx->cfg.inter_channels, Tf), g, frame_lengths);
  if (ws.overflow) return ctx->fail(VSP_ERR_WORKSPACE, "flow workspace too small (need %zu bytes)", ws.cur);
  return r.rc;
}

int vsp_flow_forward(vsp_ctx* ctx, void* stream, int B, int Tf, const float* z, const float* g,
                     const int64_t* frame_lengths, float* z_p, void* workspace, int64_t workspace_bytes) {
  int rc = check_ready(ctx);
  if (rc) return rc;
  if (B <= 0 || Tf <= 0 || !z || !g || !frame_lengths || !z_p || !workspace)
    return ctx->fail(VSP_ERR_ARG, "vsp_flow_forward: bad argument");
  if (workspace_bytes < vsp_flow_workspace_bytes(ctx, B, Tf))
    return ctx->fail(VSP_ERR_WORKSPACE, "flow workspace too small");
  Ws ws(workspace, (size_t)workspace_bytes, false);
  Run r{ctx, (hipStream_t)stream, ws};
  const long n = (long)B * ctx->cfg.inter_channels * Tf;
  r.chk(hipMemcpyAsync(z_p, z, n * sizeof(float), hipMemcpyDeviceToDevice, r.s), "z copy");
  run_flow(r, B, Tf, ext(z_p, ctx->cfg.inter_channels, Tf), g, frame_lengths, false);
  if (ws.overflow) return ctx->fail(VSP_ERR_WORKSPACE, "flow workspace too small (need %zu bytes)", ws.cur);
  return r.rc;
}

static int check_vc(vsp_ctx* ctx);

// One layer of modules.WN.forward (reference modules.py:148-176), for unit parity: which 0 .. n_flows-1 = the WN of
// flow.flows[2 * which], -1 = enc_q.enc.
static int wn_layer_impl(vsp_ctx* ctx, hipStream_t s, Ws& ws, int which, int layer, int B, int T, float* x, const float* g,
                         const int64_t* lengths, float* skip, int accumulate) {
  const vsp_config& c = ctx->cfg;
  const Model& m = ctx->model;
  const int h = c.hidden_channels;
  const bool post = which < 0;
  const Conv& cond = post ? m.enc_q.cond : m.flows[which].cond;
  const std::vector<Conv>& in = post ? m.enc_q.in : m.flows[which].in;
  const std::vector<Conv>& res = post ? m.enc_q.res : m.flows[which].res;
  const std::vector<Conv>& sk = post ? m.enc_q.skip : m.flows[which].skip;
  const int nl = post ? c.posterior_layers : c.flow_layers;
  Run r{ctx, s, ws};
  T3 ACT = ws.t3(B, h, T);
  float* gc = ws.f((size_t)B * 2 * h * nl);
  if (ws.dry) return VSP_OK;
  if (ws.overflow) return ctx->fail(VSP_ERR_WORKSPACE, "wn layer workspace too small");
  const T3 H = ext(x, h, T), OUT = ext(skip, h, T);
  r.cond(cond, g, gc, B);                              // cond_layer(g): all layers' rows, this layer's slice is used
  ConvArgs a = r.args(in[layer], H, ACT, T, T);
  a.act = 2; a.cond = gc + (size_t)layer * 2 * h; a.cond_bs = 2L * h * nl;
  r.conv(a, B);
  if (layer < nl - 1) {
    a = r.args(res[layer], ACT, H, T, T);
    a.res = H.p; a.r_bs = H.bs; a.r_cs = H.cs;
    a.lengths = lengths; a.mask_post = 1;
    a.split_row = h; a.out2 = OUT.p; a.o2_bs = OUT.bs; a.o2_cs = OUT.cs; a.acc_prev2 = accumulate ? 1 : 0;
    r.conv(a, B);
  } else {
    a = r.args(sk[layer], ACT, OUT, T, T);
    a.acc_prev = accumulate ? 1 : 0;
    a.lengths = lengths; a.mask_post = 1;
    r.conv(a, B);
  }
  return r.rc;
}

int64_t vsp_wn_layer_workspace_bytes(const vsp_ctx* ctx, int which, int B, int T) {
  if (!ctx || B <= 0 || T <= 0 || which < -1 || which >= ctx->cfg.n_flows) return VSP_ERR_ARG;
  if (which < 0 && ctx->cfg.spec_channels <= 0) return VSP_ERR_ARG;
  Ws ws(nullptr, 0, true);
  wn_layer_impl(const_cast<vsp_ctx*>(ctx), nullptr, ws, which, 0, B, T, nullptr, nullptr, nullptr, nullptr, 0);
  return (int64_t)ws.cur;
}

int vsp_wn_layer(vsp_ctx* ctx, void* stream, int which, int layer, int B, int T, float* x, const float* g,
                 const int64_t* lengths, float* skip, int accumulate, void* workspace, int64_t workspace_bytes) {
  int rc = which < 0 ? check_vc(ctx) : check_ready(ctx);
  if (rc) return rc;
  if (which < -1 || which >= ctx->cfg.n_flows || B <= 0 || T <= 0 || !x || !g || !lengths || !skip || !workspace || x == skip)
    return ctx->fail(VSP_ERR_ARG, "vsp_wn_layer: bad argument");
  const int nl = which < 0 ? ctx->cfg.posterior_layers : ctx->cfg.flow_layers;
  if (layer < 0 || layer >= nl) return ctx->fail(VSP_ERR_ARG, "vsp_wn_layer: no such layer");
  if (workspace_bytes < vsp_wn_layer_workspace_bytes(ctx, which, B, T))
    return ctx->fail(VSP_ERR_WORKSPACE, "wn layer workspace too small");
  Ws ws(workspace, (size_t)workspace_bytes, false);
  return wn_layer_impl(ctx, (hipStream_t)stream, ws, which, layer, B, T, x, g, lengths, skip, accumulate);
}

int vsp_randn(void* stream, uint64_t seed, int64_t n, float* out) { return vsp_randn_at(stream, seed, 0, n, out); }

int vsp_randn_at(void* stream, uint64_t seed, int64_t first, int64_t n, float* out) {
  if (n < 0 || first < 0 || (n > 0 && !out)) return VSP_ERR_ARG;
  return launch_randn(seed, (long)first, (long)n, out, (hipStream_t)stream) == hipSuccess ? VSP_OK : VSP_ERR_HIP;
}

int vsp_set_noise_offset(vsp_ctx* ctx, int64_t first_element) {
  if (!ctx || first_element < 0) return ctx ? ctx->fail(VSP_ERR_ARG, "vsp_set_noise_offset: negative offset") : VSP_ERR_ARG;
  ctx->noise_first = first_element;
  return VSP_OK;
}

int vsp_set_isolated(vsp_ctx* ctx, int on) {
  if (!ctx) return VSP_ERR_ARG;
  ctx->isolated = on != 0;
  return VSP_OK;
}

int vsp_get_isolated(const vsp_ctx* ctx) { return ctx ? (ctx->isolated ? 1 : 0) : VSP_ERR_ARG; }

int vsp_set_noise_seeds(vsp_ctx* ctx, const uint64_t* seeds_host, int B) {
  if (!ctx) return VSP_ERR_ARG;
  if (B < 0 || (B > 0 && !seeds_host)) return ctx->fail(VSP_ERR_ARG, "vsp_set_noise_seeds: B < 0 or null seeds");
  ctx->noise_seeds.assign(seeds_host, seeds_host + B);     // (B = 0 forgets them)
  return VSP_OK;
}

int vsp_set_row_controls(vsp_ctx* ctx, const vsp_row_control* rows_host, int B) {
  if (!ctx) return VSP_ERR_ARG;
  if (B < 0 || (B > 0 && !rows_host)) return ctx->fail(VSP_ERR_ARG, "vsp_set_row_controls: B < 0 or null rows");
  const uint32_t known = VSP_GIVEN_DURATION | VSP_GIVEN_PITCH | VSP_GIVEN_ENERGY;
  for (int b = 0; b < B; ++b) {
    const vsp_row_control& rc = rows_host[b];
    if (rc.given & ~known) return ctx->fail(VSP_ERR_ARG, "vsp_set_row_controls: row %d has unknown given bits 0x%x", b, rc.given);
    if (!std::isfinite(rc.duration_scale) || !std::isfinite(rc.pitch_scale) || !std::isfinite(rc.energy_scale) ||
        !std::isfinite(rc.noise_scale))
      return ctx->fail(VSP_ERR_ARG, "vsp_set_row_controls: row %d has a scale that is not finite", b);
  }
  ctx->row_controls.assign(rows_host, rows_host + B);     // (B = 0 forgets the table; a refused table changes nothing)
  return VSP_OK;
}

// ---------------------------------------------------------------------------------- spectrogram
int vsp_spectrogram_frames(const vsp_ctx* ctx, int L, int hop) {
  if (!ctx || ctx->cfg.spec_channels <= 1 || hop <= 0) return VSP_ERR_ARG;
  const int n_fft = 2 * (ctx->cfg.spec_channels - 1), pad = (n_fft - hop) / 2;
  if (L <= pad || n_fft < hop) return VSP_ERR_ARG;      // reflect padding needs pad < L
  return 1 + (L + 2 * pad - n_fft) / hop;
}

static int spectrogram_impl(vsp_ctx* ctx, hipStream_t s, Ws& ws, int B, int L, int hop, int T, const float* audio,
                            float* spec) {
  const vsp_config& c = ctx->cfg;
  const int n_fft = 2 * (c.spec_channels - 1);
  Run r{ctx, s, ws};
  T3 F = ws.t3(B, n_fft, T), RI = ws.t3(B, 2 * c.spec_channels, T);
  if (ws.dry) return VSP_OK;
  if (ws.overflow) return ctx->fail(VSP_ERR_WORKSPACE, "spectrogram workspace too small");
  r.chk(launch_stft_frames(audio, L, F.p, F.bs, F.cs, B, L, n_fft, hop, T, s), "stft frames");
  ConvArgs a = r.args(ctx->model.stft, F, RI, T, T);
  r.conv(a, B);
  if (r.ok()) r.chk(launch_stft_magnitude(RI.p, RI.bs, RI.cs, spec, B, c.spec_channels, T, s), "stft magnitude");
  return r.rc;
}

int64_t vsp_spectrogram_workspace_bytes(const vsp_ctx* ctx, int B, int L, int hop) {
  const int T = vsp_spectrogram_frames(ctx, L, hop);
  if (T <= 0 || B <= 0) return VSP_ERR_ARG;
  Ws ws(nullptr, 0, true);
  spectrogram_impl(const_cast<vsp_ctx*>(ctx), nullptr, ws, B, L, hop, T, nullptr, nullptr);
  return (int64_t)ws.cur;
}

int vsp_spectrogram(vsp_ctx* ctx, void* stream, int B, int L, int hop, const float* audio, float* spec, void* workspace,
                    int64_t workspace_bytes) {
  int rc = check_ready(ctx);
  if (rc) return rc;
  if (ctx->cfg.spec_channels <= 1) return ctx->fail(VSP_ERR_STATE, "context was created without spec_channels");
  const int T = vsp_spectrogram_frames(ctx, L, hop);
  if (T <= 0 || B <= 0 || !audio || !spec || !workspace)
    return ctx->fail(VSP_ERR_ARG, "vsp_spectrogram: bad argument (the signal must be longer than (n_fft - hop) / 2)");
  if (workspace_bytes < vsp_spectrogram_workspace_bytes(ctx, B, L, hop))
    return ctx->fail(VSP_ERR_WORKSPACE, "spectrogram workspace too small");
  Ws ws(workspace, (size_t)workspace_bytes, false);
  return spectrogram_impl(ctx, (hipStream_t)stream, ws, B, L, hop, T, audio, spec);
}

// ---------------------------------------------------------------------------------- voice conversion
static int check_vc(vsp_ctx* ctx) {
  const int rc = check_ready(ctx);
  if (rc) return rc;
  if (ctx->cfg.spec_channels <= 0) return ctx->fail(VSP_ERR_STATE, "context was created without spec_channels");
  if (!ctx->model.has_vc) return ctx->fail(VSP_ERR_STATE, "enc_q.* tensors were not loaded before vsp_finalize_weights");
  return VSP_OK;
}

int64_t vsp_posterior_workspace_bytes(const vsp_ctx* ctx, int B, int T) {
  if (!ctx || B <= 0 || T <= 0) return VSP_ERR_ARG;
  Ws ws(nullptr, 0, true);
  Run r{const_cast<vsp_ctx*>(ctx), nullptr, ws};
  run_posterior(r, B, T, T3{}, nullptr, nullptr, nullptr, T3{}, T3{}, T3{});
  return (int64_t)ws.cur;
}

int vsp_posterior_encoder(vsp_ctx* ctx, void* stream, int B, int T, const float* y, const int64_t* y_lengths,
                          const float* g, const float* noise, float* z, float* m, float* logs, void* workspace,
                          int64_t workspace_bytes) {
  int rc = check_vc(ctx);
  if (rc) return rc;
  if (B <= 0 || T <= 0 || !y || !y_lengths || !g || !noise || !z || !m || !logs || !workspace)
    return ctx->fail(VSP_ERR_ARG, "vsp_posterior_encoder: bad argument");
  if (workspace_bytes < vsp_posterior_workspace_bytes(ctx, B, T))
    return ctx->fail(VSP_ERR_WORKSPACE, "posterior workspace too small");
  Ws ws(workspace, (size_t)workspace_bytes, false);
  Run r{ctx, (hipStream_t)stream, ws};
  const int inter = ctx->cfg.inter_channels;
  run_posterior(r, B, T, ext(y, ctx->cfg.spec_channels, T), y_lengths, g, noise, ext(z, inter, T), ext(m, inter, T),
                ext(logs, inter, T));
  if (ws.overflow) return ctx->fail(VSP_ERR_WORKSPACE, "posterior workspace too small (need %zu bytes)", ws.cur);
  return r.rc;
}

// SynthesizerTrn.voice_conversion (reference models.py:724-732)
static int vc_impl(vsp_ctx* ctx, hipStream_t s, Ws& ws, int B, int T, const float* y, const int64_t* y_lengths,
                   const int64_t* sid_src, const int64_t* sid_tgt, const float* noise, float* o_hat, uint8_t* y_mask,
                   float* z, float* z_p, float* z_hat, float* m_q, float* logs_q) {
  const vsp_config& c = ctx->cfg;
  const Model& m = ctx->model;
  const int inter = c.inter_channels, gin = c.gin_channels;
  Run r{ctx, s, ws};
  r.iso = ctx->isolated;     // (the posterior encoder and both flows mask already: the generator call is the difference)
  float* g_src = ws.f((size_t)B * gin);
  float* g_tgt = ws.f((size_t)B * gin);
  T3 MQ = m_q ? ext(m_q, inter, T) : ws.t3(B, inter, T);
  T3 LQ = logs_q ? ext(logs_q, inter, T) : ws.t3(B, inter, T);
  if (!m_q || !logs_q) {
    // launch_reparam walks contiguous tensors: the scratch copies must be dense too
    MQ.cs = LQ.cs = T; MQ.bs = LQ.bs = (long)inter * T;
  }
  const bool live = !ws.dry && !ws.overflow;
  if (live) {
    r.chk(launch_gather_rows(sid_src, r.A(m.emb_g), c.n_speakers, g_src, B, gin, s), "emb_g");
    r.chk(launch_gather_rows(sid_tgt, r.A(m.emb_g), c.n_speakers, g_tgt, B, gin, s), "emb_g");
    r.chk(launch_mask_u8(y_lengths, y_mask, B, T, s), "y_mask");
  }
  const size_t mark = ws.cur;
  run_posterior(r, B, T, ext(y, c.spec_channels, T), y_lengths, g_src, noise, ext(z, inter, T), MQ, LQ);
  const size_t after_post = ws.cur;
  ws.cur = mark;  // the three stages run one after another on one stream: they share scratch
  const long n = (long)B * inter * T;
  if (live && r.ok()) r.chk(hipMemcpyAsync(z_p, z, n * sizeof(float), hipMemcpyDeviceToDevice, s), "z_p copy");
  run_flow(r, B, T, ext(z_p, inter, T), g_src, y_lengths, false);
  if (live && r.ok()) r.chk(hipMemcpyAsync(z_hat, z_p, n * sizeof(float), hipMemcpyDeviceToDevice, s), "z_hat copy");
  ws.cur = mark;
  run_flow(r, B, T, ext(z_hat, inter, T), g_tgt, y_lengths, true);
  const size_t after_flow = ws.cur;
  ws.cur = mark;
  // dec(z_hat * y_mask, g_tgt): z_hat is already masked by the flow's last update on x1 ... but x0
  // passes through unmasked only if the input was unmasked; z is masked, so z_hat * mask == z_hat.
  run_gen(r, B, T, ext(z_hat, inter, T), y_lengths, g_tgt, o_hat);
  ws.cur = std::max(ws.cur, std::max(after_post, after_flow));
  if (ws.overflow) return ctx->fail(VSP_ERR_WORKSPACE, "voice conversion workspace too small (need %zu bytes)", ws.cur);
  return r.rc;
}

int64_t vsp_voice_conversion_workspace_bytes(const vsp_ctx* ctx, int B, int T) {
  if (!ctx || B <= 0 || T <= 0) return VSP_ERR_ARG;
  Ws ws(nullptr, 0, true);
  vc_impl(const_cast<vsp_ctx*>(ctx), nullptr, ws, B, T, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
          nullptr, nullptr, nullptr, nullptr, nullptr);
  return (int64_t)ws.cur;
}

int vsp_voice_conversion(vsp_ctx* ctx, void* stream, int B, int T, const float* y, const int64_t* y_lengths,
                         const int64_t* sid_src, const int64_t* sid_tgt, const float* noise, float* o_hat,
                         uint8_t* y_mask, float* z, float* z_p, float* z_hat, float* m_q, float* logs_q,
                         void* workspace, int64_t workspace_bytes) {
  int rc = check_vc(ctx);
  if (rc) return rc;
  if (B <= 0 || T <= 0 || !y || !y_lengths || !sid_src || !sid_tgt || !noise || !o_hat || !y_mask || !z || !z_p ||
      !z_hat || !workspace)
    return ctx->fail(VSP_ERR_ARG, "vsp_voice_conversion: null or non-positive argument");
  const int64_t need = vsp_voice_conversion_workspace_bytes(ctx, B, T);
  if (workspace_bytes < need)
    return ctx->fail(VSP_ERR_WORKSPACE, "voice conversion workspace too small: %lld < %lld bytes",
                     (long long)workspace_bytes, (long long)need);
  Ws ws(workspace, (size_t)workspace_bytes, false);
  return vc_impl(ctx, (hipStream_t)stream, ws, B, T, y, y_lengths, sid_src, sid_tgt, noise, o_hat, y_mask, z, z_p, z_hat,
                 m_q, logs_q);
}

// ---------------------------------------------------------------------------------- conversion from audio
// Frames of a recording of n samples: host arithmetic (kernels.h, stft_ragged_frames), 0 where there is no frame.
static int convert_geometry(const vsp_ctx* ctx, int hop, int* n_fft) {
  if (!ctx || ctx->cfg.spec_channels <= 1 || hop <= 0) return VSP_ERR_ARG;
  *n_fft = 2 * (ctx->cfg.spec_channels - 1);
  return *n_fft < hop ? VSP_ERR_ARG : VSP_OK;
}

int vsp_convert_frames(const vsp_ctx* ctx, int64_t n_samples, int hop) {
  int n_fft = 0;
  if (convert_geometry(ctx, hop, &n_fft) != VSP_OK || n_samples < 0) return VSP_ERR_ARG;
  const long T = stft_ragged_frames((long)n_samples, n_fft, hop);
  return T > 0x7fffffffL ? VSP_ERR_ARG : (int)T;
}

// frames of the padded shape, or <= 0: the shape the grids and the tensors of a ragged call are sized by
static int convert_t_max(const vsp_ctx* ctx, int B, int L_max, int hop) {
  int n_fft = 0;
  if (convert_geometry(ctx, hop, &n_fft) != VSP_OK || B <= 0 || L_max <= 0 || stft_ragged_tile(n_fft, hop) <= 0) return VSP_ERR_ARG;
  return vsp_convert_frames(ctx, L_max, hop);
}

static int spectrogram_ragged_impl(vsp_ctx* ctx, hipStream_t s, Ws& ws, int B, int L_max, int hop, int T, const float* audio,
                                   int64_t audio_stride, const int64_t* n_samples, float* spec, int64_t* frames) {
  const vsp_config& c = ctx->cfg;
  const int n_fft = 2 * (c.spec_channels - 1);
  Run r{ctx, s, ws};
  T3 F = ws.t3(B, n_fft, T), RI = ws.t3(B, 2 * c.spec_channels, T);
  if (ws.dry) return VSP_OK;
  if (ws.overflow) return ctx->fail(VSP_ERR_WORKSPACE, "ragged spectrogram workspace too small");
  r.chk(launch_stft_frames_ragged(audio, (long)audio_stride, n_samples, F.p, F.bs, F.cs, B, L_max, n_fft, hop, T, s),
        "stft frames ragged");
  ConvArgs a = r.args(ctx->model.stft, F, RI, T, T);     // (the DFT of vsp_spectrogram: same convolution, same plan)
  r.conv(a, B);
  if (r.ok())
    r.chk(launch_stft_magnitude_ragged(RI.p, RI.bs, RI.cs, n_samples, spec, frames, B, L_max, n_fft, hop, c.spec_channels, T, s),
          "stft magnitude ragged");
  return r.rc;
}

int64_t vsp_spectrogram_ragged_workspace_bytes(const vsp_ctx* ctx, int B, int L_max, int hop) {
  const int T = convert_t_max(ctx, B, L_max, hop);
  if (T <= 0) return VSP_ERR_ARG;
  Ws ws(nullptr, 0, true);
  spectrogram_ragged_impl(const_cast<vsp_ctx*>(ctx), nullptr, ws, B, L_max, hop, T, nullptr, 0, nullptr, nullptr, nullptr);
  return (int64_t)ws.cur;
}

int vsp_spectrogram_ragged(vsp_ctx* ctx, void* stream, int B, int L_max, int hop, const float* audio, int64_t audio_stride,
                           const int64_t* n_samples, float* spec, int64_t* frames, void* workspace, int64_t workspace_bytes) {
  if (!ctx) return VSP_ERR_ARG;
  const int T = convert_t_max(ctx, B, L_max, hop);
  if (T <= 0 || !audio || audio_stride < L_max || !n_samples || !spec || !frames || !workspace)
    return ctx->fail(VSP_ERR_ARG, "vsp_spectrogram_ragged: bad argument (needs spec_channels, B > 0, hop > 0, a padded length "
                                  "with at least one frame, audio_stride >= L_max and no null pointer)");
  int rc = check_ready(ctx);
  if (rc) return rc;
  if (workspace_bytes < vsp_spectrogram_ragged_workspace_bytes(ctx, B, L_max, hop))
    return ctx->fail(VSP_ERR_WORKSPACE, "ragged spectrogram workspace too small");
  Ws ws(workspace, (size_t)workspace_bytes, false);
  return spectrogram_ragged_impl(ctx, (hipStream_t)stream, ws, B, L_max, hop, T, audio, audio_stride, n_samples, spec, frames);
}

// Audio to the converted latent: ragged spectrogram -> enc_q(g_src) -> flow(g_src) -> flow(g_tgt, reverse), every stage
// with the rows' own frame counts as lengths (voice_conversion, reference models.py:724-732, up to z_hat).
static int convert_latent_impl(vsp_ctx* ctx, hipStream_t s, Ws& ws, int B, int L_max, int hop, int T, const float* audio,
                               int64_t audio_stride, const int64_t* n_samples, const int64_t* sid_src, const int64_t* sid_tgt,
                               const float* noise, float noise_scale, float* z_hat, float* g_tgt, int64_t* frames,
                               uint8_t* y_mask, float* z, float* z_p) {
  const vsp_config& c = ctx->cfg;
  const Model& m = ctx->model;
  const int inter = c.inter_channels, gin = c.gin_channels;
  const long n = (long)B * inter * T;
  Run r{ctx, s, ws};
  float* g_src = ws.f((size_t)B * gin);
  float* spec = ws.f((size_t)B * c.spec_channels * T);
  float* zq = z ? z : ws.f((size_t)n);
  float* zp = z_p ? z_p : ws.f((size_t)n);
  float* m_q = ws.f((size_t)n);              // (launch_reparam walks contiguous tensors)
  float* logs_q = ws.f((size_t)n);
  float* drawn = ws.f((size_t)n);
  uint64_t* seeds_dev = reinterpret_cast<uint64_t*>(ws.bytes((size_t)B * sizeof(uint64_t)));
  const bool live = !ws.dry && !ws.overflow;
  const size_t mark = ws.cur;                // the stages run one after another on one stream: they share scratch
  int rc = spectrogram_ragged_impl(ctx, s, ws, B, L_max, hop, T, audio, audio_stride, n_samples, spec, frames);
  if (rc) return rc;
  size_t peak = ws.cur;
  ws.cur = mark;
  if (live) {
    r.chk(launch_gather_rows(sid_src, r.A(m.emb_g), c.n_speakers, g_src, B, gin, s), "emb_g");
    r.chk(launch_gather_rows(sid_tgt, r.A(m.emb_g), c.n_speakers, g_tgt, B, gin, s), "emb_g");
    r.chk(launch_mask_u8(frames, y_mask, B, T, s), "y_mask");
    if (noise_scale == 0.f) {
      noise = nullptr;                       // z = m_q: nothing is drawn, nothing is read
    } else if (!noise) {
      // row b's own draw, keyed seeds[b], laid out [inter][T_b] (vsp_set_noise_seeds).  As in vsp_decode's isolated draw:
      // the source is pageable, so the runtime stages it before this call returns (hipMemcpyAsync is asynchronous only for
      // pinned host memory) and a later vsp_set_noise_seeds cannot race the copy; it lands in THIS call's workspace
      r.chk(hipMemcpyAsync(seeds_dev, ctx->noise_seeds.data(), (size_t)B * sizeof(uint64_t), hipMemcpyHostToDevice, s), "noise seeds");
      if (r.ok()) r.chk(launch_randn_ragged(seeds_dev, frames, B, inter, T, drawn, s), "randn_ragged");
      noise = drawn;
    }
  }
  run_posterior(r, B, T, ext(spec, c.spec_channels, T), frames, g_src, noise, ext(zq, inter, T), ext(m_q, inter, T),
                ext(logs_q, inter, T), noise_scale);
  peak = std::max(peak, ws.cur);
  ws.cur = mark;
  if (live && r.ok()) r.chk(hipMemcpyAsync(zp, zq, n * sizeof(float), hipMemcpyDeviceToDevice, s), "z_p copy");
  run_flow(r, B, T, ext(zp, inter, T), g_src, frames, false);
  if (live && r.ok()) r.chk(hipMemcpyAsync(z_hat, zp, n * sizeof(float), hipMemcpyDeviceToDevice, s), "z_hat copy");
  peak = std::max(peak, ws.cur);
  ws.cur = mark;
  run_flow(r, B, T, ext(z_hat, inter, T), g_tgt, frames, true);
  ws.cur = std::max(peak, ws.cur);
  if (ws.overflow) return ctx->fail(VSP_ERR_WORKSPACE, "convert_latent workspace too small (need %zu bytes)", ws.cur);
  return r.rc;
}

int64_t vsp_convert_latent_workspace_bytes(const vsp_ctx* ctx, int B, int L_max, int hop) {
  const int T = convert_t_max(ctx, B, L_max, hop);
  if (T <= 0) return VSP_ERR_ARG;
  Ws ws(nullptr, 0, true);
  convert_latent_impl(const_cast<vsp_ctx*>(ctx), nullptr, ws, B, L_max, hop, T, nullptr, 0, nullptr, nullptr, nullptr, nullptr,
                      1.f, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  return (int64_t)ws.cur;
}

int vsp_convert_latent(vsp_ctx* ctx, void* stream, int B, int L_max, int hop, const float* audio, int64_t audio_stride,
                       const int64_t* n_samples, const int64_t* sid_src, const int64_t* sid_tgt, const float* noise,
                       float noise_scale, float* z_hat, float* g_tgt, int64_t* frames, uint8_t* y_mask, float* z, float* z_p,
                       void* workspace, int64_t workspace_bytes) {
  if (!ctx) return VSP_ERR_ARG;
  const int T = convert_t_max(ctx, B, L_max, hop);
  if (T <= 0 || !audio || audio_stride < L_max || !n_samples || !sid_src || !sid_tgt || !z_hat || !g_tgt || !frames ||
      !y_mask || !workspace || !std::isfinite(noise_scale))
    return ctx->fail(VSP_ERR_ARG, "vsp_convert_latent: bad argument (needs spec_channels, B > 0, hop > 0, a padded length with "
                                  "at least one frame, audio_stride >= L_max, a finite noise_scale and no null pointer)");
  int rc = check_vc(ctx);
  if (rc) return rc;
  if (!noise && noise_scale != 0.f && (int)ctx->noise_seeds.size() != B)
    return ctx->fail(VSP_ERR_STATE, "vsp_convert_latent draws per-row noise: vsp_set_noise_seeds for B = %d first (%d set)", B,
                     (int)ctx->noise_seeds.size());
  const int64_t need = vsp_convert_latent_workspace_bytes(ctx, B, L_max, hop);
  if (workspace_bytes < need)
    return ctx->fail(VSP_ERR_WORKSPACE, "convert_latent workspace too small: %lld < %lld bytes", (long long)workspace_bytes,
                     (long long)need);
  Ws ws(workspace, (size_t)workspace_bytes, false);
  return convert_latent_impl(ctx, (hipStream_t)stream, ws, B, L_max, hop, T, audio, audio_stride, n_samples, sid_src, sid_tgt,
                             noise, noise_scale, z_hat, g_tgt, frames, y_mask, z, z_p);
}

int64_t vsp_generator_workspace_bytes(const vsp_ctx* ctx, int B, int T) {
  if (!ctx || B <= 0 || T <= 0) return VSP_ERR_ARG;
  Ws ws(nullptr, 0, true);
  Run r{const_cast<vsp_ctx*>(ctx), nullptr, ws};
  run_gen(r, B, T, T3{}, nullptr, nullptr, nullptr);
  return (int64_t)ws.cur;
}

int vsp_generator(vsp_ctx* ctx, void* stream, int B, int T, const float* z, const float* g, float* o, void* workspace,
                  int64_t workspace_bytes) {
  int rc = check_ready(ctx);
  if (rc) return rc;
  if (B <= 0 || T <= 0 || !z || !g || !o || !workspace) return ctx->fail(VSP_ERR_ARG, "vsp_generator: bad argument");
  if (workspace_bytes < vsp_generator_workspace_bytes(ctx, B, T))
    return ctx->fail(VSP_ERR_WORKSPACE, "generator workspace too small (need %lld bytes)",
                     (long long)vsp_generator_workspace_bytes(ctx, B, T));
  Ws ws(workspace, (size_t)workspace_bytes, false);
  Run r{ctx, (hipStream_t)stream, ws};
  run_gen(r, B, T, ext(z, ctx->cfg.inter_channels, T), nullptr, g, o);
  if (ws.overflow) return ctx->fail(VSP_ERR_WORKSPACE, "generator workspace too small (need %zu bytes)", ws.cur);
  return r.rc;
}

int vsp_generator_ragged(vsp_ctx* ctx, void* stream, int B, int T, const float* z, const float* g, const int64_t* lengths,
                         float* o, void* workspace, int64_t workspace_bytes) {
  int rc = check_ready(ctx);
  if (rc) return rc;
  if (B <= 0 || T <= 0 || !z || !g || !lengths || !o || !workspace) return ctx->fail(VSP_ERR_ARG, "vsp_generator_ragged: bad argument");
  const int64_t need = vsp_generator_workspace_bytes(ctx, B, T) + (int64_t)B * (int64_t)sizeof(int);
  if (workspace_bytes < need)
    return ctx->fail(VSP_ERR_WORKSPACE, "ragged generator workspace too small (need %lld bytes)", (long long)need);
  Ws ws(workspace, (size_t)workspace_bytes, false);
  Run r{ctx, (hipStream_t)stream, ws};
  r.iso = true;
  run_gen(r, B, T, ext(z, ctx->cfg.inter_channels, T), lengths, g, o);
  if (ws.overflow) return ctx->fail(VSP_ERR_WORKSPACE, "ragged generator workspace too small (need %zu bytes)", ws.cur);
  return r.rc;
}

int vsp_generator_kind(const vsp_ctx* ctx) {
  if (!ctx) return VSP_ERR_ARG;
  return ctx->model.has_cl ? ctx->gen_mode : 0;
}

// Receptive field of the generator in input frames (one side), from the configuration: walking back from conv_post,
// every stage adds the largest ResBlock support (resblock_support) in positions at its rate, every transposed conv maps
// w positions to ceil((w + (k + s) / 2 - 1) / s), conv_pre adds 3.  (14 for configs/config.json; measured 12.33.)
int vsp_generator_halo_frames(const vsp_ctx* ctx) {
  if (!ctx) return VSP_ERR_ARG;
  const vsp_config& c = ctx->cfg;
  long w = 3;   // conv_post k7
  for (int i = c.n_upsamples - 1; i >= 0; --i) {
    long rb = 0;
    for (int j = 0; j < c.n_resblock_kernels; ++j) rb = std::max(rb, resblock_support(c, ctx->resblock, j));
    w += rb;
    const int s = c.upsample_rates[i], k = c.upsample_kernel_sizes[i];
    w = (w + (k + s) / 2 - 1 + s - 1) / s;
  }
  return (int)(w + 3);   // conv_pre k7
}

int vsp_generator_frame_dependence(const vsp_ctx* ctx, int* back, int* fwd) {
  if (!ctx || !back || !fwd) return VSP_ERR_ARG;
  generator_frame_dependence(ctx->cfg, ctx->resblock, ctx->model.g_pre.K > 0 ? ctx->model.g_pre.K : 7, ctx->model.post_k,
                             *back, *fwd);
  return VSP_OK;
}

int64_t vsp_generator_stream_workspace_bytes(const vsp_ctx* ctx, int B, int chunk_frames) {
  if (!ctx || B <= 0 || chunk_frames <= 0) return VSP_ERR_ARG;
  const int span = chunk_frames + 2 * vsp_generator_halo_frames(ctx);
  const int64_t g = vsp_generator_workspace_bytes(ctx, B, span);
  if (g < 0) return g;
  return g + (((int64_t)B * span * total_upsample(ctx->cfg) * (int64_t)sizeof(float) + 255) / 256) * 256;
}

// Streamed vocoder (BASELINE config 5): the waveform of frames [f0, f1) of z [B][inter][T], computed from those frames
// plus the halo on both sides (zero padding only at the true ends) -- bit-identical to the same samples of one
// vsp_generator call over all T frames.  o_chunk [B][1][(f1 - f0) * prod(upsample_rates)], contiguous.
int vsp_generator_stream_chunk(vsp_ctx* ctx, void* stream, int B, int T, const float* z, const float* g, int f0, int f1,
                               float* o_chunk, void* workspace, int64_t workspace_bytes) {
  int rc = check_ready(ctx);
  if (rc) return rc;
  if (B <= 0 || T <= 0 || !z || !g || !o_chunk || !workspace || f0 < 0 || f1 <= f0 || f1 > T)
    return ctx->fail(VSP_ERR_ARG, "vsp_generator_stream_chunk: bad argument");
  const int halo = vsp_generator_halo_frames(ctx);
  const int lo = std::max(0, f0 - halo), hi = std::min(T, f1 + halo), span = hi - lo;
  const long up = total_upsample(ctx->cfg);
  const int64_t gen_bytes = vsp_generator_workspace_bytes(ctx, B, span);
  const int64_t scratch = (((int64_t)B * span * up * (int64_t)sizeof(float) + 255) / 256) * 256;
  if (gen_bytes < 0 || workspace_bytes < gen_bytes + scratch)
    return ctx->fail(VSP_ERR_WORKSPACE, "stream chunk workspace too small (need %lld bytes)", (long long)(gen_bytes + scratch));
  float* o_span = static_cast<float*>(workspace);
  Ws ws(static_cast<char*>(workspace) + scratch, (size_t)(workspace_bytes - scratch), false);
  Run r{ctx, (hipStream_t)stream, ws};
  const int inter = ctx->cfg.inter_channels;
  // the frames [lo, hi) of every channel row: same strides as z, shifted start
  run_gen(r, B, span, T3{const_cast<float*>(z) + lo, (long)inter * T, (long)T}, nullptr, g, o_span);
  if (ws.overflow) return ctx->fail(VSP_ERR_WORKSPACE, "stream chunk workspace too small (need %zu bytes)", ws.cur);
  if (r.rc != VSP_OK) return r.rc;
  hipError_t e = hipMemcpy2DAsync(o_chunk, (size_t)(f1 - f0) * up * sizeof(float), o_span + (size_t)(f0 - lo) * up,
                                  (size_t)span * up * sizeof(float), (size_t)(f1 - f0) * up * sizeof(float), (size_t)B,
                                  hipMemcpyDeviceToDevice, (hipStream_t)stream);
  return e == hipSuccess ? VSP_OK : ctx->fail(VSP_ERR_HIP, "stream chunk copy: %s", hipGetErrorString(e));
}

// Streaming for batched requests: every row its own window of its own utterance, one set of generator launches.
int vsp_stream_rows_plan(const vsp_ctx* ctx, int B, const vsp_stream_row* rows, int32_t* lo, int32_t* hi, int32_t* span_max) {
  if (!ctx || !rows || B < 1 || B > STREAM_ROWS_MAX) return VSP_ERR_ARG;
  const int halo = vsp_generator_halo_frames(ctx);
  int mx = 0;
  for (int b = 0; b < B; ++b) {
    const vsp_stream_row& r = rows[b];
    if (r.f0 < 0 || r.f1 <= r.f0 || r.f1 > r.L) return VSP_ERR_ARG;
    const int l = std::max(0, r.f0 - halo);
    const int h = (int)std::min<int64_t>(r.L, (int64_t)r.f1 + halo);
    if (lo) lo[b] = l;
    if (hi) hi[b] = h;
    mx = std::max(mx, h - l);
  }
  if (span_max) *span_max = mx;
  return VSP_OK;
}

namespace {
// the workspace of a stream_rows call whose longest window is `span` frames: [span waveform | packed z | g rows | lengths |
// generator]; the packed z's row stride is span rounded up to 4 frames (every packed quad is one aligned 16-byte store)
struct StreamRowsWs {
  int64_t o_span, zp, gp, len, gen, total;
  int S4;
};
inline int64_t r256(int64_t n) { return (n + 255) / 256 * 256; }
bool stream_rows_ws(const vsp_ctx* ctx, int B, int span, StreamRowsWs& w) {
  w.S4 = (span + 3) / 4 * 4;
  const int64_t gen = vsp_generator_workspace_bytes(ctx, B, span);
  if (gen < 0) return false;
  w.o_span = 0;
  w.zp = w.o_span + r256((int64_t)B * span * total_upsample(ctx->cfg) * (int64_t)sizeof(float));
  w.gp = w.zp + r256((int64_t)B * ctx->cfg.inter_channels * w.S4 * (int64_t)sizeof(float));
  w.len = w.gp + r256((int64_t)B * ctx->cfg.gin_channels * (int64_t)sizeof(float));
  w.gen = w.len + r256((int64_t)B * (int64_t)sizeof(int64_t));
  w.total = w.gen + gen;
  return true;
}
}  // namespace

int64_t vsp_generator_stream_rows_workspace_bytes(const vsp_ctx* ctx, int B, int chunk_frames) {
  if (!ctx || B < 1 || B > STREAM_ROWS_MAX || chunk_frames <= 0) return VSP_ERR_ARG;
  StreamRowsWs w;
  if (!stream_rows_ws(ctx, B, chunk_frames + 2 * vsp_generator_halo_frames(ctx), w)) return VSP_ERR_ARG;
  return w.total;
}

namespace {
// The gather launch and the generator run of a stream_rows call: the span waveform [B][*span * up] is left at *o_span, row
// b's window starts at frame lo[b].  Every check runs before the first launch.
int stream_rows_generate(vsp_ctx* ctx, hipStream_t s, int B, const vsp_stream_row* rows, int64_t chunk_frames, void* workspace,
                         int64_t workspace_bytes, const char* who, int32_t* lo, float** o_span_out, int32_t* span_out) {
  int32_t hi[STREAM_ROWS_MAX], span = 0;
  if (vsp_stream_rows_plan(ctx, B, rows, lo, hi, &span) != VSP_OK)
    return ctx->fail(VSP_ERR_ARG, "%s: a row is not 0 <= f0 < f1 <= L", who);
  StreamGatherRows gr;
  int64_t span_len[STREAM_ROWS_MAX];
  for (int b = 0; b < B; ++b) {
    const vsp_stream_row& r = rows[b];
    if (!r.z || !r.g || r.z_channel_stride < r.L || r.f1 - r.f0 > chunk_frames)
      return ctx->fail(VSP_ERR_ARG, "%s: row %d: null z / g, channel stride below L, or a chunk of "
                                    "%d frames where out_stride holds %lld", who, b, r.f1 - r.f0, (long long)chunk_frames);
    gr.r[b] = StreamGatherRow{r.z, (long)r.z_channel_stride, r.g, lo[b], hi[b]};
    span_len[b] = hi[b] - lo[b];
  }
  StreamRowsWs w;
  if (!stream_rows_ws(ctx, B, span, w) || workspace_bytes < w.total)
    return ctx->fail(VSP_ERR_WORKSPACE, "stream rows workspace too small (need %lld bytes)", (long long)w.total);
  char* const base = static_cast<char*>(workspace);
  float* const o_span = reinterpret_cast<float*>(base + w.o_span);
  float* const zp = reinterpret_cast<float*>(base + w.zp);
  float* const gp = reinterpret_cast<float*>(base + w.gp);
  int64_t* const len = reinterpret_cast<int64_t*>(base + w.len);
  const int inter = ctx->cfg.inter_channels;
  hipError_t e = launch_stream_gather(gr, B, inter, w.S4, ctx->cfg.gin_channels, zp, gp, len, s);
  if (e != hipSuccess) return ctx->fail(VSP_ERR_HIP, "stream_gather: %s", hipGetErrorString(e));
  Ws ws(base + w.gen, (size_t)(workspace_bytes - w.gen), false);
  Run r{ctx, s, ws};
  r.iso = true;
  // the host knows every window: a tick whose windows are all `span` frames long runs without per-utterance extents
  r.host_lengths = span_len;
  run_gen(r, B, span, T3{zp, (long)inter * w.S4, (long)w.S4}, len, gp, o_span);
  if (ws.overflow) return ctx->fail(VSP_ERR_WORKSPACE, "stream rows workspace too small (need %zu bytes)", (size_t)w.gen + ws.cur);
  if (r.rc != VSP_OK) return r.rc;
  *o_span_out = o_span;
  *span_out = span;
  return VSP_OK;
}
}  // namespace

int vsp_generator_stream_rows(vsp_ctx* ctx, void* stream, int B, const vsp_stream_row* rows, void* out, int64_t out_stride,
                              int pcm, void* workspace, int64_t workspace_bytes) {
  int rc = check_ready(ctx);
  if (rc) return rc;
  const long up = total_upsample(ctx->cfg);
  if (B < 1 || B > STREAM_ROWS_MAX || !rows || !out || !workspace || (pcm != 0 && pcm != 1) || out_stride < up)
    return ctx->fail(VSP_ERR_ARG, "vsp_generator_stream_rows: bad argument (1 <= B <= %d, out_stride >= one frame)", STREAM_ROWS_MAX);
  int32_t lo[STREAM_ROWS_MAX], span = 0;
  float* o_span = nullptr;
  hipStream_t s = (hipStream_t)stream;
  rc = stream_rows_generate(ctx, s, B, rows, out_stride / up, workspace, workspace_bytes, "vsp_generator_stream_rows", lo, &o_span,
                            &span);
  if (rc) return rc;
  StreamCollectRows cr;
  for (int b = 0; b < B; ++b) cr.r[b] = StreamCollectRow{(int)((rows[b].f0 - lo[b]) * up), (int)((rows[b].f1 - rows[b].f0) * up)};
  hipError_t e = launch_stream_collect(o_span, (long)span * up, cr, B, out, (long)out_stride, pcm, s);
  return e == hipSuccess ? VSP_OK : ctx->fail(VSP_ERR_HIP, "stream_collect: %s", hipGetErrorString(e));
}

int vsp_generator_stream_rows_output(vsp_ctx* ctx, void* stream, int B, const vsp_stream_row_out* rows, void* out,
                                     int64_t out_stride, int pcm, void* workspace, int64_t workspace_bytes) {
  int rc = check_ready(ctx);
  if (rc) return rc;
  if (!ctx->out_tab) return ctx->fail(VSP_ERR_STATE, "output stage not configured (vsp_output_configure)");
  if (B < 1 || B > STREAM_ROWS_MAX || !rows || !out || !workspace || (pcm != 0 && pcm != 1) || out_stride < 1)
    return ctx->fail(VSP_ERR_ARG, "vsp_generator_stream_rows_output: bad argument (1 <= B <= %d)", STREAM_ROWS_MAX);
  const int up = (int)total_upsample(ctx->cfg);
  const int L = ctx->out_L, M = ctx->out_M, H = ctx->out_H, K = vsp_output_history_samples(L, M, H);
  vsp_stream_row plain[STREAM_ROWS_MAX];
  int64_t m0[STREAM_ROWS_MAX], m1[STREAM_ROWS_MAX];
  for (int b = 0; b < B; ++b) plain[b] = rows[b].row;
  if (vsp_stream_rows_output_plan(L, M, H, up, B, plain, m0, m1, nullptr, nullptr) != VSP_OK)
    return ctx->fail(VSP_ERR_ARG, "vsp_generator_stream_rows_output: a row is not 0 <= f0 < f1 <= L");
  for (int b = 0; b < B; ++b) {
    const vsp_stream_row_out& r = rows[b];
    if (K > 0 && (!r.hist_out || (r.row.f0 > 0 && !r.hist_in)))
      return ctx->fail(VSP_ERR_ARG, "vsp_generator_stream_rows_output: row %d: null history buffer (%d floats each)", b, K);
    if (r.hist_out && r.hist_in == r.hist_out)
      return ctx->fail(VSP_ERR_ARG, "vsp_generator_stream_rows_output: row %d: hist_in == hist_out", b);
  }
  for (int b = 0; b < B; ++b)
    if (m1[b] - m0[b] > out_stride)
      return ctx->fail(VSP_ERR_SHAPE, "vsp_generator_stream_rows_output: row %d completes %lld output samples, out_stride is %lld "
                                      "(vsp_stream_rows_out_samples)", b, (long long)(m1[b] - m0[b]), (long long)out_stride);
  int32_t lo[STREAM_ROWS_MAX], span = 0;
  float* o_span = nullptr;
  hipStream_t s = (hipStream_t)stream;
  rc = stream_rows_generate(ctx, s, B, plain, INT32_MAX, workspace, workspace_bytes, "vsp_generator_stream_rows_output", lo,
                            &o_span, &span);
  if (rc) return rc;
  StreamOutRows orows;
  for (int b = 0; b < B; ++b) {
    const vsp_stream_row& r = plain[b];
    // (a first chunk has no history: whatever the caller left in hist_in is not passed on)
    orows.r[b] = StreamOutRow{r.f0 > 0 ? rows[b].hist_in : nullptr, rows[b].hist_out, (int64_t)r.f0 * up, (int)((r.f0 - lo[b]) * up),
                              (int)((r.f1 - r.f0) * up), r.f1 == r.L, 0};
  }
  const StreamOutFilter f{ctx->out_tab, L, M, H, ctx->out_J, ctx->out_P};
  hipError_t e = launch_stream_output(o_span, (long)span * up, orows, B, f, K, out, (long)out_stride, pcm, s);
  return e == hipSuccess ? VSP_OK : ctx->fail(VSP_ERR_HIP, "stream_output: %s", hipGetErrorString(e));
}

int vsp_rq_spline(void* stream, int64_t n, int nb, const float* x, const float* uw, const float* uh, const float* ud,
                  int inverse, float tail_bound, float* y, float* logabsdet) {
  if (n < 0 || !x || !uw || !uh || !ud || !y || !logabsdet) return VSP_ERR_ARG;
  hipError_t e = launch_rq_spline(n, nb, x, uw, uh, ud, inverse, tail_bound, y, logabsdet, (hipStream_t)stream);
  return e == hipSuccess ? VSP_OK : (e == hipErrorInvalidValue ? VSP_ERR_UNSUPPORTED : VSP_ERR_HIP);
}

// -------------------------------------------------------------------------------------------- mel spectrogram
namespace {
// librosa.filters.mel with its defaults (htk = False, norm = 'slaney'), in double precision
bool mel_basis(int sr, int n_fft, int n_mels, double fmin, double fmax, std::vector<float>& w) {
  if (sr <= 0 || n_fft < 2 || (n_fft & 1) || n_mels < 1) return false;
  if (fmax <= 0.0) fmax = sr / 2.0;
  if (fmin < 0.0 || fmax <= fmin) return false;
  const int nf = n_fft / 2 + 1;
  const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
  auto hz_to_mel = [&](double f) { return f >= min_log_hz ? min_log_mel + std::log(f / min_log_hz) / logstep : f / f_sp; };
  auto mel_to_hz = [&](double m) { return m >= min_log_mel ? min_log_hz * std::exp(logstep * (m - min_log_mel)) : f_sp * m; };
  std::vector<double> mel_f(n_mels + 2);
  const double m0 = hz_to_mel(fmin), m1 = hz_to_mel(fmax);
  for (int i = 0; i < n_mels + 2; ++i) mel_f[i] = mel_to_hz(m0 + (m1 - m0) * i / (n_mels + 1));
  w.assign((size_t)n_mels * nf, 0.f);
  for (int m = 0; m < n_mels; ++m) {
    const double enorm = 2.0 / (mel_f[m + 2] - mel_f[m]);
    for (int k = 0; k < nf; ++k) {
      const double f = (sr / 2.0) * k / (nf - 1);
      const double lower = (f - mel_f[m]) / (mel_f[m + 1] - mel_f[m]), upper = (mel_f[m + 2] - f) / (mel_f[m + 2] - mel_f[m + 1]);
      const double v = std::max(0.0, std::min(lower, upper));
      w[(size_t)m * nf + k] = (float)(v * enorm);
    }
  }
  return true;
}
}  // namespace

int vsp_mel_filterbank(int sampling_rate, int n_fft, int n_mels, float fmin, float fmax, float* basis_host) {
  if (!basis_host) return VSP_ERR_ARG;
  std::vector<float> w;
  if (!mel_basis(sampling_rate, n_fft, n_mels, fmin, fmax, w)) return VSP_ERR_ARG;
  std::memcpy(basis_host, w.data(), w.size() * sizeof(float));
  return VSP_OK;
}

int vsp_spec_to_mel(void* stream, int B, int T, int n_fft, int n_mels, int sampling_rate, float fmin, float fmax,
                    const float* spec, float* mel) {
  if (!spec || !mel || B < 0 || T < 0) return VSP_ERR_ARG;
  std::vector<float> w;
  if (!mel_basis(sampling_rate, n_fft, n_mels, fmin, fmax, w)) return VSP_ERR_ARG;
  if (B == 0 || T == 0) return VSP_OK;
  const int nf = n_fft / 2 + 1;
  std::vector<int> lo(n_mels), hi(n_mels);
  for (int m = 0; m < n_mels; ++m) {
    int a = nf, b = 0;
    for (int k = 0; k < nf; ++k)
      if (w[(size_t)m * nf + k] != 0.f) { a = std::min(a, k); b = k + 1; }
    lo[m] = a < b ? a : 0; hi[m] = a < b ? b : 0;
  }
  hipStream_t s = (hipStream_t)stream;
  void *dw = nullptr, *dr = nullptr;
  hipError_t e = hipMalloc(&dw, w.size() * 4);
  if (e == hipSuccess) e = hipMalloc(&dr, (size_t)2 * n_mels * 4);
  if (e == hipSuccess) e = hipMemcpyAsync(dw, w.data(), w.size() * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(dr, lo.data(), (size_t)n_mels * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(static_cast<int*>(dr) + n_mels, hi.data(), (size_t)n_mels * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess)
    e = launch_spec_to_mel(spec, static_cast<const float*>(dw), static_cast<const int*>(dr), static_cast<const int*>(dr) + n_mels,
                           mel, B, nf, n_mels, T, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);      // (the host vectors and the scratch die with this frame)
  if (dw) (void)hipFree(dw);
  if (dr) (void)hipFree(dr);
  return e == hipSuccess ? VSP_OK : VSP_ERR_HIP;
}

// -------------------------------------------------------------------------------------------- profiling
int vsp_profile_enable(vsp_ctx* ctx, int on) {
  if (!ctx) return VSP_ERR_ARG;
  if (on && !ctx->prof_on) {          // a fresh measurement: forget whatever an earlier one left unread
    ctx->ev_used = 0;
    for (int c = 0; c < VSP_PROF_CLASSES; ++c) {
      ctx->prof_launches[c] = 0;
      ctx->prof_flops[c] = ctx->prof_bytes[c] = ctx->prof_bytes_ext[c] = ctx->prof_bytes_moved[c] = 0.0;
    }
  }
  ctx->prof_on = on != 0;
  return VSP_OK;
}

int vsp_profile_read_class(vsp_ctx* ctx, int cls, int64_t* launches, double* total_ms, double* total_flops,
                           double* total_bytes, double* total_bytes_ext, double* total_bytes_moved, int reset) {
  if (!ctx || cls < 0 || cls >= VSP_PROF_CLASSES || !launches || !total_ms || !total_flops || !total_bytes)
    return ctx ? ctx->fail(VSP_ERR_ARG, "vsp_profile_read_class: bad argument") : VSP_ERR_ARG;
  double ms = 0.0;
  for (size_t i = 0; i + 1 < ctx->ev_used; i += 2) {
    if (ctx->ev_cls[i / 2] != cls) continue;
    hipError_t e = hipEventSynchronize(ctx->ev_pool[i + 1]);
    float t = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&t, ctx->ev_pool[i], ctx->ev_pool[i + 1]);
    if (e != hipSuccess) return ctx->fail(VSP_ERR_HIP, "profile events: %s", hipGetErrorString(e));
    ms += t;
  }
  *launches = ctx->prof_launches[cls];
  *total_ms = ms;
  *total_flops = ctx->prof_flops[cls];
  *total_bytes = ctx->prof_bytes[cls];
  if (total_bytes_ext) *total_bytes_ext = ctx->prof_bytes_ext[cls];
  if (total_bytes_moved) *total_bytes_moved = ctx->prof_bytes_moved[cls];
  if (reset) {
    // the event pool is shared: drop every class's events only when the LAST class has been read; a reset of one
    // class zeroes its counters and marks its pairs as consumed
    ctx->prof_launches[cls] = 0;
    ctx->prof_flops[cls] = ctx->prof_bytes[cls] = ctx->prof_bytes_ext[cls] = ctx->prof_bytes_moved[cls] = 0.0;
    bool any = false;
    for (size_t i = 0; i + 1 < ctx->ev_used; i += 2) {
      if (ctx->ev_cls[i / 2] == cls) ctx->ev_cls[i / 2] = -1;
      else if (ctx->ev_cls[i / 2] >= 0) any = true;
    }
    if (!any) ctx->ev_used = 0;
  }
  return VSP_OK;
}

int vsp_profile_read_families(vsp_ctx* ctx, int cls, int max_families, int* family, int64_t* launches, double* total_ms,
                              double* total_flops, double* total_bytes, double* total_bytes_moved) {
  if (!ctx || cls < 0 || cls >= VSP_PROF_CLASSES || max_families < 0 || !family || !launches || !total_ms || !total_flops ||
      !total_bytes)
    return ctx ? ctx->fail(VSP_ERR_ARG, "vsp_profile_read_families: bad argument") : VSP_ERR_ARG;
  int n = 0;
  for (size_t i = 0; i + 1 < ctx->ev_used; i += 2) {
    if (ctx->ev_cls[i / 2] != cls) continue;
    hipError_t e = hipEventSynchronize(ctx->ev_pool[i + 1]);
    float t = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&t, ctx->ev_pool[i], ctx->ev_pool[i + 1]);
    if (e != hipSuccess) return ctx->fail(VSP_ERR_HIP, "profile events: %s", hipGetErrorString(e));
    const int f = ctx->ev_fam[i / 2];
    int k = 0;
    while (k < n && family[k] != f) ++k;
    if (k == n) {
      if (n == max_families) continue;
      family[n] = f; launches[n] = 0; total_ms[n] = total_flops[n] = total_bytes[n] = 0.0;
      if (total_bytes_moved) total_bytes_moved[n] = 0.0;
      ++n;
    }
    launches[k] += 1;
    total_ms[k] += t;
    total_flops[k] += ctx->ev_flops[i / 2];
    total_bytes[k] += ctx->ev_bytes[i / 2];
    if (total_bytes_moved) total_bytes_moved[k] += ctx->ev_moved[i / 2];
  }
  return n;
}

int vsp_profile_read(vsp_ctx* ctx, int64_t* launches, double* total_ms, double* total_flops, double* total_bytes,
                     int reset) {
  return vsp_profile_read_class(ctx, VSP_PROF_GENERATOR, launches, total_ms, total_flops, total_bytes, nullptr, nullptr, reset);
}

}  // extern "C"
