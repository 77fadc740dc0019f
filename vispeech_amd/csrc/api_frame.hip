// The frame-rate launch sequences (api_common.h): encoder, WN, flow and posterior encoder, and on them vsp_encode,
// vsp_decode, the one-call vsp_infer and the per-stage entry points.
#include "api_common.h"

using namespace vsp;

namespace vsp {

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

// Layer l of modules.WN.forward on the residual stream H: ACT = gate(in_layers[l](H) + cond), then res_skip_layers[l]
// (modules.py:165-172) as one launch with two destinations -- rows [0, h) are the in-place residual update
// H = (H + res) * mask, rows [h, 2 h) go to the skip sum OUT -- or, in the last layer, its skip rows alone.
// rs: that layer's res_skip convolution; acc: OUT already holds the layers before.
static void wn_layer(Run& r, const Conv& in, const Conv& rs, bool last, int B, int T, T3 H, T3 ACT, T3 OUT, const float* cond,
                     long cond_bs, const int64_t* lengths, bool acc) {
  ConvArgs a = r.args(in, H, ACT, T, T);
  a.act = 2; a.cond = cond; a.cond_bs = cond_bs;
  r.conv(a, B);
  a = r.args(rs, ACT, last ? OUT : H, T, T);
  a.lengths = lengths; a.mask_post = 1;
  if (last) a.acc_prev = acc;
  else {
    a.res = H.p; a.r_bs = H.bs; a.r_cs = H.cs;
    a.split_row = r.ctx->cfg.hidden_channels; a.out2 = OUT.p; a.o2_bs = OUT.bs; a.o2_cs = OUT.cs; a.acc_prev2 = acc;
  }
  r.conv(a, B);
}

// modules.WN.forward (reference modules.py:148-176; dilation_rate 1) on H [B][h][T]: H is the running
// residual stream (destroyed), OUT receives the masked skip sum.  gc: nl * 2h conditioning rows.
// cond != null: cond_layer(g) is evaluated here into gc [B][nl * 2h]; null: gc already holds it, batch stride gc_bs.
void run_wn(Run& r, const Conv* cond, const std::vector<Conv>& in, const std::vector<Conv>& res,
            const std::vector<Conv>& skip, int nl, int B, int T, T3 H, T3 ACT, T3 OUT, float* gc, long gc_bs, const float* g,
            const int64_t* lengths) {
  const int h = r.ctx->cfg.hidden_channels;
  if (cond) r.cond(*cond, g, gc, B);
  for (int l = 0; l < nl; ++l)
    wn_layer(r, in[l], l < nl - 1 ? res[l] : skip[l], l == nl - 1, B, T, H, ACT, OUT, gc ? gc + (size_t)l * 2 * h : nullptr, gc_bs,
             lengths, l > 0);
}

// ResidualCouplingBlock.forward in place on z [B][inter][T] (reference models.py:202-209,
// modules.py:324-343, 148-176).  reverse: x1 = (x1 - m) * mask, layers n-1 .. 0 (infer);
// forward: x1 = m + x1 * mask, layers 0 .. n-1 (voice conversion).  With an even number of flows
// layer i sees the same channel flip in both directions (i and n - i flips).
void run_flow(Run& r, int B, int T, T3 z, const float* g, const int64_t* lengths, bool reverse) {
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
                   T3 M, T3 LOGS, float noise_scale) {
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

// Row b's own draw, keyed ctx->noise_seeds[b] (vsp_set_noise_seeds; the caller has checked that there are B), laid out
// [C][lengths[b]] in row b of drawn [B][C][T] -- what a B = 1 call with T = lengths[b] and that seed draws.
// seeds_dev: B words of THIS call's workspace, not context memory the next call overwrites.  The source is pageable, so
// the runtime reads it into its own staging memory before the copy returns (hipMemcpyAsync is asynchronous only for
// pinned host memory): a later vsp_set_noise_seeds may replace the vector while the copy is still queued on the stream.
void draw_noise_rows(Run& r, uint64_t* seeds_dev, const int64_t* lengths, int B, int C, int T, float* drawn) {
  r.chk(hipMemcpyAsync(seeds_dev, r.ctx->noise_seeds.data(), (size_t)B * sizeof(uint64_t), hipMemcpyHostToDevice, r.s), "noise seeds");
  if (r.ok()) r.chk(launch_randn_ragged(seeds_dev, lengths, B, C, T, drawn, r.s), "randn_ragged");
}

}  // namespace vsp

namespace {
// The tensors and scalars of a sequence as its entry point receives them; the sizing pass hands in an empty one.
struct EncodeIO {
  const int64_t *phonemes, *lengths, *sid;
  const float *dctl, *pctl, *ectl;
  float dscale, pscale, escale, *duration, *f0, *energy;
  int64_t* frame_lengths;
  float *x_var, *g; int32_t* cum_dur;                 // (the one-call form: in its workspace)
};
struct DecodeIO {
  const int64_t* frame_lengths;
  const float* noise; uint64_t noise_seed; float noise_scale;
  float* o; uint8_t* x_mask;
  float *z, *z_p, *m_p, *logs_p;
  const float *x_var, *g; const int32_t* cum_dur;     // (the one-call form: in its workspace)
};
struct InferIO { EncodeIO enc; DecodeIO dec; };
struct WnLayerIO { float* x; const float* g; const int64_t* lengths; float* skip; int accumulate; };
}  // namespace

extern "C" {

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

static void encode_impl(Run& r, int B, int Tp, const EncodeIO& io, bool early_copy = true) {
  vsp_ctx* const ctx = r.ctx; const hipStream_t s = r.s; Ws& ws = r.ws;
  const auto [phonemes, lengths, sid, dctl, pctl, ectl, dscale, pscale, escale, duration, f0, energy, frame_lengths, x_var, g,
              cum_dur] = io;
  const vsp_config& c = ctx->cfg;
  const Model& m = ctx->model;
  const int h = c.hidden_channels, gin = c.gin_channels;
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
  return dry_bytes(ctx, [&](Run& r) { encode_impl(r, B, Tp, EncodeIO{}); });
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
  const EncodeIO io{phonemes, lengths, sid, duration_ctl, pitch_ctl, energy_ctl, duration_scale, pitch_scale, energy_scale,
                    duration, f0, energy, frame_lengths, x_var, g, cum_dur};
  return run_sized(ctx, stream, "encode", vsp_encode_workspace_bytes(ctx, B, Tp), workspace, workspace_bytes,
                   [&](Run& r) { encode_impl(r, B, Tp, io); });
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
static void decode_impl(Run& r, int B, int Tp, int Tf, int max_len, const DecodeIO& io) {
  vsp_ctx* const ctx = r.ctx; const hipStream_t s = r.s; Ws& ws = r.ws;
  auto [frame_lengths, noise, noise_seed, noise_scale, o, x_mask, z, z_p, m_p, logs_p, x_var, g, cum_dur] = io;
  const vsp_config& c = ctx->cfg;
  const Model& m = ctx->model;
  const int h = c.hidden_channels, inter = c.inter_channels;
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
    if ((int)ctx->noise_seeds.size() != B) {
      r.rc = ctx->fail(VSP_ERR_STATE, "isolated mode draws per-utterance noise: vsp_set_noise_seeds for B = %d first (%d set)",
                       B, (int)ctx->noise_seeds.size());
      return;
    }
    draw_noise_rows(r, seeds_dev, frame_lengths, B, inter, Tf, drawn);
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
}

int64_t vsp_decode_workspace_bytes(const vsp_ctx* ctx, int B, int Tp, int Tf) {
  if (!ctx || B <= 0 || Tp <= 0 || Tf <= 0) return VSP_ERR_ARG;
  return dry_bytes(ctx, [&](Run& r) { decode_impl(r, B, Tp, Tf, -1, DecodeIO{}); });
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
  const DecodeIO io{frame_lengths, noise, noise_seed, noise_scale, o, x_mask, z, z_p, m_p, logs_p, x_var, g, cum_dur};
  return run_sized(ctx, stream, "decode", vsp_decode_workspace_bytes(ctx, B, Tp, Tf), workspace, workspace_bytes,
                   [&](Run& r) { decode_impl(r, B, Tp, Tf, max_len, io); });
}

// one-call form: encode + decode with a caller-supplied frame padding, no host synchronisation; what the first half hands
// to the second (x_var, g, cum_dur) lives in the workspace, behind it the two halves share scratch
static void infer_impl(Run& r, int B, int Tp, int Tf, int max_len, InferIO io) {
  const vsp_config& c = r.ctx->cfg;
  Ws& ws = r.ws;
  io.dec.x_var = io.enc.x_var = ws.f((size_t)B * c.hidden_channels * Tp);
  io.dec.g = io.enc.g = ws.f((size_t)B * c.gin_channels);
  io.dec.cum_dur = io.enc.cum_dur = (int32_t*)ws.bytes((size_t)B * Tp * sizeof(int32_t));
  Overlay stages(ws);
  encode_impl(r, B, Tp, io.enc, /*early_copy=*/false);
  stages.next();
  if (r.rc == VSP_OK) decode_impl(r, B, Tp, Tf, max_len, io.dec);
}

int64_t vsp_infer_workspace_bytes(const vsp_ctx* ctx, int B, int Tp, int tf_pad) {
  if (!ctx || B <= 0 || Tp <= 0 || tf_pad <= 0) return VSP_ERR_ARG;
  return dry_bytes(ctx, [&](Run& r) { infer_impl(r, B, Tp, tf_pad, -1, InferIO{}); });
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
  // (x_var, g and cum_dur, the last three of either half, are infer_impl's to set)
  const InferIO io{{phonemes, lengths, sid, duration_ctl, pitch_ctl, energy_ctl, duration_scale, pitch_scale, energy_scale, duration,
                    f0, energy, frame_lengths},
                   {frame_lengths, noise, noise_seed, noise_scale, o, x_mask, z, z_p, m_p, logs_p}};
  return run_sized(ctx, stream, "infer", vsp_infer_workspace_bytes(ctx, B, Tp, tf_pad), workspace, workspace_bytes,
                   [&](Run& r) { infer_impl(r, B, Tp, tf_pad, max_len, io); });
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
  return run_sized(ctx, stream, "attention", vsp_attention_workspace_bytes(ctx, B, T), workspace, workspace_bytes, [&](Run& r) {
    const vsp_config& c = ctx->cfg;
    const int h = c.hidden_channels;
    const EncLayer& L = E.layers[layer];
    if (ctx->att_f16s)   // (the kernel lays the whole workspace out itself)
      r.chk(launch_attention_f16s(qkv, 3L * h * T, T, ctx->arena + L.ek, ctx->arena + L.ev, lengths, out, (long)h * T, T, B, h,
                                  c.n_heads, T, c.window_size, workspace, r.s), "attention");
    else
      r.chk(launch_attention(qkv, 3L * h * T, T, ctx->arena + L.ek, ctx->arena + L.ev, lengths, out, (long)h * T, T,
                             B, h, c.n_heads, T, c.window_size, ctx->att_ksplit, r.s), "attention");
  });
}

// the reference call sites pass x * x_mask (models.py:173, 469, 511): mask a private copy
static void encoder_seq(Run& r, int which, int B, int T, T3 x, const int64_t* lengths, T3 y) {
  const int h = r.ctx->cfg.hidden_channels;
  T3 XI = r.ws.t3(B, h, T);
  if (!r.dry() && r.ok()) r.chk(launch_copy3(x.p, x.bs, x.cs, XI.p, XI.bs, XI.cs, B, h, T, r.s), "copy");
  mask3(r, XI, lengths, B, h, T);
  run_encoder_masked(r, r.ctx->model.enc[which], B, T, XI, lengths, y);
}

int64_t vsp_encoder_workspace_bytes(const vsp_ctx* ctx, int B, int T) {
  if (!ctx || B <= 0 || T <= 0) return VSP_ERR_ARG;
  return dry_bytes(ctx, [&](Run& r) { encoder_seq(r, 0, B, T, T3{}, nullptr, T3{}); });
}

int vsp_encoder(vsp_ctx* ctx, void* stream, int which, int B, int T, const float* x, const int64_t* lengths, float* y,
                void* workspace, int64_t workspace_bytes) {
  int rc = check_ready(ctx);
  if (rc) return rc;
  if (which < 0 || which > 2 || B <= 0 || T <= 0 || !x || !lengths || !y || !workspace)
    return ctx->fail(VSP_ERR_ARG, "vsp_encoder: bad argument");
  const int h = ctx->cfg.hidden_channels;
  return run_sized(ctx, stream, "encoder", vsp_encoder_workspace_bytes(ctx, B, T), workspace, workspace_bytes,
                   [&](Run& r) { encoder_seq(r, which, B, T, ext(x, h, T), lengths, ext(y, h, T)); });
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
  return dry_bytes(ctx, [&](Run& r) { run_flow(r, B, Tf, T3{}, nullptr, nullptr); });
}

// the flow of z_in into z_out (the sequence transforms in place)
static int flow_entry(vsp_ctx* ctx, void* stream, int B, int Tf, const float* z_in, const float* g, const int64_t* frame_lengths,
                      float* z_out, bool reverse, void* workspace, int64_t workspace_bytes) {
  return run_sized(ctx, stream, "flow", vsp_flow_workspace_bytes(ctx, B, Tf), workspace, workspace_bytes, [&](Run& r) {
    const long n = (long)B * ctx->cfg.inter_channels * Tf;
    r.chk(hipMemcpyAsync(z_out, z_in, n * sizeof(float), hipMemcpyDeviceToDevice, r.s), "z copy");
    run_flow(r, B, Tf, ext(z_out, ctx->cfg.inter_channels, Tf), g, frame_lengths, reverse);
  });
}

int vsp_flow_reverse(vsp_ctx* ctx, void* stream, int B, int Tf, const float* z_p, const float* g,
                     const int64_t* frame_lengths, float* z, void* workspace, int64_t workspace_bytes) {
  int rc = check_ready(ctx);
  if (rc) return rc;
  if (B <= 0 || Tf <= 0 || !z_p || !g || !frame_lengths || !z || !workspace)
    return ctx->fail(VSP_ERR_ARG, "vsp_flow_reverse: bad argument");
  return flow_entry(ctx, stream, B, Tf, z_p, g, frame_lengths, z, true, workspace, workspace_bytes);
}

int vsp_flow_forward(vsp_ctx* ctx, void* stream, int B, int Tf, const float* z, const float* g,
                     const int64_t* frame_lengths, float* z_p, void* workspace, int64_t workspace_bytes) {
  int rc = check_ready(ctx);
  if (rc) return rc;
  if (B <= 0 || Tf <= 0 || !z || !g || !frame_lengths || !z_p || !workspace)
    return ctx->fail(VSP_ERR_ARG, "vsp_flow_forward: bad argument");
  return flow_entry(ctx, stream, B, Tf, z, g, frame_lengths, z_p, false, workspace, workspace_bytes);
}

// One layer of modules.WN.forward (reference modules.py:148-176), for unit parity: which 0 .. n_flows-1 = the WN of
// flow.flows[2 * which], -1 = enc_q.enc.
static void wn_layer_impl(Run& r, int which, int layer, int B, int T, const WnLayerIO& io) {
  const auto [x, g, lengths, skip, accumulate] = io;
  const vsp_config& c = r.ctx->cfg;
  const Model& m = r.ctx->model;
  const int h = c.hidden_channels;
  const bool post = which < 0;
  const Conv& cond = post ? m.enc_q.cond : m.flows[which].cond;
  const std::vector<Conv>& in = post ? m.enc_q.in : m.flows[which].in;
  const std::vector<Conv>& res = post ? m.enc_q.res : m.flows[which].res;
  const std::vector<Conv>& sk = post ? m.enc_q.skip : m.flows[which].skip;
  const int nl = post ? c.posterior_layers : c.flow_layers;
  T3 ACT = r.ws.t3(B, h, T);
  float* gc = r.ws.f((size_t)B * 2 * h * nl);
  if (r.dry() || r.ws.overflow) return;
  r.cond(cond, g, gc, B);                              // cond_layer(g): all layers' rows, this layer's slice is used
  wn_layer(r, in[layer], layer < nl - 1 ? res[layer] : sk[layer], layer == nl - 1, B, T, ext(x, h, T), ACT, ext(skip, h, T),
           gc + (size_t)layer * 2 * h, 2L * h * nl, lengths, accumulate != 0);
}

int64_t vsp_wn_layer_workspace_bytes(const vsp_ctx* ctx, int which, int B, int T) {
  if (!ctx || B <= 0 || T <= 0 || which < -1 || which >= ctx->cfg.n_flows) return VSP_ERR_ARG;
  if (which < 0 && ctx->cfg.spec_channels <= 0) return VSP_ERR_ARG;
  return dry_bytes(ctx, [&](Run& r) { wn_layer_impl(r, which, 0, B, T, WnLayerIO{}); });
}

int vsp_wn_layer(vsp_ctx* ctx, void* stream, int which, int layer, int B, int T, float* x, const float* g,
                 const int64_t* lengths, float* skip, int accumulate, void* workspace, int64_t workspace_bytes) {
  int rc = which < 0 ? check_vc(ctx) : check_ready(ctx);
  if (rc) return rc;
  if (which < -1 || which >= ctx->cfg.n_flows || B <= 0 || T <= 0 || !x || !g || !lengths || !skip || !workspace || x == skip)
    return ctx->fail(VSP_ERR_ARG, "vsp_wn_layer: bad argument");
  const int nl = which < 0 ? ctx->cfg.posterior_layers : ctx->cfg.flow_layers;
  if (layer < 0 || layer >= nl) return ctx->fail(VSP_ERR_ARG, "vsp_wn_layer: no such layer");
  const WnLayerIO io{x, g, lengths, skip, accumulate};
  return run_sized(ctx, stream, "wn layer", vsp_wn_layer_workspace_bytes(ctx, which, B, T), workspace, workspace_bytes,
                   [&](Run& r) { wn_layer_impl(r, which, layer, B, T, io); });
}

}  // extern "C"
