// The generator's launch sequences (api_common.h): Generator.forward on the f32 kernels and on the channels-last split-f16
// kernels, the ResBlock schedule (plan_resblock), and on them vsp_generator* and the streamed vocoder.
#include "api_common.h"

using namespace vsp;

namespace {

inline int64_t r256(int64_t n) { return (n + 255) / 256 * 256; }

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

// Support of the layers from stage `first` up to (not including) stage `end`, sample-exact from the configuration: an impulse
// at position 0 of stage first's INPUT tensor reaches positions [lo, hi] of stage end - 1's output, `up` of them per input
// position.  first == 0 starts in front of conv_pre, which widens the support by its padding; a transposed convolution
// (k, s, p) maps [lo, hi] to [lo s - p, hi s - p + k - 1]; a stage's ResBlocks widen it by max_k of the block's support
// (resblock_support); end == n_upsamples includes conv_post, which widens it by its padding.
void generator_support(const vsp_config& c, int resblock, int pre_k, int post_k, int first, int end, long& lo, long& hi, long& up) {
  lo = hi = 0; up = 1;
  if (first == 0) { lo = -(pre_k - 1) / 2; hi = (pre_k - 1) / 2; }
  for (int i = first; i < end && i < c.n_upsamples; ++i) {
    const long s = c.upsample_rates[i], k = c.upsample_kernel_sizes[i], p = (k - s) / 2;
    lo = lo * s - p; hi = hi * s - p + k - 1; up *= s;
    long rb = 0;
    for (int j = 0; j < c.n_resblock_kernels; ++j) rb = std::max(rb, resblock_support(c, resblock, j));
    lo -= rb; hi += rb;
  }
  if (end >= c.n_upsamples) { lo -= (post_k - 1) / 2; hi += (post_k - 1) / 2; }
}

long total_upsample(const vsp_config& c) {
  long u = 1;
  for (int i = 0; i < c.n_upsamples; ++i) u *= c.upsample_rates[i];
  return u;
}

// Exact dependence of the generator's output FRAMES on its input frames (vsp_generator_halo_frames below is the coarser
// per-stage bound the streamed vocoder uses): output frame F depends on input frames [F - back, F + fwd].
void generator_frame_dependence(const vsp_config& c, int resblock, int pre_k, int post_k, int& back, int& fwd) {
  long lo, hi, up;
  generator_support(c, resblock, pre_k, post_k, 0, c.n_upsamples, lo, hi, up);
  // output frame F = samples [up F, up F + up - 1] depends on input frames f with up f + lo <= n <= up f + hi
  back = (int)(hi / up);                     // F - floor(hi / up)
  fwd = (int)((up - 1 - lo) / up);           // F + floor((up - 1 - lo) / up)
}

// The two extents of the silence table (kernels.h): output frame F depends on frames up to F + reach1 of stage 0's OUTPUT
// tensor (up-convolution 1 .. conv_post; 2 for configs/config.json), and frame G of that tensor on input frames up to
// G + fwd0 (conv_pre and stage 0; 11).  With `per` stage-0 columns per frame and `up1` samples per column, output frame F
// = samples [per up1 F, per up1 (F + 1)) depends on columns c with up1 c + lo <= n: the last one is
// per F + floor((per up1 - 1 - lo) / up1), which lies in frame F + floor((per up1 - 1 - lo) / (per up1)).
// A generator of one stage has nothing behind stage 0: reach1 = fwd + 1 then (the whole extent; nothing to gain).
void generator_tail_reach(const vsp_config& c, int resblock, int pre_k, int post_k, int& reach1, int& fwd0) {
  int back = 0, fwd = 0;
  generator_frame_dependence(c, resblock, pre_k, post_k, back, fwd);
  reach1 = fwd + 1; fwd0 = fwd;
  if (c.n_upsamples < 2) return;
  const long total = total_upsample(c);
  long lo, hi, up;
  generator_support(c, resblock, pre_k, post_k, 1, c.n_upsamples, lo, hi, up);
  reach1 = std::max(1, (int)((total - 1 - lo) / total));
  generator_support(c, resblock, pre_k, post_k, 0, 1, lo, hi, up);
  fwd0 = (int)((up - 1 - lo) / up);
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
  // Silence table (round 18; model.h, kernels.h): an utterance whose g is a row of emb_g takes the steady frame and the
  // tensor end from the context's table, so stages 1 .. conv_post end it at len + back + reach1 frames (glen1) -- the
  // transition frames [len, len + back) see stage 0's output no further -- while conv_pre's successors in stage 0 keep
  // glen0 = len + back + 1 + fwd: stage 0's output is then exact up to frame glen0 - 1 - fwd0 >= len + back + reach1 - 1
  // (tail_table_build checks fwd0 + reach1 <= fwd + 1).  Eligible: len + back + fwd <= T -- exactly when no frame before
  // len + back sees the true tensor end, so everything from frame len + back on is the zero input's response.
  // (both arrays are part of the workspace whether the table exists or not)
  int* glen1_all = reinterpret_cast<int*>(r.ws.bytes((size_t)B * sizeof(int)));
  int* tail_row = reinterpret_cast<int*>(r.ws.bytes((size_t)B * sizeof(int)));
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
  // the table serves this call when it was built for these extents (a context whose weights changed has none)
  const float* const table = r.ctx->tail_table;
  const bool tabled = trim && !iso && table && r.ctx->tail_back == back && r.ctx->tail_fwd == fwd;
  const int* glen1 = tabled ? glen1_all : glen_all;   // the extent of stage 1 .. conv_post
  if (trim && !r.dry() && r.ok()) {
    if (tabled)
      r.chk(launch_gen_tail_rows(g, r.A(m.emb_g), c.n_speakers, c.gin_channels, B, tail_row, r.s), "gen_tail_rows");
    r.chk(iso ? launch_gen_plan_isolated(in_lengths, B, T, glen_all, r.s)
              : launch_gen_plan(in_lengths, B, T, back, fwd, tabled ? r.ctx->tail_reach1 : fwd + 1, tabled ? tail_row : nullptr,
                                glen_all, glen1_all, r.s),
          "gen_plan");
  }
  // profiled (untimed) passes charge every launch the frames it COMPUTES, in the stage it belongs to: read the plan back
  // (a host wait -- profiling only)
  std::vector<int> glen_host, glen1_host;
  if (trim && r.ctx->prof_on && !r.dry() && r.ok()) {
    glen_host.resize(B);
    glen1_host.resize(B);
    hipError_t e = hipMemcpyAsync(glen_host.data(), glen_all, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, r.s);
    if (e == hipSuccess) e = hipMemcpyAsync(glen1_host.data(), glen1, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, r.s);
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
      // stage 0 runs every utterance to glen0, the stages behind it to glen1 (the silence table; the same array without it)
      r.glen = trim ? (i == 0 ? glen_all : glen1) + b0 : nullptr;
      r.grate_in = (int)(Tn / T); r.grate_out = (int)(Tout / T);
      r.work_frac = 1.0;
      if (!glen_host.empty() && r.ok()) {
        const std::vector<int>& gh = i == 0 ? glen_host : glen1_host;
        double fr = 0.0;
        for (int b = b0; b < b0 + nb; ++b) fr += gh[b];
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
                              trim ? glen1 : nullptr, (int)(Tn / T), 1.f / r.ctx->act_scale, r.ctx->flags_dev), "conv_post_cl");
    if (trim && iso) r.chk(launch_gen_tail_zero(o, Tn, in_lengths, B, T, (int)(Tn / T), r.s), "gen_tail_zero");
    else if (trim)
      r.chk(launch_gen_tail_fill(o, Tn, in_lengths, glen_all, glen1, tabled ? tail_row : nullptr, table, B, T, back, fwd, (int)(Tn / T),
                                 r.s), "gen_tail_fill");
  }
}

}  // namespace

namespace vsp {

void run_gen(Run& r, int B, int T, T3 z, const int64_t* in_lengths, const float* g, float* o) {
  if (r.ctx->gen_mode >= 1 && r.ctx->model.has_cl) run_generator_cl(r, B, T, z, in_lengths, g, o);
  else run_generator(r, B, T, z, in_lengths, g, o);
}

void tail_table_drop(vsp_ctx* ctx) {
  if (ctx->tail_table) (void)hipFree(ctx->tail_table);
  ctx->tail_table = nullptr;
}

// The silence table of a context whose weights have just been committed (model.h): the generator's ordinary launch sequence
// on zero input of back + 1 + fwd frames, TAIL_BUILD_B speakers per run, frames [back, back + 1 + fwd) of every waveform
// kept.  Synchronous on `s` (its scratch is allocated and freed here), so every later call finds a finished table whatever
// stream it arrives on; not profiled, and the status word is not touched.  A configuration the table does not cover, or a
// build that fails, leaves the context without one: the generator then runs as it did before.
void tail_table_build(vsp_ctx* ctx, hipStream_t s) {
  constexpr int TAIL_BUILD_B = 64;
  tail_table_drop(ctx);
  const vsp_config& c = ctx->cfg;
  const Model& m = ctx->model;
  if (!ctx->tail_table_on || !ctx->trim_tails || ctx->gen_mode != 1 || !m.has_cl || !ctx->arena) return;
  if (c.n_speakers < 1 || c.n_speakers > 4096) return;
  int back = 0, fwd = 0, reach1 = 0, fwd0 = 0;
  generator_frame_dependence(c, ctx->resblock, m.g_pre.K, m.post_k, back, fwd);
  generator_tail_reach(c, ctx->resblock, m.g_pre.K, m.post_k, reach1, fwd0);
  const long up = total_upsample(c);
  if ((size_t)fwd * up * sizeof(float) > 64 * 1024) return;
  // nothing to gain, or stage 0's output would not be exact as far as the stages behind it read it
  if (reach1 >= fwd + 1 || fwd0 + reach1 > fwd + 1) return;
  const int T = back + 1 + fwd, Bc = std::min(c.n_speakers, TAIL_BUILD_B);
  const size_t row = (size_t)(1 + fwd) * up;
  const int64_t gen = dry_bytes(ctx, [&](Run& r) { run_gen(r, Bc, T, T3{}, nullptr, nullptr, nullptr); });
  if (gen < 0) return;
  const size_t z_bytes = (size_t)r256((int64_t)Bc * c.inter_channels * T * (int64_t)sizeof(float));
  const size_t o_bytes = (size_t)r256((int64_t)Bc * T * up * (int64_t)sizeof(float));
  char* scratch = nullptr;
  float* table = nullptr;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&table), (size_t)c.n_speakers * row * sizeof(float));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&scratch), z_bytes + o_bytes + (size_t)gen);
  if (e == hipSuccess) e = hipMemsetAsync(scratch, 0, z_bytes, s);
  // (the build is no call of the caller's: no profile entries, no status flags, no error text left behind)
  const bool prof_on = ctx->prof_on;
  unsigned* const flags_dev = ctx->flags_dev;
  const std::string err = ctx->err;
  ctx->prof_on = false;
  ctx->flags_dev = nullptr;
  int rc = VSP_OK;
  for (int s0 = 0; s0 < c.n_speakers && e == hipSuccess && rc == VSP_OK; s0 += Bc) {
    const int nb = std::min(Bc, c.n_speakers - s0);
    float* const z = reinterpret_cast<float*>(scratch);
    float* const o = reinterpret_cast<float*>(scratch + z_bytes);
    Ws ws(scratch + z_bytes + o_bytes, (size_t)gen, false);
    Run r{ctx, s, ws};
    run_gen(r, nb, T, ext(z, c.inter_channels, T), nullptr, ctx->arena + m.emb_g + (size_t)s0 * c.gin_channels, o);
    rc = ws.overflow ? VSP_ERR_WORKSPACE : r.rc;
    if (rc == VSP_OK)
      e = hipMemcpy2DAsync(table + (size_t)s0 * row, row * sizeof(float), o + (size_t)back * up, (size_t)T * up * sizeof(float),
                           row * sizeof(float), (size_t)nb, hipMemcpyDeviceToDevice, s);
  }
  ctx->prof_on = prof_on;
  ctx->flags_dev = flags_dev;
  ctx->err = err;
  if (scratch || table) {
    const hipError_t es = hipStreamSynchronize(s);
    if (e == hipSuccess) e = es;
  }
  if (scratch) (void)hipFree(scratch);
  if (e != hipSuccess || rc != VSP_OK) {
    if (table) (void)hipFree(table);
    (void)hipGetLastError();
    return;
  }
  ctx->tail_table = table;
  ctx->tail_back = back; ctx->tail_fwd = fwd; ctx->tail_reach1 = reach1;
}

}  // namespace vsp

extern "C" {

int64_t vsp_generator_workspace_bytes(const vsp_ctx* ctx, int B, int T) {
  if (!ctx || B <= 0 || T <= 0) return VSP_ERR_ARG;
  return dry_bytes(ctx, [&](Run& r) { run_gen(r, B, T, T3{}, nullptr, nullptr, nullptr); });
}

int vsp_generator(vsp_ctx* ctx, void* stream, int B, int T, const float* z, const float* g, float* o, void* workspace,
                  int64_t workspace_bytes) {
  int rc = check_ready(ctx);
  if (rc) return rc;
  if (B <= 0 || T <= 0 || !z || !g || !o || !workspace) return ctx->fail(VSP_ERR_ARG, "vsp_generator: bad argument");
  return run_sized(ctx, stream, "generator", vsp_generator_workspace_bytes(ctx, B, T), workspace, workspace_bytes,
                   [&](Run& r) { run_gen(r, B, T, ext(z, ctx->cfg.inter_channels, T), nullptr, g, o); });
}

int vsp_generator_ragged(vsp_ctx* ctx, void* stream, int B, int T, const float* z, const float* g, const int64_t* lengths,
                         float* o, void* workspace, int64_t workspace_bytes) {
  int rc = check_ready(ctx);
  if (rc) return rc;
  if (B <= 0 || T <= 0 || !z || !g || !lengths || !o || !workspace) return ctx->fail(VSP_ERR_ARG, "vsp_generator_ragged: bad argument");
  const int64_t need = vsp_generator_workspace_bytes(ctx, B, T) + (int64_t)B * (int64_t)sizeof(int);
  return run_sized(ctx, stream, "ragged generator", need, workspace, workspace_bytes, [&](Run& r) {
    r.iso = true;
    run_gen(r, B, T, ext(z, ctx->cfg.inter_channels, T), lengths, g, o);
  });
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

int vsp_generator_tail_extents(const vsp_ctx* ctx, int* back, int* fwd, int* reach1) {
  if (!ctx || !back || !fwd || !reach1) return VSP_ERR_ARG;
  const int pre_k = ctx->model.g_pre.K > 0 ? ctx->model.g_pre.K : 7;
  int fwd0 = 0;
  generator_frame_dependence(ctx->cfg, ctx->resblock, pre_k, ctx->model.post_k, *back, *fwd);
  generator_tail_reach(ctx->cfg, ctx->resblock, pre_k, ctx->model.post_k, *reach1, fwd0);
  return VSP_OK;
}

int64_t vsp_generator_stream_workspace_bytes(const vsp_ctx* ctx, int B, int chunk_frames) {
  if (!ctx || B <= 0 || chunk_frames <= 0) return VSP_ERR_ARG;
  const int span = chunk_frames + 2 * vsp_generator_halo_frames(ctx);
  const int64_t g = vsp_generator_workspace_bytes(ctx, B, span);
  if (g < 0) return g;
  return g + r256((int64_t)B * span * total_upsample(ctx->cfg) * (int64_t)sizeof(float));
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
  const int64_t scratch = r256((int64_t)B * span * up * (int64_t)sizeof(float));
  float* o_span = static_cast<float*>(workspace);   // [span waveform | generator]
  rc = run_sized(ctx, stream, "stream chunk", gen_bytes < 0 ? gen_bytes : gen_bytes + scratch, workspace, workspace_bytes, [&](Run& r) {
    // the frames [lo, hi) of every channel row: same strides as z, shifted start
    run_gen(r, B, span, T3{const_cast<float*>(z) + lo, (long)ctx->cfg.inter_channels * T, (long)T}, nullptr, g, o_span);
  }, scratch);
  if (rc) return rc;
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
  StreamRowsWs w{};
  const int64_t need = stream_rows_ws(ctx, B, span, w) ? w.total : -1;
  char* const base = static_cast<char*>(workspace);
  float* const o_span = reinterpret_cast<float*>(base + w.o_span);
  float* const zp = reinterpret_cast<float*>(base + w.zp);
  float* const gp = reinterpret_cast<float*>(base + w.gp);
  int64_t* const len = reinterpret_cast<int64_t*>(base + w.len);
  const int inter = ctx->cfg.inter_channels;
  *o_span_out = o_span;
  *span_out = span;
  return run_sized(ctx, s, "stream rows", need, workspace, workspace_bytes, [&](Run& r) {
    r.chk(launch_stream_gather(gr, B, inter, w.S4, ctx->cfg.gin_channels, zp, gp, len, s), "stream_gather");
    r.iso = true;
    // the host knows every window: a tick whose windows are all `span` frames long runs without per-utterance extents
    r.host_lengths = span_len;
    run_gen(r, B, span, T3{zp, (long)inter * w.S4, (long)w.S4}, len, gp, o_span);
  }, w.gen);
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
  const vsp_ctx::RateTable& t = ctx->out_stage;
  if (!t.tab) return ctx->fail(VSP_ERR_STATE, "output stage not configured (vsp_output_configure)");
  if (B < 1 || B > STREAM_ROWS_MAX || !rows || !out || !workspace || (pcm != 0 && pcm != 1) || out_stride < 1)
    return ctx->fail(VSP_ERR_ARG, "vsp_generator_stream_rows_output: bad argument (1 <= B <= %d)", STREAM_ROWS_MAX);
  const int up = (int)total_upsample(ctx->cfg);
  const int L = t.L, M = t.M, H = t.H, K = vsp_output_history_samples(L, M, H);
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
  const StreamOutFilter f{t.tab, L, M, H, t.J, t.P};
  hipError_t e = launch_stream_output(o_span, (long)span * up, orows, B, f, K, out, (long)out_stride, pcm, s);
  return e == hipSuccess ? VSP_OK : ctx->fail(VSP_ERR_HIP, "stream_output: %s", hipGetErrorString(e));
}

}  // extern "C"
