// Stand-alone operators of the C-ABI (include/vispeech_hip.h): one convolution, ResBlock, up-convolution or attention on the
// caller's tensors with host weights, no context -- what tests/test_cl_ops.py, test_c16_ops.py, test_resblock2_ops.py,
// test_cl_block_ops.py, test_cl_block_route_host.py, test_upsample_ops.py, test_attention_ops.py, test_frame_conv_epilogue.py
// and test_conv_form_host.py drive.  The channels-last ones fill their launch arguments with the builders the model's schedule
// uses (cl_args.h).  Every call allocates, uploads and synchronises: test and measurement entry points, not a hot path.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "kernels.h"

using namespace vsp;

namespace {
struct DevBuf {           // hipMalloc'd scratch of one stand-alone call
  void* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16); }
};
// dense [phases * Cout][Cin][K] host weights -> packed fragment image on the device; bias [Cout] -> device
hipError_t upload_cl_conv(const float* w_host, const float* bias_host, int Cout, int Cin, int K, DevBuf& w, DevBuf& bias,
                          hipStream_t s, int phases = 1) {
  const bool c16 = cl_is_c16(Cout, Cin, phases);         // (gen16_c16.hip's image)
  std::vector<uint16_t> packed(c16 ? packed_g16c16_halfs(K) : packed_g16_halfs(phases * Cout, Cin, K));
  if (c16) pack_g16c16_weights(packed.data(), K, w_host);
  else pack_g16_weights(packed.data(), phases * Cout, Cin, K, w_host);
  hipError_t e = w.alloc(packed.size() * 2);
  if (e == hipSuccess) e = bias.alloc((size_t)Cout * 4);
  if (e == hipSuccess) e = hipMemcpyAsync(w.p, packed.data(), packed.size() * 2, hipMemcpyHostToDevice, s);
  std::vector<float> scaled(Cout, 0.f);                  // (kernels.h: these kernels take the bias * G16_WSCALE)
  if (bias_host) for (int i = 0; i < Cout; ++i) scaled[i] = bias_host[i] * G16_WSCALE;
  if (e == hipSuccess) e = hipMemcpyAsync(bias.p, scaled.data(), (size_t)Cout * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);     // the host vectors die with this frame
  return e;
}
ClW cw(const DevBuf& w, const DevBuf& bias) { return ClW{static_cast<const uint16_t*>(w.p), static_cast<const float*>(bias.p)}; }
int op_rc(hipError_t e) { return e == hipSuccess ? VSP_OK : (e == hipErrorInvalidValue ? VSP_ERR_UNSUPPORTED : VSP_ERR_HIP); }
// HiFi-GAN's up-convolutions as the generator runs them (kernels.h ups_weight_offset): kt = K / stride taps per phase over
// the input padded by kt - 1, Nq = T + 1 input times, output rows n = stride q + r - (K - stride) / 2 kept in [0, stride T)
// -- the shapes plan_model accepts
bool ups_shape_ok(int K, int stride) { return stride >= 1 && K >= stride && K % stride == 0 && (K - stride) % 2 == 0; }
// the shapes both attention launchers take (they answer hipErrorInvalidValue to the rest)
bool attn_shape_ok(int H, int n_heads, int window) {
  if (H <= 0 || n_heads <= 0 || H % n_heads || window < 0 || 2 * window + 1 > 16) return false;
  const int dk = H / n_heads;
  return dk == 32 || dk == 64 || dk == 96;
}
// device int64 lengths [B], each in [0, T] (the kernels index keys and queries by them)
int check_lengths64(const int64_t* lengths, int B, int T, hipStream_t s) {
  if (!lengths) return VSP_OK;
  std::vector<int64_t> len(B);
  hipError_t e = hipMemcpyAsync(len.data(), lengths, (size_t)B * 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return op_rc(e);
  for (int64_t l : len)
    if (l < 0 || l > T) return VSP_ERR_ARG;
  return VSP_OK;
}
// the relative-position tables [2 window + 1][dk] -> device
hipError_t upload_emb(const float* emb_k_host, const float* emb_v_host, int window, int dk, DevBuf& ek, DevBuf& ev, hipStream_t s) {
  const size_t bytes = (size_t)(2 * window + 1) * dk * 4;
  hipError_t e = ek.alloc(bytes);
  if (e == hipSuccess) e = ev.alloc(bytes);
  if (e == hipSuccess) e = hipMemcpyAsync(ek.p, emb_k_host, bytes, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(ev.p, emb_v_host, bytes, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);     // (pageable host memory: the caller's arrays may go after the call)
  return e;
}
// device int32 lengths [B] of a ragged channels-last batch: utterance b ends after lengths[b] * grate columns, 1 <= lengths[b]
// and lengths[b] * grate <= T (a zero length is refused: the persistent kernels' cursors step to t0 = 0 of the next utterance
// and clamp reads to row T - 1; the generator's plans never produce one)
int check_glen(const int32_t* lengths, int grate, int B, int T, hipStream_t s) {
  if (!lengths) return VSP_OK;
  std::vector<int32_t> len(B);
  hipError_t e = hipMemcpyAsync(len.data(), lengths, (size_t)B * 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return op_rc(e);
  for (int32_t l : len)
    if (l < 1 || (long)l * grate > T) return VSP_ERR_ARG;
  return VSP_OK;
}

// the descriptor of vsp_cl_resblock / vsp_cl_resblock2: no accumulate, no divide, a uniform batch, the kernel-choice flags
// from the environment (read per call: the test API has no context)
vsp_cl_block_desc cl_block_plain(int kind, int mode, int B, int T, int C, int K, int n_pairs, int terms, const int* dilations,
                                 const float* x, float* out, const float* const* w_host, const float* const* bias_host) {
  vsp_cl_block_desc d;
  std::memset(&d, 0, sizeof d);
  d.kind = kind; d.mode = mode; d.B = B; d.T = T; d.C = C; d.K = K; d.n_pairs = n_pairs; d.terms = terms;
  d.dilations = dilations; d.x = x; d.out = out; d.w = w_host; d.bias = bias_host;
  d.grate = 1; d.div = 1.f;
  if (const char* ev = getenv("VSP_PAIR")) d.ring = !strcmp(ev, "ring");
  if (const char* ev = getenv("VSP_RW64")) d.rw64 = atoi(ev) != 0;
  if (const char* ev = getenv("VSP_CHAIN_RING")) d.chain_ring = atoi(ev) != 0;
  return d;
}

// vsp_cl_block_ex (include/vispeech_hip.h).  One sequence builds every launch's arguments, asks the launcher's route
// function which kernel they take, and -- unless plan_only -- launches: the report and the run cannot disagree.
int cl_block_run(void* stream, const vsp_cl_block_desc& d, vsp_cl_block_route* route_out) {
  const int B = d.B, T = d.T, C = d.C, K = d.K, mode = d.mode, terms = d.terms;
  const bool rb2 = d.kind == 2, plan = d.plan_only != 0;
  if (d.kind != 1 && d.kind != 2) return VSP_ERR_ARG;
  const int n_pairs = rb2 ? 1 : d.n_pairs, nconv = rb2 ? 2 : 2 * n_pairs;
  if (!d.x || !d.w || !d.bias || !d.dilations || !d.out || d.x == d.out || B < 0 || T < 0 || n_pairs < 1 || n_pairs > 8 ||
      mode < 0 || mode > (rb2 ? 1 : 2) || (terms != 1 && terms != 3) || (rb2 && (!d.w[0] || !d.w[1])) || !(d.div != 0.f) ||
      d.grate < 1 || (plan && !route_out))
    return VSP_ERR_ARG;
  const int* dil = d.dilations;
  const bool c16 = C == 16;                              // (g16_c16: mode 1 = a pair's two steps / the ResBlock2, mode 2 = the whole ResBlock1)
  if (C <= 0 || (!c16 && C % 32) || K < 1 || !(K & 1) || (size_t)T * C * 4 >= (size_t)1 << 31) return VSP_ERR_UNSUPPORTED;
  if (rb2) {
    for (int c = 0; c < 2; ++c)
      if (dil[c] < 1 || (K - 1) * dil[c] > 64) return VSP_ERR_UNSUPPORTED;
    if (mode == 1 && (c16 ? !g16_c16_rb2_supported(K, dil) : !g16_rb2_supported(C, K, dil))) return VSP_ERR_UNSUPPORTED;
  } else {
    for (int p = 0; p < n_pairs; ++p) {
      if (dil[p] < 1 || (K - 1) * dil[p] > 64) return VSP_ERR_UNSUPPORTED;
      if (mode == 1 && (c16 ? !g16_c16_rb1_supported(K, dil + p, 1)
                            : !g16_pair_supported(C, K, dil[p]) && !g16_pp_supported(C, K, dil[p], terms)))
        return VSP_ERR_UNSUPPORTED;
      if (!d.w[2 * p] || !d.w[2 * p + 1]) return VSP_ERR_ARG;
    }
    if (mode == 2 && (n_pairs > 3 || (c16 ? !g16_c16_rb1_supported(K, dil, n_pairs) : !g16_chain_supported(C, K, dil, n_pairs))))
      return VSP_ERR_UNSUPPORTED;
  }
  vsp_cl_block_route rt;
  std::memset(&rt, 0, sizeof rt);
  if (route_out) *route_out = rt;
  if (B == 0 || T == 0) return VSP_OK;
  hipStream_t s = (hipStream_t)stream;
  if (!plan)
    if (int rc = check_glen(d.lengths, d.grate, B, T, s); rc != VSP_OK) return rc;
  const bool fused1 = mode == 2 || (rb2 && mode == 1);   // the whole block in one launch: no intermediate tensor
  const bool image = !rb2 && mode == 0 && terms == 3 && K >= 3 && !c16 && !d.no_image;   // the pair's intermediate as an operand image
  // a plan dereferences nothing: the intermediates are then distinct aligned addresses that only answer "is there one"
  alignas(16) static float plan_buf[4][4];
  std::vector<DevBuf> w(nconv), bias(nconv);
  DevBuf t1, ya, yb, timg;
  hipError_t e = hipSuccess;
  if (!plan) {
    for (int i = 0; i < nconv && e == hipSuccess; ++i) e = upload_cl_conv(d.w[i], d.bias[i], C, C, K, w[i], bias[i], s);
    const size_t el = (size_t)B * T * C;
    if (e == hipSuccess && !fused1) e = t1.alloc(el * 4);
    if (e == hipSuccess && !fused1 && !rb2) e = ya.alloc(el * 4);
    if (e == hipSuccess && !fused1 && !rb2) e = yb.alloc(el * 4);
    if (e == hipSuccess && image) e = timg.alloc((size_t)B * cl_img_halfs(C, T) * 2);
    // Every intermediate starts as NaN (all-ones words, fp32 and f16 alike): the generator's workspace holds whatever the
    // last call left, so a launch that reads a row no launch before it wrote -- behind a ragged end, in an image's pads --
    // must show in the result instead of meeting fresh, zeroed memory.
    const std::pair<DevBuf*, size_t> scratch[] = {{&t1, el * 4}, {&ya, el * 4}, {&yb, el * 4}, {&timg, (size_t)B * cl_img_halfs(C, T) * 2}};
    for (const auto& sc : scratch)
      if (e == hipSuccess && sc.first->p) e = hipMemsetAsync(sc.first->p, 0xFF, sc.second, s);
    if (e == hipSuccess && image) e = launch_cl_img_zero_pads(static_cast<uint16_t*>(timg.p), B, C, T, s, d.lengths, d.grate);
    if (e != hipSuccess) return op_rc(e);
  }
  float* const t1p = plan ? plan_buf[0] : static_cast<float*>(t1.p);
  float* const yap = plan ? plan_buf[1] : static_cast<float*>(ya.p);
  float* const ybp = plan ? plan_buf[2] : static_cast<float*>(yb.p);
  uint16_t* const img = !image ? nullptr : plan ? reinterpret_cast<uint16_t*>(plan_buf[3]) : static_cast<uint16_t*>(timg.p);
  std::vector<ClW> conv(nconv);                         // (execution order: conv1, conv2 of pair 0, 1, ..; conv_a, conv_b)
  for (int i = 0; i < nconv; ++i) conv[i] = cw(w[i], bias[i]);
  // One launch: its route into the report, then the launch itself.  `last`: the block's last launch carries the
  // accumulate / divide epilogue (where run_generator_cl puts them); every launch carries the ragged extent.
  auto step = [&](const ClRoute& r, auto launch) -> hipError_t {
    if (r.kernel == VSP_CL_KERNEL_NONE || rt.n >= VSP_CL_BLOCK_MAX_LAUNCHES) return hipErrorInvalidValue;
    rt.launch[rt.n++] = r;
    return plan ? hipSuccess : launch();
  };
  auto one_conv = [&](ClConvArgs a, bool last) {
    if (last) { a.acc_prev = d.acc_prev ? 1 : 0; a.div = d.div; }
    a.glen = d.lengths; a.g_in = d.grate; a.g_store = d.grate;
    return step(g16_conv_route(a, B), [&] { return launch_g16_conv(a, B, s); });
  };
  // ResBlock1 pairs [p0, p0 + np), or the ResBlock2, as one launch: g16_c16 at 16 channels, else g16_rb2, g16_pair
  // (as_pair) or g16_chain
  auto fused = [&](const float* xin, float* yout, int p0, int np, bool as_pair, bool last) {
    auto fin = [&](auto& a) {
      if (last) { a.acc_prev = d.acc_prev ? 1 : 0; a.div = d.div; }
      a.glen = d.lengths; a.grate = d.grate;
    };
    if (c16) {
      ClC16Args a = cl_c16_args(d.kind, &conv[2 * p0], K, dil + p0, np, xin, yout, T, terms);
      fin(a);
      return step(g16_c16_route(a), [&] { return launch_g16_c16(a, B, s); });
    }
    if (rb2) {
      ClRb2Args a = cl_rb2_args(conv.data(), C, K, dil, xin, yout, T, terms);
      fin(a);
      return step(g16_rb2_route(a), [&] { return launch_g16_rb2(a, B, s); });
    }
    if (as_pair) {
      ClPairArgs a = cl_pair_args(&conv[2 * p0], C, K, dil[p0], xin, yout, T, terms);
      a.ring = d.ring ? 1 : 0; a.rw64 = d.rw64 ? 1 : 0;
      fin(a);
      return step(g16_pair_route(a), [&] { return launch_g16_pair(a, B, s); });
    }
    ClChainArgs a = cl_chain_args(&conv[2 * p0], C, K, dil + p0, np, xin, yout, T, terms);
    a.ring = d.chain_ring ? 1 : 0;
    fin(a);
    return step(g16_chain_route(a), [&] { return launch_g16_chain(a, B, s); });
  };
  if (fused1) {
    e = fused(d.x, d.out, 0, n_pairs, false, true);
  } else if (rb2) {
    // one g16_conv per convolution: y = x + conv_a(lrelu(x)), out = y + conv_b(lrelu(y))
    e = one_conv(cl_conv_args(conv[0], C, C, K, dil[0], d.x, T, CL_LRELU_SLOPE, d.x, t1p, terms), false);
    if (e == hipSuccess) e = one_conv(cl_conv_args(conv[1], C, C, K, dil[1], t1p, T, CL_LRELU_SLOPE, t1p, d.out, terms), true);
  } else {
    // the running y ping-pongs between two buffers (a tile reads halo rows its neighbour writes)
    const float* yin = d.x;
    for (int p = 0; p < n_pairs && e == hipSuccess; ++p) {
      const bool last = p == n_pairs - 1;
      float* yout = last ? d.out : ((p & 1) ? ybp : yap);
      if (mode == 1) {
        e = fused(yin, yout, p, 1, true, last);
      } else {
        // one launch per convolution; the intermediate as an operand image where the kernels take one (terms 3, K >= 3):
        // the path the >= 128-channel stages of the generator run
        ClConvArgs a1 = cl_conv_args(conv[2 * p], C, C, K, dil[p], yin, T, CL_LRELU_SLOPE, nullptr, img ? nullptr : t1p, terms);
        ClConvArgs a2 = cl_conv_args(conv[2 * p + 1], C, C, K, 1, t1p, T, CL_LRELU_SLOPE, yin, yout, terms);
        a1.o_img = img; a2.x_img = img;
        e = one_conv(a1, false);
        if (e == hipSuccess) e = one_conv(a2, last);
      }
      yin = yout;
    }
  }
  if (route_out) *route_out = rt;
  if (e == hipSuccess && !plan) e = hipStreamSynchronize(s);
  return op_rc(e);
}
}  // namespace

extern "C" {

int vsp_cl_conv1d(void* stream, int B, int T, int Cin, int Cout, int K, int dilation, const float* x, const float* w_host,
                  const float* bias_host, float in_slope, const float* res, int terms, float* out) {
  if (!x || !w_host || !out || B < 0 || T < 0 || (terms != 1 && terms != 3)) return VSP_ERR_ARG;
  const bool c16 = Cin == 16 && Cout == 16;              // (g16_c16; mixed 16 / 32 has no kernel)
  if (Cin <= 0 || Cout <= 0 || (!c16 && (Cin % 32 || Cout % 32)) || K < 1 || !(K & 1) || dilation < 1 || (K - 1) * dilation > 64 ||
      (size_t)T * std::max(Cin, Cout) * 4 >= (size_t)1 << 31)
    return VSP_ERR_UNSUPPORTED;
  if (c16 && x == out) return VSP_ERR_ARG;
  if (B == 0 || T == 0) return VSP_OK;
  hipStream_t s = (hipStream_t)stream;
  DevBuf w, bias;
  hipError_t e = upload_cl_conv(w_host, bias_host, Cout, Cin, K, w, bias, s);
  if (e == hipSuccess) e = launch_g16_conv(cl_conv_args(cw(w, bias), Cin, Cout, K, dilation, x, T, in_slope, res, out, terms), B, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  return op_rc(e);
}

int vsp_conv1d(void* stream, int B, int T, int Cin, int Cout, int K, int dilation, const float* x, const float* w_host,
               const float* bias_host, const int64_t* lengths, int mask_in, int in_act, float in_slope, int act,
               const float* res, int mask_out, int split_f16, float* out) {
  if (!x || !w_host || !out || B < 0 || T < 0 || act < 0 || act > 2 || ((mask_in || mask_out) && !lengths) || (act == 2 && res))
    return VSP_ERR_ARG;
  if (Cin <= 0 || Cout <= 0 || K < 1 || !(K & 1) || dilation < 1 || (K - 1) * dilation + 3 > CONV_HALO ||
      (act == 2 && Cout % 64) || ((T & 3) && T != 1))   // (rows of T floats must stay 16-byte aligned for the vector staging;
                                                        //  T = 1: the one-time-step projections, conv_t1_gemv)
    return VSP_ERR_UNSUPPORTED;
  if (B == 0 || T == 0) return VSP_OK;
  hipStream_t s = (hipStream_t)stream;
  // the gate reads its tanh / sigmoid halves from interleaved 32-row tiles (weights.cpp packs WN in_layers the same way)
  std::vector<float> wd((size_t)Cout * Cin * K), bd(Cout, 0.f);
  for (int r = 0; r < Cout; ++r) {
    int src = r;
    if (act == 2) { const int tile = r / 32, in = r % 32; src = (tile & 1) * (Cout / 2) + (tile >> 1) * 32 + in; }
    std::memcpy(&wd[(size_t)r * Cin * K], w_host + (size_t)src * Cin * K, (size_t)Cin * K * sizeof(float));
    if (bias_host) bd[r] = bias_host[src];
  }
  std::vector<float> packed(packed_conv_floats(Cout, Cin, K));
  if (split_f16) pack_conv_weights_f16s(packed.data(), Cout, Cin, K, wd.data());
  else pack_conv_weights(packed.data(), Cout, Cin, K, wd.data());
  DevBuf w, bias;
  hipError_t e = w.alloc(packed.size() * 4);
  if (e == hipSuccess) e = bias.alloc((size_t)Cout * 4);
  if (e == hipSuccess) e = hipMemcpyAsync(w.p, packed.data(), packed.size() * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(bias.p, bd.data(), (size_t)Cout * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return op_rc(e);
  const int rows_out = act == 2 ? Cout / 2 : Cout;
  ConvArgs a;
  std::memset(&a, 0, sizeof a);
  a.x = x; a.x_bs = (long)Cin * T; a.x_cs = T;
  a.wp = static_cast<const float*>(w.p); a.bias = static_cast<const float*>(bias.p);
  a.out = out; a.o_bs = (long)rows_out * T; a.o_cs = T;
  a.res = res; a.r_bs = (long)rows_out * T; a.r_cs = T;
  a.lengths = lengths;
  a.Cin = Cin; a.M = Cout; a.K = K; a.dil = dilation; a.pad = dilation * (K - 1) / 2;
  a.T_in = T; a.Nq = T; a.nchunks = (Cin + CONV_CK - 1) / CONV_CK;
  a.in_mask = mask_in ? 1 : 0; a.in_act = in_act ? 1 : 0; a.in_slope = in_slope;
  a.act = act; a.alpha = 1.f; a.div = 1.f; a.mask_post = mask_out ? 1 : 0;
  a.f16s = split_f16 ? 1 : 0;
  if (split_f16 == 2) {
    // the column-tile form (conv_cols.hip: every output row of a 64-column tile in one block) as a stand-alone operator:
    // the same weights in 16x16x32 A-fragment order; refused where that kernel does not apply
    std::vector<uint16_t> wgh(packed_g16_halfs(Cout, Cin, 1));
    DevBuf wgd;
    if (K != 1 || Cin % 32 || Cout % 16) return VSP_ERR_UNSUPPORTED;
    pack_g16_weights(wgh.data(), Cout, Cin, 1, wd.data());
    e = wgd.alloc(wgh.size() * 2);
    if (e == hipSuccess) e = hipMemcpyAsync(wgd.p, wgh.data(), wgh.size() * 2, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return op_rc(e);
    a.wg = static_cast<const uint16_t*>(wgd.p);
    if (!conv_cols_supported(a)) return VSP_ERR_UNSUPPORTED;
    e = launch_conv_cols(a, B, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return op_rc(e);
  }
  e = launch_conv(a, B, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  return op_rc(e);
}

int vsp_conv1d_ex(void* stream, const vsp_conv1d_desc* dp, vsp_conv_form* form_out) {
  if (!dp || (dp->plan_only && !form_out)) return VSP_ERR_ARG;
  const vsp_conv1d_desc& d = *dp;
  const int B = d.B, T = d.T, Cin = d.Cin, Cout = d.Cout, K = d.K;
  const bool masks = d.mask_in || d.mask_pre || d.mask_post || d.mask_post2;
  if (!d.x || !d.w || !d.out || B < 0 || T < 0 || d.act < 0 || d.act > 2 || (masks && !d.lengths) ||
      (d.act == 2 && (d.res || d.split_row)) || d.split_f16 < 0 || d.split_f16 > 1 || d.cols < 0 || d.cols > 1 || d.ln < 0 ||
      d.ln > 2 || (d.ln == 1 && !d.cols) || (d.ln != 0) != (d.ln_gamma != nullptr) || (d.ln != 0) != (d.ln_beta != nullptr) ||
      (d.split_row != 0) != (d.out2 != nullptr) || ((d.acc_prev2 || d.mask_post2) && !d.split_row) || d.cond_bs < 0 ||
      !(d.div != 0.f))
    return VSP_ERR_ARG;
  if (Cin <= 0 || Cout <= 0 || K < 1 || !(K & 1) || d.dilation < 1 || (K - 1) * d.dilation + 3 > CONV_HALO ||
      (d.act == 2 && (Cout % 64 || d.mask_pre || d.alpha != 1.f || d.acc_prev || d.div != 1.f)) ||   // (the gate's epilogue: cond, mask_post)
      (d.ln && (d.act == 2 || d.split_row || d.acc_prev)) || (d.cols && !d.split_f16))
    return VSP_ERR_UNSUPPORTED;
  if (d.split_row && (d.split_row < 0 || d.split_row >= Cout)) return VSP_ERR_ARG;
  if (d.split_row & 31) return VSP_ERR_UNSUPPORTED;
  if (form_out) *form_out = vsp_conv_form{};
  if (B == 0 || T == 0) return VSP_OK;
  // rows of the destinations; strides in elements, 0 = dense
  const int rows_out = d.act == 2 ? Cout / 2 : (d.split_row ? d.split_row : Cout), rows2 = d.split_row ? Cout - d.split_row : 0;
  struct View { long bs, cs; int rows; };
  auto view = [&](int64_t bs, int64_t cs, int rows) {
    View v{(long)bs, (long)cs, rows};
    if (!v.cs) v.cs = T;
    if (!v.bs) v.bs = (long)rows * v.cs;
    return v;
  };
  const View vx = view(d.x_bs, d.x_cs, Cin), vo = view(d.o_bs, d.o_cs, rows_out), vr = view(d.r_bs, d.r_cs, rows_out),
             v2 = view(d.o2_bs, d.o2_cs, rows2);
  for (const View* v : {&vx, &vo, &vr, &v2}) {
    if (v == &vr && !d.res) continue;
    if (v == &v2 && !d.split_row) continue;
    if (v->cs < T || (B > 1 && v->bs < (long)(v->rows - 1) * v->cs + T)) return VSP_ERR_ARG;
    // (the epilogues address a tensor with 32-bit byte offsets from the utterance's base)
    if (((long)v->rows * v->cs + T) * 4 >= (1L << 31)) return VSP_ERR_UNSUPPORTED;
  }
  hipStream_t s = (hipStream_t)stream;
  ConvArgs a;
  std::memset(&a, 0, sizeof a);
  a.x = d.x; a.x_bs = vx.bs; a.x_cs = vx.cs;
  a.out = d.out; a.o_bs = vo.bs; a.o_cs = vo.cs;
  // (ln: the residual enters the LayerNorm, not the convolution's epilogue)
  if (d.res && (!d.ln || d.ln == 1)) { a.res = d.res; a.r_bs = vr.bs; a.r_cs = vr.cs; }
  a.cond = d.cond; a.cond_bs = (long)d.cond_bs;
  a.lengths = d.lengths;
  a.Cin = Cin; a.M = Cout; a.K = K; a.dil = d.dilation; a.pad = d.dilation * (K - 1) / 2;
  a.T_in = T; a.Nq = T; a.nchunks = (Cin + CONV_CK - 1) / CONV_CK;
  a.in_mask = d.mask_in ? 1 : 0; a.in_act = d.in_act ? 1 : 0; a.in_slope = d.in_slope;
  a.act = d.act; a.mask_pre = d.mask_pre ? 1 : 0; a.alpha = d.alpha; a.acc_prev = d.acc_prev ? 1 : 0; a.div = d.div;
  a.mask_post = d.mask_post ? 1 : 0;
  a.split_row = d.split_row; a.out2 = d.out2; a.o2_bs = v2.bs; a.o2_cs = v2.cs; a.acc_prev2 = d.acc_prev2 ? 1 : 0;
  a.mask_post2 = d.mask_post2 ? 1 : 0;
  a.f16s = d.split_f16 ? 1 : 0;
  // ---- the kernel this launch takes
  const bool cols_shape = K == 1 && Cin % 32 == 0 && Cout % 16 == 0;
  vsp_conv_form form{};
  if (d.cols) {
    if (!cols_shape) return VSP_ERR_UNSUPPORTED;
    static const uint16_t no_image = 0;
    a.wg = &no_image;                                  // (any non-null address: conv_cols_supported reads no weight)
    if (!conv_cols_supported(a)) return VSP_ERR_UNSUPPORTED;
    if (d.ln == 1 && (Cout != 192 || Cin != 192 || a.mask_pre || a.mask_post || a.alpha != 1.f)) return VSP_ERR_UNSUPPORTED;
    form.kernel = d.ln == 1 ? VSP_CONV_FORM_COLS_LN : VSP_CONV_FORM_COLS;
    a.wg = nullptr;
  } else {
    form = conv_form(a, B);
    if (form.kernel == VSP_CONV_FORM_NONE) return VSP_ERR_UNSUPPORTED;
  }
  if (form_out) *form_out = form;
  if (d.plan_only) return VSP_OK;
  if (int rc = check_lengths64(d.lengths, B, T, s); rc != VSP_OK) return rc;
  // ---- weights and bias in kernel row order (the gate's interleaved 32-row tiles: weights.cpp packs WN in_layers the same way)
  std::vector<float> wd((size_t)Cout * Cin * K), bd(Cout, 0.f);
  for (int r = 0; r < Cout; ++r) {
    int src = r;
    if (d.act == 2) { const int tile = r / 32, in = r % 32; src = (tile & 1) * (Cout / 2) + (tile >> 1) * 32 + in; }
    std::memcpy(&wd[(size_t)r * Cin * K], d.w + (size_t)src * Cin * K, (size_t)Cin * K * sizeof(float));
    if (d.bias) bd[r] = d.bias[src];
  }
  DevBuf w, bias, wgd, scratch, gamma, beta;
  hipError_t e = bias.alloc((size_t)Cout * 4);
  if (e == hipSuccess) e = hipMemcpyAsync(bias.p, bd.data(), (size_t)Cout * 4, hipMemcpyHostToDevice, s);
  std::vector<float> packed;
  std::vector<uint16_t> wgh;
  if (d.cols) {
    wgh.resize(packed_g16_halfs(Cout, Cin, 1));
    pack_g16_weights(wgh.data(), Cout, Cin, 1, wd.data());
    if (e == hipSuccess) e = wgd.alloc(wgh.size() * 2);
    if (e == hipSuccess) e = hipMemcpyAsync(wgd.p, wgh.data(), wgh.size() * 2, hipMemcpyHostToDevice, s);
    a.wg = static_cast<const uint16_t*>(wgd.p);
  } else {
    packed.resize(packed_conv_floats(Cout, Cin, K));
    if (d.split_f16) pack_conv_weights_f16s(packed.data(), Cout, Cin, K, wd.data());
    else pack_conv_weights(packed.data(), Cout, Cin, K, wd.data());
    if (e == hipSuccess) e = w.alloc(packed.size() * 4);
    if (e == hipSuccess) e = hipMemcpyAsync(w.p, packed.data(), packed.size() * 4, hipMemcpyHostToDevice, s);
    a.wp = static_cast<const float*>(w.p);
  }
  if (d.bias) a.bias = static_cast<const float*>(bias.p);
  if (d.ln) {
    if (e == hipSuccess) e = gamma.alloc((size_t)Cout * 4);
    if (e == hipSuccess) e = beta.alloc((size_t)Cout * 4);
    if (e == hipSuccess) e = hipMemcpyAsync(gamma.p, d.ln_gamma, (size_t)Cout * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(beta.p, d.ln_beta, (size_t)Cout * 4, hipMemcpyHostToDevice, s);
  }
  if (d.ln == 2) {
    // the two-launch path: the convolution into a dense scratch tensor, then LayerNorm(scratch + res) into out
    if (e == hipSuccess) e = scratch.alloc((size_t)B * Cout * T * 4);
    a.out = static_cast<float*>(scratch.p); a.o_bs = (long)Cout * T; a.o_cs = T;
  }
  if (e == hipSuccess) e = hipStreamSynchronize(s);     // (pageable host memory: the vectors die with this frame)
  if (e != hipSuccess) return op_rc(e);
  if (d.ln == 1) e = launch_conv_cols(a, B, s, static_cast<const float*>(gamma.p), static_cast<const float*>(beta.p));
  else if (d.cols) e = launch_conv_cols(a, B, s);
  else e = launch_conv(a, B, s);
  if (e == hipSuccess && d.ln == 2)
    e = launch_layernorm(a.out, a.o_bs, a.o_cs, d.res, vr.bs, vr.cs, static_cast<const float*>(gamma.p),
                         static_cast<const float*>(beta.p), d.out, vo.bs, vo.cs, B, Cout, T, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  return op_rc(e);
}

int vsp_cl_block_ex(void* stream, const vsp_cl_block_desc* d, vsp_cl_block_route* route) {
  if (!d) return VSP_ERR_ARG;
  return cl_block_run(stream, *d, route);
}

int vsp_cl_resblock(void* stream, int B, int T, int C, int K, int n_pairs, const int* dilations, const float* x,
                    const float* const* w_host, const float* const* bias_host, int mode, int terms, float* out) {
  if (n_pairs < 1 || n_pairs > 8) return VSP_ERR_ARG;
  vsp_cl_block_desc d = cl_block_plain(1, mode, B, T, C, K, n_pairs, terms, dilations, x, out, w_host, bias_host);
  return cl_block_run(stream, d, nullptr);
}

int vsp_cl_resblock2(void* stream, int B, int T, int C, int K, const int* dilations, const float* x,
                     const float* const* w_host, const float* const* bias_host, int mode, int terms, float* out) {
  vsp_cl_block_desc d = cl_block_plain(2, mode, B, T, C, K, 2, terms, dilations, x, out, w_host, bias_host);
  return cl_block_run(stream, d, nullptr);
}

int vsp_cl_conv_post(void* stream, int B, int T, int C, int K, const float* x, const float* w_host, float slope, float unscale,
                     const int32_t* lengths, int grate, float* out) {
  if (!x || !w_host || !out || B < 0 || T < 0 || grate < 1) return VSP_ERR_ARG;
  if ((C != 16 && C != 32 && C != 64) || K < 1 || !(K & 1) || K > 7 || (size_t)T * C * 4 >= (size_t)1 << 31) return VSP_ERR_UNSUPPORTED;
  if (B == 0 || T == 0) return VSP_OK;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = check_glen(lengths, grate, B, T, s); rc != VSP_OK) return rc;
  // the model's tap-major image [K][C] of the reference's [1][C][K] (weights.cpp: post_wt)
  std::vector<float> wt((size_t)K * C);
  for (int c = 0; c < C; ++c)
    for (int j = 0; j < K; ++j) wt[(size_t)j * C + c] = w_host[(size_t)c * K + j];
  DevBuf w;
  hipError_t e = w.alloc(wt.size() * 4);
  if (e == hipSuccess) e = hipMemcpyAsync(w.p, wt.data(), wt.size() * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);     // (pageable host memory: the vector dies with this frame)
  if (e == hipSuccess)
    e = launch_conv_post_cl(x, (long)T * C, C, static_cast<const float*>(w.p), C, K, slope, out, T, B, T, s, lengths, grate, unscale,
                            nullptr);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  return op_rc(e);
}

int vsp_cl_conv_transpose1d(void* stream, int B, int T, int Cin, int Cout, int K, int stride, const float* x,
                            const float* w_host, const float* bias_host, float in_slope, const int32_t* lengths,
                            int terms, float* out) {
  if (!x || !w_host || !out || x == out || B < 0 || T < 0 || (terms != 1 && terms != 3)) return VSP_ERR_ARG;
  if (Cin <= 0 || Cout <= 0 || Cin % 32 || Cout % 16 || !ups_shape_ok(K, stride) || K / stride - 1 > 64 ||
      (size_t)T * std::max<size_t>(Cin, (size_t)stride * Cout) * 4 >= (size_t)1 << 31)
    return VSP_ERR_UNSUPPORTED;
  if (B == 0 || T == 0) return VSP_OK;
  hipStream_t s = (hipStream_t)stream;
  const int kt = K / stride;
  if (lengths) {                                         // (the kernels read rows [0, len) of an utterance: len > T overruns x)
    std::vector<int32_t> len(B);
    hipError_t e = hipMemcpyAsync(len.data(), lengths, (size_t)B * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return op_rc(e);
    for (int32_t l : len)
      if (l < 0 || l > T) return VSP_ERR_ARG;
  }
  // the model's channels-last packing (weights.cpp, Filler::clconv of dec.ups.*): row = phase * Cout + co
  std::vector<float> dense((size_t)stride * Cout * Cin * kt);
  for (int r = 0; r < stride; ++r)
    for (int co = 0; co < Cout; ++co)
      for (int ci = 0; ci < Cin; ++ci)
        for (int tap = 0; tap < kt; ++tap)
          dense[(((size_t)r * Cout + co) * Cin + ci) * kt + tap] = w_host[ups_weight_offset(ci, co, r, tap, Cout, stride, kt)];
  DevBuf w, bias;
  hipError_t e = upload_cl_conv(dense.data(), bias_host, Cout, Cin, kt, w, bias, s, stride);
  if (e != hipSuccess) return op_rc(e);
  ClConvArgs a = cl_ups_args(cw(w, bias), Cin, Cout, kt, stride, x, T, in_slope, out, terms);
  a.glen = lengths; a.g_in = 1; a.g_store = stride;
  e = launch_g16_conv(a, B, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  return op_rc(e);
}

int vsp_conv_transpose1d(void* stream, int B, int T, int Cin, int Cout, int K, int stride, const float* x,
                         const float* w_host, const float* bias_host, float in_slope, float* out) {
  if (!x || !w_host || !out || x == out || B < 0 || T < 0) return VSP_ERR_ARG;
  if (Cin <= 0 || Cout <= 0 || !ups_shape_ok(K, stride) || K / stride - 1 + 3 > CONV_HALO) return VSP_ERR_UNSUPPORTED;
  if (B == 0 || T == 0) return VSP_OK;
  hipStream_t s = (hipStream_t)stream;
  const int kt = K / stride, M = Cout * stride;
  // the model's f32 packing (weights.cpp, Filler::conv of dec.ups.*): row = co * stride + phase
  std::vector<float> dense((size_t)M * Cin * kt), bd(M, 0.f);
  for (int row = 0; row < M; ++row) {
    for (int ci = 0; ci < Cin; ++ci)
      for (int tap = 0; tap < kt; ++tap)
        dense[((size_t)row * Cin + ci) * kt + tap] = w_host[ups_weight_offset(ci, row / stride, row % stride, tap, Cout, stride, kt)];
    if (bias_host) bd[row] = bias_host[row / stride];
  }
  std::vector<float> packed(packed_conv_floats(M, Cin, kt));
  pack_conv_weights(packed.data(), M, Cin, kt, dense.data());
  // run_generator's tensors: time rows padded to a multiple of 64 columns; staged here from / to the caller's dense ones
  const long tp_in = ((long)T + 63) / 64 * 64, T_out = (long)T * stride, tp_out = (T_out + 63) / 64 * 64;
  DevBuf w, bias, xs, os;
  hipError_t e = w.alloc(packed.size() * 4);
  if (e == hipSuccess) e = bias.alloc((size_t)M * 4);
  if (e == hipSuccess) e = xs.alloc((size_t)B * Cin * tp_in * 4);
  if (e == hipSuccess) e = os.alloc((size_t)B * Cout * tp_out * 4);
  if (e == hipSuccess) e = hipMemcpyAsync(w.p, packed.data(), packed.size() * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(bias.p, bd.data(), (size_t)M * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemsetAsync(xs.p, 0, (size_t)B * Cin * tp_in * 4, s);
  if (e == hipSuccess)
    e = hipMemcpy2DAsync(xs.p, (size_t)tp_in * 4, x, (size_t)T * 4, (size_t)T * 4, (size_t)B * Cin, hipMemcpyDeviceToDevice, s);
  if (e != hipSuccess) return op_rc(e);
  ConvArgs a;
  std::memset(&a, 0, sizeof a);
  a.x = static_cast<const float*>(xs.p); a.x_bs = (long)Cin * tp_in; a.x_cs = tp_in;
  a.wp = static_cast<const float*>(w.p); a.bias = static_cast<const float*>(bias.p);
  a.out = static_cast<float*>(os.p); a.o_bs = (long)Cout * tp_out; a.o_cs = tp_out;
  a.Cin = Cin; a.M = M; a.K = kt; a.dil = 1; a.pad = kt - 1;
  a.T_in = T; a.Nq = T + 1; a.nchunks = (Cin + CONV_CK - 1) / CONV_CK;
  a.in_act = 1; a.in_slope = in_slope;
  a.alpha = 1.f; a.div = 1.f;
  a.ups_s = stride; a.ups_p = (K - stride) / 2; a.T_store = (int)T_out;
  e = launch_conv(a, B, s);
  if (e == hipSuccess)
    e = hipMemcpy2DAsync(out, (size_t)T_out * 4, os.p, (size_t)tp_out * 4, (size_t)T_out * 4, (size_t)B * Cout,
                         hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  return op_rc(e);
}

int vsp_rel_attention(void* stream, int B, int T, int H, int n_heads, int window, const float* qkv, const float* emb_k_host,
                      const float* emb_v_host, const int64_t* lengths, int kernel, int variant, float* out) {
  if (!qkv || !emb_k_host || !emb_v_host || !out || B < 0 || T < 0 || kernel < 0 || kernel > 1 || variant < -1 || variant > 1)
    return VSP_ERR_ARG;
  if (!attn_shape_ok(H, n_heads, window)) return VSP_ERR_UNSUPPORTED;
  if (B == 0 || T == 0) return VSP_OK;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = check_lengths64(lengths, B, T, s); rc != VSP_OK) return rc;
  const int dk = H / n_heads;
  DevBuf ek, ev, ws;
  hipError_t e = upload_emb(emb_k_host, emb_v_host, window, dk, ek, ev, s);
  const float* ekd = static_cast<const float*>(ek.p);
  const float* evd = static_cast<const float*>(ev.p);
  if (kernel == 0) {
    // variant 0 = the 32-query blocks whose waves split the keys (KSPLIT), 1 = the 128-query blocks
    if (e == hipSuccess)
      e = launch_attention(qkv, 3L * H * T, T, ekd, evd, lengths, out, (long)H * T, T, B, H, n_heads, T, window,
                           variant < 0 ? -1 : 1 - variant, s);
  } else {
    if (e == hipSuccess) e = ws.alloc(3 * attn_pack_bytes(B, n_heads, dk, T));
    if (e == hipSuccess)
      e = launch_attention_f16s(qkv, 3L * H * T, T, ekd, evd, lengths, out, (long)H * T, T, B, H, n_heads, T, window, ws.p, s,
                                variant);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  return op_rc(e);
}

int vsp_rel_attention_fused(void* stream, int B, int T, int H, int n_heads, int window, const float* x, const float* w_qkv_host,
                            const float* bias_qkv_host, const float* emb_k_host, const float* emb_v_host,
                            const int64_t* lengths, int variant, float* out) {
  if (!x || !w_qkv_host || !bias_qkv_host || !emb_k_host || !emb_v_host || !out || B < 0 || T < 0 || variant < -1 || variant > 1)
    return VSP_ERR_ARG;
  if (!attn_shape_ok(H, n_heads, window) || !attn_qkv_pack_supported(H, n_heads)) return VSP_ERR_UNSUPPORTED;
  if (B == 0 || T == 0) return VSP_OK;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = check_lengths64(lengths, B, T, s); rc != VSP_OK) return rc;
  const int dk = H / n_heads;
  // the stacked projection as the model holds it (weights.cpp: the wg image of an attention layer's qkv; the bias unscaled)
  std::vector<uint16_t> wgh(packed_g16_halfs(3 * H, H, 1));
  pack_g16_weights(wgh.data(), 3 * H, H, 1, w_qkv_host);
  DevBuf ek, ev, ws, wg, bias;
  hipError_t e = upload_emb(emb_k_host, emb_v_host, window, dk, ek, ev, s);
  if (e == hipSuccess) e = wg.alloc(wgh.size() * 2);
  if (e == hipSuccess) e = bias.alloc((size_t)3 * H * 4);
  if (e == hipSuccess) e = ws.alloc(3 * attn_pack_bytes(B, n_heads, dk, T));
  if (e == hipSuccess) e = hipMemcpyAsync(wg.p, wgh.data(), wgh.size() * 2, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(bias.p, bias_qkv_host, (size_t)3 * H * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e == hipSuccess)
    e = launch_attn_qkv_pack_f16s(x, (long)H * T, T, static_cast<const uint16_t*>(wg.p), static_cast<const float*>(bias.p),
                                  lengths, B, H, n_heads, T, ws.p, s);
  if (e == hipSuccess)
    e = launch_attention_f16s(nullptr, 3L * H * T, T, static_cast<const float*>(ek.p), static_cast<const float*>(ev.p), lengths,
                              out, (long)H * T, T, B, H, n_heads, T, window, ws.p, s, variant);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  return op_rc(e);
}

}  // extern "C"
