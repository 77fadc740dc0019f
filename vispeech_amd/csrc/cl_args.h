// Launch arguments of the channels-last split-f16 vocoder kernels (kernels.h: Cl*Args), built in ONE place for the model's
// schedule (api_generator.hip) and the stand-alone operators (ops.hip).  A builder takes device pointers and shapes and sets every
// field that follows from them -- dense tensors [B][T][C], "same" padding, the reference's leaky-relu slope, div = 1 --;
// what only the caller knows stays with the caller: acc_prev / div, ring / rw64, the ragged batch's glen / grate.
// Included by kernels.h, behind the structs.
#pragma once
#include <cstring>

namespace vsp {

// modules.LRELU_SLOPE (reference modules.py:17): the activation in front of every ResBlock convolution and up-convolution
constexpr float CL_LRELU_SLOPE = 0.1f;

// one convolution's packed fragment image (pack_g16_weights; 16 -> 16: pack_g16c16_weights) and bias * G16_WSCALE on the device
struct ClW {
  const uint16_t* w;
  const float* b;
};

template <class A>
inline A cl_zeroed() {
  A a;
  std::memset(&a, 0, sizeof a);
  return a;
}

// out = conv(lrelu(x, in_slope), dilation dil, "same" padding) + bias [+ res]: x [B][T][Cin], out and res [B][T][Cout].
// The operand-image extents (ClConvArgs::x_img / o_img) are set for these shapes: a caller only plugs the images in.
inline ClConvArgs cl_conv_args(ClW cw, int Cin, int Cout, int K, int dil, const float* x, int T, float in_slope,
                               const float* res, float* out, int terms) {
  ClConvArgs a = cl_zeroed<ClConvArgs>();
  a.x = x; a.x_bs = (long)T * Cin; a.x_ts = Cin;
  a.wh = cw.w; a.bias = cw.b;
  a.out = out; a.o_bs = (long)T * Cout; a.o_ts = Cout;
  a.res = res; a.r_bs = (long)T * Cout; a.r_ts = Cout;
  a.Cin = Cin; a.Cout = Cout; a.K = K; a.dil = dil; a.pad = dil * (K - 1) / 2;
  a.T_in = T; a.Nq = T; a.T_store = T;
  a.in_act = 1; a.in_slope = in_slope;
  a.div = 1.f; a.phases = 1;
  a.terms = terms;
  a.xi_bs = (long)cl_img_halfs(Cin, T); a.xi_tpad = cl_img_tpad(T);
  a.oi_bs = (long)cl_img_halfs(Cout, T); a.oi_tpad = cl_img_tpad(T);
  a.oi_slope = CL_LRELU_SLOPE;              // an image holds the NEXT ResBlock convolution's activated input
  return a;
}
// HiFi-GAN's up-convolution in polyphase form (ups_weight_offset above): kt = k / stride taps per phase over the input
// padded by kt - 1, T + 1 input times, output rows stride q + r - (k - stride) / 2 kept in [0, stride T).
// x [B][T][Cin] -> out [B][stride T][Cout]; cw: rows phase * Cout + co.
inline ClConvArgs cl_ups_args(ClW cw, int Cin, int Cout, int kt, int stride, const float* x, int T, float in_slope, float* out,
                              int terms) {
  ClConvArgs a = cl_conv_args(cw, Cin, Cout, kt, 1, x, T, in_slope, nullptr, out, terms);
  a.pad = kt - 1; a.Nq = T + 1;
  a.phases = stride; a.ups_p = stride * (kt - 1) / 2; a.T_store = T * stride;
  a.o_bs = (long)a.T_store * Cout; a.r_bs = a.o_bs;
  a.oi_bs = (long)cl_img_halfs(Cout, a.T_store); a.oi_tpad = cl_img_tpad(a.T_store);
  return a;
}

// The blocks below take their convolutions' weights in execution order: ResBlock1 conv1, conv2 of pair 0, 1, ..;
// ResBlock2 conv_a, conv_b.  x and out [B][T][C], x != out.
inline ClPairArgs cl_pair_args(const ClW* cw, int C, int K, int dil, const float* x, float* out, int T, int terms) {
  ClPairArgs a = cl_zeroed<ClPairArgs>();
  a.x = x; a.x_bs = (long)T * C; a.out = out; a.o_bs = (long)T * C;
  a.w1h = cw[0].w; a.b1 = cw[0].b; a.w2h = cw[1].w; a.b2 = cw[1].b;
  a.C = C; a.K = K; a.dil = dil; a.T = T;
  a.slope = CL_LRELU_SLOPE; a.div = 1.f; a.terms = terms;
  return a;
}
inline ClChainArgs cl_chain_args(const ClW* cw, int C, int K, const int* dil, int np, const float* x, float* out, int T,
                                 int terms) {
  ClChainArgs a = cl_zeroed<ClChainArgs>();
  a.x = x; a.x_bs = (long)T * C; a.out = out; a.o_bs = (long)T * C;
  for (int i = 0; i < 2 * np; ++i) { a.w[i] = cw[i].w; a.b[i] = cw[i].b; }
  for (int p = 0; p < np; ++p) a.dil[p] = dil[p];
  a.np = np; a.C = C; a.K = K; a.T = T;
  a.slope = CL_LRELU_SLOPE; a.div = 1.f; a.terms = terms;
  return a;
}
inline ClRb2Args cl_rb2_args(const ClW* cw, int C, int K, const int* dil, const float* x, float* out, int T, int terms) {
  ClRb2Args a = cl_zeroed<ClRb2Args>();
  a.x = x; a.x_bs = (long)T * C; a.out = out; a.o_bs = (long)T * C;
  for (int c = 0; c < 2; ++c) { a.w[c] = cw[c].w; a.b[c] = cw[c].b; a.dil[c] = dil[c]; }
  a.C = C; a.K = K; a.T = T;
  a.slope = CL_LRELU_SLOPE; a.div = 1.f; a.terms = terms;
  return a;
}

// g16_c16's step list (ClC16Args) of np ResBlock1 pairs -- [conv(d_p), conv(1) + add] each -- or of a ResBlock2 --
// [conv(d) + add] x 2 --: the ONE place that holds this mapping.  Returns the number of steps; dil / add hold 6.
inline int cl_c16_steps(int kind, const int* rb_dil, int np, int* dil, int* add) {
  if (kind == 2) {
    for (int c = 0; c < 2; ++c) { dil[c] = rb_dil[c]; add[c] = 1; }
    return 2;
  }
  for (int p = 0; p < np; ++p) {
    dil[2 * p] = rb_dil[p]; add[2 * p] = 0;
    dil[2 * p + 1] = 1; add[2 * p + 1] = 1;
  }
  return 2 * np;
}
// kind 1: pairs [0, np) of a ResBlock1 (np <= 3); kind 2: a ResBlock2 (np ignored).  16 channels.
inline ClC16Args cl_c16_args(int kind, const ClW* cw, int K, const int* dil, int np, const float* x, float* out, int T, int terms) {
  ClC16Args a = cl_zeroed<ClC16Args>();
  a.x = x; a.x_bs = (long)T * 16; a.out = out; a.o_bs = (long)T * 16;
  a.nsteps = cl_c16_steps(kind, dil, np, a.dil, a.add);
  for (int i = 0; i < a.nsteps; ++i) { a.w[i] = cw[i].w; a.b[i] = cw[i].b; }
  a.K = K; a.T = T;
  a.slope = CL_LRELU_SLOPE; a.div = 1.f; a.terms = terms;
  return a;
}

}  // namespace vsp
