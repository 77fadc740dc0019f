// Internal kernel launch interface of libvispeech_hip (gfx950).  Not part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "../../include/vispeech_hip.h"   // (VSP_FLAG_*: the sticky status bits the kernels raise)

namespace vsp {

// hipFuncAttributeMaxDynamicSharedMemorySize is set per DEVICE: a process may hold contexts on several GPUs (vsp_create
// takes a device index), so a launcher remembers it per (kernel, device) -- `done` is the launcher's static bit set, one
// bit per device; safe to race (the attribute call is idempotent).
inline hipError_t set_max_dynamic_lds(const void* kern, int bytes, std::atomic<uint64_t>& done) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const uint64_t bit = 1ull << (dev & 63);
  if (done.load(std::memory_order_acquire) & bit) return hipSuccess;
  e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) done.fetch_or(bit, std::memory_order_release);
  return e;
}

// ------------------------------------------------------------------------------------------
// conv1d as implicit GEMM on v_mfma_f32_32x32x2_f32 (exact f32 fmaf chain).
//   out[b][row][q] = epilogue( sum_{ci,tap} Wp[row][ci][tap] * prologue(x[b][ci][q - pad + tap*dil]) )
// Weights are pre-packed in MFMA A-fragment order by pack_conv_weights() (host).
constexpr int CONV_CK = 32;    // input channels staged per LDS chunk
constexpr int CONV_HALO = 64;  // max (K-1)*dil

struct ConvArgs {
  const float* x; long x_bs, x_cs;
  const float* wp;            // packed weights
  const float* bias;          // [M] per packed row, or null
  float* out; long o_bs, o_cs;
  const float* res; long r_bs, r_cs;
  const float* cond; long cond_bs;   // cond[b*cond_bs + row] added after bias, or null
  const int64_t* lengths;     // [B] valid length (mask = t < lengths[b]), or null
  int Cin, M, K, dil, pad;
  int T_in;                   // input extent (zero padding outside [0,T_in))
  int Nq;                     // output columns computed
  int nchunks;                // ceil(Cin / CONV_CK)
  // prologue on the staged input
  int in_mask;                // x * mask
  int in_act; float in_slope; // leaky_relu(x, slope) (slope 0 = relu)
  // epilogue
  int act;                    // 0 none, 1 relu, 2 gate: tanh(tile 2i) * sigmoid(tile 2i+1)
  int mask_pre;
  float alpha;                // v *= alpha
  int acc_prev;               // v += out (read-modify-write)
  float div;                  // v /= div
  int mask_post;
  int ups_s, ups_p, T_store;  // transposed-conv store: row=(co,r), n = s*q + r - p in [0,T_store)
  int f16s;                   // weights packed by pack_conv_weights_f16s: split-f16 MFMA path
  // two destinations (WN res_skip layer, reference modules.py:165-172, as ONE launch): rows >= split_row (a multiple of
  // 32; 0 = off) go to out2[row - split_row] (+ out2 when acc_prev2) with no residual, mask or scaling; the rows
  // below it keep the epilogue above
  int split_row; float* out2; long o2_bs, o2_cs; int acc_prev2;
  int mask_post2;             // ... except this mask on the second destination (the two halves of one projection)
  // round 6: the same weights in 16x16x32 A-fragment order (pack_g16_weights, K = 1) for the column-tile form
  // (conv_cols.hip) of small-grid 1x1 convolutions; NULL = this convolution has no such image
  const uint16_t* wg;
  long wg_min_blocks, wg_max_blocks;   // launch_conv takes the column-tile kernel for this range of 64-column tiles (B * ceil(Nq / 64))
  // round 25: ONE form whatever B and Nq (the throughput kernel's 64-row x 32-column wave tiles, chunks in ascending order),
  // for callers that promise a column's bits independent of the batch it is computed in (denoiser.hip); 0: the tree above
  int fixed_form;
};

// The kernel launch_conv takes for (a, B): which of the frame-rate kernels, and for the throughput kernel its tile tuple
// and ring / prune flags (include/vispeech_hip.h: VSP_CONV_FORM_*; kernel == VSP_CONV_FORM_NONE: launch_conv answers
// hipErrorInvalidValue).  A pure host function -- no HIP call -- of the arguments, B and the VSP_EXPERIMENTS knobs: the
// ONE place the grid-size thresholds live, shared with the tests through vsp_conv1d_ex (ops.hip).
using ConvForm = vsp_conv_form;
ConvForm conv_form(const ConvArgs& a, int B);
// the kernel and tile shape are chosen by conv_form
hipError_t launch_conv(const ConvArgs& a, int B, hipStream_t s);
// Column-tile form of a 1x1 convolution (conv_cols.hip): every output row of a 64-column tile in ONE block.
// ln_gamma / ln_beta != NULL: out = LayerNorm_channels(conv + bias + res) * gamma + beta (M = Cin = 192, no masks).
bool conv_cols_supported(const ConvArgs& a);
hipError_t launch_conv_cols(const ConvArgs& a, int B, hipStream_t s, const float* ln_gamma = nullptr,
                            const float* ln_beta = nullptr);
size_t packed_conv_floats(int M, int Cin, int K);
// W(row, ci, tap) accessor -> packed buffer (host).  dst has packed_conv_floats(M,Cin,K) floats.
void pack_conv_weights(float* dst, int M, int Cin, int K, const float* dense /* [M][Cin][K] */);
void pack_conv_weights_f16s(float* dst, int M, int Cin, int K, const float* dense /* [M][Cin][K] */);

// The channels-last split-f16 kernels take their weights AND biases * G16_WSCALE and unscale every result by G16_UNSCALE
// (powers of two: exact; g16_common.h "ONE accumulator per tile"): pack_g16_weights scales the weights itself, whoever
// fills a bias array for these kernels (weights.cpp, upload_cl_conv in ops.hip) scales the bias.
#ifndef G16_WSCALE_V          // (timing experiments only: -DG16_WSCALE_V=1.f -DG16_UNSCALE_V=1.f is the unscaled form)
#define G16_WSCALE_V 256.f
#define G16_UNSCALE_V (1.f / 256.f)
#endif
constexpr float G16_WSCALE = G16_WSCALE_V, G16_UNSCALE = G16_UNSCALE_V;

#ifdef __HIPCC__
// THE operand split of two fp32 values into f16 hi / lo pairs (hi | lo packed two per register), shared by every split-f16
// kernel (g16_common.h g16_split2; conv_mfma.hip) -- one function, so that the implementations stay bit-identical.
// Round 6 form, FOUR vector instructions per two values (rounds 3-5: six):
//   hi  = v_cvt_pk_f16_f32(x0, x1): both values ROUNDED to f16 (nearest even) in one instruction; +-inf beyond the f16
//         range -- an activation the split cannot represent poisons the product (inf / NaN down to the waveform, where
//         conv_post raises the context's sticky flag: vsp_status) where rounds 2-5's v_cvt_pkrtz saturated silently;
//   lo  = x - hi: v_fma_mix_f32 reads the f16 half directly (hi * -1.0 + x, ONE rounding of an exactly representable
//         difference: exact), so no v_and_b32 truncation and no conversion back -- one instruction per value;
//   lo pair packed by v_cvt_pkrtz_f16_f32 (|lo| <= 2^-11 |x|: 13 significant bits truncated to f16's 11, i.e. x to
//         2^-22 relative; an f16 subnormal -- multiples of 2^-24 -- where |x| < 2^-3).
// Rounds 3-5 cut the mantissa (v_and_b32 0xffffe000) for hi and subtracted in fp32: same precision class (hi truncated:
// |lo| <= 2^-10 |x|), two instructions more.  VSP_SPLIT_FORM=0 builds that form (timing A/B only; it saturates).
// (The operands come from compiler-generated vector instructions, never straight from an MFMA result: see the hazard
// note in g16_common.h.)
// A kernel reports a numeric-range event in the context's status word (vsp_status): pinned host memory mapped into the
// device's address space, so the OR is a SYSTEM-scope atomic (the host reads / clears the same word without synchronising)
__device__ __forceinline__ void vsp_raise_flag(unsigned* flags, unsigned bit) {
  __hip_atomic_fetch_or(flags, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
#ifndef VSP_SPLIT_FORM
#define VSP_SPLIT_FORM 1
#endif
__device__ __forceinline__ void vsp_split_pair(float x0, float x1, unsigned& hi, unsigned& lo) {
#if VSP_SPLIT_FORM == 0
  const float h0 = __uint_as_float(__float_as_uint(x0) & 0xffffe000u), h1 = __uint_as_float(__float_as_uint(x1) & 0xffffe000u);
  float l0, l1;
  asm("v_sub_f32 %0, %1, %2" : "=v"(l0) : "v"(x0), "v"(h0));     // (plain f32 instructions: hipcc would SLP-pack them)
  asm("v_sub_f32 %0, %1, %2" : "=v"(l1) : "v"(x1), "v"(h1));
  hi = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(h0, h1));
  lo = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(l0, l1));
#else
  float l0, l1;
  asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(hi) : "v"(x0), "v"(x1));
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(l0) : "v"(hi), "v"(x0));
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(l1) : "v"(hi), "v"(x1));
  lo = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(l0, l1));
#endif
}
#endif

// ------------------------------------------------------------------------------------------
// channels-last split-f16 vocoder conv (gen16.hip): x [B][T][Cin], out [B][T][Cout]
struct ClConvArgs {
  const float* x; long x_bs; int x_ts;
  const uint16_t* wh;                       // packed f16 A-fragment image, hi | lo interleaved (pack_g16_weights)
  const float* bias;                        // [Cout] or null
  float* out; long o_bs; int o_ts;
  const float* res; long r_bs; int r_ts;
  int Cin, Cout, K, dil, pad;
  int T_in, Nq;
  int in_act; float in_slope;
  int acc_prev; float div;
  int phases, ups_p, T_store;               // polyphase transposed conv: row n = phases*q + ph - ups_p
  int terms;                                // 3 = fp32-accurate split product (default), 1 = plain f16 operands
  // Operand images (round 4; terms == 3, phases == 1): layout [chunk32][hi | lo][plane][cl_img_tpad(T)][8 halfs] per
  // utterance, CL_IMG_PADF zero rows in front of time 0 and CL_IMG_PADB behind time T - 1 (launch_cl_img_zero_pads).
  //   x_img: read the input from a producer-written image instead of x (K >= 3; in_act / in_slope are then the
  //          PRODUCER's business); o_img: also (out != NULL) or only (out == NULL) write leaky_relu(result, oi_slope)
  //          as the next convolution's image.
  const uint16_t* x_img; long xi_bs; int xi_tpad;   // batch stride in halfs, padded rows per plane
  uint16_t* o_img; long oi_bs; int oi_tpad; float oi_slope;
  int pt_gx, pt_gy, pt_total;               // set by the persistent launcher: time tiles, row groups, tiles in all
  // Ragged batch (round 5, "trimmed tails"): glen[b] (device, int32) = frames of utterance b this launch computes; its
  // extents are then T_in = glen[b] * g_in, Nq = T_in + (Nq - T_in of the launch), T_store = glen[b] * g_store instead of
  // the launch-wide values above (which stay the MAXIMUM: grid size, strides, image padding).  Rows at and beyond an
  // utterance's own extent read as zero and are never stored: the tensor ENDS there for that utterance.  NULL = uniform.
  const int* glen; int g_in, g_store;
};
// The kernel a channels-last launcher takes for its arguments and the columns one tile of it stores
// (include/vispeech_hip.h: VSP_CL_KERNEL_*, vsp_cl_launch_route; kernel == VSP_CL_KERNEL_NONE: the launcher answers
// hipErrorInvalidValue).  The *_route functions below are pure host functions -- no HIP call; they read pointers as
// flags and addresses only -- and the ONE place each launcher's decision ladder lives: the launcher switches on its route,
// vsp_cl_block_ex (ops.hip) reports it to the tests.  A route does not repeat the launcher's argument checks.
using ClRoute = vsp_cl_launch_route;
constexpr int CL_IMG_PADF = 64, CL_IMG_PADB = 320;
inline int cl_img_tpad(int T) { return T + CL_IMG_PADF + CL_IMG_PADB; }
inline size_t cl_img_halfs(int C, int T) { return (size_t)C * 2 * cl_img_tpad(T); }   // per utterance
// zero the pad rows of B utterances' images (the data rows are the producer's); glen != NULL: utterance b's data rows end
// at glen[b] * grate (<= T), the CL_IMG_PADB zero rows follow there
hipError_t launch_cl_img_zero_pads(uint16_t* img, int B, int C, int T, hipStream_t s, const int* glen = nullptr, int grate = 0);

// Fused ResBlock1 conv pair on channels-last activations (gen16.hip):
//   out = x + conv2(lrelu(conv1(lrelu(x), dil) + b1), 1) + b2  [+ out] [/ div];  x != out.
struct ClPairArgs {
  const float* x; long x_bs;                // [B][T][C], batch stride in elements
  const uint16_t* w1h; const float* b1;     // conv1 (dilation dil): packed f16 fragment image, bias
  const uint16_t* w2h; const float* b2;     // conv2 (dilation 1)
  float* out; long o_bs;
  int C, K, dil, T;
  float slope;                              // leaky-relu slope applied to both convs' inputs
  int acc_prev; float div;                  // out = (result + out) / div
  int terms;                                // 3 = split product, 1 = plain f16 operands
  int ring;                                 // 1: the LDS-ring pair kernel (g16_pair) even where the register-weights one exists
  int rw64;                                 // 1: the register-weights kernel for 64-channel kernel-3 pairs (g16_rw64; opt-in, VSP_RW64=1)
  int tiles;                                // set by the launcher: tiles per utterance
  int xrows;                                // set by the launcher: staged window rows
  const int* glen; int grate;               // ragged batch (see ClConvArgs): utterance b's T = glen[b] * grate; NULL = uniform
  int B;                                    // set by the launcher (persistent kernels walk the utterances themselves)
};
// Fused ResBlock1 CHAIN on channels-last activations (gen16.hip): np conv pairs back to back in one launch,
//   x_{p+1} = x_p + conv2_p(lrelu(conv1_p(lrelu(x_p), dil_p) + b1_p), 1) + b2_p,   out = x_np [+ out] [/ div];  x != out.
// The running x_p stays in registers (fp32), the convolution inputs in LDS; a block recomputes the chain's halo.
struct ClChainArgs {
  const float* x; long x_bs;
  float* out; long o_bs;
  const uint16_t* w[6]; const float* b[6];  // conv1, conv2 of pair 0, 1, 2
  int dil[3]; int np;
  int C, K, T;
  float slope;
  int acc_prev; float div;
  int terms;
  int ring;                                 // 1: the LDS-ring chain kernel (g16_chain) even where the register-weights one exists
  int tiles, halo;                          // set by the launcher: tiles per utterance, columns recomputed per side
  const int* glen; int grate;               // ragged batch (see ClConvArgs): utterance b's T = glen[b] * grate; NULL = uniform
  int B;                                    // set by the launcher
};
// the kernel-3 ResBlock of the 32-channel stage as a role pipeline with the weights in registers (gen16_rc.hip);
// launch_g16_chain routes there unless ClChainArgs::ring (VSP_CHAIN_RING=1) asks for the LDS-ring chain (bit-identical)
bool g16_rc_supported(int C, int K, const int* dil, int np, int terms, int acc_prev);
hipError_t launch_g16_rc(const ClChainArgs& a, int B, hipStream_t s);
int g16_rc_tile_cols(int K, const int* dil, int np);        // RC_BT - 2 * halo
bool g16_chain_supported(int C, int K, const int* dil, int np);
// RC, or the LDS-ring tile: CHAIN (32 channels: two 4-wave blocks of 256 columns per CU; 64: 256; 128: 128) or CHAIN_WIDE
// (32 channels, one 8-wave block of 512 columns); tile_cols = the block's columns - 2 * halo
ClRoute g16_chain_route(const ClChainArgs& a);
hipError_t launch_g16_chain(const ClChainArgs& a, int B, hipStream_t s);
// Fused ResBlock2 on channels-last activations (gen16_rb2.hip, round 7): both convolutions of the block in one launch,
//   y = x + conv_a(lrelu(x), dil[0]) + b_a,   out = y + conv_b(lrelu(y), dil[1]) + b_b  [+ out] [/ div];  x != out.
struct ClRb2Args {
  const float* x; long x_bs;
  float* out; long o_bs;
  const uint16_t* w[2]; const float* b[2];  // conv_a, conv_b: packed f16 fragment images, biases (* G16_WSCALE)
  int dil[2];
  int C, K, T;
  float slope;
  int acc_prev; float div;
  int terms;
  int tiles, halo;                          // set by the launcher: tiles per utterance, columns recomputed per side
  const int* glen; int grate;               // ragged batch (see ClConvArgs): utterance b's T = glen[b] * grate; NULL = uniform
};
bool g16_rb2_supported(int C, int K, const int* dil);
ClRoute g16_rb2_route(const ClRb2Args& a);                  // RB2; variant 1 = the 512-column block; tile_cols = columns - 2 * halo
hipError_t launch_g16_rb2(const ClRb2Args& a, int B, hipStream_t s);
// C16 (16 -> 16), UPS (the streaming up-convolutions), PIPE, CONV_IMG or CONV with the row tile in `rows` (terms 3: chosen
// from the grid size B * ceil(Nq / 256)); variant 1 = the image-only epilogue through the LDS.  Every tile stores 256 columns
// (UPS: 16 input times; C16: see g16_c16_route).
ClRoute g16_conv_route(const ClConvArgs& a, int B);
hipError_t launch_g16_conv(const ClConvArgs& a, int B, hipStream_t s);
// The 16-channel last stage of a five-stage generator (gen16_c16.hip): a SEQUENCE of 1 .. 6 convolutions 16 -> 16 of one
// channels-last tensor in one launch.  Step i convolves the leaky-relu of its input with w[i] at dilation dil[i]; its result
// (+ the running tensor when add[i], which it then replaces) is the next step's input.  The running tensor starts as res
// (NULL: x).  The last step's result [+ out] [/ div] is stored.  x != out.
//   ResBlock1:  steps [conv(d_p), conv(1) + add] per pair;  ResBlock2:  [conv(d) + add] x 2;  one convolution:  one step.
struct ClC16Args {
  const float* x; long x_bs;
  const float* res; long r_bs;
  float* out; long o_bs;
  const uint16_t* w[6]; const float* b[6];  // pack_g16c16_weights images, biases (* G16_WSCALE)
  int dil[6]; int add[6];
  int nsteps, K, T;
  float slope;
  int acc_prev; float div;
  int terms;
  int tiles, halo;                          // set by the launcher: tiles per utterance, columns recomputed per side
  const int* glen; int grate;               // ragged batch (see ClConvArgs): utterance b's T = glen[b] * grate; NULL = uniform
};
constexpr int G16_C16_BT = 512;             // columns per block; a launch stores G16_C16_BT - 2 * sum_i (K - 1) dil[i] / 2 of them
bool g16_c16_supported(int K, const int* dil, int nsteps);
ClRoute g16_c16_route(const ClC16Args& a);                  // C16; tile_cols = G16_C16_BT - 2 * halo
hipError_t launch_g16_c16(const ClC16Args& a, int B, hipStream_t s);
// the step lists (cl_args.h, cl_c16_steps) of np pairs of a ResBlock1 and of a ResBlock2
bool g16_c16_rb1_supported(int K, const int* dil, int np);
bool g16_c16_rb2_supported(int K, const int* dil);
// 16 -> 16 weights [16][16][K] in 16x16x32 A-fragment order, one K-step = TWO TAPS x 16 channels: [step][hi | lo][lane][8 halfs],
// lane l: output channel l & 15, tap 2 step + (l >> 5), input channels 8 ((l >> 4) & 1) .. + 7; an odd K's last step has a
// zero second tap.  * G16_WSCALE like pack_g16_weights.
size_t packed_g16c16_halfs(int K);
void pack_g16c16_weights(uint16_t* dst, int K, const float* dense /* [16][16][K] */);
inline bool cl_is_c16(int Cout, int Cin, int phases) { return Cout == 16 && Cin == 16 && phases == 1; }
// image-input convolutions on the 128-row tile as persistent blocks pipelined across tiles (gen16_pipe.hip):
// launch_g16_conv routes tiles of at most 28 steps there (VSP_G16_PIPE=0: never, =1: always -- bit-identical)
bool g16_pipe_supported(const ClConvArgs& a);
hipError_t launch_g16_pipe(const ClConvArgs& a, int B, hipStream_t s);
bool g16_pair_supported(int C, int K, int dil);
// PP (128 channels), RW, RW64, or the LDS-ring tile PAIR (variant = waves per block); tile_cols = conv1's columns - (K - 1)
ClRoute g16_pair_route(const ClPairArgs& a);
hipError_t launch_g16_pair(const ClPairArgs& a, int B, hipStream_t s);
// the same pair with the weights held in registers by persistent blocks (gen16_rw.hip: 32 channels, kernel 7 / 11);
// launch_g16_pair routes there unless ClPairArgs::ring (VSP_PAIR=ring) asks for the LDS-ring kernel (second implementation, bit-identical)
bool g16_rw_supported(int C, int K, int dil, int terms);
int g16_rw_tile_cols(int K);                                // RW_BT - (K - 1)
hipError_t launch_g16_rw(const ClPairArgs& a, int B, hipStream_t s);
// ... and the kernel-3 pairs of the 64-channel stage (gen16_rw64.hip, round 5: two row halves x two column halves per role)
bool g16_rw64_supported(int C, int K, int dil, int terms);
int g16_rw64_tile_cols();                                   // R6_BT - (R6_K - 1)
hipError_t launch_g16_rw64(const ClPairArgs& a, int B, hipStream_t s);
// the pair of the 128-channel stage on the ping-pong tile, kernel 3 / 7 (gen16_pp.hip); VSP_PP=0 (read per context): two launches (bit-identical)
bool g16_pp_supported(int C, int K, int dil, int terms);
int g16_pp_tile_cols(int K);                                // 192 - (K - 1)
hipError_t launch_g16_pp(const ClPairArgs& a, int B, hipStream_t s);
size_t packed_g16_halfs(int rows, int Cin, int K);
void pack_g16_weights(uint16_t* dst, int rows, int Cin, int K, const float* dense /* [rows][Cin][K] */);
// HiFi-GAN's up-convolution (torch ConvTranspose1d, weight w[Cin][Cout][k], stride s, k = kt s, padding p = (k - s) / 2,
// reference models.py:253-256) in polyphase form: one kt-tap convolution per phase r < s over the input padded by kt - 1,
//   out[s q + r - p][co] = bias[co] + sum_{tap < kt} sum_ci x[q - (kt - 1) + tap][ci] * w[ci][co][s (kt - 1 - tap) + r]
// for q <= T (output rows outside [0, s T) dropped).  The offset of that weight in w: the ONE mapping behind the model's
// packing (weights.cpp: dec.ups.*) and the stand-alone operators (ops.hip: vsp_cl_conv_transpose1d, vsp_conv_transpose1d).
inline size_t ups_weight_offset(int ci, int co, int r, int tap, int Cout, int s, int kt) {
  return ((size_t)ci * Cout + co) * ((size_t)kt * s) + (size_t)s * (kt - 1 - tap) + r;
}
// mel[b][m][t] = log(max(sum_{f in [lo[m], hi[m])} basis[m][f] * spec[b][f][t], 1e-5))  (reference mel_processing.py:16-22, 73-82)
hipError_t launch_spec_to_mel(const float* spec, const float* basis, const int* lo, const int* hi, float* mel, int B,
                              int n_freq, int n_mels, int T, hipStream_t s);
// y = transpose(x) * scale (the generator's entry: the context's activation scale, model.h)
hipError_t launch_transpose_ct(const float* x, long x_bs, long x_cs, float* y, long y_bs, int y_ts, int B, int C,
                               int T, hipStream_t s, float scale = 1.f);
// o = tanh(unscale * conv(lrelu(x)));  flags != NULL: VSP_FLAG_NONFINITE_WAVE is raised there when a sum is inf / NaN
hipError_t launch_conv_post_cl(const float* x, long x_bs, int x_ts, const float* w, int C, int K, float slope,
                               float* o, long o_bs, int B, int T, hipStream_t s, const int* glen = nullptr, int grate = 0,
                               float unscale = 1.f, unsigned* flags = nullptr);
// Trimmed tails (round 5).  The generator's input behind an utterance's last frame is exactly zero (reference
// models.py:720: z * x_mask), so its output there is a bias-driven signal that depends on the distance to the utterance's
// end and to the tensor's end only: periodic in one frame once the receptive field away from both.
// Output frame F depends on input frames [F - back, F + fwd] (api_generator.hip, generator_frame_dependence).
// Silence table (round 18): the steady-state frame and the fwd tensor-end frames depend on the weights and on g only, so a
// context keeps them per speaker (model.h, vsp_ctx::tail_table: row s = [steady frame | fwd end frames] for g = emb_g[s]).
// An utterance served by the table needs the zero-input context only as far as the layers BEHIND stage 0 see: reach1 = the
// forward dependence, in frames, of the output on stage 0's output tensor (api_generator.hip, generator_support).
//   gen_tail_rows:  tail_row[b] = the lowest s with g[b] == emb_g[s] bit for bit (gin words each), else -1; one block per b;
//   gen_plan:  glen0[b] = len[b] + back + 1 + fwd where that is < T (else T): the frames conv_pre's successors up to and
//              including stage 0 compute for b;  glen1[b] = len[b] + back + reach1 where tail_row[b] >= 0 and
//              len[b] + back + fwd <= T (no frame before len + back sees the true tensor end), else glen0[b]: the frames
//              stage 1 .. conv_post compute.  tail_row == NULL: glen1 = glen0;
//   gen_tail_fill:  glen1[b] < glen0[b]: frames [len + back, T - fwd) of o[b] = the table row's steady frame, frames
//                   [T - fwd, T) = its end frames;  else glen0[b] < T: frames [len + back + 1, T - fwd) = frame len + back (the
//                   steady state), frames [T - fwd, T) = frames [len + back + 1, len + back + 1 + fwd) (the computed tensor
//                   end, staged in LDS);  else nothing.  up = samples per frame; a table row is (1 + fwd) * up floats.
hipError_t launch_gen_tail_rows(const float* g, const float* emb_g, int n_speakers, int gin, int B, int* tail_row, hipStream_t s);
hipError_t launch_gen_plan(const int64_t* lengths, int B, int T, int back, int fwd, int reach1, const int* tail_row, int* glen0,
                           int* glen1, hipStream_t s);
hipError_t launch_gen_tail_fill(float* o, long o_bs, const int64_t* lengths, const int* glen0, const int* glen1, const int* tail_row,
                                const float* table, int B, int T, int back, int fwd, int up, hipStream_t s);
// Isolated mode (round 10; include/vispeech_hip.h, vsp_set_isolated): every utterance of a batch as a B = 1 call on its
// own unpadded tensors computes it.  The generator then ENDS utterance b's tensor at its own length -- the same per-utterance
// extent as above with no frames behind the utterance -- and the padded rest of the waveform is zero.
//   gen_plan_isolated:  glen[b] = clamp(lengths[b], 1, T) (an empty utterance computes one frame, which gen_tail_zero erases);
//   gen_tail_zero:      o[b][clamp(lengths[b], 0, T) * up .. T * up) = 0.
hipError_t launch_gen_plan_isolated(const int64_t* lengths, int B, int T, int* glen, hipStream_t s);
hipError_t launch_gen_tail_zero(float* o, long o_bs, const int64_t* lengths, int B, int T, int up, hipStream_t s);

// ------------------------------------------------------------------------------------------
// attention with windowed relative position (reference attentions.py:148-179), f32 MFMA.
// qkv [B][3*H][T]: rows [0,H) = q, [H,2H) = k, [2H,3H) = v; out [B][H][T].
hipError_t launch_attention(const float* qkv, long qkv_bs, long qkv_cs, const float* emb_k,
                            const float* emb_v, const int64_t* lengths, float* out, long o_bs,
                            long o_cs, int B, int H, int n_heads, int T, int window, int ksplit_mode, hipStream_t s);

// the same on the f16 matrix core with split operands, one pass (attention_f16s.hip); workspace = 3 *
// attn_pack_bytes(B, n_heads, H / n_heads, T) bytes (the packed q | k | v operand images).  block_mode < 0: the launcher
// picks the block form from the grid size; 0 / 1 force the 64-query form with two key streams / the 128-query form
size_t attn_pack_bytes(int B, int n_heads, int DK, int T);
hipError_t launch_attention_f16s(const float* qkv, long qkv_bs, long qkv_cs, const float* emb_k, const float* emb_v,
                                 const int64_t* lengths, float* out, long o_bs, long o_cs, int B, int H, int n_heads, int T,
                                 int window, void* workspace, hipStream_t s, int block_mode = -1);
// conv_q | conv_k | conv_v of x * x_mask AND the packing of their results in one launch: fills `workspace` with the images
// launch_attention_f16s(qkv = NULL, ...) then consumes.  wg: pack_g16_weights of the stacked [3H][H] projection.
bool attn_qkv_pack_supported(int H, int n_heads);
hipError_t launch_attn_qkv_pack_f16s(const float* x, long x_bs, long x_cs, const uint16_t* wg, const float* bias,
                                     const int64_t* lengths, int B, int H, int n_heads, int T, void* workspace, hipStream_t s);

// ------------------------------------------------------------------------------------------
// small kernels (misc.hip)
// y = LN_channels(x (+ res)) * gamma + beta  (reference modules.py:29-32), eps 1e-5
hipError_t launch_layernorm(const float* x, long x_bs, long x_cs, const float* res, long r_bs, long r_cs,
                            const float* gamma, const float* beta, float* y, long y_bs, long y_cs,
                            int B, int C, int T, hipStream_t s);
// x[b][c][t] = emb[ids[b][t]][c] * scale
hipError_t launch_embed(const int64_t* ids, const float* emb, int n_vocab, float scale, float* x,
                        long x_bs, long x_cs, int B, int C, int T, hipStream_t s);
// g[b][c] = table[sid[b]][c]
hipError_t launch_gather_rows(const int64_t* idx, const float* table, int n_rows, float* out, int B, int C,
                              hipStream_t s);
// y[b][c][t] = x[b][c][t] + c[b][c]  (optionally * mask)
hipError_t launch_add_cond(const float* x, long x_bs, long x_cs, const float* cond, long cond_bs, float* y,
                           long y_bs, long y_cs, int B, int C, int T, hipStream_t s);
// out[b][t] = bias + sum_c w[c] * x[b][c][t] (* mask_in on x, * mask_out on result)
hipError_t launch_chan_dot(const float* x, long x_bs, long x_cs, const float* w, const float* bias,
                           const int64_t* lengths, int mask_in, int mask_out, float* out, int B, int C, int T,
                           hipStream_t s);
// x[b][c][t] += bias[c] + sum_j w[c][j] * s[b][t + j - 1]   (Conv1d(1,C,3,padding=1), unmasked)
hipError_t launch_prenet_add(float* x, long x_bs, long x_cs, const float* w, const float* bias,
                             const float* sig, int B, int C, int T, hipStream_t s);
// duration / F0 / energy formulas (reference models.py:681-708)
hipError_t launch_duration_from_logw(const float* logw, const int64_t* lengths, float scale, float* dur,
                                     int B, int T, hipStream_t s);
hipError_t launch_pitch(const float* pitch_ctl, const float* lf0_pred, float scale, float* lf0, float* f0,
                        int n, hipStream_t s);
hipError_t launch_energy(const float* energy_ctl, const float* e_pred, float scale, float* norm_e,
                         float* energy, int n, hipStream_t s);
// cum[b][i] = sum_{k<=i} max(int(d[b][k]),0); frame_lengths[b] = cum[b][Tp-1]
hipError_t launch_duration_cumsum(const float* dur, int32_t* cum, int64_t* frame_lengths, int B, int Tp,
                                  hipStream_t s, unsigned* flags = nullptr);
// out[b][c][f] = f < cum[b][Tp-1] ? x[b][c][upper_bound(cum[b], f)] : 0
hipError_t launch_length_regulate(const float* x, long x_bs, long x_cs, const int32_t* cum, float* out,
                                  long o_bs, long o_cs, int B, int C, int Tp, int Tf, hipStream_t s);
// z_p = m_p + noise * exp(logs_p) * noise_scale ; x_mask[b][t] = t < len[b]
hipError_t launch_reparam(const float* m_p, const float* logs_p, const float* noise, float noise_scale,
                          float* z_p, long n, hipStream_t s, float* copy = nullptr, unsigned* flags = nullptr);
// out[i] = standard normal draw first + i of the Philox4x32-10 stream keyed by `seed` (misc.hip)
hipError_t launch_randn(uint64_t seed, long first, long n, float* out, hipStream_t s);
hipError_t launch_mask_u8(const int64_t* lengths, uint8_t* mask, int B, int T, hipStream_t s);
// isolated mode: out[b][c][t] = t < L ? element c * L + t of the Philox stream keyed seeds[b] : 0, L = max(row_len[b], 0) --
// the [C][L] tensor launch_randn(seeds[b], 0, C * L) draws for utterance b alone, inside a [B][C][T] batch tensor
hipError_t launch_randn_ragged(const uint64_t* seeds, const int64_t* row_len, int B, int C, int T, float* out, hipStream_t s);
// p_k[b][t] = 0 for t >= lengths[b], k < 4 ([B][T] tensors; NULL entries skipped): the phoneme-rate signals of isolated mode
hipError_t launch_mask_rows(const int64_t* lengths, int B, int T, float* p0, float* p1, float* p2, float* p3, hipStream_t s);
// out[i][b] = max(lengths[b], 0) * rate[i], i < n <= 9: an utterance's extent at every stage rate of the channel-major generator
hipError_t launch_stage_lengths(const int64_t* lengths, int B, const long* rate, int n, int64_t* out, hipStream_t s);
// o[b][t] = tanh( sum_c sum_j w[c][j] * lrelu(x[b][c][t+j-pad], slope) )  (conv_post, no bias); tlen != NULL: utterance b's
// tensor ends at min(T, tlen[b]) -- nothing behind it is read or written
hipError_t launch_conv_post(const float* x, long x_bs, long x_cs, const float* w, int C, int K, float slope,
                            float* o, long o_bs, int B, int T, hipStream_t s, unsigned* flags = nullptr,
                            const int64_t* tlen = nullptr);
hipError_t launch_copy3(const float* x, long x_bs, long x_cs, float* y, long y_bs, long y_cs, int B, int C,
                        int T, hipStream_t s);
// x[b][c][t] = 0 for t >= lengths[b]
hipError_t launch_mask3(float* x, long x_bs, long x_cs, const int64_t* lengths, int B, int C, int T, hipStream_t s);
hipError_t launch_rq_spline(int64_t n, int nb, const float* x, const float* uw, const float* uh,
                            const float* ud, int inverse, float tail_bound, float* y, float* lad,
                            hipStream_t s);

// Streaming for batched requests (stream_rows.hip; include/vispeech_hip.h, vsp_generator_stream_rows).  The per-row
// descriptors are kernel ARGUMENTS (by value): no copy to the device, nothing to keep alive behind the launch.
constexpr int STREAM_ROWS_MAX = 64;
struct StreamGatherRow {     // 32 B: the window [lo, hi) of one utterance's latent z[c * cs + t] and its speaker vector
  const float* z; long cs; const float* g; int lo, hi;
};
struct StreamGatherRows { StreamGatherRow r[STREAM_ROWS_MAX]; };
struct StreamCollectRow { int off, n; };   // row b delivers samples [off, off + n) of its span waveform
struct StreamCollectRows { StreamCollectRow r[STREAM_ROWS_MAX]; };
// zp[b][c][t] = t < hi_b - lo_b ? z_b[c * cs_b + lo_b + t] : 0 for t < S4 (zp [B][C][S4], 16-byte aligned, S4 % 4 == 0,
// every window <= S4);  gp[b][k] = g_b[k], k < gin;  len[b] = hi_b - lo_b.  One launch.
hipError_t launch_stream_gather(const StreamGatherRows& rows, int B, int C, int S4, int gin, float* zp, float* gp,
                                int64_t* len, hipStream_t s);
// out[b][i] = i < n_b ? o_span[b * o_bs + off_b + i] : 0 for i < out_stride; float32, or int16 by the rule of
// vsp_output_chunk (pcm != 0).  off_b + n_b <= o_bs and n_b <= out_stride, checked before the launch.
hipError_t launch_stream_collect(const float* o_span, long o_bs, const StreamCollectRows& rows, int B, void* out,
                                 long out_stride, int pcm, hipStream_t s);

// The ragged output stage (resample.hip; include/vispeech_hip.h, vsp_generator_stream_rows_output): instead of the collect,
// row b's n new samples o_span[b * o_bs + off ..) -- input samples [x_first, x_first + n) of its utterance -- and its history
// hist_in = samples [k0, x_first) go through the output stage's filter; m0, m1, k0, k1 follow from (x_first, n, ended) by
// stream_output_plan, on the host and on the device alike.
struct StreamOutRow {        // 40 B
  const float* hist_in; float* hist_out; int64_t x_first; int off, n, ended, pad;
};
struct StreamOutRows { StreamOutRow r[STREAM_ROWS_MAX]; };
struct StreamOutPlan { int64_t m0, m1, k0, k1; };
struct StreamOutFilter { const float* tab; int L, M, H, J, P; };   // the context's configured output stage (tab [P][L])
__host__ __device__ inline int64_t stream_output_complete(int64_t n_seen, bool ended, int64_t L, int64_t M, int64_t H) {
  // vispeech_amd.output_stage.complete_outputs: output m is final when m M + H < L n_seen, or when the input has ended
  const int64_t total = (n_seen * L + M - 1) / M, t = L * n_seen - H;
  if (ended) return total;
  const int64_t c = t <= 0 ? 0 : (t + M - 1) / M;
  return c < total ? c : total;
}
__host__ __device__ inline int64_t stream_output_history_start(int64_t m, int64_t L, int64_t M, int64_t H) {
  // vispeech_amd.output_stage.history_start: the first input sample output m reads, ceil((m M - H) / L) clamped to 0
  const int64_t t = m * M - H;
  return t <= 0 ? 0 : (t + L - 1) / L;
}
__host__ __device__ inline StreamOutPlan stream_output_plan(int64_t x_first, int64_t n, bool ended, int64_t L, int64_t M,
                                                            int64_t H) {
  StreamOutPlan p;
  p.m0 = stream_output_complete(x_first, false, L, M, H);
  p.m1 = stream_output_complete(x_first + n, ended, L, M, H);
  const int64_t h0 = stream_output_history_start(p.m0, L, M, H), h1 = stream_output_history_start(p.m1, L, M, H);
  p.k0 = h0 < x_first ? h0 : x_first;
  p.k1 = h1 < x_first + n ? h1 : x_first + n;
  return p;
}
// out[b][j] = j < m1_b - m0_b ? y_b[m0_b + j] : 0 for j < out_stride (float32, or int16 by the rule of vsp_output_chunk);
// hist_out_b[j] = sample k1_b + j for k1_b + j < x_first_b + n_b.  K = the capacity of a history buffer in floats.  Checked
// before the launch: every m1 - m0 <= out_stride, both histories <= K, hist_in != hist_out, off + n <= o_bs.  One launch.
hipError_t launch_stream_output(const float* o_span, long o_bs, const StreamOutRows& rows, int B, const StreamOutFilter& f,
                                int K, void* out, long out_stride, int pcm, hipStream_t s);

// The input stage (input_stage.hip; include/vispeech_hip.h, vsp_input_rows): raw samples in an encoding VSP_IN_* at the
// caller's rate -> float32 at the model's rate.  A row is a window [in_first, in_first + in_len) of one recording and the
// output samples [m0, m1) to compute from it; out[m1 - m0 .. out_fill) is written as 0.  (n_total of vsp_input_row stays on
// the host: the window ends at or before it, and nothing outside the window is read.)
struct InputRow {            // 56 B
  const void* in; int64_t in_first, in_len; float* out; int64_t m0, m1, out_fill;
};
struct InputRows { InputRow r[STREAM_ROWS_MAX]; };
struct InputFilter { const float* tab; int L, M, J, P; };          // a configured input rate (tab [P][L])
// The 16-bit linear value of a G.711 code byte, by the arithmetic of include/vispeech_hip.h (host table and kernel alike)
__host__ __device__ inline int g711_ulaw_linear(int c) {
  const int u = ~c & 0xFF, e = (u >> 4) & 7, q = u & 15, t = (((q << 3) + 0x84) << e) - 0x84;
  return (u & 0x80) ? -t : t;
}
__host__ __device__ inline int g711_alaw_linear(int c) {
  const int a = (c ^ 0x55) & 0xFF, e = (a >> 4) & 7, q = a & 15;
  int t = (q << 4) + 8;
  if (e >= 1) t = (t + 0x100) << (e - 1);
  return (a & 0x80) ? t : -t;
}
// Checked before the launch: 1 <= B <= STREAM_ROWS_MAX, enc one of VSP_IN_*, a table, aligned non-null pointers.  One launch.
hipError_t launch_input_rows(const InputRows& rows, int B, const InputFilter& f, int enc, hipStream_t s);

// Output rows (output_rows.hip; include/vispeech_hip.h, vsp_output_rows): the ragged output stage with the row's rate AND
// encoding inside its descriptor.  m0, m1, k0, k1 are stream_output_plan of (x_first, n, ended) under the row's filter,
// computed on the host; `filt` indexes the launch's filter entries.
struct OutRow {              // 96 B
  const float* x; const float* hist_in; float* hist_out; void* out;
  int64_t x_first, n, m0, m1, k0, k1, out_fill;
  int enc, filt;
};
// a configured output rate (tab [P][L]) and how output_rows_kernel stages it: `pass` taps per staging pass, mode 0: the
// tile's span in LDS, mode 2: samples from global memory
struct OutFilter { const float* tab; int L, M, H, J, P, pass, mode, xs_words; };   // 40 B
constexpr int OUT_FILTERS_MAX = 8;                                  // = VSP_OUTPUT_RATES_MAX
constexpr int OUT_ROWS_PER_LAUNCH = (4096 - OUT_FILTERS_MAX * 40 - 16) / 96;     // 39: what 4 KiB of kernel arguments hold
struct OutRowsArgs { OutRow r[OUT_ROWS_PER_LAUNCH]; OutFilter f[OUT_FILTERS_MAX]; int out_tiles, pad; };
// The G.711 code byte of a 16-bit linear value, by the arithmetic of include/vispeech_hip.h ("output rows"): the
// truncating compressors, inverse to the two expanders above (host function and kernel alike)
__host__ __device__ inline int g711_ulaw_code(int s) {
  const int neg = s < 0, a = neg ? -s : s, mag = (a < 32635 ? a : 32635) + 0x84;
  const int e = (31 - __builtin_clz((unsigned)mag)) - 7, q = (mag >> (e + 3)) & 15;
  return ~((neg ? 0x80 : 0) | (e << 4) | q) & 0xFF;
}
__host__ __device__ inline int g711_alaw_code(int s) {
  const int neg = s < 0, mag = (neg ? ~s : s) >> 3;
  int e = mag ? (31 - __builtin_clz((unsigned)mag)) - 4 : 0;
  if (e < 0) e = 0;
  const int q = e == 0 ? (mag >> 1) & 15 : (mag >> e) & 15;
  return (((neg ? 0 : 0x80) | (e << 4) | q) ^ 0x55) & 0xFF;
}
// Checked before the launch: 1 <= B <= OUT_ROWS_PER_LAUNCH, every row's filt names an entry with a table.  One launch:
// grid (out_tiles + hist_blocks, B).
hipError_t launch_output_rows(OutRowsArgs& a, int B, hipStream_t s);

hipError_t launch_stft_frames(const float* audio, long a_bs, float* f, long f_bs, long f_cs, int B, int L, int n_fft,
                              int hop, int T, hipStream_t s);
hipError_t launch_stft_magnitude(const float* ri, long r_bs, long r_cs, float* spec, int B, int spec_ch, int T,
                                 hipStream_t s);

// Ragged spectrogram front end (spectrogram_ragged.hip): row b is the recording audio[b][0 .. n_b), n_b = n_samples[b]
// clamped to [0, L_max], with T_b = stft_ragged_frames(n_b) frames; grids come from T_max (the host never reads n_samples).
// The frame count of a recording of n samples: 0 where the reflect padding is undefined (n <= pad) or no window fits.
__host__ __device__ inline long stft_ragged_frames(long n, int n_fft, int hop) {
  const long pad = (n_fft - hop) / 2;
  if (n <= pad || n + 2 * pad < n_fft) return 0;
  return 1 + (n + 2 * pad - n_fft) / hop;
}
// frames of a tile whose span of samples fits the LDS budget (0: n_fft alone does not fit)
int stft_ragged_tile(int n_fft, int hop);
// f [B][n_fft][T_max] (strides f_bs, f_cs): f[b][n][t] = the reflect-padded row's sample t * hop + n for t < T_b, 0 behind;
// samples at and behind n_b are never read
hipError_t launch_stft_frames_ragged(const float* audio, long a_bs, const int64_t* n_samples, float* f, long f_bs, long f_cs,
                                     int B, int L_max, int n_fft, int hop, int T_max, hipStream_t s);
// spec [B][spec_ch][T_max] = sqrt(re^2 + im^2 + 1e-6) for t < T_b, exactly 0 behind; frames[b] = T_b
hipError_t launch_stft_magnitude_ragged(const float* ri, long r_bs, long r_cs, const int64_t* n_samples, float* spec,
                                        int64_t* frames, int B, int L_max, int n_fft, int hop, int spec_ch, int T_max,
                                        hipStream_t s);

// Denoiser and inverse STFT (denoiser.hip; include/vispeech_hip.h, vsp_denoise): the rows, their lengths and frame counts
// are those of the ragged spectrogram above; a row with n_samples[b] <= 0 is neither read nor written.
// ri [B][2 spec_ch][T_max] in place: X' = q X, q = max(m - strength[b] * bias[b][r], 0) / m (0 where m = 0), for t < T_b
hipError_t launch_denoise_subtract(float* ri, long r_bs, long r_cs, const int64_t* n_samples, const float* bias,
                                   const float* strength, int B, int L_max, int n_fft, int hop, int spec_ch, int T_max,
                                   hipStream_t s);
// frames of an overlap-add tile whose tile * hop outputs fit the LDS budget (0: one hop alone does not fit)
int istft_ola_tile(int n_fft, int hop);
// v [B][n_fft][T_max]: the windowed synthesis frames.  out[b][i] = (sum_t v[b][pad + i - t hop][t]) / (sum_t w2[pad + i - t hop])
// over the row's own frames t < T_b that cover the sample, both sums from 0 in ascending t; w2 [n_fft] = fl32(hann^2).
// hop divides n_fft, n_fft - hop is even.  Writes out[b][0 .. n_b) and nothing else.
hipError_t launch_istft_ola(const float* v, long v_bs, long v_cs, const int64_t* n_samples, const float* w2, float* out,
                            long o_bs, int B, int L_max, int n_fft, int hop, int T_max, hipStream_t s);
// f [n_fft][S] (row stride f_cs): f[n][s] = period[s][n mod hop]
hipError_t launch_denoise_bias_frames(const float* period, float* f, long f_cs, int S, int n_fft, int hop, hipStream_t s);
// bias [S][spec_ch] = sqrt(re^2 + im^2) of ri [2 spec_ch][S] (row stride r_cs)
hipError_t launch_denoise_bias_magnitude(const float* ri, long r_cs, float* bias, int S, int spec_ch, hipStream_t s);

// Live conversion windows (convert_window.hip; include/vispeech_hip.h, vsp_convert_stream_rows): row b is the window of
// frames [w0, w0 + Tw) of a recording that may still be arriving.  Descriptors by value, as for the streamed vocoder.
// The window that delivers frames [e0, e1) and the samples it reads -- the contract of vsp_convert_window_plan; host only.
int convert_window_plan(int n_fft, int hop, int halo, long n_known, int closed, int e0, int e1, int* w0, int* w1, long* s_lo,
                        long* s_hi);
struct ConvWinFrameRow {     // 48 B: sample s of the recording is audio[s - first]; n samples are known
  const float* audio; long first, n; int w0, Tw, closed, sid_src, sid_tgt, pad;
};
struct ConvWinFrameRows { ConvWinFrameRow r[STREAM_ROWS_MAX]; };
struct ConvWinNoiseRow { uint64_t seed; int w0, Tw; float scale; int pad; };      // 24 B
struct ConvWinNoiseRows { ConvWinNoiseRow r[STREAM_ROWS_MAX]; };
// f [B][n_fft][T_max]: f[b][k][j] = sample (w0_b + j) * hop + k - pad of the row, reflected at sample 0 and -- closed rows
// only -- at sample n_b, for j < Tw_b; exactly 0 behind.  len[b] = Tw_b, sid_src[b], sid_tgt[b]: the rows' scalars for the
// stages behind (written by the row's first block).  Every sample the windows read is inside the rows' buffers: the
// caller has run convert_window_plan.
hipError_t launch_window_frames(const ConvWinFrameRows& rows, float* f, long f_bs, long f_cs, int64_t* len, int64_t* sid_src,
                                int64_t* sid_tgt, int B, int n_fft, int hop, int T_max, hipStream_t s);
// spec [B][spec_ch][T_max] = sqrt(re^2 + im^2 + 1e-6) for j < len[b], exactly 0 behind
hipError_t launch_window_magnitude(const float* ri, long r_bs, long r_cs, const int64_t* len, float* spec, int B, int spec_ch,
                                   int T_max, hipStream_t s);
// out[b][c][j] = scale_b * element (w0_b + j) * C + c of the Philox stream keyed seed_b for j < Tw_b, else 0: FRAME-major in
// the stream, so a frame's noise does not depend on how long the recording turns out to be.  scale_b == 0: nothing drawn.
hipError_t launch_window_noise(const ConvWinNoiseRows& rows, int B, int C, int T_max, float* out, hipStream_t s);
// out[b][c][j] = j < n_b ? z[b][c][off_b + j] : 0 for j < span (z [B][C][T_max] dense; off_b + n_b <= T_max, n_b <= span)
hipError_t launch_window_cut(const float* z, const StreamCollectRows& rows, int B, int C, int T_max, float* out, int span,
                             hipStream_t s);

// Denoiser rows (denoiser.hip; include/vispeech_hip.h, vsp_denoise_rows): row b is the window of frames [w0, w0 + Tw) of a
// stream, framed by launch_window_frames above; frame t of the stream sits at column t - w0 of the three operands.
// Descriptors by value, as for the live conversion windows.
struct DenoiseSubRow { const float* bias; float strength; int Tw; };      // 16 B: the row's own bias [spec_ch]
struct DenoiseSubRows { DenoiseSubRow r[STREAM_ROWS_MAX]; };
// 40 B: the outputs [out_first, out_first + out_count) of the stream go to out[0 .. out_count); frames at or behind T_b
// do not exist (T(total) of a stream whose end is known, else no bound)
struct DenoiseOlaRow { float* out; long out_first, T_b; int out_count, w0, Tw, pad; };
struct DenoiseOlaRows { DenoiseOlaRow r[STREAM_ROWS_MAX]; };
// launch_denoise_subtract with the row's live columns, strength and bias in its descriptor: columns at or behind Tw_b stay 0
hipError_t launch_denoise_subtract_rows(float* ri, long r_bs, long r_cs, const DenoiseSubRows& rows, int B, int spec_ch,
                                        int T_max, hipStream_t s);
// launch_istft_ola over windows: sample j of the stream sits at padded position p = j + pad and sums the frames
// floor(p / hop) - (R - 1) .. floor(p / hop) that lie in [0, T_b), from 0 in ascending t -- the chain of launch_istft_ola
// whatever w0 --, and W likewise.  The caller's windows hold every such frame of every requested output.  Writes
// out_b[0 .. out_count_b) and nothing else.
hipError_t launch_istft_ola_rows(const float* v, long v_bs, long v_cs, const DenoiseOlaRows& rows, const float* w2, int B,
                                 int n_fft, int hop, int T_max, hipStream_t s);

// The STFT of the denoiser as an in-LDS real FFT (fft.hip, fft_plan.h) on the operands above:
// f [B][n_fft][T_max] frames, ri [B][2 spec][T_max], v [B][n_fft][T_max] windowed synthesis frames; tab = the arena's FFT
// tables (Model::fft_tab).  Columns at or behind a row's live count -- T(n_b), or Tw_b of a rows descriptor -- are neither
// read nor written.  hipErrorInvalidValue for any n_fft but FFT_N.
// f -> v with the subtraction of launch_denoise_subtract between the transforms; f == v is allowed
hipError_t launch_fft_denoise(const float* f, long f_bs, long f_cs, float* v, long v_bs, long v_cs, const float* tab,
                              const int64_t* n_samples, const float* bias, const float* strength, int B, int L_max, int n_fft,
                              int hop, int spec_ch, int T_max, hipStream_t s);
hipError_t launch_fft_denoise_rows(const float* f, long f_bs, long f_cs, float* v, long v_bs, long v_cs, const float* tab,
                                   const DenoiseSubRows& rows, int B, int n_fft, int spec_ch, int T_max, hipStream_t s);
// f -> ri and ri -> v; n_samples NULL: every row has T_max live columns
hipError_t launch_fft_forward(const float* f, long f_bs, long f_cs, float* ri, long r_bs, long r_cs, const float* tab,
                              const int64_t* n_samples, int B, int L_max, int n_fft, int hop, int T_max, hipStream_t s);
hipError_t launch_fft_inverse(const float* ri, long r_bs, long r_cs, float* v, long v_bs, long v_cs, const float* tab,
                              const int64_t* n_samples, int B, int L_max, int n_fft, int hop, int T_max, hipStream_t s);

}  // namespace vsp

#include "cl_args.h"   // (builders of the Cl*Args above)
