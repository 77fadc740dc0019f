// g16_c16: the 16-channel last stage of a five-stage generator (upsample_initial_channel 512: 256, 128, 64, 32, 16
// channels).  ONE kernel family runs a sequence of 1 .. 6 convolutions 16 -> 16 of a channels-last tensor in one launch
// (kernels.h, ClC16Args): a whole ResBlock1 ([conv(d_p), conv(1) + residual] per pair), a whole ResBlock2
// ([conv(d) + residual] x 2), or a single convolution -- the general fallback and the bit-identity reference.
// The stage is 4 % of the generator's arithmetic but runs at the full sample rate: what it costs is traffic, a row of
// 16 fp32 channels being 64 B.  Fused, a ResBlock reads its input and writes its output once.
// The scheme is g16_rb2 / g16_chain's, re-cut for one 16-row M tile:
//   * a block owns BT = 512 columns with a FIXED column <-> time mapping (column c = time tb + c); the step's input
//     image sits in LDS with GRD guard rows on either side, a tap reads row c + tap * dil - pad.  Columns within the
//     accumulated padding H = sum_i (K - 1) dil_i / 2 of a block edge compute garbage that never reaches a stored column
//     (a D column depends on its own B column only); columns [H, BT - H) are exact and are the ones stored;
//   * the running tensor lives in registers in D-tile layout (lane = column, four consecutive channels), fp32: residual
//     adds are lane-local;
//   * a step's input reaches LDS only as its leaky-relu'd hi / lo image, zero outside the utterance (the reference's
//     zero padding): two planes (channels 0 .. 7, 8 .. 15) of [row][8 halfs] per image, so a lane's B fragment is one
//     ds_read_b128;
//   * K-step = 32 = TWO TAPS x 16 channels (pack_g16c16_weights): lane group q4 multiplies tap 2 s + (q4 >> 1), channels
//     8 (q4 & 1) .. + 7.  An odd K's last step has a zero second tap, whose B fragment is read from a row of zeros (the
//     image may hold inf, and 0 * inf would poison the column).  6 steps for K = 11, 4 for K = 7, 2 for K = 3;
//   * a convolution's weights (2 KiB per step) are copied to LDS by LDS-DMA, the next convolution's while this one
//     multiplies (two buffers).
// Per output the arithmetic is g16_conv's: bias in the accumulator, steps ascending, HH / CROSS / CROSS per step (one
// product for terms == 1), acc * 2^-8 + residual, then the previous sum, then the division -- and every form is this one
// kernel, so the fused forms are BIT-IDENTICAL to one launch per convolution.
#include "g16_common.h"

#include <cstring>

namespace vsp {

namespace {
constexpr int C16_NW = 4, C16_NWV = 8, C16_CW = 16 * C16_NW, C16_BT = C16_CW * C16_NWV;
constexpr int C16_GRD = G16_HALO / 2, C16_WR = C16_BT + 2 * C16_GRD, C16_ZROW = C16_WR;
constexpr int C16_PL = (C16_WR + 1) * 16, C16_XIMG = 2 * C16_PL;
constexpr int C16_WOFF = (2 * C16_XIMG + 1023) / 1024 * 1024;     // the weight buffers start on a 1 KiB boundary
static_assert(C16_BT == G16_C16_BT, "kernels.h states the block's columns");
}  // namespace

size_t packed_g16c16_halfs(int K) { return (size_t)((K + 1) / 2) * 1024; }

void pack_g16c16_weights(uint16_t* dst, int K, const float* dense) {
  const int S = (K + 1) / 2;
  for (int s = 0; s < S; ++s)
    for (int lane = 0; lane < 64; ++lane) {
      const int co = lane & 15, q4 = lane >> 4, tap = 2 * s + (q4 >> 1), ci0 = 8 * (q4 & 1);
      for (int j = 0; j < 8; ++j) {
        const float w = tap < K ? dense[((size_t)co * 16 + ci0 + j) * K + tap] * G16_WSCALE : 0.f;
        const _Float16 h = (_Float16)w;
        const _Float16 l = (_Float16)(w - (float)h);
        std::memcpy(dst + ((size_t)(2 * s) * 64 + lane) * 8 + j, &h, 2);
        std::memcpy(dst + ((size_t)(2 * s + 1) * 64 + lane) * 8 + j, &l, 2);
      }
    }
}

template <int TERMS>
__global__ void __launch_bounds__(64 * C16_NWV) g16_c16(ClC16Args a) {
  constexpr int NW = C16_NW, NWV = C16_NWV, CW = C16_CW, BT = C16_BT, GRD = C16_GRD, PL = C16_PL, XIMG = C16_XIMG;
  extern __shared__ __attribute__((aligned(16))) char lds[];

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, q4 = lane >> 4, l15 = lane & 15;
  const int b = blockIdx.x / a.tiles, tile = blockIdx.x - b * a.tiles;

  const int K = a.K, p2 = (K - 1) >> 1, S = (K + 1) >> 1, H = a.halo;
  const int R = BT - 2 * H;                     // columns stored per block
  const int tb = tile * R - H;                  // time of column 0
  const int T = g16_len(a.glen, b, a.grate, a.T);   // (ragged batch: this utterance's own extent)
  if (tile * R >= T) return;
  const int wbytes = S * 2048;

  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(a.x) + (size_t)b * a.x_bs, 0, T * 64, 0x00020000);
  const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(a.res ? a.res + (size_t)b * a.r_bs : a.x + (size_t)b * a.x_bs), 0, T * 64, 0x00020000);
  const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(a.out + (size_t)b * a.o_bs, 0, T * 64, 0x00020000);
  const float slope = a.slope;

  // ---- a convolution's weights -> LDS buffer `buf`: 2 S pieces of 1 KiB, one per wave instruction
  auto dma = [&](const uint16_t* w, int buf) {
    const uint4* Wg = reinterpret_cast<const uint4*>(w);
    char* const dst = lds + C16_WOFF + buf * wbytes;
    for (int p = wave; p < 2 * S; p += NWV)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(Wg + (size_t)p * 64 + lane),
                                       (__attribute__((address_space(3))) void*)(dst + p * 1024), 16, 0, 0);
  };

  // ---- the input and the running tensor in D-tile layout; zero outside the utterance
  bool tval[NW];
  f32x4 in[NW], xr[NW];
#pragma unroll
  for (int j = 0; j < NW; ++j) {
    const int t = tb + wave * CW + 16 * j + l15;
    tval[j] = t >= 0 && t < T;
    const int off = tval[j] ? (t * 16 + 4 * q4) * 4 : G16_OOR;
    in[j] = g16_as_f32x4(__builtin_amdgcn_raw_buffer_load_b128(rx, off, 0, 0));
    xr[j] = a.res ? g16_as_f32x4(__builtin_amdgcn_raw_buffer_load_b128(rr, off, 0, 0)) : in[j];
  }
  // the row of zeros an odd K's absent second tap reads (hi and lo image, both planes)
  if (tid < 4) *reinterpret_cast<uint4*>(lds + tid * PL + C16_ZROW * 16) = uint4{0u, 0u, 0u, 0u};
  dma(a.w[0], 0);

  // ---- image of a D-layout tile: leaky-relu, split, zero outside the utterance.  A lane's four channels 4 q4 .. + 3
  //      sit in plane q4 >> 1 at byte 8 (q4 & 1) of the row's 16.
  auto write_image = [&](const f32x4 (&v)[NW]) {
#pragma unroll
    for (int j = 0; j < NW; ++j) {
      f16x4 eh, el;
      g16_split4(tval[j] ? v[j] : f32x4{0.f, 0.f, 0.f, 0.f}, slope, true, eh, el);
      char* dst = lds + (q4 >> 1) * PL + (GRD + wave * CW + 16 * j + l15) * 16 + 8 * (q4 & 1);
      *reinterpret_cast<f16x4*>(dst) = eh;
      if constexpr (TERMS == 3) *reinterpret_cast<f16x4*>(dst + XIMG) = el;
    }
  };

  // ---- one convolution over the image: dilation d, weights in buffer `buf`; result (* G16_WSCALE) in hh
  f32x4 hh[NW];
  auto conv = [&](const float* bias, int d, int buf) {
    const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + 4 * q4);
#pragma unroll
    for (int j = 0; j < NW; ++j) hh[j] = bv;
    const char* const Wb = lds + C16_WOFF + buf * wbytes + lane * 16;
    const char* const Xp = lds + (q4 & 1) * PL;
    const int row0 = GRD + wave * CW + l15 - d * p2;
    for (int s = 0; s < S; ++s) {
      const int tap = 2 * s + (q4 >> 1);
      const bool absent = tap >= K;
      const f16x8 Ah = *reinterpret_cast<const f16x8*>(Wb + s * 2048);
      f16x8 Al;
      if constexpr (TERMS == 3) Al = *reinterpret_cast<const f16x8*>(Wb + s * 2048 + 1024);
#pragma unroll
      for (int j = 0; j < NW; ++j) {
        const char* const p = Xp + (absent ? C16_ZROW : row0 + tap * d + 16 * j) * 16;
        const f16x8 Bh = *reinterpret_cast<const f16x8*>(p);
        hh[j] = G16_MFMA(Ah, Bh, hh[j]);
        if constexpr (TERMS == 3) {
          const f16x8 Bl = *reinterpret_cast<const f16x8*>(p + XIMG);
          hh[j] = G16_MFMA(Al, Bh, hh[j]);
          hh[j] = G16_MFMA(Ah, Bl, hh[j]);
        }
      }
    }
  };

  g16_for<6>([&](auto I) {
    constexpr int i = decltype(I)::value;
    if (i < a.nsteps) {
      write_image(in);
      g16_vmcnt<0>();                           // my pieces of this convolution's weights have landed
      G16_BARRIER();                            // image and weights visible; nobody still reads the other weight buffer
      if constexpr (i + 1 < 6)
        if (i + 1 < a.nsteps) dma(a.w[i + 1], (i + 1) & 1);
      conv(a.b[i], a.dil[i], i & 1);
      if (i + 1 < a.nsteps) {
        // the next step's input; with `add` it is also the new running tensor (the fp32 value a launch per
        // convolution would store and read back)
#pragma unroll
        for (int j = 0; j < NW; ++j) {
          if (a.add[i]) { xr[j] = hh[j] * G16_UNSCALE + xr[j]; in[j] = xr[j]; }
          else in[j] = hh[j] * G16_UNSCALE;
        }
        G16_BARRIER();                          // nobody still reads the image
      } else {
        // ---- epilogue: out = conv (+ running tensor) (+ previous resblock sum) (/ div) on the exact columns
#pragma unroll
        for (int j = 0; j < NW; ++j) {
          const int col = wave * CW + 16 * j + l15;
          const int t = tb + col;
          const int off = (col >= H && col < H + R && t < T) ? (t * 16 + 4 * q4) * 4 : G16_OOR;
          f32x4 v = a.add[i] ? hh[j] * G16_UNSCALE + xr[j] : hh[j] * G16_UNSCALE;
          if (a.acc_prev) v += g16_as_f32x4(__builtin_amdgcn_raw_buffer_load_b128(ro, off, 0, 0));
          g16_div(v, a.div);
          __builtin_amdgcn_raw_buffer_store_b128(g16_as_u32x4(v), ro, off, 0, 0);
        }
      }
    }
  });
}

static int g16_c16_halo(int K, const int* dil, int nsteps) {
  int h = 0;
  for (int i = 0; i < nsteps; ++i) h += dil[i] * ((K - 1) / 2);
  return h;
}
static size_t g16_c16_lds(int K, int nsteps) { return (size_t)C16_WOFF + (size_t)(nsteps > 1 ? 2 : 1) * ((K + 1) / 2) * 2048; }

bool g16_c16_supported(int K, const int* dil, int nsteps) {
  if (K < 1 || !(K & 1) || nsteps < 1 || nsteps > 6) return false;
  // a tap reads at most GRD = G16_HALO / 2 rows beyond the block's columns on either side
  for (int i = 0; i < nsteps; ++i)
    if (dil[i] < 1 || (K - 1) * dil[i] > G16_HALO) return false;
  // at least an eighth of the block's columns is stored; both weight buffers fit beside the image
  return C16_BT - 2 * g16_c16_halo(K, dil, nsteps) >= C16_BT / 8 && g16_c16_lds(K, nsteps) <= 160 * 1024;
}
bool g16_c16_rb1_supported(int K, const int* dil, int np) {
  int d[6], add[6];
  return np >= 1 && np <= 3 && g16_c16_supported(K, d, cl_c16_steps(1, dil, np, d, add));
}
bool g16_c16_rb2_supported(int K, const int* dil) {
  int d[6], add[6];
  return g16_c16_supported(K, d, cl_c16_steps(2, dil, 2, d, add));
}

ClRoute g16_c16_route(const ClC16Args& a) {
  return ClRoute{VSP_CL_KERNEL_C16, C16_BT - 2 * g16_c16_halo(a.K, a.dil, a.nsteps), 0, 0};
}

template <int TERMS>
static hipError_t launch_g16_c16_terms(const ClC16Args& a, int B, hipStream_t s) {
  static std::atomic<uint64_t> attr_done{0};
  auto kern = g16_c16<TERMS>;
  // (the attribute is the largest request the kernel can get: one value per process keeps the cached bit valid)
  if (hipError_t e = set_max_dynamic_lds(reinterpret_cast<const void*>(kern), 160 * 1024, attr_done); e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3((unsigned)((long)a.tiles * B)), dim3(64 * C16_NWV), g16_c16_lds(a.K, a.nsteps), s, a);
  return hipGetLastError();
}

hipError_t launch_g16_c16(const ClC16Args& a0, int B, hipStream_t s) {
  ClC16Args a = a0;
  if (!g16_c16_supported(a.K, a.dil, a.nsteps) || a.T <= 0 || B <= 0 || (a.terms != 1 && a.terms != 3) || (a.x_bs & 3) ||
      (a.o_bs & 3) || (a.r_bs & 3) || !a.x || !a.out || a.x == a.out || (reinterpret_cast<uintptr_t>(a.x) & 15) ||
      (reinterpret_cast<uintptr_t>(a.out) & 15) || (reinterpret_cast<uintptr_t>(a.res) & 15))
    return hipErrorInvalidValue;
  for (int i = 0; i < a.nsteps; ++i)
    if (!a.w[i] || !a.b[i] || (reinterpret_cast<uintptr_t>(a.w[i]) & 15) || (reinterpret_cast<uintptr_t>(a.b[i]) & 15))
      return hipErrorInvalidValue;
  // an utterance is addressed with 32-bit byte offsets (buffer descriptors: num_records, t * 64)
  if ((size_t)a.T * 64 >= (size_t)1 << 31) return hipErrorInvalidValue;
  a.halo = g16_c16_halo(a.K, a.dil, a.nsteps);
  const int R = g16_c16_route(a).tile_cols;
  a.tiles = (a.T + R - 1) / R;
  if ((long)a.tiles * B > 0x7fffffffL) return hipErrorInvalidValue;
  return a.terms == 1 ? launch_g16_c16_terms<1>(a, B, s) : launch_g16_c16_terms<3>(a, B, s);
}

}  // namespace vsp
