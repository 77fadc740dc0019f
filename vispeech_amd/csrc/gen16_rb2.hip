// g16_rb2: the whole ResBlock2 of the 32- and 64-channel stages (reference modules.py:232-249) in ONE launch (round 7):
//     y   = x + conv_a(lrelu(x), dilation d_a) + b_a
//     out = y + conv_b(lrelu(y), dilation d_b) + b_b   [+ previous resblock sum] [/ div]        (x != out)
// The machinery is g16_chain's (gen16.hip) with one convolution per step of the block instead of a pair:
//   * both convolutions run on the block's full BT columns with a FIXED column <-> time mapping (column c = time tb + c):
//     the input image sits in LDS with GRD guard rows on either side, a tap reads row c + tap * dil - pad.  Columns within
//     the accumulated padding H = (K - 1)(d_a + d_b) / 2 of a tile edge compute garbage that never reaches a stored column
//     (a D column depends on its own B column only); columns [H, BT - H) are exact and are the ones stored;
//   * the running x, then y, lives in registers in D-tile layout (lane = column, four consecutive channels), fp32: the
//     residual of BOTH convolutions is a lane-local add of the exact fp32 values the two-launch path reads back from HBM;
//     y reaches conv_b only as its operand image (leaky-relu, hi / lo split, zero outside the utterance = the reference's
//     zero padding), written from those registers over the dead x image;
//   * weights stream through the 3-slot LDS-DMA ring as one sequence of slices over the two convolutions.
// Per output the arithmetic is that of g16_conv (bias in the accumulator, chunk-major, tap-minor, HH / CROSS / CROSS per
// step, acc * 2^-8 + residual, then the previous sum, then the division): BIT-IDENTICAL to two g16_conv launches with
// in_act + res (vsp_cl_resblock2 mode 0, VSP_RB2_FUSE=0).
#include "g16_common.h"

#include <cstdlib>
#include <cstring>

namespace vsp {

template <int NCH, int NW, int G, int TERMS, int NWV>
__global__ void __launch_bounds__(64 * NWV, 2) g16_rb2(ClRb2Args a) {
  constexpr int MW = 2 * NCH, C = 32 * NCH, CW = 16 * NW;   // CW = columns per wave
  constexpr int BT = CW * NWV, GRD = G16_HALO / 2, WR = BT + G16_HALO, PL = WR * 16, XIMG = 4 * PL, XBUF = 2 * XIMG;
  constexpr int TAPB = MW * 2048;               // bytes of one tap in a ring slot
  constexpr int SLOT = G * TAPB;
  constexpr int NS = 3;
  constexpr int NPT = 2 * MW;                   // 1 KiB pieces per tap
  constexpr int NBWMAX = (G * NPT + NWV - 1) / NWV;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  char* const Xw = lds;                         // NCH chunk images of the current convolution's input
  char* const Rg = lds + NCH * XBUF;

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, q4 = lane >> 4, l15 = lane & 15;

  // XCD-aware tile numbering: XCD k gets the k-th contiguous eighth of the (utterance, tile) sequence
  const int nwg = gridDim.x, orig = blockIdx.x;
  const int xcd = orig & 7, qd = nwg >> 3, rem = nwg & 7;
  const int id = (xcd < rem ? xcd * (qd + 1) : rem * (qd + 1) + (xcd - rem) * qd) + (orig >> 3);
  const int b = id / a.tiles, tile = id - b * a.tiles;

  const int K = a.K, p2 = (K - 1) >> 1, H = a.halo;
  const int R = BT - 2 * H;                     // columns stored per block
  const int tb = tile * R - H;                  // time of column 0
  const int T = g16_len(a.glen, b, a.grate, a.T);   // (ragged batch: this utterance's own extent)
  if (tile * R >= T) return;
  const int ns = (K + G - 1) / G;               // slices per chunk
  const int S = 2 * NCH * ns;

  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(a.x) + (size_t)b * a.x_bs, 0, T * C * 4, 0x00020000);
  const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(a.out + (size_t)b * a.o_bs, 0, T * C * 4,
                                                                      0x00020000);
  const float slope = a.slope;

  // ---- x in D-tile layout; zero outside the utterance
  bool tval[NW];
  f32x4 xr[MW][NW];
#pragma unroll
  for (int j = 0; j < NW; ++j) {
    const int t = tb + wave * CW + 16 * j + l15;
    tval[j] = t >= 0 && t < T;
#pragma unroll
    for (int i = 0; i < MW; ++i)
      xr[i][j] = g16_as_f32x4(__builtin_amdgcn_raw_buffer_load_b128(rx, tval[j] ? (t * C + 16 * i + 4 * q4) * 4 : G16_OOR, 0, 0));
  }

  // ---- weight slices: one sequence over the two convolutions, chunk-major, G taps per slice
  int dv = 0, dc = 0, dsl = 0;
  auto dma_next = [&](int slot) -> int {
    const uint4* Wg = reinterpret_cast<const uint4*>(a.w[dv]);
    const int tap0 = dsl * G;
    const int pieces = ((K - tap0) < G ? (K - tap0) : G) * NPT;
    const size_t src = ((size_t)dc * K + tap0) * MW * 128;        // uint4 units
    int mine = 0;
#pragma unroll
    for (int u = 0; u < NBWMAX; ++u) {
      const int p = u * NWV + wave;
      if (p < pieces) {
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(Wg + src + (size_t)p * 64 + lane),
                                         (__attribute__((address_space(3))) void*)(Rg + slot * SLOT + p * 1024), 16, 0, 0);
        ++mine;
      }
    }
    if (++dsl == ns) { dsl = 0; if (++dc == NCH) { dc = 0; ++dv; } }
    return mine;
  };

  // ---- image of a D-layout tile set: leaky-relu, split, zero outside the utterance.  A lane's four channels
  //      16 i + 4 q4 .. + 3 sit in chunk i / 2, plane 2 (i & 1) + (q4 >> 1), at byte 8 (q4 & 1) of the row's 16.
  auto write_image = [&](const f32x4 (&v)[MW][NW]) {
#pragma unroll
    for (int i = 0; i < MW; ++i)
#pragma unroll
      for (int j = 0; j < NW; ++j) {
        f16x4 eh, el;
        g16_split4(tval[j] ? v[i][j] : f32x4{0.f, 0.f, 0.f, 0.f}, slope, true, eh, el);
        char* dst = Xw + (i >> 1) * XBUF + (2 * (i & 1) + (q4 >> 1)) * PL + (GRD + wave * CW + 16 * j + l15) * 16 + 8 * (q4 & 1);
        *reinterpret_cast<f16x4*>(dst) = eh;
        if constexpr (TERMS == 3) *reinterpret_cast<f16x4*>(dst + XIMG) = el;
      }
  };

  // ---- convolution main loop (g16_chain's): one STEP = one (chunk, tap), A fragments double-buffered in registers,
  //      B fragments re-requested in place after their last MFMA of the step, counted LDS waits.  Ring: slices n, n + 1,
  //      n + 2 resident or in flight; retire() waits for slice n + 1, barriers and requests slice n + 3 into the freed slot.
  constexpr int RA = MW * (TERMS == 3 ? 2 : 1), RB = TERMS == 3 ? 2 : 1;   // LDS reads per A set / per n-tile
  const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)lds;
  const unsigned wa_lane = lds0 + NCH * XBUF + lane * 16;
  constexpr int gs = G;                         // taps per slice (the last one of a chunk may be shorter)
  f16x8 Ah[2][MW], Al[2][MW], Bh[NW], Bl[NW];
  f32x4 hh[MW][NW];

  int n_cur = 0, n_issued = 0, pc_last = 0;     // slice being read; slices requested; my pieces of the youngest one
  auto issue_slice = [&]() {
    if (n_issued < S) { pc_last = dma_next(n_issued % NS); ++n_issued; }
  };
  auto wait_landed = [&](int n) {               // slice n (< n_issued) has landed: younger are n + 1 .. n_issued - 1
    const int younger = n_issued - 1 - n;
    if (younger <= 0) g16_vmcnt<0>();
    else if (younger == 1) { if (pc_last == 0) g16_vmcnt<0>(); else if (pc_last == 1) g16_vmcnt<1>(); else g16_vmcnt<2>(); }
    else { if (pc_last == 0) g16_vmcnt<0>(); else g16_vmcnt<1>(); }   // (stricter than needed: the older one's count is not kept)
  };
  auto retire = [&]() {
    if (n_cur + 1 < S) {
      wait_landed(n_cur + 1);
      G16_BARRIER();
      issue_slice();
    }
    ++n_cur;
  };
  auto read_a = [&](auto P, unsigned a_addr) {
    constexpr int pp = decltype(P)::value;
    g16_for<MW>([&](auto I) {
      constexpr int i = decltype(I)::value;
      Ah[pp][i] = g16_lds_read<i * 2048>(a_addr);
      if constexpr (TERMS == 3) Al[pp][i] = g16_lds_read<i * 2048 + 1024>(a_addr);
    });
  };
  auto read_b = [&](auto J, unsigned b_addr) {
    constexpr int j = decltype(J)::value;
    Bh[j] = g16_lds_read<j * 256>(b_addr);
    if constexpr (TERMS == 3) Bl[j] = g16_lds_read<j * 256 + XIMG>(b_addr);
  };
  auto mfma_col = [&](auto P, auto J) {
    constexpr int pp = decltype(P)::value, j = decltype(J)::value;
    __builtin_amdgcn_sched_barrier(0);
    g16_for<MW>([&](auto I) {
      constexpr int i = decltype(I)::value;
      hh[i][j] = G16_MFMA(Ah[pp][i], Bh[j], hh[i][j]);
      if constexpr (TERMS == 3) {
        hh[i][j] = G16_MFMA(Al[pp][i], Bh[j], hh[i][j]);
        hh[i][j] = G16_MFMA(Ah[pp][i], Bl[j], hh[i][j]);
      }
    });
    __builtin_amdgcn_sched_barrier(0);
  };

  // one convolution over the image in Xw: dilation `rowstep`, bias b; result in hh.  On entry the image and
  // slice n_cur (the convolution's first) are visible to every wave.
  auto conv = [&](const float* bias, int rowstep) {
#pragma unroll
    for (int i = 0; i < MW; ++i) {
      const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + 16 * i + 4 * q4);
#pragma unroll
      for (int j = 0; j < NW; ++j) hh[i][j] = bv;
    }
    const unsigned xb0 = lds0 + q4 * PL + (GRD + wave * CW + l15 - rowstep * p2) * 16;
    const int steps = NCH * K;
    int chunk = 0, tap = 0, gtap = 0;             // of the step being multiplied; gtap = tap within its slice
    unsigned a_addr = wa_lane + (n_cur % NS) * SLOT, b_addr = xb0;
    read_a(std::integral_constant<int, 0>{}, a_addr);
    g16_for<NW>([&](auto J) { read_b(J, b_addr); });
    auto step = [&](auto P, int st) {
      constexpr int pp = decltype(P)::value;
      if (st + 1 < steps) {
        const bool slice_end = gtap == gs - 1 || tap == K - 1;
        if (slice_end) retire();                        // (the barrier drains this wave's reads: the counted waits below still hold)
        const bool chunk_end = tap == K - 1;
        chunk = chunk_end ? chunk + 1 : chunk;
        tap = chunk_end ? 0 : tap + 1;
        gtap = slice_end ? 0 : gtap + 1;
        a_addr = wa_lane + (n_cur % NS) * SLOT + gtap * TAPB;
        b_addr = xb0 + chunk * XBUF + tap * rowstep * 16;
      }
      // (the last step of a convolution re-requests its own fragments: one code path, uniform counted waits)
      read_a(std::integral_constant<int, 1 - pp>{}, a_addr);
      g16_for<NW>([&](auto J) {
        g16_lgkmcnt<(RA + (NW - 1) * RB < 15 ? RA + (NW - 1) * RB : 15)>();   // (a 4-bit counter)
        mfma_col(P, J);
        read_b(J, b_addr);
      });
    };
    for (int st = 0; st < steps; st += 2) {
      step(std::integral_constant<int, 0>{}, st);
      if (st + 1 < steps) step(std::integral_constant<int, 1>{}, st + 1);
    }
    // nothing may still be writing the fragment registers when the compiler reuses them
    g16_lgkmcnt<0>();
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < MW; ++i) asm volatile("" ::"v"(Ah[0][i]), "v"(Ah[1][i]), "v"(Al[0][i]), "v"(Al[1][i]));
#pragma unroll
    for (int j = 0; j < NW; ++j) asm volatile("" ::"v"(Bh[j]), "v"(Bl[j]));
  };

  issue_slice(); issue_slice(); issue_slice();
  write_image(xr);
  wait_landed(0);
  G16_BARRIER();
  // ---- conv_a; y = x + conv_a (the fp32 value the two-launch path stores) replaces x in the registers
  conv(a.b[0], a.dil[0]);
#pragma unroll
  for (int i = 0; i < MW; ++i)
#pragma unroll
    for (int j = 0; j < NW; ++j) xr[i][j] = hh[i][j] * G16_UNSCALE + xr[i][j];
  retire();                                            // also: nobody still reads the x image
  write_image(xr);
  G16_BARRIER();
  // ---- conv_b
  conv(a.b[1], a.dil[1]);

  // ---- epilogue: out = conv_b + y (+ previous resblock sum) (/ div) on the exact columns
#pragma unroll
  for (int i = 0; i < MW; ++i)
#pragma unroll
    for (int j = 0; j < NW; ++j) {
      const int col = wave * CW + 16 * j + l15;
      const int t = tb + col;
      const int off = (col >= H && col < H + R && t < T) ? (t * C + 16 * i + 4 * q4) * 4 : G16_OOR;
      f32x4 v = hh[i][j] * G16_UNSCALE + xr[i][j];
      if (a.acc_prev) v += g16_as_f32x4(__builtin_amdgcn_raw_buffer_load_b128(ro, off, 0, 0));
      g16_div(v, a.div);
      __builtin_amdgcn_raw_buffer_store_b128(g16_as_u32x4(v), ro, off, 0, 0);
    }
}

template <int NCH, int NW, int G, int TERMS, int NWV>
static hipError_t launch_g16_rb2_tile(ClRb2Args a, int B, hipStream_t s, int R) {
  constexpr int BT = 16 * NW * NWV;
  constexpr size_t lds = (size_t)NCH * 2 * 4 * (BT + G16_HALO) * 16 + (size_t)3 * G * 2 * NCH * 2048;
  static_assert(lds <= 160 * 1024, "LDS budget");
  static std::atomic<uint64_t> attr_done{0};
  auto kern = g16_rb2<NCH, NW, G, TERMS, NWV>;
  if (hipError_t e = set_max_dynamic_lds(reinterpret_cast<const void*>(kern), (int)lds, attr_done); e != hipSuccess) return e;
  if (R != BT - 2 * a.halo || R < 32) return hipErrorInvalidValue;   // (the route's tile_cols: what the kernel stores per tile)
  a.tiles = (a.T + R - 1) / R;
  const long n = (long)a.tiles * B;
  if (n <= 0 || n > 0x7fffffffL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kern, dim3((unsigned)n), dim3(64 * NWV), lds, s, a);
  return hipGetLastError();
}

static int g16_rb2_halo(int K, const int* dil) { return (dil[0] + dil[1]) * ((K - 1) / 2); }

bool g16_rb2_supported(int C, int K, const int* dil) {
  if (!(C == 32 || C == 64) || K < 1 || !(K & 1)) return false;
  // a tap reads at most GRD = G16_HALO / 2 rows beyond the block's columns on either side
  for (int c = 0; c < 2; ++c)
    if (dil[c] < 1 || dil[c] * ((K - 1) / 2) > G16_HALO / 2) return false;
  return 256 - 2 * g16_rb2_halo(K, dil) >= 32;
}

ClRoute g16_rb2_route(const ClRb2Args& a) {
  const int halo = g16_rb2_halo(a.K, a.dil);
  // g16_chain's shapes: 64 channels, 8 waves x 32 columns; 32 channels, two 4-wave blocks of 256 columns per CU, or one
  // 8-wave block of 512 columns when the halo would eat more than a quarter of a 256-column tile
  const bool wide = a.C == 32 && 2 * halo > 64;
  return ClRoute{VSP_CL_KERNEL_RB2, (wide ? 512 : 256) - 2 * halo, 0, wide ? 1 : 0};
}

hipError_t launch_g16_rb2(const ClRb2Args& a0, int B, hipStream_t s) {
  ClRb2Args a = a0;
  if (!g16_rb2_supported(a.C, a.K, a.dil) || a.T <= 0 || B <= 0 || (a.terms != 1 && a.terms != 3) || (a.x_bs & 3) ||
      (a.o_bs & 3) || (reinterpret_cast<uintptr_t>(a.x) & 15) || (reinterpret_cast<uintptr_t>(a.out) & 15) || a.x == a.out ||
      !a.w[0] || !a.w[1] || !a.b[0] || !a.b[1])
    return hipErrorInvalidValue;
  // an utterance is addressed with 32-bit byte offsets (buffer descriptors: num_records, t * C * 4)
  if ((size_t)a.T * a.C * 4 >= (size_t)1 << 31) return hipErrorInvalidValue;
  a.halo = g16_rb2_halo(a.K, a.dil);
  const ClRoute r = g16_rb2_route(a);
  const bool wide = r.variant == 1;
  // <NCH, NW, G, TERMS, NWV>
  if (a.terms == 1) {
    if (a.C == 64) return launch_g16_rb2_tile<2, 2, 2, 1, 8>(a, B, s, r.tile_cols);
    return wide ? launch_g16_rb2_tile<1, 4, 4, 1, 8>(a, B, s, r.tile_cols) : launch_g16_rb2_tile<1, 4, 2, 1, 4>(a, B, s, r.tile_cols);
  }
  if (a.C == 64) return launch_g16_rb2_tile<2, 2, 2, 3, 8>(a, B, s, r.tile_cols);
  return wide ? launch_g16_rb2_tile<1, 4, 4, 3, 8>(a, B, s, r.tile_cols) : launch_g16_rb2_tile<1, 4, 2, 3, 4>(a, B, s, r.tile_cols);
}

}  // namespace vsp
