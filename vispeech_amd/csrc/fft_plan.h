// What the host and the device share of the in-LDS real FFT (fft.hip): the layout of the tables in
// the arena, the index math -- slot skew, digit reversal, twiddle index, split-step pairing -- and the arithmetic of one
// butterfly and of one split step, as functions of a work item's number.  The kernels call them with item = thread (+ a
// multiple of the block); tools/micro/fft_plan_main.cpp calls the same functions item after item on the CPU, so an index
// that leaves the frame's image is found there, under a sanitizer, before a GPU sees it.
//
// A real transform of N = 2048 points is the complex transform of M = N / 2 = 1024 points z[m] = x[2m] + i x[2m+1],
// followed by a split step (forward) or preceded by one (inverse).  M = 4^5: five radix-4 passes, M / 4 = 256 butterflies
// a pass.  Forward passes are decimation in frequency, natural order in and digit-reversed out; inverse passes are their
// mirror, digit-reversed in and natural out: no pass reorders anything, and the spectrum lives at digit-reversed positions.
// No product is contracted with a sum (fp contract off): a frame's bits are the same in every kernel that includes this
// file and in the host program.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define VSP_HD __host__ __device__
#else
#define VSP_HD
#endif

namespace vsp {

struct alignas(8) cf { float x, y; };

constexpr int FFT_N = 2048;
constexpr int FFT_M = FFT_N / 2;
constexpr int FFT_PASSES = 5;               // 4^5 = FFT_M
constexpr int FFT_THREADS = FFT_M / 4;      // one butterfly per thread, pass and frame
constexpr int FFT_SPLIT_ITEMS = FFT_M / 2 + 1;   // the pairs (k, M - k), k = 0 .. M / 2
constexpr int FFT_MAX_TILE = 16;

// The tables (floats from the table's start; weights.cpp builds them in fp64 and rounds once):
//   tw     [M]          (cos, sin)(2 pi j / M)
//   split  [M / 2 + 1]  (cos, sin)(2 pi k / N)
//   wa     [N]          hann[n]            the analysis window
//   ws     [N]          hann[n] / N        the synthesis window (the inverse passes are not normalised)
constexpr int FFT_TAB_TW = 0;
constexpr int FFT_TAB_SPLIT = FFT_TAB_TW + 2 * FFT_M;
constexpr int FFT_TAB_WA = FFT_TAB_SPLIT + 2 * FFT_SPLIT_ITEMS;
constexpr int FFT_TAB_WS = FFT_TAB_WA + FFT_N;
constexpr int FFT_TAB_FLOATS = FFT_TAB_WS + FFT_N;

// (cos, sin)(2 pi j / n) in double, n a multiple of 4, 0 <= j < n: the angle is reduced to its quadrant first, so the
// multiples of a quarter turn are exact.
inline void fft_unit(int j, int n, double* c, double* s) {
  const int quad = j / (n / 4), r = j % (n / 4);
  const double a = 2.0 * 3.14159265358979323846 * r / n, cr = std::cos(a), sr = std::sin(a);
  *c = quad == 0 ? cr : quad == 1 ? -sr : quad == 2 ? -cr : sr;
  *s = quad == 0 ? sr : quad == 1 ? cr : quad == 2 ? -sr : -cr;
}

// The FFT_TAB_FLOATS floats of the tables, each rounded once from double (host only).
inline void fft_fill_tables(float* tab) {
  double c, s;
  for (int j = 0; j < FFT_M; ++j) {
    fft_unit(j, FFT_M, &c, &s);
    tab[FFT_TAB_TW + 2 * j] = (float)c;
    tab[FFT_TAB_TW + 2 * j + 1] = (float)s;
  }
  for (int k = 0; k < FFT_SPLIT_ITEMS; ++k) {
    fft_unit(k, FFT_N, &c, &s);
    tab[FFT_TAB_SPLIT + 2 * k] = (float)c;
    tab[FFT_TAB_SPLIT + 2 * k + 1] = (float)s;
  }
  for (int n = 0; n < FFT_N; ++n) {
    const double hann = 0.5 - 0.5 * std::cos(2.0 * 3.14159265358979323846 * n / FFT_N);      // periodic Hann, as weights.cpp's
    tab[FFT_TAB_WA + n] = (float)hann;
    tab[FFT_TAB_WS + n] = (float)(hann / FFT_N);
  }
}

// Base-4 digit reversal of a position in [0, M).
VSP_HD inline int fft_rev(int k) {
  int r = 0;
  for (int d = 0; d < FFT_PASSES; ++d) { r = (r << 2) | (k & 3); k >>= 2; }
  return r;
}

// Frame tl of a tile: XORed into the low four bits of every slot, so that the `tile` frames of one sample lie in different
// banks when a tile row (tile contiguous floats of global memory) is staged: 32 lanes = tile frames x 32 / tile samples.
VSP_HD inline int fft_frame_skew(int tl, int tile) { return (tl * (FFT_MAX_TILE / tile)) & 15; }

// Slot (in cf units, within the frame's image of M slots) of position pos.  A pass of quarter q reads, per 32 lanes (an
// 8-byte LDS access is served in groups of 32 lanes over 32 bank pairs, MI355X_MICROARCH.md LDS), the positions
//   q >= 32: 32 consecutive ones;  q = 16: 16 + 16, 64 apart;  q = 4: 8 runs of 4, 16 apart;  q = 1: every fourth of 128.
// XORing bits 5 and 6 of the position into bits 0-1, 2-3 and bit 6 into bit 4 makes each of these a permutation of the 32
// bank pairs.  Only the low five bits change: a slot stays inside its aligned run of 32, and the image needs no padding.
VSP_HD inline int fft_slot(int skew, int pos) {
  return pos ^ (((pos >> 5) & 3) * 5) ^ (((pos >> 6) & 1) << 4) ^ skew;
}

// Float index of sample n of a frame (z[m] = x[2m] + i x[2m+1]) within the frame's image.
VSP_HD inline int fft_sample_slot(int skew, int n) { return 2 * fft_slot(skew, n >> 1) + (n & 1); }

// Butterfly j of pass p (p = 0: quarter M / 4, .. p = 4: quarter 1): its four positions are base + i q, and the factor of
// output (forward) or input (inverse) i is tw[i * twi].
struct FftBfly { int base, q, twi; };
VSP_HD inline FftBfly fft_bfly(int p, int j) {
  const int lq = 2 * (FFT_PASSES - 1 - p), q = 1 << lq;
  const int k = j & (q - 1), g = j >> lq;
  return FftBfly{(g << (lq + 2)) + k, q, k << (2 * p)};
}

// Split item j: the bin k <= M / 2 it pairs with M - k.  Items below M / 2 walk the positions whose bit 1 is clear -- those
// of the bins below M / 2 -- in ascending position, so that lanes read neighbouring slots; the last item is k = M / 2.
VSP_HD inline int fft_split_bin(int j) { return j < FFT_M / 2 ? fft_rev(((j >> 1) << 2) | (j & 1)) : FFT_M / 2; }
// ... and the positions of Z[k] and Z[M - k] (k = 0: both 0).
VSP_HD inline int fft_split_pos(int k) { return fft_rev(k); }
VSP_HD inline int fft_split_pair(int k) { return fft_rev((FFT_M - k) & (FFT_M - 1)); }

VSP_HD inline cf cf_add(cf a, cf b) {
#pragma clang fp contract(off)
  return cf{a.x + b.x, a.y + b.y};
}
VSP_HD inline cf cf_sub(cf a, cf b) {
#pragma clang fp contract(off)
  return cf{a.x - b.x, a.y - b.y};
}
// a e^{-i t}, w = (cos t, sin t)
VSP_HD inline cf cf_mul_conj(cf a, cf w) {
#pragma clang fp contract(off)
  const float p0 = a.x * w.x, p1 = a.y * w.y, p2 = a.y * w.x, p3 = a.x * w.y;
  return cf{p0 + p1, p2 - p3};
}
// a e^{+i t}
VSP_HD inline cf cf_mul(cf a, cf w) {
#pragma clang fp contract(off)
  const float p0 = a.x * w.x, p1 = a.y * w.y, p2 = a.y * w.x, p3 = a.x * w.y;
  return cf{p0 - p1, p2 + p3};
}

// One forward butterfly in place on the frame image z (M slots): y_i = (sum_l a_l (-i)^(i l)) e^{-2 pi i (i k) / L}.
VSP_HD inline void fft_fwd_bfly(cf* z, int skew, FftBfly b, cf w1, cf w2, cf w3) {
  const int s0 = fft_slot(skew, b.base), s1 = fft_slot(skew, b.base + b.q), s2 = fft_slot(skew, b.base + 2 * b.q),
            s3 = fft_slot(skew, b.base + 3 * b.q);
  const cf a0 = z[s0], a1 = z[s1], a2 = z[s2], a3 = z[s3];
  const cf t0 = cf_add(a0, a2), t1 = cf_sub(a0, a2), t2 = cf_add(a1, a3), t3 = cf_sub(a1, a3);
  const cf y1 = cf_add(t1, cf{t3.y, -t3.x}), y3 = cf_sub(t1, cf{t3.y, -t3.x});      // t1 -+ i t3
  z[s0] = cf_add(t0, t2);
  z[s1] = cf_mul_conj(y1, w1);
  z[s2] = cf_mul_conj(cf_sub(t0, t2), w2);
  z[s3] = cf_mul_conj(y3, w3);
}

// Its mirror: b_i = a_i e^{+2 pi i (i k) / L}, y_i = sum_l b_l (+i)^(i l).  Not normalised.
VSP_HD inline void fft_inv_bfly(cf* z, int skew, FftBfly b, cf w1, cf w2, cf w3) {
  const int s0 = fft_slot(skew, b.base), s1 = fft_slot(skew, b.base + b.q), s2 = fft_slot(skew, b.base + 2 * b.q),
            s3 = fft_slot(skew, b.base + 3 * b.q);
  const cf a0 = z[s0], a1 = cf_mul(z[s1], w1), a2 = cf_mul(z[s2], w2), a3 = cf_mul(z[s3], w3);
  const cf t0 = cf_add(a0, a2), t1 = cf_sub(a0, a2), t2 = cf_add(a1, a3), t3 = cf_sub(a1, a3);
  z[s0] = cf_add(t0, t2);
  z[s1] = cf_add(t1, cf{-t3.y, t3.x});      // t1 + i t3
  z[s2] = cf_sub(t0, t2);
  z[s3] = cf_sub(t1, cf{-t3.y, t3.x});
}

// Forward split: a = Z[k], b = Z[M - k], w = split[k] -> X[k] and X[M - k] of the real transform,
//   X[k] = E + e^{-2 pi i k / N} O, X[M - k] = conj(E - e^{-2 pi i k / N} O), E = (a + conj b) / 2, O = -i (a - conj b) / 2.
// k = 0 (a = b = Z[0]) gives X[0] and X[M], both real.
VSP_HD inline void fft_split_fwd(cf a, cf b, cf w, cf* xk, cf* xm) {
#pragma clang fp contract(off)
  const cf bc{b.x, -b.y};
  const cf s = cf_add(a, bc), d = cf_sub(a, bc);
  const cf e{0.5f * s.x, 0.5f * s.y}, o{0.5f * d.y, -0.5f * d.x};
  const cf wo = cf_mul_conj(o, w);
  *xk = cf_add(e, wo);
  const cf m = cf_sub(e, wo);
  *xm = cf{m.x, -m.y};
}

// Inverse split, twice the exact one (the synthesis window carries 1 / N for it and for the M of the passes):
//   Z[k] = E + i O, Z[M - k] = conj(E) + i conj(O), E = X[k] + conj X[M - k], O = e^{+2 pi i k / N} (X[k] - conj X[M - k]).
VSP_HD inline void fft_split_inv(cf xk, cf xm, cf w, cf* a, cf* b) {
  const cf mc{xm.x, -xm.y};
  const cf e = cf_add(xk, mc), o = cf_mul(cf_sub(xk, mc), w);
  *a = cf_add(e, cf{-o.y, o.x});
  *b = cf_add(cf{e.x, -e.y}, cf{o.y, o.x});
}

// The subtraction of denoise_subtract_kernel on one bin: q = max(m - thr, 0) / m (0 where m = 0), X' = q X.
VSP_HD inline cf fft_subtract(cf x, float thr) {
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
  const float m = sqrtf(x.x * x.x + x.y * x.y);
  const float q = m > 0.f ? fmaxf(m - thr, 0.f) / m : 0.f;
#else
  const float m = __builtin_sqrtf(x.x * x.x + x.y * x.y);
  const float q = m > 0.f ? __builtin_fmaxf(m - thr, 0.f) / m : 0.f;
#endif
  return cf{q * x.x, q * x.y};
}

}  // namespace vsp
