// Stand-alone host program for a sanitizer build: the pass structure of the in-LDS real FFT (vispeech_amd/csrc/fft_plan.h,
// fft.hip) run on the CPU in float, item after item in the order of the kernel's loops, on frame
// images of exactly FFT_M slots -- an index outside one is a heap overflow here.  Checked for N = 2048, for every frame
// skew of the tiles 4, 8 and 16: the slots are a permutation, the forward transform and the inverse are the fp64 sums of
// tests/denoiser_ref.py within a few roundings, a frame's bits do not depend on its skew, and forward, subtraction at
// strength 0 and inverse give the windowed frame back.  Exit status 0 = every check held.
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -ffp-contract=off tools/micro/fft_plan_main.cpp -o fft_plan && ./fft_plan
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../vispeech_amd/csrc/fft_plan.h"

using namespace vsp;

static int failures = 0;
#define EXPECT(cond)                                                         \
  do {                                                                       \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

static std::vector<float> tab(FFT_TAB_FLOATS);
static const cf* tw() { return reinterpret_cast<const cf*>(tab.data() + FFT_TAB_TW); }
static const cf* split() { return reinterpret_cast<const cf*>(tab.data() + FFT_TAB_SPLIT); }

// the kernel's staging loop: sample n of the frame times the analysis window
static void stage(std::vector<cf>& z, int skew, const float* x) {
  float* f = reinterpret_cast<float*>(z.data());
  for (int n = 0; n < FFT_N; ++n) f[fft_sample_slot(skew, n)] = x[n] * tab[FFT_TAB_WA + n];
}

static void forward_passes(std::vector<cf>& z, int skew) {
  for (int p = 0; p < FFT_PASSES; ++p)
    for (int j = 0; j < FFT_THREADS; ++j) {
      const FftBfly b = fft_bfly(p, j);
      EXPECT(b.base >= 0 && b.base + 3 * b.q < FFT_M && 3 * b.twi < FFT_M);
      fft_fwd_bfly(z.data(), skew, b, tw()[b.twi], tw()[2 * b.twi], tw()[3 * b.twi]);
    }
}

static void inverse_passes(std::vector<cf>& z, int skew) {
  for (int p = FFT_PASSES - 1; p >= 0; --p)
    for (int j = 0; j < FFT_THREADS; ++j) {
      const FftBfly b = fft_bfly(p, j);
      fft_inv_bfly(z.data(), skew, b, tw()[b.twi], tw()[2 * b.twi], tw()[3 * b.twi]);
    }
}

// the fused kernel's middle: split, subtraction with thr[r], inverse split, in place; spec (if given) receives X'[0 .. M]
static void split_subtract(std::vector<cf>& z, int skew, const float* thr, cf* spec) {
  std::vector<int> seen(FFT_M + 1, 0);
  for (int j = 0; j < FFT_SPLIT_ITEMS; ++j) {
    const int k = fft_split_bin(j);
    EXPECT(k >= 0 && k <= FFT_M / 2);
    const int sk = fft_slot(skew, fft_split_pos(k)), sm = fft_slot(skew, fft_split_pair(k));
    cf xk, xm, a, b;
    fft_split_fwd(z[sk], z[sm], split()[k], &xk, &xm);
    xk = fft_subtract(xk, thr[k]);
    xm = fft_subtract(xm, thr[FFT_M - k]);
    ++seen[k];
    if (k != FFT_M / 2) ++seen[FFT_M - k];
    if (spec) { spec[k] = xk; spec[FFT_M - k] = xm; }
    fft_split_inv(xk, xm, split()[k], &a, &b);
    z[sk] = a;
    if (k != 0 && k != FFT_M / 2) z[sm] = b;
  }
  for (int r = 0; r <= FFT_M; ++r) EXPECT(seen[r] == 1);
}

int main() {
  fft_fill_tables(tab.data());
  EXPECT(tab[FFT_TAB_TW] == 1.f && tab[FFT_TAB_TW + 1] == 0.f && tab[FFT_TAB_TW + 2 * (FFT_M / 4)] == 0.f);
  EXPECT(tab[FFT_TAB_SPLIT + 2 * (FFT_M / 2)] == 0.f && tab[FFT_TAB_SPLIT + 2 * (FFT_M / 2) + 1] == 1.f);

  // the index math: reversal is an involution, the slots of every frame skew are a permutation of [0, M)
  for (int k = 0; k < FFT_M; ++k) EXPECT(fft_rev(k) >= 0 && fft_rev(k) < FFT_M && fft_rev(fft_rev(k)) == k);
  for (int tile = 4; tile <= FFT_MAX_TILE; tile *= 2)
    for (int tl = 0; tl < tile; ++tl) {
      const int skew = fft_frame_skew(tl, tile);
      std::vector<int> hit(FFT_M, 0);
      for (int pos = 0; pos < FFT_M; ++pos) {
        const int s = fft_slot(skew, pos);
        EXPECT(s >= 0 && s < FFT_M);
        if (s >= 0 && s < FFT_M) ++hit[s];
      }
      for (int s = 0; s < FFT_M; ++s) EXPECT(hit[s] == 1);
    }
  // ... and conflict-free where the header says so: the 32 lanes of a group meet 32 different bank pairs in every pass
  for (int p = 0; p < FFT_PASSES; ++p)
    for (int g = 0; g < FFT_THREADS / 32; ++g)
      for (int i = 0; i < 4; ++i) {
        uint32_t banks = 0;
        for (int l = 0; l < 32; ++l) {
          const FftBfly b = fft_bfly(p, 32 * g + l);
          banks |= 1u << (fft_slot(5, b.base + i * b.q) & 31);
        }
        EXPECT(banks == 0xffffffffu);
      }

  // one frame of noise under a slow sine, peak about 1
  std::vector<float> x(FFT_N);
  uint32_t lcg = 12345u;
  for (int n = 0; n < FFT_N; ++n) {
    lcg = lcg * 1664525u + 1013904223u;
    x[n] = 0.5f * (float)std::sin(0.05 * n) + ((float)(lcg >> 8) / 16777216.f - 0.5f);
  }
  // fp64: X[r] = sum_n hann[n] x[n] e^{-2 pi i r n / N}
  std::vector<double> Xr(FFT_M + 1), Xi(FFT_M + 1), hann(FFT_N);
  const double pi = 3.14159265358979323846;
  for (int n = 0; n < FFT_N; ++n) hann[n] = 0.5 - 0.5 * std::cos(2.0 * pi * n / FFT_N);
  double peak = 0;
  for (int r = 0; r <= FFT_M; ++r) {
    double sr = 0, si = 0;
    for (int n = 0; n < FFT_N; ++n) {
      const double a = 2.0 * pi * (double)(((long)r * n) % FFT_N) / FFT_N, v = hann[n] * x[n];
      sr += v * std::cos(a);
      si -= v * std::sin(a);
    }
    Xr[r] = sr; Xi[r] = si;
    peak = std::fmax(peak, std::hypot(sr, si));
  }

  const std::vector<float> zero(FFT_M + 1, 0.f);
  std::vector<cf> first_spec(FFT_M + 1), first_out;
  double worst_f = 0, worst_i = 0, worst_id = 0;
  for (int tile = 4; tile <= FFT_MAX_TILE; tile *= 2)
    for (int tl = 0; tl < tile; ++tl) {
      const int skew = fft_frame_skew(tl, tile);
      std::vector<cf> z(FFT_M), spec(FFT_M + 1);
      stage(z, skew, x.data());
      forward_passes(z, skew);
      split_subtract(z, skew, zero.data(), spec.data());      // strength 0: q = 1, the spectrum's own bits
      for (int r = 0; r <= FFT_M; ++r)
        worst_f = std::fmax(worst_f, std::hypot(spec[r].x - Xr[r], spec[r].y - Xi[r]));
      inverse_passes(z, skew);
      // v[n] = ws[n] * (sample n of the image), against hann[n] (hann[n] x[n]): the transform pair is the identity
      std::vector<cf> out(FFT_M);
      const float* f = reinterpret_cast<const float*>(z.data());
      float* o = reinterpret_cast<float*>(out.data());
      for (int n = 0; n < FFT_N; ++n) {
        o[n] = f[fft_sample_slot(skew, n)] * tab[FFT_TAB_WS + n];
        worst_id = std::fmax(worst_id, std::fabs(o[n] - hann[n] * hann[n] * x[n]));
      }
      if (first_out.empty()) { first_out = out; first_spec = spec; }
      EXPECT(std::memcmp(out.data(), first_out.data(), sizeof(cf) * FFT_M) == 0);         // a frame's bits: any place, any tile
      EXPECT(std::memcmp(spec.data(), first_spec.data(), sizeof(cf) * (FFT_M + 1)) == 0);
    }

  // the inverse alone, as the inverse kernel stages it: X'[r] = q X[r] with a threshold that bites, rounded to float, bins
  // 0 and M packed into slot 0 (their imaginary parts are not used); against the fp64 synthesis sum of the same floats
  {
    std::vector<cf> X(FFT_M + 1);
    for (int r = 0; r <= FFT_M; ++r) X[r] = fft_subtract(cf{(float)Xr[r], (float)Xi[r]}, 0.3f * (float)peak * (r % 7) / 7.f);
    X[0].y = 0.25f; X[FFT_M].y = -0.5f;                       // (must not reach the output)
    std::vector<double> want(FFT_N);
    for (int n = 0; n < FFT_N; ++n) {
      double s = 0;
      for (int r = 0; r <= FFT_M; ++r) {
        const double a = 2.0 * pi * (double)(((long)r * n) % FFT_N) / FFT_N, w = (r == 0 || r == FFT_M) ? 1.0 : 2.0;
        s += w * (X[r].x * std::cos(a) - X[r].y * std::sin(a));
      }
      want[n] = hann[n] * s / FFT_N;
    }
    const int skew = fft_frame_skew(3, 8);
    std::vector<cf> z(FFT_M);
    float* f = reinterpret_cast<float*>(z.data());
    for (int r = 0; r <= FFT_M; ++r) {
      if (r == 0) f[2 * fft_slot(skew, 0)] = X[0].x;
      else if (r == FFT_M) f[2 * fft_slot(skew, 0) + 1] = X[FFT_M].x;
      else z[fft_slot(skew, fft_rev(r))] = X[r];
    }
    for (int j = 0; j < FFT_SPLIT_ITEMS; ++j) {
      const int k = fft_split_bin(j);
      const int sk = fft_slot(skew, fft_split_pos(k)), sm = fft_slot(skew, fft_split_pair(k));
      const cf xk = k ? z[sk] : cf{z[sk].x, 0.f}, xm = k ? z[sm] : cf{z[sk].y, 0.f};
      cf a, b;
      fft_split_inv(xk, xm, split()[k], &a, &b);
      z[sk] = a;
      if (k != 0 && k != FFT_M / 2) z[sm] = b;
    }
    inverse_passes(z, skew);
    for (int n = 0; n < FFT_N; ++n)
      worst_i = std::fmax(worst_i, std::fabs((double)(f[fft_sample_slot(skew, n)] * tab[FFT_TAB_WS + n]) - want[n]));
  }

  // sqrt(4 log2 N) roundings of 2^-24 of the peak as a random walk, times 4: far under what a wrong index or factor gives
  const double u = std::ldexp(1.0, -24), walk = 4.0 * std::sqrt(4.0 * 11.0) * u;
  std::printf("forward: largest distance %.3e of a peak %.3e (bound %.3e)\n", worst_f, peak, walk * peak);
  std::printf("inverse: largest distance %.3e (bound %.3e)\n", worst_i, walk * 1.0);
  std::printf("forward + inverse at strength 0: largest distance %.3e (bound %.3e)\n", worst_id, walk * 1.0);
  EXPECT(worst_f <= walk * peak);
  EXPECT(worst_i <= walk * 1.0);
  EXPECT(worst_id <= walk * 1.0);
  std::printf(failures ? "%d check(s) FAILED\n" : "fft plan: ok\n", failures);
  return failures ? 1 : 0;
}
