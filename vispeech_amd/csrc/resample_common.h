// What the output stage (resample.hip) and the input stage (input_stage.hip) share: the plan and the Kaiser-windowed sinc of
// include/vispeech_hip.h ("output stage" / "input stage": one formula, the rates swapped), the polyphase table [P][L] both
// kernels read, and the FMA chain of one output sample.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

#include "../../include/vispeech_hip.h"

namespace vsp {
namespace rs {

// One output sample from global memory: acc = fmaf(tab[i][col], x[ks + i], acc), i = 0 .. P - 1 ascending; `sample(k)` is
// input sample k of the utterance, 0 where it is not readable.  The LDS loops of resample_kernel and input_kernel run this
// very chain.
template <class Sample>
__device__ __forceinline__ float rs_one_output(const float* __restrict__ tcol, int L, int P, int64_t ks, Sample sample) {
  float acc = 0.f;
#pragma unroll 4
  for (int i = 0; i < P; ++i) acc = fmaf(tcol[(size_t)i * L], sample(ks + i), acc);   // (loads in flight; the order stays)
  return acc;
}

// The PCM16 value of an output sample (resample.hip and output_rows.hip alike)
__device__ __forceinline__ int rs_pcm16(float y) {
  // service.pcm16: clip(rint(y * 32767.0f), -32768, 32767), product in fp32, round half to even
  const float r = rintf(y * 32767.0f);
  return (int)fminf(fmaxf(r, -32768.f), 32767.f);
}

inline double bessel_i0(double x) {
  const double q = x * x / 4.0;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 500; ++k) {
    term *= q / ((double)k * k);
    sum += term;
    if (term < sum * 1e-18) break;
  }
  return sum;
}

struct Plan { int L = 0, M = 0, H = 0; };

// from_rate -> to_rate by L / M; the stages differ only in the largest L and M their kernels cover
inline int make_plan(int from_rate, int to_rate, int zeros, int max_L, int max_M, Plan& p) {
  if (from_rate <= 0 || to_rate <= 0 || zeros < 1) return VSP_ERR_ARG;
  const int g = std::gcd(from_rate, to_rate);
  p.L = to_rate / g;
  p.M = from_rate / g;
  if (p.L > max_L || p.M > max_M || zeros > 64) return VSP_ERR_UNSUPPORTED;
  p.H = (p.L == 1 && p.M == 1) ? 0 : zeros * std::max(p.L, p.M);    // L = M = 1: the pass-through, one unit tap
  return VSP_OK;
}

// h[n], n = -H .. H, in double precision (numpy's sinc and kaiser conventions)
inline void make_filter(const Plan& p, int zeros, double beta, double rolloff, std::vector<double>& h) {
  const int H = p.H;
  h.assign((size_t)2 * H + 1, 0.0);
  if (H == 0) { h[0] = 1.0; return; }
  const double fc = rolloff / std::max(p.L, p.M);
  const double i0b = bessel_i0(beta);
  const double pi = 3.14159265358979323846;
  for (int n = -H; n <= H; ++n) {
    const double r = (double)n / H;
    const double w = bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
    const double a = pi * fc * n;
    const double s = n == 0 ? 1.0 : std::sin(a) / a;
    h[(size_t)(n + H)] = p.L * fc * s * w;
  }
}

inline double default_rolloff(int zeros) { return 1.0 - 3.065 / zeros; }

// The polyphase table of resample.hip's header comment: tab[i][m mod L] = h[p(m) + (J - i) L], i = 0 .. P - 1, J = H / L,
// p(m) = m M mod L, zero where the tap lies outside [-H, H]; input sample k = floor(m M / L) - J + i.
inline void make_table(const Plan& p, const std::vector<double>& h, int& J, int& P, std::vector<float>& tab) {
  const int L = p.L, M = p.M, H = p.H;
  J = H / L;
  P = J + (H + L - 1) / L + 1;
  tab.assign((size_t)P * L, 0.f);
  for (int c = 0; c < L; ++c) {
    const int64_t ph = ((int64_t)c * M) % L;
    for (int i = 0; i < P; ++i) {
      const int64_t t = ph + (int64_t)(J - i) * L;
      if (t >= -H && t <= H) tab[(size_t)i * L + c] = (float)h[(size_t)(t + H)];
    }
  }
}

inline int64_t floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
inline int64_t ceil_div(int64_t a, int64_t b) { return -floor_div(-a, b); }

}  // namespace rs
}  // namespace vsp
