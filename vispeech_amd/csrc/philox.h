// Philox4x32-10 (Salmon et al., SC'11) and the Box-Muller draw of the library's noise streams, shared by the kernels that
// draw from them (misc.hip, convert_window.hip).  Element i of the stream keyed `seed` is word i % 4 of counter i / 4.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace vsp {

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t out[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// Element e of the standard-normal stream keyed `seed`, alone: the arithmetic of randn_kernel for one of its four values
// (uniforms: the top 23 bits, (x + 0.5) / 2^23 -- exact in fp32, strictly inside (0, 1)).
__device__ __forceinline__ float philox_randn_element(uint64_t seed, long e) {
  const long q = e >> 2;
  const int j = (int)(e & 3), p = j >> 1;
  uint32_t w[4];
  philox4x32_10((uint32_t)(q & 0xffffffffu), (uint32_t)((unsigned long)q >> 32), 0u, 0u, (uint32_t)(seed & 0xffffffffu),
                (uint32_t)(seed >> 32), w);
  const float u1 = ((float)(w[2 * p] >> 9) + 0.5f) * (1.f / 8388608.f);
  const float u2 = ((float)(w[2 * p + 1] >> 9) + 0.5f) * (1.f / 8388608.f);
  const float rad = sqrtf(-2.f * logf(u1));
  float sn, cs;
  sincosf(6.283185307179586f * u2, &sn, &cs);
  return (j & 1) ? rad * sn : rad * cs;
}

}  // namespace vsp
