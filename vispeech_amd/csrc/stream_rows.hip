// Streaming for batched requests (include/vispeech_hip.h, vsp_generator_stream_rows): the two copy kernels around the
// generator run.  Row b of a call is the window [lo, hi) of its OWN utterance's latent, anywhere on the device:
//   stream_gather   packs every row's z[:, lo:hi) into one [B][C][S] tensor (zero behind hi - lo), copies the speaker
//                   vectors into [B][gin] and writes the device lengths hi - lo -- what run_gen needs, in one launch;
//   stream_collect  cuts row b's delivered samples out of the span waveform, writes them as float32 or PCM16 and
//                   zeroes the rest of the row -- one launch instead of a 2D copy plus a host-side quantiser.
// The row descriptors travel BY VALUE in the kernel arguments (64 rows x 32 B, 64 x 8 B): no host-to-device copy, nothing
// to keep alive behind the launch.  A block serves one row (blockIdx.y), so a descriptor is read through scalar loads.
// Both kernels move 16 bytes per lane where the addresses allow and go element by element at the ragged edges.
#include "kernels.h"
#include "resample_common.h"   // (rs_pcm16: the output stage's PCM16 value)

namespace vsp {

namespace {

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// grid (quad blocks of C * S4 / 4  +  blocks of gin, B), 256 threads.  zp row stride S4 (a multiple of 4, zp 16-byte
// aligned: every destination quad is one aligned 16-byte store).  The source quad z[c * cs + lo + t .. + 4) is one 16-byte
// load when it lies inside the window and is aligned (lo, cs multiples of 4 on an aligned z), else up to four scalar loads.
__global__ void __launch_bounds__(256) stream_gather_kernel(const StreamGatherRows rows, int C, int S4, int gin, int z_blocks,
                                                            float* __restrict__ zp, float* __restrict__ gp,
                                                            int64_t* __restrict__ len) {
  const int b = blockIdx.y;
  const StreamGatherRow& r = rows.r[b];
  const int n = r.hi - r.lo;
  if ((int)blockIdx.x >= z_blocks) {
    const int k = ((int)blockIdx.x - z_blocks) * blockDim.x + threadIdx.x;
    if (k < gin) gp[(size_t)b * gin + k] = r.g[k];
    if (k == 0) len[b] = n;
    return;
  }
  const int q4 = S4 / 4;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= C * q4) return;
  const int c = idx / q4, t = (idx - c * q4) * 4;
  const float* src = r.z + (size_t)c * r.cs + r.lo + t;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (t + 4 <= n && aligned16(src)) {
    v = *reinterpret_cast<const float4*>(src);
  } else if (t < n) {
    v.x = src[0];
    if (t + 1 < n) v.y = src[1];
    if (t + 2 < n) v.z = src[2];
    if (t + 3 < n) v.w = src[3];
  }
  *reinterpret_cast<float4*>(zp + ((size_t)b * C + c) * S4 + t) = v;
}

// grid (quads of out_stride, B), 256 threads: out[b][i] = i < n ? o_span[b][off + i] : 0 for i < out_stride.
template <bool PCM>
__global__ void __launch_bounds__(256) stream_collect_kernel(const float* __restrict__ o_span, long o_bs,
                                                             const StreamCollectRows rows, void* __restrict__ out,
                                                             long out_stride, int vec_out) {
  const int b = blockIdx.y;
  const long off = rows.r[b].off, n = rows.r[b].n;
  const long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= out_stride) return;
  const float* src = o_span + (size_t)b * o_bs + off + i;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (i + 4 <= n && aligned16(src)) {
    const float4 f = *reinterpret_cast<const float4*>(src);
    v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i + k < n) v[k] = src[k];
  }
  const bool whole = vec_out && i + 4 <= out_stride;
  if (PCM) {
    int16_t* o = static_cast<int16_t*>(out) + (size_t)b * out_stride + i;
    // (a sample behind n is the quantised 0.0f = 0: the row's rest is exactly zero)
    if (whole) {
      const uint32_t w0 = (uint32_t)(uint16_t)rs::rs_pcm16(v[0]) | ((uint32_t)(uint16_t)rs::rs_pcm16(v[1]) << 16);
      const uint32_t w1 = (uint32_t)(uint16_t)rs::rs_pcm16(v[2]) | ((uint32_t)(uint16_t)rs::rs_pcm16(v[3]) << 16);
      *reinterpret_cast<uint2*>(o) = make_uint2(w0, w1);
      return;
    }
    for (int k = 0; k < 4 && i + k < out_stride; ++k) o[k] = (int16_t)rs::rs_pcm16(v[k]);
  } else {
    float* o = static_cast<float*>(out) + (size_t)b * out_stride + i;
    if (whole) {
      *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
      return;
    }
    for (int k = 0; k < 4 && i + k < out_stride; ++k) o[k] = v[k];
  }
}

}  // namespace

hipError_t launch_stream_gather(const StreamGatherRows& rows, int B, int C, int S4, int gin, float* zp, float* gp,
                                int64_t* len, hipStream_t s) {
  if (B <= 0 || B > STREAM_ROWS_MAX || C <= 0 || S4 <= 0 || (S4 & 3) || gin <= 0 || !zp || !gp || !len ||
      (reinterpret_cast<uintptr_t>(zp) & 15))
    return hipErrorInvalidValue;
  for (int b = 0; b < B; ++b)
    if (!rows.r[b].z || !rows.r[b].g || rows.r[b].lo < 0 || rows.r[b].hi <= rows.r[b].lo || rows.r[b].hi - rows.r[b].lo > S4)
      return hipErrorInvalidValue;
  const long quads = (long)C * (S4 / 4);
  const int z_blocks = (int)((quads + 255) / 256), g_blocks = (gin + 255) / 256;
  hipLaunchKernelGGL(stream_gather_kernel, dim3(z_blocks + g_blocks, B), dim3(256), 0, s, rows, C, S4, gin, z_blocks, zp, gp,
                     len);
  return hipGetLastError();
}

hipError_t launch_stream_collect(const float* o_span, long o_bs, const StreamCollectRows& rows, int B, void* out,
                                 long out_stride, int pcm, hipStream_t s) {
  if (B <= 0 || B > STREAM_ROWS_MAX || !o_span || !out || out_stride <= 0 || o_bs <= 0) return hipErrorInvalidValue;
  for (int b = 0; b < B; ++b)
    if (rows.r[b].off < 0 || rows.r[b].n < 0 || rows.r[b].n > out_stride || (long)rows.r[b].off + rows.r[b].n > o_bs)
      return hipErrorInvalidValue;
  // whole quads of a row are one 16-byte (float) / 8-byte (PCM16) store when every row starts on such a boundary
  const uintptr_t mask = pcm ? 7 : 15;
  const int vec_out = (reinterpret_cast<uintptr_t>(out) & mask) == 0 && out_stride % 4 == 0;
  const dim3 grid((unsigned)((out_stride + 1023) / 1024), B);
  if (pcm) hipLaunchKernelGGL(stream_collect_kernel<true>, grid, dim3(256), 0, s, o_span, o_bs, rows, out, out_stride, vec_out);
  else hipLaunchKernelGGL(stream_collect_kernel<false>, grid, dim3(256), 0, s, o_span, o_bs, rows, out, out_stride, vec_out);
  return hipGetLastError();
}

}  // namespace vsp
