// Per-row forms of the four element-wise kernels the scalar controls enter (vsp_set_row_controls; the scalar forms are in
// misc.hip and evaluate the same __device__ functions, row_controls.h).  The row index is a grid coordinate, so a row's
// table entry (20 bytes) is a wave-uniform load and the source select is a uniform branch; threads run along T, every
// global access is coalesced.  Launch-bound at every size this project runs.
#include "row_controls.h"

#include <math.h>

#include "kernels.h"   // (vsp_raise_flag)

namespace vsp {

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// duration: row b of duration_ctl where given, else ceil((exp(logw) * mask - 1) * duration_scale[b])
__global__ void __launch_bounds__(64) duration_rows_kernel(const float* __restrict__ logw, const float* __restrict__ duration_ctl,
                                                           const int64_t* __restrict__ lengths,
                                                           const vsp_row_control* __restrict__ rows, float* __restrict__ dur, int T) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (t >= T) return;
  const vsp_row_control rc = rows[b];
  const size_t i = (size_t)b * T + t;
  if (rc.given & VSP_GIVEN_DURATION) {
    dur[i] = duration_ctl[i];
  } else {
    const float m = t < (int)lengths[b] ? 1.f : 0.f;
    dur[i] = duration_from_logw(logw[i], m, rc.duration_scale);
  }
}
hipError_t launch_duration_rows(const float* logw, const float* duration_ctl, const int64_t* lengths,
                                const vsp_row_control* rows, float* dur, int B, int T, hipStream_t s) {
  if (!lengths || !rows || !dur || B <= 0 || T <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(duration_rows_kernel, dim3(cdiv(T, 64), B), dim3(64), 0, s, logw, duration_ctl, lengths, rows, dur, T);
  return hipGetLastError();
}

__global__ void __launch_bounds__(64) pitch_rows_kernel(const float* __restrict__ pitch_ctl, const float* __restrict__ lf0_pred,
                                                        const vsp_row_control* __restrict__ rows, float* __restrict__ lf0,
                                                        float* __restrict__ f0, int T) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (t >= T) return;
  const vsp_row_control rc = rows[b];
  const size_t i = (size_t)b * T + t;
  float l;
  if (rc.given & VSP_GIVEN_PITCH) {
    l = lf0_from_control(pitch_ctl[i]);
  } else {
    l = lf0_from_prediction(lf0_pred[i], rc.pitch_scale);
  }
  lf0[i] = l;
  f0[i] = f0_from_lf0(l);
}
hipError_t launch_pitch_rows(const float* pitch_ctl, const float* lf0_pred, const vsp_row_control* rows, float* lf0,
                             float* f0, int B, int T, hipStream_t s) {
  if (!rows || !lf0 || !f0 || B <= 0 || T <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pitch_rows_kernel, dim3(cdiv(T, 64), B), dim3(64), 0, s, pitch_ctl, lf0_pred, rows, lf0, f0, T);
  return hipGetLastError();
}

__global__ void __launch_bounds__(64) energy_rows_kernel(const float* __restrict__ energy_ctl, const float* __restrict__ e_pred,
                                                         const vsp_row_control* __restrict__ rows, float* __restrict__ norm_e,
                                                         float* __restrict__ energy, int T) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (t >= T) return;
  const vsp_row_control rc = rows[b];
  const size_t i = (size_t)b * T + t;
  float ne;
  if (rc.given & VSP_GIVEN_ENERGY) {
    ne = norm_energy_from_control(energy_ctl[i]);
  } else {
    ne = norm_energy_from_prediction(e_pred[i], rc.energy_scale);
  }
  norm_e[i] = ne;
  energy[i] = energy_from_norm(ne);
}
hipError_t launch_energy_rows(const float* energy_ctl, const float* e_pred, const vsp_row_control* rows, float* norm_e,
                              float* energy, int B, int T, hipStream_t s) {
  if (!rows || !norm_e || !energy || B <= 0 || T <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(energy_rows_kernel, dim3(cdiv(T, 64), B), dim3(64), 0, s, energy_ctl, e_pred, rows, norm_e, energy, T);
  return hipGetLastError();
}

// z_p = m_p + noise * exp(logs_p) * noise_scale[b] over utterance b's [row] elements; the same non-finite flag as
// reparam_kernel
__global__ void __launch_bounds__(256) reparam_rows_kernel(const float* __restrict__ m_p, const float* __restrict__ logs_p,
                                                           const float* __restrict__ noise,
                                                           const vsp_row_control* __restrict__ rows, float* __restrict__ z_p,
                                                           long row, float* __restrict__ copy, unsigned* __restrict__ flags) {
  const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (j >= row) return;
  const float noise_scale = rows[b].noise_scale;
  const long i = (long)b * row + j;
  const float nz = noise ? noise[i] : 0.f;
  const float v = reparam_value(m_p[i], logs_p[i], nz, noise_scale);
  z_p[i] = v;
  if (copy) copy[i] = v;
  if (flags && !(fabsf(v) <= 3.0e38f)) vsp_raise_flag(flags, VSP_FLAG_NONFINITE_LATENT);
}
hipError_t launch_reparam_rows(const float* m_p, const float* logs_p, const float* noise, const vsp_row_control* rows,
                               float* z_p, int B, long row, hipStream_t s, float* copy, unsigned* flags) {
  if (!m_p || !logs_p || !rows || !z_p || B <= 0 || row <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(reparam_rows_kernel, dim3(cdiv(row, 256), B), dim3(256), 0, s, m_p, logs_p, noise, rows, z_p, row, copy,
                     flags);
  return hipGetLastError();
}

}  // namespace vsp
