// Per-row controls (vsp_set_row_controls, round 13): the four element-wise formulas the scalar controls enter, each as ONE
// __device__ function that the scalar kernels (misc.hip) and the per-row kernels (row_controls.hip) both evaluate -- so a
// table whose rows all carry the same values gives the scalar call's bits -- and the per-row launches.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/vispeech_hip.h"

namespace vsp {

// duration = ceil((exp(logw) * mask - 1) * duration_control)   (reference models.py:686-688)
__device__ __forceinline__ float duration_from_logw(float logw, float mask, float scale) {
  const float e = expf(logw) * mask;
  return ceilf((e - 1.f) * scale);
}
// LF0 of a given pitch control / of the prediction, and F0 of either (reference models.py:691-698; the 2590 in the F0
// formula is the reference's constant)
__device__ __forceinline__ float lf0_from_control(float pitch) { return (2595.f * log10f(1.f + pitch / 700.f)) / 500.f; }
__device__ __forceinline__ float lf0_from_prediction(float pred, float scale) { return pred * scale; }
__device__ __forceinline__ float f0_from_lf0(float l) { return (powf(10.f, l * 500.f / 2590.f) - 1.f) * 700.f; }
// normalised energy of a given control / of the prediction, and the energy of either (reference models.py:701-708)
__device__ __forceinline__ float norm_energy_from_control(float energy) { return (energy - 60.f) / 36.f; }
__device__ __forceinline__ float norm_energy_from_prediction(float pred, float scale) {
  return (((pred * 36.f + 60.f) * scale) - 60.f) / 36.f;
}
__device__ __forceinline__ float energy_from_norm(float ne) { return ne * 36.f + 60.f; }
// z_p = m_p + noise * exp(logs_p) * noise_scale  (reference models.py:718)
__device__ __forceinline__ float reparam_value(float m_p, float logs_p, float noise, float noise_scale) {
  return m_p + noise * expf(logs_p) * noise_scale;
}

// The per-row forms: rows [B] on the device (this call's workspace), the row index from the grid.  A *_ctl / prediction
// pointer is read only in the rows that select it, so it may be NULL when no row does.
hipError_t launch_duration_rows(const float* logw, const float* duration_ctl, const int64_t* lengths,
                                const vsp_row_control* rows, float* dur, int B, int T, hipStream_t s);
hipError_t launch_pitch_rows(const float* pitch_ctl, const float* lf0_pred, const vsp_row_control* rows, float* lf0,
                             float* f0, int B, int T, hipStream_t s);
hipError_t launch_energy_rows(const float* energy_ctl, const float* e_pred, const vsp_row_control* rows, float* norm_e,
                              float* energy, int B, int T, hipStream_t s);
// m_p, logs_p, noise (or NULL), z_p, copy (or NULL): contiguous [B][row] tensors
hipError_t launch_reparam_rows(const float* m_p, const float* logs_p, const float* noise, const vsp_row_control* rows,
                               float* z_p, int B, long row, hipStream_t s, float* copy, unsigned* flags);

}  // namespace vsp
