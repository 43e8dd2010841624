// waa_curve.hpp — the WaveShaper's curve lookup (device only), shared by the chain kernels (waa_kernels.hip) and the per-instance
// shaper (waa_shaper_inst.hip): one expression, so that a shaper's output does not depend on which of the two renders it.
#pragma once
#include <hip/hip_runtime.h>

namespace waa {

// waveshaper.rs:555-573
__device__ __forceinline__ float apply_curve(const float* curve, int nn, float input) {
  if (nn == 0) return 0.f;
  const float n = (float)nn;
  const float v = (n - 1.f) / 2.0f * (input + 1.f);
  if (v <= 0.f) return curve[0];
  if (v >= n - 1.f) return curve[nn - 1];
  const float k = floorf(v);
  const float f = v - k;
  const int ki = (int)k;
  return (1.f - f) * curve[ki] + f * curve[ki + 1];
}

// the same lookup on a curve staged in LDS
__device__ __forceinline__ float apply_curve_lds(const __attribute__((address_space(3))) float* curve, int nn, float input) {
  if (nn == 0) return 0.f;
  const float n = (float)nn;
  const float v = (n - 1.f) / 2.0f * (input + 1.f);
  if (v <= 0.f) return curve[0];
  if (v >= n - 1.f) return curve[nn - 1];
  const float k = floorf(v);
  const float f = v - k;
  const int ki = (int)k;
  return (1.f - f) * curve[ki] + f * curve[ki + 1];
}

}  // namespace waa
