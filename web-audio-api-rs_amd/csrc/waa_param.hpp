// waa_param.hpp — reading an AudioParam's value on the device (ParamRef, waa_internal.hpp): one value per instance, per render
// quantum or per frame.  Shared by the chain kernels (waa_kernels.hip) and the Biquad coefficient element (waa_biquad_coef.hpp).
#ifndef WAA_PARAM_HPP
#define WAA_PARAM_HPP

#include <hip/hip_runtime.h>

#include "waa_internal.hpp"

namespace waa {

__device__ __forceinline__ float param_at(const ParamRef& p, uint32_t inst, uint32_t q, uint64_t frame) {
  if (p.mode == 0) return p.base[inst];
  if (p.mode == 1) return p.base[(uint64_t)inst * p.stride + q];
  return p.base[(uint64_t)inst * p.stride + frame];
}

}  // namespace waa

#endif  // WAA_PARAM_HPP
