// waa_biquad_coef_inst.hip — the per-frame Biquad coefficient table of a node whose instances differ in their filter TYPE
// (waa_biquad_set_type_instance): biquad_coef_kernel (waa_kernels.hip) with the type read from a table, one byte per instance,
// uploaded at plan time.  The element is biquad_coef_element (waa_biquad_coef.hpp), the shared kernel's body: same clamp, same
// exp2f for detune, same eight branches, both table layouts.  No LDS, no scratch, no spills
// (tests/test_biquad_per_instance_type.py reads the code object).
#include <hip/hip_runtime.h>

#include "waa_biquad_coef.hpp"
#include "waa_internal.hpp"

namespace waa {

// One filter type per instance (waa_biquad_set_type_instance): types[rows], one byte each, rows = n_inst.  frames_padded is a
// multiple of the tile (2048), so the 256 threads of a block lie inside one instance and the type is read once per block, from an
// address formed of blockIdx alone: the switch stays a uniform branch.  A block that straddled two instances (a frames_padded
// that is no multiple of 256) reads per thread instead and is still correct, with a divergent switch.
__global__ __launch_bounds__(256) void biquad_coef_inst_kernel(const BiquadCoefDesc d, const uint8_t* __restrict__ types) {
  const uint64_t total = (uint64_t)d.rows * d.frames_padded;
  const uint64_t first = (uint64_t)blockIdx.x * 256, idx = first + threadIdx.x;
  if (idx >= total) return;
  const uint64_t last = first + 255 < total ? first + 255 : total - 1;
  const uint64_t i0 = first / d.frames_padded, i1 = last / d.frames_padded;
  int type = types[i0];
  if (i0 != i1) type = types[idx / d.frames_padded];
  biquad_coef_element(d, idx, type);
}
void launch_biquad_coefs_inst(const BiquadCoefDesc& d, const uint8_t* types, void* stream) {
  const uint64_t total = (uint64_t)d.rows * d.frames_padded;
  hipLaunchKernelGGL(biquad_coef_inst_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d, types);
}

}  // namespace waa
