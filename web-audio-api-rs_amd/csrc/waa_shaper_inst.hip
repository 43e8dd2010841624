// waa_shaper_inst.hip — WaveShaperNode (oversample "none") with one curve per instance of the batch
// (waa_waveshaper_set_curve_instance), node-major in one launch.
//
// The chain kernels read ONE curve per launch and stage it once per workgroup, whose four wavefronts may belong to different
// instances (waa_kernels.hip).  Here the workgroup is the unit: 256 threads render one time tile (SHAPER_TILE frames) of ONE
// instance, all of its channels, so the instance's curve is staged once and serves every channel of the tile.
//   form A (LDS = true)   the curve in LDS; chosen when every curve of the node has at most SHAPER_LDS_CAP points
//   form B (LDS = false)  the curve read from global memory, where some curve of the node is longer
// An instance without a curve (ShaperRow::length 0) copies its input.  The input follows the convention of the compressor's
// kernels: a materialised signal, or a source read in place whose frames at or past `in_valid` are silence.  Frames past the
// render are written as zeros, like every signal's padding.  16-byte loads and stores throughout; no scratch, no spills
// (tests/test_waveshaper_per_instance.py reads the code object).
//
// Arithmetic: the lookup IS apply_curve / apply_curve_lds of the chain kernels (waa_curve.hpp), built like the rest of the library
// with -ffp-contract=off and -fgpu-flush-denormals-to-zero: a shaper's output does not depend on whether its curve was shared or
// per-instance.
#include <hip/hip_runtime.h>

#include "waa_curve.hpp"
#include "waa_internal.hpp"

namespace waa {

namespace {

// 4 consecutive frames of one channel; frames at or past `valid` are silence
__device__ __forceinline__ float4 shaper_read4(const float* ch, uint64_t f0, uint64_t valid) {
  if (f0 + 4 <= valid) return *reinterpret_cast<const float4*>(ch + f0);
  float r[4];
#pragma unroll
  for (int e = 0; e < 4; e++) r[e] = f0 + e < valid ? ch[f0 + e] : 0.f;
  return make_float4(r[0], r[1], r[2], r[3]);
}

}  // namespace

// grid n_inst x (frames / SHAPER_TILE) workgroups, instance-major, 256 threads; per pass a thread takes 4 frames of every channel (a wavefront covers 1 KB
// per plane and instruction), SHAPER_TILE / 1024 passes per workgroup.
template <bool LDS>
__global__ __launch_bounds__(256) void shaper_inst_kernel(const ShaperInstDesc d) {
  extern __shared__ __attribute__((aligned(16))) float curve_s[];
  const uint32_t n_tiles = (uint32_t)((d.frames + SHAPER_TILE - 1) / SHAPER_TILE);
  const uint32_t inst = blockIdx.x / n_tiles;
  const ShaperRow row = d.rows[inst];
  const float* curve = d.pool + row.offset;
  const int nn = (int)row.length;
  if constexpr (LDS) {
    // (whole 16-byte groups: a row starts on a 16-byte boundary and the pool is padded, lds_floats covers the longest row's groups)
    for (uint32_t i = threadIdx.x * 4u; i < row.length; i += 1024u)
      *reinterpret_cast<float4*>(curve_s + i) = *reinterpret_cast<const float4*>(curve + i);
    __syncthreads();
  }
  const float* in = d.in.base + (uint64_t)inst * d.in.inst_stride;
  float* out = d.out.base + (uint64_t)inst * d.out.inst_stride;
  const uint64_t rendered = (uint64_t)d.n_quanta * RQ;
  const uint64_t t0 = (uint64_t)(blockIdx.x % n_tiles) * SHAPER_TILE;
#pragma unroll 1
  for (int p = 0; p < SHAPER_TILE / 1024; p++) {
    const uint64_t f0 = t0 + (uint64_t)p * 1024 + threadIdx.x * 4u;
    if (f0 >= d.frames) return;
    for (int c = 0; c < d.nch; c++) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (f0 < rendered) {
        v = shaper_read4(in + (uint64_t)c * d.in.ch_stride, f0, d.in_valid);
        if (nn > 0) {
          if constexpr (LDS) {
            const auto* cs = (const __attribute__((address_space(3))) float*)curve_s;
            v = make_float4(apply_curve_lds(cs, nn, v.x), apply_curve_lds(cs, nn, v.y), apply_curve_lds(cs, nn, v.z), apply_curve_lds(cs, nn, v.w));
          } else {
            v = make_float4(apply_curve(curve, nn, v.x), apply_curve(curve, nn, v.y), apply_curve(curve, nn, v.z), apply_curve(curve, nn, v.w));
          }
        }
      }
      *reinterpret_cast<float4*>(out + (uint64_t)c * d.out.ch_stride + f0) = v;
    }
  }
}

void launch_shaper_inst(const ShaperInstDesc& d, void* stream) {
  const dim3 grid((uint32_t)((d.frames + SHAPER_TILE - 1) / SHAPER_TILE) * d.n_inst), block(256);  // (< 2^31: plan_shaper_per_instance)
  if (d.lds_floats)
    hipLaunchKernelGGL(shaper_inst_kernel<true>, grid, block, (size_t)d.lds_floats * sizeof(float), (hipStream_t)stream, d);
  else
    hipLaunchKernelGGL(shaper_inst_kernel<false>, grid, block, 0, (hipStream_t)stream, d);
}

}  // namespace waa
