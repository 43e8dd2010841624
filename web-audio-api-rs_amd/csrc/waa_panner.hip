// waa_panner.hip — per-frame geometry of the equal-power PannerNode when the AudioListener is automated at audio rate
// (panner.rs:720-779 a_rate_params, :830-897; spatial.rs:205-299).  With a single-valued listener the reference
// evaluates the geometry once per render quantum (from the FIRST value of every param, panner.rs:844-845) and the host
// does that (waa_plan.cpp, with the libm the reference resolves to).  As soon as one of the nine listener params is a
// 128-value slice, every frame has its own source / listener vectors: distance gain (f64), cone gain, azimuth in the
// listener's frame of reference, and from the wrapped azimuth the equal-power gains of the mono and the stereo law.
// These kernels evaluate them (panner_geom_frame, waa_panner_geom.hpp) for all frames of all instances (one table row per
// instance, or one row for the batch when nothing depends on the instance) into per-frame tables the panner op of the chain
// kernels reads like a-rate params.
// f32 vector algebra as in the reference; acosf / sinf / cosf are the device's (<= 1-2 ulp from the host libm).
#include <hip/hip_runtime.h>

#include "waa_internal.hpp"
#include "waa_panner_geom.hpp"

namespace waa {

// Everything that computes a gain is panner_geom_frame (waa_panner_geom.hpp), one definition for both kernels.  What addresses the
// descriptor — which frame, whether its quantum is single-valued, the fifteen loads, the seven stores: index arithmetic only —
// stands in each kernel: a by-value kernel argument handed to a function by reference is copied out of the kernel arguments up
// front, all 142 words of it (measured on panner_geom_kernel: 106 SGPRs with spills where it has 25, and 6 % of its time).

// one option set per node (PannerGeomDesc's scalars)
__global__ __launch_bounds__(256) void panner_geom_kernel(const PannerGeomDesc d) {
  const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (uint64_t)d.rows * d.n_frames) return;
  const uint32_t inst = (uint32_t)(idx / d.n_frames);
  const uint64_t frame = idx % d.n_frames;
  const uint32_t q = (uint32_t)(frame / RQ);
  // a single-valued listener: one geometry per quantum from the first value of every param (panner.rs:833-846)
  bool single = d.single[(uint64_t)inst * d.single_stride + q] != 0;
#pragma unroll
  for (int k = 0; k < 9; k++)
    if (d.dev_len[k]) single = single && d.dev_len[k][(uint64_t)inst * d.single_stride + q] == 1;
  const uint64_t f = single ? (uint64_t)q * RQ : frame;
  float v[15];
#pragma unroll
  for (int k = 0; k < 15; k++) {
    const ParamRef& p = d.p[k];
    v[k] = p.mode == 0 ? p.base[inst] : p.mode == 1 ? p.base[(uint64_t)inst * p.stride + q] : p.base[(uint64_t)inst * p.stride + f];
  }
  const PannerOptRow o{d.ref_distance, d.max_distance, d.rolloff, d.cone_inner, d.cone_outer, d.cone_outer_gain, d.distance_model};
  const PannerGeomOut g = panner_geom_frame(v, o);
  const uint64_t at = (uint64_t)inst * d.n_frames + frame;
  d.az[at] = g.az;
  d.gl_mono[at] = g.gl_mono;
  d.gr_mono[at] = g.gr_mono;
  d.gl_stereo[at] = g.gl_stereo;
  d.gr_stereo[at] = g.gr_stereo;
  d.dg[at] = g.dg;
  d.cg[at] = g.cg;
}

// One option set per instance (waa_panner_set_options_instance): d.opts[rows], rows = n_inst.  n_frames = n_quanta * 128 is no
// multiple of 256, so a block may straddle two instances: every thread reads the row of its own instance, and the distance
// model's branch may diverge inside such a block.
__global__ __launch_bounds__(256) void panner_geom_inst_kernel(const PannerGeomDesc d) {
  const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (uint64_t)d.rows * d.n_frames) return;
  const uint32_t inst = (uint32_t)(idx / d.n_frames);
  const uint64_t frame = idx % d.n_frames;
  const uint32_t q = (uint32_t)(frame / RQ);
  // a single-valued listener: one geometry per quantum from the first value of every param (panner.rs:833-846)
  bool single = d.single[(uint64_t)inst * d.single_stride + q] != 0;
#pragma unroll
  for (int k = 0; k < 9; k++)
    if (d.dev_len[k]) single = single && d.dev_len[k][(uint64_t)inst * d.single_stride + q] == 1;
  const uint64_t f = single ? (uint64_t)q * RQ : frame;
  float v[15];
#pragma unroll
  for (int k = 0; k < 15; k++) {
    const ParamRef& p = d.p[k];
    v[k] = p.mode == 0 ? p.base[inst] : p.mode == 1 ? p.base[(uint64_t)inst * p.stride + q] : p.base[(uint64_t)inst * p.stride + f];
  }
  const PannerOptRow o = d.opts[inst];
  const PannerGeomOut g = panner_geom_frame(v, o);
  const uint64_t at = (uint64_t)inst * d.n_frames + frame;
  d.az[at] = g.az;
  d.gl_mono[at] = g.gl_mono;
  d.gr_mono[at] = g.gr_mono;
  d.gl_stereo[at] = g.gl_stereo;
  d.gr_stereo[at] = g.gr_stereo;
  d.dg[at] = g.dg;
  d.cg[at] = g.cg;
}

void launch_panner_geom(const PannerGeomDesc& d, void* stream) {
  const uint64_t total = (uint64_t)d.rows * d.n_frames;
  if (d.opts)
    hipLaunchKernelGGL(panner_geom_inst_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d);
  else
    hipLaunchKernelGGL(panner_geom_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d);
}

}  // namespace waa
