// waa_compressor.hip — DynamicsCompressorNode (src/node/dynamics_compressor.rs:330-479), node-major in three launches.
//
// Per sample the reference computes
//     xG = lin_to_db(max_c |x_c|)                     (:397-411)   transcendental, no memory
//     xL = xG - gain_computer(xG)                     (:417-425)   three branches, no memory
//     yL = (xL > yL' ? a : r) * yL' + (1 - tau) * xL  (:431-436)   SERIAL, non-linear: the branch depends on the state
//     g  = db_to_lin(makeup - yL)                     (:440-442)   transcendental, no memory
//     out_c[n] = x_c[n - 128 * D] * g[n]              (:452-475)   the look-ahead ring, in absolute time a fixed offset
// Only the third line carries state, and it is four arithmetic instructions; the branch makes it no linear recurrence, so none
// of the scan forms of the Biquad / IIR kernels apply, and with the default release the state forgets a factor 1e-7 only after
// ~190 000 samples, so a warm-up cannot make it time-parallel either.  Hence the split:
//   compressor_level_kernel     parallel over time x context (streaming): x -> xL, one f32 plane per context
//   compressor_detector_kernel  one LANE per context, 64 contexts per wavefront, serial in time: xL -> yL in place
//   compressor_apply_kernel     parallel (streaming): yL, delayed x -> out
//   compressor_meter_kernel     only for a node with the meter on: reduction() after every quantum (:304-306), a gather out of yL
// The block constants (shifted threshold, knee_partial, the taus, the make-up gain) come from the host, per quantum (CompRow).
//
// Arithmetic.  The file is compiled like the rest of the library with -ffp-contract=off (Rust never fuses a * b + c) and
// -fgpu-flush-denormals-to-zero: the kernels run with f32 denormals FLUSHED, inputs and results, which is the mode the
// reference renders in (FTZ + DAZ, src/render/thread.rs:374-382); the detector's release tail therefore dies to an exact zero
// as it does there.  Every f32 operation is written in the reference's order; divisions are IEEE (__fdiv_rn).  The two libm
// calls per sample — log10f in lin_to_db, powf(10, .) in db_to_lin — are evaluated in f64 and rounded once to f32: that is
// the correctly rounded f32 result except in the rare double-rounding case, i.e. what a good host libm returns, and it keeps
// the device's own error out of a value the detector feeds back for thousands of samples.  f64 does not flush.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "waa_internal.hpp"

namespace waa {

namespace {

// (D: CompDesc, or the meter's CompMeterDesc — the same four fields)
template <class D>
__device__ __forceinline__ const CompRow* comp_row(const D& d, uint32_t inst, uint64_t frame) {
  const uint32_t q = min((uint32_t)(frame / RQ), d.n_quanta - 1u);
  return d.rows + (uint64_t)inst * d.row_inst_stride + (uint64_t)q * d.row_q_stride;
}

// 4 consecutive frames of one channel; frames at or past `valid` are silence
__device__ __forceinline__ float4 comp_read4(const float* ch, uint64_t f0, uint64_t valid) {
  if (f0 + 4 <= valid) return *reinterpret_cast<const float4*>(ch + f0);
  float r[4];
#pragma unroll
  for (int e = 0; e < 4; e++) r[e] = f0 + e < valid ? ch[f0 + e] : 0.f;
  return make_float4(r[0], r[1], r[2], r[3]);
}

// dynamics_compressor.rs:21-27 under DAZ: a denormal sample IS zero
__device__ __forceinline__ float comp_lin_to_db(float v) {
  if (v == 0.f || fabsf(v) < FLT_MIN) return -1000.f;
  return __fmul_rn(20.f, (float)log10((double)v));
}

// :400-425: level of one frame in dB -> attenuation xL.  The middle branch is SELECTED, never blended: with knee = 0 the
// host's knee_partial is +-inf or NaN (0 / 0 when ratio = 1) and the branch is unreachable (lo == hi == thr).
__device__ __forceinline__ float comp_attenuation(float mx, const CompRow& r) {
  const float db = comp_lin_to_db(mx);
  float att;
  if (db <= r.lo) {
    att = db;
  } else if (db <= r.hi) {
    const float t = __fadd_rn(__fsub_rn(db, r.thr), r.half_knee);
    att = __fadd_rn(db, __fmul_rn(__fmul_rn(t, t), r.knee_partial));
  } else {
    att = __fadd_rn(r.thr, __fdiv_rn(__fsub_rn(db, r.thr), r.ratio));
  }
  return __fsub_rn(db, att);
}

// :400-407: `max` starts at f32::MIN and only a sample that compares greater replaces it (a NaN never does)
__device__ __forceinline__ float comp_max(float mx, float s) {
  s = fabsf(s);
  return s > mx ? s : mx;
}

}  // namespace

// ---- level: x -> xL --------------------------------------------------------------------------------------------------
// grid (frames / 1024, n_inst), 256 threads, 4 frames per thread: 16-byte loads and stores, a wavefront covers 1 KB per plane.
__global__ __launch_bounds__(256) void compressor_level_kernel(const CompDesc d) {
  const uint32_t inst = blockIdx.y;
  const uint64_t f0 = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (f0 >= (uint64_t)d.n_quanta * RQ) return;
  const float* in = d.in.base + (uint64_t)inst * d.in.inst_stride;
  const CompRow row = *comp_row(d, inst, f0);
  const float4 a = comp_read4(in, f0, d.in_valid);
  float m[4] = {-FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX};
  m[0] = comp_max(m[0], a.x);
  m[1] = comp_max(m[1], a.y);
  m[2] = comp_max(m[2], a.z);
  m[3] = comp_max(m[3], a.w);
  if (d.nch == 2) {
    const float4 c = comp_read4(in + d.in.ch_stride, f0, d.in_valid);
    m[0] = comp_max(m[0], c.x);
    m[1] = comp_max(m[1], c.y);
    m[2] = comp_max(m[2], c.z);
    m[3] = comp_max(m[3], c.w);
  }
  float4 o;
  o.x = comp_attenuation(m[0], row);
  o.y = comp_attenuation(m[1], row);
  o.z = comp_attenuation(m[2], row);
  o.w = comp_attenuation(m[3], row);
  *reinterpret_cast<float4*>(d.xl + (uint64_t)inst * d.frames + f0) = o;
}

// ---- detector: xL -> yL, in place ------------------------------------------------------------------------------------
// One wavefront per 64 contexts, lane = context.  Time is walked in chunks of 64 frames (half a render quantum: one CompRow):
//   - the chunk of all 64 contexts (64 rows x 256 B) is fetched with 16-byte loads, 16 lanes per row = whole 256-byte runs,
//     and turned in LDS (row pitch 65 words: the lane-per-row walk below and the 4-word column writes are conflict free);
//   - the NEXT chunk's loads are issued before the serial walk and land while it runs (64 VGPRs);
//   - the walk reads 16 values at a time into registers, so that nothing but the recurrence itself is on the dependent chain:
//     compare, two selects, one multiply, one add per frame — (1 - tau) * xL is computed beside it (the compiler selects
//     1 - tau first and multiplies once: the same product, 6 VALU instructions per frame in all);
//   - yL goes back through LDS and out with 16-byte stores.
// SHARED: every context has the same row -> one wave-uniform 16-byte load of the taus per chunk (the compiler keeps it a vector
// load: the kernel also stores to global memory); else one row per lane.
// State: one float per lane, in a register for the whole render (the launch covers all of it: nothing to carry, nothing to
// reset between renders).  No scratch, no spills (tests/test_compressor.py reads the ISA).
constexpr int COMP_CHUNK = 64;
constexpr int COMP_PITCH = COMP_CHUNK + 1;

template <bool SHARED>
__global__ __launch_bounds__(64) void compressor_detector_kernel(const CompDesc d) {
  __shared__ float tile[64 * COMP_PITCH];
  const int lane = (int)threadIdx.x;
  const uint32_t inst0 = blockIdx.x * 64u;
  const uint32_t inst = min(inst0 + (uint32_t)lane, d.n_inst - 1u);  // (idle lanes shadow the last context)
  const int c4 = lane & 15, r0 = lane >> 4;  // transfer role: 16-byte column c4 of rows r0, r0 + 4, ...
  const uint64_t total = (uint64_t)d.n_quanta * RQ;
  float4 pre[16];
  auto fetch = [&](uint64_t n0) {
#pragma unroll
    for (int k = 0; k < 16; k++) {
      // (rows past the batch shadow its last context, like the idle lanes: an unconditional load keeps the load counter exact,
      // so that the walk can leave these sixteen in flight)
      const uint32_t r = min(inst0 + (uint32_t)(r0 + 4 * k), d.n_inst - 1u);
      pre[k] = *reinterpret_cast<const float4*>(d.xl + (uint64_t)r * d.frames + n0 + 4 * c4);
    }
  };
  fetch(0);
  float y = 0.f;  // prev_detector_value (:267)
  float* mine = tile + lane * COMP_PITCH;
  auto chunk = [&](uint64_t n0) {
#pragma unroll
    for (int k = 0; k < 16; k++) {
      float* w = tile + (r0 + 4 * k) * COMP_PITCH + 4 * c4;
      w[0] = pre[k].x;
      w[1] = pre[k].y;
      w[2] = pre[k].z;
      w[3] = pre[k].w;
    }
    __syncthreads();
    // (the taus are loaded BEFORE the next chunk's loads are issued: the load counter is in order, so the walk below waits for
    // this one load and leaves the sixteen behind it in flight)
    const float4 tau = *reinterpret_cast<const float4*>(&comp_row(d, SHARED ? 0u : inst, n0)->a_tau);
    const float a_tau = tau.x, a_one = tau.y, r_tau = tau.z, r_one = tau.w;
    fetch(min(n0 + COMP_CHUNK, total - COMP_CHUNK));  // (unconditional for the same reason; the last chunk fetches itself again, unused)
#pragma unroll 1
    for (int tb = 0; tb < COMP_CHUNK; tb += 16) {
      float v[16];
#pragma unroll
      for (int j = 0; j < 16; j++) v[j] = mine[tb + j];
#pragma unroll
      for (int j = 0; j < 16; j++) {
        const float pa = __fmul_rn(a_one, v[j]), pr = __fmul_rn(r_one, v[j]);  // off the chain
        const bool attack = v[j] > y;                                          // :431 (false for a NaN: release)
        y = __fadd_rn(__fmul_rn(attack ? a_tau : r_tau, y), attack ? pa : pr);  // :432 / :435
        v[j] = y;
      }
#pragma unroll
      for (int j = 0; j < 16; j++) mine[tb + j] = v[j];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; k++) {
      // (unconditional as well: a row past the batch holds the last context's yL — same input, same constants, same bits — and
      // writes them where the last context's own row does; with no branch here the next chunk's wait counts these stores and
      // does not wait for them)
      const uint32_t r = min(inst0 + (uint32_t)(r0 + 4 * k), d.n_inst - 1u);
      const float* w = tile + (r0 + 4 * k) * COMP_PITCH + 4 * c4;
      *reinterpret_cast<float4*>(d.xl + (uint64_t)r * d.frames + n0 + 4 * c4) = make_float4(w[0], w[1], w[2], w[3]);
    }
    __syncthreads();
  };
  // The first chunk is peeled so that every pass through the loop — the first included — arrives with sixteen loads and, behind
  // them, sixteen stores in flight: the wait in front of the LDS stage is then for the loads alone (vmcnt(16)), and the stores of
  // chunk k drain under the walk of chunk k + 1.  (A render has at least one quantum = two chunks.)
  chunk(0);
  for (uint64_t n0 = COMP_CHUNK; n0 < total; n0 += COMP_CHUNK) chunk(n0);
}

// ---- apply: out_c[n] = x_c[n - delay] * db_to_lin(makeup - yL[n]) ----------------------------------------------------
// Same shape as the level kernel.  Frames in front of the look-ahead are the ring's initial silence: exact zeros, like the
// reference's silent quantum (:463-468); frames past the render are zeros like every signal's padding.
__global__ __launch_bounds__(256) void compressor_apply_kernel(const CompDesc d) {
  const uint32_t inst = blockIdx.y;
  const uint64_t f0 = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (f0 >= d.frames) return;
  float* out = d.out.base + (uint64_t)inst * d.out.inst_stride;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  if (f0 < d.delay_frames || f0 >= (uint64_t)d.n_quanta * RQ) {
    for (int c = 0; c < d.nch; c++) *reinterpret_cast<float4*>(out + (uint64_t)c * d.out.ch_stride + f0) = zero;
    return;
  }
  const float makeup = comp_row(d, inst, f0)->makeup;
  const float4 yl = *reinterpret_cast<const float4*>(d.xl + (uint64_t)inst * d.frames + f0);
  float g[4];
  const float ys[4] = {yl.x, yl.y, yl.z, yl.w};
#pragma unroll
  for (int e = 0; e < 4; e++)  // :440-442, db_to_lin (:14-16): 10^(v / 20)
    g[e] = (float)exp10((double)__fdiv_rn(__fadd_rn(-ys[e], makeup), 20.f));
  const float* in = d.in.base + (uint64_t)inst * d.in.inst_stride;
  for (int c = 0; c < d.nch; c++) {
    const float4 x = comp_read4(in + (uint64_t)c * d.in.ch_stride, f0 - d.delay_frames, d.in_valid);
    *reinterpret_cast<float4*>(out + (uint64_t)c * d.out.ch_stride + f0) =
        make_float4(__fmul_rn(x.x, g[0]), __fmul_rn(x.y, g[1]), __fmul_rn(x.z, g[2]), __fmul_rn(x.w, g[3]));
  }
}

// ---- meter: reduction() after every quantum (:304-306) -----------------------------------------------------------------
// The reference stores `-detector_value + makeup_gain` of a quantum's LAST frame when the quantum is done (:440, :450); with the
// detector's yL of every frame still in the plane that is one f32 negation and one f32 add per (context, quantum), in the
// reference's order.  grid (n_quanta / 256, n_inst), one thread per value: a 4-byte read at a 512-byte stride, a dense store.
__global__ __launch_bounds__(256) void compressor_meter_kernel(const CompMeterDesc d) {
  const uint32_t inst = blockIdx.y;
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q >= d.n_quanta) return;
  const uint64_t last = (uint64_t)q * RQ + (RQ - 1);  // (< n_quanta * 128 <= frames)
  const float yl = d.yl[(uint64_t)inst * d.frames + last];
  d.out[(uint64_t)inst * d.n_quanta + q] = __fadd_rn(-yl, comp_row(d, inst, last)->makeup);
}

// level and apply have the instance on gridDim.y: a batch of more instances than a grid has rows goes in slices
template <class L>
static bool comp_sliced(const CompDesc& d, L&& launch) {
  if (d.n_inst <= MAX_GRID_ROWS) return false;
  for_grid_row_slices(d.n_inst, 1, [&](uint32_t first, uint32_t count) {
    CompDesc s = d;
    advance_instances(s.in, first);
    advance_instances(s.out, first);
    advance_instances(s.xl, first, d.frames);
    advance_instances(s.rows, first, d.row_inst_stride);
    s.n_inst = count;
    launch(s);
  });
  return true;
}

void launch_compressor_level(const CompDesc& d, void* stream) {
  if (comp_sliced(d, [&](const CompDesc& s) { launch_compressor_level(s, stream); })) return;
  const dim3 grid((uint32_t)(((uint64_t)d.n_quanta * RQ + 1023) / 1024), d.n_inst), block(256);
  hipLaunchKernelGGL(compressor_level_kernel, grid, block, 0, (hipStream_t)stream, d);
}

void launch_compressor_detector(const CompDesc& d, void* stream) {
  const dim3 grid((d.n_inst + 63) / 64), block(64);
  if (d.row_inst_stride == 0)
    hipLaunchKernelGGL(compressor_detector_kernel<true>, grid, block, 0, (hipStream_t)stream, d);
  else
    hipLaunchKernelGGL(compressor_detector_kernel<false>, grid, block, 0, (hipStream_t)stream, d);
}

void launch_compressor_apply(const CompDesc& d, void* stream) {
  if (comp_sliced(d, [&](const CompDesc& s) { launch_compressor_apply(s, stream); })) return;
  const dim3 grid((uint32_t)((d.frames + 1023) / 1024), d.n_inst), block(256);
  hipLaunchKernelGGL(compressor_apply_kernel, grid, block, 0, (hipStream_t)stream, d);
}

void launch_compressor_meter(const CompMeterDesc& d, void* stream) {
  if (d.n_inst > MAX_GRID_ROWS) {  // (whole contexts per slice, like level and apply)
    for_grid_row_slices(d.n_inst, 1, [&](uint32_t first, uint32_t count) {
      CompMeterDesc s = d;
      advance_instances(s.yl, first, d.frames);
      advance_instances(s.rows, first, d.row_inst_stride);
      advance_instances(s.out, first, d.n_quanta);
      s.n_inst = count;
      launch_compressor_meter(s, stream);
    });
    return;
  }
  const dim3 grid((d.n_quanta + 255) / 256, d.n_inst), block(256);
  hipLaunchKernelGGL(compressor_meter_kernel, grid, block, 0, (hipStream_t)stream, d);
}

}  // namespace waa
