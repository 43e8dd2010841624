// waa_quantum.hpp — shared parts of the quantum-serial interpreters (device only, everything __forceinline__): dyn_kernel
// (waa_dyn.hip, exact dynamic channel counts) and loop_kernel (waa_loop.hip, its static-count special case) walk the render
// quanta in order with one wavefront per instance and hand results from item to item through LDS.  One definition each of
//   * the small helpers: the param read, the agent-scope coherent loads, the curve lookup in global memory, M2d / mm2, lds_sync
//     (both kernels, and waa_frozen.hip for the curve);
//   * the Biquad quantum on the whole wavefront (biquad_scan_pass: one pass of two channels x 32 lanes) and on one lane per
//     channel with a coefficient set per frame (biquad_serial_frames);
//   * the DelayReader's position arithmetic (delay_position, delay_prev_next).
// loop_kernel is built from all of them.  dyn_body (waa_dyn.hip) uses the small helpers and still spells the scan (with the
// near-flush guard: biquad_scan_pass<true> is that form) and the reader arithmetic out in its one scope: see its file header.
// The files that include this are built with -ffp-contract=off: every fused multiply-add below is explicit, and the order of
// the floating-point operations is the reference's.
#ifndef WAA_QUANTUM_HPP
#define WAA_QUANTUM_HPP

#include <hip/hip_runtime.h>

#include "waa_internal.hpp"

namespace waa {

// The load_global forms, not param_at (waa_param.hpp) / apply_curve (waa_curve.hpp): those read through generic pointers (flat
// loads, which also count against the LDS counter the hand-overs below wait for); these name the global address space.
__device__ __forceinline__ float param_val(const ParamRef& p, uint32_t inst, uint32_t q, uint64_t frame) {
  if (p.mode == 0) return load_global(p.base + inst);
  if (p.mode == 1) return load_global(p.base + (uint64_t)inst * p.stride + q);
  return load_global(p.base + (uint64_t)inst * p.stride + frame);
}
// what this wave (or another one of the device) stored moments ago, served by L2
__device__ __forceinline__ float coherent_f(const float* p) {
  return __int_as_float(__hip_atomic_load((const WAA_GLOBAL_AS int*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ uint32_t coherent_u(const uint32_t* p) {
  return (uint32_t)__hip_atomic_load((const WAA_GLOBAL_AS int*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// waveshaper.rs:555-573, the curve in global memory
__device__ __forceinline__ float shape_curve(const float* curve, int nn, float input) {
  if (nn == 0) return 0.f;
  const float n = (float)nn;
  const float v = (n - 1.f) / 2.0f * (input + 1.f);
  if (v <= 0.f) return load_global(curve);
  if (v >= n - 1.f) return load_global(curve + nn - 1);
  const float k = floorf(v);
  const float f = v - k;
  const int ki = (int)k;
  return (1.f - f) * load_global(curve + ki) + f * load_global(curve + ki + 1);
}
struct M2d {
  double a, b, c, d;
};
__device__ __forceinline__ M2d mm2(const M2d& x, const M2d& y) {
  M2d r;
  r.a = __builtin_fma(x.a, y.a, x.b * y.c);
  r.b = __builtin_fma(x.a, y.b, x.b * y.d);
  r.c = __builtin_fma(x.c, y.a, x.d * y.c);
  r.d = __builtin_fma(x.c, y.b, x.d * y.d);
  return r;
}

// One workgroup = one wavefront: LDS hand-offs between lanes need program order only (the DS operations of a wave execute
// in order).  __syncthreads() would also drain every outstanding global store (its release fence waits for vmcnt(0)) —
// with four to five of them per filter item and quantum the wave waited for its own output stores a dozen times per quantum.
__device__ __forceinline__ void lds_sync() { __builtin_amdgcn_wave_barrier(); }

// ---- BiquadFilter, one coefficient set for the quantum (constant / k-rate params): the 128-frame recurrence spread over the
// wavefront like the streaming kernel does it (waa_biquad_stream.hip) — 32 lanes per channel, 4 frames per lane:
// zero-state response of the lane's frames, the lanes' true incoming states from a 5-step scan with the uniform
// powers of A = M^4 (M the one-frame transition), then the reference's evaluation order from that state.
// On two lanes the recurrence was a chain of ~640 dependent f64 operations per quantum (85 % of the kernel).
// Denormals: flushed by hardware mode like in the reference's render scope; inf / NaN: `bad`, and the caller redoes the
// quantum serially (the scan assumes linearity).
//
// One pass = two channels.  l: the lane within its channel's 32; (cx1, cx2, cy1, cy2): the channel's incoming state;
// xv: frames 4 l .. 4 l + 3 of the channel's input.  Out: the lane's four output frames, the state behind them (lane 31's
// is the channel's) and `bad`.
//
// NEAR_FLUSH: the scan is linear algebra; the reference flushes y to zero FRAME BY FRAME once it leaves the normal
// range (biquad_filter.rs:881-883).  While a tail decays through the last decades above 2.2e-308 the two differ in WHEN
// the state reaches zero — by a quantum, and the quantum in which the tail ends is the item's silence
// flag in dyn_kernel (fuzz seed 6278: a DelayNode behind it re-mixed its line one quantum early).  With the guard, any state or
// output of this quantum that is non-zero but below 1e-280 is `bad` too.
template <bool NEAR_FLUSH>
__device__ __forceinline__ void biquad_scan_pass(int l, double b0, double b1, double b2, double a1, double a2, double cx1, double cx2, double cy1,
                                                 double cy2, f4v xv, float (&yo)[4], double (&fin)[4], bool& bad) {
  auto tiny = [](double v) { return v != 0. && __builtin_fabs(v) < 1e-280; };
  const double x0 = (double)xv.x, x1 = (double)xv.y, x2 = (double)xv.z, x3 = (double)xv.w;
  double xm1 = __shfl_up(x3, 1, 32), xm2 = __shfl_up(x2, 1, 32);
  if (l == 0) {
    xm1 = cx1;
    xm2 = cx2;
  }
  // zero-state response of the lane's four frames (incoming y state 0, true x history)
  const double w0 = b0 * x0 + b1 * xm1 + b2 * xm2, w1 = b0 * x1 + b1 * x0 + b2 * xm1, w2 = b0 * x2 + b1 * x1 + b2 * x0,
               w3 = b0 * x3 + b1 * x2 + b2 * x1;
  const double z0 = w0, z1 = w1 - a1 * z0, z2 = w2 - a1 * z1 - a2 * z0, z3 = w3 - a1 * z2 - a2 * z1;
  double r1 = z3, r2 = z2;
  M2d P = {-a1, -a2, 1., 0.};
  P = mm2(P, P);
  P = mm2(P, P);  // A = M^4
  if (l == 0) {
    r1 = __builtin_fma(P.a, cy1, __builtin_fma(P.b, cy2, r1));
    r2 = __builtin_fma(P.c, cy1, __builtin_fma(P.d, cy2, r2));
  }
#pragma unroll
  for (int dd = 1; dd < 32; dd <<= 1) {
    const double q1 = __shfl_up(r1, dd, 32), q2 = __shfl_up(r2, dd, 32);
    if (l >= dd) {
      r1 = __builtin_fma(P.a, q1, __builtin_fma(P.b, q2, r1));
      r2 = __builtin_fma(P.c, q1, __builtin_fma(P.d, q2, r2));
    }
    P = mm2(P, P);
  }
  double y1 = __shfl_up(r1, 1, 32), y2 = __shfl_up(r2, 1, 32);
  if (l == 0) {
    y1 = cy1;
    y2 = cy2;
  }
  bad = NEAR_FLUSH && (tiny(y1) || tiny(y2));
  // the reference's evaluation order from the true incoming state (biquad_filter.rs:877-883)
  double p1 = xm1, p2 = xm2;
  const double xs[4] = {x0, x1, x2, x3};
#pragma unroll
  for (int e = 0; e < 4; e++) {
    const double x = xs[e];
    double y = b0 * x + b1 * p1 + b2 * p2 - a1 * y1 - a2 * y2;
    bad |= !(__builtin_fabs(y) <= 1.7976931348623157e308) || (NEAR_FLUSH && tiny(y));  // inf / NaN (, or close to the flush)
    if (!__builtin_isnormal(y)) y = 0.;
    p2 = p1;
    p1 = x;
    y2 = y1;
    y1 = y;
    yo[e] = (float)y;
  }
  fin[0] = p1;
  fin[1] = p2;
  fin[2] = y1;
  fin[3] = y2;
}

// One channel's quantum on one lane, frame by frame in the reference's order (biquad_filter.rs:857-897), frame i with coefficient
// set number first + i * stride of cbase (five doubles each): stride 1 walks per-frame sets (a-rate params, first = the quantum's
// first frame), stride 0 stays on set `first`.  s: the channel's state (x1, x2, y1, y2), row: its 128 frames in LDS, filtered in place.
__device__ __forceinline__ void biquad_serial_frames(double* s, float* row, const double* cbase, uint64_t first, uint64_t stride) {
  double x1 = s[0], x2 = s[1], y1 = s[2], y2 = s[3];
  for (int i = 0; i < RQ; i++) {
    const double* cf = cbase + (first + i * stride) * 5;
    const double x = (double)row[i];
    double y = load_global(cf) * x + load_global(cf + 1) * x1 + load_global(cf + 2) * x2 - load_global(cf + 3) * y1 -
               load_global(cf + 4) * y2;
    if (!__builtin_isnormal(y)) y = 0.;
    x2 = x1;
    x1 = x;
    y2 = y1;
    y1 = y;
    row[i] = (float)y;
  }
  s[0] = x1;
  s[1] = x2;
  s[2] = y1;
  s[3] = y2;
}

// ---- DelayReader::process (delay.rs:515-745) on the writer's line in absolute time: where frame i of the quantum reads
struct DelayPos {
  int64_t pf;  // whole frames relative to the quantum's first frame (negative: the past)
  float k;     // weight of the NEXT sample
};
// delay_s: the delayTime value that holds for frame i (i = 0 for one value per quantum: the caller adds the frame to pf)
__device__ __forceinline__ DelayPos delay_position(double delay_s, int in_cycle, double quantum_duration, double sample_rate, double i) {
  if (in_cycle) delay_s = fmax(delay_s, quantum_duration);  // delay.rs:693-701
  const double position = i - delay_s * sample_rate;
  const double fl = floor(position);
  return {(int64_t)fl, (float)(position - fl)};
}
// the two samples the reader interpolates between, as absolute frames of the line (negative: before the render began)
__device__ __forceinline__ void delay_prev_next(uint64_t f0, uint32_t q, int64_t pf, int in_cycle, int num_quanta, int64_t& prev, int64_t& next) {
  prev = (int64_t)f0 + pf;
  // frame 128 of the newest block wraps to the OLDEST ring block (delay.rs:622-626); a reader that renders
  // before its writer sees, in the slot of the current quantum, the block written ring-capacity quanta ago
  next = prev + 1;
  if (!in_cycle && pf == RQ - 1) next = ((int64_t)q - num_quanta) * RQ;
  if (in_cycle && next >= (int64_t)f0) next -= ((int64_t)num_quanta + 1) * RQ;
}

}  // namespace waa

#endif  // WAA_QUANTUM_HPP
