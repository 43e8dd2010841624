// waa_osc.hip — OscillatorNode (src/node/oscillator.rs:323-660) as an on-device source.
// The oscillator is a serial f64 phase accumulator with a conditional wrap per sample (`unroll_phase`), so its
// samples cannot be produced out of order without changing the rounding.  One LANE renders one instance, frame
// after frame, with the reference's arithmetic (table interpolation in f32 with mul_add, polyBLEP in f64,
// computed frequency in f64); 1024 contexts are 16 wavefronts.  Frequency and detune come as ParamRefs, so
// automation blocks and audio-rate modulation from the graph (FM) are the same code path.
// Latency-bound (about 100 cycles per frame and lane); stores are packed to 16 B per lane.
// The device functions — the waveform arithmetic, the store, the bodies of the serial and the prefix-sum kernel — are in
// waa_osc_wave.hpp, shared with the kernels of a node with one type per instance (waa_osc_types.hip).
#include <hip/hip_runtime.h>

#include "waa_internal.hpp"
#include "waa_osc_wave.hpp"

namespace waa {

__global__ __launch_bounds__(64) void osc_kernel(const OscDesc d) { osc_serial_body<false>(d); }

// Time-parallel variant for host-known frequencies (constants or one value per quantum, no graph modulation):
// the host replays the scheduling decisions of the reference per quantum (start/stop inside a quantum, sub-sample
// start phase, Nyquist muting) and hands over the phase at the first active frame of every quantum; inside the
// quantum the phase is phase + i * incr in closed form instead of i rounded additions.  The two differ by the
// accumulated rounding of the reference's running sum (~1e-14 after 10 s), far below one f32 ulp of the output;
// the waveform arithmetic is the reference's.  HBM-bound: 4 B written per frame.
__global__ __launch_bounds__(256) void osc_par_kernel(const OscDesc d) {
  const uint32_t inst = blockIdx.y;
  const uint64_t f0 = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (f0 >= d.frames) return;
  __builtin_amdgcn_s_setreg(1 | (6 << 6) | (1 << 11), 0);
  float* out = d.out.base + (uint64_t)inst * d.out.inst_stride;
  const float* table = table_of(d.table, d.wave_row, d.table_len, inst);
  const uint32_t q = (uint32_t)(f0 / RQ);
  float r[4] = {0.f, 0.f, 0.f, 0.f};
  if (q < d.n_quanta) {
    const OscQuantum oq = d.table_q[(uint64_t)d.tq_row[inst] * d.n_quanta + q];
    const int i0 = (int)(f0 % RQ);
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const int i = i0 + e;
      if (i >= oq.first && i < oq.end && !oq.outside_nyquist) {
        const double x = __builtin_fma((double)(i - oq.first), oq.incr, oq.phase);
        double ph = x - floor(x);
        if (ph >= 1.) ph -= 1.;
        r[e] = waveform_sample(d.type, table, d.table_len, ph, oq.incr);
      }
    }
  }
  osc_store(d, inst, out, f0, r);
}

// The time-parallel kernel with one PeriodicWave per instance (OscDesc::wave_row): the same arithmetic, the instance's table staged
// in LDS.  A workgroup of osc_par_kernel writes 4 KB and walks — at 220 Hz, 4.7 periods per 1024 frames — through all 32 KB of its
// table: with ONE table per node that table stays in every cache, with 1024 of them every workgroup pulls its 32 KB through L2
// again.  Here a workgroup stages the table once (8 x 16 B per lane) and renders OSC_LDS_SPAN x 1024 frames from it: 32 KB read per
// 32 KB written.  32 KB of LDS per workgroup: 5 workgroups (20 wavefronts) per CU.
constexpr int OSC_LDS_SPAN = 8;
__global__ __launch_bounds__(256) void osc_par_lds_kernel(const OscDesc d) {
  __shared__ float lds_table[PERIODIC_WAVE_LEN];
  const uint32_t inst = blockIdx.y;
  __builtin_amdgcn_s_setreg(1 | (6 << 6) | (1 << 11), 0);
  const float4* src = reinterpret_cast<const float4*>(d.table + (uint64_t)d.wave_row[inst] * PERIODIC_WAVE_LEN);
#pragma unroll
  for (int k = 0; k < PERIODIC_WAVE_LEN / 4 / 256; k++) reinterpret_cast<float4*>(lds_table)[k * 256 + threadIdx.x] = src[k * 256 + threadIdx.x];
  __syncthreads();
  float* out = d.out.base + (uint64_t)inst * d.out.inst_stride;
  for (int s = 0; s < OSC_LDS_SPAN; s++) {
    const uint64_t f0 = (((uint64_t)blockIdx.x * OSC_LDS_SPAN + s) * 256 + threadIdx.x) * 4;
    if (f0 >= d.frames) break;
    const uint32_t q = (uint32_t)(f0 / RQ);
    float r[4] = {0.f, 0.f, 0.f, 0.f};
    if (q < d.n_quanta) {
      const OscQuantum oq = d.table_q[(uint64_t)d.tq_row[inst] * d.n_quanta + q];
      const int i0 = (int)(f0 % RQ);
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const int i = i0 + e;
        if (i >= oq.first && i < oq.end && !oq.outside_nyquist) {
          const double x = __builtin_fma((double)(i - oq.first), oq.incr, oq.phase);
          double ph = x - floor(x);
          if (ph >= 1.) ph -= 1.;
          r[e] = table_sample(lds_table, PERIODIC_WAVE_LEN, ph);
        }
      }
    }
    osc_store(d, inst, out, f0, r);
  }
}

// a-rate / graph-modulated frequency (FM): the phase is the running sum of per-frame increments.  One wavefront per
// instance walks 256-frame groups: every lane owns 4 consecutive frames (coalesced 16 B accesses), sums its four
// increments, a 6-step wavefront scan gives every lane the sum of everything before it in the group, and the group
// total is carried on (mod 1).  The order of the f64 additions differs from the reference's frame-by-frame sum —
// same ~1e-14 phase difference as the closed form above, far below one f32 ulp of the output; the per-frame
// decisions (active range from the host replay of the reference's clock, Nyquist muting, sub-sample start phase)
// and the waveform arithmetic are the reference's.
// The a-rate oscillator in TIME SEGMENTS: one wavefront per (instance, segment) instead of one per instance — with 1024
// instances that was one wave per SIMD walking 1875 groups of 256 frames one after the other, every exposed latency
// (the frequency signal, the f64 arithmetic, the shuffles of the scan) paid in full.  PASS 0 computes the phase advance
// of every segment (the same increments, no waveform), the render pass starts each segment at the running sum of the
// segments before it.  The phase is a sum either way (the group scan was already a tree): rounding differences of the
// order of 1e-16 in the phase, as between the group-serial form and the reference's frame-serial accumulation.
template <int PASS>
__global__ __launch_bounds__(64) void osc_scan_kernel(const OscDesc d) {
  osc_scan_body<PASS, false>(d);
}

void launch_osc(const OscDesc& d, void* stream) {
  if (d.table_q && d.n_inst > MAX_GRID_ROWS) {
    // the time-parallel kernels (here and in waa_osc_types.hip) have the instance on gridDim.y: slices of a bigger batch, with
    // everything THEY read per instance moved on (the other forms have it on gridDim.x)
    for_grid_row_slices(d.n_inst, 1, [&](uint32_t first, uint32_t count) {
      OscDesc s = d;
      advance_instances(s.out, first);
      advance_instances(s.wave_row, first);
      advance_instances(s.tq_row, first);
      advance_instances(s.type_inst, first);
      for (int k = 0; k < 2; k++) advance_instances(s.post_gain[k].base, first);  // (one value per instance: osc_store)
      advance_instances(s.pa_intrinsic, first);
      s.n_inst = count;
      launch_osc(s, stream);
    });
    return;
  }
  if (d.type_inst || d.fm_type_inst) {  // one type per instance (waa_osc_types.hip)
    // pass 0 of the prefix-sum form computes no waveform of its own: only a folded modulator's types reach it
    if (d.active && !d.fm_type_inst) hipLaunchKernelGGL(osc_scan_kernel<0>, dim3(d.n_inst, OSC_SEGMENTS), dim3(64), 0, (hipStream_t)stream, d);
    launch_osc_types(d, stream);
    return;
  }
  if (d.table_q) {
    if (d.wave_row && !measure_switch("WAA_OSC_NO_LDS_TABLE")) {  // (switch: the A/B of tools/periodic_wave_probe.py; the same bits)
      const uint64_t span = 1024ull * OSC_LDS_SPAN;
      hipLaunchKernelGGL(osc_par_lds_kernel, dim3((unsigned)((d.frames + span - 1) / span), d.n_inst), dim3(256), 0, (hipStream_t)stream, d);
      return;
    }
    hipLaunchKernelGGL(osc_par_kernel, dim3((unsigned)((d.frames + 1023) / 1024), d.n_inst), dim3(256), 0, (hipStream_t)stream, d);
    return;
  }
  if (d.active) {
    hipLaunchKernelGGL(osc_scan_kernel<0>, dim3(d.n_inst, OSC_SEGMENTS), dim3(64), 0, (hipStream_t)stream, d);
    hipLaunchKernelGGL(osc_scan_kernel<1>, dim3(d.n_inst, OSC_SEGMENTS), dim3(64), 0, (hipStream_t)stream, d);
    return;
  }
  hipLaunchKernelGGL(osc_kernel, dim3((d.n_inst + 63) / 64), dim3(64), 0, (hipStream_t)stream, d);
}

}  // namespace waa
