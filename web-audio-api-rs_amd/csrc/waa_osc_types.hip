// waa_osc_types.hip — OscillatorNode with one waveform type per instance (waa_oscillator_set_type_instance; the planner comes
// here only where the resolved types of a batch DIFFER, OscDesc::type_inst).  In the reference every context owns its node and
// calls set_type on it (oscillator.rs:305-330).  The three phase forms of waa_osc.hip with the type read from a byte per
// instance: sine reads the shared 2048-point table, custom the instance's row of the PeriodicWave tables, square / sawtooth /
// triangle no table.  Phase construction, replay tables and the store do not depend on the type, and the waveform functions are
// those of waa_osc.hip (waa_osc_wave.hpp): every instance gets the bits a batch of its type alone would give it.
#include <hip/hip_runtime.h>

#include "waa_internal.hpp"
#include "waa_osc_wave.hpp"

namespace waa {

// The time-parallel form.  A workgroup lies inside one instance (blockIdx.y): the type is a scalar and the branch on it uniform.
// Like osc_par_lds_kernel a workgroup renders OSC_TYPES_SPAN x 1024 frames, so that a custom instance stages its 32 KB row in LDS
// once per 32 KB written.  A sine instance stages the shared 2048-point table (8 KB) the same way: measured against reading it
// through the caches as osc_par_kernel does, 0.89 against 0.99 ms; the polyBLEP forms read nothing.  The LDS is
// dynamic: 32 KB per workgroup when the node has a custom instance (5 workgroups, 20 wavefronts per CU, for the workgroups of every
// type), 8 KB when it has not (20 workgroups fit: the register budget bounds the occupancy, as in osc_par_kernel).
constexpr int OSC_TYPES_SPAN = 8;
template <typename Sample>
__device__ __forceinline__ void osc_types_spans(const OscDesc& d, uint32_t inst, Sample sample) {
  float* out = d.out.base + (uint64_t)inst * d.out.inst_stride;
  for (int s = 0; s < OSC_TYPES_SPAN; s++) {
    const uint64_t f0 = (((uint64_t)blockIdx.x * OSC_TYPES_SPAN + s) * 256 + threadIdx.x) * 4;
    if (f0 >= d.frames) break;
    const uint32_t q = (uint32_t)(f0 / RQ);
    float r[4] = {0.f, 0.f, 0.f, 0.f};
    if (q < d.n_quanta) {
      const OscQuantum oq = d.table_q[(uint64_t)d.tq_row[inst] * d.n_quanta + q];
      const int i0 = (int)(f0 % RQ);
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const int i = i0 + e;
        if (i >= oq.first && i < oq.end && !oq.outside_nyquist) r[e] = sample(osc_par_phase(oq, i), oq.incr);
      }
    }
    osc_store(d, inst, out, f0, r);
  }
}
__global__ __launch_bounds__(256) void osc_types_par_kernel(const OscDesc d) {
  extern __shared__ float lds_table[];  // PERIODIC_WAVE_LEN floats if d.any_custom, else 2048 (launch_osc_types)
  const uint32_t inst = blockIdx.y;
  __builtin_amdgcn_s_setreg(1 | (6 << 6) | (1 << 11), 0);
  const int type = d.type_inst[inst];
  if (type == OSC_TYPE_CUSTOM) {
    const float4* src = reinterpret_cast<const float4*>(d.table + (uint64_t)d.wave_row[inst] * PERIODIC_WAVE_LEN);
#pragma unroll
    for (int k = 0; k < PERIODIC_WAVE_LEN / 4 / 256; k++) reinterpret_cast<float4*>(lds_table)[k * 256 + threadIdx.x] = src[k * 256 + threadIdx.x];
    __syncthreads();
    osc_types_spans(d, inst, [&](double ph, double) { return table_sample(lds_table, PERIODIC_WAVE_LEN, ph); });
  } else if (type == OSC_TYPE_SINE && d.sine_in_lds) {  // (always, but for the A/B switch of launch_osc_types)
    for (int k = threadIdx.x; k < 2048 / 4; k += 256) reinterpret_cast<float4*>(lds_table)[k] = reinterpret_cast<const float4*>(d.sine_table)[k];
    __syncthreads();
    osc_types_spans(d, inst, [&](double ph, double) { return table_sample(lds_table, 2048, ph); });
  } else {
    const float* sine = d.sine_table;
    osc_types_spans(d, inst, [&](double ph, double incr) { return waveform_sample(type, sine, 2048, ph, incr); });
  }
}

// The prefix-sum form: one wavefront per (instance, segment), the type — and a folded modulator's — uniform per wavefront.
template <int PASS>
__global__ __launch_bounds__(64) void osc_types_scan_kernel(const OscDesc d) {
  osc_scan_body<PASS, true>(d);
}

// The serial cross-check form (WAA_OSC_EXACT): a lane per instance, so the switch on the type diverges within a wavefront.
__global__ __launch_bounds__(64) void osc_types_kernel(const OscDesc d) { osc_serial_body<true>(d); }

void launch_osc_types(const OscDesc& d, void* stream) {
  if (d.table_q) {
    const uint64_t span = 1024ull * OSC_TYPES_SPAN;
    OscDesc dd = d;
    // (switch: sine instances read the table through the caches as osc_par_kernel does — the A/B of tools/osc_types_probe.py; the same bits)
    dd.sine_in_lds = measure_switch("WAA_OSC_TYPES_SINE_CACHED") ? 0 : 1;
    const size_t lds = (d.any_custom ? PERIODIC_WAVE_LEN : dd.sine_in_lds ? 2048 : 0) * sizeof(float);
    hipLaunchKernelGGL(osc_types_par_kernel, dim3((unsigned)((d.frames + span - 1) / span), d.n_inst), dim3(256), lds, (hipStream_t)stream, dd);
    return;
  }
  if (d.active) {
    // (pass 0 without a folded modulator's types is launch_osc's osc_scan_kernel<0>: it computes no waveform)
    if (d.fm_type_inst) hipLaunchKernelGGL(osc_types_scan_kernel<0>, dim3(d.n_inst, OSC_SEGMENTS), dim3(64), 0, (hipStream_t)stream, d);
    hipLaunchKernelGGL(osc_types_scan_kernel<1>, dim3(d.n_inst, OSC_SEGMENTS), dim3(64), 0, (hipStream_t)stream, d);
    return;
  }
  hipLaunchKernelGGL(osc_types_kernel, dim3((d.n_inst + 63) / 64), dim3(64), 0, (hipStream_t)stream, d);
}

}  // namespace waa
