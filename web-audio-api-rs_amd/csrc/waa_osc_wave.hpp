// waa_osc_wave.hpp — the OscillatorNode's device functions (oscillator.rs:505-660): the waveform arithmetic, the store with its
// folded post ops, and the bodies of the serial and the prefix-sum kernel.  Two files instantiate them: waa_osc.hip with one type
// per node (TYPES = false: OscDesc::type / table), waa_osc_types.hip with one type per instance (TYPES = true: a byte per instance,
// OscDesc::type_inst) — one definition of the arithmetic, so a mixed batch equals single-type batches bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include "waa_internal.hpp"

namespace waa {

namespace {
__device__ __forceinline__ double unroll_phase(double phase) {  // oscillator.rs:646-654
  if (phase >= 1.) return phase - 1.;
  if (phase < 0.) return phase + 1.;
  return phase;
}
__device__ __forceinline__ double unroll_phase_unbounded(double phase) {  // rem_euclid(1.), :656-659
  const double r = fmod(phase, 1.);
  return r < 0. ? r + 1. : r;
}
__device__ __forceinline__ double poly_blep(double t, double dt) {  // :626-643 (production path)
  if (t < dt) {
    t /= dt;
    return t + t - t * t - 1.0;
  } else if (t > 1.0 - dt) {
    t = (t - 1.0) / dt;
    return __builtin_fma(t, t, t) + t + 1.0;
  }
  return 0.0;
}
__device__ __forceinline__ float table_sample(const float* table, int len, double phase) {  // :571-586, :604-619
  const double position = phase * (double)len;
  const double floored = floor(position);
  // A phase of exactly 1.0 reads entry 0, not table[len].  The single wrap of unroll_phase returns 1.0 for a phase in
  // [-2^-54, 0) (phase + 1. rounds up), which osc_kernel can reach when |phase + incr| < 2^-54; the reference indexes past
  // its table there and panics, so there is no behaviour to match.  The other two kernels fold ph >= 1 before they call.
  const int prev_index = (int)floored >= len ? 0 : (int)floored;
  int next_index = prev_index + 1;
  if (next_index == len) next_index = 0;
  const float k = (float)(position - floored);
  return __builtin_fmaf(table[prev_index], 1.f - k, table[next_index] * k);
}
__device__ __forceinline__ float waveform_sample(int type, const float* table, int table_len, double phase, double phase_incr) {  // :561-602
  switch (type) {
    case 1: {  // square
      double sample = phase < 0.5 ? 1.0 : -1.0;
      sample += poly_blep(phase, phase_incr);
      sample -= poly_blep(unroll_phase(phase + 0.5), phase_incr);
      return (float)sample;
    }
    case 2: {  // sawtooth
      const double ph = unroll_phase(phase + 0.5);
      double sample = 2.0 * ph - 1.0;
      sample -= poly_blep(ph, phase_incr);
      return (float)sample;
    }
    case 3: {  // triangle
      double sample = -4. * phase + 2.;
      if (sample > 1.)
        sample = 2. - sample;
      else if (sample < -1.)
        sample = -2. - sample;
      return (float)sample;
    }
    default: return table_sample(table, table_len, phase);  // sine (2048) or custom (8192)
  }
}
// the table an instance reads: the node's one table, or (one PeriodicWave per instance, OscDesc::wave_row) the instance's row
__device__ __forceinline__ const float* table_of(const float* table, const uint32_t* wave_row, int table_len, uint32_t inst) {
  return wave_row ? table + (uint64_t)wave_row[inst] * (uint64_t)table_len : table;
}

// what one instance renders with.  TYPES = false: the node's type and table.  TYPES = true: the instance's byte of `type_inst` —
// sine reads `sine_table` (2048 points), custom its row of `table` ([rows][8192], wave_row), the polyBLEP forms no table; a null
// `type_inst` (the other operator of a folded FM pair has the types) is the node's type and table.
constexpr int OSC_TYPE_SINE = 0, OSC_TYPE_CUSTOM = 4;  // WAA_OSC_SINE / WAA_OSC_CUSTOM of waa_hip.h (waveform_sample's cases are the rest)
struct OscWaveRef {
  int type;
  const float* table;
  int len;
};
template <bool TYPES>
__device__ __forceinline__ OscWaveRef osc_wave_ref(const uint8_t* type_inst, const float* sine_table, int type, const float* table,
                                                   const uint32_t* wave_row, int table_len, uint32_t inst) {
  if (TYPES && type_inst) {
    const int t = type_inst[inst];
    if (t == OSC_TYPE_SINE) return OscWaveRef{t, sine_table, 2048};
    if (t == OSC_TYPE_CUSTOM) return OscWaveRef{t, table + (uint64_t)wave_row[inst] * (uint64_t)PERIODIC_WAVE_LEN, PERIODIC_WAVE_LEN};
    return OscWaveRef{t, nullptr, 0};
  }
  return OscWaveRef{type, table_of(table, wave_row, table_len, inst), table_len};
}

// four consecutive frames of the oscillator's output through the folded post ops (OscDesc::post_gain / post_dup)
__device__ __forceinline__ void osc_store(const OscDesc& d, uint32_t inst, float* out, uint64_t f0, float (&r)[4]) {
#pragma unroll
  for (int k = 0; k < 2; k++)
    if (k < d.n_post) {
      const float g = d.post_gain[k].base[inst];
      const bool mute = fabsf(g) <= 1e-6f, pass = fabsf(1.f - g) <= 1e-6f;  // gain.rs:163-179
#pragma unroll
      for (int e = 0; e < 4; e++) r[e] = mute ? 0.f : (pass ? r[e] : r[e] * g);
    }
  if (d.pa_on) {  // AudioParamProcessor::mix_to_output on the way out (OP_PARAM_ADD of the chain kernel, the same arithmetic)
    const uint32_t q = (uint32_t)(f0 / RQ), qc = q < d.n_quanta ? q : d.n_quanta - 1;
    const float iv = d.pa_intrinsic.mode == 0 ? d.pa_intrinsic.base[inst] : d.pa_intrinsic.base[(uint64_t)inst * d.pa_intrinsic.stride + qc];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const float o1 = r[e] + iv;
      r[e] = o1 != o1 ? d.pa_default : fminf(fmaxf(o1, d.pa_min), d.pa_max);
    }
  }
  *reinterpret_cast<float4*>(out + f0) = make_float4(r[0], r[1], r[2], r[3]);
  if (d.post_dup) *reinterpret_cast<float4*>(out + d.out.ch_stride + f0) = make_float4(r[0], r[1], r[2], r[3]);
}

// one frame of the time-parallel form: the phase of frame i of a quantum in closed form (osc_par_kernel's comment), folded to [0, 1)
__device__ __forceinline__ double osc_par_phase(const OscQuantum& oq, int i) {
  const double x = __builtin_fma((double)(i - oq.first), oq.incr, oq.phase);
  double ph = x - floor(x);
  if (ph >= 1.) ph -= 1.;
  return ph;
}

// The serial form (osc_kernel, osc_types_kernel): one LANE renders one instance, frame after frame.
template <bool TYPES>
__device__ __forceinline__ void osc_serial_body(const OscDesc& d) {
  const uint32_t inst = blockIdx.x * 64 + threadIdx.x;
  if (inst >= d.n_inst) return;
  __builtin_amdgcn_s_setreg(1 | (6 << 6) | (1 << 11), 0);
  float* out = d.out.base + (uint64_t)inst * d.out.inst_stride;
  const OscWaveRef w = osc_wave_ref<TYPES>(d.type_inst, d.sine_table, d.type, d.table, d.wave_row, d.table_len, inst);
  double start_time = d.start[inst];
  const double stop_time = d.stop[inst];
  const double sample_rate = d.sample_rate, dt = 1. / sample_rate, nyquist = sample_rate / 2.;
  double phase = 0.;
  bool started = false;
  const bool per_frame = d.frequency.mode == 2 || d.detune.mode == 2;
  for (uint32_t q = 0; q < d.n_quanta; q++) {
    const uint64_t f0 = (uint64_t)q * RQ;
    const double block_time = (double)f0 / sample_rate;
    const double next_block_time = block_time + dt * (double)RQ;
    float4* o4 = reinterpret_cast<float4*>(out + f0);
    if (stop_time <= block_time || start_time >= next_block_time) {  // :349-375
      for (int j = 0; j < RQ / 4; j++) o4[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      continue;
    }
    double current_time = block_time;
    if (!started && start_time < current_time) start_time = current_time;  // :386-393
    // the per-sample body of generate_sample, :505-553
    auto generate = [&](bool outside_nyquist, double phase_incr) __attribute__((always_inline)) -> float {
      float v = 0.f;
      if (!(current_time < start_time || current_time >= stop_time)) {
        if (!started) {
          if (current_time > start_time) {
            const double ratio = (current_time - start_time) / dt;
            phase = outside_nyquist ? unroll_phase_unbounded(phase_incr * ratio) : unroll_phase(phase_incr * ratio);
          }
          started = true;
        }
        v = outside_nyquist ? 0.f : waveform_sample(w.type, w.table, w.len, phase, phase_incr);
        phase = outside_nyquist ? unroll_phase_unbounded(phase + phase_incr) : unroll_phase(phase + phase_incr);
      }
      current_time += dt;
      return v;
    };
    if (!per_frame) {
      const float freq = d.frequency.mode == 0 ? d.frequency.base[inst] : d.frequency.base[(uint64_t)inst * d.frequency.stride + q];
      const float detune = d.detune.mode == 0 ? d.detune.base[inst] : d.detune.base[(uint64_t)inst * d.detune.stride + q];
      const double computed_freq = (double)freq * exp2((double)detune / 1200.);  // :30-32
      const double phase_incr = computed_freq / sample_rate;
      const bool outside_nyquist = fabs(computed_freq) >= nyquist;
      const bool fully_active = started && start_time <= block_time && stop_time >= next_block_time;
      if (fully_active && !outside_nyquist) {
        for (int j = 0; j < RQ / 4; j++) {
          float r[4];
#pragma unroll
          for (int e = 0; e < 4; e++) {
            r[e] = waveform_sample(w.type, w.table, w.len, phase, phase_incr);
            phase = unroll_phase(phase + phase_incr);
          }
          o4[j] = make_float4(r[0], r[1], r[2], r[3]);
        }
      } else {
        for (int j = 0; j < RQ / 4; j++) {
          float r[4];
#pragma unroll
          for (int e = 0; e < 4; e++) r[e] = generate(outside_nyquist, phase_incr);
          o4[j] = make_float4(r[0], r[1], r[2], r[3]);
        }
      }
    } else {
      for (int j = 0; j < RQ / 4; j++) {
        float r[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const uint64_t f = f0 + j * 4 + e;
          const float freq = d.frequency.mode == 0   ? d.frequency.base[inst]
                             : d.frequency.mode == 1 ? d.frequency.base[(uint64_t)inst * d.frequency.stride + q]
                                                     : d.frequency.base[(uint64_t)inst * d.frequency.stride + f];
          const float detune = d.detune.mode == 0   ? d.detune.base[inst]
                               : d.detune.mode == 1 ? d.detune.base[(uint64_t)inst * d.detune.stride + q]
                                                    : d.detune.base[(uint64_t)inst * d.detune.stride + f];
          const double computed_freq = (double)freq * exp2((double)detune / 1200.);
          const double phase_incr = computed_freq / sample_rate;
          r[e] = generate(fabs(computed_freq) >= nyquist, phase_incr);
        }
        o4[j] = make_float4(r[0], r[1], r[2], r[3]);
      }
    }
  }
  // frames past the last quantum of the padded signal
  for (uint64_t f = (uint64_t)d.n_quanta * RQ; f < d.frames; f += 4) *reinterpret_cast<float4*>(out + f) = make_float4(0.f, 0.f, 0.f, 0.f);
}

// The prefix-sum form (osc_scan_kernel, osc_types_scan_kernel): one wavefront per (instance, time segment); see osc_scan_kernel.
template <int PASS, bool TYPES>
__device__ __forceinline__ void osc_scan_body(const OscDesc& d) {
  const uint32_t inst = blockIdx.x;
  const uint32_t seg = blockIdx.y;
  const int lane = threadIdx.x;
  __builtin_amdgcn_s_setreg(1 | (6 << 6) | (1 << 11), 0);
  const OscWaveRef w = osc_wave_ref<TYPES>(d.type_inst, d.sine_table, d.type, d.table, d.wave_row, d.table_len, inst);
  const OscWaveRef fw = osc_wave_ref<TYPES>(d.fm_type_inst, d.fm_sine_table, d.fm_type, d.fm_table, d.fm_wave_row, d.fm_table_len, inst);
  const int64_t first = d.active[(uint64_t)inst * 2], end = d.active[(uint64_t)inst * 2 + 1];
  const double ratio = d.start_ratio[inst];  // (time of frame `first` - start_time) / dt, 0 when it starts on a frame
  const double sample_rate = d.sample_rate, nyquist = sample_rate / 2.;
  const uint64_t groups = (d.frames + 255) / 256, per_seg = (groups + OSC_SEGMENTS - 1) / OSC_SEGMENTS;
  const uint64_t g_begin = (uint64_t)seg * per_seg * 256, g_end = g_begin + per_seg * 256 < d.frames ? g_begin + per_seg * 256 : d.frames;
  double carry = 0.;  // phase at the first frame of the group
  if (PASS == 1) {
    for (uint32_t sgm = 0; sgm < seg; sgm++) {
      carry += d.seg_phase[(uint64_t)inst * OSC_SEGMENTS + sgm];
      carry -= floor(carry);
    }
  }
  // a constant detune: its factor once (the f64 exp2 per frame was most of the group's arithmetic)
  const bool det_const = d.detune.mode == 0;
  const double det_mul = det_const ? exp2((double)d.detune.base[inst] / 1200.) : 1.;
  // TYPES: the single-type kernel is at the limit of its scalar registers and the two OscWaveRefs are eight more.  The AudioParam
  // rows are addressed from a copy of `inst` in a vector register (an empty asm with a "v" constraint: the same value), so their
  // per-instance offsets are not hoisted into scalar registers
  uint32_t pinst = inst;
  if (TYPES) asm("" : "+v"(pinst));
  for (uint64_t g0 = g_begin; g0 < g_end; g0 += 256) {
    const uint64_t f0 = g0 + (uint64_t)lane * 4;
    double incr[4];
    bool outside[4];
    OscQuantum mq4{};
    if (d.fm_q) {
      const uint64_t fq = f0 < (uint64_t)d.n_quanta * RQ ? f0 : (uint64_t)d.n_quanta * RQ - 1;
      mq4 = d.fm_q[(uint64_t)d.fm_row[inst] * d.n_quanta + fq / RQ];
    }
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const uint64_t f = f0 + e;
      const uint64_t fc = f < (uint64_t)d.n_quanta * RQ ? f : (uint64_t)d.n_quanta * RQ - 1;
      const uint32_t q = (uint32_t)(fc / RQ);
      float freq = d.frequency.mode == 0   ? d.frequency.base[pinst]
                   : d.frequency.mode == 1 ? d.frequency.base[(uint64_t)pinst * d.frequency.stride + q]
                                           : d.frequency.base[(uint64_t)pinst * d.frequency.stride + fc];
      if (d.fm_q) {
        // the folded modulator (osc_par_kernel's arithmetic for frame fc), the edge gain (gain.rs:163-179), then mix_to_output
        const OscQuantum& mq = mq4;  // (the four frames of a lane lie in one render quantum)
        const int i = (int)(fc % RQ);
        float m = 0.f;
        if (i >= mq.first && i < mq.end && !mq.outside_nyquist) {
          const double x = __builtin_fma((double)(i - mq.first), mq.incr, mq.phase);
          double ph = x - floor(x);
          if (ph >= 1.) ph -= 1.;
          m = waveform_sample(fw.type, fw.table, fw.len, ph, mq.incr);
        }
        if (d.fm_has_gain) {
          const float g = d.fm_gain.mode == 0 ? d.fm_gain.base[pinst] : d.fm_gain.base[(uint64_t)pinst * d.fm_gain.stride + q];
          m = fabsf(g) <= 1e-6f ? 0.f : (fabsf(1.f - g) <= 1e-6f ? m : m * g);
        }
        float o1 = m + freq;
        freq = o1 != o1 ? d.fm_default : fminf(fmaxf(o1, d.fm_min), d.fm_max);
      }
      double computed_freq;
      if (det_const) {
        computed_freq = (double)freq * det_mul;
      } else {
        const float detune = d.detune.mode == 1 ? d.detune.base[(uint64_t)pinst * d.detune.stride + q]
                                                : d.detune.base[(uint64_t)pinst * d.detune.stride + fc];
        computed_freq = (double)freq * exp2((double)detune / 1200.);
      }
      incr[e] = computed_freq / sample_rate;
      outside[e] = fabs(computed_freq) >= nyquist;
    }
    // contribution of each frame to the phase of LATER frames: inactive frames do not advance the phase
    double adv[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const int64_t f = (int64_t)(f0 + e);
      adv[e] = (f >= first && f < end) ? incr[e] : 0.;
      if (f == first) adv[e] += incr[e] * ratio;  // sub-sample start: the first frame starts at incr * ratio (:516-528)
    }
    const double local = ((adv[0] + adv[1]) + adv[2]) + adv[3];
    double incl = local;  // inclusive scan over lanes
#pragma unroll
    for (int sft = 1; sft < 64; sft <<= 1) {
      const double t = __shfl_up(incl, sft, 64);
      if (lane >= sft) incl += t;
    }
    if (PASS == 1) {
      double ph = carry + (incl - local);  // phase before this lane's first frame (may exceed 1: reduced per frame)
      float r[4];
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const int64_t f = (int64_t)(f0 + e);
        double p = ph;
        if (f == first) p += incr[e] * ratio;
        p -= floor(p);
        if (p >= 1.) p -= 1.;
        r[e] = (f >= first && f < end && !outside[e]) ? waveform_sample(w.type, w.table, w.len, p, incr[e]) : 0.f;
        ph += adv[e];
      }
      osc_store(d, pinst, d.out.base + (uint64_t)pinst * d.out.inst_stride, f0, r);
    }
    double total = __shfl(incl, 63, 64) + carry;
    total -= floor(total);
    carry = total;
  }
  if (PASS == 0 && lane == 0) d.seg_phase[(uint64_t)inst * OSC_SEGMENTS + seg] = carry;
}
}  // namespace

}  // namespace waa
