// waa_abi_nodes.cpp — per-node payloads and AudioParams in the C ABI (include/waa_hip.h): the convolver's impulse responses, the
// WaveShaper's curve, PeriodicWaves, IIR coefficients, param values / automation, and the two frequency-response helpers.
#include "../../include/waa_hip_device.h"
#include "waa_host.hpp"

using namespace waa;
using namespace waa::host;

extern "C" {

// convolver.rs:16-53
static float normalize_buffer(const float* const* ch, uint32_t n_ch, uint64_t len, float sr) {
  const float gain_calibration = 0.00125f, gain_calibration_sample_rate = 44100.f, min_power = 0.000125f;
  float power = 0.f;
  for (uint32_t c = 0; c < n_ch; c++) {
    float s = 0.f;
    for (uint64_t i = 0; i < len; i++) s += ch[c][i] * ch[c][i];
    power += s;
  }
  power = std::sqrt(power / (float)(n_ch * len));
  if (!std::isfinite(power) || std::isnan(power) || power < min_power) power = min_power;
  float scale = 1.f / power;
  scale *= gain_calibration;
  scale *= gain_calibration_sample_rate / sr;
  if (n_ch == 4) scale *= 0.5f;
  return scale;
}

waa_status waa_convolver_set_buffer(waa_batch* b, uint32_t node, const float* const* channels, uint32_t n_ch,
                                    uint64_t frames, float sr) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_CONVOLVER)) || (e = check_unplanned(b))) return e;
  if (sr != b->sr)
    return fail(WAA_ERR_NOT_SUPPORTED,
                "NotSupportedError - sample rate of the convolution buffer must match the audio context");
  if (!(n_ch == 1 || n_ch == 2 || n_ch == 4))
    return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - the convolution buffer must consist of 1, 2 or 4 channels");
  Node& n = b->nodes[node];
  if (n.per_inst_ir()) {
    // one impulse response per instance: `channels` is the table [instance][channel]; normalize_buffer runs per instance over
    // that instance's channels, like the ConvolverNode of every context of the reference
    if (!channels) return fail(WAA_ERR_INVALID_ARGUMENT, "ConvolverNode %u: the table of per-instance impulse responses is NULL", node);
    for (uint32_t i = 0; i < b->n_inst; i++)
      for (uint32_t c = 0; c < n_ch; c++)
        if (!channels[(size_t)i * n_ch + c] && frames)
          return fail(WAA_ERR_INVALID_ARGUMENT, "ConvolverNode %u: the impulse response of instance %u, channel %u is NULL", node, i, c);
    n.ir.clear();
    n.ir_len = frames;
    n.ir_nch = (int)n_ch;
    n.ir_inst.assign((size_t)b->n_inst * n_ch * frames, 0.f);
    for (uint32_t i = 0; i < b->n_inst; i++) {
      const float* const* chs = channels + (size_t)i * n_ch;
      const float scale = n.desc.i[0] ? 1.f : normalize_buffer(chs, n_ch, frames, sr);
      for (uint32_t c = 0; c < n_ch; c++) {
        float* dst = n.ir_inst.data() + ((size_t)i * n_ch + c) * frames;
        for (uint64_t f = 0; f < frames; f++) dst[f] = chs[c][f] * scale;
      }
    }
    n.has_ir = true;
    return WAA_OK;
  }
  const float scale = n.desc.i[0] ? 1.f : normalize_buffer(channels, n_ch, frames, sr);
  n.ir.assign(n_ch, std::vector<float>(frames));
  for (uint32_t c = 0; c < n_ch; c++)
    for (uint64_t i = 0; i < frames; i++) n.ir[c][i] = channels[c][i] * scale;
  n.ir_len = frames;
  n.ir_nch = (int)n_ch;
  n.has_ir = true;
  return WAA_OK;
}

// decode_audio_data_sync + ConvolverNode::set_buffer: the impulse response is decoded and resampled on the device, the
// normalisation (convolver.rs:16-53: a sequential f32 sum, order-dependent) stays where set_buffer does it
waa_status waa_convolver_set_buffer_pcm16(waa_batch* b, uint32_t node, const int16_t* interleaved, uint32_t n_ch, uint64_t frames,
                                          float sr) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_CONVOLVER)) || (e = check_unplanned(b))) return e;
  if (b->nodes[node].per_inst_ir())
    return fail(WAA_ERR_OUT_OF_SCOPE, "ConvolverNode %u takes one impulse response per instance (i[1] = 1): 16-bit responses are out of scope "
                                      "there, decode them and call waa_convolver_set_buffer", node);
  if (!(n_ch == 1 || n_ch == 2 || n_ch == 4))
    return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - the convolution buffer must consist of 1, 2 or 4 channels");
  if ((e = check_sample_rate(sr))) return e;
  if (!b->dry) HIP_TRY(hipSetDevice(b->device));
  float* d = nullptr;
  uint64_t stride = 0, target = 0;
  if ((e = decode_pcm16(b, interleaved, 1, n_ch, frames, sr, &d, &stride, &target))) return e;
  std::vector<std::vector<float>> host(n_ch, std::vector<float>(target));
  std::vector<const float*> ptrs(n_ch);
  for (uint32_t c = 0; c < n_ch; c++) {
    if (target) {
      if (b->dry)
        std::memcpy(host[c].data(), d + (size_t)c * stride, target * sizeof(float));
      else
        HIP_TRY(hipMemcpy(host[c].data(), d + (size_t)c * stride, target * sizeof(float), hipMemcpyDeviceToHost));
    }
    ptrs[c] = host[c].data();
  }
  return waa_convolver_set_buffer(b, node, ptrs.data(), n_ch, target, b->sr);
}

waa_status waa_waveshaper_set_curve(waa_batch* b, uint32_t node, const float* curve, uint32_t nn) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_WAVESHAPER)) || (e = check_unplanned(b))) return e;
  Node& n = b->nodes[node];
  if (n.has_curve) return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - cannot assign curve twice");
  n.curve.assign(curve, curve + nn);
  n.has_curve = true;
  return WAA_OK;
}

// every context of the reference constructs its own WaveShaperNode and sets its own curve (waveshaper.rs:203-217): one curve for one instance
waa_status waa_waveshaper_set_curve_instance(waa_batch* b, uint32_t node, uint32_t inst, const float* curve, uint32_t nn) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_WAVESHAPER)) || (e = check_unplanned(b))) return e;
  if (inst == WAA_ALL_INSTANCES) return waa_waveshaper_set_curve(b, node, curve, nn);
  if (inst >= b->n_inst) return fail(WAA_ERR_INVALID_ARGUMENT, "instance %u out of range (WaveShaperNode %u, %u instances)", inst, node, b->n_inst);
  if (!curve || nn == 0) return fail(WAA_ERR_INVALID_ARGUMENT, "WaveShaperNode %u, instance %u: a curve of its own has at least one point", node, inst);
  Node& n = b->nodes[node];
  if (n.per_inst_curve() && n.curve_inst_set[inst]) return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - cannot assign curve twice");
  if (!n.per_inst_curve()) {
    n.curve_inst.resize(b->n_inst);
    n.curve_inst_set.assign(b->n_inst, 0);
  }
  n.curve_inst[inst].assign(curve, curve + nn);
  n.curve_inst_set[inst] = 1;
  return WAA_OK;
}

// the table of periodic_wave.rs:164-189 on the host: the shared wave's, and what the device's generator is held against
static std::vector<float> host_periodic_wave_table(const float* real, const float* imag, uint32_t nn, bool disable_normalization) {
  const int size = 8192;
  std::vector<float> wavetable(size);
  const float pi_2 = 2.f * 3.14159265358979323846f;
  for (int i = 0; i < size; i++) {
    float sample = 0.f;
    const float phase = pi_2 * (float)i / (float)size;
    for (uint32_t j = 1; j < nn; j++) {
      const float freq = (float)j;
      const float re = real ? real[j] : 0.f, im = imag ? imag[j] : 0.f;
      const float rad = phase * freq;
      const float contrib = re * std::cos(rad) + im * std::sin(rad);
      sample += contrib;
    }
    wavetable[i] = sample;
  }
  if (!disable_normalization) {
    float max = 0.f;
    for (float v : wavetable) max = std::fabs(v) > max ? std::fabs(v) : max;
    if (max > 0.f) {
      const float norm_factor = 1.f / max;
      for (float& v : wavetable) v *= norm_factor;
    }
  }
  return wavetable;
}

static int check_periodic_wave(const float* real, const float* imag, uint32_t nn) {
  if ((!real && !imag) || nn < 2) return fail(WAA_ERR_INVALID_ARGUMENT, "IndexSizeError - `real` and `imag` length should at least 2");
  return 0;
}
static int check_wavetable(const float* table, uint32_t n) {
  if (!table || n != WAA_PERIODIC_WAVE_TABLE_LENGTH)
    return fail(WAA_ERR_INVALID_ARGUMENT, "IndexSizeError - a PeriodicWave table has %d points (got %u)", WAA_PERIODIC_WAVE_TABLE_LENGTH, n);
  return 0;
}

// periodic_wave.rs:88-190 + oscillator.rs:318-321 (control side: the wavetable is generated on the host)
waa_status waa_oscillator_set_periodic_wave(waa_batch* b, uint32_t node, const float* real, const float* imag, uint32_t nn,
                                            int32_t disable_normalization) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_OSCILLATOR)) || (e = check_unplanned(b))) return e;
  if ((e = check_periodic_wave(real, imag, nn))) return e;
  host_periodic_wave_table(real, imag, nn, disable_normalization != 0).swap(b->nodes[node].osc_wave);
  return WAA_OK;
}

// the finished table (oscillator.rs:487-493: what the render side receives)
waa_status waa_oscillator_set_wavetable(waa_batch* b, uint32_t node, const float* table, uint32_t n) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_OSCILLATOR)) || (e = check_unplanned(b))) return e;
  if ((e = check_wavetable(table, n))) return e;
  b->nodes[node].osc_wave.assign(table, table + n);
  return WAA_OK;
}

// every context of the reference builds its own PeriodicWave (periodic_wave.rs:88-190): one wave for one instance.  Only the
// coefficients are kept here; plan_oscillator has the device generate the tables of the distinct sets (waa_periodic_wave.hip)
static int osc_instance_slot(waa_batch* b, uint32_t node, uint32_t inst, Node::OscWave** slot) {
  if (inst >= b->n_inst) return fail(WAA_ERR_INVALID_ARGUMENT, "instance %u out of range (OscillatorNode %u, %u instances)", inst, node, b->n_inst);
  Node& n = b->nodes[node];
  if (!n.per_inst_wave()) n.osc_inst.resize(b->n_inst);
  *slot = &n.osc_inst[inst];
  return 0;
}

waa_status waa_oscillator_set_periodic_wave_instance(waa_batch* b, uint32_t node, uint32_t inst, const float* real, const float* imag,
                                                     uint32_t nn, int32_t disable_normalization) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_OSCILLATOR)) || (e = check_unplanned(b))) return e;
  if (inst == WAA_ALL_INSTANCES) return waa_oscillator_set_periodic_wave(b, node, real, imag, nn, disable_normalization);
  if ((e = check_periodic_wave(real, imag, nn))) return e;
  Node::OscWave* w = nullptr;
  if ((e = osc_instance_slot(b, node, inst, &w))) return e;
  w->table.clear();
  w->real.assign(nn, 0.f);
  w->imag.assign(nn, 0.f);
  if (real) std::copy(real, real + nn, w->real.begin());
  if (imag) std::copy(imag, imag + nn, w->imag.begin());
  w->real[0] = w->imag[0] = 0.f;  // (entry 0 is never read, periodic_wave.rs:170: equal sets compare equal whatever it holds)
  w->no_norm = disable_normalization != 0;
  return WAA_OK;
}

waa_status waa_oscillator_set_wavetable_instance(waa_batch* b, uint32_t node, uint32_t inst, const float* table, uint32_t n) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_OSCILLATOR)) || (e = check_unplanned(b))) return e;
  if (inst == WAA_ALL_INSTANCES) return waa_oscillator_set_wavetable(b, node, table, n);
  if ((e = check_wavetable(table, n))) return e;
  Node::OscWave* w = nullptr;
  if ((e = osc_instance_slot(b, node, inst, &w))) return e;
  w->real.clear();
  w->imag.clear();
  w->table.assign(table, table + n);
  return WAA_OK;
}

// every context of the reference owns its OscillatorNode and calls set_type on it (oscillator.rs:305-330): one built-in type for one
// instance; any number of calls, the last one wins.  An instance with a PeriodicWave of its own stays custom (Node::osc_type_of)
waa_status waa_oscillator_set_type_instance(waa_batch* b, uint32_t node, uint32_t inst, int32_t type) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_OSCILLATOR)) || (e = check_unplanned(b))) return e;
  if (inst != WAA_ALL_INSTANCES && inst >= b->n_inst)
    return fail(WAA_ERR_INVALID_ARGUMENT, "instance %u out of range (OscillatorNode %u, %u instances)", inst, node, b->n_inst);
  if (type < WAA_OSC_SINE || type > WAA_OSC_CUSTOM) return fail(WAA_ERR_INVALID_ARGUMENT, "bad oscillator type");
  if (type == WAA_OSC_CUSTOM) return fail(WAA_ERR_INVALID_STATE, "InvalidStateError: Custom type cannot be set manually");
  Node& n = b->nodes[node];
  if (inst == WAA_ALL_INSTANCES) {
    n.desc.i[0] = type;  // (the shared type: instances with a type or a wave of their own keep it)
    return WAA_OK;
  }
  if (n.osc_inst_type.empty()) n.osc_inst_type.assign(b->n_inst, (int8_t)-1);
  n.osc_inst_type[inst] = (int8_t)type;
  return WAA_OK;
}

// the table an instance renders with: its row of the plan's tables once they exist, the host's table otherwise
waa_status waa_oscillator_get_wavetable(waa_batch* b, uint32_t node, uint32_t inst, float* out, uint32_t n) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_OSCILLATOR))) return e;
  if (inst == WAA_ALL_INSTANCES) inst = 0;
  if (inst >= b->n_inst) return fail(WAA_ERR_INVALID_ARGUMENT, "instance %u out of range (OscillatorNode %u, %u instances)", inst, node, b->n_inst);
  if (!out || n != WAA_PERIODIC_WAVE_TABLE_LENGTH)
    return fail(WAA_ERR_INVALID_ARGUMENT, "IndexSizeError - a PeriodicWave table has %d points (got %u)", WAA_PERIODIC_WAVE_TABLE_LENGTH, n);
  const Node& nd = b->nodes[node];
  if (nd.osc_type_of(inst) != WAA_OSC_CUSTOM)  // (a built-in type, its own or the shared one)
    return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - oscillator %u has no PeriodicWave for instance %u", node, inst);
  if (nd.d_osc_row && b->planned && !b->dry && nd.d_osc_tables) {
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));  // (the generator runs on the batch's stream)
    uint32_t row = 0;
    HIP_TRY(hipMemcpy(&row, nd.d_osc_row + inst, sizeof row, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out, nd.d_osc_tables + (size_t)row * n, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return WAA_OK;
  }
  const Node::OscWave* w = nd.per_inst_wave() && nd.osc_inst[inst].own() ? &nd.osc_inst[inst] : nullptr;
  if (w && w->table.empty()) {
    const std::vector<float> t = host_periodic_wave_table(w->real.data(), w->imag.data(), (uint32_t)w->real.size(), w->no_norm);
    std::copy(t.begin(), t.end(), out);
    return WAA_OK;
  }
  const std::vector<float>& t = w ? w->table : nd.osc_wave;
  if (t.empty()) return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - oscillator %u has no PeriodicWave for instance %u", node, inst);
  std::copy(t.begin(), t.end(), out);
  return WAA_OK;
}

// iir_filter.rs:17-46 (validation) and :273-311 (pad to equal length, normalise by a0)
static int check_iir_coefs(const double* ff, uint32_t nff, const double* fb, uint32_t nfb) {
  if (!ff || nff == 0 || nff > WAA_MAX_IIR_COEFFS)
    return fail(WAA_ERR_NOT_SUPPORTED,
                "NotSupportedError - IIR Filter feedforward coefficients should have length >= 0 and <= %d", WAA_MAX_IIR_COEFFS);
  bool all_zero = true;
  for (uint32_t i = 0; i < nff; i++) all_zero &= ff[i] == 0.;
  if (all_zero) return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - IIR Filter feedforward coefficients cannot be all zeros");
  if (!fb || nfb == 0 || nfb > WAA_MAX_IIR_COEFFS)
    return fail(WAA_ERR_NOT_SUPPORTED,
                "NotSupportedError - IIR Filter feedback coefficients should have length >= 0 and <= %d", WAA_MAX_IIR_COEFFS);
  if (fb[0] == 0.) return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - IIR Filter feedback first coefficient cannot be zero");
  return 0;
}

// iir_filter.rs:282-309: pad to equal length, divide by a0
static void normalise_iir_coefs(const double* ff, uint32_t nff, const double* fb, uint32_t nfb, std::vector<double>& nb,
                                std::vector<double>& na) {
  const uint32_t len = std::max(nff, nfb);
  const double a0 = fb[0];
  nb.assign(len, 0.);
  na.assign(len, 0.);
  for (uint32_t i = 0; i < len; i++) {
    nb[i] = (i < nff ? ff[i] : 0.) / a0;
    na[i] = (i < nfb ? fb[i] : 0.) / a0;
  }
}

waa_status waa_iir_set_coefficients(waa_batch* b, uint32_t node, const double* ff, uint32_t nff, const double* fb,
                                    uint32_t nfb) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_IIR_FILTER)) || (e = check_unplanned(b))) return e;
  if ((e = check_iir_coefs(ff, nff, fb, nfb))) return e;
  Node& n = b->nodes[node];
  normalise_iir_coefs(ff, nff, fb, nfb, n.iir_b, n.iir_a);
  return WAA_OK;
}

// every context of the reference constructs its own IIRFilterNode (iir_filter.rs:163-189): one set for one instance
waa_status waa_iir_set_coefficients_instance(waa_batch* b, uint32_t node, uint32_t inst, const double* ff, uint32_t nff,
                                             const double* fb, uint32_t nfb) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_IIR_FILTER)) || (e = check_unplanned(b))) return e;
  if (inst == WAA_ALL_INSTANCES) return waa_iir_set_coefficients(b, node, ff, nff, fb, nfb);
  if (inst >= b->n_inst) return fail(WAA_ERR_INVALID_ARGUMENT, "instance %u out of range (IIRFilterNode %u, %u instances)", inst, node, b->n_inst);
  if ((e = check_iir_coefs(ff, nff, fb, nfb))) return e;
  Node& n = b->nodes[node];
  if (!n.per_inst_iir()) {
    n.iir_inst_b.resize(b->n_inst);
    n.iir_inst_a.resize(b->n_inst);
  }
  normalise_iir_coefs(ff, nff, fb, nfb, n.iir_inst_b[inst], n.iir_inst_a[inst]);
  return WAA_OK;
}

// every context of the reference owns its BiquadFilterNode and sets its type (biquad_filter.rs:28-373, set_type :901-906): one
// type for one instance; any number of calls, the last one wins
waa_status waa_biquad_set_type_instance(waa_batch* b, uint32_t node, uint32_t inst, int32_t type) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_BIQUAD)) || (e = check_unplanned(b))) return e;
  if (inst != WAA_ALL_INSTANCES && inst >= b->n_inst)
    return fail(WAA_ERR_INVALID_ARGUMENT, "instance %u out of range (BiquadFilterNode %u, %u instances)", inst, node, b->n_inst);
  if (type < 0 || type > 7) return fail(WAA_ERR_INVALID_ARGUMENT, "bad biquad type");
  Node& n = b->nodes[node];
  if (inst == WAA_ALL_INSTANCES) {
    n.desc.i[0] = type;  // (the shared type: instances with a type of their own keep it)
    return WAA_OK;
  }
  if (!n.per_inst_type()) n.biquad_inst_type.assign(b->n_inst, (int8_t)-1);
  n.biquad_inst_type[inst] = (int8_t)type;
  return WAA_OK;
}

// every context of the reference builds its own PannerNode from its own PannerOptions (panner.rs:146-166, setters :545-641): one
// complete set for one instance; any number of calls, the last one wins.  The panning model stays the node's (desc.i[0])
waa_status waa_panner_set_options_instance(waa_batch* b, uint32_t node, uint32_t inst, const waa_panner_options* o) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_PANNER)) || (e = check_unplanned(b))) return e;
  if (inst != WAA_ALL_INSTANCES && inst >= b->n_inst)
    return fail(WAA_ERR_INVALID_ARGUMENT, "instance %u out of range (PannerNode %u, %u instances)", inst, node, b->n_inst);
  if (!o) return fail(WAA_ERR_INVALID_ARGUMENT, "PannerNode %u: null options", node);
  if (o->reserved != 0) return fail(WAA_ERR_INVALID_ARGUMENT, "PannerNode %u: waa_panner_options.reserved is 0, got %d", node, o->reserved);
  if (o->distance_model < WAA_DISTANCE_LINEAR || o->distance_model > WAA_DISTANCE_EXPONENTIAL)
    return fail(WAA_ERR_INVALID_ARGUMENT, "bad distance model");
  if ((e = check_panner_values(o->ref_distance, o->max_distance, o->rolloff_factor, o->cone_outer_gain))) return e;
  Node& n = b->nodes[node];
  if (inst == WAA_ALL_INSTANCES) {  // (the shared set: instances with a set of their own keep it)
    n.desc.i[1] = o->distance_model;
    n.desc.d[0] = o->ref_distance;
    n.desc.d[1] = o->max_distance;
    n.desc.d[2] = o->rolloff_factor;
    n.desc.d[3] = o->cone_inner_angle;
    n.desc.d[4] = o->cone_outer_angle;
    n.desc.d[5] = o->cone_outer_gain;
    return WAA_OK;
  }
  if (n.panner_inst_set.empty()) {
    n.panner_inst_opt.assign(b->n_inst, waa_panner_options{});
    n.panner_inst_set.assign(b->n_inst, 0);
  }
  n.panner_inst_opt[inst] = *o;
  n.panner_inst_set[inst] = 1;
  return WAA_OK;
}

// DynamicsCompressorNode::reduction (dynamics_compressor.rs:304-306): what the render thread stored after a quantum (:440, :450).
// The trace of a node with the meter on is on the device after every render ([n_inst][n_quanta], compressor_meter_kernel): both
// getters copy out of it, rows [i0, i1) x quanta [q0, n_quanta), through the batch's pinned staging block if `dst` is pageable.
static int compressor_reduction_rows(waa_batch* b, uint32_t node, uint32_t i0, uint32_t i1, uint32_t q0, float* dst) {
  if (node >= b->nodes.size()) return fail(WAA_ERR_INVALID_ARGUMENT, "node %u out of range", node);
  const Node& n = b->nodes[node];
  if (n.desc.kind != WAA_NODE_DYNAMICS_COMPRESSOR)
    return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - node %u is not a DynamicsCompressorNode: it has no reduction", node);
  if (!n.comp_meter())
    return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - DynamicsCompressorNode %u was created without its meter: waa_node_desc.i[0] = 1 keeps the "
                                       "reduction trace (i[0] is %d)", node, n.desc.i[0]);
  if (b->ranged && b->ctl_q < b->n_quanta)
    return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - DynamicsCompressorNode %u: a ranged render is in progress (suspended in front of quantum %u); the "
                                       "reduction is available once the last range is rendered", node, b->ctl_q);
  if (!b->planned || !b->rendered)
    return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - DynamicsCompressorNode %u: nothing rendered yet, no reduction to read", node);
  if (!dst) return fail(WAA_ERR_INVALID_ARGUMENT, "DynamicsCompressorNode %u: null destination", node);
  const size_t width = (size_t)(b->n_quanta - q0) * sizeof(float), rows = i1 - i0;
  if (!n.d_comp_red) {
    // the node does not reach the destination: it is not rendered, the value is the initial one (:249)
    for (size_t r = 0; r < rows; r++) std::memset((char*)dst + r * width, 0, width);
    return WAA_OK;
  }
  HIP_TRY(hipSetDevice(b->device));
  if (int es = settle_loops(b)) return es;  // (a render that was repeated with settled loop blocks wrote the trace again)
  if (int e = xfer_d2h(b, dst, width, n.d_comp_red + (size_t)i0 * b->n_quanta + q0, (size_t)b->n_quanta * sizeof(float), width, rows)) return e;
  HIP_TRY(hipStreamSynchronize(b->stream));
  return WAA_OK;
}

waa_status waa_compressor_get_reduction(waa_batch* b, uint32_t node, uint32_t inst, float* value) {
  if (!b) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch");
  if (inst >= b->n_inst) return fail(WAA_ERR_INVALID_ARGUMENT, "instance %u out of range (DynamicsCompressorNode %u, %u instances)", inst, node, b->n_inst);
  return compressor_reduction_rows(b, node, inst, inst + 1, b->n_quanta - 1, value);  // (after the LAST rendered quantum)
}

waa_status waa_compressor_get_reduction_series(waa_batch* b, uint32_t node, float* dst, uint32_t n_quanta) {
  if (!b) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch");
  if (n_quanta != b->n_quanta)
    return fail(WAA_ERR_INVALID_ARGUMENT, "DynamicsCompressorNode %u: the reduction trace has one value per render quantum, %u for this batch (got n_quanta = %u)",
                node, b->n_quanta, n_quanta);
  return compressor_reduction_rows(b, node, 0, b->n_inst, 0, dst);
}

// AudioParam::set_value_at_time & co. (param.rs:428-596) on a param of the batch; evaluated at plan time
waa_status waa_param_schedule_event(waa_batch* b, uint32_t node, uint32_t param, uint32_t inst, int32_t type, float value,
                                    double time, double aux, const float* curve, uint32_t n_curve) {
  int e;
  if (!b || node >= b->nodes.size() || param >= b->nodes[node].params.size())
    return fail(WAA_ERR_INVALID_ARGUMENT, "no such param %u on node %u", param, node);
  if ((e = check_inst(b, inst)) || (e = check_unplanned(b))) return e;
  ParamStore& p = b->nodes[node].params[param];
  if (p.timelines.empty()) p.timelines.resize(b->n_inst);
  if (inst != WAA_ALL_INSTANCES) p.timelines_shared = false;
  const auto [lo, hi] = inst_range(inst, b->n_inst);
  for (uint32_t k = lo; k < hi; k++) {
    if (!p.timelines[k]) {
      p.timelines[k] = std::make_shared<Timeline>(p.defv, p.minv, p.maxv, !p.k_rate);
      // the node constructor's `param.set_value(options.x)` (e.g. gain.rs:117)
      if ((e = p.timelines[k]->schedule(WAA_EVENT_SET_VALUE, p.cst[k], 0., 0., nullptr, 0))) return e;
    }
    if ((e = p.timelines[k]->schedule_at(b->ctl_q, type, value, time, aux, curve, n_curve))) return e;
  }
  return WAA_OK;
}

waa_status waa_set_param_const(waa_batch* b, uint32_t node, uint32_t param, uint32_t inst, float value) {
  int e;
  if (!b || node >= b->nodes.size() || param >= b->nodes[node].params.size())
    return fail(WAA_ERR_INVALID_ARGUMENT, "no such param %u on node %u", param, node);
  if ((e = check_inst(b, inst)) || (e = check_unplanned(b))) return e;
  // AudioParam::set_value from a suspend callback: a SetValue event the render thread handles in front of quantum ctl_q
  // (param.rs:386-400, thread.rs:277-294) — through the timeline, which is created (seeded with the constant so far) if the
  // param had none
  if (b->ctl_q > 0) return waa_param_schedule_event(b, node, param, inst, WAA_EVENT_SET_VALUE, value, 0., 0., nullptr, 0);
  ParamStore& p = b->nodes[node].params[param];
  const auto [lo, hi] = inst_range(inst, b->n_inst);
  for (uint32_t k = lo; k < hi; k++) {
    p.cst[k] = value;
    // AudioParam::set_value after automation methods enqueues a SetValue event (param.rs:386-400): a timeline that
    // already exists was seeded with the OLD constant, so the new value has to go through it as well
    if (k < p.timelines.size() && p.timelines[k]) {
      if (inst != WAA_ALL_INSTANCES) p.timelines_shared = false;
      int st = p.timelines[k]->schedule(WAA_EVENT_SET_VALUE, value, 0., 0., nullptr, 0);
      if (st) return st;
    }
  }
  return WAA_OK;
}

waa_status waa_set_param_block(waa_batch* b, uint32_t node, uint32_t param, uint32_t inst, uint64_t q0, uint32_t nq,
                               uint32_t vpq, const float* values) {
  int e;
  if (!b || node >= b->nodes.size() || param >= b->nodes[node].params.size())
    return fail(WAA_ERR_INVALID_ARGUMENT, "no such param %u on node %u", param, node);
  if ((e = check_inst(b, inst)) || (e = check_unplanned(b))) return e;
  if (vpq != 1 && vpq != RQ) return fail(WAA_ERR_INVALID_ARGUMENT, "values_per_quantum must be 1 or 128");
  ParamBlock blk;
  blk.inst = inst;
  blk.q0 = q0;
  blk.nq = nq;
  blk.vpq = vpq;
  blk.v.assign(values, values + (size_t)nq * vpq);
  b->nodes[node].params[param].blocks.push_back(std::move(blk));
  return WAA_OK;
}

// iir_filter.rs:218-262 (control side, host)
waa_status waa_iir_frequency_response(const double* ff, uint32_t nff, const double* fb, uint32_t nfb, float sample_rate,
                                      const float* hz, float* mag, float* phase, uint32_t n) {
  if (int e = check_iir_coefs(ff, nff, fb, nfb)) return e;
  if (n && (!hz || !mag || !phase)) return fail(WAA_ERR_INVALID_ARGUMENT, "null array");
  const double sr = (double)sample_rate, nyquist = sr / 2.;
  for (uint32_t i = 0; i < n; i++) {
    const double freq = (double)hz[i];
    if (freq < 0. || freq > nyquist) {
      mag[i] = std::nanf("");
      phase[i] = std::nanf("");
      continue;
    }
    const double z = -2.0 * 3.14159265358979323846 * freq / sr;
    std::complex<double> num(0., 0.), den(0., 0.);
    for (uint32_t k = 0; k < nff; k++) num += std::complex<double>(ff[k] * std::cos((double)k * z), ff[k] * std::sin((double)k * z));
    for (uint32_t k = 0; k < nfb; k++) den += std::complex<double>(fb[k] * std::cos((double)k * z), fb[k] * std::sin((double)k * z));
    const double ns = den.real() * den.real() + den.imag() * den.imag();
    const double rr = (num.real() * den.real() + num.imag() * den.imag()) / ns;
    const double ri = (num.imag() * den.real() - num.real() * den.imag()) / ns;
    mag[i] = (float)std::hypot(rr, ri);
    phase[i] = (float)std::atan2(ri, rr);
  }
  return WAA_OK;
}

// biquad_filter.rs:670-735 (control side, host)
waa_status waa_biquad_frequency_response(int32_t type, float sample_rate, float frequency, float detune, float q,
                                         float gain, const float* hz, float* mag, float* phase, uint32_t n) {
  if (type < 0 || type > 7) return fail(WAA_ERR_INVALID_ARGUMENT, "bad filter type");
  const double PI = 3.14159265358979323846;
  const float nyq = sample_rate / 2.f;
  const Coefs c = biquad_coefs(type, (double)sample_rate, (double)computed_freq(frequency, detune), (double)gain, (double)q);
  for (uint32_t i = 0; i < n; i++) {
    const float f = hz[i];
    if (f < 0.f || f > nyq) {
      mag[i] = NAN;
      phase[i] = NAN;
      continue;
    }
    const float fn = f / nyq;
    const double omega = -PI * (double)fn;
    const double zr = std::cos(omega), zi = std::sin(omega);
    const double tr = c.b1 + c.b2 * zr, ti = c.b2 * zi;
    const double nr = c.b0 + (tr * zr - ti * zi), ni = tr * zi + ti * zr;
    const double ur = c.a1 + c.a2 * zr, ui = c.a2 * zi;
    const double dr = 1. + (ur * zr - ui * zi), di = ur * zi + ui * zr;
    const double den = dr * dr + di * di;
    const double rr = (nr * dr + ni * di) / den, ri = (ni * dr - nr * di) / den;
    mag[i] = (float)std::hypot(rr, ri);
    phase[i] = (float)std::atan2(ri, rr);
  }
  return WAA_OK;
}

}  // extern "C"
