// waa_host.hpp — host-side data model of libwaa_hip.so shared by the scheduler (waa_schedule.cpp), the planner
// (waa_plan*.cpp), the executor (waa_run.cpp) and the C ABI (waa_abi*.cpp, waa_analyser_host.cpp).  Not part of the public interface (include/waa_hip.h).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cfloat>
#include <cmath>
#include <complex>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <set>
#include <memory>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/waa_hip_device.h"
#include "waa_internal.hpp"

struct waa_batch;

namespace waa {
namespace host {

// last error of the calling thread (waa_last_error); returns `code`
int fail(int code, const char* fmt, ...);
#define HIP_TRY(expr)                                                                           \
  do {                                                                                          \
    hipError_t e_ = (expr);                                                                     \
    if (e_ != hipSuccess) return fail(WAA_ERR_DEVICE, "HIP error %s at %s:%d (%s)", hipGetErrorString(e_), __FILE__, \
                                      __LINE__, #expr);                                         \
  } while (0)

// AudioParam automation timeline (waa_automation.cpp): the reference's AudioParamProcessor on the host
class Timeline {
 public:
  Timeline(float default_value, float min_value, float max_value, bool a_rate);
  ~Timeline();
  // one automation method call (WAA_EVENT_*); returns a waa_status (the reference's panics)
  int schedule(int type, float value, double time, double aux, const float* curve, uint32_t n_curve);
  // the same call made while the render is suspended in front of quantum `arrival_q` (OfflineAudioContext::suspend_sync,
  // offline.rs:359-397): the render thread handles the control message right before it renders that quantum
  // (handle_control_messages, thread.rs:277-294) — the event enters the queue THEN, with the queue as it is then.  Argument
  // errors are reported at once, queue-dependent ones (an event inside a value curve) by apply_arrivals.
  int schedule_at(uint32_t arrival_q, int type, float value, double time, double aux, const float* curve, uint32_t n_curve);
  int apply_arrivals(uint32_t q);  // before compute() of quantum q
  bool has_arrivals() const { return !arrivals_.empty(); }
  // one block: 1 or `count` values into out (capacity >= count); returns how many
  uint32_t compute(double block_time, double dt, uint32_t count, float* out);
  float value() const;  // AudioParam::value()
  // the scheduled queue in the form timeline_kernel replays (waa_timeline.hip); `ev_off` / curve offsets are relative
  // to the arrays the events are appended to
  void export_queue(TlHeader* hdr, std::vector<TlEvent>* events, std::vector<float>* curves) const;

 private:
  struct Event;
  int insert(Event ev);
  float min_, max_, intrinsic_, current_;
  bool a_rate_;
  std::vector<Event> queue_;     // sorted by time (stable)
  std::unique_ptr<Event> last_;  // the last event that was consumed (start point of ramps and targets)
  struct Arrival {
    uint32_t q;
    int type;
    float value;
    double time, aux;
    std::vector<float> curve;
  };
  std::vector<Arrival> arrivals_;  // in call order (arrival quanta never decrease: the control clock only moves forward)
  size_t next_arrival_ = 0;
};

struct ParamBlock {
  uint32_t inst;
  uint64_t q0;
  uint32_t nq, vpq;
  std::vector<float> v;
};
struct ParamStore {
  std::vector<float> cst;
  std::vector<ParamBlock> blocks;
  std::vector<std::shared_ptr<Timeline>> timelines;  // [n_inst] or empty: scheduled automation (waa_param_schedule_event)
  bool k_rate = false;                               // AutomationRate::K (source playbackRate / detune)
  bool timelines_shared = true;                      // every event was scheduled for WAA_ALL_INSTANCES
  bool dev_tl = false;                               // the timelines are replayed on the device (per-instance automation)
  mutable bool dev_ready = false;                    // ... and their step has been planned:
  mutable ParamRef dev_ref{};                        //     per-frame values [n_inst][n_quanta * 128]
  mutable uint8_t* dev_lens = nullptr;               //     slice length per (instance, quantum)
  float defv = 0, minv = -FLT_MAX, maxv = FLT_MAX;
  void init(uint32_t n, float d, float lo, float hi) {
    cst.assign(n, d);
    defv = d;
    minv = lo;
    maxv = hi;
  }
  // AudioParamProcessor::mix_to_output clamp / NaN rule (param.rs:739-797)
  float fix(float x) const { return std::isnan(x) ? defv : std::fmin(std::fmax(x, minv), maxv); }
  int mode() const {
    if (dev_tl) return 2;
    int m = 0;
    for (auto& b : blocks) m = std::max(m, b.vpq == 1 ? 1 : 2);
    return m;
  }
};

// double-double (unevaluated sum hi + lo, ~106 bits) for the IIR transition-matrix powers
struct DD {
  double hi = 0., lo = 0.;
};
inline DD dd_add(DD a, DD b) {
  const double s = a.hi + b.hi, bb = s - a.hi;
  double e = (a.hi - (s - bb)) + (b.hi - bb);
  e += a.lo + b.lo;
  const double hi = s + e;
  return DD{hi, e - (hi - s)};
}
inline DD dd_mul(DD a, DD b) {
  const double p = a.hi * b.hi;
  double e = std::fma(a.hi, b.hi, -p);
  e += a.hi * b.lo + a.lo * b.hi;
  const double hi = p + e;
  return DD{hi, e - (hi - p)};
}

struct DeviceBuffer {  // an AudioBuffer resident in HBM
  float* base = nullptr;  // channel 0
  uint64_t ch_stride = 0;
  uint64_t frames = 0;
  uint32_t nch = 0;
  uint32_t nch_true = 0;  // != 0: the AudioBuffer's own channel count; `nch` is the widened copy's (widen_narrow_buffers)
  float sr = 0;
  bool valid = false;
  uint32_t count() const { return nch_true ? nch_true : nch; }
};
inline DeviceBuffer device_buffer(float* base, uint64_t ch_stride, uint64_t frames, uint32_t nch, float sr) {
  DeviceBuffer db;
  db.base = base;
  db.ch_stride = ch_stride;
  db.frames = frames;
  db.nch = nch;
  db.sr = sr;
  db.valid = true;
  return db;
}

struct SourceSched {  // per instance scheduling parameters
  double start = DBL_MAX, stop = DBL_MAX, offset = 0, duration = DBL_MAX;
  int looping = 0;
  double loop_start = 0, loop_end = 0;
};

struct Node {
  waa_node_desc desc{};
  int cc = 2, mode = WAA_COUNT_MODE_MAX, interp = WAA_INTERP_SPEAKERS;
  std::vector<ParamStore> params;
  // sources
  std::vector<DeviceBuffer> bufs;   // [n_inst]
  std::vector<SourceSched> sched;   // [n_inst]
  // convolver
  std::vector<std::vector<float>> ir;  // host copy, scaled
  uint64_t ir_len = 0;
  int ir_nch = 0;
  bool has_ir = false;
  // one impulse response per instance (desc.i[1] = 1): host copy, scaled per instance, flat [inst][ch][frame] with ir_nch channels
  // of ir_len frames each; `ir` stays empty then (it is the shared response's storage)
  std::vector<float> ir_inst;
  bool per_inst_ir() const { return desc.kind == WAA_NODE_CONVOLVER && desc.i[1] == 1; }
  const float* ir_of(uint32_t inst, int ch) const { return ir_inst.data() + ((size_t)inst * (size_t)ir_nch + (size_t)ch) * ir_len; }
  // the impulse response with the transfer function of the Biquad in front folded in (conv_fold_biquad_into_ir); empty = not folded
  std::vector<std::vector<float>> ir_lti;
  uint64_t ir_lti_len = 0;
  // waveshaper
  std::vector<float> curve;
  bool has_curve = false;
  float* d_curve = nullptr;
  // one curve per instance (waa_waveshaper_set_curve_instance): [n_inst] once the first instance has its own curve; an instance
  // whose flag is clear uses `curve` if the node has one (has_curve) and passes its input through otherwise
  std::vector<std::vector<float>> curve_inst;
  std::vector<uint8_t> curve_inst_set;
  bool per_inst_curve() const { return !curve_inst_set.empty(); }
  // the curve `inst` renders with; nullptr: none (waveshaper.rs:402: the input is copied)
  const std::vector<float>* curve_of(uint32_t inst) const {
    if (per_inst_curve() && curve_inst_set[inst]) return &curve_inst[inst];
    return has_curve ? &curve : nullptr;
  }
  // oscillator: custom PeriodicWave table (8192 points, periodic_wave.rs:76)
  std::vector<float> osc_wave;
  // one PeriodicWave per instance (waa_oscillator_set_periodic_wave_instance / _set_wavetable_instance): [n_inst] once the first
  // instance has its own wave.  An instance holds coefficients (the plan generates its table on the device) or a finished table;
  // one with neither uses osc_wave.  d_osc_tables / d_osc_row: the plan's [rows][8192] tables and the [n_inst] row index, made once
  struct OscWave {
    std::vector<float> real, imag, table;  // real / imag of equal length (a missing one is zeros), or the 8192-point table
    bool no_norm = false;
    bool own() const { return !real.empty() || !table.empty(); }
  };
  std::vector<OscWave> osc_inst;
  bool per_inst_wave() const { return !osc_inst.empty(); }
  float* d_osc_tables = nullptr;
  uint32_t* d_osc_row = nullptr;
  uint32_t osc_rows = 0, osc_gen_rows = 0;
  // one built-in type per instance (waa_oscillator_set_type_instance): [n_inst] once the first instance has its own type, -1 = none.
  // osc_type_of: the type an instance renders with (the order of waa_hip_device.h): its own wave, its own type, the shared wave,
  // -1 where the node has per-instance waves and this instance nothing (build_plan refuses), else the shared type (desc.i[0])
  std::vector<int8_t> osc_inst_type;
  int osc_type_of(uint32_t inst) const {
    if (per_inst_wave() && osc_inst[inst].own()) return WAA_OSC_CUSTOM;
    if (!osc_inst_type.empty() && osc_inst_type[inst] >= 0) return osc_inst_type[inst];
    if (!osc_wave.empty()) return WAA_OSC_CUSTOM;
    if (per_inst_wave()) return -1;
    return desc.i[0];
  }
  // iir filter: normalised coefficient pairs (iir_filter.rs:273-311)
  std::vector<double> iir_b, iir_a;
  // one set per instance (waa_iir_set_coefficients_instance): [n_inst] once the first instance has its own set, normalised like
  // the shared pair; an empty entry = that instance uses iir_b / iir_a
  std::vector<std::vector<double>> iir_inst_b, iir_inst_a;
  bool per_inst_iir() const { return !iir_inst_b.empty(); }
  const std::vector<double>& iir_b_of(uint32_t inst) const { return per_inst_iir() && !iir_inst_b[inst].empty() ? iir_inst_b[inst] : iir_b; }
  const std::vector<double>& iir_a_of(uint32_t inst) const { return per_inst_iir() && !iir_inst_b[inst].empty() ? iir_inst_a[inst] : iir_a; }
  // biquad filter: one type per instance (waa_biquad_set_type_instance): [n_inst] once the first instance has its own type,
  // -1 = that instance uses the shared one (desc.i[0]).  The planner asks types_differ(): a node whose instances all resolve to
  // one type plans exactly as a shared node of that type (biquad_shared_type).
  std::vector<int8_t> biquad_inst_type;
  bool per_inst_type() const { return !biquad_inst_type.empty(); }
  int biquad_type_of(uint32_t inst) const { return per_inst_type() && biquad_inst_type[inst] >= 0 ? biquad_inst_type[inst] : desc.i[0]; }
  bool biquad_types_differ() const {
    for (size_t i = 1; i < biquad_inst_type.size(); i++)
      if (biquad_type_of((uint32_t)i) != biquad_type_of(0)) return true;
    return false;
  }
  int biquad_shared_type() const { return per_inst_type() ? biquad_type_of(0) : desc.i[0]; }  // (only where !biquad_types_differ())
  // panner: one option set per instance (waa_panner_set_options_instance): [n_inst] once the first instance has its own set; an
  // instance whose flag is clear uses the shared one (desc.i[1], desc.d[0..5]).  The planner asks panner_options_differ(): a node
  // whose instances all resolve to one set plans exactly as a shared node of that set.
  std::vector<waa_panner_options> panner_inst_opt;
  std::vector<uint8_t> panner_inst_set;
  waa_panner_options panner_options_of(uint32_t inst) const {
    if (!panner_inst_set.empty() && panner_inst_set[inst]) return panner_inst_opt[inst];
    return waa_panner_options{desc.i[1], 0, desc.d[0], desc.d[1], desc.d[2], desc.d[3], desc.d[4], desc.d[5]};
  }
  bool panner_options_differ() const {
    if (panner_inst_set.empty()) return false;
    const waa_panner_options first = panner_options_of(0);  // (no padding: eight 8-byte-aligned fields in 56 bytes)
    for (size_t i = 1; i < panner_inst_set.size(); i++) {
      const waa_panner_options o = panner_options_of((uint32_t)i);
      if (std::memcmp(&o, &first, sizeof o) != 0) return true;
    }
    return false;
  }
  // analyser (control side state): the pulls of ALL instances are computed by one launch and cached until the next render
  // (current_time after an offline render never changes: repeated pulls return the same data, analysis.rs:354-357)
  struct AnBatch {
    bool computed = false;              // device results are current
    bool have_db = false, have_bytes = false, have_time = false;  // ... and downloaded
    std::vector<float> db, time;        // [n_inst][fft_size / 2], [n_inst][fft_size]
    std::vector<uint8_t> bytes;         // [n_inst][fft_size / 2]
    // a series node (desc.i[1] > 0): which kinds of the series the device buffers below hold for the current render (the rows
    // stay on the device — a series is as large as the render's output — and every getter call copies from there)
    bool s_db = false, s_bytes = false, s_time = false, s_tbytes = false;
  } an;
  // series buffers, allocated when a kind is first pulled: [n_inst][P][fft_size / 2] dB and bytes, [n_inst][P][fft_size] time domain
  float *d_ans_db = nullptr, *d_ans_time = nullptr;
  uint8_t *d_ans_bytes = nullptr, *d_ans_tbytes = nullptr;
  bool an_series() const { return desc.kind == WAA_NODE_ANALYSER && desc.i[1] > 0; }
  // pulls at q_k = i[2] + k * i[1] <= n_quanta
  uint32_t an_series_pulls(uint32_t n_quanta) const {
    return an_series() && desc.i[2] >= 0 && (uint32_t)desc.i[2] <= n_quanta ? (n_quanta - (uint32_t)desc.i[2]) / (uint32_t)desc.i[1] + 1 : 0;
  }
  // DynamicsCompressorNode with the meter on (desc.i[0] = 1): reduction() after every quantum, [n_inst][n_quanta] on the device,
  // allocated by plan_compressor and written by every render (compressor_meter_kernel)
  float* d_comp_red = nullptr;
  bool comp_meter() const { return desc.kind == WAA_NODE_DYNAMICS_COMPRESSOR && desc.i[0] == 1; }
  float* d_window = nullptr;
  Cplx *d_an_tw = nullptr, *d_an_twfull = nullptr;
  float *d_an_prev = nullptr, *d_an_db = nullptr, *d_an_time = nullptr;
  uint8_t* d_an_bytes = nullptr;
  // planning
  int in_nch = 1;      // computed input channel count
  int out_nch = 1;     // static output channel count
  bool live = false;
  bool materialized = false;
  SignalRef sig{};     // valid when materialized
  SignalRef hist{};    // DelayNode: the delay line (the node's mixed input, absolute time)
  bool hist_is_temp = false;
  std::vector<int> in_edges;   // indices into edges, in summing order
  // audio-rate inputs of this node's AudioParams (edges with to_input = WAA_PARAM_INPUT(k)), in summing order,
  // and the per-frame value signal planned for them (param.rs:686-795)
  std::vector<std::vector<int>> pin_edges;
  std::vector<ParamRef> pin_ref;
  std::vector<char> pin_ready;
  int n_consumers = 0;
  // a BufferSource that renders its AudioBuffer unchanged from frame 0 (fast track, rate 1, no loop, same layout for
  // every instance) and whose only consumer is a node-major step that takes a bounded view: it is not materialised,
  // the consumer reads the buffer in place (view_valid frames per channel, zeros beyond)
  bool is_view = false;
  // BiquadFilterNode with constant coefficients whose only consumer is a long ConvolverNode (three-pass transforms): the
  // forward transform's input stage renders it (fold_conv = the convolver; the convolver's pre_biquad = this node)
  int fold_conv = -1, pre_biquad = -1;
  // DelayNode outside a loop, constant / k-rate delayTime, consumed by chain input stages only: no reader pass, the
  // consumers gather from the delay line themselves (IN_DELAYED)
  bool delay_folded = false;
  int osc_step = -1;  // OscillatorNode: index of its launch in the plan (post ops may be folded into it later)
  uint64_t hist_valid = 0;  // frames of the delay line that may be read (zeros beyond): the padded length, or a source view's
  SignalRef view_sig{};
  uint64_t view_valid = 0;
  // dynamic plans (waa_dyn.hip): per-quantum codes of the published signal, and the quantum slot of channel 1 when the
  // signal feeds a mono-IR convolver whose second FFTConvolver only advances on stereo quanta
  // output ports (waa_plan_route.cpp): one NODE_SPLITTER_PORT node stands for every connected output of a ChannelSplitterNode —
  // `port_of` = the splitter, `port` = the output; its signal is a one-channel VIEW of the splitter's input bus.  On the splitter:
  // port_views = the bus is its only producer's signal (no launch).  silent_port: the output lies beyond the producer's channels
  // (its only consumers are ChannelMergerNodes, which write the zeros themselves).
  int port_of = -1, port = 0;
  bool port_views = false, silent_port = false;
  uint8_t* code = nullptr;
  uint8_t* in_code = nullptr;  // ConvolverNode: codes of its mixed input
  uint32_t* remap = nullptr;
};

struct ProfileEntry {
  std::string name;
  uint64_t launches = 0;
  double total_ms = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
};

// What a launch of the plan is.  The numbers are fixed: internal error messages and the launch-list dump (WAA_PLAN_LAUNCHES) print them.
enum class StepKind : int {
  Chain = 0,              // interpreter kernel over a chain of element-wise ops (or the LDS-ring kernel: Step::echo_fb / echo_ff)
  BiquadStream = 1,       // streaming biquad kernel; with Step::scan.payload its time-parallel form (waa_biquad_scan.hip)
  ConvFft = 2,            // FFT convolver: forward transform, multiply-accumulate, inverse transform
  ZeroFill = 3,           // memset of Step::zero_ptr
  ConvDirect = 4,         // direct FIR (short impulse responses)
  BiquadCoefs = 5,        // per-frame biquad coefficients from a-rate params
  IirStream = 6,          // streaming IIR kernel
  Delay = 7,              // delay gather (reader half of a DelayNode)
  Loop = 8,               // feedback loop rendered quantum by quantum inside one launch (loop_kernel)
  Osc = 9,                // oscillator
  Dyn = 10,               // dynamic-count group (dyn_kernel)
  ConvCodes = 11,         // per-quantum channel-count codes of a convolver's output
  BiquadHp = 12,          // digest of a shared per-frame coefficient table
  PannerGeom = 13,        // per-frame panner geometry
  Timeline = 14,          // automation timelines replayed on the device
  Link = 15,              // link table of a frozen-state node (waa_frozen.hip)
  QGemm = 16,             // one resampling stage of an oversampled WaveShaper (qgemm_kernel)
  Hrtf = 17,              // HRTF FIR
  BiquadTileDigest = 18,  // tile digests of an a-rate biquad (waa_biquad_lanes.hip)
  BiquadLanes = 19,       // a-rate biquad: pass A + chain + pass B (waa_biquad_lanes.hip)
  OsFft = 20,             // the oversampled WaveShaper in one launch (waa_osfft.hip)
  Compressor = 21,        // DynamicsCompressorNode: level, detector, apply (waa_compressor.hip)
  Route = 22,             // channel routing (route_kernel)
  ShaperInst = 23,        // WaveShaperNode with one curve per instance (waa_shaper_inst.hip)
};
constexpr int N_STEP_KINDS = 24;

// The per-kind facts that the planner's loop handling, its fusions and the executor ask for, in one place.
struct StepTraits {
  const char* name;     // messages and the launch-list dump
  bool once_in_loop;    // inside a feedback loop: depends only on data from outside it, runs once before the blocks (runs_once_in_loop)
  bool quantum_ranged;  // can be launched over a range of render quanta: exactly the cases of run_step_q (waa_run.cpp)
  bool frozen_state;    // launch of a frozen-state node: refused inside a block-scheduled loop
  // the echo-tail fusion (waa_plan_loops.cpp) counts the readers of a delay line from step_io's read sets and leaves the whole plan
  // alone when a launch is of a kind whose reads it takes as unknown.  ConvCodes and Link report none to step_io; Compressor,
  // Route and ShaperInst report theirs, but were added after the fusion and have not been tried with it.
  bool reads_unknown_to_echo_fusion;
};
inline const StepTraits& step_traits(StepKind k) {
  static const StepTraits traits[] = {
      // name                 once   ranged frozen unknown
      {"chain",               false, false, false, false},
      {"biquad_stream",       false, false, false, false},
      {"conv_fft",            false, true,  false, false},
      {"zero_fill",           true,  false, false, false},
      {"conv_direct",         false, false, false, false},
      {"biquad_coefs",        true,  false, false, false},
      {"iir_stream",          false, false, false, false},
      {"delay",               false, false, false, false},
      {"loop",                false, false, false, false},
      {"osc",                 false, false, false, false},
      {"dyn",                 false, true,  false, false},
      {"conv_codes",          false, true,  false, true},
      {"biquad_hp",           true,  false, false, false},
      {"panner_geom",         true,  false, false, false},
      {"timeline",            true,  false, false, false},
      {"link",                false, true,  true,  true},
      {"qgemm",               false, false, true,  false},
      {"hrtf",                false, true,  true,  false},
      {"biquad_tile_digest",  false, false, false, false},
      {"biquad_lanes",        false, false, false, false},
      {"os_fft",              false, true,  true,  false},
      {"compressor",          false, false, false, true},
      {"route",               false, false, false, true},
      {"shaper_inst",         false, false, false, true},
  };
  static_assert(sizeof traits / sizeof traits[0] == N_STEP_KINDS, "one row per StepKind, in the enum's order");
  return traits[(int)k];
}

struct Step {
  StepKind kind = StepKind::Chain;
  ChainDesc chain{};
  BiquadStreamDesc bq{};
  BiquadScanCtl scan{};   // BiquadStream with scan.payload: the time-parallel form (waa_biquad_scan.hip)
  BiquadLanesDesc lanes{};  // BiquadTileDigest and BiquadLanes, waa_biquad_lanes.hip
  ConvDesc conv{};
  BiquadCoefDesc coef{};
  const uint8_t* coef_types = nullptr;  // BiquadCoefs of a node whose instances differ in their filter type: [n_inst] on the device
  IirStreamDesc iir{};
  DelayDesc delay{};
  LoopDesc loop{};
  OscDesc osc{};
  DynDesc dyn{};
  ConvCodeDesc ccode{};
  BiquadHpDesc hp{};
  PannerGeomDesc geom{};
  TimelineDesc tl{};
  LinkDesc link{};
  QGemmDesc qgemm{};
  OsFftDesc osfft{};      // OsFft: the oversampled WaveShaper in one launch (waa_osfft.hip)
  HrtfDesc hrtf{};
  RouteDesc route{};      // Route: ChannelMergerNode / the input bus of a ChannelSplitterNode (waa_route.hip; reads / writes in loop_reads / loop_writes)
  CompDesc comp{};        // Compressor (profile slots: slot_fwd = level, slot_mac = detector, slot_inv = apply)
  ShaperInstDesc shaper{};  // ShaperInst
  // Compressor of a node with the meter on (desc.i[0] = 1): the fourth launch of the step, behind apply (meter.out != nullptr;
  // profile slot: slot_meter).  It is part of the node's step, so nothing can be ordered between it and the detector.
  CompMeterDesc meter{};
  int slot_meter = -1;
  int slot_fwd = -1, slot_mac = -1, slot_inv = -1;
  void* zero_ptr = nullptr;
  size_t zero_bytes = 0;
  int cmax = 1;
  int profile_slot = -1;
  // plan validation (host only): signals and per-frame param tables this step reads / writes; a quantum-serial loop
  // step lists the external signals its items read and the signals they publish
  std::vector<const void*> loop_reads, loop_writes;
  int group = -1;         // >= 0: member of a block-scheduled feedback loop (launched block by block)
  int qgroup = -1;        // >= 0: member of a feedback loop that is cut at frozen-state nodes and launched QUANTUM BLOCK by quantum block
                          // (dynamic-count plans, round 5: ranged dyn_kernel / link / oversampling / HRTF launches; waa_batch::qgroup_quanta)
  bool prologue = false;  // inside a group: runs once over the full range before the blocks
  // the only body step of a block-scheduled loop, and the loop qualifies for the LDS-ring kernel (waa_echo.hip): index of
  // the feedback input (-1: no) and the chunk size in 256-frame sub-tiles
  int echo_fb = -1, echo_chunk = 0, echo_ring = 16384;  // (echo_ring: frames per channel of the LDS ring)
  // ... or the LAST of three body steps (delayed read -> streaming biquad -> sum) rendered as the ring kernel's BQ form
  // (echo_bq.coefs != nullptr); the first two are marked echo_fused
  EchoBq echo_bq{};
  // ... and the line's only reader outside the loop rendered by the same launch (EchoTail): on the loop step, index of that
  // step and its descriptor; on that step itself, echo_fused = it is not launched
  int echo_tail_step = -1;
  EchoTail echo_tail{};
  bool echo_fused = false;
  // a chain step outside any loop rendered by the ring kernel with nothing fed back (echo_feed_forward): the stand-in loop
  // stage; echo_tail / echo_chunk as above
  bool echo_ff = false;
  ChainDesc echo_line{};
};

// A launch planned for a member of a feedback loop that depends only on data from outside the loop: it runs once, over the whole
// render, in front of the blocks.  Param tables and fills by kind, and a chain that is nothing but an AudioParam's summing chain.
inline bool runs_once_in_loop(const Step& st) {
  return step_traits(st.kind).once_in_loop || (st.kind == StepKind::Chain && st.chain.n_ops == 1 && st.chain.ops[0].kind == OP_PARAM_ADD);
}

struct SchedOut {
  std::vector<QRec> qrec;
  std::vector<SlowRec> slow;  // empty if no slow quantum
  std::vector<uint8_t> tile_fast;
  bool any_slow = false;
  int64_t ended_quantum = -1;  // quantum in which the renderer sends `ended` (-1: not during the render)
  bool ended_at_unload = false;  // ... or before_drop sends it after the last quantum
};
using SchedKey = std::tuple<double, double, double, double, int, double, double, uint64_t, float, float, float>;

}  // namespace host
}  // namespace waa

using namespace waa::host;  // (the opaque C handle lives in the global namespace)

constexpr uint32_t EDGE_NEVER = 0xFFFFFFFFu;
struct waa_batch {
  uint32_t n_inst = 0, n_out = 0;
  uint64_t length = 0;
  float sr = 0;
  uint32_t n_quanta = 0, n_tiles = 0;
  uint64_t lp = 0;  // padded frames per channel
  int device = 0;
  int n_cu = 256;  // compute units of the device (plan-only batches: an MI355X)
  hipStream_t stream = nullptr;
  void* stage = nullptr;  // pinned staging block for transfers from / to PAGEABLE caller memory (xfer_h2d / xfer_d2h, waa_xfer.cpp)
  std::vector<Node> nodes;
  std::vector<waa_edge_desc> edges;
  // OfflineAudioContext::suspend_sync (offline.rs:359-397): the control clock — the render quantum in front of which the render
  // is "suspended" (waa_render_range moves it); control calls made at ctl_q > 0 take effect from that quantum on.  An edge is
  // live for quanta [edge_on, edge_off): waa_connect / waa_disconnect at ctl_q > 0 (EDGE_NEVER: no end).  At plan time an edge
  // that is not live for the whole render becomes a GainNode whose gain is 1 inside the window and 0 outside
  // (desugar_timed_edges, waa_plan_prepass.cpp): gain.rs' two fast paths — pass-through and silence — are exactly "connected" and "not".
  uint32_t ctl_q = 0;
  std::vector<uint32_t> edge_on, edge_off;
  bool ranged = false;              // waa_render_range has been called: waa_render would render from the start again
  uint32_t n_user_nodes = 0;        // nodes of the caller's graph (the gates of timed edges are appended behind them)
  bool timed_edges_done = false;
  bool ports_done = false;          // the outputs of ChannelSplitterNodes have been turned into port nodes (desugar_output_ports)
  // views (one channel of another signal) by base pointer -> base of the signal that owns the memory: what a launch reads through
  // a view is what the owner's launch writes (step_io resolves reads through it)
  std::map<const void*, const void*> view_owner;
  std::string timed_note;
  std::vector<uint32_t> order;
  std::vector<uint8_t> cut;         // per DelayNode: writer->reader edge removed by the cycle breaker
  std::vector<uint32_t> group_tiles;  // block size (tiles) of every block-scheduled feedback loop
  std::vector<uint32_t> qgroup_quanta;  // block size (render quanta) of every quantum-blocked loop of a dynamic-count plan
  std::vector<int32_t*> loop_flags;     // device words a delay writer sets when a multi-quantum block was invalid (waa_dyn.hip)
  bool loops_one_quantum = false;       // ... after which the loops are rendered one quantum per block
  bool loops_unsettled = false;         // a render with multi-quantum blocks is in flight: its flags have not been looked at
  std::vector<void*> allocs;        // plan-owned device allocations
  std::vector<void*> payload_allocs;  // buffers uploaded through the API
  std::vector<std::pair<void*, size_t>> state_bufs;  // zeroed at the start of every render
  // host copies of the per-instance source tables handed to the kernels (key: the device table): a signal wider than six channels is
  // rendered in channel slices (push_chain_step), and a slice of a SOURCE is the same table with its base pointers moved on
  std::map<const waa::SrcInst*, std::vector<waa::SrcInst>> src_tables;
#ifdef WAA_MEASURE
  std::map<uint32_t, const waa::SrcInst*> src_table_of_node;  // source node -> key of its table above (waa_debug_source_records)
#endif
  std::vector<std::pair<void*, size_t>> ones_bufs;   // filled with 0xFF bytes at the start of every render
  std::vector<Step> steps;
  bool planned = false;
  // Graph-modulated playbackRate / detune of AudioBufferSourceNodes (k-rate params the HOST needs: the playhead replay).
  // prepass = true: build_plan plans only what feeds those params (the modulators and the params' summing chains); the steps
  // are run, one value per quantum is read back and installed as k-rate value blocks, the param edges are removed and the
  // real plan is built (waa_plan_prepass.cpp::resolve_source_rate_modulation).
  bool prepass = false;
  std::vector<std::pair<uint32_t, uint32_t>> prepass_params;  // (source node, param)
  std::vector<waa::ParamRef> prepass_refs;                          // per entry: the per-frame values the summing chain writes
  std::string prepass_note;
  bool no_short_ring = false;        // second planning pass: a short feedback loop tried as the LDS-ring kernel did not qualify
  std::set<uint32_t> short_ring_loops;  // DelayNodes of loops shorter than a tile planned for the ring kernel (loop_block_tiles)
  bool force_dynamic = false;        // second planning pass: a loop member the static loop kernel cannot render
  bool dynamic = false;              // the plan renders the reference's dynamic channel counts (dyn_kernel)
  uint64_t code_stride = 0;          // bytes per instance of a code table (n_quanta rounded up)
  bool rendered = false;
  // waa_render_sharded: buffers of the streamed source are allocated and registered first (the plan only needs their shape), filled
  // from the host when the sub-batch has its turn on the link (fill_pending_uploads, waa_xfer.cpp)
  bool defer_fill = false;
  struct PendingFill {
    int kind;  // 0: f32 planes, 1: interleaved 16-bit PCM through the decode kernel
    const void* host;
    float* planes;
    int16_t* staging;
    uint32_t n_items, n_ch;
    uint64_t frames, stride, target;
    float src_sr;
  };
  std::vector<PendingFill> pending_fills;
  // waa_batch_rearm: the whole-batch source uploads by node, so that a planned batch can take the NEXT set of AudioBuffers of the
  // same shape into the same device buffers (a serving loop: same graph, new audio — no plan, no allocation)
  std::map<uint32_t, PendingFill> batch_fills;
  bool rearmed = false;
  int64_t batch_fill_node = -1;
  int16_t* pcm_out = nullptr;     // staging of waa_download_all_pcm16 (allocated on first use, freed with the batch)
  size_t pcm_out_count = 0;
  void* levels_ws = nullptr;      // workspace of waa_output_levels / _level_series (waa_levels_host.cpp; first use, freed with the batch)
  void* loudness_ws = nullptr;    // workspace of waa_output_loudness / _loudness_series (waa_loudness_host.cpp; likewise)
  float* pcm_gain = nullptr;      // [n_inst] the gains of waa_download_all_pcm16_gain on the device (likewise)
  bool dry = false;                  // WAA_DEVICE_PLAN_ONLY: allocations are host memory, nothing is launched
  std::vector<std::string> plan_log;  // waa_plan_describe
  bool profiling = false;
  std::vector<ProfileEntry> prof;
  // where the first waa_render's host time goes (waa_plan_describe prints it: "timing: ..."): an offline context renders
  // once, so planning + allocation IS part of what a caller waits for
  double t_plan_ms = 0, t_alloc_ms = 0, t_upload_ms = 0;  // (alloc / upload: running totals of the batch)
  uint64_t n_alloc = 0, alloc_bytes = 0;
  uint32_t* scan_counter = nullptr;   // 8 unit counters (16 words apart) + error flag of the time-parallel biquad launches
  uint32_t scan_issued[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // host mirror of the counters during a render
  // one playhead replay per distinct (source node, schedule) and plan: the silence / count replay, the code rows and the source's
  // input tables all ask for it (a 10 s slow-track replay is milliseconds); cleared when build_plan returns
  std::map<std::pair<uint32_t, SchedKey>, std::shared_ptr<SchedOut>> sched_cache;
  double plan_alloc_ms = 0, plan_upload_ms = 0;          // ... and their part inside build_plan
  uint64_t plan_n_alloc = 0, plan_alloc_bytes = 0;
};

namespace waa {
namespace host {

// WAA_PLAN_TRACE=1 (measurement build only): how long the named sections of build_plan took, on stderr
struct PlanTrace {
  const char* what;
  std::chrono::steady_clock::time_point t0;
  bool on;
  explicit PlanTrace(const char* w) : what(w), t0(std::chrono::steady_clock::now()), on(measure_switch("WAA_PLAN_TRACE") != nullptr) {}
  ~PlanTrace() {
    if (on) fprintf(stderr, "[plan] %-40s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
};

// Device arena (waa_device_arena_reserve, include/waa_hip.h): one slab per device, reserved once — typically at process start,
// before anything else fragments the device's memory — from which the big buffers of every batch are carved in 2 MB-aligned
// pieces; the slab is one mapping with the largest page-table fragments the driver gives, so WHERE a batch's output lands no
// longer changes from batch to batch (the same kernel ran at 1.33 or 1.55 ms depending on the
// hipMalloc that happened to serve its output).  Defined in waa_arena.cpp.
void* arena_alloc(int device, size_t bytes, bool read_only = false);  // (read_only: the top end of a graded arena)
bool arena_free(int device, void* p);
void* guard_alloc(int device, size_t bytes);  // WAA_GUARD_ALLOC=1 (testing aid, waa_arena.cpp)
// bytes of one physical unit when `p` lies in a GRADED arena of `device` (units mapped side by side), else 0
size_t arena_unit_of(int device, const void* p);
// hipMemcpy2DAsync whose device side may lie in a graded arena: the runtime refuses a pitched copy whose extent exceeds ONE mapped
// physical unit ("invalid argument"; 1-D copies, memsets and kernels are not affected — tools/vmm_copy_check.hip,
// profiles/r06h_vmm_copy_check*.txt), so such a copy is issued in row groups of at most half a unit.
inline hipError_t copy2d_async(int device, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height,
                               hipMemcpyKind kind, hipStream_t stream) {
  const bool dev_is_dst = kind == hipMemcpyHostToDevice;
  const size_t unit = arena_unit_of(device, dev_is_dst ? dst : src), pitch = dev_is_dst ? dpitch : spitch;
  if (!unit || pitch * height <= unit / 2) return hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, kind, stream);
  const size_t per = std::max<size_t>((unit / 2) / pitch, 1);
  for (size_t r = 0; r < height; r += per) {
    const hipError_t e = hipMemcpy2DAsync(static_cast<char*>(dst) + r * dpitch, dpitch, static_cast<const char*>(src) + r * spitch, spitch, width,
                                          std::min(per, height - r), kind, stream);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

template <typename T>
int dev_alloc(waa_batch* b, T** out, size_t count, bool payload = false) {
  void* p = nullptr;
  size_t bytes = std::max<size_t>(count * sizeof(T), 16);
  if (b->dry) {
    // plan-only: big signal / spectrum buffers are never touched, so reserve address space lazily (calloc of a
    // huge block is not committed until written) — small tables are really filled by dev_upload
    p = std::calloc(1, bytes);
    if (!p) return fail(WAA_ERR_DEVICE, "plan-only allocation of %zu bytes failed", bytes);
    (payload ? b->payload_allocs : b->allocs).push_back(p);
    *out = reinterpret_cast<T*>(p);
    return 0;
  }
  const auto t0 = std::chrono::steady_clock::now();
  hipError_t e = hipSuccess;
  static const bool guard = getenv("WAA_GUARD_ALLOC") != nullptr;
  if (guard) p = guard_alloc(b->device, bytes);
  if (!p && bytes >= (1u << 20)) p = arena_alloc(b->device, bytes, payload);  // (small tables stay with hipMalloc; payloads are only read)
  if (!p) e = hipMalloc(&p, bytes);
  b->t_alloc_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  b->n_alloc++;
  b->alloc_bytes += bytes;
  if (e != hipSuccess) return fail(WAA_ERR_DEVICE, "hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
  // WAA_POISON_ALLOC=1 (testing aid): fresh device memory is filled with 0xFF bytes (NaNs as f32 / f64, huge indices) —
  // a kernel whose OUTPUT depends on memory nobody wrote then fails loudly and every time, instead of once in 20 000
  // graphs when the pages happen to hold something else (hipMalloc does not clear; found that way: see DESIGN.md section 5)
  static const bool poison = getenv("WAA_POISON_ALLOC") != nullptr;
  if (poison) {  // (the fill must be over before anything else touches the buffer: it runs on the null stream, the batch on its own)
    (void)hipMemset(p, 0xFF, bytes);
    (void)hipDeviceSynchronize();
  }
  (payload ? b->payload_allocs : b->allocs).push_back(p);
  *out = reinterpret_cast<T*>(p);
  return 0;
}
template <typename T>
int dev_upload(waa_batch* b, T** out, const std::vector<T>& host) {
  int e = dev_alloc(b, out, host.size());
  if (e) return e;
  if (!host.empty()) {
    if (b->dry) {
      std::memcpy(*out, host.data(), host.size() * sizeof(T));
    } else {
      const auto t0 = std::chrono::steady_clock::now();
      HIP_TRY(hipMemcpy(*out, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
      // A synchronous hipMemcpy runs on the NULL stream; the batch's kernels — also the plan-time ones, e.g. the impulse-
      // response spectra right after the IR's upload — run on a non-blocking stream of their own, which the null stream
      // does not order.  hipMemcpy returns when the host buffer may be reused, not necessarily when the last bytes have
      // landed in device memory: wait for the null stream, so that a table is THERE when dev_upload returns (a few us per
      // table at plan time).  Suspected cause of two load-dependent mismatches in 40 000 random graphs.
      HIP_TRY(hipStreamSynchronize(nullptr));
      b->t_upload_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
  }
  return 0;
}

// nodes whose render state freezes while they do not process (waa_frozen.hip): rendered node-major behind a link table
inline bool is_frozen_node(const Node& n) {
  return (n.desc.kind == WAA_NODE_WAVESHAPER && n.has_curve && n.desc.i[0] != WAA_OVERSAMPLE_NONE) ||
         (n.desc.kind == WAA_NODE_PANNER && n.desc.i[0] == WAA_PANNING_HRTF);
}
// nodes that go on rendering after their input has fallen silent (filter state, delay line, impulse response / HRIR tail)
inline bool has_memory(const Node& n) {
  const uint32_t k = n.desc.kind;
  return k == WAA_NODE_BIQUAD || k == WAA_NODE_IIR_FILTER || k == WAA_NODE_DELAY || (k == WAA_NODE_CONVOLVER && n.has_ir) ||
         (k == WAA_NODE_PANNER && n.desc.i[0] == WAA_PANNING_HRTF);
}
// what a WaveShaper's curve makes of a sample of 0 (waveshaper.rs:498-509); 0 without a curve
inline float curve_at_zero(const std::vector<float>& curve) {
  const size_t cn = curve.size();
  return cn == 0 ? 0.f : (cn % 2 ? curve[cn / 2] : (curve[cn / 2 - 1] + curve[cn / 2]) / 2.f);
}
inline float curve_at_zero(const Node& n) { return curve_at_zero(n.curve); }

// internal node kind (never in a caller's graph): one connected output of a ChannelSplitterNode (waa_plan_route.cpp)
constexpr uint32_t NODE_SPLITTER_PORT = 0x100u;
inline bool is_routing_node(const Node& n) {
  return n.desc.kind == WAA_NODE_CHANNEL_SPLITTER || n.desc.kind == WAA_NODE_CHANNEL_MERGER || n.desc.kind == NODE_SPLITTER_PORT;
}
// DynamicsCompressorNode: rendered node-major by launches of its own (waa_compressor.hip), input and output materialised
inline bool is_compressor(const Node& n) { return n.desc.kind == WAA_NODE_DYNAMICS_COMPRESSOR; }
// WaveShaperNode with one curve per instance: ends a chain like the compressor, rendered node-major by one launch of its own
// (waa_shaper_inst.hip), input and output materialised; never folded into a neighbour's kernel, whose curve is one per launch
inline bool is_shaper_per_instance(const Node& n) { return n.desc.kind == WAA_NODE_WAVESHAPER && n.per_inst_curve(); }
// quanta of look-ahead, in f32 exactly as dynamics_compressor.rs:253-254 sizes its ring (ring - 1)
inline uint32_t compressor_delay_quanta(float sample_rate) { return (uint32_t)std::ceil(sample_rate * 0.006f / (float)RQ); }

inline int check_node(waa_batch* b, uint32_t node, uint32_t kind) {
  if (!b) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch");
  if (node >= b->nodes.size() || b->nodes[node].desc.kind != kind)
    return fail(WAA_ERR_INVALID_ARGUMENT, "node %u is not of the expected kind", node);
  return 0;
}
inline int check_inst(waa_batch* b, uint32_t inst) {
  if (inst != WAA_ALL_INSTANCES && inst >= b->n_inst) return fail(WAA_ERR_INVALID_ARGUMENT, "instance out of range");
  return 0;
}
inline int check_unplanned(waa_batch* b) {
  if (b->planned) return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - the batch is frozen once rendering has started");
  return 0;
}
// PannerOptions' values (panner.rs:408-428, 20-33): waa_batch_create's check of a PANNER node's d[0..5], and that of
// waa_panner_set_options_instance
inline int check_panner_values(double ref_distance, double max_distance, double rolloff_factor, double cone_outer_gain) {
  if (!(ref_distance >= 0.)) return fail(WAA_ERR_INVALID_ARGUMENT, "RangeError - refDistance cannot be negative");
  if (!(max_distance > 0.)) return fail(WAA_ERR_INVALID_ARGUMENT, "RangeError - maxDistance must be strictly positive");
  if (!(rolloff_factor >= 0.)) return fail(WAA_ERR_INVALID_ARGUMENT, "RangeError - rolloffFactor cannot be negative");
  if (!(cone_outer_gain >= 0. && cone_outer_gain <= 1.))
    return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - coneOuterGain must be in the range [0, 1]");
  return 0;
}
inline int check_channel_count(uint32_t n_ch) {
  if (n_ch == 0 || n_ch > WAA_MAX_CHANNELS) return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - Invalid number of channels");
  return 0;
}
inline int check_sample_rate(float sr) {  // MIN/MAX_SAMPLE_RATE, src/lib.rs:149-160
  if (!(sr >= 3000.f && sr <= 768000.f)) return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - Invalid sample rate: %f", sr);
  return 0;
}
// the instances [lo, hi) a call names: one, or all `n` of them (WAA_ALL_INSTANCES)
struct InstRange { uint32_t lo, hi; };
inline InstRange inst_range(uint32_t inst, uint32_t n) { return inst == WAA_ALL_INSTANCES ? InstRange{0, n} : InstRange{inst, inst + 1}; }
inline void set_bufs(Node& n, InstRange r, const DeviceBuffer& db) { std::fill(n.bufs.begin() + r.lo, n.bufs.begin() + r.hi, db); }

}  // namespace host
}  // namespace waa

namespace waa {
namespace host {

// ---- waa_schedule.cpp: host-side arithmetic of the reference's control/render split ---------------------
struct Coefs {
  double b0, b1, b2, a1, a2;
};
Coefs biquad_coefs(int type, double sample_rate, double f0, double gain, double q);   // biquad_filter.rs:28-373
float computed_freq(float freq, float detune);                                          // biquad_filter.rs:367-373
struct V3 {
  float x, y, z;
};
constexpr float PI_F = 3.14159265358979323846f;
void azimuth_elevation(V3 sp, V3 lp, V3 lf, V3 lu, float* az, float* el);               // spatial.rs / panner.rs
float spatial_angle(V3 sp, V3 so, V3 lp);
float cone_gain(const waa_panner_options& o, V3 sp, V3 so, V3 lp);
float dist_gain(const waa_panner_options& o, V3 sp, V3 lp);
// AudioBufferSourceNode scheduler: port of audio_buffer_source.rs:422-845
void schedule_source(const waa_batch* b, const SourceSched& cfg, uint64_t frames, float buf_sr, bool has_buffer,
                     const std::vector<float>& rate_q, const std::vector<float>& detune_q, SchedOut* out);
// the same through the batch's per-plan cache (params without per-quantum blocks only: the key holds their one value)
std::shared_ptr<SchedOut> schedule_source_cached(waa_batch* b, uint32_t node, const SchedKey& key, const SourceSched& cfg, uint64_t frames,
                                                 float buf_sr, bool has_buffer, const std::vector<float>& rate_q,
                                                 const std::vector<float>& detune_q);
// one value per quantum (or a single one) of a host-evaluated param, clamped like the reference
std::vector<float> param_per_quantum(const waa_batch* b, const ParamStore& p, uint32_t inst, bool* varies);

// ---- waa_plan.cpp: graph -> launch plan -----------------------------------------------------------------
int build_plan(waa_batch* b);
// waa_plan_prepass.cpp: what waa_render / waa_plan_describe call — the two pre-passes (one renders: never on a plan-only batch), then build_plan
int plan_batch(waa_batch* b);
// ... and, for everything that hands out results: waits for a render of optimistic multi-quantum loop blocks and repeats it if flagged
int settle_loops(waa_batch* b);
// waa_run.cpp: the launches of the current plan, from the initial state
int run_steps(waa_batch* b);
// ---- waa_xfer.cpp: transfers between CALLER memory and the device, through the batch's pinned staging block if pageable ----
// `height` rows of `width` bytes, pitches in bytes; asynchronous on the batch's stream for pinned memory, complete on return otherwise
int xfer_h2d(waa_batch* b, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height);
int xfer_d2h(waa_batch* b, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height);
int fill_upload(waa_batch* b, const waa_batch::PendingFill& f);
int fill_pending_uploads(waa_batch* b);
// waa_abi_sources.cpp: 16-bit PCM -> `planes` = [n_items][n_ch][stride] at the batch's rate (sources and the convolver's response)
int decode_pcm16(waa_batch* b, const int16_t* pcm, uint32_t n_items, uint32_t n_ch, uint64_t frames, float src_sr, float** planes,
                 uint64_t* stride_out, uint64_t* target_out);
// waa_frozen_host.cpp: WaveShaper 2x / 4x and the HRTF panner as node-major steps; src_id >= 0: static plan, the node's
// only input is that source node (its host-known codes stand in for the codes a dynamic plan computes on the device)
int plan_oversampler(waa_batch* b, uint32_t id, int src_id);
int plan_hrtf(waa_batch* b, uint32_t id, int src_id);
bool hrtf_sphere_loaded();
void plan_note(waa_batch* b, const char* fmt, ...);
// the plan's line for a PannerNode whose instances differ in their option sets, once per node (waa_plan_ops.cpp)
void note_panner_options(waa_batch* b, uint32_t id, const Node& n);
int slot_for(waa_batch* b, const char* name);
// one launch: the profiling events around it when the batch is profiled and the launch has a slot, the error check behind it
template <typename L>
int timed(waa_batch* b, int slot, L&& launch) {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (b->profiling && slot >= 0) {
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    HIP_TRY(hipEventRecord(e0, b->stream));
  }
  launch();
  {
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess)
      return fail(WAA_ERR_DEVICE, "launch of %s failed: %s", slot >= 0 ? b->prof[slot].name.c_str() : "a kernel without a profile slot",
                  hipGetErrorString(le));
  }
  if (b->profiling && slot >= 0) {
    HIP_TRY(hipEventRecord(e1, b->stream));
    b->prof[slot].pending.push_back({e0, e1});
  }
  return 0;
}
void default_channel_config(Node& n, uint32_t n_out);
void compute_order(const waa_batch* b, std::vector<uint8_t>* cut, std::vector<uint8_t>* muted, std::vector<uint32_t>* items);
int computed_in_nch(const Node& n, int maxc);  // quantum.rs:543-547

}  // namespace host
}  // namespace waa
