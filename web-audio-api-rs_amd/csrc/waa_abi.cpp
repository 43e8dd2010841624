// waa_abi.cpp — the batch's life cycle in the C ABI of libwaa_hip.so (include/waa_hip.h): construction and validation (the
// reference's panics become status codes with the same message text), connections, render, download, plan description,
// profiling.  Sources: waa_abi_sources.cpp, per-node payloads and AudioParams: waa_abi_nodes.cpp, analyser pulls:
// waa_analyser_host.cpp.  All sample arithmetic happens in the HIP kernels; there is no CPU fallback: without a HIP device
// every render call fails with WAA_ERR_DEVICE.
#include <mutex>
#include <set>

#include "waa_host.hpp"

namespace waa {
namespace host {
thread_local char g_err[768];
int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}
// WAA_PLAN_DYN_ITEMS=1 (measurement build): what the dynamic-count planner puts into the item tables of its dyn_kernel launches
// and into the code kernels' descriptors, without an address in it (tests/test_launch_list.py: dyn_items.txt).  Plan-only batches
// only: their tables are host memory.
static void describe_dyn_items(const waa_batch* b, std::string& text) {
  char l[640];
  auto set = [](const void* p) { return p ? 1 : 0; };
  auto param = [&](const char* name, const ParamRef& p) {
    std::string s = std::string(" ") + name + "=m" + std::to_string(p.mode);
    if (p.mode == 0 && p.base)
      for (uint32_t i = 0; i < std::min(b->n_inst, 4u); i++) {
        snprintf(l, sizeof l, "%c%.9g", i ? ',' : ':', (double)p.base[i]);
        s += l;
      }
    return s;
  };
  for (size_t k = 0; k < b->steps.size(); k++) {
    const Step& st = b->steps[k];
    if (st.kind == StepKind::ConvCodes) {
      const ConvCodeDesc& c = st.ccode;
      snprintf(l, sizeof l, "launch %zu conv_codes: cout=%d ir_nch=%d impulse_length=%llu noise=%d in_test_nch=%d state=%d nir=", k, c.cout, c.ir_nch,
               (unsigned long long)c.impulse_length, c.noise, c.in_test_nch, set(c.state));
      text += l;
      for (int j = 0; j < 4; j++) {
        snprintf(l, sizeof l, "%s%u:%llx", j ? "," : "", c.nir[j].seg_count, (unsigned long long)c.nir[j].seg_mask);
        text += l;
      }
      text += "\n";
    }
    if (st.kind != StepKind::Dyn) continue;
    const DynDesc& d = st.dyn;
    snprintf(l, sizeof l, "launch %zu dyn: n_items=%d cmax=%d n_stages=%d stage_begin=", k, d.n_items, d.cmax, d.n_stages);
    text += l;
    for (int s = 0; s <= d.n_stages; s++) text += (s ? "," : "") + std::to_string(d.stage_begin[s]);
    snprintf(l, sizeof l, " split_ok=%u save_f=%d save_i=%d\n", d.split_ok, set(d.save_f), set(d.save_i));
    text += l;
    for (int i = 0; i < d.n_items; i++) {
      const DynItem& it = d.items[i];
      snprintf(l, sizeof l, "launch %zu item %d: kind=%d dk=%d cc=%d mode=%d interp=%d n_in=%d nch_pub=%d publish_upmix=%d compact_ch1=%d flags=%d writer_item=%d in_cycle=%d num_quanta=%d in=[",
               k, i, it.kind, it.dk, it.cc, it.mode, it.interp, it.n_in, it.nch_pub, it.publish_upmix, it.compact_ch1, it.flags, it.writer_item,
               it.in_cycle, it.num_quanta);
      text += l;
      for (int j = 0; j < it.n_in; j++) {
        snprintf(l, sizeof l, "%s%d/%d/code%d/remap%d", j ? " " : "", it.in[j].item, it.in[j].nch, set(it.in[j].code), set(it.in[j].remap));
        text += l;
      }
      text += "] op.kind=" + std::to_string(it.op.kind) + param("p0", it.op.p0) + param("p1", it.op.p1) + param("p2", it.op.p2) + param("alt1", it.alt1) +
              param("alt2", it.alt2);
      snprintf(l, sizeof l, " pmod_n=%d pmod_item=%d,%d,%d,%d pmod_min=%.9g pmod_max=%.9g pmod_def=%.9g out=%d out_code=%d aux32=%d xline=%d xaux32=%d xstate=%d\n",
               it.pmod_n, it.pmod_item[0], it.pmod_item[1], it.pmod_item[2], it.pmod_item[3], (double)it.pmod_min, (double)it.pmod_max, (double)it.pmod_def,
               set(it.out.base), set(it.out_code), set(it.aux32), set(it.xline.base), set(it.xaux32), set(it.xstate));
      text += l;
    }
  }
}
}  // namespace host
}  // namespace waa

using namespace waa;
using namespace waa::host;

extern "C" {

const char* waa_last_error(void) { return g_err; }

int32_t waa_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// number_of_outputs / number_of_inputs of a node (audio_node.rs; channel_splitter.rs:136-142, channel_merger.rs:112-118)
static uint32_t node_outputs(const Node& n) { return n.desc.kind == WAA_NODE_CHANNEL_SPLITTER ? (uint32_t)n.desc.i[0] : 1u; }
static uint32_t node_inputs(const Node& n) { return n.desc.kind == WAA_NODE_CHANNEL_MERGER ? (uint32_t)n.desc.i[0] : 1u; }
static int check_ports(const waa_batch* b, uint32_t from, uint32_t from_output, uint32_t to, uint32_t to_input) {
  if (from_output >= node_outputs(b->nodes[from]))
    return fail(WAA_ERR_INVALID_ARGUMENT, "IndexSizeError - output port %u is out of bounds", from_output);
  if (!(to_input & 0x80000000u) && to_input >= node_inputs(b->nodes[to]))
    return fail(WAA_ERR_INVALID_ARGUMENT, "IndexSizeError - input port %u is out of bounds", to_input);
  return 0;
}

// node i of a new batch (its desc is the caller's): channel configuration, AudioParams with the reference's defaults and ranges,
// the constructor's checks of its kind
static int init_node(waa_batch* b, uint32_t i) {
  const uint32_t n_inst = b->n_inst;
  const float sr = b->sr;
  Node& n = b->nodes[i];
  if (n.desc.kind >= WAA_NODE_KIND_COUNT) return fail(WAA_ERR_INVALID_ARGUMENT, "unknown node kind");
  default_channel_config(n, b->n_out);
  if (n.cc < 1 || n.cc > WAA_MAX_CHANNELS)
    return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - Invalid number of channels: %d", n.cc);
  auto P = [&](size_t k) -> ParamStore& {
    if (n.params.size() <= k) n.params.resize(k + 1);
    return n.params[k];
  };
  switch (n.desc.kind) {
    case WAA_NODE_BIQUAD:
      P(WAA_PARAM_BIQUAD_FREQUENCY).init(n_inst, 350.f, 0.f, sr / 2.f);
      P(WAA_PARAM_BIQUAD_DETUNE).init(n_inst, 0.f, -153600.f, 153600.f);
      P(WAA_PARAM_BIQUAD_Q).init(n_inst, 1.f, -FLT_MAX, FLT_MAX);
      P(WAA_PARAM_BIQUAD_GAIN).init(n_inst, 0.f, -FLT_MAX, 40.f * log10f(FLT_MAX));
      if (n.desc.i[0] < 0 || n.desc.i[0] > 7) return fail(WAA_ERR_INVALID_ARGUMENT, "bad biquad type");
      break;
    case WAA_NODE_GAIN: P(0).init(n_inst, 1.f, -FLT_MAX, FLT_MAX); break;
    case WAA_NODE_BUFFER_SOURCE:
      P(WAA_PARAM_SOURCE_PLAYBACK_RATE).init(n_inst, 1.f, -FLT_MAX, FLT_MAX);
      P(WAA_PARAM_SOURCE_DETUNE).init(n_inst, 0.f, -FLT_MAX, FLT_MAX);
      P(WAA_PARAM_SOURCE_PLAYBACK_RATE).k_rate = P(WAA_PARAM_SOURCE_DETUNE).k_rate = true;  // audio_buffer_source.rs:157,168
      n.bufs.resize(n_inst);
      n.sched.resize(n_inst);
      break;
    case WAA_NODE_CONSTANT_SOURCE:
      P(0).init(n_inst, 1.f, -FLT_MAX, FLT_MAX);
      n.sched.resize(n_inst);
      break;
    case WAA_NODE_OSCILLATOR:  // oscillator.rs:210-262
      if (n.desc.i[0] < WAA_OSC_SINE || n.desc.i[0] > WAA_OSC_CUSTOM) return fail(WAA_ERR_INVALID_ARGUMENT, "bad oscillator type");
      P(WAA_PARAM_OSCILLATOR_FREQUENCY).init(n_inst, 440.f, -sr / 2.f, sr / 2.f);
      P(WAA_PARAM_OSCILLATOR_DETUNE).init(n_inst, 0.f, -153600.f, 153600.f);
      n.sched.resize(n_inst);
      break;
    case WAA_NODE_STEREO_PANNER:
      P(0).init(n_inst, 0.f, -1.f, 1.f);
      if (n.mode == WAA_COUNT_MODE_MAX)
        return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - StereoPannerNode channel count mode cannot be set to max");
      if (n.cc > 2)
        return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - StereoPannerNode channel count cannot be greater than two");
      break;
    case WAA_NODE_PANNER: {
      static const float defs[15] = {0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, -1, 0, 1, 0};
      for (int p = 0; p < 15; p++) P(p).init(n_inst, defs[p], -FLT_MAX, FLT_MAX);
      if (n.desc.i[0] == WAA_PANNING_HRTF && !hrtf_sphere_loaded())  // (the reference embeds the database in the crate)
        return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - HRTF panning needs the HRIR sphere (waa_hrtf_load_sphere)");
      if (n.mode == WAA_COUNT_MODE_MAX)
        return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - PannerNode channel count mode cannot be set to max");
      if (n.cc > 2)
        return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - PannerNode channel count cannot be greater than two");
      // PannerOptions (panner.rs:408-428, 20-33); an all-zero d[] block means "the defaults" (panner.rs:146-166)
      if (n.desc.d[0] == 0. && n.desc.d[1] == 0. && n.desc.d[2] == 0. && n.desc.d[3] == 0. && n.desc.d[4] == 0. && n.desc.d[5] == 0.) {
        n.desc.d[0] = 1.;
        n.desc.d[1] = 10000.;
        n.desc.d[2] = 1.;
        n.desc.d[3] = 360.;
        n.desc.d[4] = 360.;
      }
      if (int e = check_panner_values(n.desc.d[0], n.desc.d[1], n.desc.d[2], n.desc.d[5])) return e;
      break;
    }
    case WAA_NODE_DELAY:  // delay.rs:283-335
      if (n.desc.d[0] == 0.) n.desc.d[0] = 1.;
      if (!(n.desc.d[0] > 0. && n.desc.d[0] < 180.))
        return fail(WAA_ERR_NOT_SUPPORTED,
                    "NotSupportedError - maxDelayTime MUST be greater than zero and less than three minutes");
      P(WAA_PARAM_DELAY_DELAY_TIME).init(n_inst, 0.f, 0.f, (float)n.desc.d[0]);
      break;
    case WAA_NODE_WAVESHAPER:
      if (n.desc.i[0] < WAA_OVERSAMPLE_NONE || n.desc.i[0] > WAA_OVERSAMPLE_X4) return fail(WAA_ERR_INVALID_ARGUMENT, "bad oversample type");
      break;
    case WAA_NODE_CONVOLVER:
      if (n.cc > 2)
        return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - ConvolverNode channel count cannot be greater than two");
      if (n.mode == WAA_COUNT_MODE_MAX)
        return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - ConvolverNode channel count mode cannot be set to max");
      if (n.desc.i[1] != 0 && n.desc.i[1] != 1)
        return fail(WAA_ERR_INVALID_ARGUMENT, "ConvolverNode: i[1] is 0 (one impulse response per batch) or 1 (one per instance), got %d", n.desc.i[1]);
      break;
    case WAA_NODE_DYNAMICS_COMPRESSOR: {  // dynamics_compressor.rs:182-247 (and :72-96 for the two constraints)
      if (n.cc > 2)
        return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - DynamicsCompressorNode channel count cannot be greater than two");
      if (n.mode == WAA_COUNT_MODE_MAX)
        return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - DynamicsCompressorNode channel count mode cannot be set to max");
      // the meter: i[0] = 1 keeps reduction() after every quantum (waa_compressor_get_reduction, include/waa_hip_device.h)
      if (n.desc.i[0] != 0 && n.desc.i[0] != 1)
        return fail(WAA_ERR_INVALID_ARGUMENT, "DynamicsCompressorNode %u: i[0] is 0 (no meter) or 1 (keep the reduction trace), got %d", i, n.desc.i[0]);
      P(WAA_PARAM_COMPRESSOR_THRESHOLD).init(n_inst, -24.f, -100.f, 0.f);
      P(WAA_PARAM_COMPRESSOR_KNEE).init(n_inst, 30.f, 0.f, 40.f);
      P(WAA_PARAM_COMPRESSOR_RATIO).init(n_inst, 12.f, 1.f, 20.f);
      P(WAA_PARAM_COMPRESSOR_ATTACK).init(n_inst, 0.003f, 0.f, 1.f);
      P(WAA_PARAM_COMPRESSOR_RELEASE).init(n_inst, 0.25f, 0.f, 1.f);
      for (auto& ps : n.params) ps.k_rate = true;
      break;
    }
    case WAA_NODE_ANALYSER: {
      int fs = n.desc.i[0] ? n.desc.i[0] : 2048;
      if (fs < 32 || fs > 32768 || (fs & (fs - 1)))
        return fail(WAA_ERR_INVALID_ARGUMENT, "IndexSizeError - Invalid fft size: %d is not a power of two", fs);
      n.desc.i[0] = fs;
      if (n.desc.d[0] == 0. && n.desc.d[1] == 0. && n.desc.d[2] == 0.) {
        n.desc.d[0] = 0.8;
        n.desc.d[1] = -100.;
        n.desc.d[2] = -30.;
      }
      if (n.desc.d[0] < 0. || n.desc.d[0] > 1.)
        return fail(WAA_ERR_INVALID_ARGUMENT, "IndexSizeError - Invalid smoothing time constant");
      if (!(n.desc.d[1] < n.desc.d[2])) return fail(WAA_ERR_INVALID_ARGUMENT, "IndexSizeError - Invalid min decibels");
      // a series of pulls: i[1] = hop in quanta (0: one pull per render), i[2] = first pull quantum
      if (n.desc.i[1] < 0 || n.desc.i[2] < 0)
        return fail(WAA_ERR_INVALID_ARGUMENT, "AnalyserNode %u: series hop i[1] = %d and first pull quantum i[2] = %d cannot be negative", i,
                    n.desc.i[1], n.desc.i[2]);
      if (n.desc.i[1] > 0 && n.an_series_pulls(b->n_quanta) == 0)
        return fail(WAA_ERR_INVALID_ARGUMENT, "AnalyserNode %u: no pull of the series falls inside the render (first pull at quantum %d, the render has %u)",
                    i, n.desc.i[2], b->n_quanta);
      break;
    }
    case WAA_NODE_CHANNEL_SPLITTER: {  // ChannelSplitterNode::new, channel_splitter.rs:146-161
      if (n.desc.i[0] == 0) n.desc.i[0] = WAA_DEFAULT_NUMBER_OF_PORTS;
      if (n.desc.i[0] < 1 || n.desc.i[0] > WAA_MAX_CHANNELS)
        return fail(WAA_ERR_INVALID_ARGUMENT, "IndexSizeError - Invalid number of channels: %d is outside range [1, %d]", n.desc.i[0], WAA_MAX_CHANNELS);
      if (n.desc.channel_count != 0) {
        // (a count that was "explicitly set" is one that differs from the default of 6, :152)
        if (n.desc.channel_count != WAA_DEFAULT_NUMBER_OF_PORTS && (int)n.desc.channel_count != n.desc.i[0])
          return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - channel count of ChannelSplitterNode must be equal to number of outputs");
        if (n.mode != WAA_COUNT_MODE_EXPLICIT)
          return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - channel count of ChannelSplitterNode must be set to Explicit");
        if (n.interp != WAA_INTERP_DISCRETE)
          return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - channel interpretation of ChannelSplitterNode must be set to Discrete");
      }
      n.cc = n.desc.i[0];
      n.mode = WAA_COUNT_MODE_EXPLICIT;
      n.interp = WAA_INTERP_DISCRETE;
      break;
    }
    case WAA_NODE_CHANNEL_MERGER: {  // ChannelMergerNode::new, channel_merger.rs:122-127
      if (n.desc.i[0] == 0) n.desc.i[0] = WAA_DEFAULT_NUMBER_OF_PORTS;
      if (n.desc.i[0] < 1 || n.desc.i[0] > WAA_MAX_CHANNELS)
        return fail(WAA_ERR_INVALID_ARGUMENT, "IndexSizeError - Invalid number of channels: %d is outside range [1, %d]", n.desc.i[0], WAA_MAX_CHANNELS);
      if (n.cc != 1) return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - channel count of ChannelMergerNode must be equal to 1");
      if (n.mode != WAA_COUNT_MODE_EXPLICIT)
        return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - channel count of ChannelMergerNode must be set to Explicit");
      break;
    }
    default: break;
  }
  return 0;
}

// Once per process and device: the first host-to-device copy out of pageable memory makes the runtime set up its staging
// buffers (6-7 ms on the GPU boxes: bench.py's first workload reported them as "uploads 6.9 ms" of a 10 ms first render).
// A process pays that once whatever it does first; paid here, at context creation, it is not part of the first
// start_rendering_sync.
static void warm_up_staging(int device) {
  static std::mutex warm_lock;
  static std::set<int> warm;
  std::lock_guard<std::mutex> l(warm_lock);
  if (warm.count(device)) return;
  // (the very calls dev_upload makes: a synchronous copy of a table-sized block out of pageable memory + the null stream's
  // synchronisation; a 4 KB asynchronous copy on the batch's stream did not take the same path — r05c: still 7.0 ms)
  void* d = nullptr;
  if (hipMalloc(&d, 256 * 1024) == hipSuccess) {
    std::vector<char> h(256 * 1024, 0);
    for (size_t bytes : {(size_t)512, (size_t)64 * 1024, (size_t)256 * 1024}) {
      (void)hipMemcpy(d, h.data(), bytes, hipMemcpyHostToDevice);
      (void)hipStreamSynchronize(nullptr);
    }
    (void)hipFree(d);
  }
  warm.insert(device);
}

waa_status waa_batch_create(const waa_graph_desc* g, uint32_t n_inst, uint32_t n_out, uint64_t length, float sr,
                            int32_t device, waa_batch** out) {
  if (!g || !out || g->n_nodes == 0 || n_inst == 0) return fail(WAA_ERR_INVALID_ARGUMENT, "invalid arguments");
  if (g->nodes[0].kind != WAA_NODE_DESTINATION) return fail(WAA_ERR_INVALID_ARGUMENT, "node 0 must be the destination");
  if (n_out == 0 || n_out > WAA_MAX_CHANNELS)
    return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - Invalid number of channels: %u", n_out);
  if (length == 0)  // assert_valid_buffer_length, src/lib.rs:222-228
    return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - Invalid length: 0 is less than or equal to minimum bound (0)");
  if (int e = check_sample_rate(sr)) return e;
  std::unique_ptr<waa_batch> b(new waa_batch);
  b->n_inst = n_inst;
  b->n_out = n_out;
  b->length = length;
  b->sr = sr;
  b->n_quanta = (uint32_t)((length + RQ - 1) / RQ);
  if (b->n_quanta == 0) b->n_quanta = 1;
  b->n_tiles = (b->n_quanta + QUANTA_PER_TILE - 1) / QUANTA_PER_TILE;
  b->lp = (uint64_t)b->n_tiles * TILE;
  for (uint32_t e = 0; e < g->n_edges; e++) {
    const waa_edge_desc& ed = g->edges[e];
    if (ed.from >= g->n_nodes || ed.to >= g->n_nodes) return fail(WAA_ERR_INVALID_ARGUMENT, "IndexSizeError - invalid edge %u", e);
    b->edges.push_back(ed);
  }
  b->edge_on.assign(b->edges.size(), 0u);
  b->edge_off.assign(b->edges.size(), EDGE_NEVER);
  b->n_user_nodes = g->n_nodes;
  b->nodes.resize(g->n_nodes);
  for (uint32_t i = 0; i < g->n_nodes; i++) {
    b->nodes[i].desc = g->nodes[i];
    if (int e = init_node(b.get(), i)) return e;
  }
  // AudioNode::connect_from_output_to_input, audio_node.rs:270-279 (the nodes' port counts are known by now)
  for (const waa_edge_desc& ed : b->edges)
    if (int e = check_ports(b.get(), ed.from, ed.from_output, ed.to, ed.to_input)) return e;
  if (device == WAA_DEVICE_PLAN_ONLY) {
    b->dry = true;
    b->device = -1;
    *out = b.release();
    return WAA_OK;
  }
  // the device is only touched from here on; a machine without a GPU still validates graphs above
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(WAA_ERR_DEVICE, "no HIP device available: libwaa_hip has no CPU fallback");
  if (device >= 0) {
    if (device >= ndev) return fail(WAA_ERR_INVALID_ARGUMENT, "device %d out of range (%d devices)", device, ndev);
    HIP_TRY(hipSetDevice(device));
    b->device = device;
  } else {
    HIP_TRY(hipGetDevice(&b->device));
  }
  HIP_TRY(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, b->device) == hipSuccess && cus > 0) b->n_cu = cus;
  }
  warm_up_staging(b->device);
  *out = b.release();
  return WAA_OK;
}

void waa_batch_destroy(waa_batch* b) {
  if (!b) return;
  if (b->dry) {
    for (void* p : b->allocs) std::free(p);
    for (void* p : b->payload_allocs) std::free(p);
    delete b;
    return;
  }
  if (b->stream) {
    (void)hipStreamSynchronize(b->stream);
    for (auto& p : b->prof)
      for (auto& ev : p.pending) {
        (void)hipEventDestroy(ev.first);
        (void)hipEventDestroy(ev.second);
      }
    for (void* p : b->allocs)
      if (!arena_free(b->device, p)) (void)hipFree(p);
    for (void* p : b->payload_allocs)
      if (!arena_free(b->device, p)) (void)hipFree(p);
    if (b->stage) (void)hipHostFree(b->stage);
    (void)hipStreamDestroy(b->stream);
  }
  delete b;
}

waa_status waa_plan_describe(waa_batch* b, char* buf, size_t cap, size_t* needed) {
  if (!b) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch");
  if (!b->planned) {
    if (!b->dry) HIP_TRY(hipSetDevice(b->device));
    int e = plan_batch(b);
    if (e) return e;
  }
  std::string text;
  char head[256];
  snprintf(head, sizeof head, "batch: %u instance(s) x %llu frames (%u quanta, %u tiles of %d) @ %g Hz, %u output channel(s)\n",
           b->n_inst, (unsigned long long)b->length, b->n_quanta, b->n_tiles, TILE, (double)b->sr, b->n_out);
  text += head;
  // (same line as the header: the plan lines below are positional in tests/test_plan.py)
  text.pop_back();
  snprintf(head, sizeof head, " | timing: build_plan %.2f ms = hipMalloc %.2f ms (%llu calls, %.3f GB) + uploads %.2f ms + host planning %.2f ms\n",
           b->t_plan_ms, b->plan_alloc_ms, (unsigned long long)b->plan_n_alloc, (double)b->plan_alloc_bytes / 1e9, b->plan_upload_ms,
           b->t_plan_ms - b->plan_alloc_ms - b->plan_upload_ms);
  text += head;
  for (auto& l : b->plan_log) text += l + "\n";
  if (measure_switch("WAA_PLAN_LAUNCHES")) {
    // the launch list itself, one positional line per step (no pointers): what the planner's loop handling and fusions decide
    // and the plan log does not show (tests/test_launch_list.py)
    char line[320];
    for (size_t k = 0; k < b->steps.size(); k++) {
      const Step& st = b->steps[k];
      snprintf(line, sizeof line, "launch %zu: kind %d %s group=%d qgroup=%d prologue=%d fused=%d ff=%d fb=%d tail=%d cmax=%d slots=%d,%d,%d,%d\n", k,
               (int)st.kind, step_traits(st.kind).name, st.group, st.qgroup, (int)st.prologue, (int)st.echo_fused, (int)st.echo_ff, st.echo_fb,
               st.echo_tail_step, st.cmax, st.profile_slot, st.slot_fwd, st.slot_mac, st.slot_inv);
      text += line;
    }
    text += "group_tiles:";
    for (uint32_t t : b->group_tiles) text += " " + std::to_string(t);
    text += "\nqgroup_quanta:";
    for (uint32_t q : b->qgroup_quanta) text += " " + std::to_string(q);
    text += "\n";
  }
  if (b->dry && measure_switch("WAA_PLAN_DYN_ITEMS")) describe_dyn_items(b, text);
  if (needed) *needed = text.size();
  if (buf && cap) {
    const size_t n = std::min(cap - 1, text.size());
    std::memcpy(buf, text.data(), n);
    buf[n] = 0;
  }
  return WAA_OK;
}

// A serving loop renders the same graph over and over with new audio: the batch keeps its plan, its device buffers and its tables;
// waa_source_set_buffer_batch / _pcm16_batch / waa_source_adopt_device then REFILL the source buffers of the shape the batch was
// planned with (anything else is an InvalidStateError), and waa_render renders from the initial state as every render does.
// A plan that holds values rendered from the graph at plan time (resolve_source_rate_modulation: a source's playbackRate / detune
// or a panner's position / orientation driven from the graph) is refused: those values came from the old audio, and re-planning
// here would break the promise of no plan and no allocation.
waa_status waa_batch_rearm(waa_batch* b) {
  if (!b) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch");
  if (b->dry) return fail(WAA_ERR_DEVICE, "plan-only batch has no device");
  if (!b->planned) return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - nothing to re-arm: the batch has not been planned (waa_render / waa_plan_describe)");
  if (!b->prepass_note.empty())
    return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - cannot re-arm: the plan holds param values rendered from the graph at plan time "
                                       "(source playbackRate / detune or panner position / orientation driven from the graph), which new "
                                       "audio may change: create a new batch");
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipStreamSynchronize(b->stream));  // (the previous render and its downloads are over before its inputs are overwritten)
  b->rearmed = true;
  b->rendered = false;
  b->pending_fills.clear();
  return WAA_OK;
}

// The quantum loop of render_audiobuffer_sync with its suspend points (thread.rs:277-294; OfflineAudioContext::suspend_sync,
// offline.rs:359-397).  The engine renders node-major, not quantum-major, so a range is not rendered when it is asked for: the
// call moves the CONTROL CLOCK to quantum0 + n_quanta, every control call made before the next one (waa_connect /
// waa_disconnect, param values and automation, start / stop) is recorded with the quantum in front of which the reference's
// render thread would have handled it, and the call that reaches the last quantum plans the graph WITH its history and renders
// all of it.  What a suspend callback cannot do through this ABI is read rendered audio (an analyser pull before the last range
// is an InvalidStateError): a host that needs that renders a shorter batch of the graph as it is so far
// (api.py::OfflineAudioContext does).
waa_status waa_render_range(waa_batch* b, uint64_t quantum0, uint32_t n_quanta) {
  if (!b) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch");
  // (a batch that has been PLANNED in front of its last range — waa_plan_describe at the last suspend point — may still render it)
  if (b->planned && !(quantum0 == b->ctl_q && quantum0 + n_quanta == b->n_quanta && !b->rendered))
    return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - the batch is frozen once rendering has started");
  if (quantum0 != b->ctl_q)
    return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - ranges are consecutive: the next one starts at quantum %u, not %llu", b->ctl_q,
                (unsigned long long)quantum0);
  if (n_quanta == 0 || quantum0 + n_quanta > b->n_quanta)
    return fail(WAA_ERR_INVALID_ARGUMENT, "RangeError - quanta [%llu, %llu) of a render of %u", (unsigned long long)quantum0,
                (unsigned long long)(quantum0 + n_quanta), b->n_quanta);
  b->ranged = true;
  b->ctl_q = (uint32_t)(quantum0 + n_quanta);
  if (b->ctl_q < b->n_quanta) return WAA_OK;
  return waa_render(b);
}

static int check_edge(waa_batch* b, uint32_t from, uint32_t from_output, uint32_t to, uint32_t to_input) {
  if (!b) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch");
  if (from >= b->n_user_nodes || to >= b->n_user_nodes)
    return fail(WAA_ERR_INVALID_ARGUMENT, "IndexSizeError - invalid edge %u:%u -> %u:%u", from, from_output, to, to_input);
  if (int e = check_ports(b, from, from_output, to, to_input)) return e;
  if ((to_input & 0x80000000u) && (to_input & 0x7fffffffu) >= b->nodes[to].params.size())
    return fail(WAA_ERR_INVALID_ARGUMENT, "no such param %u on node %u", to_input & 0x7fffffffu, to);
  return check_unplanned(b);
}

// AudioNode::connect_from_output_to_input (audio_node.rs:247-289) after the batch was created — at a suspend point when the
// control clock has moved.  Connecting what is connected already is a no-op, as in the reference (graph.rs add_edge on a set).
waa_status waa_connect(waa_batch* b, uint32_t from, uint32_t from_output, uint32_t to, uint32_t to_input) {
  if (int e = check_edge(b, from, from_output, to, to_input)) return e;
  for (size_t k = 0; k < b->edges.size(); k++) {
    const waa_edge_desc& ed = b->edges[k];
    if (ed.from == from && ed.from_output == from_output && ed.to == to && ed.to_input == to_input && b->edge_off[k] == EDGE_NEVER) return WAA_OK;
  }
  b->edges.push_back(waa_edge_desc{from, from_output, to, to_input});
  b->edge_on.push_back(b->ctl_q);
  b->edge_off.push_back(EDGE_NEVER);
  return WAA_OK;
}

// AudioNode::disconnect_dest_from_output_to_input (audio_node.rs:341-420): the connection must exist
waa_status waa_disconnect(waa_batch* b, uint32_t from, uint32_t from_output, uint32_t to, uint32_t to_input) {
  if (int e = check_edge(b, from, from_output, to, to_input)) return e;
  for (size_t k = b->edges.size(); k-- > 0;) {
    const waa_edge_desc& ed = b->edges[k];
    if (!(ed.from == from && ed.from_output == from_output && ed.to == to && ed.to_input == to_input) || b->edge_off[k] != EDGE_NEVER) continue;
    if (b->edge_on[k] >= b->ctl_q) {  // made and cut at the same point: it never carried a quantum
      b->edges.erase(b->edges.begin() + (long)k);
      b->edge_on.erase(b->edge_on.begin() + (long)k);
      b->edge_off.erase(b->edge_off.begin() + (long)k);
    } else {
      b->edge_off[k] = b->ctl_q;
    }
    return WAA_OK;
  }
  return fail(WAA_ERR_INVALID_ARGUMENT, "InvalidAccessError - attempting to disconnect unconnected nodes");
}

waa_status waa_render(waa_batch* b) {
  if (!b) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch");
  if (b->ranged && b->ctl_q < b->n_quanta)
    return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - a ranged render is in progress (suspended in front of quantum %u): waa_render_range renders the rest", b->ctl_q);
  if (b->dry) return fail(WAA_ERR_DEVICE, "plan-only batch (WAA_DEVICE_PLAN_ONLY) cannot render: there is no CPU fallback");
  HIP_TRY(hipSetDevice(b->device));
  if (!b->planned) {
    int e = plan_batch(b);
    if (e) return e;
  }
  b->rendered = true;
  return run_steps(b);
}

static int drain_profile(waa_batch* b) {
  for (auto& p : b->prof) {
    for (auto& ev : p.pending) {
      float ms = 0.f;
      HIP_TRY(hipEventSynchronize(ev.second));
      HIP_TRY(hipEventElapsedTime(&ms, ev.first, ev.second));
      p.total_ms += (double)ms;
      p.launches++;
      (void)hipEventDestroy(ev.first);
      (void)hipEventDestroy(ev.second);
    }
    p.pending.clear();
  }
  return 0;
}

// Debugging aid of the dynamic-count path (WAA_DUMP_CODES=<file>): the per-quantum codes (count | 0x80 if silent) of every
// node's published signal, [n_inst][n_nodes][n_quanta] behind a 3-word header; 0xFF where a node has no code table.
static int dump_codes(waa_batch* b) {
  const char* path = measure_switch("WAA_DUMP_CODES");
  if (!path || !b->dynamic) return 0;
  const uint32_t N = (uint32_t)b->nodes.size(), nq = b->n_quanta;
  std::vector<uint8_t> all((size_t)b->n_inst * N * nq, 0xFF), tab((size_t)b->n_inst * b->code_stride);
  for (uint32_t id = 0; id < N; id++) {
    if (!b->nodes[id].code) continue;
    HIP_TRY(hipMemcpy(tab.data(), b->nodes[id].code, tab.size(), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < b->n_inst; i++)
      std::memcpy(&all[((size_t)i * N + id) * nq], &tab[(size_t)i * b->code_stride], nq);
  }
  if (FILE* f = fopen(path, "wb")) {
    const uint32_t hdr[3] = {b->n_inst, N, nq};
    fwrite(hdr, sizeof hdr, 1, f);
    fwrite(all.data(), 1, all.size(), f);
    fclose(f);
  }
  return 0;
}

waa_status waa_sync(waa_batch* b) {
  if (!b) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch");
  if (b->dry) return fail(WAA_ERR_DEVICE, "plan-only batch has no device");
  HIP_TRY(hipStreamSynchronize(b->stream));
  if (int es = settle_loops(b)) return es;
  if (b->scan_counter) {  // a bounded spin of the chained scan gave up: the render is not to be trusted
    uint32_t words[1] = {0};
    HIP_TRY(hipMemcpy(words, b->scan_counter + 8 * 16, sizeof words, hipMemcpyDeviceToHost));
    if (words[0]) return fail(WAA_ERR_DEVICE, "internal: the time-parallel biquad gave up waiting for a predecessor tile");
  }
  if (int e = dump_codes(b)) return e;
  return drain_profile(b);
}

waa_status waa_download(waa_batch* b, uint32_t inst, uint32_t ch, float* dst, uint64_t frames) {
  if (!b || inst >= b->n_inst || ch >= b->n_out || frames > b->length)
    return fail(WAA_ERR_INVALID_ARGUMENT, "download out of range");
  if (!b->planned || !b->rendered) return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - nothing rendered yet");
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipStreamSynchronize(b->stream));
  if (int es = settle_loops(b)) return es;
  const SignalRef& s = b->nodes[0].sig;
  if ((int)ch < s.nch) {
    if (int e = xfer_d2h(b, dst, frames * sizeof(float), s.base + (size_t)inst * s.inst_stride + (size_t)ch * s.ch_stride, frames * sizeof(float),
                         frames * sizeof(float), 1))
      return e;
    HIP_TRY(hipStreamSynchronize(b->stream));
  } else {
    std::memset(dst, 0, frames * sizeof(float));
  }
  return WAA_OK;
}

waa_status waa_download_all(waa_batch* b, float* dst) {
  if (!b) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch");
  if (!b->planned || !b->rendered) return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - nothing rendered yet");
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipStreamSynchronize(b->stream));
  if (int es = settle_loops(b)) return es;
  const SignalRef& s = b->nodes[0].sig;
  if (b->length == 0) return WAA_OK;
  if ((uint32_t)s.nch == b->n_out) {
    if (int e = xfer_d2h(b, dst, b->length * sizeof(float), s.base, s.ch_stride * sizeof(float), b->length * sizeof(float), (size_t)b->n_inst * b->n_out))
      return e;
    HIP_TRY(hipStreamSynchronize(b->stream));
  } else {
    for (uint32_t i = 0; i < b->n_inst; i++)
      for (uint32_t c = 0; c < b->n_out; c++) {
        int e = waa_download(b, i, c, dst + ((size_t)i * b->n_out + c) * b->length, b->length);
        if (e) return e;
      }
  }
  return WAA_OK;
}

waa_status waa_output_device(waa_batch* b, const float** p, uint64_t* is, uint64_t* cs) {
  if (!b || !b->planned) return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - nothing rendered yet");
  const SignalRef& s = b->nodes[0].sig;
  *p = s.base;
  *is = s.inst_stride;
  *cs = s.ch_stride;
  return WAA_OK;
}

waa_status waa_profile_enable(waa_batch* b, int32_t on) {
  if (!b) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch");
  b->profiling = on != 0;
  return WAA_OK;
}
int32_t waa_profile_count(waa_batch* b) { return b ? (int32_t)b->prof.size() : 0; }
waa_status waa_profile_get(waa_batch* b, int32_t i, const char** name, uint64_t* launches, double* ms) {
  if (!b || i < 0 || i >= (int32_t)b->prof.size()) return fail(WAA_ERR_INVALID_ARGUMENT, "profile index out of range");
  *name = b->prof[i].name.c_str();
  *launches = b->prof[i].launches;
  *ms = b->prof[i].total_ms;
  return WAA_OK;
}
waa_status waa_profile_reset(waa_batch* b) {
  if (!b) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch");
  for (auto& p : b->prof) {
    p.launches = 0;
    p.total_ms = 0;
    // ... and the event pairs of launches not yet folded into the totals (they are resolved lazily by waa_profile_get):
    // a reset after warm-up launches must not leave them to be counted with the timed ones (bench.py, round 4)
    for (auto& ev : p.pending) {
      (void)hipEventDestroy(ev.first);
      (void)hipEventDestroy(ev.second);
    }
    p.pending.clear();
  }
  return WAA_OK;
}

}  // extern "C"
