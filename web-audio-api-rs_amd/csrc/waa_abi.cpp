// waa_abi.cpp — the C ABI of libwaa_hip.so (include/waa_hip.h): batch construction and validation (the reference's
// panics become status codes with the same message text), payload uploads, render, download, analyser pulls,
// control-side helpers, profiling.  All sample arithmetic happens in the HIP kernels; there is no CPU fallback:
// without a HIP device every render call fails with WAA_ERR_DEVICE.
#include <map>
#include <mutex>
#include <set>

#include "../../include/waa_hip_device.h"
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
}  // namespace host
}  // namespace waa

using namespace waa;
using namespace waa::host;

// =======================================================================================
// C ABI
// =======================================================================================
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

waa_status waa_batch_create(const waa_graph_desc* g, uint32_t n_inst, uint32_t n_out, uint64_t length, float sr,
                            int32_t device, waa_batch** out) {
  if (!g || !out || g->n_nodes == 0 || n_inst == 0) return fail(WAA_ERR_INVALID_ARGUMENT, "invalid arguments");
  if (g->nodes[0].kind != WAA_NODE_DESTINATION) return fail(WAA_ERR_INVALID_ARGUMENT, "node 0 must be the destination");
  if (n_out == 0 || n_out > WAA_MAX_CHANNELS)
    return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - Invalid number of channels: %u", n_out);
  if (length == 0)  // assert_valid_buffer_length, src/lib.rs:222-228
    return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - Invalid length: 0 is less than or equal to minimum bound (0)");
  if (!(sr >= 3000.f && sr <= 768000.f))  // MIN/MAX_SAMPLE_RATE, src/lib.rs:149-160
    return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - Invalid sample rate: %f", sr);
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
    Node& n = b->nodes[i];
    n.desc = g->nodes[i];
    if (n.desc.kind >= WAA_NODE_KIND_COUNT) return fail(WAA_ERR_INVALID_ARGUMENT, "unknown node kind");
    default_channel_config(n, n_out);
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
        if (!(n.desc.d[0] >= 0.)) return fail(WAA_ERR_INVALID_ARGUMENT, "RangeError - refDistance cannot be negative");
        if (!(n.desc.d[1] > 0.)) return fail(WAA_ERR_INVALID_ARGUMENT, "RangeError - maxDistance must be strictly positive");
        if (!(n.desc.d[2] >= 0.)) return fail(WAA_ERR_INVALID_ARGUMENT, "RangeError - rolloffFactor cannot be negative");
        if (!(n.desc.d[5] >= 0. && n.desc.d[5] <= 1.))
          return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - coneOuterGain must be in the range [0, 1]");
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
  {
    // Once per process and device: the first host-to-device copy out of pageable memory makes the runtime set up its staging
    // buffers (6-7 ms on the GPU boxes: bench.py's first workload reported them as "uploads 6.9 ms" of a 10 ms first render).
    // A process pays that once whatever it does first; paid here, at context creation, it is not part of the first
    // start_rendering_sync.
    static std::mutex warm_lock;
    static std::set<int> warm;
    std::lock_guard<std::mutex> l(warm_lock);
    if (!warm.count(b->device)) {
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
      warm.insert(b->device);
    }
  }
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

int waa_internal_xfer_h2d(waa_batch* b, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height);
int waa_internal_xfer_d2h(waa_batch* b, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height);

static int upload_buffer(waa_batch* b, const float* const* channels, uint32_t n_ch, uint64_t frames, float sr,
                         DeviceBuffer* out) {
  const uint64_t stride = (frames + 3) / 4 * 4;
  float* d = nullptr;
  int e = dev_alloc(b, &d, (size_t)n_ch * std::max<uint64_t>(stride, 4), true);
  if (e) return e;
  for (uint32_t c = 0; c < n_ch; c++)
    if (frames) {
      if (b->dry) {
        std::memcpy(d + (size_t)c * stride, channels[c], frames * sizeof(float));
      } else {
        if (int e2 = waa_internal_xfer_h2d(b, d + (size_t)c * stride, frames * sizeof(float), channels[c], frames * sizeof(float), frames * sizeof(float), 1)) return e2;
        HIP_TRY(hipStreamSynchronize(b->stream));
      }
    }
  out->base = d;
  out->ch_stride = stride;
  out->frames = frames;
  out->nch = n_ch;
  out->sr = sr;
  out->valid = true;
  return 0;
}

// ---- transfers between CALLER memory and the device --------------------------------------------------------------------------
// Pinned caller memory (hipHostMalloc / hipHostRegister: what a host that cares about the link hands over — bench.py, the sharded
// path) is copied directly.  PAGEABLE caller memory (a numpy array, a Rust Vec) goes through a pinned block of the batch: the runtime
// would otherwise lock the caller's pages on the fly and let its copy kernels read / write them in place — and a destination that
// has just been mapped and never touched (numpy's np.empty, a fresh Vec) is exactly what the round-6 campaigns saw go wrong under
// several processes (one download that never arrived: a render "of zeros"; "Memory access fault by GPU ... Write access to a
// read-only page").  Through the staging block the GPU only ever touches memory this library pinned.
namespace {
constexpr size_t STAGE_BYTES = 8u << 20;
bool caller_memory_is_pinned(const void* p) {
  hipPointerAttribute_t a{};
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeHost;
}
int stage_of(waa_batch* b, char** out) {
  if (!b->stage) HIP_TRY(hipHostMalloc(&b->stage, STAGE_BYTES, hipHostMallocDefault));
  *out = static_cast<char*>(b->stage);
  return 0;
}
}  // namespace
// `height` rows of `width` bytes, pitches in bytes; asynchronous on the batch's stream for pinned memory, complete on return otherwise
int waa_internal_xfer_h2d(waa_batch* b, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height) {
  if (!width || !height) return 0;
  if (caller_memory_is_pinned(src)) {
    if (dpitch == width && spitch == width)
      HIP_TRY(hipMemcpyAsync(dst, src, width * height, hipMemcpyHostToDevice, b->stream));
    else
      HIP_TRY(copy2d_async(b->device, dst, dpitch, src, spitch, width, height, hipMemcpyHostToDevice, b->stream));
    return 0;
  }
  char* st = nullptr;
  if (int e = stage_of(b, &st)) return e;
  for (size_t r = 0; r < height;) {
    if (width > STAGE_BYTES) {  // a row longer than the block: in pieces
      for (size_t o = 0; o < width; o += STAGE_BYTES) {
        const size_t n = std::min(STAGE_BYTES, width - o);
        std::memcpy(st, static_cast<const char*>(src) + r * spitch + o, n);
        HIP_TRY(hipMemcpyAsync(static_cast<char*>(dst) + r * dpitch + o, st, n, hipMemcpyHostToDevice, b->stream));
        HIP_TRY(hipStreamSynchronize(b->stream));
      }
      r++;
      continue;
    }
    const size_t rows = std::min(height - r, STAGE_BYTES / width);
    for (size_t k = 0; k < rows; k++) std::memcpy(st + k * width, static_cast<const char*>(src) + (r + k) * spitch, width);
    if (dpitch == width)
      HIP_TRY(hipMemcpyAsync(static_cast<char*>(dst) + r * dpitch, st, rows * width, hipMemcpyHostToDevice, b->stream));
    else
      HIP_TRY(copy2d_async(b->device, static_cast<char*>(dst) + r * dpitch, dpitch, st, width, width, rows, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    r += rows;
  }
  return 0;
}
int waa_internal_xfer_d2h(waa_batch* b, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height) {
  if (!width || !height) return 0;
  if (caller_memory_is_pinned(dst)) {
    if (dpitch == width && spitch == width)
      HIP_TRY(hipMemcpyAsync(dst, src, width * height, hipMemcpyDeviceToHost, b->stream));
    else
      HIP_TRY(copy2d_async(b->device, dst, dpitch, src, spitch, width, height, hipMemcpyDeviceToHost, b->stream));
    return 0;
  }
  char* st = nullptr;
  if (int e = stage_of(b, &st)) return e;
  for (size_t r = 0; r < height;) {
    if (width > STAGE_BYTES) {
      for (size_t o = 0; o < width; o += STAGE_BYTES) {
        const size_t n = std::min(STAGE_BYTES, width - o);
        HIP_TRY(hipMemcpyAsync(st, static_cast<const char*>(src) + r * spitch + o, n, hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(hipStreamSynchronize(b->stream));
        std::memcpy(static_cast<char*>(dst) + r * dpitch + o, st, n);
      }
      r++;
      continue;
    }
    const size_t rows = std::min(height - r, STAGE_BYTES / width);
    if (spitch == width)
      HIP_TRY(hipMemcpyAsync(st, static_cast<const char*>(src) + r * spitch, rows * width, hipMemcpyDeviceToHost, b->stream));
    else
      HIP_TRY(copy2d_async(b->device, st, width, static_cast<const char*>(src) + r * spitch, spitch, width, rows, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    for (size_t k = 0; k < rows; k++) std::memcpy(static_cast<char*>(dst) + (r + k) * dpitch, st + k * width, width);
    r += rows;
  }
  return 0;
}

// The data movement of a batch-wide source buffer (waa_source_set_buffer_batch / _pcm16_batch), apart from its allocation:
// waa_render_sharded registers the buffers first, plans, and fills them when the sub-batch has its turn on the link.
static int fill_upload(waa_batch* b, const waa_batch::PendingFill& f) {
  if (f.kind == 0) {
    // on the batch's own stream (and waited for: the caller may free `data` on return): blocking copies on the null
    // stream of several host threads serialise, and the upload of one sub-batch could not overlap the download of
    // another (PCIe is full duplex) — SURVEY 8(e)
    // (contiguous on both sides -> a plain 1-D copy: those go through the DMA engines, one per direction; pitched 2-D
    // copies run as a copy kernel and did not overlap with a download on another stream)
    if (int e = waa_internal_xfer_h2d(b, f.planes, f.stride * sizeof(float), f.host, f.frames * sizeof(float), f.frames * sizeof(float), (size_t)f.n_items * f.n_ch))
      return e;
    HIP_TRY(hipStreamSynchronize(b->stream));
    return 0;
  }
  const size_t bytes = (size_t)f.n_items * f.frames * f.n_ch * sizeof(int16_t);
  if (int e = waa_internal_xfer_h2d(b, f.staging, bytes, f.host, bytes, bytes, 1)) return e;
  hipError_t he = hipSuccess;
  {
    const bool same = std::fabs(f.src_sr - b->sr) <= 0.1f;
    waa::DecodeDesc dd{};
    dd.pcm = f.staging;
    dd.out = f.planes;
    dd.frames = f.frames;
    dd.target_frames = f.target;
    dd.out_item_stride = (uint64_t)f.n_ch * f.stride;
    dd.out_ch_stride = f.stride;
    dd.nch = f.n_ch;
    dd.n_items = f.n_items;
    dd.resample = same ? 0 : 1;
    dd.scale = 1.f;
    waa::launch_pcm16_resample(dd, b->stream);
    he = hipGetLastError();
  }
  if (he == hipSuccess) he = hipStreamSynchronize(b->stream);
  if (he != hipSuccess) return fail(WAA_ERR_DEVICE, "HIP error %s in the PCM decode path", hipGetErrorString(he));
  return 0;
}
extern "C++" {
namespace waa {
namespace host {
int fill_pending_uploads(waa_batch* b) {
  HIP_TRY(hipSetDevice(b->device));
  for (const auto& f : b->pending_fills)
    if (int e = fill_upload(b, f)) return e;
  b->pending_fills.clear();
  return 0;
}
}  // namespace host
}  // namespace waa
}  // extern "C++"

waa_status waa_source_set_buffer(waa_batch* b, uint32_t node, uint32_t inst, const float* const* channels,
                                 uint32_t n_ch, uint64_t frames, float sr) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_BUFFER_SOURCE)) || (e = check_inst(b, inst)) || (e = check_unplanned(b))) return e;
  if (n_ch == 0 || n_ch > WAA_MAX_CHANNELS) return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - Invalid number of channels");
  if (!b->dry) HIP_TRY(hipSetDevice(b->device));
  DeviceBuffer db;
  if ((e = upload_buffer(b, channels, n_ch, frames, sr, &db))) return e;
  Node& n = b->nodes[node];
  uint32_t lo = inst == WAA_ALL_INSTANCES ? 0 : inst, hi = inst == WAA_ALL_INSTANCES ? b->n_inst : inst + 1;
  for (uint32_t k = lo; k < hi; k++) n.bufs[k] = db;
  return WAA_OK;
}

// A re-armed batch (waa_batch_rearm) takes the next AudioBuffers of a source into the device buffers it was planned with
static int refill_source(waa_batch* b, uint32_t node, int kind, const void* data, uint32_t n_ch, uint64_t frames, float sr) {
  auto it = b->batch_fills.find(node);
  if (it == b->batch_fills.end() || it->second.kind != kind || it->second.n_ch != n_ch || it->second.frames != frames || it->second.src_sr != sr)
    return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - a re-armed batch takes source buffers of the shape it was planned with (node %u)", node);
  HIP_TRY(hipSetDevice(b->device));
  waa_batch::PendingFill pf = it->second;
  pf.host = data;
  if (b->defer_fill) {
    b->pending_fills.push_back(pf);
    return 0;
  }
  return fill_upload(b, pf);
}

waa_status waa_source_set_buffer_batch(waa_batch* b, uint32_t node, const float* data, uint32_t n_ch, uint64_t frames,
                                       float sr) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_BUFFER_SOURCE))) return e;
  if (b->planned && b->rearmed) return refill_source(b, node, 0, data, n_ch, frames, sr);
  if ((e = check_unplanned(b))) return e;
  if (n_ch == 0 || n_ch > WAA_MAX_CHANNELS) return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - Invalid number of channels");
  if (!b->dry) HIP_TRY(hipSetDevice(b->device));
  const uint64_t stride = (frames + 3) / 4 * 4;
  float* d = nullptr;
  if ((e = dev_alloc(b, &d, (size_t)b->n_inst * n_ch * std::max<uint64_t>(stride, 4), true))) return e;
  if (frames && !b->dry) {
    waa_batch::PendingFill pf{0, data, d, nullptr, b->n_inst, n_ch, frames, stride, frames, sr};
    b->batch_fills[node] = pf;
    if (b->defer_fill)
      b->pending_fills.push_back(pf);
    else if ((e = fill_upload(b, pf)))
      return e;
  }
  Node& n = b->nodes[node];
  for (uint32_t k = 0; k < b->n_inst; k++) {
    DeviceBuffer db;
    db.base = d + (size_t)k * n_ch * stride;
    db.ch_stride = stride;
    db.frames = frames;
    db.nch = n_ch;
    db.sr = sr;
    db.valid = true;
    n.bufs[k] = db;
  }
  return WAA_OK;
}

// BaseAudioContext::decode_audio_data_sync for decoded 16-bit PCM (decoding.rs:15-54): sample conversion and
// AudioBuffer::resample to the context's rate run on the device (waa_decode.hip); `planes` = [n_items][n_ch][stride]
static int decode_pcm16(waa_batch* b, const int16_t* pcm, uint32_t n_items, uint32_t n_ch, uint64_t frames, float src_sr,
                        float** planes, uint64_t* stride_out, uint64_t* target_out) {
  const bool same = std::fabs(src_sr - b->sr) <= 0.1f || frames == 0;  // buffer.rs:315-324
  const uint64_t target = same ? frames : (uint64_t)std::ceil((double)frames * ((double)b->sr / (double)src_sr));
  const uint64_t stride = (target + 3) / 4 * 4;
  float* d = nullptr;
  int e = dev_alloc(b, &d, (size_t)n_items * n_ch * std::max<uint64_t>(stride, 4), true);
  if (e) return e;
  *planes = d;
  *stride_out = stride;
  *target_out = target;
  if (frames == 0) return 0;
  if (b->dry) {  // plan-only batches have no device: the same arithmetic on the host
    std::vector<float> plane(frames);
    for (uint32_t it = 0; it < n_items; it++)
      for (uint32_t c = 0; c < n_ch; c++) {
        for (uint64_t i = 0; i < frames; i++) plane[i] = (float)pcm[((uint64_t)it * frames + i) * n_ch + c] / 32768.f;
        waa_buffer_resample(plane.data(), frames, src_sr, b->sr, d + ((size_t)it * n_ch + c) * stride, target);
      }
    return 0;
  }
  // the interleaved PCM's staging buffer belongs to the batch like every other buffer (freed with it; out of the device arena when
  // one is reserved): a hipMalloc / hipFree pair per upload synchronised the whole device — in waa_render_sharded's pipeline the
  // render of one sub-batch then waited for the upload of the next (WAA_SHARD_TRACE)
  int16_t* d_pcm = nullptr;
  if (int ea = dev_alloc(b, &d_pcm, (size_t)n_items * frames * n_ch, true)) return ea;
  waa_batch::PendingFill pf{1, pcm, d, d_pcm, n_items, n_ch, frames, stride, target, src_sr};
  if (b->batch_fill_node >= 0 && n_items == b->n_inst) b->batch_fills[(uint32_t)b->batch_fill_node] = pf;
  if (b->defer_fill && n_items == b->n_inst) {
    b->pending_fills.push_back(pf);
    return 0;
  }
  return fill_upload(b, pf);
}

waa_status waa_source_set_buffer_pcm16(waa_batch* b, uint32_t node, uint32_t inst, const int16_t* interleaved, uint32_t n_ch,
                                       uint64_t frames, float sr) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_BUFFER_SOURCE)) || (e = check_inst(b, inst)) || (e = check_unplanned(b))) return e;
  if (n_ch == 0 || n_ch > WAA_MAX_CHANNELS) return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - Invalid number of channels");
  if (!(sr >= 3000.f && sr <= 768000.f)) return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - Invalid sample rate: %f", sr);
  if (!b->dry) HIP_TRY(hipSetDevice(b->device));
  float* d = nullptr;
  uint64_t stride = 0, target = 0;
  if ((e = decode_pcm16(b, interleaved, 1, n_ch, frames, sr, &d, &stride, &target))) return e;
  DeviceBuffer db;
  db.base = d;
  db.ch_stride = stride;
  db.frames = target;
  db.nch = n_ch;
  db.sr = b->sr;
  db.valid = true;
  Node& n = b->nodes[node];
  uint32_t lo = inst == WAA_ALL_INSTANCES ? 0 : inst, hi = inst == WAA_ALL_INSTANCES ? b->n_inst : inst + 1;
  for (uint32_t k = lo; k < hi; k++) n.bufs[k] = db;
  return WAA_OK;
}

waa_status waa_source_set_buffer_pcm16_batch(waa_batch* b, uint32_t node, const int16_t* data, uint32_t n_ch, uint64_t frames,
                                             float sr) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_BUFFER_SOURCE))) return e;
  if (b->planned && b->rearmed) return refill_source(b, node, 1, data, n_ch, frames, sr);
  if ((e = check_unplanned(b))) return e;
  if (n_ch == 0 || n_ch > WAA_MAX_CHANNELS) return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - Invalid number of channels");
  if (!(sr >= 3000.f && sr <= 768000.f)) return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - Invalid sample rate: %f", sr);
  if (!b->dry) HIP_TRY(hipSetDevice(b->device));
  float* d = nullptr;
  uint64_t stride = 0, target = 0;
  b->batch_fill_node = (int64_t)node;  // (decode_pcm16 records the fill for waa_batch_rearm)
  e = decode_pcm16(b, data, b->n_inst, n_ch, frames, sr, &d, &stride, &target);
  b->batch_fill_node = -1;
  if (e) return e;
  Node& n = b->nodes[node];
  for (uint32_t k = 0; k < b->n_inst; k++) {
    DeviceBuffer db;
    db.base = d + (size_t)k * n_ch * stride;
    db.ch_stride = stride;
    db.frames = target;
    db.nch = n_ch;
    db.sr = b->sr;
    db.valid = true;
    n.bufs[k] = db;
  }
  return WAA_OK;
}

waa_status waa_source_adopt_device(waa_batch* b, uint32_t node, const float* device_data, uint32_t n_ch, uint64_t frames,
                                   float sr) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_BUFFER_SOURCE))) return e;
  if (b->planned && b->rearmed) {  // (the plan's tables hold the address: the caller refilled the SAME device buffer)
    const DeviceBuffer& cur = b->nodes[node].bufs[0];
    if (cur.base == device_data && cur.nch == n_ch && cur.frames == frames && cur.sr == sr) return WAA_OK;
    return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - a re-armed batch reads the device buffer it was planned with (node %u)", node);
  }
  if ((e = check_unplanned(b))) return e;
  if (!device_data || n_ch == 0 || n_ch > WAA_MAX_CHANNELS) return fail(WAA_ERR_INVALID_ARGUMENT, "bad device buffer");
  Node& n = b->nodes[node];
  for (uint32_t k = 0; k < b->n_inst; k++) {
    DeviceBuffer db;
    db.base = const_cast<float*>(device_data) + (size_t)k * n_ch * frames;
    db.ch_stride = frames;
    db.frames = frames;
    db.nch = n_ch;
    db.sr = sr;
    db.valid = true;
    n.bufs[k] = db;
  }
  return WAA_OK;
}

waa_status waa_source_start(waa_batch* b, uint32_t node, uint32_t inst, double when, double offset, double duration) {
  int e;
  if (!b || node >= b->nodes.size()) return fail(WAA_ERR_INVALID_ARGUMENT, "bad node");
  const uint32_t kind = b->nodes[node].desc.kind;
  if (kind != WAA_NODE_BUFFER_SOURCE && kind != WAA_NODE_CONSTANT_SOURCE && kind != WAA_NODE_OSCILLATOR)
    return fail(WAA_ERR_INVALID_ARGUMENT, "node %u is not a scheduled source", node);
  if ((e = check_inst(b, inst)) || (e = check_unplanned(b))) return e;
  if (!std::isfinite(when) || !std::isfinite(offset) || !std::isfinite(duration))
    return fail(WAA_ERR_INVALID_ARGUMENT, "TypeError - The provided time value is non-finite.");
  if (when < 0. || offset < 0. || duration < 0.)
    return fail(WAA_ERR_INVALID_ARGUMENT, "RangeError - The provided time value cannot be negative");
  Node& n = b->nodes[node];
  uint32_t lo = inst == WAA_ALL_INSTANCES ? 0 : inst, hi = inst == WAA_ALL_INSTANCES ? b->n_inst : inst + 1;
  // A start message handled in front of quantum ctl_q (a suspend point): the node is unscheduled — silent — before, and a start
  // time that has passed by then becomes that block's time (audio_buffer_source.rs:516-518 `if !started && start_time <
  // block_time { start_time = block_time }`, constant_source.rs:225-231 / oscillator.rs:400-406: start_index 0): the schedule
  // replay sees the time the reference's renderer ends up with.  (block time as thread.rs:366: frames as f64 / rate as f64)
  if (b->ctl_q > 0) when = std::max(when, (double)((uint64_t)b->ctl_q * RQ) / (double)b->sr);
  for (uint32_t k = lo; k < hi; k++) {
    if (n.sched[k].start != DBL_MAX) return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - Cannot call `start` twice");
    n.sched[k].start = when;
    if (kind == WAA_NODE_BUFFER_SOURCE) {
      n.sched[k].offset = offset;
      n.sched[k].duration = duration;
    }
  }
  return WAA_OK;
}

waa_status waa_source_stop(waa_batch* b, uint32_t node, uint32_t inst, double when) {
  int e;
  if (!b || node >= b->nodes.size()) return fail(WAA_ERR_INVALID_ARGUMENT, "bad node");
  const uint32_t kind = b->nodes[node].desc.kind;
  if (kind != WAA_NODE_BUFFER_SOURCE && kind != WAA_NODE_CONSTANT_SOURCE && kind != WAA_NODE_OSCILLATOR)
    return fail(WAA_ERR_INVALID_ARGUMENT, "node %u is not a scheduled source", node);
  if ((e = check_inst(b, inst)) || (e = check_unplanned(b))) return e;
  if (!std::isfinite(when)) return fail(WAA_ERR_INVALID_ARGUMENT, "TypeError - The provided time value is non-finite.");
  if (when < 0.) return fail(WAA_ERR_INVALID_ARGUMENT, "RangeError - The provided time value cannot be negative");
  Node& n = b->nodes[node];
  uint32_t lo = inst == WAA_ALL_INSTANCES ? 0 : inst, hi = inst == WAA_ALL_INSTANCES ? b->n_inst : inst + 1;
  if (b->ctl_q > 0) {
    when = std::max(when, (double)((uint64_t)b->ctl_q * RQ) / (double)b->sr);  // (a stop in the past stops at this block)
    // ONE stop time is what the schedule replay knows.  The reference accepts any number of stop messages and its renderer follows
    // the stop time as it changes from suspend point to suspend point (a source that fell silent may even come back): a second
    // stop message at a suspend point is legal there and out of scope here
    for (uint32_t k = lo; k < hi; k++)
      if (n.sched[k].stop != DBL_MAX)
        return fail(WAA_ERR_OUT_OF_SCOPE, "a second stop() of source node %u arriving at a suspend point is out of scope (one stop time per source)", node);
  }
  for (uint32_t k = lo; k < hi; k++) {
    if (n.sched[k].start == DBL_MAX) return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - Cannot stop before start");
    n.sched[k].stop = when;
  }
  return WAA_OK;
}

waa_status waa_source_set_loop(waa_batch* b, uint32_t node, uint32_t inst, int32_t looping, double ls, double le) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_BUFFER_SOURCE)) || (e = check_inst(b, inst)) || (e = check_unplanned(b))) return e;
  Node& n = b->nodes[node];
  uint32_t lo = inst == WAA_ALL_INSTANCES ? 0 : inst, hi = inst == WAA_ALL_INSTANCES ? b->n_inst : inst + 1;
  for (uint32_t k = lo; k < hi; k++) {
    n.sched[k].looping = looping;
    n.sched[k].loop_start = ls;
    n.sched[k].loop_end = le;
  }
  return WAA_OK;
}

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
  if (!(sr >= 3000.f && sr <= 768000.f)) return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - Invalid sample rate: %f", sr);
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

// the table an instance renders with: its row of the plan's tables once they exist, the host's table otherwise
waa_status waa_oscillator_get_wavetable(waa_batch* b, uint32_t node, uint32_t inst, float* out, uint32_t n) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_OSCILLATOR))) return e;
  if (inst == WAA_ALL_INSTANCES) inst = 0;
  if (inst >= b->n_inst) return fail(WAA_ERR_INVALID_ARGUMENT, "instance %u out of range (OscillatorNode %u, %u instances)", inst, node, b->n_inst);
  if (!out || n != WAA_PERIODIC_WAVE_TABLE_LENGTH)
    return fail(WAA_ERR_INVALID_ARGUMENT, "IndexSizeError - a PeriodicWave table has %d points (got %u)", WAA_PERIODIC_WAVE_TABLE_LENGTH, n);
  const Node& nd = b->nodes[node];
  if (nd.per_inst_wave() && b->planned && !b->dry && nd.d_osc_tables) {
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
  const uint32_t lo = inst == WAA_ALL_INSTANCES ? 0 : inst, hi = inst == WAA_ALL_INSTANCES ? b->n_inst : inst + 1;
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
  ParamStore& p = b->nodes[node].params[param];
  uint32_t lo = inst == WAA_ALL_INSTANCES ? 0 : inst, hi = inst == WAA_ALL_INSTANCES ? b->n_inst : inst + 1;
  if (b->ctl_q > 0) {
    // AudioParam::set_value from a suspend callback: a SetValue event the render thread handles in front of quantum ctl_q
    // (param.rs:386-400, thread.rs:277-294) — through the timeline, which is created (seeded with the constant so far) if the
    // param had none
    if (p.timelines.empty()) p.timelines.resize(b->n_inst);
    if (inst != WAA_ALL_INSTANCES) p.timelines_shared = false;
    for (uint32_t k = lo; k < hi; k++) {
      if (!p.timelines[k]) {
        p.timelines[k] = std::make_shared<Timeline>(p.defv, p.minv, p.maxv, !p.k_rate);
        if ((e = p.timelines[k]->schedule(WAA_EVENT_SET_VALUE, p.cst[k], 0., 0., nullptr, 0))) return e;
      }
      if ((e = p.timelines[k]->schedule_at(b->ctl_q, WAA_EVENT_SET_VALUE, value, 0., 0., nullptr, 0))) return e;
    }
    return WAA_OK;
  }
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

// build_plan under a stopwatch; the split (hipMalloc / blocking uploads / the rest = host planning: ordering, scheduling
// replay, coefficient and automation evaluation) goes into the plan description
int waa_settle_loops(waa_batch* b);

// AudioBufferSourceNode::playback_rate / detune with an input from the graph (k-rate: value + the first sample of the
// mixed input, NaN -> default, clamped, once per render quantum: param.rs:739-760; audio_buffer_source.rs:176-197).  The
// playhead replay that turns those values into the source's per-quantum schedule runs on the host, so the modulating
// subgraph is rendered FIRST, by the ordinary plan machinery (prepass), one value per quantum is read back and installed
// as a k-rate value block per instance; the param edges are then removed and the real plan is built.
static int resolve_source_rate_modulation(waa_batch* b) {
  std::vector<std::pair<uint32_t, uint32_t>> mods;
  for (auto& ed : b->edges) {
    if (!(ed.to_input & 0x80000000u) || ed.to >= b->nodes.size()) continue;
    const uint32_t pid = ed.to_input & 0x7fffffffu;
    const Node& tn = b->nodes[ed.to];
    if (tn.desc.kind == WAA_NODE_BUFFER_SOURCE) {
      if (pid != WAA_PARAM_SOURCE_PLAYBACK_RATE && pid != WAA_PARAM_SOURCE_DETUNE) continue;
    } else if (tn.desc.kind == WAA_NODE_PANNER && pid <= WAA_PARAM_PANNER_ORIENTATION_Z && tn.params.size() >= 15) {
      // PannerNode position / orientation: with a single-valued AudioListener the reference uses the first value of every
      // param per quantum (panner.rs:833-846, HRTF :781-829): k-rate in effect, resolved like the source rates.  With
      // audio-rate listener automation the params are consumed per frame: left to build_plan, which refuses the edge.
      bool listener_a_rate = false;
      for (int k = 6; k < 15; k++) listener_a_rate |= tn.params[(size_t)k].mode() == 2 || !tn.params[(size_t)k].timelines.empty();
      if (listener_a_rate) continue;
    } else {
      continue;
    }
    const std::pair<uint32_t, uint32_t> key(ed.to, pid);
    if (std::find(mods.begin(), mods.end(), key) == mods.end()) mods.push_back(key);
  }
  if (mods.empty() || b->dry) return 0;  // (plan-only batch: build_plan refuses the edges with the reason)
  b->prepass = true;
  b->prepass_params = mods;
  b->prepass_refs.assign(mods.size(), ParamRef{});
  int e = build_plan(b);
  const size_t n_steps = b->steps.size();
  if (!e) e = run_steps(b);
  std::vector<std::vector<float>> heads(mods.size());
  if (!e) {
    float* d_heads = nullptr;
    const size_t count = (size_t)b->n_inst * b->n_quanta;
    // (no early return from here on: the prepass state installed above must be torn down on every path)
    const hipError_t me = hipMalloc(&d_heads, count * sizeof(float));
    if (me != hipSuccess) e = fail(WAA_ERR_DEVICE, "hipMalloc of the per-quantum param values: %s", hipGetErrorString(me));
    for (size_t k = 0; k < mods.size() && !e; k++) {
      const ParamRef& r = b->prepass_refs[k];
      if (r.mode != 2 || !r.base) {
        e = fail(WAA_ERR_INVALID_STATE, "internal: the modulated param %u of source node %u has no per-frame values", mods[k].second, mods[k].first);
        break;
      }
      launch_quantum_heads(r.base, r.stride, b->n_inst, b->n_quanta, d_heads, b->stream);
      heads[k].resize(count);
      hipError_t he = hipMemcpyAsync(heads[k].data(), d_heads, count * sizeof(float), hipMemcpyDeviceToHost, b->stream);
      if (he == hipSuccess) he = hipStreamSynchronize(b->stream);
      if (he != hipSuccess) e = fail(WAA_ERR_DEVICE, "reading back the modulated playbackRate / detune values: %s", hipGetErrorString(he));
    }
    (void)hipFree(d_heads);
  }
  // back to an unplanned batch (what the second planning pass of a dynamic plan does, plus the prepass switch)
  b->prepass = false;
  b->steps.clear();
  b->group_tiles.clear();
  b->qgroup_quanta.clear();
  b->state_bufs.clear();
  b->ones_bufs.clear();
  b->plan_log.clear();
  b->force_dynamic = false;
  for (auto& nd : b->nodes) {
    nd.sig = SignalRef{};
    nd.hist = SignalRef{};
    nd.hist_is_temp = false;
  }
  if (e) return e;
  for (size_t k = 0; k < mods.size(); k++) {
    ParamStore& p = b->nodes[mods[k].first].params[mods[k].second];
    p.blocks.clear();  // (the chain added the intrinsic value — constants, value blocks, evaluated automation — already)
    p.timelines.clear();
    p.dev_tl = false;
    for (uint32_t i = 0; i < b->n_inst; i++) {
      ParamBlock blk;
      blk.inst = i;
      blk.q0 = 0;
      blk.nq = b->n_quanta;
      blk.vpq = 1;
      blk.v.assign(heads[k].begin() + (size_t)i * b->n_quanta, heads[k].begin() + (size_t)(i + 1) * b->n_quanta);
      p.blocks.push_back(std::move(blk));
    }
  }
  b->edges.erase(std::remove_if(b->edges.begin(), b->edges.end(),
                                [&](const waa_edge_desc& ed) {
                                  if (!(ed.to_input & 0x80000000u)) return false;
                                  const std::pair<uint32_t, uint32_t> key(ed.to, ed.to_input & 0x7fffffffu);
                                  return std::find(mods.begin(), mods.end(), key) != mods.end();
                                }),
                 b->edges.end());
  char note[512];
  snprintf(note, sizeof note,
           "%zu host-evaluated k-rate param(s) (source playbackRate / detune, panner position / orientation) modulated from the graph: the modulating subgraph was rendered at plan time "
           "(%zu launch step(s)), one value per render quantum read back (k-rate, param.rs:739-760)",
           mods.size(), n_steps);
  b->prepass_note = note;
  return 0;
}

// An edge that is live for quanta [on, off) only (waa_connect / waa_disconnect at a suspend point) becomes
//   from -> GainNode(gain = 1 inside the window, 0 outside, one value per quantum, every instance) -> to
// before the graph is planned.  gain.rs:163-179: a gain of exactly 1 passes the input through (clone: same channels, same
// samples), a gain of exactly 0 makes the output silent (one silent channel) — what the destination's input sees of a connection
// that exists resp. does not (quantum.rs mixing: a silent mono input changes neither the sum nor the computed channel count).
// The gate inherits nothing else: count mode max / speakers (a GainNode's defaults) forwards whatever count arrives.
// A window that is empty drops the edge; the summation ORDER at the destination follows the processing order of the gates
// instead of the sources' (three or more summands may differ in the last bit from the reference).
static int desugar_timed_edges(waa_batch* b) {
  if (b->timed_edges_done) return 0;
  b->timed_edges_done = true;
  {
    // A connection INSIDE a feedback loop made or cut at a suspend point changes what the reference's graph ordering does from then
    // on (graph.rs:323-487: the cycle is gone, the DelayNode's writer renders before its reader again while the reader's in_cycle
    // flag stays set, delay.rs:535-541) — the gate keeps the loop a loop for the whole render.  Found by the suspend fuzz
    // (tests/test_fuzz_suspend.py, seeds 71 / 365 / 525: 3 of 600).  Strongly connected components of the union of all connections;
    // a timed edge whose ends share one is out of scope.
    bool any_timed = false;
    for (size_t k = 0; k < b->edges.size(); k++) any_timed |= b->edge_on[k] != 0 || b->edge_off[k] < b->n_quanta;
    if (any_timed) {
      const uint32_t n = (uint32_t)b->nodes.size();
      std::vector<std::vector<uint32_t>> adj(n);
      for (const waa_edge_desc& ed : b->edges) adj[ed.from].push_back(ed.to);
      std::vector<int> index(n, -1), low(n, 0), comp(n, -1);
      std::vector<uint8_t> on_stack(n, 0);
      std::vector<uint32_t> stack;
      int next_index = 0, n_comp = 0;
      struct Frame {
        uint32_t v;
        size_t child;
      };
      for (uint32_t root = 0; root < n; root++) {
        if (index[root] >= 0) continue;
        std::vector<Frame> call{{root, 0}};
        index[root] = low[root] = next_index++;
        stack.push_back(root);
        on_stack[root] = 1;
        while (!call.empty()) {
          Frame& f = call.back();
          if (f.child < adj[f.v].size()) {
            const uint32_t w = adj[f.v][f.child++];
            if (index[w] < 0) {
              index[w] = low[w] = next_index++;
              stack.push_back(w);
              on_stack[w] = 1;
              call.push_back({w, 0});
            } else if (on_stack[w]) {
              low[f.v] = std::min(low[f.v], index[w]);
            }
          } else {
            const uint32_t v = f.v;
            if (low[v] == index[v]) {
              for (;;) {
                const uint32_t w = stack.back();
                stack.pop_back();
                on_stack[w] = 0;
                comp[w] = n_comp;
                if (w == v) break;
              }
              n_comp++;
            }
            call.pop_back();
            if (!call.empty()) low[call.back().v] = std::min(low[call.back().v], low[v]);
          }
        }
      }
      for (size_t k = 0; k < b->edges.size(); k++) {
        if (b->edge_on[k] == 0 && b->edge_off[k] >= b->n_quanta) continue;
        const waa_edge_desc& ed = b->edges[k];
        if (comp[ed.from] == comp[ed.to])
          return fail(WAA_ERR_OUT_OF_SCOPE, "the connection %u -> %u lies inside a feedback loop and is made or cut at a suspend point: out of scope",
                      ed.from, ed.to);
      }
      // ... and a connection OUTSIDE every loop can still move the place where the reference breaks one: order_nodes walks the
      // edges in insertion order, and which DelayNode of a loop with several of them meets the walk first — and loses its
      // writer -> reader edge, i.e. renders one quantum late — depends on every edge the walk passes (suspend fuzz seed 10216: the
      // source -> delay connection cut at quantum 15 moved the breaker to the loop's other DelayNode, 2.7 of full scale).  The plan
      // has ONE order: the reference's ordering is computed for the connections of every epoch, and the epochs must agree on the
      // cut DelayNodes and on the muted nodes.
      std::vector<uint32_t> pts{0};
      for (size_t k = 0; k < b->edges.size(); k++) {
        if (b->edge_on[k] > 0 && b->edge_on[k] < b->n_quanta) pts.push_back(b->edge_on[k]);
        if (b->edge_off[k] < b->n_quanta) pts.push_back(b->edge_off[k]);
      }
      std::sort(pts.begin(), pts.end());
      pts.erase(std::unique(pts.begin(), pts.end()), pts.end());
      const std::vector<waa_edge_desc> all = b->edges;
      std::vector<uint8_t> cut0, muted0;
      // (... and on the ORDER in which the members of every loop are rendered: inside a loop the order decides who hears this quantum's
      // and who last quantum's output of whom — suspend fuzz seed 122641 of the wide generator, round 6: cutting an oscillator's
      // connection into a loop's second DelayNode left the breaker where it was and still moved that DelayNode's reader in front of
      // the loop's first members, 1.0 of full scale)
      std::vector<uint32_t> comp_size(n_comp, 0);
      for (uint32_t v = 0; v < b->nodes.size(); v++) comp_size[comp[v]]++;
      std::vector<uint32_t> loop_order0;
      // (... and, where a signal can be wider than stereo, on the order in which every summing node hears its producers: the reference
      // adds a producer's output to its consumers' input buses WHEN IT RENDERS (graph.rs:524-535), so the order of the sum is the render
      // order, and above stereo the sum is not commutative — the bus is up-mixed input by input, mono -> stereo -> 5.1 is not
      // mono -> 5.1 (DESIGN.md section 5 "Channels").  Same seed: the cut also moved the oscillator behind the loop in the order, and
      // the analyser behind both heard it on the centre channel instead of L and R.)
      int widest = (int)b->n_out;
      for (const Node& nd : b->nodes) {
        widest = std::max(widest, nd.cc);
        for (const DeviceBuffer& bf : nd.bufs)
          if (bf.valid) widest = std::max(widest, (int)bf.nch);
      }
      // (the plan renders the UNION of the connections, gated: its order is the reference for every epoch)
      std::vector<int64_t> pos0(b->nodes.size(), -1);
      {
        std::vector<uint8_t> cutu, mutedu;
        std::vector<uint32_t> itemsu;
        compute_order(b, &cutu, &mutedu, &itemsu);
        for (size_t k = 0; k < itemsu.size(); k++) {
          const uint32_t v = itemsu[k], id = v & 0x7fffffffu;
          if ((v & 0x80000000u) || b->nodes[id].desc.kind != WAA_NODE_DELAY) pos0[id] = (int64_t)k;
        }
      }
      int bad = 0;
      for (size_t e = 0; e < pts.size() && !bad; e++) {
        b->edges.clear();
        for (size_t k = 0; k < all.size(); k++)
          if (b->edge_on[k] <= pts[e] && pts[e] < b->edge_off[k]) b->edges.push_back(all[k]);
        std::vector<uint8_t> cut, muted;
        std::vector<uint32_t> items;
        compute_order(b, &cut, &muted, &items);
        std::vector<uint32_t> loop_order;
        for (uint32_t v : items)
          if (comp_size[comp[v & 0x7fffffffu]] > 1) loop_order.push_back(v);  // (bit 31: a DelayNode's reader vertex, waa_plan_parts.hpp)
        std::vector<int64_t> pos(b->nodes.size(), -1);  // render position of every node's OUTPUT (a DelayNode: its reader's)
        for (size_t k = 0; k < items.size(); k++) {
          const uint32_t v = items[k], id = v & 0x7fffffffu;
          if ((v & 0x80000000u) || b->nodes[id].desc.kind != WAA_NODE_DELAY) pos[id] = (int64_t)k;
        }
        if (e == 0) {
          cut0 = cut;
          muted0 = muted;
          loop_order0 = loop_order;
        } else if (cut != cut0 || muted != muted0 || loop_order != loop_order0) {
          bad = (int)pts[e];
        }
        if (!bad && widest > 2) {
          for (size_t k1 = 0; k1 < b->edges.size() && !bad; k1++)
            for (size_t k2 = k1 + 1; k2 < b->edges.size() && !bad; k2++) {
              const waa_edge_desc &a = b->edges[k1], &c = b->edges[k2];
              if (a.to != c.to || a.to_input != c.to_input || a.from == c.from) continue;
              if (pos[a.from] < 0 || pos[c.from] < 0 || pos0[a.from] < 0 || pos0[c.from] < 0) continue;
              if ((pos[a.from] < pos[c.from]) != (pos0[a.from] < pos0[c.from])) bad = (int)pts[e];
            }
        }
      }
      b->edges = all;
      if (bad)
        return fail(WAA_ERR_OUT_OF_SCOPE, "the connections made or cut at the suspend point in front of quantum %d change where the reference breaks a "
                                          "feedback loop, which nodes it mutes, the order in which it renders a loop's members or (with signals wider than stereo) the order in which a node sums its inputs: out of scope", bad);
    }
  }
  std::vector<waa_edge_desc> edges;
  size_t n_gates = 0;
  for (size_t k = 0; k < b->edges.size(); k++) {
    const uint32_t on = b->edge_on[k], off = std::min(b->edge_off[k], b->n_quanta);
    if (on == 0 && off >= b->n_quanta) {
      edges.push_back(b->edges[k]);
      continue;
    }
    if (on >= off) continue;  // never live
    const uint32_t gid = (uint32_t)b->nodes.size();
    b->nodes.emplace_back();
    Node& g = b->nodes.back();
    g.desc = waa_node_desc{};
    g.desc.kind = WAA_NODE_GAIN;
    default_channel_config(g, b->n_out);
    g.params.resize(1);
    g.params[0].init(b->n_inst, on == 0 ? 1.f : 0.f, -FLT_MAX, FLT_MAX);
    ParamBlock blk;
    blk.inst = WAA_ALL_INSTANCES;
    blk.q0 = 0;
    blk.nq = b->n_quanta;
    blk.vpq = 1;
    blk.v.assign(b->n_quanta, 0.f);
    for (uint32_t q = on; q < off; q++) blk.v[q] = 1.f;
    g.params[0].blocks.push_back(std::move(blk));
    edges.push_back(waa_edge_desc{b->edges[k].from, b->edges[k].from_output, gid, 0});
    edges.push_back(waa_edge_desc{gid, 0, b->edges[k].to, b->edges[k].to_input});
    n_gates++;
  }
  if (n_gates) {
    char note[200];
    snprintf(note, sizeof note, "%zu connection(s) made or cut at suspend points (waa_connect / waa_disconnect after waa_render_range): gated by GainNodes %u..%u",
             n_gates, b->n_user_nodes, (uint32_t)b->nodes.size() - 1);
    b->timed_note = note;
  }
  b->edges = std::move(edges);
  b->edge_on.assign(b->edges.size(), 0u);
  b->edge_off.assign(b->edges.size(), EDGE_NEVER);
  return 0;
}

static int timed_build_plan(waa_batch* b) {
  if (int et = desugar_timed_edges(b)) return et;
  const auto t0 = std::chrono::steady_clock::now();
  const double a0 = b->t_alloc_ms, u0 = b->t_upload_ms;
  const uint64_t n0 = b->n_alloc, by0 = b->alloc_bytes;
  int e = resolve_source_rate_modulation(b);
  if (!e) e = build_plan(b);
  if (!e && !b->prepass_note.empty()) b->plan_log.push_back(b->prepass_note);
  if (!e && !b->timed_note.empty()) b->plan_log.push_back(b->timed_note);
  for (uint32_t i = 0; !e && i < b->n_user_nodes; i++) {
    const Node& n = b->nodes[i];
    if (!n.an_series()) continue;
    char note[200];
    snprintf(note, sizeof note, "analyser series: node %u, %u pull(s) every %d quanta from quantum %d, fft_size %d", i,
             n.an_series_pulls(b->n_quanta), n.desc.i[1], n.desc.i[2], n.desc.i[0]);
    b->plan_log.push_back(note);
  }
  b->t_plan_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  b->plan_alloc_ms = b->t_alloc_ms - a0;
  b->plan_upload_ms = b->t_upload_ms - u0;
  b->plan_n_alloc = b->n_alloc - n0;
  b->plan_alloc_bytes = b->alloc_bytes - by0;
  return e;
}

waa_status waa_plan_describe(waa_batch* b, char* buf, size_t cap, size_t* needed) {
  if (!b) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch");
  if (!b->planned) {
    if (!b->dry) HIP_TRY(hipSetDevice(b->device));
    int e = timed_build_plan(b);
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

// Quantum-blocked loops rendered in blocks of several quanta are optimistic about ONE thing (waa_plan_dyn.cpp: the ring's channel
// count as the reader of a split delay pair sees it).  Every entry point that hands out results waits for the render and looks at
// the writers' flags first; a flagged render is repeated with one quantum per block — the round-5 form, always right.
int waa_settle_loops(waa_batch* b) {
  if (!b->loops_unsettled || b->dry) return 0;
  HIP_TRY(hipStreamSynchronize(b->stream));
  b->loops_unsettled = false;
  bool bad = false;
  for (int32_t* f : b->loop_flags) {
    int32_t v = 0;
    HIP_TRY(hipMemcpy(&v, f, sizeof v, hipMemcpyDeviceToHost));
    bad |= v != 0;
  }
  if (!bad) return 0;
  b->loops_one_quantum = true;
  b->plan_log.push_back("a feedback loop's channel counts moved inside a block of several quanta: rendered again one quantum per block (and from now on)");
  int e = run_steps(b);
  if (e) return e;
  HIP_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

waa_status waa_render(waa_batch* b) {
  if (!b) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch");
  if (b->ranged && b->ctl_q < b->n_quanta)
    return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - a ranged render is in progress (suspended in front of quantum %u): waa_render_range renders the rest", b->ctl_q);
  if (b->dry) return fail(WAA_ERR_DEVICE, "plan-only batch (WAA_DEVICE_PLAN_ONLY) cannot render: there is no CPU fallback");
  HIP_TRY(hipSetDevice(b->device));
  if (!b->planned) {
    int e = timed_build_plan(b);
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
  if (int es = waa_settle_loops(b)) return es;
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
  if (int es = waa_settle_loops(b)) return es;
  const SignalRef& s = b->nodes[0].sig;
  if ((int)ch < s.nch) {
    if (int e = waa_internal_xfer_d2h(b, dst, frames * sizeof(float), s.base + (size_t)inst * s.inst_stride + (size_t)ch * s.ch_stride, frames * sizeof(float),
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
  if (int es = waa_settle_loops(b)) return es;
  const SignalRef& s = b->nodes[0].sig;
  if (b->length == 0) return WAA_OK;
  if ((uint32_t)s.nch == b->n_out) {
    if (int e = waa_internal_xfer_d2h(b, dst, b->length * sizeof(float), s.base, s.ch_stride * sizeof(float), b->length * sizeof(float), (size_t)b->n_inst * b->n_out))
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

// AnalyserNode pulls (analysis.rs:261-401).  current_time after an offline render never changes, so the spectra of ALL
// instances are computed once per render — one launch, one workgroup per context — and every pull, per instance or for
// the whole batch, is a view into that result (repeated pulls return the same data, analysis.rs:354-357).
enum { AN_DB = 0, AN_BYTES = 1, AN_TIME = 2, AN_TBYTES = 3 };
// the Blackman window and the twiddles of the packed real transform, uploaded on first use
static int analyser_tables(waa_batch* b, Node& n) {
  if (n.d_window) return 0;
  const int N = n.desc.i[0], M = N / 2;
  int e;
  // generate_blackman (analysis.rs:14-24), f32 with the host libm the reference's f32::cos resolves to
  std::vector<float> win(N);
  const float alpha = 0.16f, a0 = (1.f - alpha) / 2.f, a1 = 1.f / 2.f, a2 = alpha / 2.f;
  for (int i = 0; i < N; i++)
    win[i] = a0 - a1 * cosf(2.f * PI_F * (float)i / (float)N) + a2 * cosf(4.f * PI_F * (float)i / (float)N);
  std::vector<Cplx> tw(M), twf(M);
  for (int t = 0; t < M; t++) {
    const double x = -2.0 * 3.14159265358979323846 * (double)t / (double)M;
    const double y = -2.0 * 3.14159265358979323846 * (double)t / (double)N;
    tw[t] = Cplx{(float)std::cos(x), (float)std::sin(x)};
    twf[t] = Cplx{(float)std::cos(y), (float)std::sin(y)};
  }
  if ((e = dev_upload(b, &n.d_window, win)) || (e = dev_upload(b, &n.d_an_tw, tw)) || (e = dev_upload(b, &n.d_an_twfull, twf))) return e;
  return 0;
}
static int analyser_compute(waa_batch* b, uint32_t node, int what) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_ANALYSER))) return e;
  Node& n = b->nodes[node];
  const int N = n.desc.i[0], M = N / 2;
  const size_t ni = b->n_inst;
  const bool on_device = b->planned && b->rendered && n.live && !b->dry;
  if (on_device)
    if (int es = waa_settle_loops(b)) return es;  // (run_steps resets the analysers' caches: the pull below sees the settled render)
  if (!on_device) {
    // nothing rendered (or the node does not reach the destination): an all-zero ring buffer
    if (!n.an.have_db) {
      n.an.db.assign(ni * M, -INFINITY);   // 20 log10(0)
      n.an.bytes.assign(ni * M, 0);        // (-inf - min) scaled and clamped
      n.an.time.assign(ni * N, 0.f);
      n.an.have_db = n.an.have_bytes = n.an.have_time = true;
    }
    return 0;
  }
  HIP_TRY(hipSetDevice(b->device));
  if (!n.an.computed) {
    if ((e = analyser_tables(b, n))) return e;
    if (!n.d_an_db) {
      std::vector<float> zeros(M, 0.f);
      if ((e = dev_upload(b, &n.d_an_prev, zeros)) || (e = dev_alloc(b, &n.d_an_db, ni * M)) || (e = dev_alloc(b, &n.d_an_bytes, ni * M)) ||
          (e = dev_alloc(b, &n.d_an_time, ni * N)))
        return e;
    }
    AnalyserDesc ad{};
    ad.sig = n.sig;
    ad.n_inst = b->n_inst;
    ad.fft_size = N;
    ad.frames_written = (uint64_t)b->n_quanta * RQ;
    ad.smoothing = (float)n.desc.d[0];
    ad.min_db = (float)n.desc.d[1];
    ad.max_db = (float)n.desc.d[2];
    ad.window = n.d_window;
    ad.tw = n.d_an_tw;
    ad.tw_full = n.d_an_twfull;
    ad.prev = n.d_an_prev;
    ad.db_out = n.d_an_db;
    ad.byte_out = n.d_an_bytes;
    ad.time_out = n.d_an_time;
    ad.code = b->dynamic ? n.code : nullptr;
    ad.code_stride = b->code_stride;
    int slot = -1;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (b->profiling) {
      slot = slot_for(b, "analyser_kernel");
      HIP_TRY(hipEventCreate(&e0));
      HIP_TRY(hipEventCreate(&e1));
      HIP_TRY(hipEventRecord(e0, b->stream));
    }
    launch_analyser(ad, b->stream);
    HIP_TRY(hipGetLastError());
    if (slot >= 0) {
      HIP_TRY(hipEventRecord(e1, b->stream));
      b->prof[slot].pending.push_back({e0, e1});
    }
    n.an.computed = true;
  }
  // one transfer per kind of result, on first use (asynchronous on the batch's stream, then waited for)
  if (what == AN_DB && !n.an.have_db) {
    n.an.db.resize(ni * M);
    HIP_TRY(hipMemcpyAsync(n.an.db.data(), n.d_an_db, ni * M * sizeof(float), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    n.an.have_db = true;
  } else if (what == AN_BYTES && !n.an.have_bytes) {
    n.an.bytes.resize(ni * M);
    HIP_TRY(hipMemcpyAsync(n.an.bytes.data(), n.d_an_bytes, ni * M, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    n.an.have_bytes = true;
  } else if (what == AN_TIME && !n.an.have_time) {
    n.an.time.resize(ni * N);
    HIP_TRY(hipMemcpyAsync(n.an.time.data(), n.d_an_time, ni * N * sizeof(float), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    n.an.have_time = true;
  }
  return 0;
}

// A series node (desc.i[1] > 0, include/waa_hip.h): the rows of ALL pulls of ALL instances, computed once per render and per kind
// on the device (waa_analyser_series.hip) and kept there; a getter call copies its rows [i0, i1) x [P] out, `nn` elements apart.
static int analyser_series_rows(waa_batch* b, uint32_t node, int what, uint32_t i0, uint32_t i1, void* dst, uint32_t nn) {
  Node& n = b->nodes[node];
  const uint32_t N = (uint32_t)n.desc.i[0], M = N / 2, P = n.an_series_pulls(b->n_quanta);
  const size_t ni = b->n_inst;
  const bool freq = what == AN_DB || what == AN_BYTES, bytes = what == AN_BYTES || what == AN_TBYTES;
  const uint32_t W = freq ? M : N, len = std::min(nn, W);
  const size_t es = bytes ? 1 : sizeof(float), rows = (size_t)(i1 - i0) * P;
  const bool on_device = b->planned && b->rendered && n.live && !b->dry;
  if (on_device)
    if (int es2 = waa_settle_loops(b)) return es2;  // (run_steps resets the analysers' caches: the pulls below see the settled render)
  if (what == AN_TBYTES && nn > len)  // analysis.rs:268-276: elements past fft_size come from a zeroed tmp
    for (size_t r = 0; r < rows; r++) std::memset((uint8_t*)dst + r * nn + len, 128, nn - len);
  if (!on_device) {
    // nothing rendered (or the node does not reach the destination): every pull sees an all-zero ring buffer
    for (size_t r = 0; r < rows; r++) {
      if (what == AN_DB)
        std::fill_n((float*)dst + r * nn, len, -INFINITY);  // 20 log10(0)
      else if (what == AN_BYTES)
        std::memset((uint8_t*)dst + r * nn, 0, len);         // (-inf - min) scaled and clamped
      else if (what == AN_TIME)
        std::fill_n((float*)dst + r * nn, len, 0.f);
      else
        std::memset((uint8_t*)dst + r * nn, 128, len);
    }
    return WAA_OK;
  }
  HIP_TRY(hipSetDevice(b->device));
  int e;
  if ((e = analyser_tables(b, n))) return e;
  AnalyserSeriesDesc sd{};
  sd.a.sig = n.sig;
  sd.a.n_inst = b->n_inst;
  sd.a.fft_size = (int32_t)N;
  sd.a.smoothing = (float)n.desc.d[0];
  sd.a.min_db = (float)n.desc.d[1];
  sd.a.max_db = (float)n.desc.d[2];
  sd.a.window = n.d_window;
  sd.a.tw = n.d_an_tw;
  sd.a.tw_full = n.d_an_twfull;
  sd.a.code = b->dynamic ? n.code : nullptr;
  sd.a.code_stride = b->code_stride;
  sd.hop = n.desc.i[1];
  sd.first = n.desc.i[2];
  sd.pulls = (int32_t)P;
  sd.frames = (uint64_t)b->n_quanta * RQ;
  analyser_series_shape(&sd);
  auto timed = [&](const char* name, auto&& launch) -> int {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const int slot = b->profiling ? slot_for(b, name) : -1;
    if (slot >= 0) {
      HIP_TRY(hipEventCreate(&e0));
      HIP_TRY(hipEventCreate(&e1));
      HIP_TRY(hipEventRecord(e0, b->stream));
    }
    launch();
    HIP_TRY(hipGetLastError());
    if (slot >= 0) {
      HIP_TRY(hipEventRecord(e1, b->stream));
      b->prof[slot].pending.push_back({e0, e1});
    }
    return 0;
  };
  const size_t nf = ni * P * M, nt = ni * P * N;
  const void* src = nullptr;
  if (freq) {
    const bool smooth = sd.a.smoothing > 0.f;
    if (what == AN_BYTES && !n.d_ans_bytes && (e = dev_alloc(b, &n.d_ans_bytes, nf))) return e;
    // dB rows: asked for, the recursion's workspace (the unsmoothed magnitudes in f32), or there from an earlier render and not
    // current — the pass that is about to run fills them too, so that float rows asked for later do not transform again
    const bool need_db = what == AN_DB || (smooth && !n.an.s_bytes) || (n.d_ans_db && !n.an.s_db);
    if (need_db && !n.d_ans_db && (e = dev_alloc(b, &n.d_ans_db, nf))) return e;
    sd.db_out = n.d_ans_db;
    sd.byte_out = n.d_ans_bytes;
    if (what == AN_BYTES && !n.an.s_bytes && n.an.s_db) {
      if ((e = timed("analyser_series_bytes_kernel", [&] { launch_analyser_series_bytes(sd, b->stream); }))) return e;
      n.an.s_bytes = true;
    } else if (!(what == AN_DB ? n.an.s_db : n.an.s_bytes)) {
      // one transform pass for every frequency kind that has a buffer by now and is not current
      if (!need_db) sd.db_out = nullptr;
      if (n.an.s_bytes) sd.byte_out = nullptr;
      sd.lin = smooth ? 1 : 0;
      if ((e = timed("analyser_series_fft_kernel", [&] { launch_analyser_series_fft(sd, b->stream); }))) return e;
      if (smooth && (e = timed("analyser_series_smooth_kernel", [&] { launch_analyser_series_smooth(sd, b->stream); }))) return e;
      n.an.s_db |= sd.db_out != nullptr;
      n.an.s_bytes |= sd.byte_out != nullptr;
    }
    src = what == AN_DB ? (const void*)n.d_ans_db : (const void*)n.d_ans_bytes;
  } else {
    if (what == AN_TIME && !n.d_ans_time && (e = dev_alloc(b, &n.d_ans_time, nt))) return e;
    if (what == AN_TBYTES && !n.d_ans_tbytes && (e = dev_alloc(b, &n.d_ans_tbytes, nt))) return e;
    if (!(what == AN_TIME ? n.an.s_time : n.an.s_tbytes)) {
      // (both forms in one gather when both have a buffer and neither is current)
      sd.time_out = n.an.s_time ? nullptr : n.d_ans_time;
      sd.tbyte_out = n.an.s_tbytes ? nullptr : n.d_ans_tbytes;
      if ((e = timed("analyser_series_time_kernel", [&] { launch_analyser_series_time(sd, b->stream); }))) return e;
      n.an.s_time |= sd.time_out != nullptr;
      n.an.s_tbytes |= sd.tbyte_out != nullptr;
    }
    src = what == AN_TIME ? (const void*)n.d_ans_time : (const void*)n.d_ans_tbytes;
  }
  // ring_buffer.read hands out the most recent `len` frames (analysis.rs:114-127); frequency rows start at bin 0
  const char* from = (const char*)src + ((size_t)i0 * P * W + (freq ? 0 : W - len)) * es;
  // (pageable caller memory goes through the batch's pinned staging block: the device only touches memory this library pinned)
  if ((e = waa_internal_xfer_d2h(b, dst, (size_t)nn * es, from, (size_t)W * es, (size_t)len * es, rows))) return e;
  HIP_TRY(hipStreamSynchronize(b->stream));
  return WAA_OK;
}
// rows [i0, i1) of one result kind -> dst rows of `nn` elements
static int analyser_rows(waa_batch* b, uint32_t node, int what, uint32_t i0, uint32_t i1, void* dst, uint32_t nn) {
  int e = check_node(b, node, WAA_NODE_ANALYSER);
  if (e) return e;
  if (b->nodes[node].an_series()) return analyser_series_rows(b, node, what, i0, i1, dst, nn);
  if ((e = analyser_compute(b, node, what))) return e;
  const Node& n = b->nodes[node];
  const uint32_t N = (uint32_t)n.desc.i[0], M = N / 2;
  for (uint32_t i = i0; i < i1; i++) {
    const size_t row = (size_t)(i - i0) * nn;
    if (what == AN_DB) {
      std::memcpy((float*)dst + row, &n.an.db[(size_t)i * M], std::min(nn, M) * sizeof(float));
    } else if (what == AN_BYTES) {
      std::memcpy((uint8_t*)dst + row, &n.an.bytes[(size_t)i * M], std::min(nn, M));
    } else {
      // ring_buffer.read: the most recent `len` frames (analysis.rs:114-127)
      const uint32_t len = std::min(nn, N);
      std::memcpy((float*)dst + row, &n.an.time[(size_t)i * N + (N - len)], len * sizeof(float));
    }
  }
  return WAA_OK;
}
static int analyser_byte_time_rows(waa_batch* b, uint32_t node, uint32_t i0, uint32_t i1, uint8_t* dst, uint32_t nn) {
  int e = check_node(b, node, WAA_NODE_ANALYSER);
  if (e) return e;
  if (b->nodes[node].an_series()) return analyser_series_rows(b, node, AN_TBYTES, i0, i1, dst, nn);
  if ((e = analyser_compute(b, node, AN_TIME))) return e;
  const Node& n = b->nodes[node];
  const uint32_t N = (uint32_t)n.desc.i[0];
  const uint32_t len = std::min(nn, N);
  for (uint32_t i = i0; i < i1; i++) {
    const float* t = &n.an.time[(size_t)i * N + (N - len)];
    uint8_t* o = dst + (size_t)(i - i0) * nn;
    for (uint32_t k = 0; k < nn; k++) {  // analysis.rs:268-276 (elements past fft_size read a zeroed tmp)
      const float v = k < len ? t[k] : 0.f;
      const float scaled = 128.f * (1.f + v);
      const float clamped = scaled < 0.f ? 0.f : scaled > 255.f ? 255.f : scaled;
      o[k] = (uint8_t)clamped;
    }
  }
  return WAA_OK;
}
static int an_inst(waa_batch* b, uint32_t inst) {
  if (!b) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch");
  if (inst >= b->n_inst) return fail(WAA_ERR_INVALID_ARGUMENT, "instance out of range");
  return 0;
}

waa_status waa_analyser_get_float_frequency_data(waa_batch* b, uint32_t node, uint32_t inst, float* dst, uint32_t nn) {
  if (int e = an_inst(b, inst)) return e;
  return analyser_rows(b, node, AN_DB, inst, inst + 1, dst, nn);
}
waa_status waa_analyser_get_byte_frequency_data(waa_batch* b, uint32_t node, uint32_t inst, uint8_t* dst, uint32_t nn) {
  if (int e = an_inst(b, inst)) return e;
  return analyser_rows(b, node, AN_BYTES, inst, inst + 1, dst, nn);
}
waa_status waa_analyser_get_float_time_domain_data(waa_batch* b, uint32_t node, uint32_t inst, float* dst, uint32_t nn) {
  if (int e = an_inst(b, inst)) return e;
  return analyser_rows(b, node, AN_TIME, inst, inst + 1, dst, nn);
}
waa_status waa_analyser_get_byte_time_domain_data(waa_batch* b, uint32_t node, uint32_t inst, uint8_t* dst, uint32_t nn) {
  if (int e = an_inst(b, inst)) return e;
  return analyser_byte_time_rows(b, node, inst, inst + 1, dst, nn);
}
waa_status waa_analyser_get_float_frequency_data_batch(waa_batch* b, uint32_t node, float* dst, uint32_t nn) {
  if (!b) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch");
  return analyser_rows(b, node, AN_DB, 0, b->n_inst, dst, nn);
}
waa_status waa_analyser_get_byte_frequency_data_batch(waa_batch* b, uint32_t node, uint8_t* dst, uint32_t nn) {
  if (!b) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch");
  return analyser_rows(b, node, AN_BYTES, 0, b->n_inst, dst, nn);
}
waa_status waa_analyser_get_float_time_domain_data_batch(waa_batch* b, uint32_t node, float* dst, uint32_t nn) {
  if (!b) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch");
  return analyser_rows(b, node, AN_TIME, 0, b->n_inst, dst, nn);
}
waa_status waa_analyser_get_byte_time_domain_data_batch(waa_batch* b, uint32_t node, uint8_t* dst, uint32_t nn) {
  if (!b) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch");
  return analyser_byte_time_rows(b, node, 0, b->n_inst, dst, nn);
}

// buffer.rs:311-363 (input prep, host side)
uint64_t waa_buffer_resample(const float* src, uint64_t frames, float source_sr, float target_sr, float* dst, uint64_t cap) {
  if (std::fabs(source_sr - target_sr) <= 0.1f || frames == 0) {
    if (dst)
      for (uint64_t i = 0; i < frames && i < cap; i++) dst[i] = src[i];
    return frames;
  }
  const double ratio = (double)target_sr / (double)source_sr;
  const uint64_t tl = (uint64_t)std::ceil((double)frames * ratio);
  if (!dst) return tl;
  for (uint64_t i = 0; i < tl && i < cap; i++) {
    const double position = (double)i / (double)(tl - 1);
    const double playhead = position * (double)(frames - 1);
    const double pf = std::floor(playhead);
    const uint64_t prev = (uint64_t)pf;
    const uint64_t next = std::min<uint64_t>(prev + 1, frames - 1);
    const float k = (float)(playhead - pf), kinv = 1.f - k;
    dst[i] = kinv * src[prev] + k * src[next];
  }
  return tl;
}

// When the reference dispatches `ended` for a scheduled source (host-side replay of the renderers' scheduling;
// processor.rs:53-58, thread.rs:398-411)
waa_status waa_source_ended(waa_batch* b, uint32_t node, uint32_t inst, int64_t* quantum) {
  if (!b || node >= b->nodes.size() || !quantum) return fail(WAA_ERR_INVALID_ARGUMENT, "bad node");
  Node& n = b->nodes[node];
  const uint32_t kind = n.desc.kind;
  if (kind != WAA_NODE_BUFFER_SOURCE && kind != WAA_NODE_CONSTANT_SOURCE && kind != WAA_NODE_OSCILLATOR)
    return fail(WAA_ERR_INVALID_ARGUMENT, "node %u is not a scheduled source", node);
  if (inst >= b->n_inst) return fail(WAA_ERR_INVALID_ARGUMENT, "instance %u out of range", inst);
  if (!b->planned) {  // automation of playbackRate / detune is evaluated by the planner
    if (!b->dry) HIP_TRY(hipSetDevice(b->device));
    int e = build_plan(b);
    if (e) return e;
  }
  const SourceSched& ss = n.sched[inst];
  const double sr = (double)b->sr, dt = 1. / sr;
  const double end_time = (double)((uint64_t)b->n_quanta * RQ) / sr;
  *quantum = WAA_ENDED_NEVER;
  if (kind == WAA_NODE_BUFFER_SOURCE) {
    const DeviceBuffer& bf = n.bufs[inst];
    SchedOut so;
    schedule_source(b, ss, bf.frames, bf.sr, bf.valid, param_per_quantum(b, n.params[WAA_PARAM_SOURCE_PLAYBACK_RATE], inst, nullptr),
                    param_per_quantum(b, n.params[WAA_PARAM_SOURCE_DETUNE], inst, nullptr), &so);
    if (so.ended_quantum >= 0)
      *quantum = so.ended_quantum;
    else if (so.ended_at_unload)
      *quantum = WAA_ENDED_AT_UNLOAD;
    return WAA_OK;
  }
  // ConstantSource (constant_source.rs:204-262) and Oscillator (oscillator.rs:382-465): the first quantum whose end
  // reaches the stop time (the oscillator also tests the start of the quantum)
  for (uint32_t q = 0; q < b->n_quanta; q++) {
    const double ct = (double)((uint64_t)q * RQ) / sr, nbt = ct + dt * (double)RQ;
    if ((kind == WAA_NODE_OSCILLATOR && ss.stop <= ct) || ss.stop <= nbt) {
      *quantum = q;
      return WAA_OK;
    }
  }
  if (end_time >= ss.start || end_time >= ss.stop) *quantum = WAA_ENDED_AT_UNLOAD;
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
