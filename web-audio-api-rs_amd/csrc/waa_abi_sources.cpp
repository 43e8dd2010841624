// waa_abi_sources.cpp — the scheduled sources in the C ABI (include/waa_hip.h): AudioBuffers of AudioBufferSourceNodes (f32 planes,
// 16-bit PCM decoded on the device, device memory the caller owns), start / stop / loop, `ended`, and the host-side resampler.
#include "waa_host.hpp"

using namespace waa;
using namespace waa::host;

// BaseAudioContext::decode_audio_data_sync for decoded 16-bit PCM (decoding.rs:15-54): sample conversion and
// AudioBuffer::resample to the context's rate run on the device (waa_decode.hip); `planes` = [n_items][n_ch][stride]
int waa::host::decode_pcm16(waa_batch* b, const int16_t* pcm, uint32_t n_items, uint32_t n_ch, uint64_t frames, float src_sr,
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

extern "C" {

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
        if (int e2 = xfer_h2d(b, d + (size_t)c * stride, frames * sizeof(float), channels[c], frames * sizeof(float), frames * sizeof(float), 1)) return e2;
        HIP_TRY(hipStreamSynchronize(b->stream));
      }
    }
  *out = device_buffer(d, stride, frames, n_ch, sr);
  return 0;
}

waa_status waa_source_set_buffer(waa_batch* b, uint32_t node, uint32_t inst, const float* const* channels,
                                 uint32_t n_ch, uint64_t frames, float sr) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_BUFFER_SOURCE)) || (e = check_inst(b, inst)) || (e = check_unplanned(b))) return e;
  if ((e = check_channel_count(n_ch))) return e;
  if (!b->dry) HIP_TRY(hipSetDevice(b->device));
  DeviceBuffer db;
  if ((e = upload_buffer(b, channels, n_ch, frames, sr, &db))) return e;
  set_bufs(b->nodes[node], inst_range(inst, b->n_inst), db);
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
  if ((e = check_channel_count(n_ch))) return e;
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
  for (uint32_t k = 0; k < b->n_inst; k++) n.bufs[k] = device_buffer(d + (size_t)k * n_ch * stride, stride, frames, n_ch, sr);
  return WAA_OK;
}

waa_status waa_source_set_buffer_pcm16(waa_batch* b, uint32_t node, uint32_t inst, const int16_t* interleaved, uint32_t n_ch,
                                       uint64_t frames, float sr) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_BUFFER_SOURCE)) || (e = check_inst(b, inst)) || (e = check_unplanned(b))) return e;
  if ((e = check_channel_count(n_ch)) || (e = check_sample_rate(sr))) return e;
  if (!b->dry) HIP_TRY(hipSetDevice(b->device));
  float* d = nullptr;
  uint64_t stride = 0, target = 0;
  if ((e = decode_pcm16(b, interleaved, 1, n_ch, frames, sr, &d, &stride, &target))) return e;
  set_bufs(b->nodes[node], inst_range(inst, b->n_inst), device_buffer(d, stride, target, n_ch, b->sr));
  return WAA_OK;
}

waa_status waa_source_set_buffer_pcm16_batch(waa_batch* b, uint32_t node, const int16_t* data, uint32_t n_ch, uint64_t frames,
                                             float sr) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_BUFFER_SOURCE))) return e;
  if (b->planned && b->rearmed) return refill_source(b, node, 1, data, n_ch, frames, sr);
  if ((e = check_unplanned(b))) return e;
  if ((e = check_channel_count(n_ch)) || (e = check_sample_rate(sr))) return e;
  if (!b->dry) HIP_TRY(hipSetDevice(b->device));
  float* d = nullptr;
  uint64_t stride = 0, target = 0;
  b->batch_fill_node = (int64_t)node;  // (decode_pcm16 records the fill for waa_batch_rearm)
  e = decode_pcm16(b, data, b->n_inst, n_ch, frames, sr, &d, &stride, &target);
  b->batch_fill_node = -1;
  if (e) return e;
  Node& n = b->nodes[node];
  for (uint32_t k = 0; k < b->n_inst; k++) n.bufs[k] = device_buffer(d + (size_t)k * n_ch * stride, stride, target, n_ch, b->sr);
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
  for (uint32_t k = 0; k < b->n_inst; k++) n.bufs[k] = device_buffer(const_cast<float*>(device_data) + (size_t)k * n_ch * frames, frames, frames, n_ch, sr);
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
  const auto [lo, hi] = inst_range(inst, b->n_inst);
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
  const auto [lo, hi] = inst_range(inst, b->n_inst);
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
  const auto [lo, hi] = inst_range(inst, b->n_inst);
  for (uint32_t k = lo; k < hi; k++) {
    n.sched[k].looping = looping;
    n.sched[k].loop_start = ls;
    n.sched[k].loop_end = le;
  }
  return WAA_OK;
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
    // a target length of 1 makes position 0 / 0: Rust's `as usize` turns the NaN playhead into index 0 (a saturating cast; in
    // C++ the conversion of a NaN is undefined), k stays NaN and the one sample emitted is NaN
    const uint64_t prev = pf == pf ? (uint64_t)pf : 0;
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

}  // extern "C"
