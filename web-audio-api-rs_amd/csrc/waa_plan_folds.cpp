// waa_plan_folds.cpp — which nodes get a signal of their own and which are folded into a neighbour: the single source in front
// of a frozen-state node, block-scheduled loops, DelayNodes read from their line by their consumers, materialisation points,
// sources and gains that ride on an input edge, BufferSources read in place, a Biquad folded into the Convolver behind it.
// The passes run in this order (build_plan_rest); each reads what the ones above it decided.
#include "waa_host.hpp"
#include "waa_plan_parts.hpp"

namespace waa {
namespace host {

// Nodes whose state freezes while they do not process (WaveShaper 2x / 4x, HRTF panner; waa_frozen.hip) follow the
// per-quantum silence / count codes of their input EXACTLY.  Directly behind one source those codes are host-known
// (the scheduling replay); behind anything else they come out of the dynamic-count rendering.
void choose_frozen_sources(waa_batch* b, PlanPass& pass) {
  const uint32_t N = (uint32_t)b->nodes.size();
  pass.frozen_src.assign(N, -1);
  for (uint32_t id = 0; id < N && !pass.dynamic(b); id++) {
    Node& n = b->nodes[id];
    if (!n.live || !is_frozen_node(n)) continue;
    bool simple = n.in_edges.size() == 1 && pass.scc_of[id] < 0 && !measure_switch("WAA_FROZEN_DYNAMIC");
    if (simple) {
      const uint32_t p = b->edges[n.in_edges[0]].from;
      const uint32_t pk = b->nodes[p].desc.kind;
      simple = (pk == WAA_NODE_BUFFER_SOURCE || pk == WAA_NODE_CONSTANT_SOURCE || pk == WAA_NODE_OSCILLATOR) &&
               b->nodes[p].out_nch == n.in_nch && n.in_nch <= (n.desc.kind == WAA_NODE_WAVESHAPER ? 6 : 2);
      if (simple) pass.frozen_src[id] = (int)p;
    }
    if (!simple && !measure_switch("WAA_STATIC_CHANNEL_COUNTS")) {
      plan_note(b, "node %u keeps frozen state over silent quanta and is not fed by a single source -> exact per-quantum codes (dyn_kernel)", id);
      pass.count_change_found = true;
    }
  }
}

// A feedback loop whose loop-breaking delays are all longer than a block of tiles is rendered block by block with the kernels
// of a static plan (loop_block_tiles, waa_plan_loops.cpp); static plans only.
void choose_block_loops(waa_batch* b, PlanPass& pass) {
  pass.scc_block.assign((size_t)pass.n_scc, 0);
  if (pass.dynamic(b) || measure_switch("WAA_NO_LOOP_FOLD")) return;
  for (int sc = 0; sc < pass.n_scc; sc++) {
    std::vector<uint32_t> loop_items;
    for (uint32_t v : pass.items)
      if (pass.scc_of[v & ~VTX_READER] == sc) loop_items.push_back(v);
    pass.scc_block[(size_t)sc] = loop_block_tiles(b, loop_items);
  }
}

// A DelayNode outside a feedback loop whose delayTime is one value per quantum and whose consumers are all input
// stages of chain kernels is not rendered by a pass of its own: the consumers gather from the delay line (IN_DELAYED).
// (Static plans only; an echo — source -> Delay -> Gain -> bus — then costs one pass instead of three.)
// Inside a feedback loop the same holds when the loop is block-scheduled (every loop-breaking delay longer than a block:
// the gather then only reaches into earlier blocks), and a GainNode of such a loop can ride on an input edge like
// outside: the classic echo loop Delay <-> Gain is ONE launch per block (line = source + gain * delayed(line)).
void choose_folded_delays(waa_batch* b, const PlanPass& pass) {
  const uint32_t N = (uint32_t)b->nodes.size();
  const std::vector<int>& scc_of = pass.scc_of;
  for (uint32_t id = 0; id < N; id++) {
    Node& n = b->nodes[id];
    n.delay_folded = false;
    if (!n.live || n.desc.kind != WAA_NODE_DELAY || pass.dynamic(b) || measure_switch("WAA_NO_DELAY_FOLD")) continue;
    if ((scc_of[id] >= 0 || (id < b->cut.size() && b->cut[id])) && !pass.block_loop(id)) continue;
    const ParamStore& dt = n.params[WAA_PARAM_DELAY_DELAY_TIME];
    bool ok = dt.mode() != 2 && n.in_edges.size() >= 1;
    if ((size_t)WAA_PARAM_DELAY_DELAY_TIME < n.pin_edges.size() && !n.pin_edges[WAA_PARAM_DELAY_DELAY_TIME].empty()) ok = false;
    int consumers = 0;
    for (auto& e : b->edges) {
      if (e.from != id || !b->nodes[e.to].live) continue;
      consumers++;
      const Node& c = b->nodes[e.to];
      const uint32_t ck = c.desc.kind;
      const bool other_loop = scc_of[e.to] >= 0 && !(scc_of[e.to] == scc_of[id] && pass.block_loop(id));
      if ((e.to_input & 0x80000000u) || other_loop || (ck == WAA_NODE_CONVOLVER && c.has_ir) || is_frozen_node(c) || is_compressor(c) || is_shaper_per_instance(c) || c.in_nch > 2 ||
          n.out_nch > 2 || is_routing_node(c))
        ok = false;
    }
    n.delay_folded = ok && consumers > 0;
  }
}

// materialisation points: the nodes whose output is a signal in memory
void choose_materialisation(waa_batch* b, PlanPass& pass) {
  const uint32_t N = (uint32_t)b->nodes.size();
  const std::vector<int>& scc_of = pass.scc_of;
  pass.mat_hard.assign(N, 0);
  pass.fan_in_only.assign(N, 0);
  for (uint32_t id = 0; id < N; id++) {
    Node& n = b->nodes[id];
    if (!n.live) continue;
    if (n.delay_folded) {
      n.materialized = false;
      continue;
    }
    bool mat = false, fan = false;
    const uint32_t kind = n.desc.kind;
    if (kind == WAA_NODE_DESTINATION || kind == WAA_NODE_ANALYSER || kind == WAA_NODE_CONVOLVER || kind == WAA_NODE_DELAY) mat = true;
    if (is_frozen_node(n)) mat = true;  // rendered node-major (waa_frozen.hip)
    if (is_compressor(n)) mat = true;   // rendered node-major (waa_compressor.hip)
    if (is_shaper_per_instance(n)) mat = true;  // rendered node-major (waa_shaper_inst.hip)
    if (is_routing_node(n)) mat = true; // views / one route launch (waa_plan_route.cpp)
    // (a GainNode of a block-scheduled loop may ride on an input edge of its consumer, see choose_folded_delays)
    const bool relaxed = kind == WAA_NODE_GAIN && pass.block_loop(id);
    if (scc_of[id] >= 0 && !relaxed) mat = true;  // loop members publish their own signal
    if (kind == WAA_NODE_OSCILLATOR) mat = true;  // rendered by its own (lane-per-instance) kernel
    int live_consumers = 0;
    for (auto& e : b->edges)
      if (e.from == id && b->nodes[e.to].live) {
        live_consumers++;
        const Node& c = b->nodes[e.to];
        if ((c.desc.kind == WAA_NODE_CONVOLVER && c.has_ir) || is_frozen_node(c) || is_compressor(c) || is_shaper_per_instance(c)) mat = true;
        if (is_routing_node(c)) mat = true;  // the route launch and the port views read whole signals
        if (c.desc.kind == WAA_NODE_DELAY) {
          // a DelayNode mixes its inputs like a summing chain head (node_input_signal): materialised unless foldable
          if (relaxed)
            fan = true;
          else
            mat = true;
        }
        if (e.to_input & 0x80000000u) {
          // feeds an AudioParam: read back as a per-frame value signal — except a plain GainNode (the depth of an LFO),
          // which rides on the input edge of the param's summing chain like on any other summing input
          if (kind == WAA_NODE_GAIN && scc_of[id] < 0 && !pass.dynamic(b) && !measure_switch("WAA_NO_EDGE_FOLD"))
            fan = true;
          else
            mat = true;
        }
        if (scc_of[e.to] >= 0 && !(relaxed && scc_of[e.to] == scc_of[id])) mat = true;  // feeds a feedback loop
        int live_in = 0;
        for (int ie : c.in_edges)
          if (b->nodes[b->edges[ie].from].live) live_in++;
        if (live_in > 1) fan = true;
      }
    if (live_consumers != 1) mat = true;
    pass.mat_hard[id] = mat;
    pass.fan_in_only[id] = !mat && fan;
    n.materialized = mat || fan;
  }
}

// A producer that is materialised ONLY because its single consumer sums several inputs can instead be folded
// into that consumer's input stage: a source is fetched by the summing kernel itself, and a GainNode on a
// materialised signal (or on a source) becomes a per-edge gain — the mixer pattern source->Gain->bus costs no
// pass through HBM of its own.
void fold_fan_in_edges(waa_batch* b, const PlanPass& pass) {
  const uint32_t N = (uint32_t)b->nodes.size();
  auto is_source_kind = [](uint32_t k) { return k == WAA_NODE_BUFFER_SOURCE || k == WAA_NODE_CONSTANT_SOURCE; };
  if (measure_switch("WAA_NO_EDGE_FOLD")) return;
  for (uint32_t id = 0; id < N; id++) {
    Node& n = b->nodes[id];
    if (!n.live || !pass.fan_in_only[id]) continue;
    if (is_source_kind(n.desc.kind)) {
      n.materialized = false;
      continue;
    }
    if (n.desc.kind != WAA_NODE_GAIN || n.in_edges.size() != 1 || n.in_nch != n.out_nch) continue;
    bool modulated = false;
    for (auto& pe : n.pin_edges) modulated |= !pe.empty();
    if (modulated) continue;
    const uint32_t x = b->edges[n.in_edges[0]].from;
    const Node& xn = b->nodes[x];
    if (!xn.live || xn.out_nch != n.in_nch) continue;
    // x is either materialised for its own reasons, or a source whose only consumer is this gain
    if (pass.mat_hard[x] || xn.delay_folded || (is_source_kind(xn.desc.kind) && !pass.fan_in_only[x])) n.materialized = false;
  }
}

// Does BufferSource `n` render its AudioBuffer unchanged — fast track from frame 0: start 0, no offset / duration / stop /
// loop, playbackRate 1, detune 0, buffer at the context's rate, one layout for all instances?  Then `view` is that buffer as
// a signal (instance stride 0: one AudioBuffer shared by every instance, set_buffer(ALL)).
static bool source_is_its_buffer(const waa_batch* b, const Node& n, SignalRef* view) {
  const ParamStore& pr = n.params[WAA_PARAM_SOURCE_PLAYBACK_RATE];
  const ParamStore& pd = n.params[WAA_PARAM_SOURCE_DETUNE];
  bool ok = pr.blocks.empty() && pd.blocks.empty() && pr.timelines.empty() && pd.timelines.empty() && !pr.dev_tl && !pd.dev_tl;
  const DeviceBuffer& b0 = n.bufs[0];
  ok = ok && b0.valid && b0.sr == b->sr && (uintptr_t)b0.base % 16 == 0 && b0.ch_stride % 4 == 0 && b0.frames % RQ == 0 && b0.frames > 0;
  const int64_t inst_stride = b->n_inst > 1 && n.bufs[1].valid ? n.bufs[1].base - b0.base : (int64_t)b0.ch_stride * b0.nch;
  ok = ok && inst_stride >= 0 && inst_stride % 4 == 0;
  for (uint32_t i = 0; i < b->n_inst && ok; i++) {
    const DeviceBuffer& bf = n.bufs[i];
    const SourceSched& ss = n.sched[i];
    ok = bf.valid && bf.base == b0.base + (int64_t)i * inst_stride && bf.ch_stride == b0.ch_stride && bf.frames == b0.frames &&
         bf.nch == b0.nch && bf.sr == b0.sr && pr.cst[i] == 1.f && pd.cst[i] == 0.f && ss.start == 0. && ss.stop == DBL_MAX &&
         ss.offset == 0. && ss.duration == DBL_MAX && !ss.looping;
  }
  if (ok) *view = SignalRef{b0.base, (uint64_t)inst_stride, b0.ch_stride, (int32_t)b0.nch, 0};
  return ok;
}

// A BufferSource whose output IS its AudioBuffer (source_is_its_buffer) and whose single consumer is a node-major step that
// accepts a bounded view: read in place, no copy through HBM.
void choose_source_views(waa_batch* b, const PlanPass& pass) {
  const uint32_t N = (uint32_t)b->nodes.size();
  const std::vector<int>& scc_of = pass.scc_of;
  for (uint32_t id = 0; id < N && !measure_switch("WAA_NO_SOURCE_VIEW"); id++) {
    Node& n = b->nodes[id];
    n.is_view = false;
    if (!n.live || n.desc.kind != WAA_NODE_BUFFER_SOURCE || !n.materialized || pass.dynamic(b)) continue;
    int consumer = -1, n_live = 0;
    for (auto& e : b->edges)
      if (e.from == id && b->nodes[e.to].live) {
        n_live++;
        consumer = (e.to_input & 0x80000000u) ? -1 : (int)e.to;
      }
    // ... or whose consumers are all summing input stages (chain heads, DelayNode mixes: they fetch a source themselves)
    // and folded single-input DelayNodes (whose delay line the source's buffer then IS): no copy either
    bool shared_ok = n_live >= 2;
    for (auto& e : b->edges) {
      if (e.from != id || !b->nodes[e.to].live || !shared_ok) continue;
      const Node& c = b->nodes[e.to];
      const uint32_t ck = c.desc.kind;
      if ((e.to_input & 0x80000000u) || (scc_of[e.to] >= 0 && !pass.block_loop(e.to)) || (ck == WAA_NODE_CONVOLVER && c.has_ir) ||
          is_frozen_node(c) || is_compressor(c) || is_shaper_per_instance(c) || ck == WAA_NODE_IIR_FILTER || is_routing_node(c))
        shared_ok = false;
    }
    if (!shared_ok && (n_live != 1 || consumer < 0)) continue;
    const Node& c = b->nodes[(uint32_t)(shared_ok ? 0 : consumer)];
    const bool conv = !shared_ok && ((c.desc.kind == WAA_NODE_CONVOLVER && c.has_ir) || is_compressor(c) || is_shaper_per_instance(c));  // (all take a bounded view)
    bool frozen_ok = shared_ok;
    if (!shared_ok && is_frozen_node(c) && pass.frozen_src[(uint32_t)consumer] == (int)id)
      // (a shaper that processes silent quanta would read them from the view: copy instead)
      frozen_ok = c.desc.kind == WAA_NODE_PANNER || std::fabs(curve_at_zero(c)) < 1e-9f;
    if (!(conv || frozen_ok)) continue;
    if (!shared_ok && (c.in_edges.size() != 1 || c.in_nch != n.out_nch || scc_of[(uint32_t)consumer] >= 0)) continue;
    SignalRef view;
    bool ok = source_is_its_buffer(b, n, &view);
    // ... and every quantum the reference renders as ACTIVE lies inside the buffer.  The quantum right behind a buffer that ends on
    // a quantum boundary can be one: the source's clock reaches the duration by additions of dt, and where it still compares below it
    // the renderer produces one more quantum — of zeros, but not the silent block — before it ends (audio_buffer_source.rs:560-600).
    // Read in place that quantum is the next context's first one (frozen-state fuzz seed 38723, round 6: a 2304-frame buffer in
    // front of an HRTF panner; 0.2 of full scale for two of three contexts in the panner's tail).
    const ParamStore& pr = n.params[WAA_PARAM_SOURCE_PLAYBACK_RATE];
    const ParamStore& pd = n.params[WAA_PARAM_SOURCE_DETUNE];
    for (uint32_t i = 0; i < b->n_inst && ok; i++) {
      const DeviceBuffer& bf = n.bufs[i];
      const SourceSched& ss = n.sched[i];
      const SchedKey key(ss.start, ss.stop, ss.offset, ss.duration, ss.looping, ss.loop_start, ss.loop_end, bf.frames, bf.sr, pr.fix(pr.cst[i]),
                         pd.fix(pd.cst[i]));
      const auto so = schedule_source_cached(b, id, key, ss, bf.frames, bf.sr, true, param_per_quantum(b, pr, i, nullptr), param_per_quantum(b, pd, i, nullptr));
      for (size_t q = 0; q < so->qrec.size() && ok; q++)
        if (so->qrec[q].mode != Q_SILENT)
          ok = so->qrec[q].mode == Q_FAST && so->qrec[q].start == (int64_t)q * RQ && (uint64_t)(q + 1) * RQ <= bf.frames;
    }
    if (!ok) continue;
    const uint64_t frames = n.bufs[0].frames;
    n.is_view = true;
    n.materialized = false;
    n.view_sig = view;
    n.view_valid = frames;
    if (shared_ok)
      plan_note(b, "source node %u renders its AudioBuffer unchanged: its %d consumers read it in place (%llu frames per channel)", id, n_live,
                (unsigned long long)frames);
    else
      plan_note(b, "source node %u renders its AudioBuffer unchanged: node %d reads it in place (%llu frames per channel)", id, consumer,
                (unsigned long long)frames);
  }
}

// A BiquadFilterNode with constant coefficients directly in front of a long ConvolverNode (source -> Biquad -> Convolver,
// the north-star graph): the forward transform's input stage filters its blocks itself (conv_fft3_fwd_bq_kernel) — the
// filtered signal never crosses HBM and the Biquad costs no launch.  Its own input must be a plain signal: a
// BufferSource that renders its AudioBuffer unchanged (read in place) or a signal some other node materialises anyway.
void fold_biquad_into_convolver(waa_batch* b, const PlanPass& pass) {
  const uint32_t N = (uint32_t)b->nodes.size();
  const std::vector<int>& scc_of = pass.scc_of;
  for (auto& n : b->nodes) n.fold_conv = n.pre_biquad = -1;
  if (pass.dynamic(b) || measure_switch("WAA_NO_CONV_BIQUAD_FOLD") || measure_switch("WAA_CONV_FFT_R4")) return;
  for (uint32_t cid = 0; cid < N; cid++) {
    Node& c = b->nodes[cid];
    if (!c.live || c.desc.kind != WAA_NODE_CONVOLVER || !c.has_ir || scc_of[cid] >= 0 || c.in_edges.size() != 1) continue;
    if (conv_block_size(b, c) != 8192) continue;
    const uint32_t qid = b->edges[c.in_edges[0]].from;
    Node& q = b->nodes[qid];
    if (!q.live || q.desc.kind != WAA_NODE_BIQUAD || scc_of[qid] >= 0 || q.in_nch != q.out_nch || q.out_nch != c.in_nch || q.in_nch > 2 ||
        q.in_edges.size() != 1)
      continue;
    int q_consumers = 0;
    for (auto& e : b->edges) q_consumers += e.from == qid && b->nodes[e.to].live;
    bool plain = q_consumers == 1;
    for (auto& pe : q.pin_edges) plain = plain && pe.empty();
    for (auto& ps : q.params) plain = plain && ps.mode() == 0 && ps.timelines.empty() && !ps.dev_tl;
    if (!plain) continue;
    const uint32_t sid = b->edges[q.in_edges[0]].from;
    Node& sn = b->nodes[sid];
    if (!sn.live || sn.out_nch != q.in_nch) continue;
    if (sn.desc.kind == WAA_NODE_BUFFER_SOURCE && !sn.materialized && !sn.is_view && !measure_switch("WAA_NO_SOURCE_VIEW")) {
      int s_consumers = 0;
      for (auto& e : b->edges) s_consumers += e.from == sid && b->nodes[e.to].live;
      bool ok = s_consumers == 1;
      for (auto& pe : sn.pin_edges) ok = ok && pe.empty();
      SignalRef view;
      if (!ok || !source_is_its_buffer(b, sn, &view)) continue;
      sn.is_view = true;
      sn.view_sig = view;
      sn.view_valid = sn.bufs[0].frames;
    } else if (!(pass.mat_hard[sid] && !sn.is_view && !sn.delay_folded)) {
      continue;
    }
    q.fold_conv = (int)cid;
    q.materialized = false;
    c.pre_biquad = (int)qid;
    if (conv_fold_biquad_into_ir(b, c, q))
      plan_note(b, "biquad node %u has the same constant coefficients on every context and only feeds convolver node %u: both are LTI, its "
                   "transfer function is folded into the impulse response (%llu -> %llu taps)%s",
                qid, cid, (unsigned long long)c.ir_len, (unsigned long long)c.ir_lti_len, sn.is_view ? " (its source is read in place)" : "");
    else
      plan_note(b, "biquad node %u has constant coefficients and only feeds convolver node %u: filtered by the forward transform's input stage%s",
                qid, cid, sn.is_view ? " (its source is read in place)" : "");
  }
}

}  // namespace host
}  // namespace waa
