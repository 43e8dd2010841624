// waa_plan_graph.cpp — the planner's graph analysis: processing order with the reference's cycle breaker, feedback loops,
// incoming edges in summing order, liveness, static channel counts, planning units.  Nothing here touches the device.
#include "waa_host.hpp"
#include "waa_plan_parts.hpp"

namespace waa {
namespace host {

// graph.rs:323-487 order_nodes / visit.  A DelayNode is two graph nodes in the reference (delay.rs:283-366:
// writer, then reader, edge writer->reader); vertex `id` is the writer (or a plain node), `id | VTX_READER` the
// reader.  Cycles are broken at the first DelayNode writer on the detected loop (its writer->reader edge is
// cleared and the ordering restarts); nodes of a loop without one are dropped from the ordering (muted).
struct OrderCtx {
  const waa_batch* b;
  std::vector<uint8_t> cut;
  std::vector<uint32_t> marked, temp, ordered, in_cycle;
  uint32_t breaker = 0;
};
bool order_visit(OrderCtx& c, uint32_t v) {
  auto pos = std::find(c.temp.begin(), c.temp.end(), v);
  if (pos != c.temp.end()) {
    for (auto it = pos; it != c.temp.end(); ++it)
      if (!(*it & VTX_READER) && is_delay(c.b, *it)) {
        c.breaker = *it;
        return true;
      }
    c.in_cycle.insert(c.in_cycle.end(), pos, c.temp.end());
    return false;
  }
  if (std::find(c.marked.begin(), c.marked.end(), v) != c.marked.end()) return false;
  c.marked.push_back(v);
  c.temp.push_back(v);
  std::vector<uint32_t> targets;
  vertex_targets(c.b, v, c.cut, targets);
  for (uint32_t t : targets)
    if (order_visit(c, t)) return true;
  c.ordered.push_back(v);
  c.temp.erase(std::remove(c.temp.begin(), c.temp.end(), v), c.temp.end());
  return false;
}

bool is_delay(const waa_batch* b, uint32_t id) { return b->nodes[id].desc.kind == WAA_NODE_DELAY; }
// outgoing edges of a vertex of the expanded graph, in insertion order
void vertex_targets(const waa_batch* b, uint32_t v, const std::vector<uint8_t>& cut, std::vector<uint32_t>& out) {
  const uint32_t id = v & ~VTX_READER;
  if (!(v & VTX_READER) && is_delay(b, id)) {
    if (!cut[id]) out.push_back(id | VTX_READER);
    return;
  }
  for (auto& e : b->edges) {
    if (e.from != id) continue;
    // inputs go to the writer half; delayTime belongs to the reader half (delay.rs:316-318)
    out.push_back(is_delay(b, e.to) && (e.to_input & 0x80000000u) ? (e.to | VTX_READER) : e.to);
  }
}

// graph.rs:323-487 for the batch's current nodes and edges: which DelayNodes lose their writer->reader edge (`cut`), which nodes
// sit in a cycle without one (`muted`), and the render order (two entries per DelayNode: writer, reader; none for muted nodes)
void compute_order(const waa_batch* b, std::vector<uint8_t>* cut_out, std::vector<uint8_t>* muted_out, std::vector<uint32_t>* items_out) {
  const uint32_t N = (uint32_t)b->nodes.size();
  std::vector<uint32_t>& items = *items_out;
  std::vector<uint8_t>& muted = *muted_out;
  items.clear();
  muted.assign(N, 0);
  OrderCtx c;
  c.b = b;
  c.cut.assign(N, 0);
  for (;;) {
    c.marked.clear();
    c.temp.clear();
    c.ordered.clear();
    c.in_cycle.clear();
    bool applied = false;
    for (uint32_t i = 0; i < N && !applied; i++) {
      applied = order_visit(c, i);
      if (!applied && is_delay(b, i)) applied = order_visit(c, i | VTX_READER);
      // the AudioListener is the reference's graph node 1, right behind the destination, with an edge to every
      // PannerNode in creation order (concrete_base.rs:511-534): visited as a DFS root it pulls the panner branches
      // to the front of the traversal, i.e. to the back of the reversed post-order — which decides the f32 summing
      // order wherever three or more signals meet
      if (i == 0)
        for (uint32_t pn = 0; pn < N && !applied; pn++)
          if (b->nodes[pn].desc.kind == WAA_NODE_PANNER) applied = order_visit(c, pn);
    }
    if (!applied) break;
    c.cut[c.breaker] = 1;
  }
  for (uint32_t v : c.in_cycle) muted[v & ~VTX_READER] = 1;
  for (auto it = c.ordered.rbegin(); it != c.ordered.rend(); ++it)
    if (!muted[*it & ~VTX_READER]) items.push_back(*it);
  *cut_out = c.cut;
}

// Feedback loops: strongly connected components of the graph with the writer->reader edges in place (Tarjan); their
// members are rendered quantum by quantum by the loop kernel, or block by block.
namespace {
struct Tarjan {
  const waa_batch* b;
  const std::vector<uint8_t>& muted;
  const uint32_t N;
  std::vector<int> index, low, comp, comp_size;
  std::vector<uint8_t> on;
  std::vector<uint32_t> stk;
  const std::vector<uint8_t> no_cut;
  int counter = 0, n_comp = 0;
  Tarjan(const waa_batch* b_, const std::vector<uint8_t>& muted_)
      : b(b_), muted(muted_), N((uint32_t)b_->nodes.size()), index(2 * N, -1), low(2 * N, 0), comp(2 * N, -1), on(2 * N, 0), no_cut(N, 0) {}
  uint32_t vidx(uint32_t v) const { return (v & VTX_READER) ? N + (v & ~VTX_READER) : v; }
  void strong(uint32_t v) {
    const uint32_t vi = vidx(v);
    index[vi] = low[vi] = counter++;
    stk.push_back(v);
    on[vi] = 1;
    std::vector<uint32_t> ts;
    vertex_targets(b, v, no_cut, ts);
    for (uint32_t t : ts) {
      if (muted[t & ~VTX_READER]) continue;
      const uint32_t ti = vidx(t);
      if (index[ti] < 0) {
        strong(t);
        low[vi] = std::min(low[vi], low[ti]);
      } else if (on[ti]) {
        low[vi] = std::min(low[vi], index[ti]);
      }
    }
    if (low[vi] == index[vi]) {
      int size = 0;
      for (;;) {
        const uint32_t w = stk.back();
        stk.pop_back();
        on[vidx(w)] = 0;
        comp[vidx(w)] = n_comp;
        size++;
        if (w == v) break;
      }
      comp_size.push_back(size);
      n_comp++;
    }
  }
};
}  // namespace
void find_loops(const waa_batch* b, PlanPass& pass) {
  const uint32_t N = (uint32_t)b->nodes.size();
  pass.scc_of.assign(N, -1);
  pass.n_scc = 0;
  Tarjan t(b, pass.muted);
  for (uint32_t i = 0; i < N; i++) {
    if (pass.muted[i]) continue;
    if (t.index[i] < 0) t.strong(i);
    if (is_delay(b, i) && t.index[N + i] < 0) t.strong(i | VTX_READER);
  }
  std::map<int, int> renum;
  for (uint32_t i = 0; i < N; i++) {
    if (pass.muted[i] || t.comp[i] < 0 || t.comp_size[t.comp[i]] < 2) continue;
    auto it = renum.find(t.comp[i]);
    if (it == renum.end()) it = renum.emplace(t.comp[i], pass.n_scc++).first;
    pass.scc_of[i] = it->second;
  }
}

// Incoming edges in summing order: by processing position of the producer, then edge insertion order.  Refuses the edges into
// AudioParams that no kernel reads per frame.
int collect_edges(waa_batch* b, const PlanPass& pass) {
  const std::vector<uint8_t>& muted = pass.muted;
  std::vector<uint32_t> pos(b->nodes.size(), 0xffffffffu);
  for (uint32_t i = 0; i < b->order.size(); i++) pos[b->order[i]] = i;
  for (auto& n : b->nodes) {
    n.in_edges.clear();
    n.pin_edges.assign(n.params.size(), {});
    n.pin_ref.assign(n.params.size(), ParamRef{});
    n.pin_ready.assign(n.params.size(), 0);
    n.n_consumers = 0;
    n.live = n.materialized = false;
  }
  for (uint32_t e = 0; e < b->edges.size(); e++) {
    const waa_edge_desc& ed = b->edges[e];
    Node& to = b->nodes[ed.to];
    if (muted[ed.from] || muted[ed.to]) continue;  // a muted node renders nothing and contributes nothing
    if (ed.to_input & 0x80000000u) {
      const uint32_t pid = ed.to_input & 0x7fffffffu;
      if (pid >= to.params.size()) return fail(WAA_ERR_INVALID_ARGUMENT, "IndexSizeError - node %u has no param %u", ed.to, pid);
      const uint32_t k = to.desc.kind;
      const bool source_rate = k == WAA_NODE_BUFFER_SOURCE && (pid == WAA_PARAM_SOURCE_PLAYBACK_RATE || pid == WAA_PARAM_SOURCE_DETUNE);
      if (source_rate && !b->prepass)  // (with a device these edges are resolved before the plan is built, waa_plan_prepass.cpp)
        return fail(WAA_ERR_OUT_OF_SCOPE,
                    "playbackRate / detune of source node %u are modulated from the graph: the modulator is rendered at plan time, "
                    "which needs the device (plan-only batch)", ed.to);
      // PannerNode position / orientation with a single-valued AudioListener: the reference takes the FIRST value of every
      // param per quantum (panner.rs:833-846; HRTF: :781-829) — the same plan-time resolution (round 4).  Edges that are still
      // here outside the prepass were not resolved: an audio-rate listener next to them, or a plan-only batch.
      const bool panner_geom = k == WAA_NODE_PANNER && pid <= WAA_PARAM_PANNER_ORIENTATION_Z;
      if (panner_geom && !b->prepass)
        return fail(WAA_ERR_OUT_OF_SCOPE,
                    "position / orientation of panner node %u are modulated from the graph: resolved at plan time on the device for a "
                    "single-valued AudioListener only (audio-rate listener automation next to it, or a plan-only batch)", ed.to);
      if (k == WAA_NODE_DYNAMICS_COMPRESSOR)
        return fail(WAA_ERR_OUT_OF_SCOPE, "DynamicsCompressorNode %u: an edge into its AudioParam %u — the block constants of the node are computed on the host from "
                                          "host-known k-rate values (dynamics_compressor.rs:353-389): a param driven from the graph is out of scope", ed.to, pid);
      if (!(k == WAA_NODE_GAIN || k == WAA_NODE_BIQUAD || k == WAA_NODE_DELAY || k == WAA_NODE_STEREO_PANNER ||
            k == WAA_NODE_CONSTANT_SOURCE || k == WAA_NODE_OSCILLATOR || source_rate || panner_geom))
        return fail(WAA_ERR_OUT_OF_SCOPE, "audio-rate modulation of a host-evaluated param (node %u) is out of scope", ed.to);
      to.pin_edges[pid].push_back((int)e);
    } else {
      to.in_edges.push_back((int)e);
    }
    b->nodes[ed.from].n_consumers++;
  }
  auto by_position = [&](int x, int y) { return pos[b->edges[x].from] < pos[b->edges[y].from]; };
  for (auto& n : b->nodes) {
    std::stable_sort(n.in_edges.begin(), n.in_edges.end(), by_position);
    for (auto& pe : n.pin_edges) std::stable_sort(pe.begin(), pe.end(), by_position);
  }
  return 0;
}

// liveness: everything that reaches the destination or an analyser
void mark_live(waa_batch* b) {
  const uint32_t N = (uint32_t)b->nodes.size();
  std::vector<uint32_t> stack;
  for (uint32_t i = 0; i < N; i++)
    if (!b->prepass && (b->nodes[i].desc.kind == WAA_NODE_DESTINATION || b->nodes[i].desc.kind == WAA_NODE_ANALYSER)) stack.push_back(i);
  // (prepass: only what feeds the graph-modulated playbackRate / detune params)
  if (b->prepass)
    for (auto& pp : b->prepass_params) {
      // only what feeds the modulated PARAM: a PannerNode's audio input is not part of the prepass
      b->nodes[pp.first].live = true;
      for (int e : b->nodes[pp.first].pin_edges[pp.second]) stack.push_back(b->edges[e].from);
    }
  while (!stack.empty()) {
    uint32_t id = stack.back();
    stack.pop_back();
    if (b->nodes[id].live) continue;
    b->nodes[id].live = true;
    for (int e : b->nodes[id].in_edges) stack.push_back(b->edges[e].from);
    for (auto& pe : b->nodes[id].pin_edges)
      for (int e : pe) stack.push_back(b->edges[e].from);
  }
}

// The node kinds that only static plans outside feedback loops render: refused inside a loop (in_loops), and anywhere in a
// graph that needs the dynamic-count plan.  A WaveShaperNode with one curve per instance is one of them, and is refused with
// oversample 2x / 4x wherever it stands.
int refuse_static_only_nodes(waa_batch* b, const PlanPass& pass, bool in_loops) {
  const uint32_t N = (uint32_t)b->nodes.size();
  const char* where = in_loops ? "inside a feedback loop" : "in a graph that needs exact per-quantum channel counts (dyn_kernel)";
  auto here = [&](uint32_t i) { return b->nodes[i].live && (!in_loops || pass.scc_of[i] >= 0); };
  for (uint32_t i = 0; i < N; i++)
    if (here(i) && is_compressor(b->nodes[i]))
      return fail(WAA_ERR_OUT_OF_SCOPE, "DynamicsCompressorNode %u %s is out of scope: %s", i, where,
                  in_loops ? "its detector is rendered over the whole render by one launch, not quantum by quantum"
                           : "the node is rendered by static plans only");
  for (uint32_t i = 0; i < N; i++) {
    const Node& n = b->nodes[i];
    if (!n.live || !is_shaper_per_instance(n)) continue;
    // (wherever the node stands; asked once, by the first of the two calls)
    if (in_loops && n.desc.i[0] != WAA_OVERSAMPLE_NONE)
      return fail(WAA_ERR_OUT_OF_SCOPE, "WaveShaperNode %u with one curve per instance and oversample %s is out of scope: the oversampling transform stages "
                                        "its one curve in LDS per workgroup; per-instance curves are rendered with oversample none only",
                  i, n.desc.i[0] == WAA_OVERSAMPLE_X2 ? "2x" : "4x");
    if (here(i))
      return fail(WAA_ERR_OUT_OF_SCOPE, "WaveShaperNode %u with one curve per instance %s is out of scope: %s", i, where,
                  in_loops ? "the node is rendered over the whole render by one launch, not quantum by quantum"
                           : "per-instance curves are rendered by static plans only");
  }
  for (uint32_t i = 0; i < N; i++) {
    const uint32_t k = b->nodes[i].desc.kind;
    if (here(i) && (k == WAA_NODE_CHANNEL_SPLITTER || k == WAA_NODE_CHANNEL_MERGER))
      return fail(WAA_ERR_OUT_OF_SCOPE, "%s %u %s is out of scope: the node is rendered by static plans only%s",
                  k == WAA_NODE_CHANNEL_SPLITTER ? "ChannelSplitterNode" : "ChannelMergerNode", i, where,
                  in_loops ? ", over the whole render by views and one launch, not quantum by quantum" : "");
  }
  for (uint32_t i = 0; i < N; i++)
    if (here(i) && b->nodes[i].per_inst_ir() && b->nodes[i].has_ir)
      return fail(WAA_ERR_OUT_OF_SCOPE, "ConvolverNode %u with one impulse response per instance %s is out of scope: "
                                        "per-instance responses are rendered by static plans %sonly", i, where, in_loops ? "outside loops " : "");
  return 0;
}

// (prepass) a modulated source that itself feeds the modulating subgraph of a modulated source: its own schedule is
// not known before ITS modulation has been resolved — a second prepass level nobody has asked for yet; refused loudly
// (it used to be skipped by plan_single and the outer param chain read an empty signal)
int refuse_nested_source_modulation(const waa_batch* b) {
  const uint32_t N = (uint32_t)b->nodes.size();
  if (!b->prepass) return 0;
  for (auto& ed : b->edges) {
    if (ed.from >= N || ed.to >= N || !b->nodes[ed.to].live) continue;
    for (auto& pp : b->prepass_params)
      if (pp.first == ed.from)
        return fail(WAA_ERR_OUT_OF_SCOPE, "source node %u has a graph-modulated playbackRate / detune and feeds the modulation of source node %u: nested modulation of source rates is out of scope", ed.from, ed.to);
  }
  return 0;
}

// Static channel counts (the reference's counts are dynamic: a silent quantum is mono; every case the static count differs
// from the dynamic one carries zeros — see DESIGN.md "Silence and channel counts").  Instances that play AudioBuffers of
// different widths get the dynamic-count plan (b->force_dynamic).
int static_channel_counts(waa_batch* b, PlanPass& pass) {
  for (auto& n : b->nodes) n.in_nch = n.out_nch = 1;
  pass.mixed_buffer_counts = false;
  // (inside a feedback loop a producer can come later in the order: iterate to the fixed point; counts only grow)
  for (int it = 0; it < 16; it++) {
    bool changed = false;
    for (uint32_t id : b->order) {
      Node& n = b->nodes[id];
      if (!n.live) continue;
      const int old_in = n.in_nch, old_out = n.out_nch;
      int maxc = 1;
      for (int e : n.in_edges) maxc = std::max(maxc, b->nodes[b->edges[e].from].out_nch);
      n.in_nch = computed_in_nch(n, maxc);
      switch (n.desc.kind) {
        case WAA_NODE_BUFFER_SOURCE: {
          // instances may play AudioBuffers of different channel counts: the signal is laid out for the widest one, the
          // per-quantum codes of the dynamic-count plan carry every instance's own count (below: widen_narrow_buffers)
          uint32_t nch = 0;
          for (auto& bf : n.bufs)
            if (bf.valid) {
              if (nch && bf.count() != nch) pass.mixed_buffer_counts = true;
              nch = std::max(nch, bf.count());
            }
          n.out_nch = nch ? (int)nch : 1;
          break;
        }
        case WAA_NODE_CONSTANT_SOURCE:
        case WAA_NODE_OSCILLATOR: n.out_nch = 1; break;
        case WAA_NODE_STEREO_PANNER:
        case WAA_NODE_PANNER: n.out_nch = 2; break;
        case NODE_SPLITTER_PORT: n.out_nch = 1; break;              // channel_splitter.rs:198
        case WAA_NODE_CHANNEL_MERGER: n.out_nch = n.desc.i[0]; break;  // channel_merger.rs:160-165 (static: some input is active)
        case WAA_NODE_CONVOLVER:
          if (!n.has_ir)
            n.out_nch = n.in_nch;
          else
            n.out_nch = (n.in_nch == 1 && n.ir_nch == 1) ? 1 : 2;
          break;
        default: n.out_nch = n.in_nch; break;
      }
      if (n.in_nch > WAA_MAX_CHANNELS || n.out_nch > WAA_MAX_CHANNELS)
        return fail(WAA_ERR_OUT_OF_SCOPE, "at most %d channels per signal (node %u needs %d)", WAA_MAX_CHANNELS, id, std::max(n.in_nch, n.out_nch));
      changed |= n.in_nch != old_in || n.out_nch != old_out;
    }
    if (!changed || pass.n_scc == 0) break;
  }
  if (pass.mixed_buffer_counts) {
    // buffer.rs / audio_buffer_source.rs:560-600: the source's output has the channel count of ITS buffer; with several
    // counts in one batch no static count fits every instance -> the dynamic-count plan, whose codes are per instance
    if (measure_switch("WAA_STATIC_CHANNEL_COUNTS"))
      return fail(WAA_ERR_OUT_OF_SCOPE, "instances of one batch must use AudioBuffers with the same channel count (WAA_STATIC_CHANNEL_COUNTS)");
    if (b->prepass)
      return fail(WAA_ERR_OUT_OF_SCOPE, "the graph that modulates a host-evaluated param plays AudioBuffers of different channel counts across instances: out of scope");
    for (auto& n : b->nodes)
      if (n.live && n.desc.kind == WAA_NODE_BUFFER_SOURCE)
        if (int e = widen_narrow_buffers(b, n, (uint32_t)n.out_nch)) return e;
    b->force_dynamic = true;
  }
  return 0;
}

// Planning units: single nodes and whole feedback loops, producers first (the condensed graph is acyclic), otherwise in
// processing order.
static void visit_unit(const waa_batch* b, PlanPass& pass, std::vector<uint8_t>& node_done, std::vector<uint8_t>& scc_done, uint32_t id) {
  const std::vector<int>& scc_of = pass.scc_of;
  const int sc = scc_of[id];
  if (sc >= 0 ? scc_done[sc] : node_done[id]) return;
  std::vector<uint32_t> members;
  if (sc >= 0) {
    scc_done[sc] = 1;
    for (uint32_t m : b->order)
      if (scc_of[m] == sc) members.push_back(m);
  } else {
    node_done[id] = 1;
    members.push_back(id);
  }
  for (uint32_t m : members) {
    for (int e : b->nodes[m].in_edges)
      if (sc < 0 || scc_of[b->edges[e].from] != sc) visit_unit(b, pass, node_done, scc_done, b->edges[e].from);
    for (auto& pe : b->nodes[m].pin_edges)
      for (int e : pe)
        if (sc < 0 || scc_of[b->edges[e].from] != sc) visit_unit(b, pass, node_done, scc_done, b->edges[e].from);
  }
  pass.units.push_back(Unit{sc, id});
}
void order_units(const waa_batch* b, PlanPass& pass) {
  std::vector<uint8_t> node_done(b->nodes.size(), 0), scc_done(pass.n_scc, 0);
  pass.units.clear();
  for (uint32_t id : b->order) visit_unit(b, pass, node_done, scc_done, id);
}

}  // namespace host
}  // namespace waa
