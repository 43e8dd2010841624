// waa_plan_prepass.cpp — what happens to a batch's graph between the last control call and build_plan (plan_batch): connections
// made or cut at suspend points become gated ones, and k-rate params that the HOST evaluates but the graph modulates are rendered
// and read back first (the one planner pass that needs the device); settle_loops is the matching step behind a render.
#include "waa_host.hpp"

namespace waa {
namespace host {

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

// Strongly connected components of the graph of `n` nodes with `edges` (Tarjan, iterative): comp[v] = component of node v; returns
// how many there are.  (The planner's own, waa_plan_graph.cpp, walks writer / reader vertices and skips muted nodes.)
static int strong_components(uint32_t n, const std::vector<waa_edge_desc>& edges, std::vector<int>* comp) {
  std::vector<std::vector<uint32_t>> adj(n);
  for (const waa_edge_desc& ed : edges) adj[ed.from].push_back(ed.to);
  std::vector<int> index(n, -1), low(n, 0);
  comp->assign(n, -1);
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
            (*comp)[w] = n_comp;
            if (w == v) break;
          }
          n_comp++;
        }
        call.pop_back();
        if (!call.empty()) low[call.back().v] = std::min(low[call.back().v], low[v]);
      }
    }
  }
  return n_comp;
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
      std::vector<int> comp;
      const int n_comp = strong_components((uint32_t)b->nodes.size(), b->edges, &comp);
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

// build_plan under a stopwatch; the split (hipMalloc / blocking uploads / the rest = host planning: ordering, scheduling
// replay, coefficient and automation evaluation) goes into the plan description
int plan_batch(waa_batch* b) {
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

// Quantum-blocked loops rendered in blocks of several quanta are optimistic about ONE thing (waa_plan_dyn_loop.cpp: the ring's channel
// count as the reader of a split delay pair sees it).  Every entry point that hands out results waits for the render and looks at
// the writers' flags first; a flagged render is repeated with one quantum per block — the round-5 form, always right.
int settle_loops(waa_batch* b) {
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

}  // namespace host
}  // namespace waa
