// waa_plan_route.cpp — output and input ports in the planner: ChannelSplitterNode and ChannelMergerNode (kernel: waa_route.hip).
//
// Ports.  Everywhere else in the planner "the output of node P" is one signal (Node::sig, Node::out_nch), and every consumer kind —
// chain input stages, the node-major steps, AudioParam summing chains — reads it through the same two fields.  The only node with
// more than one output is the ChannelSplitterNode, so an output port is modelled as a node of its own: before the plan is built,
// every CONNECTED output k of a splitter S becomes an internal node T (NODE_SPLITTER_PORT, one input, one mono output), the edges
// S:k -> X become T -> X, and S -> T is added.  T's signal is a one-channel VIEW of S's input bus,
//     SignalRef{bus.base + k * bus.ch_stride, bus.inst_stride, bus.ch_stride, 1}
// (channel strides are whole tiles: a view is 16-byte aligned like its owner), so every consumer learns which output it reads by
// reading its producer's signal, as it always did — no consumer kind needs to know about ports.  T costs no launch and no bytes.
// Input ports exist on the ChannelMergerNode only: its in_edges stay in summing order and are grouped by to_input here.
//
// The splitter's input bus (explicit count N, discrete: channel k of the bus = sum of channel k of every connection that has
// one).  With a single connection from a producer the bus IS the producer's signal: the views point into it ("views of node P, no
// launch"); an output at or beyond the producer's count is silent, which only a ChannelMergerNode can consume without reading
// memory (it writes the zeros itself) — any other consumer of such an output makes the bus a signal of its own.  Otherwise one
// route launch writes the N-channel bus ("mixed by route launch").
#include "waa_host.hpp"
#include "waa_plan_parts.hpp"

namespace waa {
namespace host {

int desugar_output_ports(waa_batch* b) {
  if (b->ports_done) return 0;
  b->ports_done = true;
  const uint32_t n0 = (uint32_t)b->nodes.size();
  const size_t e0 = b->edges.size();
  for (uint32_t s = 0; s < n0; s++) {
    if (b->nodes[s].desc.kind != WAA_NODE_CHANNEL_SPLITTER) continue;
    std::map<uint32_t, uint32_t> port_node;  // output -> port node
    for (size_t k = 0; k < e0; k++) {
      if (b->edges[k].from != s) continue;
      const uint32_t port = b->edges[k].from_output;
      auto it = port_node.find(port);
      if (it == port_node.end()) {
        const uint32_t tid = (uint32_t)b->nodes.size();
        b->nodes.emplace_back();
        Node& t = b->nodes.back();
        t.desc = waa_node_desc{};
        t.desc.kind = NODE_SPLITTER_PORT;
        t.desc.i[0] = (int32_t)port;
        t.cc = 1;
        t.mode = WAA_COUNT_MODE_EXPLICIT;
        t.interp = WAA_INTERP_DISCRETE;
        t.port_of = (int)s;
        t.port = (int)port;
        it = port_node.emplace(port, tid).first;
        b->edges.push_back(waa_edge_desc{s, port, tid, 0});
        b->edge_on.push_back(0u);
        b->edge_off.push_back(EDGE_NEVER);
      }
      b->edges[k].from = it->second;
      b->edges[k].from_output = 0;
    }
  }
  return 0;
}

namespace {

const void* owner_of(const waa_batch* b, const void* p) {
  auto it = b->view_owner.find(p);
  return it == b->view_owner.end() ? p : it->second;
}

// one route launch: rows[r] = the terms of output channel r
int push_route_step(waa_batch* b, const std::vector<std::vector<RouteTerm>>& rows, const SignalRef& out) {
  std::vector<RouteTerm> terms;
  std::vector<uint32_t> row_off{0u};
  Step st;
  st.kind = StepKind::Route;
  for (const auto& r : rows) {
    for (const RouteTerm& t : r) {
      terms.push_back(t);
      st.loop_reads.push_back(owner_of(b, t.base));
    }
    row_off.push_back((uint32_t)terms.size());
  }
  const uint64_t blocks = (uint64_t)b->n_tiles * rows.size() * b->n_inst;
  if (blocks > 0x7fffffffull)
    return fail(WAA_ERR_OUT_OF_SCOPE, "channel routing of %u instance(s) x %zu channel(s) x %u tile(s) exceeds one launch", b->n_inst, rows.size(), b->n_tiles);
  RouteTerm* d_terms = nullptr;
  uint32_t* d_off = nullptr;
  int e;
  if ((e = dev_upload(b, &d_terms, terms)) || (e = dev_upload(b, &d_off, row_off))) return e;
  RouteDesc& d = st.route;
  std::memset(&d, 0, sizeof d);
  d.out = out;
  d.terms = d_terms;
  d.row_off = d_off;
  d.n_inst = b->n_inst;
  d.rows = (uint32_t)rows.size();
  d.frames = b->lp;
  st.loop_writes.push_back(out.base);
  st.profile_slot = slot_for(b, "route_kernel");
  b->steps.push_back(st);
  return 0;
}

RouteTerm channel_term(const SignalRef& s, int ch) {
  RouteTerm t{};
  t.base = s.base;
  t.inst_stride = s.inst_stride;
  t.ch_stride = s.ch_stride;
  t.mode = RT_CHANNEL;
  t.ch = ch;
  return t;
}

int alloc_out(waa_batch* b, Node& n, int nch) {
  float* p = nullptr;
  if (int e = dev_alloc(b, &p, (size_t)b->n_inst * nch * b->lp)) return e;
  n.sig = SignalRef{p, (uint64_t)nch * b->lp, b->lp, nch, 0};
  return 0;
}

}  // namespace

int plan_splitter(waa_batch* b, uint32_t id, bool producer_in_loop) {
  Node& n = b->nodes[id];
  const int N = n.desc.i[0];
  n.port_views = false;
  for (int ie : n.in_edges)
    if (!b->nodes[b->edges[ie].from].materialized || !b->nodes[b->edges[ie].from].sig.base)
      return fail(WAA_ERR_INVALID_STATE, "internal: input %u of ChannelSplitterNode %u is not materialised", b->edges[ie].from, id);
  if (n.in_edges.size() == 1 && !producer_in_loop) {
    const uint32_t pid = b->edges[n.in_edges[0]].from;
    const Node& p = b->nodes[pid];
    // outputs beyond the producer's channels are silent: fine as long as only ChannelMergerNodes listen to them
    bool ok = true;
    for (const waa_edge_desc& e : b->edges) {
      const Node& t = b->nodes[e.from];
      if (t.port_of != (int)id || t.port < p.out_nch || !b->nodes[e.to].live) continue;
      ok = ok && b->nodes[e.to].desc.kind == WAA_NODE_CHANNEL_MERGER && !(e.to_input & 0x80000000u);
    }
    if (ok) {
      n.port_views = true;
      n.sig = p.sig;
      n.sig.nch = std::min(p.out_nch, N);
      plan_note(b, "splitter node %u: %d output(s), views of node %u (%dch), no launch", id, N, pid, p.out_nch);
      return 0;
    }
  }
  if (int e = alloc_out(b, n, N)) return e;
  std::vector<std::vector<RouteTerm>> rows((size_t)N);
  size_t n_terms = 0;
  for (int ie : n.in_edges) {
    const Node& p = b->nodes[b->edges[ie].from];
    for (int k = 0; k < std::min(N, p.out_nch); k++) {
      rows[(size_t)k].push_back(channel_term(p.sig, k));
      n_terms++;
    }
  }
  if (int e = push_route_step(b, rows, n.sig)) return e;
  plan_note(b, "splitter node %u: %d output(s), %zu connection(s), mixed by route launch -> route_kernel (%zu term(s))", id, N, n.in_edges.size(), n_terms);
  return 0;
}

int plan_splitter_port(waa_batch* b, uint32_t id) {
  Node& t = b->nodes[id];
  const Node& s = b->nodes[(size_t)t.port_of];
  t.silent_port = false;
  t.sig = SignalRef{};
  if (!s.sig.base) return fail(WAA_ERR_INVALID_STATE, "internal: ChannelSplitterNode %d has not been planned before its output %d", t.port_of, t.port);
  if (t.port >= s.sig.nch) {  // (views of a narrower producer)
    t.silent_port = true;
    return 0;
  }
  t.sig = SignalRef{s.sig.base + (uint64_t)t.port * s.sig.ch_stride, s.sig.inst_stride, s.sig.ch_stride, 1, 0};
  if (t.sig.base != s.sig.base) b->view_owner[t.sig.base] = owner_of(b, s.sig.base);
  return 0;
}

int plan_merger(waa_batch* b, uint32_t id) {
  Node& n = b->nodes[id];
  const int N = n.desc.i[0];
  if (int e = alloc_out(b, n, N)) return e;
  std::vector<std::vector<RouteTerm>> rows((size_t)N);
  size_t n_terms = 0, n_down = 0;
  for (int ie : n.in_edges) {  // (summing order; grouped by input port)
    const waa_edge_desc& ed = b->edges[ie];
    const Node& p = b->nodes[ed.from];
    if (ed.to_input >= (uint32_t)N) return fail(WAA_ERR_INVALID_STATE, "internal: input port %u of ChannelMergerNode %u", ed.to_input, id);
    if (p.desc.kind == NODE_SPLITTER_PORT && p.silent_port) continue;  // a channel the splitter's input does not have
    if (!p.materialized || !p.sig.base || p.sig.nch < p.out_nch)
      return fail(WAA_ERR_INVALID_STATE, "internal: input %u of ChannelMergerNode %u is not materialised", ed.from, id);
    RouteTerm t = channel_term(p.sig, 0);
    if (n.interp == WAA_INTERP_SPEAKERS) {  // count 1, explicit: AudioRenderQuantum::mix to one channel (quantum.rs:285-432)
      if (p.out_nch == 2) t.mode = RT_DOWN2;
      if (p.out_nch == 4) t.mode = RT_DOWN4;
      if (p.out_nch == 6) t.mode = RT_DOWN6;
    }
    n_down += t.mode != RT_CHANNEL;
    rows[ed.to_input].push_back(t);
    n_terms++;
  }
  if (int e = push_route_step(b, rows, n.sig)) return e;
  plan_note(b, "merger node %u: %d input(s) (%s), %zu connection(s), %zu of them down-mixed to mono -> route_kernel (%zu term(s))", id, N,
            n.interp == WAA_INTERP_SPEAKERS ? "speakers" : "discrete", n.in_edges.size(), n_down, n_terms);
  return 0;
}

}  // namespace host
}  // namespace waa
