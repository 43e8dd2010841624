// waa_plan_dyn.cpp — the dynamic-count plan (waa_dyn.hip): the dynamic-group builder, split out of build_plan in round 4.
//
// Sources, oscillators, FFT convolvers and the frozen-state nodes stay node-major launches; every other live node becomes an item of
// a quantum-serial dyn_kernel launch that carries per-quantum codes (count | silent) with every signal.  A convolver / frozen-state
// node splits the items into groups (its input is produced by the group in front of it, its output consumed by the group behind it).
//
// From the bottom up: plan_dynamic_groups walks the planning units and reads as a list of cases; flush_group turns the pending
// vertices into one launch (the item builders, split_ok, the stage partitioner); DynPlan (waa_plan_parts.hpp) is what they share.
// The case of a loop with node-major members inside: waa_plan_dyn_loop.cpp.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <set>
#include <string>

#include "waa_host.hpp"
#include "waa_plan_parts.hpp"

namespace waa {
namespace host {

bool is_node_major(const Node& n) { return is_frozen_node(n) || (n.desc.kind == WAA_NODE_CONVOLVER && n.has_ir); }

static bool is_src(uint32_t k) { return k == WAA_NODE_BUFFER_SOURCE || k == WAA_NODE_CONSTANT_SOURCE || k == WAA_NODE_OSCILLATOR; }
// a mono impulse response behind a stereo input: channel 1 runs in compacted time
static bool mono_ir_stereo_in(const Node& n) { return n.ir_nch == 1 && n.in_nch == 2; }
static int alloc_codes(DynPlan& p, uint8_t** out) { return dev_alloc(p.b, out, (size_t)p.b->n_inst * p.cs); }
// ring capacity - 1 of a DelayNode, for its writer and its reader
static int32_t delay_ring_quanta(const waa_batch* b, const Node& n) { return (int32_t)std::ceil(n.desc.d[0] * (double)b->sr / (double)RQ); }

static int refuse_wide_narrow_only_nodes(const waa_batch* b) {
  for (uint32_t id = 0; id < (uint32_t)b->nodes.size(); id++) {
    const Node& n = b->nodes[id];
    // layouts up to 5.1 are rendered by dyn_kernel<6> (round 3) for Gain / Biquad / IIR / WaveShaper / the panners / DelayNodes
    // (whose line is then re-mixed in place when the count changes) / analysers (whose kernel follows the per-quantum codes)
    // / the destination; convolver and frozen-node inputs are stereo by their channel config: those stay mono / stereo
    const uint32_t k = n.desc.kind;
    // (round 6) signals of 7 ... 32 channels in a dynamic plan: dyn_kernel<8 / 16 / 32> — the same count rules, every mix above six
    // channels discrete; an oversampled WaveShaper renders its channel pairs whatever their number (one launch per pair, one link table)
    const bool narrow_only = (k == WAA_NODE_CONVOLVER && n.has_ir) || (is_frozen_node(n) && k == WAA_NODE_PANNER);  // (an oversampled WaveShaper renders channel pairs, round 4)
    if (n.live && narrow_only && (n.in_nch > 2 || n.out_nch > 2))
      return fail(WAA_ERR_OUT_OF_SCOPE,
                  "node %u: the reference's channel count changes mid-render and a signal is wider than stereo (%d channels): "
                  "exact dynamic counts above stereo are not rendered for this node kind",
                  id, std::max(n.in_nch, n.out_nch));
  }
  return 0;
}

// ---- host-known codes of a source: active quanta carry the source's channel count
static int upload_source_codes(DynPlan& p, uint32_t id) {
  std::vector<uint8_t> host;
  int e = source_code_rows(p.b, id, p.cs, &host);
  if (e) return e;
  uint8_t* dcode = nullptr;
  if ((e = dev_upload(p.b, &dcode, host))) return e;
  p.b->nodes[id].code = dcode;
  return 0;
}

// ---- the items of a launch, one builder per DI_* kind -------------------------------------------------------------------------
// the inputs of item k: outputs of earlier items of the launch (out_item) or signals published by launches in front of it
static int item_inputs(DynPlan& p, uint32_t id, size_t k, const std::map<uint32_t, int>& out_item, DynItem& li, Step& st) {
  waa_batch* b = p.b;
  const Node& n = b->nodes[id];
  if (n.in_edges.size() > (size_t)DYN_MAX_IN)
    return fail(WAA_ERR_OUT_OF_SCOPE, "more than %d inputs on node %u of a dynamic-count graph", DYN_MAX_IN, id);
  li.n_in = (int)n.in_edges.size();
  for (int j = 0; j < li.n_in; j++) {
    const uint32_t pid = b->edges[n.in_edges[j]].from;
    const Node& pn = b->nodes[pid];
    DynInput& in = li.in[j];
    auto it = out_item.find(pid);
    if (it != out_item.end()) {
      // same quantum through LDS; a producer that renders LATER in the quantum is only legal for ... nothing:
      // the cycle breaker guarantees producers first, except through a delay reader (which reads the line)
      if (it->second >= (int)k) return fail(WAA_ERR_INVALID_STATE, "internal: dynamic group member order (node %u)", id);
      in.item = it->second;
    } else {
      if (!pn.sig.base || !p.planned_node[pid])
        return fail(WAA_ERR_INVALID_STATE, "internal: input %u of node %u is not planned yet", pid, id);
      in.item = -1;
      in.nch = pn.out_nch;
      in.sig = pn.sig;
      in.code = pn.code;
      in.remap = pn.remap;
      in.code_stride = p.cs;
      st.loop_reads.push_back(pn.sig.base);
    }
  }
  return 0;
}

// the cross-segment resources of a DelayNode, if the cuts of the current quantum-blocked loop split it
static const XDelay* split_pair(const DynPlan& p, uint32_t id) {
  const auto xd = p.cur_qgroup >= 0 ? p.xdelay.find(id) : p.xdelay.end();
  return xd == p.xdelay.end() ? nullptr : &xd->second;
}

static int delay_writer_item(DynPlan& p, uint32_t id, DynItem& li) {
  waa_batch* b = p.b;
  const Node& n = b->nodes[id];
  li.kind = DI_DELAY_W;
  li.num_quanta = delay_ring_quanta(b, n);
  if (const XDelay* xd = split_pair(p, id)) {  // (the reader sits in another launch: line, codes and ring state were allocated for both)
    li.out = xd->line;
    li.aux32 = xd->aux32;
    li.xstate = xd->state;
  } else {
    int e = temp_signal(b, n.in_nch, &li.out);  // the delay line in absolute time, native layout
    if (e) return e;
    if ((e = dev_alloc(b, &li.aux32, (size_t)b->n_inst * p.cs))) return e;
  }
  li.nch_pub = n.in_nch;
  return 0;
}

static int delay_reader_item(DynPlan& p, uint32_t id, size_t k, const std::map<uint32_t, int>& writer_item, DynItem& li) {
  waa_batch* b = p.b;
  Node& n = b->nodes[id];
  li.kind = DI_DELAY_R;
  li.out = n.sig;
  li.nch_pub = n.out_nch;
  if (const XDelay* xd = split_pair(p, id)) {
    li.writer_item = -1;
    li.xline = xd->line;
    li.xaux32 = xd->aux32;
    li.xstate = xd->state;
    li.in_cycle = xd->writer_seg > xd->reader_seg ? 1 : 0;  // (the writer's launch of this quantum comes later)
  } else {
    li.writer_item = writer_item.at(id);
    li.in_cycle = li.writer_item > (int)k ? 1 : 0;
  }
  li.num_quanta = delay_ring_quanta(b, n);
  int e = node_param(b, id, WAA_PARAM_DELAY_DELAY_TIME, &li.op.p0);
  if (e) return e;
  if ((e = alloc_codes(p, &n.code))) return e;
  li.out_code = n.code;
  return 0;
}

// emit_node_ops reads the input width and the AudioParam inputs from the node itself.  The two callers below that need the ops of
// ANOTHER width, or without the param's inputs, change the node for the one call and put it back here.
static int emit_ops_at_width(waa_batch* b, uint32_t id, int nch, std::vector<OpDesc>& ops) {
  Node& n = b->nodes[id];
  const int keep = n.in_nch;
  int out_nch = 0;
  n.in_nch = nch;
  const int e = emit_node_ops(b, id, nch, true, ops, &out_nch);
  n.in_nch = keep;
  return e;
}
static int emit_ops_without_gain_inputs(waa_batch* b, uint32_t id, std::vector<OpDesc>& ops) {
  Node& n = b->nodes[id];
  std::vector<int> saved;
  int out_nch = 0;
  saved.swap(n.pin_edges[0]);  // (the intrinsic value alone: constants / value blocks / automation)
  const int e = emit_node_ops(b, id, n.in_nch, true, ops, &out_nch);
  saved.swap(n.pin_edges[0]);
  return e;
}

// a StereoPanner / equal-power Panner: both laws, the gains for a mono input (alt) and for a stereo input (op)
static int panner_two_laws(waa_batch* b, uint32_t id, DynItem& li, std::vector<OpDesc>& ops) {
  int e = emit_ops_at_width(b, id, 1, ops);
  if (e) return e;
  li.alt1 = ops[0].p1;
  li.alt2 = ops[0].p2;
  ops.clear();
  return emit_ops_at_width(b, id, 2, ops);
}

// (round 6) the gain param is modulated from inside the node's own loop: its inputs are items of this launch (same quantum, out of
// the ring) instead of a node-major param chain in front of the group
static bool gain_modulated_from_its_loop(const DynPlan& p, uint32_t id) {
  const Node& n = p.b->nodes[id];
  const std::vector<int>& scc_of = p.pass.scc_of;
  return n.desc.kind == WAA_NODE_GAIN && scc_of[id] >= 0 && !n.pin_edges.empty() && !n.pin_edges[0].empty() &&
         scc_of[p.b->edges[n.pin_edges[0][0]].from] == scc_of[id];
}
static int gain_modulated_item(DynPlan& p, uint32_t id, size_t k, DynItem& li, std::vector<OpDesc>& ops) {
  waa_batch* b = p.b;
  const Node& n = b->nodes[id];
  const std::vector<int>& scc_of = p.pass.scc_of;
  const std::vector<int>& mods = n.pin_edges[0];
  if (mods.size() > 4) return fail(WAA_ERR_OUT_OF_SCOPE, "more than 4 inputs on the gain param of node %u inside a feedback loop", id);
  for (size_t j = 0; j < mods.size(); j++) {
    const uint32_t from = b->edges[mods[j]].from;
    const uint32_t want = is_delay(b, from) ? (from | VTX_READER) : from;
    int found = -1;
    for (size_t k2 = 0; k2 < k; k2++)
      if (p.pending[k2] == want) found = (int)k2;
    if (found < 0 || scc_of[from] != scc_of[id])
      return fail(WAA_ERR_OUT_OF_SCOPE, "an AudioParam of node %u is modulated from inside its own feedback loop (producer %u is not rendered in front of it)", id, from);
    li.pmod_item[j] = found;
  }
  li.pmod_n = (int32_t)mods.size();
  li.pmod_min = n.params[0].minv;
  li.pmod_max = n.params[0].maxv;
  li.pmod_def = n.params[0].defv;
  return emit_ops_without_gain_inputs(b, id, ops);
}

// DK_* of the one op a member emits, -1: none
static int dk_of_op(int op_kind) {
  switch (op_kind) {
    case OP_GAIN: return DK_GAIN;
    case OP_BIQUAD: return DK_BIQUAD;
    case OP_IIR: return DK_IIR;
    case OP_WAVESHAPER: return DK_WAVESHAPER;
    case OP_STEREO_PAN: return DK_STEREO_PAN;
    case OP_PANNER: return DK_PANNER;
    default: return -1;
  }
}
// DynItem::flags bit 0 of a plain WaveShaper: can_propagate_silence (curve(0) == 0, or no curve at all)
static int32_t shaper_silence_flag(const Node& n) {
  const size_t cn = n.curve.size();
  const float mid = cn == 0 ? 0.f : (cn % 2 ? n.curve[cn / 2] : (n.curve[cn / 2 - 1] + n.curve[cn / 2]) / 2.f);
  return (!n.has_curve || cn == 0 || std::fabs(mid) < 1e-9f) ? 1 : 0;
}
// A node-major member (convolver with a response, frozen-state node): the item publishes the node's INPUT (n.hist) and its codes;
// n.sig is written by the node-major steps that follow the launch
static int conv_in_item(DynPlan& p, Node& n, DynItem& li) {
  waa_batch* b = p.b;
  li.dk = DK_CONV_IN;
  int e = temp_signal(b, n.in_nch, &n.hist);
  if (e) return e;
  li.out = n.hist;
  li.nch_pub = n.in_nch;
  if ((e = alloc_codes(p, &n.in_code))) return e;
  li.out_code = n.in_code;
  if (n.desc.kind == WAA_NODE_CONVOLVER && mono_ir_stereo_in(n)) {
    li.compact_ch1 = 1;
    if ((e = dev_alloc(b, &n.remap, (size_t)b->n_inst * p.cs))) return e;
    li.aux32 = n.remap;
    // channel 1 is written in compacted time: quanta it never reaches must read as zeros
    b->state_bufs.push_back({n.hist.base, (size_t)b->n_inst * n.hist.inst_stride * sizeof(float)});
  } else {
    li.publish_upmix = 1;
  }
  return 0;
}

static int node_item(DynPlan& p, uint32_t id, size_t k, DynItem& li) {
  waa_batch* b = p.b;
  Node& n = b->nodes[id];
  const uint32_t kind = n.desc.kind;
  li.kind = DI_NODE;
  li.out = n.sig;
  li.nch_pub = n.out_nch;
  int e = alloc_codes(p, &n.code);
  if (e) return e;
  li.out_code = n.code;
  std::vector<OpDesc> ops;
  int out_nch = 0;
  if ((kind == WAA_NODE_STEREO_PANNER || kind == WAA_NODE_PANNER) && !is_frozen_node(n))
    e = panner_two_laws(b, id, li, ops);
  else if (is_node_major(n))
    e = 0;  // (the mixed input of the node; its node-major steps follow the launch)
  else if (gain_modulated_from_its_loop(p, id))
    e = gain_modulated_item(p, id, k, li, ops);
  else
    e = emit_node_ops(b, id, n.in_nch, true, ops, &out_nch);
  if (e) return e;
  if (ops.size() > 1) return fail(WAA_ERR_DEVICE, "internal: node %u emitted %zu ops", id, ops.size());
  li.dk = DK_PASS;
  if (!ops.empty()) {
    li.op = ops[0];
    if ((li.dk = dk_of_op(ops[0].kind)) < 0) return fail(WAA_ERR_DEVICE, "internal: op %d in a dynamic-count group", ops[0].kind);
  }
  if (kind == WAA_NODE_WAVESHAPER && !is_frozen_node(n)) {
    li.dk = DK_WAVESHAPER;  // (without a curve: ptr0 == null, output = input)
    li.flags = shaper_silence_flag(n);
  }
  if (kind == WAA_NODE_CONVOLVER && !n.has_ir) li.flags |= 2;
  if (kind == WAA_NODE_ANALYSER) li.publish_upmix = 1;  // the analyser FFT reads a static stereo signal
  return is_node_major(n) ? conv_in_item(p, n, li) : 0;
}

// item k of the launch (vertex p.pending[k]) and its name in the plan note
static int build_item(DynPlan& p, size_t k, const std::map<uint32_t, int>& out_item, const std::map<uint32_t, int>& writer_item, DynItem& li, Step& st,
               char (&name)[64]) {
  waa_batch* b = p.b;
  const uint32_t v = p.pending[k], id = v & ~VTX_READER;
  const Node& n = b->nodes[id];
  std::memset(&li, 0, sizeof li);
  li.cc = n.cc;
  li.mode = n.mode;
  li.interp = n.interp;
  li.code_stride = p.cs;
  li.writer_item = -1;
  int e = 0;
  if (is_delay(b, id) && (v & VTX_READER)) {
    if ((e = delay_reader_item(p, id, k, writer_item, li))) return e;
    snprintf(name, sizeof name, "delayR%u%s", id, li.in_cycle ? "(clamped)" : "");
    return 0;
  }
  if ((e = item_inputs(p, id, k, out_item, li, st))) return e;
  if (is_delay(b, id)) {
    if ((e = delay_writer_item(p, id, li))) return e;
    snprintf(name, sizeof name, "delayW%u", id);
    return 0;
  }
  if ((e = node_item(p, id, k, li))) return e;
  snprintf(name, sizeof name, "%s%u", li.dk == DK_PASS ? "pass" : li.dk == DK_CONV_IN ? "convIn" : op_name(li.op.kind), id);
  return 0;
}

// (round 6) items without state from quantum to quantum — gains, mixes, curves, the destination's pass, DelayNode halves whose
// partner sits in another launch: no quantum of the launch depends on an earlier one, the launcher spreads the quanta over
// workgroups (a block of a quantum-blocked loop, or the whole render of such a group) instead of walking them one by one
static bool quanta_are_independent(const std::vector<DynItem>& host, int cmax) {
  if (cmax > 2) return false;
  for (const DynItem& li : host) {
    bool ok = false;
    if (li.kind == DI_DELAY_R)
      ok = li.writer_item < 0 && li.xstate;
    else if (li.kind == DI_DELAY_W)
      ok = li.xstate != nullptr;
    else
      ok = li.dk == DK_PASS || li.dk == DK_GAIN || li.dk == DK_WAVESHAPER || (li.dk == DK_CONV_IN && !li.compact_ch1);
    if (!ok) return false;
  }
  return true;
}

// ---- the quantum pipeline (waa_dyn.hip, W > 1): cut the items — in thirds: unit 3 i = item i's gather + mix of its inputs, unit
// 3 i + 1 = its node, unit 3 i + 2 = the publication of its result — into up to DYN_MAX_STAGES contiguous stages of about equal cost.  Never between a DelayNode's
// writer and reader (the reader looks at the writer's ring state of ITS quantum) nor inside a feedback loop (its members see
// each other's output of the same quantum through the delay line).
struct Stages {
  int n = 1;
  int begin[DYN_MAX_STAGES + 1] = {0};
};
// the item spans [first, last] of a launch that no cut may divide: every DelayNode pair, every feedback loop
static std::vector<std::pair<int, int>> uncut_spans(const DynPlan& p, const std::vector<DynItem>& host) {
  std::vector<std::pair<int, int>> spans;
  std::map<int, std::pair<int, int>> scc_span;
  for (int k = 0; k < (int)host.size(); k++) {
    const int scc = p.pass.scc_of[p.pending[(size_t)k] & ~VTX_READER];
    if (host[(size_t)k].kind == DI_DELAY_R) spans.push_back({std::min(k, host[(size_t)k].writer_item), std::max(k, host[(size_t)k].writer_item)});
    if (scc < 0) continue;
    auto it = scc_span.find(scc);
    if (it == scc_span.end())
      scc_span[scc] = {k, k};
    else
      it->second.second = k;
  }
  for (auto& sp : scc_span) spans.push_back(sp.second);
  return spans;
}
// No side effects: the stages of `host` on a device of n_cu compute units that renders n_inst contexts; max_pick > 0: at most that
// many stages (WAA_DYN_STAGES).
static Stages partition_stages(const std::vector<DynItem>& host, const std::vector<std::pair<int, int>>& spans, int n_cu, uint32_t n_inst, int cmax,
                        int max_pick) {
  const int n = (int)host.size(), nu = 3 * n;
  Stages out;
  out.begin[1] = nu;
  std::vector<uint8_t> nocut((size_t)nu, 0);  // nocut[u]: units u and u + 1 stay together
  for (auto& sp : spans)
    for (int u = 3 * sp.first; u < 3 * sp.second + 2; u++) nocut[(size_t)u] = 1;
  for (int k = 0; k < n; k++)
    if (host[(size_t)k].kind == DI_DELAY_R) nocut[(size_t)(3 * k)] = 1;  // (a reader has no inputs to gather: its first third is empty)
  // cost per unit in thousands of cycles per quantum (every phase costs 1.2-2 k cycles whatever it computes;
  // WAA_DYN_CYCLES on the probe graph: Biquad gather 4.0 (two external inputs) / node 4.1 / hand-over 2.0, StereoPanner 1.6 /
  // 3.1 / 1.9, pass 1.6 / 1.2 / 1.8)
  std::vector<double> pre((size_t)nu + 1, 0.);
  for (int k = 0; k < n; k++) {
    const DynItem& li = host[(size_t)k];
    double front = li.kind == DI_DELAY_R ? 0. : 1.1, node = 0.6, pub = li.out.base ? 1.4 : 0.2;
    for (int j = 0; j < li.n_in; j++) front += li.in[j].item < 0 ? 1.4 : 0.5;
    if (li.kind == DI_DELAY_R) node += 4.0;
    else if (li.kind == DI_DELAY_W) node += 1.0;
    else if (li.dk == DK_BIQUAD) node += 4.1;
    else if (li.dk == DK_IIR) node += 9.0;
    else if (li.dk == DK_STEREO_PAN || li.dk == DK_PANNER) node += 3.1;
    else if (li.dk == DK_WAVESHAPER) node += 2.5;
    else if (li.dk == DK_GAIN) node += 1.5;
    else node += 1.2;
    pre[(size_t)(3 * k) + 1] = pre[(size_t)(3 * k)] + front;
    pre[(size_t)(3 * k) + 2] = pre[(size_t)(3 * k) + 1] + node;
    pre[(size_t)(3 * k) + 3] = pre[(size_t)(3 * k) + 2] + pub;
  }
  // best[s][i]: smallest possible largest-stage cost of the first i units in s stages; cut[s][i]: where the last stage starts
  const double INF = 1e300;
  std::vector<std::vector<double>> best(DYN_MAX_STAGES + 1, std::vector<double>((size_t)nu + 1, INF));
  std::vector<std::vector<int>> cut(DYN_MAX_STAGES + 1, std::vector<int>((size_t)nu + 1, 0));
  for (int i = 1; i <= nu; i++) best[1][(size_t)i] = pre[(size_t)i];
  for (int sN = 2; sN <= DYN_MAX_STAGES; sN++)
    for (int i = sN; i <= nu; i++)
      for (int j = sN - 1; j < i; j++) {  // the last stage = units [j, i)
        if (nocut[(size_t)j - 1] || best[sN - 1][(size_t)j] >= INF) continue;
        const double v = std::max(best[sN - 1][(size_t)j], pre[(size_t)i] - pre[(size_t)j]);
        if (v < best[sN][(size_t)i]) {
          best[sN][(size_t)i] = v;
          cut[sN][(size_t)i] = j;
        }
      }
  // Every stage is a wavefront, and all of a launch's wavefronts must be resident at once or the launch takes a second round
  // (r05e: five stages x 1024 contexts = 5120 wavefronts on a device that holds 4096 of this kernel — 107 registers: four per
  // SIMD — ran SLOWER than one stage): at most (CUs x 4 SIMDs x 4) / contexts stages.
  // (A 96-register build — five wavefronts per SIMD, eight spilled registers — made a fifth stage resident at 1024 contexts and
  // ran it at 20.8 ms against 13.1 ms for four stages, r05k: not kept.)
  const int max_stages = std::max(1, std::min(DYN_MAX_STAGES, (int)((uint64_t)n_cu * 16 / std::max<uint32_t>(n_inst, 1))));
  int pick = 1;
  double pick_cost = best[1][(size_t)nu];
  for (int sN = 2; sN <= max_stages; sN++) {
    if (best[sN][(size_t)nu] >= INF) continue;
    // (... and so must their local memory: contexts / CUs workgroups share a CU's 160 KB)
    const uint64_t wg_per_cu = ((uint64_t)n_inst + (uint64_t)n_cu - 1) / (uint64_t)n_cu;
    if (dyn_lds_bytes(n, cmax, sN) * std::min<uint64_t>(wg_per_cu, 16) > 150 * 1024) continue;
    const double cst = best[sN][(size_t)nu] + 0.3 + 0.05 * sN;  // (+ the step's barrier, which waits for the slowest of sN waves)
    if (cst < 0.93 * pick_cost) {
      pick = sN;
      pick_cost = cst;
    }
  }
  if (max_pick > 0)  // (A/B aid: at most this many stages)
    while (pick > max_pick || (pick > 1 && best[pick][(size_t)nu] >= INF)) pick--;
  if (pick > 1) {
    out.n = pick;
    int i = nu;
    for (int sN = pick; sN >= 1; sN--) {
      out.begin[sN] = i;
      i = sN > 1 ? cut[sN][(size_t)i] : 0;
    }
    out.begin[0] = 0;
  }
  return out;
}

static void note_group(waa_batch* b, const DynDesc& d, const std::string& desc) {
  std::string cuts;
  for (int sN = 1; sN < d.n_stages; sN++)
    cuts += (cuts.empty() ? "" : ",") + std::to_string(d.stage_begin[sN] / 3) + (d.stage_begin[sN] % 3 == 1 ? "b" : d.stage_begin[sN] % 3 == 2 ? "c" : "");
  plan_note(b, "dynamic-count group: %d item(s) per quantum [%s]%s%s%s", d.n_items, desc.c_str(),
            d.n_stages > 1 ? (", pipelined over the quanta in " + std::to_string(d.n_stages) + " stages, cut in front of item(s) ").c_str() : "",
            cuts.c_str(), d.split_ok ? ", no item keeps state from quantum to quantum: the quanta are spread over workgroups" : "");
}

// ---- one dyn_kernel launch for the pending vertices
int flush_group(DynPlan& p) {
  waa_batch* b = p.b;
  std::vector<uint32_t>& pending = p.pending;
  if (pending.empty()) return 0;
  std::sort(pending.begin(), pending.end(), [&p](uint32_t x, uint32_t y) { return p.vpos[x] < p.vpos[y]; });
  if (pending.size() > (size_t)DYN_MAX_ITEMS)
    return fail(WAA_ERR_OUT_OF_SCOPE, "more than %d nodes in one dynamic-count group", DYN_MAX_ITEMS);
  std::map<uint32_t, int> out_item, writer_item;  // node id -> item producing its output / its delay line
  for (size_t k = 0; k < pending.size(); k++) {
    const uint32_t v = pending[k], id = v & ~VTX_READER;
    (is_delay(b, id) && !(v & VTX_READER) ? writer_item : out_item)[id] = (int)k;
  }
  std::vector<DynItem> host(pending.size());
  Step st;
  st.kind = StepKind::Dyn;
  std::string desc;
  for (size_t k = 0; k < pending.size(); k++) {
    char name[64];
    if (int e = build_item(p, k, out_item, writer_item, host[k], st, name)) return e;
    st.loop_writes.push_back(host[k].out.base);
    desc += desc.empty() ? name : std::string(",") + name;
  }
  DynItem* dev = nullptr;
  int e = dev_upload(b, &dev, host);
  if (e) return e;
  DynDesc& d = st.dyn;
  std::memset(&d, 0, sizeof d);
  d.items = dev;
  d.n_items = (int32_t)host.size();
  d.n_inst = b->n_inst;
  d.n_quanta = b->n_quanta;
  d.sample_rate = (double)b->sr;
  d.quantum_duration = (double)RQ * (1. / (double)b->sr);  // delay.rs:546-548
  d.cmax = 1;
  for (uint32_t v : pending) {
    const Node& pn = b->nodes[v & ~VTX_READER];
    d.cmax = std::max(d.cmax, std::max(pn.in_nch, pn.out_nch));
    for (int ie : pn.in_edges) d.cmax = std::max(d.cmax, b->nodes[b->edges[ie].from].out_nch);
  }
  if (dyn_lds_bytes(d.n_items, d.cmax) > 160 * 1024)
    return fail(WAA_ERR_OUT_OF_SCOPE, "dynamic-count group of %d nodes with %d-channel signals does not fit the kernel's local memory",
                d.n_items, d.cmax);
  d.n_stages = 1;
  d.stage_begin[0] = 0;
  d.stage_begin[1] = 3 * d.n_items;
  d.split_ok = quanta_are_independent(host, d.cmax) ? 1 : 0;
  if (p.cur_qgroup >= 0) {
    // a segment of a quantum-blocked loop: ranged launches that carry the items' state through memory; no quantum pipeline
    const int cm = dyn_planes(d.cmax);
    e = dev_alloc(b, &d.save_f, (size_t)b->n_inst * (size_t)d.n_items * cm * DYN_STATE);
    if (!e) e = dev_alloc(b, &d.save_i, (size_t)b->n_inst * (size_t)d.n_items * 4);
    if (e) return e;
    st.qgroup = p.cur_qgroup;
  } else if (d.cmax <= 2 && !d.split_ok) {
    const char* force = measure_switch("WAA_DYN_STAGES");
    const Stages stages = partition_stages(host, uncut_spans(p, host), b->n_cu, b->n_inst, d.cmax, force ? std::max(1, atoi(force)) : 0);
    d.n_stages = stages.n;
    std::copy(stages.begin, stages.begin + stages.n + 1, d.stage_begin);
  }
  st.profile_slot = slot_for(b, "dyn_kernel");
  b->steps.push_back(st);
  note_group(b, d, desc);
  for (uint32_t v : pending) p.planned_node[v & ~VTX_READER] = 1;
  pending.clear();
  p.pending_nodes.clear();
  return 0;
}

// a vertex joins the current group
int enqueue_vertex(DynPlan& p, uint32_t v) {
  Node& m = p.b->nodes[v & ~VTX_READER];
  if (!m.sig.base)
    if (int e = alloc_signal(p.b, m)) return e;
  if (std::find(p.pending.begin(), p.pending.end(), v) == p.pending.end()) p.pending.push_back(v);
  p.pending_nodes.insert(v & ~VTX_READER);
  return 0;
}

// ---- a ConvolverNode of a dynamic plan behind the group that published its mixed input: FFT steps + the code kernel --------------
// (round 5) where the reference's FFT convolver leaves roundoff noise instead of exact zeros: one automaton per
// FFTConvolver of the node (convolver.rs:291-306: one per channel of the response, at least two), fed by the non-zero flags of
// the input quanta; waa_conv_noise.hpp.  Here: the segments of each trimmed response and which of them hold a tap.
static void conv_noise_segments(const Node& n, ConvNoiseIr (&nir)[4]) {
  const int ncv = std::max(n.ir_nch, 2);
  for (int k = 0; k < 4; k++) {
    ConvNoiseIr& ni = nir[k];
    ni = ConvNoiseIr{};
    if (k >= ncv) continue;
    const std::vector<float>& h = n.ir[std::min(k, n.ir_nch - 1)];
    uint64_t l = n.ir_len;
    while (l > 0 && std::fabs(h[l - 1]) < 0.000001f) l--;  // (fft-convolver's init drops the end of the response below 1e-6)
    const uint64_t blk = (uint64_t)RQ * CONV_NOISE_BLOCK_QUANTA;
    ni.seg_count = (uint32_t)((l + blk - 1) / blk);
    ni.seg_mask = 0;
    for (uint64_t sgm = 0; sgm < ni.seg_count && sgm < 64; sgm++)
      for (uint64_t i = sgm * blk; i < std::min(l, (sgm + 1) * blk); i++)
        if (h[i] != 0.f) {
          ni.seg_mask |= (uint64_t)1 << sgm;
          break;
        }
  }
}

int plan_dyn_convolver(DynPlan& p, uint32_t id) {
  waa_batch* b = p.b;
  Node& n = b->nodes[id];
  uint8_t* in_code = n.in_code;  // published by the DK_CONV_IN item of the group just flushed
  if (!in_code) return fail(WAA_ERR_INVALID_STATE, "internal: convolver input codes");
  int e = plan_convolver(b, id);
  if (e) return e;
  if ((e = alloc_codes(p, &n.code))) return e;
  Step cst;
  cst.kind = StepKind::ConvCodes;
  ConvCodeDesc& cd = cst.ccode;
  std::memset(&cd, 0, sizeof cd);
  cd.in_code = in_code;
  cd.out_code = n.code;
  cd.code_stride = p.cs;
  cd.impulse_length = n.ir_len;
  cd.ir_nch = n.ir_nch;
  cd.n_inst = b->n_inst;
  cd.n_quanta = b->n_quanta;
  // (a mono impulse response on a stereo input keeps channel 1 in compacted time: only channel 0 is cleared in place)
  cd.cout = mono_ir_stereo_in(n) ? 1 : n.out_nch;
  cd.out = n.sig;
  if ((e = dev_alloc(b, &cd.clean, (size_t)b->n_inst * p.cs))) return e;
  cd.noise = n.hist.base && !measure_switch("WAA_NO_CONV_NOISE_FLOOR") ? 1 : 0;
  if (cd.noise) {
    cd.in = n.hist;
    cd.in_test_nch = mono_ir_stereo_in(n) ? 1 : std::min(n.in_nch, 2);
    conv_noise_segments(n, cd.nir);
  }
  cst.loop_writes.push_back(n.sig.base);
  cst.profile_slot = slot_for(b, "conv_code_kernel");
  b->steps.push_back(cst);
  return 0;
}

// ---- the driver's questions about a unit ------------------------------------------------------------------------------------------
static std::vector<uint32_t> unit_vertices(const waa_batch* b, const PlanPass& pass, const Unit& unit) {
  std::vector<uint32_t> verts;
  if (unit.scc >= 0) {
    for (uint32_t v : pass.items)
      if (pass.scc_of[v & ~VTX_READER] == unit.scc) verts.push_back(v);
  } else {
    if (is_delay(b, unit.id)) verts.push_back(unit.id);
    verts.push_back(is_delay(b, unit.id) ? (unit.id | VTX_READER) : unit.id);
  }
  return verts;
}
static bool any_live(const waa_batch* b, const std::vector<uint32_t>& verts) {
  for (uint32_t v : verts)
    if (b->nodes[v & ~VTX_READER].live) return true;
  return false;
}
// does the loop hold node-major members (then it is rendered quantum block by quantum block), and may it?
static int loop_has_cut_nodes(const waa_batch* b, const std::vector<uint32_t>& verts, bool* frozen_loop) {
  for (uint32_t v : verts) {
    const Node& m = b->nodes[v & ~VTX_READER];
    if (m.desc.kind == WAA_NODE_CONVOLVER && m.has_ir) {
      // (round 5) a response of at most 24 x 128 frames has 128-frame partitions: its transforms can follow the loop quantum by
      // quantum like the frozen-state nodes.  Longer responses (a partition spans several quanta) and a mono response behind a
      // stereo input (channel 1 runs in compacted time) stay out of scope.
      const bool ok = !(v & VTX_READER) && conv_block_size(b, m) == RQ && !mono_ir_stereo_in(m) && !measure_switch("WAA_NO_FROZEN_LOOPS");
      if (!ok)
        return fail(WAA_ERR_OUT_OF_SCOPE, "a ConvolverNode inside a feedback loop is out of scope (node %u)", v & ~VTX_READER);
      *frozen_loop = true;
    }
    if (is_frozen_node(m)) {
      if (measure_switch("WAA_NO_FROZEN_LOOPS"))
        return fail(WAA_ERR_OUT_OF_SCOPE, "an oversampled WaveShaperNode / HRTF PannerNode inside a feedback loop is out of scope (node %u)",
                    v & ~VTX_READER);
      *frozen_loop = true;
    }
  }
  return 0;
}
// AudioParam inputs are summed by a node-major chain in front of the group: their producers must be complete (*param_dep: one of
// them is still pending).  A producer inside the unit's own loop is refused — the one place that does — with one exception:
static int check_param_producers(const DynPlan& p, const Unit& unit, const std::vector<uint32_t>& verts, bool frozen_loop, bool* param_dep) {
  const waa_batch* b = p.b;
  for (uint32_t v : verts) {
    const Node& owner = b->nodes[v & ~VTX_READER];
    for (auto& pe : owner.pin_edges)
      for (int e : pe) {
        const uint32_t from = b->edges[e].from;
        if (unit.scc >= 0 && p.pass.scc_of[from] == unit.scc) {
          // (round 6) a GainNode's gain from inside its own loop is rendered by the group itself (DynItem::pmod_*), unless the
          // loop is quantum-blocked
          const bool gain_param = owner.desc.kind == WAA_NODE_GAIN && &pe == &owner.pin_edges[0] && !frozen_loop;
          if (!gain_param)
            return fail(WAA_ERR_OUT_OF_SCOPE, "an AudioParam of node %u is modulated from inside its own feedback loop",
                        v & ~VTX_READER);
          continue;
        }
        *param_dep |= p.pending_nodes.count(from) != 0;
      }
  }
  return 0;
}
static int plan_dyn_source(DynPlan& p, uint32_t id) {
  waa_batch* b = p.b;
  Node& n = b->nodes[id];
  int e = alloc_signal(b, n);
  if (e) return e;
  e = n.desc.kind == WAA_NODE_OSCILLATOR ? plan_oscillator(b, id) : plan_single(b, p.pass, id);
  if (e) return e;
  if ((e = upload_source_codes(p, id))) return e;
  p.planned_node[id] = 1;
  return 0;
}
// a frozen-state node outside loops: the group ends with the node's mixed input and its codes; then the link table (which also
// writes the node's output codes) and the node-major steps
static int plan_frozen_behind_its_group(DynPlan& p, uint32_t id) {
  const Node& n = p.b->nodes[id];
  if (int e = flush_group(p)) return e;
  if (!n.in_code) return fail(WAA_ERR_INVALID_STATE, "internal: input codes of node %u", id);
  return n.desc.kind == WAA_NODE_PANNER ? plan_hrtf(p.b, id, -1) : plan_oversampler(p.b, id, -1);
}

int plan_dynamic_groups(waa_batch* b, const PlanPass& pass) {
  if (!pass.count_change_found && pass.mixed_buffer_counts)
    plan_note(b, "instances play AudioBuffers of different channel counts -> per-instance counts through dyn_kernel");
  else if (!pass.count_change_found)
    plan_note(b, "a feedback loop needs quantum-serial rendering with node kinds the loop kernel does not cover -> dyn_kernel");
  b->dynamic = true;
  b->code_stride = ((uint64_t)b->n_quanta + 15) & ~(uint64_t)15;
  if (int e = refuse_wide_narrow_only_nodes(b)) return e;
  for (auto& n : b->nodes) n.materialized = n.live;  // every signal is published
  DynPlan p{b, pass, b->code_stride};
  for (size_t k = 0; k < pass.items.size(); k++) p.vpos[pass.items[k]] = k;
  p.planned_node.assign(b->nodes.size(), 0);
  for (const Unit& unit : pass.units) {
    const std::vector<uint32_t> verts = unit_vertices(b, pass, unit);
    if (!any_live(b, verts)) continue;
    bool frozen_loop = false, param_dep = false;
    if (unit.scc >= 0)
      if (int e = loop_has_cut_nodes(b, verts, &frozen_loop)) return e;
    if (int e = check_param_producers(p, unit, verts, frozen_loop, &param_dep)) return e;
    if (param_dep)
      if (int e = flush_group(p)) return e;
    const Node& n = b->nodes[unit.id];
    if (frozen_loop) {
      if (int e = plan_quantum_blocked_loop(p, verts)) return e;
    } else if (unit.scc < 0 && is_src(n.desc.kind)) {
      if (int e = plan_dyn_source(p, unit.id)) return e;
    } else {
      for (uint32_t v : verts)
        if (int e = enqueue_vertex(p, v)) return e;
      if (unit.scc < 0 && is_frozen_node(n)) {
        if (int e = plan_frozen_behind_its_group(p, unit.id)) return e;
      } else if (unit.scc < 0 && n.desc.kind == WAA_NODE_CONVOLVER && n.has_ir) {
        // the group ends with the convolver's mixed input; then the node-major FFT steps and the code kernel
        if (int e = flush_group(p)) return e;
        if (int e = plan_dyn_convolver(p, unit.id)) return e;
      }
    }
  }
  if (int e = flush_group(p)) return e;
  if (measure_switch("WAA_DEBUG_REVERSE_PLAN")) std::reverse(b->steps.begin(), b->steps.end());
  if (int e = validate_plan(b)) return e;
  b->planned = true;
  return 0;
}

}  // namespace host
}  // namespace waa
