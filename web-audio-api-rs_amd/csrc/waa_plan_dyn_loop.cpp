// waa_plan_dyn_loop.cpp — the dynamic-count plan of a feedback loop with node-major members (waa_plan_dyn.cpp has the rest).
//
// A feedback loop with node-major members inside (round 5): cut into segments at those nodes, every segment one RANGED
// dyn_kernel launch, the node's link / transform / FIR launches ranged too, all of them launched quantum block by quantum block
// (Step::qgroup): [items up to a frozen-state node -> its mixed input] [its link / transform / FIR launches] [the items behind it
// ...] — every launch over the same quantum, then the next quantum.
// (One quantum: the loop's delays are at least that long, delay.rs:693-701, and a split delay pair's reader must see the ring
// state of ITS quantum.  More than one where loop_block_quanta finds room.)
#include <algorithm>
#include <cmath>
#include <map>

#include "waa_host.hpp"
#include "waa_plan_parts.hpp"

namespace waa {
namespace host {

// segment of every vertex
static std::map<uint32_t, int> loop_segments(const waa_batch* b, const std::vector<uint32_t>& verts) {
  std::map<uint32_t, int> seg_of;
  int sg = 0;
  for (uint32_t v : verts) {
    seg_of[v] = sg;
    if (!(v & VTX_READER) && is_node_major(b->nodes[v])) sg++;
  }
  return seg_of;
}
// p.xdelay: line, codes and ring state of the delay pairs that the cuts split
static int alloc_split_pairs(DynPlan& p, const std::vector<uint32_t>& verts, const std::map<uint32_t, int>& seg_of) {
  waa_batch* b = p.b;
  for (uint32_t v : verts) {
    const uint32_t did = v & ~VTX_READER;
    if (!is_delay(b, did) || !(v & VTX_READER)) continue;
    const int rs = seg_of.at(v), ws = seg_of.at(did);
    if (rs == ws) continue;
    XDelay xd;
    xd.reader_seg = rs;
    xd.writer_seg = ws;
    int e = temp_signal(b, b->nodes[did].in_nch, &xd.line);
    if (!e) e = dev_alloc(b, &xd.aux32, (size_t)b->n_inst * p.cs);
    if (!e) e = dev_alloc(b, &xd.state, (size_t)b->n_inst * 2 + 4);  // (+ the block-violation flag behind the instances' pairs)
    if (e) return e;
    b->state_bufs.push_back({xd.state, ((size_t)b->n_inst * 2 + 4) * sizeof(int32_t)});  // (count 1, never mixed to mono: zeros)
    b->loop_flags.push_back(xd.state + (size_t)b->n_inst * 2);
    p.xdelay[did] = xd;
  }
  return 0;
}
// The block size (round-5 review, weak 6: one quantum per block = 15 000 launch sets for a 10 s render,
// 333 ms for 1024 contexts).  Every path from a later segment back into an earlier one goes through a DelayNode whose
// writer and reader the cuts separated; the reader of block [t, t + bq) reads the line up to frame
// (t + bq) * 128 - delay + 1 (linear interpolation, delay.rs:560-590), which must have been written by EARLIER blocks:
// bq <= (delay_frames - 1) / 128 for every split pair.  Known at plan time when delayTime is a constant; an automated or
// modulated delayTime keeps one quantum (delay.rs:693-701 guarantees no more than that).
static uint32_t loop_block_quanta(const waa_batch* b, const std::map<uint32_t, XDelay>& xdelay) {
  uint32_t bq = xdelay.empty() ? 1u : b->n_quanta;
  for (auto& kv : xdelay) {
    const Node& dn = b->nodes[kv.first];
    const ParamStore& dp = dn.params[WAA_PARAM_DELAY_DELAY_TIME];
    const bool constant = dp.mode() == 0 && dp.timelines.empty() && !dp.dev_tl &&
                          (dn.pin_edges.size() <= (size_t)WAA_PARAM_DELAY_DELAY_TIME || dn.pin_edges[WAA_PARAM_DELAY_DELAY_TIME].empty());
    if (!constant) {
      bq = 1;
      break;
    }
    float mn = dp.cst.empty() ? 0.f : dp.cst[0];
    for (float v2 : dp.cst) mn = std::min(mn, v2);
    const double frames = std::floor((double)dp.fix(mn) * (double)b->sr);
    bq = std::min(bq, frames >= 2. * RQ + 1. ? (uint32_t)((frames - 1.) / RQ) : 1u);
  }
  // (what the delay does NOT bound: the reader's channel count follows the writer's input with ONE quantum of lag whatever the
  // delay time — ring[0].number_of_channels() — so a block is only right while that count stands still inside it.  It does
  // almost always (it moves when a source starts or ends and when the loop falls silent); the writer flags the blocks where it
  // did not, and the render is repeated one quantum per block: waa_plan_prepass.cpp::settle_loops.)
  if (measure_switch("WAA_LOOP_ONE_QUANTUM")) bq = 1;  // (A/B: the round-5 form)
  return std::max(bq, 1u);
}
// a node-major member of the loop behind the segment that ends with its mixed input: its launches, ranged
static int plan_cut_node(DynPlan& p, uint32_t vid) {
  waa_batch* b = p.b;
  Node& m = b->nodes[vid];
  if (int e = flush_group(p)) return e;
  if (!m.in_code) return fail(WAA_ERR_INVALID_STATE, "internal: input codes of node %u", vid);
  const size_t first = b->steps.size();
  int e = m.desc.kind == WAA_NODE_CONVOLVER ? plan_dyn_convolver(p, vid)
          : m.desc.kind == WAA_NODE_PANNER  ? plan_hrtf(b, vid, -1)
                                            : plan_oversampler(b, vid, -1);
  if (e) return e;
  for (size_t k2 = first; k2 < b->steps.size(); k2++) {
    Step& fs = b->steps[k2];
    // (a cut node plans no dyn_kernel group of its own: the one ranged kind that is refused here)
    if (!step_traits(fs.kind).quantum_ranged || fs.kind == StepKind::Dyn)
      return fail(WAA_ERR_OUT_OF_SCOPE, "node %u inside a feedback loop: this form of the node has no ranged launch (step kind %d)", vid, (int)fs.kind);
    if (fs.kind == StepKind::ConvFft && fs.conv.block != RQ)
      return fail(WAA_ERR_OUT_OF_SCOPE, "a ConvolverNode inside a feedback loop is out of scope (node %u: %d-frame partitions)", vid, fs.conv.block);
    fs.qgroup = p.cur_qgroup;
    if (fs.kind == StepKind::Link || fs.kind == StepKind::ConvCodes) {
      int32_t* lst = nullptr;
      const size_t ints = fs.kind == StepKind::ConvCodes ? (size_t)CONV_CODE_STATE_INTS : 4;
      if ((e = dev_alloc(b, &lst, (size_t)b->n_inst * ints))) return e;
      b->state_bufs.push_back({lst, (size_t)b->n_inst * ints * sizeof(int32_t)});
      (fs.kind == StepKind::Link ? fs.link.state : fs.ccode.state) = lst;
    }
  }
  return 0;
}
// Everything else the members' planning launched — AudioParam tables and summing chains (automation, modulation from OUTSIDE
// the loop: from inside is refused by the driver), per-frame coefficient tables — depends on nothing inside the loop: once, over the
// whole render, in front of the blocks (r05h: left untagged they cut the loop's launches into two runs — garbage, and not
// even the same garbage twice).
static int tag_loop_launches(DynPlan& p, size_t first_loop_step) {
  waa_batch* b = p.b;
  size_t n_ranged = 0;
  for (size_t k2 = first_loop_step; k2 < b->steps.size(); k2++) {
    Step& ls = b->steps[k2];
    const bool ranged = step_traits(ls.kind).quantum_ranged;
    if (ranged && ls.qgroup != p.cur_qgroup) return fail(WAA_ERR_INVALID_STATE, "internal: ranged launch outside its loop");
    if (!ranged) {
      if (!runs_once_in_loop(ls))
        return fail(WAA_ERR_OUT_OF_SCOPE, "a feedback loop with a frozen-state node inside needs a launch of kind %d per block: out of scope", (int)ls.kind);
      ls.qgroup = p.cur_qgroup;
      ls.prologue = true;
    }
    n_ranged += ranged;
  }
  const uint32_t bq = b->qgroup_quanta.back(), n_blocks = (b->n_quanta + bq - 1) / bq;
  plan_note(b, "feedback loop with a frozen-state node inside (oversampled WaveShaper / HRTF panner / short ConvolverNode): cut at the node(s), "
               "%zu launch step(s) per block of %u render quanta (the shortest delay across a cut allows no more), %u blocks = %zu launches per render"
               " — a correctness path: expect ~10 us of host + device time per launch, whatever the batch size",
            n_ranged, bq, n_blocks, (size_t)n_blocks * n_ranged);
  return 0;
}

int plan_quantum_blocked_loop(DynPlan& p, const std::vector<uint32_t>& verts) {
  waa_batch* b = p.b;
  if (int e = flush_group(p)) return e;  // what was pending is complete before the loop starts
  const size_t first_loop_step = b->steps.size();
  p.cur_qgroup = (int)b->qgroup_quanta.size();
  b->qgroup_quanta.push_back(1);
  if (int e = alloc_split_pairs(p, verts, loop_segments(b, verts))) return e;
  b->qgroup_quanta.back() = loop_block_quanta(b, p.xdelay);
  for (uint32_t v : verts) {
    if (int e = enqueue_vertex(p, v)) return e;
    if (!(v & VTX_READER) && is_node_major(b->nodes[v]))
      if (int e = plan_cut_node(p, v)) return e;
  }
  if (int e = flush_group(p)) return e;
  if (int e = tag_loop_launches(p, first_loop_step)) return e;
  p.cur_qgroup = -1;
  p.xdelay.clear();
  return 0;
}

}  // namespace host
}  // namespace waa
