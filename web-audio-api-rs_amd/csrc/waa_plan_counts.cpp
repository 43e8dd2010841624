// waa_plan_counts.cpp — static vs dynamic channel counts: the planner's replay of the reference's per-quantum silence and
// channel-count propagation.
//
// The reference counts a silent input as mono, so the channel count of a signal changes mid-render when a narrow and a wide
// producer are not active over the same quanta, when a source ends, when a Gain is (at times) zero.  Count-sensitive nodes then
// differ from the static plan, which renders the static (maximal) count throughout: filters keep per-channel state, the
// panners use another law for mono input, the convolver routes by count, a DelayNode re-mixes its whole line to the count of
// the current input, layouts above stereo and the discrete interpretation do not commute with an earlier speakers up-mix.
// The planner replays the propagation per quantum from what the host knows (source windows, delay times, zero gains;
// data-dependent filter tails are bounded from both sides) and reports the first affected node in the plan;
// WAA_STRICT_CHANNEL_COUNTS turns the note into status 4.
#include "waa_host.hpp"
#include "waa_plan_parts.hpp"

namespace waa {
namespace host {

bool inputs_mix_in_order_differs(const waa_batch* b, const Node& n, uint64_t active);

namespace {

// what the host knows about one instance: first and last active quantum of every source, the shortest and longest delay of
// every DelayNode in quanta, the quanta in which a GainNode is zero, whether a WaveShaper's curve turns silence into a signal;
// `sig` is all of it as bytes (instances with the same signature are simulated once)
struct ReplayInputs {
  std::vector<double> lo, hi, shift, shift_hi;
  std::vector<std::vector<uint8_t>> zero_gain;
  std::vector<uint8_t> wakes;  // WaveShaperNode: the centre of THIS instance's curve is not 0 (waveshaper.rs:498-509)
  std::string sig;
};
// per node and quantum: active or silent, channel count; of the node's output and of its mixed input
struct ReplayState {
  std::vector<std::vector<uint8_t>> act, cnt, in_act, in_cnt;
  ReplayState(uint32_t N, uint32_t nq)
      : act(N, std::vector<uint8_t>(nq)), cnt(N, std::vector<uint8_t>(nq)), in_act(N, std::vector<uint8_t>(nq)), in_cnt(N, std::vector<uint8_t>(nq)) {}
};
using EndCache = std::map<std::pair<uint32_t, SchedKey>, int64_t>;  // (source node, schedule) -> quantum of its end

bool is_source(uint32_t kind) { return kind == WAA_NODE_BUFFER_SOURCE || kind == WAA_NODE_CONSTANT_SOURCE || kind == WAA_NODE_OSCILLATOR; }
bool in_cut_loop(const waa_batch* b, uint32_t id) { return id < b->cut.size() && b->cut[id]; }

// the quantum in which a BufferSource really ends: the scheduling replay with this instance's playbackRate and detune per
// quantum (an automated rate moves the end; an estimate from the slowest rate claimed the source active — and the signal
// stereo — for longer than the reference renders it)
int64_t source_end_quantum(waa_batch* b, uint32_t id, uint32_t inst, EndCache& end_cache) {
  Node& n = b->nodes[id];
  const SourceSched& ss = n.sched[inst];
  const DeviceBuffer& bf = n.bufs[inst];
  const ParamStore& p_rate = n.params[WAA_PARAM_SOURCE_PLAYBACK_RATE];
  const ParamStore& p_det = n.params[WAA_PARAM_SOURCE_DETUNE];
  const bool automated = !p_rate.blocks.empty() || !p_det.blocks.empty();
  // (constant params: the key needs their one value; the per-quantum vectors only for a replay)
  const SchedKey key(ss.start, ss.stop, ss.offset, ss.duration, ss.looping, ss.loop_start, ss.loop_end, bf.frames, bf.sr,
                     p_rate.fix(p_rate.cst[inst]), p_det.fix(p_det.cst[inst]));
  auto it = automated ? end_cache.end() : end_cache.find(std::make_pair(id, key));
  if (it != end_cache.end()) return it->second;
  std::vector<float> rate_q = param_per_quantum(b, p_rate, inst, nullptr);
  std::vector<float> det_q = param_per_quantum(b, p_det, inst, nullptr);
  if (automated) {
    SchedOut so;
    schedule_source(b, ss, bf.frames, bf.sr, true, rate_q, det_q, &so);
    return so.ended_quantum;
  }
  const int64_t endq = schedule_source_cached(b, id, key, ss, bf.frames, bf.sr, true, rate_q, det_q)->ended_quantum;
  end_cache[std::make_pair(id, key)] = endq;
  return endq;
}

void replay_inputs(waa_batch* b, uint32_t inst, EndCache& end_cache, ReplayInputs& in) {
  const uint32_t N = (uint32_t)b->nodes.size(), nq = b->n_quanta;
  const double qsec = (double)RQ / (double)b->sr;
  in.lo.assign(N, 1e300);
  in.hi.assign(N, -1.);
  in.shift.assign(N, 0.);
  in.shift_hi.assign(N, 0.);
  in.zero_gain.assign(N, {});
  in.wakes.assign(N, 0);
  in.sig.clear();
  auto add_sig = [&](double v) { in.sig.append(reinterpret_cast<const char*>(&v), sizeof v); };
  for (uint32_t id : b->order) {
    Node& n = b->nodes[id];
    if (!n.live) continue;
    const uint32_t kind = n.desc.kind;
    if (is_source(kind)) {
      const SourceSched& ss = n.sched[inst];
      in.lo[id] = ss.start == DBL_MAX ? 1e300 : std::floor(ss.start / qsec);
      in.hi[id] = ss.stop != DBL_MAX ? std::ceil(ss.stop / qsec) : 1e300;
      // a ConstantSourceNode is silent until it starts and NEVER again: past its stop time it keeps rendering zeros
      // into a non-silent mono quantum (constant_source.rs:203-258) — a narrower-than-static input for whatever
      // count-sensitive node it feeds together with a wider source that has ended (fuzz seed 1579), yet nothing
      // but zeros for the nodes whose silence is data dependent (a DelayNode behind it falls silent: seed 3071).
      // Both readings are simulated (const_forever).
      if (kind == WAA_NODE_BUFFER_SOURCE && n.bufs[inst].valid) {
        const int64_t endq = source_end_quantum(b, id, inst, end_cache);
        if (endq >= 0) in.hi[id] = std::min(in.hi[id], (double)endq + 1.);
      }
      if (kind == WAA_NODE_BUFFER_SOURCE && !n.bufs[inst].valid) in.lo[id] = 1e300;
      add_sig(in.lo[id]);
      add_sig(in.hi[id]);
    } else if (kind == WAA_NODE_DELAY) {
      // a delay that is not a whole number of quanta: whether the first delayed samples land in this quantum or
      // the next depends on where inside its quantum the input started — both are simulated.  A delayTime that
      // varies (k-rate or a-rate automation) is simulated at its shortest and at its longest value; one that is
      // modulated by the graph is only known to lie in [0, maxDelayTime].
      const ParamStore& pd = n.params[WAA_PARAM_DELAY_DELAY_TIME];
      double dmin = (double)pd.fix(pd.cst[inst]), dmax = dmin;
      for (auto& blk : pd.blocks) {
        if (!(blk.inst == WAA_ALL_INSTANCES || blk.inst == inst)) continue;
        for (float dv : blk.v) {
          dmin = std::min(dmin, (double)pd.fix(dv));
          dmax = std::max(dmax, (double)pd.fix(dv));
        }
      }
      const bool modulated = (WAA_PARAM_DELAY_DELAY_TIME < n.pin_edges.size() && !n.pin_edges[WAA_PARAM_DELAY_DELAY_TIME].empty()) ||
                             pd.dev_tl;  // (replayed on the device: only known to lie in [0, maxDelayTime])
      if (modulated) {
        dmin = 0.;
        dmax = n.desc.d[0];
      }
      in.shift[id] = std::floor(dmin / qsec);
      in.shift_hi[id] = std::ceil(dmax / qsec);
      if (in_cut_loop(b, id)) {  // inside a loop: >= one quantum
        in.shift[id] = std::max(in.shift[id], 1.);
        in.shift_hi[id] = std::max(in.shift_hi[id], 1.);
      }
      add_sig(in.shift[id]);
      add_sig(in.shift_hi[id]);
    } else if (kind == WAA_NODE_GAIN && param_mode(n, 0) != 2) {
      std::vector<uint8_t>& zero = in.zero_gain[id];
      const auto gv = param_per_quantum(b, n.params[0], inst, nullptr);
      bool any = false;
      if (gv.size() == 1) {
        // one value for the whole render (the usual case): no per-quantum table unless that value is a zero —
        // filling and scanning n_quanta entries per instance and GainNode was 7.7 ms of a 1024-context plan
        any = std::fabs(gv[0]) <= 1e-6f;
        if (any) zero.assign(nq, 1);
      } else {
        zero.assign(nq, 0);
        for (uint32_t q = 0; q < nq; q++) {
          zero[q] = std::fabs(gv[q]) <= 1e-6f;
          any |= zero[q] != 0;
        }
      }
      if (!any) zero.clear();
      for (uint8_t z : zero) in.sig.push_back((char)z);
      in.sig.push_back('|');
    } else if (kind == WAA_NODE_WAVESHAPER) {
      const std::vector<float>* curve = n.curve_of(inst);
      in.wakes[id] = curve && !(std::fabs(curve_at_zero(*curve)) < 1e-9f);
      // (one curve per instance: two instances that differ only in this flag are two simulations)
      if (n.per_inst_curve()) in.sig.push_back(in.wakes[id] ? 'w' : 's');
    }
  }
}

// One simulation: delays at `dshift` quanta, the nodes of `long_tail` never silent again once they were active (the others
// fall silent with their input), a stopped ConstantSource silent (or, const_forever, rendering zeros on one channel).
void simulate(const waa_batch* b, const PlanPass& pass, const ReplayInputs& in, const std::vector<double>& dshift,
              const std::vector<uint8_t>& long_tail, bool const_forever, ReplayState& s) {
  const uint32_t N = (uint32_t)b->nodes.size(), nq = b->n_quanta;
  std::vector<std::vector<uint8_t>>&act = s.act, &cnt = s.cnt, &in_act = s.in_act, &in_cnt = s.in_cnt;
  for (uint32_t id = 0; id < N; id++) {
    std::fill(act[id].begin(), act[id].end(), 0);
    std::fill(cnt[id].begin(), cnt[id].end(), 1);
  }
  const int passes = pass.n_scc > 0 ? 4 : 1;  // activity travels once around a feedback loop per pass
  for (int it = 0; it < passes; it++)
    for (uint32_t id : b->order) {
      const Node& n = b->nodes[id];
      if (!n.live) continue;
      const uint32_t kind = n.desc.kind;
      if (is_source(kind)) {
        for (uint32_t q = 0; q < nq; q++) {
          act[id][q] = (double)q >= in.lo[id] && ((double)q < in.hi[id] || (const_forever && kind == WAA_NODE_CONSTANT_SOURCE));
          cnt[id][q] = act[id][q] ? (uint8_t)n.out_nch : 1;
        }
        continue;
      }
      for (uint32_t q = 0; q < nq; q++) {
        uint8_t a = 0, c = 1;
        for (int e : n.in_edges) {
          const uint32_t p = b->edges[e].from;
          a |= act[p][q];
          c = std::max(c, cnt[p][q]);
        }
        in_act[id][q] = a;
        in_cnt[id][q] = (uint8_t)computed_in_nch(n, c);
      }
      const bool memory = has_memory(n);
      for (uint32_t q = 0; q < nq; q++) {
        uint8_t a = in_act[id][q], c = in_cnt[id][q];
        if (kind == WAA_NODE_DELAY) {
          // the data is `shift` quanta old; the channel count is the line's, which follows the writer's CURRENT
          // input (delay.rs:469-489) — of the previous quantum when the reader renders first (inside a loop)
          const int64_t qs = (int64_t)q - (int64_t)dshift[id];
          a = qs >= 0 ? in_act[id][qs] : 0;
          const int64_t qc = in_cut_loop(b, id) ? (int64_t)q - 1 : (int64_t)q;
          c = qc >= 0 ? in_cnt[id][qc] : 1;
        } else if (kind == WAA_NODE_DYNAMICS_COMPRESSOR) {
          // the output is the quantum that entered the look-ahead ring D quanta ago, with its channel count; the ring
          // starts out silent (dynamics_compressor.rs:343-349, 452-468)
          const int64_t qs = (int64_t)q - (int64_t)compressor_delay_quanta(b->sr);
          a = qs >= 0 ? in_act[id][qs] : 0;
          c = qs >= 0 ? in_cnt[id][qs] : 1;
        } else if (kind == NODE_SPLITTER_PORT) {
          // channel_splitter.rs:197-206: output k is one channel — channel k of the input bus where an active connection of the
          // splitter has one, the silent block otherwise
          uint8_t widest = 0;
          for (int e : b->nodes[(size_t)n.port_of].in_edges) {
            const uint32_t p = b->edges[e].from;
            if (act[p][q]) widest = std::max(widest, cnt[p][q]);
          }
          a = a && (int)widest > n.port;
          c = 1;
        } else if (kind == WAA_NODE_CHANNEL_MERGER) {
          c = (uint8_t)n.desc.i[0];  // channel_merger.rs:160-168: N channels when any input is active, else one silent channel
        } else if (kind == WAA_NODE_GAIN && !in.zero_gain[id].empty() && in.zero_gain[id][q]) {
          a = 0;
        } else if (kind == WAA_NODE_WAVESHAPER && !a) {
          // a curve that does not map 0 to 0 turns silence into a signal (waveshaper.rs:498-509): active, mono
          if (in.wakes[id]) a = 1;
        }
        if (a) {
          if (kind == WAA_NODE_STEREO_PANNER || kind == WAA_NODE_PANNER) c = 2;
          if (kind == WAA_NODE_CONVOLVER && n.has_ir) c = (c == 1 && n.ir_nch == 1) ? 1 : 2;
        }
        if (memory && long_tail[id] && !a && q > 0 && act[id][q - 1]) {  // still ringing, with the old layout
          a = 1;
          c = cnt[id][q - 1];
        }
        act[id][q] = a;
        cnt[id][q] = a ? c : 1;
      }
    }
}

// A GainNode whose `gain` has an audio-rate input that is SILENT in some quantum: the param is then one value for that quantum
// (param.rs:737-760) and gain.rs:163-179's fast paths apply — a value of 0 emits the silent block (ONE channel), where the
// modulated form of the kernels multiplies by a per-frame table of zeros and keeps the static layout.  Only the zero matters (a
// value of 1 is the same samples either way); rendering it differently from the reference is not on offer: status 4 (suspend
// fuzz seed 90491, round 6: an LFO stopped at a suspend point in front of a k-rate gain that visits 0).
int refuse_zero_gain_behind_a_silent_modulator(const waa_batch* b, uint32_t inst, const ReplayState& s) {
  const uint32_t nq = b->n_quanta;
  for (uint32_t id : b->order) {
    const Node& n = b->nodes[id];
    if (!n.live || n.desc.kind != WAA_NODE_GAIN || n.pin_edges.empty() || n.pin_edges[0].empty() || s.in_act[id].empty()) continue;
    const auto gv = param_per_quantum(b, n.params[0], inst, nullptr);
    for (uint32_t q = 0; q < nq; q++) {
      if (!(std::fabs(gv[gv.size() == 1 ? 0 : q]) <= 1e-6f) || !s.in_act[id][q]) continue;
      bool mod_active = false;
      for (int e : n.pin_edges[0]) mod_active |= s.act[b->edges[e].from][q] != 0;
      if (!mod_active)
        return fail(WAA_ERR_OUT_OF_SCOPE,
                    "gain node %u: its gain is 0 in quantum %u (instance %u) while the audio-rate input of the param is silent — the reference emits "
                    "a silent (one-channel) quantum there (gain.rs:163-171), the modulated gain kernels do not: out of scope",
                    id, q, inst);
    }
  }
  return 0;
}

// What the simulation finds at node `id`, if anything: how its input differs from the static plan (nullptr: it does not) and
// the first quantum where it does.
const char* find_count_change(const waa_batch* b, uint32_t id, const ReplayState& s, uint32_t* at_out) {
  const std::vector<std::vector<uint8_t>>&act = s.act, &cnt = s.cnt, &in_act = s.in_act, &in_cnt = s.in_cnt;
  const uint32_t nq = b->n_quanta;
  const double qsec = (double)RQ / (double)b->sr;
  const Node& n = b->nodes[id];
  if (!n.live || n.in_edges.empty()) return nullptr;
  {
    bool wide_producer = false;
    for (int e : n.in_edges) wide_producer |= b->nodes[b->edges[e].from].out_nch > 2;
    if (n.in_nch <= 1 && !wide_producer) return nullptr;
  }
  const uint32_t kind = n.desc.kind;
  const bool line = kind == WAA_NODE_DELAY || (kind == WAA_NODE_CONVOLVER && n.has_ir);
  bool sensitive = kind == WAA_NODE_BIQUAD || kind == WAA_NODE_IIR_FILTER || kind == WAA_NODE_STEREO_PANNER ||
                   kind == WAA_NODE_PANNER || line || n.in_nch > 2 || n.interp == WAA_INTERP_DISCRETE;
  // (a producer wider than stereo into a mono / stereo node: its DOWN-mix does not commute with the up-mix the static plan made
  // upstream either — a 5.1 signal that is in fact mono goes to L and R as it is, its static 5.1 form through the 5.1 -> stereo
  // matrix; round 6, wide fuzz seed 293: a WaveShaper with curve(0) != 0 on a silent 5.1 input in front of a stereo destination)
  for (int e : n.in_edges) sensitive |= b->nodes[b->edges[e].from].out_nch > 2;
  if (!sensitive) return nullptr;
  // a DelayNode up-mixes its line by copying when the wide signal arrives (= the static plan) but collapses it
  // when the input narrows or falls silent while the line still holds wide material
  const bool narrowing_only = kind == WAA_NODE_DELAY && n.in_nch <= 2 && n.interp != WAA_INTERP_DISCRETE;
  int64_t last_wide = -1;
  const int64_t memory_q = kind == WAA_NODE_DELAY ? (int64_t)std::ceil(n.desc.d[0] / qsec) + 1
                           : kind == WAA_NODE_CONVOLVER ? (int64_t)(n.ir_len / RQ) + 2 : 0;
  const char* what = nullptr;
  uint32_t at = 0;
  for (uint32_t q = 0; q < nq && !what; q++) {
    const bool wide_now = in_act[id][q] && in_cnt[id][q] >= n.in_nch;
    if (in_act[id][q] && !wide_now && !(narrowing_only && last_wide < 0)) {
      if (!narrowing_only || (int64_t)q - last_wide <= memory_q) {
        what = "is narrower than its static channel count";
        at = q;
      }
    }
    if (line && !in_act[id][q] && last_wide >= 0 && (int64_t)q - last_wide <= memory_q && (int64_t)q - last_wide >= 1) {
      what = "falls silent (= mono) while the node still holds multi-channel material";
      at = q;
    }
    if (wide_now) last_wide = q;
  }
  // A ChannelMergerNode directly in front of a panner, and every input of the merger stops before the render does: the
  // merger's output changes from N channels to the one silent channel of channel_merger.rs:166-168 mid-render, and the
  // panning law depends on the count of its input (stereo_panner.rs / panner.rs: mono and stereo laws).  Zeros pan to
  // zeros under either law, so this is CONSERVATIVE: the count change is reported like any other one, and the two
  // routing nodes are static-plan only (refuse_static_only_nodes).
  if (!what && (kind == WAA_NODE_PANNER || kind == WAA_NODE_STEREO_PANNER))
    for (int e : n.in_edges) {
      const uint32_t p = b->edges[e].from;
      if (b->nodes[p].desc.kind != WAA_NODE_CHANNEL_MERGER || b->nodes[p].out_nch < 2) continue;
      bool was_active = false;
      for (uint32_t q = 0; q < nq && !what; q++) {
        if (act[p][q]) {
          was_active = true;
        } else if (was_active) {
          what = "comes from a ChannelMergerNode whose output falls back to one silent channel";
          at = q;
        }
      }
    }
  // mixing rules that do not commute with the speakers up-mix the static plan applied upstream: an input that
  // is active but narrower than its static width, into a discrete or wider-than-stereo mix
  if (!what)
    for (int e : n.in_edges) {
      const uint32_t p = b->edges[e].from;
      const int pw = b->nodes[p].out_nch;
      if (!(n.interp == WAA_INTERP_DISCRETE || n.in_nch > 2 || pw > 2)) continue;
      for (uint32_t q = 0; q < nq && !what; q++)
        if (act[p][q] && cnt[p][q] < pw) {
          what = "mixes a signal that is narrower than its static width with a rule that does not commute with the "
                 "speakers up-mix made upstream (discrete interpretation or more than two channels);";
          at = q;
        }
    }
  // the order of the inputs matters to the mix (inputs_mix_in_order) and not all of them are active over the same quanta: the
  // widths the bus takes — and with them an earlier input's path — change with the activity of the later ones
  if (!what && n.mode != WAA_COUNT_MODE_EXPLICIT && n.in_edges.size() >= 2 && n.in_edges.size() <= 64) {
    std::map<uint64_t, bool> seen;  // (few distinct activity patterns per node)
    for (uint32_t q = 0; q < nq && !what; q++) {
      uint64_t mask = 0;
      for (size_t k = 0; k < n.in_edges.size(); k++)
        if (act[b->edges[n.in_edges[k]].from][q]) mask |= (uint64_t)1 << k;
      if (!mask) continue;
      auto it = seen.find(mask);
      if (it == seen.end()) it = seen.emplace(mask, inputs_mix_in_order_differs(b, n, mask)).first;
      if (it->second) {
        what = "sums signals of different widths whose up-mixes depend on the order and on which of them are active (the reference's input bus grows input by input);";
        at = q;
      }
    }
  }
  *at_out = at;
  return what;
}

}  // namespace

int replay_channel_counts(waa_batch* b, PlanPass& pass) {
  const uint32_t N = (uint32_t)b->nodes.size();
  pass.count_change_found = false;
  ReplayState state(N, b->n_quanta);
  ReplayInputs in;
  std::map<std::string, bool> seen;  // instances with identical host-known inputs are simulated once
  EndCache end_cache;
  bool reported = false;
  for (uint32_t inst = 0; inst < b->n_inst && !reported; inst++) {
    replay_inputs(b, inst, end_cache, in);
    if (seen.count(in.sig)) continue;
    seen[in.sig] = true;
    // Tails are data dependent (a filter renders until its state has decayed).  Both bounds are simulated per node
    // with memory: it falls silent with its input (tail 0), or never again once it was active (tail infinite); a
    // finding under any combination is reported.
    std::vector<uint32_t> mem_nodes;
    for (uint32_t id : b->order)
      if (b->nodes[id].live && has_memory(b->nodes[id])) mem_nodes.push_back(id);
    // every combination of short / long tails for up to 8 nodes with memory, the two uniform bounds beyond that
    const uint32_t n_modes = mem_nodes.size() <= 8 ? (1u << mem_nodes.size()) : 2u;
    std::vector<uint8_t> long_tail(N, 0);
    bool stopped_constant = false;
    for (uint32_t id : b->order)
      stopped_constant |= b->nodes[id].live && b->nodes[id].desc.kind == WAA_NODE_CONSTANT_SOURCE && in.hi[id] < 1e299;
    for (int const_forever = 0; const_forever < (stopped_constant ? 2 : 1) && !reported; const_forever++)
      for (uint32_t mode_index = 0; mode_index < 2 * n_modes && !reported; mode_index++) {
        // (odd: the delays at their longest)
        const uint32_t tail_mode = mode_index >> 1;
        if ((mode_index & 1) && in.shift_hi == in.shift) continue;
        for (size_t k = 0; k < mem_nodes.size(); k++)
          long_tail[mem_nodes[k]] = mem_nodes.size() <= 8 ? ((tail_mode >> k) & 1u) : (uint8_t)tail_mode;
        simulate(b, pass, in, (mode_index & 1) ? in.shift_hi : in.shift, long_tail, const_forever != 0, state);
        if (int e = refuse_zero_gain_behind_a_silent_modulator(b, inst, state)) return e;
        for (uint32_t id : b->order) {
          uint32_t at = 0;
          const char* what = find_count_change(b, id, state, &at);
          if (!what) continue;
          const bool keep_static = measure_switch("WAA_STATIC_CHANNEL_COUNTS") != nullptr;  // A/B aid: the round-1 behaviour
          if (keep_static)
            plan_note(b,
                      "note: the input of node %u %s at quantum %u (instance %u): the reference's dynamic channel count changes "
                      "mid-render, the device renders %d channel(s) throughout (DESIGN.md section 5)",
                      id, what, at, inst, b->nodes[id].in_nch);
          else
            plan_note(b,
                      "the input of node %u %s at quantum %u (instance %u): the reference's channel count changes mid-render -> "
                      "exact per-quantum channel counts (dyn_kernel, DESIGN.md section 3.4)",
                      id, what, at, inst);
          reported = true;
          pass.count_change_found = !keep_static;
          if (keep_static && getenv("WAA_STRICT_CHANNEL_COUNTS"))
            return fail(WAA_ERR_OUT_OF_SCOPE, "node %u: a dynamic channel-count change is not rendered exactly on the device path", id);
          break;
        }
      }
  }
  return 0;
}

}  // namespace host
}  // namespace waa
