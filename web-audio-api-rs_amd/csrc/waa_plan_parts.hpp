// waa_plan_parts.hpp — what the parts of the planner share.  Host only.
//   waa_plan.cpp         build_plan and its driver build_plan_rest, params, chains (plan_single / plan_chain), block-scheduled loops
//   waa_plan_graph.cpp   processing order, feedback loops, edges in summing order, liveness, static channel counts, units
//   waa_plan_counts.cpp  the replay of the reference's per-quantum silence and channel counts
//   waa_plan_folds.cpp   frozen-node sources, folded delays, materialisation points, edge folds, source views, Biquad-into-Convolver
//   waa_plan_dyn.cpp     dynamic-count groups;  waa_plan_dyn_loop.cpp  ... their loops with node-major members inside
//   waa_plan_loops.cpp   quantum-serial loops, delays;  waa_plan_sources.cpp, waa_plan_conv.cpp,
//   waa_plan_comp.cpp, waa_plan_shaper.cpp, waa_plan_route.cpp, waa_plan_ops.cpp  the node kinds;  waa_plan_check.cpp  validation
#pragma once
#include <map>
#include <set>
#include <vector>

#include "waa_host.hpp"

namespace waa {
namespace host {

// what a launch reads and writes (plan validation, and the prologue decision of block-scheduled loops)
struct StepIo {
  std::vector<const void*> reads, writes;
  bool feedback_reader = false;
};
struct OrderCtx;
// planning units: single nodes and whole feedback loops (scc >= 0), producers first
struct Unit {
  int scc;
  uint32_t id;
};
// What the passes of build_plan hand each other (waa_plan.cpp: build_plan_rest lists them in order).  Everything else they
// decide lives in the nodes (Node::in_edges / live / in_nch / materialized / delay_folded / is_view / fold_conv ...).
struct PlanPass {
  std::vector<uint32_t> items;  // compute_order: vertices in processing order (two per DelayNode)
  std::vector<uint8_t> muted;   // compute_order: nodes of a cycle without a DelayNode
  std::vector<int> scc_of;      // find_loops: feedback loop of a node, -1 outside loops
  int n_scc = 0;
  bool mixed_buffer_counts = false;  // static_channel_counts: instances play AudioBuffers of different widths
  bool count_change_found = false;   // replay_channel_counts, choose_frozen_sources: the plan needs exact per-quantum counts
  std::vector<int> frozen_src;       // choose_frozen_sources: the one source in front of a frozen-state node, or -1
  std::vector<uint32_t> scc_block;   // choose_block_loops: tiles per block of a block-scheduled loop, 0 = quantum-serial
  std::vector<uint8_t> mat_hard, fan_in_only;  // choose_materialisation: materialised for its own reasons / only for a summing consumer
  std::vector<Unit> units;           // order_units
  bool block_loop(uint32_t id) const { return scc_of[id] >= 0 && scc_block[(size_t)scc_of[id]] > 0; }
  bool dynamic(const waa_batch* b) const { return count_change_found || b->force_dynamic; }
};
// waa_plan_graph.cpp
void find_loops(const waa_batch* b, PlanPass& pass);                 // reads muted; writes scc_of, n_scc
int collect_edges(waa_batch* b, const PlanPass& pass);              // reads muted, b->order; writes Node::in_edges / pin_edges / n_consumers, clears live / materialized
void mark_live(waa_batch* b);                                        // reads the edges; writes Node::live
int refuse_static_only_nodes(waa_batch* b, const PlanPass& pass, bool in_loops);  // live compressor / routing / per-instance-IR / per-instance-curve nodes
int refuse_nested_source_modulation(const waa_batch* b);            // (prepass) reads Node::live
int static_channel_counts(waa_batch* b, PlanPass& pass);            // writes Node::in_nch / out_nch, mixed_buffer_counts, b->force_dynamic
void order_units(const waa_batch* b, PlanPass& pass);               // reads scc_of, the edges; writes units
// waa_plan_counts.cpp
int replay_channel_counts(waa_batch* b, PlanPass& pass);            // reads the edges, counts, schedules; writes count_change_found
// waa_plan_folds.cpp (each reads what the ones above it wrote)
void choose_frozen_sources(waa_batch* b, PlanPass& pass);           // writes frozen_src, count_change_found
void choose_block_loops(waa_batch* b, PlanPass& pass);              // writes scc_block
void choose_folded_delays(waa_batch* b, const PlanPass& pass);      // writes Node::delay_folded
void choose_materialisation(waa_batch* b, PlanPass& pass);          // writes Node::materialized, mat_hard, fan_in_only
void fold_fan_in_edges(waa_batch* b, const PlanPass& pass);         // clears Node::materialized of sources / gains that ride on an edge
void choose_source_views(waa_batch* b, const PlanPass& pass);       // writes Node::is_view / view_sig / view_valid
void fold_biquad_into_convolver(waa_batch* b, const PlanPass& pass);  // writes Node::fold_conv / pre_biquad
// waa_plan.cpp
int alloc_signal(waa_batch* b, Node& n);
int plan_single(waa_batch* b, const PlanPass& pass, uint32_t id);   // one node outside a loop or of a block-scheduled loop, with the chain that ends in it
// waa_plan_dyn.cpp
int plan_dynamic_groups(waa_batch* b, const PlanPass& pass);
// ... and what its parts share (waa_plan_dyn.cpp, waa_plan_dyn_loop.cpp)
// A DelayNode of a quantum-blocked loop whose writer and reader fall into different segments talks through memory (DynItem::xline ...)
struct XDelay {
  SignalRef line{};
  uint32_t* aux32 = nullptr;
  int32_t* state = nullptr;
  int writer_seg = -1, reader_seg = -1;
};
struct DynPlan {
  waa_batch* b;
  const PlanPass& pass;
  uint64_t cs;                         // b->code_stride
  std::map<uint32_t, size_t> vpos;     // position of every vertex in the processing order
  std::vector<uint32_t> pending;       // vertices of the current group
  std::set<uint32_t> pending_nodes;    // their node ids
  std::vector<uint8_t> planned_node;
  int cur_qgroup = -1;                 // the quantum-blocked loop whose segments are being planned, or -1
  std::map<uint32_t, XDelay> xdelay;   // ... its delay node id -> cross-segment resources (only pairs that ARE split)
};
bool is_node_major(const Node& n);  // rendered node-major behind the group that publishes its mixed input (convolver with a response, frozen-state node): a loop is cut there
int enqueue_vertex(DynPlan& p, uint32_t v);
int flush_group(DynPlan& p);                     // one dyn_kernel launch for the pending vertices
int plan_dyn_convolver(DynPlan& p, uint32_t id);  // FFT steps + the code kernel behind the group that published the convolver's mixed input
int plan_quantum_blocked_loop(DynPlan& p, const std::vector<uint32_t>& verts);  // waa_plan_dyn_loop.cpp
// vertices of the expanded graph the cycle breaker works on: a DelayNode is two (writer `id`, reader `id | VTX_READER`)
constexpr uint32_t VTX_READER = 0x80000000u;

int device_timeline_param(waa_batch* b, const ParamStore& p, ParamRef* ref);
int upload_param(waa_batch* b, const ParamStore& p, ParamRef* ref);
int param_mode(const Node& n, size_t k);
int node_param(waa_batch* b, uint32_t id, size_t k, ParamRef* ref);
int build_edge_input(waa_batch* b, uint32_t head, int ie, InputRef* out);
int upload_values(waa_batch* b, const std::vector<float>& host, int mode, ParamRef* ref);
int computed_in_nch(const Node& n, int maxc);
bool order_visit(OrderCtx& c, uint32_t v);
void plan_note(waa_batch* b, const char* fmt, ...);
const char* input_kind_name(int k);
const char* op_name(int k);
int slot_for(waa_batch* b, const char* name);
int push_chain_step(waa_batch* b, const std::vector<InputRef>& inputs, int in_nch, int in_interp, const std::vector<OpDesc>& ops, const SignalRef& out);
int temp_signal(waa_batch* b, int nch, SignalRef* out);
int emit_segments(waa_batch* b, std::vector<InputRef> inputs, int in_nch, int in_interp, const std::vector<OpDesc>& ops, const SignalRef& out);
bool is_delay(const waa_batch* b, uint32_t id);
void vertex_targets(const waa_batch* b, uint32_t v, const std::vector<uint8_t>& cut, std::vector<uint32_t>& out);
int materialise_automation(waa_batch* b);
int source_code_rows(waa_batch* b, uint32_t id, uint64_t cs, std::vector<uint8_t>* out);
int build_plan(waa_batch* b);
void io_param(const ParamRef& p, StepIo& io);
void io_input(const InputRef& in, StepIo& io);
StepIo step_io(const waa_batch* b, const Step& st);  // (reads through a view are reported by the owning signal, b->view_owner)
int validate_plan(waa_batch* b);
void fuse_echo_tails(waa_batch* b);
void ring_feed_forward_echoes(waa_batch* b);
void fuse_fm_operators(waa_batch* b);
void fuse_lfo_params(waa_batch* b);
int plan_delay_writer(waa_batch* b, uint32_t id);
int plan_folded_delay_line(waa_batch* b, uint32_t id);
int plan_delay_reader(waa_batch* b, uint32_t id);
uint32_t loop_block_tiles(waa_batch* b, const std::vector<uint32_t>& loop_items);
int plan_loop(waa_batch* b, const std::vector<uint32_t>& loop_items);
int prepare_source_input(waa_batch* b, uint32_t id, InputRef* in);
int widen_narrow_buffers(waa_batch* b, Node& n, uint32_t nch);
int reduce_fan_in(waa_batch* b, std::vector<InputRef>& ins, int in_nch, int interp);
int premix_ordered_inputs(waa_batch* b, uint32_t id, std::vector<InputRef>& ins);
int node_input_signal(waa_batch* b, uint32_t id, SignalRef* out_sig, const SignalRef* target = nullptr, uint64_t* valid = nullptr);
int plan_oscillator(waa_batch* b, uint32_t id);
int conv_block_size(const waa_batch* b, const Node& n);
// source -> Biquad(the same constant coefficients on every context) -> long Convolver: Biquad and Convolver are both LTI, so
// (x * h_biquad) * h_ir = x * (h_biquad * h_ir): fills conv.ir_lti with the filtered impulse response when the filter's memory
// dies out inside the partitions the response occupies anyway (true: folded; the Biquad then costs nothing per render)
bool conv_fold_biquad_into_ir(const waa_batch* b, Node& conv, const Node& q);
int plan_convolver(waa_batch* b, uint32_t id);
int plan_compressor(waa_batch* b, uint32_t id);
int plan_shaper_per_instance(waa_batch* b, uint32_t id);  // waa_plan_shaper.cpp
// waa_plan_route.cpp: ChannelSplitterNode / ChannelMergerNode
int desugar_output_ports(waa_batch* b);
int plan_splitter(waa_batch* b, uint32_t id, bool producer_in_loop);
int plan_splitter_port(waa_batch* b, uint32_t id);
int plan_merger(waa_batch* b, uint32_t id);
int emit_node_ops(waa_batch* b, uint32_t id, int cur_nch, bool head, std::vector<OpDesc>& ops, int* out_nch);
void default_channel_config(Node& n, uint32_t n_out);

}  // namespace host
}  // namespace waa
