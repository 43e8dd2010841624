// waa_plan_shaper.cpp — WaveShaperNode with one curve per instance as a node-major step (kernel: waa_shaper_inst.hip).  The node
// ends a chain like a DynamicsCompressorNode: its mixed input is a materialised signal (or a source read in place), it is
// rendered by one launch of its own, its output is a materialised signal.
#include "waa_host.hpp"
#include "waa_plan_parts.hpp"

namespace waa {
namespace host {

int plan_shaper_per_instance(waa_batch* b, uint32_t id) {
  Node& n = b->nodes[id];
  if (n.in_nch < 1 || n.in_nch > MAX_CH || n.out_nch != n.in_nch)
    return fail(WAA_ERR_INVALID_STATE, "internal: WaveShaperNode %u with per-instance curves planned with %d -> %d channels", id, n.in_nch, n.out_nch);
  if (n.desc.i[0] != WAA_OVERSAMPLE_NONE)
    return fail(WAA_ERR_INVALID_STATE, "internal: oversampled WaveShaperNode %u with per-instance curves got past refuse_static_only_nodes", id);
  const uint64_t n_tiles = (b->lp + SHAPER_TILE - 1) / SHAPER_TILE;
  if (n_tiles * b->n_inst >= (1ull << 31))
    return fail(WAA_ERR_OUT_OF_SCOPE, "WaveShaperNode %u with per-instance curves: %llu time tiles x %u instances exceed one launch", id,
                (unsigned long long)n_tiles, b->n_inst);
  SignalRef in_sig{};
  uint64_t in_valid = b->lp;
  int e = node_input_signal(b, id, &in_sig, nullptr, &in_valid);
  if (e) return e;
  // the pool: one row per distinct curve (found by content), every row on a 16-byte boundary, the pool padded to whole 16-byte
  // groups (the kernel stages a row with 16-byte loads)
  std::map<std::string, uint32_t> row_of_key;
  std::vector<float> pool;
  std::vector<ShaperRow> rows(b->n_inst);
  uint32_t shortest = 0xffffffffu, longest = 0, n_pass = 0;
  for (uint32_t i = 0; i < b->n_inst; i++) {
    const std::vector<float>* c = n.curve_of(i);
    if (!c) {
      rows[i] = ShaperRow{0, 0};
      n_pass++;
      continue;
    }
    if (c->empty())  // (waa_waveshaper_set_curve takes one: apply_curve then returns 0 for every sample, a length of 0 here means "no curve")
      return fail(WAA_ERR_OUT_OF_SCOPE, "WaveShaperNode %u with per-instance curves: the shared curve has no points (instance %u uses it)", id, i);
    const std::string key(reinterpret_cast<const char*>(c->data()), c->size() * sizeof(float));
    auto it = row_of_key.find(key);
    if (it == row_of_key.end()) {
      it = row_of_key.emplace(key, (uint32_t)pool.size()).first;
      pool.insert(pool.end(), c->begin(), c->end());
      pool.resize((pool.size() + 3) / 4 * 4, 0.f);
    }
    rows[i] = ShaperRow{it->second, (uint32_t)c->size()};
    shortest = std::min(shortest, rows[i].length);
    longest = std::max(longest, rows[i].length);
  }
  if (pool.empty()) return fail(WAA_ERR_INVALID_STATE, "internal: WaveShaperNode %u in per-instance mode without any curve", id);
  float* d_pool = nullptr;
  ShaperRow* d_rows = nullptr;
  if ((e = dev_upload(b, &d_pool, pool)) || (e = dev_upload(b, &d_rows, rows))) return e;
  const bool in_lds = longest <= (uint32_t)SHAPER_LDS_CAP;
  Step st;
  st.kind = StepKind::ShaperInst;
  ShaperInstDesc& d = st.shaper;
  std::memset(&d, 0, sizeof d);
  d.in = in_sig;
  d.in_valid = in_valid;
  d.out = n.sig;
  d.pool = d_pool;
  d.rows = d_rows;
  d.n_inst = b->n_inst;
  d.n_quanta = b->n_quanta;
  d.frames = b->lp;
  d.nch = n.in_nch;
  d.lds_floats = in_lds ? (longest + 3) / 4 * 4 : 0u;
  st.profile_slot = slot_for(b, "shaper_inst_kernel");
  b->steps.push_back(st);
  plan_note(b, "shaper node %u: %dch, one curve per instance: %zu distinct curve(s) of %u .. %u points, %u instance(s) without a curve pass through; "
               "form %s (cap %d points) -> shaper_inst_kernel",
            id, d.nch, row_of_key.size(), shortest, longest, n_pass,
            in_lds ? "A: every instance's curve staged in LDS" : "B: curves read from global memory", SHAPER_LDS_CAP);
  return 0;
}

}  // namespace host
}  // namespace waa
