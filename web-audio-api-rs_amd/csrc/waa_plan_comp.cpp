// waa_plan_comp.cpp — DynamicsCompressorNode as a node-major step (kernels: waa_compressor.hip).  The node ends a chain like a
// ConvolverNode with a response: its mixed input is a materialised signal (or a source read in place), it is rendered by three
// launches of its own, its output is a materialised signal.
#include "waa_host.hpp"
#include "waa_plan_parts.hpp"

namespace waa {
namespace host {

namespace {

// dynamics_compressor.rs:14-27
float db_to_lin(float v) { return std::pow(10.0f, v / 20.f); }
float lin_to_db(float v) { return v == 0.f ? -1000.f : 20.f * std::log10(v); }

// The block constants of dynamics_compressor.rs:353-389 — every operation in f32, in the reference's order, with the host's
// expf / powf / log10f (the libm calls the reference's f32::exp / powf / log10 end in; this file is built without contraction).
CompRow compressor_row(float threshold, float knee, float ratio, float attack, float release, float sample_rate) {
  CompRow r{};
  const float thr = knee > 0.f ? threshold + knee / 2.f : threshold;
  r.thr = thr;
  r.half_knee = knee / 2.f;
  r.lo = thr - r.half_knee;
  r.hi = thr + r.half_knee;
  r.knee_partial = (1.f / ratio - 1.f) / (2.f * knee);  // (knee = 0: +-inf or NaN, never used: the kernel selects, waa_compressor.hip)
  r.ratio = ratio;
  r.a_tau = std::exp(-1.f / (attack * sample_rate));    // (attack = 0: exp(-inf) = 0, an ordinary value)
  r.r_tau = std::exp(-1.f / (release * sample_rate));
  r.a_one = 1.f - r.a_tau;
  r.r_one = 1.f - r.r_tau;
  const float full_range_gain = thr + (-thr / ratio);
  const float full_range_makeup = 1.f / db_to_lin(full_range_gain);
  r.makeup = lin_to_db(std::pow(full_range_makeup, 0.6f));
  return r;
}

}  // namespace

int plan_compressor(waa_batch* b, uint32_t id) {
  Node& n = b->nodes[id];
  if (n.in_nch < 1 || n.in_nch > 2 || n.out_nch != n.in_nch)
    return fail(WAA_ERR_INVALID_STATE, "internal: DynamicsCompressorNode %u planned with %d -> %d channels", id, n.in_nch, n.out_nch);
  for (size_t k = 0; k < n.params.size(); k++)
    if (n.params[k].mode() == 2 || n.params[k].dev_tl)
      return fail(WAA_ERR_OUT_OF_SCOPE, "DynamicsCompressorNode %u: param %zu has per-frame values; its params are k-rate (dynamics_compressor.rs:187-247)", id, k);
  SignalRef in_sig{};
  uint64_t in_valid = b->lp;
  int e = node_input_signal(b, id, &in_sig, nullptr, &in_valid);
  if (e) return e;
  // the per-quantum table: one row per quantum when every context shares the params ([instance][quantum] otherwise); params that
  // are one constant for the whole render collapse to a single row
  bool shared = true;
  for (const ParamStore& p : n.params) {
    for (uint32_t i = 1; i < b->n_inst; i++) shared = shared && p.cst[i] == p.cst[0];
    for (const ParamBlock& blk : p.blocks) shared = shared && blk.inst == WAA_ALL_INSTANCES;
  }
  const uint32_t n_rows_inst = shared ? 1u : b->n_inst;
  std::vector<std::vector<float>> pv((size_t)n_rows_inst * 5);
  bool varies = false;
  for (uint32_t i = 0; i < n_rows_inst; i++)
    for (size_t k = 0; k < 5; k++) {
      pv[(size_t)i * 5 + k] = param_per_quantum(b, n.params[k], i, nullptr);
      varies |= pv[(size_t)i * 5 + k].size() > 1;
    }
  const uint32_t n_rows_q = varies ? b->n_quanta : 1u;
  std::vector<CompRow> rows((size_t)n_rows_inst * n_rows_q);
  for (uint32_t i = 0; i < n_rows_inst; i++)
    for (uint32_t q = 0; q < n_rows_q; q++) {
      auto at = [&](size_t k) {
        const std::vector<float>& v = pv[(size_t)i * 5 + k];
        return v[v.size() == 1 ? 0 : q];
      };
      rows[(size_t)i * n_rows_q + q] =
          compressor_row(at(WAA_PARAM_COMPRESSOR_THRESHOLD), at(WAA_PARAM_COMPRESSOR_KNEE), at(WAA_PARAM_COMPRESSOR_RATIO),
                         at(WAA_PARAM_COMPRESSOR_ATTACK), at(WAA_PARAM_COMPRESSOR_RELEASE), b->sr);
    }
  CompRow* d_rows = nullptr;
  if ((e = dev_upload(b, &d_rows, rows))) return e;
  float* xl = nullptr;
  if ((e = dev_alloc(b, &xl, (size_t)b->n_inst * b->lp))) return e;
  Step st;
  st.kind = StepKind::Compressor;
  CompDesc& d = st.comp;
  std::memset(&d, 0, sizeof d);
  d.in = in_sig;
  d.in_valid = in_valid;
  d.out = n.sig;
  d.xl = xl;
  d.rows = d_rows;
  d.row_inst_stride = shared ? 0u : n_rows_q;
  d.row_q_stride = varies ? 1u : 0u;
  d.n_inst = b->n_inst;
  d.n_quanta = b->n_quanta;
  d.frames = b->lp;
  d.delay_frames = compressor_delay_quanta(b->sr) * (uint32_t)RQ;
  d.nch = n.in_nch;
  st.slot_fwd = slot_for(b, "compressor_level_kernel");
  st.slot_mac = slot_for(b, "compressor_detector_kernel");
  st.slot_inv = slot_for(b, "compressor_apply_kernel");
  if (n.comp_meter()) {
    // reduction() after every quantum (dynamics_compressor.rs:304-306, stored at :440 / :450): the detector leaves yL of every
    // frame in `xl`, the make-up gain of every (context, quantum) is in the rows — one gather launch behind apply.  The buffer
    // belongs to the plan: a re-armed batch renders a fresh trace into it.
    if ((e = dev_alloc(b, &n.d_comp_red, (size_t)b->n_inst * b->n_quanta))) return e;
    CompMeterDesc& m = st.meter;
    m.yl = xl;
    m.rows = d_rows;
    m.row_inst_stride = d.row_inst_stride;
    m.row_q_stride = d.row_q_stride;
    m.out = n.d_comp_red;
    m.n_inst = b->n_inst;
    m.n_quanta = b->n_quanta;
    m.frames = b->lp;
    st.slot_meter = slot_for(b, "compressor_meter_kernel");
  }
  b->steps.push_back(st);
  plan_note(b, "compressor node %u: %dch, look-ahead %u quanta, %u x %u row(s) of block constants (%s, %s) -> compressor_level_kernel, "
               "compressor_detector_kernel (%u wavefront(s), one lane per context), compressor_apply_kernel; first row: threshold=%g knee=%g "
               "ratio=%g attack=%g release=%g",
            id, d.nch, d.delay_frames / (uint32_t)RQ, n_rows_inst, n_rows_q, shared ? "shared" : "per instance",
            varies ? "per quantum" : "constant", (b->n_inst + 63) / 64, (double)pv[0][0], (double)pv[1][0], (double)pv[2][0], (double)pv[3][0],
            (double)pv[4][0]);
  if (n.comp_meter()) plan_note(b, "compressor node %u: reduction trace, %u x %u values -> compressor_meter_kernel", id, b->n_inst, b->n_quanta);
  return 0;
}

}  // namespace host
}  // namespace waa
