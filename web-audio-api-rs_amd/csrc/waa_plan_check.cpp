// waa_plan_check.cpp — what every launch of a plan reads and writes (step_io) and the read-before-write validation of the
// finished launch list (split out of waa_plan.cpp in round 4).
#include <array>
#include <set>

#include "waa_host.hpp"
#include "waa_plan_parts.hpp"

namespace waa {
namespace host {

// ---- plan validation -----------------------------------------------------------------------------------------
// The plan is a linear list of launches over shared device buffers; nothing but their order makes a consumer see
// its producer's data.  This check walks the list once and refuses a plan in which a launch reads a buffer that
// some launch of the plan writes, but none has written yet — an ordering bug of the planner would otherwise
// render stale or zero data silently.  The only legal read-before-write is a DelayNode reader inside a feedback
// loop (it reads the PREVIOUS quanta of a line that is filled later in the same pass).
void io_param(const ParamRef& p, StepIo& io) {
  if (p.base && p.mode == 2) io.reads.push_back(p.base);  // per-frame values: possibly produced by a param chain
}
void io_input(const InputRef& in, StepIo& io) {
  if (in.kind == IN_SIGNAL || (in.kind == IN_DELAYED && !in.feedback)) io.reads.push_back(in.sig.base);
  if (in.kind == IN_CONSTANT) io_param(in.offset, io);
  if (in.has_gain) io_param(in.gain, io);
}
// A read through a VIEW (one channel of another signal: an output of a ChannelSplitterNode, waa_plan_route.cpp) is a read of the signal
// that owns the memory: reads are reported by the owner's base (waa_batch::view_owner), so that the read-after-write check below
// and every fusion that asks "who else reads this signal" see them.
static StepIo step_io_raw(const Step& st);
StepIo step_io(const waa_batch* b, const Step& st) {
  StepIo io = step_io_raw(st);
  if (!b->view_owner.empty())
    for (const void*& r : io.reads) {
      auto it = b->view_owner.find(r);
      if (it != b->view_owner.end()) r = it->second;
    }
  return io;
}
static StepIo step_io_raw(const Step& st) {
  StepIo io;
  switch (st.kind) {  // (every kind, no default: a new kind that forgets its case is a compiler warning, not an empty read set)
    case StepKind::Chain: {
      const ChainDesc& c = st.chain;
      for (int k = 0; k < c.n_inputs; k++) io_input(c.in[k], io);
      for (int o = 0; o < c.n_ops; o++) {
        const OpDesc& op = c.ops[o];
        io_param(op.p0, io);
        io_param(op.p1, io);
        io_param(op.p2, io);
        io_param(op.p3, io);
        io_param(op.p4, io);
        if (op.kind == OP_BIQUAD && op.i0 == 2) io.reads.push_back(op.ptr0);  // per-frame coefficient table
      }
      io.writes.push_back(c.out.base);
      break;
    }
    case StepKind::BiquadStream:
      io_input(st.bq.in, io);
      if (st.bq.vary >= 2) io.reads.push_back(st.bq.coefs);
      if (st.bq.vary == 3) io.reads.push_back(st.bq.hp);
      io.writes.push_back(st.bq.out.base);
      break;
    case StepKind::ConvFft:
    case StepKind::ConvDirect:
      io.reads.push_back(st.conv.in.base);
      io.writes.push_back(st.conv.out.base);
      break;
    case StepKind::Compressor:
      io.reads.push_back(st.comp.in.base);
      io.writes.push_back(st.comp.out.base);
      if (st.meter.out) io.writes.push_back(st.meter.out);  // (the reduction trace: read by the getters alone)
      break;
    case StepKind::ShaperInst:
      io.reads.push_back(st.shaper.in.base);
      io.writes.push_back(st.shaper.out.base);
      break;
    case StepKind::ZeroFill:
      io.writes.push_back(st.zero_ptr);
      break;
    case StepKind::BiquadCoefs:
      io_param(st.coef.frequency, io);
      io_param(st.coef.detune, io);
      io_param(st.coef.q, io);
      io_param(st.coef.gain, io);
      if (st.coef_types) io.reads.push_back(st.coef_types);  // one filter type per instance (uploaded at plan time)
      io.writes.push_back(st.coef.coefs);
      break;
    case StepKind::Timeline:
      io.writes.push_back(st.tl.out);
      break;
    case StepKind::PannerGeom:
      for (int k = 0; k < 15; k++) io_param(st.geom.p[k], io);
      if (st.geom.opts) io.reads.push_back(st.geom.opts);  // one option set per instance (uploaded at plan time)
      io.writes.push_back(st.geom.az);
      io.writes.push_back(st.geom.gl_mono);
      io.writes.push_back(st.geom.gr_mono);
      io.writes.push_back(st.geom.gl_stereo);
      io.writes.push_back(st.geom.gr_stereo);
      io.writes.push_back(st.geom.dg);
      io.writes.push_back(st.geom.cg);
      break;
    case StepKind::BiquadHp:
      if (st.hp.coefs) {
        io.reads.push_back(st.hp.coefs);
        io.writes.push_back(st.hp.hp);
      }
      break;
    case StepKind::BiquadTileDigest:
      io.reads.push_back(st.lanes.coefs);
      io.writes.push_back(st.lanes.ht);
      break;
    case StepKind::BiquadLanes:
      io_input(st.lanes.in, io);
      io.reads.push_back(st.lanes.coefs);
      io.reads.push_back(st.lanes.ht);
      io.writes.push_back(st.lanes.out.base);
      break;
    case StepKind::IirStream:
      io_input(st.iir.in, io);
      io.writes.push_back(st.iir.out.base);
      break;
    case StepKind::Delay:
      io.reads.push_back(st.delay.in.base);
      io_param(st.delay.delay, io);
      io.writes.push_back(st.delay.out.base);
      io.feedback_reader = st.delay.in_cycle != 0;
      break;
    case StepKind::Route:  // (the terms of a route launch: recorded by the planner, views resolved)
    case StepKind::Loop:
    case StepKind::Dyn:
    case StepKind::QGemm:
    case StepKind::Hrtf:
    case StepKind::OsFft:
      io.reads = st.loop_reads;
      io.writes = st.loop_writes;
      break;
    case StepKind::Osc:
      io_param(st.osc.frequency, io);
      io_param(st.osc.detune, io);
      io.writes.push_back(st.osc.out.base);
      break;
    case StepKind::ConvCodes:
    case StepKind::Link:
      // nothing reported: both work on per-quantum code tables and state words, which no launch list entry orders.  ConvCodes also
      // tests the convolver's input and clears quanta of its output in place; it is planned right behind the ConvFft launch that
      // reports both signals.  (This is why the echo-tail fusion takes their reads as unknown: StepTraits.)
      break;
  }
  return io;
}

int validate_plan(waa_batch* b) {
  std::vector<StepIo> ios;
  std::set<const void*> produced, written;
  for (const Step& st : b->steps) {
    ios.push_back(step_io(b, st));
    for (const void* w : ios.back().writes)
      if (w) produced.insert(w);
  }
  for (size_t k = 0; k < b->steps.size(); k++) {
    const StepIo& io = ios[k];
    const StepKind kind = b->steps[k].kind;
    if (kind == StepKind::Loop || kind == StepKind::Dyn) {  // the items of a quantum-serial launch hand over inside the kernel
      for (const void* w : io.writes) written.insert(w);
    }
    for (const void* r : io.reads) {
      if (!r || !produced.count(r) || written.count(r)) continue;
      if (io.feedback_reader && r == b->steps[k].delay.in.base) continue;
      return fail(WAA_ERR_INVALID_STATE, "internal: launch %zu of the plan (kind %d, %s) reads a buffer that a later launch produces", k,
                  (int)kind, step_traits(kind).name);
    }
    for (const void* w : io.writes)
      if (w) written.insert(w);
  }
  return 0;
}

}  // namespace host
}  // namespace waa
