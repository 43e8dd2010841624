// waa_run.cpp — the executor: the launches of a finished plan (waa_batch::steps), in order, on the batch's stream.  One switch
// over StepKind per range form (tiles, render quanta); feedback loops block by block.
#include "waa_host.hpp"

using namespace waa;
using namespace waa::host;

// the three shapes nearly every kind has: the descriptor as it stands, or a copy with its tile / quantum range set
template <typename D>
static int launch_whole(waa_batch* b, int slot, const D& d, void (*launch)(const D&, void*)) {
  return timed(b, slot, [&] { launch(d, b->stream); });
}
template <typename D>
static int launch_tiles(waa_batch* b, int slot, D d, uint32_t t0, uint32_t t1, void (*launch)(const D&, void*)) {
  d.tile0 = t0;
  d.tile1 = t1;
  return launch_whole(b, slot, d, launch);
}
template <typename D>
static int launch_quanta(waa_batch* b, int slot, D d, uint32_t q0, uint32_t q1, void (*launch)(const D&, void*)) {
  d.q0 = q0;
  d.q1 = q1;
  return launch_whole(b, slot, d, launch);
}

// one step over the tile range [t0, t1)
static int run_step(waa_batch* b, const Step& st, uint32_t t0, uint32_t t1) {
  const int slot = st.profile_slot;
  switch (st.kind) {  // (every kind, no default: -Werror=switch on this file)
    case StepKind::Chain: {
      if (st.echo_ff && t0 == 0 && t1 == b->n_tiles) {  // the feed-forward echo out of the LDS ring (waa_echo.hip)
        ChainDesc d = st.echo_line;
        d.tile0 = t0;
        d.tile1 = t1;
        return timed(b, slot, [&] { launch_echo_ring(d, d.n_inputs, st.echo_chunk, st.echo_ring, &st.echo_tail, b->stream); });
      }
      ChainDesc d = st.chain;
      d.tile0 = t0;
      d.tile1 = t1;
      return timed(b, slot, [&] { launch_chain(d, st.cmax, b->stream); });
    }
    case StepKind::BiquadStream: {
      if (!st.scan.payload) return launch_tiles(b, slot, st.bq, t0, t1, launch_biquad_stream);
      BiquadStreamDesc d = st.bq;
      d.tile0 = t0;
      d.tile1 = t1;
      return timed(b, slot, [&] { launch_biquad_scan(d, st.scan, b->scan_issued, b->stream); });
    }
    case StepKind::ConvFft: {
      // (inside a block-scheduled feedback loop: the partitions of this tile range; loop_block_tiles made the range a
      // whole number of them)
      ConvDesc d = st.conv;
      d.kb0 = (int)std::min<uint64_t>((uint64_t)t0 * TILE / (uint64_t)d.block, (uint64_t)d.nb);
      d.kb1 = (int)std::min<uint64_t>(((uint64_t)t1 * TILE + (uint64_t)d.block - 1) / (uint64_t)d.block, (uint64_t)d.nb);
      if (d.kb1 <= d.kb0) return 0;
      if (int e = launch_whole(b, st.slot_fwd, d, launch_conv_forward)) return e;
      if (int e = launch_whole(b, st.slot_mac, d, d.per_inst ? launch_conv_inst_mac : launch_conv_mac)) return e;
      return launch_whole(b, st.slot_inv, d, launch_conv_inverse);
    }
    case StepKind::ZeroFill: HIP_TRY(hipMemsetAsync(st.zero_ptr, 0, st.zero_bytes, b->stream)); return 0;
    case StepKind::ConvDirect: {
      ConvDesc d = st.conv;
      d.kb0 = (int)std::min<uint64_t>((uint64_t)t0 * (TILE / 1024), (uint64_t)st.conv.kb1);
      d.kb1 = (int)std::min<uint64_t>((uint64_t)t1 * (TILE / 1024), (uint64_t)st.conv.kb1);
      if (d.kb1 <= d.kb0) return 0;
      return launch_whole(b, st.slot_mac, d, d.per_inst ? launch_conv_inst_direct : launch_conv_direct);
    }
    case StepKind::BiquadCoefs:
      if (st.coef_types) return timed(b, slot, [&] { launch_biquad_coefs_inst(st.coef, st.coef_types, b->stream); });
      return launch_whole(b, slot, st.coef, launch_biquad_coefs);
    case StepKind::IirStream: return launch_tiles(b, slot, st.iir, t0, t1, launch_iir_stream);
    case StepKind::Delay: return launch_tiles(b, slot, st.delay, t0, t1, launch_delay);
    case StepKind::Loop: return launch_whole(b, slot, st.loop, launch_loop);
    case StepKind::Osc: return launch_whole(b, slot, st.osc, launch_osc);
    case StepKind::Dyn: return launch_whole(b, slot, st.dyn, launch_dyn);
    case StepKind::ConvCodes: return launch_whole(b, slot, st.ccode, launch_conv_codes);
    case StepKind::BiquadHp: return st.hp.coefs ? launch_whole(b, slot, st.hp, launch_biquad_hp) : 0;
    case StepKind::PannerGeom: return launch_whole(b, slot, st.geom, launch_panner_geom);
    case StepKind::Timeline: return launch_whole(b, slot, st.tl, launch_timeline);
    case StepKind::Link: return launch_whole(b, slot, st.link, launch_link);
    case StepKind::QGemm: return launch_whole(b, slot, st.qgemm, launch_qgemm);
    case StepKind::Hrtf: return launch_whole(b, slot, st.hrtf, launch_hrtf);
    case StepKind::BiquadTileDigest: return launch_whole(b, slot, st.lanes, launch_biquad_tile_digest);
    case StepKind::BiquadLanes: return launch_tiles(b, slot, st.lanes, t0, t1, launch_biquad_lanes);
    case StepKind::OsFft: return launch_whole(b, slot, st.osfft, launch_osfft);
    case StepKind::Compressor:  // (never inside a feedback loop: always the whole render)
      if (int e = launch_whole(b, st.slot_fwd, st.comp, launch_compressor_level)) return e;
      if (int e = launch_whole(b, st.slot_mac, st.comp, launch_compressor_detector)) return e;
      if (int e = launch_whole(b, st.slot_inv, st.comp, launch_compressor_apply)) return e;
      return st.meter.out ? launch_whole(b, st.slot_meter, st.meter, launch_compressor_meter) : 0;  // (the meter is opt-in: desc.i[0])
    case StepKind::Route: return launch_whole(b, slot, st.route, launch_route);  // (never inside a feedback loop)
    case StepKind::ShaperInst: return launch_whole(b, slot, st.shaper, launch_shaper_inst);  // (never inside a feedback loop: the whole render)
  }
  return fail(WAA_ERR_INVALID_STATE, "internal: step kind %d is not a StepKind", (int)st.kind);
}

// one ranged step of a quantum-blocked loop (dynamic-count plans): only the kinds the planner puts there — the cases with a
// launch are StepTraits::quantum_ranged, which is what the planner asks
static int run_step_q(waa_batch* b, const Step& st, uint32_t q0, uint32_t q1) {
  const int slot = st.profile_slot;
  switch (st.kind) {
    case StepKind::Dyn: return launch_quanta(b, slot, st.dyn, q0, q1, launch_dyn);
    case StepKind::Link: return launch_quanta(b, slot, st.link, q0, q1, launch_link);
    case StepKind::Hrtf: return launch_quanta(b, slot, st.hrtf, q0, q1, launch_hrtf);
    case StepKind::OsFft: return launch_quanta(b, slot, st.osfft, q0, q1, launch_osfft);
    case StepKind::ConvFft: {  // a ConvolverNode with 128-frame partitions: block k of its transforms IS render quantum k
      ConvDesc d = st.conv;
      if (d.block != RQ) return fail(WAA_ERR_INVALID_STATE, "internal: a convolver with %d-frame partitions inside a quantum-blocked loop", d.block);
      d.kb0 = (int)std::min<uint32_t>(q0, (uint32_t)d.nb);
      d.kb1 = (int)std::min<uint32_t>(q1, (uint32_t)d.nb);
      if (d.kb1 <= d.kb0) return 0;
      if (int e = launch_whole(b, st.slot_fwd, d, launch_conv_forward)) return e;
      if (int e = launch_whole(b, st.slot_mac, d, launch_conv_mac)) return e;
      return launch_whole(b, st.slot_inv, d, launch_conv_inverse);
    }
    case StepKind::ConvCodes: return launch_quanta(b, slot, st.ccode, q0, q1, launch_conv_codes);
    case StepKind::Chain:
    case StepKind::BiquadStream:
    case StepKind::ZeroFill:
    case StepKind::ConvDirect:
    case StepKind::BiquadCoefs:
    case StepKind::IirStream:
    case StepKind::Delay:
    case StepKind::Loop:
    case StepKind::Osc:
    case StepKind::BiquadHp:
    case StepKind::PannerGeom:
    case StepKind::Timeline:
    case StepKind::QGemm:
    case StepKind::BiquadTileDigest:
    case StepKind::BiquadLanes:
    case StepKind::Compressor:
    case StepKind::Route:
    case StepKind::ShaperInst: break;
  }
  return fail(WAA_ERR_INVALID_STATE, "internal: step kind %d inside a quantum-blocked loop", (int)st.kind);
}

namespace waa {
namespace host {

int run_steps(waa_batch* b) {
  // every render starts from the initial state (offline contexts render exactly once; re-rendering the
  // same batch is what the benchmark loop does)
  for (auto& sb : b->state_bufs) HIP_TRY(hipMemsetAsync(sb.first, 0, sb.second, b->stream));
  for (auto& sb : b->ones_bufs) HIP_TRY(hipMemsetAsync(sb.first, 0xFF, sb.second, b->stream));
  for (auto& n : b->nodes) n.an = Node::AnBatch{};
  for (auto& v : b->scan_issued) v = 0;
  for (size_t i = 0; i < b->steps.size();) {
    const Step& st = b->steps[i];
    if (st.qgroup >= 0) {
      // a feedback loop cut at frozen-state nodes: its launches in order, over the same few quanta each, block after block
      size_t j = i;
      while (j < b->steps.size() && b->steps[j].qgroup == st.qgroup) j++;
      for (size_t k = i; k < j; k++)
        if (b->steps[k].prologue) {  // param tables and chains that only depend on data from outside the loop: once, whole render
          int e = run_step(b, b->steps[k], 0, b->n_tiles);
          if (e) return e;
        }
      const uint32_t bq = b->loops_one_quantum ? 1u : std::max<uint32_t>(1, b->qgroup_quanta[(size_t)st.qgroup]);
      if (bq > 1) b->loops_unsettled = true;
      // (the first block is one quantum: every delay line starts as one silent channel, so the count moves in quantum 0 of
      // nearly every graph — and a change in a block's LAST quantum is the one place where it is harmless)
      for (uint32_t q0 = 0; q0 < b->n_quanta;) {
        const uint32_t q1 = std::min<uint32_t>(b->n_quanta, q0 + (q0 == 0 ? 1u : bq));
        for (size_t k = i; k < j; k++) {
          if (b->steps[k].prologue) continue;
          int e = run_step_q(b, b->steps[k], q0, q1);
          if (e) return e;
        }
        q0 = q1;
      }
      i = j;
      continue;
    }
    if (st.group < 0) {
      if (!st.echo_fused) {  // (a fused tail was rendered by its loop's launch)
        int e = run_step(b, st, 0, b->n_tiles);
        if (e) return e;
      }
      i++;
      continue;
    }
    // block-scheduled feedback loop: steps [i, j) block by block (graph.rs cycle breaker, see build_plan)
    size_t j = i;
    while (j < b->steps.size() && b->steps[j].group == st.group) j++;
    for (size_t k = i; k < j; k++)
      if (b->steps[k].prologue) {
        int e = run_step(b, b->steps[k], 0, b->n_tiles);
        if (e) return e;
      }
    const uint32_t bt = b->group_tiles[st.group];
    {
      // a loop that is ONE element-wise launch per block (the echo loop): one persistent launch can walk the blocks itself
      // (WAA_PERSISTENT_LOOP=1).  Measured on the fb workload (1024 contexts x 10 s, 47 blocks): 5.17-5.20 ms against
      // 5.19-5.37 ms for the 47 launches — the loop is bound by its 3 x 3.9 GB per pass at 16 wavefronts per CU, not by the
      // launches; opt-in, parity-tested (tests/test_cycles.py), not the default.
      size_t n_body = 0, body = 0;
      for (size_t k = i; k < j; k++)
        if (!b->steps[k].prologue && !b->steps[k].echo_fused) {  // (fused: body launches the ring kernel's BQ form stands for)
          n_body++;
          body = k;
        }
      if (n_body == 1 && b->steps[body].kind == StepKind::Chain && b->steps[body].echo_fb >= 0) {  // (decided by the planner)
        // the echo loop with its delay line in LDS: the whole loop in one launch (waa_echo.hip)
        const Step& bs = b->steps[body];
        ChainDesc d = bs.chain;
        d.tile0 = 0;
        d.tile1 = b->n_tiles;
        int e = timed(b, bs.profile_slot, [&] {
          launch_echo_ring(d, bs.echo_fb, bs.echo_chunk, bs.echo_ring, bs.echo_tail_step >= 0 ? &bs.echo_tail : nullptr, b->stream,
                           bs.echo_bq.coefs ? &bs.echo_bq : nullptr);
        });
        if (e) return e;
        i = j;
        continue;
      }
      if (n_body == 1 && b->steps[body].kind == StepKind::Chain && b->steps[body].cmax <= 2 && measure_switch("WAA_PERSISTENT_LOOP")) {
        const Step& bs = b->steps[body];
        bool element_wise = true;
        for (int o = 0; o < bs.chain.n_ops; o++) element_wise &= bs.chain.ops[o].kind != OP_BIQUAD;
        int curve_op = -1;
        if (element_wise && !resample_shape(bs.chain, &curve_op)) {
          ChainDesc d = bs.chain;
          d.tile0 = 0;
          d.tile1 = b->n_tiles;
          d.persist_block = bt * (TILE / 256);
          int e = timed(b, bs.profile_slot, [&] { launch_chain(d, bs.cmax, b->stream); });
          if (e) return e;
          i = j;
          continue;
        }
      }
    }
    for (uint32_t t0 = 0; t0 < b->n_tiles; t0 += bt) {
      const uint32_t t1 = std::min(b->n_tiles, t0 + bt);
      for (size_t k = i; k < j; k++)
        if (!b->steps[k].prologue && !b->steps[k].echo_fused) {
          int e = run_step(b, b->steps[k], t0, t1);
          if (e) return e;
        }
    }
    i = j;
  }
  return WAA_OK;
}

}  // namespace host
}  // namespace waa
