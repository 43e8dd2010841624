// waa_levels_host.cpp — the host side of waa_output_levels, waa_output_level_series and waa_download_all_pcm16_gain
// (include/waa_hip_device.h; the kernels: waa_levels.hip).  Extensions like waa_download_all_pcm16: they read the destination's
// signal where the render left it and are no plan step.  Every call computes from the output as it lies on the device — nothing is
// kept between calls but the workspace, which the batch owns like its PCM staging.
#include <cmath>
#include <cstddef>

#include "../../include/waa_hip_device.h"
#include "waa_host.hpp"
#include "waa_output_calls.hpp"

static_assert(sizeof(waa_level_stats) == 40 && sizeof(waa::LevelRec) == 40, "one 40-byte record per row");
static_assert(offsetof(waa_level_stats, sum_sq) == offsetof(waa::LevelRec, sum_sq) &&
                  offsetof(waa_level_stats, n_nonfinite) == offsetof(waa::LevelRec, n_nonfinite) &&
                  offsetof(waa_level_stats, first_nonfinite) == offsetof(waa::LevelRec, first_nonfinite) &&
                  offsetof(waa_level_stats, n_clipped) == offsetof(waa::LevelRec, n_clipped) &&
                  offsetof(waa_level_stats, peak) == offsetof(waa::LevelRec, peak_bits) &&
                  offsetof(waa_level_stats, reserved) == offsetof(waa::LevelRec, reserved),
              "the device's record is waa_level_stats");

namespace {

// both levels kernels over the destination's signal; *out describes where the results lie in the batch's workspace
int run_levels(waa_batch* b, waa::LevelsDesc* out) {
  const uint64_t rows = (uint64_t)b->n_inst * b->n_out, nq = b->n_quanta;
  const uint64_t n_blocks = (nq + waa::LEVEL_BLOCK_QUANTA - 1) / waa::LEVEL_BLOCK_QUANTA;
  // f64 per (row, quantum) | records per (row, block) | records per row | f32 per (row, quantum): every part 8-byte aligned
  const size_t o_blocks = rows * nq * sizeof(double), o_rows = o_blocks + rows * n_blocks * sizeof(waa::LevelRec),
               o_peak = o_rows + rows * sizeof(waa::LevelRec), bytes = o_peak + rows * nq * sizeof(uint32_t);
  if (!b->levels_ws) {  // (the batch's size never changes)
    char* p = nullptr;
    if (int e = dev_alloc(b, &p, bytes)) return e;
    b->levels_ws = p;
  }
  char* ws = static_cast<char*>(b->levels_ws);
  const waa::SignalRef& s = b->nodes[0].sig;
  waa::LevelsDesc d{};
  d.in = s.base;
  d.frames = b->length;
  d.in_item_stride = s.inst_stride;
  d.in_ch_stride = s.ch_stride;
  d.nch_in = s.base ? (uint32_t)s.nch : 0u;  // (no signal at all: every row is zeros)
  d.nch_out = b->n_out;
  d.n_items = b->n_inst;
  d.n_quanta = b->n_quanta;
  d.n_blocks = (uint32_t)n_blocks;
  d.q_sum_sq = reinterpret_cast<double*>(ws);
  d.blocks = reinterpret_cast<waa::LevelRec*>(ws + o_blocks);
  d.rows = reinterpret_cast<waa::LevelRec*>(ws + o_rows);
  d.q_peak = reinterpret_cast<uint32_t*>(ws + o_peak);
  if (int e = call_launch(b, "output_levels_kernel", [&] { waa::launch_output_levels(d, b->stream); })) return e;
  if (int e = call_launch(b, "output_level_rows_kernel", [&] { waa::launch_output_level_rows(d, b->stream); })) return e;
  *out = d;
  return 0;
}

}  // namespace

extern "C" {

waa_status waa_output_levels(waa_batch* b, waa_level_stats* out) {
  if (!b || !out) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch / destination");
  if (int e = check_rendered(b)) return e;
  if (b->length == 0 || b->n_inst == 0 || b->n_out == 0) return WAA_OK;
  if (int e = wait_for_render(b)) return e;
  waa::LevelsDesc d{};
  if (int e = run_levels(b, &d)) return e;
  const size_t bytes = (size_t)b->n_inst * b->n_out * sizeof(waa_level_stats);
  if (int e = xfer_d2h(b, out, bytes, d.rows, bytes, bytes, 1)) return e;
  HIP_TRY(hipStreamSynchronize(b->stream));
  return WAA_OK;
}

waa_status waa_output_level_series(waa_batch* b, float* peak, double* sum_sq) {
  if (!b || (!peak && !sum_sq)) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch / both destinations null");
  if (int e = check_rendered(b)) return e;
  if (b->length == 0 || b->n_inst == 0 || b->n_out == 0) return WAA_OK;
  if (int e = wait_for_render(b)) return e;
  waa::LevelsDesc d{};
  if (int e = run_levels(b, &d)) return e;
  const size_t count = (size_t)b->n_inst * b->n_out * b->n_quanta;
  if (peak)
    if (int e = xfer_d2h(b, peak, count * sizeof(float), d.q_peak, count * sizeof(float), count * sizeof(float), 1)) return e;
  if (sum_sq)
    if (int e = xfer_d2h(b, sum_sq, count * sizeof(double), d.q_sum_sq, count * sizeof(double), count * sizeof(double), 1)) return e;
  HIP_TRY(hipStreamSynchronize(b->stream));
  return WAA_OK;
}

waa_status waa_download_all_pcm16_gain(waa_batch* b, int16_t* dst, const float* gain) {
  if (!b || !dst || !gain) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch / destination / gains");
  if (int e = check_rendered(b)) return e;
  for (uint32_t i = 0; i < b->n_inst; i++)
    if (!std::isfinite(gain[i])) return fail(WAA_ERR_INVALID_ARGUMENT, "the gain of instance %u is not finite (%g)", i, (double)gain[i]);
  if (b->length == 0 || b->n_inst == 0 || b->n_out == 0) return WAA_OK;
  if (int e = wait_for_render(b)) return e;
  const size_t count = (size_t)b->n_inst * b->length * b->n_out;
  if (!b->pcm_out) {  // (shared with waa_download_all_pcm16)
    if (int e = dev_alloc(b, &b->pcm_out, count, true)) return e;
    b->pcm_out_count = count;
  }
  if (!b->pcm_gain)
    if (int e = dev_alloc(b, &b->pcm_gain, b->n_inst)) return e;
  const size_t gbytes = (size_t)b->n_inst * sizeof(float);
  if (int e = xfer_h2d(b, b->pcm_gain, gbytes, gain, gbytes, gbytes, 1)) return e;
  const waa::SignalRef& s = b->nodes[0].sig;
  waa::EncodeGainDesc d{};
  d.e.in = s.base;
  d.e.pcm = b->pcm_out;
  d.e.frames = b->length;
  d.e.in_item_stride = s.inst_stride;
  d.e.in_ch_stride = s.ch_stride;
  d.e.nch_in = s.base ? (uint32_t)s.nch : 0u;
  d.e.nch_out = b->n_out;
  d.e.n_items = b->n_inst;
  d.gain = b->pcm_gain;
  if (int e = call_launch(b, "pcm16_pack_gain_kernel", [&] { waa::launch_pcm16_pack_gain(d, b->stream); })) return e;
  if (int e = xfer_d2h(b, dst, count * sizeof(int16_t), b->pcm_out, count * sizeof(int16_t), count * sizeof(int16_t), 1)) return e;
  HIP_TRY(hipStreamSynchronize(b->stream));
  return WAA_OK;
}

}  // extern "C"
