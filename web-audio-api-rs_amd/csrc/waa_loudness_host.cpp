// waa_loudness_host.cpp — the host side of waa_output_loudness, waa_output_loudness_series, waa_loudness_hop and
// waa_loudness_from_series (include/waa_hip_device.h; the kernels: waa_loudness.hip).  An extension like the levels
// calls of waa_levels_host.cpp, whose refusals, wait and launches it shares (waa_output_calls.hpp): it reads the destination's signal
// where the render left it and is no plan step.  The device computes the sub-block energies z; blocks, gates and the logarithms are
// host work on n_sub doubles per row — the same code whether z comes from the device or from a caller.
#include <cmath>
#include <cstddef>
#include <limits>
#include <vector>

#include "../../include/waa_hip_device.h"
#include "waa_host.hpp"
#include "waa_loudness.hpp"
#include "waa_output_calls.hpp"

static_assert(sizeof(waa_loudness_stats) == 40 && offsetof(waa_loudness_stats, n_blocks) == 32 && offsetof(waa_loudness_stats, n_gated) == 36,
              "one 40-byte record per instance");

namespace {

constexpr double NEG_INF = -std::numeric_limits<double>::infinity();
constexpr double PI = 3.14159265358979323846;

uint32_t hop_of(double sr) { return sr > 0 && sr < 4e10 ? (uint32_t)std::floor(sr / 10.0 + 0.5) : 0u; }

// the two biquads of the K-weighting at `sr`, in f64, as the header writes them
void k_coefficients(double sr, waa::LoudnessDesc* d) {
  {
    const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
    const double K = std::tan(PI * f0 / sr), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
    const double a0 = 1.0 + K / Q + K * K;
    d->b0 = (Vh + Vb * K / Q + K * K) / a0;
    d->b1 = 2.0 * (K * K - Vh) / a0;
    d->b2 = (Vh - Vb * K / Q + K * K) / a0;
    d->a1 = 2.0 * (K * K - 1.0) / a0;
    d->a2 = (1.0 - K / Q + K * K) / a0;
  }
  {
    const double f0 = 38.13547087602444, Q = 0.5003270373238773;
    const double K = std::tan(PI * f0 / sr), a0 = 1.0 + K / Q + K * K;
    d->c1 = 2.0 * (K * K - 1.0) / a0;
    d->c2 = (1.0 - K / Q + K * K) / a0;
  }
}
// M^h: the state (p1, p2, q1, q2) after `hop` frames of zero input from each unit state, by the kernels' own recurrence
// (this file is built without contraction, like them)
void k_transition(waa::LoudnessDesc* d) {
  for (int c = 0; c < 4; c++) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    s[c] = 1.0;
    for (uint32_t i = 0; i < d->hop; i++) {
      const double x = 0.0;
      const double v = d->b0 * x + s[0];
      s[0] = (d->b1 * x - d->a1 * v) + s[1];
      s[1] = d->b2 * x - d->a2 * v;
      const double w = v + s[2];
      s[2] = (-2.0 * v - d->c1 * w) + s[3];
      s[3] = v - d->c2 * w;
    }
    for (int r = 0; r < 4; r++) d->m[r * 4 + c] = s[r];
  }
}

// the caller's weights, or the Web Audio layouts' (5.1: L R C LFE SL SR; quad: L R SL SR)
int channel_weights(const double* weights, uint32_t nch, std::vector<double>* g) {
  g->assign(nch, 1.0);
  if (weights) {
    for (uint32_t c = 0; c < nch; c++) {
      if (!std::isfinite(weights[c]) || weights[c] < 0.0)
        return fail(WAA_ERR_INVALID_ARGUMENT, "the weight of channel %u is negative or not finite (%g)", c, weights[c]);
      (*g)[c] = weights[c];
    }
  } else if (nch == 6) {
    *g = {1.0, 1.0, 1.0, 0.0, 1.41, 1.41};
  } else if (nch == 4) {
    *g = {1.0, 1.0, 1.41, 1.41};
  }
  return 0;
}
double lufs(double p) { return p > 0.0 ? -0.691 + 10.0 * std::log10(p) : NEG_INF; }
// P of the window of `n` sub-blocks at k: sum_c G_c (z_c[k] + ... + z_c[k + n - 1]) / (n h), every sum ascending
double window_power(const double* z, uint32_t nch, uint32_t n_sub, const double* g, uint32_t k, uint32_t n, uint32_t hop) {
  double p = 0.0;
  for (uint32_t c = 0; c < nch; c++) {
    const double* zc = z + (size_t)c * n_sub + k;
    double s = zc[0];
    for (uint32_t i = 1; i < n; i++) s = s + zc[i];
    p = p + g[c] * s;
  }
  return p / ((double)n * (double)hop);
}
// blocks, both gates and the maxima of one context from its sub-block energies z[nch][n_sub]
void gate(const double* z, uint32_t nch, uint32_t n_sub, uint32_t hop, const double* g, waa_loudness_stats* out) {
  waa_loudness_stats r;
  r.integrated = r.momentary_max = r.short_term_max = r.relative_threshold = NEG_INF;
  r.n_blocks = n_sub >= 4 ? n_sub - 3 : 0;
  r.n_gated = 0;
  std::vector<double> p(r.n_blocks), l(r.n_blocks);
  double sum_a = 0.0;
  uint32_t n_a = 0;
  for (uint32_t k = 0; k < r.n_blocks; k++) {
    p[k] = window_power(z, nch, n_sub, g, k, 4, hop);
    l[k] = lufs(p[k]);
    if (l[k] > r.momentary_max) r.momentary_max = l[k];
    if (l[k] > -70.0) sum_a = sum_a + p[k], n_a++;
  }
  if (n_a) {
    r.relative_threshold = lufs(sum_a / (double)n_a) - 10.0;
    double sum_b = 0.0;
    for (uint32_t k = 0; k < r.n_blocks; k++)
      if (l[k] > -70.0 && l[k] > r.relative_threshold) sum_b = sum_b + p[k], r.n_gated++;
    if (r.n_gated) r.integrated = lufs(sum_b / (double)r.n_gated);
  }
  for (uint32_t k = 0; k + 30 <= n_sub; k++) {
    const double s = lufs(window_power(z, nch, n_sub, g, k, 30, hop));
    if (s > r.short_term_max) r.short_term_max = s;
  }
  *out = r;
}

// the three launches over the destination's signal; *out describes where z lies in the batch's workspace.  n_sub >= 1.
int run_loudness(waa_batch* b, uint32_t hop, uint32_t n_sub, waa::LoudnessDesc* out) {
  const uint64_t rows = (uint64_t)b->n_inst * b->n_out, lanes = rows * n_sub;
  if (!b->loudness_ws) {  // (the batch's size never changes): 4 + 4 + 1 doubles per lane
    double* p = nullptr;
    if (int e = dev_alloc(b, &p, lanes * 9)) return e;
    b->loudness_ws = p;
  }
  double* ws = static_cast<double*>(b->loudness_ws);
  const waa::SignalRef& s = b->nodes[0].sig;
  waa::LoudnessDesc d{};
  d.in = s.base;
  d.in_item_stride = s.inst_stride;
  d.in_ch_stride = s.ch_stride;
  d.nch_in = s.base ? (uint32_t)s.nch : 0u;  // (no signal at all: every row is zeros)
  d.nch_out = b->n_out;
  d.n_items = b->n_inst;
  d.hop = hop;
  d.n_sub = n_sub;
  k_coefficients((double)b->sr, &d);
  k_transition(&d);
  d.end_state = ws;
  d.start_state = ws + lanes * 4;
  d.z = ws + lanes * 8;
  if (int e = call_launch(b, "loudness_state_kernel", [&] { waa::launch_loudness_state(d, b->stream); })) return e;
  if (int e = call_launch(b, "loudness_chain_kernel", [&] { waa::launch_loudness_chain(d, b->stream); })) return e;
  if (int e = call_launch(b, "loudness_energy_kernel", [&] { waa::launch_loudness_energy(d, b->stream); })) return e;
  *out = d;
  return 0;
}

}  // namespace

extern "C" {

uint32_t waa_loudness_hop(double sample_rate) { return hop_of(sample_rate); }

waa_status waa_loudness_from_series(const double* z, uint32_t n_channels, uint32_t n_sub, uint32_t hop, const double* weights,
                                    waa_loudness_stats* out) {
  if (!out || (!z && n_channels && n_sub)) return fail(WAA_ERR_INVALID_ARGUMENT, "null series / destination");
  if (hop == 0) return fail(WAA_ERR_INVALID_ARGUMENT, "a sub-block of no frames");
  std::vector<double> g;
  if (int e = channel_weights(weights, n_channels, &g)) return e;
  gate(z, n_channels, n_sub, hop, g.data(), out);
  return WAA_OK;
}

waa_status waa_output_loudness(waa_batch* b, const double* weights, waa_loudness_stats* out) {
  if (!b || !out) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch / destination");
  if (int e = check_rendered(b)) return e;
  std::vector<double> g;
  if (int e = channel_weights(weights, b->n_out, &g)) return e;
  const uint32_t hop = hop_of((double)b->sr);
  const uint64_t n_sub64 = hop ? b->length / hop : 0;
  if (n_sub64 > 0xffffffffull) return fail(WAA_ERR_INVALID_ARGUMENT, "more than 2^32 sub-blocks per row");
  const uint32_t n_sub = (uint32_t)n_sub64;
  if (n_sub == 0 || b->n_out == 0) {  // (shorter than one sub-block: there is nothing to measure)
    for (uint32_t i = 0; i < b->n_inst; i++) gate(nullptr, 0, 0, hop ? hop : 1, g.data(), out + i);
    return WAA_OK;
  }
  if (b->n_inst == 0) return WAA_OK;
  if (int e = wait_for_render(b)) return e;
  waa::LoudnessDesc d{};
  if (int e = run_loudness(b, hop, n_sub, &d)) return e;
  const size_t per = (size_t)b->n_out * n_sub;
  std::vector<double> z((size_t)b->n_inst * per);
  const size_t bytes = z.size() * sizeof(double);
  if (int e = xfer_d2h(b, z.data(), bytes, d.z, bytes, bytes, 1)) return e;
  HIP_TRY(hipStreamSynchronize(b->stream));
  for (uint32_t i = 0; i < b->n_inst; i++) gate(z.data() + i * per, b->n_out, n_sub, hop, g.data(), out + i);
  return WAA_OK;
}

waa_status waa_output_loudness_series(waa_batch* b, double* z) {
  if (!b || !z) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch / destination");
  if (int e = check_rendered(b)) return e;
  const uint32_t hop = hop_of((double)b->sr);
  const uint64_t n_sub64 = hop ? b->length / hop : 0;
  if (n_sub64 > 0xffffffffull) return fail(WAA_ERR_INVALID_ARGUMENT, "more than 2^32 sub-blocks per row");
  if (n_sub64 == 0 || b->n_inst == 0 || b->n_out == 0) return WAA_OK;
  if (int e = wait_for_render(b)) return e;
  waa::LoudnessDesc d{};
  if (int e = run_loudness(b, hop, (uint32_t)n_sub64, &d)) return e;
  const size_t bytes = (size_t)b->n_inst * b->n_out * n_sub64 * sizeof(double);
  if (int e = xfer_d2h(b, z, bytes, d.z, bytes, bytes, 1)) return e;
  HIP_TRY(hipStreamSynchronize(b->stream));
  return WAA_OK;
}

}  // extern "C"
