// waa_loudness.hip — the K-weighted sub-block energies behind waa_output_loudness and waa_output_loudness_series (the definitions:
// include/waa_hip_device.h).  An extension like the levels pass of waa_levels.hip: it reads the destination's signal
// where the render left it.  Nothing here is a plan step.
//
// The K-weighting is a recursive filter — two biquads in f64 — over the whole row, and a row's sub-block energies are sums over its
// output.  It is made parallel over time in the way of waa_biquad_lanes.hip, with constant coefficients: one LANE per (row,
// sub-block of `hop` frames), the lanes of all rows flattened onto the grid, so that a batch of many short clips fills its
// wavefronts as a batch of few long ones does.
//   loudness_state_kernel   the cascade from ZERO state over the lane's sub-block; stores the end state E[j] (four doubles)
//   loudness_chain_kernel   one thread per row: S[0] = 0, S[j + 1] = M^h S[j] + E[j], ascending — the cascade is linear, so the
//                           state after a sub-block is the zero-input answer to its start state plus the zero-state answer to its
//                           samples.  M^h (4 x 4) comes from the host.
//   loudness_energy_kernel  the cascade again from S[j], z[j] = (...((0 + w_0^2) + w_1^2) + ...)
// A lane's arithmetic is the definition's serial recurrence and nothing else: no value depends on the lane's place in the grid or on
// the shape of its loads, so a row gives the same bits whatever its batch.  The coefficients arrive in the kernel's arguments and
// stay in scalar registers.
//
// Loads: a lane walks its own sub-block, 16 bytes at a time, the next load in flight while it works on this one.  Neighbouring lanes
// are `hop` frames apart, so a wavefront's load touches 64 cache lines and each line serves eight consecutive loads of its lane from
// the cache.  A row may start on any 4-byte boundary and `hop` may be odd: a lane takes single frames up to its first 16-byte
// boundary and behind its last whole one.  Nothing behind frame n_sub * hop - 1 of a row is read.
#include <hip/hip_runtime.h>

#include "waa_internal.hpp"
#include "waa_loudness.hpp"

namespace waa {

namespace {
// one wavefront per workgroup: the lanes share nothing, and a grid of small workgroups ends evenly (a lane runs for `hop` frames)
constexpr uint32_t LANE_BLOCK = 64;
struct KState {
  double p1, p2, q1, q2;
};
// one frame through both stages, transposed direct form II, unfused (the build never contracts); returns w.  The sample is decided
// on its bits as in the levels pass: e == 255 and e == 0 enter as +0.0.  The high-pass's b = (1, -2, 1): 1 * v is v and -2 * v is
// exact, the same bits as the general form.
__device__ __forceinline__ double k_step(const LoudnessDesc& d, KState& s, float xf) {
  const uint32_t e = (__float_as_uint(xf) & 0x7fffffffu) >> 23;
  const double x = e >= 1u && e <= 254u ? (double)xf : 0.0;
  const double v = d.b0 * x + s.p1;
  s.p1 = (d.b1 * x - d.a1 * v) + s.p2;
  s.p2 = d.b2 * x - d.a2 * v;
  const double w = v + s.q1;
  s.q1 = (-2.0 * v - d.c1 * w) + s.q2;
  s.q2 = v - d.c2 * w;
  return w;
}
// the lane's `hop` frames at src, in order; ENERGY: returns the sum of w^2
template <bool ENERGY>
__device__ __forceinline__ double k_block(const LoudnessDesc& d, KState& s, const float* src) {
  double z = 0.0;
  const uint32_t hop = d.hop;
  uint32_t i = 0;
  auto one = [&](float xf) {
    const double w = k_step(d, s, xf);
    if (ENERGY) z = z + w * w;
  };
  // single frames up to the first 16-byte boundary (at most three)
  const uint32_t mis = (uint32_t)((reinterpret_cast<uintptr_t>(src) >> 2) & 3u);
  const uint32_t head = mis ? (4u - mis < hop ? 4u - mis : hop) : 0u;
  for (; i < head; i++) one(load_global(src + i));
  const uint32_t n4 = (hop - i) >> 2;
  if (n4) {
    f4v cur = load_global_f4(src + i);
#pragma unroll 1
    for (uint32_t t = 0; t < n4; t++) {
      // (the last round loads its own four frames again rather than anything behind them)
      const f4v nxt = load_global_f4(src + i + (t + 1 < n4 ? 4u : 0u));
      one(cur.x);
      one(cur.y);
      one(cur.z);
      one(cur.w);
      cur = nxt;
      i += 4;
    }
  }
  for (; i < hop; i++) one(load_global(src + i));
  return z;
}
__device__ __forceinline__ const float* lane_source(const LoudnessDesc& d, uint64_t g, bool* carried) {
  const uint64_t row = g / d.n_sub, j = g - row * d.n_sub;
  const uint64_t item = row / d.nch_out, c = row - item * d.nch_out;
  *carried = c < d.nch_in;
  return d.in + item * d.in_item_stride + c * d.in_ch_stride + j * d.hop;
}
}  // namespace

__global__ __launch_bounds__(LANE_BLOCK) void loudness_state_kernel(const LoudnessDesc d) {
  const uint64_t lanes = (uint64_t)d.n_items * d.nch_out * d.n_sub;
  for (uint64_t g = (uint64_t)blockIdx.x * LANE_BLOCK + threadIdx.x; g < lanes; g += (uint64_t)gridDim.x * LANE_BLOCK) {
    if (g % d.n_sub == d.n_sub - 1u) continue;  // (nothing follows a row's last sub-block: its end state is never read)
    bool carried;
    const float* src = lane_source(d, g, &carried);
    KState s = {0.0, 0.0, 0.0, 0.0};
    if (carried) k_block<false>(d, s, src);  // (a row of zeros from zero state ends in zero state)
    double* e = d.end_state + g * 4;
    store_global(e, s.p1);
    store_global(e + 1, s.p2);
    store_global(e + 2, s.q1);
    store_global(e + 3, s.q2);
  }
}

__global__ __launch_bounds__(256) void loudness_chain_kernel(const LoudnessDesc d) {
  const uint64_t row = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= (uint64_t)d.n_items * d.nch_out) return;
  const double* e = d.end_state + row * d.n_sub * 4;
  double* st = d.start_state + row * d.n_sub * 4;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (uint32_t j = 0; j < d.n_sub; j++) {  // ascending and sequential
    double n[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
      store_global(st + (uint64_t)j * 4 + r, s[r]);
      n[r] = 0.0;
    }
    if (j + 1 == d.n_sub) break;
#pragma unroll
    for (int r = 0; r < 4; r++)
      n[r] = (((d.m[r * 4] * s[0] + d.m[r * 4 + 1] * s[1]) + d.m[r * 4 + 2] * s[2]) + d.m[r * 4 + 3] * s[3]) + load_global(e + (uint64_t)j * 4 + r);
#pragma unroll
    for (int r = 0; r < 4; r++) s[r] = n[r];
  }
}

__global__ __launch_bounds__(LANE_BLOCK) void loudness_energy_kernel(const LoudnessDesc d) {
  const uint64_t lanes = (uint64_t)d.n_items * d.nch_out * d.n_sub;
  for (uint64_t g = (uint64_t)blockIdx.x * LANE_BLOCK + threadIdx.x; g < lanes; g += (uint64_t)gridDim.x * LANE_BLOCK) {
    bool carried;
    const float* src = lane_source(d, g, &carried);
    double z = 0.0;
    if (carried) {  // (a row of zeros: its states are zeros and so is its energy)
      const double* st = d.start_state + g * 4;
      KState s = {load_global(st), load_global(st + 1), load_global(st + 2), load_global(st + 3)};
      z = k_block<true>(d, s, src);
    }
    store_global(d.z + g, z);
  }
}

namespace {
unsigned lane_blocks(uint64_t lanes) {
  const uint64_t blocks = (lanes + LANE_BLOCK - 1) / LANE_BLOCK;
  return (unsigned)(blocks < 0x7fffffffull ? blocks : 0x7fffffffull);  // (more lanes than that: strides of the grid)
}
}  // namespace
void launch_loudness_state(const LoudnessDesc& d, void* stream) {
  const uint64_t lanes = (uint64_t)d.n_items * d.nch_out * d.n_sub;
  if (lanes == 0) return;
  hipLaunchKernelGGL(loudness_state_kernel, dim3(lane_blocks(lanes)), dim3(LANE_BLOCK), 0, (hipStream_t)stream, d);
}
void launch_loudness_chain(const LoudnessDesc& d, void* stream) {
  const uint64_t rows = (uint64_t)d.n_items * d.nch_out;
  if (rows == 0 || d.n_sub == 0) return;
  hipLaunchKernelGGL(loudness_chain_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d);
}
void launch_loudness_energy(const LoudnessDesc& d, void* stream) {
  const uint64_t lanes = (uint64_t)d.n_items * d.nch_out * d.n_sub;
  if (lanes == 0) return;
  hipLaunchKernelGGL(loudness_energy_kernel, dim3(lane_blocks(lanes)), dim3(LANE_BLOCK), 0, (hipStream_t)stream, d);
}

}  // namespace waa
