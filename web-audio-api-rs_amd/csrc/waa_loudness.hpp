// waa_loudness.hpp — what waa_loudness.hip and waa_loudness_host.cpp share: the descriptor of the three launches behind
// waa_output_loudness / waa_output_loudness_series (include/waa_hip_device.h).  A header of its own, so that a change
// here rebuilds those two files and nothing else.
#pragma once
#include <cstdint>

namespace waa {

// A row is one (item, output channel); a channel >= nch_in is a row of zeros.  A LANE is one (row, sub-block j) of `hop` frames:
// lane g = row * n_sub + j.  The state of the cascade is (p1, p2, q1, q2): the shelf's and the high-pass's two values each.
struct LoudnessDesc {
  const float* in;           // planes: in[item * in_item_stride + ch * in_ch_stride + frame]
  uint64_t in_item_stride, in_ch_stride;
  uint32_t nch_in, nch_out, n_items;
  uint32_t hop, n_sub, pad;  // frames per sub-block; whole sub-blocks per row
  double b0, b1, b2, a1, a2; // the shelf
  double c1, c2;             // the high-pass's a1, a2 (its b is 1, -2, 1)
  double m[16];              // M^h, row-major: the state after `hop` frames of zero input, m[r * 4 + c] from unit state c
  double* end_state;         // [lanes][4] E[j]: the state after sub-block j from zero state
  double* start_state;       // [lanes][4] S[j]: the state in front of sub-block j
  double* z;                 // [rows][n_sub] the sub-block energies
};
void launch_loudness_state(const LoudnessDesc& d, void* stream);   // E[j] of every lane
void launch_loudness_chain(const LoudnessDesc& d, void* stream);   // S[j + 1] = M^h S[j] + E[j], one thread per row
void launch_loudness_energy(const LoudnessDesc& d, void* stream);  // z[j] of every lane, from S[j]

}  // namespace waa
