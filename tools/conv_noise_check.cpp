// conv_noise_check.cpp — csrc/waa_conv_noise.hpp on the CPU (tests/test_conv_noise.py): a C entry point over the automaton, so that
// the test can hold it against the oracle's restated FFTConvolver (oracle/waa_oracle.c::orc_fftconvolver_run) on the same inputs.
//   g++ -O2 -std=c++17 -shared -fPIC -o conv_noise_check.so tools/conv_noise_check.cpp
#include <cmath>
#include <cstdint>

#include "../web-audio-api-rs_amd/csrc/waa_conv_noise.hpp"

extern "C" {
// the planner's part (waa_plan_dyn.cpp::conv_noise_segments): segments of the trimmed response and which of them hold a tap
void cn_describe(const float* h, uint64_t len, uint32_t* seg_count, uint64_t* seg_mask) {
  uint64_t l = len;
  while (l > 0 && std::fabs(h[l - 1]) < 0.000001f) l--;
  const uint64_t blk = 128u * waa::CONV_NOISE_BLOCK_QUANTA;
  *seg_count = (uint32_t)((l + blk - 1) / blk);
  *seg_mask = 0;
  for (uint64_t s = 0; s < *seg_count && s < 64; s++)
    for (uint64_t i = s * blk; i < (l < (s + 1) * blk ? l : (s + 1) * blk); i++)
      if (h[i] != 0.f) {
        *seg_mask |= (uint64_t)1 << s;
        break;
      }
}
// the kernel's part: quanta of input x (n_quanta x 128 frames) -> noisy[q] = the reference's output quantum holds a non-zero sample
void cn_predict(uint32_t seg_count, uint64_t seg_mask, const float* x, uint32_t n_quanta, uint8_t* noisy) {
  waa::ConvNoiseIr ir{seg_count, 0, seg_mask};
  waa::ConvNoiseState s;
  waa::conv_noise_reset(s);
  for (uint32_t q = 0; q < n_quanta; q++) {
    bool nz = false;
    for (int i = 0; i < 128; i++) nz |= x[(uint64_t)q * 128 + i] != 0.f;
    noisy[q] = waa::conv_noise_step(ir, s, nz) ? 1 : 0;
  }
}
// a whole ConvolverNode (the tail counter and the routing around its FFTConvolvers): code[q] = input channels | 0x80 when the input
// quantum is silent, nz[q] = bit c: channel c of it holds a non-zero sample -> out[q] = waa::conv_noise_node_step's answer
void cn_node(int ir_nch, const uint32_t* seg_count, const uint64_t* seg_mask, uint64_t impulse_length, uint32_t n_quanta,
             const uint8_t* code, const uint8_t* nz, uint8_t* out) {
  waa::ConvNoiseIr ir[4];
  for (int k = 0; k < 4; k++) ir[k] = waa::ConvNoiseIr{seg_count[k], 0, seg_mask[k]};
  waa::ConvNoiseNode s;
  waa::conv_noise_node_reset(s);
  for (uint32_t q = 0; q < n_quanta; q++)
    out[q] = (uint8_t)waa::conv_noise_node_step(ir, ir_nch, impulse_length, s, (code[q] & 0x80) != 0, code[q] & 7, nz[q]);
}
float cn_floor() { return waa::CONV_NOISE_FLOOR; }
}
