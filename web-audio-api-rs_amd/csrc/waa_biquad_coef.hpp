// waa_biquad_coef.hpp — one element of the per-frame Biquad coefficient table of a-rate params (biquad_filter.rs:837-855): the
// body of biquad_coef_kernel (waa_kernels.hip, one filter type per node) and of biquad_coef_inst_kernel (waa_biquad_coef_inst.hip,
// one type per instance).  Both evaluate this one function, so a context's coefficients do not depend on how its type reached
// the kernel.  Device code only; built like the rest of the library with -ffp-contract=off.
#ifndef WAA_BIQUAD_COEF_HPP
#define WAA_BIQUAD_COEF_HPP

#include <hip/hip_runtime.h>

#include "waa_internal.hpp"
#include "waa_param.hpp"

namespace waa {

// ---- per-frame biquad coefficients (biquad_filter.rs:28-373 calculate_coefs, get_computed_freq) in f64 ----
__device__ __forceinline__ void norm_coefs(double b0, double b1, double b2, double a0, double a1, double a2, double* o) {
  const double s = 1. / a0;
  o[0] = b0 * s;
  o[1] = b1 * s;
  o[2] = b2 * s;
  o[3] = a1 * s;
  o[4] = a2 * s;
}
__device__ __forceinline__ void raw_coefs(double b0, double* o) {
  o[0] = b0;
  o[1] = o[2] = o[3] = o[4] = 0.;
}
// One element of the table: row `idx / frames_padded`, frame slot `idx % frames_padded`, filter type `type`.
__device__ __forceinline__ void biquad_coef_element(const BiquadCoefDesc& d, uint64_t idx, int type) {
  const uint32_t inst = (uint32_t)(idx / d.frames_padded);
  const uint64_t r = idx % d.frames_padded;
  uint64_t frame = r, slot = r * 5, cstep = 1;
  if (d.lane_major) {
    // a wave covers the 64 lanes of one (tile, k): the streaming kernel's lane l owns frames tile*2048 + l*32 + k, and
    // its loads of coefficient c for step k are 64 consecutive doubles
    const uint64_t tile = r / TILE, in = r % TILE, k = in / 64, lane = in % 64;
    frame = tile * TILE + lane * TILE_K + k;
    slot = ((tile * TILE_K + k) * 5) * 64 + lane;
    cstep = 64;
  }
  if (frame >= d.n_frames) frame = d.n_frames - 1;  // padded tail of the last tile: any finite set will do
  const uint32_t q = (uint32_t)(frame / RQ);
  const float freq = param_at(d.frequency, inst, q, frame), det = param_at(d.detune, inst, q, frame);
  const double Q = (double)param_at(d.q, inst, q, frame), gain = (double)param_at(d.gain, inst, q, frame);
  const float cf = det != 0.f ? freq * exp2f(det / 1200.f) : freq;  // get_computed_freq: f32
  const double PI = 3.14159265358979323846;
  const double nyq = (double)d.sample_rate / 2.;
  double f = (double)cf / nyq;
  f = f < 0. ? 0. : f > 1. ? 1. : f;
  double o[5];
  const double A = pow(10., gain / 40.);
  const double w0 = PI * f, sw = sin(w0), cw = cos(w0);
  switch (type) {
    case 0: {  // lowpass
      if (f == 1.) { raw_coefs(1., o); break; }
      const double al = sw / (2. * pow(10., Q / 20.)), be = (1. - cw) / 2.;
      norm_coefs(be, 2. * be, be, 1. + al, -2. * cw, 1. - al, o);
      break;
    }
    case 1: {  // highpass
      if (f == 1.) { raw_coefs(0., o); break; }
      if (f == 0.) { raw_coefs(1., o); break; }
      const double al = sw / (2. * pow(10., Q / 20.)), be = (1. + cw) / 2.;
      norm_coefs(be, -2. * be, be, 1. + al, -2. * cw, 1. - al, o);
      break;
    }
    case 2: {  // bandpass
      if (!(f > 0. && f < 1.)) { raw_coefs(0., o); break; }
      if (!(Q > 0.)) { raw_coefs(1., o); break; }
      const double al = sw / (2. * Q);
      norm_coefs(al, 0., -al, 1. + al, -2. * cw, 1. - al, o);
      break;
    }
    case 3: {  // notch
      if (!(f > 0. && f < 1.)) { raw_coefs(1., o); break; }
      if (!(Q > 0.)) { raw_coefs(0., o); break; }
      const double al = sw / (2. * Q);
      norm_coefs(1., -2. * cw, 1., 1. + al, -2. * cw, 1. - al, o);
      break;
    }
    case 4: {  // allpass
      if (!(f > 0. && f < 1.)) { raw_coefs(1., o); break; }
      if (!(Q > 0.)) { raw_coefs(-1., o); break; }
      const double al = sw / (2. * Q);
      norm_coefs(1. - al, -2. * cw, 1. + al, 1. + al, -2. * cw, 1. - al, o);
      break;
    }
    case 5: {  // peaking
      if (!(f > 0. && f < 1.)) { raw_coefs(1., o); break; }
      if (!(Q > 0.)) { raw_coefs(A * A, o); break; }
      const double al = sw / (2. * Q);
      norm_coefs(1. + al * A, -2. * cw, 1. - al * A, 1. + al / A, -2. * cw, 1. - al / A, o);
      break;
    }
    case 6: {  // lowshelf
      if (f == 1.) { raw_coefs(A * A, o); break; }
      if (f == 0.) { raw_coefs(1., o); break; }
      const double as = sw / 2. * 1.41421356237309504880, k = 2. * as * sqrt(A), ap = A + 1., am = A - 1.;
      norm_coefs(A * (ap - am * cw + k), 2. * A * (am - ap * cw), A * (ap - am * cw - k), ap + am * cw + k,
                 -2. * (am + ap * cw), ap + am * cw - k, o);
      break;
    }
    default: {  // highshelf
      if (f == 1.) { raw_coefs(1., o); break; }
      if (!(f > 0.)) { raw_coefs(A * A, o); break; }
      const double as = sw / 2. * 1.41421356237309504880, k = 2. * as * sqrt(A), ap = A + 1., am = A - 1.;
      norm_coefs(A * (ap + am * cw + k), -2. * A * (am + ap * cw), A * (ap + am * cw - k), ap - am * cw + k,
                 2. * (am - ap * cw), ap - am * cw - k, o);
      break;
    }
  }
  double* out = d.coefs + (uint64_t)inst * d.frames_padded * 5 + slot;
#pragma unroll
  for (int c = 0; c < 5; c++) out[(uint64_t)c * cstep] = o[c];
}

}  // namespace waa

#endif  // WAA_BIQUAD_COEF_HPP
