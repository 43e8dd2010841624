// waa_analyser_common.hpp — what the AnalyserNode kernels share (waa_conv.hip: one pull per render; waa_analyser_series.hip: a
// series of pulls): the complex helpers, the in-place radix-4 transform in LDS and the mono down-mix of the analyser's input.
#pragma once
#include <hip/hip_runtime.h>

#include "waa_internal.hpp"

namespace waa {
namespace {

__device__ __forceinline__ Cplx cmul(Cplx a, Cplx b) {
  Cplx r;
  r.re = __builtin_fmaf(a.re, b.re, -(a.im * b.im));
  r.im = __builtin_fmaf(a.re, b.im, a.im * b.re);
  return r;
}
__device__ __forceinline__ Cplx cadd(Cplx a, Cplx b) { return Cplx{a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ Cplx csub(Cplx a, Cplx b) { return Cplx{a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ Cplx mul_negi(Cplx a) { return Cplx{a.im, -a.re}; }  // a * (-i)
__device__ __forceinline__ Cplx mul_posi(Cplx a) { return Cplx{-a.im, a.re}; }  // a * (+i)
__device__ __forceinline__ Cplx conj(Cplx a) { return Cplx{a.re, -a.im}; }

// in-place radix-4 decimation-in-frequency FFT: natural order in, bit-reversed order out. n = 4^m.
// n = 4^m or 2 * 4^m (a trailing radix-2 stage on adjacent pairs)
__device__ __forceinline__ void fft_dif(Cplx* a, const Cplx* tw, int n, int tid, int nthreads) {
  int L = n;
  for (; L >= 4; L >>= 2) {
    const int q = L >> 2;
    const int tstep = n / (4 * q);
    for (int b = tid; b < (n >> 2); b += nthreads) {
      const int j = b % q, base = (b / q) * 4 * q + j;
      const Cplx x0 = a[base], x1 = a[base + q], x2 = a[base + 2 * q], x3 = a[base + 3 * q];
      const Cplx s02 = cadd(x0, x2), d02 = csub(x0, x2), s13 = cadd(x1, x3), d13 = mul_negi(csub(x1, x3));
      const Cplx w1 = tw[j * tstep];
      const Cplx w2 = cmul(w1, w1), w3 = cmul(w2, w1);
      a[base] = cadd(s02, s13);
      a[base + q] = cmul(csub(s02, s13), w2);
      a[base + 2 * q] = cmul(cadd(d02, d13), w1);
      a[base + 3 * q] = cmul(csub(d02, d13), w3);
    }
    __syncthreads();
  }
  if (L == 2) {
    for (int b = tid; b < (n >> 1); b += nthreads) {
      const Cplx u = a[2 * b], v = a[2 * b + 1];
      a[2 * b] = cadd(u, v);
      a[2 * b + 1] = csub(u, v);
    }
    __syncthreads();
  }
}

// mono down-mix of frame f >= 0 of the analyser's input (analyser.rs:277-280, quantum.rs:387-432).  Dynamic-count plans: the
// count of this frame's quantum (`code`: count | silent, per instance and quantum); null: the signal's static width.
__device__ __forceinline__ float analyser_mono(const SignalRef& sig, const uint8_t* code, uint64_t code_stride, uint32_t inst, int64_t f) {
  const float* p0 = sig.base + (uint64_t)inst * sig.inst_stride;
  const uint64_t cs = sig.ch_stride;
  int nch = sig.nch;
  if (code) {
    const uint32_t c = code[(uint64_t)inst * code_stride + (uint64_t)(f >> 7)];
    nch = (c & 0x80u) ? 0 : (int)(c & 63u);
  }
  switch (nch) {  // quantum.rs:387-429 speaker down-mix to mono
    case 0: return 0.f;  // (a silent quantum)
    case 1: return p0[f];
    case 2: return 0.5f * (p0[f] + p0[cs + f]);
    case 4: return 0.25f * (p0[f] + p0[cs + f] + p0[2 * cs + f] + p0[3 * cs + f]);
    case 6:
      return __builtin_fmaf(0.70710678118654752440f, p0[f] + p0[cs + f],
                            __builtin_fmaf(0.5f, p0[4 * cs + f] + p0[5 * cs + f], p0[2 * cs + f]));
    default: return p0[f];  // other layouts: truncate
  }
}

// |X[k]| / N of the real transform whose packed half-size complex transform (z[n] = x[2n] + i x[2n+1], fft_dif's bit-reversed
// order) lies in `a`: M = N / 2 bins, lg = log2(M), tw_full[k] = exp(-2 pi i k / N), nf = 1 / N (analysis.rs:335-341)
__device__ __forceinline__ float analyser_bin_norm(const Cplx* a, const Cplx* tw_full, int k, int M, int lg, float nf) {
  const int k2 = (M - k) & (M - 1);
  const Cplx z = a[__brev((unsigned)k) >> (32 - lg)];
  const Cplx zc = conj(a[__brev((unsigned)k2) >> (32 - lg)]);
  const Cplx e = Cplx{0.5f * (z.re + zc.re), 0.5f * (z.im + zc.im)};
  const Cplx o = mul_negi(Cplx{0.5f * (z.re - zc.re), 0.5f * (z.im - zc.im)});
  const Cplx w = tw_full[k];
  const Cplx x = cadd(e, cmul(o, w));
  return hypotf(x.re, x.im) * nf;
}
// analysis.rs:388-400 (bscale = 255 / (max_db - min_db); a NaN becomes 0 as Rust's `as u8` makes it)
__device__ __forceinline__ uint8_t analyser_byte(float db, float min_db, float bscale) {
  const float scaled = bscale * (db - min_db);
  const float clamped = scaled < 0.f ? 0.f : scaled > 255.f ? 255.f : scaled;
  return isnan(scaled) ? (uint8_t)0 : (uint8_t)clamped;
}

}  // namespace
}  // namespace waa
