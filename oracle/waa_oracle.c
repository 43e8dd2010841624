/*
 * waa_oracle.c — CPU ORACLE.  TEST INFRASTRUCTURE ONLY.
 *
 * A plain-C restatement of the reference's (web-audio-api 1.6.0) per-quantum offline render
 * path, written node by node from the reference source; every function cites the
 * reference file:line it follows.  It renders quantum-major, node-at-a-time, one context
 * at a time, exactly like the reference does (src/render/thread.rs:260-302,
 * src/render/graph.rs:490-591) including the dynamic channel counts and the pointer-
 * identity "silent" flag of AudioRenderQuantum (src/render/quantum.rs:89-160).
 *
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load this
 * library; the product (libwaa_hip.so) never links, loads or calls it.
 *
 * PARITY PIN STATUS:
 *   - in-tree arithmetic (biquad, gain, mixing, panners, buffer source, waveshaper,
 *     analyser ring/window, resample, normalisation): pinned by the reference's own
 *     known-answer tests re-typed in tests/test_oracle_kat.py.
 *   - ConvolverNode: the arithmetic lives in the third-party crate fft-convolver "0.3"
 *     (not vendored, no lockfile).  orc restates its published algorithm (HiFi-LoFi
 *     FFTConvolver: uniformly partitioned overlap-add, block 1024, segment 2048) in f32
 *     with its own radix-2 FFT, and offers an exact f64 direct convolution
 *     (orc_convolve_exact) as the mathematical definition.  Pinned by the reference's
 *     convolver tests (<=256 taps); multi-partition behaviour is PARITY UNPINNED by the
 *     reference and anchored on the exact convolution instead.
 *   - AnalyserNode dB values: realfft "3.3" is third-party; pinned only by the loose
 *     reference tests (peak bin, -inf on silence) => "parity unpinned" beyond DFT maths.
 *   - almost::equal/zero (crate almost "0.2", not vendored): restated from its published
 *     behaviour (tolerance sqrt(f64::EPSILON)); edge cases unverifiable here.
 *   - WaveShaper 2x/4x oversampling: the resamplers are rubato "0.16" FftFixedInOut (third
 *     party, not vendored).  orc restates its synchronous FFT resampler (windowed-sinc
 *     anti-alias filter applied in the frequency domain, spectrum zero-padded / truncated,
 *     overlap-add) from the crate's published source as remembered; the reference's tests
 *     only construct such nodes (waveshaper.rs:608-670) => PARITY UNPINNED, the written
 *     definition is DESIGN.md section 3.5.
 *   - HRTF panning: crate hrtf "0.8.1" (third party, not vendored).  orc restates its
 *     published algorithm (HRIR sphere file format, barycentric interpolation of the three
 *     HRIRs of the triangle the direction pierces, linear convolution of the block with the
 *     previous input samples as history, distance gain) with an exact f64 direct
 *     convolution; the reference only asserts "differs from the input, non-zero tail"
 *     (panner.rs:1226-1269) => PARITY UNPINNED, definition in DESIGN.md section 3.6.  That covers
 *     the resampling of the sphere to the context's rate as well (the crate runs one chunk of
 *     rubato's SincFixedIn over every impulse response; here: the band-limited signal evaluated
 *     directly with the same window and cutoff): only at the sphere's own rate (44.1 kHz for
 *     the IRC_1003_C set) are the HRIRs the file's; at every other context rate - 48 kHz included -
 *     they are this definition's, shared by the oracle and the device path, and unpinned against
 *     the crates (include/waa_hip.h says so at waa_hrtf_load_sphere).
 *
 * Exports the same entry points as include/waa_hip.h with the prefix orc_.
 */
#define _GNU_SOURCE
#include <float.h>
#include <math.h>
#include <pthread.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#if defined(__x86_64__)
#include <xmmintrin.h>
#include <pmmintrin.h>
#endif

#include "../include/waa_hip.h"

#define RQ 128
#define ORC_MAXC 32 /* MAX_CHANNELS, src/lib.rs:21 (the speakers mix rules are defined up to 6: everything wider mixes discretely, quantum.rs:296-306) */
#define ORC_MAX_INPUTS 1

static __thread char g_err[512];
static int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}
const char* orc_last_error(void) { return g_err; }
int32_t orc_device_count(void) { return 0; }

/* ------------------------------------------------------------------------------------ */
/* AudioRenderQuantum (src/render/quantum.rs:178-586)                                     */
/* ------------------------------------------------------------------------------------ */
typedef struct {
  int n;                          /* number_of_channels */
  unsigned char silent[ORC_MAXC]; /* Rc::ptr_eq(data, alloc.zeroes) per channel, quantum.rs:109-111 */
  float d[ORC_MAXC][RQ];
} Quantum;

static void q_make_silent(Quantum* q) { /* quantum.rs:511-516 */
  q->n = 1;
  q->silent[0] = 1;
  memset(q->d[0], 0, sizeof q->d[0]);
}
static int q_is_silent(const Quantum* q) { /* quantum.rs:254-256 */
  for (int c = 0; c < q->n; c++)
    if (!q->silent[c]) return 0;
  return 1;
}
static void q_copy_channel(Quantum* dst, int dc, const Quantum* src, int sc) {
  dst->silent[dc] = src->silent[sc];
  memcpy(dst->d[dc], src->d[sc], sizeof dst->d[dc]);
}
static void q_copy(Quantum* dst, const Quantum* src) {
  dst->n = src->n;
  for (int c = 0; c < src->n; c++) q_copy_channel(dst, c, src, c);
}
static void q_silence_channel(Quantum* q, int c) {
  q->silent[c] = 1;
  memset(q->d[c], 0, sizeof q->d[c]);
}
/* quantum.rs:207-222: new channels are clones of channel 0 ("garbage"), excess truncated */
static void q_set_number_of_channels(Quantum* q, int n) {
  for (int c = q->n; c < n; c++) q_copy_channel(q, c, q, 0);
  q->n = n;
}

/* quantum.rs:285-505 mix_inner */
static void q_mix(Quantum* q, int to, int interp) {
  int from = q->n;
  if (from == to) return;
  if (interp == WAA_INTERP_DISCRETE || from > 6 || to > 6) {
    for (int c = from; c < to; c++) q_silence_channel(q, c);
    q->n = to;
    return;
  }
  const float sqrt05 = sqrtf(0.5f);
  if (from == 1 && to == 2) {
    q_copy_channel(q, 1, q, 0);
  } else if (from == 1 && to == 4) {
    q_copy_channel(q, 1, q, 0);
    q_silence_channel(q, 2);
    q_silence_channel(q, 3);
  } else if (from == 1 && to == 6) {
    q_copy_channel(q, 2, q, 0);
    q_silence_channel(q, 0);
    q_silence_channel(q, 1);
    q_silence_channel(q, 3);
    q_silence_channel(q, 4);
    q_silence_channel(q, 5);
  } else if (from == 2 && to == 4) {
    q_silence_channel(q, 2);
    q_silence_channel(q, 3);
  } else if (from == 2 && to == 6) {
    for (int c = 2; c < 6; c++) q_silence_channel(q, c);
  } else if (from == 4 && to == 5) {
    /* L, R, 0, SL, SR */
    q_copy_channel(q, 4, q, 3);
    q_copy_channel(q, 3, q, 2);
    q_silence_channel(q, 2);
  } else if (from == 4 && to == 6) {
    q_copy_channel(q, 4, q, 2);
    q_copy_channel(q, 5, q, 3);
    q_silence_channel(q, 2);
    q_silence_channel(q, 3);
  } else if (from == 2 && to == 1) {
    /* the reference writes through make_mut => channel is no longer "silent" by pointer */
    for (int i = 0; i < RQ; i++) q->d[0][i] = 0.5f * (q->d[0][i] + q->d[1][i]);
    q->silent[0] = 0;
  } else if (from == 4 && to == 1) {
    for (int i = 0; i < RQ; i++) q->d[0][i] = 0.25f * (q->d[0][i] + q->d[1][i] + q->d[2][i] + q->d[3][i]);
    q->silent[0] = 0;
  } else if (from == 6 && to == 1) {
    for (int i = 0; i < RQ; i++)
      q->d[0][i] = fmaf(sqrt05, q->d[0][i] + q->d[1][i], fmaf(0.5f, q->d[4][i] + q->d[5][i], q->d[2][i]));
    q->silent[0] = 0;
  } else if (from == 4 && to == 2) {
    for (int i = 0; i < RQ; i++) q->d[0][i] = 0.5f * (q->d[0][i] + q->d[2][i]);
    for (int i = 0; i < RQ; i++) q->d[1][i] = 0.5f * (q->d[1][i] + q->d[3][i]);
    q->silent[0] = q->silent[1] = 0;
  } else if (from == 6 && to == 2) {
    for (int i = 0; i < RQ; i++) q->d[0][i] += sqrt05 * (q->d[2][i] + q->d[4][i]);
    for (int i = 0; i < RQ; i++) q->d[1][i] += sqrt05 * (q->d[2][i] + q->d[5][i]);
    q->silent[0] = q->silent[1] = 0;
  } else if (from == 6 && to == 4) {
    /* swap_remove(3): [L,R,C,SR,SL]; swap_remove(2) -> center, channels [L,R,SL,SR] */
    Quantum tmp;
    tmp.n = 1;
    q_copy_channel(&tmp, 0, q, 2); /* center */
    q_copy_channel(q, 2, q, 4);    /* SL */
    q_copy_channel(q, 3, q, 5);    /* SR */
    for (int i = 0; i < RQ; i++) q->d[0][i] += sqrt05 * tmp.d[0][i];
    for (int i = 0; i < RQ; i++) q->d[1][i] += sqrt05 * tmp.d[0][i];
    q->silent[0] = q->silent[1] = 0;
  } else {
    for (int c = from; c < to; c++) q_silence_channel(q, c);
  }
  q->n = to;
}

/* quantum.rs:114-120 AudioRenderQuantumChannel::add */
static void q_channel_add(Quantum* self, int sc, const Quantum* other, int oc) {
  if (self->silent[sc]) {
    q_copy_channel(self, sc, other, oc);
  } else if (!other->silent[oc]) {
    for (int i = 0; i < RQ; i++) self->d[sc][i] += other->d[oc][i];
  }
}

/* quantum.rs:532-569 AudioRenderQuantum::add.
 * The pointer-identity fast path (:549-558, all channels identical => sum in mono, then
 * up-mix) yields the same values as the general path for Speakers up-mixes, so it is
 * not modelled separately. */
static void q_add(Quantum* self, const Quantum* other, int count, int mode, int interp) {
  int maxc = self->n > other->n ? self->n : other->n;
  int newc = mode == WAA_COUNT_MODE_MAX ? maxc : mode == WAA_COUNT_MODE_EXPLICIT ? count : (maxc < count ? maxc : count);
  q_mix(self, newc, interp);
  Quantum om;
  q_copy(&om, other);
  q_mix(&om, newc, interp);
  for (int c = 0; c < newc; c++) q_channel_add(self, c, &om, c);
}

/* ------------------------------------------------------------------------------------ */
/* almost crate 0.2 (third party, restated): tolerance = sqrt(f64::EPSILON)               */
/* ------------------------------------------------------------------------------------ */
static const double ALMOST_TOL = 1.4901161193847656e-8;
static int almost_zero(double a) { return fabs(a) < ALMOST_TOL; }
static int almost_equal(double a, double b) {
  if (a == b) return 1;
  if (!isfinite(a) || !isfinite(b)) return 0;
  double scale = fmax(fabs(a), fabs(b));
  if (scale < 1.0) scale = 1.0;
  return fabs(a - b) < scale * ALMOST_TOL;
}

/* ------------------------------------------------------------------------------------ */
/* f32 FFT (stand-in for realfft/rustfft): iterative radix-2, twiddles from f64           */
/* ------------------------------------------------------------------------------------ */
typedef struct {
  int n;      /* complex size */
  float* wre; /* n/2 twiddles e^{-2 pi i k / n} */
  float* wim;
  int* rev;
} FftPlan;

static FftPlan* fft_plan_new(int n) {
  FftPlan* p = (FftPlan*)calloc(1, sizeof *p);
  p->n = n;
  p->wre = (float*)malloc(sizeof(float) * (n / 2 + 1));
  p->wim = (float*)malloc(sizeof(float) * (n / 2 + 1));
  p->rev = (int*)malloc(sizeof(int) * n);
  for (int k = 0; k < n / 2; k++) {
    double a = -2.0 * M_PI * (double)k / (double)n;
    p->wre[k] = (float)cos(a);
    p->wim[k] = (float)sin(a);
  }
  int bits = 0;
  while ((1 << bits) < n) bits++;
  for (int i = 0; i < n; i++) {
    int r = 0;
    for (int b = 0; b < bits; b++)
      if (i & (1 << b)) r |= 1 << (bits - 1 - b);
    p->rev[i] = r;
  }
  return p;
}
static void fft_plan_free(FftPlan* p) {
  if (!p) return;
  free(p->wre);
  free(p->wim);
  free(p->rev);
  free(p);
}
/* in-place complex FFT, forward (sign -1) or inverse (sign +1, unscaled) */
static void fft_c2c(const FftPlan* p, float* re, float* im, int inverse) {
  int n = p->n;
  for (int i = 0; i < n; i++) {
    int r = p->rev[i];
    if (r > i) {
      float t = re[i];
      re[i] = re[r];
      re[r] = t;
      t = im[i];
      im[i] = im[r];
      im[r] = t;
    }
  }
  for (int len = 2; len <= n; len <<= 1) {
    int half = len >> 1, step = n / len;
    for (int i = 0; i < n; i += len) {
      for (int k = 0; k < half; k++) {
        float wr = p->wre[k * step], wi = inverse ? -p->wim[k * step] : p->wim[k * step];
        float ar = re[i + k], ai = im[i + k];
        float br = re[i + k + half], bi = im[i + k + half];
        float tr = br * wr - bi * wi, ti = br * wi + bi * wr;
        re[i + k] = ar + tr;
        im[i + k] = ai + ti;
        re[i + k + half] = ar - tr;
        im[i + k + half] = ai - ti;
      }
    }
  }
}

typedef struct {
  int n; /* real size */
  FftPlan* half;
  float* tre; /* n/2 twiddles e^{-2 pi i k / n}, k < n/2 */
  float* tim;
} RfftPlan; /* read-only after creation: shared by all instances / threads; scratch is the caller's */

static RfftPlan* rfft_plan_new(int n) {
  RfftPlan* p = (RfftPlan*)calloc(1, sizeof *p);
  p->n = n;
  p->half = fft_plan_new(n / 2);
  p->tre = (float*)malloc(sizeof(float) * (n / 2 + 1));
  p->tim = (float*)malloc(sizeof(float) * (n / 2 + 1));
  for (int k = 0; k <= n / 2; k++) {
    double a = -2.0 * M_PI * (double)k / (double)n;
    p->tre[k] = (float)cos(a);
    p->tim[k] = (float)sin(a);
  }
  return p;
}
static void rfft_plan_free(RfftPlan* p) {
  if (!p) return;
  fft_plan_free(p->half);
  free(p->tre);
  free(p->tim);
  free(p);
}
/* real -> n/2+1 complex bins (unnormalised); sre/sim: caller-owned scratch of n/2+1 floats each */
static void rfft_forward(const RfftPlan* p, float* sre, float* sim, const float* x, float* ore, float* oim) {
  int n = p->n, h = n / 2;
  for (int i = 0; i < h; i++) {
    sre[i] = x[2 * i];
    sim[i] = x[2 * i + 1];
  }
  fft_c2c(p->half, sre, sim, 0);
  for (int k = 0; k <= h; k++) {
    int k1 = k % h, k2 = (h - k) % h;
    float zr = sre[k1], zi = sim[k1];
    float cr = sre[k2], ci = -sim[k2]; /* conj(Z[h-k]) */
    float er = 0.5f * (zr + cr), ei = 0.5f * (zi + ci);
    float dr = 0.5f * (zr - cr), di = 0.5f * (zi - ci);
    /* odd = -i * d ; X = e + w^k * odd */
    float odr = di, odi = -dr;
    float wr = p->tre[k], wi = p->tim[k];
    ore[k] = er + (odr * wr - odi * wi);
    oim[k] = ei + (odr * wi + odi * wr);
  }
}
/* n/2+1 complex bins -> real, scaled by 1/n (true inverse) */
static void rfft_inverse(const RfftPlan* p, float* sre, float* sim, const float* ire, const float* iim, float* x) {
  int n = p->n, h = n / 2;
  for (int k = 0; k < h; k++) {
    float ar = ire[k], ai = iim[k];
    float br = ire[h - k], bi = -iim[h - k]; /* conj(X[h-k]) */
    float er = 0.5f * (ar + br), ei = 0.5f * (ai + bi);
    float dr = 0.5f * (ar - br), di = 0.5f * (ai - bi);
    /* odd = d * conj(w^k); Z = e + i * odd */
    float wr = p->tre[k], wi = -p->tim[k];
    float odr = dr * wr - di * wi, odi = dr * wi + di * wr;
    sre[k] = er - odi;
    sim[k] = ei + odr;
  }
  fft_c2c(p->half, sre, sim, 1);
  float s = 1.0f / (float)h;
  for (int i = 0; i < h; i++) {
    x[2 * i] = sre[i] * s;
    x[2 * i + 1] = sim[i] * s;
  }
}

/* ------------------------------------------------------------------------------------ */
/* rubato 0.16 FftFixedInOut / FftResampler (synchro.rs), restated from the crate's        */
/* published source: the WaveShaper's oversamplers.  Call sites: waveshaper.rs:290-347      */
/* (Resampler::new / process), :232-287 (chunk sizes and rates).  With fs_out = R * fs_in   */
/* (or fs_in = R * fs_out) and chunk_size_in = 128 (128 * R) rubato picks                   */
/* fft_size_in = chunk_size_in and fft_size_out = chunk_size_in * fs_out / fs_in.           */
/* PARITY UNPINNED by the reference (its tests only construct such nodes).                  */
/* ------------------------------------------------------------------------------------ */
typedef struct OsResampler {
  int fi, fo;        /* fft_size_in, fft_size_out */
  float *fre, *fim;  /* filter_f: fi + 1 bins */
  RfftPlan *fwd, *inv; /* real FFTs of 2 * fi and 2 * fo points */
} OsResampler;

static float os_sinc(float value) { /* rubato sinc(): sin(pi x) / (pi x) in the sample type */
  const float pi = 3.14159265358979323846f;
  if (value == 0.f) return 1.f;
  return sinf(value * pi) / (value * pi);
}
/* FftResampler::new: anti-alias cutoff, make_sincs(fft_size_in, 1, cutoff, BlackmanHarris2), filter / (2 fi), FFT */
static OsResampler* os_resampler_new(int fi, int fo) {
  OsResampler* r = (OsResampler*)calloc(1, sizeof *r);
  r->fi = fi;
  r->fo = fo;
  float cutoff = fi > fo ? powf(0.4f, 16.0f / (float)fi) * (float)fo / (float)fi : powf(0.4f, 16.0f / (float)fi);
  const float pi = 3.14159265358979323846f;
  const float pi2 = 2.f * pi, pi4 = 4.f * pi, pi6 = 6.f * pi, np = (float)fi;
  float* y = (float*)malloc(sizeof(float) * (size_t)fi);
  float sum = 0.f;
  for (int x = 0; x < fi; x++) {
    float xf = (float)x;
    float bh = 0.35875f - 0.48829f * cosf(pi2 * xf / np) + 0.14128f * cosf(pi4 * xf / np) - 0.01168f * cosf(pi6 * xf / np);
    float w = bh * bh; /* WindowFunction::BlackmanHarris2 */
    float val = w * os_sinc((xf - (float)(fi / 2)) * cutoff / 1.f);
    sum += val;
    y[x] = val;
  }
  float* ft = (float*)calloc((size_t)2 * fi, sizeof(float));
  for (int n = 0; n < fi; n++) ft[n] = (y[n] / sum) / (float)(2 * fi);
  free(y);
  r->fwd = rfft_plan_new(2 * fi);
  r->inv = rfft_plan_new(2 * fo);
  r->fre = (float*)calloc((size_t)fi + 1, sizeof(float));
  r->fim = (float*)calloc((size_t)fi + 1, sizeof(float));
  float* sre = (float*)malloc(sizeof(float) * ((size_t)fi + 1));
  float* sim = (float*)malloc(sizeof(float) * ((size_t)fi + 1));
  rfft_forward(r->fwd, sre, sim, ft, r->fre, r->fim);
  free(sre);
  free(sim);
  free(ft);
  return r;
}
static void os_resampler_free(OsResampler* r) {
  if (!r) return;
  rfft_plan_free(r->fwd);
  rfft_plan_free(r->inv);
  free(r->fre);
  free(r->fim);
  free(r);
}
/* FftResampler::resample_unit: wave_in (fi frames) -> wave_out (fo frames), overlap (fo frames) carried */
static void os_resample_unit(const OsResampler* r, const float* in, float* out, float* overlap) {
  const int fi = r->fi, fo = r->fo;
  float inbuf[2 * 512], ire[513], iim[513], ore[513] = {0}, oim[513] = {0}, sre[513], sim[513], obuf[2 * 512];
  memcpy(inbuf, in, sizeof(float) * (size_t)fi);
  memset(inbuf + fi, 0, sizeof(float) * (size_t)fi);
  rfft_forward(r->fwd, sre, sim, inbuf, ire, iim);
  const int new_len = fi < fo ? fi + 1 : fo;
  for (int k = 0; k <= fo; k++) {
    if (k < new_len) { /* spec *= filt */
      ore[k] = ire[k] * r->fre[k] - iim[k] * r->fim[k];
      oim[k] = ire[k] * r->fim[k] + iim[k] * r->fre[k];
    } else {
      ore[k] = oim[k] = 0.f;
    }
  }
  rfft_inverse(r->inv, sre, sim, ore, oim, obuf);
  const float unnorm = (float)(2 * fo); /* realfft's inverse is unnormalised; rfft_inverse divides by its length */
  for (int n = 0; n < fo; n++) out[n] = obuf[n] * unnorm + overlap[n];
  for (int n = 0; n < fo; n++) overlap[n] = obuf[fo + n] * unnorm;
}

/* ------------------------------------------------------------------------------------ */
/* FFTConvolver (crate fft-convolver 0.3 = HiFi-LoFi FFTConvolver, restated)              */
/* call sites: src/node/convolver.rs:284-306 (init), :384-466 (process)                   */
/* ------------------------------------------------------------------------------------ */
typedef struct {
  int block, seg, seg_count, csize;
  RfftPlan* plan;
  float* ir_re; /* [seg_count][csize] (shared between instances) */
  float* ir_im;
} ConvIR;

typedef struct {
  const ConvIR* ir;
  float* seg_re; /* [seg_count][csize] */
  float* seg_im;
  float* pre_re;
  float* pre_im;
  float* conv_re;
  float* conv_im;
  float* fftbuf;   /* seg */
  float* overlap;  /* block */
  float* inbuf;    /* block */
  float* sre;      /* FFT scratch, seg/2+1 each (per state: states render on different threads) */
  float* sim;
  int inbuf_fill;
  int current;
} ConvState;

static ConvIR* convir_new(int block_size, const float* ir, size_t len) {
  ConvIR* c = (ConvIR*)calloc(1, sizeof *c);
  /* ignore zeros at the end of the impulse response */
  while (len > 0 && fabsf(ir[len - 1]) < 0.000001f) len--;
  if (len == 0) return c; /* seg_count == 0: process() outputs zeros */
  int b = 1;
  while (b < block_size) b <<= 1;
  c->block = b;
  c->seg = 2 * b;
  c->seg_count = (int)((len + (size_t)b - 1) / (size_t)b);
  c->csize = c->seg / 2 + 1;
  c->plan = rfft_plan_new(c->seg);
  c->ir_re = (float*)calloc((size_t)c->seg_count * c->csize, sizeof(float));
  c->ir_im = (float*)calloc((size_t)c->seg_count * c->csize, sizeof(float));
  float* buf = (float*)calloc(c->seg, sizeof(float));
  float* sre = (float*)calloc(c->seg / 2 + 1, sizeof(float));
  float* sim = (float*)calloc(c->seg / 2 + 1, sizeof(float));
  for (int s = 0; s < c->seg_count; s++) {
    size_t remaining = len - (size_t)s * b;
    size_t cp = remaining < (size_t)b ? remaining : (size_t)b;
    memset(buf, 0, sizeof(float) * c->seg);
    memcpy(buf, ir + (size_t)s * b, cp * sizeof(float));
    rfft_forward(c->plan, sre, sim, buf, c->ir_re + (size_t)s * c->csize, c->ir_im + (size_t)s * c->csize);
  }
  free(buf);
  free(sre);
  free(sim);
  return c;
}
static void convir_free(ConvIR* c) {
  if (!c) return;
  rfft_plan_free(c->plan);
  free(c->ir_re);
  free(c->ir_im);
  free(c);
}
/* touch every page once so that a timed render does not measure first-touch page faults */
static void prefault(void* p, size_t bytes) {
  volatile unsigned char* c = (volatile unsigned char*)p;
  for (size_t i = 0; i < bytes; i += 4096) c[i] = c[i];
  if (bytes) c[bytes - 1] = c[bytes - 1];
}

static ConvState* convstate_new(const ConvIR* ir) {
  ConvState* s = (ConvState*)calloc(1, sizeof *s);
  s->ir = ir;
  if (ir->seg_count == 0) return s;
  s->seg_re = (float*)calloc((size_t)ir->seg_count * ir->csize, sizeof(float));
  s->seg_im = (float*)calloc((size_t)ir->seg_count * ir->csize, sizeof(float));
  s->pre_re = (float*)calloc(ir->csize, sizeof(float));
  s->pre_im = (float*)calloc(ir->csize, sizeof(float));
  s->conv_re = (float*)calloc(ir->csize, sizeof(float));
  s->conv_im = (float*)calloc(ir->csize, sizeof(float));
  s->fftbuf = (float*)calloc(ir->seg, sizeof(float));
  s->overlap = (float*)calloc(ir->block, sizeof(float));
  s->inbuf = (float*)calloc(ir->block, sizeof(float));
  s->sre = (float*)calloc(ir->seg / 2 + 1, sizeof(float));
  s->sim = (float*)calloc(ir->seg / 2 + 1, sizeof(float));
  prefault(s->seg_re, (size_t)ir->seg_count * ir->csize * sizeof(float));
  prefault(s->seg_im, (size_t)ir->seg_count * ir->csize * sizeof(float));
  return s;
}
static void convstate_free(ConvState* s) {
  if (!s) return;
  free(s->seg_re);
  free(s->seg_im);
  free(s->pre_re);
  free(s->pre_im);
  free(s->conv_re);
  free(s->conv_im);
  free(s->fftbuf);
  free(s->overlap);
  free(s->inbuf);
  free(s->sre);
  free(s->sim);
  free(s);
}
static void cmac(float* __restrict__ rre, float* __restrict__ rim, const float* __restrict__ are,
                 const float* __restrict__ aim, const float* __restrict__ bre, const float* __restrict__ bim, int n) {
  for (int i = 0; i < n; i++) {
    rre[i] += are[i] * bre[i] - aim[i] * bim[i];
    rim[i] += are[i] * bim[i] + aim[i] * bre[i];
  }
}
static void conv_process(ConvState* s, const float* input, float* output, int len) {
  const ConvIR* ir = s->ir;
  if (ir->seg_count == 0) {
    memset(output, 0, sizeof(float) * len);
    return;
  }
  int processed = 0;
  int cs = ir->csize;
  while (processed < len) {
    int was_empty = (s->inbuf_fill == 0);
    int processing = len - processed;
    if (processing > ir->block - s->inbuf_fill) processing = ir->block - s->inbuf_fill;
    int pos = s->inbuf_fill;
    memcpy(s->inbuf + pos, input + processed, sizeof(float) * processing);
    /* forward FFT of the zero-padded input block */
    memcpy(s->fftbuf, s->inbuf, sizeof(float) * ir->block);
    memset(s->fftbuf + ir->block, 0, sizeof(float) * ir->block);
    rfft_forward(ir->plan, s->sre, s->sim, s->fftbuf, s->seg_re + (size_t)s->current * cs, s->seg_im + (size_t)s->current * cs);
    /* complex multiplication */
    if (was_empty) {
      memset(s->pre_re, 0, sizeof(float) * cs);
      memset(s->pre_im, 0, sizeof(float) * cs);
      for (int i = 1; i < ir->seg_count; i++) {
        int ia = (s->current + i) % ir->seg_count;
        cmac(s->pre_re, s->pre_im, ir->ir_re + (size_t)i * cs, ir->ir_im + (size_t)i * cs,
             s->seg_re + (size_t)ia * cs, s->seg_im + (size_t)ia * cs, cs);
      }
    }
    memcpy(s->conv_re, s->pre_re, sizeof(float) * cs);
    memcpy(s->conv_im, s->pre_im, sizeof(float) * cs);
    cmac(s->conv_re, s->conv_im, s->seg_re + (size_t)s->current * cs, s->seg_im + (size_t)s->current * cs,
         ir->ir_re, ir->ir_im, cs);
    /* backward FFT */
    rfft_inverse(ir->plan, s->sre, s->sim, s->conv_re, s->conv_im, s->fftbuf);
    /* add overlap */
    for (int i = 0; i < processing; i++) output[processed + i] = s->fftbuf[pos + i] + s->overlap[pos + i];
    s->inbuf_fill += processing;
    if (s->inbuf_fill == ir->block) {
      memset(s->inbuf, 0, sizeof(float) * ir->block);
      s->inbuf_fill = 0;
      memcpy(s->overlap, s->fftbuf + ir->block, sizeof(float) * ir->block);
      s->current = (s->current > 0) ? (s->current - 1) : (ir->seg_count - 1);
    }
    processed += processing;
  }
}

/* ------------------------------------------------------------------------------------ */
/* AudioParam automation timeline (src/param.rs:151-235 events + queue, :796-1047          */
/* handle_incoming_event, :1049-1584 compute_*_automation + compute_buffer)                */
/* ------------------------------------------------------------------------------------ */
typedef struct {
  int type;
  float value;
  double time;
  int has_time_constant, has_cancel_time, has_duration;
  double time_constant, cancel_time, duration;
  float* values; /* owned */
  int n_values;
} TlEvent;

struct orc_timeline {
  float default_value, min_value, max_value;
  float intrinsic_value;
  float current_value;
  int a_rate;
  TlEvent* ev; /* the event queue, sorted by time (stable) unless `dirty` */
  int n, cap;
  int has_last;
  TlEvent last_event; /* values pointer not owned here (never read) */
  float buffer[1024];
  int blen;
};
typedef struct orc_timeline orc_timeline;

#define SNAP_TO_TARGET 1e-10f /* param.rs:22 */

static float tl_linear_ramp_sample(double start_time, double duration, float start_value, float diff, double time) {
  double phase = (time - start_time) / duration; /* :66-76 */
  return fmaf(diff, (float)phase, start_value);
}
static float tl_exponential_ramp_sample(double start_time, double duration, float start_value, float ratio, double time) {
  double phase = (time - start_time) / duration; /* :79-90 */
  return start_value * powf(ratio, (float)phase);
}
static float tl_set_target_sample(double start_time, double time_constant, float end_value, float diff, double time) {
  double exponent = -((time - start_time) / time_constant); /* :93-103 */
  return fmaf(diff, (float)exp(exponent), end_value);
}
static float tl_set_value_curve_sample(double start_time, double duration, const float* values, int n, double time) {
  if (time - start_time >= duration) return values[n - 1]; /* :107-121 */
  double position = (double)(n - 1) * (time - start_time) / duration;
  int k = position > 0. ? (int)position : 0; /* `as usize` saturates: negative (sample time before the start) -> 0 */
  float phase = (float)(position - floor(position));
  return fmaf(values[k + 1] - values[k], phase, values[k]);
}

orc_timeline* orc_timeline_create(float default_value, float min_value, float max_value, int32_t a_rate) {
  orc_timeline* t = (orc_timeline*)calloc(1, sizeof *t);
  t->default_value = default_value;
  t->min_value = min_value;
  t->max_value = max_value;
  t->intrinsic_value = default_value;
  t->current_value = default_value;
  t->a_rate = a_rate != 0;
  return t;
}
void orc_timeline_destroy(orc_timeline* t) {
  if (!t) return;
  for (int i = 0; i < t->n; i++) free(t->ev[i].values);
  free(t->ev);
  free(t);
}
float orc_timeline_value(const orc_timeline* t) { return t->current_value; }

static void tl_push(orc_timeline* t, TlEvent e) {
  if (t->n == t->cap) {
    t->cap = t->cap ? t->cap * 2 : 32;
    t->ev = (TlEvent*)realloc(t->ev, sizeof(TlEvent) * (size_t)t->cap);
  }
  t->ev[t->n++] = e;
}
static void tl_sort(orc_timeline* t) { /* stable sort by time (Vec::sort_by is stable), :222-226 */
  for (int i = 1; i < t->n; i++) {
    TlEvent e = t->ev[i];
    int j = i - 1;
    while (j >= 0 && t->ev[j].time > e.time) {
      t->ev[j + 1] = t->ev[j];
      j--;
    }
    t->ev[j + 1] = e;
  }
}
static TlEvent tl_pop(orc_timeline* t) { /* remove(0), :186-192 */
  TlEvent e = t->ev[0];
  memmove(t->ev, t->ev + 1, sizeof(TlEvent) * (size_t)(t->n - 1));
  t->n--;
  return e;
}
static void tl_set_last(orc_timeline* t, TlEvent e) {
  free(e.values); /* the curve of a finished SetValueCurve is never read again */
  e.values = NULL;
  t->last_event = e;
  t->has_last = 1;
}
static TlEvent tl_plain(int type, float value, double time) {
  TlEvent e;
  memset(&e, 0, sizeof e);
  e.type = type;
  e.value = value;
  e.time = time;
  return e;
}

/* control side: the *_raw constructors (param.rs:399-596) + render side: handle_incoming_event (:796-1047) */
waa_status orc_timeline_event(orc_timeline* t, int32_t type, float value, double time, double aux, const float* curve,
                              uint32_t n_curve) {
  if (!t) return fail(WAA_ERR_INVALID_ARGUMENT, "null timeline");
  TlEvent event = tl_plain(type, value, time);
  switch (type) {
    case WAA_EVENT_SET_VALUE:
      if (!isfinite(value)) return fail(WAA_ERR_INVALID_ARGUMENT, "TypeError - The provided value is non-finite.");
      t->current_value = fminf(fmaxf(value, t->min_value), t->max_value);
      event.time = 0.;
      break;
    case WAA_EVENT_SET_VALUE_AT_TIME:
    case WAA_EVENT_LINEAR_RAMP:
      if (!isfinite(value)) return fail(WAA_ERR_INVALID_ARGUMENT, "TypeError - The provided value is non-finite.");
      break;
    case WAA_EVENT_EXPONENTIAL_RAMP:
      if (!isfinite(value)) return fail(WAA_ERR_INVALID_ARGUMENT, "TypeError - The provided value is non-finite.");
      if (value == 0.f) return fail(WAA_ERR_INVALID_ARGUMENT, "RangeError - value (0.0) should not be equal to zero");
      break;
    case WAA_EVENT_SET_TARGET:
      if (!isfinite(value)) return fail(WAA_ERR_INVALID_ARGUMENT, "TypeError - The provided value is non-finite.");
      if (!isfinite(aux)) return fail(WAA_ERR_INVALID_ARGUMENT, "TypeError - The provided time value is non-finite.");
      if (aux < 0.) return fail(WAA_ERR_INVALID_ARGUMENT, "RangeError - The provided time value cannot be negative");
      if (aux == 0.) { /* "the output value jumps immediately to the final value", :497-507 */
        event.type = WAA_EVENT_SET_VALUE_AT_TIME;
      } else {
        event.has_time_constant = 1;
        event.time_constant = aux;
      }
      break;
    case WAA_EVENT_CANCEL_SCHEDULED_VALUES:
    case WAA_EVENT_CANCEL_AND_HOLD: event.value = 0.f; break;
    case WAA_EVENT_SET_VALUE_CURVE:
      if (!curve || n_curve < 2)
        return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - sequence length (%u) should not be less than 2", n_curve);
      if (!isfinite(aux)) return fail(WAA_ERR_INVALID_ARGUMENT, "TypeError - The provided value is non-finite.");
      if (!(aux > 0.)) return fail(WAA_ERR_INVALID_ARGUMENT, "RangeError - duration (%g) should be strictly positive", aux);
      event.value = 0.f;
      event.has_duration = 1;
      event.duration = aux;
      break;
    default: return fail(WAA_ERR_INVALID_ARGUMENT, "unknown automation event type %d", type);
  }
  if (type != WAA_EVENT_SET_VALUE) { /* assert_valid_time_value */
    if (!isfinite(time)) return fail(WAA_ERR_INVALID_ARGUMENT, "TypeError - The provided time value is non-finite.");
    if (time < 0.) return fail(WAA_ERR_INVALID_ARGUMENT, "RangeError - The provided time value cannot be negative");
  }

  /* ---- handle_incoming_event ---- */
  if (event.type == WAA_EVENT_CANCEL_SCHEDULED_VALUES) { /* :808-864 */
    if (t->n > 0) {
      const TlEvent* cur = &t->ev[0];
      if ((cur->type == WAA_EVENT_LINEAR_RAMP || cur->type == WAA_EVENT_EXPONENTIAL_RAMP) && cur->time >= event.time && t->has_last)
        t->intrinsic_value = t->last_event.value;
    }
    int k = 0;
    for (int i = 0; i < t->n; i++) {
      if (t->ev[i].time < event.time)
        t->ev[k++] = t->ev[i];
      else
        free(t->ev[i].values);
    }
    t->n = k;
    return WAA_OK;
  }
  if (event.type == WAA_EVENT_CANCEL_AND_HOLD) { /* :866-945 */
    int e1 = -1, e2 = -1;
    double t1 = -DBL_MAX, t2 = DBL_MAX;
    tl_sort(t);
    for (int i = 0; i < t->n; i++) {
      if (t->ev[i].time >= t1 && t->ev[i].time <= event.time) {
        t1 = t->ev[i].time;
        e1 = i;
      } else if (t->ev[i].time < t2 && t->ev[i].time > event.time) {
        t2 = t->ev[i].time;
        e2 = i;
      }
    }
    if (e2 >= 0) {
      if (t->ev[e2].type == WAA_EVENT_LINEAR_RAMP || t->ev[e2].type == WAA_EVENT_EXPONENTIAL_RAMP) {
        t->ev[e2].has_cancel_time = 1;
        t->ev[e2].cancel_time = event.time;
      }
    } else if (e1 >= 0) {
      if (t->ev[e1].type == WAA_EVENT_SET_TARGET) {
        t->ev[e1].has_cancel_time = 1;
        t->ev[e1].cancel_time = event.time;
      } else if (t->ev[e1].type == WAA_EVENT_SET_VALUE_CURVE) {
        if (event.time <= t->ev[e1].time + t->ev[e1].duration) {
          t->ev[e1].has_cancel_time = 1;
          t->ev[e1].cancel_time = event.time;
        }
      }
    }
    int k = 0;
    for (int i = 0; i < t->n; i++) {
      double tt = t->ev[i].has_cancel_time ? t->ev[i].cancel_time : t->ev[i].time;
      if (tt <= event.time)
        t->ev[k++] = t->ev[i];
      else
        free(t->ev[i].values);
    }
    t->n = k;
    return WAA_OK;
  }
  if (event.type == WAA_EVENT_SET_VALUE_CURVE) { /* :947-968 */
    double start_time = event.time, end_time = start_time + event.duration;
    for (int i = 0; i < t->n; i++)
      if (!(t->ev[i].time <= start_time || t->ev[i].time >= end_time))
        return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - scheduling SetValueCurveAtTime at time of another automation event");
  }
  if (event.type == WAA_EVENT_SET_VALUE_AT_TIME || event.type == WAA_EVENT_SET_VALUE || event.type == WAA_EVENT_LINEAR_RAMP ||
      event.type == WAA_EVENT_EXPONENTIAL_RAMP || event.type == WAA_EVENT_SET_TARGET) { /* :970-993 */
    for (int i = 0; i < t->n; i++)
      if (t->ev[i].type == WAA_EVENT_SET_VALUE_CURVE) {
        double start_time = t->ev[i].time, end_time = start_time + t->ev[i].duration;
        if (!(event.time <= start_time || event.time >= end_time))
          return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - scheduling automation event during SetValueCurveAtTime");
      }
  }
  if (event.type == WAA_EVENT_SET_VALUE) t->intrinsic_value = event.value; /* :995-998 */
  if (t->n == 0 && !t->has_last && (event.type == WAA_EVENT_LINEAR_RAMP || event.type == WAA_EVENT_EXPONENTIAL_RAMP))
    tl_push(t, tl_plain(WAA_EVENT_SET_VALUE, t->intrinsic_value, 0.)); /* :1000-1022 */
  if (t->n == 0 && event.type == WAA_EVENT_SET_TARGET) tl_push(t, tl_plain(WAA_EVENT_SET_VALUE, t->intrinsic_value, 0.)); /* :1024-1043 */
  if (event.type == WAA_EVENT_SET_VALUE_CURVE) {
    event.values = (float*)malloc(sizeof(float) * n_curve);
    memcpy(event.values, curve, sizeof(float) * n_curve);
    event.n_values = (int)n_curve;
  }
  tl_push(t, event);
  tl_sort(t);
  return WAA_OK;
}

typedef struct {
  double block_time, dt, next_block_time;
  int count, is_a_rate;
} TlBlock;

static int tl_end_index(const TlBlock* b, double end_time) { /* ((end_time - block_time).max(0.) / dt).round() as usize, clipped */
  double v = round(fmax(end_time - b->block_time, 0.) / b->dt);
  if (v > (double)b->count) return b->count;
  return (int)v;
}

/* :1049-1096 */
static int tl_compute_set_value(orc_timeline* t, const TlBlock* b) {
  TlEvent* event = &t->ev[0];
  double time = event->time;
  if (time == 0.) time = b->block_time;
  if (b->is_a_rate) {
    int end_index_clipped = tl_end_index(b, time);
    for (int i = t->blen; i < end_index_clipped; i++) t->buffer[t->blen++] = t->intrinsic_value;
  }
  if (time > b->next_block_time) return 1;
  t->intrinsic_value = event->value;
  TlEvent e = tl_pop(t);
  e.time = time;
  tl_set_last(t, e);
  return 0;
}
/* :1100-1170 */
static int tl_compute_linear_ramp(orc_timeline* t, const TlBlock* b) {
  TlEvent* event = &t->ev[0];
  double start_time = t->last_event.time, end_time = event->time;
  double duration = end_time - start_time;
  if (event->has_cancel_time) end_time = event->cancel_time;
  float start_value = t->last_event.value, end_value = event->value, diff = end_value - start_value;
  if (b->is_a_rate) {
    int start_index = t->blen, end_index_clipped = tl_end_index(b, end_time);
    if (end_index_clipped > start_index) {
      double time = fma((double)start_index, b->dt, b->block_time);
      float value = 0.f;
      for (int i = start_index; i < end_index_clipped; i++) {
        value = tl_linear_ramp_sample(start_time, duration, start_value, diff, time);
        t->buffer[t->blen++] = value;
        time += b->dt;
      }
      t->intrinsic_value = value;
    }
  }
  if (end_time >= b->next_block_time) {
    t->intrinsic_value = tl_linear_ramp_sample(start_time, duration, start_value, diff, b->next_block_time);
    return 1;
  }
  if (event->has_cancel_time) {
    float value = tl_linear_ramp_sample(start_time, duration, start_value, diff, end_time);
    t->intrinsic_value = value;
    TlEvent e = tl_pop(t);
    e.time = end_time;
    e.value = value;
    tl_set_last(t, e);
  } else {
    t->intrinsic_value = end_value;
    tl_set_last(t, tl_pop(t));
  }
  return 0;
}
/* :1174-1278 */
static int tl_compute_exponential_ramp(orc_timeline* t, const TlBlock* b) {
  TlEvent* event = &t->ev[0];
  double start_time = t->last_event.time, end_time = event->time;
  double duration = end_time - start_time;
  if (event->has_cancel_time) end_time = event->cancel_time;
  float start_value = t->last_event.value, end_value = event->value, ratio = end_value / start_value;
  if (start_value == 0.f || start_value * end_value < 0.f) {
    free(t->ev[0].values);
    t->ev[0] = tl_plain(WAA_EVENT_SET_VALUE_AT_TIME, end_value, end_time); /* replace_peek */
    return 0;
  }
  if (b->is_a_rate) {
    int start_index = t->blen, end_index_clipped = tl_end_index(b, end_time);
    if (end_index_clipped > start_index) {
      double time = fma((double)start_index, b->dt, b->block_time);
      float value = 0.f;
      for (int i = start_index; i < end_index_clipped; i++) {
        value = tl_exponential_ramp_sample(start_time, duration, start_value, ratio, time);
        t->buffer[t->blen++] = value;
        time += b->dt;
      }
      t->intrinsic_value = value;
    }
  }
  if (end_time >= b->next_block_time) {
    t->intrinsic_value = tl_exponential_ramp_sample(start_time, duration, start_value, ratio, b->next_block_time);
    return 1;
  }
  if (event->has_cancel_time) {
    float value = tl_exponential_ramp_sample(start_time, duration, start_value, ratio, end_time);
    t->intrinsic_value = value;
    TlEvent e = tl_pop(t);
    e.time = end_time;
    e.value = value;
    tl_set_last(t, e);
  } else {
    t->intrinsic_value = end_value;
    tl_set_last(t, tl_pop(t));
  }
  return 0;
}
/* :1286-1420 */
static int tl_compute_set_target(orc_timeline* t, const TlBlock* b) {
  TlEvent* event = &t->ev[0];
  double end_time = b->next_block_time;
  int ended = 0;
  if (t->n > 1) {
    const TlEvent* next_event = &t->ev[1];
    if (next_event->type == WAA_EVENT_LINEAR_RAMP || next_event->type == WAA_EVENT_EXPONENTIAL_RAMP) {
      end_time = b->block_time;
      ended = 1;
    } else if (next_event->time < b->next_block_time) {
      end_time = next_event->time;
      ended = 1;
    }
  }
  if (event->has_cancel_time && event->cancel_time < b->next_block_time) {
    end_time = event->cancel_time;
    ended = 1;
  }
  double start_time = event->time;
  float start_value = t->last_event.value, end_value = event->value, diff = start_value - end_value;
  double time_constant = event->time_constant;
  if (b->is_a_rate) {
    int start_index = t->blen, end_index_clipped = tl_end_index(b, end_time);
    if (end_index_clipped > start_index) {
      double time = fma((double)start_index, b->dt, b->block_time);
      float value = 0.f;
      for (int i = start_index; i < end_index_clipped; i++) {
        value = (time - start_time < 0.) ? t->intrinsic_value : tl_set_target_sample(start_time, time_constant, end_value, diff, time);
        t->buffer[t->blen++] = value;
        time += b->dt;
      }
      t->intrinsic_value = value;
    }
  }
  if (!ended) {
    float value = tl_set_target_sample(start_time, time_constant, end_value, diff, b->next_block_time);
    float d = fabsf(end_value - value);
    if (d < SNAP_TO_TARGET) {
      t->intrinsic_value = end_value;
      if (end_value == 0.f)
        for (int i = 0; i < t->blen; i++)
          if (fpclassify(t->buffer[i]) == FP_SUBNORMAL) t->buffer[i] = 0.f;
      free(t->ev[0].values);
      t->ev[0] = tl_plain(WAA_EVENT_SET_VALUE_AT_TIME, end_value, b->next_block_time); /* replace_peek */
    } else {
      t->intrinsic_value = value;
    }
    return 1;
  }
  float value = tl_set_target_sample(start_time, time_constant, end_value, diff, end_time);
  t->intrinsic_value = value;
  TlEvent e = tl_pop(t);
  e.time = end_time;
  e.value = value;
  tl_set_last(t, e);
  return 0;
}
/* :1422-1496 */
static int tl_compute_set_value_curve(orc_timeline* t, const TlBlock* b) {
  TlEvent* event = &t->ev[0];
  double start_time = event->time, duration = event->duration;
  const float* values = event->values;
  int n = event->n_values;
  double end_time = start_time + duration;
  if (event->has_cancel_time) end_time = event->cancel_time;
  if (b->is_a_rate) {
    int start_index = t->blen, end_index_clipped = tl_end_index(b, end_time);
    if (end_index_clipped > start_index) {
      double time = fma((double)start_index, b->dt, b->block_time);
      float value = 0.f;
      for (int i = start_index; i < end_index_clipped; i++) {
        value = time < start_time ? t->intrinsic_value : tl_set_value_curve_sample(start_time, duration, values, n, time);
        t->buffer[t->blen++] = value;
        time += b->dt;
      }
      t->intrinsic_value = value;
    }
  }
  if (end_time >= b->next_block_time) {
    t->intrinsic_value = tl_set_value_curve_sample(start_time, duration, values, n, b->next_block_time);
    return 1;
  }
  float value = event->has_cancel_time ? tl_set_value_curve_sample(start_time, duration, values, n, end_time) : values[n - 1];
  t->intrinsic_value = value;
  TlEvent e = tl_pop(t);
  e.time = end_time;
  e.value = value;
  tl_set_last(t, e);
  return 0;
}

/* compute_buffer, :1498-1584; returns the number of values (1 or count) */
uint32_t orc_timeline_compute(orc_timeline* t, double block_time, double dt, uint32_t count, float* out) {
  if (count > 1024) count = 1024;
  t->current_value = fminf(fmaxf(t->intrinsic_value, t->min_value), t->max_value);
  t->blen = 0;
  TlBlock b;
  b.block_time = block_time;
  b.dt = dt;
  b.count = (int)count;
  b.is_a_rate = t->a_rate;
  b.next_block_time = fma(dt, (double)count, block_time);
  int is_constant_block = 1;
  if (t->n > 0) {
    const TlEvent* e = &t->ev[0];
    if (e->type != WAA_EVENT_LINEAR_RAMP && e->type != WAA_EVENT_EXPONENTIAL_RAMP)
      is_constant_block = e->time >= b.next_block_time;
    else
      is_constant_block = 0;
  }
  if (!b.is_a_rate || is_constant_block) {
    t->buffer[t->blen++] = t->intrinsic_value;
    if (is_constant_block) goto done;
  }
  for (;;) {
    int exit_loop;
    if (t->n == 0) {
      if (b.is_a_rate)
        for (int i = t->blen; i < b.count; i++) t->buffer[t->blen++] = t->intrinsic_value;
      exit_loop = 1;
    } else {
      switch (t->ev[0].type) {
        case WAA_EVENT_SET_VALUE:
        case WAA_EVENT_SET_VALUE_AT_TIME: exit_loop = tl_compute_set_value(t, &b); break;
        case WAA_EVENT_LINEAR_RAMP: exit_loop = tl_compute_linear_ramp(t, &b); break;
        case WAA_EVENT_EXPONENTIAL_RAMP: exit_loop = tl_compute_exponential_ramp(t, &b); break;
        case WAA_EVENT_SET_TARGET: exit_loop = tl_compute_set_target(t, &b); break;
        case WAA_EVENT_SET_VALUE_CURVE: exit_loop = tl_compute_set_value_curve(t, &b); break;
        default: exit_loop = 1; break;
      }
    }
    if (exit_loop) break;
  }
done:
  memcpy(out, t->buffer, sizeof(float) * (size_t)t->blen);
  return (uint32_t)t->blen;
}

/* Same entry point as the product's waa_timeline_render_device (the device replay of a timeline): here it is simply the
 * per-quantum evaluation above on a copy of the timeline, so that the parity tests can drive both libraries alike. */
waa_status orc_timeline_render_device(const orc_timeline* t, uint32_t n_quanta, float sample_rate, float* out, uint8_t* lens) {
  if (!t || !out || !lens || n_quanta == 0) return fail(WAA_ERR_INVALID_ARGUMENT, "bad arguments");
  orc_timeline* c = (orc_timeline*)malloc(sizeof *c);
  *c = *t;
  c->ev = (TlEvent*)malloc(sizeof(TlEvent) * (size_t)(t->cap ? t->cap : 1));
  c->cap = t->cap ? t->cap : 1;
  for (int i = 0; i < t->n; i++) {
    c->ev[i] = t->ev[i];
    if (t->ev[i].values) {
      c->ev[i].values = (float*)malloc(sizeof(float) * (size_t)t->ev[i].n_values);
      memcpy(c->ev[i].values, t->ev[i].values, sizeof(float) * (size_t)t->ev[i].n_values);
    }
  }
  double sr = (double)sample_rate, dt = 1. / sr;
  for (uint32_t q = 0; q < n_quanta; q++) {
    float buf[RQ];
    uint32_t n = orc_timeline_compute(c, (double)((uint64_t)q * RQ) / sr, dt, RQ, buf);
    lens[q] = (uint8_t)(n == 1 ? 1 : RQ);
    for (uint32_t i = 0; i < RQ; i++) out[(size_t)q * RQ + i] = n == 1 ? buf[0] : buf[i];
  }
  orc_timeline_destroy(c);
  return WAA_OK;
}

/* ------------------------------------------------------------------------------------ */
/* context / nodes                                                                        */
/* ------------------------------------------------------------------------------------ */
typedef struct {
  uint64_t q0;
  uint32_t nq, vpq;
  float* v;
  int owned;
} ParamBlock;

typedef struct {
  float* cst;          /* [n_inst] */
  ParamBlock* blk;     /* [n_inst] */
  float defv, minv, maxv;
  orc_timeline** tl;   /* [n_inst] automation timelines (NULL until an event is scheduled) */
  float* tl_vals;      /* [n_inst][RQ] this quantum's intrinsic values: the AudioParam is its own graph node and runs
                        * ONCE in EVERY quantum (param.rs:686-699), whether or not its owner processes */
  int* tl_vlen;        /* [n_inst] 1 or RQ */
  int k_rate;          /* AutomationRate::K (source playbackRate / detune) */
  double sample_rate;
} Param;

typedef struct {
  float** ch; /* [n_ch] -> frames */
  uint32_t n_ch;
  uint64_t frames;
  float sr;
  int* refcnt;
} Buf;

typedef struct {
  waa_node_desc desc;
  int cc, ccmode, ccinterp;
  int n_params;
  Param params[WAA_MAX_PARAMS];
  /* buffer source (per instance arrays) */
  Buf* bufs;           /* [n_inst] */
  double *start_time, *stop_time, *offset, *duration; /* [n_inst] */
  unsigned char* msg_started;                          /* [n_inst] start() called at a suspend point (a control message) */
  int* is_looping;
  double *loop_start, *loop_end;
  /* convolver (shared) */
  ConvIR* conv_ir[4];
  int n_conv;
  uint64_t impulse_length;
  int impulse_channels;
  int has_ir;
  /* waveshaper (shared) */
  float* curve;
  uint32_t curve_n;
  int has_curve;
  int can_propagate_silence;
  /* oscillator: custom wavetable (periodic_wave.rs:76, 8192 points), shared */
  float* osc_wave;
  /* iir filter (shared): normalised (b, a) pairs, iir_filter.rs:273-311 */
  double iir_b[WAA_MAX_IIR_COEFFS], iir_a[WAA_MAX_IIR_COEFFS];
  int iir_len;
  /* waveshaper oversampling (shared, read-only): the up / down resamplers of waveshaper.rs:232-287 */
  struct OsResampler *os_up, *os_dn;
  int os_factor; /* 1 (none), 2, 4 */
  /* HRTF panner (shared, read-only): the HRIR sphere at the context's sample rate (panner.rs:39-68) */
  const struct HrirSphere* hrtf;
} NodeCfg;

typedef struct {
  Quantum in, out;
  /* biquad */
  double xy[ORC_MAXC][4];
  int xy_len;
  /* oscillator render state (oscillator.rs:323-334) */
  double osc_phase;
  int osc_started;
  /* audio-rate inputs of this node's AudioParams (param.rs:686-699), allocated for modulated params only */
  Quantum* pin[WAA_MAX_PARAMS];
  /* delay line (delay.rs:297-303): ring of num_quanta + 1 render quanta shared by writer and reader */
  Quantum* dl_ring;
  int dl_cap, dl_windex, dl_rindex;
  uint64_t dl_latest_frame_written;
  int dl_written_once, dl_in_cycle;
  /* iir filter: per-channel state, iir_filter.rs:269 */
  double iir_state[ORC_MAXC][WAA_MAX_IIR_COEFFS];
  int iir_nch;
  /* buffer source render state (audio_buffer_source.rs:352-370) */
  double buffer_time, buffer_time_elapsed;
  double start_time, stop_time, offset, duration;
  int started, entered_loop, is_aligned, ended;
  int is_looping;
  double loop_start, loop_end;
  /* constant source / oscillator */
  int ended_triggered;
  /* quantum in which the renderer called send_ended_event() (processor.rs:53-58); -1: not yet; after the last quantum
   * WAA_ENDED_AT_UNLOAD if before_drop sends it (thread.rs:398-411) */
  int64_t ended_q;
  /* convolver */
  ConvState* conv[4];
  uint64_t tail_count;
  /* analyser ring (analysis.rs:80-127) */
  float* ring;
  size_t write_index;
  float* last_fft_output;
  double last_fft_time;
  int has_inputs;
  /* waveshaper oversampling: overlap of the up / down resampler per channel; channel count they were built for
   * minus one (zero-initialised = the renderer's initial channels_x2 = channels_x4 = 1, waveshaper.rs:526-527) */
  float *os_up_ovl, *os_dn_ovl;
  int os_channels_m1;
  /* HRTF panner: the last hrir_len - 1 input samples (HrtfState::prev_left_samples; left == right for a mono
   * source), tail counter (panner.rs:682) */
  float* hrtf_prev;
  uint64_t hrtf_tail_counter;
} NodeState;

#define MAX_FFT_SIZE 32768
#define RING_BUFFER_SIZE (MAX_FFT_SIZE + RQ)

static const struct HrirSphere* hrir_for_rate(uint32_t sample_rate); /* HRTF panner, below */

/* A control message submitted while the render is suspended in front of quantum q (OfflineAudioContext::suspend_sync,
 * offline.rs:359-397): the render thread handles it right before that quantum (thread.rs:277-294).  Unlike the product
 * library — which renders node-major and therefore COMPILES the history into the plan (gated connections, clamped start
 * times, events that enter the automation queue late) — this interpreter really is a quantum loop and applies the message
 * when its quantum comes: an independent statement of the same semantics. */
enum { CTL_EVENT = 1, CTL_START = 2, CTL_STOP = 3 };
typedef struct {
  uint32_t q;
  int kind;
  uint32_t node, param, inst;
  int32_t type;
  float value;
  double t, aux, offset, duration;
  float* curve;
  uint32_t n_curve;
} CtlMsg;
typedef struct {
  uint32_t q0;            /* first quantum of the epoch */
  unsigned char* active;  /* [n_edges] the connections that exist during it */
  uint32_t* order;
  uint32_t n_order;
} Epoch;
#define ORC_EDGE_NEVER 0xFFFFFFFFu
struct orc_batch {
  uint32_t n_nodes, n_edges, n_inst, n_out;
  uint64_t length;
  float sr;
  NodeCfg* nodes;
  waa_edge_desc* edges;
  uint32_t *edge_on, *edge_off; /* [n_edges] live for quanta [on, off) */
  uint32_t edge_cap;
  const unsigned char* edge_active; /* the epoch order_nodes is asked about (NULL: every edge) */
  uint32_t ctl_q;               /* the control clock: orc_render_range */
  int ranged;
  CtlMsg* msgs;
  uint32_t n_msgs, msg_cap;
  Epoch* epochs;
  uint32_t n_epochs;
  uint32_t* order;
  uint32_t n_order;
  NodeState** st; /* [n_inst][n_nodes] */
  float* out;     /* [n_inst][n_out][length] */
  int rendered;
  int n_threads;
  int exact_conv;
  unsigned char* dbg_codes; /* [n_inst][n_nodes][n_quanta], ORC_DUMP_CODES only */
};
typedef struct orc_batch orc_batch;

static void ctl_push(orc_batch* b, CtlMsg m) {
  if (b->n_msgs == b->msg_cap) {
    b->msg_cap = b->msg_cap ? 2 * b->msg_cap : 16;
    b->msgs = (CtlMsg*)realloc(b->msgs, sizeof(CtlMsg) * b->msg_cap);
  }
  m.q = b->ctl_q;
  b->msgs[b->n_msgs++] = m;
}

static void param_init(Param* p, uint32_t n_inst, float defv, float minv, float maxv) {
  p->cst = (float*)malloc(sizeof(float) * n_inst);
  for (uint32_t i = 0; i < n_inst; i++) p->cst[i] = defv;
  p->blk = (ParamBlock*)calloc(n_inst, sizeof(ParamBlock));
  p->defv = defv;
  p->minv = minv;
  p->maxv = maxv;
}
/* AudioParamValues::get (src/render/processor.rs:186-229): slice of len 1 or 128.
 * Values handed in by the host already went through the timeline; the clamp / NaN rule of
 * AudioParamProcessor::mix_to_output (src/param.rs:739-797) is applied here. */
static float param_fix(const Param* p, float x) { /* param.rs:755-761: NaN -> default, max then min */
  return isnan(x) ? p->defv : fminf(fmaxf(x, p->minv), p->maxv);
}
/* AudioParamValues::get of one param for this quantum = AudioParamProcessor::process (param.rs:686-795):
 * intrinsic values (a constant or a caller-computed block: the timeline of param.rs:1050-1600 stays on the
 * host) mixed with the param's audio-rate input `in` (NULL when nothing is connected).  All params the device
 * path modulates are a-rate. */
static const float* param_get_in(const Param* p, const Quantum* in, uint32_t inst, uint64_t q, int* len, float* tmp) {
  const ParamBlock* b = &p->blk[inst];
  float one;
  float tlbuf[RQ];
  const float* v = &one;
  int vlen = 1;
  one = p->cst[inst];
  if (p->tl && p->tl[inst]) { /* evaluated by params_advance() at the start of the quantum */
    (void)tlbuf;
    v = p->tl_vals + (size_t)inst * RQ;
    vlen = p->tl_vlen[inst];
  } else if (b->v && q >= b->q0 && q < b->q0 + b->nq) {
    v = b->v + (size_t)(q - b->q0) * b->vpq;
    vlen = (int)b->vpq;
  }
  int in_silent = !in || q_is_silent(in);
  if (vlen == 1) {
    if (in_silent) { /* single-valued output */
      tmp[0] = param_fix(p, v[0] + (in ? in->d[0][0] : 0.f));
      *len = 1;
    } else {
      for (int i = 0; i < RQ; i++) tmp[i] = param_fix(p, in->d[0][i] + v[0]);
      *len = RQ;
    }
  } else {
    for (int i = 0; i < RQ; i++) tmp[i] = param_fix(p, (in ? in->d[0][i] : 0.f) + v[i]);
    *len = RQ;
  }
  return tmp;
}
/* AudioParamProcessor::process of every automated param for quantum q: compute_intrinsic_values(current_time, 1/sr,
 * 128) (param.rs:686-699).  The timeline is stateful (events are consumed, a SetValue at time 0 takes the time of the
 * block that consumes it, param.rs:1060-1062), so it has to run exactly once per quantum from quantum 0 on — not
 * only in the quanta in which the owning node happens to read it (a node with a silent input returns early). */
static void param_advance(Param* p, uint32_t inst, uint64_t q) {
  if (!p->tl || !p->tl[inst]) return;
  double block_time = (double)(q * RQ) / p->sample_rate;
  p->tl_vlen[inst] = (int)orc_timeline_compute(p->tl[inst], block_time, 1. / p->sample_rate, RQ, p->tl_vals + (size_t)inst * RQ);
}
static inline const float* param_get(const Param* p, uint32_t inst, uint64_t q, int* len, float* tmp) {
  return param_get_in(p, NULL, inst, q, len, tmp);
}

/* graph.rs:323-487 order_nodes/visit: DFS post-order over outgoing edges in insertion order, reversed; cycles
 * are broken at the first cycle breaker on the detected loop (a DelayNode's WRITER half: its writer->reader edge
 * is cleared and the ordering restarts, graph.rs:340-361,440-452); nodes of a cycle without a breaker are
 * dropped from the ordering (muted, graph.rs:362-368,455-458).  A DelayNode is two graph nodes in the reference
 * (delay.rs:283-366: writer registered first, reader second, edge writer->reader); here the node id is the
 * writer and id | ORC_READER the reader. */
#define ORC_READER 0x80000000u
typedef struct {
  const orc_batch* b;
  const unsigned char* cut; /* [n_nodes] writer->reader edge cleared */
  uint32_t *marked, n_marked, *temp, n_temp, *ordered, n_ordered, *in_cycle, n_in_cycle;
  uint32_t breaker;
} OrderCtx;
static int vtx_in(const uint32_t* a, uint32_t n, uint32_t v) {
  for (uint32_t i = 0; i < n; i++)
    if (a[i] == v) return (int)i;
  return -1;
}
static int order_visit(OrderCtx* c, uint32_t v) {
  const orc_batch* b = c->b;
  int pos = vtx_in(c->temp, c->n_temp, v);
  if (pos >= 0) {
    for (uint32_t i = (uint32_t)pos; i < c->n_temp; i++) {
      uint32_t t = c->temp[i];
      if (!(t & ORC_READER) && b->nodes[t].desc.kind == WAA_NODE_DELAY) { /* cycle_breaker == true */
        c->breaker = t;
        return 1;
      }
    }
    for (uint32_t i = (uint32_t)pos; i < c->n_temp; i++) c->in_cycle[c->n_in_cycle++] = c->temp[i];
    return 0;
  }
  if (vtx_in(c->marked, c->n_marked, v) >= 0) return 0;
  c->marked[c->n_marked++] = v;
  c->temp[c->n_temp++] = v;
  uint32_t id = v & ~ORC_READER;
  if (!(v & ORC_READER) && b->nodes[id].desc.kind == WAA_NODE_DELAY) {
    if (!c->cut[id] && order_visit(c, id | ORC_READER)) return 1;
  } else {
    for (uint32_t e = 0; e < b->n_edges; e++) {
      if (b->edges[e].from != id || (b->edge_active && !b->edge_active[e])) continue;
      uint32_t to = b->edges[e].to;
      /* inputs go to the writer; a param edge goes to the param's owner: delayTime belongs to the reader */
      if (b->nodes[to].desc.kind == WAA_NODE_DELAY && (b->edges[e].to_input & 0x80000000u)) to |= ORC_READER;
      if (order_visit(c, to)) return 1;
    }
  }
  c->ordered[c->n_ordered++] = v;
  uint32_t k = 0;
  for (uint32_t i = 0; i < c->n_temp; i++)
    if (c->temp[i] != v) c->temp[k++] = c->temp[i];
  c->n_temp = k;
  return 0;
}
/* fills b->order (render order) and b->n_order */
static void order_nodes(orc_batch* b) {
  uint32_t cap = 2 * b->n_nodes + 2;
  unsigned char* cut = (unsigned char*)calloc(b->n_nodes, 1);
  OrderCtx c;
  c.b = b;
  c.cut = cut;
  c.marked = (uint32_t*)malloc(sizeof(uint32_t) * cap);
  c.temp = (uint32_t*)malloc(sizeof(uint32_t) * cap);
  c.ordered = (uint32_t*)malloc(sizeof(uint32_t) * cap);
  c.in_cycle = (uint32_t*)malloc(sizeof(uint32_t) * cap * 4);
  for (;;) {
    c.n_marked = c.n_temp = c.n_ordered = c.n_in_cycle = 0;
    int applied = 0;
    for (uint32_t i = 0; i < b->n_nodes && !applied; i++) {
      applied = order_visit(&c, i);
      if (!applied && b->nodes[i].desc.kind == WAA_NODE_DELAY) applied = order_visit(&c, i | ORC_READER);
      /* The AudioListener is graph node 1 (LISTENER_NODE_ID, context/mod.rs:26), right behind the destination, with one
       * outgoing edge per PannerNode in creation order (concrete_base.rs:511-534 connect_listener_to_panner): as a DFS
       * root it pulls every panner branch to the front of the traversal, which moves those branches BACK in the
       * reversed post-order and thereby fixes the f32 summing order of fan-ins of three or more signals. */
      if (i == 0)
        for (uint32_t pn = 0; pn < b->n_nodes && !applied; pn++)
          if (b->nodes[pn].desc.kind == WAA_NODE_PANNER) applied = order_visit(&c, pn);
    }
    if (!applied) break;
    cut[c.breaker] = 1;
  }
  b->n_order = 0;
  for (uint32_t i = c.n_ordered; i-- > 0;)
    if (vtx_in(c.in_cycle, c.n_in_cycle, c.ordered[i]) < 0) b->order[b->n_order++] = c.ordered[i];
  free(cut);
  free(c.marked);
  free(c.temp);
  free(c.ordered);
  free(c.in_cycle);
}

static int default_channel_config(NodeCfg* n, uint32_t n_out) {
  /* per-kind defaults of AudioNodeOptions */
  int cc = 2, mode = WAA_COUNT_MODE_MAX, interp = WAA_INTERP_SPEAKERS;
  switch (n->desc.kind) {
    case WAA_NODE_DESTINATION: /* destination.rs:103-107 */
      cc = (int)n_out;
      mode = WAA_COUNT_MODE_EXPLICIT;
      break;
    case WAA_NODE_CONVOLVER: /* convolver.rs:75-79 */
    case WAA_NODE_STEREO_PANNER: /* stereo_panner.rs:40-44 */
    case WAA_NODE_PANNER: /* panner.rs:168-172 */
      cc = 2;
      mode = WAA_COUNT_MODE_CLAMPED_MAX;
      break;
    default:
      break;
  }
  if (n->desc.channel_count != 0) {
    cc = (int)n->desc.channel_count;
    mode = (int)n->desc.channel_count_mode;
    interp = (int)n->desc.channel_interpretation;
  }
  n->cc = cc;
  n->ccmode = mode;
  n->ccinterp = interp;
  return 0;
}

waa_status orc_batch_create(const waa_graph_desc* g, uint32_t n_inst, uint32_t n_out, uint64_t length, float sr,
                            int32_t device, orc_batch** out) {
  (void)device;
  if (!g || !out || g->n_nodes == 0 || n_inst == 0) return fail(WAA_ERR_INVALID_ARGUMENT, "invalid arguments");
  if (g->nodes[0].kind != WAA_NODE_DESTINATION) return fail(WAA_ERR_INVALID_ARGUMENT, "node 0 must be the destination");
  if (n_out == 0 || n_out > ORC_MAXC)
    return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - Invalid number of channels: %u", n_out);
  if (length == 0) /* assert_valid_buffer_length, src/lib.rs:222-228 */
    return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - Invalid length: 0 is less than or equal to minimum bound (0)");
  if (!(sr >= 3000.f && sr <= 768000.f))  /* MIN/MAX_SAMPLE_RATE, src/lib.rs:149-160 */ /* offline.rs / context mod.rs assert_valid_sample_rate */
    return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - Invalid sample rate: %f", sr);
  orc_batch* b = (orc_batch*)calloc(1, sizeof *b);
  b->n_nodes = g->n_nodes;
  b->n_edges = g->n_edges;
  b->n_inst = n_inst;
  b->n_out = n_out;
  b->length = length;
  b->sr = sr;
  b->n_threads = 1;
  b->nodes = (NodeCfg*)calloc(g->n_nodes, sizeof(NodeCfg));
  b->edge_cap = g->n_edges + 16;
  b->edges = (waa_edge_desc*)malloc(sizeof(waa_edge_desc) * b->edge_cap);
  memcpy(b->edges, g->edges, sizeof(waa_edge_desc) * g->n_edges);
  b->edge_on = (uint32_t*)calloc(b->edge_cap, sizeof(uint32_t));
  b->edge_off = (uint32_t*)malloc(sizeof(uint32_t) * b->edge_cap);
  for (uint32_t e = 0; e < b->edge_cap; e++) b->edge_off[e] = ORC_EDGE_NEVER;
  for (uint32_t e = 0; e < g->n_edges; e++) {
    if (g->edges[e].from >= g->n_nodes || g->edges[e].to >= g->n_nodes || g->edges[e].from_output != 0 ||
        (g->edges[e].to_input != 0 && !(g->edges[e].to_input & 0x80000000u)))
      return fail(WAA_ERR_INVALID_ARGUMENT, "IndexSizeError - invalid edge %u", e);
  }
  for (uint32_t i = 0; i < g->n_nodes; i++) {
    NodeCfg* n = &b->nodes[i];
    n->desc = g->nodes[i];
    if (n->desc.kind >= WAA_NODE_KIND_COUNT) return fail(WAA_ERR_INVALID_ARGUMENT, "unknown node kind");
    default_channel_config(n, n_out);
    if (n->cc < 1 || n->cc > ORC_MAXC)
      return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - Invalid number of channels: %d", n->cc);
    switch (n->desc.kind) {
      case WAA_NODE_BIQUAD: /* biquad_filter.rs:556-594 */
        n->n_params = 4;
        param_init(&n->params[WAA_PARAM_BIQUAD_FREQUENCY], n_inst, 350.f, 0.f, sr / 2.f);
        param_init(&n->params[WAA_PARAM_BIQUAD_DETUNE], n_inst, 0.f, -153600.f, 153600.f);
        param_init(&n->params[WAA_PARAM_BIQUAD_Q], n_inst, 1.f, -FLT_MAX, FLT_MAX);
        param_init(&n->params[WAA_PARAM_BIQUAD_GAIN], n_inst, 0.f, -FLT_MAX, 40.f * log10f(FLT_MAX));
        break;
      case WAA_NODE_GAIN: /* gain.rs:96-103 */
        n->n_params = 1;
        param_init(&n->params[0], n_inst, 1.f, -FLT_MAX, FLT_MAX);
        break;
      case WAA_NODE_BUFFER_SOURCE: /* audio_buffer_source.rs:150-175 */
        n->n_params = 2;
        param_init(&n->params[WAA_PARAM_SOURCE_PLAYBACK_RATE], n_inst, 1.f, -FLT_MAX, FLT_MAX);
        param_init(&n->params[WAA_PARAM_SOURCE_DETUNE], n_inst, 0.f, -FLT_MAX, FLT_MAX);
        n->params[WAA_PARAM_SOURCE_PLAYBACK_RATE].k_rate = 1; /* audio_buffer_source.rs:157,168 */
        n->params[WAA_PARAM_SOURCE_DETUNE].k_rate = 1;
        n->bufs = (Buf*)calloc(n_inst, sizeof(Buf));
        n->start_time = (double*)malloc(sizeof(double) * n_inst);
        n->stop_time = (double*)malloc(sizeof(double) * n_inst);
        n->offset = (double*)calloc(n_inst, sizeof(double));
        n->duration = (double*)malloc(sizeof(double) * n_inst);
        n->is_looping = (int*)calloc(n_inst, sizeof(int));
        n->loop_start = (double*)calloc(n_inst, sizeof(double));
        n->loop_end = (double*)calloc(n_inst, sizeof(double));
        for (uint32_t k = 0; k < n_inst; k++) {
          n->start_time[k] = DBL_MAX;
          n->stop_time[k] = DBL_MAX;
          n->duration[k] = DBL_MAX;
        }
        break;
      case WAA_NODE_CONSTANT_SOURCE: /* constant_source.rs:120-130 */
        n->n_params = 1;
        param_init(&n->params[0], n_inst, 1.f, -FLT_MAX, FLT_MAX);
        n->start_time = (double*)malloc(sizeof(double) * n_inst);
        n->stop_time = (double*)malloc(sizeof(double) * n_inst);
        for (uint32_t k = 0; k < n_inst; k++) {
          n->start_time[k] = DBL_MAX;
          n->stop_time[k] = DBL_MAX;
        }
        break;
      case WAA_NODE_STEREO_PANNER: /* stereo_panner.rs:150-160 */
        n->n_params = 1;
        param_init(&n->params[0], n_inst, 0.f, -1.f, 1.f);
        if (n->ccmode == WAA_COUNT_MODE_MAX)
          return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - StereoPannerNode channel count mode cannot be set to max");
        if (n->cc > 2)
          return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - StereoPannerNode channel count cannot be greater than two");
        break;
      case WAA_NODE_PANNER: { /* panner.rs:390-470 */
        n->n_params = 15;
        static const float defs[15] = {0, 0, 0, 1, 0, 0, /* listener */ 0, 0, 0, 0, 0, -1, 0, 1, 0};
        for (int p = 0; p < 15; p++) param_init(&n->params[p], n_inst, defs[p], -FLT_MAX, FLT_MAX);
        if (n->desc.i[0] == WAA_PANNING_HRTF) {
          n->hrtf = hrir_for_rate((uint32_t)sr);
          if (!n->hrtf)
            return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - HRTF panning needs the HRIR sphere (waa_hrtf_load_sphere)");
        }
        if (n->ccmode == WAA_COUNT_MODE_MAX)
          return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - PannerNode channel count mode cannot be set to max");
        if (n->cc > 2)
          return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - PannerNode channel count cannot be greater than two");
        /* PannerOptions (panner.rs:408-428, 20-33); an all-zero d[] block means "the defaults" (panner.rs:146-166) */
        if (n->desc.d[0] == 0. && n->desc.d[1] == 0. && n->desc.d[2] == 0. && n->desc.d[3] == 0. && n->desc.d[4] == 0. &&
            n->desc.d[5] == 0.) {
          n->desc.d[0] = 1.;
          n->desc.d[1] = 10000.;
          n->desc.d[2] = 1.;
          n->desc.d[3] = 360.;
          n->desc.d[4] = 360.;
        }
        if (!(n->desc.d[0] >= 0.)) return fail(WAA_ERR_INVALID_ARGUMENT, "RangeError - refDistance cannot be negative");
        if (!(n->desc.d[1] > 0.)) return fail(WAA_ERR_INVALID_ARGUMENT, "RangeError - maxDistance must be strictly positive");
        if (!(n->desc.d[2] >= 0.)) return fail(WAA_ERR_INVALID_ARGUMENT, "RangeError - rolloffFactor cannot be negative");
        if (!(n->desc.d[5] >= 0. && n->desc.d[5] <= 1.))
          return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - coneOuterGain must be in the range [0, 1]");
        break;
      }
      case WAA_NODE_OSCILLATOR: { /* oscillator.rs:210-262 */
        if (n->desc.i[0] < WAA_OSC_SINE || n->desc.i[0] > WAA_OSC_CUSTOM) return fail(WAA_ERR_INVALID_ARGUMENT, "bad oscillator type");
        n->n_params = 2;
        param_init(&n->params[WAA_PARAM_OSCILLATOR_FREQUENCY], n_inst, 440.f, -sr / 2.f, sr / 2.f);
        param_init(&n->params[WAA_PARAM_OSCILLATOR_DETUNE], n_inst, 0.f, -153600.f, 153600.f);
        n->start_time = (double*)malloc(sizeof(double) * n_inst);
        n->stop_time = (double*)malloc(sizeof(double) * n_inst);
        for (uint32_t k = 0; k < n_inst; k++) {
          n->start_time[k] = DBL_MAX;
          n->stop_time[k] = DBL_MAX;
        }
        break;
      }
      case WAA_NODE_DELAY: { /* delay.rs:283-335 */
        if (n->desc.d[0] == 0.) n->desc.d[0] = 1.;
        if (!(n->desc.d[0] > 0. && n->desc.d[0] < 180.))
          return fail(WAA_ERR_NOT_SUPPORTED,
                      "NotSupportedError - maxDelayTime MUST be greater than zero and less than three minutes");
        n->n_params = 1;
        param_init(&n->params[0], n_inst, 0.f, 0.f, (float)n->desc.d[0]);
        break;
      }
      case WAA_NODE_WAVESHAPER:
        n->os_factor = n->desc.i[0] == WAA_OVERSAMPLE_X2 ? 2 : n->desc.i[0] == WAA_OVERSAMPLE_X4 ? 4 : 1;
        if (n->os_factor > 1) { /* waveshaper.rs:232-287: chunk 128 up, 128 * R down */
          n->os_up = os_resampler_new(RQ, RQ * n->os_factor);
          n->os_dn = os_resampler_new(RQ * n->os_factor, RQ);
        }
        n->can_propagate_silence = 1;
        break;
      case WAA_NODE_CONVOLVER: /* convolver.rs:195-215 */
        if (n->cc > 2)
          return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - ConvolverNode channel count cannot be greater than two");
        if (n->ccmode == WAA_COUNT_MODE_MAX)
          return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - ConvolverNode channel count mode cannot be set to max");
        break;
      case WAA_NODE_ANALYSER: {
        int fs = n->desc.i[0] ? n->desc.i[0] : 2048;
        if (fs < 32 || fs > MAX_FFT_SIZE || (fs & (fs - 1)))
          return fail(WAA_ERR_INVALID_ARGUMENT, "IndexSizeError - Invalid fft size: %d is not a power of two", fs);
        n->desc.i[0] = fs;
        if (n->desc.d[0] == 0. && n->desc.d[1] == 0. && n->desc.d[2] == 0.) {
          n->desc.d[0] = 0.8;
          n->desc.d[1] = -100.;
          n->desc.d[2] = -30.;
        }
        if (n->desc.d[0] < 0. || n->desc.d[0] > 1.)
          return fail(WAA_ERR_INVALID_ARGUMENT, "IndexSizeError - Invalid smoothing time constant");
        if (!(n->desc.d[1] < n->desc.d[2])) return fail(WAA_ERR_INVALID_ARGUMENT, "IndexSizeError - Invalid min decibels");
        break;
      }
      default:
        break;
    }
  }
  /* ordering */
  b->order = (uint32_t*)malloc(sizeof(uint32_t) * (2 * g->n_nodes + 2));
  order_nodes(b);
  /* state */
  b->st = (NodeState**)calloc(n_inst, sizeof(NodeState*));
  for (uint32_t k = 0; k < n_inst; k++) b->st[k] = (NodeState*)calloc(g->n_nodes, sizeof(NodeState));
  for (uint32_t e = 0; e < g->n_edges; e++) { /* node.connect(&param): src/param.rs:300-320 */
    uint32_t ti = g->edges[e].to_input;
    if (!(ti & 0x80000000u)) continue;
    uint32_t pid = ti & 0x7fffffffu, to = g->edges[e].to;
    NodeCfg* dn = &b->nodes[to];
    if ((int)pid >= dn->n_params) return fail(WAA_ERR_INVALID_ARGUMENT, "IndexSizeError - node %u has no param %u", to, pid);
    uint32_t kind = dn->desc.kind;
    if (!(kind == WAA_NODE_GAIN || kind == WAA_NODE_BIQUAD || kind == WAA_NODE_DELAY || kind == WAA_NODE_STEREO_PANNER ||
          kind == WAA_NODE_CONSTANT_SOURCE || kind == WAA_NODE_OSCILLATOR ||
          (kind == WAA_NODE_BUFFER_SOURCE && (pid == WAA_PARAM_SOURCE_PLAYBACK_RATE || pid == WAA_PARAM_SOURCE_DETUNE)) ||
          /* PannerNode position / orientation (panner.rs:430-449: a-rate AudioParams of the node; the AudioListener's nine
           * params belong to the listener node and stay host values here) */
          (kind == WAA_NODE_PANNER && pid <= WAA_PARAM_PANNER_ORIENTATION_Z)))
      return fail(WAA_ERR_OUT_OF_SCOPE, "audio-rate modulation of a host-evaluated param (node %u) is out of scope", to);
    for (uint32_t k = 0; k < n_inst; k++)
      if (!b->st[k][to].pin[pid]) {
        b->st[k][to].pin[pid] = (Quantum*)malloc(sizeof(Quantum));
        q_make_silent(b->st[k][to].pin[pid]);
      }
  }
  b->out = (float*)calloc((size_t)n_inst * n_out * (length ? length : 1), sizeof(float));
  prefault(b->out, (size_t)n_inst * n_out * (length ? length : 1) * sizeof(float));
  *out = b;
  return WAA_OK;
}

static void buf_release(Buf* bf) {
  if (!bf->refcnt) return;
  if (--*bf->refcnt == 0) {
    for (uint32_t c = 0; c < bf->n_ch; c++) free(bf->ch[c]);
    free(bf->ch);
    free(bf->refcnt);
  }
  memset(bf, 0, sizeof *bf);
}

/* waa_device_arena_reserve: a device-memory placement aid of the product library; nothing to do on the CPU */
waa_status orc_device_arena_reserve(int32_t device, uint64_t bytes) {
  (void)device;
  (void)bytes;
  return WAA_OK;
}
waa_status orc_device_arena_reserve_graded(int32_t device, uint64_t bytes, uint64_t candidate_bytes) {
  (void)device; (void)bytes; (void)candidate_bytes;
  return WAA_OK;
}
waa_status orc_device_arena_grades(int32_t device, waa_arena_grades* out, float* unit_ms, uint32_t capacity) {
  (void)device; (void)unit_ms; (void)capacity;
  if (out) memset(out, 0, sizeof *out);
  return WAA_OK;
}
waa_status orc_device_arena_stats(int32_t device, waa_arena_stats* out) {
  (void)device;
  if (!out) return WAA_ERR_INVALID_ARGUMENT;
  memset(out, 0, sizeof *out);
  return WAA_OK;
}
void orc_batch_destroy(orc_batch* b) {
  if (!b) return;
  for (uint32_t k = 0; k < b->n_inst; k++) {
    for (uint32_t i = 0; i < b->n_nodes; i++) {
      NodeState* s = &b->st[k][i];
      for (int c = 0; c < 4; c++) convstate_free(s->conv[c]);
      free(s->ring);
      free(s->dl_ring);
      for (int p = 0; p < WAA_MAX_PARAMS; p++) free(s->pin[p]);
      free(s->last_fft_output);
      free(s->os_up_ovl);
      free(s->os_dn_ovl);
      free(s->hrtf_prev);
    }
    free(b->st[k]);
  }
  free(b->st);
  for (uint32_t i = 0; i < b->n_nodes; i++) {
    NodeCfg* n = &b->nodes[i];
    for (int p = 0; p < n->n_params; p++) {
      for (uint32_t k = 0; k < b->n_inst; k++)
        if (n->params[p].blk[k].owned) free(n->params[p].blk[k].v);
      free(n->params[p].cst);
      free(n->params[p].blk);
      if (n->params[p].tl) {
        for (uint32_t k = 0; k < b->n_inst; k++) orc_timeline_destroy(n->params[p].tl[k]);
        free(n->params[p].tl);
        free(n->params[p].tl_vals);
        free(n->params[p].tl_vlen);
      }
    }
    if (n->bufs) {
      for (uint32_t k = 0; k < b->n_inst; k++) buf_release(&n->bufs[k]);
      free(n->bufs);
    }
    free(n->start_time);
    free(n->msg_started);
    free(n->stop_time);
    free(n->offset);
    free(n->duration);
    free(n->is_looping);
    free(n->loop_start);
    free(n->loop_end);
    for (int c = 0; c < 4; c++) convir_free(n->conv_ir[c]);
    free(n->curve);
    free(n->osc_wave);
    os_resampler_free(n->os_up);
    os_resampler_free(n->os_dn);
  }
  free(b->nodes);
  free(b->edges);
  free(b->order);
  free(b->edge_on);
  free(b->edge_off);
  for (uint32_t k = 0; k < b->n_msgs; k++) free(b->msgs[k].curve);
  free(b->msgs);
  for (uint32_t k = 0; k < b->n_epochs; k++) {
    free(b->epochs[k].active);
    free(b->epochs[k].order);
  }
  free(b->epochs);
  free(b->out);
  free(b->dbg_codes);
  free(b);
}

static int check_node(orc_batch* b, uint32_t node, uint32_t kind) {
  if (!b) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch");
  if (node >= b->n_nodes || b->nodes[node].desc.kind != kind)
    return fail(WAA_ERR_INVALID_ARGUMENT, "node %u is not of the expected kind", node);
  return 0;
}
static int check_inst(orc_batch* b, uint32_t inst) {
  if (inst != WAA_ALL_INSTANCES && inst >= b->n_inst) return fail(WAA_ERR_INVALID_ARGUMENT, "instance out of range");
  return 0;
}

static Buf buf_make(const float* const* channels, uint32_t n_ch, uint64_t frames, float sr) {
  Buf bf;
  bf.n_ch = n_ch;
  bf.frames = frames;
  bf.sr = sr;
  bf.ch = (float**)malloc(sizeof(float*) * n_ch);
  for (uint32_t c = 0; c < n_ch; c++) {
    bf.ch[c] = (float*)malloc(sizeof(float) * (frames ? frames : 1));
    memcpy(bf.ch[c], channels[c], sizeof(float) * frames);
  }
  bf.refcnt = (int*)malloc(sizeof(int));
  *bf.refcnt = 0;
  return bf;
}

waa_status orc_source_set_buffer(orc_batch* b, uint32_t node, uint32_t inst, const float* const* channels,
                                 uint32_t n_ch, uint64_t frames, float sr) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_BUFFER_SOURCE)) || (e = check_inst(b, inst))) return e;
  if (n_ch == 0 || n_ch > ORC_MAXC) return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - Invalid number of channels");
  NodeCfg* n = &b->nodes[node];
  Buf bf = buf_make(channels, n_ch, frames, sr);
  uint32_t lo = inst == WAA_ALL_INSTANCES ? 0 : inst, hi = inst == WAA_ALL_INSTANCES ? b->n_inst : inst + 1;
  for (uint32_t k = lo; k < hi; k++) {
    buf_release(&n->bufs[k]);
    n->bufs[k] = bf;
    ++*bf.refcnt;
  }
  return WAA_OK;
}
waa_status orc_source_set_buffer_batch(orc_batch* b, uint32_t node, const float* data, uint32_t n_ch, uint64_t frames,
                                       float sr) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_BUFFER_SOURCE))) return e;
  const float* chans[ORC_MAXC];
  if (n_ch == 0 || n_ch > ORC_MAXC) return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - Invalid number of channels");
  for (uint32_t k = 0; k < b->n_inst; k++) {
    for (uint32_t c = 0; c < n_ch; c++) chans[c] = data + ((size_t)k * n_ch + c) * frames;
    if ((e = orc_source_set_buffer(b, node, k, chans, n_ch, frames, sr))) return e;
  }
  return WAA_OK;
}
waa_status orc_source_adopt_device(orc_batch* b, uint32_t node, const float* d, uint32_t n_ch, uint64_t frames, float sr) {
  return orc_source_set_buffer_batch(b, node, d, n_ch, frames, sr); /* host pointer for the oracle */
}
waa_status orc_source_start(orc_batch* b, uint32_t node, uint32_t inst, double when, double offset, double duration) {
  int e;
  if (!b || node >= b->n_nodes) return fail(WAA_ERR_INVALID_ARGUMENT, "bad node");
  uint32_t kind = b->nodes[node].desc.kind;
  if (kind != WAA_NODE_BUFFER_SOURCE && kind != WAA_NODE_CONSTANT_SOURCE && kind != WAA_NODE_OSCILLATOR)
    return fail(WAA_ERR_INVALID_ARGUMENT, "node %u is not a scheduled source", node);
  if ((e = check_inst(b, inst))) return e;
  if (!(when >= 0.) || !(offset >= 0.) || !(duration >= 0.)) /* scheduled_source.rs assert_valid_time_value */
    return fail(WAA_ERR_INVALID_ARGUMENT, "RangeError - timing value should be finite and positive");
  NodeCfg* n = &b->nodes[node];
  uint32_t lo = inst == WAA_ALL_INSTANCES ? 0 : inst, hi = inst == WAA_ALL_INSTANCES ? b->n_inst : inst + 1;
  if (b->ctl_q > 0) { /* at a suspend point: a control message (the renderer's times change when it is handled) */
    if (!n->msg_started) n->msg_started = (unsigned char*)calloc(b->n_inst, 1);
    for (uint32_t k = lo; k < hi; k++) {
      if (n->start_time[k] != DBL_MAX || n->msg_started[k]) return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - Cannot call `start` twice");
      n->msg_started[k] = 1;
    }
    CtlMsg m;
    memset(&m, 0, sizeof m);
    m.kind = CTL_START;
    m.node = node;
    m.inst = inst;
    m.t = when;
    m.offset = offset;
    m.duration = duration;
    ctl_push(b, m);
    return WAA_OK;
  }
  for (uint32_t k = lo; k < hi; k++) {
    if (n->start_time[k] != DBL_MAX) return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - Cannot call `start` twice");
    n->start_time[k] = when;
    if (kind == WAA_NODE_BUFFER_SOURCE) {
      n->offset[k] = offset;
      n->duration[k] = duration;
    }
  }
  return WAA_OK;
}
waa_status orc_source_stop(orc_batch* b, uint32_t node, uint32_t inst, double when) {
  int e;
  if (!b || node >= b->n_nodes) return fail(WAA_ERR_INVALID_ARGUMENT, "bad node");
  uint32_t kind = b->nodes[node].desc.kind;
  if (kind != WAA_NODE_BUFFER_SOURCE && kind != WAA_NODE_CONSTANT_SOURCE && kind != WAA_NODE_OSCILLATOR)
    return fail(WAA_ERR_INVALID_ARGUMENT, "node %u is not a scheduled source", node);
  if ((e = check_inst(b, inst))) return e;
  if (!(when >= 0.)) return fail(WAA_ERR_INVALID_ARGUMENT, "RangeError - timing value should be finite and positive");
  NodeCfg* n = &b->nodes[node];
  uint32_t lo = inst == WAA_ALL_INSTANCES ? 0 : inst, hi = inst == WAA_ALL_INSTANCES ? b->n_inst : inst + 1;
  if (b->ctl_q > 0) {
    for (uint32_t k = lo; k < hi; k++)
      if (n->start_time[k] == DBL_MAX && !(n->msg_started && n->msg_started[k]))
        return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - Cannot stop before start");
    CtlMsg m;
    memset(&m, 0, sizeof m);
    m.kind = CTL_STOP;
    m.node = node;
    m.inst = inst;
    m.t = when;
    ctl_push(b, m);
    return WAA_OK;
  }
  for (uint32_t k = lo; k < hi; k++) {
    if (n->start_time[k] == DBL_MAX)
      return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - Cannot stop before start");
    n->stop_time[k] = when;
  }
  return WAA_OK;
}
waa_status orc_source_set_loop(orc_batch* b, uint32_t node, uint32_t inst, int32_t looping, double ls, double le) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_BUFFER_SOURCE)) || (e = check_inst(b, inst))) return e;
  NodeCfg* n = &b->nodes[node];
  uint32_t lo = inst == WAA_ALL_INSTANCES ? 0 : inst, hi = inst == WAA_ALL_INSTANCES ? b->n_inst : inst + 1;
  for (uint32_t k = lo; k < hi; k++) {
    n->is_looping[k] = looping;
    n->loop_start[k] = ls;
    n->loop_end[k] = le;
  }
  return WAA_OK;
}

/* convolver.rs:16-53 normalize_buffer */
static float normalize_buffer(const float* const* ch, uint32_t n_ch, uint64_t len, float sr) {
  const float gain_calibration = 0.00125f, gain_calibration_sample_rate = 44100.f, min_power = 0.000125f;
  float power = 0.f;
  for (uint32_t c = 0; c < n_ch; c++) {
    float s = 0.f;
    for (uint64_t i = 0; i < len; i++) s += ch[c][i] * ch[c][i];
    power += s;
  }
  power = sqrtf(power / (float)(n_ch * len));
  if (!isfinite(power) || isnan(power) || power < min_power) power = min_power;
  float scale = 1.f / power;
  scale *= gain_calibration;
  scale *= gain_calibration_sample_rate / sr;
  if (n_ch == 4) scale *= 0.5f;
  return scale;
}
float orc_convolver_normalization_scale(const float* const* ch, uint32_t n_ch, uint64_t len, float sr) {
  return normalize_buffer(ch, n_ch, len, sr);
}

/* convolver.rs:259-317 set_buffer */
waa_status orc_convolver_set_buffer(orc_batch* b, uint32_t node, const float* const* channels, uint32_t n_ch,
                                    uint64_t frames, float sr) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_CONVOLVER))) return e;
  if (sr != b->sr)
    return fail(WAA_ERR_NOT_SUPPORTED,
                "NotSupportedError - sample rate of the convolution buffer must match the audio context");
  if (!(n_ch == 1 || n_ch == 2 || n_ch == 4))
    return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - the convolution buffer must consist of 1, 2 or 4 channels");
  NodeCfg* n = &b->nodes[node];
  float scale = n->desc.i[0] ? 1.f : normalize_buffer(channels, n_ch, frames, sr);
  for (int c = 0; c < 4; c++) {
    convir_free(n->conv_ir[c]);
    n->conv_ir[c] = NULL;
  }
  uint32_t ncv = n_ch > 2 ? n_ch : 2;
  float* scaled = (float*)malloc(sizeof(float) * (frames ? frames : 1));
  for (uint32_t idx = 0; idx < ncv; idx++) {
    uint32_t c = idx < n_ch - 1 ? idx : n_ch - 1;
    for (uint64_t i = 0; i < frames; i++) scaled[i] = channels[c][i] * scale;
    n->conv_ir[idx] = convir_new(RQ * 8, scaled, frames);
  }
  free(scaled);
  n->n_conv = (int)ncv;
  n->impulse_length = frames;
  n->impulse_channels = (int)n_ch;
  n->has_ir = 1;
  for (uint32_t k = 0; k < b->n_inst; k++) {
    NodeState* s = &b->st[k][node];
    for (int c = 0; c < 4; c++) {
      convstate_free(s->conv[c]);
      s->conv[c] = NULL;
    }
    for (uint32_t c = 0; c < ncv; c++) s->conv[c] = convstate_new(n->conv_ir[c]);
  }
  return WAA_OK;
}

/* waveshaper.rs:489-509 */
/* BaseAudioContext::decode_audio_data_sync (context/base.rs:68-73 -> decoding.rs:15-54) for input that decodes to
 * 16-bit PCM: symphonia's i16 -> f32 conversion (third party; restated: sample / 32768), then AudioBuffer::resample to
 * the context's rate (buffer.rs:311-363).  Returns planes [n_ch][*target] (malloc). */
uint64_t orc_buffer_resample(const float* src, uint64_t frames, float source_sr, float target_sr, float* dst, uint64_t cap);
static float* decode_pcm16(const int16_t* pcm, uint32_t n_ch, uint64_t frames, float src_sr, float ctx_sr, uint64_t* target) {
  float* plane = (float*)calloc(frames ? frames : 1, sizeof(float));
  *target = orc_buffer_resample(plane, frames, src_sr, ctx_sr, NULL, 0);
  float* out = (float*)malloc(sizeof(float) * (size_t)n_ch * (*target ? *target : 1));
  for (uint32_t c = 0; c < n_ch; c++) {
    for (uint64_t i = 0; i < frames; i++) plane[i] = (float)pcm[i * n_ch + c] / 32768.f;
    orc_buffer_resample(plane, frames, src_sr, ctx_sr, out + (size_t)c * *target, *target);
  }
  free(plane);
  return out;
}
waa_status orc_source_set_buffer_pcm16(orc_batch* b, uint32_t node, uint32_t inst, const int16_t* interleaved, uint32_t n_ch,
                                       uint64_t frames, float sr) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_BUFFER_SOURCE)) || (e = check_inst(b, inst))) return e;
  if (n_ch == 0 || n_ch > ORC_MAXC) return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - Invalid number of channels");
  if (!(sr >= 3000.f && sr <= 768000.f)) return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - Invalid sample rate: %f", sr);
  uint64_t target = 0;
  float* planes = decode_pcm16(interleaved, n_ch, frames, sr, b->sr, &target);
  const float* chans[ORC_MAXC];
  for (uint32_t c = 0; c < n_ch; c++) chans[c] = planes + (size_t)c * target;
  e = orc_source_set_buffer(b, node, inst, chans, n_ch, target, b->sr);
  free(planes);
  return e;
}
waa_status orc_source_set_buffer_pcm16_batch(orc_batch* b, uint32_t node, const int16_t* data, uint32_t n_ch, uint64_t frames,
                                             float sr) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_BUFFER_SOURCE))) return e;
  for (uint32_t k = 0; k < b->n_inst; k++)
    if ((e = orc_source_set_buffer_pcm16(b, node, k, data + (size_t)k * frames * n_ch, n_ch, frames, sr))) return e;
  return WAA_OK;
}
waa_status orc_convolver_set_buffer(orc_batch* b, uint32_t node, const float* const* channels, uint32_t n_ch, uint64_t frames,
                                    float sr);
waa_status orc_convolver_set_buffer_pcm16(orc_batch* b, uint32_t node, const int16_t* interleaved, uint32_t n_ch, uint64_t frames,
                                          float sr) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_CONVOLVER))) return e;
  if (!(n_ch == 1 || n_ch == 2 || n_ch == 4))
    return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - the convolution buffer must consist of 1, 2 or 4 channels");
  if (!(sr >= 3000.f && sr <= 768000.f)) return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - Invalid sample rate: %f", sr);
  uint64_t target = 0;
  float* planes = decode_pcm16(interleaved, n_ch, frames, sr, b->sr, &target);
  const float* chans[4];
  for (uint32_t c = 0; c < n_ch; c++) chans[c] = planes + (size_t)c * target;
  e = orc_convolver_set_buffer(b, node, chans, n_ch, target, b->sr);
  free(planes);
  return e;
}

waa_status orc_waveshaper_set_curve(orc_batch* b, uint32_t node, const float* curve, uint32_t nn) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_WAVESHAPER))) return e;
  NodeCfg* n = &b->nodes[node];
  if (n->has_curve) return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - cannot assign curve twice");
  n->curve = (float*)malloc(sizeof(float) * (nn ? nn : 1));
  memcpy(n->curve, curve, sizeof(float) * nn);
  n->curve_n = nn;
  n->has_curve = 1;
  if (nn == 0) {
    n->can_propagate_silence = 1; /* apply_curve returns 0 for an empty curve */
  } else if (nn % 2 == 1) {
    n->can_propagate_silence = fabsf(curve[nn / 2]) < 1e-9f;
  } else {
    float a = curve[nn / 2 - 1], c = curve[nn / 2];
    n->can_propagate_silence = fabsf((a + c) / 2.f) < 1e-9f;
  }
  return WAA_OK;
}

/* iir_filter.rs:17-46 (validation), :273-311 (IirFilterRenderer::new: pad to equal length, normalise by a0) */
waa_status orc_iir_set_coefficients(orc_batch* b, uint32_t node, const double* ff, uint32_t nff, const double* fb,
                                    uint32_t nfb) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_IIR_FILTER))) return e;
  if (!ff || nff == 0 || nff > WAA_MAX_IIR_COEFFS)
    return fail(WAA_ERR_NOT_SUPPORTED,
                "NotSupportedError - IIR Filter feedforward coefficients should have length >= 0 and <= %d", WAA_MAX_IIR_COEFFS);
  int all_zero = 1;
  for (uint32_t i = 0; i < nff; i++) all_zero &= ff[i] == 0.;
  if (all_zero) return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - IIR Filter feedforward coefficients cannot be all zeros");
  if (!fb || nfb == 0 || nfb > WAA_MAX_IIR_COEFFS)
    return fail(WAA_ERR_NOT_SUPPORTED,
                "NotSupportedError - IIR Filter feedback coefficients should have length >= 0 and <= %d", WAA_MAX_IIR_COEFFS);
  if (fb[0] == 0.) return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - IIR Filter feedback first coefficient cannot be zero");
  NodeCfg* n = &b->nodes[node];
  uint32_t len = nff > nfb ? nff : nfb;
  double a0 = fb[0];
  for (uint32_t i = 0; i < len; i++) {
    n->iir_b[i] = (i < nff ? ff[i] : 0.) / a0;
    n->iir_a[i] = (i < nfb ? fb[i] : 0.) / a0;
  }
  n->iir_len = (int)len;
  return WAA_OK;
}

/* periodic_wave.rs:88-190 + oscillator.rs:318-321 */
waa_status orc_oscillator_set_periodic_wave(orc_batch* b, uint32_t node, const float* real, const float* imag, uint32_t nn,
                                            int32_t disable_normalization) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_OSCILLATOR))) return e;
  if ((!real && !imag) || nn < 2) return fail(WAA_ERR_INVALID_ARGUMENT, "IndexSizeError - `real` and `imag` length should at least 2");
  NodeCfg* n = &b->nodes[node];
  const int size = 8192;
  float* wavetable = (float*)malloc(sizeof(float) * size);
  const float pi_2 = 2.f * 3.14159265358979323846f;
  for (int i = 0; i < size; i++) {
    float sample = 0.f;
    float phase = pi_2 * (float)i / (float)size;
    for (uint32_t j = 1; j < nn; j++) {
      float freq = (float)j;
      float re = real ? real[j] : 0.f, im = imag ? imag[j] : 0.f;
      float rad = phase * freq;
      float contrib = re * cosf(rad) + im * sinf(rad);
      sample += contrib;
    }
    wavetable[i] = sample;
  }
  if (!disable_normalization) {
    float max = 0.f;
    for (int i = 0; i < size; i++) {
      float a = fabsf(wavetable[i]);
      if (a > max) max = a;
    }
    if (max > 0.f) {
      float norm_factor = 1.f / max;
      for (int i = 0; i < size; i++) wavetable[i] *= norm_factor;
    }
  }
  free(n->osc_wave);
  n->osc_wave = wavetable;
  return WAA_OK;
}

/* the finished table (oscillator.rs:487-493) */
waa_status orc_oscillator_set_wavetable(orc_batch* b, uint32_t node, const float* table, uint32_t n) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_OSCILLATOR))) return e;
  if (!table || n != WAA_PERIODIC_WAVE_TABLE_LENGTH)
    return fail(WAA_ERR_INVALID_ARGUMENT, "IndexSizeError - a PeriodicWave table has %d points (got %u)", WAA_PERIODIC_WAVE_TABLE_LENGTH, n);
  NodeCfg* nd = &b->nodes[node];
  float* copy = (float*)malloc(sizeof(float) * n);
  memcpy(copy, table, sizeof(float) * n);
  free(nd->osc_wave);
  nd->osc_wave = copy;
  return WAA_OK;
}

/* AudioParam::set_value_at_time & co. (param.rs:428-596) on a param of the batch */
waa_status orc_param_schedule_event(orc_batch* b, uint32_t node, uint32_t param, uint32_t inst, int32_t type, float value,
                                    double time, double aux, const float* curve, uint32_t n_curve) {
  int e;
  if (!b || node >= b->n_nodes || (int)param >= b->nodes[node].n_params)
    return fail(WAA_ERR_INVALID_ARGUMENT, "no such param %u on node %u", param, node);
  if ((e = check_inst(b, inst))) return e;
  Param* p = &b->nodes[node].params[param];
  if (!p->tl) {
    p->tl = (orc_timeline**)calloc(b->n_inst, sizeof(orc_timeline*));
    p->tl_vals = (float*)calloc((size_t)b->n_inst * RQ, sizeof(float));
    p->tl_vlen = (int*)calloc(b->n_inst, sizeof(int));
  }
  p->sample_rate = (double)b->sr;
  uint32_t lo = inst == WAA_ALL_INSTANCES ? 0 : inst, hi = inst == WAA_ALL_INSTANCES ? b->n_inst : inst + 1;
  for (uint32_t k = lo; k < hi; k++) {
    if (!p->tl[k]) {
      p->tl[k] = orc_timeline_create(p->defv, p->minv, p->maxv, !p->k_rate);
      /* the node constructor's `param.set_value(options.x)` (e.g. gain.rs:117) */
      if ((e = orc_timeline_event(p->tl[k], WAA_EVENT_SET_VALUE, p->cst[k], 0., 0., NULL, 0))) return e;
    }
    if (b->ctl_q > 0) continue; /* (a control message, below) */
    if ((e = orc_timeline_event(p->tl[k], type, value, time, aux, curve, n_curve))) return e;
  }
  if (b->ctl_q > 0) {
    { /* the control-side assertions now, on a scratch timeline (only argument checks can fire) */
      orc_timeline* probe = orc_timeline_create(p->defv, p->minv, p->maxv, !p->k_rate);
      e = orc_timeline_event(probe, type, value, time, aux, curve, n_curve);
      orc_timeline_destroy(probe);
      if (e) return e;
    }
    CtlMsg m;
    memset(&m, 0, sizeof m);
    m.kind = CTL_EVENT;
    m.node = node;
    m.param = param;
    m.inst = inst;
    m.type = type;
    m.value = value;
    m.t = time;
    m.aux = aux;
    if (curve && n_curve) {
      m.curve = (float*)malloc(sizeof(float) * n_curve);
      memcpy(m.curve, curve, sizeof(float) * n_curve);
      m.n_curve = n_curve;
    }
    ctl_push(b, m);
  }
  return WAA_OK;
}

waa_status orc_set_param_const(orc_batch* b, uint32_t node, uint32_t param, uint32_t inst, float value) {
  int e;
  if (!b || node >= b->n_nodes || (int)param >= b->nodes[node].n_params)
    return fail(WAA_ERR_INVALID_ARGUMENT, "no such param %u on node %u", param, node);
  if ((e = check_inst(b, inst))) return e;
  Param* p = &b->nodes[node].params[param];
  uint32_t lo = inst == WAA_ALL_INSTANCES ? 0 : inst, hi = inst == WAA_ALL_INSTANCES ? b->n_inst : inst + 1;
  if (b->ctl_q > 0) /* AudioParam::set_value from a suspend callback: a SetValue event handled in front of that quantum */
    return orc_param_schedule_event(b, node, param, inst, WAA_EVENT_SET_VALUE, value, 0., 0., NULL, 0);
  for (uint32_t k = lo; k < hi; k++) {
    p->cst[k] = value;
    /* AudioParam::set_value after automation methods is one more SetValue event (param.rs:392-415) */
    if (p->tl && p->tl[k] && (e = orc_timeline_event(p->tl[k], WAA_EVENT_SET_VALUE, value, 0., 0., NULL, 0))) return e;
  }
  return WAA_OK;
}
waa_status orc_set_param_block(orc_batch* b, uint32_t node, uint32_t param, uint32_t inst, uint64_t q0, uint32_t nq,
                               uint32_t vpq, const float* values) {
  int e;
  if (!b || node >= b->n_nodes || (int)param >= b->nodes[node].n_params)
    return fail(WAA_ERR_INVALID_ARGUMENT, "no such param %u on node %u", param, node);
  if ((e = check_inst(b, inst))) return e;
  if (vpq != 1 && vpq != RQ) return fail(WAA_ERR_INVALID_ARGUMENT, "values_per_quantum must be 1 or 128");
  Param* p = &b->nodes[node].params[param];
  float* v = (float*)malloc(sizeof(float) * (size_t)nq * vpq);
  memcpy(v, values, sizeof(float) * (size_t)nq * vpq);
  uint32_t lo = inst == WAA_ALL_INSTANCES ? 0 : inst, hi = inst == WAA_ALL_INSTANCES ? b->n_inst : inst + 1;
  /* a block set for ALL is shared; the first instance of the range owns the allocation.
   * (re-setting a shared block is not supported by the oracle: tests set each param once) */
  for (uint32_t k = lo; k < hi; k++) {
    if (p->blk[k].owned && inst != WAA_ALL_INSTANCES) free(p->blk[k].v);
    p->blk[k].q0 = q0;
    p->blk[k].nq = nq;
    p->blk[k].vpq = vpq;
    p->blk[k].v = v;
    p->blk[k].owned = (k == lo);
  }
  return WAA_OK;
}

/* ------------------------------------------------------------------------------------ */
/* biquad coefficients (src/node/biquad_filter.rs:28-373)                                 */
/* ------------------------------------------------------------------------------------ */
typedef struct {
  double b0, b1, b2, a1, a2;
} Coefs;
static Coefs coefs_raw(double b0, double b1, double b2, double a1, double a2) {
  Coefs c = {b0, b1, b2, a1, a2};
  return c;
}
static Coefs normalize_coefs(double b0, double b1, double b2, double a0, double a1, double a2) { /* :28-38 */
  double scale = 1. / a0;
  return coefs_raw(b0 * scale, b1 * scale, b2 * scale, a1 * scale, a2 * scale);
}
static Coefs lowpass_coefs(double freq, double q) { /* :40-66 */
  if (freq == 1.) return coefs_raw(1., 0., 0., 0., 0.);
  double w0 = M_PI * freq;
  double alpha = sin(w0) / (2. * pow(10., q / 20.));
  double cw = cos(w0);
  double beta = (1. - cw) / 2.;
  return normalize_coefs(beta, 2. * beta, beta, 1. + alpha, -2. * cw, 1. - alpha);
}
static Coefs highpass_coefs(double freq, double q) { /* :68-104 */
  if (freq == 1.) return coefs_raw(0., 0., 0., 0., 0.);
  if (freq == 0.) return coefs_raw(1., 0., 0., 0., 0.);
  double w0 = M_PI * freq;
  double alpha = sin(w0) / (2. * pow(10., q / 20.));
  double cw = cos(w0);
  double beta = (1. + cw) / 2.;
  return normalize_coefs(beta, -2. * beta, beta, 1. + alpha, -2. * cw, 1. - alpha);
}
static Coefs bandpass_coefs(double freq, double q) { /* :106-143 */
  if (freq > 0. && freq < 1.) {
    if (q > 0.) {
      double w0 = M_PI * freq;
      double alpha = sin(w0) / (2. * q);
      double cw = cos(w0);
      return normalize_coefs(alpha, 0., -alpha, 1. + alpha, -2. * cw, 1. - alpha);
    }
    return coefs_raw(1., 0., 0., 0., 0.);
  }
  return coefs_raw(0., 0., 0., 0., 0.);
}
static Coefs notch_coefs(double freq, double q) { /* :145-181 */
  if (freq > 0. && freq < 1.) {
    if (q > 0.) {
      double w0 = M_PI * freq;
      double alpha = sin(w0) / (2. * q);
      double cw = cos(w0);
      return normalize_coefs(1., -2. * cw, 1., 1. + alpha, -2. * cw, 1. - alpha);
    }
    return coefs_raw(0., 0., 0., 0., 0.);
  }
  return coefs_raw(1., 0., 0., 0., 0.);
}
static Coefs allpass_coefs(double freq, double q) { /* :183-217 */
  if (freq > 0. && freq < 1.) {
    if (q > 0.) {
      double w0 = M_PI * freq;
      double alpha = sin(w0) / (2. * q);
      double cw = cos(w0);
      return normalize_coefs(1. - alpha, -2. * cw, 1. + alpha, 1. + alpha, -2. * cw, 1. - alpha);
    }
    return coefs_raw(-1., 0., 0., 0., 0.);
  }
  return coefs_raw(1., 0., 0., 0., 0.);
}
static Coefs peaking_coefs(double freq, double q, double gain) { /* :219-259 */
  double A = pow(10., gain / 40.);
  if (freq > 0. && freq < 1.) {
    if (q > 0.) {
      double w0 = M_PI * freq;
      double alpha = sin(w0) / (2. * q);
      double cw = cos(w0);
      return normalize_coefs(1. + alpha * A, -2. * cw, 1. - alpha * A, 1. + alpha / A, -2. * cw, 1. - alpha / A);
    }
    return coefs_raw(A * A, 0., 0., 0., 0.);
  }
  return coefs_raw(1., 0., 0., 0., 0.);
}
static Coefs lowshelf_coefs(double freq, double gain) { /* :261-300 */
  double A = pow(10., gain / 40.);
  if (freq == 1.) return coefs_raw(A * A, 0., 0., 0., 0.);
  if (freq == 0.) return coefs_raw(1., 0., 0., 0., 0.);
  double w0 = M_PI * freq;
  double cw = cos(w0);
  double alpha_s = sin(w0) / 2. * M_SQRT2;
  double k = 2. * alpha_s * sqrt(A);
  double ap = A + 1., am = A - 1.;
  return normalize_coefs(A * (ap - am * cw + k), 2. * A * (am - ap * cw), A * (ap - am * cw - k), ap + am * cw + k,
                         -2. * (am + ap * cw), ap + am * cw - k);
}
static Coefs highshelf_coefs(double freq, double gain) { /* :302-341 */
  double A = pow(10., gain / 40.);
  if (freq == 1.) return coefs_raw(1., 0., 0., 0., 0.);
  if (freq > 0.) {
    double w0 = M_PI * freq;
    double cw = cos(w0);
    double alpha_s = sin(w0) / 2. * M_SQRT2;
    double k = 2. * alpha_s * sqrt(A);
    double ap = A + 1., am = A - 1.;
    return normalize_coefs(A * (ap + am * cw + k), -2. * A * (am + ap * cw), A * (ap + am * cw - k), ap - am * cw + k,
                           2. * (am - ap * cw), ap - am * cw - k);
  }
  return coefs_raw(A * A, 0., 0., 0., 0.);
}
static Coefs calculate_coefs(int type, double sample_rate, double f0, double gain, double q) { /* :343-364 */
  double nyquist = sample_rate / 2.;
  double nf = f0 / nyquist;
  nf = nf < 0. ? 0. : nf > 1. ? 1. : nf;
  switch (type) {
    case WAA_BIQUAD_LOWPASS: return lowpass_coefs(nf, q);
    case WAA_BIQUAD_HIGHPASS: return highpass_coefs(nf, q);
    case WAA_BIQUAD_BANDPASS: return bandpass_coefs(nf, q);
    case WAA_BIQUAD_NOTCH: return notch_coefs(nf, q);
    case WAA_BIQUAD_ALLPASS: return allpass_coefs(nf, q);
    case WAA_BIQUAD_PEAKING: return peaking_coefs(nf, q, gain);
    case WAA_BIQUAD_LOWSHELF: return lowshelf_coefs(nf, gain);
    default: return highshelf_coefs(nf, gain);
  }
}
static float get_computed_freq(float freq, float detune) { /* :367-373 (f32 exp2) */
  if (detune != 0.f) return freq * exp2f(detune / 1200.f);
  return freq;
}

/* biquad_filter.rs:670-735 get_frequency_response */
waa_status orc_biquad_frequency_response(int32_t type, float sample_rate, float frequency, float detune, float q,
                                         float gain, const float* hz, float* mag, float* phase, uint32_t n) {
  if (type < 0 || type > 7) return fail(WAA_ERR_INVALID_ARGUMENT, "bad filter type");
  float nyq = sample_rate / 2.f;
  float cf = get_computed_freq(frequency, detune);
  Coefs c = calculate_coefs(type, (double)sample_rate, (double)cf, (double)gain, (double)q);
  for (uint32_t i = 0; i < n; i++) {
    float f = hz[i];
    if (f < 0.f || f > nyq) {
      mag[i] = NAN;
      phase[i] = NAN;
      continue;
    }
    float fn = f / nyq;
    double omega = -M_PI * (double)fn;
    double zr = cos(omega), zi = sin(omega);
    /* numerator = b0 + (b1 + b2*z)*z */
    double tr = c.b1 + c.b2 * zr, ti = c.b2 * zi;
    double nr = c.b0 + (tr * zr - ti * zi), ni = tr * zi + ti * zr;
    double ur = c.a1 + c.a2 * zr, ui = c.a2 * zi;
    double dr = 1. + (ur * zr - ui * zi), di = ur * zi + ui * zr;
    double den = dr * dr + di * di;
    double rr = (nr * dr + ni * di) / den, ri = (ni * dr - nr * di) / den;
    mag[i] = (float)hypot(rr, ri);
    phase[i] = (float)atan2(ri, rr);
  }
  return WAA_OK;
}


/* when `ended` was dispatched for a scheduled source (after orc_render) */
waa_status orc_source_ended(orc_batch* b, uint32_t node, uint32_t inst, int64_t* quantum) {
  if (!b || node >= b->n_nodes || inst >= b->n_inst || !quantum) return fail(WAA_ERR_INVALID_ARGUMENT, "bad node / instance");
  uint32_t kind = b->nodes[node].desc.kind;
  if (kind != WAA_NODE_BUFFER_SOURCE && kind != WAA_NODE_CONSTANT_SOURCE && kind != WAA_NODE_OSCILLATOR)
    return fail(WAA_ERR_INVALID_ARGUMENT, "not a scheduled source");
  if (!b->rendered) return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - nothing rendered yet");
  *quantum = b->st[inst][node].ended_q;
  return WAA_OK;
}
/* iir_filter.rs:218-262 */
waa_status orc_iir_frequency_response(const double* ff, uint32_t nff, const double* fb, uint32_t nfb, float sample_rate,
                                      const float* hz, float* mag, float* phase, uint32_t n) {
  if (!ff || !fb || nff == 0 || nfb == 0 || nff > WAA_MAX_IIR_COEFFS || nfb > WAA_MAX_IIR_COEFFS)
    return fail(WAA_ERR_NOT_SUPPORTED, "NotSupportedError - invalid IIR coefficient arrays");
  double sr = (double)sample_rate, nyq = sr / 2.;
  for (uint32_t i = 0; i < n; i++) {
    double freq = (double)hz[i];
    if (freq < 0. || freq > nyq) {
      mag[i] = NAN;
      phase[i] = NAN;
      continue;
    }
    double z = -2.0 * M_PI * freq / sr;
    double nr = 0., ni = 0., dr = 0., di = 0.;
    for (uint32_t k = 0; k < nff; k++) {
      nr += ff[k] * cos((double)k * z);
      ni += ff[k] * sin((double)k * z);
    }
    for (uint32_t k = 0; k < nfb; k++) {
      dr += fb[k] * cos((double)k * z);
      di += fb[k] * sin((double)k * z);
    }
    double den = dr * dr + di * di;
    double rr = (nr * dr + ni * di) / den, ri = (ni * dr - nr * di) / den;
    mag[i] = (float)hypot(rr, ri);
    phase[i] = (float)atan2(ri, rr);
  }
  return WAA_OK;
}

/* buffer.rs:311-363 AudioBuffer::resample (one channel) */
uint64_t orc_buffer_resample(const float* src, uint64_t frames, float source_sr, float target_sr, float* dst,
                             uint64_t cap) {
  if (fabsf(source_sr - target_sr) <= 0.1f || frames == 0) {
    if (dst)
      for (uint64_t i = 0; i < frames && i < cap; i++) dst[i] = src[i];
    return frames;
  }
  double ratio = (double)target_sr / (double)source_sr;
  uint64_t tl = (uint64_t)ceil((double)frames * ratio);
  if (!dst) return tl;
  for (uint64_t i = 0; i < tl && i < cap; i++) {
    double position = (double)i / (double)(tl - 1);
    double playhead = position * (double)(frames - 1);
    double pf = floor(playhead);
    /* a target length of 1 makes position 0 / 0: Rust's `as usize` turns the NaN playhead into index 0 (a saturating
     * cast; in C the conversion of a NaN is undefined), k stays NaN and the one sample emitted is NaN */
    uint64_t prev = pf == pf ? (uint64_t)pf : 0;
    uint64_t next = prev + 1 < frames - 1 ? prev + 1 : frames - 1;
    float k = (float)(playhead - pf);
    float kinv = 1.f - k;
    dst[i] = kinv * src[prev] + k * src[next];
  }
  return tl;
}

/* ------------------------------------------------------------------------------------ */
/* node processors                                                                        */
/* ------------------------------------------------------------------------------------ */
typedef struct {
  uint64_t current_frame;
  double current_time;
  float sample_rate;
  uint64_t quantum;
} Scope;

/* src/node/audio_buffer_source.rs:422-845 */
static void process_buffer_source(orc_batch* b, NodeCfg* n, NodeState* s, uint32_t inst, const Scope* sc) {
  Quantum* output = &s->out;
  if (s->ended) {
    q_make_silent(output);
    return;
  }
  double sample_rate = (double)sc->sample_rate;
  double dt = 1. / sample_rate;
  double block_duration = dt * (double)RQ;
  double next_block_time = sc->current_time + block_duration;
  const Buf* buffer = n->bufs[inst].refcnt ? &n->bufs[inst] : NULL;

  if (!buffer && s->start_time != DBL_MAX) {
    q_make_silent(output);
    s->ended = 1;
    s->ended_q = (int64_t)sc->quantum;
    return;
  }
  if (s->start_time >= next_block_time) {
    q_make_silent(output);
    if (s->stop_time <= next_block_time) {
      s->ended = 1;
      s->ended_q = (int64_t)sc->quantum;
    }
    return;
  }
  if (!buffer) {
    q_make_silent(output);
    return;
  }
  int is_looping = s->is_looping;
  double loop_start = s->loop_start, loop_end = s->loop_end;
  double actual_loop_start = 0., actual_loop_end = 0.;

  float tmp[RQ];
  int len;
  /* k-rate params (audio_buffer_source.rs:157,168): with an input from the graph the value of the quantum is the
   * intrinsic value + the FIRST sample of the mixed input, NaN -> default, clamped (param.rs:739-760) - element 0 of what
   * param_get_in forms in either of its branches */
  double detune = (double)param_get_in(&n->params[WAA_PARAM_SOURCE_DETUNE], s->pin[WAA_PARAM_SOURCE_DETUNE], inst, sc->quantum, &len, tmp)[0];
  double playback_rate =
      (double)param_get_in(&n->params[WAA_PARAM_SOURCE_PLAYBACK_RATE], s->pin[WAA_PARAM_SOURCE_PLAYBACK_RATE], inst, sc->quantum, &len, tmp)[0];
  double computed_playback_rate = playback_rate * exp2(detune / 1200.);

  uint64_t buffer_length = buffer->frames;
  double buffer_duration = (double)buffer->frames / (double)buffer->sr; /* buffer.rs duration(): length / sample_rate (f64) */
  double sampling_ratio = (double)buffer->sr / sample_rate;
  double buffer_time = s->buffer_time;

  /* output.set_number_of_channels(buffer.number_of_channels()) then every sample is written */
  output->n = (int)buffer->n_ch;
  for (int c = 0; c < output->n; c++) output->silent[c] = 0;

  double block_time = sc->current_time;
  if (!s->started && s->start_time < block_time) s->start_time = block_time;
  if (s->start_time == block_time && s->offset == 0.) s->is_aligned = 1;
  if (sampling_ratio != 1. || computed_playback_rate != 1.) s->is_aligned = 0;
  if (loop_start != 0. || loop_end != buffer_duration) s->is_aligned = 0;
  if (buffer_time + block_duration > s->duration || block_time + block_duration > s->stop_time) s->is_aligned = 0;

  if (s->is_aligned) {
    if (s->start_time == block_time) s->started = 1;
    if (buffer_time + block_duration > buffer_duration) {
      uint64_t end_index = buffer->frames;
      int loop_point_index = -1;
      for (uint32_t c = 0; c < buffer->n_ch; c++) {
        const float* ch = buffer->ch[c];
        uint64_t start_index = (uint64_t)llround(buffer_time * sample_rate);
        uint64_t off = 0;
        for (int index = 0; index < RQ; index++) {
          uint64_t bi = start_index + (uint64_t)index - off;
          float v;
          if (bi < end_index) {
            v = ch[bi];
          } else {
            if (is_looping && bi >= end_index) {
              loop_point_index = index;
              start_index = 0;
              off = (uint64_t)index;
              bi = 0;
            }
            v = is_looping ? ch[bi] : 0.f;
          }
          output->d[c][index] = v;
        }
      }
      if (loop_point_index >= 0)
        buffer_time = fmod((double)(RQ - loop_point_index) / sample_rate, buffer_duration);
      else
        buffer_time += block_duration;
    } else {
      uint64_t start_index = (uint64_t)llround(buffer_time * sample_rate);
      for (uint32_t c = 0; c < buffer->n_ch; c++) memcpy(output->d[c], buffer->ch[c] + start_index, sizeof(float) * RQ);
      buffer_time += block_duration;
    }
    s->buffer_time_elapsed += block_duration;
  } else {
    if (is_looping) {
      if (loop_start >= 0. && loop_end > 0. && loop_start < loop_end) {
        actual_loop_start = loop_start;
        actual_loop_end = loop_end;
      } else {
        actual_loop_start = 0.;
        actual_loop_end = buffer_duration;
      }
    } else {
      s->entered_loop = 0;
    }
    int64_t pi_prev[RQ];
    double pi_k[RQ];
    for (int i = 0; i < RQ; i++) {
      pi_prev[i] = -1;
      double current_time = block_time + (double)i * dt;
      if (!s->started && almost_equal(current_time, s->start_time)) s->start_time = current_time;
      if (almost_equal(s->buffer_time_elapsed, s->duration)) s->buffer_time_elapsed = s->duration;
      if (current_time < s->start_time || current_time >= s->stop_time || s->buffer_time_elapsed >= s->duration) continue;
      if (!s->started) {
        double delta = current_time - s->start_time;
        s->offset += delta * computed_playback_rate;
        s->offset = fmin(fmax(s->offset, 0.), buffer_duration);
        if (is_looping && computed_playback_rate >= 0. && s->offset > actual_loop_end) s->offset = actual_loop_end;
        if (is_looping && computed_playback_rate < 0. && s->offset < actual_loop_start) s->offset = actual_loop_start;
        buffer_time = s->offset;
        s->buffer_time_elapsed = fabs(delta * computed_playback_rate);
        s->started = 1;
      }
      if (is_looping) {
        if (almost_equal(buffer_time, actual_loop_end)) buffer_time = actual_loop_end;
        if (almost_equal(buffer_time, actual_loop_start)) buffer_time = actual_loop_start;
        if (!s->entered_loop) {
          if (s->offset < actual_loop_end && buffer_time >= actual_loop_start) s->entered_loop = 1;
          if (s->offset >= actual_loop_end && buffer_time < actual_loop_end) s->entered_loop = 1;
        }
        if (s->entered_loop) {
          while (buffer_time >= actual_loop_end) buffer_time -= actual_loop_end - actual_loop_start;
          while (buffer_time < actual_loop_start) buffer_time += actual_loop_end - actual_loop_start;
        }
      }
      if (almost_zero(buffer_time)) buffer_time = 0.;
      if (buffer_time >= 0. && buffer_time < buffer_duration) {
        double position = buffer_time * sampling_ratio;
        double playhead = position * sample_rate;
        double pf = floor(playhead);
        uint64_t prev = (uint64_t)pf;
        double k = playhead - pf;
        if (prev < buffer_length) {
          pi_prev[i] = (int64_t)prev;
          pi_k[i] = k;
        }
      }
      double time_incr = dt * computed_playback_rate;
      buffer_time += time_incr;
      s->buffer_time_elapsed += fabs(time_incr);
    }
    for (uint32_t c = 0; c < buffer->n_ch; c++) {
      const float* ch = buffer->ch[c];
      for (int i = 0; i < RQ; i++) {
        if (pi_prev[i] < 0) {
          output->d[c][i] = 0.f;
          continue;
        }
        uint64_t prev = (uint64_t)pi_prev[i];
        double k = pi_k[i];
        double prev_sample = (double)ch[prev];
        double next_sample;
        if (prev + 1 < buffer_length) {
          next_sample = (double)ch[prev + 1];
        } else if (is_looping) {
          if (playback_rate >= 0.) {
            double sp = actual_loop_start * sample_rate;
            uint64_t si = (floor(sp) == sp) ? (uint64_t)sp : (uint64_t)sp + 1;
            next_sample = si < buffer_length ? (double)ch[si] : 0.;
          } else {
            double ep = actual_loop_end * sample_rate;
            uint64_t ei = (uint64_t)ep;
            /* the reference indexes buffer_channel[end_index] here (audio_buffer_source.rs:795-797), which is one
             * past the end when loop_end == duration: a Rust panic (the node is muted).  Defined here as 0. */
            next_sample = ei < buffer_length ? (double)ch[ei] : 0.;
          }
        } else {
          if (almost_equal(k, 1.) || prev == 0)
            next_sample = 0.;
          else
            next_sample = 2. * prev_sample - (double)ch[prev - 1];
        }
        output->d[c][i] = (float)fma(1. - k, prev_sample, k * next_sample);
      }
    }
  }
  s->buffer_time = buffer_time;
  if (next_block_time >= s->stop_time || s->buffer_time_elapsed >= s->duration ||
      (!is_looping && ((computed_playback_rate > 0. && buffer_time >= buffer_duration) ||
                       (computed_playback_rate < 0. && buffer_time < 0.)))) {
    s->ended = 1;
    s->ended_q = (int64_t)sc->quantum;
  }
  (void)b;
}

/* src/node/constant_source.rs:190-275 */
static void process_constant_source(NodeCfg* n, NodeState* s, uint32_t inst, const Scope* sc) {
  Quantum* output = &s->out;
  double dt = 1. / (double)sc->sample_rate;
  double next_block_time = sc->current_time + dt * (double)RQ;
  if (s->start_time >= next_block_time) {
    q_make_silent(output);
    if (s->stop_time <= next_block_time && !s->ended_triggered) { /* :207-212 */
      s->ended_triggered = 1;
      s->ended_q = (int64_t)sc->quantum;
    }
    return;
  }
  if (!(s->stop_time > next_block_time) && !s->ended_triggered) { /* :254-262, `still_running` */
    s->ended_triggered = 1;
    s->ended_q = (int64_t)sc->quantum;
  }
  output->n = 1;
  output->silent[0] = 0;
  float tmp[RQ];
  int len;
  const float* offset = param_get_in(&n->params[0], s->pin[0], inst, sc->quantum, &len, tmp);
  if (len == 1 && s->start_time <= sc->current_time && s->stop_time >= next_block_time) {
    for (int i = 0; i < RQ; i++) output->d[0][i] = offset[0];
  } else {
    double current_time = sc->current_time;
    for (int i = 0; i < RQ; i++) {
      float value = offset[len == 1 ? 0 : i];
      output->d[0][i] = (current_time < s->start_time || current_time >= s->stop_time) ? 0.f : value;
      current_time += dt;
    }
  }
}

/* src/node/biquad_filter.rs:764-899 */
static void process_biquad(NodeCfg* n, NodeState* s, uint32_t inst, const Scope* sc) {
  const Quantum* input = &s->in;
  Quantum* output = &s->out;
  int in_silent = q_is_silent(input);
  if (in_silent) {
    int ended = 1;
    for (int c = 0; c < s->xy_len && ended; c++)
      for (int j = 0; j < 4; j++)
        if (isnormal(s->xy[c][j])) {
          ended = 0;
          break;
        }
    if (ended) {
      q_make_silent(output);
      return;
    }
  }
  if (!in_silent) {
    int nc = input->n;
    if (nc != s->xy_len) {
      /* truncate then push zeros */
      for (int c = s->xy_len; c < nc; c++) memset(s->xy[c], 0, sizeof s->xy[c]);
      s->xy_len = nc;
    }
    q_set_number_of_channels(output, nc);
  } else {
    q_set_number_of_channels(output, s->xy_len);
  }
  float tf[RQ], td[RQ], tq[RQ], tg[RQ];
  int lf, ld, lq, lg;
  const float* frequency = param_get_in(&n->params[WAA_PARAM_BIQUAD_FREQUENCY], s->pin[WAA_PARAM_BIQUAD_FREQUENCY], inst, sc->quantum, &lf, tf);
  const float* detune = param_get_in(&n->params[WAA_PARAM_BIQUAD_DETUNE], s->pin[WAA_PARAM_BIQUAD_DETUNE], inst, sc->quantum, &ld, td);
  const float* q = param_get_in(&n->params[WAA_PARAM_BIQUAD_Q], s->pin[WAA_PARAM_BIQUAD_Q], inst, sc->quantum, &lq, tq);
  const float* gain = param_get_in(&n->params[WAA_PARAM_BIQUAD_GAIN], s->pin[WAA_PARAM_BIQUAD_GAIN], inst, sc->quantum, &lg, tg);
  double srd = (double)sc->sample_rate;
  int type = n->desc.i[0];
  Coefs coefs[RQ];
  coefs[0] = calculate_coefs(type, srd, (double)get_computed_freq(frequency[0], detune[0]), (double)gain[0], (double)q[0]);
  if (lf != 1 || ld != 1 || lq != 1 || lg != 1) {
    for (int i = 1; i < RQ; i++)
      coefs[i] = calculate_coefs(type, srd, (double)get_computed_freq(frequency[i % lf], detune[i % ld]),
                                 (double)gain[i % lg], (double)q[i % lq]);
  } else {
    for (int i = 1; i < RQ; i++) coefs[i] = coefs[0];
  }
  for (int c = 0; c < output->n; c++) {
    const float* in = in_silent ? input->d[0] : input->d[c];
    double x1 = s->xy[c][0], x2 = s->xy[c][1], y1 = s->xy[c][2], y2 = s->xy[c][3];
    for (int i = 0; i < RQ; i++) {
      const Coefs* k = &coefs[i];
      double x = (double)in[i];
      double y = k->b0 * x + k->b1 * x1 + k->b2 * x2 - k->a1 * y1 - k->a2 * y2;
      if (!isnormal(y)) y = 0.;
      x2 = x1;
      x1 = x;
      y2 = y1;
      y1 = y;
      output->d[c][i] = (float)y;
    }
    output->silent[c] = 0;
    s->xy[c][0] = x1;
    s->xy[c][1] = x2;
    s->xy[c][2] = y1;
    s->xy[c][3] = y2;
  }
}

/* src/node/iir_filter.rs:323-405 (f64 transposed direct form II) */
static void process_iir(NodeCfg* n, NodeState* s) {
  const Quantum* input = &s->in;
  Quantum* output = &s->out;
  const int len = n->iir_len;
  int in_silent = q_is_silent(input);
  if (s->iir_nch == 0) s->iir_nch = 2; /* "eagerly assume stereo input", :303-306 */
  if (in_silent) {
    int ended = 1;
    for (int c = 0; c < s->iir_nch && ended; c++)
      for (int j = 0; j < len; j++)
        if (isnormal(s->iir_state[c][j])) {
          ended = 0;
          break;
        }
    if (ended) {
      q_make_silent(output);
      return;
    }
  }
  if (!in_silent) {
    int nc = input->n;
    if (nc != s->iir_nch) {
      for (int c = s->iir_nch; c < nc; c++) memset(s->iir_state[c], 0, sizeof s->iir_state[c]);
      s->iir_nch = nc;
    }
    q_set_number_of_channels(output, nc);
  } else {
    q_set_number_of_channels(output, s->iir_nch);
  }
  for (int c = 0; c < output->n; c++) {
    const float* in = in_silent ? input->d[0] : input->d[c];
    double* st = s->iir_state[c];
    for (int i = 0; i < RQ; i++) {
      double x = (double)in[i];
      double y = fma(n->iir_b[0], x, st[0]);
      if (!isnormal(y)) y = 0.;
      for (int k = 1; k < len; k++) {
        double next = k < WAA_MAX_IIR_COEFFS ? st[k] : 0.;
        st[k - 1] = n->iir_b[k] * x - n->iir_a[k] * y + next;
      }
      output->d[c][i] = (float)y;
    }
    output->silent[c] = 0;
  }
}

/* src/node/delay.rs: DelayWriter::process :428-466 and DelayReader::process :515-680.  Outside a cycle the
 * writer->reader edge of delay.rs:361 makes the writer render first (sub-quantum delays work); inside one the
 * cycle breaker removes that edge, the reader renders first and clamps the delay to one render quantum. */
typedef struct {
  int prev_block_index, prev_frame_index;
  float k;
} PlaybackInfo;

/* delay.rs:682-745 */
static PlaybackInfo delay_playback_infos(double delay, int in_cycle, double sample_index, double quantum_duration,
                                         double sample_rate, int ring_size, int ring_index) {
  double clamped_delay = in_cycle ? fmax(delay, quantum_duration) : delay; /* :693-701 */
  double num_samples = clamped_delay * sample_rate;
  double position = sample_index - num_samples;
  double position_floored = floor(position);
  int num_frames = RQ;
  double block_offset = floor(position_floored / (double)num_frames);
  int prev_block_index = ring_index + (int)block_offset;
  if (prev_block_index < 0) prev_block_index += ring_size;
  int frame_offset = (int)position_floored % num_frames; /* C and Rust: sign of the dividend */
  if (frame_offset == 0) frame_offset = -num_frames;
  int prev_frame_index = frame_offset <= 0 ? num_frames + frame_offset : frame_offset;
  PlaybackInfo r = {prev_block_index, prev_frame_index, (float)(position - position_floored)};
  return r;
}

static void delay_check_ring(NodeCfg* n, NodeState* s, double sample_rate) {
  if (s->dl_ring) return; /* delay.rs:297-303 + check_ring_buffer_size :386-397: filled with silent quanta */
  int num_quanta = (int)ceil(n->desc.d[0] * sample_rate / (double)RQ);
  s->dl_cap = num_quanta + 1;
  s->dl_ring = (Quantum*)malloc(sizeof(Quantum) * (size_t)s->dl_cap);
  for (int i = 0; i < s->dl_cap; i++) q_make_silent(&s->dl_ring[i]);
}

/* DelayWriter::process, delay.rs:428-466 */
static void process_delay_writer(NodeCfg* n, NodeState* s, const Scope* sc) {
  const Quantum* input = &s->in;
  delay_check_ring(n, s, (double)sc->sample_rate);
  if (s->dl_ring[0].n != input->n) /* check_ring_buffer_up_down_mix :469-489 */
    for (int i = 0; i < s->dl_cap; i++) q_mix(&s->dl_ring[i], input->n, WAA_INTERP_SPEAKERS);
  q_copy(&s->dl_ring[s->dl_windex], input);
  s->dl_windex = (s->dl_windex + 1) % s->dl_cap;
  s->dl_latest_frame_written = sc->current_frame;
  s->dl_written_once = 1;
}

/* DelayReader::process, delay.rs:515-680 */
static void process_delay_reader(NodeCfg* n, NodeState* s, uint32_t inst, const Scope* sc) {
  Quantum* output = &s->out;
  double sample_rate = (double)sc->sample_rate;
  delay_check_ring(n, s, sample_rate);
  const Quantum* ring = s->dl_ring;
  int nch = ring[0].n;
  q_make_silent(output);
  q_set_number_of_channels(output, nch);
  if (!s->dl_in_cycle) /* :535-541: the writer has not rendered this quantum => the cycle breaker was applied */
    s->dl_in_cycle = !(s->dl_written_once && s->dl_latest_frame_written == sc->current_frame);
  float tmp[RQ];
  int len;
  const float* delay = param_get_in(&n->params[0], s->pin[0], inst, sc->quantum, &len, tmp);
  double dt = 1. / sample_rate;
  double quantum_duration = (double)RQ * dt;
  int ring_size = s->dl_cap, ring_index = s->dl_rindex;
  PlaybackInfo infos[RQ];
  if (len == 1) {
    infos[0] = delay_playback_infos((double)delay[0], s->dl_in_cycle, 0., quantum_duration, sample_rate, ring_size, ring_index);
    for (int i = 1; i < RQ; i++) {
      PlaybackInfo p = infos[i - 1];
      p.prev_frame_index += 1;
      if (p.prev_frame_index >= RQ) {
        p.prev_block_index = (p.prev_block_index + 1) % ring_size;
        p.prev_frame_index = 0;
      }
      infos[i] = p;
    }
  } else {
    for (int i = 0; i < RQ; i++)
      infos[i] = delay_playback_infos((double)delay[i], s->dl_in_cycle, (double)i, quantum_duration, sample_rate, ring_size,
                                      ring_index);
  }
  int active = 0;
  for (int c = 0; c < nch; c++) {
    for (int i = 0; i < RQ; i++) {
      PlaybackInfo p = infos[i];
      int next_block_index = p.prev_block_index, next_frame_index = p.prev_frame_index + 1;
      if (next_frame_index >= RQ) {
        next_block_index = (next_block_index + 1) % ring_size;
        next_frame_index = 0;
      }
      float prev_sample = ring[p.prev_block_index].d[c][p.prev_frame_index];
      float next_sample = ring[next_block_index].d[c][next_frame_index];
      float value = fmaf(1.f - p.k, prev_sample, p.k * next_sample);
      if (isnormal(value)) active = 1;
      output->d[c][i] = value;
    }
    output->silent[c] = 0;
  }
  if (!active) q_make_silent(output);
  s->dl_rindex = (s->dl_rindex + 1) % s->dl_cap;
}

/* src/node/oscillator.rs:323-660 */
#define OSC_SINE_TABLE_LEN 2048
static const float* osc_sine_table(void) { /* oscillator.rs:16-28 */
  static float table[OSC_SINE_TABLE_LEN];
  static int ready = 0;
  if (!ready) {
    const float pi = 3.14159265358979323846f;
    for (int x = 0; x < OSC_SINE_TABLE_LEN; x++) table[x] = sinf(((float)x) * 2.0f * pi * (1.f / (float)OSC_SINE_TABLE_LEN));
    ready = 1;
  }
  return table;
}
static double osc_unroll_phase(double phase) { /* :646-654 */
  if (phase >= 1.) return phase - 1.;
  if (phase < 0.) return phase + 1.;
  return phase;
}
static double osc_unroll_phase_unbounded(double phase) { /* :656-659 rem_euclid(1.) */
  double r = fmod(phase, 1.);
  return r < 0. ? r + 1. : r;
}
static double osc_poly_blep(double t, double dt) { /* :630-643 (production: cfg!(test) == false) */
  if (t < dt) {
    t /= dt;
    return t + t - t * t - 1.0;
  } else if (t > 1.0 - dt) {
    t = (t - 1.0) / dt;
    return fma(t, t, t) + t + 1.0;
  }
  return 0.0;
}
/* As in the reference, a phase of exactly 1.0 would index table[len]: osc_unroll_phase returns 1.0 for a phase in
 * [-2^-54, 0) (phase + 1. rounds up), reachable when |phase + incr| < 2^-54.  The reference panics there; the oracle is
 * left as the reference is written, and no test steers into it (tests/test_oscillator_kernels.py keeps |incr| >= 1e-9
 * or exactly 0).  The device's table_sample (waa_osc.hip) wraps that index to 0. */
static float osc_table_sample(const float* table, int len, double phase) { /* :571-586, :604-619 */
  double position = phase * (double)len;
  double floored = floor(position);
  int prev_index = (int)floored;
  int next_index = prev_index + 1;
  if (next_index == len) next_index = 0;
  float k = (float)(position - floored);
  return fmaf(table[prev_index], 1.f - k, table[next_index] * k);
}
static float osc_waveform_sample(const NodeCfg* n, double phase, double phase_incr) { /* :561-602 */
  switch (n->osc_wave ? WAA_OSC_CUSTOM : n->desc.i[0]) {
    case WAA_OSC_SINE: return osc_table_sample(osc_sine_table(), OSC_SINE_TABLE_LEN, phase);
    case WAA_OSC_SAWTOOTH: {
      double ph = osc_unroll_phase(phase + 0.5);
      double sample = 2.0 * ph - 1.0;
      sample -= osc_poly_blep(ph, phase_incr);
      return (float)sample;
    }
    case WAA_OSC_SQUARE: {
      double sample = phase < 0.5 ? 1.0 : -1.0;
      sample += osc_poly_blep(phase, phase_incr);
      double shift_phase = osc_unroll_phase(phase + 0.5);
      sample -= osc_poly_blep(shift_phase, phase_incr);
      return (float)sample;
    }
    case WAA_OSC_TRIANGLE: {
      double sample = -4. * phase + 2.;
      if (sample > 1.)
        sample = 2. - sample;
      else if (sample < -1.)
        sample = -2. - sample;
      return (float)sample;
    }
    default: return osc_table_sample(n->osc_wave, 8192, phase);
  }
}
/* generate_sample, :505-553 */
static double osc_generate_sample(const NodeCfg* n, NodeState* s, float* output, int outside_nyquist, double phase_incr,
                                  double current_time, double dt) {
  if (current_time < s->start_time || current_time >= s->stop_time) {
    *output = 0.f;
    return current_time + dt;
  }
  if (!s->osc_started) {
    if (current_time > s->start_time) {
      double ratio = (current_time - s->start_time) / dt;
      s->osc_phase = outside_nyquist ? osc_unroll_phase_unbounded(phase_incr * ratio) : osc_unroll_phase(phase_incr * ratio);
    }
    s->osc_started = 1;
  }
  *output = outside_nyquist ? 0.f : osc_waveform_sample(n, s->osc_phase, phase_incr);
  s->osc_phase = outside_nyquist ? osc_unroll_phase_unbounded(s->osc_phase + phase_incr) : osc_unroll_phase(s->osc_phase + phase_incr);
  return current_time + dt;
}
static void process_oscillator(NodeCfg* n, NodeState* s, uint32_t inst, const Scope* sc) {
  Quantum* output = &s->out;
  q_make_silent(output); /* 1 channel */
  double sample_rate = (double)sc->sample_rate;
  double dt = 1. / sample_rate;
  double next_block_time = sc->current_time + dt * (double)RQ;
  if (s->stop_time <= sc->current_time) { /* :382-390 */
    if (!s->ended_triggered) {
      s->ended_triggered = 1;
      s->ended_q = (int64_t)sc->quantum;
    }
    return;
  }
  if (s->stop_time <= next_block_time && !s->ended_triggered) { /* :394-399 and :461-466: both branches test this */
    s->ended_triggered = 1;
    s->ended_q = (int64_t)sc->quantum;
  }
  if (s->start_time >= next_block_time) return;
  float tf[RQ], td[RQ];
  int lf, ld;
  const float* frequency_values = param_get_in(&n->params[WAA_PARAM_OSCILLATOR_FREQUENCY], s->pin[WAA_PARAM_OSCILLATOR_FREQUENCY],
                                               inst, sc->quantum, &lf, tf);
  const float* detune_values = param_get_in(&n->params[WAA_PARAM_OSCILLATOR_DETUNE], s->pin[WAA_PARAM_OSCILLATOR_DETUNE], inst,
                                            sc->quantum, &ld, td);
  double current_time = sc->current_time;
  if (!s->osc_started && s->start_time < current_time) s->start_time = current_time;
  double nyquist = sample_rate / 2.;
  float* channel_data = output->d[0];
  output->silent[0] = 0;
  if (lf == 1 && ld == 1) {
    double computed_freq = (double)frequency_values[0] * exp2((double)detune_values[0] / 1200.);
    double phase_incr = computed_freq / sample_rate;
    int outside_nyquist = fabs(computed_freq) >= nyquist;
    int fully_active = s->osc_started && s->start_time <= sc->current_time && s->stop_time >= next_block_time;
    if (fully_active && !outside_nyquist) {
      for (int i = 0; i < RQ; i++) {
        channel_data[i] = osc_waveform_sample(n, s->osc_phase, phase_incr);
        s->osc_phase = osc_unroll_phase(s->osc_phase + phase_incr);
      }
    } else {
      for (int i = 0; i < RQ; i++)
        current_time = osc_generate_sample(n, s, &channel_data[i], outside_nyquist, phase_incr, current_time, dt);
    }
  } else {
    for (int i = 0; i < RQ; i++) {
      double computed_freq = (double)frequency_values[i % lf] * exp2((double)detune_values[i % ld] / 1200.);
      double phase_incr = computed_freq / sample_rate;
      int outside_nyquist = fabs(computed_freq) >= nyquist;
      current_time = osc_generate_sample(n, s, &channel_data[i], outside_nyquist, phase_incr, current_time, dt);
    }
  }
}

/* src/node/gain.rs:143-199 */
static void process_gain(NodeCfg* n, NodeState* s, uint32_t inst, const Scope* sc) {
  const Quantum* input = &s->in;
  Quantum* output = &s->out;
  if (q_is_silent(input)) {
    q_make_silent(output);
    return;
  }
  float tmp[RQ];
  int len;
  const float* gain = param_get_in(&n->params[0], s->pin[0], inst, sc->quantum, &len, tmp);
  if (len == 1) {
    float threshold = 1e-6f;
    if (fabsf(gain[0]) <= threshold) {
      q_make_silent(output);
      return;
    }
    if (fabsf(1.f - gain[0]) <= threshold) {
      q_copy(output, input);
      return;
    }
  }
  q_copy(output, input);
  for (int c = 0; c < output->n; c++) {
    /* channel.iter_mut() goes through make_mut: a silent channel becomes a written one */
    output->silent[c] = 0;
    if (len == 1) {
      float g = gain[0];
      for (int i = 0; i < RQ; i++) output->d[c][i] *= g;
    } else {
      for (int i = 0; i < RQ; i++) output->d[c][i] *= gain[i];
    }
  }
}

/* src/node/stereo_panner.rs:74-79 */
static void get_stereo_gains(float x, float* gl, float* gr) {
  const float PI_F = 3.14159265358979323846f;
  *gl = sinf((1.f - x) * PI_F / 2.f);
  *gr = sinf(x * PI_F / 2.f);
}
/* src/node/stereo_panner.rs:218-317 */
static void process_stereo_panner(NodeCfg* n, NodeState* s, uint32_t inst, const Scope* sc) {
  const Quantum* input = &s->in;
  Quantum* output = &s->out;
  if (q_is_silent(input)) {
    q_make_silent(output);
    return;
  }
  float tmp[RQ];
  int len;
  const float* pan_values = param_get_in(&n->params[0], s->pin[0], inst, sc->quantum, &len, tmp);
  float (*L) = output->d[0], (*R) = output->d[1];
  if (input->n == 1) {
    const float* in = input->d[0];
    if (len == 1) {
      float x = (pan_values[0] + 1.f) * 0.5f, gl, gr;
      get_stereo_gains(x, &gl, &gr);
      for (int i = 0; i < RQ; i++) {
        float v = in[i];
        L[i] = v * gl;
        R[i] = v * gr;
      }
    } else {
      for (int i = 0; i < RQ; i++) {
        float x = (pan_values[i] + 1.f) * 0.5f, gl, gr;
        get_stereo_gains(x, &gl, &gr);
        float v = in[i];
        L[i] = v * gl;
        R[i] = v * gr;
      }
    }
  } else { /* 2 */
    const float *il = input->d[0], *ir = input->d[1];
    for (int i = 0; i < RQ; i++) {
      float pan = pan_values[len == 1 ? 0 : i];
      float x = pan <= 0.f ? pan + 1.f : pan, gl, gr;
      get_stereo_gains(x, &gl, &gr);
      float a = il[i], bb = ir[i];
      if (pan <= 0.f) {
        L[i] = fmaf(bb, gl, a);
        R[i] = bb * gr;
      } else {
        L[i] = a * gl;
        R[i] = fmaf(a, gr, bb);
      }
    }
  }
  output->n = 2;
  output->silent[0] = output->silent[1] = 0;
}

/* vecmath helpers as used by src/spatial.rs */
static void v3_sub(const float* a, const float* b, float* o) {
  o[0] = a[0] - b[0];
  o[1] = a[1] - b[1];
  o[2] = a[2] - b[2];
}
static float v3_dot(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
static float v3_sqlen(const float* a) { return a[0] * a[0] + a[1] * a[1] + a[2] * a[2]; }
static float v3_len(const float* a) { return sqrtf(v3_sqlen(a)); }
static void v3_scale(const float* a, float s, float* o) {
  o[0] = a[0] * s;
  o[1] = a[1] * s;
  o[2] = a[2] * s;
}
static void v3_normalized(const float* a, float* o) { v3_scale(a, 1.f / v3_len(a), o); }
static void v3_cross(const float* a, const float* b, float* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
static const float PI_F32 = 3.14159265358979323846f;

/* src/spatial.rs:205-270 */
static void azimuth_and_elevation(const float* sp, const float* lp, const float* lf, const float* lu, float* az,
                                  float* el) {
  float rel[3];
  v3_sub(sp, lp, rel);
  if (v3_sqlen(rel) <= FLT_MIN) {
    *az = 0.f;
    *el = 0.f;
    return;
  }
  float sl[3], right[3];
  v3_normalized(rel, sl);
  v3_cross(lf, lu, right);
  if (v3_sqlen(right) == 0.f) {
    *az = 0.f;
    *el = 0.f;
    return;
  }
  float rn[3], fn[3], up[3];
  v3_normalized(right, rn);
  v3_normalized(lf, fn);
  v3_cross(rn, fn, up);
  float elevation = 90.f - 180.f * acosf(v3_dot(sl, up)) / PI_F32;
  if (elevation > 90.f)
    elevation = 180.f - elevation;
  else if (elevation < -90.f)
    elevation = -180.f - elevation;
  float up_proj = v3_dot(sl, up);
  float upscaled[3], ps[3];
  v3_scale(up, up_proj, upscaled);
  v3_sub(sl, upscaled, ps);
  if (v3_sqlen(ps) == 0.f) {
    *az = 0.f;
    *el = elevation;
    return;
  }
  float psn[3];
  v3_normalized(ps, psn);
  float azimuth = 180.f * acosf(v3_dot(psn, rn)) / PI_F32;
  float front_back = v3_dot(psn, fn);
  if (front_back < 0.f) azimuth = 360.f - azimuth;
  if (azimuth >= 0.f && azimuth <= 270.f)
    azimuth = 90.f - azimuth;
  else
    azimuth = 450.f - azimuth;
  *az = azimuth;
  *el = elevation;
}
/* src/spatial.rs:278-299 */
static float spatial_angle(const float* sp, const float* so, const float* lp) {
  if (v3_sqlen(so) == 0.f) return 0.f;
  float son[3], rel[3], sl[3];
  v3_normalized(so, son);
  v3_sub(sp, lp, rel);
  if (v3_sqlen(rel) <= FLT_MIN) return 0.f;
  v3_normalized(rel, sl);
  float angle = 180.f * acosf(v3_dot(sl, son)) / PI_F32;
  return fabsf(angle);
}
/* src/node/panner.rs:927-953 */
static float cone_gain(const NodeCfg* n, const float* sp, const float* so, const float* lp) {
  float abs_inner = (float)fabs(n->desc.d[3]) / 2.f;
  float abs_outer = (float)fabs(n->desc.d[4]) / 2.f;
  if (abs_inner >= 180.f && abs_outer >= 180.f) return 1.f;
  float cog = (float)n->desc.d[5];
  float a = spatial_angle(sp, so, lp);
  if (a < abs_inner) return 1.f;
  if (a >= abs_outer) return cog;
  float x = (a - abs_inner) / (abs_outer - abs_inner);
  return (1.f - x) + cog * x;
}
/* src/node/panner.rs:955-985 */
static float dist_gain(const NodeCfg* n, const float* sp, const float* lp) {
  float rel[3];
  v3_sub(sp, lp, rel);
  double distance = (double)v3_len(rel);
  double ref = n->desc.d[0], maxd = n->desc.d[1], roll = n->desc.d[2];
  double g;
  switch (n->desc.i[1]) {
    case WAA_DISTANCE_LINEAR: {
      double rf = roll < 0. ? 0. : roll > 1. ? 1. : roll;
      double d2ref = fmin(ref, maxd), d2max = fmax(ref, maxd);
      double dc = distance < d2ref ? d2ref : distance > d2max ? d2max : distance;
      g = 1. - rf * (dc - d2ref) / (d2max - d2ref);
      break;
    }
    case WAA_DISTANCE_INVERSE: {
      double rf = fmax(roll, 0.);
      if (distance > 0.)
        g = ref / (ref + rf * (fmax(ref, distance) - ref));
      else
        g = 1.;
      break;
    }
    default: {
      double rf = fmax(roll, 0.);
      g = pow(fmax(distance, ref) / ref, -rf);
      break;
    }
  }
  return (float)g;
}
typedef struct {
  float dist_gain, cone_gain, azimuth, elevation;
} SpatialParams;

static float wrap_azimuth(float azimuth) { /* panner.rs:996-1004 */
  azimuth = azimuth < -180.f ? -180.f : azimuth > 180.f ? 180.f : azimuth;
  if (azimuth < -90.f)
    azimuth = -180.f - azimuth;
  else if (azimuth > 90.f)
    azimuth = 180.f - azimuth;
  return azimuth;
}
/* src/node/panner.rs:988-1014 */
static void apply_mono_to_stereo_gain(SpatialParams p, float* l, float* r) {
  float azimuth = wrap_azimuth(p.azimuth);
  float x = (azimuth + 90.f) / 180.f;
  float gl = cosf(x * PI_F32 / 2.f), gr = sinf(x * PI_F32 / 2.f);
  *l *= gl * p.dist_gain * p.cone_gain;
  *r *= gr * p.dist_gain * p.cone_gain;
}
/* src/node/panner.rs:1016-1057 */
static void apply_stereo_to_stereo_gain(SpatialParams p, float il, float ir, float* ol, float* orr) {
  float azimuth = wrap_azimuth(p.azimuth);
  float x = azimuth <= 0.f ? (azimuth + 90.f) / 90.f : azimuth / 90.f;
  float gl = cosf(x * PI_F32 / 2.f), gr = sinf(x * PI_F32 / 2.f);
  if (azimuth <= 0.f) {
    *ol = (il + ir * gl) * p.dist_gain * p.cone_gain;
    *orr = ir * gr * p.dist_gain * p.cone_gain;
  } else {
    *ol = il * gl * p.dist_gain * p.cone_gain;
    *orr = (ir + il * gr) * p.dist_gain * p.cone_gain;
  }
}
/* ---- HRTF panning: crate hrtf 0.8.1 restated (HrirSphere::new, sample_bilinear, HrtfProcessor::process_samples);
 * call sites panner.rs:39-68 (load_hrtf_processor: resources/IRC_1003_C.bin, interpolation_steps = 1, block 128),
 * :225-275 (HrtfState::process), :781-829.  PARITY UNPINNED by the reference (see the header). ---- */
typedef struct HrirSphere {
  uint32_t sr;  /* sample rate the HRIRs are stored at */
  int len;      /* taps per HRIR */
  int nv, nf;
  uint32_t* faces; /* [nf][3] */
  float* pos;      /* [nv][3] */
  float *left, *right; /* [nv][len] */
} HrirSphere;
static HrirSphere* g_hrir_file;          /* as loaded (orc_hrtf_load_sphere) */
static HrirSphere* g_hrir_cache[16];     /* resampled, one per sample rate (panner.rs:39-60 caches the same way) */
static pthread_mutex_t g_hrir_lock = PTHREAD_MUTEX_INITIALIZER;

static void hrir_free(HrirSphere* h) {
  if (!h) return;
  free(h->faces);
  free(h->pos);
  free(h->left);
  free(h->right);
  free(h);
}
/* The file format of the hrtf crate ("HRIR", sample rate, length, vertex count, index count : u32 LE; indices u32;
 * per vertex x y z f32, left[length] f32, right[length] f32). */
waa_status orc_hrtf_load_sphere(const void* data, uint64_t size) {
  const unsigned char* d = (const unsigned char*)data;
  if (!d || size < 20 || memcmp(d, "HRIR", 4) != 0) return fail(WAA_ERR_INVALID_ARGUMENT, "HRIR sphere: bad magic");
  uint32_t hdr[4];
  memcpy(hdr, d + 4, 16);
  const uint64_t len = hdr[1], nv = hdr[2], ni = hdr[3];
  if (len == 0 || ni % 3 != 0 || size != 20 + 4 * ni + nv * (12 + 8 * len))
    return fail(WAA_ERR_INVALID_ARGUMENT, "HRIR sphere: inconsistent sizes");
  HrirSphere* h = (HrirSphere*)calloc(1, sizeof *h);
  h->sr = hdr[0];
  h->len = (int)len;
  h->nv = (int)nv;
  h->nf = (int)(ni / 3);
  h->faces = (uint32_t*)malloc(4 * ni);
  memcpy(h->faces, d + 20, 4 * ni);
  for (uint64_t i = 0; i < ni; i++)
    if (h->faces[i] >= nv) {
      hrir_free(h);
      return fail(WAA_ERR_INVALID_ARGUMENT, "HRIR sphere: face index out of range");
    }
  h->pos = (float*)malloc(12 * nv);
  h->left = (float*)malloc(4 * nv * len);
  h->right = (float*)malloc(4 * nv * len);
  const unsigned char* p = d + 20 + 4 * ni;
  for (uint64_t v = 0; v < nv; v++) {
    memcpy(h->pos + 3 * v, p, 12);
    memcpy(h->left + v * len, p + 12, 4 * len);
    memcpy(h->right + v * len, p + 12 + 4 * len, 4 * len);
    p += 12 + 8 * len;
  }
  pthread_mutex_lock(&g_hrir_lock);
  hrir_free(g_hrir_file);
  g_hrir_file = h;
  for (int i = 0; i < 16; i++) {
    hrir_free(g_hrir_cache[i]);
    g_hrir_cache[i] = NULL;
  }
  pthread_mutex_unlock(&g_hrir_lock);
  return WAA_OK;
}
/* HRIRs at another sample rate.  The crate resamples every HRIR once with rubato's asynchronous sinc resampler
 * (sinc_len 256, f_cutoff 0.95, BlackmanHarris2, 160x oversampled table + cubic interpolation), one 512-frame chunk;
 * neither crate is available, so this is OUR definition of that step: output n is the band-limited
 * signal at input position t_n = (n + 1) / ratio - 128 (the resampler starts half a filter length before the chunk),
 * kernel = sinc(fc * x) * BH2(x) evaluated directly (no table), fc = 0.95 * min(1, ratio), gain fc; output n exists
 * while t_n < len - 257 - 1/ratio (the chunk-end rule). */
static double hrir_kernel(double x, double fc) {
  if (fabs(x) >= 128.) return 0.;
  const double u = (x + 128.) / 256.;
  const double bh = 0.35875 - 0.48829 * cos(2. * M_PI * u) + 0.14128 * cos(4. * M_PI * u) - 0.01168 * cos(6. * M_PI * u);
  const double a = M_PI * x * fc;
  return bh * bh * (x == 0. ? 1. : sin(a) / a) * fc;
}
static int hrir_resampled_len(int len, double ratio) {
  int n = 0;
  while ((double)(n + 1) / ratio - 128. < (double)len - 257. - 1. / ratio) n++;
  return n;
}
static void hrir_resample(const float* in, int len, double ratio, float* out, int out_len) {
  const double fc = 0.95 * (ratio < 1. ? ratio : 1.);
  for (int n = 0; n < out_len; n++) {
    const double t = (double)(n + 1) / ratio - 128.;
    int m0 = (int)ceil(t - 128.), m1 = (int)floor(t + 128.);
    if (m0 < 0) m0 = 0;
    if (m1 > len - 1) m1 = len - 1;
    double acc = 0.;
    for (int m = m0; m <= m1; m++) acc += (double)in[m] * hrir_kernel(t - (double)m, fc);
    out[n] = (float)acc;
  }
}
static const HrirSphere* hrir_for_rate(uint32_t sample_rate) {
  if (sample_rate < 27000) sample_rate = 27000; /* panner.rs:46-49 */
  pthread_mutex_lock(&g_hrir_lock);
  const HrirSphere* res = NULL;
  if (g_hrir_file) {
    if (g_hrir_file->sr == sample_rate) res = g_hrir_file;
    int slot = -1;
    for (int i = 0; i < 16 && !res; i++) {
      if (g_hrir_cache[i] && g_hrir_cache[i]->sr == sample_rate) res = g_hrir_cache[i];
      if (!g_hrir_cache[i] && slot < 0) slot = i;
    }
    if (!res && slot >= 0) {
      const HrirSphere* f = g_hrir_file;
      const double ratio = (double)sample_rate / (double)f->sr;
      HrirSphere* h = (HrirSphere*)calloc(1, sizeof *h);
      h->sr = sample_rate;
      h->len = hrir_resampled_len(f->len, ratio);
      h->nv = f->nv;
      h->nf = f->nf;
      h->faces = (uint32_t*)malloc(12 * (size_t)f->nf);
      memcpy(h->faces, f->faces, 12 * (size_t)f->nf);
      h->pos = (float*)malloc(12 * (size_t)f->nv);
      memcpy(h->pos, f->pos, 12 * (size_t)f->nv);
      h->left = (float*)malloc(4 * (size_t)f->nv * h->len);
      h->right = (float*)malloc(4 * (size_t)f->nv * h->len);
      for (int v = 0; v < f->nv; v++) {
        hrir_resample(f->left + (size_t)v * f->len, f->len, ratio, h->left + (size_t)v * h->len, h->len);
        hrir_resample(f->right + (size_t)v * f->len, f->len, ratio, h->right + (size_t)v * h->len, h->len);
      }
      g_hrir_cache[slot] = h;
      res = h;
    }
  }
  pthread_mutex_unlock(&g_hrir_lock);
  return res;
}
uint32_t orc_hrtf_hrir_length(float sample_rate) {
  const HrirSphere* h = hrir_for_rate((uint32_t)sample_rate);
  return h ? (uint32_t)h->len : 0;
}
/* HrirSphere::sample_bilinear: the triangle the ray from the origin along `dir` pierces, barycentric weights of the
 * piercing point (u, v, w for the face's vertices a, b, c); out = a*u + b*v + c*w per tap, f32.  Of the faces whose
 * plane the ray meets in front of the origin the one with the largest smallest weight is taken (= the face that
 * contains the point; on an edge both candidates interpolate to the same HRIR). */
static void hrir_locate(const HrirSphere* h, const float dir[3], int vtx[3], float wgt[3]) {
  float best = -1e30f;
  vtx[0] = vtx[1] = vtx[2] = 0;
  wgt[0] = 1.f;
  wgt[1] = wgt[2] = 0.f;
  for (int f = 0; f < h->nf; f++) {
    const float* a = h->pos + 3 * h->faces[3 * f];
    const float* b = h->pos + 3 * h->faces[3 * f + 1];
    const float* c = h->pos + 3 * h->faces[3 * f + 2];
    float ba[3], ca[3], nrm[3];
    v3_sub(b, a, ba);
    v3_sub(c, a, ca);
    v3_cross(ba, ca, nrm);
    const float denom = v3_dot(dir, nrm);
    const float num = v3_dot(a, nrm);
    if (denom == 0.f) continue;
    const float t = num / denom;
    if (!(t > 0.f)) continue;
    float pnt[3] = {dir[0] * t, dir[1] * t, dir[2] * t}, v2[3];
    v3_sub(pnt, a, v2);
    const float d00 = v3_dot(ba, ba), d01 = v3_dot(ba, ca), d11 = v3_dot(ca, ca), d20 = v3_dot(v2, ba), d21 = v3_dot(v2, ca);
    const float den = d00 * d11 - d01 * d01;
    const float v = (d11 * d20 - d01 * d21) / den;
    const float w = (d00 * d21 - d01 * d20) / den;
    const float u = 1.0f - v - w;
    float m = u < v ? u : v;
    if (w < m) m = w;
    if (m > best) {
      best = m;
      for (int k = 0; k < 3; k++) vtx[k] = (int)h->faces[3 * f + k];
      wgt[0] = u;
      wgt[1] = v;
      wgt[2] = w;
    }
  }
}
void orc_hrtf_sample(float sample_rate, const float* dir, float* left, float* right) {
  const HrirSphere* h = hrir_for_rate((uint32_t)sample_rate);
  if (!h) return;
  int vtx[3];
  float wgt[3];
  hrir_locate(h, dir, vtx, wgt);
  for (int i = 0; i < h->len; i++) {
    left[i] = h->left[(size_t)vtx[0] * h->len + i] * wgt[0] + h->left[(size_t)vtx[1] * h->len + i] * wgt[1] +
              h->left[(size_t)vtx[2] * h->len + i] * wgt[2];
    right[i] = h->right[(size_t)vtx[0] * h->len + i] * wgt[0] + h->right[(size_t)vtx[1] * h->len + i] * wgt[1] +
               h->right[(size_t)vtx[2] * h->len + i] * wgt[2];
  }
}
/* HrtfProcessor::process_samples with interpolation_steps = 1 (t = 1: the HRIR and the distance gain of THIS block):
 * out[i] = gain * sum_j hrir[j] * x[i - j], x continued into the previous blocks by prev (hrir_len - 1 samples, the
 * raw input: overlap-save).  The crate evaluates the convolution with an FFT of block + hrir_len - 1 points (639, not
 * a power of two; k = gain / pad_length is the inverse transform's normalisation); here: exact f64 sum, rounded once. */
static void hrtf_process(const HrirSphere* h, float* prev, const float* source, float gain, const float dir[3], float* out_l,
                         float* out_r) {
  const int L = h->len;
  float* hl = (float*)malloc(sizeof(float) * 2 * (size_t)L);
  float* hr = hl + L;
  int vtx[3];
  float wgt[3];
  hrir_locate(h, dir, vtx, wgt);
  for (int i = 0; i < L; i++) {
    hl[i] = h->left[(size_t)vtx[0] * L + i] * wgt[0] + h->left[(size_t)vtx[1] * L + i] * wgt[1] + h->left[(size_t)vtx[2] * L + i] * wgt[2];
    hr[i] = h->right[(size_t)vtx[0] * L + i] * wgt[0] + h->right[(size_t)vtx[1] * L + i] * wgt[1] + h->right[(size_t)vtx[2] * L + i] * wgt[2];
  }
  for (int i = 0; i < RQ; i++) {
    double al = 0., ar = 0.;
    for (int j = 0; j < L; j++) {
      const int k = i - j;
      const double x = k >= 0 ? (double)source[k] : (double)prev[L - 1 + k];
      al += (double)hl[j] * x;
      ar += (double)hr[j] * x;
    }
    out_l[i] = (float)al * gain;
    out_r[i] = (float)ar * gain;
  }
  /* the last hrir_len - 1 raw input samples become the history of the next block */
  if (L - 1 <= RQ) {
    memcpy(prev, source + RQ - (L - 1), sizeof(float) * (size_t)(L - 1));
  } else {
    memmove(prev, prev + RQ, sizeof(float) * (size_t)(L - 1 - RQ));
    memcpy(prev + (L - 1 - RQ), source, sizeof(float) * RQ);
  }
  free(hl);
}

/* src/node/panner.rs:685-904 (equal-power branch :830-897) */
static void process_panner(NodeCfg* n, NodeState* s, uint32_t inst, const Scope* sc) {
  const Quantum* input = &s->in;
  Quantum* output = &s->out;
  if (q_is_silent(input)) {
    /* the HRTF panner has a tail as long as the impulse responses; the counter is never reset (:697-711) */
    int tail = n->hrtf && (uint64_t)n->hrtf->len > s->hrtf_tail_counter;
    if (!tail) {
      q_make_silent(output);
      return;
    }
    s->hrtf_tail_counter += RQ;
  }
  float tmp[15][RQ];
  const float* pv[15];
  int len[15];
  for (int p = 0; p < 15; p++) /* the six params of the node itself may carry an input from the graph (param.rs:739-795) */
    pv[p] = param_get_in(&n->params[p], p < 6 ? s->pin[p] : NULL, inst, sc->quantum, &len[p], tmp[p]);
  int single_valued = 1;
  for (int p = 6; p < 15; p++)
    if (len[p] != 1) single_valued = 0;
  SpatialParams sp_arr[RQ];
  int count = single_valued ? 1 : RQ;
  for (int i = 0; i < count; i++) {
    float spos[3], sori[3], lpos[3], lfw[3], lup[3];
    for (int a = 0; a < 3; a++) {
      spos[a] = pv[a][len[a] == 1 ? 0 : i];
      sori[a] = pv[3 + a][len[3 + a] == 1 ? 0 : i];
      lpos[a] = pv[6 + a][len[6 + a] == 1 ? 0 : i];
      lfw[a] = pv[9 + a][len[9 + a] == 1 ? 0 : i];
      lup[a] = pv[12 + a][len[12 + a] == 1 ? 0 : i];
    }
    sp_arr[i].dist_gain = dist_gain(n, spos, lpos);
    sp_arr[i].cone_gain = cone_gain(n, spos, sori, lpos);
    azimuth_and_elevation(spos, lpos, lfw, lup, &sp_arr[i].azimuth, &sp_arr[i].elevation);
  }
  if (n->hrtf) { /* :781-829: always k-rate, the first value of every param */
    const SpatialParams p0 = sp_arr[0];
    const float new_distance_gain = p0.cone_gain * p0.dist_gain;
    const float az_rad = p0.azimuth * PI_F32 / 180.f, el_rad = p0.elevation * PI_F32 / 180.f;
    float ps[3] = {sinf(az_rad) * cosf(el_rad), sinf(el_rad), cosf(az_rad) * cosf(el_rad)}; /* x, y, z */
    if (fabsf(ps[0]) <= 1e-6f && fabsf(ps[1]) <= 1e-6f && fabsf(ps[2]) <= 1e-6f) {
      ps[0] = ps[1] = 0.f;
      ps[2] = 1.f;
    }
    const float dir[3] = {ps[0], ps[2], ps[1]}; /* Vec3 { x: p[0], z: p[1], y: p[2] }, :246-250 */
    q_copy(output, input);
    float correction = 1.f;
    if (output->n == 2) { /* stereo input: mixed down, doubled afterwards (:800-810) */
      correction *= 2.f;
      q_mix(output, 1, WAA_INTERP_SPEAKERS);
    }
    if (!s->hrtf_prev) s->hrtf_prev = (float*)calloc((size_t)n->hrtf->len, sizeof(float));
    float ol[RQ], orr[RQ];
    hrtf_process(n->hrtf, s->hrtf_prev, output->d[0], new_distance_gain, dir, ol, orr);
    q_set_number_of_channels(output, 2);
    for (int i = 0; i < RQ; i++) {
      output->d[0][i] = correction * ol[i];
      output->d[1][i] = correction * orr[i];
    }
  } else if (input->n == 1) {
    q_copy(output, input);
    q_mix(output, 2, WAA_INTERP_SPEAKERS);
    for (int i = 0; i < RQ; i++)
      apply_mono_to_stereo_gain(sp_arr[single_valued ? 0 : i], &output->d[0][i], &output->d[1][i]);
  } else {
    output->n = 2;
    for (int i = 0; i < RQ; i++)
      apply_stereo_to_stereo_gain(sp_arr[single_valued ? 0 : i], input->d[0][i], input->d[1][i], &output->d[0][i],
                                  &output->d[1][i]);
  }
  output->silent[0] = output->silent[1] = 0;
}

/* src/node/waveshaper.rs:555-573 */
static float apply_curve(const float* curve, uint32_t nn, float input) {
  if (nn == 0) return 0.f;
  float n = (float)nn;
  float v = (n - 1.f) / 2.0f * (input + 1.f);
  if (v <= 0.f) return curve[0];
  if (v >= n - 1.f) return curve[(size_t)(n - 1.f)];
  float k = floorf(v);
  float f = v - k;
  return (1.f - f) * curve[(size_t)k] + f * curve[(size_t)(k + 1.f)];
}
/* src/node/waveshaper.rs:383-487 */
static void process_waveshaper(NodeCfg* n, NodeState* s) {
  const Quantum* input = &s->in;
  Quantum* output = &s->out;
  if (q_is_silent(input) && n->can_propagate_silence) {
    q_make_silent(output);
    return;
  }
  q_copy(output, input);
  if (!n->has_curve) return;
  if (n->os_factor <= 1) { /* OverSampleType::None, :402-407 */
    for (int c = 0; c < output->n; c++) {
      output->silent[c] = 0;
      for (int i = 0; i < RQ; i++) output->d[c][i] = apply_curve(n->curve, n->curve_n, output->d[c][i]);
    }
    return;
  }
  /* X2 / X4 (:408-481): up-sample, shape, down-sample; the resamplers are re-created (= their overlap is lost) when
   * the channel count of the quantum differs from the count they were built for */
  const int up_len = RQ * n->os_factor;
  if (!s->os_up_ovl) {
    s->os_up_ovl = (float*)calloc((size_t)ORC_MAXC * up_len, sizeof(float));
    s->os_dn_ovl = (float*)calloc((size_t)ORC_MAXC * RQ, sizeof(float));
  }
  if (output->n != s->os_channels_m1 + 1) {
    s->os_channels_m1 = output->n - 1;
    memset(s->os_up_ovl, 0, sizeof(float) * (size_t)ORC_MAXC * up_len);
    memset(s->os_dn_ovl, 0, sizeof(float) * (size_t)ORC_MAXC * RQ);
  }
  float up[512];
  for (int c = 0; c < output->n; c++) {
    os_resample_unit(n->os_up, output->d[c], up, s->os_up_ovl + (size_t)c * up_len);
    for (int i = 0; i < up_len; i++) up[i] = apply_curve(n->curve, n->curve_n, up[i]);
    os_resample_unit(n->os_dn, up, output->d[c], s->os_dn_ovl + (size_t)c * RQ);
    output->silent[c] = 0;
  }
}

/* src/node/convolver.rs:343-490 */
static void conv_run(orc_batch* b, NodeState* s, int cv, const float* in, float* out) {
  (void)b;
  conv_process(s->conv[cv], in, out, RQ);
}
static void process_convolver(orc_batch* b, NodeCfg* n, NodeState* s) {
  const Quantum* input = &s->in;
  Quantum* output = &s->out;
  int in_silent = q_is_silent(input);
  if (in_silent) {
    if (s->tail_count >= n->impulse_length) {
      q_make_silent(output);
      return;
    }
    s->tail_count += RQ;
  } else {
    s->tail_count = 0;
  }
  if (!n->has_ir) {
    q_copy(output, input);
    return;
  }
  int ic = input->n, rc = n->impulse_channels;
  if (ic == 1 && rc == 1) {
    output->n = 1;
    conv_run(b, s, 0, input->d[0], output->d[0]);
  } else if (ic == 1 && rc == 2) {
    output->n = 2;
    conv_run(b, s, 0, input->d[0], output->d[0]);
    conv_run(b, s, 1, input->d[0], output->d[1]);
  } else if (ic == 2 && (rc == 1 || rc == 2)) {
    output->n = 2;
    conv_run(b, s, 0, input->d[0], output->d[0]);
    conv_run(b, s, 1, input->d[1], output->d[1]);
  } else if (rc == 4) {
    float o2[RQ], o3[RQ];
    const float* il = input->d[0];
    const float* ir = ic == 2 ? input->d[1] : input->d[0];
    output->n = 2;
    if (ic == 2) {
      conv_run(b, s, 0, il, output->d[0]);
      conv_run(b, s, 1, il, output->d[1]);
      conv_run(b, s, 2, ir, o2);
      conv_run(b, s, 3, ir, o3);
    } else {
      conv_run(b, s, 0, il, output->d[0]);
      conv_run(b, s, 1, il, output->d[1]);
      conv_run(b, s, 2, il, o2);
      conv_run(b, s, 3, il, o3);
    }
    for (int i = 0; i < RQ; i++) output->d[0][i] += o2[i];
    for (int i = 0; i < RQ; i++) output->d[1][i] += o3[i];
  }
  for (int c = 0; c < output->n; c++) output->silent[c] = 0;
}

/* src/node/analyser.rs:265-290 + src/analysis.rs:96-112 */
static void process_analyser(NodeState* s) {
  const Quantum* input = &s->in;
  Quantum* output = &s->out;
  q_copy(output, input);
  Quantum mono;
  q_copy(&mono, input);
  q_mix(&mono, 1, WAA_INTERP_SPEAKERS);
  if (!s->ring) s->ring = (float*)calloc(RING_BUFFER_SIZE, sizeof(float));
  for (int i = 0; i < RQ; i++) s->ring[(s->write_index + (size_t)i) % RING_BUFFER_SIZE] = mono.d[0][i];
  s->write_index += RQ;
  if (s->write_index >= RING_BUFFER_SIZE) s->write_index -= RING_BUFFER_SIZE;
}

static void process_node(orc_batch* b, uint32_t id, uint32_t inst, const Scope* sc) {
  NodeCfg* n = &b->nodes[id];
  NodeState* s = &b->st[inst][id];
  switch (n->desc.kind) {
    case WAA_NODE_DESTINATION: q_copy(&s->out, &s->in); break; /* destination.rs:142-158 */
    case WAA_NODE_BUFFER_SOURCE: process_buffer_source(b, n, s, inst, sc); break;
    case WAA_NODE_CONSTANT_SOURCE: process_constant_source(n, s, inst, sc); break;
    case WAA_NODE_OSCILLATOR: process_oscillator(n, s, inst, sc); break;
    case WAA_NODE_BIQUAD: process_biquad(n, s, inst, sc); break;
    case WAA_NODE_IIR_FILTER: process_iir(n, s); break;
    case WAA_NODE_GAIN: process_gain(n, s, inst, sc); break;
    case WAA_NODE_STEREO_PANNER: process_stereo_panner(n, s, inst, sc); break;
    case WAA_NODE_PANNER: process_panner(n, s, inst, sc); break;
    case WAA_NODE_WAVESHAPER: process_waveshaper(n, s); break;
    case WAA_NODE_CONVOLVER: process_convolver(b, n, s); break;
    case WAA_NODE_ANALYSER: process_analyser(s); break;
    default: q_make_silent(&s->out); break;
  }
}

/* graph.rs:490-591 + thread.rs:355-396, one instance */
static void render_instance(orc_batch* b, uint32_t inst) {
#if defined(__x86_64__)
  /* no_denormals (thread.rs:374-382): FTZ + DAZ while rendering */
  unsigned int saved = _mm_getcsr();
  _mm_setcsr(saved | 0x8040u);
#endif
  NodeState* st = b->st[inst];
  for (uint32_t i = 0; i < b->n_nodes; i++) {
    NodeCfg* n = &b->nodes[i];
    NodeState* s = &st[i];
    q_make_silent(&s->in);
    q_make_silent(&s->out);
    s->ended_q = WAA_ENDED_NEVER;
    if (n->start_time) {
      s->start_time = n->start_time[inst];
      s->stop_time = n->stop_time[inst];
    }
    if (n->desc.kind == WAA_NODE_BUFFER_SOURCE) {
      s->offset = n->offset[inst];
      s->duration = n->duration[inst];
      s->is_looping = n->is_looping[inst];
      s->loop_start = n->loop_start[inst];
      s->loop_end = n->loop_end[inst];
      /* clamp_loop_boundaries, audio_buffer_source.rs:401-417 */
      if (n->bufs[inst].refcnt) {
        double duration = (double)n->bufs[inst].frames / (double)n->bufs[inst].sr;
        if (s->loop_start < 0.)
          s->loop_start = 0.;
        else if (s->loop_start > duration)
          s->loop_start = duration;
        if (s->loop_end <= 0. || s->loop_end > duration) s->loop_end = duration;
      }
    }
    s->last_fft_time = -INFINITY;
  }
  uint64_t num_quanta = (b->length + RQ - 1) / RQ;
  float* out = b->out + (size_t)inst * b->n_out * b->length;
  uint64_t written = 0;
  uint32_t epoch = 0, next_msg = 0;
  for (uint64_t q = 0; q < num_quanta; q++) {
    Scope sc;
    sc.current_frame = q * RQ;
    sc.current_time = (double)sc.current_frame / (double)b->sr;
    sc.sample_rate = b->sr;
    sc.quantum = q;
    /* the suspend point in front of this quantum: control messages first (thread.rs:281-287) */
    for (; next_msg < b->n_msgs && b->msgs[next_msg].q <= q; next_msg++) {
      const CtlMsg* m = &b->msgs[next_msg];
      if (m->inst != WAA_ALL_INSTANCES && m->inst != inst) continue;
      NodeState* ms = &st[m->node];
      if (m->kind == CTL_EVENT) {
        Param* mp = &b->nodes[m->node].params[m->param];
        if (mp->tl && mp->tl[inst]) (void)orc_timeline_event(mp->tl[inst], m->type, m->value, m->t, m->aux, m->curve, m->n_curve);
      } else if (m->kind == CTL_START) { /* AudioScheduledSourceNode::start_at...: onmessage sets the renderer's times */
        ms->start_time = m->t;
        if (b->nodes[m->node].desc.kind == WAA_NODE_BUFFER_SOURCE) {
          ms->offset = m->offset;
          ms->duration = m->duration;
        }
      } else if (m->kind == CTL_STOP) {
        ms->stop_time = m->t;
      }
    }
    while (epoch + 1 < b->n_epochs && b->epochs[epoch + 1].q0 <= q) epoch++;
    const uint32_t* order = b->n_epochs ? b->epochs[epoch].order : b->order;
    const uint32_t n_order = b->n_epochs ? b->epochs[epoch].n_order : b->n_order;
    const unsigned char* active = b->n_epochs ? b->epochs[epoch].active : NULL;
    for (uint32_t i = 0; i < b->n_nodes; i++)
      for (int p = 0; p < b->nodes[i].n_params; p++) param_advance(&b->nodes[i].params[p], inst, q);
    for (uint32_t oi = 0; oi < n_order; oi++) {
      uint32_t item = order[oi], id = item & ~ORC_READER;
      NodeState* s = &st[id];
      if (b->nodes[id].desc.kind == WAA_NODE_DELAY) {
        if (!(item & ORC_READER)) { /* writer half: consumes the input, produces nothing */
          process_delay_writer(&b->nodes[id], s, &sc);
          q_make_silent(&s->in);
          continue;
        }
        process_delay_reader(&b->nodes[id], s, inst, &sc);
      } else {
        process_node(b, id, inst, &sc);
      }
      if (b->dbg_codes) /* debugging aid (ORC_DUMP_CODES): number_of_channels | 0x80 if silent, per node and quantum */
        b->dbg_codes[((size_t)inst * b->n_nodes + id) * num_quanta + q] = (unsigned char)(s->out.n | (q_is_silent(&s->out) ? 0x80 : 0));
      for (uint32_t e = 0; e < b->n_edges; e++) {
        if (b->edges[e].from != id || (active && !active[e])) continue;
        NodeCfg* dn = &b->nodes[b->edges[e].to];
        NodeState* ds = &st[b->edges[e].to];
        uint32_t ti = b->edges[e].to_input;
        if (ti & 0x80000000u) /* AudioParam node: channel count 1, explicit, discrete (param.rs:309-311) */
          q_add(ds->pin[ti & 0x7fffffffu], &s->out, 1, WAA_COUNT_MODE_EXPLICIT, WAA_INTERP_DISCRETE);
        else
          q_add(&ds->in, &s->out, dn->cc, dn->ccmode, dn->ccinterp);
      }
      if (b->nodes[id].desc.kind != WAA_NODE_DELAY) q_make_silent(&s->in);
      for (int p = 0; p < WAA_MAX_PARAMS; p++)
        if (s->pin[p]) q_make_silent(s->pin[p]);
    }
    const Quantum* rendered = &st[0].out;
    uint64_t remaining = b->length - written;
    if (remaining > RQ) remaining = RQ;
    for (uint32_t c = 0; c < b->n_out; c++) {
      float* dst = out + (size_t)c * b->length + written;
      if ((int)c < rendered->n)
        memcpy(dst, rendered->d[c], sizeof(float) * remaining);
      else
        memset(dst, 0, sizeof(float) * remaining);
    }
    written += remaining;
  }
  { /* unload_graph -> before_drop (thread.rs:398-411; audio_buffer_source.rs:872-878, constant_source.rs:280-286,
     * oscillator.rs:502-508) with the time after the last quantum */
    double end_time = (double)(num_quanta * RQ) / (double)b->sr;
    for (uint32_t i = 0; i < b->n_nodes; i++) {
      uint32_t kind = b->nodes[i].desc.kind;
      if (kind != WAA_NODE_BUFFER_SOURCE && kind != WAA_NODE_CONSTANT_SOURCE && kind != WAA_NODE_OSCILLATOR) continue;
      NodeState* s = &st[i];
      if (s->ended_q < 0 && (end_time >= s->start_time || end_time >= s->stop_time)) s->ended_q = WAA_ENDED_AT_UNLOAD;
    }
  }
#if defined(__x86_64__)
  _mm_setcsr(saved);
#endif
}

typedef struct {
  orc_batch* b;
  uint32_t lo, hi, stride;
} Work;
static void* worker(void* p) {
  Work* w = (Work*)p;
  for (uint32_t k = w->lo; k < w->hi; k += w->stride) render_instance(w->b, k);
  return NULL;
}

/* oracle-only knob: number of host threads used by orc_render (one context per thread,
 * the reference's CPU-parallel pattern, SURVEY.md §8b Threading) */
waa_status orc_set_threads(orc_batch* b, int32_t n) {
  if (!b || n < 1) return fail(WAA_ERR_INVALID_ARGUMENT, "bad thread count");
  b->n_threads = n;
  return WAA_OK;
}

/* waa_batch_rearm: the product library's "same graph, new audio" entry point.  The interpreter has no plan to keep: a batch is put
 * back in front of its render (orc_rewind's state reset) and then takes new source buffers like a fresh one.  Unlike the product,
 * it accepts a graph whose source playbackRate / detune or panner position is driven from the graph: it renders those params anew
 * on every render, where the product's plan holds the values rendered at plan time and refuses the re-arm. */
waa_status orc_rewind(orc_batch* b);
waa_status orc_batch_rearm(orc_batch* b) {
  if (!b) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch");
  if (!b->rendered) return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - nothing to re-arm: the batch has not been rendered");
  int e = orc_rewind(b);
  if (e) return e;
  b->rendered = 0;
  return WAA_OK;
}
waa_status orc_render(orc_batch* b);
/* waa_render_range: the quantum loop with its suspend points (thread.rs:277-294).  The interpreter renders when the last range
 * arrives, like the product library, and applies every control message in front of the quantum it was submitted at. */
waa_status orc_render_range(orc_batch* b, uint64_t quantum0, uint32_t n_quanta) {
  if (!b) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch");
  if (b->rendered) return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - the batch is frozen once rendering has started");
  uint32_t nq = (uint32_t)((b->length + RQ - 1) / RQ);
  if (quantum0 != b->ctl_q)
    return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - ranges are consecutive: the next one starts at quantum %u, not %llu", b->ctl_q,
                (unsigned long long)quantum0);
  if (n_quanta == 0 || quantum0 + n_quanta > nq)
    return fail(WAA_ERR_INVALID_ARGUMENT, "RangeError - quanta [%llu, %llu) of a render of %u", (unsigned long long)quantum0,
                (unsigned long long)(quantum0 + n_quanta), nq);
  b->ranged = 1;
  b->ctl_q = (uint32_t)(quantum0 + n_quanta);
  if (b->ctl_q < nq) return WAA_OK;
  return orc_render(b);
}
static int orc_check_edge(orc_batch* b, uint32_t from, uint32_t from_output, uint32_t to, uint32_t to_input) {
  if (!b) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch");
  if (from >= b->n_nodes || to >= b->n_nodes || from_output != 0 || (to_input != 0 && !(to_input & 0x80000000u)))
    return fail(WAA_ERR_INVALID_ARGUMENT, "IndexSizeError - invalid edge %u:%u -> %u:%u", from, from_output, to, to_input);
  if ((to_input & 0x80000000u) && (int)(to_input & 0x7fffffffu) >= b->nodes[to].n_params)
    return fail(WAA_ERR_INVALID_ARGUMENT, "no such param %u on node %u", to_input & 0x7fffffffu, to);
  if (b->rendered) return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - the batch is frozen once rendering has started");
  return 0;
}
waa_status orc_connect(orc_batch* b, uint32_t from, uint32_t from_output, uint32_t to, uint32_t to_input) {
  int e;
  if ((e = orc_check_edge(b, from, from_output, to, to_input))) return e;
  for (uint32_t k = 0; k < b->n_edges; k++) {
    const waa_edge_desc* ed = &b->edges[k];
    if (ed->from == from && ed->from_output == from_output && ed->to == to && ed->to_input == to_input && b->edge_off[k] == ORC_EDGE_NEVER) return WAA_OK;
  }
  if (b->n_edges == b->edge_cap) {
    uint32_t cap = 2 * b->edge_cap;
    b->edges = (waa_edge_desc*)realloc(b->edges, sizeof(waa_edge_desc) * cap);
    b->edge_on = (uint32_t*)realloc(b->edge_on, sizeof(uint32_t) * cap);
    b->edge_off = (uint32_t*)realloc(b->edge_off, sizeof(uint32_t) * cap);
    b->edge_cap = cap;
  }
  waa_edge_desc ed = {from, from_output, to, to_input};
  b->edges[b->n_edges] = ed;
  b->edge_on[b->n_edges] = b->ctl_q;
  b->edge_off[b->n_edges] = ORC_EDGE_NEVER;
  b->n_edges++;
  if (to_input & 0x80000000u) { /* node.connect(&param): the param's audio-rate input (param.rs:300-320) */
    uint32_t pid = to_input & 0x7fffffffu;
    for (uint32_t k = 0; k < b->n_inst; k++)
      if (!b->st[k][to].pin[pid]) {
        b->st[k][to].pin[pid] = (Quantum*)malloc(sizeof(Quantum));
        q_make_silent(b->st[k][to].pin[pid]);
      }
  }
  if (b->ctl_q == 0) order_nodes(b);
  return WAA_OK;
}
waa_status orc_disconnect(orc_batch* b, uint32_t from, uint32_t from_output, uint32_t to, uint32_t to_input) {
  int e;
  if ((e = orc_check_edge(b, from, from_output, to, to_input))) return e;
  for (uint32_t k = b->n_edges; k-- > 0;) {
    const waa_edge_desc* ed = &b->edges[k];
    if (!(ed->from == from && ed->from_output == from_output && ed->to == to && ed->to_input == to_input) || b->edge_off[k] != ORC_EDGE_NEVER) continue;
    if (b->edge_on[k] >= b->ctl_q) { /* made and cut at the same point */
      for (uint32_t j = k; j + 1 < b->n_edges; j++) {
        b->edges[j] = b->edges[j + 1];
        b->edge_on[j] = b->edge_on[j + 1];
        b->edge_off[j] = b->edge_off[j + 1];
      }
      b->n_edges--;
      b->edge_off[b->n_edges] = ORC_EDGE_NEVER;
      b->edge_on[b->n_edges] = 0;
    } else {
      b->edge_off[k] = b->ctl_q;
    }
    if (b->ctl_q == 0) order_nodes(b);
    return WAA_OK;
  }
  return fail(WAA_ERR_INVALID_ARGUMENT, "InvalidAccessError - attempting to disconnect unconnected nodes");
}

waa_status orc_render(orc_batch* b) {
  if (!b) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch");
  if (b->rendered) /* offline.rs:163 */
    return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - Cannot call `startRendering` twice");
  for (uint32_t i = 0; i < b->n_nodes; i++) /* the reference takes the coefficients in the constructor */
    if (b->nodes[i].desc.kind == WAA_NODE_IIR_FILTER && b->nodes[i].iir_len == 0)
      return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - IIRFilterNode %u has no coefficients", i);
  if (b->ranged && b->ctl_q < (uint32_t)((b->length + RQ - 1) / RQ))
    return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - a ranged render is in progress (suspended in front of quantum %u)", b->ctl_q);
  b->rendered = 1;
  { /* the graph's epochs: the connections change at the suspend points, and with them the render order (graph.rs:490-500:
     * the graph is re-ordered whenever an edge was added or removed) */
    uint32_t nq = (uint32_t)((b->length + RQ - 1) / RQ), n_pts = 0;
    uint32_t* pts = (uint32_t*)malloc(sizeof(uint32_t) * (2 * b->n_edges + 2));
    pts[n_pts++] = 0;
    for (uint32_t e = 0; e < b->n_edges; e++) {
      if (b->edge_on[e] > 0 && b->edge_on[e] < nq) pts[n_pts++] = b->edge_on[e];
      if (b->edge_off[e] != ORC_EDGE_NEVER && b->edge_off[e] < nq) pts[n_pts++] = b->edge_off[e];
    }
    for (uint32_t i = 1; i < n_pts; i++) /* insertion sort, then unique */
      for (uint32_t j = i; j > 0 && pts[j - 1] > pts[j]; j--) {
        uint32_t t = pts[j];
        pts[j] = pts[j - 1];
        pts[j - 1] = t;
      }
    uint32_t nu = 0;
    for (uint32_t i = 0; i < n_pts; i++)
      if (nu == 0 || pts[nu - 1] != pts[i]) pts[nu++] = pts[i];
    if (nu > 1 || b->n_msgs) {
      b->epochs = (Epoch*)calloc(nu, sizeof(Epoch));
      b->n_epochs = nu;
      uint32_t* keep_order = b->order;
      uint32_t keep_n = b->n_order;
      for (uint32_t k = 0; k < nu; k++) {
        Epoch* ep = &b->epochs[k];
        ep->q0 = pts[k];
        ep->active = (unsigned char*)calloc(b->n_edges ? b->n_edges : 1, 1);
        for (uint32_t e = 0; e < b->n_edges; e++) ep->active[e] = b->edge_on[e] <= ep->q0 && ep->q0 < b->edge_off[e];
        ep->order = (uint32_t*)malloc(sizeof(uint32_t) * (2 * b->n_nodes + 2));
        b->order = ep->order;
        b->edge_active = ep->active;
        order_nodes(b);
        ep->n_order = b->n_order;
      }
      b->order = keep_order;
      b->n_order = keep_n;
      b->edge_active = NULL;
    }
    free(pts);
  }
  const char* dump = getenv("ORC_DUMP_CODES");
  uint64_t dbg_nq = (b->length + RQ - 1) / RQ;
  if (dump) {
    free(b->dbg_codes);
    b->dbg_codes = (unsigned char*)malloc((size_t)b->n_inst * b->n_nodes * (dbg_nq ? dbg_nq : 1));
    memset(b->dbg_codes, 0xFF, (size_t)b->n_inst * b->n_nodes * (dbg_nq ? dbg_nq : 1));
  }
  int nt = b->n_threads;
  if ((uint32_t)nt > b->n_inst) nt = (int)b->n_inst;
  if (nt <= 1) {
    for (uint32_t k = 0; k < b->n_inst; k++) render_instance(b, k);
  } else {
    pthread_t* th = (pthread_t*)malloc(sizeof(pthread_t) * nt);
    Work* w = (Work*)malloc(sizeof(Work) * nt);
    for (int t = 0; t < nt; t++) {
      w[t].b = b;
      w[t].lo = (uint32_t)t;
      w[t].hi = b->n_inst;
      w[t].stride = (uint32_t)nt;
      pthread_create(&th[t], NULL, worker, &w[t]);
    }
    for (int t = 0; t < nt; t++) pthread_join(th[t], NULL);
    free(th);
    free(w);
  }
  if (dump && b->dbg_codes) {
    FILE* f = fopen(dump, "wb");
    if (f) {
      uint32_t hdr[3] = {b->n_inst, b->n_nodes, (uint32_t)dbg_nq};
      fwrite(hdr, sizeof hdr, 1, f);
      fwrite(b->dbg_codes, 1, (size_t)b->n_inst * b->n_nodes * dbg_nq, f);
      fclose(f);
    }
  }
  return WAA_OK;
}
/* oracle-only TIMING aid (bench.py cpu_baseline): puts a rendered batch back into its pre-render state (every
 * renderer's state zeroed, convolver and delay lines cleared) so that the same batch can be rendered again under the
 * stopwatch; the rewind itself is outside the timed region.  Refused for batches with scheduled automation (the
 * timelines are consumed by the first render). */
waa_status orc_rewind(orc_batch* b) {
  if (!b) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch");
  for (uint32_t i = 0; i < b->n_nodes; i++)
    for (int p = 0; p < b->nodes[i].n_params; p++)
      if (b->nodes[i].params[p].tl) return fail(WAA_ERR_INVALID_STATE, "orc_rewind: batch has automation timelines");
  for (uint32_t k = 0; k < b->n_inst; k++)
    for (uint32_t i = 0; i < b->n_nodes; i++) {
      NodeState* s = &b->st[k][i];
      Quantum* pin[WAA_MAX_PARAMS];
      ConvState* conv[4];
      memcpy(pin, s->pin, sizeof pin);
      memcpy(conv, s->conv, sizeof conv);
      free(s->ring);
      free(s->dl_ring);
      free(s->last_fft_output);
      free(s->os_up_ovl);
      free(s->os_dn_ovl);
      free(s->hrtf_prev);
      memset(s, 0, sizeof *s);
      memcpy(s->pin, pin, sizeof pin);
      for (int p = 0; p < WAA_MAX_PARAMS; p++)
        if (s->pin[p]) q_make_silent(s->pin[p]);
      for (int c = 0; c < 4; c++) {
        ConvState* cs = conv[c];
        s->conv[c] = cs;
        if (!cs || cs->ir->seg_count == 0) continue;
        const ConvIR* ir = cs->ir;
        memset(cs->seg_re, 0, (size_t)ir->seg_count * ir->csize * sizeof(float));
        memset(cs->seg_im, 0, (size_t)ir->seg_count * ir->csize * sizeof(float));
        memset(cs->pre_re, 0, ir->csize * sizeof(float));
        memset(cs->pre_im, 0, ir->csize * sizeof(float));
        memset(cs->conv_re, 0, ir->csize * sizeof(float));
        memset(cs->conv_im, 0, ir->csize * sizeof(float));
        memset(cs->fftbuf, 0, ir->seg * sizeof(float));
        memset(cs->overlap, 0, ir->block * sizeof(float));
        memset(cs->inbuf, 0, ir->block * sizeof(float));
        cs->inbuf_fill = 0;
        cs->current = 0;
      }
    }
  b->rendered = 0;
  return WAA_OK;
}
waa_status orc_sync(orc_batch* b) {
  (void)b;
  return WAA_OK;
}
waa_status orc_download(orc_batch* b, uint32_t inst, uint32_t ch, float* dst, uint64_t frames) {
  if (!b || inst >= b->n_inst || ch >= b->n_out || frames > b->length)
    return fail(WAA_ERR_INVALID_ARGUMENT, "download out of range");
  if (!b->rendered) return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - nothing rendered yet");
  memcpy(dst, b->out + ((size_t)inst * b->n_out + ch) * b->length, sizeof(float) * frames);
  return WAA_OK;
}
waa_status orc_download_all(orc_batch* b, float* dst) {
  if (!b) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch");
  if (!b->rendered) return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - nothing rendered yet");
  memcpy(dst, b->out, sizeof(float) * (size_t)b->n_inst * b->n_out * b->length);
  return WAA_OK;
}
/* waa_download_all_pcm16: sample * 32768 rounded to nearest (ties to even, like the device's cvt), saturated, NaN -> 0 */
waa_status orc_download_all_pcm16(orc_batch* b, int16_t* dst) {
  if (!b || !dst) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch / destination");
  for (uint32_t i = 0; i < b->n_inst; i++)
    for (uint64_t f = 0; f < b->length; f++)
      for (uint32_t c = 0; c < b->n_out; c++) {
        float v = b->out[((size_t)i * b->n_out + c) * b->length + f] * 32768.f;
        v = v < -32768.f ? -32768.f : (v > 32767.f ? 32767.f : v);
        dst[((size_t)i * b->length + f) * b->n_out + c] = (int16_t)lrintf(v != v ? 0.f : v);
      }
  return WAA_OK;
}
/* waa_shard_range / waa_render_sharded: the same partition and the same callbacks, sub-batch after sub-batch on the
 * calling thread (the `devices` are only passed through to the callbacks) — lets the tests exercise hosts written against
 * the N-device entry point without a GPU. */
static void orc_split(uint32_t n, uint32_t part, uint32_t parts, uint32_t* lo, uint32_t* hi) {
  uint32_t base = n / parts, rem = n % parts;
  *lo = part * base + (part < rem ? part : rem);
  *hi = *lo + base + (part < rem ? 1u : 0u);
}
waa_status orc_shard_range(uint32_t n_total, uint32_t part, uint32_t n_parts, uint32_t* first, uint32_t* end) {
  if (!first || !end || n_parts == 0 || part >= n_parts) return fail(WAA_ERR_INVALID_ARGUMENT, "bad shard index %u of %u", part, n_parts);
  orc_split(n_total, part, n_parts, first, end);
  return WAA_OK;
}
/* waa_sharded_in_flight bounds device memory inside the product's pipeline; the oracle renders one sub-batch at a time anyway */
waa_status orc_sharded_in_flight(uint32_t max_sub_batches_per_device) {
  (void)max_sub_batches_per_device;
  return WAA_OK;
}
waa_status orc_render_sharded(const waa_sharded_job* job, double* seconds) {
  if (!job || !job->graph) return fail(WAA_ERR_INVALID_ARGUMENT, "null job / graph");
  if (job->n_instances == 0) return fail(WAA_ERR_INVALID_ARGUMENT, "a sharded job needs at least one context");
  if (!job->devices || job->n_devices == 0) return fail(WAA_ERR_INVALID_ARGUMENT, "a sharded job needs at least one device");
  if (!job->host_out) return fail(WAA_ERR_INVALID_ARGUMENT, "null output buffer");
  int streamed = job->source_node != WAA_NO_NODE;
  if (streamed && (!job->host_in || job->in_channels == 0 || job->in_channels > WAA_MAX_CHANNELS))
    return fail(WAA_ERR_INVALID_ARGUMENT, "the streamed source needs host_in and 1..%d channels", WAA_MAX_CHANNELS);
  size_t row_in = (size_t)job->in_channels * job->in_frames * (job->in_pcm16 ? sizeof(int16_t) : sizeof(float));
  size_t row_out = (size_t)job->n_channels_out * job->length_frames * (job->out_pcm16 ? sizeof(int16_t) : sizeof(float));
  uint32_t sub = job->sub_batches ? job->sub_batches : 1;
  struct timespec t0, t1;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  waa_status first_error = WAA_OK;
  char msg[512] = "";
  for (uint32_t di = 0; di < job->n_devices; di++) {
    uint32_t lo, hi;
    orc_split(job->n_instances, di, job->n_devices, &lo, &hi);
    uint32_t parts = hi - lo < sub ? hi - lo : sub;
    if (parts == 0) parts = 1;
    for (uint32_t p = 0; p < parts; p++) {
      uint32_t a, e;
      orc_split(hi - lo, p, parts, &a, &e);
      if (e <= a) continue;
      uint32_t first = lo + a, count = e - a;
      orc_batch* b = NULL;
      waa_status st = orc_batch_create(job->graph, count, job->n_channels_out, job->length_frames, job->sample_rate, job->devices[di], &b);
      if (!st && job->setup) st = job->setup((waa_batch*)b, first, count, job->devices[di], job->user);
      if (!st && streamed) {
        const char* src = (const char*)job->host_in + (size_t)first * row_in;
        st = job->in_pcm16 ? orc_source_set_buffer_pcm16_batch(b, job->source_node, (const int16_t*)src, job->in_channels, job->in_frames,
                                                               job->in_sample_rate)
                           : orc_source_set_buffer_batch(b, job->source_node, (const float*)src, job->in_channels, job->in_frames,
                                                         job->in_sample_rate);
      }
      if (!st) st = orc_render(b);
      if (!st && job->pull) st = job->pull((waa_batch*)b, first, count, job->devices[di], job->user);
      if (!st) {
        char* dst = (char*)job->host_out + (size_t)first * row_out;
        st = job->out_pcm16 ? orc_download_all_pcm16(b, (int16_t*)dst) : orc_download_all(b, (float*)dst);
      }
      if (st && first_error == WAA_OK) {
        first_error = st;
        snprintf(msg, sizeof msg, "%s", orc_last_error());
      }
      if (b) orc_batch_destroy(b);
    }
  }
  clock_gettime(CLOCK_MONOTONIC, &t1);
  if (seconds) *seconds = (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
  if (first_error != WAA_OK) return fail(first_error, "%s", msg);
  return WAA_OK;
}
waa_status orc_output_device(orc_batch* b, const float** p, uint64_t* is, uint64_t* cs) {
  if (!b) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch");
  *p = b->out;
  *is = (uint64_t)b->n_out * b->length;
  *cs = b->length;
  return WAA_OK;
}

/* ------------------------------------------------------------------------------------ */
/* Analyser control side (src/analysis.rs:14-24, 114-127, 261-401)                        */
/* ------------------------------------------------------------------------------------ */
static void ring_read(const NodeState* s, float* dst, size_t dst_len, size_t max_len) {
  size_t len = dst_len < max_len ? dst_len : max_len;
  for (size_t i = 0; i < len; i++) {
    size_t pos = (RING_BUFFER_SIZE + s->write_index - len + i) % RING_BUFFER_SIZE;
    dst[i] = s->ring ? s->ring[pos] : 0.f;
  }
}
static void analyser_compute_fft(NodeCfg* n, NodeState* s) {
  int fft_size = n->desc.i[0];
  float stc = (float)n->desc.d[0];
  float* input = (float*)calloc(fft_size, sizeof(float));
  ring_read(s, input, fft_size, fft_size);
  /* generate_blackman analysis.rs:14-24 (f32) */
  const float alpha = 0.16f;
  const float a0 = (1.f - alpha) / 2.f, a1 = 1.f / 2.f, a2 = alpha / 2.f;
  for (int i = 0; i < fft_size; i++) {
    float w = a0 - a1 * cosf(2.f * PI_F32 * (float)i / (float)fft_size) + a2 * cosf(4.f * PI_F32 * (float)i / (float)fft_size);
    input[i] *= w;
  }
  RfftPlan* plan = rfft_plan_new(fft_size);
  float* re = (float*)malloc(sizeof(float) * (fft_size / 2 + 1));
  float* im = (float*)malloc(sizeof(float) * (fft_size / 2 + 1));
  float* sre = (float*)malloc(sizeof(float) * (fft_size / 2 + 1));
  float* sim = (float*)malloc(sizeof(float) * (fft_size / 2 + 1));
  rfft_forward(plan, sre, sim, input, re, im);
  free(sre);
  free(sim);
  if (!s->last_fft_output) s->last_fft_output = (float*)calloc(MAX_FFT_SIZE / 2 + 1, sizeof(float));
  float nf = 1.f / (float)fft_size;
  for (int k = 0; k < fft_size / 2; k++) {
    float norm = hypotf(re[k], im[k]) * nf;
    float value = stc * s->last_fft_output[k] + (1.f - stc) * norm;
    s->last_fft_output[k] = isfinite(value) ? value : 0.f;
  }
  rfft_plan_free(plan);
  free(re);
  free(im);
  free(input);
}
static int analyser_prepare(orc_batch* b, uint32_t node, uint32_t inst, NodeCfg** n, NodeState** s, int freq) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_ANALYSER))) return e;
  if (inst >= b->n_inst) return fail(WAA_ERR_INVALID_ARGUMENT, "instance out of range");
  *n = &b->nodes[node];
  *s = &b->st[inst][node];
  if (freq) {
    /* current_time after the render = frames_played / sample_rate */
    uint64_t frames_played = b->rendered ? ((b->length + RQ - 1) / RQ) * RQ : 0;
    double current_time = (double)frames_played / (double)b->sr;
    if (current_time != (*s)->last_fft_time) {
      analyser_compute_fft(*n, *s);
      (*s)->last_fft_time = current_time;
    }
  }
  return 0;
}
waa_status orc_analyser_get_float_frequency_data(orc_batch* b, uint32_t node, uint32_t inst, float* dst, uint32_t nn) {
  NodeCfg* n;
  NodeState* s;
  int e;
  if ((e = analyser_prepare(b, node, inst, &n, &s, 1))) return e;
  uint32_t bins = (uint32_t)n->desc.i[0] / 2;
  uint32_t len = nn < bins ? nn : bins;
  for (uint32_t k = 0; k < len; k++) dst[k] = 20.f * log10f(s->last_fft_output[k]);
  return WAA_OK;
}
waa_status orc_analyser_get_byte_frequency_data(orc_batch* b, uint32_t node, uint32_t inst, uint8_t* dst, uint32_t nn) {
  NodeCfg* n;
  NodeState* s;
  int e;
  if ((e = analyser_prepare(b, node, inst, &n, &s, 1))) return e;
  float mind = (float)n->desc.d[1], maxd = (float)n->desc.d[2];
  uint32_t bins = (uint32_t)n->desc.i[0] / 2;
  uint32_t len = nn < bins ? nn : bins;
  for (uint32_t k = 0; k < len; k++) {
    float db = 20.f * log10f(s->last_fft_output[k]);
    float scaled = 255.f / (maxd - mind) * (db - mind);
    float clamped = scaled < 0.f ? 0.f : scaled > 255.f ? 255.f : scaled; /* NaN -> Rust clamp keeps NaN -> `as u8` = 0 */
    dst[k] = isnan(scaled) ? 0 : (uint8_t)clamped;
  }
  return WAA_OK;
}
waa_status orc_analyser_get_float_time_domain_data(orc_batch* b, uint32_t node, uint32_t inst, float* dst, uint32_t nn) {
  NodeCfg* n;
  NodeState* s;
  int e;
  if ((e = analyser_prepare(b, node, inst, &n, &s, 0))) return e;
  ring_read(s, dst, nn, (size_t)n->desc.i[0]);
  return WAA_OK;
}
waa_status orc_analyser_get_byte_time_domain_data(orc_batch* b, uint32_t node, uint32_t inst, uint8_t* dst, uint32_t nn) {
  NodeCfg* n;
  NodeState* s;
  int e;
  if ((e = analyser_prepare(b, node, inst, &n, &s, 0))) return e;
  float* tmp = (float*)calloc(nn ? nn : 1, sizeof(float));
  ring_read(s, tmp, nn, (size_t)n->desc.i[0]);
  for (uint32_t i = 0; i < nn; i++) {
    float scaled = 128.f * (1.f + tmp[i]);
    float clamped = scaled < 0.f ? 0.f : scaled > 255.f ? 255.f : scaled;
    dst[i] = (uint8_t)clamped;
  }
  free(tmp);
  return WAA_OK;
}

/* the batch forms of the boundary (include/waa_hip.h): here simply the per-context pulls a caller of the reference
 * runs, one after the other (src/node/analyser.rs:228-258); dst rows of nn elements */
waa_status orc_analyser_get_float_frequency_data_batch(orc_batch* b, uint32_t node, float* dst, uint32_t nn) {
  if (!b) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch");
  for (uint32_t i = 0; i < b->n_inst; i++) {
    int e = orc_analyser_get_float_frequency_data(b, node, i, dst + (size_t)i * nn, nn);
    if (e) return e;
  }
  return WAA_OK;
}
waa_status orc_analyser_get_byte_frequency_data_batch(orc_batch* b, uint32_t node, uint8_t* dst, uint32_t nn) {
  if (!b) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch");
  for (uint32_t i = 0; i < b->n_inst; i++) {
    int e = orc_analyser_get_byte_frequency_data(b, node, i, dst + (size_t)i * nn, nn);
    if (e) return e;
  }
  return WAA_OK;
}
waa_status orc_analyser_get_float_time_domain_data_batch(orc_batch* b, uint32_t node, float* dst, uint32_t nn) {
  if (!b) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch");
  for (uint32_t i = 0; i < b->n_inst; i++) {
    int e = orc_analyser_get_float_time_domain_data(b, node, i, dst + (size_t)i * nn, nn);
    if (e) return e;
  }
  return WAA_OK;
}
waa_status orc_analyser_get_byte_time_domain_data_batch(orc_batch* b, uint32_t node, uint8_t* dst, uint32_t nn) {
  if (!b) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch");
  for (uint32_t i = 0; i < b->n_inst; i++) {
    int e = orc_analyser_get_byte_time_domain_data(b, node, i, dst + (size_t)i * nn, nn);
    if (e) return e;
  }
  return WAA_OK;
}

/* ------------------------------------------------------------------------------------ */
/* oracle-only helpers                                                                    */
/* ------------------------------------------------------------------------------------ */

/* exact (f64) direct linear convolution, truncated to n_out: the mathematical definition
 * the partitioned f32 FFT convolver approximates */
void orc_convolve_exact(const float* x, uint64_t nx, const float* h, uint64_t nh, double* y, uint64_t n_out) {
  for (uint64_t n = 0; n < n_out; n++) {
    double acc = 0.;
    uint64_t kmin = n >= nx ? n - nx + 1 : 0;
    uint64_t kmax = n < nh - 1 ? n : nh - 1;
    if (nh == 0) {
      y[n] = 0.;
      continue;
    }
    for (uint64_t k = kmin; k <= kmax; k++) acc += (double)h[k] * (double)x[n - k];
    y[n] = acc;
  }
}
/* stand-alone access to the restated FFTConvolver (for validating it against the exact one) */
void orc_fftconvolver_run(const float* ir, uint64_t ir_len, const float* x, uint64_t nx, float* y) {
  ConvIR* c = convir_new(RQ * 8, ir, ir_len);
  ConvState* s = convstate_new(c);
  uint64_t done = 0;
  float in[RQ], out[RQ];
  while (done < nx) {
    uint64_t n = nx - done < RQ ? nx - done : RQ;
    memset(in, 0, sizeof in);
    memcpy(in, x + done, sizeof(float) * n);
    conv_process(s, in, out, RQ);
    memcpy(y + done, out, sizeof(float) * n);
    done += n;
  }
  convstate_free(s);
  convir_free(c);
}

/* pure helpers exposed for the known-answer tests */
void orc_biquad_coefs(int32_t type, float sample_rate, float frequency, float detune, float q, float gain, double* out5) {
  Coefs c = calculate_coefs(type, (double)sample_rate, (double)get_computed_freq(frequency, detune), (double)gain, (double)q);
  out5[0] = c.b0;
  out5[1] = c.b1;
  out5[2] = c.b2;
  out5[3] = c.a1;
  out5[4] = c.a2;
}
float orc_get_computed_freq(float f, float d) { return get_computed_freq(f, d); }
void orc_azimuth_elevation(const float* sp, const float* lp, const float* lf, const float* lu, float* az, float* el) {
  azimuth_and_elevation(sp, lp, lf, lu, az, el);
}
float orc_spatial_angle(const float* sp, const float* so, const float* lp) { return spatial_angle(sp, so, lp); }
float orc_spatial_distance(const float* sp, const float* lp) {
  float r[3];
  v3_sub(sp, lp, r);
  return v3_len(r);
}
float orc_apply_curve(const float* curve, uint32_t n, float x) { return apply_curve(curve, n, x); }
void orc_blackman(uint32_t size, float* out) {
  const float alpha = 0.16f;
  const float a0 = (1.f - alpha) / 2.f, a1 = 1.f / 2.f, a2 = alpha / 2.f;
  for (uint32_t i = 0; i < size; i++)
    out[i] = a0 - a1 * cosf(2.f * PI_F32 * (float)i / (float)size) + a2 * cosf(4.f * PI_F32 * (float)i / (float)size);
}
/* AudioRenderQuantum::mix on a bare [n_from][128] block -> [n_to][128] */
void orc_mix(const float* in, uint32_t from, uint32_t to, int32_t interp, float* out) {
  Quantum q;
  q.n = (int)from;
  for (uint32_t c = 0; c < from; c++) {
    memcpy(q.d[c], in + (size_t)c * RQ, sizeof(float) * RQ);
    q.silent[c] = 0;
  }
  q_mix(&q, (int)to, interp);
  for (uint32_t c = 0; c < to; c++) memcpy(out + (size_t)c * RQ, q.d[c], sizeof(float) * RQ);
}

waa_status orc_plan_describe(orc_batch* b, char* buf, size_t cap, size_t* needed) {
  const char* text = "oracle: quantum-major interpreter (no launch plan)\n";
  (void)b;
  if (needed) *needed = strlen(text);
  if (buf && cap) {
    strncpy(buf, text, cap - 1);
    buf[cap - 1] = 0;
  }
  return WAA_OK;
}

/* measurement API parity with the product (no-ops) */
waa_status orc_profile_enable(orc_batch* b, int32_t on) {
  (void)b;
  (void)on;
  return WAA_OK;
}
int32_t orc_profile_count(orc_batch* b) {
  (void)b;
  return 0;
}
waa_status orc_profile_get(orc_batch* b, int32_t i, const char** name, uint64_t* launches, double* ms) {
  (void)b;
  (void)i;
  (void)name;
  (void)launches;
  (void)ms;
  return fail(WAA_ERR_INVALID_ARGUMENT, "no profile entries in the oracle");
}
waa_status orc_profile_reset(orc_batch* b) {
  (void)b;
  return WAA_OK;
}
