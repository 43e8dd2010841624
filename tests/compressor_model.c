/* compressor_model.c — test infrastructure: DynamicsCompressorRenderer::process (the reference's
 * src/node/dynamics_compressor.rs:330-479) restated in C from the reference's text, twice:
 *
 *   model_f32  every operation in f32, in the reference's order, unfused, with the C library's log10f / powf / expf (what
 *              Rust's f32::log10 / powf / exp call) and FTZ + DAZ set while it runs (thread.rs:374-382): the reference's
 *              arithmetic.
 *   model_f64  the same algorithm with every operation in f64: the yardstick for how far f32 arithmetic strays from the
 *              mathematics (tests/test_compressor.py computes its tolerance from the two).
 *
 * Both take the node's INPUT (what the graph in front of it rendered) and return its output.
 *   in        [n_ch][frames] f32, n_ch 1 or 2, frames a multiple of 128
 *   params    [n_quanta][5] f32: threshold, knee, ratio, attack, release as the k-rate AudioParams deliver them (index 0 of
 *             the quantum's slice, already clamped to the param's range)
 *   live      [n_quanta] bytes or NULL: 0 = the input quantum is the SILENT quantum (one channel aliasing the zero buffer,
 *             quantum.rs:254-256) and not merely zeros: a silent delayed quantum leaves the node as silence without a
 *             multiplication (:463-468).  NULL = every quantum is live.
 *   out       [n_ch][frames] f32
 * Built by tests/compressor_model.py with -O2 -ffp-contract=off -fno-fast-math, like oracle/Makefile. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#if defined(__x86_64__)
#include <xmmintrin.h>
#endif

#define RQ 128

/* :14-16 */
float model_db_to_lin(float v) { return powf(10.0f, v / 20.f); }
/* :21-27 */
float model_lin_to_db(float v) { return v == 0.f ? -1000.f : 20.f * log10f(v); }
/* :253-254: quanta in the ring; the output is the quantum that entered ring - 1 quanta ago */
uint32_t model_ring_size(float sample_rate) { return (uint32_t)ceilf(sample_rate * 0.006f / (float)RQ) + 1u; }

#define MODEL(NAME, T, POW, LOG10, EXP, FABS, TMIN)                                                                          \
  static void NAME(const float* in, uint32_t n_ch, uint64_t frames, const float* params, const uint8_t* live,               \
                   float sample_rate_f32, float* out) {                                                                      \
    const uint32_t ring = model_ring_size(sample_rate_f32), d = ring - 1u;                                                   \
    const uint64_t nq = frames / RQ;                                                                                         \
    const T sample_rate = (T)sample_rate_f32;                                                                                \
    T prev = (T)0; /* prev_detector_value, :267 */                                                                           \
    T gains[RQ];                                                                                                             \
    for (uint64_t q = 0; q < nq; q++) {                                                                                      \
      /* :353-389 */                                                                                                         \
      T threshold = (T)params[q * 5 + 0];                                                                                    \
      const T knee = (T)params[q * 5 + 1], ratio = (T)params[q * 5 + 2];                                                     \
      const T attack = (T)params[q * 5 + 3], release = (T)params[q * 5 + 4];                                                 \
      if (knee > (T)0) threshold = threshold + knee / (T)2;                                                                  \
      const T half_knee = knee / (T)2;                                                                                       \
      const T knee_partial = ((T)1 / ratio - (T)1) / ((T)2 * knee);                                                          \
      const T attack_tau = EXP((T)-1 / (attack * sample_rate));                                                              \
      const T release_tau = EXP((T)-1 / (release * sample_rate));                                                            \
      const T full_range_gain = threshold + (-threshold / ratio);                                                            \
      const T full_range_makeup = (T)1 / POW((T)10, full_range_gain / (T)20);                                                \
      const T fm = POW(full_range_makeup, (T)0.6);                                                                           \
      const T makeup_gain = fm == (T)0 ? (T)-1000 : (T)20 * LOG10(fm);                                                       \
      const int in_live = !live || live[q];                                                                                  \
      for (int i = 0; i < RQ; i++) {                                                                                         \
        /* :400-411 (a silent input quantum is one channel of zeros) */                                                      \
        T mx = TMIN;                                                                                                         \
        for (uint32_t c = 0; c < (in_live ? n_ch : 1u); c++) {                                                               \
          const T s = in_live ? FABS((T)in[(uint64_t)c * frames + q * RQ + (uint64_t)i]) : (T)0;                             \
          if (s > mx) mx = s;                                                                                                \
        }                                                                                                                    \
        const T sample_db = mx == (T)0 ? (T)-1000 : (T)20 * LOG10(mx);                                                       \
        /* :417-425 */                                                                                                       \
        T att;                                                                                                               \
        if (sample_db <= threshold - half_knee) {                                                                            \
          att = sample_db;                                                                                                   \
        } else if (sample_db <= threshold + half_knee) {                                                                     \
          const T t = sample_db - threshold + half_knee;                                                                     \
          att = sample_db + (t * t) * knee_partial;                                                                          \
        } else {                                                                                                             \
          att = threshold + (sample_db - threshold) / ratio;                                                                 \
        }                                                                                                                    \
        const T xl = sample_db - att;                                                                                        \
        /* :431-436 */                                                                                                       \
        T det;                                                                                                               \
        if (xl > prev)                                                                                                       \
          det = attack_tau * prev + ((T)1 - attack_tau) * xl;                                                                \
        else                                                                                                                 \
          det = release_tau * prev + ((T)1 - release_tau) * xl;                                                              \
        /* :440-444 */                                                                                                       \
        gains[i] = POW((T)10, (-det + makeup_gain) / (T)20);                                                                 \
        prev = det;                                                                                                          \
      }                                                                                                                      \
      /* :452-475: the delayed quantum times the gains of the CURRENT one */                                                 \
      const int have = q >= d && (!live || live[q - d]);                                                                     \
      for (uint32_t c = 0; c < n_ch; c++) {                                                                                  \
        float* o = out + (uint64_t)c * frames + q * RQ;                                                                      \
        if (!have) {                                                                                                         \
          memset(o, 0, RQ * sizeof(float));                                                                                  \
          continue;                                                                                                          \
        }                                                                                                                    \
        const float* x = in + (uint64_t)c * frames + (q - d) * RQ;                                                           \
        for (int i = 0; i < RQ; i++) o[i] = (float)((T)x[i] * gains[i]);                                                     \
      }                                                                                                                      \
    }                                                                                                                        \
  }

MODEL(model_f32_impl, float, powf, log10f, expf, fabsf, -3.40282347e+38f)
MODEL(model_f64_impl, double, pow, log10, exp, fabs, -1.7976931348623157e+308)

void model_f32(const float* in, uint32_t n_ch, uint64_t frames, const float* params, const uint8_t* live, float sample_rate,
               float* out) {
#if defined(__x86_64__)
  const unsigned int saved = _mm_getcsr();
  _mm_setcsr(saved | 0x8040u); /* no_denormals (thread.rs:374-382): FTZ + DAZ while rendering */
#endif
  model_f32_impl(in, n_ch, frames, params, live, sample_rate, out);
#if defined(__x86_64__)
  _mm_setcsr(saved);
#endif
}

void model_f64(const float* in, uint32_t n_ch, uint64_t frames, const float* params, const uint8_t* live, float sample_rate,
               float* out) {
  model_f64_impl(in, n_ch, frames, params, live, sample_rate, out);
}
