/* compressor_reduction_model.c — test infrastructure: what DynamicsCompressorNode::reduction() returns after every render
 * quantum (the reference's src/node/dynamics_compressor.rs:304-306), restated in C from the reference's text like
 * tests/compressor_model.c restates the node's output.  The render thread computes `reduction_gain = -detector_value +
 * makeup_gain` for every frame (:440) and stores the LAST one of the quantum (:450); nothing else of the node is needed for it
 * but the level (:397-425) and the detector (:431-436), so the look-ahead ring and the output are left out.
 *
 *   reduction_f32  every operation in f32, in the reference's order, unfused, with the C library's log10f / powf / expf and
 *                  FTZ + DAZ set while it runs (thread.rs:374-382): the reference's arithmetic.
 *   reduction_f64  the same algorithm with every operation in f64: how far f32 arithmetic strays from the mathematics
 *                  (tests/test_compressor_reduction.py computes its tolerance from the two).
 *
 * Same conventions as compressor_model.c:
 *   in        [n_ch][frames] f32, n_ch 1 or 2, frames a multiple of 128
 *   params    [n_quanta][5] f32: threshold, knee, ratio, attack, release as the k-rate AudioParams deliver them
 *   live      [n_quanta] bytes or NULL: 0 = the input quantum is the SILENT quantum (one channel of zeros); NULL = all live
 *   red       [n_quanta]: red[q] = -det + makeup_gain at i = 127 of quantum q (f32 / f64)
 *   makeup    [n_quanta]: the make-up gain of quantum q in dB (:382-389), the scale of the tolerance
 * Built by tests/compressor_reduction_model.py with -O2 -ffp-contract=off -fno-fast-math, like oracle/Makefile. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#if defined(__x86_64__)
#include <xmmintrin.h>
#endif

#define RQ 128

#define REDUCTION(NAME, T, POW, LOG10, EXP, FABS, TMIN)                                                                      \
  static void NAME(const float* in, uint32_t n_ch, uint64_t frames, const float* params, const uint8_t* live,               \
                   float sample_rate_f32, T* red, T* makeup) {                                                               \
    const uint64_t nq = frames / RQ;                                                                                         \
    const T sample_rate = (T)sample_rate_f32;                                                                                \
    T prev = (T)0; /* prev_detector_value, :267 */                                                                           \
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
      T reduction_gain = (T)0; /* :393 */                                                                                    \
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
        /* :440 */                                                                                                           \
        reduction_gain = -det + makeup_gain;                                                                                 \
        prev = det;                                                                                                          \
      }                                                                                                                      \
      red[q] = reduction_gain; /* :450: the store the main thread's reduction() loads */                                     \
      makeup[q] = makeup_gain;                                                                                               \
    }                                                                                                                        \
  }

REDUCTION(reduction_f32_impl, float, powf, log10f, expf, fabsf, -3.40282347e+38f)
REDUCTION(reduction_f64_impl, double, pow, log10, exp, fabs, -1.7976931348623157e+308)

void reduction_f32(const float* in, uint32_t n_ch, uint64_t frames, const float* params, const uint8_t* live, float sample_rate,
                   float* red, float* makeup) {
#if defined(__x86_64__)
  const unsigned int saved = _mm_getcsr();
  _mm_setcsr(saved | 0x8040u); /* no_denormals (thread.rs:374-382): FTZ + DAZ while rendering */
#endif
  reduction_f32_impl(in, n_ch, frames, params, live, sample_rate, red, makeup);
#if defined(__x86_64__)
  _mm_setcsr(saved);
#endif
}

void reduction_f64(const float* in, uint32_t n_ch, uint64_t frames, const float* params, const uint8_t* live, float sample_rate,
                   double* red, double* makeup) {
  reduction_f64_impl(in, n_ch, frames, params, live, sample_rate, red, makeup);
}
