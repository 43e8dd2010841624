/* Sanitizer harness for the host resampler (test infrastructure): AudioBuffer::resample (buffer.rs:311-363) as the oracle
 * restates it, over the decode table of tests/test_caller_boundary.py — source lengths 1, 2, 3, 5, source lengths whose target
 * is 1, 2, 255, 256, 257, 511, 512, 513 and about 70 000, the rate pairs 44100 <-> 48000 and 3000 <-> 768000, the f32 edge of
 * the no-resample rule, and 2 frames at 96 kHz in an 8 kHz context (target length 1: position = 0 / 0, the playhead is NaN; the
 * reference's `as usize` makes that index 0 and emits one NaN sample).  The destination is malloc'ed at exactly the returned
 * length, so a sample written behind it is an ASan report; a NaN cast to an integer is a float-cast-overflow report:
 *   gcc -O1 -g -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all -Iinclude \
 *       tools/resample_harness.c oracle/waa_oracle.c -lm -lpthread -o resample_harness && ./resample_harness
 * Prints one line per case and exits 0 when every case kept its length, its first and last sample and the NaN rule.
 * (tests/test_caller_boundary.py compares the same cases bit for bit with a numpy model of the reference.) */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

uint64_t orc_buffer_resample(const float* src, uint64_t frames, float source_sr, float target_sr, float* dst, uint64_t cap);

static int failures = 0;

static uint64_t target_of(uint64_t frames, float src_sr, float ctx_sr) {
  if (fabsf(src_sr - ctx_sr) <= 0.1f || frames == 0) return frames;
  return (uint64_t)ceil((double)frames * ((double)ctx_sr / (double)src_sr));
}

/* the shortest source whose target length is `target` (0: none) */
static uint64_t frames_for_target(uint64_t target, float src_sr, float ctx_sr) {
  const double inv = (double)src_sr / (double)ctx_sr;
  uint64_t guess = (uint64_t)((double)target * inv);
  for (uint64_t f = guess > 300 ? guess - 300 : 1; f <= guess + 300; f++)
    if (target_of(f, src_sr, ctx_sr) == target) return f;
  return 0;
}

static void run_case(uint64_t frames, float src_sr, float ctx_sr) {
  float* src = (float*)malloc(sizeof(float) * (frames ? frames : 1));
  for (uint64_t i = 0; i < frames; i++) src[i] = (float)(int16_t)(i * 2654435761u >> 7) / 32768.f;
  if (frames) src[0] = -1.f, src[frames - 1] = 32767.f / 32768.f;
  const uint64_t want = target_of(frames, src_sr, ctx_sr);
  const uint64_t n = orc_buffer_resample(src, frames, src_sr, ctx_sr, NULL, 0);
  float* dst = (float*)malloc(sizeof(float) * (n ? n : 1));
  const uint64_t m = orc_buffer_resample(src, frames, src_sr, ctx_sr, dst, n);
  int ok = n == want && m == n;
  if (ok && n == 1 && fabsf(src_sr - ctx_sr) > 0.1f)
    ok = dst[0] != dst[0]; /* resampled to one frame: position = 0 / 0 */
  else if (ok && n)
    ok = dst[0] == src[0] && dst[n - 1] == src[frames - 1];
  for (uint64_t i = 0; ok && n > 1 && i < n; i++) ok = fabsf(dst[i]) <= 1.f;
  printf("%-4s frames %8llu  %12.4f -> %12.4f  target %8llu (expected %llu)\n", ok ? "ok" : "FAIL", (unsigned long long)frames,
         (double)src_sr, (double)ctx_sr, (unsigned long long)n, (unsigned long long)want);
  fflush(stdout);
  failures += !ok;
  free(dst);
  free(src);
}

int main(void) {
  static const float pairs[4][2] = {{44100.f, 48000.f}, {48000.f, 44100.f}, {3000.f, 768000.f}, {768000.f, 3000.f}};
  static const uint64_t lengths[] = {1, 2, 3, 5};
  static const uint64_t targets[] = {1, 2, 255, 256, 257, 511, 512, 513, 70001};
  for (int p = 0; p < 4; p++) {
    for (unsigned k = 0; k < sizeof lengths / sizeof *lengths; k++) run_case(lengths[k], pairs[p][0], pairs[p][1]);
    for (unsigned k = 0; k < sizeof targets / sizeof *targets; k++) {
      const uint64_t f = frames_for_target(targets[k], pairs[p][0], pairs[p][1]);
      if (f) run_case(f, pairs[p][0], pairs[p][1]); /* (an upsampling ratio skips some target lengths) */
    }
  }
  run_case(2, 96000.f, 8000.f); /* target length 1 */
  run_case(0, 44100.f, 48000.f);
  /* one f32 ulp at 44100 is 0.00390625: 25 ulps are inside the 0.1 window, 26 outside */
  run_case(513, 44100.f, 44100.09765625f);
  run_case(513, 44100.f, 44100.1015625f);
  run_case(513, 44100.09765625f, 44100.f);
  run_case(513, 44100.1015625f, 44100.f);
  printf("%d failure(s)\n", failures);
  return failures != 0;
}
