// waa_periodic_wave.hip — PeriodicWave::new's table (periodic_wave.rs:164-189) generated on the device: 8192 entries, each the
// serial f32 sum over the harmonics j = 1 .. n-1 of fl(fl(re_j cos(phase j)) + fl(im_j sin(phase j))), then (unless the wave
// disables it) scaled by 1 / max |entry|.  One table per DISTINCT coefficient set of a batch (one PeriodicWave per context,
// waa_oscillator_set_periodic_wave_instance): 8192 x (n - 1) cos / sin pairs per table, serial on the host, one entry per lane here.
//
// The arithmetic is the reference's step by step: phase = (2 pi i) / 8192 and rad = phase * j rounded to f32 like there, every
// product and sum rounded on its own (no contraction: the pragma below holds whatever the command line says), the harmonics
// added in order, a correctly rounded 1 / max.  The device's sinf / cosf (full range reduction: the arguments reach 2 pi 8191) are
// the only source of difference from the host's table.  The maximum is order-independent, so the result is deterministic.
//
// One workgroup per set, 256 lanes, 32 entries per lane in 8 passes of 4 (four independent sums per lane keep the VALU busy
// between the trig calls; the coefficients are uniform across the workgroup: scalar loads).  A lane writes its raw entries,
// the workgroup's maximum goes through LDS, and every lane scales the entries it wrote itself.  VALU-bound.
#include <hip/hip_runtime.h>

#include "waa_internal.hpp"

#pragma clang fp contract(off)

namespace waa {

namespace {
constexpr int PW_LANES = 256;
constexpr int PW_PER_PASS = 4;
constexpr int PW_PASSES = PERIODIC_WAVE_LEN / (PW_LANES * PW_PER_PASS);
static_assert(PW_PASSES * PW_LANES * PW_PER_PASS == PERIODIC_WAVE_LEN, "the passes cover the table exactly");
}  // namespace

__global__ __launch_bounds__(PW_LANES) void periodic_wave_kernel(const PeriodicWaveDesc d) {
  __shared__ float wave_max[PW_LANES / 64];
  const uint32_t row = blockIdx.x;
  if (row >= d.rows) return;
  const int tid = threadIdx.x;
  const float* re = d.real + (uint64_t)row * d.n;
  const float* im = d.imag + (uint64_t)row * d.n;
  float* out = d.tables + (uint64_t)d.dst_row[row] * PERIODIC_WAVE_LEN;
  const float pi_2 = 2.f * 3.14159265358979323846f;
  float max = 0.f;
#pragma unroll 1
  for (int pass = 0; pass < PW_PASSES; pass++) {
    float phase[PW_PER_PASS], sample[PW_PER_PASS];
#pragma unroll
    for (int k = 0; k < PW_PER_PASS; k++) {
      const int i = (pass * PW_PER_PASS + k) * PW_LANES + tid;
      phase[k] = pi_2 * (float)i / (float)PERIODIC_WAVE_LEN;
      sample[k] = 0.f;
    }
#pragma unroll 1
    for (uint32_t j = 1; j < d.n; j++) {
      const float freq = (float)j, r = re[j], m = im[j];
#pragma unroll
      for (int k = 0; k < PW_PER_PASS; k++) {
        const float rad = phase[k] * freq;
        const float contrib = r * cosf(rad) + m * sinf(rad);
        sample[k] += contrib;
      }
    }
#pragma unroll
    for (int k = 0; k < PW_PER_PASS; k++) {
      out[(pass * PW_PER_PASS + k) * PW_LANES + tid] = sample[k];
      const float a = fabsf(sample[k]);
      max = a > max ? a : max;  // (the host's comparison: a NaN entry is passed over)
    }
  }
  if (!d.normalize[row]) return;  // (uniform across the workgroup)
#pragma unroll
  for (int sft = 32; sft > 0; sft >>= 1) {
    const float o = __shfl_xor(max, sft, 64);
    max = o > max ? o : max;
  }
  if ((tid & 63) == 0) wave_max[tid >> 6] = max;
  __syncthreads();
  max = wave_max[0];
#pragma unroll
  for (int w = 1; w < PW_LANES / 64; w++) max = wave_max[w] > max ? wave_max[w] : max;
  if (!(max > 0.f)) return;
  const float norm_factor = __fdiv_rn(1.f, max);
#pragma unroll 1
  for (int e = 0; e < PW_PASSES * PW_PER_PASS; e++) out[e * PW_LANES + tid] *= norm_factor;  // this lane's own entries
}

void launch_periodic_wave(const PeriodicWaveDesc& d, void* stream) {
  if (!d.rows) return;
  hipLaunchKernelGGL(periodic_wave_kernel, dim3(d.rows), dim3(PW_LANES), 0, (hipStream_t)stream, d);
}

}  // namespace waa
