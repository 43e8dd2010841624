// waa_analyser_series.hip — a whole series of AnalyserNode pulls in one pass (spectrograms) on gfx950.
//
// The reference program is a fresh analyser pulled at the suspend points q_k = F + k H of an offline render (offline.rs:359-397,
// analysis.rs:278-369): pull k sees the last fft_size frames of the mono down-mix in front of frame q_k * 128 (zeros in front of
// frame 0) and smooths its magnitudes against the spectrum pull k - 1 left.  The engine renders node-major, so when the render
// ends every window of every pull lies in device memory; the number of launches here does not depend on the number of pulls:
//
//   analyser_series_fft_kernel     one workgroup per (instance, run of R consecutive pulls): the run's span of the down-mix
//                                  (fft_size + (R - 1) * 128 H frames, neighbouring windows overlap) is read ONCE into LDS, then
//                                  per pull: Blackman window, packed real transform in LDS (fft_dif, the single pull's), |X| / N.
//                                  smoothing == 0: the rows are independent — dB (and bytes) are written right here, no second
//                                  pass over memory.  smoothing > 0: the unsmoothed magnitudes are written.
//   analyser_series_smooth_kernel  the recursion value = tau * prev + (1 - tau) * norm (unfused f32, then the finite test,
//                                  analysis.rs:337-344) is serial per (instance, bin) only: one thread per (instance, bin) walks
//                                  the pulls in place — loads eight rows ahead, neighbouring lanes neighbouring bins — and turns
//                                  magnitudes into dB (and bytes).
//   analyser_series_bytes_kernel   bytes from finished dB rows (byte data asked for after float data: no second transform).
//   analyser_series_time_kernel    time-domain rows: a gather through the down-mix, float and / or byte form; no transform.
#include <hip/hip_runtime.h>

#include "waa_analyser_common.hpp"
#include "waa_internal.hpp"

namespace waa {

namespace {

constexpr int SERIES_MAX_RUN = 8;
constexpr size_t SERIES_STAGE_LDS = 48 * 1024;  // a staged run keeps three workgroups per CU (160 KB of LDS)

__global__ __launch_bounds__(1024) void analyser_series_fft_kernel(const AnalyserSeriesDesc d) {
  extern __shared__ __attribute__((aligned(16))) float lds_raw[];
  Cplx* a = reinterpret_cast<Cplx*>(lds_raw);
  const int tid = threadIdx.x, nt = blockDim.x;
  const int N = d.a.fft_size, M = N >> 1, P = d.pulls;
  float* span = lds_raw + N;
  const uint32_t n_runs = (uint32_t)((P + d.run - 1) / d.run);
  const uint32_t inst = blockIdx.x / n_runs;
  const int k0 = (int)(blockIdx.x % n_runs) * d.run;
  const int k1 = k0 + d.run < P ? k0 + d.run : P;
  const int64_t hopf = (int64_t)d.hop * RQ;
  const int64_t f0 = ((int64_t)d.first + (int64_t)k0 * d.hop) * RQ - N;  // first frame of pull k0's window (negative: zeros)
  if (d.stage_span) {
    const int len = N + (k1 - k0 - 1) * (int)hopf;
    for (int i = tid; i < len; i += nt) {
      const int64_t f = f0 + i;
      span[i] = (f >= 0 && (uint64_t)f < d.frames) ? analyser_mono(d.a.sig, d.a.code, d.a.code_stride, inst, f) : 0.f;
    }
    __syncthreads();
  }
  const int lg = 31 - __builtin_clz(M);
  const float nf = 1.f / (float)N;
  const float tau = d.a.smoothing;
  const float bscale = 255.f / (d.a.max_db - d.a.min_db);
  for (int k = k0; k < k1; k++) {
    const int off = (k - k0) * (int)hopf;
    for (int i = tid; i < N; i += nt) {
      float v;
      if (d.stage_span) {
        v = span[off + i];
      } else {
        const int64_t f = f0 + off + i;
        v = (f >= 0 && (uint64_t)f < d.frames) ? analyser_mono(d.a.sig, d.a.code, d.a.code_stride, inst, f) : 0.f;
      }
      reinterpret_cast<float*>(a)[i] = v * d.a.window[i];  // z[n] = x[2n] + i x[2n+1]
    }
    __syncthreads();
    fft_dif(a, d.a.tw, M, tid, nt);
    const uint64_t row = ((uint64_t)inst * P + k) * M;
    for (int kk = tid; kk < M; kk += nt) {
      const float norm = analyser_bin_norm(a, d.a.tw_full, kk, M, lg, nf);
      if (d.lin) {
        d.db_out[row + kk] = norm;
      } else {
        // smoothing == 0: the reference's arithmetic against a finite previous value, whose product with 0 is 0
        float value = tau * 0.f + (1.f - tau) * norm;
        value = isfinite(value) ? value : 0.f;
        const float db = 20.f * log10f(value);  // analysis.rs:365-368
        if (d.db_out) d.db_out[row + kk] = db;
        if (d.byte_out) d.byte_out[row + kk] = analyser_byte(db, d.a.min_db, bscale);
      }
    }
    __syncthreads();  // (the next pull's window overwrites the transform)
  }
}

__global__ __launch_bounds__(256) void analyser_series_smooth_kernel(const AnalyserSeriesDesc d) {
  const int M = d.a.fft_size >> 1, P = d.pulls;
  const uint32_t nb = (uint32_t)((M + (int)blockDim.x - 1) / (int)blockDim.x);
  const uint32_t inst = blockIdx.x / nb;
  const int bin = (int)(blockIdx.x % nb) * (int)blockDim.x + (int)threadIdx.x;
  if (bin >= M) return;
  const uint64_t base = (uint64_t)inst * P * M + bin;
  float* p = d.db_out + base;
  uint8_t* pb = d.byte_out ? d.byte_out + base : nullptr;
  const float tau = d.a.smoothing, one_minus = 1.f - tau;
  const float bscale = 255.f / (d.a.max_db - d.a.min_db);
  float prev = 0.f;  // a fresh analyser's last_fft_output
  constexpr int AHEAD = 8;
  for (int k = 0; k < P; k += AHEAD) {
    float x[AHEAD];
#pragma unroll
    for (int j = 0; j < AHEAD; j++) x[j] = p[(uint64_t)(k + j < P ? k + j : P - 1) * M];
#pragma unroll
    for (int j = 0; j < AHEAD; j++) {
      if (k + j < P) {
        float value = tau * prev + one_minus * x[j];  // analysis.rs:342, unfused
        value = isfinite(value) ? value : 0.f;
        prev = value;
        const float db = 20.f * log10f(value);
        p[(uint64_t)(k + j) * M] = db;
        if (pb) pb[(uint64_t)(k + j) * M] = analyser_byte(db, d.a.min_db, bscale);
      }
    }
  }
}

__global__ __launch_bounds__(256) void analyser_series_bytes_kernel(const AnalyserSeriesDesc d) {
  const uint64_t total = (uint64_t)d.a.n_inst * d.pulls * (uint64_t)(d.a.fft_size >> 1);
  const float bscale = 255.f / (d.a.max_db - d.a.min_db);
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x)
    d.byte_out[i] = analyser_byte(d.db_out[i], d.a.min_db, bscale);
}

__global__ __launch_bounds__(256) void analyser_series_time_kernel(const AnalyserSeriesDesc d) {
  const int N = d.a.fft_size, P = d.pulls;
  const uint32_t inst = blockIdx.x / (uint32_t)P;
  const int k = (int)(blockIdx.x % (uint32_t)P);
  const int64_t f0 = ((int64_t)d.first + (int64_t)k * d.hop) * RQ - N;
  const uint64_t row = (uint64_t)blockIdx.x * N;
  for (int i = threadIdx.x; i < N; i += blockDim.x) {
    const int64_t f = f0 + i;
    const float v = (f >= 0 && (uint64_t)f < d.frames) ? analyser_mono(d.a.sig, d.a.code, d.a.code_stride, inst, f) : 0.f;
    if (d.time_out) d.time_out[row + i] = v;
    if (d.tbyte_out) {  // analysis.rs:271-275
      const float scaled = 128.f * (1.f + v);
      const float clamped = scaled < 0.f ? 0.f : scaled > 255.f ? 255.f : scaled;
      d.tbyte_out[row + i] = (uint8_t)clamped;
    }
  }
}

}  // namespace

// Run length of the transform stage.  A run of R pulls reads fft_size + (R - 1) * 128 H frames instead of R * fft_size; the span
// and the transform together stay within 48 KB of LDS (three workgroups per CU), and there are at least two pulls per run or none
// is staged: one pull per workgroup reads its window straight into the transform's buffer, as the single pull does.
void analyser_series_shape(AnalyserSeriesDesc* d) {
  const size_t N = (size_t)d->a.fft_size, hopf = (size_t)d->hop * RQ;
  int run = d->pulls < SERIES_MAX_RUN ? d->pulls : SERIES_MAX_RUN;
  while (run > 1 && (2 * N + (size_t)(run - 1) * hopf) * sizeof(float) > SERIES_STAGE_LDS) run--;
  if (hopf >= N) run = 1;  // (windows that do not overlap: nothing to share)
  d->run = run;
  d->stage_span = run > 1 ? 1 : 0;
}

void launch_analyser_series_fft(const AnalyserSeriesDesc& d, void* stream) {
  const int N = d.a.fft_size, M = N / 2;
  int nt = M / 4;  // one radix-4 butterfly per thread and stage
  if (nt < 64) nt = 64;
  if (nt > 1024) nt = 1024;
  size_t lds = (size_t)N * sizeof(float);
  if (d.stage_span) lds += ((size_t)N + (size_t)(d.run - 1) * d.hop * RQ) * sizeof(float);
  if (lds > 64 * 1024) raise_lds_limit(reinterpret_cast<const void*>(analyser_series_fft_kernel));
  const uint32_t n_runs = (uint32_t)((d.pulls + d.run - 1) / d.run);
  hipLaunchKernelGGL(analyser_series_fft_kernel, dim3(d.a.n_inst * n_runs), dim3(nt), lds, (hipStream_t)stream, d);
}
void launch_analyser_series_smooth(const AnalyserSeriesDesc& d, void* stream) {
  const int M = d.a.fft_size / 2;
  const int nt = M < 256 ? (M < 64 ? 64 : M) : 256;
  const uint32_t nb = (uint32_t)((M + nt - 1) / nt);
  hipLaunchKernelGGL(analyser_series_smooth_kernel, dim3(d.a.n_inst * nb), dim3(nt), 0, (hipStream_t)stream, d);
}
void launch_analyser_series_bytes(const AnalyserSeriesDesc& d, void* stream) {
  const uint64_t total = (uint64_t)d.a.n_inst * d.pulls * (uint64_t)(d.a.fft_size / 2);
  uint64_t blocks = (total + 255) / 256;
  if (blocks > 256 * 64) blocks = 256 * 64;
  hipLaunchKernelGGL(analyser_series_bytes_kernel, dim3((uint32_t)blocks), dim3(256), 0, (hipStream_t)stream, d);
}
void launch_analyser_series_time(const AnalyserSeriesDesc& d, void* stream) {
  const int nt = d.a.fft_size < 256 ? 64 : 256;
  hipLaunchKernelGGL(analyser_series_time_kernel, dim3(d.a.n_inst * (uint32_t)d.pulls), dim3(nt), 0, (hipStream_t)stream, d);
}

}  // namespace waa
