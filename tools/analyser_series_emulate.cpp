// tools/analyser_series_emulate.cpp — host replay of the AnalyserNode series kernels (tests/test_analyser_series.py).
// Compiles web-audio-api-rs_amd/csrc/waa_analyser_series.hip for the HOST behind tools/emulate_shim/hip/hip_runtime.h and runs
// the transform stage, the recursion over the pulls, the bytes kernel and the time-domain gather on a random signal whose
// buffers have exactly the size the library gives them (a sanitizer build sees every access outside them):
//   analyser_series_emulate <fft_size> <first> <hop> <n_quanta> <channels> <tau> <out.bin>
// writes, for 3 instances, P, then the dB rows [3][P][fft/2] (f32), the byte rows (u8), the time rows [3][P][fft] (f32), the byte
// time rows (u8), the bytes-from-dB rows (u8) and the signal [3][channels][n_quanta * 128] (f32).
//   g++ -std=c++17 -O1 -ffp-contract=off -I tools/emulate_shim tools/analyser_series_emulate.cpp -o analyser_series_emulate
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

namespace waa {
namespace {
alignas(16) float lds_raw[2 * 32768 + 7 * 128 * 64];  // the kernels' dynamic LDS (`extern __shared__`)
}
}  // namespace waa
#include "../web-audio-api-rs_amd/csrc/waa_analyser_series.hip"

namespace waa {
void raise_lds_limit(const void*) {}
}  // namespace waa
using namespace waa;

int main(int argc, char** argv) {
  if (argc < 8) return 2;
  const int N = atoi(argv[1]), F = atoi(argv[2]), H = atoi(argv[3]), nq = atoi(argv[4]), nch = atoi(argv[5]), M = N / 2, ni = 3;
  const float tau = (float)atof(argv[6]);
  const int P = F <= nq ? (nq - F) / H + 1 : 0;
  const uint64_t frames = (uint64_t)nq * 128;
  std::mt19937 rng(N + 7 * F + 13 * H);
  std::uniform_real_distribution<float> uni(-1.f, 1.f);
  std::vector<float> sig((size_t)ni * nch * frames);
  for (auto& v : sig) v = uni(rng);
  const float PI_F = 3.14159265358979323846f;
  std::vector<float> win(N);
  std::vector<Cplx> tw(M), twf(M);
  const float alpha = 0.16f, a0 = (1.f - alpha) / 2.f, a1 = 1.f / 2.f, a2 = alpha / 2.f;
  for (int i = 0; i < N; i++) win[i] = a0 - a1 * cosf(2.f * PI_F * (float)i / (float)N) + a2 * cosf(4.f * PI_F * (float)i / (float)N);
  for (int t = 0; t < M; t++) {
    const double x = -2.0 * 3.14159265358979323846 * t / M, y = -2.0 * 3.14159265358979323846 * t / N;
    tw[t] = Cplx{(float)std::cos(x), (float)std::sin(x)};
    twf[t] = Cplx{(float)std::cos(y), (float)std::sin(y)};
  }
  std::vector<float> db((size_t)ni * P * M, 123.f), tim((size_t)ni * P * N, 123.f);
  std::vector<uint8_t> by((size_t)ni * P * M, 9), tby((size_t)ni * P * N, 9), by2((size_t)ni * P * M, 9);
  AnalyserSeriesDesc d{};
  d.a.sig = SignalRef{sig.data(), (uint64_t)nch * frames, frames, nch, 0};
  d.a.n_inst = ni;
  d.a.fft_size = N;
  d.a.smoothing = tau;
  d.a.min_db = -100.f;
  d.a.max_db = -30.f;
  d.a.window = win.data();
  d.a.tw = tw.data();
  d.a.tw_full = twf.data();
  d.first = F;
  d.hop = H;
  d.pulls = P;
  d.frames = frames;
  analyser_series_shape(&d);
  d.db_out = db.data();
  d.byte_out = by.data();
  d.time_out = tim.data();
  d.tbyte_out = tby.data();
  d.lin = tau > 0.f;
  emu_one_thread = true;
  launch_analyser_series_fft(d, nullptr);
  if (emu_lds_bytes > sizeof lds_raw) return 4;
  const size_t want_lds = ((size_t)N + (d.stage_span ? (size_t)N + (size_t)(d.run - 1) * H * 128 : 0)) * sizeof(float);
  if (emu_lds_bytes != want_lds) return 5;
  emu_one_thread = false;
  if (tau > 0.f) launch_analyser_series_smooth(d, nullptr);
  d.byte_out = by2.data();
  launch_analyser_series_bytes(d, nullptr);
  launch_analyser_series_time(d, nullptr);
  FILE* f = fopen(argv[7], "wb");
  if (!f) return 3;
  const int32_t head[3] = {P, d.run, d.stage_span};
  fwrite(head, sizeof head, 1, f);
  fwrite(db.data(), 4, db.size(), f);
  fwrite(by.data(), 1, by.size(), f);
  fwrite(tim.data(), 4, tim.size(), f);
  fwrite(tby.data(), 1, tby.size(), f);
  fwrite(by2.data(), 1, by2.size(), f);
  fwrite(sig.data(), 4, sig.size(), f);
  fclose(f);
  return 0;
}
