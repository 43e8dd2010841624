// waa_analyser_host.cpp — AnalyserNode pulls in the C ABI (include/waa_hip.h, analysis.rs:261-401).  current_time after an
// offline render never changes, so the spectra of ALL instances are computed once per render — one launch, one workgroup per
// context — and every pull, per instance or for the whole batch, is a view into that result (repeated pulls return the same
// data, analysis.rs:354-357).
#include "waa_host.hpp"

using namespace waa;
using namespace waa::host;

// a launch made at pull time: it gets its profile slot when it is first made on a profiled batch
template <typename L>
static int pull_launch(waa_batch* b, const char* name, L&& launch) {
  return timed(b, b->profiling ? slot_for(b, name) : -1, launch);
}

extern "C" {

enum { AN_DB = 0, AN_BYTES = 1, AN_TIME = 2, AN_TBYTES = 3 };
// the Blackman window and the twiddles of the packed real transform, uploaded on first use
static int analyser_tables(waa_batch* b, Node& n) {
  if (n.d_window) return 0;
  const int N = n.desc.i[0], M = N / 2;
  int e;
  // generate_blackman (analysis.rs:14-24), f32 with the host libm the reference's f32::cos resolves to
  std::vector<float> win(N);
  const float alpha = 0.16f, a0 = (1.f - alpha) / 2.f, a1 = 1.f / 2.f, a2 = alpha / 2.f;
  for (int i = 0; i < N; i++)
    win[i] = a0 - a1 * cosf(2.f * PI_F * (float)i / (float)N) + a2 * cosf(4.f * PI_F * (float)i / (float)N);
  std::vector<Cplx> tw(M), twf(M);
  for (int t = 0; t < M; t++) {
    const double x = -2.0 * 3.14159265358979323846 * (double)t / (double)M;
    const double y = -2.0 * 3.14159265358979323846 * (double)t / (double)N;
    tw[t] = Cplx{(float)std::cos(x), (float)std::sin(x)};
    twf[t] = Cplx{(float)std::cos(y), (float)std::sin(y)};
  }
  if ((e = dev_upload(b, &n.d_window, win)) || (e = dev_upload(b, &n.d_an_tw, tw)) || (e = dev_upload(b, &n.d_an_twfull, twf))) return e;
  return 0;
}
// what a single pull and a series have in common
static AnalyserDesc analyser_desc_of(const waa_batch* b, const Node& n) {
  AnalyserDesc ad{};
  ad.sig = n.sig;
  ad.n_inst = b->n_inst;
  ad.fft_size = n.desc.i[0];
  ad.smoothing = (float)n.desc.d[0];
  ad.min_db = (float)n.desc.d[1];
  ad.max_db = (float)n.desc.d[2];
  ad.window = n.d_window;
  ad.tw = n.d_an_tw;
  ad.tw_full = n.d_an_twfull;
  ad.code = b->dynamic ? n.code : nullptr;
  ad.code_stride = b->code_stride;
  return ad;
}
static int analyser_compute(waa_batch* b, uint32_t node, int what) {
  int e;
  if ((e = check_node(b, node, WAA_NODE_ANALYSER))) return e;
  Node& n = b->nodes[node];
  const int N = n.desc.i[0], M = N / 2;
  const size_t ni = b->n_inst;
  const bool on_device = b->planned && b->rendered && n.live && !b->dry;
  if (on_device)
    if (int es = settle_loops(b)) return es;  // (run_steps resets the analysers' caches: the pull below sees the settled render)
  if (!on_device) {
    // nothing rendered (or the node does not reach the destination): an all-zero ring buffer
    if (!n.an.have_db) {
      n.an.db.assign(ni * M, -INFINITY);   // 20 log10(0)
      n.an.bytes.assign(ni * M, 0);        // (-inf - min) scaled and clamped
      n.an.time.assign(ni * N, 0.f);
      n.an.have_db = n.an.have_bytes = n.an.have_time = true;
    }
    return 0;
  }
  HIP_TRY(hipSetDevice(b->device));
  if (!n.an.computed) {
    if ((e = analyser_tables(b, n))) return e;
    if (!n.d_an_db) {
      std::vector<float> zeros(M, 0.f);
      if ((e = dev_upload(b, &n.d_an_prev, zeros)) || (e = dev_alloc(b, &n.d_an_db, ni * M)) || (e = dev_alloc(b, &n.d_an_bytes, ni * M)) ||
          (e = dev_alloc(b, &n.d_an_time, ni * N)))
        return e;
    }
    AnalyserDesc ad = analyser_desc_of(b, n);
    ad.frames_written = (uint64_t)b->n_quanta * RQ;
    ad.prev = n.d_an_prev;
    ad.db_out = n.d_an_db;
    ad.byte_out = n.d_an_bytes;
    ad.time_out = n.d_an_time;
    if ((e = pull_launch(b, "analyser_kernel", [&] { launch_analyser(ad, b->stream); }))) return e;
    n.an.computed = true;
  }
  // one transfer per kind of result, on first use (asynchronous on the batch's stream, then waited for)
  if (what == AN_DB && !n.an.have_db) {
    n.an.db.resize(ni * M);
    HIP_TRY(hipMemcpyAsync(n.an.db.data(), n.d_an_db, ni * M * sizeof(float), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    n.an.have_db = true;
  } else if (what == AN_BYTES && !n.an.have_bytes) {
    n.an.bytes.resize(ni * M);
    HIP_TRY(hipMemcpyAsync(n.an.bytes.data(), n.d_an_bytes, ni * M, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    n.an.have_bytes = true;
  } else if (what == AN_TIME && !n.an.have_time) {
    n.an.time.resize(ni * N);
    HIP_TRY(hipMemcpyAsync(n.an.time.data(), n.d_an_time, ni * N * sizeof(float), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    n.an.have_time = true;
  }
  return 0;
}

// A series node (desc.i[1] > 0, include/waa_hip.h): the rows of ALL pulls of ALL instances, computed once per render and per kind
// on the device (waa_analyser_series.hip) and kept there; a getter call copies its rows [i0, i1) x [P] out, `nn` elements apart.
static int analyser_series_rows(waa_batch* b, uint32_t node, int what, uint32_t i0, uint32_t i1, void* dst, uint32_t nn) {
  Node& n = b->nodes[node];
  const uint32_t N = (uint32_t)n.desc.i[0], M = N / 2, P = n.an_series_pulls(b->n_quanta);
  const size_t ni = b->n_inst;
  const bool freq = what == AN_DB || what == AN_BYTES, bytes = what == AN_BYTES || what == AN_TBYTES;
  const uint32_t W = freq ? M : N, len = std::min(nn, W);
  const size_t es = bytes ? 1 : sizeof(float), rows = (size_t)(i1 - i0) * P;
  const bool on_device = b->planned && b->rendered && n.live && !b->dry;
  if (on_device)
    if (int es2 = settle_loops(b)) return es2;  // (run_steps resets the analysers' caches: the pulls below see the settled render)
  if (what == AN_TBYTES && nn > len)  // analysis.rs:268-276: elements past fft_size come from a zeroed tmp
    for (size_t r = 0; r < rows; r++) std::memset((uint8_t*)dst + r * nn + len, 128, nn - len);
  if (!on_device) {
    // nothing rendered (or the node does not reach the destination): every pull sees an all-zero ring buffer
    for (size_t r = 0; r < rows; r++) {
      if (what == AN_DB)
        std::fill_n((float*)dst + r * nn, len, -INFINITY);  // 20 log10(0)
      else if (what == AN_BYTES)
        std::memset((uint8_t*)dst + r * nn, 0, len);         // (-inf - min) scaled and clamped
      else if (what == AN_TIME)
        std::fill_n((float*)dst + r * nn, len, 0.f);
      else
        std::memset((uint8_t*)dst + r * nn, 128, len);
    }
    return WAA_OK;
  }
  HIP_TRY(hipSetDevice(b->device));
  int e;
  if ((e = analyser_tables(b, n))) return e;
  AnalyserSeriesDesc sd{};
  sd.a = analyser_desc_of(b, n);
  sd.hop = n.desc.i[1];
  sd.first = n.desc.i[2];
  sd.pulls = (int32_t)P;
  sd.frames = (uint64_t)b->n_quanta * RQ;
  analyser_series_shape(&sd);
  const size_t nf = ni * P * M, nt = ni * P * N;
  const void* src = nullptr;
  if (freq) {
    const bool smooth = sd.a.smoothing > 0.f;
    if (what == AN_BYTES && !n.d_ans_bytes && (e = dev_alloc(b, &n.d_ans_bytes, nf))) return e;
    // dB rows: asked for, the recursion's workspace (the unsmoothed magnitudes in f32), or there from an earlier render and not
    // current — the pass that is about to run fills them too, so that float rows asked for later do not transform again
    const bool need_db = what == AN_DB || (smooth && !n.an.s_bytes) || (n.d_ans_db && !n.an.s_db);
    if (need_db && !n.d_ans_db && (e = dev_alloc(b, &n.d_ans_db, nf))) return e;
    sd.db_out = n.d_ans_db;
    sd.byte_out = n.d_ans_bytes;
    if (what == AN_BYTES && !n.an.s_bytes && n.an.s_db) {
      if ((e = pull_launch(b, "analyser_series_bytes_kernel", [&] { launch_analyser_series_bytes(sd, b->stream); }))) return e;
      n.an.s_bytes = true;
    } else if (!(what == AN_DB ? n.an.s_db : n.an.s_bytes)) {
      // one transform pass for every frequency kind that has a buffer by now and is not current
      if (!need_db) sd.db_out = nullptr;
      if (n.an.s_bytes) sd.byte_out = nullptr;
      sd.lin = smooth ? 1 : 0;
      if ((e = pull_launch(b, "analyser_series_fft_kernel", [&] { launch_analyser_series_fft(sd, b->stream); }))) return e;
      if (smooth && (e = pull_launch(b, "analyser_series_smooth_kernel", [&] { launch_analyser_series_smooth(sd, b->stream); }))) return e;
      n.an.s_db |= sd.db_out != nullptr;
      n.an.s_bytes |= sd.byte_out != nullptr;
    }
    src = what == AN_DB ? (const void*)n.d_ans_db : (const void*)n.d_ans_bytes;
  } else {
    if (what == AN_TIME && !n.d_ans_time && (e = dev_alloc(b, &n.d_ans_time, nt))) return e;
    if (what == AN_TBYTES && !n.d_ans_tbytes && (e = dev_alloc(b, &n.d_ans_tbytes, nt))) return e;
    if (!(what == AN_TIME ? n.an.s_time : n.an.s_tbytes)) {
      // (both forms in one gather when both have a buffer and neither is current)
      sd.time_out = n.an.s_time ? nullptr : n.d_ans_time;
      sd.tbyte_out = n.an.s_tbytes ? nullptr : n.d_ans_tbytes;
      if ((e = pull_launch(b, "analyser_series_time_kernel", [&] { launch_analyser_series_time(sd, b->stream); }))) return e;
      n.an.s_time |= sd.time_out != nullptr;
      n.an.s_tbytes |= sd.tbyte_out != nullptr;
    }
    src = what == AN_TIME ? (const void*)n.d_ans_time : (const void*)n.d_ans_tbytes;
  }
  // ring_buffer.read hands out the most recent `len` frames (analysis.rs:114-127); frequency rows start at bin 0
  const char* from = (const char*)src + ((size_t)i0 * P * W + (freq ? 0 : W - len)) * es;
  // (pageable caller memory goes through the batch's pinned staging block: the device only touches memory this library pinned)
  if ((e = xfer_d2h(b, dst, (size_t)nn * es, from, (size_t)W * es, (size_t)len * es, rows))) return e;
  HIP_TRY(hipStreamSynchronize(b->stream));
  return WAA_OK;
}
// rows [i0, i1) of one result kind -> dst rows of `nn` elements
static int analyser_rows(waa_batch* b, uint32_t node, int what, uint32_t i0, uint32_t i1, void* dst, uint32_t nn) {
  int e = check_node(b, node, WAA_NODE_ANALYSER);
  if (e) return e;
  if (b->nodes[node].an_series()) return analyser_series_rows(b, node, what, i0, i1, dst, nn);
  if ((e = analyser_compute(b, node, what))) return e;
  const Node& n = b->nodes[node];
  const uint32_t N = (uint32_t)n.desc.i[0], M = N / 2;
  for (uint32_t i = i0; i < i1; i++) {
    const size_t row = (size_t)(i - i0) * nn;
    if (what == AN_DB) {
      std::memcpy((float*)dst + row, &n.an.db[(size_t)i * M], std::min(nn, M) * sizeof(float));
    } else if (what == AN_BYTES) {
      std::memcpy((uint8_t*)dst + row, &n.an.bytes[(size_t)i * M], std::min(nn, M));
    } else {
      // ring_buffer.read: the most recent `len` frames (analysis.rs:114-127)
      const uint32_t len = std::min(nn, N);
      std::memcpy((float*)dst + row, &n.an.time[(size_t)i * N + (N - len)], len * sizeof(float));
    }
  }
  return WAA_OK;
}
static int analyser_byte_time_rows(waa_batch* b, uint32_t node, uint32_t i0, uint32_t i1, uint8_t* dst, uint32_t nn) {
  int e = check_node(b, node, WAA_NODE_ANALYSER);
  if (e) return e;
  if (b->nodes[node].an_series()) return analyser_series_rows(b, node, AN_TBYTES, i0, i1, dst, nn);
  if ((e = analyser_compute(b, node, AN_TIME))) return e;
  const Node& n = b->nodes[node];
  const uint32_t N = (uint32_t)n.desc.i[0];
  const uint32_t len = std::min(nn, N);
  for (uint32_t i = i0; i < i1; i++) {
    const float* t = &n.an.time[(size_t)i * N + (N - len)];
    uint8_t* o = dst + (size_t)(i - i0) * nn;
    for (uint32_t k = 0; k < nn; k++) {  // analysis.rs:268-276 (elements past fft_size read a zeroed tmp)
      const float v = k < len ? t[k] : 0.f;
      const float scaled = 128.f * (1.f + v);
      const float clamped = scaled < 0.f ? 0.f : scaled > 255.f ? 255.f : scaled;
      o[k] = (uint8_t)clamped;
    }
  }
  return WAA_OK;
}
static int an_inst(waa_batch* b, uint32_t inst) {
  if (!b) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch");
  if (inst >= b->n_inst) return fail(WAA_ERR_INVALID_ARGUMENT, "instance out of range");
  return 0;
}

waa_status waa_analyser_get_float_frequency_data(waa_batch* b, uint32_t node, uint32_t inst, float* dst, uint32_t nn) {
  if (int e = an_inst(b, inst)) return e;
  return analyser_rows(b, node, AN_DB, inst, inst + 1, dst, nn);
}
waa_status waa_analyser_get_byte_frequency_data(waa_batch* b, uint32_t node, uint32_t inst, uint8_t* dst, uint32_t nn) {
  if (int e = an_inst(b, inst)) return e;
  return analyser_rows(b, node, AN_BYTES, inst, inst + 1, dst, nn);
}
waa_status waa_analyser_get_float_time_domain_data(waa_batch* b, uint32_t node, uint32_t inst, float* dst, uint32_t nn) {
  if (int e = an_inst(b, inst)) return e;
  return analyser_rows(b, node, AN_TIME, inst, inst + 1, dst, nn);
}
waa_status waa_analyser_get_byte_time_domain_data(waa_batch* b, uint32_t node, uint32_t inst, uint8_t* dst, uint32_t nn) {
  if (int e = an_inst(b, inst)) return e;
  return analyser_byte_time_rows(b, node, inst, inst + 1, dst, nn);
}
waa_status waa_analyser_get_float_frequency_data_batch(waa_batch* b, uint32_t node, float* dst, uint32_t nn) {
  if (!b) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch");
  return analyser_rows(b, node, AN_DB, 0, b->n_inst, dst, nn);
}
waa_status waa_analyser_get_byte_frequency_data_batch(waa_batch* b, uint32_t node, uint8_t* dst, uint32_t nn) {
  if (!b) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch");
  return analyser_rows(b, node, AN_BYTES, 0, b->n_inst, dst, nn);
}
waa_status waa_analyser_get_float_time_domain_data_batch(waa_batch* b, uint32_t node, float* dst, uint32_t nn) {
  if (!b) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch");
  return analyser_rows(b, node, AN_TIME, 0, b->n_inst, dst, nn);
}
waa_status waa_analyser_get_byte_time_domain_data_batch(waa_batch* b, uint32_t node, uint8_t* dst, uint32_t nn) {
  if (!b) return fail(WAA_ERR_INVALID_ARGUMENT, "null batch");
  return analyser_byte_time_rows(b, node, 0, b->n_inst, dst, nn);
}

}  // extern "C"
