// waa_loop.hip — feedback loops.  A cycle through a DelayNode (graph.rs:323-487: the delay's writer half is the
// cycle breaker) makes quantum q of every member depend on quantum q-1 of the loop, so the node-major engine
// cannot render it one node at a time.  The members of the loop are instead rendered quantum by quantum, in the
// reference's processing order, by one wavefront per instance (instances are independent, so no cross-wave
// synchronisation exists): lane l renders frames l and l + 64 of the 128-frame quantum for up to two channels.
//   * outputs of members rendered earlier in the same quantum are handed over through LDS,
//   * every member also writes its output signal to HBM (consumers outside the loop, delay lines),
//   * a delay line is the writer's mixed input in absolute time; the reader gathers from it exactly like
//     waa_delay.hip, with the in-cycle clamp of delay.rs:693-701; it reads through agent-scope loads because the
//     same wave wrote those lines moments ago,
//   * a BiquadFilter inside a loop renders its 128 frames over the whole wavefront (zero-state + scan + exact-order pass,
//     as in waa_dyn.hip); per-frame coefficient sets and quanta with inf / NaN: serially on one lane per channel.
// Latency-bound by construction (about 1-2 us per quantum and member); throughput comes from the batch.
//
// The static-count special case of dyn_kernel (waa_dyn.hip); what the two share — param / coherent loads, the curve lookup, the
// Biquad quantum scan (biquad_scan_pass) and its serial form (biquad_serial_frames), the DelayReader's position arithmetic
// (delay_position, delay_prev_next), lds_sync — is waa_quantum.hpp.  Here: loop_lds_layout (the dynamic LDS, for the kernel and
// for launch_loop), loop_gather, loop_node (loop_biquad), loop_delay_reader, loop_publish, and loop_kernel's walk over them.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "waa_internal.hpp"
#include "waa_quantum.hpp"

namespace waa {

namespace {
// quantum.rs:285-505 for the layouts a loop may carry (mono / stereo)
__device__ __forceinline__ void mix12(float (&u)[2][2], int from, int to, int interp) {
  if (from == to) return;
  if (from == 1 && to == 2) {
#pragma unroll
    for (int e = 0; e < 2; e++) u[1][e] = interp == 1 ? 0.f : u[0][e];
  } else if (from == 2 && to == 1) {
    if (interp != 1) {
#pragma unroll
      for (int e = 0; e < 2; e++) u[0][e] = 0.5f * (u[0][e] + u[1][e]);
    }
  }
}
}  // namespace

// ---- the dynamic LDS of loop_kernel: byte offsets from its start, for the kernel's pointers and for launch_loop's size
struct LoopLds {
  size_t cur;       // float [n_items][2][128] outputs of this quantum
  size_t scratch;   // float [2][128]
  size_t bq_state;  // double [n_items][2][4]
  size_t items;     // LoopItem [n_items]
  size_t total;
};
__host__ __device__ constexpr LoopLds loop_lds_layout(int n_items) {
  const size_t n = (size_t)n_items;
  LoopLds l{};
  size_t o = 0;
  l.cur = o, o += n * 2 * RQ * sizeof(float);
  l.scratch = o, o += 2 * RQ * sizeof(float);
  l.bq_state = o, o += n * 8 * sizeof(double);  // (8-byte aligned: whole quanta of floats in front)
  l.items = o, o += n * sizeof(LoopItem);
  l.total = o;
  return l;
}
// (the totals of the closed formula this replaced)
static_assert(loop_lds_layout(1).total == 2520 && loop_lds_layout(4).total == 7008 && loop_lds_layout(7).total == 11496 &&
                  loop_lds_layout(LOOP_MAX_ITEMS).total == 36928,
              "loop_kernel's LDS total moved");
static_assert(loop_lds_layout(7).bq_state % 8 == 0 && loop_lds_layout(7).items % 8 == 0, "doubles and descriptors on 8-byte boundaries");

struct LoopCtx {
  float *cur, *scratch;  // LDS (LoopLds)
  double* bq_state;
  LoopItem* items_s;
  uint32_t inst;
  int lane;
  // the quantum and the item at hand (the item itself travels as a reference parameter: held as a pointer in here the kernel
  // takes 86 vector registers instead of 66)
  uint32_t q;
  uint64_t f0;
  int it;
};

// ---- inputs: every incoming edge mixed to the computed channel count, summed in edge order
__device__ __forceinline__ void loop_gather(const LoopCtx& cx, const LoopItem& li, float (&v)[2][2]) {
  const int lane = cx.lane;
  for (int k = 0; k < li.n_in; k++) {
    float u[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
    const int nc = li.in_nch[k];
    if (li.in_item[k] >= 0) {
      const float* src = cx.cur + (size_t)li.in_item[k] * 2 * RQ;
#pragma unroll
      for (int c = 0; c < 2; c++)
        if (c < nc) {
          u[c][0] = src[c * RQ + lane];
          u[c][1] = src[c * RQ + 64 + lane];
        }
    } else {
      const SignalRef& sg = li.in_sig[k];
      const float* src = sg.base + (uint64_t)cx.inst * sg.inst_stride + cx.f0;
#pragma unroll
      for (int c = 0; c < 2; c++)
        if (c < nc) {
          u[c][0] = load_global(src + (uint64_t)c * sg.ch_stride + lane);
          u[c][1] = load_global(src + (uint64_t)c * sg.ch_stride + 64 + lane);
        }
    }
    mix12(u, nc, li.nch_in, li.interp);
#pragma unroll
    for (int c = 0; c < 2; c++)
#pragma unroll
      for (int e = 0; e < 2; e++) v[c][e] = k == 0 ? u[c][e] : v[c][e] + u[c][e];
  }
}

// biquad_filter.rs:857-897: the quantum through `scratch`, on the whole wavefront when one coefficient set holds for it
// (biquad_scan_pass, waa_quantum.hpp: the static channel count fits one pass), else — per-frame sets, quanta with inf / NaN,
// WAA_DYN_NO_SCAN — serially on one lane per channel
__device__ __forceinline__ void loop_biquad(const LoopCtx& cx, const LoopItem& li, const LoopDesc& d, float (&v)[2][2]) {
  const OpDesc& op = li.op;
  const int lane = cx.lane, it = cx.it;
  float* scratch = cx.scratch;
  lds_sync();
#pragma unroll
  for (int c = 0; c < 2; c++) {
    scratch[c * RQ + lane] = v[c][0];
    scratch[c * RQ + 64 + lane] = v[c][1];
  }
  lds_sync();
  bool scan_done = false;
  if (op.i0 != 2 && !d.no_scan) {
    const int ch = lane >> 5, l = lane & 31;
    const bool act = ch < op.nch_in;
    const double* s = cx.bq_state + ((size_t)it * 2 + ch) * 4;
    float* row = scratch + ch * RQ;
    const double* cf = reinterpret_cast<const double*>(op.ptr0) + (uint64_t)cx.inst * op.u0 + (op.i0 == 1 ? (uint64_t)cx.q * 5 : 0);
    const double b0 = load_global(cf), b1 = load_global(cf + 1), b2 = load_global(cf + 2), a1 = load_global(cf + 3),
                 a2 = load_global(cf + 4);
    const f4v xv = *reinterpret_cast<const f4v*>(row + 4 * l);
    float yo[4];
    double fin[4];
    bool bad;
    // Without the near-flush guard dyn_kernel needs (fuzz seed 6278): there the QUANTUM in which a filter's tail reaches zero is
    // the item's silence flag, and a DelayNode behind it acts on that flag; a loop's members carry no such flag — counts are
    // static and every quantum is rendered — so when the state flushes moves no decision here.  The SAMPLES of a tail within a
    // few decades of 2.2e-308 may still differ from the frame-by-frame flush (far below f32's range once rounded: they are
    // zeros either way); nobody has shown more than that, and the kernel behaves as it always has.
    // (the x half of the state matters to lane 0 alone and only lane 0 reads it, as it always has: read by all 64 lanes it costs
    // seven vector registers, one occupancy step of this kernel)
    biquad_scan_pass<false>(l, b0, b1, b2, a1, a2, l == 0 ? s[0] : 0., l == 0 ? s[1] : 0., s[2], s[3], xv, yo, fin, bad);
    bad = act && bad;
    if (!__any(bad)) {
      scan_done = true;
      if (act) {
        *reinterpret_cast<f4v*>(row + 4 * l) = f4v{yo[0], yo[1], yo[2], yo[3]};
        if (l == 31) {
          double* sw = cx.bq_state + ((size_t)it * 2 + ch) * 4;
          sw[0] = fin[0];
          sw[1] = fin[1];
          sw[2] = fin[2];
          sw[3] = fin[3];
        }
      }
    }
  }
  if (!scan_done && lane < op.nch_in) {
    const double* cbase = reinterpret_cast<const double*>(op.ptr0) + (uint64_t)cx.inst * op.u0;
    // (the coefficient set of frame i: the constant one, the quantum's, or the frame's own)
    biquad_serial_frames(cx.bq_state + ((size_t)it * 2 + lane) * 4, scratch + lane * RQ, cbase,
                         op.i0 == 0 ? 0 : op.i0 == 1 ? (uint64_t)cx.q : cx.f0, op.i0 == 2 ? 1 : 0);
  }
  lds_sync();
#pragma unroll
  for (int c = 0; c < 2; c++) {
    v[c][0] = scratch[c * RQ + lane];
    v[c][1] = scratch[c * RQ + 64 + lane];
  }
}

__device__ __forceinline__ void loop_node(const LoopCtx& cx, const LoopItem& li, const LoopDesc& d, float (&v)[2][2]) {
  const OpDesc& op = li.op;
  const uint32_t inst = cx.inst, q = cx.q;
  switch (op.kind) {
    case OP_GAIN: {
      if (op.p0.mode == 2) {
#pragma unroll
        for (int e = 0; e < 2; e++) {
          const float g = load_global(op.p0.base + (uint64_t)inst * op.p0.stride + cx.f0 + e * 64 + cx.lane);
          v[0][e] *= g;
          v[1][e] *= g;
        }
      } else {  // gain.rs:163-179
        const float g = param_val(op.p0, inst, q, 0);
        const bool mute = fabsf(g) <= 1e-6f, pass = fabsf(1.f - g) <= 1e-6f;
#pragma unroll
        for (int c = 0; c < 2; c++)
#pragma unroll
          for (int e = 0; e < 2; e++) v[c][e] = mute ? 0.f : (pass ? v[c][e] : v[c][e] * g);
      }
      break;
    }
    case OP_WAVESHAPER: {
      const float* curve = reinterpret_cast<const float*>(op.ptr0);
#pragma unroll
      for (int c = 0; c < 2; c++)
        if (c < op.nch_in) {
#pragma unroll
          for (int e = 0; e < 2; e++) v[c][e] = shape_curve(curve, op.i0, v[c][e]);
        }
      break;
    }
    case OP_STEREO_PAN: {  // stereo_panner.rs:218-317, k-rate pan (gains from the host tables)
#pragma unroll
      for (int e = 0; e < 2; e++) {
        const float pan = param_val(op.p0, inst, q, 0);
        const float gl = param_val(op.p1, inst, q, 0), gr = param_val(op.p2, inst, q, 0);
        if (op.nch_in == 1) {
          const float in = v[0][e];
          v[0][e] = in * gl;
          v[1][e] = in * gr;
        } else {
          const float il = v[0][e], ir = v[1][e];
          if (pan <= 0.f) {
            v[0][e] = __builtin_fmaf(ir, gl, il);
            v[1][e] = ir * gr;
          } else {
            v[0][e] = il * gl;
            v[1][e] = __builtin_fmaf(il, gr, ir);
          }
        }
      }
      break;
    }
    case OP_BIQUAD: loop_biquad(cx, li, d, v); break;
    default: break;  // pass-through (analyser, waveshaper without a curve)
  }
}

// delay.rs:515-745 in absolute time (see waa_delay.hip; positions: waa_quantum.hpp).  Static counts: the line is read as it was written
__device__ __forceinline__ void loop_delay_reader(const LoopCtx& cx, const LoopItem& li, const LoopDesc& d, float (&v)[2][2]) {
  const uint32_t inst = cx.inst, q = cx.q;
  const uint64_t f0 = cx.f0;
  __syncthreads();  // the writer's stores of this quantum (if it rendered first) have reached L2
  const SignalRef& hs = cx.items_s[li.writer_item].out;
  const OpDesc& op = li.op;
  DelayPos p0 = {0, 0.f};
  if (op.p0.mode != 2) p0 = delay_position((double)param_val(op.p0, inst, q, 0), li.in_cycle, d.quantum_duration, d.sample_rate, 0.);
#pragma unroll
  for (int e = 0; e < 2; e++) {
    const int i = e * 64 + cx.lane;
    DelayPos p;
    if (op.p0.mode != 2) {
      p.pf = p0.pf + i;
      p.k = p0.k;
    } else {
      p = delay_position((double)load_global(op.p0.base + (uint64_t)inst * op.p0.stride + f0 + i), li.in_cycle, d.quantum_duration,
                         d.sample_rate, (double)i);
    }
    int64_t prev, next;
    delay_prev_next(f0, q, p.pf, li.in_cycle, li.num_quanta, prev, next);
    const float* hb = hs.base + (uint64_t)inst * hs.inst_stride;
#pragma unroll
    for (int c = 0; c < 2; c++)
      if (c < li.nch_out) {
        const float ps = prev >= 0 ? coherent_f(hb + (uint64_t)c * hs.ch_stride + prev) : 0.f;
        const float nsv = next >= 0 ? coherent_f(hb + (uint64_t)c * hs.ch_stride + next) : 0.f;
        v[c][e] = __builtin_fmaf(1.f - p.k, ps, p.k * nsv);
      }
  }
}

// ---- hand over (LDS) and publish (HBM)
__device__ __forceinline__ void loop_publish(const LoopCtx& cx, const LoopItem& li, const float (&v)[2][2]) {
  const int lane = cx.lane;
  const int nco = li.kind == LI_DELAY_W ? li.nch_in : li.nch_out;
  float* dst = cx.cur + (size_t)cx.it * 2 * RQ;
  float* gout = li.out.base + (uint64_t)cx.inst * li.out.inst_stride + cx.f0;
#pragma unroll
  for (int c = 0; c < 2; c++)
    if (c < nco) {
      dst[c * RQ + lane] = v[c][0];
      dst[c * RQ + 64 + lane] = v[c][1];
      store_global(gout + (uint64_t)c * li.out.ch_stride + lane, v[c][0]);
      store_global(gout + (uint64_t)c * li.out.ch_stride + 64 + lane, v[c][1]);
    }
  lds_sync();
}

__global__ __launch_bounds__(64) void loop_kernel(const LoopDesc d) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const LoopLds l = loop_lds_layout(d.n_items);
  char* base = reinterpret_cast<char*>(lds);
  LoopCtx cx;
  cx.cur = reinterpret_cast<float*>(base + l.cur);
  cx.scratch = reinterpret_cast<float*>(base + l.scratch);
  cx.bq_state = reinterpret_cast<double*>(base + l.bq_state);
  // the item descriptors once into LDS (through the kernel argument they are dependent vector loads, see waa_dyn.hip)
  cx.items_s = reinterpret_cast<LoopItem*>(base + l.items);
  cx.inst = blockIdx.x;
  const int lane = cx.lane = threadIdx.x;
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(d.items);
    uint32_t* dst = reinterpret_cast<uint32_t*>(cx.items_s);
    const int words = d.n_items * (int)(sizeof(LoopItem) / 4);
    for (int i = lane; i < words; i += 64) dst[i] = load_global(src + i);
  }
  __builtin_amdgcn_s_setreg(1 | (6 << 6) | (1 << 11), 0);  // f64 denormals flushed (FTZ/DAZ render scope)
  for (int i = lane; i < d.n_items * 8; i += 64) cx.bq_state[i] = 0.;
  lds_sync();

  for (uint32_t q = 0; q < d.n_quanta; q++) {
    cx.q = q;
    cx.f0 = (uint64_t)q * RQ;
    for (int it = 0; it < d.n_items; it++) {
      cx.it = it;
      const LoopItem& li = cx.items_s[it];
      const int kind = li.kind;
      float v[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
      if (kind != LI_DELAY_R) loop_gather(cx, li, v);
      if (kind == LI_NODE)
        loop_node(cx, li, d, v);
      else if (kind == LI_DELAY_R)
        loop_delay_reader(cx, li, d, v);
      loop_publish(cx, li, v);
    }
  }
}

void launch_loop(const LoopDesc& d, void* stream) {
  const size_t lds = loop_lds_layout(d.n_items).total;
  if (lds > 64 * 1024)
    raise_lds_limit(reinterpret_cast<const void*>(loop_kernel));
  LoopDesc dd = d;
  dd.no_scan = measure_switch("WAA_DYN_NO_SCAN") ? 1u : 0u;
  hipLaunchKernelGGL(loop_kernel, dim3(d.n_inst), dim3(64), lds, (hipStream_t)stream, dd);
}

}  // namespace waa
