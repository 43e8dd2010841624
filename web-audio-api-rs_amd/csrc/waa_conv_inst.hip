// waa_conv_inst.hip — ConvolverNode with ONE IMPULSE RESPONSE PER INSTANCE (waa_node_desc.i[1] = 1) on gfx950.
//
// The shared-response path (waa_conv.hip, waa_conv3.hip) packs two instances' real streams into one complex transform,
// Z = A + iB, and multiplies by the one response spectrum H: (a + i b) * h = a * h + i (b * h).  With two different responses
// the wanted spectrum is  Y = A H_a + i B H_b.  The transforms in front of and behind the product stay what they are; the
// product separates the pair first.  For real a, b:  conj(Z[N - k]) = A[k] - i B[k], hence with
//     S[k] = Z[k] + conj(Z[N - k]) = 2 A[k]          D[k] = Z[k] - conj(Z[N - k]) = 2 i B[k]
//     Y[k]           = (S[k] H_a[k] + D[k] H_b[k]) / 2
//     conj(Y[N - k]) = (S[k] H_a[k] - D[k] H_b[k]) / 2          (H_a[N - k] = conj(H_a[k]): the responses are real)
// — the identity  Y[k] = Z[k] H_s[k] + conj(Z[N - k]) H_d[k],  H_s/d = (H_a +- H_b) / 2, regrouped: two complex multiply-adds per
// partition for the two outputs Y[k] and Y[N - k] instead of four, and the spectra are stored per INSTANCE (H_a, H_b: a pair's
// members are read by instance index, an odd batch's last instance is its own partner).  A thread owns position p and its
// mirror m = conv_mirror(p) (waa_conv_mirror.hpp), takes part when p <= m, reads Z[p] and Z[m] of every block once and only
// H[p] of the two instances (half of each spectrum is ever read).  Bins 0 and N / 2 are their own mirrors: p == m, S = 2 Re Z,
// D = 2 i Im Z, one store.  The division by two is exact.
//
// Two forms, as in waa_conv.hip:
//   conv_inst_win_kernel<KT, PC>  one term per output channel and 8 < P <= PC: the sliding register window of conv_mac_win_kernel —
//                                 both response columns stay in registers, every X value is read once.
//   conv_inst_mac_kernel<KT, PC>  any routing (the two-term outputs of a 4-channel response) and any P <= 24: partitions in chunks
//                                 of PC, KT output blocks per register tile, the inputs of a tile re-read per chunk (L2 hits).
// Loads are unconditional with a clamped index and the zero is selected afterwards (behind
// `cond ? load : 0` the compiler waits for every load on the spot).  No LDS, no scratch.
#include <hip/hip_runtime.h>

#include "waa_conv_mirror.hpp"
#include "waa_internal.hpp"

namespace waa {

namespace {

typedef float c2v __attribute__((ext_vector_type(2)));  // one complex value in a 64-bit register pair: (re, im)

// acc += h * x: the two packed FMAs of waa_conv.hip's cmac_pk (same four FMAs in the same order as the scalar form)
__device__ __forceinline__ void cmac_pk(c2v& acc, const c2v h, const c2v x) {
  asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[0,1,1]" : "+v"(acc) : "v"(h), "v"(x));
  asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[1,0,0]" : "+v"(acc) : "v"(h), "v"(x));
}
// S = u + conj(v), D = u - conj(v)
__device__ __forceinline__ c2v sum_conj(c2v u, c2v v) { return c2v{u.x + v.x, u.y - v.y}; }
__device__ __forceinline__ c2v dif_conj(c2v u, c2v v) { return c2v{u.x - v.x, u.y + v.y}; }

struct InstPos {
  uint32_t pos, mir;
  uint32_t pair, ia, ib;
  int co;
  bool active, self;
};
__device__ __forceinline__ InstPos inst_pos(const ConvDesc& d, int log2n) {
  InstPos r;
  r.pos = blockIdx.x * 256 + threadIdx.x;
  r.mir = conv_mirror(r.pos, d.fft3 ? CONV_ORDER_FFT3 : CONV_ORDER_BREV, log2n);
  r.active = r.pos <= r.mir;
  r.self = r.pos == r.mir;
  r.pair = blockIdx.y / (uint32_t)d.cout;
  r.co = (int)(blockIdx.y % (uint32_t)d.cout);
  r.ia = r.pair * 2;
  r.ib = r.ia + 1 < d.n_inst ? r.ia + 1 : r.ia;  // (an odd batch's last instance: its own partner, b = 0 from the forward transform)
  return r;
}
__device__ __forceinline__ void inst_store(const ConvDesc& d, const InstPos& q, Cplx* Yc, int k, c2v accp, c2v accm) {
  c2v* y = reinterpret_cast<c2v*>(Yc + (uint64_t)k * d.n);
  y[q.pos] = c2v{0.5f * (accp.x + accm.x), 0.5f * (accp.y + accm.y)};
  if (!q.self) y[q.mir] = c2v{0.5f * (accp.x - accm.x), -0.5f * (accp.y - accm.y)};
}

template <int KT, int PC>
__global__ __launch_bounds__(256) void conv_inst_mac_kernel(const ConvDesc d, int log2n) {
  const InstPos q = inst_pos(d, log2n);
  if (!q.active) return;
  const int n = d.n, nb = d.nb, P = d.parts;
  const uint64_t h_inst = (uint64_t)d.ir_nch * P * n;
  Cplx* Yc = d.Y + ((uint64_t)q.pair * d.cout + q.co) * nb * n;
  const c2v zero = {0.f, 0.f};
  for (int k0 = d.kb0; k0 < d.kb1; k0 += KT) {
    c2v accp[KT], accm[KT];
#pragma unroll
    for (int i = 0; i < KT; i++) accp[i] = accm[i] = zero;
    for (int t = 0; t < d.n_terms; t++) {
      if (d.terms[t].out_ch != q.co) continue;
      const c2v* Ha = reinterpret_cast<const c2v*>(d.H + (uint64_t)q.ia * h_inst + (uint64_t)d.terms[t].ir_ch * P * n + q.pos);
      const c2v* Hb = reinterpret_cast<const c2v*>(d.H + (uint64_t)q.ib * h_inst + (uint64_t)d.terms[t].ir_ch * P * n + q.pos);
      const c2v* Xc = reinterpret_cast<const c2v*>(d.X + ((uint64_t)q.pair * d.cin + d.terms[t].in_ch) * nb * n);
      for (int pc0 = 0; pc0 < P; pc0 += PC) {
        c2v ha[PC], hb[PC];
#pragma unroll
        for (int i = 0; i < PC; i++) {
          const uint64_t off = (uint64_t)(pc0 + i < P ? pc0 + i : 0) * n;
          ha[i] = Ha[off];
          hb[i] = Hb[off];
        }
#pragma unroll
        for (int i = 0; i < PC; i++)
          if (pc0 + i >= P) ha[i] = hb[i] = zero;
#pragma clang loop unroll(full)
        for (int jj = 0; jj < KT + PC - 1; jj++) {
          const int j = k0 - pc0 - (PC - 1) + jj;
          const bool ok = j >= 0 && j < nb;
          const uint64_t off = (uint64_t)(ok ? j : 0) * n;
          const c2v u = Xc[off + q.pos], v = Xc[off + q.mir];
          const c2v s = ok ? sum_conj(u, v) : zero, dd = ok ? dif_conj(u, v) : zero;
#pragma clang loop unroll(full)
          for (int i = 0; i < KT; i++) {
            const int pl = i + (PC - 1) - jj;  // local partition index, compile-time after unrolling
            if (pl >= 0 && pl < PC) {
              cmac_pk(accp[i], ha[pl], s);
              cmac_pk(accm[i], hb[pl], dd);
            }
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < KT; i++)
      if (k0 + i < d.kb1) inst_store(d, q, Yc, k0 + i, accp[i], accm[i]);
  }
}

template <int KT, int PC>
__global__ __launch_bounds__(256) void conv_inst_win_kernel(const ConvDesc d, int log2n) {
  const InstPos q = inst_pos(d, log2n);
  if (!q.active) return;
  const int n = d.n, nb = d.nb, P = d.parts;
  const uint64_t h_inst = (uint64_t)d.ir_nch * P * n;
  int term = 0;
  for (int t = 0; t < d.n_terms; t++)
    if (d.terms[t].out_ch == q.co) term = t;
  Cplx* Yc = d.Y + ((uint64_t)q.pair * d.cout + q.co) * nb * n;
  const c2v* Ha = reinterpret_cast<const c2v*>(d.H + (uint64_t)q.ia * h_inst + (uint64_t)d.terms[term].ir_ch * P * n + q.pos);
  const c2v* Hb = reinterpret_cast<const c2v*>(d.H + (uint64_t)q.ib * h_inst + (uint64_t)d.terms[term].ir_ch * P * n + q.pos);
  const c2v* Xc = reinterpret_cast<const c2v*>(d.X + ((uint64_t)q.pair * d.cin + d.terms[term].in_ch) * nb * n);
  const c2v zero = {0.f, 0.f};
  c2v ha[PC], hb[PC];
#pragma unroll
  for (int i = 0; i < PC; i++) {
    const uint64_t off = (uint64_t)(i < P ? i : 0) * n;
    ha[i] = Ha[off];
    hb[i] = Hb[off];
  }
#pragma unroll
  for (int i = 0; i < PC; i++)
    if (i >= P) ha[i] = hb[i] = zero;
  c2v ws[PC - 1], wd[PC - 1];  // S and D of blocks k0 - (PC - 1) .. k0 - 1
#pragma unroll
  for (int i = 0; i < PC - 1; i++) ws[i] = wd[i] = zero;
  if (d.kb0 > 0) {  // a later block range: the window's history comes back from X
#pragma unroll
    for (int i = 0; i < PC - 1; i++) {
      const int j = d.kb0 - (PC - 1) + i;
      const uint64_t off = (uint64_t)(j >= 0 ? j : 0) * n;
      const c2v u = Xc[off + q.pos], v = Xc[off + q.mir];
      ws[i] = j >= 0 ? sum_conj(u, v) : zero;
      wd[i] = j >= 0 ? dif_conj(u, v) : zero;
    }
  }
  const int kend = d.kb1;
  for (int k0 = d.kb0; k0 < kend; k0 += KT) {
    c2v xs[KT], xd[KT];  // S and D of blocks k0 .. k0 + KT - 1
#pragma unroll
    for (int i = 0; i < KT; i++) {
      const uint64_t off = (uint64_t)(k0 + i < kend ? k0 + i : kend - 1) * n;
      const c2v u = Xc[off + q.pos], v = Xc[off + q.mir];
      xs[i] = sum_conj(u, v);
      xd[i] = dif_conj(u, v);
    }
#pragma unroll
    for (int i = 0; i < KT; i++)
      if (k0 + i >= kend) xs[i] = xd[i] = zero;
    c2v accp[KT], accm[KT];
#pragma unroll
    for (int i = 0; i < KT; i++) accp[i] = accm[i] = zero;
#pragma clang loop unroll(full)
    for (int jj = 0; jj < KT + PC - 1; jj++) {
      const c2v s = jj < PC - 1 ? ws[jj < PC - 1 ? jj : 0] : xs[jj >= PC - 1 ? jj - (PC - 1) : 0];
      const c2v dd = jj < PC - 1 ? wd[jj < PC - 1 ? jj : 0] : xd[jj >= PC - 1 ? jj - (PC - 1) : 0];
#pragma clang loop unroll(full)
      for (int i = 0; i < KT; i++) {
        const int pl = i + (PC - 1) - jj;  // partition index, compile-time after unrolling
        if (pl >= 0 && pl < PC) {
          cmac_pk(accp[i], ha[pl], s);
          cmac_pk(accm[i], hb[pl], dd);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < KT; i++)
      if (k0 + i < kend) inst_store(d, q, Yc, k0 + i, accp[i], accm[i]);
    // slide the window by KT blocks
#pragma unroll
    for (int w = 0; w < PC - 1; w++) {
      const int src = w + KT;  // index into the concatenation [window | tile]
      ws[w] = src < PC - 1 ? ws[src < PC - 1 ? src : 0] : xs[src >= PC - 1 ? src - (PC - 1) : 0];
      wd[w] = src < PC - 1 ? wd[src < PC - 1 ? src : 0] : xd[src >= PC - 1 ? src - (PC - 1) : 0];
    }
  }
}

// conv_direct_kernel (waa_conv.hip) with the taps of the workgroup's own instance: direct time-domain FIR, f64 accumulation,
// per term the f64 sum rounded to f32 and the terms added in f32 (convolver.rs:430-441)
constexpr int DIRECT_TILE = 1024;
__global__ __launch_bounds__(256) void conv_inst_direct_kernel(const ConvDesc d) {
  __shared__ float xs[2][DIRECT_TILE + DIRECT_MAX_TAPS];
  __shared__ float hs[4][DIRECT_MAX_TAPS];
  const int tid = threadIdx.x;
  const uint64_t f0 = ((uint64_t)blockIdx.x + (uint64_t)d.kb0) * DIRECT_TILE;  // (kb0 / kb1: 1024-frame pieces here)
  const int co = blockIdx.y;
  const uint32_t inst = blockIdx.z;
  const int taps = (int)d.ir_len;
  for (int c = 0; c < d.cin; c++) {
    const float* p = d.in.base + (uint64_t)inst * d.in.inst_stride + (uint64_t)c * d.in.ch_stride;
    for (int i = tid; i < DIRECT_TILE + DIRECT_MAX_TAPS; i += 256) {
      const int64_t f = (int64_t)f0 - DIRECT_MAX_TAPS + i;
      xs[c][i] = (f >= 0 && (uint64_t)f < d.in_valid) ? p[f] : 0.f;
    }
  }
  const float* ir = d.ir + (uint64_t)inst * d.ir_inst_stride;
  for (int t = 0; t < d.n_terms; t++)
    for (int i = tid; i < DIRECT_MAX_TAPS; i += 256) hs[t][i] = i < taps ? ir[(uint64_t)d.terms[t].ir_ch * d.ir_len + i] : 0.f;
  __syncthreads();
  float* o = d.out.base + (uint64_t)inst * d.out.inst_stride + (uint64_t)co * d.out.ch_stride;
  for (int i = tid; i < DIRECT_TILE; i += 256) {
    float sum = 0.f;
    bool first = true;
    for (int t = 0; t < d.n_terms; t++) {
      if (d.terms[t].out_ch != co) continue;
      const float* x = xs[d.terms[t].in_ch] + DIRECT_MAX_TAPS + i;
      double acc = 0.;
      for (int k = 0; k < taps; k++) acc = __builtin_fma((double)hs[t][k], (double)x[-k], acc);
      sum = first ? (float)acc : sum + (float)acc;
      first = false;
    }
    const uint64_t f = f0 + i;
    if (f < d.frames) o[f] = sum;
  }
}

}  // namespace

void launch_conv_inst_direct(const ConvDesc& d, void* stream) {
  if (conv_instances_sliced(d, [&](const ConvDesc& s) { launch_conv_inst_direct(s, stream); })) return;  // (gridDim.z)
  dim3 grid((unsigned)(d.kb1 - d.kb0), d.cout, d.n_inst);
  hipLaunchKernelGGL(conv_inst_direct_kernel, grid, dim3(256), 0, (hipStream_t)stream, d);
}

void launch_conv_inst_mac(const ConvDesc& d, void* stream) {
  if (conv_pairs_sliced(d, (uint32_t)d.cout, [&](const ConvDesc& s) { launch_conv_inst_mac(s, stream); })) return;  // (gridDim.y)
  dim3 grid(d.n / 256, d.n_pairs * (uint32_t)d.cout);
  const int log2n = 31 - __builtin_clz((unsigned)d.n);
  bool one_term = true;
  for (int co = 0; co < d.cout; co++) {
    int cnt = 0;
    for (int t = 0; t < d.n_terms; t++) cnt += d.terms[t].out_ch == co;
    one_term &= cnt == 1;
  }
  if (one_term && d.parts > 8 && d.parts <= 24) {
    if (d.parts <= 12)
      hipLaunchKernelGGL((conv_inst_win_kernel<8, 12>), grid, dim3(256), 0, (hipStream_t)stream, d, log2n);
    else if (d.parts <= 16)
      hipLaunchKernelGGL((conv_inst_win_kernel<8, 16>), grid, dim3(256), 0, (hipStream_t)stream, d, log2n);
    else
      hipLaunchKernelGGL((conv_inst_win_kernel<4, 24>), grid, dim3(256), 0, (hipStream_t)stream, d, log2n);
    return;
  }
  hipLaunchKernelGGL((conv_inst_mac_kernel<16, 8>), grid, dim3(256), 0, (hipStream_t)stream, d, log2n);
}

}  // namespace waa
