// waa_route.hip — ChannelSplitterNode / ChannelMergerNode (src/node/channel_splitter.rs:183-210, channel_merger.rs:145-172):
// the one place of channel routing where samples have to move.
//
// A ChannelMergerNode's output channel k is its input port k: the port's connections, each mixed to ONE channel with the node's
// interpretation (quantum.rs:285-432), summed in connection order.  A ChannelSplitterNode whose input has more than one
// connection needs its input bus: channel k of the bus is the sum of channel k of every connection that has one (explicit,
// discrete).  Both are "row r of the output = sum of a short list of terms", and a term is a channel of a source signal or one
// of the three speakers down-mixes to mono:
//     2 -> 1   0.5 * (l + r)                                        quantum.rs:387-397
//     4 -> 1   0.25 * (l + r + sl + sr)                             quantum.rs:398-412
//     6 -> 1   sqrt05.mul_add(l + r, 0.5.mul_add(sl + sr, c))       quantum.rs:413-432 (the one fused form of the file)
// every other count, and the discrete interpretation, keep channel 0.  Each term is ONE expression in the reference's order (the
// file is built with -ffp-contract=off: only the fmaf calls fuse); successive terms are added left to right in f32.
//
// Shape: pure streaming, no state, no LDS.  One workgroup of four wavefronts per (instance, row, 2048-frame tile); a wavefront
// owns a 512-frame sub-tile and every lane two 16-byte pieces of it, 1 KiB apart, so that a wave's loads are two fully coalesced
// 1 KiB requests per source channel.  All loads of a term (2 .. 10 of 16 bytes per lane) are issued before the first arithmetic
// on them, and the two stores come last.  Signals are padded to whole tiles, so there are no tails; a row without terms is
// written as zeros (the allocator's contents are never relied on: WAA_POISON_ALLOC).
#include <hip/hip_runtime.h>

#include "waa_internal.hpp"

namespace waa {

namespace {

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float down2(float l, float r) { return 0.5f * (l + r); }
__device__ __forceinline__ float down4(float l, float r, float sl, float sr) { return 0.25f * (l + r + sl + sr); }
__device__ __forceinline__ float down6(float l, float r, float c, float sl, float sr) {
  const float sqrt05 = 0.70710678118654752440f;  // (0.5_f32).sqrt()
  return fmaf(sqrt05, l + r, fmaf(0.5f, sl + sr, c));
}

// the two 16-byte pieces (frames f and f + 256 of the tile) of one term
__device__ __forceinline__ void route_term(const RouteTerm& t, uint32_t inst, uint64_t f, float4* v0, float4* v1) {
  const float* p = t.base + (uint64_t)inst * t.inst_stride + f;
  const uint64_t cs = t.ch_stride;
  switch (t.mode) {
    case RT_DOWN2: {
      const float4 l0 = ld4(p), l1 = ld4(p + 256), r0 = ld4(p + cs), r1 = ld4(p + cs + 256);
      *v0 = make_float4(down2(l0.x, r0.x), down2(l0.y, r0.y), down2(l0.z, r0.z), down2(l0.w, r0.w));
      *v1 = make_float4(down2(l1.x, r1.x), down2(l1.y, r1.y), down2(l1.z, r1.z), down2(l1.w, r1.w));
      break;
    }
    case RT_DOWN4: {
      const float4 l0 = ld4(p), l1 = ld4(p + 256), r0 = ld4(p + cs), r1 = ld4(p + cs + 256);
      const float4 a0 = ld4(p + 2 * cs), a1 = ld4(p + 2 * cs + 256), b0 = ld4(p + 3 * cs), b1 = ld4(p + 3 * cs + 256);
      *v0 = make_float4(down4(l0.x, r0.x, a0.x, b0.x), down4(l0.y, r0.y, a0.y, b0.y), down4(l0.z, r0.z, a0.z, b0.z),
                        down4(l0.w, r0.w, a0.w, b0.w));
      *v1 = make_float4(down4(l1.x, r1.x, a1.x, b1.x), down4(l1.y, r1.y, a1.y, b1.y), down4(l1.z, r1.z, a1.z, b1.z),
                        down4(l1.w, r1.w, a1.w, b1.w));
      break;
    }
    case RT_DOWN6: {  // (channel 3, the LFE, is not part of the mix)
      const float4 l0 = ld4(p), l1 = ld4(p + 256), r0 = ld4(p + cs), r1 = ld4(p + cs + 256);
      const float4 c0 = ld4(p + 2 * cs), c1 = ld4(p + 2 * cs + 256);
      const float4 a0 = ld4(p + 4 * cs), a1 = ld4(p + 4 * cs + 256), b0 = ld4(p + 5 * cs), b1 = ld4(p + 5 * cs + 256);
      *v0 = make_float4(down6(l0.x, r0.x, c0.x, a0.x, b0.x), down6(l0.y, r0.y, c0.y, a0.y, b0.y), down6(l0.z, r0.z, c0.z, a0.z, b0.z),
                        down6(l0.w, r0.w, c0.w, a0.w, b0.w));
      *v1 = make_float4(down6(l1.x, r1.x, c1.x, a1.x, b1.x), down6(l1.y, r1.y, c1.y, a1.y, b1.y), down6(l1.z, r1.z, c1.z, a1.z, b1.z),
                        down6(l1.w, r1.w, c1.w, a1.w, b1.w));
      break;
    }
    default: {
      const float* q = p + (uint64_t)t.ch * cs;
      *v0 = ld4(q);
      *v1 = ld4(q + 256);
      break;
    }
  }
}

__global__ __launch_bounds__(256) void route_kernel(const RouteDesc d) {
  const uint32_t n_tiles = (uint32_t)(d.frames / TILE);
  uint32_t bid = blockIdx.x;
  const uint32_t tile = bid % n_tiles;
  bid /= n_tiles;
  const uint32_t row = bid % d.rows, inst = bid / d.rows;
  if (inst >= d.n_inst) return;
  // frames [f, f + 4) and [f + 256, f + 260): wavefront w owns frames [512 w, 512 w + 512) of the tile
  const uint64_t f = (uint64_t)tile * TILE + (uint64_t)(threadIdx.x >> 6) * 512 + (uint64_t)(threadIdx.x & 63) * 4;
  const uint32_t t0 = d.row_off[row], t1 = d.row_off[row + 1];
  float4 acc0 = make_float4(0.f, 0.f, 0.f, 0.f), acc1 = acc0;
  if (t0 < t1) {
    route_term(d.terms[t0], inst, f, &acc0, &acc1);
    if (t0 + 1 < t1) {
      // two terms (a port with two connections, a splitter behind two sources): the second one's loads are in flight with the first's
      float4 v0, v1;
      route_term(d.terms[t0 + 1], inst, f, &v0, &v1);
      acc0 = add4(acc0, v0);
      acc1 = add4(acc1, v1);
      for (uint32_t t = t0 + 2; t < t1; t++) {
        route_term(d.terms[t], inst, f, &v0, &v1);
        acc0 = add4(acc0, v0);
        acc1 = add4(acc1, v1);
      }
    }
  }
  float* out = d.out.base + (uint64_t)inst * d.out.inst_stride + (uint64_t)row * d.out.ch_stride + f;
  *reinterpret_cast<float4*>(out) = acc0;
  *reinterpret_cast<float4*>(out + 256) = acc1;
}

}  // namespace

void launch_route(const RouteDesc& d, void* stream) {
  // (the planner refuses a batch whose block count would not fit the grid's x dimension)
  const uint64_t blocks = (d.frames / TILE) * (uint64_t)d.rows * d.n_inst;
  if (blocks == 0) return;
  hipLaunchKernelGGL(route_kernel, dim3((uint32_t)blocks), dim3(256), 0, (hipStream_t)stream, d);
}

}  // namespace waa
