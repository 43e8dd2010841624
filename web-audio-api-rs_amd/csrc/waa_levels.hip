// waa_levels.hip — levels of the rendered output and the gained PCM pack (waa_output_levels, waa_output_level_series,
// waa_download_all_pcm16_gain; the definitions: include/waa_hip_device.h).  An extension like the packer of
// waa_decode.hip: the reference hands back f32 planes and nothing else.  Nothing here is a plan step.
//
// Every value is defined on the sample's bits (a = bits & 0x7fffffff, e = a >> 23), so that the library's
// -fgpu-flush-denormals-to-zero decides nothing: a denormal takes part in the peak with its own bits and in the energy as +0.0.
//
// output_levels_kernel: one workgroup of 256 threads per (row, block of 64 quanta).  Half a wavefront — 32 lanes — holds one
// quantum, a lane four adjacent frames: s = (s0 + s1) + (s2 + s3), then an xor-butterfly over the 32 lanes (masks 1 .. 16).  IEEE
// addition commutes, so both partners of an exchange compute the same bits and every lane ends with the root of the adjacent-pairs
// tree in index order.  A wavefront walks 16 of the block's quanta, two at a time, the next pair's load in flight while it works on
// this one; the 64 roots meet in LDS, where the first wavefront runs the same butterfly over 64 lanes for the block's b_m.  Counts
// are 32-bit integers in each lane (a block has 8192 frames) and the first non-finite frame an offset into the block; they become
// the record's 64-bit values once per block.
// output_level_rows_kernel: one thread per row adds the row's b_m in ascending order — the one sequential sum of the definition.
#include <hip/hip_runtime.h>

#include "waa_internal.hpp"

namespace waa {

namespace {
__device__ __forceinline__ double xor_add(double v, int mask) { return v + __shfl_xor(v, mask, 64); }
__device__ __forceinline__ uint32_t shfl_xor_u32(uint32_t v, int mask) { return (uint32_t)__shfl_xor((int)v, mask, 64); }
__device__ __forceinline__ uint32_t xor_max(uint32_t v, int mask) {
  const uint32_t o = shfl_xor_u32(v, mask);
  return o > v ? o : v;
}
__device__ __forceinline__ uint32_t xor_min(uint32_t v, int mask) {
  const uint32_t o = shfl_xor_u32(v, mask);
  return o < v ? o : v;
}
constexpr uint32_t NO_FRAME = 0xffffffffu;

// a lane's four frames f0 .. f0 + 3 of a row of `frames`; a frame past the end, and every frame of a row the signal does not carry,
// is +0.0 (e == 0: it adds nothing to any value).  Nothing past the row's last frame is read.
__device__ __forceinline__ f4v load_frames(const float* src, uint64_t f0, uint64_t frames, bool carried, bool aligned) {
  f4v v = {0.f, 0.f, 0.f, 0.f};
  if (!carried || f0 >= frames) return v;
  const uint64_t left = frames - f0;
  if (left >= 4 && aligned) return load_global_f4(src + f0);
  v.x = load_global(src + f0);
  if (left > 1) v.y = load_global(src + f0 + 1);
  if (left > 2) v.z = load_global(src + f0 + 2);
  if (left > 3) v.w = load_global(src + f0 + 3);
  return v;
}
// one quantum in half a wavefront: this lane's four frames `cur` at offset `off` of the block.  The lane's counts go on in n_*;
// the quantum's e_q and p_q go to LDS from the half's first lane.
struct LaneCounts {
  uint32_t n_nonfinite, n_clipped, first;
};
__device__ __forceinline__ void quantum(const f4v cur, uint32_t off, uint32_t l32, LaneCounts& k, double* s_e, uint32_t* s_p) {
  const float x[4] = {cur.x, cur.y, cur.z, cur.w};
  double s[4];
  uint32_t pk = 0;
#pragma unroll
  for (uint32_t j = 0; j < 4; j++) {
    const uint32_t a = __float_as_uint(x[j]) & 0x7fffffffu, e = a >> 23;
    const bool finite = e != 255u;
    pk = finite && a > pk ? a : pk;
    const double xd = (double)x[j];
    s[j] = e >= 1u && e <= 254u ? xd * xd : 0.0;
    const float v = x[j] * 32768.f;
    k.n_clipped += finite && (v > 32767.f || v < -32768.f) ? 1u : 0u;
    k.n_nonfinite += finite ? 0u : 1u;
    k.first = !finite && off + j < k.first ? off + j : k.first;
  }
  double t = (s[0] + s[1]) + (s[2] + s[3]);
#pragma unroll
  for (int m = 1; m < 32; m <<= 1) {
    t = xor_add(t, m);
    pk = xor_max(pk, m);
  }
  if (l32 == 0) {
    s_e[off >> 7] = t;  // (off >> 7: the quantum of the block)
    s_p[off >> 7] = pk;
  }
}
}  // namespace

// (eight wavefronts per SIMD: the pass is a stream of loads, and 512 / 8 = 64 vector registers are enough for it)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void output_levels_kernel(const LevelsDesc d) {
  __shared__ double s_e[LEVEL_BLOCK_QUANTA];
  __shared__ uint32_t s_p[LEVEL_BLOCK_QUANTA];
  __shared__ uint32_t s_cnt[4][3];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, half = lane >> 5, l32 = lane & 31u;
  const uint32_t n_rows = d.n_items * d.nch_out;
  const uint64_t block_frame0 = (uint64_t)blockIdx.x * LEVEL_BLOCK_QUANTA * 128;
  // this lane's frames of the block: quantum wave * 16 + it * 2 + half (it = 0 .. 7), frames l32 * 4 .. + 3 of it
  const uint32_t off0 = (wave * 16 + half) * 128 + l32 * 4;
  // (more rows than a grid has: strides of the grid's rows, like the packer)
  for (uint32_t row = blockIdx.y; row < n_rows; row += gridDim.y) {
    const uint32_t item = row / d.nch_out, c = row - item * d.nch_out;
    const bool carried = c < d.nch_in;
    const float* src = d.in + (uint64_t)item * d.in_item_stride + (uint64_t)c * d.in_ch_stride;
    // 16-byte loads need the ROW's address aligned (a quantum starts 512 bytes further on); the strides promise nothing
    const bool aligned = (reinterpret_cast<uintptr_t>(src) & 15u) == 0;
    LaneCounts k = {0u, 0u, NO_FRAME};
    if (carried && aligned && block_frame0 + LEVEL_BLOCK_QUANTA * 128 <= d.frames) {
      // a whole block of an aligned row, the same for every lane of the workgroup: nothing to decide per load, and the next pair of
      // quanta is in flight while this one is worked on (the last iteration loads the first pair again rather than branch)
      const float* p = src + block_frame0 + off0;
      f4v cur = load_global_f4(p);
#pragma unroll 1
      for (uint32_t it = 0; it < 8; it++) {
        const f4v nxt = load_global_f4(p + ((it + 1) & 7u) * 256);
        quantum(cur, off0 + it * 256, l32, k, s_e, s_p);
        cur = nxt;
      }
    } else {
      // the row's last block, a row that starts off a 16-byte boundary, a channel the signal does not carry
#pragma unroll 1
      for (uint32_t it = 0; it < 8; it++)
        quantum(load_frames(src, block_frame0 + off0 + it * 256, d.frames, carried, aligned), off0 + it * 256, l32, k, s_e, s_p);
    }
    uint32_t n_nonfinite = k.n_nonfinite, n_clipped = k.n_clipped, first = k.first;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
      n_nonfinite += shfl_xor_u32(n_nonfinite, m);
      n_clipped += shfl_xor_u32(n_clipped, m);
      first = xor_min(first, m);
    }
    if (lane == 0) s_cnt[wave][0] = n_nonfinite, s_cnt[wave][1] = first, s_cnt[wave][2] = n_clipped;
    __syncthreads();
    if (wave == 0) {
      double t = s_e[lane];
      uint32_t pk = s_p[lane];
      // the per-quantum values of the block: 64 adjacent values per array
      const uint64_t q = (uint64_t)blockIdx.x * LEVEL_BLOCK_QUANTA + lane;
      if (q < d.n_quanta) {
        store_global(d.q_sum_sq + (uint64_t)row * d.n_quanta + q, t);
        store_global(d.q_peak + (uint64_t)row * d.n_quanta + q, pk);
      }
#pragma unroll
      for (int m = 1; m < 64; m <<= 1) {
        t = xor_add(t, m);
        pk = xor_max(pk, m);
      }
      if (lane == 0) {
        uint32_t f = s_cnt[0][1];
        for (int w = 1; w < 4; w++) f = s_cnt[w][1] < f ? s_cnt[w][1] : f;
        LevelRec r;
        r.sum_sq = t;
        r.n_nonfinite = (uint64_t)s_cnt[0][0] + s_cnt[1][0] + s_cnt[2][0] + s_cnt[3][0];
        r.first_nonfinite = f == NO_FRAME ? ~0ull : block_frame0 + f;
        r.n_clipped = (uint64_t)s_cnt[0][2] + s_cnt[1][2] + s_cnt[2][2] + s_cnt[3][2];
        r.peak_bits = pk;
        r.reserved = 0;
        d.blocks[(uint64_t)row * d.n_blocks + blockIdx.x] = r;
      }
    }
    __syncthreads();  // (the next row of a strided walk writes the same LDS)
  }
}

__global__ __launch_bounds__(256) void output_level_rows_kernel(const LevelsDesc d) {
  const uint64_t row = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= (uint64_t)d.n_items * d.nch_out) return;
  const LevelRec* blk = d.blocks + row * d.n_blocks;
  LevelRec r;
  r.sum_sq = 0.0;
  r.n_nonfinite = 0, r.n_clipped = 0, r.first_nonfinite = ~0ull;
  r.peak_bits = 0, r.reserved = 0;
  for (uint32_t m = 0; m < d.n_blocks; m++) {  // ascending and sequential: the definition's order
    const LevelRec k = blk[m];
    r.sum_sq = r.sum_sq + k.sum_sq;
    r.n_nonfinite += k.n_nonfinite;
    r.n_clipped += k.n_clipped;
    r.first_nonfinite = k.first_nonfinite < r.first_nonfinite ? k.first_nonfinite : r.first_nonfinite;
    r.peak_bits = k.peak_bits > r.peak_bits ? k.peak_bits : r.peak_bits;
  }
  d.rows[row] = r;
}

void launch_output_levels(const LevelsDesc& d, void* stream) {
  const uint64_t n_rows = (uint64_t)d.n_items * d.nch_out;
  if (d.frames == 0 || n_rows == 0) return;
  dim3 grid(d.n_blocks, (unsigned)(n_rows < MAX_GRID_ROWS ? n_rows : MAX_GRID_ROWS));
  hipLaunchKernelGGL(output_levels_kernel, grid, dim3(256), 0, (hipStream_t)stream, d);
}
void launch_output_level_rows(const LevelsDesc& d, void* stream) {
  const uint64_t n_rows = (uint64_t)d.n_items * d.nch_out;
  if (d.frames == 0 || n_rows == 0) return;
  hipLaunchKernelGGL(output_level_rows_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d);
}

// pcm16_pack_kernel (waa_decode.hip) with the context's gain in front: one f32 multiply of its own (the build never contracts),
// then the packer's steps word for word.  x * 1.0f is x, so a gain of one gives the packer's bits.
__global__ __launch_bounds__(256) void pcm16_pack_gain_kernel(const EncodeGainDesc g) {
  const EncodeDesc& d = g.e;
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= d.frames) return;
  for (uint32_t item = blockIdx.y; item < d.n_items; item += gridDim.y) {  // (more than 65535 contexts: strides of the grid's rows)
    const float gain = load_global(g.gain + item);
    int16_t* dst = d.pcm + ((uint64_t)item * d.frames + i) * d.nch_out;
    for (uint32_t c = 0; c < d.nch_out; c++) {
      float v = c < d.nch_in ? load_global(d.in + (uint64_t)item * d.in_item_stride + (uint64_t)c * d.in_ch_stride + i) : 0.f;
      v = v * gain;
      v = v * 32768.f;
      v = v < -32768.f ? -32768.f : (v > 32767.f ? 32767.f : v);
      dst[c] = (int16_t)__float2int_rn(v != v ? 0.f : v);
    }
  }
}
void launch_pcm16_pack_gain(const EncodeGainDesc& d, void* stream) {
  if (d.e.frames == 0 || d.e.n_items == 0) return;
  dim3 grid((unsigned)((d.e.frames + 255) / 256), d.e.n_items < MAX_GRID_ROWS ? d.e.n_items : MAX_GRID_ROWS);
  hipLaunchKernelGGL(pcm16_pack_gain_kernel, grid, dim3(256), 0, (hipStream_t)stream, d);
}

}  // namespace waa
