// tools/emulate_shim/hip/hip_runtime.h — stands in for the HIP runtime header when a kernel file is compiled for the HOST
// (tools/analyser_series_emulate.cpp): kernels become plain functions, a launch becomes a loop over the blocks.  A kernel with
// barriers runs as ONE thread per block (every `for (i = tid; i < n; i += nt)` loop is then the whole loop and a barrier a no-op);
// kernels without barriers run thread by thread with the launch's block size (emu_one_thread = false).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
using std::isfinite;
using std::isnan;
#define __device__
#define __global__
#define __shared__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __syncthreads() ((void)0)
struct dim3 {
  unsigned x, y, z;
  dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {}
};
static dim3 threadIdx(0, 0, 0), blockIdx(0, 0, 0), blockDim(1, 1, 1), gridDim(1, 1, 1);
static inline unsigned __brev(unsigned v) {
  unsigned r = 0;
  for (int i = 0; i < 32; i++) r |= ((v >> i) & 1u) << (31 - i);
  return r;
}
typedef void* hipStream_t;
static bool emu_one_thread = true;
static size_t emu_lds_bytes = 0;  // dynamic LDS the last launch asked for
#define hipLaunchKernelGGL(k, grid, block, lds, stream, ...)                                  \
  do {                                                                                        \
    const dim3 g_ = (grid), b_ = (block);                                                     \
    gridDim = g_;                                                                             \
    blockDim = emu_one_thread ? dim3(1) : b_;                                                 \
    emu_lds_bytes = (lds);                                                                    \
    for (unsigned bx_ = 0; bx_ < g_.x; bx_++)                                                 \
      for (unsigned tx_ = 0; tx_ < blockDim.x; tx_++) {                                       \
        blockIdx = dim3(bx_, 0, 0);                                                           \
        threadIdx = dim3(tx_, 0, 0);                                                          \
        k(__VA_ARGS__);                                                                       \
      }                                                                                       \
    threadIdx = dim3(0, 0, 0);                                                                \
  } while (0)
