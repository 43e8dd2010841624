// waa_conv_mirror.hpp — where the mirror bin N - k of a spectrum lives, in the two position orders the ConvolverNode's
// transforms store their spectra in (waa_conv_inst.hip: the product for per-instance impulse responses needs Z[k] and Z[N - k]).
//
//   CONV_ORDER_BREV  fft_dif_padded / conv_fft_pipe_kernel (waa_conv.hip): radix-4 decimation in frequency whose butterflies put
//                    output r of a stage into slot (0, 2, 1, 3)[r] — two radix-2 steps each — so position p holds bin
//                    bitreverse(p) over log2 N bits.
//   CONV_ORDER_FFT3  the three-pass transforms (waa_fft3.hpp, N = 16384): position p = k3 * 1024 + k1 * 32 + k2 holds bin
//                    k1 + 32 * k2 + 1024 * k3   (k1, k2 < 32, k3 < 16).
//
// Both maps are involutions with the fixed points bin 0 and bin N / 2.  What a 256-position workgroup of the product sees:
// bit-reversed order — the low bits of p are the HIGH bits of the bin, so the mirrors of 256 consecutive positions are 256
// consecutive positions in reverse (the two blocks whose low bin bits are 0 or N / 512 mirror into themselves); fft3 order —
// k2 runs fastest, the mirrors of a 32-position run are a 32-position run in reverse (256 B segments either way).
//
// Also compiled for the HOST (tests/test_convolver_per_instance.py, clang++): plain integer arithmetic.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define WAA_MIRROR_FN __host__ __device__ __forceinline__
#else
#define WAA_MIRROR_FN inline
#endif

namespace waa {

enum : int32_t { CONV_ORDER_BREV = 0, CONV_ORDER_FFT3 = 1 };

// the low `bits` bits of v in reverse order
WAA_MIRROR_FN uint32_t conv_bitrev(uint32_t v, int bits) {
  v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
  v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
  v = ((v >> 4) & 0x0f0f0f0fu) | ((v & 0x0f0f0f0fu) << 4);
  v = ((v >> 8) & 0x00ff00ffu) | ((v & 0x00ff00ffu) << 8);
  v = (v >> 16) | (v << 16);
  return v >> (32 - bits);
}
// bit-reversed order, N = 2^log2n: position of bin (N - bin(p)) mod N
WAA_MIRROR_FN uint32_t conv_mirror_brev(uint32_t p, int log2n) {
  const uint32_t mask = (1u << log2n) - 1u;
  return conv_bitrev((0u - conv_bitrev(p, log2n)) & mask, log2n);
}
// fft3 order, N = 16384
WAA_MIRROR_FN uint32_t conv_fft3_bin(uint32_t p) { return ((p >> 5) & 31u) + 32u * (p & 31u) + 1024u * (p >> 10); }
WAA_MIRROR_FN uint32_t conv_fft3_pos(uint32_t bin) { return (bin >> 10) * 1024u + (bin & 31u) * 32u + ((bin >> 5) & 31u); }
WAA_MIRROR_FN uint32_t conv_mirror_fft3(uint32_t p) { return conv_fft3_pos((16384u - conv_fft3_bin(p)) & 16383u); }

WAA_MIRROR_FN uint32_t conv_mirror(uint32_t p, int32_t order, int log2n) {
  return order == CONV_ORDER_FFT3 ? conv_mirror_fft3(p) : conv_mirror_brev(p, log2n);
}

}  // namespace waa
