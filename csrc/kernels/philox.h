// Counter-based dropout masks: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3",
// SC'11; the Random123 constants).  The mask of element e of a contiguous tensor is a pure function of
// (key, e), so a backward pass regenerates it instead of reading a stored one:
//   group g = e >> 3, counter (g & 0xffffffff, g >> 32, 0, 0), key (k0, k1) = (low, high) word of an int64 the
//   kernel reads from device memory; one call yields w0..w3 for the 8 elements of the group (one 16-byte bf16
//   vector); element j = e & 7 draws u = (w[j >> 1] >> (16 * (j & 1))) & 0xffff and is kept iff u >= thr.
// The same definition is implemented by ops/dropout.py's torch fallback and by tests/dropout_ref.py.
#pragma once
#include "common.h"

namespace pdt {
namespace philox {

struct Words {
  uint32_t w[4];
};

__host__ __device__ __forceinline__ uint32_t mulhi32(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
#endif
}

__host__ __device__ __forceinline__ Words philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                                         uint32_t k0, uint32_t k1) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = mulhi32(M0, c0), lo0 = M0 * c0;
    const uint32_t hi1 = mulhi32(M1, c2), lo1 = M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += W0;
    k1 += W1;
  }
  return Words{{c0, c1, c2, c3}};
}

// the four words that serve elements [8 g, 8 g + 8)
__host__ __device__ __forceinline__ Words group_words(uint64_t g, uint32_t k0, uint32_t k1) {
  return philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), 0u, 0u, k0, k1);
}

// the 16-bit draw of element j (0..7) of a group
__host__ __device__ __forceinline__ uint32_t draw16(const Words& w, int j) {
  return (w.w[j >> 1] >> (16 * (j & 1))) & 0xffffu;
}

// bit j set = element j of group g is kept.  Callers select on the bit (never multiply by 0): a dropped element
// is exactly 0 even where the input is inf / NaN, and a dropped residual leaves the stream's bits alone.
__host__ __device__ __forceinline__ uint32_t group_keep(uint64_t g, uint32_t k0, uint32_t k1, uint32_t thr) {
  const Words w = group_words(g, k0, k1);
  uint32_t m = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) m |= (draw16(w, j) >= thr ? 1u : 0u) << j;
  return m;
}

}  // namespace philox
}  // namespace pdt
