// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants) and the
// dropout mask built on it (dropout.hip, include/svt_mi355.h "dropout"; tests/dropout_cases.py restates both in numpy).  Plain C++:
// the same text compiles for the host, where the generator's published known answers check it.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SVT_HD __host__ __device__ __forceinline__
#else
#define SVT_HD inline
#endif

namespace svt {

struct Philox4 { uint32_t w[4]; };

// ten rounds; the key is bumped by the Weyl constants between rounds (nine times)
SVT_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// One dropout site of one forward: element e (its LOGICAL index in the tensor) is kept iff
//     philox4x32_10(counter = (q_lo, q_hi, site | layer << 8, step), key = (seed_lo, seed_hi))[e & 3] >= thr,   q = e >> 2,
// thr = floor(p * 2^32); a kept value is multiplied by scale = float(1 / (1 - p)), a dropped one becomes +0
struct DropSpec {
  uint32_t thr = 0;
  float scale = 1.f;
  uint32_t seed_lo = 0, seed_hi = 0;
  uint32_t site_layer = 0;   // site | layer << 8
  uint32_t step = 0;
};

// the four words of the group q = e >> 2
SVT_HD Philox4 drop_words(const DropSpec& d, uint64_t q) {
  return philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), d.site_layer, d.step, d.seed_lo, d.seed_hi);
}

}  // namespace svt
