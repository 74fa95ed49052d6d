// What the files of HBM-bound kernels share (stats.hip, layernorm.hip, conv0.hip, encoder_ops.hip, small_ops.hip): wave64 shuffle
// reductions, typed loads / stores, the pair-row cut of the split-operand modes, and two launch helpers.  The kernels are wave64 designs:
// one wavefront per row where a row reduction is needed (shuffle reductions, no LDS), 16-byte accesses where the layout allows.
// Also here, for gemm_ring.h and attention_core.h, which both include this file: the LDS-DMA pointer types and lds_base.
#pragma once
#include "common.h"

namespace svt {
namespace {

template <typename V>
__device__ __forceinline__ V wave_sum(V v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// LDS-DMA (the GEMM ring of gemm_ring.h, the K / V stages of attention_core.h): the builtin's pointer types, and the LDS byte address
// of a __shared__ array as the asm forms take it in m0
typedef const void __attribute__((address_space(1)))* gptr_t;
typedef void __attribute__((address_space(3)))* lptr_t;
__device__ __forceinline__ unsigned lds_base(uint4* lds) { return __builtin_amdgcn_readfirstlane((unsigned)(size_t)(lptr_t)lds); }

template <typename T> __device__ __forceinline__ float ld(const T* p, long i);
template <> __device__ __forceinline__ float ld<float>(const float* p, long i) { return p[i]; }
template <> __device__ __forceinline__ float ld<bf16_t>(const bf16_t* p, long i) { return (float)p[i]; }
template <typename T> __device__ __forceinline__ void st(T* p, long i, float v);
template <> __device__ __forceinline__ void st<float>(float* p, long i, float v) { p[i] = v; }
template <> __device__ __forceinline__ void st<bf16_t>(bf16_t* p, long i, float v) { p[i] = (bf16_t)v; }

// ---- "pair rows" of the split-operand modes (GemmArgs::a_pairs): every 32 consecutive elements of a row are stored as
// [32 hi pieces | 32 lo pieces] (16-bit, IEEE half for kind 3 / bf16 for kind 2) in the 128 bytes of the fp32 slab they replace, so
// element offsets are those of the fp32 tensor.  PK = 0: no pair output, 2 = bf16 pieces, 3 = fp16 pieces (= svt_precision).
template <int PK> __device__ __forceinline__ void cut_piece(float x, unsigned short& hi, unsigned short& lo) {
  if constexpr (PK == 3) {
    const _Float16 a = (_Float16)x, b = (_Float16)(x - (float)a);
    hi = __builtin_bit_cast(unsigned short, a); lo = __builtin_bit_cast(unsigned short, b);
  } else {
    const __bf16 a = (__bf16)x, b = (__bf16)(x - (float)a);
    hi = __builtin_bit_cast(unsigned short, a); lo = __builtin_bit_cast(unsigned short, b);
  }
}
// N (4 or 8) consecutive elements starting at element index e (a multiple of N) of a pair-row tensor whose fp32 image starts at `base`
template <int PK, int N> __device__ __forceinline__ void store_pairs(void* base, int64_t e, const float (&v)[N]) {
  static_assert(N == 4 || N == 8, "pieces of 4 or 8 elements");
  unsigned short h[N], l[N];
#pragma unroll
  for (int i = 0; i < N; ++i) cut_piece<PK>(v[i], h[i], l[i]);
  char* d = (char*)base + (e >> 5) * 128 + (e & 31) * 2;
  if constexpr (N == 8) {
    *(uint4*)d = uint4{(unsigned)h[0] | ((unsigned)h[1] << 16), (unsigned)h[2] | ((unsigned)h[3] << 16), (unsigned)h[4] | ((unsigned)h[5] << 16), (unsigned)h[6] | ((unsigned)h[7] << 16)};
    *(uint4*)(d + 64) = uint4{(unsigned)l[0] | ((unsigned)l[1] << 16), (unsigned)l[2] | ((unsigned)l[3] << 16), (unsigned)l[4] | ((unsigned)l[5] << 16), (unsigned)l[6] | ((unsigned)l[7] << 16)};
  } else {
    *(uint2*)d = uint2{(unsigned)h[0] | ((unsigned)h[1] << 16), (unsigned)h[2] | ((unsigned)h[3] << 16)};
    *(uint2*)(d + 64) = uint2{(unsigned)l[0] | ((unsigned)l[1] << 16), (unsigned)l[2] | ((unsigned)l[3] << 16)};
  }
}

// conv layer 0: one input channel, 10 taps; the window moments behind its GroupNorm statistics (stats.hip): 10 first + 55 second
constexpr int K0 = 10;
constexpr int NWM = K0 + K0 * (K0 + 1) / 2;  // 65

inline int grid_for(int64_t n, int block = 256, int cap = 8192) {
  int64_t g = (n + block - 1) / block;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}
// no pointer has a bit of `mask` set (15: 16-byte accesses); a null pointer passes, so optional buffers can be listed
template <class... P> inline bool aligned(unsigned mask, P... p) { return !((... | (uintptr_t)p) & mask); }

}  // namespace
}  // namespace svt
