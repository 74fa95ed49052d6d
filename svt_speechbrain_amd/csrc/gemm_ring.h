// What the LDS-DMA contraction kernels share (gemm_pp8, gemm_pers, gemm_pps, gemm_p1w, gemm_x3s, gemm_x3p, gemm_x3q, gemm_p1x): the fixed
// parts of one pipeline.  What differs between them -- the slot schedule and the epilogue -- stays in the kernel files.  (gemm.hip, the
// register-staged kernel, takes apply_act and xcd_tile from here.)
//
// K is consumed in 128-byte slabs per row (64 16-bit elements, 32 fp32 values or one pair-row slab) that are moved global -> LDS by
// LDS-DMA (global_load_lds_dwordx4: no VGPR staging, no ds_write).  LDS is a ring of five 32 KiB slots holding alternating A / W units
// of successive K slabs (unit u: A_0 W_0 A_1 W_1 ..., in slot u % 5); three units are in flight while a slab is multiplied, retired
// by a counted s_waitcnt vmcnt across raw s_barriers.
//   * DMA source mapping: 8 consecutive lanes fetch the 8 16-byte chunks of one 128-byte row (one request per line for the texture
//     addresser; a lane-per-row mapping costs one request per lane and halves the fill rate), lane (row r, slot s) takes chunk s ^ r,
//     so the row-major LDS image is XOR-swizzled and the MFMA operand read of (row, chunk C) at slot C ^ row is a conflict-free
//     ds_read_b128.
//   * W rows are fetched in MFMA order, permuted (free with per-lane DMA source addresses) so that a lane ends up with consecutive
//     output columns of one row; every kernel has its own permutation, matched to its epilogue.
#pragma once
#include "device_util.h"   // gptr_t, lptr_t, lds_base; cut_piece<PK>: one fp32 value -> its (hi, lo) 16-bit pieces

namespace svt {
namespace {

typedef unsigned u32x4v __attribute__((ext_vector_type(4)));   // register image of a 16-byte fragment (an ext vector: usable as an asm operand)
typedef _Float16 f16x8v __attribute__((ext_vector_type(8)));

template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// one LDS-DMA instruction: 64 lanes x 16 bytes from sbase + voff (per lane) to LDS bytes [lds_addr, lds_addr + 1024).  Issued from
// asm in the `voffset + SGPR base` form: the compiler sees no LDS write and no VMEM load, so it never adds a vmcnt(0) of its own
__device__ __forceinline__ void dma_sv(unsigned voff, const void* sbase, unsigned lds_addr) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(lds_addr), "v"(voff), "s"(sbase) : "memory");
}
// LDS byte address (lds_base of the ring) of the 1 KiB piece (8 rows x 128 B) that DMA instruction i of a wave fills in a slot: the eight
// waves of a workgroup take the pieces of a unit round-robin.  (gemm_x3q, and the four-wave gemm_p1w / gemm_p1x with `wave + 4 * i`, keep
// this expression in a lambda of their own: with the function hipcc schedules those kernels differently.)
__device__ __forceinline__ unsigned lds_unit(unsigned lds0, int wave, int slot, int i) {
  return lds0 + (unsigned)(slot * 2048 + (wave + 8 * i) * 64) * 16u;
}

// split-operand modes: one 16 x 16 x 32 MFMA on 16-bit pieces (F16: IEEE half, else bf16)
template <bool F16> __device__ __forceinline__ f32x4 mma3(const u32x4v& a, const u32x4v& b, const f32x4& c) {
  if constexpr (F16) return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8v, a), __builtin_bit_cast(f16x8v, b), c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(real_bf16x8, a), __builtin_bit_cast(real_bf16x8, b), c, 0, 0, 0);
}
// eight fp32 values -> packed (hi, lo) 16-bit pieces
template <bool F16> __device__ __forceinline__ void cut8(const float (&v)[8], u32x4v& hi, u32x4v& lo) {
  if constexpr (F16) {
    f16x8v h, l;
#pragma unroll
    for (int j = 0; j < 8; ++j) { h[j] = (_Float16)v[j]; l[j] = (_Float16)(v[j] - (float)h[j]); }
    hi = __builtin_bit_cast(u32x4v, h);
    lo = __builtin_bit_cast(u32x4v, l);
  } else {
    real_bf16x8 h, l;
#pragma unroll
    for (int j = 0; j < 8; ++j) { h[j] = (__bf16)v[j]; l[j] = (__bf16)(v[j] - (float)h[j]); }
    hi = __builtin_bit_cast(u32x4v, h);
    lo = __builtin_bit_cast(u32x4v, l);
  }
}
// the same for 8 fp32 of one lane as they come out of LDS (two 16-byte chunks)
template <bool F16> __device__ __forceinline__ void cut8(const u32x4v& r0, const u32x4v& r1, u32x4v& hi, u32x4v& lo) {
  const f32x4 v0 = __builtin_bit_cast(f32x4, r0), v1 = __builtin_bit_cast(f32x4, r1);
  if constexpr (F16) {
    f16x8v h, l;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      h[j] = (_Float16)v0[j]; l[j] = (_Float16)(v0[j] - (float)h[j]);
      h[4 + j] = (_Float16)v1[j]; l[4 + j] = (_Float16)(v1[j] - (float)h[4 + j]);
    }
    hi = __builtin_bit_cast(u32x4v, h);
    lo = __builtin_bit_cast(u32x4v, l);
  } else {
    real_bf16x8 h, l;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      h[j] = (__bf16)v0[j]; l[j] = (__bf16)(v0[j] - (float)h[j]);
      h[4 + j] = (__bf16)v1[j]; l[4 + j] = (__bf16)(v1[j] - (float)h[4 + j]);
    }
    hi = __builtin_bit_cast(u32x4v, h);
    lo = __builtin_bit_cast(u32x4v, l);
  }
}

__device__ __forceinline__ float apply_act(float v, int act) {
  if (act == ACT_GELU) return gelu_erf(v);
  if (act == ACT_RELU) return v > 0.f ? v : 0.f;
  return v;
}

// byte offset of row m of A (GemmArgs: implicit-conv rows overlap) for elements of esz bytes
__device__ __forceinline__ long a_row_off(const GemmArgs& p, int m, int esz = 4) {
  return ((long)(m / p.a_rpb) * p.a_bstride + (long)(m % p.a_rpb) * p.a_rstride) * esz;
}

// One tile per workgroup: blocks b, b + 8, b + 16 ... run on one XCD (round-robin dispatch) and share its L2, so each XCD gets a
// contiguous range of the nblk logical tiles.  Returns the logical tile of block bid.
__device__ __forceinline__ int xcd_tile(int bid, int nblk) {
  const int xcd = bid & 7, q = nblk >> 3, r = nblk & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}
// Persistent kernels (a launch of nblk workgroups, a multiple of 8; workgroup b takes the logical tiles first, first + nblk, ...):
// blocks b and b + 8 share an XCD, so in every round an XCD works on nblk / 8 consecutive logical tiles (n fastest)
__device__ __forceinline__ int xcd_first_tile(int b, int nblk) {
  const int per = nblk >> 3;
  return (b & 7) * per + (b >> 3);
}

}  // namespace
}  // namespace svt
