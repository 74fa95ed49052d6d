// Fused self/cross attention for gfx950 (16-bit operands, fp32 softmax state): softmax(scale * Q K^T) V
// without materialising the (T x T) scores.  No mask (the reference passes none); only
// the key tail of the last tile is masked.  T is arbitrary (T = 499 for 10 s clips), head_dim 64
// (wav2vec2/HuBERT) or 128 (RCA fusion).
//
// Mapping (wave64, v_mfma_f32_32x32x16_bf16):
//   * block = 4 waves = 128 queries of one (clip, head), or 8 waves = 256 queries when the launch has enough workgroups
//     (half the K / V traffic per query); each wave owns 32 queries for the whole sweep.
//   * K and V tiles of 64 keys are moved global -> LDS by LDS-DMA (no staging registers, no ds_write) into a row-major
//     image with an XOR swizzle of the 16-byte chunks, applied on the SOURCE address (8 consecutive lanes fetch one
//     128-byte row: one request per line); two stages, the next tile is in flight during the current tile's MFMAs,
//     one barrier per tile.
//   * S^T = K Q^T is computed with keys on the MFMA rows, so a lane holds 16 keys x 1 query per 32-key
//     block: the row max / row sum are in-register reductions plus ONE cross-lane exchange
//     (lane ^ 32).  The S accumulator, converted pairwise to bf16, is directly the B operand of
//     O^T += V^T P^T (k order permuted consistently on the V side) — P never touches LDS.
//   * V is read TRANSPOSED out of its row-major LDS tile by ds_read_b64_tr_b16 (4 keys x 16 d blocks delivered
//     column-major): the 4-key runs of the permuted k order are exactly two such blocks per operand, so no
//     transposed copy of V ever exists in memory.
//   * softmax: scale folded into the exponent FMA, running max raised only when a row grows by > 2^8 (deferred
//     rescale), MFMA accumulators kept in VGPRs (-mllvm -amdgpu-mfma-vgpr-form, see Makefile).
//
// This header is what the four kernels of the family share (attention_bf16.hip: flash_attn_kernel, flash_attn_stag_kernel on 16-bit
// operands; attention_x3.hip: flash_attn_x3_kernel, flash_attn_x3_stag_kernel on (hi, lo) planes): the per-lane address maps (query row,
// LDS-DMA source, transposing V reads, the staggered kernels' block map), and the steps of one tile -- products, softmax head, P -- and
// the epilogues, each defined once.  What differs between the kernels stays in the kernel files: the barrier and stage schedule (lockstep
// with two stages, or two wave groups half a tile apart with three) and the number of planes per tile.
//
// Most of it is SVT_ATTN_* macros, not functions: the code of every kernel was held identical across this sharing, and hipcc compiles
// a kernel differently as soon as a step that takes the lane index or the accumulators reaches it through a __forceinline__ function
// (the callee is simplified on its own before it is inlined -- without the range of `lane`, for one -- and the scheduler's ties fall
// differently; gemm_ring.h records the same for lds_unit).  Tried per step, in both builds, before settling on text: arrays by
// reference and by value, results returned by value or in a struct, the lane index passed in or taken from threadIdx inside, the
// tail-mask branch left at the call site.  The macros name the kernel's own variables; each says which.  Functions where the code
// stayed the same: attn_block_map, x3_mma, and cut_piece / lds_base of device_util.h.
#pragma once
#include "device_util.h"   // gptr_t, lptr_t, lds_base, cut_piece<PK>

namespace svt {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) s16x4* lds_s16x4_t;

// The staggered kernels issue their LDS-DMA from inline asm (the compiler tracks the DMA it emits for the builtin and guards later LDS
// reads it cannot prove distinct from the destination with s_waitcnt vmcnt(0) -- there the late group's V reads right behind its
// requests); the explicit vmcnt(0) in front of every barrier is the only wait on it.
__device__ __forceinline__ void attn_dma16(const void* gsrc, unsigned lds_byte_addr) {
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(gsrc), "s"(lds_byte_addr) : "memory");
}

// Split-operand kernels: one 32 x 32 x 16 MFMA on 16-bit pieces (F16: IEEE half, else bf16); A as it comes out of LDS
template <bool F16> struct X3T;
template <> struct X3T<false> { typedef real_bf16x8 v8; };
template <> struct X3T<true> { typedef _Float16 v8 __attribute__((ext_vector_type(8))); };
template <bool F16, typename A>
__device__ __forceinline__ f32x16 x3_mma(const A& a, const typename X3T<F16>::v8& b, const f32x16& c) {
  if constexpr (F16) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(typename X3T<true>::v8, a), b, c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(real_bf16x8, a), b, c, 0, 0, 0);
}

// ---- per-lane address maps: on the kernel's lane, wave, T, q0 and its constants DH, DB, CPR, RB ----

// Declares QP, the row of Q (at Qb, pitch ldq) that a lane's fragments (B operand of S^T = K Q^T) come from: lane holds
// Q[q0 + (lane&31)][ks*16 + 8*(lane>>5) .. +7]; rows past the end read row T - 1 (their results are never stored)
#define SVT_ATTN_Q_ROW(QP)                                                                                                    \
  int q = q0 + (lane & 31);                                                                                                   \
  if (q > T - 1) q = T - 1;                                                                                                   \
  const auto* QP = Qb + (long)q * ldq + 8 * (lane >> 5);

// LDS-DMA source mapping: a wave instruction moves 64 x 16 B = 1 KB = 64 / CPR whole rows; PIECE is which KB of the tile.  Lane (row r =
// lane / CPR, slot = lane % CPR) fetches chunk slot ^ g(key) of its row, so the linear LDS image holds chunk c of a key at slot
// c ^ g(key) -- the same swizzled row-major layout the MFMA operand reads expect (K: g = (key>>1)&7 for 128-byte rows, key&15 for
// 256-byte rows; V: (key>>1 & 1) << 2, resp. (key & 3) << 2).  Sets DKEY: key within the tile; KCH / VCH: element offset in the K / V row.
#define SVT_ATTN_DMA_SRC(PIECE, DKEY, KCH, VCH)                                                                               \
  {                                                                                                                           \
    const int kk = (PIECE) * (64 / CPR) + lane / CPR;                                                                         \
    const int slot = lane % CPR;                                                                                              \
    const int g = (DH == 64) ? ((kk >> 1) & 7) : (kk & 15);                                                                   \
    const int sw = (DH == 64) ? (((kk >> 1) & 1) << 2) : ((kk & 3) << 2);                                                     \
    DKEY = kk;                                                                                                                \
    KCH = (slot ^ g) * 8;                                                                                                     \
    VCH = (slot ^ sw) * 8;                                                                                                    \
  }

// Fills vbase[DB], the transposing-read addresses into the V tile at VTILE (stage 0): lane 16g+4q+p supplies row (key) q, columns
// 4p..4p+3 of its group's 4 x 16 block
#define SVT_ATTN_VBASE(VTILE)                                                                                                 \
  {                                                                                                                           \
    const int g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;                                                              \
    const int key0 = 4 * (g >> 1) + q;                                                                                        \
    const int sw = (DH == 64) ? (((q >> 1) & 1) << 2) : (q << 2);                                                             \
    _Pragma("unroll") for (int db = 0; db < DB; ++db) {                                                                       \
      const int chunk = db * 4 + 2 * (g & 1) + (pp >> 1);                                                                     \
      vbase[db] = (const char*)(VTILE) + key0 * RB + ((chunk ^ sw) * 16) + 8 * (pp & 1);                                      \
    }                                                                                                                         \
  }

// Staggered kernels: 1-D grid of NQB x (B * H) workgroups, mapped so that the NQB query blocks of one (clip, head) are blocks L, L + 8,
// L + 16, ...: consecutive blocks are dealt round-robin over the 8 XCDs, so those land on ONE XCD and the K / V of the head are fetched
// into one L2 instead of NQB (speed only: profiles/r04_attention_pmc.txt, 147 MB of HBM-side traffic per launch against 98 MB algorithmic)
__device__ __forceinline__ void attn_block_map(int nqb, int& bh, int& qblk) {
  const int L = blockIdx.x, BH = (int)gridDim.x / nqb;
  const int full = (BH / 8) * 8 * nqb;   // blocks covered by whole groups of 8 heads
  if (L < full) { bh = (L & 7) + 8 * (L / (8 * nqb)); qblk = (L >> 3) % nqb; }
  else { const int r = L - full; bh = (BH / 8) * 8 + r / nqb; qblk = r % nqb; }
}

// ---- the steps of one tile ----
// Names every step uses: f32x16 s[2] (scores of the tile's two 32-key blocks), o[DB], float m, l (running max, row sum), int hh = lane >>
// 5, kl = lane & 31, kg (swizzle of key kl), T, and the constants KSD, DB, CPR, RB, TILE16, STAGE_BYTES of the kernel.

// s = K Q^T of the tile at KF; uses qf[KSD]
#define SVT_ATTN_S(KF)                                                                                                       \
  {                                                                                                                           \
    const uint4* Kf = (KF);                                                                                                   \
    _Pragma("unroll") for (int kb = 0; kb < 2; ++kb) {                                                                        \
      _Pragma("unroll") for (int r = 0; r < 16; ++r) s[kb][r] = 0.f;                                                          \
      _Pragma("unroll") for (int ks = 0; ks < KSD; ++ks)                                                                      \
        s[kb] = SVT_MFMA_32x32x16(__builtin_bit_cast(bf16x8, Kf[(kb * 32 + kl) * CPR + ((2 * ks + hh) ^ kg)]), qf[ks], s[kb]); \
    }                                                                                                                         \
  }
// the same on (hi, lo) planes, K hi at KH and K lo a tile behind it: s = Kl Qh^T + Kh Ql^T + Kh Qh^T; uses qh[KSD], ql[KSD]
#define SVT_ATTN_X3_S(KH)                                                                                                     \
  {                                                                                                                           \
    const uint4* Kh = (KH);                                                                                                   \
    const uint4* Kl = Kh + TILE16;                                                                                            \
    _Pragma("unroll") for (int kb = 0; kb < 2; ++kb) {                                                                        \
      _Pragma("unroll") for (int r = 0; r < 16; ++r) s[kb][r] = 0.f;                                                          \
      _Pragma("unroll") for (int ks = 0; ks < KSD; ++ks) {                                                                    \
        const int idx = (kb * 32 + kl) * CPR + ((2 * ks + hh) ^ kg);                                                          \
        const uint4 kh = Kh[idx], klo = Kl[idx];                                                                              \
        s[kb] = x3_mma<F16>(klo, qh[ks], s[kb]);                                                                              \
        s[kb] = x3_mma<F16>(kh, ql[ks], s[kb]);                                                                               \
        s[kb] = x3_mma<F16>(kh, qh[ks], s[kb]);                                                                               \
      }                                                                                                                       \
    }                                                                                                                         \
  }

// Softmax head, in the scaled log2 domain (p = exp2(s * CS - m) follows in the kernel): keys >= T are masked in the last tile only, the
// row max is taken on the raw scores, and the running max is only raised (o and l rescaled) when some row of the wave grew by more than
// 2^8 (deferred rescale: P stays <= 256, exact in fp32 and safe in bf16)
#define SVT_ATTN_SOFTMAX_HEAD(TILE, CS)                                                                                       \
  {                                                                                                                           \
    if (__builtin_expect((TILE) * 64 + 64 > T, 0)) {  /* wave-uniform, last tile only */                                      \
      const int kbase = (TILE) * 64 + 4 * hh;                                                                                 \
      _Pragma("unroll") for (int kb = 0; kb < 2; ++kb)                                                                        \
        _Pragma("unroll") for (int r = 0; r < 16; ++r) {                                                                      \
          const int key = kbase + kb * 32 + (r & 3) + 8 * (r >> 2);                                                           \
          asm volatile("" : "+v"(s[kb][r]));  /* keep the masking inside this (rare) branch instead of 32 selects per tile */ \
          if (key >= T) s[kb][r] = -3e38f;                                                                                    \
        }                                                                                                                     \
    }                                                                                                                         \
    float mx = fmaxf(s[0][0], s[1][0]);                                                                                       \
    _Pragma("unroll") for (int r = 1; r < 16; ++r) mx = fmaxf(fmaxf(mx, s[0][r]), s[1][r]);  /* v_max3_f32 */                 \
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64)) * (CS);                                                                            \
    if (!__all(mx - m <= 8.0f)) {                                                                                             \
      const float mnew = fmaxf(m, mx);                                                                                        \
      const float alpha = __builtin_amdgcn_exp2f(m - mnew);                                                                   \
      l *= alpha;                                                                                                             \
      m = mnew;                                                                                                               \
      _Pragma("unroll") for (int i = 0; i < DB; ++i)                                                                          \
        _Pragma("unroll") for (int r = 0; r < 16; ++r) o[i][r] *= alpha;                                                      \
    }                                                                                                                         \
  }
// P (bf16) fragments straight from the S accumulators, which hold P by now: k-step ss of key block kb = regs 8ss..8ss+7; fills pf[2][2].
// (How P and its row sum are formed stays in the two kernels: flash_attn_kernel works on packed pairs, flash_attn_stag_kernel on two
// scalar chains -- different orders of the sum.)
#define SVT_ATTN_PF                                                                                                           \
  _Pragma("unroll") for (int kb = 0; kb < 2; ++kb)                                                                            \
    _Pragma("unroll") for (int ss = 0; ss < 2; ++ss)                                                                          \
      _Pragma("unroll") for (int j = 0; j < 8; ++j) pf[kb][ss][j] = (bf16_t)s[kb][ss * 8 + j];
// Split kernels: P = exp2(s c - m) cut into (hi, lo) pieces; the row sum is taken over the fp32 values; fills pfh[2][2], pfl[2][2]
#define SVT_ATTN_X3_P                                                                                                         \
  {                                                                                                                           \
    float sum = 0.f;                                                                                                          \
    unsigned short ph[2][16], pl[2][16];                                                                                      \
    _Pragma("unroll") for (int kb = 0; kb < 2; ++kb)                                                                          \
      _Pragma("unroll") for (int r = 0; r < 16; ++r) {                                                                        \
        const float pv = __builtin_amdgcn_exp2f(fmaf(s[kb][r], c, -m));                                                       \
        sum += pv;                                                                                                            \
        cut_piece<F16 ? 3 : 2>(pv, ph[kb][r], pl[kb][r]);                                                                     \
      }                                                                                                                       \
    sum += __shfl_xor(sum, 32, 64);                                                                                           \
    l += sum;                                                                                                                 \
    _Pragma("unroll") for (int kb = 0; kb < 2; ++kb)                                                                          \
      _Pragma("unroll") for (int ss = 0; ss < 2; ++ss) {                                                                      \
        s16x8 th, tl;                                                                                                         \
        _Pragma("unroll") for (int j = 0; j < 8; ++j) { th[j] = (short)ph[kb][ss * 8 + j]; tl[j] = (short)pl[kb][ss * 8 + j]; } \
        pfh[kb][ss] = __builtin_bit_cast(v8, th);                                                                             \
        pfl[kb][ss] = __builtin_bit_cast(v8, tl);                                                                             \
      }                                                                                                                       \
  }

// o += V P of the tile in stage ST.  A operand of O^T += V^T P^T straight from the row-major V tile: two ds_read_b64_tr_b16 (4 keys x
// 16 d blocks, delivered column-major) give this lane V[key][d] for its d and the permuted k-slots {16s+4h+0..3, 16s+8+4h+0..3}; uses
// vbase[DB], pf
#define SVT_ATTN_PV(ST)                                                                                                       \
  {                                                                                                                           \
    _Pragma("unroll") for (int db = 0; db < DB; ++db)                                                                         \
      _Pragma("unroll") for (int kb = 0; kb < 2; ++kb)                                                                        \
        _Pragma("unroll") for (int ss = 0; ss < 2; ++ss) {                                                                    \
          const char* vp = vbase[db] + (ST) * STAGE_BYTES + (kb * 32 + ss * 16) * RB;                                         \
          const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t)(vp));                                        \
          const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t)(vp + 8 * RB));                               \
          const s16x8 vv = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);                                           \
          o[db] = SVT_MFMA_32x32x16(__builtin_bit_cast(bf16x8, vv), pf[kb][ss], o[db]);                                       \
        }                                                                                                                     \
  }
// the same on planes, V lo PLANE_BYTES behind V hi: o += Vl Ph + Vh Pl + Vh Ph; uses vbase[DB], pfh, pfl
#define SVT_ATTN_X3_PV(ST)                                                                                                    \
  {                                                                                                                           \
    _Pragma("unroll") for (int db = 0; db < DB; ++db)                                                                         \
      _Pragma("unroll") for (int kb = 0; kb < 2; ++kb)                                                                        \
        _Pragma("unroll") for (int ss = 0; ss < 2; ++ss) {                                                                    \
          const char* vp = vbase[db] + (ST) * STAGE_BYTES + (kb * 32 + ss * 16) * RB;                                         \
          const s16x4 hlo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t)(vp));                                       \
          const s16x4 hhi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t)(vp + 8 * RB));                              \
          const s16x4 llo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t)(vp + PLANE_BYTES));                         \
          const s16x4 lhi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t)(vp + PLANE_BYTES + 8 * RB));                \
          const s16x8 vh = __builtin_shufflevector(hlo, hhi, 0, 1, 2, 3, 4, 5, 6, 7);                                         \
          const s16x8 vl = __builtin_shufflevector(llo, lhi, 0, 1, 2, 3, 4, 5, 6, 7);                                         \
          o[db] = x3_mma<F16>(vl, pfh[kb][ss], o[db]);                                                                        \
          o[db] = x3_mma<F16>(vh, pfl[kb][ss], o[db]);                                                                        \
          o[db] = x3_mma<F16>(vh, pfh[kb][ss], o[db]);                                                                        \
        }                                                                                                                     \
  }

// ---- training-mode dropout on the probabilities (attention_drop.hip; the mask function: philox.h, which the kernel file includes) ----
// Element (b, h, i, j) of the (B, H, T, T) probabilities has the LOGICAL index e = E0 + ((b*H + h)*T + i)*T + j and is kept iff word e & 3
// of its four-element group e >> 2 reaches the threshold.  A tile's 64 keys of one query are 64 consecutive elements: 16 groups when the
// row's first element is a multiple of 4, else 17.  Lanes l and l ^ 32 hold the same query (runs of four keys at 8k and 8k + 4), so the
// pair splits the groups -- lanes 0-31 compute groups 0..7 of the tile, lanes 32-63 groups 8..16 -- turns each word into one keep bit and
// exchanges the bits, not the words: two half exchanges (v_permlane32_swap: groups 0..15, then group 16) per tile give both lanes the
// row's 68 bits, of which a lane reads the 60 from its first key on.  Nine Philox
// calls per lane and tile at any alignment (a naive lane needs two calls per run: 16), eight when every row of the wave is aligned.
//
// Declares the lane's constants: drow = index of (b, h, i = q0 + (lane & 31), key 0); dg0 = the first group this lane computes in tile 0;
// dsh = the bit of the lane's first key in the row's bits (alignment of the row + 4 for the upper lane); dninth = some row of the wave
// is unaligned (wave-uniform).  Rows past T get indices of their own that nobody reads.
#define SVT_ATTN_DROP_ROW(E0)                                                                                                 \
  const uint64_t drow = (E0) + ((uint64_t)((long)b * H + h) * (uint64_t)T + (uint64_t)(q0 + (lane & 31))) * (uint64_t)T;      \
  const uint64_t dg0 = (drow >> 2) + (uint64_t)(8 * hh);                                                                      \
  const unsigned dsh = (unsigned)(drow & 3) + 4u * (unsigned)hh;                                                              \
  const bool dninth = __any((int)(drow & 3) != 0);

// Zeroes the dropped probabilities of tile TILE in s (after the row sum took them, before P is cut to 16 bits); D: the DropSpec.
// Bit n of (dw0, dw1) is the keep bit of the lane's key kb*32 + 8*(r>>2) + (r&3) with n = that number: the key map of SVT_ATTN_SOFTMAX_HEAD
// less the lane's 4*hh, which dsh holds.  Keys >= T have p = 0 already; their bits belong to other rows and change nothing.
#define SVT_ATTN_DROP(TILE, D)                                                                                                \
  {                                                                                                                           \
    const uint64_t dg = dg0 + (uint64_t)(TILE) * 16;                                                                          \
    unsigned mlo = 0, mhi = 0;                                                                                                \
    _Pragma("unroll") for (int cc = 0; cc < 8; ++cc) {                                                                        \
      const Philox4 pw = drop_words((D), dg + cc);                                                                            \
      _Pragma("unroll") for (int k = 0; k < 4; ++k) mlo |= (unsigned)(pw.w[k] >= (D).thr) << (4 * cc + k);                    \
    }                                                                                                                         \
    if (dninth) {  /* wave-uniform: group 16 of the row, which an unaligned row's last keys reach (lanes 32-63; 0-31: unread) */ \
      const Philox4 pw = drop_words((D), dg + 8);                                                                             \
      _Pragma("unroll") for (int k = 0; k < 4; ++k) mhi |= (unsigned)(pw.w[k] >= (D).thr) << k;                               \
    }                                                                                                                         \
    /* swap(x, x): element 0 = the lower lane's x in both lanes of a pair, element 1 = the upper lane's */                    \
    const auto x0 = __builtin_amdgcn_permlane32_swap(mlo, mlo, false, false);                                                 \
    const auto x1 = __builtin_amdgcn_permlane32_swap(mhi, mhi, false, false);                                                 \
    const unsigned dw0 = __builtin_amdgcn_alignbit(x0[1], x0[0], dsh);   /* bits dsh .. dsh + 31 of the row's 68 */           \
    const unsigned dw1 = __builtin_amdgcn_alignbit(x1[1], x0[1], dsh);   /* bits dsh + 32 .. dsh + 63 */                      \
    _Pragma("unroll") for (int kb = 0; kb < 2; ++kb)                                                                          \
      _Pragma("unroll") for (int r = 0; r < 16; ++r) {                                                                        \
        const int bit = 8 * (r >> 2) + (r & 3);                                                                               \
        /* v_bfe_i32: all ones or zero (hipcc turns the C form and the sbfe builtin into and + compare + select); the pair in ONE asm   \
           so that no 32 extracted masks stay live beside s: apart, hipcc hoists them all and the kernel takes 162 VGPRs for 128 */   \
        const float pv = s[kb][r];   /* a copy: __builtin_bit_cast on the vector element itself reads element 0 (hipcc 7.2) */ \
        float pk;                                                                                                             \
        asm("v_bfe_i32 %0, %1, %2, 1\n\tv_and_b32 %0, %0, %3" : "=&v"(pk) : "v"(kb ? dw1 : dw0), "n"(bit), "v"(pv));           \
        s[kb][r] = pk;                                                                                                        \
      }                                                                                                                       \
  }

// ---- epilogues: O[q][d] = o * inv (inv = 1 / l) to the lane's row `op`; lane (q = lane&31, hh) holds d = db*32 + (r&3) + 8*(r>>2) + 4*hh

// 16-bit output.  A lane holds 4 consecutive d per (db, g) and its partner lane ^ 32 (same query) the other 4 of the same 8: a half
// exchange (v_permlane32_swap) per dword gives lanes 0-31 the 8 values of group g and lanes 32-63 those of group g + 1 -- one 16-byte
// store per pair of groups instead of two 8-byte ones (the store tail of a row-per-lane epilogue is bound by store ISSUE, not bytes)
#define SVT_ATTN_STORE_O16                                                                                                    \
  _Pragma("unroll") for (int db = 0; db < DB; ++db)                                                                           \
    _Pragma("unroll") for (int g = 0; g < 4; g += 2) {                                                                        \
      unsigned w[2][2];   /* [group g / g + 1][dword] */                                                                      \
      _Pragma("unroll") for (int u = 0; u < 2; ++u) {                                                                         \
        bf16x4 v;                                                                                                             \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) v[j] = (bf16_t)(o[db][(g + u) * 4 + j] * inv);                          \
        const uint2 pk = __builtin_bit_cast(uint2, v);                                                                        \
        w[u][0] = pk.x; w[u][1] = pk.y;                                                                                       \
      }                                                                                                                       \
      _Pragma("unroll") for (int d2 = 0; d2 < 2; ++d2) {                                                                      \
        const auto r = __builtin_amdgcn_permlane32_swap(w[0][d2], w[1][d2], false, false);                                    \
        w[0][d2] = r[0]; w[1][d2] = r[1];                                                                                     \
      }                                                                                                                       \
      *(uint4*)(op + db * 32 + 8 * (g + hh)) = uint4{w[0][0], w[0][1], w[1][0], w[1][1]};                                     \
    }
// Split kernels, fp32 `op`; ends the kernel.  With o_pairs the output projection's operand as pair rows (gemm_x3q.hip): [32 hi | 32 lo]
// per 32 elements, in the bytes of the fp32 slab (ldo, o_bstride and h * DH are multiples of 32 elements: the launcher checks).  There
// a lane holds 4 consecutive d per (db, g) -- 8 bytes per plane -- and its partner lane ^ 32 the other 4 of the same 8: two half exchanges
// (v_permlane32_swap) per plane and pair of groups give lanes 0-31 the 8 pieces of group g and lanes 32-63 those of group g + 1, i.e. one
// 16-byte store per plane instead of two 8-byte ones (the 8-byte form cost 14 us of a 113 us launch: store issue)
#define SVT_ATTN_X3_STORE                                                                                                     \
  if (o_pairs) {                                                                                                              \
    char* pp = (char*)op;                                                                                                     \
    _Pragma("unroll") for (int db = 0; db < DB; ++db)                                                                         \
      _Pragma("unroll") for (int g = 0; g < 4; g += 2) {                                                                      \
        unsigned hx[2][2], lx[2][2];   /* [group g / g + 1][dword] */                                                         \
        _Pragma("unroll") for (int u = 0; u < 2; ++u) {                                                                       \
          unsigned short ph_[4], pl_[4];                                                                                      \
          _Pragma("unroll") for (int j = 0; j < 4; ++j) cut_piece<F16 ? 3 : 2>(o[db][(g + u) * 4 + j] * inv, ph_[j], pl_[j]); \
          hx[u][0] = (unsigned)ph_[0] | ((unsigned)ph_[1] << 16); hx[u][1] = (unsigned)ph_[2] | ((unsigned)ph_[3] << 16);     \
          lx[u][0] = (unsigned)pl_[0] | ((unsigned)pl_[1] << 16); lx[u][1] = (unsigned)pl_[2] | ((unsigned)pl_[3] << 16);     \
        }                                                                                                                     \
        _Pragma("unroll") for (int w = 0; w < 2; ++w) {                                                                       \
          const auto rh = __builtin_amdgcn_permlane32_swap(hx[0][w], hx[1][w], false, false);                                 \
          hx[0][w] = rh[0]; hx[1][w] = rh[1];                                                                                 \
          const auto rl = __builtin_amdgcn_permlane32_swap(lx[0][w], lx[1][w], false, false);                                 \
          lx[0][w] = rl[0]; lx[1][w] = rl[1];                                                                                 \
        }                                                                                                                     \
        char* d = pp + db * 128 + (8 * (g + hh)) * 2;                                                                         \
        *(uint4*)d = uint4{hx[0][0], hx[0][1], hx[1][0], hx[1][1]};                                                           \
        *(uint4*)(d + 64) = uint4{lx[0][0], lx[0][1], lx[1][0], lx[1][1]};                                                    \
      }                                                                                                                       \
    return;                                                                                                                   \
  }                                                                                                                           \
  _Pragma("unroll") for (int db = 0; db < DB; ++db)                                                                           \
    _Pragma("unroll") for (int g = 0; g < 4; ++g) {                                                                           \
      const float4 v = {o[db][g * 4] * inv, o[db][g * 4 + 1] * inv, o[db][g * 4 + 2] * inv, o[db][g * 4 + 3] * inv};          \
      *(float4*)(op + db * 32 + 8 * g + 4 * hh) = v;                                                                          \
    }

}  // namespace
}  // namespace svt
