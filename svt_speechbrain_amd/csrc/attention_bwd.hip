// Backward of the fused attention (16-bit operands, both library builds, head size 64), with the forward's position-defined dropout
// mask and no (B, H, T, T) tensor.  HF eager order, softmax -> dropout -> . V; keep_ij = the site-2 mask at element
// e0 + ((b H + h) T + i) T + j, s = float(1 / (1 - p)), c = scale log2 e:
//
//     P_ij  = exp2(c (q_i . k_j) - L_i)        L_i = m_i + log2 l_i  (row log-sum-exp, base 2, over ALL keys)
//     dV_j  = s sum_i keep_ij P_ij dO_i
//     dP_ij = s keep_ij (dO_i . v_j)           delta_i = dO_i . O_i
//     dS_ij = P_ij (dP_ij - delta_i)
//     dQ_i  = scale sum_j dS_ij k_j            dK_j = scale sum_i dS_ij q_i
//
// Three launches, no float atomics: every output element is summed by one lane in one order, so two calls give the same bytes.
//
//   a) attn_bwd_prep_kernel: L and delta, (B, H, T) fp32 each, into the workspace.  L from a sweep of S alone -- the forward's
//      S^T = K Q^T step and softmax head (SVT_ATTN_S, SVT_ATTN_SOFTMAX_HEAD) without V, P V or the mask; delta from the saved 16-bit O
//      and dO, one row per lane, 16-byte loads, fp32 sum.
//   b) attn_bwd_dq_kernel<DROP>: one workgroup per 128 queries of a (clip, head), sweeping key tiles of 64 -- the forward's lockstep
//      structure (LDS-DMA, two stages, one barrier per tile), one product wider: S^T = K Q^T and dP^T = V dO^T (q and dO fragments in
//      registers, K and V read as row operands, both in the K swizzle), P from L, the mask on dP (SVT_ATTN_DROP_ROW / SVT_ATTN_DROP as
//      they stand: the lane layout of S^T is the forward's), dS, and dQ^T += K^T dS^T with the dS accumulators cut to 16 bits as the B
//      operand and K read through the transposing LDS reads, as the forward's O^T += V^T P^T with K in V's place.  K is staged as TWO
//      images per tile, one in each swizzle (8 KB each; 24 KB per stage with V): no one swizzle was sought that serves both reads.
//   c) attn_bwd_dkv_kernel<DROP>: one workgroup per 128 keys (32 per wave, k and v fragments in registers), sweeping query tiles of
//      64.  S = Q K^T and dP = dO V^T are computed with QUERIES on the MFMA rows: dV and dK contract over queries, and an accumulator
//      can serve as an MFMA operand only along its register-resident index.  dV^T += dO^T P~ and dK^T += Q^T dS take the accumulators
//      as the B operand and read dO and Q transposed, so both tiles are staged in both swizzles (32 KB per stage).  L_i and delta_i of
//      the tile's 64 queries travel through LDS (4-byte LDS-DMA): every register of a lane belongs to another query.  Rows i >= T of
//      the last tile get the score -3e38, so P = 0 there and both P~ and dS are exactly zero (the DMA clamps their source row to
//      T - 1).  The mask: a lane holds one key and 32 queries per tile, 32 Philox calls taken directly; instead lane t of a wave
//      computes the keep bits of the tile's query t over the wave's 32 keys (8 or 9 four-word groups: 9 calls), writes them as one
//      word into a per-wave LDS bitmap, and every lane reads the words of its 32 queries (eight 16-byte reads) and takes its key's bit.
//
// Roundings: S and dP are fp32 MFMA sums of exact 16-bit products; L, delta, P and dS are fp32; P~ (dV) and dS (dQ, dK) are cut to the
// operand type once, as MFMA operands; the gradients are rounded once, at the store.  s multiplies dP in fp32 and the dV sum once.
#include "api.h"   // AttnBwdArgs
#include "attention_core.h"
#include "philox.h"

namespace svt {
namespace {

// ---- steps of the backward kernels, beside attention_core.h's (whose text is pinned): the same products on named accumulators ----
// ACC[2] = rows of the tile at KF (K swizzle) times the fragments BF[KSD]: SVT_ATTN_S on any accumulator / fragment pair
#define SVT_ATTN_BWD_ROWPROD(ACC, KF, BF)                                                                                     \
  {                                                                                                                           \
    const uint4* Kf = (KF);                                                                                                   \
    _Pragma("unroll") for (int kb = 0; kb < 2; ++kb) {                                                                        \
      _Pragma("unroll") for (int r = 0; r < 16; ++r) ACC[kb][r] = 0.f;                                                        \
      _Pragma("unroll") for (int ks = 0; ks < KSD; ++ks)                                                                      \
        ACC[kb] = SVT_MFMA_32x32x16(__builtin_bit_cast(bf16x8, Kf[(kb * 32 + kl) * CPR + ((2 * ks + hh) ^ kg)]), BF[ks], ACC[kb]); \
    }                                                                                                                         \
  }
// PFR[2][2] = the accumulators ACC[2] cut to 16 bits: SVT_ATTN_PF on named arrays
#define SVT_ATTN_BWD_PF(PFR, ACC)                                                                                             \
  _Pragma("unroll") for (int kb = 0; kb < 2; ++kb)                                                                            \
    _Pragma("unroll") for (int ss = 0; ss < 2; ++ss)                                                                          \
      _Pragma("unroll") for (int j = 0; j < 8; ++j) PFR[kb][ss][j] = (bf16_t)ACC[kb][ss * 8 + j];
// ACC[DB] += (tile at vbase + OFF, V swizzle, read transposed) times PFR: SVT_ATTN_PV on a named accumulator, tile and operand
#define SVT_ATTN_BWD_TRPROD(ACC, OFF, ST, PFR)                                                                                \
  {                                                                                                                           \
    _Pragma("unroll") for (int db = 0; db < DB; ++db)                                                                         \
      _Pragma("unroll") for (int kb = 0; kb < 2; ++kb)                                                                        \
        _Pragma("unroll") for (int ss = 0; ss < 2; ++ss) {                                                                    \
          const char* vp = vbase[db] + (OFF) + (ST) * STAGE_BYTES + (kb * 32 + ss * 16) * RB;                                 \
          const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t)(vp));                                        \
          const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t)(vp + 8 * RB));                               \
          const s16x8 vv = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);                                           \
          ACC[db] = SVT_MFMA_32x32x16(__builtin_bit_cast(bf16x8, vv), PFR[kb][ss], ACC[db]);                                  \
        }                                                                                                                     \
  }
// SVT_ATTN_STORE_O16 on a named accumulator: row OP gets ACC * MUL in the operand type, 16-byte stores
#define SVT_ATTN_BWD_STORE16(ACC, MUL, OP)                                                                                    \
  _Pragma("unroll") for (int db = 0; db < DB; ++db)                                                                           \
    _Pragma("unroll") for (int g = 0; g < 4; g += 2) {                                                                        \
      unsigned w[2][2];                                                                                                       \
      _Pragma("unroll") for (int u = 0; u < 2; ++u) {                                                                         \
        bf16x4 v;                                                                                                             \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) v[j] = (bf16_t)(ACC[db][(g + u) * 4 + j] * (MUL));                      \
        const uint2 pk = __builtin_bit_cast(uint2, v);                                                                        \
        w[u][0] = pk.x; w[u][1] = pk.y;                                                                                       \
      }                                                                                                                       \
      _Pragma("unroll") for (int d2 = 0; d2 < 2; ++d2) {                                                                      \
        const auto r = __builtin_amdgcn_permlane32_swap(w[0][d2], w[1][d2], false, false);                                    \
        w[0][d2] = r[0]; w[1][d2] = r[1];                                                                                     \
      }                                                                                                                       \
      *(uint4*)((OP) + db * 32 + 8 * (g + hh)) = uint4{w[0][0], w[0][1], w[1][0], w[1][1]};                                   \
    }

// One LDS-DMA fill of a 64-row tile image: rows ROW0 + dkey[i] (clamped to T - 1) of BASE (pitch LD), chunk offset CH[i], into IMG
#define SVT_ATTN_BWD_DMA(IMG, BASE, LD, ROW0, CH)                                                                             \
  _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                                                             \
    int row_ = (ROW0) + dkey[i];                                                                                              \
    if (row_ > T - 1) row_ = T - 1;                                                                                           \
    __builtin_amdgcn_global_load_lds((gptr_t)((BASE) + (long)row_ * (LD) + CH[i]), (lptr_t)((IMG) + (wave * 2 + i) * 64), 16, 0, 0); \
  }

constexpr int DH = 64;
constexpr int KSD = DH / 16, CPR = DH / 8, RB = 2 * DH, TILE16 = 64 * CPR;

// (a) L[b, h, i] = m_i + log2 l_i of the scaled scores and delta[b, h, i] = dO_i . O_i.  Grid (ceil(T / 128), H, B), 256 threads.
__global__ __launch_bounds__(256) void attn_bwd_prep_kernel(const bf16_t* __restrict__ Q, long ldq, const bf16_t* __restrict__ K, long ldk,
                                                            const bf16_t* __restrict__ O, long ldo, const bf16_t* __restrict__ dO,
                                                            long lddo, float* __restrict__ Lws, float* __restrict__ Dws, int T, int H,
                                                            float c) {
  constexpr int DB = 0;   // no O accumulators: the softmax head's rescale loop over o[DB] is empty
  __shared__ __attribute__((aligned(16))) uint4 KS[2][TILE16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, h = blockIdx.y;
  const long bh = (long)b * H + h;

  if (tid < 128) {   // delta: one row per lane
    const int i = blockIdx.x * 128 + tid;
    if (i < T) {
      const uint4* op = (const uint4*)(O + ((long)b * T + i) * ldo + (long)h * DH);
      const uint4* gp = (const uint4*)(dO + ((long)b * T + i) * lddo + (long)h * DH);
      float sum = 0.f;
#pragma unroll
      for (int ch = 0; ch < CPR; ++ch) {
        const bf16x8 ov = __builtin_bit_cast(bf16x8, op[ch]), gv = __builtin_bit_cast(bf16x8, gp[ch]);
#pragma unroll
        for (int j = 0; j < 8; ++j) sum = fmaf((float)gv[j], (float)ov[j], sum);
      }
      Dws[bh * T + i] = sum;
    }
  }

  const int q0 = blockIdx.x * 128 + wave * 32;
  const bf16_t* Qb = Q + (long)b * T * ldq + (long)h * DH;
  const bf16_t* Kb = K + (long)b * T * ldk + (long)h * DH;
  bf16x8 qf[KSD];
  {
    SVT_ATTN_Q_ROW(qp)
#pragma unroll
    for (int ks = 0; ks < KSD; ++ks) qf[ks] = *(const bf16x8*)(qp + ks * 16);
  }
  int dkey[2], kch[2], vch[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) SVT_ATTN_DMA_SRC(wave * 2 + i, dkey[i], kch[i], vch[i])
  (void)vch;

  f32x16 o[1];
  float m = -1e30f, l = 0.f;
  const int hh = lane >> 5;
  const int kl = lane & 31;
  const int kg = (kl >> 1) & 7;
  const int ntiles = (T + 63) / 64;
  SVT_ATTN_BWD_DMA(KS[0], Kb, ldk, 0, kch)
  for (int tile = 0; tile < ntiles; ++tile) {
    const int st = tile & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tile + 1 < ntiles) SVT_ATTN_BWD_DMA(KS[st ^ 1], Kb, ldk, (tile + 1) * 64, kch)
    f32x16 s[2];
    SVT_ATTN_S(KS[st])
    SVT_ATTN_SOFTMAX_HEAD(tile, c)
    float sum = 0.f;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) sum += __builtin_amdgcn_exp2f(fmaf(s[kb][r], c, -m));
    sum += __shfl_xor(sum, 32, 64);
    l += sum;
  }
  const int q = q0 + (lane & 31);
  if (q < T && hh == 0) Lws[bh * T + q] = m + log2f(l);
}

// (b) dQ.  Grid (ceil(T / 128), H, B), 256 threads; LDS per stage: K (K swizzle) | K (V swizzle) | V (K swizzle)
template <bool DROP>
__global__ __launch_bounds__(256) void attn_bwd_dq_kernel(const bf16_t* __restrict__ Q, long ldq, const bf16_t* __restrict__ K,
                                                          const bf16_t* __restrict__ V, long ldk, const bf16_t* __restrict__ dO,
                                                          long lddo, bf16_t* __restrict__ dQ, long lddq, const float* __restrict__ Lws,
                                                          const float* __restrict__ Dws, int T, int H, float c, float scale,
                                                          uint64_t e0, DropSpec drop) {
  constexpr int DB = DH / 32;
  __shared__ __attribute__((aligned(16))) uint4 KV[2][3 * TILE16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, h = blockIdx.y;
  const int q0 = blockIdx.x * 128 + wave * 32;
  const bf16_t* Qb = Q + (long)b * T * ldq + (long)h * DH;
  const bf16_t* Kb = K + (long)b * T * ldk + (long)h * DH;
  const bf16_t* Vb = V + (long)b * T * ldk + (long)h * DH;
  const bf16_t* Gb = dO + (long)b * T * lddo + (long)h * DH;

  bf16x8 qf[KSD], gf[KSD];
  float Lq, dl;
  {
    SVT_ATTN_Q_ROW(qp)
    const bf16_t* gp = Gb + (long)q * lddo + 8 * (lane >> 5);
#pragma unroll
    for (int ks = 0; ks < KSD; ++ks) { qf[ks] = *(const bf16x8*)(qp + ks * 16); gf[ks] = *(const bf16x8*)(gp + ks * 16); }
    Lq = Lws[((long)b * H + h) * T + q];
    dl = Dws[((long)b * H + h) * T + q];
  }
  int dkey[2], kch[2], vch[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) SVT_ATTN_DMA_SRC(wave * 2 + i, dkey[i], kch[i], vch[i])
#define SVT_STAGE_DMA(TILE, STAGE)                                     \
  {                                                                    \
    SVT_ATTN_BWD_DMA(KV[STAGE], Kb, ldk, (TILE) * 64, kch)             \
    SVT_ATTN_BWD_DMA(KV[STAGE] + TILE16, Kb, ldk, (TILE) * 64, vch)    \
    SVT_ATTN_BWD_DMA(KV[STAGE] + 2 * TILE16, Vb, ldk, (TILE) * 64, kch) \
  }

  f32x16 o[DB];
#pragma unroll
  for (int i = 0; i < DB; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[i][r] = 0.f;
  const int hh = lane >> 5;
  const int kl = lane & 31;
  const int kg = (kl >> 1) & 7;
  const int ntiles = (T + 63) / 64;
  const char* vbase[DB];
  SVT_ATTN_VBASE(&KV[0][TILE16])
  SVT_ATTN_DROP_ROW(e0)
  if constexpr (!DROP) { (void)dg0; (void)dsh; (void)dninth; }
  const float ds = DROP ? drop.scale : 1.0f;

  constexpr long STAGE_BYTES = (long)3 * TILE16 * 16;
  SVT_STAGE_DMA(0, 0)
  for (int tile = 0; tile < ntiles; ++tile) {
    const int st = tile & 1;
    // own fills of this tile have landed, everyone's have after the barrier, and every wave is done reading the other stage
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tile + 1 < ntiles) SVT_STAGE_DMA(tile + 1, st ^ 1)
    f32x16 sc[2], s[2];
    SVT_ATTN_BWD_ROWPROD(sc, KV[st], qf)
    SVT_ATTN_BWD_ROWPROD(s, KV[st] + 2 * TILE16, gf)
    if (__builtin_expect(tile * 64 + 64 > T, 0)) {   // wave-uniform, last tile only: keys >= T get P = 0
      const int kbase = tile * 64 + 4 * hh;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (kbase + kb * 32 + (r & 3) + 8 * (r >> 2) >= T) sc[kb][r] = -3e38f;
    }
    if constexpr (DROP) SVT_ATTN_DROP(tile, drop)   // zeroes the dropped dP
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float pv = __builtin_amdgcn_exp2f(fmaf(sc[kb][r], c, -Lq));
        s[kb][r] = pv * fmaf(s[kb][r], ds, -dl);   // dS
      }
    bf16x8 pf[2][2];
    SVT_ATTN_BWD_PF(pf, s)
    SVT_ATTN_BWD_TRPROD(o, 0, st, pf)
  }
#undef SVT_STAGE_DMA

  const int q = q0 + (lane & 31);
  if (q >= T) return;
  bf16_t* op = dQ + ((long)b * T + q) * lddq + (long)h * DH;
  SVT_ATTN_BWD_STORE16(o, scale, op)
}

// (c) dK and dV.  Grid (ceil(T / 128), H, B), 256 threads; LDS per stage: Q (K swizzle) | Q (V swizzle) | dO (K swizzle) | dO (V swizzle),
// then L | delta of the tile's 64 queries, and one 64-word keep bitmap per wave
template <bool DROP>
__global__ __launch_bounds__(256) void attn_bwd_dkv_kernel(const bf16_t* __restrict__ Q, long ldq, const bf16_t* __restrict__ K,
                                                           const bf16_t* __restrict__ V, long ldk, const bf16_t* __restrict__ dO,
                                                           long lddo, bf16_t* __restrict__ dK, bf16_t* __restrict__ dV, long lddkv,
                                                           const float* __restrict__ Lws, const float* __restrict__ Dws, int T, int H,
                                                           float c, float scale, uint64_t e0, DropSpec drop) {
  constexpr int DB = DH / 32;
  __shared__ __attribute__((aligned(16))) uint4 QG[2][4 * TILE16];
  __shared__ __attribute__((aligned(16))) float LD[2][128];
  __shared__ __attribute__((aligned(16))) unsigned BM[4][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, h = blockIdx.y;
  const int hh = lane >> 5;
  const int kl = lane & 31;
  const int kg = (kl >> 1) & 7;
  const int k0 = blockIdx.x * 128 + wave * 32;
  const bf16_t* Qb = Q + (long)b * T * ldq + (long)h * DH;
  const bf16_t* Gb = dO + (long)b * T * lddo + (long)h * DH;
  const float* Lb = Lws + ((long)b * H + h) * T;
  const float* Db = Dws + ((long)b * H + h) * T;

  bf16x8 kf[KSD], vf[KSD];
  {
    int key = k0 + kl;
    if (key > T - 1) key = T - 1;   // results of these lanes are never stored
    const bf16_t* kp = K + ((long)b * T + key) * ldk + (long)h * DH + 8 * hh;
    const bf16_t* vp = V + ((long)b * T + key) * ldk + (long)h * DH + 8 * hh;
#pragma unroll
    for (int ks = 0; ks < KSD; ++ks) { kf[ks] = *(const bf16x8*)(kp + ks * 16); vf[ks] = *(const bf16x8*)(vp + ks * 16); }
  }
  int dkey[2], kch[2], vch[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) SVT_ATTN_DMA_SRC(wave * 2 + i, dkey[i], kch[i], vch[i])
#define SVT_STAGE_DMA(TILE, STAGE)                                                                                          \
  {                                                                                                                         \
    SVT_ATTN_BWD_DMA(QG[STAGE], Qb, ldq, (TILE) * 64, kch)                                                                  \
    SVT_ATTN_BWD_DMA(QG[STAGE] + TILE16, Qb, ldq, (TILE) * 64, vch)                                                         \
    SVT_ATTN_BWD_DMA(QG[STAGE] + 2 * TILE16, Gb, lddo, (TILE) * 64, kch)                                                    \
    SVT_ATTN_BWD_DMA(QG[STAGE] + 3 * TILE16, Gb, lddo, (TILE) * 64, vch)                                                    \
    if (wave < 2) {   /* wave 0: L, wave 1: delta of query TILE * 64 + lane (clamped), four bytes per lane */               \
      int row_ = (TILE) * 64 + lane;                                                                                        \
      if (row_ > T - 1) row_ = T - 1;                                                                                       \
      __builtin_amdgcn_global_load_lds((gptr_t)((wave ? Db : Lb) + row_), (lptr_t)(&LD[STAGE][wave * 64]), 4, 0, 0);        \
    }                                                                                                                       \
  }

  f32x16 dk[DB], dv[DB];
#pragma unroll
  for (int i = 0; i < DB; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) { dk[i][r] = 0.f; dv[i][r] = 0.f; }
  const int ntiles = (T + 63) / 64;
  const char* vbase[DB];
  SVT_ATTN_VBASE(&QG[0][TILE16])
  constexpr long STAGE_BYTES = (long)4 * TILE16 * 16;
  constexpr long G_OFF = (long)2 * TILE16 * 16;   // the dO image in the V swizzle, from Q's
  const float ds = DROP ? drop.scale : 1.0f;
  // element index of (b, h, query 0, the wave's first key); lane t computes the bits of query tile * 64 + t
  const uint64_t ebase = e0 + (uint64_t)((long)b * H + h) * (uint64_t)T * (uint64_t)T + (uint64_t)k0;

  SVT_STAGE_DMA(0, 0)
  for (int tile = 0; tile < ntiles; ++tile) {
    const int st = tile & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tile + 1 < ntiles) SVT_STAGE_DMA(tile + 1, st ^ 1)
#ifndef SVT_ATTN_BWD_DIRECT_MASK
    if constexpr (DROP) {
      const uint64_t erow = ebase + (uint64_t)(tile * 64 + lane) * (uint64_t)T;
      const uint64_t g0 = erow >> 2;
      const unsigned al = (unsigned)(erow & 3);
      unsigned mlo = 0, mhi = 0;
#pragma unroll
      for (int cc = 0; cc < 8; ++cc) {
        const Philox4 pw = drop_words(drop, g0 + cc);
#pragma unroll
        for (int k = 0; k < 4; ++k) mlo |= (unsigned)(pw.w[k] >= drop.thr) << (4 * cc + k);
      }
      if (__any((int)al != 0)) {   // wave-uniform: the ninth group, which an unaligned row's last keys reach
        const Philox4 pw = drop_words(drop, g0 + 8);
#pragma unroll
        for (int k = 0; k < 4; ++k) mhi |= (unsigned)(pw.w[k] >= drop.thr) << k;
      }
      BM[wave][lane] = __builtin_amdgcn_alignbit(mhi, mlo, al);   // bit n: key k0 + n of this row
      __builtin_amdgcn_wave_barrier();   // the wave's own LDS write, read back below: in order within a wave
    }
#endif
    f32x16 sc[2], dp[2];
    SVT_ATTN_BWD_ROWPROD(sc, QG[st], kf)
    SVT_ATTN_BWD_ROWPROD(dp, QG[st] + 2 * TILE16, vf)
    if (__builtin_expect(tile * 64 + 64 > T, 0)) {   // wave-uniform, last tile only: rows i >= T get P = 0, so P~ = dS = 0 exactly
      const int ibase = tile * 64 + 4 * hh;
#pragma unroll
      for (int qb = 0; qb < 2; ++qb)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (ibase + qb * 32 + (r & 3) + 8 * (r >> 2) >= T) sc[qb][r] = -3e38f;
    }
#pragma unroll
    for (int qb = 0; qb < 2; ++qb)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int row = qb * 32 + 8 * g + 4 * hh;
        const float4 l4 = *(const float4*)&LD[st][row];
        const float4 d4 = *(const float4*)&LD[st][64 + row];
        const float lv[4] = {l4.x, l4.y, l4.z, l4.w}, dv4[4] = {d4.x, d4.y, d4.z, d4.w};
        unsigned wv[4] = {0, 0, 0, 0};
        if constexpr (DROP) {
          const uint4 w4 = *(const uint4*)&BM[wave][row];
          wv[0] = w4.x; wv[1] = w4.y; wv[2] = w4.z; wv[3] = w4.w;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int r = 4 * g + j;
          const float pv = __builtin_amdgcn_exp2f(fmaf(sc[qb][r], c, -lv[j]));
          float pk = pv, dpv = dp[qb][r];
          if constexpr (DROP) {
#ifdef SVT_ATTN_BWD_DIRECT_MASK   // the measured-and-dropped form (an experimental build only): one Philox call per element, 32 per lane and tile
            const uint64_t e = ebase + (uint64_t)kl + (uint64_t)(tile * 64 + row + j) * (uint64_t)T;
            const Philox4 pw = drop_words(drop, e >> 2);
            const unsigned e3 = (unsigned)e & 3, ww = e3 == 0 ? pw.w[0] : e3 == 1 ? pw.w[1] : e3 == 2 ? pw.w[2] : pw.w[3];
            const int keepm = ww >= drop.thr ? -1 : 0;
            (void)wv;
#else
            const int keepm = (int)(wv[j] << (31 - kl)) >> 31;   // all ones: kept
#endif
            pk = __builtin_bit_cast(float, __builtin_bit_cast(int, pv) & keepm);
            dpv = __builtin_bit_cast(float, __builtin_bit_cast(int, dpv) & keepm);
          }
          sc[qb][r] = pk;                          // keep P (s joins at the store)
          dp[qb][r] = pv * fmaf(dpv, ds, -dv4[j]);  // dS
        }
      }
    bf16x8 pf[2][2];
    SVT_ATTN_BWD_PF(pf, sc)
    SVT_ATTN_BWD_TRPROD(dv, G_OFF, st, pf)
    SVT_ATTN_BWD_PF(pf, dp)
    SVT_ATTN_BWD_TRPROD(dk, 0, st, pf)
  }
#undef SVT_STAGE_DMA

  const int key = k0 + kl;
  if (key >= T) return;
  bf16_t* kp = dK + ((long)b * T + key) * lddkv + (long)h * DH;
  bf16_t* vp = dV + ((long)b * T + key) * lddkv + (long)h * DH;
  SVT_ATTN_BWD_STORE16(dk, scale, kp)
  SVT_ATTN_BWD_STORE16(dv, ds, vp)
}

}  // namespace

// svt_debug_set key 46 returns it: which form the last attention backward launched (0 = none yet, 1 = plain, 2 = masked)
int g_attn_bwd_id = 0;

size_t attention_backward_workspace_bytes(int B, int H, int T) { return 2 * align_up((size_t)B * H * T * sizeof(float)); }

int launch_attention_backward(const AttnBwdArgs& a, hipStream_t s) {
  auto refuse = [](const char* why) { set_error(std::string("attention_backward: ") + why); return -1; };
  if (a.dh != 64) return refuse("head_dim must be 64");
  if (a.prec != 1) return refuse("precision must be SVT_PREC_BF16 (the build's 16-bit operand type)");
  if (a.gate || a.relpb) return refuse("a position bias is not served");
  if (!a.Q || !a.K || !a.V || !a.O || !a.dO || !a.dQ || !a.dK || !a.dV || !a.ws) return refuse("null argument");
  if (a.B < 1 || a.T < 1 || a.H < 1) return refuse("batch, t and heads must be positive");
  if ((a.ldq | a.ldkv | a.ldo | a.lddo | a.lddq | a.lddkv) % 8) return refuse("strides must be multiples of 8 elements");
  const long D = (long)a.H * a.dh;
  if (a.ldq < D || a.ldkv < D || a.ldo < D || a.lddo < D || a.lddq < D || a.lddkv < D) return refuse("a row stride is shorter than heads * head_dim");
  if ((((uintptr_t)a.Q | (uintptr_t)a.K | (uintptr_t)a.V | (uintptr_t)a.O | (uintptr_t)a.dO | (uintptr_t)a.dQ | (uintptr_t)a.dK |
        (uintptr_t)a.dV) & 15) || ((uintptr_t)a.ws & 3))
    return refuse("q, k, v, o, do, dq, dk, dv must be 16-byte aligned");
  const float c = a.scale * 1.44269504088896340736f;
  const dim3 grid((a.T + 127) / 128, a.H, a.B);
  float* Lws = (float*)a.ws;
  float* Dws = (float*)((char*)a.ws + align_up((size_t)a.B * a.H * a.T * sizeof(float)));
  const bf16_t *Q = (const bf16_t*)a.Q, *K = (const bf16_t*)a.K, *V = (const bf16_t*)a.V, *O = (const bf16_t*)a.O, *G = (const bf16_t*)a.dO;
  const double pair = 2.0 * a.B * a.H * (double)a.T * a.T * a.dh;   // flops of one product
  prof_begin(s);
  hipLaunchKernelGGL(attn_bwd_prep_kernel, grid, dim3(256), 0, s, Q, a.ldq, K, a.ldkv, O, a.ldo, G, a.lddo, Lws, Dws, a.T, a.H, c);
  const DropSpec none{};
  if (a.drop) {
    hipLaunchKernelGGL(attn_bwd_dq_kernel<true>, grid, dim3(256), 0, s, Q, a.ldq, K, V, a.ldkv, G, a.lddo, (bf16_t*)a.dQ, a.lddq, Lws, Dws,
                       a.T, a.H, c, a.scale, a.e0, *a.drop);
    hipLaunchKernelGGL(attn_bwd_dkv_kernel<true>, grid, dim3(256), 0, s, Q, a.ldq, K, V, a.ldkv, G, a.lddo, (bf16_t*)a.dK, (bf16_t*)a.dV,
                       a.lddkv, Lws, Dws, a.T, a.H, c, a.scale, a.e0, *a.drop);
    g_attn_bwd_id = 2;
  } else {
    hipLaunchKernelGGL(attn_bwd_dq_kernel<false>, grid, dim3(256), 0, s, Q, a.ldq, K, V, a.ldkv, G, a.lddo, (bf16_t*)a.dQ, a.lddq, Lws, Dws,
                       a.T, a.H, c, a.scale, (uint64_t)0, none);
    hipLaunchKernelGGL(attn_bwd_dkv_kernel<false>, grid, dim3(256), 0, s, Q, a.ldq, K, V, a.ldkv, G, a.lddo, (bf16_t*)a.dK, (bf16_t*)a.dV,
                       a.lddkv, Lws, Dws, a.T, a.H, c, a.scale, (uint64_t)0, none);
    g_attn_bwd_id = 1;
  }
  prof_end(s, 8.0 * pair, 0.0, 2);
  SVT_LAUNCH_CHECK();
  return 0;
}
}  // namespace svt
