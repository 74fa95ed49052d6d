// Fused attention on 16-bit operands (bf16, or IEEE half in the f16 build): the lockstep kernel and its staggered eight-wave form, and
// their launcher.  The design and the steps shared with the split-operand kernels are in attention_core.h.
#include "attention_core.h"

namespace svt {
namespace {

// BIAS: WavLM's gated relative position bias, scores += gate[b,h,q] * pb[h][key - q + T - 1] (pb row of 2T-1 floats kept
// in LDS; added in the scaled log2 domain before the row max).
template <int DH, bool BIAS = false, int NW = 4>
__global__ __launch_bounds__(64 * NW) void flash_attn_kernel(const bf16_t* __restrict__ Q, long ldq, long q_bstride,
                                                         const bf16_t* __restrict__ K, long ldk, long k_bstride,
                                                         const bf16_t* __restrict__ V, int /*unused*/, bf16_t* __restrict__ O,
                                                         long ldo, long o_bstride, int T, int H, float c,
                                                         const float* __restrict__ gate, const float* __restrict__ pbias) {
  constexpr int KSD = DH / 16;   // k-steps over head_dim for S
  constexpr int DB = DH / 32;    // 32-row blocks of O^T
  constexpr int CPR = DH / 8;    // 16-byte chunks per K row
  constexpr int RB = 2 * DH;     // bytes per K / V row in LDS
  // two stages of { K tile, V tile }, each tile row-major [key][slot] with slot = chunk ^ swizzle(key); filled by LDS-DMA
  constexpr int TILE16 = 64 * CPR;  // uint4 per tile
  __shared__ __attribute__((aligned(16))) uint4 KV[2][2 * TILE16];
  extern __shared__ float pbl[];  // BIAS: this head's 2T-1 bias values

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, h = blockIdx.y;
  const int q0 = blockIdx.x * (32 * NW) + wave * 32;  // NW waves x 32 queries: every workgroup streams all of K and V once
  const bf16_t* Qb = Q + (long)b * q_bstride + (long)h * DH;
  const bf16_t* Kb = K + (long)b * k_bstride + (long)h * DH;
  const bf16_t* Vb = V + (long)b * k_bstride + (long)h * DH;

  bf16x8 qf[KSD];
  {
    SVT_ATTN_Q_ROW(qp)
#pragma unroll
    for (int ks = 0; ks < KSD; ++ks) qf[ks] = *(const bf16x8*)(qp + ks * 16);
  }

  float gq = 0.f;   // gate of this lane's query, pre-multiplied by log2(e)
  int qrel = 0;     // T - 1 - query
  if constexpr (BIAS) {
    for (int i = tid; i < 2 * T - 1; i += 64 * NW) pbl[i] = pbias[(long)h * (2 * T - 1) + i];
    int q = q0 + (lane & 31);
    if (q > T - 1) q = T - 1;
    gq = gate[((long)b * H + h) * T + q] * 1.44269504088896340736f;
    qrel = T - 1 - q;
  }
  // LDS-DMA staging (SVT_ATTN_DMA_SRC): no staging registers, no ds_write; the next tile is in flight while the current one is
  // multiplied (two stages, one barrier per tile)
  constexpr int DMA_PER_WAVE = CPR / NW;   // instructions per wave per tile and operand (2 / 4 with four waves)
  static_assert(DMA_PER_WAVE >= 1, "too many waves for the tile's fill");
  int dkey[DMA_PER_WAVE], kch[DMA_PER_WAVE], vch[DMA_PER_WAVE];
#pragma unroll
  for (int i = 0; i < DMA_PER_WAVE; ++i) SVT_ATTN_DMA_SRC(wave * DMA_PER_WAVE + i, dkey[i], kch[i], vch[i])
#define SVT_STAGE_DMA(TILE, STAGE)                                                                                  \
  {                                                                                                                  \
    const int key0_ = (TILE) * 64;                                                                                   \
    _Pragma("unroll") for (int i = 0; i < DMA_PER_WAVE; ++i) {                                                       \
      int key_ = key0_ + dkey[i];                                                                                    \
      if (key_ > T - 1) key_ = T - 1;                                                                                \
      const bf16_t* kp_ = Kb + (long)key_ * ldk;                                                                     \
      __builtin_amdgcn_global_load_lds((gptr_t)(kp_ + kch[i]),                                                       \
                                       (lptr_t)(&KV[STAGE][(wave * DMA_PER_WAVE + i) * 64]), 16, 0, 0);              \
      __builtin_amdgcn_global_load_lds((gptr_t)(kp_ + (Vb - Kb) + vch[i]),                                           \
                                       (lptr_t)(&KV[STAGE][TILE16 + (wave * DMA_PER_WAVE + i) * 64]), 16, 0, 0);     \
    }                                                                                                                \
  }

  f32x16 o[DB];
#pragma unroll
  for (int i = 0; i < DB; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[i][r] = 0.f;
  float m = -1e30f, l = 0.f;
  const int hh = lane >> 5;
  const int kl = lane & 31;                                     // key within a 32-key block
  const int kg = (DH == 64) ? ((kl >> 1) & 7) : (kl & 15);      // its swizzle (same for both key blocks: 32 % 16 == 0)
  const int ntiles = (T + 63) / 64;
  const char* vbase[DB];
  SVT_ATTN_VBASE(&KV[0][TILE16])

  constexpr long STAGE_BYTES = (long)2 * TILE16 * 16;
  SVT_STAGE_DMA(0, 0)
  for (int tile = 0; tile < ntiles; ++tile) {
    const int st = tile & 1;
    // own fills of this tile have landed (explicit vmcnt(0): hipcc's own placement of that wait is an alias-analysis
    // artefact, not a contract), everyone's have after the barrier, and every wave is done reading the other stage
    // (tile - 1), which the next fill overwrites
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tile + 1 < ntiles) {
      if (st) SVT_STAGE_DMA(tile + 1, 0) else SVT_STAGE_DMA(tile + 1, 1)
    }
    f32x16 s[2];
    SVT_ATTN_S(KV[st])
    if constexpr (BIAS) {
      // x = s*c + gate*log2e * pb[key - q + T - 1]; from here on the scores ARE in the log2 domain (cs = 1 below)
      const int kb0 = tile * 64 + 4 * hh + qrel;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          int idx = kb0 + kb * 32 + (r & 3) + 8 * (r >> 2);
          if (idx > 2 * T - 2) idx = 2 * T - 2;   // keys >= T of the last tile (masked below)
          s[kb][r] = fmaf(s[kb][r], c, gq * pbl[idx]);
        }
    }
    const float cs = BIAS ? 1.0f : c;
    SVT_ATTN_SOFTMAX_HEAD(tile, cs)
    // exponent arguments and row sums on pairs (v_pk_fma_f32 / v_pk_add_f32: two values per issue slot)
    typedef float f32x2v __attribute__((ext_vector_type(2)));
    f32x2v sum2 = {0.f, 0.f};
    const f32x2v c2 = {cs, cs}, nm2 = {-m, -m};
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        const f32x2v e = f32x2v{s[kb][r], s[kb][r + 1]} * c2 + nm2;
        const f32x2v pp = {__builtin_amdgcn_exp2f(e.x), __builtin_amdgcn_exp2f(e.y)};
        s[kb][r] = pp.x;
        s[kb][r + 1] = pp.y;
        sum2 += pp;
      }
    float sum = sum2.x + sum2.y;
    sum += __shfl_xor(sum, 32, 64);
    l += sum;
    bf16x8 pf[2][2];
    SVT_ATTN_PF
    SVT_ATTN_PV(st)
  }

  const int q = q0 + (lane & 31);
  if (q >= T) return;
  const float inv = 1.f / l;
  bf16_t* op = O + (long)b * o_bstride + (long)q * ldo + (long)h * DH;
  SVT_ATTN_STORE_O16
}

#undef SVT_STAGE_DMA

// ---------------------------------------------------------------------------------------------------------------------
// Staggered form of the eight-wave lockstep flash_attn_kernel (round 4; the lockstep form, flash_attn_kernel<64, false, 8>, is retired).
// What the counters said about that kernel at 32 x 12 heads x 499 frames
// (profiles/r04_attention_pmc.txt): 16 MFMAs (512 cycles of the matrix pipe) and ~150 vector instructions (~550 cycles of the vector
// pipe: 32 quarter-rate exponentials are half of it) per wave and 64-key tile -- the two pipes are BALANCED -- yet a SIMD retires a
// wave-tile only every ~1 340 cycles (matrix pipe busy 0.24 of the kernel, waves parked at waits and barriers for 43 % of their
// cycles): the workgroup's barrier per tile keeps its eight waves in the same phase, so the two waves a workgroup has on a SIMD
// multiply at the same time and exponentiate at the same time, and only the other workgroup of the CU ever fills the idle pipe.
// Here waves 4-7 run HALF A TILE behind waves 0-3, the way the GEMM kernels stagger their wave groups: every wave executes the
// same per-tile sequence S = K Q^T -> softmax -> O += V P, but waves 0-3 pass the tile's barrier in front of S and waves 4-7 between
// the softmax and the P V product of the previous tile -- when one group is in its MFMA phases the SIMD partner is in its softmax.
// The barrier of tile j still means "tile j has landed, and tile j + 1 may be requested": with the late group still reading V of tile
// j - 1 at that point the request needs a third stage (tile j + 1 overwrites tile j - 2): 48 KiB per workgroup, two workgroups per CU.
// The LDS-DMA is issued from inline asm (attn_dma16).
template <int DH>
__global__ __launch_bounds__(512) void flash_attn_stag_kernel(const bf16_t* __restrict__ Q, long ldq, long q_bstride,
                                                              const bf16_t* __restrict__ K, long ldk, long k_bstride,
                                                              const bf16_t* __restrict__ V, bf16_t* __restrict__ O, long ldo,
                                                              long o_bstride, int T, int H, float c, int nqb) {
  static_assert(DH == 64, "built for head_dim 64");
  constexpr int NW = 8, NST = 3;
  constexpr int KSD = DH / 16, DB = DH / 32, CPR = DH / 8, RB = 2 * DH;
  constexpr int TILE16 = 64 * CPR;                   // uint4 per tile
  constexpr int STAGE16 = 2 * TILE16;                // K tile + V tile
  constexpr long STAGE_BYTES = (long)STAGE16 * 16;
  __shared__ __attribute__((aligned(16))) uint4 KV[NST * STAGE16];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int bh, qblk;
  attn_block_map(nqb, bh, qblk);
  const int b = bh / H, h = bh - b * H;
  const int q0 = qblk * (32 * NW) + wave * 32;
  const bf16_t* Qb = Q + (long)b * q_bstride + (long)h * DH;
  const bf16_t* Kb = K + (long)b * k_bstride + (long)h * DH;
  const bf16_t* Vb = V + (long)b * k_bstride + (long)h * DH;

  bf16x8 qf[KSD];
  {
    SVT_ATTN_Q_ROW(qp)
#pragma unroll
    for (int ks = 0; ks < KSD; ++ks) qf[ks] = *(const bf16x8*)(qp + ks * 16);
  }
  // one LDS-DMA instruction per wave, tile and operand (8 rows x 128 B)
  int dkey, kch, vch;
  SVT_ATTN_DMA_SRC(wave, dkey, kch, vch)
  const unsigned lds0 = lds_base(KV);
  auto stage_dma = [&](int tile, int stage) {
    int key = tile * 64 + dkey;
    if (key > T - 1) key = T - 1;
    const bf16_t* kp = Kb + (long)key * ldk;
    const unsigned dst = lds0 + (unsigned)((stage * STAGE16 + wave * 64) * 16);
    attn_dma16(kp + kch, dst);
    attn_dma16(kp + (Vb - Kb) + vch, dst + TILE16 * 16);
  };

  f32x16 o[DB];
#pragma unroll
  for (int i = 0; i < DB; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[i][r] = 0.f;
  float m = -1e30f, l = 0.f;
  const int hh = lane >> 5;
  const int kl = lane & 31;
  const int kg = (kl >> 1) & 7;
  const int ntiles = (T + 63) / 64;
  const char* vbase[DB];
  SVT_ATTN_VBASE(&KV[TILE16])
  f32x16 s[2];
  bf16x8 pf[2][2];

  // the barrier of tile j: this wave's share of tile j has landed; behind the barrier everyone's has, and every wave is done with
  // tile j - 2, whose stage the request for tile j + 1 overwrites
#define SVT_AT_BAR(J)                                                                                   \
  {                                                                                                     \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                    \
    __builtin_amdgcn_s_barrier();                                                                       \
    if ((J) + 1 < ntiles) stage_dma((J) + 1, st_next);                                                  \
  }
  // softmax: P = exp2(s c - m) on two scalar chains -> bf16
#define SVT_AT_SM(TILE)                                                                                 \
  {                                                                                                     \
    SVT_ATTN_SOFTMAX_HEAD(TILE, c)                                                                      \
    float sa = 0.f, sb = 0.f;                                                                           \
    _Pragma("unroll") for (int kb = 0; kb < 2; ++kb)                                                    \
      _Pragma("unroll") for (int r = 0; r < 16; r += 2) {                                               \
        const float p0 = __builtin_amdgcn_exp2f(fmaf(s[kb][r], c, -m));                                 \
        const float p1 = __builtin_amdgcn_exp2f(fmaf(s[kb][r + 1], c, -m));                             \
        s[kb][r] = p0; s[kb][r + 1] = p1;                                                               \
        sa += p0; sb += p1;                                                                             \
      }                                                                                                 \
    float sum = sa + sb;                                                                                \
    sum += __shfl_xor(sum, 32, 64);                                                                     \
    l += sum;                                                                                           \
    SVT_ATTN_PF                                                                                         \
  }

  stage_dma(0, 0);
  int st = 0;   // stage of the tile being multiplied
  if (wave < 4) {
    for (int tile = 0; tile < ntiles; ++tile) {
      const int st_next = st + 1 == NST ? 0 : st + 1;
      SVT_AT_BAR(tile)
      SVT_ATTN_S(KV + st * STAGE16)
      SVT_AT_SM(tile)
      SVT_ATTN_PV(st)
      st = st_next;
    }
  } else {
    {
      const int st_next = 1;
      SVT_AT_BAR(0)
    }
    for (int tile = 0; tile < ntiles; ++tile) {
      const int st1 = st + 1 == NST ? 0 : st + 1;
      SVT_ATTN_S(KV + st * STAGE16)
      SVT_AT_SM(tile)
      if (tile + 1 < ntiles) {
        const int st_next = st1 + 1 == NST ? 0 : st1 + 1;   // stage of tile + 2
        SVT_AT_BAR(tile + 1)
      }
      SVT_ATTN_PV(st)
      st = st1;
    }
  }
#undef SVT_AT_BAR
#undef SVT_AT_SM

  const int q = q0 + (lane & 31);
  if (q >= T) return;
  const float inv = 1.f / l;
  bf16_t* op = O + (long)b * o_bstride + (long)q * ldo + (long)h * DH;
  SVT_ATTN_STORE_O16
}

}  // namespace

// svt_debug_set key 38 returns it: which fused attention kernel the last launch of this process chose (0 = none yet), so that the
// tests name the kernel they reached instead of restating the launchers' predicates.  1 = flash_attn_kernel<64>, 2 = flash_attn_kernel<128>,
// 3 = flash_attn_stag_kernel<64>, 4 = flash_attn_kernel<64, true>, 5 = flash_attn_kernel<64, true, 8>, 6 = flash_attn_x3_kernel<64, F16>,
// 7 = flash_attn_x3_kernel<128, F16>, 8 = flash_attn_x3_stag_kernel<F16> (6-8: attention_x3.hip)
int g_flash_kernel_id = 0;

int g_flash_wide = 1;  // svt_debug_set key 8: 1 = 8-wave (256-query) workgroups where they pay, 0 = 4-wave ones.  (Round 3: four-wave workgroups held to
                       // three per CU by 16 KiB of unused LDS -- 1 536 workgroups = exactly two rounds instead of 1.5 -- measured 51.1 against 48.5 us
                       // at C2, 138.6 against 130.9 at C3: the kernel is bound by issue throughput, not by the half-empty second round.  A four-stage
                       // K / V ring with three tiles in flight (asm LDS-DMA, counted vmcnt): 47.9 against 46.6-49.1 us, 131 against 125-128:
                       // not waiting for K / V either.  Both removed.)
// V row-major (same layout and strides as K): no transposed copy of V is needed
int launch_flash_attention(const void* Q, long ldq, long q_bstride, const void* K, const void* V, long ldk, long k_bstride,
                           void* O, long ldo, long o_bstride, int B, int T, int H, int dh, float scale, hipStream_t s,
                           const float* gate, const float* pb) {
  if ((ldq | ldk | ldo | q_bstride | k_bstride | o_bstride) % 8 || ((uintptr_t)O & 15) || ((uintptr_t)Q & 15)) {
    set_error("flash_attention: strides must be multiples of 8 elements and Q / O 16-byte aligned"); return -1; }
  const float c = scale * 1.44269504088896340736f;
  dim3 grid((T + 127) / 128, H, B);
  // eight-wave workgroups (256 queries) halve the K / V traffic per query; used when a head has more than 128 queries
  // (measured 45.7 vs 46.9 us at 32 x 12 heads x 499 frames, 114.2 vs 118.7 us at 64 x 16; with few workgroups -- one 5 s
  // utterance: 12 -- the four-wave form spreads over more CUs and stays)
  const bool wide = g_flash_wide && dh == 64 && T > 128 && (long)B * H * ((T + 255) / 256) >= 512;
  if (wide) grid.x = (T + 255) / 256;
  const double flops = 4.0 * B * H * (double)T * T * dh;
  // one launch of flash_attn_kernel<DH, BIAS, NW> on `grid`
  auto lockstep = [&](auto kernel, int threads, size_t dyn) {
    hipLaunchKernelGGL(kernel, grid, dim3(threads), dyn, s, (const bf16_t*)Q, ldq, q_bstride, (const bf16_t*)K, ldk, k_bstride,
                       (const bf16_t*)V, 0, (bf16_t*)O, ldo, o_bstride, T, H, c, gate, pb);
  };
  if (gate && pb) {
    if (dh != 64) { set_error("flash_attention: the relative-position-bias variant is built for head_dim 64"); return -1; }
    const size_t dyn = (size_t)(2 * T - 1) * 4;
    if (dyn > 32768) { set_error("flash_attention: sequence too long for the LDS-resident position-bias row"); return -1; }
    prof_begin(s);
    if (wide) lockstep(flash_attn_kernel<64, true, 8>, 512, dyn);
    else lockstep(flash_attn_kernel<64, true>, 256, dyn);
    g_flash_kernel_id = wide ? 5 : 4;
    prof_end(s, flops, 0.0, 2);
    SVT_LAUNCH_CHECK();
    return 0;
  }
  gate = pb = nullptr;   // the kernels without BIAS get no bias pointers (one of the two alone selects nothing)
  prof_begin(s);
  if (dh == 64 && wide) {
    // staggered form (flash_attn_stag_kernel, round 4): three K / V stages, waves 4-7 half a tile behind waves 0-3
    const int nqb = (T + 255) / 256;
    hipLaunchKernelGGL((flash_attn_stag_kernel<64>), dim3((unsigned)(nqb * B * H)), dim3(512), 0, s, (const bf16_t*)Q, ldq, q_bstride,
                       (const bf16_t*)K, ldk, k_bstride, (const bf16_t*)V, (bf16_t*)O, ldo, o_bstride, T, H, c, nqb);
    g_flash_kernel_id = 3;
  }
  else if (dh == 64) { lockstep(flash_attn_kernel<64>, 256, 0); g_flash_kernel_id = 1; }
  else if (dh == 128) { lockstep(flash_attn_kernel<128>, 256, 0); g_flash_kernel_id = 2; }
  else { set_error("flash_attention: head_dim must be 64 or 128"); return -1; }
  prof_end(s, flops, 0.0, 2);
  SVT_LAUNCH_CHECK();
  return 0;
}
}  // namespace svt
