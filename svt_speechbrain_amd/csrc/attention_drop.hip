// Fused attention with the training-mode dropout mask inside (16-bit operands, both library builds): softmax -> dropout -> P V in HF's
// eager order without the (B, H, T, T) scores.  flash_attn_drop_kernel is the lockstep flash_attn_kernel<DH, false, NW> of
// attention_bf16.hip -- LDS-DMA staging, two stages, one barrier per tile, S^T product, transposing V reads, deferred rescale, the
// 16-byte epilogue stores -- with one more step between the row sum and the cut of P to 16 bits: SVT_ATTN_DROP (attention_core.h)
// zeroes the dropped probabilities.  The row sum l runs over ALL keys (dropout does not renormalise) and the scale float(1 / (1 - p))
// is applied once, in the epilogue, folded into 1 / l.  The mask is a function of the element's logical position (philox.h, DropSpec;
// include/svt_mi355.h "svt_dropout"), so it is bit for bit the mask launch_softmax_dropout lays on the score-matrix path.
#include "attention_core.h"
#include "philox.h"

namespace svt {
namespace {

template <int DH, int NW>
__global__ __launch_bounds__(64 * NW) void flash_attn_drop_kernel(const bf16_t* __restrict__ Q, long ldq, long q_bstride,
                                                              const bf16_t* __restrict__ K, long ldk, long k_bstride,
                                                              const bf16_t* __restrict__ V, bf16_t* __restrict__ O, long ldo,
                                                              long o_bstride, int T, int H, float c, uint64_t e0, DropSpec drop) {
  constexpr int KSD = DH / 16;   // k-steps over head_dim for S
  constexpr int DB = DH / 32;    // 32-row blocks of O^T
  constexpr int CPR = DH / 8;    // 16-byte chunks per K row
  constexpr int RB = 2 * DH;     // bytes per K / V row in LDS
  constexpr int TILE16 = 64 * CPR;  // uint4 per tile
  __shared__ __attribute__((aligned(16))) uint4 KV[2][2 * TILE16];   // two stages of { K tile, V tile }

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, h = blockIdx.y;
  const int q0 = blockIdx.x * (32 * NW) + wave * 32;
  const bf16_t* Qb = Q + (long)b * q_bstride + (long)h * DH;
  const bf16_t* Kb = K + (long)b * k_bstride + (long)h * DH;
  const bf16_t* Vb = V + (long)b * k_bstride + (long)h * DH;

  bf16x8 qf[KSD];
  {
    SVT_ATTN_Q_ROW(qp)
#pragma unroll
    for (int ks = 0; ks < KSD; ++ks) qf[ks] = *(const bf16x8*)(qp + ks * 16);
  }
  constexpr int DMA_PER_WAVE = CPR / NW;   // LDS-DMA instructions per wave per tile and operand
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
  const int kl = lane & 31;
  const int kg = (DH == 64) ? ((kl >> 1) & 7) : (kl & 15);
  const int ntiles = (T + 63) / 64;
  const char* vbase[DB];
  SVT_ATTN_VBASE(&KV[0][TILE16])
  SVT_ATTN_DROP_ROW(e0)

  constexpr long STAGE_BYTES = (long)2 * TILE16 * 16;
  SVT_STAGE_DMA(0, 0)
  for (int tile = 0; tile < ntiles; ++tile) {
    const int st = tile & 1;
    // own fills of this tile have landed, everyone's have after the barrier, and every wave is done reading the other stage
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tile + 1 < ntiles) {
      if (st) SVT_STAGE_DMA(tile + 1, 0) else SVT_STAGE_DMA(tile + 1, 1)
    }
    f32x16 s[2];
    SVT_ATTN_S(KV[st])
    SVT_ATTN_SOFTMAX_HEAD(tile, c)
    typedef float f32x2v __attribute__((ext_vector_type(2)));
    f32x2v sum2 = {0.f, 0.f};
    const f32x2v c2 = {c, c}, nm2 = {-m, -m};
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
    l += sum;   // over ALL keys: the dropped ones count
    SVT_ATTN_DROP(tile, drop)
    bf16x8 pf[2][2];
    SVT_ATTN_PF
    SVT_ATTN_PV(st)
  }

  const int q = q0 + (lane & 31);
  if (q >= T) return;
  const float inv = drop.scale / l;
  bf16_t* op = O + (long)b * o_bstride + (long)q * ldo + (long)h * DH;
  SVT_ATTN_STORE_O16
}

#undef SVT_STAGE_DMA

}  // namespace

// The plain launcher's checks; kernel ids (svt_debug_set key 38): 9 = flash_attn_drop_kernel<64, 4>, 10 = flash_attn_drop_kernel<128, 4>
int launch_flash_attention_dropout(const void* Q, long ldq, long q_bstride, const void* K, const void* V, long ldk, long k_bstride,
                                   void* O, long ldo, long o_bstride, int B, int T, int H, int dh, float scale, uint64_t e0,
                                   const DropSpec& d, hipStream_t s) {
  if ((ldq | ldk | ldo | q_bstride | k_bstride | o_bstride) % 8 || ((uintptr_t)O & 15) || ((uintptr_t)Q & 15)) {
    set_error("flash_attention_dropout: strides must be multiples of 8 elements and Q / O 16-byte aligned"); return -1; }
  if (dh != 64 && dh != 128) { set_error("flash_attention_dropout: head_dim must be 64 or 128"); return -1; }
  const float c = scale * 1.44269504088896340736f;
  const dim3 grid((T + 127) / 128, H, B);
  const double flops = 4.0 * B * H * (double)T * T * dh;
  auto lockstep = [&](auto kernel, int threads) {
    hipLaunchKernelGGL(kernel, grid, dim3(threads), 0, s, (const bf16_t*)Q, ldq, q_bstride, (const bf16_t*)K, ldk, k_bstride,
                       (const bf16_t*)V, (bf16_t*)O, ldo, o_bstride, T, H, c, e0, d);
  };
  prof_begin(s);
  // (the eight-wave form, flash_attn_drop_kernel<64, 8> on 256-query workgroups, was measured and is not built: 105.2 against 98.3 us at
  //  32 x 12 heads x 499 frames, 202 against 184 us at 64 x 12 x 499 -- the kernel is bound by vector issue, not by K / V traffic; id 11
  //  stays unassigned)
  if (dh == 64) { lockstep(flash_attn_drop_kernel<64, 4>, 256); g_flash_kernel_id = 9; }
  else { lockstep(flash_attn_drop_kernel<128, 4>, 256); g_flash_kernel_id = 10; }
  prof_end(s, flops, 0.0, 2);
  SVT_LAUNCH_CHECK();
  return 0;
}
}  // namespace svt
