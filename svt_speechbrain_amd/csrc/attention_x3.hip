// Split-operand fused attention (precision "bf16x3" / "fp16x3").  Q, K, V arrive as 16-bit (hi, lo) PLANES of the fp32
// projections (split_planes_kernel below; plane = same (rows, ld) layout, lo plane `plane` elements after the hi plane);
// every product is three MFMAs accumulated in fp32:
//     S^T = Kh Qh^T + Kl Qh^T + Kh Ql^T,     O^T += Vh^T Ph^T + Vl^T Ph^T + Vh^T Pl^T   with P = (Ph, Pl) cut in registers
// Everything else is flash_attn_kernel (attention_bf16.hip; the shared steps are in attention_core.h): keys on the MFMA rows, softmax
// state in fp32 registers, K / V tiles by LDS-DMA into two stages (four tiles per stage: K hi, K lo, V hi, V lo), V read transposed out
// of its row-major tiles, deferred rescale.  Output fp32.  Replaces, in the split modes, QK^T GEMM + softmax_rows + transpose_v + PV GEMM
// over a materialised (B, H, T, T) score tensor: 8.2 of the 23.2 ms of a 32 x 10 s wav2vec2-base step went there.
#include "attention_core.h"

namespace svt {
namespace {

template <int DH, bool F16>
__global__ __launch_bounds__(256) void flash_attn_x3_kernel(const unsigned short* __restrict__ Q, long ldq, long q_bstride, long q_plane,
                                                            const unsigned short* __restrict__ K, const unsigned short* __restrict__ V,
                                                            long ldk, long k_bstride, long k_plane, float* __restrict__ O, long ldo,
                                                            long o_bstride, int T, int H, float c, int o_pairs) {
  typedef typename X3T<F16>::v8 v8;
  constexpr int NW = 4;
  constexpr int KSD = DH / 16, DB = DH / 32, CPR = DH / 8, RB = 2 * DH;
  constexpr int TILE16 = 64 * CPR;  // uint4 per tile
  // two stages of { K hi, K lo, V hi, V lo }
  __shared__ __attribute__((aligned(16))) uint4 KV[2][4 * TILE16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, h = blockIdx.y;
  const int q0 = blockIdx.x * (32 * NW) + wave * 32;
  const unsigned short* Qb = Q + (long)b * q_bstride + (long)h * DH;
  const unsigned short* Kb = K + (long)b * k_bstride + (long)h * DH;
  const unsigned short* Vb = V + (long)b * k_bstride + (long)h * DH;
  v8 qh[KSD], ql[KSD];
  {
    SVT_ATTN_Q_ROW(qp)
#pragma unroll
    for (int ks = 0; ks < KSD; ++ks) {
      qh[ks] = *(const v8*)(qp + ks * 16);
      ql[ks] = *(const v8*)(qp + q_plane + ks * 16);
    }
  }
  constexpr int DMA_PER_WAVE = CPR / NW;
  static_assert(DMA_PER_WAVE >= 1, "too many waves for the tile's fill");
  int dkey[DMA_PER_WAVE], kch[DMA_PER_WAVE], vch[DMA_PER_WAVE];
#pragma unroll
  for (int i = 0; i < DMA_PER_WAVE; ++i) SVT_ATTN_DMA_SRC(wave * DMA_PER_WAVE + i, dkey[i], kch[i], vch[i])
#define SVT_STAGE_X3(TILE, STAGE)                                                                                  \
  {                                                                                                                  \
    const int key0_ = (TILE) * 64;                                                                                   \
    _Pragma("unroll") for (int i = 0; i < DMA_PER_WAVE; ++i) {                                                       \
      int key_ = key0_ + dkey[i];                                                                                    \
      if (key_ > T - 1) key_ = T - 1;                                                                                \
      const unsigned short* kp_ = Kb + (long)key_ * ldk;                                                             \
      const unsigned short* vp_ = Vb + (long)key_ * ldk;                                                             \
      uint4* dst_ = &KV[STAGE][(wave * DMA_PER_WAVE + i) * 64];                                                      \
      __builtin_amdgcn_global_load_lds((gptr_t)(kp_ + kch[i]), (lptr_t)(dst_), 16, 0, 0);                            \
      __builtin_amdgcn_global_load_lds((gptr_t)(kp_ + k_plane + kch[i]), (lptr_t)(dst_ + TILE16), 16, 0, 0);        \
      __builtin_amdgcn_global_load_lds((gptr_t)(vp_ + vch[i]), (lptr_t)(dst_ + 2 * TILE16), 16, 0, 0);               \
      __builtin_amdgcn_global_load_lds((gptr_t)(vp_ + k_plane + vch[i]), (lptr_t)(dst_ + 3 * TILE16), 16, 0, 0);     \
    }                                                                                                                \
  }
  f32x16 o[DB];
#pragma unroll
  for (int i = 0; i < DB; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[i][r] = 0.f;
  float m = -1e30f, l = 0.f;
  const int hh = lane >> 5, kl = lane & 31;
  const int kg = (DH == 64) ? ((kl >> 1) & 7) : (kl & 15);
  const int ntiles = (T + 63) / 64;
  const char* vbase[DB];
  SVT_ATTN_VBASE(&KV[0][2 * TILE16])
  constexpr long STAGE_BYTES = (long)4 * TILE16 * 16;
  constexpr long PLANE_BYTES = (long)TILE16 * 16;
  SVT_STAGE_X3(0, 0)
  for (int tile = 0; tile < ntiles; ++tile) {
    const int st = tile & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tile + 1 < ntiles) {
      if (st) SVT_STAGE_X3(tile + 1, 0) else SVT_STAGE_X3(tile + 1, 1)
    }
    f32x16 s[2];
    v8 pfh[2][2], pfl[2][2];
    SVT_ATTN_X3_S(KV[st])
    SVT_ATTN_SOFTMAX_HEAD(tile, c)
    SVT_ATTN_X3_P
    SVT_ATTN_X3_PV(st)
  }
  const int q = q0 + (lane & 31);
  if (q >= T) return;
  const float inv = 1.f / l;
  float* op = O + (long)b * o_bstride + (long)q * ldo + (long)h * DH;
  SVT_ATTN_X3_STORE
}
#undef SVT_STAGE_X3

// Eight-wave staggered form of flash_attn_x3_kernel (round 4; see flash_attn_stag_kernel): three stages of { K hi, K lo, V hi, V lo }
// (96 KiB: one workgroup per CU, as before -- 172 registers), waves 4-7 half a tile behind waves 0-3, LDS-DMA from inline asm, 1-D
// grid with the query blocks of a (clip, head) on one XCD.  With ONE workgroup per CU the lockstep form had nobody to fill the matrix
// pipe during the softmax of its eight waves.
template <bool F16>
__global__ __launch_bounds__(512) void flash_attn_x3_stag_kernel(const unsigned short* __restrict__ Q, long ldq, long q_bstride, long q_plane,
                                                                 const unsigned short* __restrict__ K, const unsigned short* __restrict__ V,
                                                                 long ldk, long k_bstride, long k_plane, float* __restrict__ O, long ldo,
                                                                 long o_bstride, int T, int H, float c, int o_pairs, int nqb) {
  typedef typename X3T<F16>::v8 v8;
  constexpr int DH = 64, NW = 8, NST = 3;
  constexpr int KSD = DH / 16, DB = DH / 32, CPR = DH / 8, RB = 2 * DH;
  constexpr int TILE16 = 64 * CPR;           // uint4 per tile
  constexpr int STAGE16 = 4 * TILE16;        // K hi, K lo, V hi, V lo
  constexpr long STAGE_BYTES = (long)STAGE16 * 16;
  constexpr long PLANE_BYTES = (long)TILE16 * 16;
  extern __shared__ __attribute__((aligned(16))) uint4 KV[];   // NST * STAGE16 (96 KiB: dynamic)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int bh, qblk;
  attn_block_map(nqb, bh, qblk);
  const int b = bh / H, h = bh - b * H;
  const int q0 = qblk * (32 * NW) + wave * 32;
  const unsigned short* Qb = Q + (long)b * q_bstride + (long)h * DH;
  const unsigned short* Kb = K + (long)b * k_bstride + (long)h * DH;
  const unsigned short* Vb = V + (long)b * k_bstride + (long)h * DH;
  v8 qh[KSD], ql[KSD];
  {
    SVT_ATTN_Q_ROW(qp)
#pragma unroll
    for (int ks = 0; ks < KSD; ++ks) {
      qh[ks] = *(const v8*)(qp + ks * 16);
      ql[ks] = *(const v8*)(qp + q_plane + ks * 16);
    }
  }
  int dkey, kch, vch;
  SVT_ATTN_DMA_SRC(wave, dkey, kch, vch)
  const unsigned lds0 = lds_base(KV);
  auto stage_dma = [&](int tile, int stage) {
    int key = tile * 64 + dkey;
    if (key > T - 1) key = T - 1;
    const unsigned short* kp = Kb + (long)key * ldk;
    const unsigned short* vp = Vb + (long)key * ldk;
    const unsigned dst = lds0 + (unsigned)((stage * STAGE16 + wave * 64) * 16);
    attn_dma16(kp + kch, dst);
    attn_dma16(kp + k_plane + kch, dst + TILE16 * 16);
    attn_dma16(vp + vch, dst + 2 * TILE16 * 16);
    attn_dma16(vp + k_plane + vch, dst + 3 * TILE16 * 16);
  };
  f32x16 o[DB];
#pragma unroll
  for (int i = 0; i < DB; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[i][r] = 0.f;
  float m = -1e30f, l = 0.f;
  const int hh = lane >> 5, kl = lane & 31;
  const int kg = (kl >> 1) & 7;
  const int ntiles = (T + 63) / 64;
  const char* vbase[DB];
  SVT_ATTN_VBASE(&KV[2 * TILE16])
  f32x16 s[2];
  v8 pfh[2][2], pfl[2][2];
#define SVT_X3_BAR(J)                                                                                   \
  {                                                                                                     \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                    \
    __builtin_amdgcn_s_barrier();                                                                       \
    if ((J) + 1 < ntiles) stage_dma((J) + 1, st_next);                                                  \
  }
  stage_dma(0, 0);
  int st = 0;
  if (wave < 4) {
    for (int tile = 0; tile < ntiles; ++tile) {
      const int st_next = st + 1 == NST ? 0 : st + 1;
      SVT_X3_BAR(tile)
      SVT_ATTN_X3_S(KV + st * STAGE16)
      SVT_ATTN_SOFTMAX_HEAD(tile, c)
      SVT_ATTN_X3_P
      SVT_ATTN_X3_PV(st)
      st = st_next;
    }
  } else {
    {
      const int st_next = 1;
      SVT_X3_BAR(0)
    }
    for (int tile = 0; tile < ntiles; ++tile) {
      const int st1 = st + 1 == NST ? 0 : st + 1;
      SVT_ATTN_X3_S(KV + st * STAGE16)
      SVT_ATTN_SOFTMAX_HEAD(tile, c)
      SVT_ATTN_X3_P
      if (tile + 1 < ntiles) {
        const int st_next = st1 + 1 == NST ? 0 : st1 + 1;
        SVT_X3_BAR(tile + 1)
      }
      SVT_ATTN_X3_PV(st)
      st = st1;
    }
  }
#undef SVT_X3_BAR
  const int q = q0 + (lane & 31);
  if (q >= T) return;
  const float inv = 1.f / l;
  float* op = O + (long)b * o_bstride + (long)q * ldo + (long)h * DH;
  SVT_ATTN_X3_STORE
}

// fp32 (rows, cols) with row pitch ld_src -> 16-bit (hi, lo) planes (rows, cols) with row pitch ld_dst, lo plane `plane`
// elements after the hi plane; cols % 4 == 0
template <bool F16>
__global__ void split_planes_kernel(const float* __restrict__ src, long ld_src, long rows, int cols, unsigned short* __restrict__ dst,
                                    long ld_dst, long plane) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int c4 = cols / 4;
  if (i >= rows * c4) return;
  const long r = i / c4;
  const int c = (int)(i % c4) * 4;
  const float4 v = *(const float4*)(src + r * ld_src + c);
  const float x[4] = {v.x, v.y, v.z, v.w};
  unsigned short hi[4], lo[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) cut_piece<F16 ? 3 : 2>(x[j], hi[j], lo[j]);
  unsigned short* d = dst + r * ld_dst + c;
  *(uint2*)d = uint2{(unsigned)hi[0] | ((unsigned)hi[1] << 16), (unsigned)hi[2] | ((unsigned)hi[3] << 16)};
  *(uint2*)(d + plane) = uint2{(unsigned)lo[0] | ((unsigned)lo[1] << 16), (unsigned)lo[2] | ((unsigned)lo[3] << 16)};
}

// the kernels of one piece type (F16: IEEE half, else bf16); the two instantiations of a kernel have one signature
struct X3Kernels {
  decltype(&flash_attn_x3_kernel<64, false>) dh64, dh128;
  decltype(&flash_attn_x3_stag_kernel<false>) stag;
  decltype(&split_planes_kernel<false>) split;
};
template <bool F16> constexpr X3Kernels x3_kernels() {
  return {flash_attn_x3_kernel<64, F16>, flash_attn_x3_kernel<128, F16>, flash_attn_x3_stag_kernel<F16>, split_planes_kernel<F16>};
}
// kind = svt_precision: 3 = fp16 pieces, else bf16 pieces
inline X3Kernels x3_kernels(int kind) { return kind == 3 ? x3_kernels<true>() : x3_kernels<false>(); }

}  // namespace

int launch_split_planes(int kind, const float* src, long ld_src, long rows, int cols, void* dst, long ld_dst, long plane, hipStream_t s) {
  if (cols % 4 || ld_src % 4 || ld_dst % 4 || plane % 4) { set_error("split_planes: columns and pitches must be multiples of 4"); return -1; }
  const long n = rows * (cols / 4);
  hipLaunchKernelGGL(x3_kernels(kind).split, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, ld_src, rows, cols, (unsigned short*)dst, ld_dst, plane);
  SVT_LAUNCH_CHECK();
  return 0;
}

bool flash_attention_x3_ok(int dh) { return dh == 64 || dh == 128; }
// Q / K / V: 16-bit (hi, lo) planes (launch_split_planes); O fp32
int launch_flash_attention_x3(int kind, const void* Q, long ldq, long q_bstride, long q_plane, const void* K, const void* V, long ldk,
                              long k_bstride, long k_plane, float* O, long ldo, long o_bstride, int B, int T, int H, int dh, float scale,
                              hipStream_t s, int o_pairs) {
  if ((ldq | ldk | q_bstride | k_bstride | q_plane | k_plane) % 8 || (ldo | o_bstride) % 4) { set_error("flash_attention_x3: strides"); return -1; }
  if (o_pairs && ((ldo | o_bstride | dh) % 32 || ((uintptr_t)O & 127))) { set_error("flash_attention_x3: pair-row output needs strides in multiples of 32 elements"); return -1; }
  const float c = scale * 1.44269504088896340736f;
  const bool wide = dh == 64 && T > 128 && (long)B * H * ((T + 255) / 256) >= 512;
  const double flops = 4.0 * B * H * (double)T * T * dh;
  const unsigned short *q = (const unsigned short*)Q, *k = (const unsigned short*)K, *v = (const unsigned short*)V;
  const X3Kernels kn = x3_kernels(kind);
  auto lockstep = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3((T + 127) / 128, H, B), dim3(256), 0, s, q, ldq, q_bstride, q_plane, k, v, ldk, k_bstride, k_plane, O, ldo,
                       o_bstride, T, H, c, o_pairs);
  };
  prof_begin(s);
  if (wide) {
    const int nqb = (T + 255) / 256;
    const int lds_bytes = 3 * 4 * 512 * 16;   // three stages of four 8 KiB tiles
    if (int r_ = ensure_dyn_lds((const void*)kn.stag, lds_bytes)) return r_;
    hipLaunchKernelGGL(kn.stag, dim3((unsigned)(nqb * B * H)), dim3(512), lds_bytes, s, q, ldq, q_bstride, q_plane, k, v, ldk, k_bstride, k_plane, O,
                       ldo, o_bstride, T, H, c, o_pairs, nqb);
    g_flash_kernel_id = 8;
  }
  else if (dh == 64) { lockstep(kn.dh64); g_flash_kernel_id = 6; }
  else if (dh == 128) { lockstep(kn.dh128); g_flash_kernel_id = 7; }
  else { set_error("flash_attention_x3: head_dim must be 64 or 128"); return -1; }
  prof_end(s, flops, 0.0, 2);
  SVT_LAUNCH_CHECK();
  return 0;
}
}  // namespace svt
