// Coalesced epilogue of the one-tile LDS-DMA kernels (gemm_pp8.hip, gemm_x3s.hip; force-inlined into both).  After the MFMA
// loop a lane holds, per 16-row block, 16 consecutive columns of ONE row
// (lane & 15 = row): storing straight from registers makes every lane of a wave-instruction touch a different
// 128-byte line (one texture-addresser request per lane; measured 10-27 us per tile, ~45 % of the kernel).
// Instead each wave transposes its 16 x 64 block through a private LDS patch (row pitch 272 B: conflict-free both
// ways) and stores row-contiguous: 16 (fp32) / 8 (bf16) consecutive lanes cover whole 128-byte lines.  Bias,
// activation and the fp32 residual are applied on the read-back side with the same coalesced addressing.
#pragma once
#include "gemm_ring.h"
#include <utility>

namespace svt {
namespace {

// this lane's bias values on the read-back side of epilogue_block (column base c4 = (lane & 15) * 4 for fp32 output,
// c8 = (lane & 7) * 8 for bf16): loaded ONCE per wave and tile, not once per 16-row block (eight dependent L2 round trips)
struct BiasRegs { float v[8]; };
template <bool OUT32>
__device__ __forceinline__ BiasRegs load_bias_regs(const GemmArgs& p, const float* bias, int lane, int wn, int n0) {
  BiasRegs b;
#pragma unroll
  for (int j = 0; j < 8; ++j) b.v[j] = 0.f;
  const int n = n0 + wn * 64 + (OUT32 ? (lane & 15) * 4 : (lane & 7) * 8);
  if (bias && n < p.N) {
    const float4 b0 = *(const float4*)(bias + n);
    b.v[0] = b0.x; b.v[1] = b0.y; b.v[2] = b0.z; b.v[3] = b0.w;
    if (!OUT32) {
      const float4 b1 = *(const float4*)(bias + n + 4);
      b.v[4] = b1.x; b.v[5] = b1.y; b.v[6] = b1.z; b.v[7] = b1.w;
    }
  }
  return b;
}

template <int MB, int BM, bool OUT32>
__device__ __forceinline__ void epilogue_block(const GemmArgs& p, const f32x4& a0, const f32x4& a1, const f32x4& a2,
                                               const f32x4& a3, int mb, float* patch, int lane, int wm, int wn, int m0,
                                               int n0, long coff, const BiasRegs& br) {
  constexpr int PITCH = 68;  // floats
  const int m16 = lane & 15, q = lane >> 4;
  constexpr bool out32 = OUT32;
  {
    const f32x4 accs[4] = {a0, a1, a2, a3};
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
      f32x4 v = accs[nb];
      v[0] *= p.alpha; v[1] *= p.alpha; v[2] *= p.alpha; v[3] *= p.alpha;
      *(f32x4*)(patch + m16 * PITCH + q * 16 + nb * 4) = v;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int mbase = m0 + wm * (BM / 2) + mb * 16;
    if (out32) {
      const int c4 = (lane & 15) * 4;
      const int n = n0 + wn * 64 + c4;
      const float4 b4 = float4{br.v[0], br.v[1], br.v[2], br.v[3]};
#pragma unroll
      for (int pass = 0; pass < 4; ++pass) {
        const int r = pass * 4 + (lane >> 4);
        const int m = mbase + r;
        float4 v = *(const float4*)(patch + r * PITCH + c4);
        if (m < p.M && n < p.N) {
          v.x = apply_act(v.x + b4.x, p.act); v.y = apply_act(v.y + b4.y, p.act);
          v.z = apply_act(v.z + b4.z, p.act); v.w = apply_act(v.w + b4.w, p.act);
          const long idx = coff + (long)m * p.ldc + n;
          if (p.resid) {
            const float4 r4 = *(const float4*)(p.resid + idx);
            v.x += r4.x; v.y += r4.y; v.z += r4.z; v.w += r4.w;
          }
          if (p.planes) {   // (hi, lo) planes instead of fp32 (GemmArgs::planes): 8 + 8 bytes per lane, whole 128-byte lines per row
            const float x[4] = {v.x, v.y, v.z, v.w};
            unsigned short hi[4], lo[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              if (p.planes_f16) cut_piece<3>(x[j], hi[j], lo[j]);
              else cut_piece<2>(x[j], hi[j], lo[j]);
            }
            *(uint2*)(p.planes + idx) = uint2{(unsigned)hi[0] | ((unsigned)hi[1] << 16), (unsigned)hi[2] | ((unsigned)hi[3] << 16)};
            *(uint2*)(p.planes + p.plane_stride + idx) = uint2{(unsigned)lo[0] | ((unsigned)lo[1] << 16), (unsigned)lo[2] | ((unsigned)lo[3] << 16)};
          } else {
            *(float4*)((float*)p.C + idx) = v;
          }
        }
      }
    } else {
      const int c8 = (lane & 7) * 8;
      const int n = n0 + wn * 64 + c8;
      float bb[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) bb[j] = br.v[j];
#pragma unroll
      for (int pass = 0; pass < 2; ++pass) {
        const int r = pass * 8 + (lane >> 3);
        const int m = mbase + r;
        const float4 v0 = *(const float4*)(patch + r * PITCH + c8), v1 = *(const float4*)(patch + r * PITCH + c8 + 4);
        if (m < p.M && n < p.N) {
          float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
          const long idx = coff + (long)m * p.ldc + n;
          if (p.resid) {
            const float4 r0 = *(const float4*)(p.resid + idx), r1 = *(const float4*)(p.resid + idx + 4);
            const float rr[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = apply_act(v[j] + bb[j], p.act) + rr[j];
          } else if (p.act == ACT_GELU) {
            f32x2_t g[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) g[j] = f32x2_t{v[2 * j] + bb[2 * j], v[2 * j + 1] + bb[2 * j + 1]};
            gelu_bf16x2_x4(g);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              v[2 * j] = g[j].x;
              v[2 * j + 1] = g[j].y;
            }
          } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = apply_act(v[j] + bb[j], p.act);
          }
          bf16x8 o;
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] = (bf16_t)v[j];
          *(bf16x8*)((bf16_t*)p.C + idx) = o;
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

template <int MB, int BM, bool OUT32, int... I>
__device__ __forceinline__ void epilogue_seq(std::integer_sequence<int, I...>, const GemmArgs& p, f32x4 (&acc)[4][MB],
                                             float* patch, int lane, int wm, int wn, int m0, int n0, long coff,
                                             const float* bias) {
  const BiasRegs br = load_bias_regs<OUT32>(p, bias, lane, wn, n0);
  // fold over compile-time block indices: every acc[][] index is static (a runtime-indexed accumulator array
  // would be demoted to scratch)
  (epilogue_block<MB, BM, OUT32>(p, acc[0][I], acc[1][I], acc[2][I], acc[3][I], I, patch, lane, wm, wn, m0, n0, coff, br),
   ...);
}

template <int MB, int BM>
__device__ __forceinline__ void epilogue_coalesced(const GemmArgs& p, f32x4 (&acc)[4][MB], float* patch, int lane, int wm,
                                                   int wn, int m0, int n0, long coff, const float* bias) {
  if (p.out_f32)
    epilogue_seq<MB, BM, true>(std::make_integer_sequence<int, MB>{}, p, acc, patch, lane, wm, wn, m0, n0, coff, bias);
  else
    epilogue_seq<MB, BM, false>(std::make_integer_sequence<int, MB>{}, p, acc, patch, lane, wm, wn, m0, n0, coff, bias);
}

}  // namespace
}  // namespace svt
