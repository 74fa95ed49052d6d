// Row LayerNorm in its six forms (fp32 / 16-bit rows, pair rows of the split-operand modes, the (hi, lo) bf16 residual stream) and the
// launchers that choose among them.  HBM-bound; a wave or half a wave owns a row.
#include "device_util.h"
#include <type_traits>

namespace svt {
namespace {
// Row LayerNorm: one wave per row, two-pass statistics from registers-free re-reads (rows <= 4 KB
// stay in L1/L2).  Optional exact-erf GELU (conv "layer" mode).
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void layernorm_kernel(const TI* x, const float* add, float* sumF, int64_t rows, int D,
                                                        const float* gamma, const float* beta, float eps, int gelu,
                                                        TO* yT, float* yF) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const TI* xr = x + row * D;
  const float* ar = add ? add + row * D : nullptr;
  float s = 0.f;
  for (int i = lane; i < D; i += 64) s += ld<TI>(xr, i) + (ar ? ar[i] : 0.f);
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
  for (int i = lane; i < D; i += 64) { const float d = ld<TI>(xr, i) + (ar ? ar[i] : 0.f) - mean; q += d * d; }
  const float rstd = rsqrtf(wave_sum(q) / (float)D + eps);
  for (int i = lane; i < D; i += 64) {
    const float xv = ld<TI>(xr, i) + (ar ? ar[i] : 0.f);
    if (sumF) sumF[row * D + i] = xv;
    float v = (xv - mean) * rstd * gamma[i] + beta[i];
    if (gelu) v = gelu_erf(v);
    if (yT) st<TO>(yT, row * D + i, v);
    if (yF) yF[row * D + i] = v;
  }
}

// Register-resident variant for D = 64*VPT (512 / 768 / 1024): the row is read ONCE with 16-byte loads
// (fp32 in) and kept in VPT registers per lane; statistics by two in-register passes + wave shuffles.
// PK != 0: additionally (or only) writes the result as pair rows into yP (the next split-operand product's operand)
template <int VPT, typename TO, typename TI = float, int PK = 0>
__global__ __launch_bounds__(256) void layernorm_f32_vec_kernel(const TI* x, const float* add, float* sumF,
                                                                int64_t rows, const float* gamma, const float* beta,
                                                                float eps, int gelu, TO* yT, float* yF, void* yP = nullptr,
                                                                const void* addP = nullptr) {
  constexpr int D = 64 * VPT, NV = VPT / 4;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float v[VPT];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    float4 t;
    if constexpr (sizeof(TI) == 4) {
      t = ((const float4*)(x + row * D))[lane + 64 * j];
    } else {
      const bf16x4 tb = ((const bf16x4*)(x + row * D))[lane + 64 * j];
      t = float4{(float)tb[0], (float)tb[1], (float)tb[2], (float)tb[3]};
    }
    if (add) {
      const float4 a = ((const float4*)(add + row * D))[lane + 64 * j];
      t.x += a.x; t.y += a.y; t.z += a.z; t.w += a.w;
    }
    if constexpr (PK != 0) {
      if (addP) {   // the addend as pair rows (the post-LN residual stream of the split modes: hi + lo = 22 mantissa bits)
        const int64_t e = row * D + (lane + 64 * j) * 4;
        const char* pp = (const char*)addP + (e >> 5) * 128 + (e & 31) * 2;
        const uint2 h = *(const uint2*)pp, l = *(const uint2*)(pp + 64);
        const unsigned hw[2] = {h.x, h.y}, lw[2] = {l.x, l.y};
        float a[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const unsigned short hs = (unsigned short)(hw[i >> 1] >> (16 * (i & 1))), ls = (unsigned short)(lw[i >> 1] >> (16 * (i & 1)));
          if constexpr (PK == 3) a[i] = (float)__builtin_bit_cast(_Float16, hs) + (float)__builtin_bit_cast(_Float16, ls);
          else a[i] = (float)__builtin_bit_cast(__bf16, hs) + (float)__builtin_bit_cast(__bf16, ls);
        }
        t.x += a[0]; t.y += a[1]; t.z += a[2]; t.w += a[3];
      }
    }
    if (sumF) ((float4*)(sumF + row * D))[lane + 64 * j] = t;
    v[4 * j] = t.x; v[4 * j + 1] = t.y; v[4 * j + 2] = t.z; v[4 * j + 3] = t.w;
    s += (t.x + t.y) + (t.z + t.w);
  }
  const float mean = wave_sum(s) * (1.f / D);
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < VPT; ++i) { v[i] -= mean; q = fmaf(v[i], v[i], q); }
  const float rstd = rsqrtf(wave_sum(q) * (1.f / D) + eps);
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int c = (lane + 64 * j) * 4;
    const float4 g = *(const float4*)(gamma + c), b = *(const float4*)(beta + c);
    float o0 = fmaf(v[4 * j] * rstd, g.x, b.x), o1 = fmaf(v[4 * j + 1] * rstd, g.y, b.y);
    float o2 = fmaf(v[4 * j + 2] * rstd, g.z, b.z), o3 = fmaf(v[4 * j + 3] * rstd, g.w, b.w);
    if (gelu) {
      if (sizeof(TO) == 2 && PK == 0 && !yF) {
        // results stored ONLY in 16 bits (the conv stack of the layer-norm extractor in the throughput modes): the polynomial GELU of the GEMM
        // epilogues (common.h) -- with the exact-erf form (rcp + exp: quarter-rate instructions) this pass ran at 3.7 TB/s, VALU-bound
        f32x2_t ga = {o0, o1}, gb = {o2, o3};
        ga = gelu_bf16x2(ga); gb = gelu_bf16x2(gb);
        o0 = ga.x; o1 = ga.y; o2 = gb.x; o3 = gb.y;
      } else {
        o0 = gelu_erf(o0); o1 = gelu_erf(o1); o2 = gelu_erf(o2); o3 = gelu_erf(o3);
      }
    }
    if (yT) {
      if constexpr (sizeof(TO) == 2) {
        bf16x4 o;
        o[0] = (bf16_t)o0; o[1] = (bf16_t)o1; o[2] = (bf16_t)o2; o[3] = (bf16_t)o3;
        *(bf16x4*)((bf16_t*)yT + row * D + c) = o;
      } else {
        *(float4*)((float*)yT + row * D + c) = float4{o0, o1, o2, o3};
      }
    }
    if (yF) *(float4*)(yF + row * D + c) = float4{o0, o1, o2, o3};
    if constexpr (PK != 0) {
      const float ov[4] = {o0, o1, o2, o3};
      store_pairs<PK, 4>(yP, row * D + c, ov);
    }
  }
}

// LayerNorm (+ GELU) over rows stored in the 16-bit operand type, half a wave per row, 16-byte accesses: the conv stack of the
// layer-norm extractor in the throughput modes normalises the conv GEMM's output in place (2 bytes read + 2 written per element; with
// a wave per row and 8-byte accesses the pass ran at 3.8 TB/s).
template <int D>
__global__ __launch_bounds__(256) void layernorm_op16_rows2_kernel(const bf16_t* x, int64_t rows, const float* gamma, const float* beta,
                                                                   float eps, int gelu, bf16_t* y) {
  constexpr int NC = D / 256;
  const int lane = threadIdx.x & 63, sub = lane & 31;
  const int64_t row = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 6) * 2 + (lane >> 5);
  if (row >= rows) return;
  float v[NC][8];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const bf16x8 h = *(const bf16x8*)(x + row * D + (sub + 32 * j) * 8);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[j][i] = (float)h[i];
    s += ((v[j][0] + v[j][1]) + (v[j][2] + v[j][3])) + ((v[j][4] + v[j][5]) + (v[j][6] + v[j][7]));
  }
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  const float mean = s * (1.f / D);
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < NC; ++j)
#pragma unroll
    for (int i = 0; i < 8; ++i) { v[j][i] -= mean; q = fmaf(v[j][i], v[j][i], q); }
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
  const float rstd = rsqrtf(q * (1.f / D) + eps);
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const int c = (sub + 32 * j) * 8;
    const float4 g0 = *(const float4*)(gamma + c), g1 = *(const float4*)(gamma + c + 4);
    const float4 b0 = *(const float4*)(beta + c), b1 = *(const float4*)(beta + c + 4);
    const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w}, bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
    f32x2_t o2[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) o2[i] = f32x2_t{fmaf(v[j][2 * i] * rstd, gg[2 * i], bb[2 * i]), fmaf(v[j][2 * i + 1] * rstd, gg[2 * i + 1], bb[2 * i + 1])};
    if (gelu) gelu_bf16x2_x4(o2);
    bf16x8 ob;
#pragma unroll
    for (int i = 0; i < 4; ++i) { ob[2 * i] = (bf16_t)o2[i].x; ob[2 * i + 1] = (bf16_t)o2[i].y; }
    *(bf16x8*)(y + row * D + c) = ob;
  }
}

// D = 512 / 768 / 1024, the widths the register-resident kernels exist for (the caller has checked D): f(integral_constant<int, VPT>),
// VPT = D / 64 = the values a lane holds when a wave owns a row
template <class F> void ln_width(int D, F&& f) {
  if (D == 512) f(std::integral_constant<int, 8>{});
  else if (D == 768) f(std::integral_constant<int, 12>{});
  else f(std::integral_constant<int, 16>{});
}
}  // namespace
int g_ln_two_rows = 1;   // svt_debug_set key 20: 0 = one row per wave in the (hi, lo) and 16-bit-row LayerNorms (A/B)
int g_ln_kernel_id = 0;  // svt_debug_set key 40 (query): 1000 * kernel + instantiation of the last launch (include/svt_mi355.h lists the ids)
int launch_layernorm(const LnArgs& a, hipStream_t s) {
  const int prec = a.prec, x_is_f32 = a.x_is_f32, D = a.D, gelu = a.gelu, pair_kind = a.pair_kind;
  const void *const x = a.x, *const addP = a.addP;
  const int64_t rows = a.rows;
  const float *const gamma = a.gamma, *const beta = a.beta, *const add = a.add;
  const float eps = a.eps;
  void *const yT = a.yT, *const yP = a.yP;
  float *const yF = a.yF, *const sumF = a.sumF;
  if (addP && !yP) { set_error("layernorm: a pair-row addend needs the pair-row output form"); return -1; }
  const dim3 grid((unsigned)((rows + 3) / 4)), grid2((unsigned)((rows + 7) / 8)), block(256);
  const bool wide = D == 512 || D == 768 || D == 1024;
  if (yP) {
    // split-operand modes: the result leaves as pair rows (and optionally as fp32: yF / sumF) -- fp32 input, D in {512, 768, 1024}
    if (prec || !x_is_f32 || yT || !wide || (pair_kind != 2 && pair_kind != 3) || !aligned(15, x, yF, add, sumF, gamma, beta) || !aligned(127, yP)) { set_error("layernorm: the pair-row output needs an fp32 input, D in {512, 768, 1024} and aligned buffers"); return -1; }
    g_ln_kernel_id = pair_kind == 3 ? 2300 : 2200;
    ln_width(D, [&](auto vpt) {
      constexpr int VPT = decltype(vpt)::value;
      if (pair_kind == 3) hipLaunchKernelGGL((layernorm_f32_vec_kernel<VPT, float, float, 3>), grid, block, 0, s, (const float*)x, add, sumF, rows, gamma, beta, eps, gelu, (float*)nullptr, yF, yP, addP);
      else hipLaunchKernelGGL((layernorm_f32_vec_kernel<VPT, float, float, 2>), grid, block, 0, s, (const float*)x, add, sumF, rows, gamma, beta, eps, gelu, (float*)nullptr, yF, yP, addP);
    });
  } else if (prec && !x_is_f32 && wide && yT && !yF && !add && !sumF && g_ln_two_rows && aligned(15, x, yT, gamma, beta)) {
    // 16-bit rows in, 16-bit rows out (in place for the conv stack of the layer-norm extractor): half a wave per row
    g_ln_kernel_id = 3000;
    ln_width(D, [&](auto vpt) {
      hipLaunchKernelGGL((layernorm_op16_rows2_kernel<64 * decltype(vpt)::value>), grid2, block, 0, s, (const bf16_t*)x, rows, gamma, beta, eps, gelu, (bf16_t*)yT);
    });
  } else if (prec && !x_is_f32 && wide && aligned(7, x) && aligned(15, yT, yF, add, sumF)) {
    // bf16 branch output + fp32 residual (throughput mode)
    g_ln_kernel_id = 2011;
    ln_width(D, [&](auto vpt) {
      hipLaunchKernelGGL((layernorm_f32_vec_kernel<decltype(vpt)::value, bf16_t, bf16_t>), grid, block, 0, s, (const bf16_t*)x, add, sumF, rows, gamma, beta, eps, gelu, (bf16_t*)yT, yF);
    });
  } else if (add && !x_is_f32) {
    set_error("layernorm: the addend form needs an fp32 input (or bf16 with D in {512,768,1024})");
    return -1;
  } else if (x_is_f32 && wide && aligned(15, x, yT, yF, gamma, beta, add, sumF)) {
    g_ln_kernel_id = prec ? 2001 : 2000;
    ln_width(D, [&](auto vpt) {
      constexpr int VPT = decltype(vpt)::value;
      if (prec) hipLaunchKernelGGL((layernorm_f32_vec_kernel<VPT, bf16_t>), grid, block, 0, s, (const float*)x, add, sumF, rows, gamma, beta, eps, gelu, (bf16_t*)yT, yF);
      else hipLaunchKernelGGL((layernorm_f32_vec_kernel<VPT, float>), grid, block, 0, s, (const float*)x, add, sumF, rows, gamma, beta, eps, gelu, (float*)yT, yF);
    });
  } else if (!prec) {
    g_ln_kernel_id = 1000;
    hipLaunchKernelGGL((layernorm_kernel<float, float>), grid, block, 0, s, (const float*)x, add, sumF, rows, D, gamma, beta, eps, gelu, (float*)yT, yF);
  } else if (x_is_f32) {
    g_ln_kernel_id = 1001;
    hipLaunchKernelGGL((layernorm_kernel<float, bf16_t>), grid, block, 0, s, (const float*)x, add, sumF, rows, D, gamma, beta, eps, gelu, (bf16_t*)yT, yF);
  } else {
    g_ln_kernel_id = 1011;
    hipLaunchKernelGGL((layernorm_kernel<bf16_t, bf16_t>), grid, block, 0, s, (const bf16_t*)x, add, sumF, rows, D, gamma, beta, eps, gelu, (bf16_t*)yT, yF);
  }
  SVT_LAUNCH_CHECK();
  return 0;
}

namespace {
// Post-LN residual stream kept as a bf16 pair (hi = the operand copy the next GEMM reads anyway, lo = bf16(x - hi):
// 16 mantissa bits, 2^-17 relative) instead of an extra fp32 copy: y = LN(branch + hi + lo) -> (hi', lo').  Per
// element 6 bytes read + 4 written instead of 6 + 6 (the kernel is at the HBM roofline, so -17 % bytes = -17 % time).
// yF (optional) also receives the full fp32 result (last layer: the whole-batch output norm reads it).
template <int VPT>
__global__ __launch_bounds__(256) void layernorm_hilo_kernel(const bf16_t* branch, const bf16_t* rh, const bf16_t* rl,
                                                             int64_t rows, const float* gamma, const float* beta, float eps,
                                                             bf16_t* yh, bf16_t* yl, float* yF) {
  constexpr int D = 64 * VPT, NV = VPT / 4;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float v[VPT];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const long o = row * D + (lane + 64 * j) * 4;
    const bf16x4 h = *(const bf16x4*)(rh + o), l = *(const bf16x4*)(rl + o);
    float4 t = float4{(float)h[0] + (float)l[0], (float)h[1] + (float)l[1], (float)h[2] + (float)l[2], (float)h[3] + (float)l[3]};
    if (branch) {
      const bf16x4 a = *(const bf16x4*)(branch + o);
      t.x += (float)a[0]; t.y += (float)a[1]; t.z += (float)a[2]; t.w += (float)a[3];
    }
    v[4 * j] = t.x; v[4 * j + 1] = t.y; v[4 * j + 2] = t.z; v[4 * j + 3] = t.w;
    s += (t.x + t.y) + (t.z + t.w);
  }
  const float mean = wave_sum(s) * (1.f / D);
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < VPT; ++i) { v[i] -= mean; q = fmaf(v[i], v[i], q); }
  const float rstd = rsqrtf(wave_sum(q) * (1.f / D) + eps);
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int c = (lane + 64 * j) * 4;
    const float4 g = *(const float4*)(gamma + c), b = *(const float4*)(beta + c);
    const float o[4] = {fmaf(v[4 * j] * rstd, g.x, b.x), fmaf(v[4 * j + 1] * rstd, g.y, b.y),
                        fmaf(v[4 * j + 2] * rstd, g.z, b.z), fmaf(v[4 * j + 3] * rstd, g.w, b.w)};
    bf16x4 oh, ol;
#pragma unroll
    for (int i = 0; i < 4; ++i) { oh[i] = (bf16_t)o[i]; ol[i] = (bf16_t)(o[i] - (float)oh[i]); }
    *(bf16x4*)(yh + row * D + c) = oh;
    *(bf16x4*)(yl + row * D + c) = ol;
    if (yF) *(float4*)(yF + row * D + c) = float4{o[0], o[1], o[2], o[3]};
  }
}

// Two rows per wave (round 4): a HALF-wave owns a row and every access is 16 bytes (8 bf16 per lane), so a 768-wide row is three
// accesses per stream and lane instead of three 8-byte ones over twice the lanes, and the two reductions run over five exchange steps
// instead of six: 23.2 -> 20.5 us per pass at 32 x 10 s (HBM-bound: the same bytes at a higher achieved rate).  The sums are taken in a
// different order than in the one-row kernel, which moves near-tie frames of the bf16 mode (tests/test_gpu_parity.py
// check_16bit_mode_bound holds the mode to the operand-rounding simulation, not to one summation order).
// PARTS: the branch arrives as `nparts` fp32 partial products of a K-split GEMM (gemm_skinny.hip, ksplit) + its bias: they are added in
// part order, the bias last, and the sum is rounded to the operand type -- the value the un-split GEMM's epilogue would have stored
// (same rounding points as the 16-bit modes' stored-activation simulation, tools/sim_split.py)
template <int D, bool PARTS = false>
__global__ __launch_bounds__(256) void layernorm_hilo2_kernel(const bf16_t* branch, const bf16_t* rh, const bf16_t* rl,
                                                              int64_t rows, const float* gamma, const float* beta, float eps,
                                                              bf16_t* yh, bf16_t* yl, float* yF, const float* parts = nullptr, int nparts = 0,
                                                              long part_stride = 0, const float* pbias = nullptr) {
  constexpr int NC = D / 256;   // 16-byte chunks (8 elements) per lane: 32 lanes x NC x 8 = D
  const int lane = threadIdx.x & 63, sub = lane & 31;
  const int64_t row = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 6) * 2 + (lane >> 5);
  if (row >= rows) return;
  float v[NC][8];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const long o = row * D + (sub + 32 * j) * 8;
    const bf16x8 h = *(const bf16x8*)(rh + o), l = *(const bf16x8*)(rl + o);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[j][i] = (float)h[i] + (float)l[i];
    if constexpr (PARTS) {
      float a[8];
      {
        const float4 t0 = *(const float4*)(parts + o), t1 = *(const float4*)(parts + o + 4);
        a[0] = t0.x; a[1] = t0.y; a[2] = t0.z; a[3] = t0.w; a[4] = t1.x; a[5] = t1.y; a[6] = t1.z; a[7] = t1.w;
      }
      for (int k = 1; k < nparts; ++k) {
        const float4 t0 = *(const float4*)(parts + k * part_stride + o), t1 = *(const float4*)(parts + k * part_stride + o + 4);
        a[0] += t0.x; a[1] += t0.y; a[2] += t0.z; a[3] += t0.w; a[4] += t1.x; a[5] += t1.y; a[6] += t1.z; a[7] += t1.w;
      }
      const int c = (sub + 32 * j) * 8;
      const float4 b0 = *(const float4*)(pbias + c), b1 = *(const float4*)(pbias + c + 4);
      const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
      for (int i = 0; i < 8; ++i) v[j][i] += (float)(bf16_t)(a[i] + bb[i]);
    } else if (branch) {
      const bf16x8 a = *(const bf16x8*)(branch + o);
#pragma unroll
      for (int i = 0; i < 8; ++i) v[j][i] += (float)a[i];
    }
    s += ((v[j][0] + v[j][1]) + (v[j][2] + v[j][3])) + ((v[j][4] + v[j][5]) + (v[j][6] + v[j][7]));
  }
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  const float mean = s * (1.f / D);
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < NC; ++j)
#pragma unroll
    for (int i = 0; i < 8; ++i) { v[j][i] -= mean; q = fmaf(v[j][i], v[j][i], q); }
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
  const float rstd = rsqrtf(q * (1.f / D) + eps);
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const int c = (sub + 32 * j) * 8;
    const float4 g0 = *(const float4*)(gamma + c), g1 = *(const float4*)(gamma + c + 4);
    const float4 b0 = *(const float4*)(beta + c), b1 = *(const float4*)(beta + c + 4);
    const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w}, bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
    float o[8];
    bf16x8 oh, ol;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      o[i] = fmaf(v[j][i] * rstd, gg[i], bb[i]);
      oh[i] = (bf16_t)o[i];
      ol[i] = (bf16_t)(o[i] - (float)oh[i]);
    }
    *(bf16x8*)(yh + row * D + c) = oh;
    *(bf16x8*)(yl + row * D + c) = ol;
    if (yF) {
      *(float4*)(yF + row * D + c) = float4{o[0], o[1], o[2], o[3]};
      *(float4*)(yF + row * D + c + 4) = float4{o[4], o[5], o[6], o[7]};
    }
  }
}
// fp32 -> (hi, lo) bf16 pair with a LayerNorm in front (first LN of the post-LN encoder): x fp32 in
template <int VPT>
__global__ __launch_bounds__(256) void layernorm_f32_to_hilo_kernel(const float* x, int64_t rows, const float* gamma,
                                                                    const float* beta, float eps, bf16_t* yh, bf16_t* yl) {
  constexpr int D = 64 * VPT, NV = VPT / 4;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float v[VPT];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const float4 t = ((const float4*)(x + row * D))[lane + 64 * j];
    v[4 * j] = t.x; v[4 * j + 1] = t.y; v[4 * j + 2] = t.z; v[4 * j + 3] = t.w;
    s += (t.x + t.y) + (t.z + t.w);
  }
  const float mean = wave_sum(s) * (1.f / D);
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < VPT; ++i) { v[i] -= mean; q = fmaf(v[i], v[i], q); }
  const float rstd = rsqrtf(wave_sum(q) * (1.f / D) + eps);
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int c = (lane + 64 * j) * 4;
    const float4 g = *(const float4*)(gamma + c), b = *(const float4*)(beta + c);
    const float o[4] = {fmaf(v[4 * j] * rstd, g.x, b.x), fmaf(v[4 * j + 1] * rstd, g.y, b.y),
                        fmaf(v[4 * j + 2] * rstd, g.z, b.z), fmaf(v[4 * j + 3] * rstd, g.w, b.w)};
    bf16x4 oh, ol;
#pragma unroll
    for (int i = 0; i < 4; ++i) { oh[i] = (bf16_t)o[i]; ol[i] = (bf16_t)(o[i] - (float)oh[i]); }
    *(bf16x4*)(yh + row * D + c) = oh;
    *(bf16x4*)(yl + row * D + c) = ol;
  }
}
}  // namespace
bool layernorm_hilo_ok(int D) { return D == 512 || D == 768 || D == 1024; }
int launch_layernorm_hilo_parts(const float* parts, int nparts, long part_stride, const float* pbias, const bf16_t* rh, const bf16_t* rl, int64_t rows,
                                int D, const float* gamma, const float* beta, float eps, bf16_t* yh, bf16_t* yl, float* yF, hipStream_t s) {
  if (!parts || nparts < 1 || !pbias || !(D == 512 || D == 768 || D == 1024) || (part_stride & 3) || !aligned(15, parts, pbias, rh, rl, yh, yl, yF, gamma, beta)) { set_error("layernorm (K-split branch): D in {512, 768, 1024} and 16-byte aligned buffers"); return -1; }
  const dim3 grid2((unsigned)((rows + 7) / 8)), block(256);
  g_ln_kernel_id = 5001;
  ln_width(D, [&](auto vpt) {
    hipLaunchKernelGGL((layernorm_hilo2_kernel<64 * decltype(vpt)::value, true>), grid2, block, 0, s, nullptr, rh, rl, rows, gamma, beta, eps, yh, yl, yF, parts, nparts, part_stride, pbias);
  });
  SVT_LAUNCH_CHECK();
  return 0;
}
// branch == nullptr && x32 != nullptr: y = LN(x32);  otherwise y = LN(branch + rh + rl)
int launch_layernorm_hilo(const bf16_t* branch, const bf16_t* rh, const bf16_t* rl, const float* x32, int64_t rows, int D,
                          const float* gamma, const float* beta, float eps, bf16_t* yh, bf16_t* yl, float* yF, hipStream_t s) {
  const dim3 grid((unsigned)((rows + 3) / 4)), grid2((unsigned)((rows + 7) / 8)), block(256);
  g_ln_kernel_id = x32 ? 6000 : g_ln_two_rows && aligned(15, branch, rh, rl, yh, yl, yF, gamma, beta) ? 5000 : 4000;
  ln_width(D, [&](auto vpt) {
    constexpr int VPT = decltype(vpt)::value;
    if (x32) hipLaunchKernelGGL((layernorm_f32_to_hilo_kernel<VPT>), grid, block, 0, s, x32, rows, gamma, beta, eps, yh, yl);
    else if (g_ln_two_rows && aligned(15, branch, rh, rl, yh, yl, yF, gamma, beta)) hipLaunchKernelGGL((layernorm_hilo2_kernel<64 * VPT>), grid2, block, 0, s, branch, rh, rl, rows, gamma, beta, eps, yh, yl, yF);
    else hipLaunchKernelGGL((layernorm_hilo_kernel<VPT>), grid, block, 0, s, branch, rh, rl, rows, gamma, beta, eps, yh, yl, yF);
  });
  SVT_LAUNCH_CHECK();
  return 0;
}

}  // namespace svt
