// conv layer 0 (one input channel, 10 taps) on the vector ALU, fused with its norm and GELU: "group" mode applies the coefficients that
// stats.hip folds the GroupNorm into, "layer" mode normalises over the channels in the same kernel.  conv0_mfma.hip holds the matrix-pipe
// forms of both for the 16-bit modes.  The fp32 <-> pair-row re-layouts are here too: see below.
#include "device_util.h"

namespace svt {
namespace {
// out[b,t,c] = gelu( sum_j coef[b,c,j] * wav[b, t*stride + j] + coef[b,c,K0] ), channels-last.
// One wave writes whole (b,t) rows: lane = 8 consecutive channels -> 16 B (bf16) / 32 B (fp32) per lane.
template <typename TO, int PK = 0>   // PK != 0 (TO = float): the output is written as pair rows
__global__ __launch_bounds__(256) void conv0_group_apply_kernel(const float* wav, int64_t L, int stride, int64_t T1,
                                                                int C, const float* coef, TO* out) {
  constexpr int FPW = 32;  // frames per wave
  __shared__ float xs[4][FPW * 5 + 16];  // stride <= 5 supported by this tile size
  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t t0 = ((int64_t)blockIdx.x * 4 + wave) * FPW;
  if (t0 >= T1) return;
  const float* x = wav + (int64_t)b * L;
  const int nfr = (int)((T1 - t0 < FPW) ? (T1 - t0) : FPW);
  const int ns = (nfr - 1) * stride + K0;
  for (int i = lane; i < ns; i += 64) xs[wave][i] = x[t0 * stride + i];
  // (wave-private LDS region: no block barrier needed, but the wave must see its own writes)
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  const int c0 = lane * 8;
  if (c0 >= C) return;
  float cf[8][K0 + 1];
  const float* cp = coef + ((int64_t)b * C + c0) * (K0 + 1);
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j <= K0; ++j) cf[i][j] = cp[i * (K0 + 1) + j];
  for (int f = 0; f < nfr; ++f) {
    float xv[K0];
#pragma unroll
    for (int j = 0; j < K0; ++j) xv[j] = xs[wave][f * stride + j];
    float o[8];
    f32x2_t a4[4];
#pragma unroll
    for (int i = 0; i < 8; i += 2) {
      f32x2_t a = {cf[i][K0], cf[i + 1][K0]};
#pragma unroll
      for (int j = 0; j < K0; ++j) a = f32x2_t{cf[i][j], cf[i + 1][j]} * xv[j] + a;
      a4[i >> 1] = a;
    }
    // the kernel is VALU-bound on the GELU (10 FMAs vs ~30 issue slots of erf per channel pair): results stored as
    // bf16 take the polynomial form (no transcendental slots, four chains interleaved), fp32 results the 1.5e-7 form
    if constexpr (sizeof(TO) == 2) {
      gelu_bf16x2_x4(a4);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) a4[i] = gelu_fast2(a4[i]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) { o[2 * i] = a4[i].x; o[2 * i + 1] = a4[i].y; }
    TO* dst = out + ((int64_t)b * T1 + t0 + f) * C + c0;
    if constexpr (PK != 0) {
      store_pairs<PK, 8>(out, ((int64_t)b * T1 + t0 + f) * C + c0, o);
    } else if constexpr (sizeof(TO) == 2) {
      bf16x8 v;
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = (bf16_t)o[i];
      *(bf16x8*)dst = v;
    } else {
      *(float4*)dst = float4{o[0], o[1], o[2], o[3]};
      *(float4*)(dst + 4) = float4{o[4], o[5], o[6], o[7]};
    }
  }
}
}  // namespace
int launch_conv0_group_apply(int prec, const float* wav, int B, int64_t L, int k, int stride, int64_t T1, int C,
                             const float* coef, void* out, hipStream_t s, int pair_kind) {
  if (k != K0 || stride > 5 || C > 512 || C % 8) { set_error("conv0: unsupported geometry"); return -1; }
  dim3 grid((unsigned)((T1 + 127) / 128), B);
  if (pair_kind) {
    if (prec || C % 32 || ((uintptr_t)out & 127) || (pair_kind != 2 && pair_kind != 3)) { set_error("conv0: pair-row output needs fp32 storage and C % 32 == 0"); return -1; }
    if (pair_kind == 3) hipLaunchKernelGGL((conv0_group_apply_kernel<float, 3>), grid, dim3(256), 0, s, wav, L, stride, T1, C, coef, (float*)out);
    else hipLaunchKernelGGL((conv0_group_apply_kernel<float, 2>), grid, dim3(256), 0, s, wav, L, stride, T1, C, coef, (float*)out);
  } else if (prec)
    hipLaunchKernelGGL((conv0_group_apply_kernel<bf16_t>), grid, dim3(256), 0, s, wav, L, stride, T1, C, coef,
                       (bf16_t*)out);
  else
    hipLaunchKernelGGL((conv0_group_apply_kernel<float>), grid, dim3(256), 0, s, wav, L, stride, T1, C, coef,
                       (float*)out);
  g_c0_kernel_id = 400 + (pair_kind ? 10 * pair_kind : prec ? 1 : 0);
  SVT_LAUNCH_CHECK();
  return 0;
}

namespace {
// conv layer 0, "layer" mode: conv (+bias) -> LayerNorm over C -> GELU, one wave per frame.
template <typename TO, int PK = 0>
__global__ __launch_bounds__(256) void conv0_layer_kernel(const float* wav, int64_t L, int stride, int64_t T1, int C,
                                                          const double* wav_mom, int64_t n_wav, float eps_wav,
                                                          const float* w0, const float* b0, const float* gamma,
                                                          const float* beta, float eps, TO* out, int cpg) {
  constexpr int FPW = 16;
  const int b = blockIdx.y;
  if (wav_mom) wav_mom += 2 * (b / cpg);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t t0 = ((int64_t)blockIdx.x * 4 + wave) * FPW;
  if (t0 >= T1) return;
  float mu = 0.f, r = 1.f;
  if (wav_mom) {
    const double m = wav_mom[0] / (double)n_wav;
    const double var = wav_mom[1] / (double)n_wav - m * m;
    mu = (float)m;
    r = (float)(1.0 / sqrt(var + (double)eps_wav));
  }
  const float* x = wav + (int64_t)b * L;
  const int c0 = lane * 8;
  const bool active = c0 < C;
  float w[8][K0], bb[8], g[8], be[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = active ? c0 + i : 0;
#pragma unroll
    for (int j = 0; j < K0; ++j) w[i][j] = w0[c * K0 + j];
    bb[i] = b0 ? b0[c] : 0.f;
    g[i] = gamma[c];
    be[i] = beta[c];
  }
  const int nfr = (int)((T1 - t0 < FPW) ? (T1 - t0) : FPW);
  // the wave's normalised samples staged once in a wave-private LDS strip (was: ten broadcast global loads per frame)
  __shared__ float xs[4][FPW * 5 + 16];  // stride <= 5
  {
    const int ns = (nfr - 1) * stride + K0;
    for (int i = lane; i < ns; i += 64) xs[wave][i] = (x[t0 * stride + i] - mu) * r;
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  }
  // two frames per iteration: the two wave-wide reductions of a frame (mean, variance) are dependent shuffle chains of ~150 cycles
  // each; with a second, independent frame in flight the vector ALU has work while they run (hubert-large 64 x 10 s: 1 021 -> 981 us;
  // what remains is the arithmetic itself: ~150 vector instructions per frame and lane)
  for (int f0 = 0; f0 < nfr; f0 += 2) {
    const int fr[2] = {f0, f0 + 1 < nfr ? f0 + 1 : f0};
    float y[2][8], s[2] = {0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      float xv[K0];
#pragma unroll
      for (int j = 0; j < K0; ++j) xv[j] = xs[wave][fr[u] * stride + j];
#pragma unroll
      for (int i = 0; i < 8; i += 2) {  // channel pairs on packed fp32 math
        f32x2_t a = {bb[i], bb[i + 1]};
#pragma unroll
        for (int j = 0; j < K0; ++j) a = f32x2_t{w[i][j], w[i + 1][j]} * xv[j] + a;
        y[u][i] = a.x;
        y[u][i + 1] = a.y;
        if (active) s[u] += a.x + a.y;
      }
    }
    float mean[2], q[2] = {0.f, 0.f}, rstd[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) mean[u] = wave_sum(s[u]) / (float)C;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int i = 0; i < 8; ++i) { const float d = y[u][i] - mean[u]; if (active) q[u] += d * d; }
#pragma unroll
    for (int u = 0; u < 2; ++u) rstd[u] = rsqrtf(wave_sum(q[u]) / (float)C + eps);
    if (!active) continue;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (u == 1 && fr[1] == fr[0]) break;   // odd tail: the second frame is a repeat of the first
      float o[8];
      if constexpr (sizeof(TO) == 2) {
        // bf16 result: polynomial GELU, four pair-chains interleaved (common.h)
        f32x2_t a4[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
          a4[i] = f32x2_t{(y[u][2 * i] - mean[u]) * rstd[u] * g[2 * i] + be[2 * i], (y[u][2 * i + 1] - mean[u]) * rstd[u] * g[2 * i + 1] + be[2 * i + 1]};
        gelu_bf16x2_x4(a4);
#pragma unroll
        for (int i = 0; i < 4; ++i) { o[2 * i] = a4[i].x; o[2 * i + 1] = a4[i].y; }
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = gelu_erf((y[u][i] - mean[u]) * rstd[u] * g[i] + be[i]);
      }
      TO* dst = out + ((int64_t)b * T1 + t0 + fr[u]) * C + c0;
      if constexpr (PK != 0) {
        store_pairs<PK, 8>(out, ((int64_t)b * T1 + t0 + fr[u]) * C + c0, o);
      } else if constexpr (sizeof(TO) == 2) {
        bf16x8 v;
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (bf16_t)o[i];
        *(bf16x8*)dst = v;
      } else {
        *(float4*)dst = float4{o[0], o[1], o[2], o[3]};
        *(float4*)(dst + 4) = float4{o[4], o[5], o[6], o[7]};
      }
    }
  }
}
}  // namespace
int launch_conv0_layer(int prec, const float* wav, int B, int64_t L, int k, int stride, int64_t T1, int C,
                       const double* wav_moments, int64_t n_wav, float eps_wav, const float* w0, const float* b0,
                       const float* gamma, const float* beta, float eps, void* out, hipStream_t s, int cpg, int pair_kind) {
  if (k != K0 || stride > 5 || C > 512 || C % 8) { set_error("conv0: unsupported geometry"); return -1; }   // (the LDS strip holds stride <= 5)
  dim3 grid((unsigned)((T1 + 63) / 64), B);
  if (pair_kind) {
    if (prec || C % 32 || ((uintptr_t)out & 127) || (pair_kind != 2 && pair_kind != 3)) { set_error("conv0: pair-row output needs fp32 storage and C % 32 == 0"); return -1; }
    if (pair_kind == 3)
      hipLaunchKernelGGL((conv0_layer_kernel<float, 3>), grid, dim3(256), 0, s, wav, L, stride, T1, C, wav_moments, n_wav, eps_wav, w0, b0, gamma, beta, eps, (float*)out, cpg);
    else
      hipLaunchKernelGGL((conv0_layer_kernel<float, 2>), grid, dim3(256), 0, s, wav, L, stride, T1, C, wav_moments, n_wav, eps_wav, w0, b0, gamma, beta, eps, (float*)out, cpg);
  } else if (prec)
    hipLaunchKernelGGL((conv0_layer_kernel<bf16_t>), grid, dim3(256), 0, s, wav, L, stride, T1, C, wav_moments, n_wav,
                       eps_wav, w0, b0, gamma, beta, eps, (bf16_t*)out, cpg);
  else
    hipLaunchKernelGGL((conv0_layer_kernel<float>), grid, dim3(256), 0, s, wav, L, stride, T1, C, wav_moments, n_wav,
                       eps_wav, w0, b0, gamma, beta, eps, (float*)out, cpg);
  g_c0_kernel_id = 500 + (pair_kind ? 10 * pair_kind : prec ? 1 : 0);
  SVT_LAUNCH_CHECK();
  return 0;
}

namespace {
// fp32 <-> pair rows (test / debug hooks and re-layouts outside the hot path): one thread per 8 consecutive elements
// They share store_pairs<PK, 8> with the kernels above, and hipcc propagates value ranges into such an internal function from ALL its callers
// in the translation unit: compiled apart from the conv kernels, f32_to_pairs_kernel comes out with a different address mask.
template <int PK>
__global__ void f32_to_pairs_kernel(const float* __restrict__ x, void* __restrict__ out, int64_t n8) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n8) return;
  const float4 a = ((const float4*)x)[2 * i], b = ((const float4*)x)[2 * i + 1];
  const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  store_pairs<PK, 8>(out, i * 8, v);
}
template <int PK>
__global__ void pairs_to_f32_kernel(const void* __restrict__ in, float* __restrict__ y, int64_t n8, const void* lo_plane) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n8) return;
  const int64_t e = i * 8;
  // lo_plane == nullptr: pair rows; else `in` / `lo_plane` are separate (hi, lo) planes with the element layout of y
  const char* ph = lo_plane ? (const char*)in + e * 2 : (const char*)in + (e >> 5) * 128 + (e & 31) * 2;
  const char* pl = lo_plane ? (const char*)lo_plane + e * 2 : ph + 64;
  const uint4 h = *(const uint4*)ph, l = *(const uint4*)pl;
  const unsigned hw[4] = {h.x, h.y, h.z, h.w}, lw[4] = {l.x, l.y, l.z, l.w};
  float o[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const unsigned short hs = (unsigned short)(hw[j >> 1] >> (16 * (j & 1))), ls = (unsigned short)(lw[j >> 1] >> (16 * (j & 1)));
    if constexpr (PK == 3) o[j] = (float)__builtin_bit_cast(_Float16, hs) + (float)__builtin_bit_cast(_Float16, ls);
    else o[j] = (float)__builtin_bit_cast(__bf16, hs) + (float)__builtin_bit_cast(__bf16, ls);
  }
  ((float4*)y)[2 * i] = float4{o[0], o[1], o[2], o[3]};
  ((float4*)y)[2 * i + 1] = float4{o[4], o[5], o[6], o[7]};
}
}  // namespace
int launch_f32_to_pairs(int kind, const float* x, void* out, int64_t n, hipStream_t s) {
  if (n % 32 || !aligned(15, x) || !aligned(127, out) || (kind != 2 && kind != 3)) { set_error("f32_to_pairs: n % 32, alignment or kind"); return -1; }
  const int64_t n8 = n / 8;
  if (kind == 3) hipLaunchKernelGGL((f32_to_pairs_kernel<3>), dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, x, out, n8);
  else hipLaunchKernelGGL((f32_to_pairs_kernel<2>), dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, x, out, n8);
  SVT_LAUNCH_CHECK();
  return 0;
}
int launch_pairs_to_f32(int kind, const void* in, const void* lo_plane, float* y, int64_t n, hipStream_t s) {
  if (n % 32 || !aligned(15, y, in, lo_plane) || (kind != 2 && kind != 3)) { set_error("pairs_to_f32: n % 32, alignment or kind"); return -1; }
  const int64_t n8 = n / 8;
  if (kind == 3) hipLaunchKernelGGL((pairs_to_f32_kernel<3>), dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, in, y, n8, lo_plane);
  else hipLaunchKernelGGL((pairs_to_f32_kernel<2>), dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, in, y, n8, lo_plane);
  SVT_LAUNCH_CHECK();
  return 0;
}

}  // namespace svt
