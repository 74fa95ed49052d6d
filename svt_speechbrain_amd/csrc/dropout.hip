// Training-mode dropout of the encoder (svt_encoder_set_dropout; HF modeling_wav2vec2.py: feat_proj_dropout, hidden_dropout,
// attention_dropout, activation_dropout).  The mask is a function of POSITION, not of a launch geometry: element e -- its logical index
// in the tensor, (b*T + t)*W + c, or ((b*H + h)*T + i)*T + j for the attention probabilities -- is kept iff word e & 3 of
//     Philox4x32-10(counter = (q_lo, q_hi, site | layer << 8, step), key = (seed_lo, seed_hi)),   q = e >> 2,
// is >= floor(p * 2^32); a kept value is multiplied by float(1 / (1 - p)) (one rounding), a dropped one becomes +0 (philox.h).  Padding,
// pitch and tiling never enter, so another kernel or tile shape cannot change a mask.  Streaming kernels, in place, one Philox call per
// four elements:
//   dropout_rows_kernel<T, .>     a flat tensor of n elements in fp32 or the 16-bit operand type.  A thread owns one 16-byte piece:
//                                 4 fp32 (one Philox group) or 8 halves (two groups), loaded and stored as one access when the first
//                                 logical index e0 is a multiple of 4 -- the encoder's case, e0 = 0 -- and the piece lies inside the
//                                 tensor; a ragged tail, or the groups of an e0 that is no multiple of 4 (the debug entry's, to reach
//                                 q_hi != 0 with a small tensor), go element by element.
//   dropout_hilo_kernel           the bf16 (hi, lo) residual stream of post_ln_hilo: the stream's VALUE v = float(hi) + float(lo) (one
//                                 fp32 add) is scaled or zeroed and cut again as layernorm_hilo_kernel cuts: hi' = T(o), lo' = T(o - hi').
//   softmax_dropout_kernel<TO>    softmax_rows_kernel's arithmetic (encoder_ops.hip: a wave per row, the same lanes take the same
//                                 columns for the maximum and the sum, so both are bit for bit the plain kernel's), then the mask on the
//                                 normalised probabilities as they are written: HF eager's softmax -> dropout -> P V.  The write pass
//                                 walks the row's Philox groups, a lane per group; pad columns [T, Tp) are zeroed as the plain kernel does.
// Offsets are 64-bit throughout.
#include "device_util.h"
#include "philox.h"

#include <cmath>

namespace svt {
int g_dropout_kernel_id = 0;   // svt_debug_set key 44 (query): the kernel the last dropout launch chose (include/svt_mi355.h lists the ids)

namespace {
constexpr int64_t kDropMaxBlocks = 16384;

// The product is ONE plain fp32 multiplication.  The two empty asm statements pin its operand and its result in fp32 registers: left
// alone, the half build folds the conversions around it into v_fma_mixlo_f16 (x * scale + 0), whose +0 addend turns a kept -0 into +0
__device__ __forceinline__ float drop_apply(float v, uint32_t word, const DropSpec& d) {
  asm volatile("" : "+v"(v));
  float r = __fmul_rn(v, d.scale);
  asm volatile("" : "+v"(r));
  return word >= d.thr ? r : 0.f;
}

template <typename T> struct Vec16;
template <> struct Vec16<float> { typedef f32x4 type; static constexpr int N = 4; };
template <> struct Vec16<bf16_t> { typedef bf16x8 type; static constexpr int N = 8; };

// x[i], i in [0, n): logical index e0 + i.  ALIGNED: e0 % 4 == 0 and x 16-byte aligned -- whole pieces as one access
template <typename T, bool ALIGNED>
__global__ __launch_bounds__(256) void dropout_rows_kernel(T* __restrict__ x, int64_t n, uint64_t e0, DropSpec d, int64_t pieces) {
  typedef typename Vec16<T>::type V;
  constexpr int N = Vec16<T>::N, G = N / 4;
  const unsigned off = (unsigned)(e0 & 3);
  const uint64_t q0 = e0 >> 2;
  for (int64_t pc = (int64_t)blockIdx.x * 256 + threadIdx.x; pc < pieces; pc += (int64_t)gridDim.x * 256) {
    // piece pc = Philox groups q0 + pc*G .. + G-1; element k of group g sits at memory index (pc*G + g)*4 + k - off
    const int64_t i0 = pc * N - off;
    Philox4 w[G];
#pragma unroll
    for (int g = 0; g < G; ++g) w[g] = drop_words(d, q0 + (uint64_t)pc * G + g);
    if (ALIGNED && i0 + N <= n) {
      V v = *(const V*)(x + i0);
#pragma unroll
      for (int j = 0; j < N; ++j) v[j] = (T)drop_apply((float)v[j], w[j >> 2].w[j & 3], d);
      *(V*)(x + i0) = v;
    } else {
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const int64_t i = i0 + j;
        if (i >= 0 && i < n) x[i] = (T)drop_apply((float)x[i], w[j >> 2].w[j & 3], d);
      }
    }
  }
}

template <bool ALIGNED>
__global__ __launch_bounds__(256) void dropout_hilo_kernel(bf16_t* __restrict__ xh, bf16_t* __restrict__ xl, int64_t n, uint64_t e0, DropSpec d,
                                                            int64_t pieces) {
  constexpr int N = 8, G = 2;
  const unsigned off = (unsigned)(e0 & 3);
  const uint64_t q0 = e0 >> 2;
  for (int64_t pc = (int64_t)blockIdx.x * 256 + threadIdx.x; pc < pieces; pc += (int64_t)gridDim.x * 256) {
    const int64_t i0 = pc * N - off;
    Philox4 w[G];
#pragma unroll
    for (int g = 0; g < G; ++g) w[g] = drop_words(d, q0 + (uint64_t)pc * G + g);
    if (ALIGNED && i0 + N <= n) {
      bf16x8 h = *(const bf16x8*)(xh + i0), l = *(const bf16x8*)(xl + i0);
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const float o = drop_apply(__fadd_rn((float)h[j], (float)l[j]), w[j >> 2].w[j & 3], d);
        h[j] = (bf16_t)o;
        l[j] = (bf16_t)__fsub_rn(o, (float)h[j]);
      }
      *(bf16x8*)(xh + i0) = h;
      *(bf16x8*)(xl + i0) = l;
    } else {
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const int64_t i = i0 + j;
        if (i < 0 || i >= n) continue;
        const float o = drop_apply(__fadd_rn((float)xh[i], (float)xl[i]), w[j >> 2].w[j & 3], d);
        const bf16_t oh = (bf16_t)o;
        xh[i] = oh;
        xl[i] = (bf16_t)__fsub_rn(o, (float)oh);
      }
    }
  }
}

// row r of S (pitch Tp, T real columns): logical index of column j = e0 + r*T + j
template <typename TO>
__global__ __launch_bounds__(256) void softmax_dropout_kernel(const float* __restrict__ S, int64_t rows, int T, int Tp, TO* __restrict__ P, uint64_t e0,
                                                               DropSpec d) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* s = S + row * Tp;
  float mx = -INFINITY;
  for (int i = lane; i < T; i += 64) mx = fmaxf(mx, s[i]);
  mx = wave_max(mx);
  float sum = 0.f;
  for (int i = lane; i < T; i += 64) sum += expf(s[i] - mx);
  const float inv = 1.f / wave_sum(sum);
  const uint64_t er = e0 + (uint64_t)row * (uint64_t)T;       // logical index of column 0
  const uint64_t qa = er >> 2, qb = (er + (uint64_t)T - 1) >> 2;   // the row's first and last Philox group
  for (uint64_t q = qa + lane; q <= qb; q += 64) {
    const Philox4 w = drop_words(d, q);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t j = (int64_t)(q * 4 + k - er);
      if (j >= 0 && j < T) st<TO>(P, row * Tp + j, drop_apply(expf(s[j] - mx) * inv, w.w[k], d));
    }
  }
  for (int i = T + lane; i < Tp; i += 64) st<TO>(P, row * Tp + i, 0.f);
}

int64_t drop_pieces(int64_t n, uint64_t e0, int N) { return ((int64_t)(e0 & 3) + n + N - 1) / N; }
unsigned drop_grid(int64_t pieces) {
  const int64_t g = (pieces + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > kDropMaxBlocks ? kDropMaxBlocks : g));
}
}  // namespace

DropSpec make_drop_spec(double p, uint64_t seed, uint32_t step, int site, int layer) {
  DropSpec d;
  d.thr = (uint32_t)(int64_t)std::floor(p * 4294967296.0);
  d.scale = (float)(1.0 / (1.0 - p));
  d.seed_lo = (uint32_t)seed; d.seed_hi = (uint32_t)(seed >> 32);
  d.site_layer = (uint32_t)site | ((uint32_t)layer << 8);
  d.step = step;
  return d;
}

// kind 0: fp32, 1: the 16-bit operand type.  In place on x[0, n), logical indices e0 ..; one launch
int launch_dropout_rows(int kind, void* x, int64_t n, uint64_t e0, const DropSpec& d, hipStream_t s) {
  if (!x || n < 1 || n > (int64_t)1 << 60) { set_error("dropout: bad geometry"); return -1; }
  if (!aligned(kind ? 1 : 3, x)) { set_error("dropout: misaligned pointer"); return -1; }
  const bool al = !(e0 & 3) && aligned(15, x);
  const int64_t pieces = drop_pieces(n, e0, kind ? 8 : 4);
  const dim3 grid(drop_grid(pieces));
  if (kind) {
    if (al) hipLaunchKernelGGL((dropout_rows_kernel<bf16_t, true>), grid, dim3(256), 0, s, (bf16_t*)x, n, e0, d, pieces);
    else hipLaunchKernelGGL((dropout_rows_kernel<bf16_t, false>), grid, dim3(256), 0, s, (bf16_t*)x, n, e0, d, pieces);
  } else {
    if (al) hipLaunchKernelGGL((dropout_rows_kernel<float, true>), grid, dim3(256), 0, s, (float*)x, n, e0, d, pieces);
    else hipLaunchKernelGGL((dropout_rows_kernel<float, false>), grid, dim3(256), 0, s, (float*)x, n, e0, d, pieces);
  }
  g_dropout_kernel_id = (kind ? 2 : 1) + (al ? 0 : 10);
  SVT_LAUNCH_CHECK();
  return 0;
}

int launch_dropout_hilo(bf16_t* xh, bf16_t* xl, int64_t n, uint64_t e0, const DropSpec& d, hipStream_t s) {
  if (!xh || !xl || n < 1 || n > (int64_t)1 << 60) { set_error("dropout: bad geometry"); return -1; }
  if (!aligned(1, xh, xl)) { set_error("dropout: misaligned pointer"); return -1; }
  const bool al = !(e0 & 3) && aligned(15, xh, xl);
  const int64_t pieces = drop_pieces(n, e0, 8);
  const dim3 grid(drop_grid(pieces));
  if (al) hipLaunchKernelGGL((dropout_hilo_kernel<true>), grid, dim3(256), 0, s, xh, xl, n, e0, d, pieces);
  else hipLaunchKernelGGL((dropout_hilo_kernel<false>), grid, dim3(256), 0, s, xh, xl, n, e0, d, pieces);
  g_dropout_kernel_id = 3 + (al ? 0 : 10);
  SVT_LAUNCH_CHECK();
  return 0;
}

// launch_softmax_rows with the site's mask on the probabilities; prec: the type of P (0 fp32, else the operand type)
int launch_softmax_dropout(int prec, const float* S, int64_t rows, int T, int Tp, void* P, uint64_t e0, const DropSpec& d, hipStream_t s) {
  if (!S || !P || rows < 1 || T < 1 || Tp < T || rows > ((int64_t)1 << 33)) { set_error("softmax dropout: bad geometry"); return -1; }
  const dim3 grid((unsigned)((rows + 3) / 4));
  if (prec) hipLaunchKernelGGL((softmax_dropout_kernel<bf16_t>), grid, dim3(256), 0, s, S, rows, T, Tp, (bf16_t*)P, e0, d);
  else hipLaunchKernelGGL((softmax_dropout_kernel<float>), grid, dim3(256), 0, s, S, rows, T, Tp, (float*)P, e0, d);
  g_dropout_kernel_id = prec ? 5 : 4;
  SVT_LAUNCH_CHECK();
  return 0;
}

}  // namespace svt
