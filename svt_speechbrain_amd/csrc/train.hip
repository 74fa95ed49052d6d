// Head-only training step of the recipes' linear-probe stage (MIR_ST500/train_audio_ssl.py:192-199: the encoder frozen, the
// 20-way Linear head learning): the recipe's objective and its gradient w.r.t. the logits in one pass, the head's weight gradient,
// and clip_grad_norm_ + Adadelta.  Every reduction has a fixed order -- no float atomics, no inter-workgroup flags; a split
// reduction is combined by a second launch -- so two calls on the same inputs give the same bits.
#include "common.h"

namespace svt {
namespace {

constexpr int kMaxOut = 32;   // widest head the objective and the weight gradient take (registers hold a whole logit row)

__device__ __forceinline__ double block_sum_d256(double v, double* sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}

// number of t in [0, T) with (float)t < lim: t < 2^24 is exact in fp32, so it is ceil(lim) clamped to [0, T] (0 for NaN)
__device__ __forceinline__ int64_t mask_count(float lim, int64_t T) {
  if (!(lim > 0.f)) return 0;
  const float c = ceilf(lim);
  return c >= (float)T ? T : (int64_t)c;
}

// log-softmax + NLL over the columns [a, a + C) of a register row, with the gradient of
// (1 - ls) * (-logp[k]) + ls * (-mean_c logp) w.r.t. the logits.  The log-softmax is svt_softmax's (softmax_small_kernel: max,
// sequential sum of exp, (x - max) - log(sum)) and the loss / mean are nll_loss_kernel's, so the sums match svt_nll_loss on
// svt_softmax's output.  k == -100 is ignored (loss 0, only the smoothing part of the gradient).
__device__ __forceinline__ void nll_group(const float (&v)[kMaxOut], float (&g)[kMaxOut], int a, int C, int64_t k, float smoothing,
                                          float& loss, float& mean, bool& bad) {
  float mx = v[a];
#pragma unroll
  for (int i = 0; i < kMaxOut; ++i)
    if (i > a && i < a + C) mx = fmaxf(mx, v[i]);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < kMaxOut; ++i)
    if (i >= a && i < a + C) s += expf(v[i] - mx);
  const float ls = logf(s);
  const bool valid = k >= 0 && k < C;
  if (k != -100 && !valid) bad = true;
  loss = 0.f;
  mean = 0.f;
  const float inv_c = 1.f / (float)C;
#pragma unroll
  for (int i = 0; i < kMaxOut; ++i) {
    if (i >= a && i < a + C) {
      const float lp = (v[i] - mx) - ls;
      mean += lp;
      const bool hit = valid && i - a == k;
      if (hit) loss = -lp;
      const float p = expf(v[i] - mx) / s;
      const float gn = valid ? p - (hit ? 1.f : 0.f) : 0.f;
      g[i] = smoothing == 0.f ? gn : (1.f - smoothing) * gn + smoothing * (p - inv_c);
    }
  }
}

// One workgroup per batch item, frame t on thread t % 256 (the thread -> frame map and block reduction of bce_loss_kernel /
// nll_loss_kernel).  Columns: [onset, offset, octave x C_o, class x C_c].  Per block: 7 double sums {onset, offset, octave loss,
// octave mean-logp, class loss, class mean-logp, mask} and a bad-target flag.  dx = d(sum of the four mean losses)/dx, zero on
// masked frames and on the truncated tail t >= T.
__global__ __launch_bounds__(256) void amt_objective_grad_kernel(
    const float* __restrict__ x, int64_t B, int64_t t_pred, int n_out, int n_oct_cols, const float* __restrict__ on_t,
    const float* __restrict__ off_t, const int64_t* __restrict__ oct_t, const int64_t* __restrict__ cls_t, int64_t t_tgt,
    int64_t T, const float* __restrict__ rel_len, float pw, float smoothing, float* __restrict__ dx, double* __restrict__ sums,
    int* __restrict__ bad_out) {
  __shared__ double sh[4];
  const int64_t b = blockIdx.x;
  // the mean's denominator (sum of the mask over the whole batch), from each item's limit: the same integer the loss sums count
  int64_t cnt = 0;
  for (int64_t i = 0; i < B; ++i) cnt += rel_len ? mask_count(__fmul_rn(rel_len[i], (float)T), T) : T;
  const float den = (float)(double)cnt;
  const float lim = rel_len ? __fmul_rn(rel_len[b], (float)T) : 0.f;
  const int a_oct = 2, a_cls = 2 + n_oct_cols, n_cls_cols = n_out - a_cls;
  double s_on = 0.0, s_off = 0.0, s_oct = 0.0, r_oct = 0.0, s_cls = 0.0, r_cls = 0.0, s_m = 0.0;
  bool bad = false;
  for (int64_t t = threadIdx.x; t < t_pred; t += 256) {
    const float* row = x + (b * t_pred + t) * n_out;
    float* drow = dx + (b * t_pred + t) * n_out;
    if (t >= T) {
      for (int c = 0; c < n_out; ++c) drow[c] = 0.f;
      continue;
    }
    float v[kMaxOut], g[kMaxOut];
#pragma unroll
    for (int c = 0; c < kMaxOut; ++c) { v[c] = c < n_out ? row[c] : 0.f; g[c] = 0.f; }
    const float m = rel_len ? ((float)t < lim ? 1.f : 0.f) : 1.f;
    // BCE with logits (bce_loss_kernel's expression): (1 - y) x + (1 + (pw - 1) y) softplus(-x); d/dx = (1 - y) - lw sigmoid(-x)
    const float xo = v[0], yo = on_t[b * t_tgt + t];
    const float spo = log1pf(expf(-fabsf(xo))) + fmaxf(-xo, 0.f);
    const float lwo = 1.f + (pw - 1.f) * yo;
    const float l_on = ((1.f - yo) * xo + lwo * spo) * m;
    g[0] = (1.f - yo) - lwo / (1.f + expf(xo));
    const float xf = v[1], yf = off_t[b * t_tgt + t];
    const float spf = log1pf(expf(-fabsf(xf))) + fmaxf(-xf, 0.f);
    const float l_off = ((1.f - yf) * xf + 1.f * spf) * m;
    g[1] = (1.f - yf) - 1.f / (1.f + expf(xf));
    float l_oct, mean_oct, l_cls, mean_cls;
    nll_group(v, g, a_oct, n_oct_cols, oct_t[b * t_tgt + t], smoothing, l_oct, mean_oct, bad);
    nll_group(v, g, a_cls, n_cls_cols, cls_t[b * t_tgt + t], smoothing, l_cls, mean_cls, bad);
    l_oct *= m;
    l_cls *= m;
    mean_oct = mean_oct / (float)n_oct_cols * m;
    mean_cls = mean_cls / (float)n_cls_cols * m;
#pragma unroll
    for (int c = 0; c < kMaxOut; ++c)
      if (c < n_out) drow[c] = m != 0.f ? g[c] / den : 0.f;
    s_on += (double)l_on;
    s_off += (double)l_off;
    s_oct += (double)l_oct;
    r_oct += (double)mean_oct;
    s_cls += (double)l_cls;
    r_cls += (double)mean_cls;
    s_m += (double)m;
  }
  s_on = block_sum_d256(s_on, sh);
  s_off = block_sum_d256(s_off, sh);
  s_oct = block_sum_d256(s_oct, sh);
  r_oct = block_sum_d256(r_oct, sh);
  s_cls = block_sum_d256(s_cls, sh);
  r_cls = block_sum_d256(r_cls, sh);
  s_m = block_sum_d256(s_m, sh);
  const int any_bad = __syncthreads_or(bad ? 1 : 0);
  if (threadIdx.x == 0) {
    double* o = sums + b * 8;
    o[0] = s_on; o[1] = s_off; o[2] = s_oct; o[3] = r_oct; o[4] = s_cls; o[5] = r_cls; o[6] = s_m; o[7] = 0.0;
    bad_out[b] = any_bad;
  }
}

// reduction "mean" of the four terms (loss_reduce_kernel's arithmetic) and their sum in the recipe's order; one thread.
// out: terms[5]; status: {int32 bad target, float terms[5]} for the host copy
__global__ void amt_objective_reduce_kernel(const double* sums, const int* bad, int B, float smoothing, float* terms, int* status) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double acc[7] = {0, 0, 0, 0, 0, 0, 0};
  int any = 0;
  for (int b = 0; b < B; ++b) {
    for (int i = 0; i < 7; ++i) acc[i] += sums[b * 8 + i];
    any |= bad[b];
  }
  const float den = (float)acc[6];
  const float on = (float)acc[0] / den, off = (float)acc[1] / den;
  float oct = (float)acc[2] / den, cls = (float)acc[4] / den;
  if (smoothing != 0.f) {
    oct = -smoothing * ((float)acc[3] / den) + (1.f - smoothing) * oct;
    cls = -smoothing * ((float)acc[5] / den) + (1.f - smoothing) * cls;
  }
  const float total = ((on + off) + oct) + cls;
  const float t5[5] = {on, off, oct, cls, total};
  float* st = (float*)(status + 1);
  for (int i = 0; i < 5; ++i) { terms[i] = t5[i]; st[i] = t5[i]; }
  status[0] = any;
}

// ---- head weight gradient: dW (N x D) = dY^T X, db = sum_rows dY ----
// Grid (slabs, column tiles of 256).  Each wave of a workgroup walks rows wave, wave + 4, ... of its slab, a lane holding 4 adjacent
// columns of X (one 16-byte load per row) and their N x 4 partial sums; the dY row is wave-uniform (scalar loads).  kRowUnroll rows
// of X are in flight per wave.  The four waves are combined in LDS in a fixed tree ((w0 + w2) + (w1 + w3)) and the slab's partial
// is stored; linear_wgrad_combine_kernel sums the slabs in order.
constexpr int kRowUnroll = 16;

template <int NB>
__global__ __launch_bounds__(256) void linear_wgrad_partial_kernel(const float* __restrict__ x, const float* __restrict__ dy, int64_t rows,
                                                                   int D, int N, int64_t rows_per_slab, float* __restrict__ part) {
  __shared__ f32x4 red[2][NB][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t slab = blockIdx.x;
  const int col = blockIdx.y * 256 + lane * 4;
  const bool on = col < D;   // D % 4 == 0: a lane's four columns are all inside or all outside
  const int64_t r0 = slab * rows_per_slab;
  const int64_t r1 = r0 + rows_per_slab < rows ? r0 + rows_per_slab : rows;
  f32x4 acc[NB];
#pragma unroll
  for (int n = 0; n < NB; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int64_t r = r0 + wave; r < r1; r += 4 * kRowUnroll) {
    f32x4 xv[kRowUnroll];
#pragma unroll
    for (int u = 0; u < kRowUnroll; ++u) {
      const int64_t rr = r + 4 * u;
      xv[u] = (on && rr < r1) ? *(const f32x4*)(x + rr * D + col) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int u = 0; u < kRowUnroll; ++u) {
      const int64_t rr = r + 4 * u;
      if (rr < r1) {
        const float* d = dy + rr * N;
#pragma unroll
        for (int n = 0; n < NB; ++n) {
          const float dv = n < N ? d[n] : 0.f;
          acc[n] += dv * xv[u];
        }
      }
    }
  }
  if (wave >= 2) {
#pragma unroll
    for (int n = 0; n < NB; ++n) red[wave - 2][n][lane] = acc[n];
  }
  __syncthreads();
  if (wave < 2) {
#pragma unroll
    for (int n = 0; n < NB; ++n) acc[n] += red[wave][n][lane];
  }
  __syncthreads();
  if (wave == 1) {
#pragma unroll
    for (int n = 0; n < NB; ++n) red[0][n][lane] = acc[n];
  }
  __syncthreads();
  if (wave == 0 && on) {
#pragma unroll
    for (int n = 0; n < NB; ++n)
      if (n < N) *(f32x4*)(part + (slab * N + n) * D + col) = acc[n] + red[0][n][lane];
  }
}

// blocks [0, ceil(N*D/4 / 16)): dW, 16 groups of 4 adjacent columns x 16 slab lanes per block -- lane l sums slabs l, l + 16, ...
// in order, then lane 0 adds the 16 lane sums in order; the last N blocks: db[n] (block n's threads stride the rows, then a fixed
// shuffle / LDS tree)
__global__ __launch_bounds__(256) void linear_wgrad_combine_kernel(const float* __restrict__ part, int64_t slabs, const float* __restrict__ dy,
                                                                   int64_t rows, int D, int N, int dw_blocks, float* __restrict__ dw,
                                                                   float* __restrict__ db) {
  __shared__ float sh[4];
  __shared__ f32x4 red[16][16];
  if ((int)blockIdx.x < dw_blocks) {
    const int j = threadIdx.x & 15, sl = threadIdx.x >> 4;
    const int64_t per_n = D / 4;
    const int64_t i4 = (int64_t)blockIdx.x * 16 + j;
    const bool ok = i4 < (int64_t)N * per_n;
    const int64_t n = ok ? i4 / per_n : 0, c = ok ? (i4 % per_n) * 4 : 0;
    f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
    if (ok)
      for (int64_t k = sl; k < slabs; k += 16) s += *(const f32x4*)(part + (k * N + n) * D + c);
    red[sl][j] = s;
    __syncthreads();
    if (sl == 0 && ok) {
      f32x4 t = red[0][j];
#pragma unroll
      for (int q = 1; q < 16; ++q) t += red[q][j];
      *(f32x4*)(dw + n * D + c) = t;
    }
    return;
  }
  if (!db) return;
  const int n = (int)blockIdx.x - dw_blocks;
  float s = 0.f;
  for (int64_t r = threadIdx.x; r < rows; r += 256) s += dy[r * N + n];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) db[n] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// ---- clip_grad_norm_ + Adadelta ----
struct AdaTensors {
  float* p[kAdaMaxTensors];
  float* g[kAdaMaxTensors];
  float* sq[kAdaMaxTensors];
  float* acc[kAdaMaxTensors];
  int64_t n[kAdaMaxTensors];
  int64_t chunk0[kAdaMaxTensors + 1];   // first sum-of-squares chunk of each tensor (prefix of ceil(n / kAdaChunk))
  int count;
};

__device__ __forceinline__ int ada_tensor_of(const AdaTensors& t, int64_t chunk) {
  int i = 0;
  while (i + 1 < t.count && chunk >= t.chunk0[i + 1]) ++i;
  return i;
}

// one block per chunk of kAdaChunk elements of one tensor: sum of g^2 in double, fixed tree
__global__ __launch_bounds__(256) void ada_sumsq_kernel(AdaTensors t, double* __restrict__ part) {
  __shared__ double sh[4];
  const int64_t chunk = blockIdx.x;
  const int i = ada_tensor_of(t, chunk);
  const int64_t lo = (chunk - t.chunk0[i]) * kAdaChunk;
  const int64_t hi = lo + kAdaChunk < t.n[i] ? lo + kAdaChunk : t.n[i];
  const float* g = t.g[i];
  double s = 0.0;
  for (int64_t e = lo + threadIdx.x; e < hi; e += 256) { const double v = (double)g[e]; s += v * v; }
  s = block_sum_d256(s, sh);
  if (threadIdx.x == 0) part[chunk] = s;
}

// clip_grad_norm_: norm_i = ||g_i|| (fp32), total = ||[norm_i]||, coef = min(max_norm / (total + 1e-6), 1); one thread, in order
__global__ void ada_norm_kernel(AdaTensors t, const double* __restrict__ part, float max_norm, float* __restrict__ coef,
                                float* __restrict__ total_out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double tot = 0.0;
  for (int i = 0; i < t.count; ++i) {
    double s = 0.0;
    for (int64_t c = t.chunk0[i]; c < t.chunk0[i + 1]; ++c) s += part[c];
    const float ni = (float)sqrt(s);
    tot += (double)ni * (double)ni;
  }
  const float total = (float)sqrt(tot);
  if (total_out) *total_out = total;
  if (coef) {
    const float c = __fdiv_rn(max_norm, __fadd_rn(total, 1e-6f));
    *coef = c < 1.f ? c : 1.f;
  }
}

// torch.optim.Adadelta's single-tensor update (torch/optim/adadelta.py), element-wise in torch's order and roundings; with `coef` the
// gradient is first scaled in place by the clip coefficient (clip_grad_norm_'s g.mul_(coef))
__global__ __launch_bounds__(256) void ada_update_kernel(AdaTensors t, const float* __restrict__ coef, float lr, float rho, float one_minus_rho,
                                                         float eps, float weight_decay, int maximize) {
  const float cf = coef ? *coef : 1.f;
  for (int i = 0; i < t.count; ++i) {
    float* __restrict__ p = t.p[i];
    float* __restrict__ gp = t.g[i];
    float* __restrict__ sq = t.sq[i];
    float* __restrict__ ac = t.acc[i];
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < t.n[i]; e += (int64_t)gridDim.x * 256) {
      float g = gp[e];
      if (coef) { g = __fmul_rn(g, cf); gp[e] = g; }
      if (maximize) g = -g;
      const float pv = p[e];
      if (weight_decay != 0.f) g = __fmaf_rn(pv, weight_decay, g);
      const float s = __fadd_rn(__fmul_rn(sq[e], rho), __fmul_rn(__fmul_rn(one_minus_rho, g), g));
      const float std_ = __fsqrt_rn(__fadd_rn(s, eps));
      const float d = __fmul_rn(__fdiv_rn(__fsqrt_rn(__fadd_rn(ac[e], eps)), std_), g);
      ac[e] = __fadd_rn(__fmul_rn(ac[e], rho), __fmul_rn(__fmul_rn(one_minus_rho, d), d));
      sq[e] = s;
      p[e] = __fmaf_rn(d, -lr, pv);
    }
  }
}

}  // namespace

int launch_amt_objective_grad(const float* x, int64_t B, int64_t t_pred, int n_out, int n_oct_cols, const float* on_t,
                              const float* off_t, const int64_t* oct_t, const int64_t* cls_t, int64_t t_tgt, int64_t T,
                              const float* rel_len, float pos_weight, float smoothing, float* dx, float* terms, void* ws,
                              hipStream_t s) {
  double* sums = (double*)ws;
  int* bad = (int*)(sums + B * 8);
  int* status = (int*)((char*)ws + amt_objective_status_offset(B));
  hipLaunchKernelGGL(amt_objective_grad_kernel, dim3((unsigned)B), dim3(256), 0, s, x, B, t_pred, n_out, n_oct_cols, on_t, off_t,
                     oct_t, cls_t, t_tgt, T, rel_len, pos_weight, smoothing, dx, sums, bad);
  SVT_LAUNCH_CHECK();
  hipLaunchKernelGGL(amt_objective_reduce_kernel, dim3(1), dim3(64), 0, s, sums, bad, (int)B, smoothing, terms, status);
  SVT_LAUNCH_CHECK();
  return 0;
}

size_t amt_objective_status_offset(int64_t B) { return ((size_t)B * 68 + 15) / 16 * 16; }
size_t amt_objective_workspace_bytes(int64_t B) { return amt_objective_status_offset(B) + 32; }

// slabs: about 256 workgroups in all (one per CU), at least 64 rows per slab; a function of (rows, D) only, so the order of every sum
// is fixed by the shapes
int64_t linear_wgrad_slabs(int64_t rows, int D) {
  const int64_t tiles = (D + 255) / 256;
  int64_t slabs = (256 + tiles - 1) / tiles;
  const int64_t cap = (rows + 63) / 64;
  if (slabs > cap) slabs = cap;
  return slabs < 1 ? 1 : slabs;
}
size_t linear_wgrad_workspace_bytes(int64_t rows, int D, int N) { return (size_t)linear_wgrad_slabs(rows, D) * N * D * sizeof(float); }

int launch_linear_wgrad(const float* x, const float* dy, int64_t rows, int D, int N, float* dw, float* db, void* ws, hipStream_t s) {
  const int64_t slabs = linear_wgrad_slabs(rows, D);
  const int64_t rps = (rows + slabs - 1) / slabs;
  float* part = (float*)ws;
  const dim3 grid((unsigned)slabs, (unsigned)((D + 255) / 256));
  const int nb = (N + 3) / 4 * 4;
  switch (nb) {
#define SVT_WGRAD_CASE(K) \
    case K: hipLaunchKernelGGL(linear_wgrad_partial_kernel<K>, grid, dim3(256), 0, s, x, dy, rows, D, N, rps, part); break;
    SVT_WGRAD_CASE(4) SVT_WGRAD_CASE(8) SVT_WGRAD_CASE(12) SVT_WGRAD_CASE(16)
    SVT_WGRAD_CASE(20) SVT_WGRAD_CASE(24) SVT_WGRAD_CASE(28) SVT_WGRAD_CASE(32)
#undef SVT_WGRAD_CASE
    default: set_error("linear_wgrad: out_features must be in 1..32"); return -1;
  }
  SVT_LAUNCH_CHECK();
  const int dw_blocks = (int)(((int64_t)N * (D / 4) + 15) / 16);
  hipLaunchKernelGGL(linear_wgrad_combine_kernel, dim3((unsigned)(dw_blocks + (db ? N : 0))), dim3(256), 0, s, part, slabs, dy, rows, D, N,
                     dw_blocks, dw, db);
  SVT_LAUNCH_CHECK();
  return 0;
}

int64_t ada_chunks(const int64_t* numels, int count) {
  int64_t c = 0;
  for (int i = 0; i < count; ++i) c += (numels[i] + kAdaChunk - 1) / kAdaChunk;
  return c;
}
size_t ada_workspace_bytes(const int64_t* numels, int count) { return (size_t)ada_chunks(numels, count) * sizeof(double) + 16; }

int launch_clip_adadelta(int count, float* const* params, float* const* grads, float* const* square_avg, float* const* acc_delta,
                         const int64_t* numels, float lr, float rho, float one_minus_rho, float eps, float weight_decay, int maximize,
                         float max_norm, float* total_norm, void* ws, hipStream_t s) {
  AdaTensors t{};
  t.count = count;
  int64_t total = 0, chunks = 0;
  for (int i = 0; i < count; ++i) {
    t.p[i] = params[i]; t.g[i] = grads[i]; t.sq[i] = square_avg[i]; t.acc[i] = acc_delta[i]; t.n[i] = numels[i];
    t.chunk0[i] = chunks;
    chunks += (numels[i] + kAdaChunk - 1) / kAdaChunk;
    if (numels[i] > total) total = numels[i];
  }
  t.chunk0[count] = chunks;
  const bool clip = max_norm > 0.f;
  double* part = (double*)ws;
  float* coef = (float*)(part + chunks);
  if (clip || total_norm) {
    if (chunks > 0) {
      hipLaunchKernelGGL(ada_sumsq_kernel, dim3((unsigned)chunks), dim3(256), 0, s, t, part);
      SVT_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(ada_norm_kernel, dim3(1), dim3(64), 0, s, t, part, max_norm, clip ? coef : nullptr, total_norm);
    SVT_LAUNCH_CHECK();
  }
  if (total > 0) {
    int64_t blocks = (total + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(ada_update_kernel, dim3((unsigned)blocks), dim3(256), 0, s, t, clip ? coef : nullptr, lr, rho, one_minus_rho, eps,
                       weight_decay, maximize);
    SVT_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace svt
