// Training step of the audio-visual recipe (N20EMv2/audio_visual/train_rca_av.py:174-185): the backward of the two RCA layers of
// FusionRCA on frozen features, and the device-side refresh of the handle's operand-format weights after the optimizer step.
//
// One RCA layer (post-LN): [q_s | k | v] = W_in kv + b_in, q_c = W_q q + b_q (the first D rows of W_in), a_s = attn(q_s, k, v),
// a_c = attn(q_c, k, v), y1 = kv + W_o (alpha a_s + (1 - alpha) a_c) + b_o, x = LN1(y1), y2 = x + W_2 relu(W_1 x + b_1) + b_2,
// out = LN2(y2).  The inputs are data: no gradient w.r.t. kv / q.  Every reduction has a fixed order -- no float atomics; a split
// reduction is combined by a second launch -- so two calls on the same inputs give the same bits.
#include "common.h"

namespace svt {
namespace {

template <typename T> __device__ __forceinline__ float ldv(const T* p, int64_t i) { return (float)p[i]; }
template <typename T> __device__ __forceinline__ void stv(T* p, int64_t i, float v) { p[i] = (T)v; }

__device__ __forceinline__ float wsum64(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wmax64(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// ---- weight refresh: fp32 master tensors -> the handle's operand-format copies (and transposes), one launch ----
// blockIdx.y = job; a job writes dst (rows x cols, or cols x rows when transposed) from src (rows x cols fp32)
template <typename TO>
__global__ __launch_bounds__(256) void rca_refresh_kernel(RcaRefreshJobs t) {
  const RcaRefreshJob& jb = t.j[blockIdx.y];
  const int64_t n = jb.rows * jb.cols;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    int64_t si = e;
    if (jb.transpose) {   // dst[a][b] (cols x rows) = src[b][a]
      const int64_t a = e / jb.rows, b = e - a * jb.rows;
      si = b * jb.cols + a;
    }
    const float v = jb.src[si];
    if (jb.f32) ((float*)jb.dst)[e] = v;
    else ((TO*)jb.dst)[e] = (TO)v;   // f32_to_bf16_kernel's conversion: the bits a fresh upload gives
  }
}

// ---- attention statistics ----
// log-sum-exp of scale q_i . k_j over the T keys of row i, per (clip, head, row): one wave per row, lanes over keys
template <typename TQ>
__global__ __launch_bounds__(256) void rca_attn_lse_kernel(const TQ* __restrict__ Q, long ldq, const TQ* __restrict__ K, long ldk, int B,
                                                           int T, int H, int dh, float scale, float* __restrict__ lse) {
  __shared__ float qs[4][128];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t gi = (int64_t)blockIdx.x * 4 + wave;   // (b * H + h) * T + i
  const bool ok = gi < (int64_t)B * H * T;
  const int64_t i = ok ? gi % T : 0, bh = ok ? gi / T : 0;
  const int64_t b = bh / H, h = bh % H;
  const TQ* qr = Q + (b * T + i) * ldq + h * dh;
  for (int d = lane; d < dh; d += 64) qs[wave][d] = ok ? ldv(qr, d) : 0.f;
  __syncthreads();
  if (!ok) return;
  float m = -INFINITY;
  for (int j = lane; j < T; j += 64) {
    const TQ* kr = K + (b * T + j) * ldk + h * dh;
    float s = 0.f;
    for (int d = 0; d < dh; ++d) s += qs[wave][d] * ldv(kr, d);
    m = fmaxf(m, s * scale);
  }
  m = wmax64(m);
  float l = 0.f;
  for (int j = lane; j < T; j += 64) {
    const TQ* kr = K + (b * T + j) * ldk + h * dh;
    float s = 0.f;
    for (int d = 0; d < dh; ++d) s += qs[wave][d] * ldv(kr, d);
    l += expf(s * scale - m);
  }
  l = wsum64(l);
  if (lane == 0) lse[gi] = m + logf(l);
}

// delta_i = rowsum(dO_i o O_i) per (stream, clip, head, row) with dO = coef[stream] * dblend; one thread per (row, head, stream)
template <typename TQ>
__global__ __launch_bounds__(256) void rca_attn_delta_kernel(const float* __restrict__ dbl, const TQ* __restrict__ O0, const TQ* __restrict__ O1,
                                                             int B, int T, int H, int dh, float c0, float c1, float* __restrict__ delta) {
  const int64_t n = (int64_t)B * T * H;
  const int64_t D = (int64_t)H * dh;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < 2 * n; g += (int64_t)gridDim.x * 256) {
    const int st = (int)(g / n);
    const int64_t e = g % n, row = e / H, h = e % H;
    const TQ* o = (st ? O1 : O0) + row * D + h * dh;
    const float* d = dbl + row * D + h * dh;
    float s = 0.f;
    for (int k = 0; k < dh; ++k) s += d[k] * ldv(o, k);
    const int64_t b = row / T, i = row % T;
    delta[(int64_t)st * n + (b * H + h) * T + i] = (st ? c1 : c0) * s;
  }
}

// ---- attention backward ----
// P = exp(scale q k^T - lse) recomputed from the saved log-sum-exp; dS = P o (dO v^T - delta).  No (B, H, T, T) tensor.
constexpr int kKT = 32;   // keys per tile
constexpr int kQT = 16;   // queries per tile

struct AttnBwdArgs {
  const void *q[2], *k, *v;        // q[0]: self query (qkv), q[1]: cross query (qc); k / v: the kv stream's
  long ldq[2], ldkv;
  const float* dbl;                // d(blend) (rows, D) fp32; dO of stream s = coef[s] * dbl
  float coef[2];
  const float *lse, *delta;        // [stream][B][H][T]
  float* dq[2];                    // dQ per stream, fp32, row strides lddq
  long lddq[2];
  float *dk, *dv;                  // fp32, row stride lddkv
  long lddkv;
  int B, T, H;
  float scale;
};

// one tile of S / dP between the query tile in Qs / dOs (rows q0 + [0, kQT)) and the key tile in Ks / Vs (keys j0 + [0, kKT)):
// thread t -> query t / 16, keys t % 16 and t % 16 + 16; writes P and dS (zero outside [0, T))
template <int DH>
__device__ __forceinline__ void attn_tile_pds(const float (&Qs)[kQT][DH + 1], const float (&dOs)[kQT][DH + 1], const float (&Ks)[kKT][DH + 1],
                                              const float (&Vs)[kKT][DH + 1], const float* lse_s, const float* del_s, int q0, int j0,
                                              int T, float scale, float (&Ps)[kQT][kKT + 1], float (&dSs)[kQT][kKT + 1]) {
  const int i = threadIdx.x >> 4;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int j = (threadIdx.x & 15) + 16 * u;
    float s = 0.f, dp = 0.f;
#pragma unroll 8
    for (int d = 0; d < DH; ++d) {
      s += Qs[i][d] * Ks[j][d];
      dp += dOs[i][d] * Vs[j][d];
    }
    const bool in = q0 + i < T && j0 + j < T;
    const float p = in ? expf(s * scale - lse_s[i]) : 0.f;
    Ps[i][j] = p;
    dSs[i][j] = p * (dp - del_s[i]);
  }
}

template <int DH, typename TQ>
__device__ __forceinline__ void load_rows(float (&dst)[kKT][DH + 1], int nrows, const TQ* base, long ld, int r0, int T, float mul = 1.f) {
  for (int e = threadIdx.x; e < nrows * DH; e += 256) {
    const int r = e / DH, d = e % DH;
    dst[r][d] = r0 + r < T ? mul * ldv(base + (int64_t)(r0 + r) * ld, d) : 0.f;
  }
}
template <int DH, typename TQ>
__device__ __forceinline__ void load_rows(float (&dst)[kQT][DH + 1], int nrows, const TQ* base, long ld, int r0, int T, float mul = 1.f) {
  for (int e = threadIdx.x; e < nrows * DH; e += 256) {
    const int r = e / DH, d = e % DH;
    dst[r][d] = r0 + r < T ? mul * ldv(base + (int64_t)(r0 + r) * ld, d) : 0.f;
  }
}

// dK / dV of one key tile: walks the query tiles of BOTH streams (the self and the cross query share k and v).  Grid (key tiles, B*H).
template <int DH, typename TQ>
__global__ __launch_bounds__(256) void rca_attn_bwd_kv_kernel(AttnBwdArgs a) {
  __shared__ float Ks[kKT][DH + 1], Vs[kKT][DH + 1], Qs[kQT][DH + 1], dOs[kQT][DH + 1];
  __shared__ float Ps[kQT][kKT + 1], dSs[kQT][kKT + 1], lse_s[kQT], del_s[kQT];
  constexpr int NU = DH / 8;
  const int T = a.T, H = a.H;
  const int j0 = blockIdx.x * kKT;
  const int bh = blockIdx.y, b = bh / H, h = bh % H;
  const int64_t D = (int64_t)H * DH;
  const TQ* kb = (const TQ*)a.k + (int64_t)b * T * a.ldkv + h * DH;
  const TQ* vb = (const TQ*)a.v + (int64_t)b * T * a.ldkv + h * DH;
  load_rows<DH>(Ks, kKT, kb, a.ldkv, j0, T);
  load_rows<DH>(Vs, kKT, vb, a.ldkv, j0, T);
  const int jj = threadIdx.x >> 3, dd = threadIdx.x & 7;
  float dk[NU], dv[NU];
#pragma unroll
  for (int u = 0; u < NU; ++u) { dk[u] = 0.f; dv[u] = 0.f; }
  for (int st = 0; st < 2; ++st) {
    const TQ* qb = (const TQ*)a.q[st] + (int64_t)b * T * a.ldq[st] + h * DH;
    const float* ob = a.dbl + (int64_t)b * T * D + h * DH;
    const float* ls = a.lse + ((int64_t)st * a.B * H + bh) * T;
    const float* dl = a.delta + ((int64_t)st * a.B * H + bh) * T;
    for (int q0 = 0; q0 < T; q0 += kQT) {
      __syncthreads();
      load_rows<DH>(Qs, kQT, qb, a.ldq[st], q0, T);
      load_rows<DH>(dOs, kQT, ob, D, q0, T, a.coef[st]);
      if (threadIdx.x < kQT) {
        const int i = q0 + threadIdx.x;
        lse_s[threadIdx.x] = i < T ? ls[i] : 0.f;
        del_s[threadIdx.x] = i < T ? dl[i] : 0.f;
      }
      __syncthreads();
      attn_tile_pds<DH>(Qs, dOs, Ks, Vs, lse_s, del_s, q0, j0, T, a.scale, Ps, dSs);
      __syncthreads();
#pragma unroll 4
      for (int i = 0; i < kQT; ++i) {
        const float p = Ps[i][jj], ds = dSs[i][jj];
#pragma unroll
        for (int u = 0; u < NU; ++u) {
          dv[u] += p * dOs[i][dd + 8 * u];
          dk[u] += ds * Qs[i][dd + 8 * u];
        }
      }
    }
  }
  if (j0 + jj < T) {
    const int64_t row = (int64_t)b * T + j0 + jj;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      a.dk[row * a.lddkv + h * DH + dd + 8 * u] = dk[u] * a.scale;
      a.dv[row * a.lddkv + h * DH + dd + 8 * u] = dv[u];
    }
  }
}

// dQ of one query tile of one stream.  Grid (query tiles, B*H, 2 streams).
template <int DH, typename TQ>
__global__ __launch_bounds__(256) void rca_attn_bwd_q_kernel(AttnBwdArgs a) {
  __shared__ float Ks[kKT][DH + 1], Vs[kKT][DH + 1], Qs[kQT][DH + 1], dOs[kQT][DH + 1];
  __shared__ float Ps[kQT][kKT + 1], dSs[kQT][kKT + 1], lse_s[kQT], del_s[kQT];
  constexpr int NU = DH / 16;
  const int T = a.T, H = a.H, st = blockIdx.z;
  const int q0 = blockIdx.x * kQT;
  const int bh = blockIdx.y, b = bh / H, h = bh % H;
  const int64_t D = (int64_t)H * DH;
  const TQ* kb = (const TQ*)a.k + (int64_t)b * T * a.ldkv + h * DH;
  const TQ* vb = (const TQ*)a.v + (int64_t)b * T * a.ldkv + h * DH;
  const TQ* qb = (const TQ*)a.q[st] + (int64_t)b * T * a.ldq[st] + h * DH;
  const float* ob = a.dbl + (int64_t)b * T * D + h * DH;
  const float* ls = a.lse + ((int64_t)st * a.B * H + bh) * T;
  const float* dl = a.delta + ((int64_t)st * a.B * H + bh) * T;
  load_rows<DH>(Qs, kQT, qb, a.ldq[st], q0, T);
  load_rows<DH>(dOs, kQT, ob, D, q0, T, a.coef[st]);
  if (threadIdx.x < kQT) {
    const int i = q0 + threadIdx.x;
    lse_s[threadIdx.x] = i < T ? ls[i] : 0.f;
    del_s[threadIdx.x] = i < T ? dl[i] : 0.f;
  }
  const int ii = threadIdx.x >> 4, dd = threadIdx.x & 15;
  float dq[NU];
#pragma unroll
  for (int u = 0; u < NU; ++u) dq[u] = 0.f;
  for (int j0 = 0; j0 < T; j0 += kKT) {
    __syncthreads();
    load_rows<DH>(Ks, kKT, kb, a.ldkv, j0, T);
    load_rows<DH>(Vs, kKT, vb, a.ldkv, j0, T);
    __syncthreads();
    attn_tile_pds<DH>(Qs, dOs, Ks, Vs, lse_s, del_s, q0, j0, T, a.scale, Ps, dSs);
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < kKT; ++j) {
      const float ds = dSs[ii][j];
#pragma unroll
      for (int u = 0; u < NU; ++u) dq[u] += ds * Ks[j][dd + 16 * u];
    }
  }
  if (q0 + ii < T) {
    const int64_t row = (int64_t)b * T + q0 + ii;
#pragma unroll
    for (int u = 0; u < NU; ++u) a.dq[st][row * a.lddq[st] + h * DH + dd + 16 * u] = dq[u] * a.scale;
  }
}

// ---- LayerNorm backward ----
// y = LN(x + add): one wave per row, mean / rstd recomputed from the saved fp32 input as layernorm_kernel computes them;
// dx = rstd (g - mean(g) - xhat mean(g xhat)), g = dy gamma.  stats[2 row] = {mean, rstd} for the parameter gradients.
template <typename TO>
__global__ __launch_bounds__(256) void rca_ln_bwd_kernel(const float* __restrict__ x, const float* __restrict__ add, const float* __restrict__ gamma,
                                                         const float* __restrict__ dy, int64_t rows, int D, float eps, float* __restrict__ dxF,
                                                         TO* __restrict__ dxT, float* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + row * D;
  const float* ar = add + row * D;
  const float* dr = dy + row * D;
  float s = 0.f;
  for (int i = lane; i < D; i += 64) s += xr[i] + ar[i];
  const float mean = wsum64(s) / (float)D;
  float q = 0.f;
  for (int i = lane; i < D; i += 64) { const float d = xr[i] + ar[i] - mean; q += d * d; }
  const float rstd = rsqrtf(wsum64(q) / (float)D + eps);
  float sg = 0.f, sgx = 0.f;
  for (int i = lane; i < D; i += 64) {
    const float g = dr[i] * gamma[i], xh = (xr[i] + ar[i] - mean) * rstd;
    sg += g;
    sgx += g * xh;
  }
  const float mg = wsum64(sg) / (float)D, mgx = wsum64(sgx) / (float)D;
  for (int i = lane; i < D; i += 64) {
    const float g = dr[i] * gamma[i], xh = (xr[i] + ar[i] - mean) * rstd;
    const float v = rstd * (g - mg - xh * mgx);
    dxF[row * D + i] = v;
    if (dxT) stv(dxT, row * D + i, v);
  }
  if (lane == 0) { stats[2 * row] = mean; stats[2 * row + 1] = rstd; }
}

// d gamma / d beta: grid (column tiles of 64, slabs); 4 row groups per block combined in LDS in a fixed order; part[slab][2][D]
__global__ __launch_bounds__(256) void rca_ln_param_partial_kernel(const float* __restrict__ x, const float* __restrict__ add,
                                                                   const float* __restrict__ dy, const float* __restrict__ stats, int64_t rows,
                                                                   int D, int64_t rows_per_slab, float* __restrict__ part) {
  __shared__ float red[2][4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), rg = threadIdx.x >> 6;
  const int64_t slab = blockIdx.y, r0 = slab * rows_per_slab;
  const int64_t r1 = r0 + rows_per_slab < rows ? r0 + rows_per_slab : rows;
  float sg = 0.f, sb = 0.f;
  if (c < D)
    for (int64_t r = r0 + rg; r < r1; r += 4) {
      const float g = dy[r * D + c];
      sg += g * ((x[r * D + c] + add[r * D + c] - stats[2 * r]) * stats[2 * r + 1]);
      sb += g;
    }
  red[0][rg][threadIdx.x & 63] = sg;
  red[1][rg][threadIdx.x & 63] = sb;
  __syncthreads();
  if (rg < 2 && c < D) {
    const int l = threadIdx.x & 63;
    const float v = (red[rg][0][l] + red[rg][1][l]) + (red[rg][2][l] + red[rg][3][l]);
    part[(slab * 2 + rg) * D + c] = v;
  }
}

__global__ __launch_bounds__(256) void rca_ln_param_combine_kernel(const float* __restrict__ part, int64_t slabs, int D, float* __restrict__ dg,
                                                                   float* __restrict__ db) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= 2 * (int64_t)D) return;
  const int w = (int)(e / D), c = (int)(e % D);
  float s = 0.f;
  for (int64_t k = 0; k < slabs; ++k) s += part[(k * 2 + w) * D + c];
  (w ? db : dg)[c] = s;
}

// ---- ReLU mask: dh *= (h > 0) in place (fp32), and the operand-type copy for the next product ----
template <typename TO>
__global__ __launch_bounds__(256) void rca_relu_mask_kernel(float* __restrict__ dh, const TO* __restrict__ h, int64_t n, TO* __restrict__ dhT) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const float v = ldv(h, e) > 0.f ? dh[e] : 0.f;
    dh[e] = v;
    if (dhT) stv(dhT, e, v);
  }
}

// ---- weight gradient: dW (N x C) = sum over rows of dY[r][n] X[r][c] ----
// The rows are the concatenation of up to two segments (dY_s, X_s, rows each): the in-projection's first D rows take the self and the
// cross query in one sum.  Grid (column tiles of 64, n tiles of 64, slabs of rows); four waves, each a 32 x 32 block of dW on
// v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulate: dY stays fp32, a 16-bit X is widened), 32-row chunks staged in LDS.
// A = dY^T: lane l supplies A[n = l & 31][k = l >> 5] = Ys[k][n]; B = X: B[k = l >> 5][c = l & 31] = Xs[k][c]; C/D: column l & 31,
// row (v & 3) + 8 (v >> 2) + 4 (l >> 5) of register v.  slabs == 1 writes dW; otherwise part[slab][N][C], summed in slab order by
// rca_wgrad_combine_kernel.
struct WgradSeg {
  const float* dy[2];
  const void* x[2];
  long ldy[2], ldx[2];
  int nseg;
};
constexpr int kWgK = 32;   // rows per LDS chunk
typedef float f32x16 __attribute__((ext_vector_type(16)));

template <typename TX>
__global__ __launch_bounds__(256) void rca_wgrad_partial_kernel(WgradSeg sg, int64_t rows, int N, int C, int64_t rows_per_slab, float* __restrict__ out) {
  __shared__ float Ys[kWgK][64], Xs[kWgK][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wn = wave >> 1, wc = wave & 1;
  const int n0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
  const int64_t vrows = rows * sg.nseg;
  const int64_t r0 = (int64_t)blockIdx.z * rows_per_slab;
  const int64_t r1 = r0 + rows_per_slab < vrows ? r0 + rows_per_slab : vrows;
  f32x16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  for (int64_t r = r0; r < r1; r += kWgK) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kWgK * 64 / 256; ++u) {
      const int e = threadIdx.x + 256 * u, k = e >> 6, col = e & 63;
      const int64_t vr = r + k;
      float yv = 0.f, xv = 0.f;
      if (vr < r1) {
        const int s = vr >= rows ? 1 : 0;
        const int64_t rr = vr - (s ? rows : 0);
        if (n0 + col < N) yv = sg.dy[s][rr * sg.ldy[s] + n0 + col];
        if (c0 + col < C) xv = ldv((const TX*)sg.x[s], rr * sg.ldx[s] + c0 + col);
      }
      Ys[k][col] = yv;
      Xs[k][col] = xv;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kWgK; kk += 2) {
      const float a = Ys[kk + (lane >> 5)][wn * 32 + (lane & 31)];
      const float b = Xs[kk + (lane >> 5)][wc * 32 + (lane & 31)];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
    }
  }
  float* o = out + (int64_t)blockIdx.z * N * C;
  const int c = c0 + wc * 32 + (lane & 31);
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int n = n0 + wn * 32 + (v & 3) + 8 * (v >> 2) + 4 * (lane >> 5);
    if (n < N && c < C) o[(int64_t)n * C + c] = acc[v];
  }
}

// blocks [0, dw_blocks): dW[e] = sum of the slab partials in slab order (skipped when slabs == 1: the partial kernel wrote dW);
// the next ceil(N / 64) blocks: db[n] = sum over the (virtual) rows of dY, 4 row groups combined in a fixed order
__global__ __launch_bounds__(256) void rca_wgrad_combine_kernel(const float* __restrict__ part, int64_t slabs, int64_t nc, int dw_blocks,
                                                                WgradSeg sg, int64_t rows, int N, float* __restrict__ dw, float* __restrict__ db) {
  __shared__ float red[4][64];
  if ((int)blockIdx.x < dw_blocks) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nc) return;
    float s = 0.f;
    for (int64_t k = 0; k < slabs; ++k) s += part[k * nc + e];
    dw[e] = s;
    return;
  }
  const int n = ((int)blockIdx.x - dw_blocks) * 64 + (threadIdx.x & 63), rg = threadIdx.x >> 6;
  float s = 0.f;
  if (n < N)
    for (int seg = 0; seg < sg.nseg; ++seg)
      for (int64_t r = rg; r < rows; r += 4) s += sg.dy[seg][r * sg.ldy[seg] + n];
  red[rg][threadIdx.x & 63] = s;
  __syncthreads();
  if (rg == 0 && n < N) {
    const int l = threadIdx.x & 63;
    db[n] = (red[0][l] + red[1][l]) + (red[2][l] + red[3][l]);
  }
}

// ---- Linear backward, data half: dx (rows x D) = dy (rows x N) W (N x D) ----
__global__ __launch_bounds__(256) void linear_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ w, int64_t rows, int D, int N,
                                                           float* __restrict__ dx) {
  const int64_t r = blockIdx.x;
  const float* d = dy + r * N;
  for (int c = threadIdx.x * 4; c < D; c += 1024) {
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int n = 0; n < N; ++n) acc += d[n] * *(const f32x4*)(w + (int64_t)n * D + c);
    *(f32x4*)(dx + r * D + c) = acc;
  }
}

unsigned grid_1d(int64_t n, int64_t cap = 4096) {
  int64_t b = (n + 255) / 256;
  if (b > cap) b = cap;
  return (unsigned)(b < 1 ? 1 : b);
}

}  // namespace

int launch_rca_refresh(int prec, const RcaRefreshJobs& jobs, hipStream_t s) {
  int64_t most = 0;
  for (int i = 0; i < jobs.n; ++i) most = std::max<int64_t>(most, jobs.j[i].rows * jobs.j[i].cols);
  const dim3 grid(grid_1d(most, 1024), (unsigned)jobs.n);
  if (prec) hipLaunchKernelGGL(rca_refresh_kernel<bf16_t>, grid, dim3(256), 0, s, jobs);
  else hipLaunchKernelGGL(rca_refresh_kernel<float>, grid, dim3(256), 0, s, jobs);
  SVT_LAUNCH_CHECK();
  return 0;
}

int launch_rca_attn_lse(int prec, const void* Q, long ldq, const void* K, long ldk, int B, int T, int H, int dh, float scale, float* lse,
                        hipStream_t s) {
  if (dh > 128) { set_error("rca training: head size above 128"); return -1; }
  const unsigned grid = (unsigned)(((int64_t)B * H * T + 3) / 4);
  if (prec) hipLaunchKernelGGL(rca_attn_lse_kernel<bf16_t>, dim3(grid), dim3(256), 0, s, (const bf16_t*)Q, ldq, (const bf16_t*)K, ldk, B, T, H, dh, scale, lse);
  else hipLaunchKernelGGL(rca_attn_lse_kernel<float>, dim3(grid), dim3(256), 0, s, (const float*)Q, ldq, (const float*)K, ldk, B, T, H, dh, scale, lse);
  SVT_LAUNCH_CHECK();
  return 0;
}

int launch_rca_attn_bwd(int prec, const RcaAttnBwd& p, hipStream_t s) {
  const int dh = p.dh;
  if (dh != 64 && dh != 128) { set_error("rca training: the attention backward takes head sizes 64 and 128"); return -1; }
  const int64_t n = (int64_t)p.B * p.T * p.H;
  if (prec) hipLaunchKernelGGL(rca_attn_delta_kernel<bf16_t>, dim3(grid_1d(2 * n, 1 << 20)), dim3(256), 0, s, p.dbl, (const bf16_t*)p.o[0], (const bf16_t*)p.o[1], p.B, p.T, p.H, dh, p.coef[0], p.coef[1], p.delta);
  else hipLaunchKernelGGL(rca_attn_delta_kernel<float>, dim3(grid_1d(2 * n, 1 << 20)), dim3(256), 0, s, p.dbl, (const float*)p.o[0], (const float*)p.o[1], p.B, p.T, p.H, dh, p.coef[0], p.coef[1], p.delta);
  SVT_LAUNCH_CHECK();
  AttnBwdArgs a;
  for (int i = 0; i < 2; ++i) { a.q[i] = p.q[i]; a.ldq[i] = p.ldq[i]; a.coef[i] = p.coef[i]; a.dq[i] = p.dq[i]; a.lddq[i] = p.lddq[i]; }
  a.k = p.k; a.v = p.v; a.ldkv = p.ldkv; a.dbl = p.dbl; a.lse = p.lse; a.delta = p.delta; a.dk = p.dk; a.dv = p.dv; a.lddkv = p.lddkv;
  a.B = p.B; a.T = p.T; a.H = p.H; a.scale = p.scale;
  const dim3 gkv((unsigned)((p.T + kKT - 1) / kKT), (unsigned)(p.B * p.H));
  const dim3 gq((unsigned)((p.T + kQT - 1) / kQT), (unsigned)(p.B * p.H), 2);
#define SVT_ATTN_BWD(DH, TQ)                                                           \
  do {                                                                                \
    hipLaunchKernelGGL((rca_attn_bwd_kv_kernel<DH, TQ>), gkv, dim3(256), 0, s, a);   \
    SVT_LAUNCH_CHECK();                                                               \
    hipLaunchKernelGGL((rca_attn_bwd_q_kernel<DH, TQ>), gq, dim3(256), 0, s, a);     \
    SVT_LAUNCH_CHECK();                                                               \
  } while (0)
  if (prec) { if (dh == 64) SVT_ATTN_BWD(64, bf16_t); else SVT_ATTN_BWD(128, bf16_t); }
  else { if (dh == 64) SVT_ATTN_BWD(64, float); else SVT_ATTN_BWD(128, float); }
#undef SVT_ATTN_BWD
  return 0;
}

int64_t rca_ln_slabs(int64_t rows) {
  int64_t sl = (rows + 63) / 64;
  return sl > 64 ? 64 : (sl < 1 ? 1 : sl);
}
size_t rca_ln_bwd_scratch_bytes(int64_t rows, int D) { return ((size_t)rows * 2 + (size_t)rca_ln_slabs(rows) * 2 * D) * sizeof(float); }

int launch_rca_ln_bwd(int prec, const float* x, const float* add, const float* gamma, const float* dy, int64_t rows, int D, float eps,
                      float* dxF, void* dxT, float* dgamma, float* dbeta, void* scratch, hipStream_t s) {
  float* stats = (float*)scratch;
  float* part = stats + 2 * rows;
  const unsigned grid = (unsigned)((rows + 3) / 4);
  if (prec) hipLaunchKernelGGL(rca_ln_bwd_kernel<bf16_t>, dim3(grid), dim3(256), 0, s, x, add, gamma, dy, rows, D, eps, dxF, (bf16_t*)dxT, stats);
  else hipLaunchKernelGGL(rca_ln_bwd_kernel<float>, dim3(grid), dim3(256), 0, s, x, add, gamma, dy, rows, D, eps, dxF, (float*)dxT, stats);
  SVT_LAUNCH_CHECK();
  const int64_t slabs = rca_ln_slabs(rows), rps = (rows + slabs - 1) / slabs;
  hipLaunchKernelGGL(rca_ln_param_partial_kernel, dim3((unsigned)((D + 63) / 64), (unsigned)slabs), dim3(256), 0, s, x, add, dy, stats, rows, D, rps, part);
  SVT_LAUNCH_CHECK();
  hipLaunchKernelGGL(rca_ln_param_combine_kernel, dim3(grid_1d(2 * (int64_t)D, 1 << 20)), dim3(256), 0, s, part, slabs, D, dgamma, dbeta);
  SVT_LAUNCH_CHECK();
  return 0;
}

int launch_rca_relu_mask(int prec, float* dh, const void* h, int64_t n, void* dhT, hipStream_t s) {
  if (prec) hipLaunchKernelGGL(rca_relu_mask_kernel<bf16_t>, dim3(grid_1d(n)), dim3(256), 0, s, dh, (const bf16_t*)h, n, (bf16_t*)dhT);
  else hipLaunchKernelGGL(rca_relu_mask_kernel<float>, dim3(grid_1d(n)), dim3(256), 0, s, dh, (const float*)h, n, (float*)nullptr);
  SVT_LAUNCH_CHECK();
  return 0;
}

// slabs: about 1024 workgroups in all, at least 256 rows per slab; a function of the shapes only
int64_t rca_wgrad_slabs(int64_t vrows, int N, int C) {
  const int64_t tiles = (int64_t)((N + 63) / 64) * ((C + 63) / 64);
  int64_t sl = (1024 + tiles - 1) / tiles;
  const int64_t cap = (vrows + 255) / 256;
  if (sl > cap) sl = cap;
  return sl < 1 ? 1 : sl;
}
size_t rca_wgrad_scratch_bytes(int64_t vrows, int N, int C) {
  const int64_t sl = rca_wgrad_slabs(vrows, N, C);
  return sl > 1 ? (size_t)sl * N * C * sizeof(float) : 0;
}

int launch_rca_wgrad(int prec, const RcaWgrad& w, float* dw, float* db, void* scratch, hipStream_t s) {
  WgradSeg sg;
  sg.nseg = w.nseg;
  for (int i = 0; i < 2; ++i) { sg.dy[i] = w.dy[i]; sg.x[i] = w.x[i]; sg.ldy[i] = w.ldy[i]; sg.ldx[i] = w.ldx[i]; }
  const int64_t vrows = w.rows * w.nseg;
  const int64_t slabs = rca_wgrad_slabs(vrows, w.N, w.C);
  const int64_t rps = ((vrows + slabs - 1) / slabs + kWgK - 1) / kWgK * kWgK;
  float* out = slabs > 1 ? (float*)scratch : dw;
  const dim3 grid((unsigned)((w.C + 63) / 64), (unsigned)((w.N + 63) / 64), (unsigned)slabs);
  if (prec) hipLaunchKernelGGL(rca_wgrad_partial_kernel<bf16_t>, grid, dim3(256), 0, s, sg, w.rows, w.N, w.C, rps, out);
  else hipLaunchKernelGGL(rca_wgrad_partial_kernel<float>, grid, dim3(256), 0, s, sg, w.rows, w.N, w.C, rps, out);
  SVT_LAUNCH_CHECK();
  const int64_t nc = (int64_t)w.N * w.C;
  const int dw_blocks = slabs > 1 ? (int)((nc + 255) / 256) : 0;
  const int b_blocks = db ? (w.N + 63) / 64 : 0;
  if (dw_blocks + b_blocks > 0) {
    hipLaunchKernelGGL(rca_wgrad_combine_kernel, dim3((unsigned)(dw_blocks + b_blocks)), dim3(256), 0, s, (const float*)scratch, slabs, nc, dw_blocks,
                       sg, w.rows, w.N, dw, db);
    SVT_LAUNCH_CHECK();
  }
  return 0;
}

int launch_linear_dgrad(const float* dy, const float* w, int64_t rows, int D, int N, float* dx, hipStream_t s) {
  hipLaunchKernelGGL(linear_dgrad_kernel, dim3((unsigned)rows), dim3(256), 0, s, dy, w, rows, D, N, dx);
  SVT_LAUNCH_CHECK();
  return 0;
}

}  // namespace svt
