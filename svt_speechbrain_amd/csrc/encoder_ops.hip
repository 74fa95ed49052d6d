// What the encoder and RCA entry points (api_encoder.hip, api_rca.hip) launch between the products: the 16-bit operand copy, fills and
// copies, the positional conv's gather / scatter, the helpers of the materialised-score path, WavLM's relative position bias.
#include "device_util.h"

namespace svt {
namespace {
__global__ void f32_to_bf16_kernel(const float* in, bf16_t* out, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) out[i] = (bf16_t)in[i];
}
}  // namespace
int launch_f32_to_bf16(const float* in, bf16_t* out, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL(f32_to_bf16_kernel, dim3(grid_for(n)), dim3(256), 0, s, in, out, n);
  SVT_LAUNCH_CHECK();
  return 0;
}

// Fills and copies as KERNELS of this library, not hipMemsetAsync / hipMemcpyAsync (round 6): inside a captured hipGraph the runtime's
// memset node ran out of order from the second replay on -- the statistics region of the workspace was zeroed AFTER the moments kernel had
// written it, the output norm saw (0, 0) and scaled by 1 / sqrt(eps) (tools/graph_debug.py; tests/test_gpu_graph.py).  A kernel
// node keeps stream order.  Sizes and addresses are multiples of 16 bytes (the workspace carve is 256-byte aligned).
namespace {
__global__ __launch_bounds__(256) void zero16_kernel(uint4* p, int64_t n16) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n16; i += stride) p[i] = uint4{0u, 0u, 0u, 0u};
}
__global__ __launch_bounds__(256) void copy16_kernel(const uint4* in, uint4* out, int64_t n16, const float* in_tail, float* out_tail, int n_tail) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (i < n_tail) out_tail[i] = in_tail[i];
  for (; i < n16; i += stride) out[i] = in[i];
}
// rows x cols fp32 block with row pitch ld (elements) set to zero (cols, ld multiples of 4, 16-byte aligned base: the launcher checks)
__global__ __launch_bounds__(256) void zero_cols_kernel(float* p, int64_t rows, int cols4, int64_t ld) {
  const int64_t n = rows * cols4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / cols4;
    const int c = (int)(i - r * cols4);
    *(float4*)(p + r * ld + 4 * c) = float4{0.f, 0.f, 0.f, 0.f};
  }
}
}  // namespace
int launch_zero_bytes(void* p, size_t bytes, hipStream_t s) {
  if (bytes % 16 || ((uintptr_t)p & 15)) { set_error("launch_zero_bytes: 16-byte granularity"); return -1; }
  if (!bytes) return 0;
  hipLaunchKernelGGL(zero16_kernel, dim3(grid_for((int64_t)(bytes / 16))), dim3(256), 0, s, (uint4*)p, (int64_t)(bytes / 16));
  SVT_LAUNCH_CHECK();
  return 0;
}
int launch_copy_f32(const float* in, float* out, int64_t n, hipStream_t s) {
  if (n <= 0) return 0;
  if (!aligned(15, in, out)) { set_error("launch_copy_f32: 16-byte alignment"); return -1; }
  const int64_t n16 = n / 4;
  hipLaunchKernelGGL(copy16_kernel, dim3(grid_for(n16 > 0 ? n16 : 1)), dim3(256), 0, s, (const uint4*)in, (uint4*)out, n16, in + 4 * n16, out + 4 * n16,
                     (int)(n - 4 * n16));
  SVT_LAUNCH_CHECK();
  return 0;
}
int launch_zero_cols(float* p, int64_t rows, int cols, int64_t ld, hipStream_t s) {
  if (cols % 4 || ld % 4 || ((uintptr_t)p & 15)) { set_error("launch_zero_cols: 16-byte granularity"); return -1; }
  if (rows <= 0 || cols <= 0) return 0;
  hipLaunchKernelGGL(zero_cols_kernel, dim3(grid_for(rows * (cols / 4))), dim3(256), 0, s, p, rows, cols / 4, ld);
  SVT_LAUNCH_CHECK();
  return 0;
}

namespace {
template <typename TO>
__global__ void posconv_gather_kernel(const float* h, int B, int T, int D, int G, int kp, int Tp, TO* out, const float* sc, const float* sh) {
  const int cg = D / G;
  const int64_t n = (int64_t)B * G * Tp * cg;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const int ci = (int)(i % cg);
    int64_t r = i / cg;
    const int tp = (int)(r % Tp); r /= Tp;
    const int g = (int)(r % G);
    const int b = (int)(r / G);
    const int t = tp - kp / 2;
    float v = (t >= 0 && t < T) ? h[((int64_t)b * T + t) * D + g * cg + ci] : 0.f;
    if (sc && t >= 0 && t < T) v = fmaf(v, sc[g * cg + ci], sh[g * cg + ci]);  // eval-mode BatchNorm1d in front of the conv: the zero padding stays zero
    st<TO>(out, i, v);
  }
}

// bf16 output, 8 channels (16 bytes out, 32 bytes in) per thread
__global__ void posconv_gather_bf16x8_kernel(const float* h, int B, int T, int D, int G, int kp, int Tp, bf16_t* out, const float* sc, const float* sh) {
  const int cg = D / G, c8 = cg / 8;
  const int64_t n = (int64_t)B * G * Tp * c8;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int ci = (int)(i % c8) * 8;
    int64_t r = i / c8;
    const int tp = (int)(r % Tp); r /= Tp;
    const int g = (int)(r % G);
    const int b = (int)(r / G);
    const int t = tp - kp / 2;
    bf16x8 o;
    if (t >= 0 && t < T) {
      const float* src = h + ((int64_t)b * T + t) * D + g * cg + ci;
      float4 a = *(const float4*)src, c = *(const float4*)(src + 4);
      if (sc) {
        const float4 s0 = *(const float4*)(sc + g * cg + ci), s1 = *(const float4*)(sc + g * cg + ci + 4);
        const float4 t0 = *(const float4*)(sh + g * cg + ci), t1 = *(const float4*)(sh + g * cg + ci + 4);
        a = float4{fmaf(a.x, s0.x, t0.x), fmaf(a.y, s0.y, t0.y), fmaf(a.z, s0.z, t0.z), fmaf(a.w, s0.w, t0.w)};
        c = float4{fmaf(c.x, s1.x, t1.x), fmaf(c.y, s1.y, t1.y), fmaf(c.z, s1.z, t1.z), fmaf(c.w, s1.w, t1.w)};
      }
      o[0] = (bf16_t)a.x; o[1] = (bf16_t)a.y; o[2] = (bf16_t)a.z; o[3] = (bf16_t)a.w;
      o[4] = (bf16_t)c.x; o[5] = (bf16_t)c.y; o[6] = (bf16_t)c.z; o[7] = (bf16_t)c.w;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = (bf16_t)0.f;
    }
    *(bf16x8*)(out + (((int64_t)b * G + g) * Tp + tp) * cg + ci) = o;
  }
}
}  // namespace
int g_glue_kernel_id = 0;  // svt_debug_set key 45 (query): the kernel the last launch of the encoder's glue chose (include/svt_mi355.h lists the ids)
int launch_posconv_gather(int prec, const float* h, int B, int T, int D, int G, int kp, int Tp, void* out, hipStream_t s, const float* sc,
                          const float* sh) {
  const int64_t n = (int64_t)B * Tp * D;
  if (prec && (D / G) % 8 == 0 && aligned(15, h, out)) {
    hipLaunchKernelGGL(posconv_gather_bf16x8_kernel, dim3(grid_for(n / 8)), dim3(256), 0, s, h, B, T, D, G, kp, Tp, (bf16_t*)out, sc, sh);
    g_glue_kernel_id = 13;
  } else if (prec) {
    hipLaunchKernelGGL((posconv_gather_kernel<bf16_t>), dim3(grid_for(n)), dim3(256), 0, s, h, B, T, D, G, kp, Tp,
                       (bf16_t*)out, sc, sh);
    g_glue_kernel_id = 12;
  } else {
    hipLaunchKernelGGL((posconv_gather_kernel<float>), dim3(grid_for(n)), dim3(256), 0, s, h, B, T, D, G, kp, Tp,
                       (float*)out, sc, sh);
    g_glue_kernel_id = 11;
  }
  SVT_LAUNCH_CHECK();
  return 0;
}

// multi-frame positional conv: y[g][b*Tq + q][j*cg + c] (bf16, GELU applied) holds frame t = q*P + j of group g;
// pre[b][t][g*cg + c] = h[b][t][g*cg + c] + y[...]  (8 channels per thread)
template <typename TY>
__global__ void posconv_scatter_add_kernel(const float* h, const TY* y, int B, int T, int D, int G, int P, int Tq, float* pre) {
  const int cg = D / G, c8n = D / 8;
  const int64_t n = (int64_t)B * T * c8n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int ch = (int)(i % c8n) * 8;
    const int64_t r = i / c8n;
    const int t = (int)(r % T), b = (int)(r / T);
    const int g = ch / cg, c = ch - g * cg;
    const int q = t / P, j = t - q * P;
    const TY* yp = y + (((int64_t)g * B + b) * Tq + q) * (P * cg) + j * cg + c;
    float v[8];
    if constexpr (sizeof(TY) == 2) {
      const bf16x8 vb = *(const bf16x8*)yp;
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = (float)vb[i];
    } else {
      const float4 a0 = *(const float4*)yp, a1 = *(const float4*)(yp + 4);
      v[0] = a0.x; v[1] = a0.y; v[2] = a0.z; v[3] = a0.w; v[4] = a1.x; v[5] = a1.y; v[6] = a1.z; v[7] = a1.w;
    }
    const float* hp = h + r * D + ch;
    const float4 h0 = *(const float4*)hp, h1 = *(const float4*)(hp + 4);
    float* op = pre + r * D + ch;
    *(float4*)op = float4{h0.x + v[0], h0.y + v[1], h0.z + v[2], h0.w + v[3]};
    *(float4*)(op + 4) = float4{h1.x + v[4], h1.y + v[5], h1.z + v[6], h1.w + v[7]};
  }
}
int launch_posconv_scatter_add(const float* h, const void* y, int B, int T, int D, int G, int P, int Tq, float* pre, hipStream_t s, int y_f32) {
  const int64_t n = (int64_t)B * T * (D / 8);
  if (y_f32) hipLaunchKernelGGL((posconv_scatter_add_kernel<float>), dim3(grid_for(n)), dim3(256), 0, s, h, (const float*)y, B, T, D, G, P, Tq, pre);
  else hipLaunchKernelGGL((posconv_scatter_add_kernel<bf16_t>), dim3(grid_for(n)), dim3(256), 0, s, h, (const bf16_t*)y, B, T, D, G, P, Tq, pre);
  g_glue_kernel_id = y_f32 ? 21 : 22;
  SVT_LAUNCH_CHECK();
  return 0;
}

namespace {
template <typename TO>
__global__ __launch_bounds__(256) void softmax_rows_kernel(const float* S, int64_t rows, int T, int Tp, TO* P) {
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
  for (int i = lane; i < Tp; i += 64) st<TO>(P, row * Tp + i, i < T ? expf(s[i] - mx) * inv : 0.f);
}

// (B*T, ld)[.., voff + h*dh + d] -> Vt (B, H, dh, Tp); 32x32 LDS tile transpose, zero padded keys
template <typename TV>
__global__ __launch_bounds__(256) void transpose_v_kernel(const TV* qkv, int T, int H, int dh, long ldq, long voff,
                                                          int Tp, TV* Vt) {
  __shared__ float tile[32][33];
  const int bh = blockIdx.z;
  const int b = bh / H, h = bh % H;
  const int t0 = blockIdx.x * 32, d0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int i = ty; i < 32; i += 8) {
    const int t = t0 + i, d = d0 + tx;
    tile[i][tx] = (t < T && d < dh) ? ld<TV>(qkv, ((long)b * T + t) * ldq + voff + (long)h * dh + d) : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int d = d0 + i, t = t0 + tx;
    if (d < dh && t < Tp) st<TV>(Vt, (((long)b * H + h) * dh + d) * Tp + t, tile[tx][i]);
  }
}
}  // namespace
int launch_softmax_rows(int prec, const float* S, int64_t rows, int T, int Tp, void* P, hipStream_t s) {
  const dim3 grid((unsigned)((rows + 3) / 4));
  if (prec)
    hipLaunchKernelGGL((softmax_rows_kernel<bf16_t>), grid, dim3(256), 0, s, S, rows, T, Tp, (bf16_t*)P);
  else
    hipLaunchKernelGGL((softmax_rows_kernel<float>), grid, dim3(256), 0, s, S, rows, T, Tp, (float*)P);
  SVT_LAUNCH_CHECK();
  return 0;
}
int launch_transpose_v(int prec, const void* qkv, int B, int T, int H, int dh, long ld, long voff, int Tp, void* Vt,
                       hipStream_t s) {
  dim3 grid((Tp + 31) / 32, (dh + 31) / 32, B * H);
  if (prec)
    hipLaunchKernelGGL((transpose_v_kernel<bf16_t>), grid, dim3(256), 0, s, (const bf16_t*)qkv, T, H, dh, ld, voff, Tp,
                       (bf16_t*)Vt);
  else
    hipLaunchKernelGGL((transpose_v_kernel<float>), grid, dim3(256), 0, s, (const float*)qkv, T, H, dh, ld, voff, Tp,
                       (float*)Vt);
  SVT_LAUNCH_CHECK();
  return 0;
}

namespace {
template <typename TX>
__global__ void axpby_kernel(const TX* x, const TX* y, float a, float b, TX* out, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) st<TX>(out, i, a * ld<TX>(x, i) + b * ld<TX>(y, i));
}

template <typename TO>
__global__ void add_pe_kernel(const float* x, int B, int T, int Tsrc, int D, const float* pe, float* outF, TO* outT) {
  const int64_t n = (int64_t)B * T * D;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const int d = (int)(i % D);
    const int64_t r = i / D;
    const int t = (int)(r % T);
    const int b = (int)(r / T);
    const float xv = t < Tsrc ? x[((int64_t)b * Tsrc + t) * D + d] : 0.f;
    const float v = xv + pe[(int64_t)t * D + d];
    outF[i] = v;
    if (outT) st<TO>(outT, i, v);
  }
}

__global__ void add_f32_kernel(const float* a, const float* b, float* out, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) out[i] = a[i] + b[i];
}
}  // namespace
int launch_axpby(int prec, const void* x, const void* y, float a, float b, void* out, int64_t n, hipStream_t s) {
  if (prec)
    hipLaunchKernelGGL((axpby_kernel<bf16_t>), dim3(grid_for(n)), dim3(256), 0, s, (const bf16_t*)x, (const bf16_t*)y,
                       a, b, (bf16_t*)out, n);
  else
    hipLaunchKernelGGL((axpby_kernel<float>), dim3(grid_for(n)), dim3(256), 0, s, (const float*)x, (const float*)y, a,
                       b, (float*)out, n);
  SVT_LAUNCH_CHECK();
  return 0;
}
int launch_add_pe(int prec, const float* x, int B, int T, int Tsrc, int D, const float* pe, float* outF, void* outT,
                  hipStream_t s) {
  const int64_t n = (int64_t)B * T * D;
  if (prec)
    hipLaunchKernelGGL((add_pe_kernel<bf16_t>), dim3(grid_for(n)), dim3(256), 0, s, x, B, T, Tsrc, D, pe, outF,
                       (bf16_t*)outT);
  else
    hipLaunchKernelGGL((add_pe_kernel<float>), dim3(grid_for(n)), dim3(256), 0, s, x, B, T, Tsrc, D, pe, outF,
                       (float*)nullptr);
  SVT_LAUNCH_CHECK();
  return 0;
}
int launch_add_f32(const float* a, const float* b, float* out, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL(add_f32_kernel, dim3(grid_for(n)), dim3(256), 0, s, a, b, out, n);
  SVT_LAUNCH_CHECK();
  return 0;
}

namespace {
// ---- WavLM gated relative position bias (HF modeling_wavlm.py WavLMAttention) ----
// pb[h][d + T - 1] = embed[bucket(d)][h], d = key - query in (-T, T): half of the buckets per sign, exact below max_exact,
// log-spaced above, with torch's fp32 arithmetic (log(|d| / max_exact) / log(max_distance / max_exact) * (nb - max_exact),
// truncated)
__global__ void relpos_table_kernel(const float* embed, int H, int T, int num_buckets, int max_distance, float* pb) {
  const int n = 2 * T - 1;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * H) return;
  const int h = i / n, di = i - h * n;
  const int d = di - (T - 1);
  const int nb = num_buckets / 2, max_exact = nb / 2;
  int bucket = d > 0 ? nb : 0;
  const int a = d < 0 ? -d : d;
  if (a < max_exact) bucket += a;
  else {
    float v = logf((float)a / (float)max_exact);
    v = v / (float)log((double)max_distance / (double)max_exact);
    v = v * (float)(nb - max_exact);
    long lb = (long)((float)max_exact + v);
    if (lb > nb - 1) lb = nb - 1;
    bucket += (int)lb;
  }
  pb[i] = embed[bucket * H + h];
}
}  // namespace
int launch_relpos_table(const float* embed, int H, int T, int num_buckets, int max_distance, float* pb, hipStream_t s) {
  const int n = (2 * T - 1) * H;
  hipLaunchKernelGGL(relpos_table_kernel, dim3((n + 255) / 256), dim3(256), 0, s, embed, H, T, num_buckets, max_distance, pb);
  g_glue_kernel_id = 30;
  SVT_LAUNCH_CHECK();
  return 0;
}
namespace {
// gate[b][h][t] = ga * (gb * const[h] - 1) + 2,  ga / gb = sigmoid(u_h . wa + ba), sigmoid(u_h . wb + bb); u = the attention
// input (operand type), wa / wb = the sums of rows 0-3 / 4-7 of gru_rel_pos_linear (folded at finalize)
template <typename T>
__global__ void relpos_gate_kernel(const T* u, int64_t rows, int Tt, int H, int dh, const float* wab, const float* bab,
                                   const float* cst, float* gate) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * H) return;
  const int h = (int)(i % H);
  const int64_t row = i / H;
  const T* x = u + row * (int64_t)H * dh + (int64_t)h * dh;
  float sa = bab[0], sb = bab[1];
  for (int d = 0; d < dh; ++d) {
    const float xv = (float)x[d];
    sa = fmaf(xv, wab[d], sa);
    sb = fmaf(xv, wab[dh + d], sb);
  }
  const float ga = 1.f / (1.f + expf(-sa)), gb = 1.f / (1.f + expf(-sb));
  const int64_t b = row / Tt, t = row % Tt;
  gate[(b * H + h) * Tt + t] = ga * (gb * cst[h] - 1.f) + 2.f;
}
// Coalesced form: dh / 8 consecutive lanes own one (row, head) -- each loads 8 consecutive features (a wave reads 512
// consecutive elements of u) and the two dot products are folded across the group with lane exchanges.  (The one-thread-per-
// head form above reads 64 different lines per load instruction: 55 us per layer at 32 x 499 frames x 12 heads instead of 8.)
template <typename T>
__global__ __launch_bounds__(256) void relpos_gate_vec_kernel(const T* u, int64_t n, int Tt, int H, int dh, const float* wab,
                                                              const float* bab, const float* cst, float* gate) {
  const int lph = dh >> 3;  // lanes per head: a power of two <= 64 (checked by the launcher)
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t grp = tid / lph;
  const int sub = (int)(tid % lph);
  const bool ok = grp < n;
  float sa = 0.f, sb = 0.f;
  if (ok) {
    const T* x = u + grp * dh + sub * 8;
    const float* wa = wab + sub * 8;
    const float* wb = wab + dh + sub * 8;
    float xv[8];
    if constexpr (sizeof(T) == 2) {
      const bf16x8 v = *(const bf16x8*)x;  // one 16-byte load per lane
#pragma unroll
      for (int j = 0; j < 8; ++j) xv[j] = (float)v[j];
    } else {
      const float4 v0 = *(const float4*)x, v1 = *(const float4*)(x + 4);
      xv[0] = v0.x; xv[1] = v0.y; xv[2] = v0.z; xv[3] = v0.w; xv[4] = v1.x; xv[5] = v1.y; xv[6] = v1.z; xv[7] = v1.w;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      sa = fmaf(xv[j], wa[j], sa);
      sb = fmaf(xv[j], wb[j], sb);
    }
  }
  for (int o = lph >> 1; o > 0; o >>= 1) {
    sa += __shfl_xor(sa, o, 64);
    sb += __shfl_xor(sb, o, 64);
  }
  if (ok && sub == 0) {
    sa += bab[0];
    sb += bab[1];
    const float ga = 1.f / (1.f + expf(-sa)), gb = 1.f / (1.f + expf(-sb));
    const int h = (int)(grp % H);
    const int64_t row = grp / H;
    const int64_t b = row / Tt, t = row % Tt;
    gate[(b * H + h) * Tt + t] = ga * (gb * cst[h] - 1.f) + 2.f;
  }
}
}  // namespace
int launch_relpos_gate(int prec, const void* u, int64_t rows, int T, int H, int dh, const float* wab, const float* bab,
                       const float* cst, float* gate, hipStream_t s) {
  const int64_t n = rows * H;
  const int lph = dh / 8;
  if (dh % 8 == 0 && lph >= 1 && lph <= 64 && (lph & (lph - 1)) == 0 && !((uintptr_t)u & 15)) {
    const int64_t threads = n * lph;
    const dim3 grid((unsigned)((threads + 255) / 256));
    if (prec) hipLaunchKernelGGL(relpos_gate_vec_kernel<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)u, n, T, H, dh, wab, bab, cst, gate);
    else hipLaunchKernelGGL(relpos_gate_vec_kernel<float>, grid, dim3(256), 0, s, (const float*)u, n, T, H, dh, wab, bab, cst, gate);
    g_glue_kernel_id = prec ? 42 : 41;
    SVT_LAUNCH_CHECK();
    return 0;
  }
  if (prec) hipLaunchKernelGGL(relpos_gate_kernel<bf16_t>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const bf16_t*)u, rows, T, H, dh, wab, bab, cst, gate);
  else hipLaunchKernelGGL(relpos_gate_kernel<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float*)u, rows, T, H, dh, wab, bab, cst, gate);
  g_glue_kernel_id = prec ? 44 : 43;
  SVT_LAUNCH_CHECK();
  return 0;
}
namespace {
// materialised-score path: S[b,h,q,k] += gate[b,h,q] * pb[h][k - q + T - 1]
__global__ void scores_add_relbias_kernel(float* S, int64_t BH, int H, int T, int Tp, const float* gate, const float* pb) {
  const int64_t n = BH * T * (int64_t)T;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int k = (int)(i % T);
    int64_t r = i / T;
    const int q = (int)(r % T);
    const int64_t bh = r / T;
    const int h = (int)(bh % H);
    S[(bh * T + q) * Tp + k] += gate[bh * T + q] * pb[(int64_t)h * (2 * T - 1) + (k - q + T - 1)];
  }
}
}  // namespace
int launch_scores_add_relbias(float* S, int64_t BH, int H, int T, int Tp, const float* gate, const float* pb, hipStream_t s) {
  hipLaunchKernelGGL(scores_add_relbias_kernel, dim3(grid_for(BH * T * (int64_t)T)), dim3(256), 0, s, S, BH, H, T, Tp, gate, pb);
  SVT_LAUNCH_CHECK();
  return 0;
}

// ---- clock stamps (svt_debug_clock): one (shader clock, 100 MHz wall clock) pair per XCD ----
__global__ void clock_stamp_kernel(long long* out) {
  if (threadIdx.x == 0) {
    unsigned xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    xcc &= 7u;
    const long long t = __builtin_amdgcn_s_memtime();
    const long long r = __builtin_amdgcn_s_memrealtime();
    out[2 * xcc] = t;
    out[2 * xcc + 1] = r;
  }
}
int launch_clock_stamp(long long* out16, hipStream_t s) {
  hipLaunchKernelGGL(clock_stamp_kernel, dim3(64), dim3(64), 0, s, out16);  // 64 blocks: round-robin over the 8 XCDs
  SVT_LAUNCH_CHECK();
  return 0;
}

}  // namespace svt
