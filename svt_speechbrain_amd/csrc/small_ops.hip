// The kernels behind api_ops.hip: the narrow fp32 linear layers, the recipes' validation losses, Fbank with its deltas and context
// window, the per-frame decode and the greedy CTC decode.
#include "device_util.h"

namespace svt {
namespace {
// Frame head: y[row, n] = x[row,:] . w[n,:] + b[n], N <= 32, fp32 throughout.  One wave per row; the
// row of x is read once, the N partial sums live in registers, shuffle-reduced at the end.
__global__ __launch_bounds__(256) void linear_small_kernel(const float* x, int64_t rows, int K, const float* w,
                                                           const float* b, int N, float* y) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + row * K;
  float acc[32];
#pragma unroll
  for (int n = 0; n < 32; ++n) acc[n] = 0.f;
  for (int k = lane; k < K; k += 64) {
    const float xv = xr[k];
#pragma unroll
    for (int n = 0; n < 32; ++n)
      if (n < N) acc[n] = fmaf(xv, w[(long)n * K + k], acc[n]);
  }
#pragma unroll
  for (int n = 0; n < 32; ++n) {
    if (n < N) {
      const float r = wave_sum(acc[n]);
      if (lane == 0) y[row * N + n] = r + (b ? b[n] : 0.f);
    }
  }
}
}  // namespace
int launch_linear_f32(const float* x, int64_t rows, int K, const float* w, const float* b, int N, float* y,
                      hipStream_t s) {
  if (N > 32) { set_error("linear_small: N > 32"); return -1; }
  hipLaunchKernelGGL(linear_small_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, x, rows, K, w, b, N, y);
  SVT_LAUNCH_CHECK();
  return 0;
}

namespace {
// Frame head for the encoder widths (K = 256 * KC): the N x K weight is staged once per workgroup in LDS, a wave
// handles four rows at a time (x read once from HBM with 16-byte accesses, every weight fragment reused by the four
// rows), and the 4 x N partial sums are folded across the wave with a halving exchange (7 shuffles per output column
// instead of 24).  HBM-bound: rows * K * 4 bytes in, rows * N * 4 bytes out.
template <int KC>
__global__ __launch_bounds__(256) void linear_head_kernel(const float* __restrict__ x, int64_t rows,
                                                          const float* __restrict__ w, const float* __restrict__ b, int N,
                                                          float* __restrict__ y) {
  constexpr int K = KC * 256;
  extern __shared__ __attribute__((aligned(16))) float wl[];
  for (int i = threadIdx.x * 4; i < N * K; i += 1024) *(float4*)(wl + i) = *(const float4*)(w + i);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool hi32 = (lane & 32) != 0, hi16 = (lane & 16) != 0;
  const int myrow = (hi32 ? 2 : 0) + (hi16 ? 1 : 0);
  for (int64_t r0 = ((int64_t)blockIdx.x * 4 + wave) * 4; r0 < rows; r0 += (int64_t)gridDim.x * 16) {
    float4 xv[4][KC];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int64_t row = r0 + rr < rows ? r0 + rr : rows - 1;
#pragma unroll
      for (int c = 0; c < KC; ++c) xv[rr][c] = *(const float4*)(x + row * K + c * 256 + lane * 4);
    }
    float out0 = 0.f, out1 = 0.f;
    for (int n = 0; n < N; ++n) {
      float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < KC; ++c) {
        const float4 wv = *(const float4*)(wl + n * K + c * 256 + lane * 4);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          s[rr] = fmaf(xv[rr][c].x, wv.x, s[rr]);
          s[rr] = fmaf(xv[rr][c].y, wv.y, s[rr]);
          s[rr] = fmaf(xv[rr][c].z, wv.z, s[rr]);
          s[rr] = fmaf(xv[rr][c].w, wv.w, s[rr]);
        }
      }
      // lanes 0-31 end up with rows {0,1}, lanes 32-63 with rows {2,3}; then bit 4 of the lane picks the row
      float k0 = hi32 ? s[2] : s[0], k1 = hi32 ? s[3] : s[1];
      const float g0 = hi32 ? s[0] : s[2], g1 = hi32 ? s[1] : s[3];
      k0 += __shfl_xor(g0, 32, 64);
      k1 += __shfl_xor(g1, 32, 64);
      float v = hi16 ? k1 : k0;
      v += __shfl_xor(hi16 ? k0 : k1, 16, 64);
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if ((lane & 15) == (n & 15)) { if (n < 16) out0 = v; else out1 = v; }
    }
    const int64_t row = r0 + myrow;
    if (row < rows) {
      const int n0 = lane & 15;
      if (n0 < N) y[row * N + n0] = out0 + (b ? b[n0] : 0.f);
      if (n0 + 16 < N) y[row * N + n0 + 16] = out1 + (b ? b[n0 + 16] : 0.f);
    }
  }
}
}  // namespace
template <int KC>
static int launch_linear_head_kc(const float* x, int64_t rows, const float* w, const float* b, int N, float* y, hipStream_t s) {
  const size_t lds = (size_t)N * KC * 256 * 4;
  if (lds > 65536)
    if (int r_ = ensure_dyn_lds((const void*)linear_head_kernel<KC>, (int)lds)) return r_;
  const int64_t groups = (rows + 15) / 16;
  const unsigned grid = (unsigned)(groups < 512 ? groups : 512);
  hipLaunchKernelGGL((linear_head_kernel<KC>), dim3(grid), dim3(256), lds, s, x, rows, w, b, N, y);
  SVT_LAUNCH_CHECK();
  return 0;
}

bool linear_head_eligible(int K, int N) { return N >= 1 && N <= 32 && (K == 512 || K == 768 || K == 1024); }
int launch_linear_head(const float* x, int64_t rows, int K, const float* w, const float* b, int N, float* y, hipStream_t s) {
  if (K == 512) return launch_linear_head_kc<2>(x, rows, w, b, N, y, s);
  if (K == 768) return launch_linear_head_kc<3>(x, rows, w, b, N, y, s);
  if (K == 1024) return launch_linear_head_kc<4>(x, rows, w, b, N, y, s);
  set_error("linear_head: unsupported K");
  return -1;
}

namespace {
// Validation losses of the recipes (speechbrain/nnet/losses.py:402-519 nll_loss / bce_loss over
// compute_masked_loss :624-684).  One workgroup per batch item: per-frame loss x length mask, block-reduced in a
// fixed order (deterministic) into double sums {sum loss*mask, sum mask, sum mean_c(logp)*mask}; a second tiny
// kernel applies the reduction mode.  mask[b,t] = (float)t < rel_len[b] * (float)T, the fp32 comparison
// length_to_mask makes (speechbrain/dataio/dataio.py:661-706).
__device__ __forceinline__ double block_sum_256(double v, double* sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}

__global__ __launch_bounds__(256) void bce_loss_kernel(const float* x, int64_t t_pred, const float* y, int64_t t_tgt, int64_t T,
                                                       const float* rel_len, const float* pos_weight, float* per_frame,
                                                       double* sums) {
  __shared__ double sh[4];
  const int b = blockIdx.x;
  const float lim = rel_len ? __fmul_rn(rel_len[b], (float)T) : 0.f;
  const float pw = pos_weight ? pos_weight[0] : 1.f;
  double sl = 0.0, sm = 0.0;
  for (int64_t t = threadIdx.x; t < T; t += 256) {
    const float xv = x[b * t_pred + t], yv = y[b * t_tgt + t];
    const float m = rel_len ? ((float)t < lim ? 1.f : 0.f) : 1.f;
    // torch binary_cross_entropy_with_logits: (1 - y) x + (1 + (pw - 1) y) (log1p(exp(-|x|)) + max(-x, 0))
    const float sp = log1pf(expf(-fabsf(xv))) + fmaxf(-xv, 0.f);
    const float lw = pos_weight ? 1.f + (pw - 1.f) * yv : 1.f;
    const float l = ((1.f - yv) * xv + lw * sp) * m;
    if (per_frame) per_frame[b * T + t] = l;
    sl += (double)l;
    sm += (double)m;
  }
  sl = block_sum_256(sl, sh);
  sm = block_sum_256(sm, sh);
  if (threadIdx.x == 0) { sums[b * 3 + 0] = sl; sums[b * 3 + 1] = sm; sums[b * 3 + 2] = 0.0; }
}

__global__ __launch_bounds__(256) void nll_loss_kernel(const float* logp, int64_t t_pred, int C, const int64_t* tgt, int64_t t_tgt,
                                                       int64_t T, const float* rel_len, float* per_frame, double* sums,
                                                       int* bad_target) {
  __shared__ double sh[4];
  const int b = blockIdx.x;
  const float lim = rel_len ? __fmul_rn(rel_len[b], (float)T) : 0.f;
  double sl = 0.0, sm = 0.0, sr = 0.0;
  for (int64_t t = threadIdx.x; t < T; t += 256) {
    const float* row = logp + (b * t_pred + t) * C;
    const int64_t k = tgt[b * t_tgt + t];
    const float m = rel_len ? ((float)t < lim ? 1.f : 0.f) : 1.f;
    float l = 0.f;
    if (k == -100) l = 0.f;  // torch.nn.functional.nll_loss ignore_index default
    else if (k < 0 || k >= C) { atomicExch(bad_target, 1); }
    else l = -row[k];
    l *= m;
    float mean = 0.f;
    for (int c = 0; c < C; ++c) mean += row[c];
    mean = mean / (float)C * m;
    if (per_frame) per_frame[b * T + t] = l;
    sl += (double)l;
    sm += (double)m;
    sr += (double)mean;
  }
  sl = block_sum_256(sl, sh);
  sm = block_sum_256(sm, sh);
  sr = block_sum_256(sr, sh);
  if (threadIdx.x == 0) { sums[b * 3 + 0] = sl; sums[b * 3 + 1] = sm; sums[b * 3 + 2] = sr; }
}

// reduction: 0 mean, 1 batchmean, 2 batch (B outputs); label smoothing as compute_masked_loss :670-684
__global__ void loss_reduce_kernel(const double* sums, int B, int reduction, float smoothing, float* out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  if (reduction == 2) {
    for (int b = 0; b < B; ++b) {
      const float l = (float)sums[b * 3] / (float)sums[b * 3 + 1];
      const float r = (float)sums[b * 3 + 2] / (float)sums[b * 3 + 1];
      out[b] = smoothing == 0.f ? l : -smoothing * r + (1.f - smoothing) * l;
    }
    return;
  }
  double sl = 0.0, sm = 0.0, sr = 0.0;
  for (int b = 0; b < B; ++b) { sl += sums[b * 3]; sm += sums[b * 3 + 1]; sr += sums[b * 3 + 2]; }
  const float den = reduction == 0 ? (float)sm : (float)B;
  const float l = (float)sl / den, r = (float)sr / den;
  out[0] = smoothing == 0.f ? l : -smoothing * r + (1.f - smoothing) * l;
}

// y = log_softmax(x) / softmax(x) over the last axis (speechbrain/nnet/activations.py Softmax): one thread per row for
// the narrow heads of this path (n <= 64), fp32
__global__ void softmax_small_kernel(const float* x, int64_t rows, int n, int apply_log, float* y) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const float* xr = x + r * n;
  float mx = xr[0];
  for (int i = 1; i < n; ++i) mx = fmaxf(mx, xr[i]);
  float s = 0.f;
  for (int i = 0; i < n; ++i) s += expf(xr[i] - mx);
  const float ls = logf(s);
  for (int i = 0; i < n; ++i) y[r * n + i] = apply_log ? (xr[i] - mx) - ls : expf(xr[i] - mx) / s;
}
}  // namespace
int launch_bce_loss(const float* x, int64_t B, int64_t t_pred, const float* y, int64_t t_tgt, int64_t T, const float* rel_len,
                    const float* pos_weight, float* per_frame, double* sums, hipStream_t s) {
  hipLaunchKernelGGL(bce_loss_kernel, dim3((unsigned)B), dim3(256), 0, s, x, t_pred, y, t_tgt, T, rel_len, pos_weight, per_frame, sums);
  SVT_LAUNCH_CHECK();
  return 0;
}
int launch_nll_loss(const float* logp, int64_t B, int64_t t_pred, int C, const int64_t* tgt, int64_t t_tgt, int64_t T,
                    const float* rel_len, float* per_frame, double* sums, int* bad_target, hipStream_t s) {
  hipLaunchKernelGGL(nll_loss_kernel, dim3((unsigned)B), dim3(256), 0, s, logp, t_pred, C, tgt, t_tgt, T, rel_len, per_frame, sums,
                     bad_target);
  SVT_LAUNCH_CHECK();
  return 0;
}
int launch_loss_reduce(const double* sums, int B, int reduction, float smoothing, float* out, hipStream_t s) {
  hipLaunchKernelGGL(loss_reduce_kernel, dim3(1), dim3(64), 0, s, sums, B, reduction, smoothing, out);
  SVT_LAUNCH_CHECK();
  return 0;
}
int launch_softmax_small(const float* x, int64_t rows, int n, int apply_log, float* y, hipStream_t s) {
  hipLaunchKernelGGL(softmax_small_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, x, rows, n, apply_log, y);
  SVT_LAUNCH_CHECK();
  return 0;
}

namespace {
// Fbank add-ons (speechbrain/processing/features.py: Deltas :788-850, ContextWindow :853-940).
// delta[b,t,c] = sum_{k=-n..n} k * x[b, clamp(t+k), c] / denom   (replicate padding), x and out (B,T,ld) with column offsets
__global__ void deltas_kernel(const float* x, long ldx, int B, int T, int C, int n, float inv_denom, float* out, long ldo) {
  const long total = (long)B * T * C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const long r = i / C;
    const int t = (int)(r % T);
    const long b = r / T;
    float acc = 0.f;
    for (int k = -n; k <= n; ++k) {
      int tt = t + k;
      tt = tt < 0 ? 0 : (tt > T - 1 ? T - 1 : tt);
      acc = fmaf((float)k, x[(b * T + tt) * ldx + c], acc);
    }
    out[(b * T + t) * ldo + c] = acc * inv_denom;
  }
}
// out[b,t,c*ctx + j] = x[b, t + j - left', c] with zero padding, where the kernel is eye(ctx, klen) rolled by
// max(right - left, 0): tap j reads offset j + lag - pad, pad = max(left, right)
__global__ void context_window_kernel(const float* x, int B, int T, int C, int ctx, int lag, int pad, float* out) {
  const long total = (long)B * T * C * ctx;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int j = (int)(i % ctx);
    long r = i / ctx;
    const int c = (int)(r % C);
    r /= C;
    const int t = (int)(r % T);
    const long b = r / T;
    const int tt = t + j + lag - pad;
    out[i] = (tt >= 0 && tt < T) ? x[(b * T + tt) * C + c] : 0.f;
  }
}
}  // namespace
int launch_deltas(const float* x, long ldx, int B, int T, int C, int n, float inv_denom, float* out, long ldo, hipStream_t s) {
  hipLaunchKernelGGL(deltas_kernel, dim3(grid_for((int64_t)B * T * C)), dim3(256), 0, s, x, ldx, B, T, C, n, inv_denom, out, ldo);
  SVT_LAUNCH_CHECK();
  return 0;
}
int launch_context_window(const float* x, int B, int T, int C, int ctx, int lag, int pad, float* out, hipStream_t s) {
  hipLaunchKernelGGL(context_window_kernel, dim3(grid_for((int64_t)B * T * C * ctx)), dim3(256), 0, s, x, B, T, C, ctx, lag, pad, out);
  SVT_LAUNCH_CHECK();
  return 0;
}

namespace {
__global__ void decode_frames_kernel(const float* logits, int64_t rows, int n_out, int n_oct, int n_cls,
                                     FrameOut* out) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const float* l = logits + r * n_out;
  FrameOut f;
  f.p_on = 1.f / (1.f + expf(-l[0]));
  f.p_off = 1.f / (1.f + expf(-l[1]));
  int bo = 0;
  float bv = l[2];
  for (int i = 1; i <= n_oct; ++i)
    if (l[2 + i] > bv) { bv = l[2 + i]; bo = i; }
  int bc = 0;
  const float* c = l + 2 + n_oct + 1;
  bv = c[0];
  for (int i = 1; i <= n_cls; ++i)
    if (c[i] > bv) { bv = c[i]; bc = i; }
  f.octave = bo;
  f.pitch_class = bc;
  out[r] = f;
}
}  // namespace
int launch_decode_frames(const float* logits, int64_t rows, int n_out, int n_oct, int n_cls, FrameOut* out,
                         hipStream_t s) {
  hipLaunchKernelGGL(decode_frames_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, logits, rows, n_out,
                     n_oct, n_cls, out);
  SVT_LAUNCH_CHECK();
  return 0;
}

namespace {
// CTC greedy: one block per sequence.  argmax per frame, then order-preserving compaction of
// "first of a run, not blank, inside the relative length".
__global__ __launch_bounds__(256) void ctc_greedy_kernel(const float* probs, int T, int V, const float* rel_lens,
                                                         int blank, int32_t* tokens, int32_t* out_lens) {
  extern __shared__ int32_t ids[];  // T
  __shared__ int wave_tot[4];
  __shared__ int running;
  const int b = blockIdx.x;
  const float* p = probs + (int64_t)b * T * V;
  int n = (int)rintf(rel_lens[b] * (float)T);
  if (n > T) n = T;
  if (n < 0) n = 0;
  for (int t = threadIdx.x; t < n; t += blockDim.x) {
    const float* q = p + (int64_t)t * V;
    int best = 0;
    float bv = q[0];
    for (int v = 1; v < V; ++v)
      if (q[v] > bv) { bv = q[v]; best = v; }
    ids[t] = best;
  }
  if (threadIdx.x == 0) running = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int base = 0; base < n; base += blockDim.x) {
    const int t = base + threadIdx.x;
    bool keep = false;
    int id = 0;
    if (t < n) {
      id = ids[t];
      keep = (t == 0 || id != ids[t - 1]) && id != blank;
    }
    const unsigned long long m = __ballot(keep);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wave_tot[wave] = __popcll(m);
    __syncthreads();
    int off = running;
    for (int w = 0; w < wave; ++w) off += wave_tot[w];
    if (keep) tokens[(int64_t)b * T + off + before] = id;
    __syncthreads();
    if (threadIdx.x == 0) running += wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
    __syncthreads();
  }
  if (threadIdx.x == 0) out_lens[b] = running;
}
}  // namespace
int launch_ctc_greedy(const float* probs, int B, int T, int V, const float* rel_lens, int blank, int32_t* tokens,
                      int32_t* out_lens, hipStream_t s) {
  const size_t lds = (size_t)T * sizeof(int32_t);
  if (lds > 60000) { set_error("ctc_greedy: T too large for one block"); return -1; }
  hipLaunchKernelGGL(ctc_greedy_kernel, dim3(B), dim3(256), lds, s, probs, T, V, rel_lens, blank, tokens, out_lens);
  SVT_LAUNCH_CHECK();
  return 0;
}

namespace {
// Fbank pieces: framing (centred, zero padded) * window; power spectrum; dB + per-sequence top_db clip
__global__ void fbank_frames_kernel(const float* wav, int64_t L, int n_fft, int hop, int64_t nframes,
                                    const float* window, float* frames, int64_t total) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    const int k = (int)(i % n_fft);
    const int64_t r = i / n_fft;
    const int64_t f = r % nframes;
    const int64_t b = r / nframes;
    const int64_t pos = f * hop + k - n_fft / 2;
    const float v = (pos >= 0 && pos < L) ? wav[b * L + pos] : 0.f;
    frames[i] = v * window[k];
  }
}

__global__ void power_spectrum_kernel(const float* reim, int64_t rows, int nb, int imoff, int ld, float* power, int ldp) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t total = rows * ldp;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    const int k = (int)(i % ldp);
    const int64_t r = i / ldp;
    float v = 0.f;
    if (k < nb) {
      const float re = reim[r * ld + k], im = reim[r * ld + imoff + k];
      v = re * re + im * im;
    }
    power[i] = v;
  }
}

__global__ __launch_bounds__(256) void fbank_db_kernel(float* fb, int64_t per_seq, float top_db) {
  __shared__ float sh[4];
  float* x = fb + (int64_t)blockIdx.x * per_seq;
  float mx = -INFINITY;
  for (int64_t i = threadIdx.x; i < per_seq; i += blockDim.x) {
    const float v = 10.f * log10f(fmaxf(x[i], 1e-10f));
    x[i] = v;
    mx = fmaxf(mx, v);
  }
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = mx;
  __syncthreads();
  const float floor_db = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3])) - top_db;
  for (int64_t i = threadIdx.x; i < per_seq; i += blockDim.x) x[i] = fmaxf(x[i], floor_db);
}
}  // namespace
int launch_fbank_frames(const float* wav, int B, int64_t L, int n_fft, int hop, int64_t nframes, const float* window,
                        float* frames, hipStream_t s) {
  const int64_t total = (int64_t)B * nframes * n_fft;
  hipLaunchKernelGGL(fbank_frames_kernel, dim3(grid_for(total)), dim3(256), 0, s, wav, L, n_fft, hop, nframes, window,
                     frames, total);
  SVT_LAUNCH_CHECK();
  return 0;
}
int launch_power_spectrum(const float* reim, int64_t rows, int nb, int imoff, int ld, float* power, int ldp,
                          hipStream_t s) {
  hipLaunchKernelGGL(power_spectrum_kernel, dim3(grid_for(rows * ldp)), dim3(256), 0, s, reim, rows, nb, imoff, ld,
                     power, ldp);
  SVT_LAUNCH_CHECK();
  return 0;
}
int launch_fbank_db(float* fb, int B, int64_t per_seq, float top_db, hipStream_t s) {
  hipLaunchKernelGGL(fbank_db_kernel, dim3(B), dim3(256), 0, s, fb, per_seq, top_db);
  SVT_LAUNCH_CHECK();
  return 0;
}

}  // namespace svt
