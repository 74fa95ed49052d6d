// clip_grad_norm_ + torch.optim.Adam / AdamW over a parameter list of any length (the recipes' wav2vec_opt_class / encoder_opt_class:
// N20EMv2/audio_only/hparams/train_audio_ssl.yaml:155, N20EMv2/video_only/hparams/train_video_ssl.yaml:134).  DESIGN §4.50.
//
// The work is split by chunks of kAdaChunk elements, not by tensors: one workgroup per chunk of whichever tensor the chunk falls in, so a
// 4096 x 1024 weight and a 1024-element bias in one list load the chip evenly.  The tensor table (five pointers, numel, first chunk,
// the per-tensor step size and sqrt(bias correction 2)) lives in the caller's workspace: launch_clip_adam writes it there with
// adam_table_kernel, kAdamSlice entries per launch out of its kernel arguments (3 KiB of the 4 KiB limit), so one call takes any number
// of tensors without a copy on the stream or a host-device synchronisation, and every later kernel finds a chunk's tensor by a
// binary search over the table's chunk prefix (a wave-uniform walk of <= log2(n) entries).
//
// Accesses are 16 bytes per lane wherever a tensor allows it.  Torch parameters that are views into one flat buffer start at 4-byte-
// but not 16-byte-aligned addresses: when the arrays of a tensor share one offset from a 16-byte boundary, each chunk peels up to three
// scalar head elements and up to three tail elements around its float4 body; when they do not (or amsgrad's fifth array disagrees), that
// tensor alone takes 4-byte accesses.  The sum of squares reads only the gradient, so it vectorises on the gradient's own offset.
//
// Every reduction has a fixed order (no float atomics, no inter-workgroup flags): two calls on equal inputs at equal addresses give equal
// bits.
#include "common.h"

namespace svt {
namespace {

struct alignas(16) AdamEntry {
  float* p;
  float* g;
  float* m;
  float* v;
  float* vmax;        // null without amsgrad
  int64_t n;
  int32_t chunk0;     // first chunk of this tensor: prefix sum of ceil(n / kAdaChunk)
  float step_size;    // lr / (1 - beta1^step), computed in double on the host
  float bc2_sqrt;     // sqrt(1 - beta2^step), likewise
  int8_t head;        // scalar elements in front of the first 16-byte-aligned element of all arrays (0..3); -1: 4-byte accesses only
  int8_t ghead;       // the same for the gradient alone (the sum of squares)
  int8_t pad[2];
};
static_assert(sizeof(AdamEntry) == 64, "AdamEntry is one 64-byte line");

constexpr int kAdamSlice = 48;   // table entries per adam_table_kernel launch (48 * 64 B + 8 B of kernel arguments)
struct AdamSlice {
  AdamEntry e[kAdamSlice];
  int first, count;
};

__global__ __launch_bounds__(64) void adam_table_kernel(AdamSlice sl, AdamEntry* __restrict__ table) {
  const int t = threadIdx.x;
  if (t < sl.count) table[sl.first + t] = sl.e[t];
}

// the tensor whose chunks contain `chunk`: the last entry with chunk0 <= chunk (a 0-element tensor shares its chunk0 with its successor
// and is never the last such entry unless nothing follows it, and then no chunk reaches it)
__device__ __forceinline__ int adam_tensor_of(const AdamEntry* __restrict__ table, int count, int chunk) {
  int lo = 0, hi = count;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (table[mid].chunk0 <= chunk) lo = mid; else hi = mid;
  }
  return lo;
}

// the shape of one chunk: `hd` scalar head elements, `nvec` float4 groups, `ntail` scalar tail elements from `tail0` (chunk-local)
struct ChunkShape {
  int cnt, hd, nvec, tail0, ntail;
};
__device__ __forceinline__ ChunkShape chunk_shape(int64_t n, int64_t lo, int head) {
  ChunkShape c;
  c.cnt = (int)(n - lo < kAdaChunk ? n - lo : kAdaChunk);
  if (head < 0) { c.hd = 0; c.nvec = 0; c.tail0 = 0; c.ntail = c.cnt; return c; }   // 4-byte accesses: the whole chunk is "tail"
  c.hd = head < c.cnt ? head : c.cnt;   // kAdaChunk is a multiple of 4: every chunk of a tensor has the tensor's offset
  c.nvec = (c.cnt - c.hd) >> 2;
  c.tail0 = c.hd + 4 * c.nvec;
  c.ntail = c.cnt - c.tail0;
  return c;
}

__device__ __forceinline__ double block_sum_d256(double v, double* sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// one workgroup per chunk: sum of g^2 in double.  Thread t adds, in this order, head element t, the float4 groups t, t + 256, ... (x, y,
// z, w each), tail element t; then the 64-lane butterfly and (w0 + w1) + (w2 + w3)
__global__ __launch_bounds__(256) void adam_sumsq_kernel(const AdamEntry* __restrict__ table, int count, double* __restrict__ part) {
  __shared__ double sh[4];
  const int chunk = blockIdx.x;
  const AdamEntry& e = table[adam_tensor_of(table, count, chunk)];
  const int64_t lo = (int64_t)(chunk - e.chunk0) * kAdaChunk;
  const ChunkShape c = chunk_shape(e.n, lo, e.ghead);
  const float* __restrict__ g = e.g + lo;
  const int t = threadIdx.x;
  double s = 0.0;
  if (t < c.hd) { const double x = (double)g[t]; s += x * x; }
  const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g + c.hd);
  for (int j = t; j < c.nvec; j += 256) {
    const float4 q = g4[j];
    s += (double)q.x * (double)q.x;
    s += (double)q.y * (double)q.y;
    s += (double)q.z * (double)q.z;
    s += (double)q.w * (double)q.w;
  }
  for (int j = t; j < c.ntail; j += 256) { const double x = (double)g[c.tail0 + j]; s += x * x; }
  s = block_sum_d256(s, sh);
  if (t == 0) part[chunk] = s;
}

// one wave per tensor: norm_i = (float)sqrt(sum of its chunks' partials), lane l adding chunks l, l + 64, ... in order, then the butterfly
__global__ __launch_bounds__(256) void adam_norm_kernel(const AdamEntry* __restrict__ table, int count, int total_chunks,
                                                        const double* __restrict__ part, float* __restrict__ norms) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= count) return;
  const int c0 = table[i].chunk0, c1 = i + 1 < count ? table[i + 1].chunk0 : total_chunks;
  double s = 0.0;
  for (int c = c0 + lane; c < c1; c += 64) s += part[c];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) norms[i] = (float)sqrt(s);
}

// clip_grad_norm_: total = ||[norm_i]|| (thread t adds norm_i^2 of tensors t, t + 256, ... in double, then the fixed tree), coef =
// min(max_norm / (total + 1e-6), 1)
__global__ __launch_bounds__(256) void adam_coef_kernel(const float* __restrict__ norms, int count, float max_norm, float* __restrict__ coef,
                                                        float* __restrict__ total_out) {
  __shared__ double sh[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < count; i += 256) { const double x = (double)norms[i]; s += x * x; }
  s = block_sum_d256(s, sh);
  if (threadIdx.x != 0) return;
  const float total = (float)sqrt(s);
  if (total_out) *total_out = total;
  if (coef) {
    const float c = __fdiv_rn(max_norm, __fadd_rn(total, 1e-6f));
    *coef = c < 1.f ? c : 1.f;
  }
}

// torch.optim.Adam's single-tensor update (torch/optim/adam.py _single_tensor_adam) for one element, every operation rounded once to fp32
// in this order:
//   g   = g * coef                        (the clip; this g is stored)
//   g'  = maximize ? -g : g
//   decoupled:  p = p * (1 - lr wd)       (the factor rounded from double)         coupled:  g' = fma(p, wd, g')
//   m   = fma(1 - beta1, g' - m, m)       (lerp_; for 1 - beta1 >= 0.5 torch's other branch: g' - (g' - m) * (1 - (1 - beta1)))
//   v   = v * beta2 + ((1 - beta2) * g') * g'
//   vmax = max(vmax, v)                   (amsgrad, NaN propagating)
//   denom = sqrt(v or vmax) / sqrt(bc2) + eps
//   p   = p + (-(lr / bc1) * m) / denom   (addcdiv_: value * tensor1 / tensor2)
template <bool kAms>
__device__ __forceinline__ void adam_element(float& p, float& g, float& m, float& v, float& vmax, const AdamHyper& h, bool clip, float cf,
                                             float neg_step, float bc2_sqrt) {
  if (clip) g = __fmul_rn(g, cf);
  float gu = h.maximize ? -g : g;
  if (h.weight_decay != 0.f) {
    if (h.decoupled) p = __fmul_rn(p, h.decay_mul);
    else gu = __fmaf_rn(p, h.weight_decay, gu);
  }
  const float d = __fsub_rn(gu, m);
  m = h.lerp_far ? __fsub_rn(gu, __fmul_rn(d, h.one_minus_w1)) : __fmaf_rn(h.w1, d, m);
  v = __fadd_rn(__fmul_rn(v, h.beta2), __fmul_rn(__fmul_rn(h.one_minus_beta2, gu), gu));
  float root = v;
  if (kAms) {
    vmax = (v > vmax || v != v) ? v : vmax;
    root = vmax;
  }
  const float denom = __fadd_rn(__fdiv_rn(__fsqrt_rn(root), bc2_sqrt), h.eps);
  p = __fadd_rn(p, __fdiv_rn(__fmul_rn(neg_step, m), denom));
}

template <bool kAms>
__device__ __forceinline__ void adam_scalar(const AdamEntry& e, int64_t at, const AdamHyper& h, bool clip, float cf, float neg_step) {
  float p = e.p[at], g = e.g[at], m = e.m[at], v = e.v[at], vmax = kAms ? e.vmax[at] : 0.f;
  adam_element<kAms>(p, g, m, v, vmax, h, clip, cf, neg_step, e.bc2_sqrt);
  e.p[at] = p;
  if (clip) e.g[at] = g;
  e.m[at] = m;
  e.v[at] = v;
  if (kAms) e.vmax[at] = vmax;
}

// one workgroup per chunk of kAdaChunk elements: up to 3 scalar head elements, float4 groups t, t + 256, ..., up to 3 scalar tail elements
template <bool kAms>
__global__ __launch_bounds__(256) void adam_update_kernel(const AdamEntry* __restrict__ table, int count, const float* __restrict__ coef,
                                                          AdamHyper h) {
  const int chunk = blockIdx.x;
  const AdamEntry e = table[adam_tensor_of(table, count, chunk)];
  const int64_t lo = (int64_t)(chunk - e.chunk0) * kAdaChunk;
  const ChunkShape c = chunk_shape(e.n, lo, e.head);
  const bool clip = coef != nullptr;
  const float cf = clip ? *coef : 1.f;
  const float neg_step = -e.step_size;
  const int t = threadIdx.x;
  if (t < c.hd) adam_scalar<kAms>(e, lo + t, h, clip, cf, neg_step);
  float4* __restrict__ p4 = reinterpret_cast<float4*>(e.p + lo + c.hd);
  float4* __restrict__ g4 = reinterpret_cast<float4*>(e.g + lo + c.hd);
  float4* __restrict__ m4 = reinterpret_cast<float4*>(e.m + lo + c.hd);
  float4* __restrict__ v4 = reinterpret_cast<float4*>(e.v + lo + c.hd);
  float4* __restrict__ x4 = kAms ? reinterpret_cast<float4*>(e.vmax + lo + c.hd) : nullptr;
#pragma unroll 2
  for (int j = t; j < c.nvec; j += 256) {
    float4 p = p4[j], g = g4[j], m = m4[j], v = v4[j], x = kAms ? x4[j] : make_float4(0.f, 0.f, 0.f, 0.f);
    adam_element<kAms>(p.x, g.x, m.x, v.x, x.x, h, clip, cf, neg_step, e.bc2_sqrt);
    adam_element<kAms>(p.y, g.y, m.y, v.y, x.y, h, clip, cf, neg_step, e.bc2_sqrt);
    adam_element<kAms>(p.z, g.z, m.z, v.z, x.z, h, clip, cf, neg_step, e.bc2_sqrt);
    adam_element<kAms>(p.w, g.w, m.w, v.w, x.w, h, clip, cf, neg_step, e.bc2_sqrt);
    p4[j] = p;
    if (clip) g4[j] = g;
    m4[j] = m;
    v4[j] = v;
    if (kAms) x4[j] = x;
  }
  for (int j = t; j < c.ntail; j += 256) adam_scalar<kAms>(e, lo + c.tail0 + j, h, clip, cf, neg_step);
}

inline size_t round16(size_t v) { return (v + 15) / 16 * 16; }

}  // namespace

int64_t adam_chunks(const int64_t* numels, int count) {
  int64_t c = 0;
  for (int i = 0; i < count; ++i) c += (numels[i] + kAdaChunk - 1) / kAdaChunk;
  return c;
}

// table | per-chunk partial sums (double) | per-tensor norms (float) | clip coefficient
size_t adam_workspace_bytes(const int64_t* numels, int count) {
  return (size_t)count * sizeof(AdamEntry) + (size_t)adam_chunks(numels, count) * sizeof(double) + round16((size_t)count * sizeof(float)) + 16;
}

int launch_clip_adam(int count, float* const* params, float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                     float* const* max_exp_avg_sq, const int64_t* numels, const float* step_size, const float* bc2_sqrt,
                     const AdamHyper& h, float max_norm, float* total_norm, void* ws, hipStream_t s) {
  const int64_t chunks = adam_chunks(numels, count);
  AdamEntry* table = (AdamEntry*)ws;
  double* part = (double*)(table + count);
  float* norms = (float*)(part + chunks);
  float* coef = (float*)((char*)norms + round16((size_t)count * sizeof(float)));
  const bool ams = max_exp_avg_sq != nullptr;
  AdamSlice sl{};
  int64_t c0 = 0;
  for (int first = 0; first < count; first += kAdamSlice) {
    sl.first = first;
    sl.count = count - first < kAdamSlice ? count - first : kAdamSlice;
    for (int k = 0; k < sl.count; ++k) {
      const int i = first + k;
      AdamEntry& e = sl.e[k];
      e.p = params[i]; e.g = grads[i]; e.m = exp_avg[i]; e.v = exp_avg_sq[i]; e.vmax = ams ? max_exp_avg_sq[i] : nullptr;
      e.n = numels[i];
      e.chunk0 = (int32_t)c0;
      e.step_size = step_size[i];
      e.bc2_sqrt = bc2_sqrt[i];
      const unsigned off = (unsigned)(((uintptr_t)e.p >> 2) & 3);
      const auto same = [off](const float* q) { return (unsigned)(((uintptr_t)q >> 2) & 3) == off; };
      e.head = (same(e.g) && same(e.m) && same(e.v) && (!ams || same(e.vmax))) ? (int8_t)((4 - off) & 3) : (int8_t)-1;
      e.ghead = (int8_t)((4 - (unsigned)(((uintptr_t)e.g >> 2) & 3)) & 3);
      c0 += (numels[i] + kAdaChunk - 1) / kAdaChunk;
    }
    hipLaunchKernelGGL(adam_table_kernel, dim3(1), dim3(64), 0, s, sl, table);
    SVT_LAUNCH_CHECK();
  }
  const bool clip = max_norm > 0.f;
  if (clip || total_norm) {
    if (chunks > 0) {
      hipLaunchKernelGGL(adam_sumsq_kernel, dim3((unsigned)chunks), dim3(256), 0, s, table, count, part);
      SVT_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(adam_norm_kernel, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, s, table, count, (int)chunks, part, norms);
    SVT_LAUNCH_CHECK();
    hipLaunchKernelGGL(adam_coef_kernel, dim3(1), dim3(256), 0, s, norms, count, max_norm, clip ? coef : nullptr, total_norm);
    SVT_LAUNCH_CHECK();
  }
  if (chunks > 0) {
    if (ams) hipLaunchKernelGGL(adam_update_kernel<true>, dim3((unsigned)chunks), dim3(256), 0, s, table, count, clip ? coef : nullptr, h);
    else hipLaunchKernelGGL(adam_update_kernel<false>, dim3((unsigned)chunks), dim3(256), 0, s, table, count, clip ? coef : nullptr, h);
    SVT_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace svt
