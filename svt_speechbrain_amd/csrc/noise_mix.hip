// Noise mixing at several SNRs (svt_noise_mix; N20EMv2/audio_visual/synthesis_noise.py:123-137 over speechbrain's compute_amplitude and
// dB_to_amplitude): for a clean track a, a noise track v and S signal-to-noise ratios,
//     f_s = 1 / (10^(snr_s / 20) + 1)        A_a = mean |a|, A_v = mean |v|        out_s = (1 - f_s) a + (f_s A_a / (A_v + 1e-14)) v
// in two launches and nine passes over a track where the reference's per-SNR chain takes about sixty:
//   noise_abs_sums_kernel   both tracks in one launch (blockIdx.y = track): sum |x| in fp64, one partial per workgroup, plain stores.
//   noise_mix_kernel<S>     every workgroup adds the partials of both tracks in workgroup order (at most kNoiseAmpBlocks each: one load per
//                           thread and track, then a shuffle tree of fixed shape -- every workgroup computes the same bits, no atomics, no
//                           ticket, nothing to zero), derives the 2 S coefficients in fp64 and rounds each ONCE to fp32, then reads a[i] and
//                           v[i] once and writes the S rows out[s * ld + i] = fma(c2_s, v[i], c1_s * a[i]).
// The sums are reproducible bit for bit, hence so are the mixtures.  A zero noise track (A_v == 0) takes c2 = 0: the mixture is c1 a.
// out == null: the amplitudes alone.
// Addressing: any 4-byte-aligned a, v, out and any ld >= n.  The scalar head peel brings the body to a 16-byte boundary of the track
// (sums) or of out's first row (mix); the other streams of the mix use 16-byte accesses that promise 4-byte alignment only, which is all
// global_load_dwordx4 / global_store_dwordx4 ask for.  Nothing is written at out[s * ld + n .. (s + 1) * ld).
#include "device_util.h"

namespace svt {
namespace {
constexpr int kNoiseAmpBlocks = 256;    // SVT_NOISE_AMP_WORKGROUPS: workgroups per track of the sums (one partial each)
constexpr int kNoiseMixBlocks = 2048;   // SVT_NOISE_MIX_MAX_WORKGROUPS: the mix grid's cap; beyond it the loop strides
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));   // 16 bytes at a 4-byte-aligned address

__device__ __forceinline__ int64_t head_peel(const void* p, int64_t n) {   // elements in front of p's next 16-byte boundary
  const int64_t h = (int64_t)((0 - ((uintptr_t)p >> 2)) & 3);
  return h < n ? h : n;
}
__device__ __forceinline__ double abs_sum4(f32x4 v) {
  return ((double)fabsf(v.x) + (double)fabsf(v.y)) + ((double)fabsf(v.z) + (double)fabsf(v.w));
}

// part[track * gridDim.x + block] = this workgroup's share of sum |x| (fp64 adds of the exact fp32 magnitudes, in a fixed order)
__global__ __launch_bounds__(256) void noise_abs_sums_kernel(const float* clean, const float* noise, int64_t n, double* part) {
  __shared__ double sh[4];
  const float* x = blockIdx.y ? noise : clean;
  const int64_t head = head_peel(x, n), n4 = (n - head) >> 2;
  const f32x4* x4 = (const f32x4*)(x + head);
  const int64_t stride = (int64_t)gridDim.x * 256;
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double s = 0.0;
  for (; i + 3 * stride < n4; i += 4 * stride) {   // four 16-byte loads in flight per lane
    const f32x4 v0 = x4[i], v1 = x4[i + stride], v2 = x4[i + 2 * stride], v3 = x4[i + 3 * stride];
    s += (abs_sum4(v0) + abs_sum4(v1)) + (abs_sum4(v2) + abs_sum4(v3));
  }
  for (; i < n4; i += stride) s += abs_sum4(x4[i]);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    for (int64_t j = 0; j < head; ++j) s += (double)fabsf(x[j]);
    for (int64_t j = head + (n4 << 2); j < n; ++j) s += (double)fabsf(x[j]);
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

struct NoiseFactors { double f[8]; };   // f_s of every row, computed on the host in double as the reference's Python does

template <int S>
__global__ __launch_bounds__(256) void noise_mix_kernel(const float* __restrict__ a, const float* __restrict__ v, int64_t n,
                                                        float* __restrict__ out, int64_t ld, NoiseFactors fac,
                                                        const double* __restrict__ part, int n_part, double* __restrict__ amps_out) {
  __shared__ double sh[2][4];
  __shared__ float cs[2][8];
  double pa = 0.0, pv = 0.0;
  for (int b = threadIdx.x; b < n_part; b += 256) { pa += part[b]; pv += part[n_part + b]; }
  pa = wave_sum(pa);
  pv = wave_sum(pv);
  if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = pa; sh[1][threadIdx.x >> 6] = pv; }
  __syncthreads();
  if (threadIdx.x < S) {
    const double amp_a = ((sh[0][0] + sh[0][1]) + (sh[0][2] + sh[0][3])) / (double)n;
    const double amp_v = ((sh[1][0] + sh[1][1]) + (sh[1][2] + sh[1][3])) / (double)n;
    double f = 0.0;
#pragma unroll
    for (int s = 0; s < S; ++s) f = (int)threadIdx.x == s ? fac.f[s] : f;
    // each coefficient: fp64 throughout, ONE rounding to fp32.  A silent noise track has nothing to scale: c2 = 0 (the quotient
    // f A_a / 1e-14 may exceed fp32's range, and inf * 0 must not reach the output)
    cs[0][threadIdx.x] = (float)(1.0 - f);
    cs[1][threadIdx.x] = amp_v == 0.0 ? 0.f : (float)(f * amp_a / (amp_v + 1e-14));
    if (amps_out && blockIdx.x == 0 && threadIdx.x == 0) { amps_out[0] = amp_a; amps_out[1] = amp_v; }
  }
  if (!out) return;   // the amplitudes alone (one workgroup)
  __syncthreads();
  float c1[S], c2[S];
#pragma unroll
  for (int s = 0; s < S; ++s) { c1[s] = cs[0][s]; c2[s] = cs[1][s]; }
  const int64_t head = head_peel(out, n), n4 = (n - head) >> 2;
  const f32x4u* a4 = (const f32x4u*)(a + head);
  const f32x4u* v4 = (const f32x4u*)(v + head);
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    const f32x4u x = a4[i], y = v4[i];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      f32x4u r;
      r.x = fmaf(c2[s], y.x, c1[s] * x.x);
      r.y = fmaf(c2[s], y.y, c1[s] * x.y);
      r.z = fmaf(c2[s], y.z, c1[s] * x.z);
      r.w = fmaf(c2[s], y.w, c1[s] * x.w);
      *(f32x4u*)(out + s * ld + head + (i << 2)) = r;
    }
  }
  if (blockIdx.x == 0) {   // the peels: lanes 0-2 the head, lanes 64-66 the tail, one element and S rows each
    const int64_t tail0 = head + (n4 << 2);
    int64_t j = -1;
    if ((int64_t)threadIdx.x < head) j = threadIdx.x;
    else if (threadIdx.x >= 64 && tail0 + (threadIdx.x - 64) < n && threadIdx.x < 68) j = tail0 + (threadIdx.x - 64);
    if (j >= 0) {
      const float x = a[j], y = v[j];
#pragma unroll
      for (int s = 0; s < S; ++s) out[s * ld + j] = fmaf(c2[s], y, c1[s] * x);
    }
  }
}

template <int S>
int launch_mix_s(const float* a, const float* v, int64_t n, float* out, int64_t ld, const NoiseFactors& f, const double* part, int n_part,
                 double* amps, hipStream_t s) {
  hipLaunchKernelGGL((noise_mix_kernel<S>), dim3(out ? grid_for(n / 4 + 1, 256, kNoiseMixBlocks) : 1), dim3(256), 0, s, a, v, n, out, ld, f,
                     part, n_part, amps);
  SVT_LAUNCH_CHECK();
  return 0;
}
}  // namespace

size_t noise_mix_scratch_bytes() { return (size_t)2 * kNoiseAmpBlocks * sizeof(double); }

int launch_noise_mix(const float* clean, const float* noise, int64_t n, const double* factors, int n_snr, float* out, int64_t ld,
                     double* amps_out, void* scratch, hipStream_t s) {
  if (n < 1 || n_snr < 1 || n_snr > 8 || ld < n || (!out && !amps_out)) { set_error("noise_mix: bad geometry"); return -1; }
  if (!aligned(3, clean, noise, out) || !aligned(7, amps_out, scratch) || !scratch) { set_error("noise_mix: alignment"); return -1; }
  double* part = (double*)scratch;
  const int n_part = grid_for(n / 4 + 1, 256, kNoiseAmpBlocks);
  hipLaunchKernelGGL(noise_abs_sums_kernel, dim3(n_part, 2), dim3(256), 0, s, clean, noise, n, part);
  SVT_LAUNCH_CHECK();
  NoiseFactors f;
  for (int i = 0; i < 8; ++i) f.f[i] = i < n_snr ? factors[i] : 0.0;
  switch (n_snr) {
    case 1: return launch_mix_s<1>(clean, noise, n, out, ld, f, part, n_part, amps_out, s);
    case 2: return launch_mix_s<2>(clean, noise, n, out, ld, f, part, n_part, amps_out, s);
    case 3: return launch_mix_s<3>(clean, noise, n, out, ld, f, part, n_part, amps_out, s);
    case 4: return launch_mix_s<4>(clean, noise, n, out, ld, f, part, n_part, amps_out, s);
    case 5: return launch_mix_s<5>(clean, noise, n, out, ld, f, part, n_part, amps_out, s);
    case 6: return launch_mix_s<6>(clean, noise, n, out, ld, f, part, n_part, amps_out, s);
    case 7: return launch_mix_s<7>(clean, noise, n, out, ld, f, part, n_part, amps_out, s);
    default: return launch_mix_s<8>(clean, noise, n, out, ld, f, part, n_part, amps_out, s);
  }
}

}  // namespace svt
