// Everything that sums over the workgroups of a launch: the whole-batch moments of the wrapper's two norms, the window moments of conv
// layer 0's GroupNorm, and the fused frame head with the output norm's moments.  They share the ticket reduction below, whose A/B switch
// is ONE __device__ variable -- so they share this translation unit (tests/test_gpu_statistics.py tests it as a unit).
#include "device_util.h"

namespace svt {
namespace {
// ---- sums over the workgroups of a launch, reproducible bit for bit ----
// fp64 atomicAdd gives a sum whose last bits depend on the order in which the workgroups arrive; conv layer 0's GroupNorm variance is a
// quadratic form of the window moments with heavy cancellation (low-pass audio against random filters: 1e3-1e5), so a changed last bit
// of a moment can flip the last bit of an fp32 coefficient, and one flipped bf16 rounding downstream moves every logit by ~1e-4.  (This
// was the first suspect when the eight-rank dry run of bench.py --verify on one GPU began to fail; the forwards that differed there
// turned out to come from a split load in head_dots_kernel, below -- but arrival order was the one input of the forward that is not a
// function of its arguments, so it went too.)
// Instead every workgroup stores its partial sums and takes a ticket; the one that draws the last ticket adds the partials in workgroup
// order and writes the result (no zeroed accumulator needed; the ticket must be 0 at launch and is put back to 0).
// (No fence: an agent-scope release fence is an L2 write-back on this chip, and one per workgroup made the three statistics kernels
// 30-50 us slower each.  The partials are WRITE-THROUGH stores -- st_partial -- whose acknowledgement the vmcnt wait below awaits, the
// ticket is an agent-scope atomic behind it, and the reader uses loads that bypass the non-coherent caches -- ld_partial.)
__device__ __forceinline__ void st_partial(double* p, double v) {
  __hip_atomic_store((unsigned long long*)p, __builtin_bit_cast(unsigned long long, v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// A/B arm (svt_debug_set key 32 = 1): the ticket as an agent-scope ACQUIRE-RELEASE atomic -- the form the HIP / LLVM memory
// model asks for (release: this workgroup's partials are visible before the ticket; acquire: the last workgroup sees everyone's).  The
// default (0) is the relaxed form described above, which leans on what gfx950 does with write-through stores and cache-bypassing loads;
// tests/test_gpu_statistics.py holds BOTH arms to host fp64 sums of the same inputs and to each other, bit for bit.
__device__ int d_ticket_fenced = 0;
__device__ __forceinline__ bool last_workgroup(unsigned* ticket, unsigned n_groups) {
  __shared__ unsigned s_last;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this thread's partials have reached the level every XCD reads from
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned t = d_ticket_fenced ? __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT)
                                       : __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = t == n_groups - 1 ? 1u : 0u;
    if (s_last) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  return s_last != 0;
}
// a partial written by another workgroup (possibly on another XCD): read past the non-coherent caches
__device__ __forceinline__ double ld_partial(const double* p) {
  return __builtin_bit_cast(double, __hip_atomic_load((const unsigned long long*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
}  // namespace
int set_ticket_fenced(int on) {   // svt_debug_set key 32
  const int v = on ? 1 : 0;
  SVT_HIP(hipMemcpyToSymbol(HIP_SYMBOL(d_ticket_fenced), &v, sizeof(int)));
  return 0;
}

namespace {
// sum / sum of squares in fp64 (two whole-batch layer norms of the wrapper)
// blockIdx.y = norm group: group g covers x[g*n, (g+1)*n) and WRITES mom[2g], mom[2g+1] (the last workgroup of the group adds the
// per-workgroup partials `part[(g * gridDim.x + block) * 2 ..]` in block order: last_workgroup above)
__global__ __launch_bounds__(256) void moments_kernel(const float* x, int64_t n, double* mom, double* part, unsigned* ticket) {
  __shared__ double sh[2][4];
  x += (int64_t)blockIdx.y * n;
  mom += 2 * blockIdx.y;
  part += (size_t)blockIdx.y * gridDim.x * 2;
  double s = 0.0, ss = 0.0;
  const int64_t n4 = n >> 2;
  const float4* x4 = (const float4*)x;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n4; i += stride) {
    const float4 v = x4[i];
    // fp32 partial of 4 terms, then fp64: keeps the stream cheap and the long sum exact enough
    const float a = (v.x + v.y) + (v.z + v.w);
    const float b = (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
    s += (double)a;
    ss += (double)b;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    for (int64_t j = n4 << 2; j < n; ++j) { s += (double)x[j]; ss += (double)x[j] * (double)x[j]; }
  }
  s = wave_sum(s);
  ss = wave_sum(ss);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { sh[0][wave] = s; sh[1][wave] = ss; }
  __syncthreads();
  if (threadIdx.x == 0) {
    st_partial(part + blockIdx.x * 2, sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3]);
    st_partial(part + blockIdx.x * 2 + 1, sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3]);
  }
  if (!last_workgroup(ticket + blockIdx.y, gridDim.x)) return;
  s = 0.0; ss = 0.0;
  for (unsigned b = threadIdx.x; b < gridDim.x; b += 256) { s += ld_partial(part + b * 2); ss += ld_partial(part + b * 2 + 1); }
  s = wave_sum(s);
  ss = wave_sum(ss);
  if (lane == 0) { sh[0][wave] = s; sh[1][wave] = ss; }
  __syncthreads();
  if (threadIdx.x == 0) {
    mom[0] = sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3];
    mom[1] = sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3];
  }
}

__global__ void global_norm_kernel(const float* x, float* y, int64_t n, const double* mom, float eps, double n_stat) {
  x += (int64_t)blockIdx.y * n;
  y += (int64_t)blockIdx.y * n;
  mom += 2 * blockIdx.y;
  const double mean = mom[0] / n_stat;   // n_stat: the elements the moments were summed over (= n, or the global count when
  const double var = mom[1] / n_stat - mean * mean;   // the sums were reduced over ranks: svt_encoder_set_norm_reduce)
  const float mu = (float)mean;
  const float rs = (float)(1.0 / sqrt(var + (double)eps));
  const int64_t n4 = n >> 2;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n4; i += stride) {
    float4 v = ((const float4*)x)[i];
    v.x = (v.x - mu) * rs; v.y = (v.y - mu) * rs; v.z = (v.z - mu) * rs; v.w = (v.w - mu) * rs;
    ((float4*)y)[i] = v;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (int64_t j = n4 << 2; j < n; ++j) y[j] = (x[j] - mu) * rs;
}
}  // namespace
// scratch of one launch_moments call over at most `groups_max` groups: a ticket per group, then two fp64 partials per workgroup
static int moments_grid(int64_t n, int groups) {
  return groups > 1 ? grid_for(n / 4 + 1, 256, 512 / (groups < 64 ? groups : 64) + 1) : grid_for(n / 4 + 1, 256, 512);
}
int g_c0_kernel_id = 0;  // svt_debug_set key 41 (query): 100 * kernel + 10 * PK + (16-bit rows) of the last front-end launch (include/svt_mi355.h lists the ids)
size_t moments_ticket_bytes(int groups) { return ((size_t)groups * 4 + 255) & ~(size_t)255; }
size_t moments_scratch_bytes(int groups_max) {
  // groups < 64: groups * (512 / groups + 1) <= 512 + groups workgroups; otherwise 9 per group
  const size_t wgs = (size_t)(groups_max < 64 ? 512 + groups_max : 576) + 9 * (size_t)groups_max;
  return moments_ticket_bytes(groups_max) + wgs * 2 * sizeof(double);
}

int launch_moments(const float* x, int64_t n, double* moments, void* scratch, int groups_max, hipStream_t s, int groups) {
  if (groups > 1 && (n & 3)) { set_error("moments: per-group length must be a multiple of 4 elements"); return -1; }
  if (groups > groups_max || !scratch || ((uintptr_t)scratch & 7)) { set_error("moments: scratch"); return -1; }
  const int gx = moments_grid(n, groups);
  if (moments_ticket_bytes(groups_max) + (size_t)gx * groups * 2 * sizeof(double) > moments_scratch_bytes(groups_max)) { set_error("moments: scratch too small"); return -1; }
  unsigned* ticket = (unsigned*)scratch;
  double* part = (double*)((char*)scratch + moments_ticket_bytes(groups_max));
  g_c0_kernel_id = 100;
  hipLaunchKernelGGL(moments_kernel, dim3(gx, groups), dim3(256), 0, s, x, n, moments, part, ticket);
  SVT_LAUNCH_CHECK();
  return 0;
}

int launch_global_norm(const float* x, float* y, int64_t n, const double* moments, float eps, hipStream_t s, int groups, double n_stat) {
  if (groups > 1 && (n & 3)) { set_error("global_norm: per-group length must be a multiple of 4 elements"); return -1; }
  hipLaunchKernelGGL(global_norm_kernel, dim3(grid_for(n / 4 + 1), groups), dim3(256), 0, s, x, y, n, moments, eps,
                     n_stat > 0 ? n_stat : (double)n);
  SVT_LAUNCH_CHECK();
  return 0;
}

// conv layer 0, "group" mode.  GroupNorm(C groups) needs per-(clip,channel) mean/var over ALL frames
// before the GELU.  Because Cin = 1, y[c,t] = w_c . window_t, so the statistics of all C channels
// follow exactly from the first and second moments of the 10-sample windows:
//   mean_c = w_c . E[win] ,  E[y_c^2] = w_c^T E[win win^T] w_c
// (65 fp64 sums per clip) — one cheap pass over the waveform instead of a second pass over the
// (B, T1, 512) activation.
namespace {
__global__ __launch_bounds__(256) void conv0_window_moments_kernel(const float* wav, int64_t L, int stride, int64_t T1,
                                                                   double* wm, double* part, unsigned* ticket) {
  __shared__ double sh[4][NWM];
  const int b = blockIdx.y;
  const float* x = wav + (int64_t)b * L;
  double acc[NWM];
#pragma unroll
  for (int i = 0; i < NWM; ++i) acc[i] = 0.0;
  constexpr int WPT = 8;  // windows per thread
  const int64_t t0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * WPT;
  for (int w = 0; w < WPT; ++w) {
    const int64_t t = t0 + w;
    if (t >= T1) break;
    float v[K0];
#pragma unroll
    for (int j = 0; j < K0; ++j) v[j] = x[t * stride + j];
    int idx = K0;
#pragma unroll
    for (int j = 0; j < K0; ++j) {
      acc[j] += (double)v[j];
#pragma unroll
      for (int j2 = j; j2 < K0; ++j2) acc[idx++] += (double)(v[j] * v[j2]);
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NWM; ++i) {
    const double r = wave_sum(acc[i]);
    if (lane == 0) sh[wave][i] = r;
  }
  __syncthreads();
  // per-workgroup partials, added in workgroup order by the clip's last workgroup (last_workgroup above): wm is written, not accumulated
  part += (size_t)b * gridDim.x * NWM;
  if (threadIdx.x < NWM)
    st_partial(part + blockIdx.x * NWM + threadIdx.x, sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x]);
  if (!last_workgroup(ticket + b, gridDim.x)) return;
  if (threadIdx.x < NWM) {
    // (eight loads in flight, added in workgroup order: one load per trip made the loop a chain of memory round trips)
    double t = 0.0;
    unsigned k = 0;
    for (; k + 8 <= gridDim.x; k += 8) {
      double v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = ld_partial(part + (k + j) * NWM + threadIdx.x);
#pragma unroll
      for (int j = 0; j < 8; ++j) t += v[j];
    }
    for (; k < gridDim.x; ++k) t += ld_partial(part + k * NWM + threadIdx.x);
    wm[b * NWM + threadIdx.x] = t;
  }
}

__global__ void conv0_group_coef_kernel(const double* wav_mom, int64_t n_wav, const double* wm, int64_t T1, int C,
                                        const float* w0, const float* b0, const float* gamma, const float* beta,
                                        float eps_wav, float eps_gn, float* coef, int cpg) {
  const int b = blockIdx.y;
  if (wav_mom) wav_mom += 2 * (b / cpg);  // the waveform norm group of this clip
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double mu = 0.0, r = 1.0;
  if (wav_mom) {
    mu = wav_mom[0] / (double)n_wav;
    const double var = wav_mom[1] / (double)n_wav - mu * mu;
    r = 1.0 / sqrt(var + (double)eps_wav);
  }
  const double* m = wm + b * NWM;
  const double invT = 1.0 / (double)T1;
  double w[K0], mn[K0];
  double wsum = 0.0;
  for (int j = 0; j < K0; ++j) { w[j] = (double)w0[c * K0 + j]; wsum += w[j]; mn[j] = r * (m[j] * invT - mu); }
  const double bias = b0 ? (double)b0[c] : 0.0;
  double dot = 0.0;
  for (int j = 0; j < K0; ++j) dot += w[j] * mn[j];
  double quad = 0.0;
  int idx = K0;
  for (int j = 0; j < K0; ++j)
    for (int j2 = j; j2 < K0; ++j2) {
      const double R = r * r * (m[idx] * invT - mu * m[j] * invT - mu * m[j2] * invT + mu * mu);
      quad += (j == j2 ? 1.0 : 2.0) * w[j] * w[j2] * R;
      ++idx;
    }
  const double mean = dot + bias;
  const double e2 = quad + 2.0 * bias * dot + bias * bias;
  double var = e2 - mean * mean;
  if (var < 0.0) var = 0.0;
  const double a = (double)gamma[c] / sqrt(var + (double)eps_gn);
  const double shift = (double)beta[c] - mean * a;
  float* o = coef + ((int64_t)b * C + c) * (K0 + 1);
  for (int j = 0; j < K0; ++j) o[j] = (float)(a * r * w[j]);
  o[K0] = (float)(a * (bias - r * mu * wsum) + shift);
}
}  // namespace
// scratch: a ticket per clip, then 65 fp64 partials per workgroup
size_t conv0_window_moments_scratch_bytes(int B, int64_t T1) {
  const size_t gx = (size_t)((T1 + 2047) / 2048);
  return moments_ticket_bytes(B) + (size_t)B * gx * NWM * sizeof(double);
}

int launch_conv0_window_moments(const float* wav, int B, int64_t L, int k, int stride, int64_t T1, double* wm, void* scratch,
                                hipStream_t s) {
  if (k != K0) { set_error("conv layer 0 kernel size must be 10"); return -1; }
  if (!scratch || ((uintptr_t)scratch & 7)) { set_error("conv0 window moments: scratch"); return -1; }
  const int per_block = 256 * 8;
  dim3 grid((unsigned)((T1 + per_block - 1) / per_block), B);
  unsigned* ticket = (unsigned*)scratch;
  double* part = (double*)((char*)scratch + moments_ticket_bytes(B));
  g_c0_kernel_id = 200;
  hipLaunchKernelGGL(conv0_window_moments_kernel, grid, dim3(256), 0, s, wav, L, stride, T1, wm, part, ticket);
  SVT_LAUNCH_CHECK();
  return 0;
}

int launch_conv0_group_coef(const double* wav_moments, int64_t n_wav, const double* wm, int B, int64_t T1, int C,
                            int k, const float* w0, const float* b0, const float* gamma, const float* beta,
                            float eps_wav, float eps_gn, float* coef, hipStream_t s, int cpg) {
  if (k != K0) { set_error("conv layer 0 kernel size must be 10"); return -1; }
  dim3 grid((C + 63) / 64, B);
  g_c0_kernel_id = 300;
  hipLaunchKernelGGL(conv0_group_coef_kernel, grid, dim3(64), 0, s, wav_moments, n_wav, wm, T1, C, w0, b0, gamma, beta,
                     eps_wav, eps_gn, coef, cpg);
  SVT_LAUNCH_CHECK();
  return 0;
}

// Fused tail of the audio recipes ("fuse with a2's out-LN and a9"): the wrapper's whole-batch output norm
// (huggingface_interface.py:294-295), the 20-way frame head (speechbrain/nnet/linear.py:63-76) and the per-frame
// sigmoid / argmax (train_audio_ssl.py:93-100) WITHOUT materialising the normalised features.  The head is linear, so
//     logits[r][j] = ((x[r] - mu) * rs) . w[j] + b[j] = (x[r] . w[j] - mu * sum_k w[j][k]) * rs + b[j]
// and the raw dots x[r] . w[j] can be taken in the same single pass over the un-normalised encoder output that sums the
// two moments of the norm (per group of rows: clips_per_norm_group).  Pass 1 = head_dots_kernel (the frame-head kernel
// plus fp64 row-sum accumulation); pass 2 = head_finish_kernel over rows x N values: affine fix-up, logits, decode.
// Replaces moments + global_norm + linear_head + decode_frames (three reads and one write of the 49 MB feature tensor
// at 32 x 10 s) by one read.
namespace {
template <int KC>
__global__ __launch_bounds__(256) void head_dots_kernel(const float* __restrict__ x, int64_t rows, const float* __restrict__ w, int N,
                                                        float* __restrict__ dots, double* __restrict__ mom, int64_t rows_per_group,
                                                        double* __restrict__ slots, unsigned* __restrict__ ticket, int slots_per_group) {
  constexpr int K = KC * 256;
  extern __shared__ __attribute__((aligned(16))) float wl[];
  for (int i = threadIdx.x * 4; i < N * K; i += 1024) *(float4*)(wl + i) = *(const float4*)(w + i);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool hi32 = (lane & 32) != 0, hi16 = (lane & 16) != 0;
  const int myrow = (hi32 ? 2 : 0) + (hi16 ? 1 : 0);
  // per-lane running (sum, sum of squares) of the norm group this wave is in: folded across the wave and stored when the wave's rows
  // cross into another group (and at the end) -- no shuffles and no division per row.  The statistics are reproducible bit for bit
  // (last_workgroup above): wave W = 4 blockIdx.x + wave owns the 4-row chunks W, W + NW, W + 2 NW ... (NW = waves of the launch), so the
  // waves that meet norm group g are those of the chunks ja = first row of g / 4 ... jb = last row of g / 4, taken modulo NW; a wave stores
  // its (sum, sum of squares) for g ONCE, in slot (g, (W - ja) mod NW) -- every slot 0 .. min(NW, jb - ja + 1) - 1 of a group is written by
  // exactly one wave, none needs zeroing -- and the launch's last workgroup adds each group's slots in slot order.
  const int NW = (int)gridDim.x * 4, W = (int)blockIdx.x * 4 + wave;
  int64_t cur_g = -1, g_end = 0;
  float la = 0.f, lq = 0.f;
  auto flush = [&]() {
    if (cur_g < 0) return;
    const double sa = wave_sum((double)la), sq = wave_sum((double)lq);
    if (lane == 0) {
      const int64_t ja = (cur_g * rows_per_group) >> 2;
      const int p = (int)(((W - ja) % NW + NW) % NW);
      double* sl = slots + ((size_t)cur_g * slots_per_group + p) * 2;
      st_partial(sl, sa);
      st_partial(sl + 1, sq);
    }
    la = 0.f; lq = 0.f;
  };
  for (int64_t r0 = ((int64_t)blockIdx.x * 4 + wave) * 4; r0 < rows; r0 += (int64_t)gridDim.x * 16) {
    float4 xv[4][KC];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int64_t row = r0 + rr < rows ? r0 + rr : rows - 1;
      // 16-byte loads the compiler cannot take apart (raw buffer loads).  Round 4 wrote `*(const float4*)`; hipcc split the first chunk of
      // every row into an OVERLAPPING pair -- global_load_dwordx3 at byte 4 + global_load_dwordx2 at byte 0 -- and placed its own counted
      // `s_waitcnt vmcnt(14 / 13 / 12 ...)` in front of the packed squares.  With other processes loading the same GPU the sum of squares
      // then came out short by 12-35 elements' worth in ~0.15 % of the forwards (sum and dots intact; every logit moved by 2e-4 .. 1e-3
      // through the output norm): tools/determinism_stress.py, 10 of 6 400 forwards.  Three rebuilds, 6 400 forwards each, all clean: a
      // full wait in front of the statistics; scalar FMAs; and this one -- the same packed arithmetic and the same counted waits behind
      // UNSPLIT loads.  WHICH instruction of the round-4 sequence misbehaves is not isolated: a microbenchmark of the pair, the counted wait
      // and reads / overwrites of the destination registers right behind it (tools/microbench/split_load_probe.hip) saw no stale value in
      // 2e10 lane-rows under the same eight-process load.  The kernel-level evidence stands; tests/test_build_isa.py keeps split pairs out.
      const auto xrs = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, 0x7FFFFFF0, 0x00020000);
#pragma unroll
      for (int c = 0; c < KC; ++c) {
        typedef float f4v __attribute__((ext_vector_type(4)));
        const f4v t = __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(xrs, (unsigned)((row * K + c * 256 + lane * 4) * 4), 0, 0));
        xv[rr][c] = float4{t[0], t[1], t[2], t[3]};
      }
    }
    if (mom) {
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        if (r0 + rr >= rows) break;  // wave-uniform
        if (r0 + rr >= g_end || cur_g < 0) {  // rare: first row of the wave, or a group boundary
          flush();
          cur_g = (r0 + rr) / rows_per_group;
          g_end = (cur_g + 1) * rows_per_group;
        }
        float a = 0.f, q = 0.f;
#pragma unroll
        for (int c = 0; c < KC; ++c) {
          const float4 v = xv[rr][c];
          a += (v.x + v.y) + (v.z + v.w);
          q += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
        }
        la += a;
        lq += q;
      }
    }
    float out0 = 0.f, out1 = 0.f;
    for (int n = 0; n < N; ++n) {
      float sacc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < KC; ++c) {
        const float4 wv = *(const float4*)(wl + n * K + c * 256 + lane * 4);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          sacc[rr] = fmaf(xv[rr][c].x, wv.x, sacc[rr]);
          sacc[rr] = fmaf(xv[rr][c].y, wv.y, sacc[rr]);
          sacc[rr] = fmaf(xv[rr][c].z, wv.z, sacc[rr]);
          sacc[rr] = fmaf(xv[rr][c].w, wv.w, sacc[rr]);
        }
      }
      float k0 = hi32 ? sacc[2] : sacc[0], k1 = hi32 ? sacc[3] : sacc[1];
      const float g0 = hi32 ? sacc[0] : sacc[2], g1 = hi32 ? sacc[1] : sacc[3];
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
      if (n0 < N) dots[row * N + n0] = out0;
      if (n0 + 16 < N) dots[row * N + n0 + 16] = out1;
    }
  }
  if (mom) {
    flush();
    if (!last_workgroup(ticket, gridDim.x)) return;
    // the last workgroup: group g's slots in slot order, one wave per group (lane-strided partial sums, then the shuffle tree: a fixed shape)
    const int64_t n_groups = (rows + rows_per_group - 1) / rows_per_group;
    for (int64_t g = wave; g < n_groups; g += 4) {
      const int64_t a = g * rows_per_group, b = (g + 1) * rows_per_group < rows ? (g + 1) * rows_per_group : rows;
      const int64_t nj = ((b - 1) >> 2) - (a >> 2) + 1;
      const int n = (int)(nj < NW ? nj : NW);
      const double* sl = slots + (size_t)g * slots_per_group * 2;
      double ta = 0.0, tq = 0.0;
      int i = lane;
      for (; i + 3 * 64 < n; i += 4 * 64) {   // eight loads in flight per lane, added in slot order
        double va[4], vq[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { va[j] = ld_partial(sl + 2 * (i + 64 * j)); vq[j] = ld_partial(sl + 2 * (i + 64 * j) + 1); }
#pragma unroll
        for (int j = 0; j < 4; ++j) { ta += va[j]; tq += vq[j]; }
      }
      for (; i < n; i += 64) { ta += ld_partial(sl + 2 * i); tq += ld_partial(sl + 2 * i + 1); }
      ta = wave_sum(ta);
      tq = wave_sum(tq);
      if (lane == 0) { mom[2 * g] = ta; mom[2 * g + 1] = tq; }
    }
  }
}

// one thread per row: logits = (dots - mean * wsum) * rstd + bias; optional per-frame decode (same rule as decode_frames_kernel)
__global__ void head_finish_kernel(const float* __restrict__ dots, int64_t rows, int N, const float* __restrict__ wsum,
                                   const float* __restrict__ bias, const double* __restrict__ mom, int64_t rows_per_group,
                                   double group_elems, float eps, float* __restrict__ logits, FrameOut* __restrict__ frames,
                                   int n_oct, int n_cls) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  float mu = 0.f, rs = 1.f;
  if (mom) {
    const int64_t g = r / rows_per_group;
    const double mean = mom[2 * g] / group_elems;
    const double var = mom[2 * g + 1] / group_elems - mean * mean;
    mu = (float)mean;
    rs = (float)(1.0 / sqrt(var + (double)eps));
  }
  float l[32];
#pragma unroll
  for (int j = 0; j < 32; ++j)
    if (j < N) {
      l[j] = fmaf(dots[r * N + j] - mu * wsum[j], rs, bias ? bias[j] : 0.f);
      logits[r * N + j] = l[j];
    }
  if (frames) {
    FrameOut f;
    f.p_on = 1.f / (1.f + expf(-l[0]));
    f.p_off = 1.f / (1.f + expf(-l[1]));
    int bo = 0;
    float bv = l[2];
#pragma unroll
    for (int j = 3; j < 32; ++j)
      if (j <= 2 + n_oct && l[j] > bv) { bv = l[j]; bo = j - 2; }
    int bc = 0;
    const int c0 = 2 + n_oct + 1;
    bv = -3.4e38f;
#pragma unroll
    for (int j = 3; j < 32; ++j)
      if (j >= c0 && j <= c0 + n_cls) {
        if (j == c0) { bv = l[j]; bc = 0; }
        else if (l[j] > bv) { bv = l[j]; bc = j - c0; }
      }
    f.octave = bo;
    f.pitch_class = bc;
    frames[r] = f;
  }
}
}  // namespace
static unsigned head_dots_grid(int64_t rows) {
  const int64_t blocks = (rows + 15) / 16;
  return (unsigned)(blocks < 512 ? blocks : 512);
}
// scratch of the output-norm statistics (head_dots_kernel): a ticket, then one (sum, sum of squares) slot per wave and norm group it meets:
// at most rows / 4 + 2 slots per group, never more than the launch has waves
static int head_slots_per_group(int64_t rows, int64_t rpg) {
  const int64_t nw = (int64_t)head_dots_grid(rows) * 4, per = (rpg + 3) / 4 + 1;
  return (int)(per < nw ? per : nw);
}
size_t head_scratch_bytes(int64_t rows, int groups_max) {
  // for any group size: groups * min(NW, rpg / 4 + 2) <= rows / 4 + 2 groups
  return 256 + ((size_t)rows / 4 + 2 * (size_t)groups_max + 8) * 2 * sizeof(double);
}

template <int KC>
static int launch_head_dots_kc(const float* x, int64_t rows, const float* w, int N, float* dots, double* mom, int64_t rpg, void* scratch,
                               hipStream_t s) {
  const size_t lds = (size_t)N * KC * 256 * 4;
  if (int r_ = ensure_dyn_lds((const void*)head_dots_kernel<KC>, 32 * KC * 256 * 4)) return r_;
  const unsigned grid = head_dots_grid(rows);
  if (mom && (!scratch || ((uintptr_t)scratch & 7))) { set_error("head_fused: scratch"); return -1; }
  if ((unsigned long)rows * KC * 256 * 4 > 0x7FFFFFF0ul) { set_error("head_fused: more than 2 GiB of encoder output (32-bit buffer offsets)"); return -1; }
  unsigned* ticket = (unsigned*)scratch;
  double* slots = scratch ? (double*)((char*)scratch + 256) : nullptr;
  hipLaunchKernelGGL((head_dots_kernel<KC>), dim3(grid), dim3(256), lds, s, x, rows, w, N, dots, mom, rpg, slots, ticket,
                     mom ? head_slots_per_group(rows, rpg) : 0);
  SVT_LAUNCH_CHECK();
  return 0;
}
int launch_head_fused(const float* x, int64_t rows, int K, const float* w, const float* wsum, const float* b, int N, float* dots,
                      double* mom /*2 per group (written); null = no output norm*/, int64_t rows_per_group, float eps, float* logits,
                      FrameOut* frames, int n_oct, int n_cls, hipStream_t s, double n_stat, int (*between)(void*), void* between_arg,
                      void* scratch /*head_scratch_bytes(rows, groups); its first 4 bytes ZERO*/) {
  if (!linear_head_eligible(K, N)) { set_error("head_fused: unsupported head geometry"); return -1; }
  if (frames && (N != 2 + n_oct + 1 + n_cls + 1 || N > 32)) { set_error("head_fused: n_out != 2 + (n_octave+1) + (n_class+1)"); return -1; }
  if (mom) {
    const int64_t groups = (rows + rows_per_group - 1) / rows_per_group;
    if (256 + (size_t)groups * head_slots_per_group(rows, rows_per_group) * 16 > head_scratch_bytes(rows, (int)groups)) { set_error("head_fused: scratch too small"); return -1; }
  }
  int r = K == 512 ? launch_head_dots_kc<2>(x, rows, w, N, dots, mom, rows_per_group, scratch, s)
        : K == 768 ? launch_head_dots_kc<3>(x, rows, w, N, dots, mom, rows_per_group, scratch, s)
                   : launch_head_dots_kc<4>(x, rows, w, N, dots, mom, rows_per_group, scratch, s);
  if (r) return r;
  if (between) { if (int rb = between(between_arg)) return rb; }   // the moments are complete here: cross-rank reduction hook
  hipLaunchKernelGGL(head_finish_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, dots, rows, N, wsum, b, mom,
                     rows_per_group, n_stat > 0 ? n_stat : (double)rows_per_group * (double)K, eps, logits, frames, n_oct, n_cls);
  SVT_LAUNCH_CHECK();
  return 0;
}

}  // namespace svt
