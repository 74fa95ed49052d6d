// Polyphase resampling with an optional stereo downmix (svt_resample; speechbrain/processing/speech_augmentation.py:479-789, Kaldi's
// LinearResample, and the `.mean(dim=0)` the prepare scripts run behind it).  With S input samples and P outputs per unit,
//     y[n * P + p] = sum_{j < W} x[n * S + first[p] + j] * w[p][j]        x = 0 outside [0, n_in)
// in ONE launch where the reference loops over the P phases (conv1d, conv_transpose1d against an identity, two pads and a += over the
// whole output per phase: ~800 launches at 44.1 -> 16 kHz).
//   resample_kernel<MIX>   a workgroup of 256 threads owns one output row (MIX: one channel pair) and a tile of G consecutive units =
//                          G * P outputs at a time; the grid is capped (three workgroups of up to 64 KB LDS per CU on 256 CUs) and a
//                          workgroup goes on to the tile gridDim.x further, so the table is staged once per workgroup, not per tile.
//                          It stages the table -- first[] clamped to [-W, S], w with the odd row pitch W | 1 so that the
//                          lanes' consecutive phases fall into different banks -- and the input span
//                          [n0 S + min first, (n0 + g - 1) S + max first + W) into LDS, then every thread takes the output indices
//                          tid, tid + 256, ... of the tile (coalesced stores) and forms its fp32 sum over the W taps in ascending order.
//                          MIX: both channels against one read of each weight, out = 0.5 * (y0 + y1).  Then the span of its next tile.
// Staging: 16-byte loads typed with 4-byte alignment (all global_load_dwordx4 asks for) where the four samples lie inside [0, n_in),
// element by element with zeros where they do not: no address outside a row's n_in samples is touched.  Indices into the rows are 64-bit.
// G: the smallest with G * P >= SVT_RESAMPLE_TILE_OUTPUTS, lowered until table + span fit SVT_RESAMPLE_LDS_BYTES (the span is sized on the
// host for the widest first[] range the clamp allows, S + W, since the table is not read there; the kernel stages the range it finds).
#include "device_util.h"

namespace svt {
namespace {
constexpr int64_t kResampleLdsBytes = 65536;   // SVT_RESAMPLE_LDS_BYTES
constexpr int kResampleTileOutputs = 1024;     // SVT_RESAMPLE_TILE_OUTPUTS
constexpr int64_t kResampleMaxBlocks = 768;    // SVT_RESAMPLE_MAX_WORKGROUPS: the grid's cap; beyond it the workgroups take further tiles
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));   // 16 bytes at a 4-byte-aligned address

// floats of one channel's span buffer for G units: (G - 1) S + (max first - min first <= S + W) + W, up to a multiple of 4
inline int64_t span_floats(int64_t G, int W, int S) { return ((G - 1) * S + S + 2 * (int64_t)W + 3) & ~(int64_t)3; }
// span buffers | weights (P rows of W | 1) | first (P) | the range of first (2)
inline int64_t lds_bytes(int64_t G, int P, int W, int S, bool mix) {
  return 4 * ((mix ? 2 : 1) * span_floats(G, W, S) + (int64_t)P * (W | 1) + P + 2);
}

template <bool MIX>
__global__ __launch_bounds__(256) void resample_kernel(const float* __restrict__ in, int64_t n_in, int64_t ld_in, const float* __restrict__ w,
                                                       const int32_t* __restrict__ first, int P, int W, int S, int G, int span_cap,
                                                       int64_t tiles, int64_t jobs, float* __restrict__ out, int64_t n_out,
                                                       int64_t ld_out) {
  extern __shared__ __align__(16) float lds[];
  constexpr int C = MIX ? 2 : 1;
  const int Wp = W | 1, tid = threadIdx.x;
  float* xs = lds;
  float* ws = lds + C * span_cap;
  int* fs = (int*)(ws + P * Wp);
  int* range = fs + P;

  if (tid == 0) { range[0] = S; range[1] = -W; }
  __syncthreads();
  int lo = S, hi = -W;
  for (int p = tid; p < P; p += 256) {
    const int f = max(-W, min(S, first[p]));
    fs[p] = f;
    lo = min(lo, f);
    hi = max(hi, f);
  }
  if (tid < P) { atomicMin(&range[0], lo); atomicMax(&range[1], hi); }   // LDS atomics
  for (int i = tid; i < P * W; i += 256) {
    const int p = i / W;
    ws[p * Wp + (i - p * W)] = w[i];
  }
  __syncthreads();
  const int fmin = range[0], fmax = range[1];
  const int64_t units = (n_out + P - 1) / P;

  // job = (row, tile), the tiles of a row next to each other; a workgroup takes the jobs blockIdx.x, blockIdx.x + gridDim.x, ...
  for (int64_t job = blockIdx.x; job < jobs; job += gridDim.x) {
    const int64_t row = job / tiles, tile = job - row * tiles;
    const int64_t n0 = tile * G;
    const int g = (int)min((int64_t)G, units - n0);                 // units of this tile (the last tile may hold fewer)
    const int span = (g - 1) * S + (fmax - fmin) + W;               // <= span_cap by the clamp
    const int64_t x0 = n0 * S + fmin;                               // the span's first sample, possibly in front of the row
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float* x = in + (row * C + c) * ld_in;
      float* xd = xs + c * span_cap;
      for (int q = tid * 4; q < span; q += 1024) {
        const int64_t s0 = x0 + q;
        if (s0 >= 0 && s0 + 4 <= n_in) {
          const f32x4u v = *(const f32x4u*)(x + s0);
          *(f32x4*)(xd + q) = f32x4{v.x, v.y, v.z, v.w};
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int64_t s = s0 + e;
            xd[q + e] = (s >= 0 && s < n_in) ? x[s] : 0.f;
          }
        }
      }
    }
    __syncthreads();

    const int n_loc = g * P;
    const int64_t o0 = n0 * P;
    float* y = out + row * ld_out;
    for (int l = tid; l < n_loc; l += 256) {
      const int64_t o = o0 + l;
      if (o >= n_out) break;
      const int u = l / P, p = l - u * P;
      const float* xp = xs + u * S + (fs[p] - fmin);
      const float* wp = ws + p * Wp;
      float a0 = 0.f, a1 = 0.f;
      for (int j = 0; j < W; ++j) {
        const float c = wp[j];
        a0 = fmaf(xp[j], c, a0);
        if (MIX) a1 = fmaf(xp[span_cap + j], c, a1);
      }
      y[o] = MIX ? 0.5f * (a0 + a1) : a0;
    }
    __syncthreads();   // the next job overwrites the span
  }
}
}  // namespace

int resample_units_per_tile(int P, int W, int S, bool downmix) {
  if (P < 1 || W < 1 || S < 1) return 0;
  int64_t G = (kResampleTileOutputs + P - 1) / P;
  while (G >= 1 && lds_bytes(G, P, W, S, downmix) > kResampleLdsBytes) --G;
  return (int)G;
}

int launch_resample(const float* in, int rows_out, int64_t n_in, int64_t ld_in, const float* w, const int32_t* first, int P, int W, int S,
                    float* out, int64_t n_out, int64_t ld_out, bool downmix, hipStream_t s) {
  const int G = resample_units_per_tile(P, W, S, downmix);
  if (G < 1) { set_error("resample: the table does not fit the LDS cap"); return -1; }
  if (rows_out < 1 || n_in < 1 || n_out < 1 || ld_in < n_in || ld_out < n_out) { set_error("resample: bad geometry"); return -1; }
  if (!in || !w || !first || !out || !aligned(3, in, w, first, out)) { set_error("resample: null or misaligned pointer"); return -1; }
  const int64_t units = (n_out + P - 1) / P, tiles = (units + G - 1) / G;
  const int64_t jobs = tiles * rows_out;
  const unsigned grid = (unsigned)std::min<int64_t>(jobs, kResampleMaxBlocks);
  const int span_cap = (int)span_floats(G, W, S);
  const size_t bytes = (size_t)lds_bytes(G, P, W, S, downmix);
  if (downmix)
    hipLaunchKernelGGL((resample_kernel<true>), dim3(grid), dim3(256), bytes, s, in, n_in, ld_in, w, first, P, W, S, G, span_cap, tiles, jobs,
                       out, n_out, ld_out);
  else
    hipLaunchKernelGGL((resample_kernel<false>), dim3(grid), dim3(256), bytes, s, in, n_in, ld_in, w, first, P, W, S, G, span_cap, tiles, jobs,
                       out, n_out, ld_out);
  SVT_LAUNCH_CHECK();
  return 0;
}

}  // namespace svt
