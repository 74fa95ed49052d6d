// Frequency and chunk dropping of a waveform batch (svt_drop_freq_chunk; speechbrain/processing/speech_augmentation.py:876-1140, the
// DropFreq and DropChunk steps of speechbrain/lobes/augment.py TimeDomainSpecAugment): with h = taps / 2,
//     y[r][t] = 0                                              if start <= t < end for any chunk of row r
//             = sum_{k < taps} f[k] * x[r][t + k - h]           otherwise,   x = 0 outside [0, n)
// in ONE launch where the reference runs a conv1d (with a transpose, a clone and a squeeze around it) and then one slice assignment per
// dropped chunk from a Python loop over the batch.
//   drop_kernel<FIR>   a workgroup of 256 threads takes one (row, tile) job of kDropTile = 1024 consecutive outputs at a time, the tiles
//                      of a row next to each other; up to kDropMaxBlocks jobs it is one job per workgroup (the dispatcher balances
//                      them), beyond that the grid is cut so that every workgroup takes the same number of jobs, gridDim.x apart.  Per job:
//                      1. the row's chunk table, 256 pairs at a time, clipped to the tile ([lo, hi) in 0 .. tile length) into LDS; every
//                         lane ORs the chunks that touch its four outputs into a 4-bit mask.  A tile that lies wholly inside ONE chunk
//                         is written as zeros at once: no read of x.
//                      2. FIR: the span [t0 - h, t0 + len + h) into LDS -- 16-byte loads typed with 4-byte alignment where the four
//                         samples lie inside [0, n), element by element with zeros where they do not, so no address outside the row's n
//                         samples is touched.  A lane owns the outputs 4 l .. 4 l + 3 and walks the taps four at a time: one
//                         ds_read_b128 of the next four samples (16-byte lane pitch: conflict-free) against 16 fused multiply-adds;
//                         the taps are read at wave-uniform addresses.  Each output is one fma chain over the taps in ascending order.
//                         !FIR: the four samples straight from global memory, no LDS, no halo.
//                      3. masked outputs are REPLACED by 0.0f (not multiplied: a NaN the filter produced there does not survive), 16-byte
//                         stores where the four outputs lie inside the row, element by element at the row's end.
// Indices into the rows are 64-bit; tile-local ones 32-bit.
#include "device_util.h"

namespace svt {
namespace {
constexpr int kDropTile = 1024;            // SVT_DROP_TILE_OUTPUTS: 256 lanes x 4 outputs
constexpr int kDropMaxTaps = 255;          // SVT_DROP_MAX_TAPS
constexpr int64_t kDropMaxBlocks = 8192;   // SVT_DROP_MAX_WORKGROUPS: four rounds of the 8 workgroups (57 VGPRs, ~7 KB LDS) a CU holds
constexpr int kDropSpan = kDropTile + kDropMaxTaps + 9;   // the staged span and the reads of the last tap group behind it (never used)
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));   // 16 bytes at a 4-byte-aligned address

template <bool FIR>
__global__ __launch_bounds__(256, 8) void drop_kernel(const float* __restrict__ in, int64_t n, int64_t ld_in, const float* __restrict__ filter,
                                                   int taps, const int64_t* __restrict__ chunks, int max_chunks, int64_t tiles,
                                                   int64_t jobs, float* __restrict__ out, int64_t ld_out) {
  __shared__ __align__(16) float xs[FIR ? kDropSpan : 4];
  __shared__ int2 cs[256];
  const int tid = threadIdx.x, half = taps >> 1, l0 = tid * 4;

  for (int64_t job = blockIdx.x; job < jobs; job += gridDim.x) {
    const int64_t row = job / tiles, t0 = (job - row * tiles) * kDropTile;
    const int len = (int)min((int64_t)kDropTile, n - t0);           // outputs of this tile
    const float* x = in + row * ld_in;
    float* y = out + row * ld_out;

    // 1. the chunks of the row against this tile
    int mask = 0, covered = 0;
    for (int c0 = 0; c0 < max_chunks; c0 += 256) {
      const int cn = min(256, max_chunks - c0);
      int full = 0;
      if (tid < cn) {
        const int64_t* c = chunks + ((int64_t)row * max_chunks + c0 + tid) * 2;
        const int64_t s = max((int64_t)0, min(n, c[0])), e = max((int64_t)0, min(n, c[1]));   // into the row first: no overflow below
        const int lo = (int)max((int64_t)0, min((int64_t)len, s - t0));
        const int hi = (int)max((int64_t)0, min((int64_t)len, e - t0));
        cs[tid] = int2{lo, hi};
        full = lo == 0 && hi == len;
      }
      covered |= __syncthreads_or(full);                            // the barrier that publishes cs
      if (!covered)
        for (int c = 0; c < cn; ++c) {
          const int2 v = cs[c];                                     // a broadcast read
          if (v.x >= v.y) continue;                                 // empty, or outside this tile: uniform
#pragma unroll
          for (int j = 0; j < 4; ++j) mask |= (l0 + j >= v.x && l0 + j < v.y) ? 1 << j : 0;
        }
      __syncthreads();                                              // the next batch overwrites cs
    }
    if (covered) mask = 15;

    // 2. the four outputs of this lane
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (FIR) {
      if (!covered) {
        const int span = len + taps - 1;
        const int64_t x0 = t0 - half;                               // the span's first sample, possibly in front of the row
        for (int q = l0; q < span; q += 1024) {
          const int64_t s0 = x0 + q;
          if (s0 >= 0 && s0 + 4 <= n) {
            const f32x4u v = *(const f32x4u*)(x + s0);
            *(f32x4*)(xs + q) = f32x4{v.x, v.y, v.z, v.w};
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int64_t s = s0 + e;
              xs[q + e] = (s >= 0 && s < n) ? x[s] : 0.f;
            }
          }
        }
        __syncthreads();
        if (l0 < len) {
          const float* xp = xs + l0;
          f32x4 cur = *(const f32x4*)xp;
          int k = 0;
          for (; k + 4 <= taps; k += 4) {
            const f32x4 nxt = *(const f32x4*)(xp + k + 4);
            const float f0 = filter[k], f1 = filter[k + 1], f2 = filter[k + 2], f3 = filter[k + 3];
            a0 = fmaf(f0, cur.x, a0); a1 = fmaf(f0, cur.y, a1); a2 = fmaf(f0, cur.z, a2); a3 = fmaf(f0, cur.w, a3);
            a0 = fmaf(f1, cur.y, a0); a1 = fmaf(f1, cur.z, a1); a2 = fmaf(f1, cur.w, a2); a3 = fmaf(f1, nxt.x, a3);
            a0 = fmaf(f2, cur.z, a0); a1 = fmaf(f2, cur.w, a1); a2 = fmaf(f2, nxt.x, a2); a3 = fmaf(f2, nxt.y, a3);
            a0 = fmaf(f3, cur.w, a0); a1 = fmaf(f3, nxt.x, a1); a2 = fmaf(f3, nxt.y, a2); a3 = fmaf(f3, nxt.z, a3);
            cur = nxt;
          }
          const int rest = taps - k;                                // 1 .. 3: taps is odd
          const f32x4 nxt = *(const f32x4*)(xp + k + 4);
          const float w[7] = {cur.x, cur.y, cur.z, cur.w, nxt.x, nxt.y, nxt.z};
#pragma unroll
          for (int i = 0; i < 3; ++i)
            if (i < rest) {
              const float f = filter[k + i];
              a0 = fmaf(f, w[i], a0); a1 = fmaf(f, w[i + 1], a1); a2 = fmaf(f, w[i + 2], a2); a3 = fmaf(f, w[i + 3], a3);
            }
        }
        __syncthreads();                                            // the next job overwrites the span
      }
    } else if (mask != 15 && l0 < len) {
      const int64_t s0 = t0 + l0;
      if (l0 + 4 <= len) {
        const f32x4u v = *(const f32x4u*)(x + s0);
        a0 = v.x; a1 = v.y; a2 = v.z; a3 = v.w;
      } else {
        a0 = x[s0];
        if (l0 + 1 < len) a1 = x[s0 + 1];
        if (l0 + 2 < len) a2 = x[s0 + 2];
      }
    }

    // 3. dropped elements are zeros, whatever the sum gave
    if (l0 < len) {
      f32x4u r;
      r.x = (mask & 1) ? 0.f : a0; r.y = (mask & 2) ? 0.f : a1; r.z = (mask & 4) ? 0.f : a2; r.w = (mask & 8) ? 0.f : a3;
      float* yp = y + t0 + l0;
      if (l0 + 4 <= len) {
        *(f32x4u*)yp = r;
      } else {
        yp[0] = r.x;
        if (l0 + 1 < len) yp[1] = r.y;
        if (l0 + 2 < len) yp[2] = r.z;
      }
    }
  }
}
}  // namespace

int launch_drop_freq_chunk(const float* in, int rows, int64_t n, int64_t ld_in, const float* filter, int taps, const int64_t* chunks,
                           int max_chunks, float* out, int64_t ld_out, hipStream_t s) {
  if (rows < 1 || n < 1 || ld_in < n || ld_out < n || max_chunks < 0) { set_error("drop_freq_chunk: bad geometry"); return -1; }
  if ((filter != nullptr) != (taps != 0) || (chunks != nullptr) != (max_chunks != 0)) { set_error("drop_freq_chunk: a table without its count"); return -1; }
  if (taps && (!(taps & 1) || taps < 1 || taps > kDropMaxTaps)) { set_error("drop_freq_chunk: taps"); return -1; }
  if (!in || !out || !aligned(3, in, filter, out) || !aligned(7, chunks)) { set_error("drop_freq_chunk: null or misaligned pointer"); return -1; }
  const int64_t tiles = (n + kDropTile - 1) / kDropTile;
  const int64_t jobs = tiles * rows;
  const int64_t trips = (jobs + kDropMaxBlocks - 1) / kDropMaxBlocks;   // jobs per workgroup
  const unsigned grid = (unsigned)((jobs + trips - 1) / trips);
  if (taps)
    hipLaunchKernelGGL((drop_kernel<true>), dim3(grid), dim3(256), 0, s, in, n, ld_in, filter, taps, chunks, max_chunks, tiles, jobs, out, ld_out);
  else
    hipLaunchKernelGGL((drop_kernel<false>), dim3(grid), dim3(256), 0, s, in, n, ld_in, filter, taps, chunks, max_chunks, tiles, jobs, out, ld_out);
  SVT_LAUNCH_CHECK();
  return 0;
}

}  // namespace svt
