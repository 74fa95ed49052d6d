// bf16 dense contraction for gfx950 on the LDS-DMA ring (gemm_ring.h), LOCKSTEP PERSISTENT form: the tile, wave layout and contract of
// gemm_pp8_kernel (gemm_pp8.hip) without batches, generalised addressing or residual.  One workgroup per CU walks a list of output tiles; the
// (tile, k-slab) pairs form ONE stream for the LDS-DMA ring, so the first slabs of tile i+1 are already
// in flight while tile i runs its epilogue, and the epilogue's global stores (fire-and-forget) drain
// while the next tile multiplies.  Without this every CU of a single-round launch reaches its epilogue
// at the same moment and the 50-100 MB store burst is pure serial time (measured: 40 % of out_proj).
// The epilogue uses buffer stores with hardware bounds checking (rows >= M are dropped by the memory
// pipeline, never by a branch), so the number of VMEM operations a wave has in flight after an epilogue
// is a compile-time constant and the counted s_waitcnt vmcnt of the ring stays exact.
#include "gemm_ring.h"

namespace svt {
namespace {

template <int BM>
__global__ __launch_bounds__(512) void gemm_pers_kernel(GemmArgs p, int tiles_n, int ntiles) {
  constexpr int BN = 256, BK = 64, NSLOT = 5;
  constexpr int MB = BM / 32;
  constexpr int GA = BM / 64;
  constexpr int GW = BN / 64;
  constexpr int SLOT = 2048;
  extern __shared__ __attribute__((aligned(16))) uint4 lds[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int nblk = gridDim.x, b = blockIdx.x;
  const int lbase = xcd_first_tile(b, nblk);
  int my_tiles = 0;
  while (my_tiles * nblk + lbase < ntiles) ++my_tiles;
  if (my_tiles == 0) return;

  const bf16_t* A = (const bf16_t*)p.A;
  const bf16_t* W = (const bf16_t*)p.W;
  const int r8 = lane >> 3, ch = (lane & 7) ^ (lane >> 3);

  const bf16_t* asrc[GA];
  const bf16_t* wsrc[GW];
  const bf16_t* asrc2[GA];
  const bf16_t* wsrc2[GW];
  auto setup = [&](int logical, const bf16_t* (&as)[GA], const bf16_t* (&ws)[GW]) {
    const int tile_n = logical % tiles_n, tile_m = logical / tiles_n;
    const int m0 = tile_m * BM, n0 = tile_n * BN;
#pragma unroll
    for (int i = 0; i < GA; ++i) {
      int m = m0 + (wave + 8 * i) * 8 + r8;
      if (m > p.M - 1) m = p.M - 1;
      as[i] = A + (long)(m / p.a_rpb) * p.a_bstride + (long)(m % p.a_rpb) * p.a_rstride + ch * 8;
    }
#pragma unroll
    for (int i = 0; i < GW; ++i) {
      const int rho = (wave + 8 * i) * 8 + r8;
      const int i16 = rho & 15;
      int n = n0 + (rho >> 6) * 64 + (i16 >> 2) * 16 + ((rho >> 4) & 3) * 4 + (i16 & 3);
      if (n > p.N - 1) n = p.N - 1;
      ws[i] = W + (long)n * p.ldw + ch * 8;
    }
  };
  auto issue_a = [&](const bf16_t* const (&as)[GA], int kt, int slot) {
#pragma unroll
    for (int i = 0; i < GA; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)(as[i] + kt * BK), (lptr_t)(lds + slot * SLOT + (wave + 8 * i) * 64), 16, 0, 0);
  };
  auto issue_w = [&](const bf16_t* const (&ws)[GW], int kt, int slot) {
#pragma unroll
    for (int i = 0; i < GW; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)(ws[i] + kt * BK), (lptr_t)(lds + slot * SLOT + (wave + 8 * i) * 64), 16, 0, 0);
  };
  // one DMA instruction of a unit (the steady-state loop spreads a unit's instructions between MFMA groups: a burst
  // of 8 per wave right after the barrier queues 64 requests on the CU's texture addresser in front of every wave)
  auto issue_a1 = [&](const bf16_t* const (&as)[GA], int i, int kt, int slot) {
    __builtin_amdgcn_global_load_lds((gptr_t)(as[i] + kt * BK), (lptr_t)(lds + slot * SLOT + (wave + 8 * i) * 64), 16, 0, 0);
  };
  auto issue_w1 = [&](const bf16_t* const (&ws)[GW], int i, int kt, int slot) {
    __builtin_amdgcn_global_load_lds((gptr_t)(ws[i] + kt * BK), (lptr_t)(lds + slot * SLOT + (wave + 8 * i) * 64), 16, 0, 0);
  };

  f32x4 acc[4][MB];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < MB; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int cq = lane >> 4, r16 = lane & 15, rr8 = r16 & 7;
  const int frag0 = (r16 >> 3) * 64 + rr8 * 8 + (cq ^ rr8);
  const int frag1 = (r16 >> 3) * 64 + rr8 * 8 + ((4 + cq) ^ rr8);
  const int xoff = (wm * (MB * 2)) * 64;
  const int woff = (wn * 8) * 64;

  const bool tr = p.trace != nullptr;
  long long t_begin = 0, t_first = 0, t_main = 0, t_epi = 0, t_mark = 0;
  if (tr) t_begin = wall_clock64();
  const int nk = p.K / BK;            // >= 2 (checked by the launcher)
  const int G = my_tiles * nk;        // slabs in this workgroup's stream
  int ti = 0;                         // index of the tile being multiplied
  setup(lbase, asrc, wsrc);
  if (my_tiles > 1) setup(nblk + lbase, asrc2, wsrc2);
  issue_a(asrc, 0, 0);
  issue_w(wsrc, 0, 1);
  issue_a(asrc, 1, 2);
  int sa = 0, sw = 1, kt = 0;
  bool after_epilogue = false;
  // static priority for the younger half of the workgroup (waves 4-7 share SIMDs with 0-3 and lose issue arbitration
  // by age: measured 39 % vs 7 % of the time parked at the barrier)
  if (wave >= 4 && p.dbg == 8) __builtin_amdgcn_s_setprio(1);
  for (int g = 0; g < G; ++g) {
    // retire slab g: allowed in flight = A unit of slab g+1 (+ the previous tile's epilogue stores, which are younger)
    if (g + 1 < G) {
      if (!after_epilogue) wait_vm<GA>();
      else if (p.out_f32) wait_vm<GA + MB * 4>();
      else wait_vm<GA + MB * 2>();
    } else {
      wait_vm<0>();
    }
    after_epilogue = false;
    __builtin_amdgcn_s_barrier();
    if (tr && g == 0) t_first = t_mark = wall_clock64();
    const uint4* xa = lds + sa * SLOT + xoff;
    const uint4* wa = lds + sw * SLOT + woff;
    const bool have_w = g + 1 < G, have_a = g + 2 < G;
    const bool w_cur = kt + 1 < nk, a_cur = kt + 2 < nk;
    const int wslot = (2 * g + 3) % NSLOT, aslot = (2 * g + 4) % NSLOT;
    const int wkt = w_cur ? kt + 1 : 0, akt = a_cur ? kt + 2 : kt + 2 - nk;
    {
      // Quarter-phase software pipeline: the slab is multiplied in four groups of 4 x MB/2 MFMAs ((k-step, M half));
      // the fragments of group q+1 are requested BEFORE the MFMAs of group q (two register sets, static indices), so
      // only the first group's LDS latency is exposed after the barrier.  The ring's DMA instructions are spread two
      // per group.
      constexpr int HM = MB / 2;
      bf16x8 wfr[2][4], xfr[2][HM];
      auto rd_w = [&](int ks, bf16x8 (&w)[4]) {
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) w[nb] = __builtin_bit_cast(bf16x8, wa[nb * 128 + (ks ? frag1 : frag0)]);
      };
      auto rd_x = [&](int ks, int half, bf16x8 (&x)[HM]) {
#pragma unroll
        for (int j = 0; j < HM; ++j) x[j] = __builtin_bit_cast(bf16x8, xa[(half * HM + j) * 128 + (ks ? frag1 : frag0)]);
      };
      rd_w(0, wfr[0]);
      rd_x(0, 0, xfr[0]);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int ks = q >> 1, half = q & 1;
        // DMA: W unit during k-step 0, A unit during k-step 1
        if (ks == 0) {
          if (have_w) {
#pragma unroll
            for (int i2 = half * 2; i2 < half * 2 + 2; ++i2) {
              if (w_cur) issue_w1(wsrc, i2, wkt, wslot); else issue_w1(wsrc2, i2, wkt, wslot);
            }
          }
        } else {
          if (have_a) {
#pragma unroll
            for (int i2 = half * ((GA + 1) / 2); i2 < (half ? GA : (GA + 1) / 2); ++i2) {
              if (a_cur) issue_a1(asrc, i2, akt, aslot); else issue_a1(asrc2, i2, akt, aslot);
            }
          }
        }
        // request the next group's fragments
        if (q == 0) rd_x(0, 1, xfr[1]);
        if (q == 1) { rd_w(1, wfr[1]); rd_x(1, 0, xfr[0]); }
        if (q == 2) rd_x(1, 1, xfr[1]);
#pragma unroll
        for (int j = 0; j < HM; ++j)
#pragma unroll
          for (int nb = 0; nb < 4; ++nb)
            acc[nb][half * HM + j] = SVT_MFMA_16x16x32(wfr[ks][nb], xfr[half][j], acc[nb][half * HM + j]);
      }
    }
    sa = (sa + 2) % NSLOT;
    sw = (sw + 2) % NSLOT;
    if (++kt == nk) {
      // ---- epilogue of tile ti (registers -> global, bounds-checked buffer stores) ----
      kt = 0;
      if (tr) { const long long t = wall_clock64(); t_main += t - t_mark; t_mark = t; }
      const int logical = ti * nblk + lbase;
      const int tile_n = logical % tiles_n, tile_m = logical / tiles_n;
      const int m0 = tile_m * BM, n0 = tile_n * BN;
      const int esz = p.out_f32 ? 4 : 2;
      // descriptor over the rows [m0, M) of C (and of the residual): a row >= M lands beyond num_records
      const long rows_left = (long)p.M - m0;
      const unsigned long nbytes = (unsigned long)rows_left * p.ldc * esz;
      const unsigned nrec = nbytes > 0xFFFFFFF0ul ? 0xFFFFFFF0u : (unsigned)nbytes;
      char* cbase = (char*)p.C + (long)m0 * p.ldc * esz;
      const auto crsrc = __builtin_amdgcn_make_buffer_rsrc(cbase, 0, nrec, 0x00020000);
      const int nbase = n0 + wn * 64 + (lane >> 4) * 16;
      // one branch around the four bias loads (hipcc waits vmcnt(0) at the first use of an ordinary load while LDS-DMA is in
      // flight; a branch per load made that four serial waits per tile -- measured: no difference, the waits overlap the
      // epilogue's own latency; kept because it is the simpler code)
      float bv[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) bv[j] = 0.f;
      if (p.bias) {
        const float4* bp = (const float4*)(p.bias + nbase);
        const float4 b0 = bp[0], b1 = bp[1], b2 = bp[2], b3 = bp[3];
        bv[0] = b0.x; bv[1] = b0.y; bv[2] = b0.z; bv[3] = b0.w; bv[4] = b1.x; bv[5] = b1.y; bv[6] = b1.z; bv[7] = b1.w;
        bv[8] = b2.x; bv[9] = b2.y; bv[10] = b2.z; bv[11] = b2.w; bv[12] = b3.x; bv[13] = b3.y; bv[14] = b3.z; bv[15] = b3.w;
      }
      if (p.out_f32) {
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
          const int ml = wm * (BM / 2) + mb * 16 + (lane & 15);
          const unsigned off = (unsigned)(((long)ml * p.ldc + nbase) * 4);
#pragma unroll
          for (int nb = 0; nb < 4; ++nb) {
            f32x4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = acc[nb][mb][r] * p.alpha + bv[nb * 4 + r];
            // activation selected once per block of four (wave-uniform), not per element
            if (p.act == ACT_GELU) {
#pragma unroll
              for (int r = 0; r < 4; ++r) v[r] = gelu_erf(v[r]);
            } else if (p.act == ACT_RELU) {
#pragma unroll
              for (int r = 0; r < 4; ++r) v[r] = v[r] > 0.f ? v[r] : 0.f;
            }
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, v), crsrc, off + nb * 16, 0, 0);
          }
        }
      } else {
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
          const int ml = wm * (BM / 2) + mb * 16 + (lane & 15);
          const unsigned off = (unsigned)(((long)ml * p.ldc + nbase) * 2);
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            bf16x8 o;
            if (p.act == ACT_GELU) {
              f32x2_t g[4];
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                const int n0r = h * 8 + 2 * j, n1r = n0r + 1;
                g[j] = f32x2_t{acc[n0r >> 2][mb][n0r & 3] * p.alpha + bv[n0r], acc[n1r >> 2][mb][n1r & 3] * p.alpha + bv[n1r]};
              }
              gelu_bf16x2_x4(g);
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                o[2 * j] = (bf16_t)g[j].x;
                o[2 * j + 1] = (bf16_t)g[j].y;
              }
            } else if (p.act == ACT_RELU) {
#pragma unroll
              for (int j = 0; j < 8; ++j) {
                const int nbr = h * 8 + j;
                const float x = acc[nbr >> 2][mb][nbr & 3] * p.alpha + bv[nbr];
                o[j] = (bf16_t)(x > 0.f ? x : 0.f);
              }
            } else {
#pragma unroll
              for (int j = 0; j < 8; ++j) {
                const int nbr = h * 8 + j;
                o[j] = (bf16_t)(acc[nbr >> 2][mb][nbr & 3] * p.alpha + bv[nbr]);
              }
            }
            if (p.dbg != 10) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, o), crsrc, off + h * 16, 0, 0);
            else asm volatile("" ::"v"(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, o)));
          }
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < MB; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (tr) { const long long t = wall_clock64(); t_epi += t - t_mark; t_mark = t; }
      after_epilogue = true;
      ++ti;
      // rotate the pointer sets: next tile becomes current, precompute the one after
#pragma unroll
      for (int i = 0; i < GA; ++i) asrc[i] = asrc2[i];
#pragma unroll
      for (int i = 0; i < GW; ++i) wsrc[i] = wsrc2[i];
      if (ti + 1 < my_tiles && p.dbg != 11) setup((ti + 1) * nblk + lbase, asrc2, wsrc2);
    }
  }
  if (tr && lane == 0 && (wave & 3) == 0) {
    wait_vm<0>();
    long long* o = p.trace + ((long)blockIdx.x * 2 + (wave >> 2)) * 8;
    o[0] = t_begin; o[1] = t_first; o[2] = t_main; o[3] = t_epi; o[4] = wall_clock64(); o[5] = my_tiles;
  }
}

template <int BM>
int launch_pers(const GemmArgs& a, hipStream_t s) {
  const int tiles_m = (a.M + BM - 1) / BM, tiles_n = (a.N + 255) / 256;
  const int ntiles = tiles_m * tiles_n;
  const size_t lds_bytes = 5 * 32768;
  if (int r_ = ensure_dyn_lds((const void*)gemm_pers_kernel<BM>, (int)lds_bytes)) return r_;
  // (one workgroup per CU: svt_debug_set key 37 does not apply to this kernel)
  hipLaunchKernelGGL((gemm_pers_kernel<BM>), dim3(persistent_blocks(ntiles, 256)), dim3(512), lds_bytes, s, a, tiles_n, ntiles);
  SVT_LAUNCH_CHECK();
  return 0;
}
}  // namespace

// bm: 256 / 192 / 128, anything else 64 (gemm_dispatch.hip, height_of_4, names the height that runs for svt_debug_set key 39: keep them in step)
int launch_gemm_pers(const GemmArgs& a, int bm, hipStream_t s) {
  if (bm == 256) return launch_pers<256>(a, s);
  if (bm == 192) return launch_pers<192>(a, s);
  if (bm == 128) return launch_pers<128>(a, s);
  return launch_pers<64>(a, s);
}

}  // namespace svt
