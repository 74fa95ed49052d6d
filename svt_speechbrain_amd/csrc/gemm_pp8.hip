// bf16 dense contraction for gfx950 on the LDS-DMA ring (gemm_ring.h), ONE TILE PER WORKGROUP: BM x 256 output tile per 512-thread
// workgroup (8 waves as 2(M) x 4(N), wave tile BM/2 x 64, v_mfma_f32_16x16x32_bf16), K in 64-element slabs, the LDS-transposed coalesced
// epilogue of gemm_epilogue.h.  Same contract as gemm.hip (GemmArgs: overlapping A rows for implicit conv, bias / activation epilogue).
// The dispatcher (gemm_dispatch.hip) picks BM in {128,192,256} and, per problem, this kernel or the persistent gemm_pers_kernel.
//   * gemm_pp8_kernel<BM, GEN = true, NBW> is the same pipeline with generalised addressing (GemmArgs::gen): A rows at
//     m*stride + floor(m/d1)*e1 + floor(m/d2)*e2, K made of equal runs a fixed distance apart, C rows likewise -- the
//     3x3 / 1x1 convolutions of the lip front-end's ResNet over zero-haloed channels-last tensors -- with bias +
//     residual (operand type) + per-column PReLU in the epilogue; NBW = 2 gives a 128-column tile for 128-channel layers.
#include "gemm_epilogue.h"

namespace svt {
namespace {

// generalised variant (GemmArgs::gen): rows land at c_base + m*ldc + (m/c_d1)*c_e1 + (m/c_d2)*c_e2 (interior of a
// zero-haloed channels-last tensor), optional residual in the operand type added BEFORE the activation, per-column
// PReLU slope.  bf16 output only.  NBW = 16-column MFMA blocks per wave (tile width 64 * NBW).
template <int MB, int BM, int NBW, int I>
__device__ __forceinline__ void epilogue_block_gen(const GemmArgs& p, f32x4 (&acc)[NBW][MB], float* patch, int lane, int wm,
                                                   int wn, int m0, int n0, const float (&bb)[8], const float (&ss)[8]) {
  constexpr int WC = 16 * NBW;       // columns per wave
  constexpr int PITCH = WC + 4;      // floats
  constexpr int LPR = 2 * NBW;       // lanes per row on the read-back side (8 columns each)
  constexpr int RPP = 64 / LPR;      // rows per pass
  constexpr int PASSES = RPP >= 16 ? 1 : 16 / RPP;
  const int m16 = lane & 15, q = lane >> 4;
#pragma unroll
  for (int nb = 0; nb < NBW; ++nb) {
    f32x4 v = acc[nb][I];
    v[0] *= p.alpha; v[1] *= p.alpha; v[2] *= p.alpha; v[3] *= p.alpha;
    *(f32x4*)(patch + m16 * PITCH + q * (4 * NBW) + nb * 4) = v;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const int mbase = m0 + wm * (BM / 2) + I * 16;
  const int c8 = (lane % LPR) * 8;
  const int n = n0 + wn * WC + c8;
#pragma unroll
  for (int pass = 0; pass < PASSES; ++pass) {
    const int r = pass * RPP + lane / LPR;
    const int m = mbase + r;
    if (r < 16 && m < p.M && n < p.N) {
      const float4 v0 = *(const float4*)(patch + r * PITCH + c8), v1 = *(const float4*)(patch + r * PITCH + c8 + 4);
      float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
      const long idx = p.c_base + (long)m * p.ldc + (long)(m / p.c_d1) * p.c_e1 + (long)(m / p.c_d2) * p.c_e2 + n +
                       (p.c_nsplit && n >= p.c_nsplit ? p.c_nstride - p.c_nsplit : 0);
      float rr[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) rr[j] = 0.f;
      if (p.resid) {
        const bf16x8 r8 = *(const bf16x8*)((const bf16_t*)p.resid + idx);
#pragma unroll
        for (int j = 0; j < 8; ++j) rr[j] = (float)r8[j];
      }
      bf16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float x = v[j] + bb[j];
        if (p.resid_first) x += rr[j];
        if (p.act == ACT_PRELU) x = x > 0.f ? x : x * ss[j];
        else x = apply_act(x, p.act);
        if (!p.resid_first) x += rr[j];
        o[j] = (bf16_t)x;
      }
      *(bf16x8*)((bf16_t*)p.C + idx) = o;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

template <int MB, int BM, int NBW, int... I>
__device__ __forceinline__ void epilogue_seq_gen(std::integer_sequence<int, I...>, const GemmArgs& p, f32x4 (&acc)[NBW][MB],
                                                 float* patch, int lane, int wm, int wn, int m0, int n0, const float* bias) {
  // bias / slope of the lane's 8 columns ONCE per tile: inside the per-block function they sit behind its wave fences, where the
  // compiler re-issues the four loads for every 16-row block and every block waits out their round trip
  const int n = n0 + wn * (16 * NBW) + (lane % (2 * NBW)) * 8;
  float bb[8], ss[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { bb[j] = 0.f; ss[j] = 0.f; }
  if (n < p.N) {
    if (bias) {
      const float4 b0 = *(const float4*)(bias + n), b1 = *(const float4*)(bias + n + 4);
      bb[0] = b0.x; bb[1] = b0.y; bb[2] = b0.z; bb[3] = b0.w; bb[4] = b1.x; bb[5] = b1.y; bb[6] = b1.z; bb[7] = b1.w;
    }
    if (p.slope) {
      const float4 s0 = *(const float4*)(p.slope + n), s1 = *(const float4*)(p.slope + n + 4);
      ss[0] = s0.x; ss[1] = s0.y; ss[2] = s0.z; ss[3] = s0.w; ss[4] = s1.x; ss[5] = s1.y; ss[6] = s1.z; ss[7] = s1.w;
    }
  }
  (epilogue_block_gen<MB, BM, NBW, I>(p, acc, patch, lane, wm, wn, m0, n0, bb, ss), ...);
}

// One tile per workgroup.  The LDS is a ring of 5 slots of 32 KiB; units alternate A-slab / W-slab of the same
// 64-deep K step (A_0 W_0 A_1 W_1 ...), each filled by full-line LDS-DMA (8 rows x 128 B per wave-instruction).
// While slab j is multiplied, units A_{j+1}, W_{j+1}, A_{j+2} are in flight, retired by a counted vmcnt.
template <int BM, bool GEN = false, int NBW = 4>
__global__ __launch_bounds__(512) void gemm_pp8_kernel(GemmArgs p) {
  static_assert(GEN || NBW == 4, "narrow tiles are served by the generalised variant only");
  constexpr int BN = 64 * NBW, BK = 64, NSLOT = 5;
  constexpr int MB = BM / 32;
  constexpr int GA = BM / 64;       // DMA instructions per wave per A unit (BM/8 groups over 8 waves)
  constexpr int GW = BN / 64;       // per W unit
  constexpr int SLOT = 2048;        // uint4 per slot (32 KiB)
  extern __shared__ __attribute__((aligned(16))) uint4 lds[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;

  const int tiles_m = (p.M + BM - 1) / BM, tiles_n = (p.N + BN - 1) / BN;
  const int nblk = tiles_m * tiles_n;
  const int wg = xcd_tile(blockIdx.x, nblk);
  const int tile_n = wg % tiles_n, tile_m = wg / tiles_n;
  const int z = blockIdx.y;
  const int z1 = z / p.nz2, z2 = z % p.nz2;
  const int m0 = tile_m * BM, n0 = tile_n * BN;

  const bf16_t* A = (const bf16_t*)p.A + (z1 * p.a_z1 + z2 * p.a_z2);
  const bf16_t* W = (const bf16_t*)p.W + (z1 * p.w_z1 + z2 * p.w_z2);

  // coalesced + swizzled DMA source: 8 consecutive lanes fetch the 8 chunks of ONE 128-byte row (one line request
  // instead of eight), lane (row r8 = l>>3, slot = l&7) takes chunk (slot ^ r8); the LDS image of a group is then
  // row-major [row][slot] and the MFMA read of (row, chunk C) goes to slot C ^ row -> conflict-free ds_read_b128.
  const int r8 = lane >> 3, ch = (lane & 7) ^ (lane >> 3);
  const bf16_t* asrc[GA];
  const bf16_t* wsrc[GW];
#pragma unroll
  for (int i = 0; i < GA; ++i) {
    int m = m0 + (wave + 8 * i) * 8 + r8;
    if (m > p.M - 1) m = p.M - 1;
    if constexpr (GEN) asrc[i] = A + (long)m * p.a_rstride + (long)(m / p.a_d1) * p.a_e1 + (long)(m / p.a_d2) * p.a_e2 + ch * 8;
    else asrc[i] = A + (long)(m / p.a_rpb) * p.a_bstride + (long)(m % p.a_rpb) * p.a_rstride + ch * 8;
  }
#pragma unroll
  for (int i = 0; i < GW; ++i) {
    const int rho = (wave + 8 * i) * 8 + r8;
    const int i16 = rho & 15;
    int n = n0 + (rho / (16 * NBW)) * (16 * NBW) + (i16 >> 2) * (4 * NBW) + ((rho >> 4) % NBW) * 4 + (i16 & 3);
    if (n > p.N - 1) n = p.N - 1;
    wsrc[i] = W + (long)n * p.ldw + ch * 8;
  }
  // GEN: K is made of kseg-element runs kseg_stride apart; the element offset of the NEXT A slab to fetch is tracked
  // incrementally (aoff), a_left = slabs left in the current run
  long aoff = 0;
  const int spk = GEN ? (p.kseg ? p.kseg / BK : 0x7fffffff) : 0;
  int a_left = spk;
  auto a_advance = [&]() {
    if constexpr (GEN) {
      aoff += BK;
      if (--a_left == 0) { a_left = spk; aoff += p.kseg_stride - p.kseg; }
    }
  };
  // unit u: even -> A slab u/2, odd -> W slab u/2; slot u % 5
  auto issue_a = [&](int kt, int slot) {
#pragma unroll
    for (int i = 0; i < GA; ++i) {
      if constexpr (GEN)
        __builtin_amdgcn_global_load_lds((gptr_t)(asrc[i] + aoff), (lptr_t)(lds + slot * SLOT + (wave + 8 * i) * 64), 16, 0, 0);
      else
        __builtin_amdgcn_global_load_lds((gptr_t)(asrc[i] + kt * BK), (lptr_t)(lds + slot * SLOT + (wave + 8 * i) * 64), 16, 0, 0);
    }
    a_advance();
  };
  auto issue_w = [&](int kt, int slot) {
#pragma unroll
    for (int i = 0; i < GW; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)(wsrc[i] + kt * BK), (lptr_t)(lds + slot * SLOT + (wave + 8 * i) * 64), 16, 0, 0);
  };

  f32x4 acc[NBW][MB];
#pragma unroll
  for (int i = 0; i < NBW; ++i)
#pragma unroll
    for (int j = 0; j < MB; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int cq = lane >> 4, r16 = lane & 15;
  // uint4 index inside a slot of fragment (16-row block blk, k-step ks): group (2*blk + (r16>>3)) * 64 + row*8 + slot
  const int rr8 = r16 & 7;
  const int frag0 = (r16 >> 3) * 64 + rr8 * 8 + ((cq) ^ rr8);        // ks = 0: chunk = cq
  const int frag1 = (r16 >> 3) * 64 + rr8 * 8 + ((4 + cq) ^ rr8);    // ks = 1: chunk = 4 + cq
  const int xoff = (wm * (MB * 2)) * 64;
  const int woff = (wn * 2 * NBW) * 64;

  // Staggered quarter-phase schedule ("8-phase"): the slab is multiplied in four groups of 4 x MB/2 MFMAs, each preceded
  // by a LOAD slot (its LDS fragment reads + two DMA instructions of the ring).  Slots are separated by raw barriers and
  // waves 4-7 run one slot behind waves 0-3, so on every SIMD one wave is in an MFMA slot while its partner is in a
  // LOAD slot: the matrix pipe never waits for LDS latency or DMA issue of its own wave.
  const int nk = p.K / BK;
  constexpr int HM = MB / 2;
  bf16x8 wfr[NBW], xfr[HM];
  const int grp = wave >> 2;
  const bool tr = p.trace != nullptr;
  long long t_begin = 0, t_first = 0, t_main = 0, c_first = 0, c_main = 0;  // t_*: s_memrealtime (100 MHz), c_*: s_memtime (core clock)
  if (tr) t_begin = wall_clock64();
  issue_a(0, 0);
  issue_w(0, 1);
  if (nk > 1) issue_a(1, 2);
  if (nk > 1) wait_vm<GA>(); else wait_vm<0>();
  __builtin_amdgcn_s_barrier();
  if (tr) { t_first = wall_clock64(); c_first = __builtin_amdgcn_s_memtime(); }
  int sa = 0, sw = 1;
#define SVT_LOAD(Q)                                                                                              \
  {                                                                                                              \
    constexpr int ks_ = (Q) >> 1, half_ = (Q)&1;                                                                 \
    if (half_ == 0) {                                                                                            \
      _Pragma("unroll") for (int nb = 0; nb < NBW; ++nb) wfr[nb] = __builtin_bit_cast(bf16x8, wa[nb * 128 + (ks_ ? frag1 : frag0)]); \
    }                                                                                                            \
    _Pragma("unroll") for (int jj = 0; jj < HM; ++jj)                                                            \
        xfr[jj] = __builtin_bit_cast(bf16x8, xa[(half_ * HM + jj) * 128 + (ks_ ? frag1 : frag0)]);               \
    if (ks_ == 0) {                                                                                              \
      if (kt + 1 < nk) {                                                                                         \
        _Pragma("unroll") for (int i2 = half_ * ((GW + 1) / 2); i2 < (half_ ? GW : (GW + 1) / 2); ++i2)          \
            __builtin_amdgcn_global_load_lds((gptr_t)(wsrc[i2] + (kt + 1) * BK),                                 \
                                             (lptr_t)(lds + ((2 * kt + 3) % NSLOT) * SLOT + (wave + 8 * i2) * 64), 16, 0, 0); \
      }                                                                                                          \
    } else {                                                                                                     \
      if (kt + 2 < nk) {                                                                                         \
        _Pragma("unroll") for (int i2 = half_ * ((GA + 1) / 2); i2 < (half_ ? GA : (GA + 1) / 2); ++i2)          \
            __builtin_amdgcn_global_load_lds((gptr_t)(asrc[i2] + (GEN ? aoff : (long)(kt + 2) * BK)),            \
                                             (lptr_t)(lds + ((2 * kt + 4) % NSLOT) * SLOT + (wave + 8 * i2) * 64), 16, 0, 0); \
        if (half_) a_advance();                                                                                  \
      }                                                                                                          \
    }                                                                                                            \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                           \
    __builtin_amdgcn_sched_barrier(0);                                                                           \
  }
#define SVT_MMA(Q)                                                                                               \
  {                                                                                                              \
    constexpr int half_ = (Q)&1;                                                                                 \
    __builtin_amdgcn_s_setprio(1);                                                                               \
    _Pragma("unroll") for (int jj = 0; jj < HM; ++jj)                                                            \
      _Pragma("unroll") for (int nb = 0; nb < NBW; ++nb)                                                         \
        acc[nb][half_ * HM + jj] = SVT_MFMA_16x16x32(wfr[nb], xfr[jj], acc[nb][half_ * HM + jj]); \
    __builtin_amdgcn_s_setprio(0);                                                                               \
    __builtin_amdgcn_sched_barrier(0);                                                                           \
  }
#define SVT_RETIRE_NEXT()                                                                                        \
  {                                                                                                              \
    if (kt + 2 < nk) wait_vm<GA>();                                                                              \
    else if (kt + 1 < nk) wait_vm<0>();                                                                          \
  }
  if (grp == 0) {
    for (int kt = 0; kt < nk; ++kt) {
      const uint4* xa = lds + sa * SLOT + xoff;
      const uint4* wa = lds + sw * SLOT + woff;
      SVT_LOAD(0) __builtin_amdgcn_s_barrier(); SVT_MMA(0) __builtin_amdgcn_s_barrier();
      SVT_LOAD(1) __builtin_amdgcn_s_barrier(); SVT_MMA(1) __builtin_amdgcn_s_barrier();
      SVT_LOAD(2) __builtin_amdgcn_s_barrier(); SVT_MMA(2) __builtin_amdgcn_s_barrier();
      SVT_LOAD(3) __builtin_amdgcn_s_barrier(); SVT_MMA(3)
      SVT_RETIRE_NEXT()
      __builtin_amdgcn_s_barrier();
      sa = (sa + 2) % NSLOT;
      sw = (sw + 2) % NSLOT;
    }
  } else {
    __builtin_amdgcn_s_barrier();  // one slot behind
    for (int kt = 0; kt < nk; ++kt) {
      const uint4* xa = lds + sa * SLOT + xoff;
      const uint4* wa = lds + sw * SLOT + woff;
      SVT_LOAD(0) __builtin_amdgcn_s_barrier(); SVT_MMA(0) __builtin_amdgcn_s_barrier();
      SVT_LOAD(1) __builtin_amdgcn_s_barrier(); SVT_MMA(1) __builtin_amdgcn_s_barrier();
      SVT_LOAD(2) __builtin_amdgcn_s_barrier(); SVT_MMA(2) __builtin_amdgcn_s_barrier();
      SVT_LOAD(3)
      SVT_RETIRE_NEXT()
      __builtin_amdgcn_s_barrier();
      SVT_MMA(3)
      if (kt + 1 < nk) __builtin_amdgcn_s_barrier();
      sa = (sa + 2) % NSLOT;
      sw = (sw + 2) % NSLOT;
    }
  }
#undef SVT_LOAD
#undef SVT_MMA
#undef SVT_RETIRE_NEXT
  // ---- epilogue ----
  const long coff = z1 * p.c_z1 + z2 * p.c_z2;
  const float* bias = p.bias ? p.bias + z2 * p.bias_z2 : nullptr;
  if (tr) { t_main = wall_clock64(); c_main = __builtin_amdgcn_s_memtime(); }
  __syncthreads();  // every wave is done with the ring before it is reused as transpose patches
  if constexpr (GEN)
    epilogue_seq_gen<MB, BM, NBW>(std::make_integer_sequence<int, MB>{}, p, acc, (float*)lds + wave * (16 * (16 * NBW + 4)), lane, wm, wn,
                                  m0, n0, bias);
  else {
    if constexpr (NBW == 4) {
      if (p.dbg != 3)
        epilogue_coalesced<MB, BM>(p, acc, (float*)lds + wave * (16 * 68), lane, wm, wn, m0, n0, coff, bias);
      else if (acc[0][0][0] == 123.456f) ((float*)p.C)[0] = 1.f;
    }
  }
  if (tr && lane == 0 && (wave & 3) == 0) {
    long long* o = p.trace + ((long)blockIdx.x * 2 + (wave >> 2)) * 8;
    o[0] = t_begin; o[1] = t_first; o[2] = t_main - t_first; o[3] = wall_clock64() - t_main; o[4] = wall_clock64(); o[5] = 1;
    o[6] = c_main - c_first; o[7] = BM;
  }
}

template <int BM, bool GEN = false, int NBW = 4>
int launch_pp8(const GemmArgs& a, hipStream_t s) {
  const int tiles_m = (a.M + BM - 1) / BM, tiles_n = (a.N + 64 * NBW - 1) / (64 * NBW);
  dim3 grid(tiles_m * tiles_n, a.nz, 1);
  const size_t lds_bytes = 5 * 32768;
  if (int r_ = ensure_dyn_lds((const void*)gemm_pp8_kernel<BM, GEN, NBW>, (int)lds_bytes)) return r_;
  hipLaunchKernelGGL((gemm_pp8_kernel<BM, GEN, NBW>), grid, dim3(512), lds_bytes, s, a);
  SVT_LAUNCH_CHECK();
  return 0;
}
}  // namespace

bool gemm_dma_eligible(const GemmArgs& a) { return a.K % 64 == 0 && a.N >= 128 && a.M >= 128 && a.c_vec && a.N % 8 == 0; }

// bm: 256 / 192 / 128, anything else 64 (generalised addressing: 128); bn = 128 (generalised addressing only, 256-row tiles) or 256
// (gemm_dispatch.hip, height_of_4 / height_of_3, names the height that runs for svt_debug_set key 39: keep them in step)
int launch_gemm_pp8(const GemmArgs& a, int bm, int bn, hipStream_t s) {
  if (a.gen) {
    if (bn == 128) return launch_pp8<256, true, 2>(a, s);
    if (bm == 256) return launch_pp8<256, true>(a, s);
    if (bm == 192) return launch_pp8<192, true>(a, s);
    return launch_pp8<128, true>(a, s);
  }
  if (bm == 256) return launch_pp8<256>(a, s);
  if (bm == 192) return launch_pp8<192>(a, s);
  if (bm == 128) return launch_pp8<128>(a, s);
  return launch_pp8<64>(a, s);
}

}  // namespace svt
