// Split-operand products (precision "bf16x3" / "fp16x3") on the LDS-DMA pipeline.  A stays fp32 in memory; the weight
// matrix was cut ONCE (svt_*_finalize -> split_weights_register) into 16-bit (hi, lo) pieces stored per row and 32-deep
// K slab as [hi k0..31 | lo k0..31] (128 bytes, the same bytes as the fp32 row).  Tile 256 x 256, K in 32-element slabs:
// an A unit is 256 rows x 128 B of fp32, a W unit 256 rows x 128 B of pieces, both moved by full-line LDS-DMA into the
// five-slot ring of the bf16 kernels (three units in flight across one raw barrier per slab, counted vmcnt).
// Wave layout 8 (M) x 1 (N): a wave owns 32 rows x all 256 columns, so every A element is cut into its pieces by exactly
// one wave (16 values per lane and slab: ~45 VALU instructions against 96 MFMAs), while the W pieces come out of LDS
// ready-made.  Per 16 x 16 x 32 block: Wl*Xh + Wh*Xl + Wh*Xh accumulated in fp32 (three MFMAs of 16 cycles; the exact
// fp32 form is eight of 32).  Epilogue: the LDS-transposed coalesced fp32 store of the bf16 kernels (bias, activation,
// residual).  The register-staged split kernel of gemm.hip (which cuts BOTH operands in every workgroup, four waves in
// lockstep around one barrier per slab) ran at 185-212 TFLOP/s on these shapes.
// LDS-DMA issued from inline asm (M0 = LDS byte address of the wave's 1 KiB piece, saved and restored around it).  hipcc
// tracks the LDS-DMA it emits itself for a builtin and puts an s_waitcnt vmcnt(0) in front of a later LDS read whose
// address it cannot prove distinct from the DMA's destination -- here the W fragment reads of every slab, i.e. the ring
// would be drained once per slab.  Through asm the compiler sees no LDS write; the counted vmcnt + barrier below order it.
//
// Staggered schedule (round 3).  The lockstep kernel first built on this plan (gemm_x3_kernel: git history) kept the matrix pipe busy
// for 0.43 of its cycles: all eight waves read their W fragments, issue their LDS-DMA and cut their A pieces at the same moments, so the two waves of a SIMD never
// cover each other.  Here waves 4-7 run ONE SLOT behind waves 0-3, exactly like gemm_pp8_kernel: a 32-deep slab is four MMA slots of
// NBS W blocks x 2 row blocks x 3 products (24 MFMAs at NBS = 4) and four LOAD slots that carry the next slot's W fragment reads
// (hi + lo pieces), two LDS-DMA instructions of the ring, and -- for the NEXT slab -- the raw fp32 reads of this wave's A rows (slot 0)
// and their cuts into (hi, lo) pieces (slots 1 and 2).  On every SIMD one wave multiplies while its partner loads.
// Ring (five 32 KiB slots, unit u = 2g (A_g) / 2g + 1 (W_g) in slot u % 5): slab g reads W_g and, for cutting, A_{g+1}; it requests
// A_{g+2} during its first two LOAD slots (into the slot W_{g-1} left) and W_{g+2} during the last two (into the slot of A_g, which has
// lived in registers since slab g - 1); the counted wait that retires the slab leaves only W_{g+2} in flight.  Requests past the last
// slab re-read slab nk - 1 (never used) so that the counts stay constant; one vmcnt(0) drains them before the LDS-transposed epilogue.
// NBS = 4: 256-column tiles; NBS = 3: 192-column tiles (N = 768: 63 x 4 = 252 tiles fill the 256 CUs; 256-column tiles give 189).
#include "gemm_epilogue.h"

namespace svt {
namespace {

// DBG (diagnostic builds, svt_debug_set key 3 = 31 / 33): 1 = no LDS-DMA after the head of the stream, 3 = no epilogue
template <bool F16, int NBS, int DBG = 0>
__global__ __launch_bounds__(512) void gemm_x3s_kernel(GemmArgs p, const void* wsplit) {
  constexpr int BM = 256, BN = 64 * NBS, BK = 32, NSLOT = 5, SLOT = 2048, GA = 4, GW = NBS;
  constexpr int NB = 4 * NBS;   // 16-column W blocks per tile
  extern __shared__ __attribute__((aligned(16))) uint4 lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tiles_m = (p.M + BM - 1) / BM, tiles_n = (p.N + BN - 1) / BN;
  const int nblk = tiles_m * tiles_n;
  const int wg = xcd_tile(blockIdx.x, nblk);
  const int tile_n = wg % tiles_n, tile_m = wg / tiles_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  // batch (blockIdx.y = z = z1 * nz2 + z2, the grouped positional conv): element offsets of the fp32 problem; a packed weight row
  // takes the bytes of its fp32 row
  const int zb = blockIdx.y, z1 = zb / p.nz2, z2 = zb - z1 * p.nz2;
  const float* A = (const float*)p.A + ((long)z1 * p.a_z1 + (long)z2 * p.a_z2);
  const unsigned short* W = (const unsigned short*)wsplit + 2 * ((long)z1 * p.w_z1 + (long)z2 * p.w_z2);  // [N][K / 32][64]: 32 hi pieces, 32 lo pieces
  const long czoff = (long)z1 * p.c_z1 + (long)z2 * p.c_z2;
  const int r8 = lane >> 3, ch = (lane & 7) ^ (lane >> 3);
  // ring requests in the `voffset + SGPR base` form (as gemm_x3p_kernel): a 64-bit scalar base per operand (A: the tile's first row -- the
  // tensor may exceed 4 GiB, a tile's span may not: gemm_x3p_eligible), one 32-bit offset per lane and request, the K advance scalar.
  // With per-lane 64-bit pointers every request cost two vector additions in its LOAD slot, ~70 cycles per slot under the partner's
  // MFMA issue: the slots with requests ran 356-376 cycles against 288 of MFMAs (profiles/r03_gemm_x3_slots.txt).
  const long a_o0 = a_row_off(p, m0);
  const char* abase = (const char*)A + a_o0;
  const char* wbase = (const char*)W;
  unsigned aoff[GA], woff[GW];
#pragma unroll
  for (int i = 0; i < GA; ++i) {
    int m = m0 + (wave + 8 * i) * 8 + r8;
    if (m > p.M - 1) m = p.M - 1;
    aoff[i] = (unsigned)(a_row_off(p, m) - a_o0) + ch * 16;
  }
#pragma unroll
  for (int i = 0; i < GW; ++i) {
    const int rho = (wave + 8 * i) * 8 + r8;
    const int i16 = rho & 15;
    int n = n0 + (rho >> 6) * 64 + (i16 >> 2) * 16 + ((rho >> 4) & 3) * 4 + (i16 & 3);
    if (n > p.N - 1) n = p.N - 1;
    woff[i] = (unsigned)((long)n * p.K * 4 + ch * 16);
  }
  const unsigned lds0 = lds_base(lds);
  auto unit_addr = [&](int slot, int i) -> unsigned { return __builtin_amdgcn_readfirstlane(lds_unit(lds0, wave, slot, i)); };
  const int nk = p.K / BK;
  auto kc = [&](int k) { return k < nk ? k : nk - 1; };   // requests past the end re-read the last slab
  f32x4 acc[NB][2];
#pragma unroll
  for (int i = 0; i < NB; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int cq = lane >> 4, r16 = lane & 15, rr8 = r16 & 7;
  const int rowb = (r16 >> 3) * 64 + rr8 * 8;
  const int fa0 = rowb + ((2 * cq) ^ rr8), fa1 = rowb + ((2 * cq + 1) ^ rr8);
  const int fwh = rowb + (cq ^ rr8), fwl = rowb + ((4 + cq) ^ rr8);
  const u32x4v* ldsv = (const u32x4v*)lds;
  // the IEEE-half build rejects the split modes but keeps this kernel's symbols, and has always cut its "bf16" pieces as bf16_t = halves
  constexpr bool CUT16 = F16 || std::is_same<bf16_t, _Float16>::value;
  // head of the stream: A_0 -> slot 0, W_0 -> slot 1, A_1 -> slot 2, W_1 -> slot 3; everything but W_1 landed before slab 0
#pragma unroll
  for (int i = 0; i < GA; ++i) dma_sv(aoff[i], abase, unit_addr(0, i));
#pragma unroll
  for (int i = 0; i < GW; ++i) dma_sv(woff[i], wbase, unit_addr(1, i));
#pragma unroll
  for (int i = 0; i < GA; ++i) dma_sv(aoff[i], abase + (long)kc(1) * (BK * 4), unit_addr(2, i));
#pragma unroll
  for (int i = 0; i < GW; ++i) dma_sv(woff[i], wbase + (long)kc(1) * 128, unit_addr(3, i));
  wait_vm<GW>();
  __builtin_amdgcn_s_barrier();
  u32x4v xh[2], xl[2], nh[2], nl[2], raw[2][2], wh[NBS], wl[NBS];
#pragma unroll
  for (int mb = 0; mb < 2; ++mb) cut8<CUT16>(ldsv[(wave * 2 + mb) * 128 + fa0], ldsv[(wave * 2 + mb) * 128 + fa1], xh[mb], xl[mb]);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();   // every wave holds its pieces of A_0 before the first slab's requests may reuse slots
  int sw = 1;                     // slot of W_g; A_{g+1} sits in the next one
  const int grp = wave >> 2;
  // DBG 11..14: s_memtime at both ends of slots 2 (DBG - 11), 2 (DBG - 11) + 1 of slab nk / 2 (tools/gemm_trace.py --x3-slots --one-tile)
  constexpr int STQ = DBG >= 11 && DBG <= 14 ? DBG - 10 : 0;
  unsigned sraw[5], sst[5];
  const int gs = nk / 2;
  if constexpr (STQ != 0) {
#pragma unroll
    for (int i = 0; i < 5; ++i) sst[i] = 0;
  }
#define X3S_S(k)                                                                                                    \
  if constexpr (STQ != 0 && (k) >= 4 * (STQ - 1) && (k) <= 4 * (STQ - 1) + 4 && (k) < 16)                           \
    sraw[((k) - 4 * (STQ - 1)) % 5] = (unsigned)__builtin_amdgcn_s_memtime();                                       \
  if constexpr (STQ == 4 && (k) == 0) sraw[4] = (unsigned)__builtin_amdgcn_s_memtime();
#define X3S_COMMIT()                                                                                                \
  if constexpr (STQ != 0) {                                                                                         \
    if (g == gs) { _Pragma("unroll") for (int i = 0; i < (STQ == 4 ? 4 : 5); ++i) sst[i] = sraw[i]; }               \
    if (STQ == 4 && g == gs + 1) sst[4] = sraw[4];                                                                  \
  }
#define X3S_LOAD(Q)                                                                                                 \
  {                                                                                                                 \
    _Pragma("unroll") for (int i = 0; i < NBS; ++i) {                                                               \
      wh[i] = wa[((Q) * NBS + i) * 128 + fwh];                                                                      \
      wl[i] = wa[((Q) * NBS + i) * 128 + fwl];                                                                      \
    }                                                                                                               \
    if ((Q) == 0) {                                                                                                 \
      _Pragma("unroll") for (int mb = 0; mb < 2; ++mb) { raw[mb][0] = xn[mb * 128 + fa0]; raw[mb][1] = xn[mb * 128 + fa1]; } \
    }                                                                                                               \
    if (DBG == 1) {                                                                                                 \
    } else if ((Q) < 2) {   /* A_{g+2} -> the slot W_{g-1} left */                                                  \
      _Pragma("unroll") for (int i2 = (Q) * 2; i2 < (Q) * 2 + 2; ++i2)                                              \
          dma_sv(aoff[i2], abase + (long)kc(g + 2) * (BK * 4), unit_addr(s3, i2));                  \
    } else {         /* W_{g+2} -> the slot of A_g */                                                               \
      _Pragma("unroll") for (int i2 = ((Q) - 2) * 2; i2 < ((Q) == 2 ? 2 : GW); ++i2)                                \
          dma_sv(woff[i2], wbase + (long)kc(g + 2) * 128, unit_addr(s4, i2));                        \
    }                                                                                                               \
    __builtin_amdgcn_sched_barrier(0);                                                                              \
    /* The cuts run BEHIND the slot's LDS reads and ring requests, under the LDS latency: while the partner wave issues its MFMAs \
       this wave's vector instructions get every other issue slot, so the 18 instructions of a cut take ~300 cycles (slot stamps \
       of gemm_x3p_kernel, tools/gemm_trace.py --x3-slots).  The cut pieces are "used" HERE: their only real use is the copy at the \
       end of the slab, and LLVM sinks a computation to its use -- both cuts ended up in the loop latch, behind the slab's last    \
       barrier, in front of the next LOAD slot 0 */                                                                      \
    if ((Q) == 1) { cut8<CUT16>(raw[0][0], raw[0][1], nh[0], nl[0]); asm volatile("" : "+v"(nh[0]), "+v"(nl[0])); }         \
    if ((Q) == 2) { cut8<CUT16>(raw[1][0], raw[1][1], nh[1], nl[1]); asm volatile("" : "+v"(nh[1]), "+v"(nl[1])); }         \
    __builtin_amdgcn_sched_barrier(0);                                                                              \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                              \
    if ((Q) == 0) asm volatile("" : "+v"(raw[0][0]), "+v"(raw[0][1]), "+v"(raw[1][0]), "+v"(raw[1][1]));            \
    _Pragma("unroll") for (int i = 0; i < NBS; ++i) asm volatile("" : "+v"(wh[i]), "+v"(wl[i]));                    \
    __builtin_amdgcn_sched_barrier(0);                                                                              \
  }
#define X3S_MMA(Q)                                                                                                  \
  {                                                                                                                 \
    __builtin_amdgcn_s_setprio(1);                                                                                  \
    _Pragma("unroll") for (int i = 0; i < NBS; ++i) {                                                               \
      _Pragma("unroll") for (int mb = 0; mb < 2; ++mb) acc[(Q) * NBS + i][mb] = mma3<F16>(wl[i], xh[mb], acc[(Q) * NBS + i][mb]); \
      _Pragma("unroll") for (int mb = 0; mb < 2; ++mb) acc[(Q) * NBS + i][mb] = mma3<F16>(wh[i], xl[mb], acc[(Q) * NBS + i][mb]); \
      _Pragma("unroll") for (int mb = 0; mb < 2; ++mb) acc[(Q) * NBS + i][mb] = mma3<F16>(wh[i], xh[mb], acc[(Q) * NBS + i][mb]); \
    }                                                                                                               \
    __builtin_amdgcn_s_setprio(0);                                                                                  \
    __builtin_amdgcn_sched_barrier(0);                                                                              \
  }
#define X3S_VARS()                                                                                                  \
  const u32x4v* wa = ldsv + sw * SLOT;                                                                            \
  const int s1 = sw + 1 >= NSLOT ? sw + 1 - NSLOT : sw + 1, s3 = sw + 3 >= NSLOT ? sw + 3 - NSLOT : sw + 3,         \
            s4 = sw + 4 >= NSLOT ? sw + 4 - NSLOT : sw + 4;                                                         \
  const u32x4v* xn = ldsv + s1 * SLOT + (wave * 2) * 128;
#define X3S_END()                                                                                                   \
  _Pragma("unroll") for (int mb = 0; mb < 2; ++mb) { xh[mb] = nh[mb]; xl[mb] = nl[mb]; }                            \
  sw = sw + 2 >= NSLOT ? sw + 2 - NSLOT : sw + 2;
  if (grp == 0) {
    for (int g = 0; g < nk; ++g) {
      X3S_VARS()
      X3S_S(0) X3S_LOAD(0) X3S_S(1) __builtin_amdgcn_s_barrier(); X3S_S(2) X3S_MMA(0) X3S_S(3) __builtin_amdgcn_s_barrier();
      X3S_S(4) X3S_LOAD(1) X3S_S(5) __builtin_amdgcn_s_barrier(); X3S_S(6) X3S_MMA(1) X3S_S(7) __builtin_amdgcn_s_barrier();
      X3S_S(8) X3S_LOAD(2) X3S_S(9) __builtin_amdgcn_s_barrier(); X3S_S(10) X3S_MMA(2) X3S_S(11) __builtin_amdgcn_s_barrier();
      X3S_S(12) X3S_LOAD(3) X3S_S(13) __builtin_amdgcn_s_barrier(); X3S_S(14) X3S_MMA(3)
      if (DBG != 1) wait_vm<GW>();
      __builtin_amdgcn_sched_barrier(0);
      X3S_S(15)
      __builtin_amdgcn_s_barrier();
      X3S_COMMIT()
      X3S_END()
    }
  } else {
    __builtin_amdgcn_s_barrier();  // one slot behind
    for (int g = 0; g < nk; ++g) {
      X3S_VARS()
      X3S_S(0) X3S_LOAD(0) X3S_S(1) __builtin_amdgcn_s_barrier(); X3S_S(2) X3S_MMA(0) X3S_S(3) __builtin_amdgcn_s_barrier();
      X3S_S(4) X3S_LOAD(1) X3S_S(5) __builtin_amdgcn_s_barrier(); X3S_S(6) X3S_MMA(1) X3S_S(7) __builtin_amdgcn_s_barrier();
      X3S_S(8) X3S_LOAD(2) X3S_S(9) __builtin_amdgcn_s_barrier(); X3S_S(10) X3S_MMA(2) X3S_S(11) __builtin_amdgcn_s_barrier();
      X3S_S(12) X3S_LOAD(3)
      if (DBG != 1) wait_vm<GW>();
      __builtin_amdgcn_sched_barrier(0);
      X3S_S(13)
      __builtin_amdgcn_s_barrier();
      X3S_S(14) X3S_MMA(3)
      X3S_S(15)
      if (g + 1 < nk) __builtin_amdgcn_s_barrier();
      X3S_COMMIT()
      X3S_END()
    }
  }
  if constexpr (STQ != 0) {
    if (p.trace && lane == 0) {
      long long* o = p.trace + 65536 + ((long)blockIdx.x * 8 + wave) * 32;
#pragma unroll
      for (int i = 0; i < 5; ++i) o[i] = sst[i];
      o[9] = nk; o[10] = gs; o[11] = STQ;
    }
  }
#undef X3S_S
#undef X3S_COMMIT
#undef X3S_LOAD
#undef X3S_MMA
#undef X3S_VARS
#undef X3S_END
  // ---- epilogue: LDS-transposed coalesced fp32 stores (epilogue_block: row base m0 + wm * (BM_/2) + mb * 16 with BM_ = 64, wm = wave;
  //      column base n0 + wn * 64 with wn = the 64-column group) ----
  wait_vm<0>();   // the surplus requests of the last two slabs: the ring becomes transpose patches
  __syncthreads();
  const float* bias = p.bias ? p.bias + (long)z2 * p.bias_z2 : nullptr;
  float* patch = (float*)lds + wave * (16 * 68);
  if constexpr (DBG == 3) {   // every accumulator stays live: a check of two of them lets hipcc delete the MFMAs of all the others
#pragma unroll
    for (int i = 0; i < NB; ++i) asm volatile("" ::"v"(acc[i][0]), "v"(acc[i][1]));
    return;
  }
#pragma unroll
  for (int g = 0; g < NBS; ++g) {
    const BiasRegs br = load_bias_regs<true>(p, bias, lane, g, n0);
    epilogue_block<2, 64, true>(p, acc[4 * g][0], acc[4 * g + 1][0], acc[4 * g + 2][0], acc[4 * g + 3][0], 0, patch, lane, wave, g, m0, n0, czoff, br);
    epilogue_block<2, 64, true>(p, acc[4 * g][1], acc[4 * g + 1][1], acc[4 * g + 2][1], acc[4 * g + 3][1], 1, patch, lane, wave, g, m0, n0, czoff, br);
  }
}

// DBG > 0 (the diagnostic forms) launch one z only
template <bool F16, int NBS, int DBG = 0>
int launch_x3s(const GemmArgs& a, const void* packed, hipStream_t s) {
  const long tiles = (long)((a.M + 255) / 256) * ((a.N + 64 * NBS - 1) / (64 * NBS));
  const size_t lds_bytes = 5 * 32768;
  if (int r_ = ensure_dyn_lds((const void*)gemm_x3s_kernel<F16, NBS, DBG>, (int)lds_bytes)) return r_;
  hipLaunchKernelGGL((gemm_x3s_kernel<F16, NBS, DBG>), dim3((unsigned)tiles, DBG ? 1u : (unsigned)a.nz), dim3(512), lds_bytes, s, a, packed);
  SVT_LAUNCH_CHECK();
  return 0;
}

#ifdef SVT_DIAG
template <int NBS>
int launch_x3s_stamped(int form, const GemmArgs& a, const void* packed, hipStream_t s) {
  if (form == 11) return launch_x3s<true, NBS, 11>(a, packed, s);
  if (form == 12) return launch_x3s<true, NBS, 12>(a, packed, s);
  if (form == 13) return launch_x3s<true, NBS, 13>(a, packed, s);
  return launch_x3s<true, NBS, 14>(a, packed, s);
}
#endif
}  // namespace

// kind = svt_precision (2 = bf16 pieces, 3 = fp16 pieces); nbs = 3 / 4 (192- / 256-column tiles); form: 0, or in DIAG builds (fp16 pieces)
// 1 / 3 = the timing ablations of the 256-column tile (svt_debug_set key 3 = 31 / 33) and 11-14 = the slot stamps (key 15 = 1-4)
int launch_gemm_x3s(int kind, const GemmArgs& a, const void* packed, int nbs, int form, hipStream_t s) {
#ifdef SVT_DIAG
  if (form == 1) return launch_x3s<true, 4, 1>(a, packed, s);
  if (form == 3) return launch_x3s<true, 4, 3>(a, packed, s);
  if (form >= 11) return nbs == 3 ? launch_x3s_stamped<3>(form, a, packed, s) : launch_x3s_stamped<4>(form, a, packed, s);
#endif
  if (kind == 3) return nbs == 3 ? launch_x3s<true, 3>(a, packed, s) : launch_x3s<true, 4>(a, packed, s);
  return nbs == 3 ? launch_x3s<false, 3>(a, packed, s) : launch_x3s<false, 4>(a, packed, s);
}

}  // namespace svt
