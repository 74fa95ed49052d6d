// GEMM selection.  Every dense product of the library enters at launch_gemm, and this file decides everything about its launch: the
// kernel family, the kernel inside the family, the tile height (one cost model), the tile width, the tile walk of the persistent
// kernels, the K order of the kernel-3 convolutions and every override of svt_debug_set.  It also brackets each product once for the
// profiler.  The kernel files launch exactly the configuration they are given (common.h).
#include "common.h"
#include <cstdint>

namespace svt {

// ---- switches of svt_debug_set (api.hip; keys in common.h) ----
int g_gemm_dbg = 0;
int g_gemm_force_bm = 0;
int g_gemm_ring = 0;
int g_gemm_variant = 0;
int g_gemm_skinny = 1;
int g_gemm_skinny_max_tiles = 32;
int g_gemm_x3 = 1;
int g_stamp_ends = 0;
int g_x3_pairs = 1;
int g_gemm_p1w = 1;   // 1 (default) = gemm_p1w_kernel where it measured faster than gemm_pps_kernel, 2 = everywhere (traced launches included), 0 = never
// key 30 = 1: gemm_p1x_kernel for every gemm_x3q-eligible launch with K >= 96, 0 (default) = gemm_x3q_kernel.  Measured
// (profiles/r05_gemm_p1x_ab.txt): bit-identical outputs and the SAME speed -- isolated launches within +-2 % (QKV -5 %, FFN-1 with GELU +3 %),
// C2 fp16x3 2 567-2 570 against 2 570-2 578 clips/s, C3 1 015 both.  With three MFMAs per algorithmic multiply-add the split products are
// bound by the matrix pipe at the clock the chip holds under that load, not by how the slab's loads are scheduled around it; the 16-bit
// products, where the single-wave loop gained (gemm_p1w.hip), are not.  Kept as the A/B arm and as a second implementation the tests compare.
int g_gemm_p1x = 0;
int g_gemm_skinny_small_tiles = 96;
int g_gemm_walk = -1;
int g_conv_kperm = 1;
int g_gemm_persist_wgs = 256;
// key 39 (query): which kernel the last product of this process ran on, 1000 * family + tile rows (+ 10000: a split-operand instantiation of
// the register-staged kernel); 0 = none yet.  Families: 1 gemm_skinny_kernel, 2 gemm_kernel (register-staged), 3 gemm_pp8_kernel,
// 4 gemm_pers_kernel, 5 gemm_pps_kernel, 6 gemm_p1w_kernel, 7 gemm_x3s_kernel (tile rows 256; 192 names its 192-COLUMN form),
// 8 gemm_x3p_kernel, 9 gemm_x3q_kernel, 10 gemm_p1x_kernel.  Written here, behind a launcher's call when it returned 0 (a refused launch
// leaves the id of the last product that ran), with the height the launcher instantiates (height_of_* below); the kernel files do not know it.
int g_gemm_kernel_id = 0;

namespace {

// the tile heights the launchers instantiate for a requested bm: 256 / 192 / 128, anything else 64 (launch_gemm_pp8, launch_gemm_pers) or 128
// (launch_gemm_pps, launch_gemm_p1w, the generalised forms of launch_gemm_pp8); the stamped gemm_p1w forms exist at 256 / 192 only.  The
// launchers' comments point back here: a launcher that changes its set of instantiations changes these with it.
int height_of_4(int bm) { return bm == 256 || bm == 192 || bm == 128 ? bm : 64; }
int height_of_3(int bm) { return bm == 256 || bm == 192 ? bm : 128; }
// records the kernel of a launch that was made (rc = the launcher's return value, passed through)
int ran(int family, int rows, int rc) {
  if (!rc) g_gemm_kernel_id = 1000 * family + rows;
  return rc;
}

// Tile height: minimise (rounds of 256 CUs) x (time of one K slab at that height).  The slab times are measured (tools/gemm_trace.py /
// gemm_bench.py --bm): 1.67 / 1.37 / 1.05 / 0.85 us for 256 / 192 / 128 / 64 rows -- a shorter tile does proportionally less MFMA work
// but moves the same 32 KiB of W per slab through the CU, so it only pays when it saves whole rounds.  Ties go to the larger tile.
// Candidates: the first n_heights of 256 / 192 / 128 / 64; col_tiles = tiles per row of tiles times the batch.
int pick_tile_height(long M, long col_tiles, int n_heights) {
  static const int heights[4] = {256, 192, 128, 64};
  static const int slab_cost[4] = {167, 137, 105, 85};
  long best_cost = -1;
  int best = 256;
  for (int i = 0; i < n_heights; ++i) {
    const long blocks = ((M + heights[i] - 1) / heights[i]) * col_tiles;
    const long cost = ((blocks + 255) / 256) * slab_cost[i];
    if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = heights[i]; }
  }
  return best;
}

// Panel height of the persistent tile walk (common.h tile_walk; svt_debug_set key 34).  The automatic choice: panels when W does not fit
// an XCD's L2 beside the A stream and the problem has enough columns of tiles to form them.
int gemm_walk_pm(const GemmArgs& a, int bm) {
  if (g_gemm_walk >= 0) return g_gemm_walk;
  const int tiles_n = a.N / 256, tiles_m = (a.M + bm - 1) / bm;
  const double w_bytes = (double)a.N * a.K * 2.0;
  // measured (profiles/r06_gemm_tile_walk.txt, us at pm = 0 / 8): FFN-1 of the base model (W 4.5 MiB) 76.1 / 70.6, the large FFN-1 (8 MiB) 262 / 255,
  // the large QKV (6 MiB) 181 / 177, 8192^3 800 / 746; QKV of the base model (W 3.4 MiB: resident) 52.3 / 53.5 -- hence the 4 MiB line
  if (tiles_n < 8 || tiles_m < 16 || w_bytes <= 4.0 * 1024 * 1024) return 0;
  return 8;
}

// One profiling bracket per product (bench.py's roofline leg): 2 M N K flops, and the bytes of both operands and of the output, per z.
// kind as for prof_end: 0 = the dominant family, 1 = the other dense contractions.
template <class Launch>
int profiled(const GemmArgs& a, int op_bytes, int out_bytes, int kind, hipStream_t s, Launch&& launch) {
  prof_begin(s);
  if (int r = launch()) return r;
  const double flops = 2.0 * a.M * (double)a.N * a.K * a.nz;
  const double bytes = ((double)a.M * a.K + (double)a.N * a.K) * op_bytes * a.nz + (double)a.M * a.N * a.nz * out_bytes;
  prof_end(s, flops, bytes, kind);
  return 0;
}

// svt_debug_set key 0 = 9 (tools/gemm_trace.py): the caller's `resid` is the kernels' trace buffer
GemmArgs unpack_trace(const GemmArgs& a) {
  GemmArgs g = a;
  if (g_gemm_dbg == 9 && a.resid) {
    g.trace = (long long*)a.resid;
    g.resid = nullptr;
  }
  return g;
}

// The 16-bit LDS-DMA family: the products gemm_dma_eligible admits, and the generalised ones (GemmArgs::gen).  Problems with at least
// two full rounds of tiles run a persistent kernel (epilogue stores and the next tile's fills overlap the MFMAs); single-round problems
// run the one-tile-per-workgroup kernel, whose LDS-transposed epilogue stores whole 128-byte lines.
int launch_dma(const GemmArgs& a0, hipStream_t s) {
  GemmArgs a = unpack_trace(a0);
  a.dbg = g_gemm_dbg == 9 && g_gemm_variant ? g_gemm_variant : g_gemm_dbg;
  const int tiles_n = (a.N + 255) / 256;
  int best = pick_tile_height(a.M, (long)tiles_n * a.nz, 4);
  if (g_gemm_force_bm) best = g_gemm_force_bm;
  // the persistent kernels are instantiated at 256 / 192 / 128 rows (the stamped gemm_p1w forms at 256 / 192): the walk is planned for the
  // height that runs
  auto persistent = [&](GemmArgs b, int bm, bool stamped_p1w) {
    b.walk_pm = gemm_walk_pm(b, bm == 256 || bm == 192 ? bm : stamped_p1w ? 192 : 128);
    return b;
  };
  return profiled(a, 2, a.out_f32 ? 4 : 2, 0, s, [&]() -> int {
    if (a.gen) {  // generalised addressing: one-tile kernel only (it also carries the residual epilogue)
      // 128-channel outputs (second stage of the lip front-end) get a 128-column tile: a 256-wide tile would multiply
      // zeros for half of its MFMAs
      // (a 64-column tile is LDS-read bound -- 18 fragment reads per 16 MFMAs -- and measured slower than the
      // register-staged kernel: 64-channel layers stay there)
      return a.N <= 128 ? ran(3, 256, launch_gemm_pp8(a, 256, 128, s)) : ran(3, height_of_3(best), launch_gemm_pp8(a, best, 256, s));
    }
    const long ntiles = (long)((a.M + best - 1) / best) * tiles_n;
    // Persistent staggered kernel (gemm_pps.hip): bf16 outputs without residual, from 100 tiles up.  With several tiles per workgroup
    // the prologue, the epilogue stores and the next tile's fills overlap; on single-round launches its register epilogue costs
    // 1.3 us against 4 us for the LDS-transposed one of gemm_pp8_kernel, and since its slab loop lost the per-slab register swaps
    // (gemm_pps.hip) it is as fast per slab: FFN-2 (252 tiles, K = 3072) 68.3 -> 61.1 us, the 138-tile FFN-2 of a 35-utterance song
    // 52.7 -> 48.0, 4096^3 115 -> 109; large FFN-2 (500 tiles, K = 4096) equal.  Measured per shape:
    // profiles/r03_gemm_vendor_library_yardstick.txt.  Write-through (sc1) stores: the output leaves L2 while the kernel runs instead
    // of at the kernel boundary (FFN-1: 98 MB, 16 us).
    // svt_debug_set key 3: 50 - 79 force it (the last digit is its dbg: 53 / 73 = without epilogue), 49 switches it off.
    if (g_gemm_variant >= 50 && g_gemm_variant < 80 && gemm_pps_eligible(a)) {
      const int bm = g_gemm_force_bm ? g_gemm_force_bm : (best < 128 ? 128 : best);
      GemmArgs b = persistent(a, bm, false);
      b.dbg = g_gemm_variant % 10;
      return ran(5, height_of_3(bm), launch_gemm_pps(b, bm, s));
    }
    if (g_gemm_variant != 49 && g_gemm_ring == 0 && best >= 128 && ntiles >= 100 && gemm_pps_eligible(a)) {
      // single-wave-per-SIMD kernel (gemm_p1w.hip, round 5): 5-11 % faster per launch wherever its un-overlapped epilogue is small beside the
      // tile -- everything except GELU launches with fewer than 16 K slabs (FFN-1 of the base model: 12 slabs, 72.8 us here against 81.9)
      if (g_gemm_p1w && a.K >= 192 && (!a.trace || g_gemm_p1w == 2) && (g_gemm_p1w == 2 || !(a.act == ACT_GELU && a.K < 1024))) {
        GemmArgs b = persistent(a, best, a.trace != nullptr);
        if (a.W_kperm && g_conv_kperm && a.kperm_taps >= 2 && a.kperm_taps <= 3 && a.kperm_cin % 64 == 0 && a.K == a.kperm_taps * a.kperm_cin && a.ldw == a.K) {
          // a kernel-3 convolution: tap-minor K order (GemmArgs::k_taps; the caller's second copy of W is stored that way)
          b.W = a.W_kperm; b.k_taps = a.kperm_taps; b.k_cin = a.kperm_cin;
        }
        return ran(6, a.trace ? (best == 256 ? 256 : 192) : height_of_3(best), launch_gemm_p1w(b, best, s));
      }
      return ran(5, height_of_3(best), launch_gemm_pps(persistent(a, best, false), best, s));
    }
    const bool pers_ok = !a.resid && a.nz == 1 && a.K >= 128 && a.N % 256 == 0 && a.c_z1 == 0 && a.c_z2 == 0 &&
                         a.a_z1 == 0 && a.a_z2 == 0 && a.w_z1 == 0 && a.w_z2 == 0;
    int mode = g_gemm_ring;
    if (mode == 0) mode = (pers_ok && ntiles >= 512) ? 4 : 2;
    if (mode == 4 && pers_ok) return ran(4, height_of_4(best), launch_gemm_pers(a, best, s));
    return ran(3, height_of_4(best), launch_gemm_pp8(a, best, 256, s));   // 64-row tiles for mid-size problems (2-16 utterances): twice the workgroups of the 128-row tile
  });
}

// The split-operand LDS-DMA family (precision "bf16x3" / "fp16x3", kind = 2 / 3) against a registered weight matrix.
// Returns 0 when launched, 1 when the caller has to use the register-staged split kernel instead, < 0 on error.
int launch_x3(int kind, const GemmArgs& a, hipStream_t s) {
  if (a.a_pairs) {
    // pair-row operand: only gemm_x3q_kernel reads it (the callers in api_encoder.hip ask gemm_x3q_eligible before they choose the layout)
    if (!gemm_x3q_eligible(a) || a.ldw != a.K) { set_error("gemm: pair-row operand outside the contract of gemm_x3q_kernel"); return -1; }
    const void* packed = split_weights_find(a.W, kind, a.K, a.N);
    if (!packed) { set_error("gemm: pair-row product against a weight matrix that was not registered as split"); return -1; }
    int bm = pick_tile_height(a.M, a.N / 256, 3);
    if (g_gemm_force_bm == 256 || g_gemm_force_bm == 192 || g_gemm_force_bm == 128) bm = g_gemm_force_bm;
    GemmArgs g = a;
    g.planes_f16 = kind == 3;
    return profiled(a, 4, 4, 0, s, [&] {
      // one wave per SIMD (gemm_p1x.hip; svt_debug_set key 30 = 1: A/B, same bits)
      const bool p1x = g_gemm_p1x && g.K >= 96;
      return ran(p1x ? 10 : 9, bm, p1x ? launch_gemm_p1x(kind, g, packed, bm, s) : launch_gemm_x3q(kind, g, packed, bm, s));
    });
  }
  // batched problems (nz > 1: the grouped positional conv, one z per group): the one-tile kernel with blockIdx.y = z; the registered
  // matrix holds the groups' rows one after the other
  const bool batched = a.nz > 1;
  if (a.gen || a.nz < 1 || a.K % 32 || a.N < 128 || a.M < 128 || !a.c_vec || a.ldw != a.K || a.alpha != 1.f || (a.a_rstride & 3) ||
      (a.a_bstride & 3) || ((uintptr_t)a.A & 15))
    return 1;
  if (!batched && (a.w_z1 || a.w_z2 || a.a_z1 || a.a_z2 || a.c_z1 || a.c_z2)) return 1;
  if (batched && (a.planes || a.resid || a.nz2 < 1 || a.nz % a.nz2 || (a.a_z1 & 3) || (a.a_z2 & 3) || (a.c_z1 & 3) || (a.c_z2 & 3) || (a.bias_z2 & 3) ||
                  a.w_z1 % a.K || a.w_z2 % a.K || a.nz > 65535))
    return 1;
  const size_t last_z_row = batched ? ((size_t)(a.nz / a.nz2 - 1) * a.w_z1 + (size_t)(a.nz2 - 1) * a.w_z2) / (size_t)a.K : 0;
  const void* packed = split_weights_find(a.W, kind, a.K, (long)last_z_row + a.N);
  if (!packed || !tile_span_fits(a)) return 1;
  GemmArgs g = unpack_trace(a);
  g.out_f32 = 1;
  g.planes_f16 = kind == 3;
  if (g.trace) g.stamp_ends = g_stamp_ends;
  // tile width: 192 columns when that fills the chip better (N = 768: 252 tiles against 189)
  const long tm = (a.M + 255) / 256;
  const long t256 = tm * ((a.N + 255) / 256), t192 = tm * ((a.N + 191) / 192);
  auto rounds = [](long t) { return (t + 255) / 256; };
  const int nbs = a.N % 192 == 0 && rounds(t192) * 3 < rounds(t256) * 4 ? 3 : 4;
  // persistent form (gemm_x3p.hip: register epilogue, stores under the next tile's MFMAs) wherever it is eligible; 192-column tiles of
  // the one-tile kernel when they fill the chip better and the launch is a single round anyway (svt_debug_set key 3: 32 = never the
  // persistent form, 34 = always when eligible, 30 / 31 / 33 = the one-tile kernel's arms -- A/B)
  // Measured per shape (profiles/r03_gemm_x3_variants.txt): the persistent form is ahead on the launches with a heavy epilogue and
  // several tiles per CU (conv 1-4, FFN-1: GELU over fp32 outputs), the one-tile kernel on the plain projections (QKV, out-proj, FFN-2).
  const bool x3p_ok = !batched && gemm_x3p_eligible(g) && g_gemm_variant != 30 && g_gemm_variant != 31 && g_gemm_variant != 32 && g_gemm_variant != 33;
  return profiled(a, 4, 4, 0, s, [&]() -> int {
    if (x3p_ok && (g_gemm_variant == 34 || (a.act == ACT_GELU && t256 > 256) || t256 >= 1024)) {   // (large QKV, 1 500 tiles: 547 against 583 us)
      g.dbg = g_gemm_dbg == 9 ? 0 : g_gemm_dbg;
      return ran(8, 256, launch_gemm_x3p(kind, g, packed, s));
    }
#ifdef SVT_DIAG
    // slot stamps of the one-tile kernel, and its timing ablations (diagnostics; make DIAG=1)
    if (g.trace && kind == 3 && g.stamp_ends >= 1 && g.stamp_ends <= 4) return ran(7, nbs == 3 ? 192 : 256, launch_gemm_x3s(kind, g, packed, nbs, 10 + g.stamp_ends, s));
    if ((g_gemm_variant == 31 || g_gemm_variant == 33) && kind == 3) return ran(7, 256, launch_gemm_x3s(kind, g, packed, 4, g_gemm_variant - 30, s));
#endif
    return ran(7, nbs == 3 ? 192 : 256, launch_gemm_x3s(kind, g, packed, nbs, 0, s));
  });
}

}  // namespace

// the small-problem kernel: 32 x 32 tiles while the 64 x 64 tiling has at most g_gemm_skinny_small_tiles workgroups
int launch_gemm_skinny(const GemmArgs& a, hipStream_t s) {
  const long tiles64 = (long)((a.M + 63) / 64) * ((a.N + 63) / 64) * a.nz;
  const int tile = tiles64 <= g_gemm_skinny_small_tiles ? 32 : 64;
  return profiled(a, 2, a.out_f32 ? 4 : 2, 1, s, [&] { return ran(1, tile, launch_gemm_skinny_tile(a, tile, s)); });
}

// prec: 0 = fp32 operands, exact fp32 MFMA; 1 = bf16 operands; 2 / 3 = fp32 operands in memory, bf16x3 / fp16x3
// split-operand products (every other argument as for prec 0)
int launch_gemm(int prec_in, const GemmArgs& a, hipStream_t s) {
  if (a.M <= 0 || a.N <= 0 || a.K <= 0) { set_error("gemm: empty problem"); return -1; }
  // pair rows are understood by the split-operand LDS-DMA kernels only: every other kernel would read them as fp32 words
  if ((a.a_pairs || a.c_pairs) && (prec_in < 2 || !g_gemm_x3)) {
    set_error("gemm: pair-row operands / outputs need a split-operand precision and the LDS-DMA split kernels (svt_debug_set key 11 = 1)");
    return -1;
  }
  if (a.planes) {
    // C as (hi, lo) planes (split-operand modes only): written by the LDS-DMA split kernel's epilogue; any other kernel writes the
    // fp32 C and the planes are cut from it afterwards
    if (prec_in < 2 || a.nz != 1 || a.gen) { set_error("gemm: (hi, lo) plane output is served for plain split-operand products"); return -1; }
    if (g_gemm_x3) {
      GemmArgs gp = a;
      gp.c_vec = !(a.ldc & 3) && !((uintptr_t)a.C & 15) && !((uintptr_t)a.resid & 15) && !((uintptr_t)a.bias & 15) && !(a.plane_stride & 3) &&
                 !((uintptr_t)a.planes & 7);
      const int r = launch_x3(prec_in, gp, s);
      if (r <= 0) return r;
    }
    GemmArgs g2 = a;
    g2.planes = nullptr;
    if (int r = launch_gemm(prec_in, g2, s)) return r;
    return launch_split_planes(prec_in, (const float*)a.C, a.ldc, a.M, a.N, a.planes, a.ldc, a.plane_stride, s);
  }
  const int split = prec_in >= 2 ? prec_in - 1 : 0;
  const int prec = prec_in >= 2 ? 0 : prec_in;
  const int epp = prec ? 8 : 4;
  if (a.K % epp != 0) { set_error("gemm: K must be a multiple of the 16-byte piece"); return -1; }
  auto mult = [](long v, long m) { return v % m == 0; };
  if (!mult(a.a_rstride, epp) || !mult(a.a_bstride, epp) || !mult(a.a_z1, epp) || !mult(a.a_z2, epp) || !mult(a.ldw, epp) ||
      !mult(a.w_z1, epp) || !mult(a.w_z2, epp) || ((uintptr_t)a.A & 15) || ((uintptr_t)a.W & 15)) {
    set_error("gemm: operand rows must be 16-byte aligned");
    return -1;
  }
  GemmArgs g = a;
  const int cel = (a.out_f32 || !prec) ? 4 : 8;  // elements per 16 bytes of C
  g.c_vec = mult(a.ldc, cel) && mult(a.c_z1, cel) && mult(a.c_z2, cel) && !((uintptr_t)a.C & 15) &&
            mult(a.ldc, 4) && mult(a.c_z1, 4) && mult(a.c_z2, 4) && !((uintptr_t)a.resid & 15) &&
            mult(a.bias_z2, 4) && !((uintptr_t)a.bias & 15);
  // the register-staged kernel: 256 x 64 tiles for narrow outputs, 128 x 128 otherwise
  auto staged = [&] {
    const int bn = a.N <= 64 ? 64 : 128;
    return profiled(g, prec ? 2 : 4, (g.out_f32 || !prec) ? 4 : 2, split ? 0 : 1, s,
                    [&] { return ran(split ? 12 : 2, bn == 64 ? 256 : 128, launch_gemm_staged(prec_in, g, bn, s)); });   // (family 12 = 10000 + family 2)
  };
  if (a.gen) {
    const int kel = prec ? 64 : 32;
    if (a.kseg && (a.kseg % kel || a.K % a.kseg)) { set_error("gemm: kseg must divide K and be a multiple of the K slab"); return -1; }
    if (!mult(a.a_e1, epp) || !mult(a.a_e2, epp) || !mult(a.kseg_stride, epp)) { set_error("gemm: generalised A strides must be 16-byte aligned"); return -1; }
    g.c_vec = g.c_vec && mult(a.c_e1, cel) && mult(a.c_e2, cel) && mult(a.c_base, cel) &&
              (!a.resid || !a.resid_op_type || !((uintptr_t)a.resid & 15));
    // N >= 128 with bf16 output: the LDS-DMA pipeline (needs 64-element K slabs inside every run and nz == 1)
    if (prec && a.K % 64 == 0 && a.N >= 128 && a.N % 8 == 0 && a.M >= 128 && g.c_vec && !a.out_f32 && a.nz == 1 &&
        (!a.resid || a.resid_op_type) && a.alpha == 1.f && (a.kseg == 0 || a.kseg % 64 == 0))
      return launch_dma(g, s);
    return staged();
  }
  if (prec && g_gemm_skinny && gemm_skinny_eligible(g)) return launch_gemm_skinny(g, s);
  if (prec && gemm_dma_eligible(g)) return launch_dma(g, s);
  if (prec) return staged();
  if (split && g_gemm_x3) {
    const int r = launch_x3(prec_in, g, s);
    if (r <= 0) return r;
  }
  if (a.a_pairs || a.c_pairs) { set_error("gemm: this geometry is outside the pair-row kernels' contract"); return -1; }
  return staged();
}

}  // namespace svt
