// Attention selection.  Every attention of the library enters at launch_attention: plan_attention (host.cpp) names the path from the
// geometry, this file checks that the workspace holds what that path needs and launches it; carve_attention cuts a workspace from the same
// plan.  The wide / narrow and staggered choices inside the fused launchers (g_flash_wide, the grid size) stay in the kernel files.
// Host code only.
#include "api.h"
#include "common.h"

namespace svt {

AttnGeom attn_geom(const AttnArgs& a) {
  const long D = (long)a.H * a.dh;
  const size_t es = esize(a.prec);
  AttnGeom g;
  g.prec = a.prec; g.gp = a.gp < 0 ? a.prec : a.gp; g.dh = a.dh; g.T = a.T;
  g.bias = a.gate != nullptr; g.drop = a.drop != nullptr; g.fused_drop = a.fused_drop;
  g.packed_kv = a.ldkv == 3 * D && (const char*)a.V == (const char*)a.K + D * es;
  g.q_packed = g.packed_kv && a.ldq == 3 * D && (const char*)a.Q == (const char*)a.K - D * es;
  return g;
}

AttnBufs carve_attention(Carver& cv, const AttnPlan& plan, size_t B, size_t H, size_t T, size_t dh, size_t es) {
  const size_t Tp = (size_t)plan.Tp, rows = B * T, D = H * dh;
  AttnBufs ab{};
  if (plan.scores) {
    ab.S = (float*)cv.take(B * H * T * Tp * 4);
    ab.P = cv.take(B * H * T * Tp * es);
  }
  if (plan.vt) ab.Vt = cv.take(B * H * dh * Tp * es);
  if (plan.planes_qkv) ab.pl_qkv = cv.take(rows * 3 * D * 4);
  if (plan.planes_q) ab.pl_q = cv.take(rows * D * 4);
  return ab;
}

namespace {

// split-operand fused attention: cut the fp32 projections into 16-bit planes once, then three MFMAs per product
// (attention_x3.hip flash_attn_x3_kernel) -- no (B, H, T, T) score tensor
int fused_x3(const AttnArgs& a, int gp, bool q_packed, const AttnBufs& ab, hipStream_t s) {
  const int B = a.B, T = a.T, H = a.H, dh = a.dh;
  const long D = (long)H * dh, rows = (long)B * T;
  const float* kv0 = (const float*)a.K - D;                     // start of the packed (rows, 3D) projection
  const long pl3 = rows * 3 * D;
  unsigned short* p3 = (unsigned short*)ab.pl_qkv;
  if (!a.kv_ready)
    if (int r = launch_split_planes(gp, kv0, 3 * D, rows, (int)(3 * D), p3, 3 * D, pl3, s)) return r;
  const unsigned short* qp;
  long qld, qpl;
  if (q_packed) { qp = p3; qld = 3 * D; qpl = pl3; }
  else {
    if (int r = launch_split_planes(gp, (const float*)a.Q, a.ldq, rows, (int)D, ab.pl_q, D, rows * D, s)) return r;
    qp = (const unsigned short*)ab.pl_q; qld = D; qpl = rows * D;
  }
  return launch_flash_attention_x3(gp, qp, qld, (long)T * qld, qpl, p3 + D, p3 + 2 * D, 3 * D, (long)T * 3 * D, pl3, (float*)a.out, a.ldo,
                                   (long)T * a.ldo, B, T, H, dh, a.scale, s, a.o_pairs);
}

// materialised scores: S = scale q k^T [+ gated bias] -> P = softmax(S) [masked] -> out = P V, as two batched products
int scores(const AttnArgs& a, int gp, int Tp, const AttnBufs& ab, hipStream_t s) {
  const int prec = a.prec, B = a.B, T = a.T, H = a.H, dh = a.dh;
  GemmArgs g;
  g.A = a.Q; g.W = a.K; g.C = ab.S;
  g.M = T; g.N = T; g.K = dh;
  g.a_rpb = T; g.a_bstride = 0; g.a_rstride = a.ldq;
  g.ldw = a.ldkv; g.ldc = Tp;
  g.nz = B * H; g.nz2 = H;
  g.a_z1 = (long)T * a.ldq; g.a_z2 = dh;
  g.w_z1 = (long)T * a.ldkv; g.w_z2 = dh;
  g.c_z1 = (long)H * T * Tp; g.c_z2 = (long)T * Tp;
  g.alpha = a.scale; g.out_f32 = 1;
  if (int r = launch_gemm(gp, g, s)) return r;
  if (a.gate)
    if (int r = launch_scores_add_relbias(ab.S, (int64_t)B * H, H, T, Tp, a.gate, a.relpb, s)) return r;
  if (a.drop) { if (int r = launch_softmax_dropout(prec, ab.S, (int64_t)B * H * T, T, Tp, ab.P, 0, *a.drop, s)) return r; }
  else if (int r = launch_softmax_rows(prec, ab.S, (int64_t)B * H * T, T, Tp, ab.P, s)) return r;
  if (!a.kv_ready)
    if (int r = launch_transpose_v(prec, a.V, B, T, H, dh, a.ldkv, 0, Tp, ab.Vt, s)) return r;
  GemmArgs o;
  o.A = ab.P; o.W = ab.Vt; o.C = a.out;
  o.M = T; o.N = dh; o.K = Tp;
  o.a_rpb = T; o.a_rstride = Tp;
  o.ldw = Tp; o.ldc = a.ldo;
  o.nz = B * H; o.nz2 = H;
  o.a_z1 = (long)H * T * Tp; o.a_z2 = (long)T * Tp;
  o.w_z1 = (long)H * dh * Tp; o.w_z2 = (long)dh * Tp;
  o.c_z1 = (long)T * a.ldo; o.c_z2 = dh;
  return launch_gemm(gp, o, s);
}

}  // namespace

int launch_attention(const AttnArgs& a, const AttnBufs& ab, hipStream_t s) {
  const AttnGeom geom = attn_geom(a);
  const AttnPlan plan = plan_attention(geom);
  if (a.o_pairs && plan.path != ATTN_FUSED_X3) { set_error("attention: pair-row output is served by the fused split attention only"); return -1; }
  if (plan.scores && !(ab.S && ab.P)) { set_error("attention: no workspace for the scores"); return -1; }
  if (plan.vt && !ab.Vt) { set_error("attention: no workspace for V^T"); return -1; }
  if (plan.planes_qkv && !ab.pl_qkv) { set_error("attention: no workspace for the planes of the packed projection"); return -1; }
  if (plan.planes_q && !ab.pl_q) { set_error("attention: no workspace for the query planes"); return -1; }
  const int T = a.T;
  switch (plan.path) {
    case ATTN_FUSED_X3:
      return fused_x3(a, geom.gp, geom.q_packed, ab, s);
    case ATTN_FUSED16:
      return launch_flash_attention(a.Q, a.ldq, (long)T * a.ldq, a.K, a.V, a.ldkv, (long)T * a.ldkv, a.out, a.ldo, (long)T * a.ldo, a.B, T,
                                    a.H, a.dh, a.scale, s, a.gate, a.gate ? a.relpb : nullptr);
    case ATTN_FUSED16_DROP:
      return launch_flash_attention_dropout(a.Q, a.ldq, (long)T * a.ldq, a.K, a.V, a.ldkv, (long)T * a.ldkv, a.out, a.ldo, (long)T * a.ldo,
                                            a.B, T, a.H, a.dh, a.scale, 0, *a.drop, s);
    case ATTN_SCORES:
      return scores(a, geom.gp, plan.Tp, ab, s);
  }
  return -1;
}

}  // namespace svt
