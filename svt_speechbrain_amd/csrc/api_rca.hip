// C ABI of FusionRCA, the audio-visual fusion of two cross-attention layers: finalize, forward, and the training step (forward with
// saved intermediates, backward, parameter refresh), with the debug hooks that run its training kernels alone.  Host code only.
#include "../../include/svt_mi355.h"
#include "api.h"
#include "common.h"
#include "host.h"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

using namespace svt;

struct RcaLayerW {
  DevBuf win, bin, wo, bo, w1, b1, w2, b2, n1g, n1b, n2g, n2b;
  DevBuf woT, w1T, w2T;   // transposed operand copies for the backward's dX products (written by svt_rca_refresh_params only)
};
struct svt_rca {
  int D = 0, H = 0, F = 0, max_len = 0, prec = 0, gp = 0, device = 0;  // prec: storage type, gp: product engine
  float alpha = 0.5f;
  bool finalized = false;
  bool uploaded = false;   // device buffers exist: the next finalize is a RE-upload into live buffers
  bool transposed = false; // woT / w1T / w2T hold the current weights (svt_rca_refresh_params since the last finalize)
  ParamMap params;
  DevBuf pe;
  RcaLayerW L[2];
};

namespace {
struct RcaWs {
  float *s1F, *s2F;
  void *s1T, *s2T;
  void* qkv;     // (rows, 3D) projections of the kv stream
  void* qc;      // (rows, D) cross query
  AttnBufs ab;
  void *att_s, *att_c, *blend;
  float *preF, *xF;
  void* xT;
  void* ffn;
  float *o1, *o2;
  size_t total;
};
RcaWs carve_rca(const svt_rca* r, int B, int T, void* base) {
  Carver cv(base);
  RcaWs w;
  const size_t es = esize(r->prec), rows = (size_t)B * T, D = r->D;
  const int dh = r->D / r->H;
  w.s1F = (float*)cv.take(rows * D * 4);
  w.s2F = (float*)cv.take(rows * D * 4);
  w.s1T = r->prec ? cv.take(rows * D * es) : (void*)w.s1F;
  w.s2T = r->prec ? cv.take(rows * D * es) : (void*)w.s2F;
  w.qkv = cv.take(rows * 3 * D * es);
  w.qc = cv.take(rows * D * es);
  // one set of buffers serves both attentions of a layer: k | v packed in both, the cross query in a buffer of its own
  // (kept on purpose: V^T on the fused paths, S and P in the split modes, which nothing reads -- attn_workspace_plan)
  AttnGeom ag;
  ag.prec = r->prec; ag.gp = r->gp; ag.dh = dh; ag.T = T; ag.packed_kv = true;
  w.ab = carve_attention(cv, attn_workspace_plan(plan_attention(ag), true), B, r->H, T, dh, es);
  w.att_s = cv.take(rows * D * es);
  w.att_c = cv.take(rows * D * es);
  w.blend = cv.take(rows * D * es);
  w.preF = (float*)cv.take(rows * D * 4);
  w.xT = cv.take(rows * D * es);
  w.xF = r->prec ? (float*)cv.take(rows * D * 4) : (float*)w.xT;
  w.ffn = cv.take(rows * r->F * es);
  w.o1 = (float*)cv.take(rows * D * 4);
  w.o2 = (float*)cv.take(rows * D * 4);
  w.total = cv.off;
  return w;
}

// what svt_rca_forward_train keeps per layer for svt_rca_backward
struct RcaSave {
  void *qkv, *qc, *att_s, *att_c, *blend, *xT, *ffn;
  float *pre1, *pre2;   // fp32 inputs of LN1 / LN2 before the residual add (LN1 adds the kv stream, LN2 the LN1 output)
  float* xF;            // LN1 output, fp32
  float* lse;           // [2][B][H][T]: self, cross
};
// backward scratch (shared by the two layers)
struct RcaBwdWs {
  float *dy2F, *dhF, *dxF, *dy1F, *dblF, *dqkv, *dqc, *delta;
  void *dyT, *dhT;      // operand copies of the dX products' A operand (16-bit mode; fp32 mode: the fp32 buffers)
  void *ln_scr, *wg_scr;
};
struct RcaTrainWs {
  RcaWs f;
  RcaSave L[2];
  RcaBwdWs b;
  size_t total;
};
RcaTrainWs carve_rca_train(const svt_rca* r, int B, int T, void* base) {
  RcaTrainWs w;
  w.f = carve_rca(r, B, T, base);
  Carver cv(base);
  cv.off = w.f.total;
  const size_t es = esize(r->prec), rows = (size_t)B * T, D = r->D, F = r->F;
  for (int l = 0; l < 2; ++l) {
    RcaSave& S = w.L[l];
    S.qkv = cv.take(rows * 3 * D * es);
    S.qc = cv.take(rows * D * es);
    S.att_s = cv.take(rows * D * es);
    S.att_c = cv.take(rows * D * es);
    S.blend = cv.take(rows * D * es);
    S.pre1 = (float*)cv.take(rows * D * 4);
    S.pre2 = (float*)cv.take(rows * D * 4);
    S.xT = cv.take(rows * D * es);
    S.xF = r->prec ? (float*)cv.take(rows * D * 4) : (float*)S.xT;
    S.ffn = cv.take(rows * F * es);
    S.lse = (float*)cv.take((size_t)2 * B * r->H * T * 4);
  }
  RcaBwdWs& b = w.b;
  b.dy2F = (float*)cv.take(rows * D * 4);
  b.dhF = (float*)cv.take(rows * F * 4);
  b.dxF = (float*)cv.take(rows * D * 4);
  b.dy1F = (float*)cv.take(rows * D * 4);
  b.dblF = (float*)cv.take(rows * D * 4);
  b.dqkv = (float*)cv.take(rows * 3 * D * 4);
  b.dqc = (float*)cv.take(rows * D * 4);
  b.delta = (float*)cv.take((size_t)2 * B * r->H * T * 4);
  b.dyT = r->prec ? cv.take(rows * D * es) : nullptr;
  b.dhT = r->prec ? cv.take(rows * F * es) : nullptr;
  b.ln_scr = cv.take(rca_ln_bwd_scratch_bytes((int64_t)rows, (int)D));
  size_t wg = 0;
  const int64_t R = (int64_t)rows;
  for (size_t need : {rca_wgrad_scratch_bytes(2 * R, (int)D, (int)D), rca_wgrad_scratch_bytes(R, 2 * (int)D, (int)D),
                      rca_wgrad_scratch_bytes(R, (int)D, (int)D), rca_wgrad_scratch_bytes(R, (int)F, (int)D),
                      rca_wgrad_scratch_bytes(R, (int)D, (int)F)})
    wg = std::max(wg, need);
  b.wg_scr = cv.take(std::max<size_t>(wg, 16));
  w.total = cv.off;
  return w;
}

int rca_check_call(const char* who, const svt_rca* r, int B, int T1, int T2) {
  if (!r->finalized) { set_error(std::string(who) + ": parameters not finalized"); return SVT_ERR_STATE; }
  if (B < 1 || T1 < 1 || T2 < 1) { set_error(std::string(who) + ": empty input"); return SVT_ERR_INVALID; }
  if (T1 > r->max_len) { set_error(std::string(who) + ": sequence longer than the positional table"); return SVT_ERR_INVALID; }
  return SVT_OK;
}

// the forward of svt_rca_forward; with `save` (svt_rca_forward_train) every per-layer intermediate goes to its own buffer and the
// attention log-sum-exps are written after the forward's kernels -- the same kernels, so the output has the same bits
int rca_forward_run(svt_rca* r, const float* audio, int T1, const float* video, int T2, int B, float* out, const RcaWs& w,
                    const RcaSave* save, hipStream_t s) {
  const int prec = r->prec, D = r->D, H = r->H, F = r->F, dh = D / H, T = T1;
  const int64_t rows = (int64_t)B * T;
  const size_t es = esize(prec);
  // frame alignment (fusion.py:195-205) + positional encoding (fusion.py:60-61)
  if (int rc = launch_add_pe(prec, audio, B, T, T, D, r->pe.as<float>(), w.s1F, prec ? w.s1T : nullptr, s)) return rc;
  // video: T2 frames per clip in memory; frames >= T1 are dropped, frames in [T2, T1) read as zero
  if (int rc = launch_add_pe(prec, video, B, T, T2, D, r->pe.as<float>(), w.s2F, prec ? w.s2T : nullptr, s)) return rc;
  const float scale = 1.0f / std::sqrt((float)dh);
  auto gemm_rows = [&](const void* A, int K, const void* W, const float* bias, int N, void* C, int out_f32, int act,
                       const float* resid) -> int {
    GemmArgs g;
    g.A = A; g.W = W; g.C = C; g.bias = bias; g.resid = resid;
    g.M = (int)rows; g.N = N; g.K = K; g.a_rpb = (int)rows; g.a_rstride = K; g.ldw = K; g.ldc = N; g.out_f32 = out_f32; g.act = act;
    return launch_gemm(r->gp, g, s);
  };
  auto layer = [&](const RcaLayerW& L, const void* kvT, const float* kvF, const void* qT, float* outF, const RcaSave* S) -> int {
    void* qkv = S ? S->qkv : w.qkv;
    void* qc = S ? S->qc : w.qc;
    void* att_s = S ? S->att_s : w.att_s;
    void* att_c = S ? S->att_c : w.att_c;
    void* blend = S ? S->blend : w.blend;
    float* pre1 = S ? S->pre1 : w.preF;
    float* pre2 = S ? S->pre2 : w.preF;
    void* xT = S ? S->xT : w.xT;
    float* xF = S ? S->xF : w.xF;
    void* ffn = S ? S->ffn : w.ffn;
    // one packed in-projection of the kv stream gives the self-attention q, and k, v for BOTH attentions
    if (int rc = gemm_rows(kvT, D, L.win.p, L.bin.as<float>(), 3 * D, qkv, 0, ACT_NONE, nullptr)) return rc;
    if (int rc = gemm_rows(qT, D, L.win.p, L.bin.as<float>(), D, qc, 0, ACT_NONE, nullptr)) return rc;
    const char* kp = (const char*)qkv + (size_t)D * es;
    const char* vp = (const char*)qkv + (size_t)2 * D * es;
    AttnArgs a;
    a.prec = prec; a.gp = r->gp; a.Q = qkv; a.K = kp; a.V = vp; a.ldq = a.ldkv = 3L * D; a.out = att_s; a.ldo = D;
    a.B = B; a.T = T; a.H = H; a.dh = dh; a.scale = scale;
    if (int rc = launch_attention(a, w.ab, s)) return rc;
    a.Q = qc; a.ldq = D; a.out = att_c; a.kv_ready = true;   // cross attention: the same k, v
    if (int rc = launch_attention(a, w.ab, s)) return rc;
    // out_proj is linear: alpha*Wo(a_s) + (1-alpha)*Wo(a_c) + bo = Wo(alpha*a_s + (1-alpha)*a_c) + bo
    if (int rc = launch_axpby(prec, att_s, att_c, r->alpha, 1.f - r->alpha, blend, rows * D, s)) return rc;
    if (int rc = gemm_rows(blend, D, L.wo.p, L.bo.as<float>(), D, pre1, 1, ACT_NONE, nullptr)) return rc;
    LnArgs n1;   // x = LN(kv + attention branch): operand copy for FFN-1 (+ the fp32 value where that copy is 16-bit)
    n1.prec = prec; n1.x = pre1; n1.add = kvF; n1.rows = rows; n1.D = D; n1.gamma = L.n1g.as<float>(); n1.beta = L.n1b.as<float>(); n1.eps = 1e-6f;
    n1.yT = xT; n1.yF = prec ? xF : nullptr;
    if (int rc = launch_layernorm(n1, s)) return rc;
    if (int rc = gemm_rows(xT, D, L.w1.p, L.b1.as<float>(), F, ffn, 0, ACT_RELU, nullptr)) return rc;
    if (int rc = gemm_rows(ffn, F, L.w2.p, L.b2.as<float>(), D, pre2, 1, ACT_NONE, nullptr)) return rc;
    LnArgs n2;   // out = LN(x + FFN branch), fp32
    n2.x = pre2; n2.add = xF; n2.rows = rows; n2.D = D; n2.gamma = L.n2g.as<float>(); n2.beta = L.n2b.as<float>(); n2.eps = 1e-6f; n2.yT = outF;
    if (int rc = launch_layernorm(n2, s)) return rc;
    if (S) {
      const size_t bht = (size_t)B * H * T;
      if (int rc = launch_rca_attn_lse(prec, qkv, 3L * D, kp, 3L * D, B, T, H, dh, scale, S->lse, s)) return rc;
      if (int rc = launch_rca_attn_lse(prec, qc, D, kp, 3L * D, B, T, H, dh, scale, S->lse + bht, s)) return rc;
    }
    return 0;
  };
  if (int rc = layer(r->L[0], w.s1T, w.s1F, w.s2T, w.o1, save ? &save[0] : nullptr)) return rc;
  if (int rc = layer(r->L[1], w.s2T, w.s2F, w.s1T, w.o2, save ? &save[1] : nullptr)) return rc;
  return launch_add_f32(w.o1, w.o2, out, rows * D, s);
}
}  // namespace

extern "C" {

int svt_rca_create(int32_t d_model, int32_t nhead, int32_t d_ffn, float alpha, int32_t max_len, int32_t precision,
                   int device, svt_rca** out) {
  if (!out || d_model < 8 || nhead < 1 || d_model % nhead || (d_model / nhead) % 8 || d_ffn % 8 || d_model % 8) {
    set_error("svt_rca_create: bad geometry");
    return SVT_ERR_INVALID;
  }
  if (!valid_precision(precision)) { set_error("svt_rca_create: precision"); return SVT_ERR_INVALID; }
  if (int r = check_device(device)) return r;
  svt_rca* r = new svt_rca();
  r->D = d_model; r->H = nhead; r->F = d_ffn; r->alpha = alpha; r->max_len = max_len; r->prec = storage_prec(precision); r->gp = precision; r->device = device;
  *out = r;
  return SVT_OK;
}
void svt_rca_destroy(svt_rca* r) {
  if (!r) return;
  (void)hipSetDevice(r->device);
  delete r;
}
int svt_rca_load_param(svt_rca* r, const char* key, const void* data_host, int dtype, const int64_t* shape, int ndim) {
  if (!r) { set_error("null rca"); return SVT_ERR_INVALID; }
  r->finalized = false;
  return load_param_into(r->params, key, data_host, dtype, shape, ndim);
}
int svt_rca_finalize(svt_rca* r) {
  if (!r) { set_error("null rca"); return SVT_ERR_INVALID; }
  SVT_HIP(hipSetDevice(r->device));
  if (int rc = begin_upload(r->uploaded)) return rc;
  r->transposed = false;   // the transposed copies are the old weights' until the next svt_rca_refresh_params
  const ParamMap& P = r->params;
  const Param* p = nullptr;
  const int D = r->D, F = r->F;
  if (int rc = need(P, "fusion.positional_encoding.pe", {1, r->max_len, D}, &p)) return rc;
  if (int rc = upload_f32(r->pe, p->v.data(), p->v.size())) return rc;
  for (int l = 0; l < 2; ++l) {
    const std::string pre = std::string("fusion.layer") + (l ? "2" : "1") + ".";
    RcaLayerW& L = r->L[l];
    if (int rc = need(P, pre + "self_att.att.in_proj_weight", {3 * D, D}, &p)) return rc;
    if (int rc = upload_weight(r->gp, L.win, p->v.data(), (size_t)3 * D, (size_t)D)) return rc;
    if (int rc = need(P, pre + "self_att.att.in_proj_bias", {3 * D}, &p)) return rc;
    if (int rc = upload_f32(L.bin, p->v.data(), p->v.size())) return rc;
    if (int rc = need(P, pre + "self_att.att.out_proj.weight", {D, D}, &p)) return rc;
    if (int rc = upload_weight(r->gp, L.wo, p->v.data(), (size_t)D, (size_t)D)) return rc;
    if (int rc = need(P, pre + "self_att.att.out_proj.bias", {D}, &p)) return rc;
    if (int rc = upload_f32(L.bo, p->v.data(), p->v.size())) return rc;
    if (int rc = need(P, pre + "pos_ffn.ffn.0.weight", {F, D}, &p)) return rc;
    if (int rc = upload_weight(r->gp, L.w1, p->v.data(), (size_t)F, (size_t)D)) return rc;
    if (int rc = need(P, pre + "pos_ffn.ffn.0.bias", {F}, &p)) return rc;
    if (int rc = upload_f32(L.b1, p->v.data(), p->v.size())) return rc;
    if (int rc = need(P, pre + "pos_ffn.ffn.3.weight", {D, F}, &p)) return rc;
    if (int rc = upload_weight(r->gp, L.w2, p->v.data(), (size_t)D, (size_t)F)) return rc;
    if (int rc = need(P, pre + "pos_ffn.ffn.3.bias", {D}, &p)) return rc;
    if (int rc = upload_f32(L.b2, p->v.data(), p->v.size())) return rc;
    if (int rc = need(P, pre + "norm1.norm.weight", {D}, &p)) return rc;
    if (int rc = upload_f32(L.n1g, p->v.data(), p->v.size())) return rc;
    if (int rc = need(P, pre + "norm1.norm.bias", {D}, &p)) return rc;
    if (int rc = upload_f32(L.n1b, p->v.data(), p->v.size())) return rc;
    if (int rc = need(P, pre + "norm2.norm.weight", {D}, &p)) return rc;
    if (int rc = upload_f32(L.n2g, p->v.data(), p->v.size())) return rc;
    if (int rc = need(P, pre + "norm2.norm.bias", {D}, &p)) return rc;
    if (int rc = upload_f32(L.n2b, p->v.data(), p->v.size())) return rc;
  }
  SVT_HIP(hipDeviceSynchronize());
  r->finalized = true;
  return SVT_OK;
}
int64_t svt_rca_workspace_bytes(const svt_rca* r, int32_t batch, int32_t t_audio) {
  if (!r || batch < 1 || t_audio < 1) { set_error("svt_rca_workspace_bytes: bad argument"); return -1; }
  return (int64_t)carve_rca(r, batch, t_audio, nullptr).total;
}

int svt_rca_forward(svt_rca* r, const float* audio, int32_t T1, const float* video, int32_t T2, int32_t B, float* out,
                    void* workspace, size_t workspace_bytes, void* stream) {
  if (!r || !audio || !video || !out || !workspace) { set_error("svt_rca_forward: null argument"); return SVT_ERR_INVALID; }
  if (int rc = rca_check_call("svt_rca_forward", r, B, T1, T2)) return rc;
  RcaWs w = carve_rca(r, B, T1, workspace);
  if (w.total > workspace_bytes) { set_error("svt_rca_forward: workspace too small"); return SVT_ERR_WORKSPACE; }
  SVT_HIP(hipSetDevice(r->device));
  return rca_forward_run(r, audio, T1, video, T2, B, out, w, nullptr, (hipStream_t)stream);
}

// ---- training step of FusionRCA (train_rca_av.py:174-185) ----
static int rca_train_ok(const char* who, const svt_rca* r) {
  if (r->gp != SVT_PREC_FP32 && r->gp != SVT_PREC_BF16) {
    set_error(std::string(who) + ": training takes precision fp32 or bf16"); return SVT_ERR_INVALID;
  }
#ifdef SVT_OPERAND_F16
  set_error(std::string(who) + ": training takes precision fp32 or bf16 (not the IEEE-half build)"); return SVT_ERR_INVALID;
#endif
  const int dh = r->D / r->H;
  if (dh != 64 && dh != 128) { set_error(std::string(who) + ": training takes head sizes 64 and 128"); return SVT_ERR_INVALID; }
  return SVT_OK;
}

int svt_rca_refresh_params(svt_rca* r, const float* const* params, int32_t n, void* stream) {
  const char* who = "svt_rca_refresh_params";
  if (!r || !params) { set_error(std::string(who) + ": null argument"); return SVT_ERR_INVALID; }
  if (n != 24) { set_error(std::string(who) + ": expected the 24 fusion tensors"); return SVT_ERR_INVALID; }
  if (!r->finalized) { set_error(std::string(who) + ": parameters not finalized"); return SVT_ERR_STATE; }
  if (int rc = rca_train_ok(who, r)) return rc;
  for (int i = 0; i < 24; ++i)
    if (!params[i]) { set_error(std::string(who) + ": null tensor pointer"); return SVT_ERR_INVALID; }
  SVT_HIP(hipSetDevice(r->device));
  const int64_t D = r->D, F = r->F;
  const size_t es = esize(r->prec);
  RcaRefreshJobs jobs{};
  auto job = [&](const float* src, void* dst, int64_t rows, int64_t cols, int tr, int f32) {
    jobs.j[jobs.n++] = RcaRefreshJob{src, dst, rows, cols, tr, f32};
  };
  for (int l = 0; l < 2; ++l) {
    RcaLayerW& L = r->L[l];
    const float* const* p = params + 12 * l;
    if (int rc = L.woT.alloc((size_t)D * D * es)) return rc;
    if (int rc = L.w1T.alloc((size_t)D * F * es)) return rc;
    if (int rc = L.w2T.alloc((size_t)D * F * es)) return rc;
    job(p[0], L.win.p, 3 * D, D, 0, 0);
    job(p[1], L.bin.p, 1, 3 * D, 0, 1);
    job(p[2], L.wo.p, D, D, 0, 0);
    job(p[2], L.woT.p, D, D, 1, 0);
    job(p[3], L.bo.p, 1, D, 0, 1);
    job(p[4], L.w1.p, F, D, 0, 0);
    job(p[4], L.w1T.p, F, D, 1, 0);
    job(p[5], L.b1.p, 1, F, 0, 1);
    job(p[6], L.w2.p, D, F, 0, 0);
    job(p[6], L.w2T.p, D, F, 1, 0);
    job(p[7], L.b2.p, 1, D, 0, 1);
    job(p[8], L.n1g.p, 1, D, 0, 1);
    job(p[9], L.n1b.p, 1, D, 0, 1);
    job(p[10], L.n2g.p, 1, D, 0, 1);
    job(p[11], L.n2b.p, 1, D, 0, 1);
  }
  if (launch_rca_refresh(r->prec, jobs, (hipStream_t)stream)) return SVT_ERR_HIP;
  r->transposed = true;
  return SVT_OK;
}

int64_t svt_rca_train_workspace_bytes(const svt_rca* r, int32_t batch, int32_t t_audio) {
  if (!r || batch < 1 || t_audio < 1) { set_error("svt_rca_train_workspace_bytes: bad argument"); return -1; }
  return (int64_t)carve_rca_train(r, batch, t_audio, nullptr).total;
}

int svt_rca_forward_train(svt_rca* r, const float* audio, int32_t T1, const float* video, int32_t T2, int32_t B, float* out,
                          void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "svt_rca_forward_train";
  if (!r || !audio || !video || !out || !workspace) { set_error(std::string(who) + ": null argument"); return SVT_ERR_INVALID; }
  if (int rc = rca_check_call(who, r, B, T1, T2)) return rc;
  if (int rc = rca_train_ok(who, r)) return rc;
  RcaTrainWs w = carve_rca_train(r, B, T1, workspace);
  if (w.total > workspace_bytes) { set_error(std::string(who) + ": workspace too small"); return SVT_ERR_WORKSPACE; }
  SVT_HIP(hipSetDevice(r->device));
  return rca_forward_run(r, audio, T1, video, T2, B, out, w.f, w.L, (hipStream_t)stream);
}

int svt_rca_backward(svt_rca* r, const float* dout, int32_t B, int32_t T1, float* const* grads, void* workspace, size_t workspace_bytes,
                     void* stream) {
  const char* who = "svt_rca_backward";
  if (!r || !dout || !grads || !workspace) { set_error(std::string(who) + ": null argument"); return SVT_ERR_INVALID; }
  if (int rc = rca_check_call(who, r, B, T1, 1)) return rc;
  if (int rc = rca_train_ok(who, r)) return rc;
  if (!r->transposed) { set_error(std::string(who) + ": call svt_rca_refresh_params after svt_rca_finalize"); return SVT_ERR_STATE; }
  for (int i = 0; i < 24; ++i)
    if (!grads[i]) { set_error(std::string(who) + ": null gradient pointer"); return SVT_ERR_INVALID; }
  RcaTrainWs w = carve_rca_train(r, B, T1, workspace);
  if (w.total > workspace_bytes) { set_error(std::string(who) + ": workspace too small"); return SVT_ERR_WORKSPACE; }
  hipStream_t s = (hipStream_t)stream;
  SVT_HIP(hipSetDevice(r->device));
  const int prec = r->prec, D = r->D, H = r->H, F = r->F, dh = D / H, T = T1;
  const int64_t rows = (int64_t)B * T;
  const float scale = 1.0f / std::sqrt((float)dh);
  const RcaBwdWs& b = w.b;
  auto dx_gemm = [&](const void* A, int K, const void* Wt, int N, float* C, const float* resid) -> int {
    GemmArgs g;
    g.A = A; g.W = Wt; g.C = C; g.resid = resid;
    g.M = (int)rows; g.N = N; g.K = K; g.a_rpb = (int)rows; g.a_rstride = K; g.ldw = K; g.ldc = N; g.out_f32 = 1; g.act = ACT_NONE;
    return launch_gemm(r->gp, g, s);
  };
  auto wgrad = [&](const float* dy0, long ldy0, const void* x0, const float* dy1, const void* x1, int N, int C, float* dw, float* db) -> int {
    RcaWgrad a;
    a.dy[0] = dy0; a.dy[1] = dy1; a.x[0] = x0; a.x[1] = x1;
    a.ldy[0] = ldy0; a.ldy[1] = ldy0; a.ldx[0] = C; a.ldx[1] = C;
    a.nseg = dy1 ? 2 : 1; a.rows = rows; a.N = N; a.C = C;
    return launch_rca_wgrad(prec, a, dw, db, b.wg_scr, s);
  };
  for (int l = 0; l < 2; ++l) {
    const RcaLayerW& L = r->L[l];
    const RcaSave& S = w.L[l];
    float* const* g = grads + 12 * l;
    const void* kvT = l ? w.f.s2T : w.f.s1T;
    const float* kvF = l ? w.f.s2F : w.f.s1F;
    const void* qT = l ? w.f.s1T : w.f.s2T;
    // LN2: y2 = pre2 + x; both layers receive d(feats) (feats = o1 + o2)
    void* dy2T = prec ? b.dyT : (void*)b.dy2F;
    if (int rc = launch_rca_ln_bwd(prec, S.pre2, S.xF, L.n2g.as<float>(), dout, rows, D, 1e-6f, b.dy2F, prec ? b.dyT : nullptr, g[10], g[11],
                                   b.ln_scr, s)) return rc;
    // FFN: dW2 = dy2^T h, db2; dh = dy2 W2, masked by the ReLU; dW1 = dh^T x, db1; dx = dh W1 + dy2 (the residual)
    if (int rc = wgrad(b.dy2F, D, S.ffn, nullptr, nullptr, D, F, g[6], g[7])) return rc;
    if (int rc = dx_gemm(dy2T, D, L.w2T.p, F, b.dhF, nullptr)) return rc;
    if (int rc = launch_rca_relu_mask(prec, b.dhF, S.ffn, rows * F, b.dhT, s)) return rc;
    if (int rc = wgrad(b.dhF, F, S.xT, nullptr, nullptr, F, D, g[4], g[5])) return rc;
    if (int rc = dx_gemm(prec ? b.dhT : (void*)b.dhF, F, L.w1T.p, D, b.dxF, b.dy2F)) return rc;
    // LN1: y1 = pre1 + kv (the kv stream is data: no gradient past it)
    if (int rc = launch_rca_ln_bwd(prec, S.pre1, kvF, L.n1g.as<float>(), b.dxF, rows, D, 1e-6f, b.dy1F, prec ? b.dyT : nullptr, g[8], g[9],
                                   b.ln_scr, s)) return rc;
    if (int rc = wgrad(b.dy1F, D, S.blend, nullptr, nullptr, D, D, g[2], g[3])) return rc;
    if (int rc = dx_gemm(prec ? b.dyT : (void*)b.dy1F, D, L.woT.p, D, b.dblF, nullptr)) return rc;
    // the two attentions (d a_s = alpha d blend, d a_c = (1 - alpha) d blend) -> dQ_s, dK, dV into dqkv, dQ_c into dqc
    const size_t es = esize(prec);
    RcaAttnBwd a;
    a.q[0] = S.qkv; a.q[1] = S.qc; a.k = (const char*)S.qkv + (size_t)D * es; a.v = (const char*)S.qkv + (size_t)2 * D * es;
    a.o[0] = S.att_s; a.o[1] = S.att_c;
    a.ldq[0] = 3L * D; a.ldq[1] = D; a.ldkv = 3L * D;
    a.dbl = b.dblF; a.coef[0] = r->alpha; a.coef[1] = 1.f - r->alpha;
    a.lse = S.lse; a.delta = b.delta;
    a.dq[0] = b.dqkv; a.dq[1] = b.dqc; a.lddq[0] = 3L * D; a.lddq[1] = D;
    a.dk = b.dqkv + D; a.dv = b.dqkv + 2 * D; a.lddkv = 3L * D;
    a.B = B; a.T = T; a.H = H; a.dh = dh; a.scale = scale;
    if (int rc = launch_rca_attn_bwd(prec, a, s)) return rc;
    // in_proj: rows [0, D) from both query streams ([dQ_s | dQ_c]^T [kv ; q]), rows [D, 3D) from the kv stream
    float* dwin = g[0];
    float* dbin = g[1];
    {
      RcaWgrad q;
      q.dy[0] = b.dqkv; q.dy[1] = b.dqc; q.x[0] = kvT; q.x[1] = qT;
      q.ldy[0] = 3L * D; q.ldy[1] = D; q.ldx[0] = D; q.ldx[1] = D;
      q.nseg = 2; q.rows = rows; q.N = D; q.C = D;
      if (int rc = launch_rca_wgrad(prec, q, dwin, dbin, b.wg_scr, s)) return rc;
    }
    if (int rc = wgrad(b.dqkv + D, 3L * D, kvT, nullptr, nullptr, 2 * D, D, dwin + (size_t)D * D, dbin + D)) return rc;
  }
  return SVT_OK;
}

// the RCA training kernels alone, for the unit tests (operand type by precision: 0 fp32, 1 bf16)
int svt_debug_rca_wgrad(int32_t precision, const float* dy0, int64_t ldy0, const void* x0, const float* dy1, int64_t ldy1, const void* x1,
                        int64_t rows, int32_t n_out, int32_t n_in, float* dw, float* db, void* workspace, size_t* workspace_bytes, int device,
                        void* stream) {
  const char* who = "svt_debug_rca_wgrad";
  if ((precision != SVT_PREC_FP32 && precision != SVT_PREC_BF16) || rows < 1 || n_out < 1 || n_in < 1) {
    set_error(std::string(who) + ": bad argument"); return SVT_ERR_INVALID;
  }
  const int nseg = dy1 ? 2 : 1;
  bool query = false;
  if (int r = ws_query(who, workspace, workspace_bytes, std::max<size_t>(16, rca_wgrad_scratch_bytes(rows * nseg, n_out, n_in)), &query)) return r;
  if (query) return SVT_OK;
  if (!dy0 || !x0 || !dw || (dy1 && !x1)) { set_error(std::string(who) + ": null argument"); return SVT_ERR_INVALID; }
  if (int r = check_device(device)) return r;
  SVT_HIP(hipSetDevice(device));
  RcaWgrad a;
  a.dy[0] = dy0; a.dy[1] = dy1; a.x[0] = x0; a.x[1] = x1; a.ldy[0] = ldy0; a.ldy[1] = ldy1; a.ldx[0] = n_in; a.ldx[1] = n_in;
  a.nseg = nseg; a.rows = rows; a.N = n_out; a.C = n_in;
  if (launch_rca_wgrad(precision, a, dw, db, workspace, (hipStream_t)stream)) return SVT_ERR_HIP;
  return SVT_OK;
}

int svt_debug_rca_attn_bwd(int32_t precision, const void* qkv, const void* qc, const void* o_self, const void* o_cross, const float* dblend,
                           float alpha, int32_t batch, int32_t t, int32_t heads, int32_t head_dim, float* dqkv, float* dqc, void* workspace,
                           size_t* workspace_bytes, int device, void* stream) {
  const char* who = "svt_debug_rca_attn_bwd";
  if ((precision != SVT_PREC_FP32 && precision != SVT_PREC_BF16) || batch < 1 || t < 1 || heads < 1 || (head_dim != 64 && head_dim != 128)) {
    set_error(std::string(who) + ": bad argument"); return SVT_ERR_INVALID;
  }
  const size_t bht = (size_t)batch * heads * t;
  bool query = false;
  if (int r = ws_query(who, workspace, workspace_bytes, 4 * bht * sizeof(float), &query)) return r;
  if (query) return SVT_OK;
  if (!qkv || !qc || !o_self || !o_cross || !dblend || !dqkv || !dqc) { set_error(std::string(who) + ": null argument"); return SVT_ERR_INVALID; }
  if (int r = check_device(device)) return r;
  SVT_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  const long D = (long)heads * head_dim;
  const size_t es = precision ? 2 : 4;
  const float scale = 1.0f / std::sqrt((float)head_dim);
  float* lse = (float*)workspace;
  const void* kp = (const char*)qkv + D * es;
  if (launch_rca_attn_lse(precision, qkv, 3 * D, kp, 3 * D, batch, t, heads, head_dim, scale, lse, s)) return SVT_ERR_HIP;
  if (launch_rca_attn_lse(precision, qc, D, kp, 3 * D, batch, t, heads, head_dim, scale, lse + bht, s)) return SVT_ERR_HIP;
  RcaAttnBwd a;
  a.q[0] = qkv; a.q[1] = qc; a.k = kp; a.v = (const char*)qkv + 2 * D * es; a.o[0] = o_self; a.o[1] = o_cross;
  a.ldq[0] = 3 * D; a.ldq[1] = D; a.ldkv = 3 * D; a.dbl = dblend; a.coef[0] = alpha; a.coef[1] = 1.f - alpha;
  a.lse = lse; a.delta = lse + 2 * bht; a.dq[0] = dqkv; a.dq[1] = dqc; a.lddq[0] = 3 * D; a.lddq[1] = D;
  a.dk = dqkv + D; a.dv = dqkv + 2 * D; a.lddkv = 3 * D; a.B = batch; a.T = t; a.H = heads; a.dh = head_dim; a.scale = scale;
  if (launch_rca_attn_bwd(precision, a, s)) return SVT_ERR_HIP;
  return SVT_OK;
}

}  // extern "C"
