// C ABI of the encoder (include/svt_mi355.h): parameter intake by HF key, the one-time re-layout / fold / cast at finalize, workspace
// carving and the launch sequence of a forward, with or without the fused frame-head tail.  Host code only: no allocation and no
// synchronisation inside a forward call.
#include "../../include/svt_mi355.h"
#include "api.h"
#include "common.h"
#include "host.h"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

using namespace svt;

int svt::g_conv_ln_bf16 = 1;     // svt_debug_set(9, 0): fp32 conv output + LayerNorm (A/B)

struct ConvLayerW {
  DevBuf w;      // layer 0: fp32 (C,k); others: operand type (Cout, k*Cin) tap-major
  DevBuf w_kperm;   // 16-bit modes, kernel 3 / stride 2: the same matrix with its K axis in tap-minor slab order (svt_encoder_finalize)
  DevBuf bias;   // fp32 or empty
  DevBuf gamma, beta;
};
struct EncLayerW {
  DevBuf wqkv, bqkv, wo, bo, ln1g, ln1b, w1, b1, w2, b2, ln2g, ln2b;
  DevBuf g_wab, g_bab, g_const;   // WavLM gate: folded gru_rel_pos_linear (2 x dh, 2) and gru_rel_pos_const (H)
};

struct svt_encoder {
  svt_encoder_config cfg;
  int device = 0;
  bool finalized = false;
  bool uploaded = false;   // device buffers exist: the next finalize is a RE-upload into live buffers
  ParamMap params;
  std::vector<ConvLayerW> conv;
  DevBuf fp_g, fp_b, proj_w, proj_b, pos_w, pos_b, enc_g, enc_b;
  DevBuf pos_bn_sc, pos_bn_sh;  // HuBERT conv_pos_batch_norm: eval-mode BatchNorm1d folded to a per-channel affine (fp32)
  DevBuf pos_wP, pos_bP;   // multi-frame form of the positional conv (bf16 mode): P frames per GEMM row
  int pos_P = 0;
  std::vector<DevBuf> pos_ws, pos_bs;   // data2vec-audio: one plain grouped conv per stacked positional layer
  DevBuf rel_embed;                     // WavLM: (buckets, H) relative position embedding of layer 0
  DevBuf ones, zeros;                   // LayerNorm without affine parameters
  std::vector<EncLayerW> layers;
  // optional cross-rank reduction of the wrapper's two whole-batch norm statistics (svt_encoder_set_norm_reduce)
  svt_norm_reduce_fn reduce_fn = nullptr;
  void* reduce_user = nullptr;
  int64_t reduce_global_clips = 0;
};

extern "C" {

int svt_encoder_create(const svt_encoder_config* cfg, int device, svt_encoder** out) {
  if (!cfg || !out) { set_error("svt_encoder_create: null argument"); return SVT_ERR_INVALID; }
  if (int r = validate_cfg(*cfg)) return r;
  if (int r = check_device(device)) return r;
  svt_encoder* e = new svt_encoder();
  e->cfg = *cfg;
  e->device = device;
  *out = e;
  return SVT_OK;
}

void svt_encoder_destroy(svt_encoder* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  delete e;
}

int svt_encoder_set_norm_reduce(svt_encoder* e, svt_norm_reduce_fn fn, void* user, int64_t global_clips) {
  if (!e) { set_error("svt_encoder_set_norm_reduce: null encoder"); return SVT_ERR_INVALID; }
  if (fn && global_clips < 1) { set_error("svt_encoder_set_norm_reduce: global_clips must be the clip count of the whole global batch"); return SVT_ERR_INVALID; }
  e->reduce_fn = fn;
  e->reduce_user = user;
  e->reduce_global_clips = fn ? global_clips : 0;
  return SVT_OK;
}

int svt_encoder_load_param(svt_encoder* e, const char* key, const void* data_host, int dtype, const int64_t* shape,
                           int ndim) {
  if (!e) { set_error("null encoder"); return SVT_ERR_INVALID; }
  e->finalized = false;
  return load_param_into(e->params, key, data_host, dtype, shape, ndim);
}

int svt_encoder_get_param(svt_encoder* e, const char* key, void* out_host, int64_t capacity_elems) {
  if (!e || !key || !out_host) { set_error("get_param: null argument"); return SVT_ERR_INVALID; }
  const Param* p = find(e->params, key);
  if (!p) { set_error(std::string("unknown parameter: ") + key); return SVT_ERR_KEY; }
  if ((int64_t)p->v.size() > capacity_elems) { set_error("get_param: buffer too small"); return SVT_ERR_INVALID; }
  memcpy(out_host, p->v.data(), p->v.size() * 4);
  return SVT_OK;
}

int svt_encoder_finalize(svt_encoder* e) {
  if (!e) { set_error("null encoder"); return SVT_ERR_INVALID; }
  SVT_HIP(hipSetDevice(e->device));
  if (int r = begin_upload(e->uploaded)) return r;
  const svt_encoder_config& c = e->cfg;
  const int prec = storage_prec(c.precision);
  const ParamMap& P = e->params;
  const Param* p = nullptr;
  if ((int)e->conv.size() != c.num_conv_layers) { e->conv.clear(); e->conv.resize(c.num_conv_layers); }   // a re-upload keeps the buffers
  int cin = c.num_conv_layers == 0 ? c.conv_dim[0] : 1;  // features-in mode: the projection reads the given features
  for (int i = 0; i < c.num_conv_layers; ++i) {
    const std::string pre = "feature_extractor.conv_layers." + std::to_string(i) + ".";
    const int co = c.conv_dim[i], k = c.conv_kernel[i];
    if (int r = need(P, pre + "conv.weight", {co, cin, k}, &p)) return r;
    ConvLayerW& L = e->conv[i];
    if (i == 0) {
      if (int r = upload_f32(L.w, p->v.data(), p->v.size())) return r;
    } else {
      // (Cout, Cin, k) -> (Cout, k*Cin) tap-major: the implicit-GEMM row of output frame t is the
      // contiguous channels-last slice x[t*s : t*s+k, :]
      std::vector<float> wt((size_t)co * k * cin);
      for (int o = 0; o < co; ++o)
        for (int ci = 0; ci < cin; ++ci)
          for (int j = 0; j < k; ++j) wt[((size_t)o * k + j) * cin + ci] = p->v[((size_t)o * cin + ci) * k + j];
      if (int r = upload_weight(c.precision, L.w, wt.data(), (size_t)co, (size_t)k * cin)) return r;
      // 16-bit modes, kernel 3: a second copy with the K axis in TAP-MINOR slab order -- slab g = tap g % 3 of channels [(g / 3) * 64, + 64)
      // -- for gemm_p1w_kernel (GemmArgs::k_taps): the input frame two neighbouring output rows share is re-read two slabs later instead
      // of sixteen, i.e. out of L2 (1.5 MiB per layer)
      if (prec && k == 3 && cin % 64 == 0 && c.conv_stride[i] == 2) {
        std::vector<float> wp((size_t)co * k * cin);
        const int nb = cin / 64;
        for (int o = 0; o < co; ++o)
          for (int cb = 0; cb < nb; ++cb)
            for (int j = 0; j < k; ++j)
              memcpy(&wp[((size_t)o * k * nb + (size_t)cb * k + j) * 64], &wt[((size_t)o * k + j) * cin + (size_t)cb * 64], 64 * sizeof(float));
        if (int r = upload_weight(c.precision, L.w_kperm, wp.data(), (size_t)co, (size_t)k * cin)) return r;
      } else L.w_kperm.release();
    }
    if (c.conv_bias) {
      if (int r = need(P, pre + "conv.bias", {co}, &p)) return r;
      if (int r = upload_f32(L.bias, p->v.data(), p->v.size())) return r;
    }
    const bool has_norm = c.feat_extract_norm == SVT_NORM_LAYER || i == 0;
    if (has_norm) {
      if (int r = need(P, pre + "layer_norm.weight", {co}, &p)) return r;
      if (int r = upload_f32(L.gamma, p->v.data(), p->v.size())) return r;
      if (int r = need(P, pre + "layer_norm.bias", {co}, &p)) return r;
      if (int r = upload_f32(L.beta, p->v.data(), p->v.size())) return r;
    }
    cin = co;
  }
  const int D = c.hidden_size, F = c.intermediate_size;
  if (c.feat_proj_layer_norm) {
    if (int r = need(P, "feature_projection.layer_norm.weight", {cin}, &p)) return r;
    if (int r = upload_f32(e->fp_g, p->v.data(), p->v.size())) return r;
    if (int r = need(P, "feature_projection.layer_norm.bias", {cin}, &p)) return r;
    if (int r = upload_f32(e->fp_b, p->v.data(), p->v.size())) return r;
  }
  if (int r = need(P, "feature_projection.projection.weight", {D, cin}, &p)) return r;
  if (int r = upload_weight(c.precision, e->proj_w, p->v.data(), (size_t)D, (size_t)cin)) return r;
  if (int r = need(P, "feature_projection.projection.bias", {D}, &p)) return r;
  if (int r = upload_f32(e->proj_b, p->v.data(), p->v.size())) return r;

  if (c.pos_conv_depth > 1) {
    // data2vec-audio: plain grouped convs "encoder.pos_conv_embed.layers.<i>.conv.{weight,bias}", (D, cg, kp) -> per group
    // (cg_out, kp*cg_in) tap-major like the single-layer form
    const int kp = c.pos_conv_kernel, G = c.pos_conv_groups, cg = D / G;
    if ((int)e->pos_ws.size() != c.pos_conv_depth) { e->pos_ws.clear(); e->pos_bs.clear(); e->pos_ws.resize(c.pos_conv_depth); e->pos_bs.resize(c.pos_conv_depth); }
    for (int i = 0; i < c.pos_conv_depth; ++i) {
      const std::string pl = "encoder.pos_conv_embed.layers." + std::to_string(i) + ".conv.";
      if (int r = need(P, pl + "weight", {D, cg, kp}, &p)) return r;
      std::vector<float> wt(p->v.size());
      for (int o = 0; o < D; ++o)
        for (int ci = 0; ci < cg; ++ci)
          for (int j = 0; j < kp; ++j) wt[((size_t)o * kp + j) * cg + ci] = p->v[((size_t)o * cg + ci) * kp + j];
      if (int r = upload_operand(prec, e->pos_ws[i], wt.data(), wt.size())) return r;
      if (int r = need(P, pl + "bias", {D}, &p)) return r;
      if (int r = upload_f32(e->pos_bs[i], p->v.data(), p->v.size())) return r;
    }
    std::vector<float> one((size_t)D, 1.f), zero((size_t)D, 0.f);
    if (int r = upload_f32(e->ones, one.data(), one.size())) return r;
    if (int r = upload_f32(e->zeros, zero.data(), zero.size())) return r;
    e->pos_P = 0;
  } else
  // positional conv: fold weight-norm (dim=2): W[:,:,j] = g[j] v[:,:,j] / ||v[:,:,j]||_F ; accept both spellings
  {
    const int kp = c.pos_conv_kernel, G = c.pos_conv_groups, cg = D / G;
    const std::string pc = "encoder.pos_conv_embed.conv.";
    std::vector<float> w((size_t)D * cg * kp);
    const Param *g = find(P, pc + "parametrizations.weight.original0"), *v = find(P, pc + "parametrizations.weight.original1");
    if (!g || !v) { g = find(P, pc + "weight_g"); v = find(P, pc + "weight_v"); }
    if (g && v) {
      if (g->numel() != kp || v->shape != std::vector<int64_t>({D, cg, kp})) { set_error("pos_conv weight-norm tensors have the wrong shape"); return SVT_ERR_INVALID; }
      std::vector<double> nrm(kp, 0.0);
      for (size_t i = 0; i < v->v.size(); ++i) nrm[i % kp] += (double)v->v[i] * (double)v->v[i];
      for (int j = 0; j < kp; ++j) nrm[j] = std::sqrt(nrm[j]);
      for (size_t i = 0; i < v->v.size(); ++i) w[i] = (float)((double)g->v[i % kp] * (double)v->v[i] / nrm[i % kp]);
    } else if (const Param* pw = find(P, pc + "weight")) {
      if (pw->shape != std::vector<int64_t>({D, cg, kp})) { set_error("pos_conv weight has the wrong shape"); return SVT_ERR_INVALID; }
      w = pw->v;
    } else {
      set_error("missing parameter: " + pc + "parametrizations.weight.original0/1 (or weight_g/weight_v)");
      return SVT_ERR_KEY;
    }
    // (D, cg, kp) -> per group (cg_out, kp*cg_in) tap-major
    std::vector<float> wt(w.size());
    for (int o = 0; o < D; ++o)
      for (int ci = 0; ci < cg; ++ci)
        for (int j = 0; j < kp; ++j) wt[((size_t)o * kp + j) * cg + ci] = w[((size_t)o * cg + ci) * kp + j];
    if (int r = upload_operand(prec, e->pos_w, wt.data(), wt.size())) return r;
    if (int r = need(P, pc + "bias", {D}, &p)) return r;
    if (int r = upload_f32(e->pos_b, p->v.data(), p->v.size())) return r;
    if (c.pos_conv_batch_norm) {
      // y = (x - running_mean) / sqrt(running_var + 1e-5) * weight + bias   (nn.BatchNorm1d defaults, eval mode)
      const std::string bn = "encoder.pos_conv_embed.batch_norm.";
      const Param *bw, *bb, *bm, *bv;
      if (int r = need(P, bn + "weight", {D}, &bw)) return r;
      if (int r = need(P, bn + "bias", {D}, &bb)) return r;
      if (int r = need(P, bn + "running_mean", {D}, &bm)) return r;
      if (int r = need(P, bn + "running_var", {D}, &bv)) return r;
      std::vector<float> sc(D), sh(D);
      for (int i = 0; i < D; ++i) {
        const double k = (double)bw->v[i] / std::sqrt((double)bv->v[i] + 1e-5);
        sc[i] = (float)k;
        sh[i] = (float)((double)bb->v[i] - (double)bm->v[i] * k);
      }
      if (int r = upload_f32(e->pos_bn_sc, sc.data(), sc.size())) return r;
      if (int r = upload_f32(e->pos_bn_sh, sh.data(), sh.size())) return r;
    }
    // Multi-frame form (throughput mode).  The grouped conv has only cg = D/G (48 / 64) output channels per group: a
    // 64-wide product.  With Pf consecutive output frames per GEMM row the product is Pf*cg (240 / 256) wide and K grows
    // only from kp*cg to (kp+Pf-1)*cg (+3 %, the kernel is 128 taps long): row j*cg+co of a group holds the same filter
    // shifted by j taps.  That runs on the LDS-DMA kernel instead of the 64-wide register-staged one.
    e->pos_P = 0;
    const int Pf = cg > 0 ? 256 / cg : 0;
    // (split modes, round 4: the same form in fp32 storage -- the batched one-tile split kernel, gemm_x3s_kernel with blockIdx.y = group,
    //  replaces 512 register-staged (clip, group) products of 48 columns: 963 us of a 14.8 ms fp16x3 step)
    if ((prec || c.precision >= 2) && Pf >= 2 && cg % 8 == 0 && ((kp + Pf - 1) * cg) % 64 == 0) {
      const size_t Np = (size_t)Pf * cg, Kp = (size_t)(kp + Pf - 1) * cg;
      std::vector<float> wp((size_t)G * Np * Kp, 0.f), bp((size_t)G * Np);
      for (int g = 0; g < G; ++g)
        for (int j = 0; j < Pf; ++j)
          for (int co = 0; co < cg; ++co) {
            const int o = g * cg + co;
            bp[(size_t)g * Np + (size_t)j * cg + co] = p->v[o];
            float* row = wp.data() + ((size_t)g * Np + (size_t)j * cg + co) * Kp;
            for (int k = 0; k < kp; ++k)
              for (int ci = 0; ci < cg; ++ci) row[(size_t)(k + j) * cg + ci] = w[((size_t)o * cg + ci) * kp + k];
          }
      if (prec) { if (int r = upload_operand(1, e->pos_wP, wp.data(), wp.size())) return r; }
      else { if (int r = upload_weight(c.precision, e->pos_wP, wp.data(), (size_t)G * Np, Kp)) return r; }
      if (int r = upload_f32(e->pos_bP, bp.data(), bp.size())) return r;
      e->pos_P = Pf;
    }
  }
  if (int r = need(P, "encoder.layer_norm.weight", {D}, &p)) return r;
  if (int r = upload_f32(e->enc_g, p->v.data(), p->v.size())) return r;
  if (int r = need(P, "encoder.layer_norm.bias", {D}, &p)) return r;
  if (int r = upload_f32(e->enc_b, p->v.data(), p->v.size())) return r;

  if ((int)e->layers.size() != c.num_layers) { e->layers.clear(); e->layers.resize(c.num_layers); }
  for (int l = 0; l < c.num_layers; ++l) {
    const std::string pre = "encoder.layers." + std::to_string(l) + ".";
    EncLayerW& L = e->layers[l];
    std::vector<float> wqkv((size_t)3 * D * D), bqkv((size_t)3 * D);
    const char* names[3] = {"q_proj", "k_proj", "v_proj"};
    for (int i = 0; i < 3; ++i) {
      if (int r = need(P, pre + "attention." + names[i] + ".weight", {D, D}, &p)) return r;
      memcpy(wqkv.data() + (size_t)i * D * D, p->v.data(), (size_t)D * D * 4);
      if (int r = need(P, pre + "attention." + names[i] + ".bias", {D}, &p)) return r;
      memcpy(bqkv.data() + (size_t)i * D, p->v.data(), (size_t)D * 4);
    }
    if (int r = upload_weight(c.precision, L.wqkv, wqkv.data(), (size_t)3 * D, (size_t)D)) return r;
    if (int r = upload_f32(L.bqkv, bqkv.data(), bqkv.size())) return r;
    if (int r = need(P, pre + "attention.out_proj.weight", {D, D}, &p)) return r;
    if (int r = upload_weight(c.precision, L.wo, p->v.data(), (size_t)D, (size_t)D)) return r;
    if (int r = need(P, pre + "attention.out_proj.bias", {D}, &p)) return r;
    if (int r = upload_f32(L.bo, p->v.data(), p->v.size())) return r;
    if (int r = need(P, pre + "layer_norm.weight", {D}, &p)) return r;
    if (int r = upload_f32(L.ln1g, p->v.data(), p->v.size())) return r;
    if (int r = need(P, pre + "layer_norm.bias", {D}, &p)) return r;
    if (int r = upload_f32(L.ln1b, p->v.data(), p->v.size())) return r;
    if (int r = need(P, pre + "feed_forward.intermediate_dense.weight", {F, D}, &p)) return r;
    if (int r = upload_weight(c.precision, L.w1, p->v.data(), (size_t)F, (size_t)D)) return r;
    if (int r = need(P, pre + "feed_forward.intermediate_dense.bias", {F}, &p)) return r;
    if (int r = upload_f32(L.b1, p->v.data(), p->v.size())) return r;
    if (int r = need(P, pre + "feed_forward.output_dense.weight", {D, F}, &p)) return r;
    if (int r = upload_weight(c.precision, L.w2, p->v.data(), (size_t)D, (size_t)F)) return r;
    if (int r = need(P, pre + "feed_forward.output_dense.bias", {D}, &p)) return r;
    if (int r = upload_f32(L.b2, p->v.data(), p->v.size())) return r;
    if (int r = need(P, pre + "final_layer_norm.weight", {D}, &p)) return r;
    if (int r = upload_f32(L.ln2g, p->v.data(), p->v.size())) return r;
    if (int r = need(P, pre + "final_layer_norm.bias", {D}, &p)) return r;
    if (int r = upload_f32(L.ln2b, p->v.data(), p->v.size())) return r;
    if (c.rel_pos_buckets) {
      // gate = a (b const - 1) + 2, a / b = sigmoid of the sums of rows 0-3 / 4-7 of gru_rel_pos_linear(x_head): fold the row sums
      const int Hh = c.num_heads, dhh = D / Hh;
      const Param *gw = nullptr, *gb = nullptr, *gc = nullptr;
      if (int r = need(P, pre + "attention.gru_rel_pos_linear.weight", {8, dhh}, &gw)) return r;
      if (int r = need(P, pre + "attention.gru_rel_pos_linear.bias", {8}, &gb)) return r;
      if (int r = need(P, pre + "attention.gru_rel_pos_const", {1, Hh, 1, 1}, &gc)) return r;
      std::vector<float> wab((size_t)2 * dhh, 0.f), bab(2, 0.f);
      for (int j = 0; j < 8; ++j) {
        for (int d = 0; d < dhh; ++d) wab[(size_t)(j / 4) * dhh + d] += gw->v[(size_t)j * dhh + d];
        bab[j / 4] += gb->v[j];
      }
      if (int r = upload_f32(L.g_wab, wab.data(), wab.size())) return r;
      if (int r = upload_f32(L.g_bab, bab.data(), bab.size())) return r;
      if (int r = upload_f32(L.g_const, gc->v.data(), gc->v.size())) return r;
      if (l == 0) {
        if (int r = need(P, pre + "attention.rel_attn_embed.weight", {c.rel_pos_buckets, Hh}, &p)) return r;
        if (int r = upload_f32(e->rel_embed, p->v.data(), p->v.size())) return r;
      }
    }
  }
  SVT_HIP(hipDeviceSynchronize());
  e->finalized = true;
  return SVT_OK;
}

int64_t svt_encoder_num_frames(const svt_encoder* e, int64_t n_samples) {
  if (!e) return -1;
  int64_t t = n_samples;
  for (int i = 0; i < e->cfg.num_conv_layers; ++i) {
    if (t < e->cfg.conv_kernel[i]) return 0;
    t = (t - e->cfg.conv_kernel[i]) / e->cfg.conv_stride[i] + 1;
  }
  return t;
}

}  // extern "C"

namespace {

struct EncWs {
  double* mom;      // [0..1] wav, [2..3] out, [4 ..] window moments B*65
  size_t mom_bytes;
  size_t mom_scr[4];  // byte offsets in mom of the ordered sums' scratch: waveform moments, output moments, conv0 window moments, fused tail
  size_t mom_zero;    // leading bytes of mom a forward zeroes (statistics + every ticket)
  float* coef;
  void* c0tab;      // conv layer 0 on the matrix pipe: weight-side tables (32 KiB per clip), 16-bit modes
  void* act[2];
  float* convF;     // fp32 pre-LN conv output (layer mode)
  void* xln;
  float* hF;
  float* preF;
  void* xb;
  float* xF;
  void* xlo;
  void* posg;
  void* posy;
  float* gate;
  float* relpb;
  void* qkv;
  AttnBufs ab;
  void* attn_o;
  void* ffn;
  float* dots;      // fused tail: raw head dots, rows x 32
  float* ksplit;    // partial products of a K-split small GEMM (FFN-2 of a few utterances): 4 x rows x D fp32, or null
  size_t total;
};

// FFN-2 of a small batch splits K four ways over workgroups and leaves the sum to the LayerNorm behind it (gemm_skinny.hip, ksplit;
// svt_debug_set key 36 = 0 switches it off): up to this many rows (8 utterances of 5 s)
static const size_t kKsplitMaxRows = 2048;

EncWs carve_encoder(const svt_encoder* e, int B, int64_t L, void* base) {
  const svt_encoder_config& c = e->cfg;
  const int sp = storage_prec(c.precision);
  const size_t es = esize(sp);
  Carver cv(base);
  EncWs w;
  // 2 x (sum, sumsq) per norm group (<= B groups) + conv0 window moments, then the scratch of the three ordered sums (tickets + per-workgroup
  // partials: stats.hip, last_workgroup); the whole region is zeroed at the start of every forward (the tickets must be)
  {
    const int64_t t1 = c.num_conv_layers > 0 ? (L - c.conv_kernel[0]) / c.conv_stride[0] + 1 : 1;
    w.mom_scr[0] = align_up((4 * (size_t)B + (size_t)B * 65) * sizeof(double));
    w.mom_scr[1] = w.mom_scr[0] + align_up(moments_scratch_bytes(B));
    w.mom_scr[2] = w.mom_scr[1] + align_up(moments_scratch_bytes(B));
    w.mom_scr[3] = w.mom_scr[2] + align_up(conv0_window_moments_scratch_bytes(B, t1 > 0 ? t1 : 1));
    w.mom_zero = w.mom_scr[3] + 256;   // ... up to and including the fused tail's ticket: what a forward zeroes
    int64_t t = L;
    for (int i = 0; i < c.num_conv_layers; ++i) t = (t - c.conv_kernel[i]) / c.conv_stride[i] + 1;
    w.mom_bytes = w.mom_scr[3] + align_up(head_scratch_bytes((int64_t)B * (t > 0 ? t : 1), B));
  }
  w.mom = (double*)cv.take(w.mom_bytes);
  w.coef = (float*)cv.take((size_t)B * c.conv_dim[0] * 11 * 4);
  w.c0tab = (sp || c.precision >= 2) ? cv.take(conv0_mfma_table_bytes(B)) : nullptr;
  size_t max_act = 0, max_f = 0;
  int64_t t = L;
  for (int i = 0; i < c.num_conv_layers; ++i) {
    t = (t - c.conv_kernel[i]) / c.conv_stride[i] + 1;
    const size_t n = (size_t)B * t * c.conv_dim[i];
    if (n * es > max_act) max_act = n * es;
    if (i > 0 && n * 4 > max_f) max_f = n * 4;
  }
  const int64_t T = t;
  if (c.num_conv_layers == 0) max_act = (size_t)B * T * c.conv_dim[0] * es;
  w.act[0] = cv.take(max_act);
  w.act[1] = cv.take(max_act);
  w.convF = c.feat_extract_norm == SVT_NORM_LAYER ? (float*)cv.take(max_f) : nullptr;
  const int D = c.hidden_size, F = c.intermediate_size, H = c.num_heads, dh = D / H;
  const size_t rows = (size_t)B * T;
  const int Tp = attn_tp(sp, dh, (int)T, c.rel_pos_buckets > 0);
  const bool flash = use_flash(sp, dh, c.rel_pos_buckets > 0, (int64_t)T);
  w.xln = cv.take(rows * c.conv_dim[c.num_conv_layers > 0 ? c.num_conv_layers - 1 : 0] * es);
  w.hF = (float*)cv.take(rows * D * 4);
  w.preF = (float*)cv.take(rows * D * 4);
  w.xb = cv.take(rows * D * es);
  // split modes: xb holds the layer input as pair rows (the products' operand) and xF the fp32 residual stream beside it
  w.xF = (sp || c.precision >= 2) ? (float*)cv.take(rows * D * 4) : (float*)w.xb;
  w.xlo = sp ? cv.take(rows * D * 2) : nullptr;  // low half of the (hi, lo) bf16 residual stream (post-LN, bf16 mode)
  {
    const int Pf = e->pos_P;
    const size_t Tq = Pf ? (T + Pf - 1) / Pf : 0;
    const size_t Tp = Pf ? Tq * Pf + c.pos_conv_kernel : (size_t)(T + c.pos_conv_kernel);
    w.posg = cv.take((size_t)B * Tp * D * es);
    w.posy = Pf ? cv.take((size_t)B * Tq * Pf * D * es) : nullptr;
  }
  w.qkv = cv.take(rows * 3 * D * es);
  const bool flash3 = c.precision >= 2 && flash_attention_x3_ok(dh) && !c.rel_pos_buckets;
  w.ab.S = (flash || flash3) ? nullptr : (float*)cv.take((size_t)B * H * T * Tp * 4);
  w.ab.P = (flash || flash3) ? nullptr : cv.take((size_t)B * H * T * Tp * es);
  w.ab.Vt = cv.take((size_t)B * H * dh * Tp * es);
  w.ab.pl_qkv = (c.precision >= 2 && flash_attention_x3_ok(dh) && !c.rel_pos_buckets) ? cv.take(rows * 3 * D * 4) : nullptr;
  w.attn_o = cv.take(rows * D * es);
  w.ffn = cv.take(rows * F * es);
  w.gate = c.rel_pos_buckets ? (float*)cv.take((size_t)B * H * T * 4) : nullptr;
  w.relpb = c.rel_pos_buckets ? (float*)cv.take((size_t)H * (2 * T - 1) * 4) : nullptr;
  w.dots = (float*)cv.take(rows * 32 * 4);
  w.ksplit = (sp && rows <= kKsplitMaxRows) ? (float*)cv.take((size_t)4 * rows * D * 4) : nullptr;
  w.total = cv.off;
  return w;
}

// Tail of a forward call: either the features (the wrapper's output) or, with a head, logits (+ decoded frames) straight
// from the un-normalised encoder output (fused out-norm + head + decode, stats.hip head_dots_kernel).
struct TailSpec {
  float* feats = nullptr;
  const svt_linear* head = nullptr;
  float* logits = nullptr;
  svt_frame* frames = nullptr;
  int n_oct = 0, n_cls = 0;
};

}  // namespace

extern "C" {

int svt_debug_encoder_layout(const svt_encoder* e, int32_t batch, int64_t n_samples, int64_t* offsets, int n) {
  if (!e || batch < 1 || !offsets || n < 1) { set_error("svt_debug_encoder_layout: bad argument"); return SVT_ERR_INVALID; }
  if (svt_encoder_num_frames(e, n_samples) < 1) { set_error("waveform shorter than the receptive field"); return SVT_ERR_INVALID; }
  char* const fake = (char*)(uintptr_t)(1ull << 40);   // never dereferenced: carve_encoder only adds offsets to it
  const EncWs w = carve_encoder(e, batch, n_samples, fake);
  const void* r[24] = {w.mom, w.coef, w.c0tab, w.act[0], w.act[1], w.convF, w.xln, w.hF, w.preF, w.xb, w.xF, w.xlo, w.posg, w.posy, w.qkv,
                       w.ab.S, w.ab.P, w.ab.Vt, w.ab.pl_qkv, w.attn_o, w.ffn, w.gate, w.relpb, w.dots};
  int k = 0;
  for (; k < 24 && k < n; ++k) offsets[k] = r[k] == nullptr ? -1 : (int64_t)((const char*)r[k] - fake);
  if (k < n) offsets[k++] = (int64_t)w.total;
  return k;
}

int64_t svt_encoder_workspace_bytes(const svt_encoder* e, int32_t batch, int64_t n_samples) {
  if (!e || batch < 1) { set_error("workspace_bytes: bad argument"); return -1; }
  if (svt_encoder_num_frames(e, n_samples) < 1) { set_error("waveform shorter than the receptive field"); return -1; }
  return (int64_t)carve_encoder(e, batch, n_samples, nullptr).total;
}

}  // extern "C"

static int encoder_forward_impl(svt_encoder* e, const float* wav, int32_t B, int64_t L, const TailSpec& tail, void* workspace,
                                size_t workspace_bytes, void* stream, int32_t clips_per_norm_group);

extern "C" {

int svt_encoder_forward(svt_encoder* e, const float* wav, int32_t B, int64_t L, float* feats, void* workspace,
                        size_t workspace_bytes, void* stream) {
  return svt_encoder_forward_ex(e, wav, B, L, feats, workspace, workspace_bytes, stream, 0);
}

int svt_encoder_forward_ex(svt_encoder* e, const float* wav, int32_t B, int64_t L, float* feats, void* workspace,
                           size_t workspace_bytes, void* stream, int32_t clips_per_norm_group) {
  if (!feats) { set_error("encoder_forward: null argument"); return SVT_ERR_INVALID; }
  TailSpec t;
  t.feats = feats;
  return encoder_forward_impl(e, wav, B, L, t, workspace, workspace_bytes, stream, clips_per_norm_group);
}

int svt_encoder_forward_head(svt_encoder* e, const svt_linear* head, const float* wav, int32_t B, int64_t L, float* logits,
                             svt_frame* frames, int32_t n_octave, int32_t n_class, void* workspace, size_t workspace_bytes,
                             void* stream, int32_t clips_per_norm_group) {
  if (!head || !logits) { set_error("encoder_forward_head: null argument"); return SVT_ERR_INVALID; }
  if (!head->loaded) { set_error("encoder_forward_head: head weights not loaded"); return SVT_ERR_STATE; }
  if (!e || head->in_f != e->cfg.hidden_size || head->device != e->device) {
    set_error("encoder_forward_head: the head must take hidden_size inputs and live on the encoder's device"); return SVT_ERR_INVALID; }
  if (!linear_head_eligible(head->in_f, head->out_f)) {
    set_error("encoder_forward_head: the fused tail is built for hidden sizes 512 / 768 / 1024 and at most 32 outputs"); return SVT_ERR_INVALID; }
  if (frames && head->out_f != 2 + n_octave + 1 + n_class + 1) {
    set_error("encoder_forward_head: n_out != 2 + (n_octave+1) + (n_class+1)"); return SVT_ERR_INVALID; }
  TailSpec t;
  t.head = head; t.logits = logits; t.frames = frames; t.n_oct = n_octave; t.n_cls = n_class;
  return encoder_forward_impl(e, wav, B, L, t, workspace, workspace_bytes, stream, clips_per_norm_group);
}

}  // extern "C"

static int encoder_forward_impl(svt_encoder* e, const float* wav, int32_t B, int64_t L, const TailSpec& tail, void* workspace,
                                size_t workspace_bytes, void* stream, int32_t clips_per_norm_group) {
  float* feats = tail.feats;
  if (!e || !wav || !workspace) { set_error("encoder_forward: null argument"); return SVT_ERR_INVALID; }
  if (!e->finalized) { set_error("encoder_forward: parameters not finalized"); return SVT_ERR_STATE; }
  if (B < 1) { set_error("encoder_forward: batch < 1"); return SVT_ERR_INVALID; }
  const int64_t T = svt_encoder_num_frames(e, L);
  if (T < 1) { set_error("encoder_forward: waveform shorter than the receptive field"); return SVT_ERR_INVALID; }
  const svt_encoder_config& c = e->cfg;
  const int prec = storage_prec(c.precision);  // storage type of activations / weights
  const int gp = c.precision;                  // engine of the dense products (launch_gemm)
  EncWs w = carve_encoder(e, B, L, workspace);
  if (w.total > workspace_bytes) { set_error("encoder_forward: workspace too small (" + std::to_string(workspace_bytes) + " < " + std::to_string(w.total) + ")"); return SVT_ERR_WORKSPACE; }
  hipStream_t s = (hipStream_t)stream;
  SVT_HIP(hipSetDevice(e->device));
  // the wrapper's two whole-tensor layer norms run over groups of `cpg` consecutive clips: cpg = B is the reference on a
  // batch (and per device shard under DataParallel / DDP), cpg = 1 makes a batch of B clips equal to B batch-1 forwards --
  // the reference's evaluation loop (train_audio_ssl.py:90 asserts batch 1) without its one-utterance-at-a-time cost
  const int cpg = clips_per_norm_group > 0 ? clips_per_norm_group : B;
  if (B % cpg) { set_error("encoder_forward: batch must be a multiple of clips_per_norm_group"); return SVT_ERR_INVALID; }
  const int groups = B / cpg;
  if (groups > 1 && c.num_conv_layers > 0 && (L & 3)) {
    set_error("encoder_forward: norm groups need a waveform length that is a multiple of 4 samples");
    return SVT_ERR_INVALID;
  }
  if (groups > 1 && c.num_conv_layers == 0 && c.normalize_wav) {
    set_error("encoder_forward: features-in mode has no input norm to group");
    return SVT_ERR_INVALID;
  }
  if (launch_zero_bytes(w.mom, w.mom_zero, s)) return SVT_ERR_HIP;   // (a kernel, not a memset node: see encoder_ops.hip)
  double* wav_mom = c.normalize_wav ? w.mom : nullptr;
  double* out_mom = w.mom + 2 * (size_t)B;
  double* wm = w.mom + 4 * (size_t)B;
  int64_t n_wav = (int64_t)cpg * L;
  if (c.normalize_wav)
    if (int r = launch_moments(wav, n_wav, wav_mom, (char*)w.mom + w.mom_scr[0], B, s, groups)) return r;
  // "global-batch-equivalent" norms (optional): the batch is a shard of a larger one; the caller's function sums the
  // (sum, sum of squares) pair over the ranks -- 16 bytes per norm -- and the statistics are then those of the whole global batch
  struct ReduceCtx { svt_encoder* e; double* mom; hipStream_t s; } rctx{e, nullptr, s};
  auto reduce_now = [](void* a) -> int {
    ReduceCtx* rc = (ReduceCtx*)a;
    if (rc->e->reduce_fn(rc->mom, 2, (void*)rc->s, rc->e->reduce_user)) { set_error("encoder_forward: the norm-reduce callback reported an error"); return SVT_ERR_INVALID; }
    return 0;
  };
  const bool global_norm = e->reduce_fn != nullptr;
  if (global_norm) {
    if (groups != 1) { set_error("encoder_forward: the cross-rank norm reduction applies to whole-batch norms (clips_per_norm_group = 0)"); return SVT_ERR_INVALID; }
    if (e->reduce_global_clips < B) { set_error("encoder_forward: global_clips of the norm reduction is smaller than this batch"); return SVT_ERR_INVALID; }
    if (c.normalize_wav) {
      rctx.mom = wav_mom;
      if (int r = reduce_now(&rctx)) return r;
      n_wav = e->reduce_global_clips * L;
    }
  }

  // ---- split modes: which products take PAIR ROWS (gemm_x3q.hip: operands cut by their producers) ----
  // front = conv 1..n-1 and the feature projection, enc = the four products of every encoder layer; a section switches as a whole,
  // and only when every product in it fits gemm_x3q_kernel's contract (otherwise its activations stay fp32 and the products cut them)
  const int pk_mode = (gp >= 2 && g_x3_pairs && g_gemm_x3) ? gp : 0;
  auto x3q_fits = [&](const void* A, int M, int N, int K, int a_rpb, long a_bstride, long a_rstride, const void* Wp, int c_pairs, long ldc) -> bool {
    GemmArgs g;
    g.A = A; g.W = Wp; g.C = const_cast<void*>(A); g.M = M; g.N = N; g.K = K; g.a_rpb = a_rpb; g.a_bstride = a_bstride; g.a_rstride = a_rstride;
    g.ldw = K; g.ldc = ldc; g.a_pairs = 1; g.c_pairs = c_pairs;
    return gemm_x3q_eligible(g);
  };
  bool pk_front_ok = pk_mode != 0 && c.num_conv_layers >= 2 && c.conv_dim[0] % 32 == 0 && c.conv_dim[0] <= 512 && c.conv_stride[0] <= 5;
  if (pk_front_ok) {
    int64_t ti_ = (L - c.conv_kernel[0]) / c.conv_stride[0] + 1;
    for (int i = 1; i < c.num_conv_layers && pk_front_ok; ++i) {
      const int cin = c.conv_dim[i - 1], co = c.conv_dim[i], k = c.conv_kernel[i], st = c.conv_stride[i];
      const int64_t to_ = (ti_ - k) / st + 1;
      if ((int64_t)B * to_ > 2147483647LL) { pk_front_ok = false; break; }
      pk_front_ok = x3q_fits(w.act[0], (int)((int64_t)B * to_), co, k * cin, (int)to_, ti_ * cin, (long)st * cin, e->conv[i].w.p, 1, co) &&
                    (c.feat_extract_norm != SVT_NORM_LAYER || co == 512 || co == 768 || co == 1024);
      ti_ = to_;
    }
    const int Cl = c.conv_dim[c.num_conv_layers - 1];
    const int64_t rows_ = (int64_t)B * T;
    pk_front_ok = pk_front_ok && x3q_fits(w.xln, (int)rows_, c.hidden_size, Cl, (int)rows_, 0, Cl, e->proj_w.p, 0, c.hidden_size) &&
                  (!c.feat_proj_layer_norm || Cl == 512 || Cl == 768 || Cl == 1024);
  }
  const int pk_front = pk_front_ok ? pk_mode : 0;

  // ---- conv feature extractor (channels-last activations) ----
  int64_t tin = L;
  int cur = 0;
  if (c.num_conv_layers == 0) {
    // features-in mode: `wav` is the (B, T, C) fp32 feature tensor
    const int64_t n = (int64_t)B * L * c.conv_dim[0];
    if (prec) { if (int r = launch_f32_to_bf16(wav, (bf16_t*)w.act[0], n, s)) return r; }
    else if (launch_copy_f32(wav, (float*)w.act[0], n, s)) return SVT_ERR_HIP;
  } else {
  int64_t t1 = (L - c.conv_kernel[0]) / c.conv_stride[0] + 1;
  const ConvLayerW& c0 = e->conv[0];
  if (c.feat_extract_norm == SVT_NORM_GROUP) {
    if (int r = launch_conv0_window_moments(wav, B, L, c.conv_kernel[0], c.conv_stride[0], t1, wm, (char*)w.mom + w.mom_scr[2], s)) return r;
    if (int r = launch_conv0_group_coef(wav_mom, n_wav, wm, B, t1, c.conv_dim[0], c.conv_kernel[0], c0.w.as<float>(),
                                        c.conv_bias ? c0.bias.as<float>() : nullptr, c0.gamma.as<float>(),
                                        c0.beta.as<float>(), 1e-5f, 1e-5f, w.coef, s, cpg)) return r;
    if (conv0_mfma_ok(prec, pk_front, c.conv_kernel[0], c.conv_stride[0], c.conv_dim[0]) && w.c0tab) {
      if (int r = launch_conv0_mfma_group(wav, B, L, c.conv_stride[0], t1, w.coef, w.c0tab, w.act[0], s, pk_front)) return r;
    } else
    if (int r = launch_conv0_group_apply(prec, wav, B, L, c.conv_kernel[0], c.conv_stride[0], t1, c.conv_dim[0], w.coef,
                                         w.act[0], s, pk_front)) return r;
  } else {
    if (conv0_mfma_ok(prec, pk_front, c.conv_kernel[0], c.conv_stride[0], c.conv_dim[0]) && w.c0tab) {
      if (int r = launch_conv0_mfma_layer(wav, B, L, c.conv_stride[0], t1, wav_mom, n_wav, 1e-5f, c0.w.as<float>(),
                                          c.conv_bias ? c0.bias.as<float>() : nullptr, c0.gamma.as<float>(), c0.beta.as<float>(), 1e-5f,
                                          w.c0tab, w.act[0], s, cpg, pk_front)) return r;
    } else
    if (int r = launch_conv0_layer(prec, wav, B, L, c.conv_kernel[0], c.conv_stride[0], t1, c.conv_dim[0], wav_mom, n_wav,
                                   1e-5f, c0.w.as<float>(), c.conv_bias ? c0.bias.as<float>() : nullptr,
                                   c0.gamma.as<float>(), c0.beta.as<float>(), 1e-5f, w.act[0], s, cpg, pk_front)) return r;
  }
  tin = t1;
  }
  for (int i = 1; i < c.num_conv_layers; ++i) {
    const int cin = c.conv_dim[i - 1], co = c.conv_dim[i], k = c.conv_kernel[i], st = c.conv_stride[i];
    const int64_t tout = (tin - k) / st + 1;
    const ConvLayerW& Lw = e->conv[i];
    GemmArgs g;
    g.A = w.act[cur]; g.W = Lw.w.p;
    g.M = (int)((int64_t)B * tout); g.N = co; g.K = k * cin;
    g.a_rpb = (int)tout; g.a_bstride = tin * cin; g.a_rstride = (long)st * cin;
    g.ldw = g.K; g.ldc = co;
    if (Lw.w_kperm.p) { g.W_kperm = Lw.w_kperm.p; g.kperm_taps = k; g.kperm_cin = cin; }
    g.bias = c.conv_bias ? Lw.bias.as<float>() : nullptr;
    if ((int64_t)B * tout > 2147483647LL) { set_error("encoder_forward: batch*frames exceeds 2^31"); return SVT_ERR_INVALID; }
    // pair rows: this layer reads them; it writes them too unless the feature projection's LayerNorm (an fp32 reader) comes next
    g.a_pairs = pk_front ? 1 : 0;
    const bool pairs_out = pk_front && !(i + 1 == c.num_conv_layers && c.feat_proj_layer_norm);
    if (pk_front && c.feat_extract_norm == SVT_NORM_LAYER) {
      g.C = w.convF; g.out_f32 = 1; g.act = ACT_NONE;
      if (int r = launch_gemm(gp, g, s)) return r;
      if (int r = launch_layernorm(prec, w.convF, 1, (int64_t)B * tout, co, Lw.gamma.as<float>(), Lw.beta.as<float>(), 1e-5f, 1,
                                   pairs_out ? nullptr : w.act[cur ^ 1], nullptr, s, nullptr, nullptr, pairs_out ? w.act[cur ^ 1] : nullptr,
                                   pk_front)) return r;
    } else if (pk_front) {
      g.C = w.act[cur ^ 1]; g.act = ACT_GELU; g.out_f32 = 1; g.c_pairs = pairs_out ? 1 : 0;
      if (int r = launch_gemm(gp, g, s)) return r;
    } else
    if (c.feat_extract_norm == SVT_NORM_LAYER && prec && co == 512 && g_conv_ln_bf16) {
      // throughput mode: the conv output goes to HBM once, in the operand type, and is normalised in place (a wave owns a
      // row: it reads all of it before it writes) -- the fp32 round trip below moves 3x the bytes (conv1 at 64 x 10 s:
      // 2.1 GB written + 2.1 GB read + 1.05 GB written)
      g.C = w.act[cur ^ 1]; g.out_f32 = 0; g.act = ACT_NONE;
      if (int r = launch_gemm(gp, g, s)) return r;
      if (int r = launch_layernorm(prec, w.act[cur ^ 1], 0, (int64_t)B * tout, co, Lw.gamma.as<float>(), Lw.beta.as<float>(),
                                   1e-5f, 1, w.act[cur ^ 1], nullptr, s)) return r;
    } else if (c.feat_extract_norm == SVT_NORM_LAYER) {
      g.C = w.convF; g.out_f32 = 1; g.act = ACT_NONE;
      if (int r = launch_gemm(gp, g, s)) return r;
      if (int r = launch_layernorm(prec, w.convF, 1, (int64_t)B * tout, co, Lw.gamma.as<float>(), Lw.beta.as<float>(),
                                   1e-5f, 1, w.act[cur ^ 1], nullptr, s)) return r;
    } else {
      g.C = w.act[cur ^ 1]; g.act = ACT_GELU;
      if (int r = launch_gemm(gp, g, s)) return r;
    }
    cur ^= 1;
    tin = tout;
  }
  const int C = c.conv_dim[c.num_conv_layers > 0 ? c.num_conv_layers - 1 : 0];
  const int D = c.hidden_size, F = c.intermediate_size, H = c.num_heads, dh = D / H;
  const int64_t rows = (int64_t)B * T;
  const float eps = c.layer_norm_eps;

  // ---- feature projection ----
  const void* proj_in = w.act[cur];
  if (c.feat_proj_layer_norm) {
    if (int r = launch_layernorm(prec, w.act[cur], prec ? 0 : 1, rows, C, e->fp_g.as<float>(), e->fp_b.as<float>(), eps, 0,
                                 pk_front ? nullptr : w.xln, nullptr, s, nullptr, nullptr, pk_front ? w.xln : nullptr, pk_front)) return r;
    proj_in = w.xln;
  }
  {
    GemmArgs g;
    g.A = proj_in; g.W = e->proj_w.p; g.C = w.hF; g.bias = e->proj_b.as<float>();
    g.M = (int)rows; g.N = D; g.K = C; g.a_rpb = (int)rows; g.a_rstride = C; g.ldw = C; g.ldc = D; g.out_f32 = 1;
    g.a_pairs = pk_front ? 1 : 0;
    if (int r = launch_gemm(gp, g, s)) return r;
  }
  // ---- positional conv embedding: pre = h + gelu(grouped_conv(h) + b) ----
  {
    const int kp = c.pos_conv_kernel, G = c.pos_conv_groups, cg = D / G;
    const int Pf = e->pos_P;
    const float* bn_sc = c.pos_conv_batch_norm ? e->pos_bn_sc.as<float>() : nullptr;
    const float* bn_sh = c.pos_conv_batch_norm ? e->pos_bn_sh.as<float>() : nullptr;
    if (c.pos_conv_depth > 1) {
      // data2vec-audio: pos = stack of [grouped conv -> LayerNorm(no affine, eps 1e-5) -> GELU]; pre = h + pos
      const float* cur = w.hF;
      float* lnout = w.xF;  // fp32 scratch (rows x D): free until the encoder's first LayerNorm
      for (int i = 0; i < c.pos_conv_depth; ++i) {
        if (int r = launch_posconv_gather(prec, cur, B, (int)T, D, G, kp, (int)T + kp, w.posg, s)) return r;
        GemmArgs g;
        g.A = w.posg; g.W = e->pos_ws[i].p; g.C = w.preF; g.bias = e->pos_bs[i].as<float>();
        g.M = (int)T; g.N = cg; g.K = kp * cg;
        g.a_rpb = (int)T; g.a_rstride = cg;
        g.ldw = g.K; g.ldc = D;
        g.nz = B * G; g.nz2 = G;
        g.a_z1 = (long)G * (T + kp) * cg; g.a_z2 = (long)(T + kp) * cg;
        g.w_z1 = 0; g.w_z2 = (long)cg * g.K;
        g.c_z1 = (long)T * D; g.c_z2 = cg; g.bias_z2 = cg;
        g.act = ACT_NONE; g.out_f32 = 1;
        if (int r = launch_gemm(gp, g, s)) return r;
        if (int r = launch_layernorm(prec, w.preF, 1, rows, D, e->ones.as<float>(), e->zeros.as<float>(), 1e-5f, 1, nullptr,
                                     lnout, s)) return r;
        cur = lnout;
      }
      if (int r = launch_add_f32(w.hF, cur, w.preF, rows * (int64_t)D, s)) return r;
    } else if (Pf && (int64_t)B * ((T + Pf - 1) / Pf) >= 128) {
      const int Tq = (int)((T + Pf - 1) / Pf), Tp = Tq * Pf + kp;
      if (int r = launch_posconv_gather(prec, w.hF, B, (int)T, D, G, kp, Tp, w.posg, s, bn_sc, bn_sh)) return r;
      GemmArgs g;
      g.A = w.posg; g.W = e->pos_wP.p; g.C = w.posy; g.bias = e->pos_bP.as<float>();
      g.M = B * Tq; g.N = Pf * cg; g.K = (kp + Pf - 1) * cg;
      g.a_rpb = Tq; g.a_bstride = (long)G * Tp * cg; g.a_rstride = (long)Pf * cg;
      g.ldw = g.K; g.ldc = g.N;
      g.nz = G; g.nz2 = G;
      g.a_z2 = (long)Tp * cg; g.w_z2 = (long)g.N * g.K; g.c_z2 = (long)B * Tq * g.N; g.bias_z2 = g.N;
      g.act = ACT_GELU; g.out_f32 = 0;
      if (int r = launch_gemm(gp, g, s)) return r;
      if (int r = launch_posconv_scatter_add(w.hF, w.posy, B, (int)T, D, G, Pf, Tq, w.preF, s, prec ? 0 : 1)) return r;
    } else {
    if (int r = launch_posconv_gather(prec, w.hF, B, (int)T, D, G, kp, (int)T + kp, w.posg, s, bn_sc, bn_sh)) return r;
    GemmArgs g;
    g.A = w.posg; g.W = e->pos_w.p; g.C = w.preF; g.bias = e->pos_b.as<float>(); g.resid = w.hF;
    g.M = (int)T; g.N = cg; g.K = kp * cg;
    g.a_rpb = (int)T; g.a_rstride = cg;
    g.ldw = g.K; g.ldc = D;
    g.nz = B * G; g.nz2 = G;
    g.a_z1 = (long)G * (T + kp) * cg; g.a_z2 = (long)(T + kp) * cg;
    g.w_z1 = 0; g.w_z2 = (long)cg * g.K;
    g.c_z1 = (long)T * D; g.c_z2 = cg; g.bias_z2 = cg;
    g.act = ACT_GELU; g.out_f32 = 1;
    if (int r = launch_gemm(gp, g, s)) return r;
    }
  }
  const float scale = 1.0f / std::sqrt((float)dh);
  if (c.rel_pos_buckets)
    if (int r = launch_relpos_table(e->rel_embed.as<float>(), H, (int)T, c.rel_pos_buckets, c.rel_pos_max_distance, w.relpb, s)) return r;
  // split-operand modes with the fused attention: the QKV projection's epilogue writes the planes the attention reads
  const bool qkv_planes = gp >= 2 && !c.rel_pos_buckets && flash_attention_x3_ok(dh) && w.ab.pl_qkv != nullptr;
  unsigned short* const qkv_pl = qkv_planes ? (unsigned short*)w.ab.pl_qkv : nullptr;
  // encoder layers on pair rows: the layer input (LayerNorm output), the attention output and the FFN intermediate are written as
  // pair rows by their producers; the residual stream stays fp32 beside them (w.xF)
  const bool pk_enc_ok = pk_mode != 0 && qkv_planes && c.num_layers > 0 && (D == 512 || D == 768 || D == 1024) && dh % 32 == 0 &&
                         x3q_fits(w.xb, (int)rows, 3 * D, D, (int)rows, 0, D, e->layers[0].wqkv.p, 0, 3 * D) &&
                         x3q_fits(w.attn_o, (int)rows, D, D, (int)rows, 0, D, e->layers[0].wo.p, 0, D) &&
                         x3q_fits(w.xb, (int)rows, F, D, (int)rows, 0, D, e->layers[0].w1.p, 1, F) &&
                         x3q_fits(w.ffn, (int)rows, D, F, (int)rows, 0, F, e->layers[0].w2.p, 0, D);
  const int pk_enc = pk_enc_ok ? pk_mode : 0;
  if (!prec && !pk_enc) w.xF = (float*)w.xb;   // fp32 storage without pair rows: the layer input IS the residual stream (one buffer)
  int cur_layer = 0;
  auto attention = [&](void) -> int {
    const float* gate = nullptr;
    if (c.rel_pos_buckets) {
      // WavLM: the gate of the relative position bias is a function of the attention INPUT (w.xb, operand type)
      const EncLayerW& Lg = e->layers[cur_layer];
      if (int r = launch_relpos_gate(prec, w.xb, rows, (int)T, H, dh, Lg.g_wab.as<float>(), Lg.g_bab.as<float>(),
                                     Lg.g_const.as<float>(), w.gate, s)) return r;
      gate = w.gate;
    }
    ++cur_layer;
    return attention_scores_path(prec, w.qkv, 3L * D, (const char*)w.qkv + (size_t)D * esize(prec),
                                 (const char*)w.qkv + (size_t)2 * D * esize(prec), 3L * D, B, (int)T, H, dh, scale, w.ab,
                                 qkv_planes, w.attn_o, D, s, gate, w.relpb, gp, pk_enc ? 1 : 0);
  };
  // planes: the product additionally / instead leaves as 16-bit (hi, lo) planes for the fused split attention (QKV projection)
  auto gemm_rows = [&](const void* A, int K, const DevBuf& W, const DevBuf& bias, int N, void* Cout, int out_f32, int act,
                       const float* resid, unsigned short* planes = nullptr, int c_pairs = 0) -> int {
    GemmArgs g;
    g.A = A; g.W = W.p; g.C = Cout; g.bias = bias.as<float>(); g.resid = resid;
    g.M = (int)rows; g.N = N; g.K = K; g.a_rpb = (int)rows; g.a_rstride = K; g.ldw = K; g.ldc = N;
    g.out_f32 = out_f32; g.act = act;
    g.planes = planes; g.plane_stride = (long)rows * N;
    g.a_pairs = pk_enc ? 1 : 0; g.c_pairs = c_pairs;
    return launch_gemm(gp, g, s);
  };

  float* final_x = nullptr;
  // The residual add lives in the LayerNorm kernel (LN(x + branch)), not in the GEMM epilogue: the GEMM epilogue
  // is then store-only (fire-and-forget under the next tile's MFMAs in the persistent kernel).  tmp = w.hF is free
  // after the positional conv.
  float* tmp = w.hF;
  // branch outputs (out-proj / FFN-2) are stored in the operand type (bf16 in throughput mode: half the store burst of
  // the GEMM epilogue and half the read of the LayerNorm) and widened when added to the fp32 residual stream
  const bool vecD = (D == 512 || D == 768 || D == 1024);
  const int tmp_f32 = (prec && vecD) ? 0 : 1;
  if (!c.stable_layer_norm && prec && layernorm_hilo_ok(D) && c.num_layers > 0) {
    // throughput mode: the residual stream lives as a bf16 (hi, lo) pair -- hi IS the operand copy the next GEMM
    // reads -- so a LayerNorm moves 10 bytes per element instead of 12 (see layernorm.hip, layernorm_hilo_kernel)
    bf16_t* xh = (bf16_t*)w.xb;
    bf16_t* xl = (bf16_t*)w.xlo;
    if (int r = launch_layernorm_hilo(nullptr, nullptr, nullptr, w.preF, rows, D, e->enc_g.as<float>(), e->enc_b.as<float>(), eps,
                                      xh, xl, nullptr, s)) return r;
    // FFN-2 as a K-split small GEMM: when the one-utterance kernel would serve it with less than one workgroup per CU (gemm_skinny.hip)
    bool ffn2_split = false;
    if (g_ffn2_ksplit && w.ksplit && gp == 1 && F % 256 == 0 && F >= 2048 && g_ln_two_rows) {
      GemmArgs g;
      g.A = w.ffn; g.W = e->layers[0].w2.p; g.C = tmp; g.M = (int)rows; g.N = D; g.K = F; g.a_rpb = (int)rows; g.a_rstride = F; g.ldw = F; g.ldc = D;
      ffn2_split = g_gemm_skinny && gemm_skinny_eligible(g) && (long)((rows + 31) / 32) * (D / 32) <= 256;
    }
    for (int l = 0; l < c.num_layers; ++l) {
      const EncLayerW& Lw = e->layers[l];
      const bool last = l + 1 == c.num_layers;
      if (int r = gemm_rows(w.xb, D, Lw.wqkv, Lw.bqkv, 3 * D, w.qkv, 0, ACT_NONE, nullptr, qkv_pl)) return r;
      if (int r = attention()) return r;
      // (rounds 1-2 fused this projection with the residual add and the LayerNorm in one row-complete kernel, 44 us against 29 + 23; with
      //  the projection on gemm_pps_kernel the pair costs 20.6 + 23.9 us and the fused kernel -- every workgroup streaming all of W,
      //  0.16 of the matrix pipe -- is gone: C2 6 093-6 110 against 6 066-6 074 clips/s on one box)
      if (int r = gemm_rows(w.attn_o, D, Lw.wo, Lw.bo, D, tmp, 0, ACT_NONE, nullptr)) return r;
      if (int r = launch_layernorm_hilo((const bf16_t*)tmp, xh, xl, nullptr, rows, D, Lw.ln1g.as<float>(), Lw.ln1b.as<float>(), eps,
                                        xh, xl, nullptr, s)) return r;
      if (int r = gemm_rows(w.xb, D, Lw.w1, Lw.b1, F, w.ffn, 0, ACT_GELU, nullptr)) return r;
      if (ffn2_split) {
        // a few utterances: K = F split four ways over workgroups, raw fp32 partial tiles, summed (+ bias, rounded to the operand type
        // like the un-split product's stored result) by the LayerNorm that reads them
        GemmArgs g;
        g.A = w.ffn; g.W = Lw.w2.p; g.C = w.ksplit; g.M = (int)rows; g.N = D; g.K = F; g.a_rpb = (int)rows; g.a_rstride = F; g.ldw = F; g.ldc = D;
        g.out_f32 = 1; g.ksplit = 4; g.ksplit_stride = (long)rows * D;
        if (int r = launch_gemm_skinny(g, s)) return r;
        if (int r = launch_layernorm_hilo_parts(w.ksplit, 4, (long)rows * D, Lw.b2.as<float>(), xh, xl, rows, D, Lw.ln2g.as<float>(), Lw.ln2b.as<float>(),
                                                eps, xh, xl, last ? w.xF : nullptr, s)) return r;
        continue;
      }
      if (int r = gemm_rows(w.ffn, F, Lw.w2, Lw.b2, D, tmp, 0, ACT_NONE, nullptr)) return r;
      if (int r = launch_layernorm_hilo((const bf16_t*)tmp, xh, xl, nullptr, rows, D, Lw.ln2g.as<float>(), Lw.ln2b.as<float>(), eps,
                                        xh, xl, last ? w.xF : nullptr, s)) return r;
    }
    final_x = w.xF;
  } else if (!c.stable_layer_norm && pk_enc) {
    // split modes on pair rows.  fp16 pieces (kind 3): the layer input w.xb (pair rows) IS the residual stream -- LN(branch + (hi + lo))
    // -> (hi', lo') in place, 12 bytes per element and pass instead of 16 with an fp32 copy beside it: hi + lo of two IEEE halves
    // carries 22 of fp32's 24 mantissa bits.  bf16 pieces (kind 2) carry 16: there the residual stream stays fp32 (w.xF, updated in
    // place) beside the pair rows the products read, as in round 3.  The products see exactly the same pieces either way; the last
    // layer also leaves the fp32 result for the whole-batch output norm.
    const bool pair_resid = pk_enc == 3;
    float* const keepF = pair_resid ? nullptr : w.xF;
    if (int r = launch_layernorm(prec, w.preF, 1, rows, D, e->enc_g.as<float>(), e->enc_b.as<float>(), eps, 0, nullptr, keepF, s, nullptr,
                                 nullptr, w.xb, pk_enc)) return r;
    auto ln_resid = [&](const float* g_, const float* b_, bool want_f32) -> int {
      if (pair_resid)
        return launch_layernorm(prec, tmp, 1, rows, D, g_, b_, eps, 0, nullptr, want_f32 ? w.xF : nullptr, s, nullptr, nullptr, w.xb,
                                pk_enc, w.xb);
      // every lane holds its part of the row in registers before anything is stored: add and yF may be the same buffer
      return launch_layernorm(prec, tmp, 1, rows, D, g_, b_, eps, 0, nullptr, w.xF, s, w.xF, nullptr, w.xb, pk_enc, nullptr);
    };
    for (int l = 0; l < c.num_layers; ++l) {
      const EncLayerW& Lw = e->layers[l];
      const bool last = l + 1 == c.num_layers;
      if (int r = gemm_rows(w.xb, D, Lw.wqkv, Lw.bqkv, 3 * D, w.qkv, 0, ACT_NONE, nullptr, qkv_pl)) return r;
      if (int r = attention()) return r;
      if (int r = gemm_rows(w.attn_o, D, Lw.wo, Lw.bo, D, tmp, 1, ACT_NONE, nullptr)) return r;
      if (int r = ln_resid(Lw.ln1g.as<float>(), Lw.ln1b.as<float>(), false)) return r;
      if (int r = gemm_rows(w.xb, D, Lw.w1, Lw.b1, F, w.ffn, 1, ACT_GELU, nullptr, nullptr, 1)) return r;
      if (int r = gemm_rows(w.ffn, F, Lw.w2, Lw.b2, D, tmp, 1, ACT_NONE, nullptr)) return r;
      if (int r = ln_resid(Lw.ln2g.as<float>(), Lw.ln2b.as<float>(), last)) return r;
    }
    final_x = w.xF;
  } else if (!c.stable_layer_norm) {
    if (int r = launch_layernorm(prec, w.preF, 1, rows, D, e->enc_g.as<float>(), e->enc_b.as<float>(), eps, 0, w.xb,
                                 prec ? w.xF : nullptr, s)) return r;
    for (int l = 0; l < c.num_layers; ++l) {
      const EncLayerW& Lw = e->layers[l];
      if (int r = gemm_rows(w.xb, D, Lw.wqkv, Lw.bqkv, 3 * D, w.qkv, 0, ACT_NONE, nullptr, qkv_pl)) return r;
      if (int r = attention()) return r;
      if (int r = gemm_rows(w.attn_o, D, Lw.wo, Lw.bo, D, tmp, tmp_f32, ACT_NONE, nullptr)) return r;
      if (int r = launch_layernorm(prec, tmp, tmp_f32, rows, D, Lw.ln1g.as<float>(), Lw.ln1b.as<float>(), eps, 0, w.xb,
                                   prec ? w.xF : nullptr, s, w.xF)) return r;
      if (int r = gemm_rows(w.xb, D, Lw.w1, Lw.b1, F, w.ffn, 0, ACT_GELU, nullptr)) return r;
      if (int r = gemm_rows(w.ffn, F, Lw.w2, Lw.b2, D, tmp, tmp_f32, ACT_NONE, nullptr)) return r;
      if (int r = launch_layernorm(prec, tmp, tmp_f32, rows, D, Lw.ln2g.as<float>(), Lw.ln2b.as<float>(), eps, 0, w.xb,
                                   prec ? w.xF : nullptr, s, w.xF)) return r;
    }
    final_x = w.xF;
  } else {
    float* h = w.preF;
    const void* pending = nullptr;  // branch output not yet added to h
    // branch outputs in the operand type in throughput mode (bf16: half the GEMM store burst and 2 of the 14 bytes per
    // element the LayerNorm moves); the fp32 residual stream h is updated in place by the LayerNorm kernel (sumF)
    auto ln_add = [&](const float* g_, const float* b_, const void* branch, void* y_op, float* y_f32) -> int {
      if (pk_enc && y_op)   // pair rows for the products; h (fp32) += branch in place
        return launch_layernorm(prec, h, 1, rows, D, g_, b_, eps, 0, nullptr, nullptr, s, (const float*)branch, branch ? h : nullptr, y_op, pk_enc);
      if (!branch) return launch_layernorm(prec, h, 1, rows, D, g_, b_, eps, 0, y_op, y_f32, s, nullptr, nullptr);
      if (!tmp_f32)  // x = bf16 branch, add = fp32 residual, sumF = residual updated in place
        return launch_layernorm(prec, branch, 0, rows, D, g_, b_, eps, 0, y_op, y_f32, s, h, y_op ? h : nullptr);
      return launch_layernorm(y_op ? prec : 0, h, 1, rows, D, g_, b_, eps, 0, y_op ? y_op : (void*)y_f32, nullptr, s,
                              (const float*)branch, y_op ? h : nullptr);
    };
    for (int l = 0; l < c.num_layers; ++l) {
      const EncLayerW& Lw = e->layers[l];
      if (int r = ln_add(Lw.ln1g.as<float>(), Lw.ln1b.as<float>(), pending, w.xb, nullptr)) return r;
      if (int r = gemm_rows(w.xb, D, Lw.wqkv, Lw.bqkv, 3 * D, w.qkv, 0, ACT_NONE, nullptr, qkv_pl)) return r;
      if (int r = attention()) return r;
      if (int r = gemm_rows(w.attn_o, D, Lw.wo, Lw.bo, D, tmp, tmp_f32, ACT_NONE, nullptr)) return r;
      if (int r = ln_add(Lw.ln2g.as<float>(), Lw.ln2b.as<float>(), tmp, w.xb, nullptr)) return r;
      if (int r = gemm_rows(w.xb, D, Lw.w1, Lw.b1, F, w.ffn, 0, ACT_GELU, nullptr, nullptr, pk_enc ? 1 : 0)) return r;
      if (int r = gemm_rows(w.ffn, F, Lw.w2, Lw.b2, D, tmp, tmp_f32, ACT_NONE, nullptr)) return r;
      pending = tmp;
    }
    // final LN(h + last FFN branch) -> fp32 (xF is unused in this family when prec == 0 it aliases xb: use qkv space)
    float* fin = (float*)w.qkv;
    if (int r = ln_add(e->enc_g.as<float>(), e->enc_b.as<float>(), pending, nullptr, fin)) return r;
    final_x = fin;
  }
  // ---- wrapper's whole-batch output LayerNorm (+ frame head + decode when a head was given) ----
  const int64_t n_out = rows * D;
  const double n_out_stat = global_norm ? (double)e->reduce_global_clips * (double)(rows / B) * (double)D : 0.0;
  rctx.mom = out_mom;
  if (tail.head) {
    static_assert(sizeof(svt_frame) == sizeof(FrameOut), "frame layout");
    if (launch_head_fused(final_x, rows, D, tail.head->w.as<float>(), tail.head->wsum.as<float>(),
                          tail.head->has_bias ? tail.head->b.as<float>() : nullptr, tail.head->out_f, w.dots,
                          c.output_norm ? out_mom : nullptr, rows / groups, 1e-5f, tail.logits, (FrameOut*)tail.frames, tail.n_oct,
                          tail.n_cls, s, n_out_stat, global_norm && c.output_norm ? +reduce_now : nullptr, &rctx,
                          (char*)w.mom + w.mom_scr[3])) return SVT_ERR_HIP;
    return SVT_OK;
  }
  if (c.output_norm) {
    if (int r = launch_moments(final_x, n_out / groups, out_mom, (char*)w.mom + w.mom_scr[1], B, s, groups)) return r;
    if (global_norm) { if (int r = reduce_now(&rctx)) return r; }
    if (int r = launch_global_norm(final_x, feats, n_out / groups, out_mom, 1e-5f, s, groups, n_out_stat)) return r;
  } else {
    if (launch_copy_f32(final_x, feats, n_out, s)) return SVT_ERR_HIP;
  }
  return SVT_OK;
}
