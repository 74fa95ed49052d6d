// C ABI of the encoder (include/svt_mi355.h): parameter intake by HF key, the one-time re-layout / fold / cast at finalize, workspace
// carving and the launch sequence of a forward, with or without the fused frame-head tail.  Host code only: no allocation and no
// synchronisation inside a forward call.
//   finalize: finalize_conv_stack -> finalize_projection -> finalize_pos_conv(_stack) -> encoder LayerNorm -> finalize_layer
//   forward:  plan_encoder (plan_attention) -> carve_encoder -> input_statistics -> choose_pair_rows -> conv_layer0 -> conv_stack -> feature_projection
//             [-> spec_augment] -> positional_conv -> encoder_layers (post_ln_layers / pre_ln_layers) -> forward_tail
//   training mode (svt_encoder_set_dropout): drop_rows / launch_dropout_hilo / the softmax form at the six sites of the header, skipped layers launch nothing
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
  DevBuf w_kperm;   // 16-bit modes, kernel 3 / stride 2: the same matrix with its K axis in tap-minor slab order (finalize_conv_stack)
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
  // optional SpecAugment masks (svt_encoder_set_spec_augment): caller-owned device bytes, the geometry they were made for, and the
  // parameter "masked_spec_embed" (fp32; empty when the checkpoint had none)
  const uint8_t* sa_time = nullptr;
  const uint8_t* sa_feat = nullptr;
  int sa_B = 0, sa_T = 0;
  DevBuf spec_embed;
  // optional training-mode state (svt_encoder_set_dropout): rates, (seed, step) and the skipped layers of the forwards to come
  bool drop_on = false;
  svt_dropout drop = {};
};

// every mode but plain fp32 (16-bit storage, or fp32 storage with split-operand products): conv layer 0 on the matrix pipe, the
// multi-frame positional conv, and a residual stream kept in fp32 beside the products' operand copy
static bool reduced_mode(const svt_encoder_config& c) { return c.precision != SVT_PREC_FP32; }

// frames the conv stack makes of n_samples (features-in mode: n_samples itself), 0 for a waveform shorter than the receptive field;
// frames[i] = output frames of conv layer i
static int64_t conv_frames(const svt_encoder_config& c, int64_t n_samples, int64_t* frames = nullptr) {
  int64_t t = n_samples;
  for (int i = 0; i < c.num_conv_layers; ++i) {
    if (t < c.conv_kernel[i]) return 0;
    t = (t - c.conv_kernel[i]) / c.conv_stride[i] + 1;
    if (frames) frames[i] = t;
  }
  return t;
}

// ---------------------------------------------------------------- finalize: one step per parameter group
namespace {

int finalize_conv_stack(svt_encoder* e) {
  const svt_encoder_config& c = e->cfg;
  const ParamMap& P = e->params;
  if ((int)e->conv.size() != c.num_conv_layers) { e->conv.clear(); e->conv.resize(c.num_conv_layers); }   // a re-upload keeps the buffers
  int cin = 1;
  for (int i = 0; i < c.num_conv_layers; ++i) {
    const std::string pre = "feature_extractor.conv_layers." + std::to_string(i) + ".";
    const int co = c.conv_dim[i], k = c.conv_kernel[i];
    const Param* p = nullptr;
    if (int r = need(P, pre + "conv.weight", {co, cin, k}, &p)) return r;
    ConvLayerW& L = e->conv[i];
    if (i == 0) {
      if (int r = upload_f32(L.w, p->v.data(), p->v.size())) return r;
    } else {
      const std::vector<float> wt = tap_major(p->v.data(), co, cin, k);
      if (int r = upload_weight(c.precision, L.w, wt.data(), (size_t)co, (size_t)k * cin)) return r;
      // 16-bit modes, kernel 3: a second copy with the K axis in TAP-MINOR slab order -- slab g = tap g % 3 of channels [(g / 3) * 64, + 64)
      // -- for gemm_p1w_kernel (GemmArgs::k_taps): the input frame two neighbouring output rows share is re-read two slabs later instead
      // of sixteen, i.e. out of L2 (1.5 MiB per layer)
      if (storage_prec(c.precision) && k == 3 && cin % 64 == 0 && c.conv_stride[i] == 2) {
        const std::vector<float> wp = tap_minor_slabs(wt.data(), co, cin, k);
        if (int r = upload_weight(c.precision, L.w_kperm, wp.data(), (size_t)co, (size_t)k * cin)) return r;
      } else L.w_kperm.release();
    }
    if (c.conv_bias)
      if (int r = upload_vec(P, pre + "conv.bias", co, &L.bias)) return r;
    if (c.feat_extract_norm == SVT_NORM_LAYER || i == 0) {
      if (int r = upload_vec(P, pre + "layer_norm.weight", co, &L.gamma)) return r;
      if (int r = upload_vec(P, pre + "layer_norm.bias", co, &L.beta)) return r;
    }
    cin = co;
  }
  return SVT_OK;
}

int finalize_projection(svt_encoder* e) {
  const svt_encoder_config& c = e->cfg;
  const ParamMap& P = e->params;
  const int cin = c.conv_dim[c.num_conv_layers > 0 ? c.num_conv_layers - 1 : 0];   // features-in mode: the projection reads the given features
  if (c.feat_proj_layer_norm) {
    if (int r = upload_vec(P, "feature_projection.layer_norm.weight", cin, &e->fp_g)) return r;
    if (int r = upload_vec(P, "feature_projection.layer_norm.bias", cin, &e->fp_b)) return r;
  }
  if (int r = upload_mat(c.precision, P, "feature_projection.projection.weight", c.hidden_size, cin, &e->proj_w)) return r;
  return upload_vec(P, "feature_projection.projection.bias", c.hidden_size, &e->proj_b);
}

// data2vec-audio: plain grouped convs "encoder.pos_conv_embed.layers.<i>.conv.{weight,bias}", (D, cg, kp) -> per group
// (cg_out, kp*cg_in) tap-major like the single-layer form
int finalize_pos_conv_stack(svt_encoder* e) {
  const svt_encoder_config& c = e->cfg;
  const ParamMap& P = e->params;
  const int D = c.hidden_size, kp = c.pos_conv_kernel, cg = D / c.pos_conv_groups;
  if ((int)e->pos_ws.size() != c.pos_conv_depth) { e->pos_ws.clear(); e->pos_bs.clear(); e->pos_ws.resize(c.pos_conv_depth); e->pos_bs.resize(c.pos_conv_depth); }
  for (int i = 0; i < c.pos_conv_depth; ++i) {
    const std::string pl = "encoder.pos_conv_embed.layers." + std::to_string(i) + ".conv.";
    const Param* p = nullptr;
    if (int r = need(P, pl + "weight", {D, cg, kp}, &p)) return r;
    const std::vector<float> wt = tap_major(p->v.data(), D, cg, kp);
    if (int r = upload_operand(storage_prec(c.precision), e->pos_ws[i], wt.data(), wt.size())) return r;
    if (int r = upload_vec(P, pl + "bias", D, &e->pos_bs[i])) return r;
  }
  const std::vector<float> one((size_t)D, 1.f), zero((size_t)D, 0.f);
  if (int r = upload_f32(e->ones, one.data(), one.size())) return r;
  if (int r = upload_f32(e->zeros, zero.data(), zero.size())) return r;
  e->pos_P = 0;
  return SVT_OK;
}

// the single positional conv: weight-norm (dim=2) folded, W[:,:,j] = g[j] v[:,:,j] / ||v[:,:,j]||_F ; both spellings are accepted
int pos_conv_weight(const svt_encoder* e, std::vector<float>* w) {
  const svt_encoder_config& c = e->cfg;
  const ParamMap& P = e->params;
  const int D = c.hidden_size, kp = c.pos_conv_kernel, cg = D / c.pos_conv_groups;
  const std::string pc = "encoder.pos_conv_embed.conv.";
  const Param *g = find(P, pc + "parametrizations.weight.original0"), *v = find(P, pc + "parametrizations.weight.original1");
  if (!g || !v) { g = find(P, pc + "weight_g"); v = find(P, pc + "weight_v"); }
  if (g && v) {
    if (g->numel() != kp || v->shape != std::vector<int64_t>({D, cg, kp})) { set_error("pos_conv weight-norm tensors have the wrong shape"); return SVT_ERR_INVALID; }
    *w = weight_norm_fold(g->v.data(), v->v.data(), v->v.size(), kp);
  } else if (const Param* pw = find(P, pc + "weight")) {
    if (pw->shape != std::vector<int64_t>({D, cg, kp})) { set_error("pos_conv weight has the wrong shape"); return SVT_ERR_INVALID; }
    *w = pw->v;
  } else {
    set_error("missing parameter: " + pc + "parametrizations.weight.original0/1 (or weight_g/weight_v)");
    return SVT_ERR_KEY;
  }
  return SVT_OK;
}

int finalize_pos_conv(svt_encoder* e) {
  const svt_encoder_config& c = e->cfg;
  const ParamMap& P = e->params;
  const int prec = storage_prec(c.precision);
  const int D = c.hidden_size, kp = c.pos_conv_kernel, G = c.pos_conv_groups, cg = D / G;
  std::vector<float> w;
  if (int r = pos_conv_weight(e, &w)) return r;
  // (D, cg, kp) -> per group (cg_out, kp*cg_in) tap-major
  const std::vector<float> wt = tap_major(w.data(), D, cg, kp);
  if (int r = upload_operand(prec, e->pos_w, wt.data(), wt.size())) return r;
  const Param* bias = nullptr;
  if (int r = need(P, "encoder.pos_conv_embed.conv.bias", {D}, &bias)) return r;
  if (int r = upload_f32(e->pos_b, bias->v.data(), bias->v.size())) return r;
  if (c.pos_conv_batch_norm) {
    // y = (x - running_mean) / sqrt(running_var + 1e-5) * weight + bias   (nn.BatchNorm1d defaults, eval mode)
    const std::string bn = "encoder.pos_conv_embed.batch_norm.";
    const Param *bw, *bb, *bm, *bv;
    if (int r = need(P, bn + "weight", {D}, &bw)) return r;
    if (int r = need(P, bn + "bias", {D}, &bb)) return r;
    if (int r = need(P, bn + "running_mean", {D}, &bm)) return r;
    if (int r = need(P, bn + "running_var", {D}, &bv)) return r;
    std::vector<float> sc, sh;
    batch_norm_fold(bw->v.data(), bb->v.data(), bm->v.data(), bv->v.data(), D, &sc, &sh);
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
  if (reduced_mode(c) && Pf >= 2 && cg % 8 == 0 && ((kp + Pf - 1) * cg) % 64 == 0) {
    std::vector<float> wp, bp;
    posconv_multiframe(w.data(), bias->v.data(), G, cg, kp, Pf, &wp, &bp);
    if (prec) { if (int r = upload_operand(1, e->pos_wP, wp.data(), wp.size())) return r; }
    else { if (int r = upload_weight(c.precision, e->pos_wP, wp.data(), (size_t)G * Pf * cg, (size_t)(kp + Pf - 1) * cg)) return r; }
    if (int r = upload_f32(e->pos_bP, bp.data(), bp.size())) return r;
    e->pos_P = Pf;
  }
  return SVT_OK;
}

int finalize_layer(svt_encoder* e, int l) {
  const svt_encoder_config& c = e->cfg;
  const ParamMap& P = e->params;
  const int D = c.hidden_size, F = c.intermediate_size, gp = c.precision;
  const std::string pre = "encoder.layers." + std::to_string(l) + ".";
  EncLayerW& L = e->layers[l];
  // q, k and v projections packed into one (3D, D) product
  std::vector<float> wqkv((size_t)3 * D * D), bqkv((size_t)3 * D);
  const char* names[3] = {"q_proj", "k_proj", "v_proj"};
  for (int i = 0; i < 3; ++i) {
    const Param* p = nullptr;
    if (int r = need(P, pre + "attention." + names[i] + ".weight", {D, D}, &p)) return r;
    memcpy(wqkv.data() + (size_t)i * D * D, p->v.data(), (size_t)D * D * 4);
    if (int r = need(P, pre + "attention." + names[i] + ".bias", {D}, &p)) return r;
    memcpy(bqkv.data() + (size_t)i * D, p->v.data(), (size_t)D * 4);
  }
  if (int r = upload_weight(gp, L.wqkv, wqkv.data(), (size_t)3 * D, (size_t)D)) return r;
  if (int r = upload_f32(L.bqkv, bqkv.data(), bqkv.size())) return r;
  if (int r = upload_mat(gp, P, pre + "attention.out_proj.weight", D, D, &L.wo)) return r;
  if (int r = upload_vec(P, pre + "attention.out_proj.bias", D, &L.bo)) return r;
  if (int r = upload_vec(P, pre + "layer_norm.weight", D, &L.ln1g)) return r;
  if (int r = upload_vec(P, pre + "layer_norm.bias", D, &L.ln1b)) return r;
  if (int r = upload_mat(gp, P, pre + "feed_forward.intermediate_dense.weight", F, D, &L.w1)) return r;
  if (int r = upload_vec(P, pre + "feed_forward.intermediate_dense.bias", F, &L.b1)) return r;
  if (int r = upload_mat(gp, P, pre + "feed_forward.output_dense.weight", D, F, &L.w2)) return r;
  if (int r = upload_vec(P, pre + "feed_forward.output_dense.bias", D, &L.b2)) return r;
  if (int r = upload_vec(P, pre + "final_layer_norm.weight", D, &L.ln2g)) return r;
  if (int r = upload_vec(P, pre + "final_layer_norm.bias", D, &L.ln2b)) return r;
  if (!c.rel_pos_buckets) return SVT_OK;
  // gate = a (b const - 1) + 2, a / b = sigmoid of the sums of rows 0-3 / 4-7 of gru_rel_pos_linear(x_head): fold the row sums
  const int H = c.num_heads, dh = D / H;
  const Param *gw = nullptr, *gb = nullptr, *gc = nullptr;
  if (int r = need(P, pre + "attention.gru_rel_pos_linear.weight", {8, dh}, &gw)) return r;
  if (int r = need(P, pre + "attention.gru_rel_pos_linear.bias", {8}, &gb)) return r;
  if (int r = need(P, pre + "attention.gru_rel_pos_const", {1, H, 1, 1}, &gc)) return r;
  std::vector<float> wab, bab;
  gate_rowsum_fold(gw->v.data(), gb->v.data(), dh, &wab, &bab);
  if (int r = upload_f32(L.g_wab, wab.data(), wab.size())) return r;
  if (int r = upload_f32(L.g_bab, bab.data(), bab.size())) return r;
  if (int r = upload_f32(L.g_const, gc->v.data(), gc->v.size())) return r;
  if (l == 0) {
    const Param* p = nullptr;
    if (int r = need(P, pre + "attention.rel_attn_embed.weight", {c.rel_pos_buckets, H}, &p)) return r;
    if (int r = upload_f32(e->rel_embed, p->v.data(), p->v.size())) return r;
  }
  return SVT_OK;
}

}  // namespace

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

int svt_encoder_set_spec_augment(svt_encoder* e, const uint8_t* time_mask, const uint8_t* feature_mask, int32_t batch, int32_t frames) {
  if (!e) { set_error("svt_encoder_set_spec_augment: null encoder"); return SVT_ERR_INVALID; }
  if (!time_mask && !feature_mask) { e->sa_time = e->sa_feat = nullptr; e->sa_B = e->sa_T = 0; return SVT_OK; }
  if (batch < 1 || frames < 1) { set_error("svt_encoder_set_spec_augment: batch and frames are the geometry the masks were made for"); return SVT_ERR_INVALID; }
  if ((uintptr_t)feature_mask & 3) { set_error("svt_encoder_set_spec_augment: feature_mask_dev must be 4-byte aligned"); return SVT_ERR_INVALID; }
  if (e->cfg.hidden_size % 4) { set_error("svt_encoder_set_spec_augment: hidden_size must be a multiple of 4"); return SVT_ERR_INVALID; }
  if (time_mask && !find(e->params, "masked_spec_embed")) {
    set_error("svt_encoder_set_spec_augment: a time mask needs the parameter masked_spec_embed, which this encoder never received");
    return SVT_ERR_KEY;
  }
  e->sa_time = time_mask; e->sa_feat = feature_mask; e->sa_B = batch; e->sa_T = frames;
  return SVT_OK;
}

int svt_encoder_set_dropout(svt_encoder* e, const svt_dropout* st) {
  auto refuse = [](const std::string& why) { set_error("svt_encoder_set_dropout: " + why); return SVT_ERR_INVALID; };
  if (!e) return refuse("null encoder");
  if (!st) { e->drop_on = false; e->drop = svt_dropout{}; return SVT_OK; }
  // the structure as it was before fused_attention was appended is accepted and means 0
  const bool old_size = st->struct_size == (int32_t)offsetof(svt_dropout, fused_attention);
  if (!old_size && st->struct_size != (int32_t)sizeof(svt_dropout)) return refuse("struct_size");
  const svt_encoder_config& c = e->cfg;
  const double rates[5] = {st->feat_proj_dropout, st->hidden_dropout, st->attention_dropout, st->activation_dropout, st->layerdrop};
  for (double r : rates)
    if (!(r >= 0.0 && r < 1.0)) return refuse("every rate must lie in [0, 1)");
  if (st->skip_mask && c.num_layers > 64) return refuse("the skip bitmask serves up to 64 layers");
  if (c.num_layers < 64 && (st->skip_mask >> c.num_layers)) return refuse("skip_mask names a layer at or above num_layers");
  const bool elem = st->feat_proj_dropout > 0 || st->hidden_dropout > 0 || st->attention_dropout > 0 || st->activation_dropout > 0;
  if (elem && c.precision >= 2)
    return refuse(std::string("precision ") + (c.precision == SVT_PREC_FP16X3 ? "fp16x3" : "bf16x3") +
                  " serves layerdrop only: the split-operand modes keep their activations as pair rows, which the dropout kernels do not "
                  "read; use fp32, bf16 or fp16 for a nonzero element dropout");
  if (st->attention_dropout > 0 && c.rel_pos_buckets > 0)
    return refuse("attention_dropout > 0 with a relative position bias (WavLM) is not served: the reference runs torch's fused multi-head "
                  "attention there, which offers no seam to pin a mask against; set attention_dropout to 0");
  const uint64_t all_layers = c.num_layers >= 64 ? ~0ull : ((1ull << c.num_layers) - 1);
  if ((st->skip_mask & 1) && c.rel_pos_buckets > 0 && (st->skip_mask & all_layers) != all_layers)
    return refuse("layer 0 of an encoder with a relative position bias (WavLM) cannot be skipped: only that layer holds the position "
                  "embedding, and the reference fails in the next layer");
  e->drop = svt_dropout{};
  memcpy(&e->drop, st, (size_t)st->struct_size);
  e->drop.struct_size = (int32_t)sizeof(svt_dropout);
  e->drop_on = true;
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
  if (int r = finalize_conv_stack(e)) return r;
  if (int r = finalize_projection(e)) return r;
  if (int r = c.pos_conv_depth > 1 ? finalize_pos_conv_stack(e) : finalize_pos_conv(e)) return r;
  if (int r = upload_vec(e->params, "encoder.layer_norm.weight", c.hidden_size, &e->enc_g)) return r;
  if (int r = upload_vec(e->params, "encoder.layer_norm.bias", c.hidden_size, &e->enc_b)) return r;
  if (find(e->params, "masked_spec_embed")) {   // optional: only svt_encoder_set_spec_augment reads it
    if (int r = upload_vec(e->params, "masked_spec_embed", c.hidden_size, &e->spec_embed)) return r;
  } else e->spec_embed.release();
  if ((int)e->layers.size() != c.num_layers) { e->layers.clear(); e->layers.resize(c.num_layers); }
  for (int l = 0; l < c.num_layers; ++l)
    if (int r = finalize_layer(e, l)) return r;
  SVT_HIP(hipDeviceSynchronize());
  e->finalized = true;
  return SVT_OK;
}

int64_t svt_encoder_num_frames(const svt_encoder* e, int64_t n_samples) {
  return e ? conv_frames(e->cfg, n_samples) : -1;
}

}  // extern "C"

// ---------------------------------------------------------------- plan and workspace of a forward
namespace {

// FFN-2 of a small batch splits K four ways over workgroups and leaves the sum to the LayerNorm behind it (gemm_skinny.hip, ksplit;
// svt_debug_set key 36 = 0 switches it off): up to this many rows (8 utterances of 5 s)
const size_t kKsplitMaxRows = 2048;

// Everything a forward of (encoder, B, L) decides from the configuration alone, computed once: carve_encoder, svt_debug_encoder_layout
// and every stage of the forward read it.  (The pair-row decisions also need buffer addresses: choose_pair_rows, after the carve.)
struct EncPlan {
  int B = 0;
  int64_t L = 0;
  int64_t frames[SVT_MAX_CONV_LAYERS] = {};   // output frames of conv layer i
  int64_t t1 = 1;          // frames of conv layer 0 (1 in features-in mode)
  int64_t T = 0, rows = 0; // encoder frames per clip (features-in mode: L), B * T
  int C = 0;               // width of the feature projection's input
  int D = 0, F = 0, H = 0, dh = 0;
  int sp = 0;              // storage type of activations / weights (storage_prec)
  int gp = 0;              // engine of the dense products (launch_gemm)
  bool reduced = false;    // reduced_mode()
  bool rel = false;        // WavLM relative position bias
  AttnPlan attn;           // the layers' attention: its path and the buffers it needs (plan_attention); on ATTN_FUSED_X3 the QKV
                           // projection's epilogue writes the (hi, lo) planes the kernel reads
  int Pf = 0;              // frames per row of the multi-frame positional conv the encoder holds (0: none)
  int64_t pos_Tq = 0;      // ... its GEMM rows per clip
  int64_t pos_Tp = 0;      // frames per clip the gathered positional-conv input is carved for: pos_Tq * Pf + kernel (multi-frame), else T + kernel
  bool pos_multi = false;  // this batch has enough rows for the multi-frame form
  bool hilo = false;       // post-LN encoder with the residual stream as a bf16 (hi, lo) pair
  bool ksplit_ws = false;  // few enough rows for the K-split FFN-2: its partial products get workspace
  bool attn_drop = false;  // training mode with attention_dropout > 0: the score-matrix attention for every geometry, unless
                           // svt_dropout.fused_attention opted in and the plain forward runs a fused 16-bit kernel: its masked form
};

// false: the waveform is shorter than the receptive field
bool plan_encoder(const svt_encoder* e, int B, int64_t L, EncPlan* out) {
  const svt_encoder_config& c = e->cfg;
  EncPlan p;
  p.B = B; p.L = L;
  p.T = conv_frames(c, L, p.frames);
  if (p.T < 1) return false;
  p.rows = (int64_t)B * p.T;
  p.t1 = c.num_conv_layers > 0 ? p.frames[0] : 1;
  p.C = c.conv_dim[c.num_conv_layers > 0 ? c.num_conv_layers - 1 : 0];
  p.D = c.hidden_size; p.F = c.intermediate_size; p.H = c.num_heads; p.dh = p.D / p.H;
  p.sp = storage_prec(c.precision); p.gp = c.precision; p.reduced = reduced_mode(c);
  p.rel = c.rel_pos_buckets > 0;
  p.attn_drop = e->drop_on && e->drop.attention_dropout > 0;
  AttnGeom ag;   // attention_block's call: q | k | v are the columns of one (rows, 3D) projection
  ag.prec = p.sp; ag.gp = p.gp; ag.dh = p.dh; ag.T = p.T; ag.bias = p.rel;
  ag.drop = p.attn_drop; ag.fused_drop = e->drop.fused_attention != 0;
  ag.packed_kv = ag.q_packed = true;
  p.attn = plan_attention(ag);
  p.Pf = e->pos_P;
  p.pos_Tq = p.Pf ? (p.T + p.Pf - 1) / p.Pf : 0;
  p.pos_Tp = p.Pf ? p.pos_Tq * p.Pf + c.pos_conv_kernel : p.T + c.pos_conv_kernel;
  p.pos_multi = p.Pf && (int64_t)B * p.pos_Tq >= 128;
  p.hilo = !c.stable_layer_norm && p.sp && layernorm_hilo_ok(p.D) && c.num_layers > 0;
  p.ksplit_ws = p.sp && (size_t)p.rows <= kKsplitMaxRows;
  *out = p;
  return true;
}

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

EncWs carve_encoder(const svt_encoder* e, const EncPlan& p, void* base) {
  const svt_encoder_config& c = e->cfg;
  const size_t es = esize(p.sp);
  const size_t B = (size_t)p.B, rows = (size_t)p.rows, T = (size_t)p.T, D = (size_t)p.D, H = (size_t)p.H;
  Carver cv(base);
  EncWs w;
  // 2 x (sum, sumsq) per norm group (<= B groups) + conv0 window moments, then the scratch of the three ordered sums (tickets + per-workgroup
  // partials: stats.hip, last_workgroup); the whole region is zeroed at the start of every forward (the tickets must be)
  w.mom_scr[0] = align_up((4 * B + B * 65) * sizeof(double));
  w.mom_scr[1] = w.mom_scr[0] + align_up(moments_scratch_bytes(p.B));
  w.mom_scr[2] = w.mom_scr[1] + align_up(moments_scratch_bytes(p.B));
  w.mom_scr[3] = w.mom_scr[2] + align_up(conv0_window_moments_scratch_bytes(p.B, p.t1));
  w.mom_zero = w.mom_scr[3] + 256;   // ... up to and including the fused tail's ticket: what a forward zeroes
  w.mom_bytes = w.mom_scr[3] + align_up(head_scratch_bytes(p.rows, p.B));
  w.mom = (double*)cv.take(w.mom_bytes);
  w.coef = (float*)cv.take(B * c.conv_dim[0] * 11 * 4);
  w.c0tab = p.reduced ? cv.take(conv0_mfma_table_bytes(p.B)) : nullptr;
  size_t max_act = 0, max_f = 0;
  for (int i = 0; i < c.num_conv_layers; ++i) {
    const size_t n = B * p.frames[i] * c.conv_dim[i];
    if (n * es > max_act) max_act = n * es;
    if (i > 0 && n * 4 > max_f) max_f = n * 4;
  }
  if (c.num_conv_layers == 0) max_act = rows * c.conv_dim[0] * es;
  w.act[0] = cv.take(max_act);
  w.act[1] = cv.take(max_act);
  w.convF = c.feat_extract_norm == SVT_NORM_LAYER ? (float*)cv.take(max_f) : nullptr;
  w.xln = cv.take(rows * p.C * es);
  w.hF = (float*)cv.take(rows * D * 4);
  w.preF = (float*)cv.take(rows * D * 4);
  w.xb = cv.take(rows * D * es);
  // reduced modes: xb holds the layer input in the products' operand form and xF the fp32 residual stream beside it; in plain fp32 they
  // are one buffer (the split modes without pair rows use xb alone all the same: choose_pair_rows)
  w.xF = p.reduced ? (float*)cv.take(rows * D * 4) : (float*)w.xb;
  w.xlo = p.sp ? cv.take(rows * D * 2) : nullptr;  // low half of the (hi, lo) bf16 residual stream (post-LN, bf16 mode)
  w.posg = cv.take(B * p.pos_Tp * D * es);
  w.posy = p.Pf ? cv.take(B * p.pos_Tq * p.Pf * D * es) : nullptr;
  w.qkv = cv.take(rows * 3 * D * es);
  // (kept on purpose: V^T is carved on the fused paths too, where nothing reads it -- attn_workspace_plan)
  w.ab = carve_attention(cv, attn_workspace_plan(p.attn, false), B, H, T, (size_t)p.dh, es);
  w.attn_o = cv.take(rows * D * es);
  w.ffn = cv.take(rows * p.F * es);
  w.gate = p.rel ? (float*)cv.take(B * H * T * 4) : nullptr;
  w.relpb = p.rel ? (float*)cv.take(H * (2 * T - 1) * 4) : nullptr;
  w.dots = (float*)cv.take(rows * 32 * 4);
  w.ksplit = p.ksplit_ws ? (float*)cv.take((size_t)4 * rows * D * 4) : nullptr;
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
  EncPlan p;
  if (!plan_encoder(e, batch, n_samples, &p)) { set_error("waveform shorter than the receptive field"); return SVT_ERR_INVALID; }
  char* const fake = (char*)(uintptr_t)(1ull << 40);   // never dereferenced: carve_encoder only adds offsets to it
  const EncWs w = carve_encoder(e, p, fake);
  const void* r[24] = {w.mom, w.coef, w.c0tab, w.act[0], w.act[1], w.convF, w.xln, w.hF, w.preF, w.xb, w.xF, w.xlo, w.posg, w.posy, w.qkv,
                       w.ab.S, w.ab.P, w.ab.Vt, w.ab.pl_qkv, w.attn_o, w.ffn, w.gate, w.relpb, w.dots};
  int k = 0;
  for (; k < 24 && k < n; ++k) offsets[k] = r[k] == nullptr ? -1 : (int64_t)((const char*)r[k] - fake);
  if (k < n) offsets[k++] = (int64_t)w.total;
  return k;
}

int64_t svt_encoder_workspace_bytes(const svt_encoder* e, int32_t batch, int64_t n_samples) {
  if (!e || batch < 1) { set_error("workspace_bytes: bad argument"); return -1; }
  EncPlan p;
  if (!plan_encoder(e, batch, n_samples, &p)) { set_error("waveform shorter than the receptive field"); return -1; }
  return (int64_t)carve_encoder(e, p, nullptr).total;
}

}  // extern "C"

// ---------------------------------------------------------------- the forward, stage by stage
namespace {

struct ReduceCtx { const svt_encoder* e; double* mom; hipStream_t s; };
// "global-batch-equivalent" norms (optional): the batch is a shard of a larger one; the caller's function sums the
// (sum, sum of squares) pair over the ranks -- 16 bytes per norm -- and the statistics are then those of the whole global batch
int reduce_now(void* a) {
  ReduceCtx* rc = (ReduceCtx*)a;
  if (rc->e->reduce_fn(rc->mom, 2, (void*)rc->s, rc->e->reduce_user)) { set_error("encoder_forward: the norm-reduce callback reported an error"); return SVT_ERR_INVALID; }
  return 0;
}

// one forward in flight: what every stage reads
struct EncRun {
  const svt_encoder* e;
  const svt_encoder_config& c;
  const EncPlan& p;
  EncWs w;
  hipStream_t s;
  // the wrapper's two whole-tensor layer norms run over groups of `cpg` consecutive clips: cpg = B is the reference on a
  // batch (and per device shard under DataParallel / DDP), cpg = 1 makes a batch of B clips equal to B batch-1 forwards --
  // the reference's evaluation loop (train_audio_ssl.py:90 asserts batch 1) without its one-utterance-at-a-time cost
  int cpg = 0, groups = 1;
  // input_statistics
  double* wav_mom = nullptr;   // 2 per group, or null without the input norm
  double* out_mom = nullptr;
  double* win_mom = nullptr;   // conv layer 0 window moments
  int64_t n_wav = 0;           // samples behind one pair of wav_mom
  bool global_norm = false;
  ReduceCtx rctx{nullptr, nullptr, nullptr};
  // choose_pair_rows
  int pk_front = 0, pk_enc = 0;  // pair rows (kind of the pieces: 2 = bf16, 3 = fp16; 0 = none) for conv 1..n-1 + the feature projection / the encoder layers
  float* resid = nullptr;      // the fp32 residual stream of the encoder layers: w.xF, or w.xb where the layer input is itself fp32
  // training mode (svt_encoder_set_dropout), or null: the plain forward
  const svt_dropout* drop = nullptr;
  bool skipped(int l) const { return drop && l < 64 && ((drop->skip_mask >> l) & 1); }
  int last_active() const {    // the last layer that runs, -1: none
    for (int l = c.num_layers - 1; l >= 0; --l) if (!skipped(l)) return l;
    return -1;
  }
};

// one dropout site on a whole (rows, W) tensor, in place; kind 0 = fp32, 1 = the 16-bit operand type.  rate 0: nothing is launched
int drop_rows(const EncRun& x, int site, int layer, double p, void* buf, int kind, int64_t n) {
  if (!x.drop || !(p > 0)) return SVT_OK;
  return launch_dropout_rows(kind, buf, n, 0, make_drop_spec(p, x.drop->seed, x.drop->step, site, layer), x.s) ? SVT_ERR_HIP : SVT_OK;
}

LnArgs ln_f32(const EncRun& x, const void* in, int64_t rows, int D, const DevBuf& gamma, const DevBuf& beta, float eps) {
  LnArgs a;
  a.prec = x.p.sp; a.x = in; a.rows = rows; a.D = D; a.gamma = gamma.as<float>(); a.beta = beta.as<float>(); a.eps = eps;
  return a;
}

// the checks that need the batch: norm groups
int check_norm_groups(EncRun& x, int32_t clips_per_norm_group) {
  const svt_encoder_config& c = x.c;
  x.cpg = clips_per_norm_group > 0 ? clips_per_norm_group : x.p.B;
  if (x.p.B % x.cpg) { set_error("encoder_forward: batch must be a multiple of clips_per_norm_group"); return SVT_ERR_INVALID; }
  x.groups = x.p.B / x.cpg;
  if (x.groups > 1 && c.num_conv_layers > 0 && (x.p.L & 3)) {
    set_error("encoder_forward: norm groups need a waveform length that is a multiple of 4 samples");
    return SVT_ERR_INVALID;
  }
  if (x.groups > 1 && c.num_conv_layers == 0 && c.normalize_wav) {
    set_error("encoder_forward: features-in mode has no input norm to group");
    return SVT_ERR_INVALID;
  }
  return SVT_OK;
}

// zeroes the statistics region, takes the waveform moments and (optionally) reduces them over the ranks
int input_statistics(EncRun& x, const float* wav) {
  const svt_encoder_config& c = x.c;
  const EncWs& w = x.w;
  const size_t B = (size_t)x.p.B;
  if (launch_zero_bytes(w.mom, w.mom_zero, x.s)) return SVT_ERR_HIP;   // (a kernel, not a memset node: see encoder_ops.hip)
  x.wav_mom = c.normalize_wav ? w.mom : nullptr;
  x.out_mom = w.mom + 2 * B;
  x.win_mom = w.mom + 4 * B;
  x.n_wav = (int64_t)x.cpg * x.p.L;
  if (c.normalize_wav)
    if (int r = launch_moments(wav, x.n_wav, x.wav_mom, (char*)w.mom + w.mom_scr[0], x.p.B, x.s, x.groups)) return r;
  x.rctx = ReduceCtx{x.e, nullptr, x.s};
  x.global_norm = x.e->reduce_fn != nullptr;
  if (x.global_norm) {
    if (x.groups != 1) { set_error("encoder_forward: the cross-rank norm reduction applies to whole-batch norms (clips_per_norm_group = 0)"); return SVT_ERR_INVALID; }
    if (x.e->reduce_global_clips < x.p.B) { set_error("encoder_forward: global_clips of the norm reduction is smaller than this batch"); return SVT_ERR_INVALID; }
    if (c.normalize_wav) {
      x.rctx.mom = x.wav_mom;
      if (int r = reduce_now(&x.rctx)) return r;
      x.n_wav = x.e->reduce_global_clips * x.p.L;
    }
  }
  return SVT_OK;
}

bool x3q_fits(const void* A, int M, int N, int K, int a_rpb, long a_bstride, long a_rstride, const void* Wp, int c_pairs, long ldc) {
  GemmArgs g;
  g.A = A; g.W = Wp; g.C = const_cast<void*>(A); g.M = M; g.N = N; g.K = K; g.a_rpb = a_rpb; g.a_bstride = a_bstride; g.a_rstride = a_rstride;
  g.ldw = K; g.ldc = ldc; g.a_pairs = 1; g.c_pairs = c_pairs;
  return gemm_x3q_eligible(g);
}

// Split modes: which products take PAIR ROWS (gemm_x3q.hip: operands cut by their producers).  front = conv 1..n-1 and the feature
// projection, enc = the four products of every encoder layer; a section switches as a whole, and only when every product in it fits
// gemm_x3q_kernel's contract, alignment of its buffers included (otherwise its activations stay fp32 and the products cut them).
void choose_pair_rows(EncRun& x) {
  const svt_encoder_config& c = x.c;
  const EncPlan& p = x.p;
  const EncWs& w = x.w;
  const svt_encoder* e = x.e;
  const int B = p.B, D = p.D, F = p.F, rows = (int)p.rows;
  const int pk_mode = (p.gp >= 2 && g_x3_pairs && g_gemm_x3) ? p.gp : 0;
  bool front = pk_mode != 0 && c.num_conv_layers >= 2 && c.conv_dim[0] % 32 == 0 && c.conv_dim[0] <= 512 && c.conv_stride[0] <= 5;
  for (int i = 1; i < c.num_conv_layers && front; ++i) {
    const int cin = c.conv_dim[i - 1], co = c.conv_dim[i], k = c.conv_kernel[i], st = c.conv_stride[i];
    const int64_t ti = p.frames[i - 1], to = p.frames[i];
    front = (int64_t)B * to <= 2147483647LL &&
            x3q_fits(w.act[0], (int)((int64_t)B * to), co, k * cin, (int)to, ti * cin, (long)st * cin, e->conv[i].w.p, 1, co) &&
            (c.feat_extract_norm != SVT_NORM_LAYER || co == 512 || co == 768 || co == 1024);
  }
  front = front && x3q_fits(w.xln, rows, D, p.C, rows, 0, p.C, e->proj_w.p, 0, D) &&
          (!c.feat_proj_layer_norm || p.C == 512 || p.C == 768 || p.C == 1024);
  x.pk_front = front ? pk_mode : 0;
  // encoder layers on pair rows: the layer input (LayerNorm output), the attention output and the FFN intermediate are written as
  // pair rows by their producers; the residual stream stays fp32 beside them (w.xF)
  const bool enc = pk_mode != 0 && p.attn.path == ATTN_FUSED_X3 && c.num_layers > 0 && (D == 512 || D == 768 || D == 1024) && p.dh % 32 == 0 &&
                   x3q_fits(w.xb, rows, 3 * D, D, rows, 0, D, e->layers[0].wqkv.p, 0, 3 * D) &&
                   x3q_fits(w.attn_o, rows, D, D, rows, 0, D, e->layers[0].wo.p, 0, D) &&
                   x3q_fits(w.xb, rows, F, D, rows, 0, D, e->layers[0].w1.p, 1, F) &&
                   x3q_fits(w.ffn, rows, D, F, rows, 0, F, e->layers[0].w2.p, 0, D);
  x.pk_enc = enc ? pk_mode : 0;
  // fp32 storage without pair rows: the layer input IS the residual stream (one buffer, w.xb), also where the carve gave a split
  // mode a w.xF of its own (that one then only serves as the stacked positional conv's scratch)
  x.resid = (!p.sp && !x.pk_enc) ? (float*)w.xb : w.xF;
}

// conv layer 0 with its norm (group or layer) and GELU, from the waveform into w.act[0] (channels-last)
int conv_layer0(const EncRun& x, const float* wav) {
  const svt_encoder_config& c = x.c;
  const EncWs& w = x.w;
  const int B = x.p.B, k = c.conv_kernel[0], st = c.conv_stride[0], C0 = c.conv_dim[0], prec = x.p.sp;
  const int64_t L = x.p.L, t1 = x.p.t1;
  const ConvLayerW& c0 = x.e->conv[0];
  const float* b0 = c.conv_bias ? c0.bias.as<float>() : nullptr;
  const bool mfma = conv0_mfma_ok(prec, x.pk_front, k, st, C0) && w.c0tab;
  if (c.feat_extract_norm == SVT_NORM_GROUP) {
    if (int r = launch_conv0_window_moments(wav, B, L, k, st, t1, x.win_mom, (char*)w.mom + w.mom_scr[2], x.s)) return r;
    if (int r = launch_conv0_group_coef(x.wav_mom, x.n_wav, x.win_mom, B, t1, C0, k, c0.w.as<float>(), b0, c0.gamma.as<float>(),
                                        c0.beta.as<float>(), 1e-5f, 1e-5f, w.coef, x.s, x.cpg)) return r;
    if (mfma) return launch_conv0_mfma_group(wav, B, L, st, t1, w.coef, w.c0tab, w.act[0], x.s, x.pk_front);
    return launch_conv0_group_apply(prec, wav, B, L, k, st, t1, C0, w.coef, w.act[0], x.s, x.pk_front);
  }
  if (mfma)
    return launch_conv0_mfma_layer(wav, B, L, st, t1, x.wav_mom, x.n_wav, 1e-5f, c0.w.as<float>(), b0, c0.gamma.as<float>(),
                                   c0.beta.as<float>(), 1e-5f, w.c0tab, w.act[0], x.s, x.cpg, x.pk_front);
  return launch_conv0_layer(prec, wav, B, L, k, st, t1, C0, x.wav_mom, x.n_wav, 1e-5f, c0.w.as<float>(), b0, c0.gamma.as<float>(),
                            c0.beta.as<float>(), 1e-5f, w.act[0], x.s, x.cpg, x.pk_front);
}

// conv layers 1..n-1 as implicit GEMMs between w.act[0] and w.act[1]; *cur = the buffer the last one wrote
int conv_stack(const EncRun& x, int* cur_out) {
  const svt_encoder_config& c = x.c;
  const EncWs& w = x.w;
  const int prec = x.p.sp, gp = x.p.gp, pk = x.pk_front;
  const bool layer_norm = c.feat_extract_norm == SVT_NORM_LAYER;
  int cur = 0;
  for (int i = 1; i < c.num_conv_layers; ++i) {
    const int cin = c.conv_dim[i - 1], co = c.conv_dim[i], k = c.conv_kernel[i], st = c.conv_stride[i];
    const int64_t tin = x.p.frames[i - 1], tout = x.p.frames[i], rows = (int64_t)x.p.B * tout;
    const ConvLayerW& Lw = x.e->conv[i];
    void* const out = w.act[cur ^ 1];
    if (rows > 2147483647LL) { set_error("encoder_forward: batch*frames exceeds 2^31"); return SVT_ERR_INVALID; }
    GemmArgs g;
    g.A = w.act[cur]; g.W = Lw.w.p;
    g.M = (int)rows; g.N = co; g.K = k * cin;
    g.a_rpb = (int)tout; g.a_bstride = tin * cin; g.a_rstride = (long)st * cin;
    g.ldw = g.K; g.ldc = co;
    if (Lw.w_kperm.p) { g.W_kperm = Lw.w_kperm.p; g.kperm_taps = k; g.kperm_cin = cin; }
    g.bias = c.conv_bias ? Lw.bias.as<float>() : nullptr;
    // pair rows: this layer reads them; it writes them too unless the feature projection's LayerNorm (an fp32 reader) comes next
    g.a_pairs = pk ? 1 : 0;
    const bool pairs_out = pk && !(i + 1 == c.num_conv_layers && c.feat_proj_layer_norm);
    LnArgs n = ln_f32(x, w.convF, rows, co, Lw.gamma, Lw.beta, 1e-5f);
    n.gelu = 1;
    if (pk && layer_norm) {
      g.C = w.convF; g.out_f32 = 1; g.act = ACT_NONE;
      if (int r = launch_gemm(gp, g, x.s)) return r;
      (pairs_out ? n.yP : n.yT) = out; n.pair_kind = pk;
      if (int r = launch_layernorm(n, x.s)) return r;
    } else if (pk) {
      g.C = out; g.act = ACT_GELU; g.out_f32 = 1; g.c_pairs = pairs_out ? 1 : 0;
      if (int r = launch_gemm(gp, g, x.s)) return r;
    } else if (layer_norm && prec && co == 512 && g_conv_ln_bf16) {
      // throughput mode: the conv output goes to HBM once, in the operand type, and is normalised in place (a wave owns a
      // row: it reads all of it before it writes) -- the fp32 round trip below moves 3x the bytes (conv1 at 64 x 10 s:
      // 2.1 GB written + 2.1 GB read + 1.05 GB written)
      g.C = out; g.out_f32 = 0; g.act = ACT_NONE;
      if (int r = launch_gemm(gp, g, x.s)) return r;
      n.x = out; n.x_is_f32 = 0; n.yT = out;
      if (int r = launch_layernorm(n, x.s)) return r;
    } else if (layer_norm) {
      g.C = w.convF; g.out_f32 = 1; g.act = ACT_NONE;
      if (int r = launch_gemm(gp, g, x.s)) return r;
      n.yT = out;
      if (int r = launch_layernorm(n, x.s)) return r;
    } else {
      g.C = out; g.act = ACT_GELU;
      if (int r = launch_gemm(gp, g, x.s)) return r;
    }
    cur ^= 1;
  }
  *cur_out = cur;
  return SVT_OK;
}

// optional LayerNorm over the conv channels, then the projection to the hidden size: w.act[cur] -> w.hF (fp32)
int feature_projection(const EncRun& x, int cur) {
  const svt_encoder_config& c = x.c;
  const EncWs& w = x.w;
  const int C = x.p.C, D = x.p.D, rows = (int)x.p.rows, pk = x.pk_front;
  const void* proj_in = w.act[cur];
  if (c.feat_proj_layer_norm) {
    LnArgs n = ln_f32(x, w.act[cur], rows, C, x.e->fp_g, x.e->fp_b, c.layer_norm_eps);
    n.x_is_f32 = x.p.sp ? 0 : 1;
    (pk ? n.yP : n.yT) = w.xln; n.pair_kind = pk;
    if (int r = launch_layernorm(n, x.s)) return r;
    proj_in = w.xln;
  }
  GemmArgs g;
  g.A = proj_in; g.W = x.e->proj_w.p; g.C = w.hF; g.bias = x.e->proj_b.as<float>();
  g.M = rows; g.N = D; g.K = C; g.a_rpb = rows; g.a_rstride = C; g.ldw = C; g.ldc = D; g.out_f32 = 1;
  g.a_pairs = pk ? 1 : 0;
  return launch_gemm(x.p.gp, g, x.s);
}

// SpecAugment (svt_encoder_set_spec_augment), in place on w.hF between the projection and the positional conv: one launch
int spec_augment(const EncRun& x) {
  const svt_encoder* e = x.e;
  return launch_spec_augment(x.w.hF, x.p.B, (int)x.p.T, x.p.D, x.p.D, e->sa_time, e->sa_feat, e->spec_embed.as<float>(), x.s) ? SVT_ERR_HIP : SVT_OK;
}

// the grouped conv over the gathered input w.posg as one batched product per (clip, group): kp*cg -> cg columns of C (fp32, row stride D)
GemmArgs posconv_gemm(const EncRun& x, const DevBuf& W, const DevBuf& bias) {
  const int T = (int)x.p.T, D = x.p.D, G = x.c.pos_conv_groups, cg = D / G, kp = x.c.pos_conv_kernel;
  GemmArgs g;
  g.A = x.w.posg; g.W = W.p; g.C = x.w.preF; g.bias = bias.as<float>();
  g.M = T; g.N = cg; g.K = kp * cg;
  g.a_rpb = T; g.a_rstride = cg;
  g.ldw = g.K; g.ldc = D;
  g.nz = x.p.B * G; g.nz2 = G;
  g.a_z1 = (long)G * (T + kp) * cg; g.a_z2 = (long)(T + kp) * cg;
  g.w_z1 = 0; g.w_z2 = (long)cg * g.K;
  g.c_z1 = (long)T * D; g.c_z2 = cg; g.bias_z2 = cg;
  g.out_f32 = 1;
  return g;
}

// positional conv embedding, w.hF -> w.preF: pre = h + gelu(grouped_conv(h) + b), in one of three forms.  Leaves svt_debug_set key 45 =
// 1000 * form (1 plain, 2 multi-frame, 3 stack) + 100 * gather kernel + 10 * scatter kernel (the launchers' own ids less 10 / 20; 0: none)
int positional_conv(const EncRun& x) {
  const svt_encoder_config& c = x.c;
  const svt_encoder* e = x.e;
  const EncWs& w = x.w;
  const int prec = x.p.sp, gp = x.p.gp, B = x.p.B, T = (int)x.p.T, D = x.p.D, kp = c.pos_conv_kernel, G = c.pos_conv_groups, cg = D / G;
  const float* bn_sc = c.pos_conv_batch_norm ? e->pos_bn_sc.as<float>() : nullptr;
  const float* bn_sh = c.pos_conv_batch_norm ? e->pos_bn_sh.as<float>() : nullptr;
  int gather_id = 0;
  if (c.pos_conv_depth > 1) {
    // data2vec-audio: pos = stack of [grouped conv -> LayerNorm(no affine, eps 1e-5) -> GELU]; pre = h + pos
    const float* cur = w.hF;
    float* lnout = w.xF;  // fp32 scratch (rows x D): free until the encoder's first LayerNorm
    for (int i = 0; i < c.pos_conv_depth; ++i) {
      if (int r = launch_posconv_gather(prec, cur, B, T, D, G, kp, T + kp, w.posg, x.s)) return r;
      gather_id = g_glue_kernel_id - 10;
      GemmArgs g = posconv_gemm(x, e->pos_ws[i], e->pos_bs[i]);
      g.act = ACT_NONE;
      if (int r = launch_gemm(gp, g, x.s)) return r;
      LnArgs n = ln_f32(x, w.preF, x.p.rows, D, e->ones, e->zeros, 1e-5f);
      n.gelu = 1; n.yF = lnout;
      if (int r = launch_layernorm(n, x.s)) return r;
      cur = lnout;
    }
    if (int r = launch_add_f32(w.hF, cur, w.preF, x.p.rows * (int64_t)D, x.s)) return r;
    g_glue_kernel_id = 3000 + 100 * gather_id;
    return SVT_OK;
  }
  if (x.p.pos_multi) {
    // multi-frame form (finalize_pos_conv): Pf output frames per GEMM row, 16-bit result scattered back onto h
    const int Pf = x.p.Pf, Tq = (int)x.p.pos_Tq, Tp = (int)x.p.pos_Tp;
    if (int r = launch_posconv_gather(prec, w.hF, B, T, D, G, kp, Tp, w.posg, x.s, bn_sc, bn_sh)) return r;
    gather_id = g_glue_kernel_id - 10;
    GemmArgs g;
    g.A = w.posg; g.W = e->pos_wP.p; g.C = w.posy; g.bias = e->pos_bP.as<float>();
    g.M = B * Tq; g.N = Pf * cg; g.K = (kp + Pf - 1) * cg;
    g.a_rpb = Tq; g.a_bstride = (long)G * Tp * cg; g.a_rstride = (long)Pf * cg;
    g.ldw = g.K; g.ldc = g.N;
    g.nz = G; g.nz2 = G;
    g.a_z2 = (long)Tp * cg; g.w_z2 = (long)g.N * g.K; g.c_z2 = (long)B * Tq * g.N; g.bias_z2 = g.N;
    g.act = ACT_GELU; g.out_f32 = 0;
    if (int r = launch_gemm(gp, g, x.s)) return r;
    if (int r = launch_posconv_scatter_add(w.hF, w.posy, B, T, D, G, Pf, Tq, w.preF, x.s, prec ? 0 : 1)) return r;
    g_glue_kernel_id = 2000 + 100 * gather_id + 10 * (g_glue_kernel_id - 20);
    return SVT_OK;
  }
  if (int r = launch_posconv_gather(prec, w.hF, B, T, D, G, kp, T + kp, w.posg, x.s, bn_sc, bn_sh)) return r;
  gather_id = g_glue_kernel_id - 10;
  GemmArgs g = posconv_gemm(x, e->pos_w, e->pos_b);
  g.resid = w.hF; g.act = ACT_GELU;
  if (int r = launch_gemm(gp, g, x.s)) return r;
  g_glue_kernel_id = 1000 + 100 * gather_id;
  return SVT_OK;
}

// ---- encoder layers.  Every family runs the same five products per layer; they differ in the type the products leave in and in the
// LayerNorm step between them.
struct LayerForm {
  int branch_f32 = 1;      // out-projection and FFN-2 leave in fp32 (1) or in the operand type (0) in w.hF, for the LayerNorm to add
  int ffn1_f32 = 0;        // FFN-1's out_f32 flag
  int ffn1_pairs = 0;      // FFN-1 writes pair rows
  bool ffn2_ksplit = false;  // FFN-2 as a K-split small GEMM: raw partial products in w.ksplit, summed by the LayerNorm behind it
};

// a product over all rows: (rows, K) x W^T + bias -> (rows, N)
// planes: the product additionally / instead leaves as 16-bit (hi, lo) planes for the fused split attention (QKV projection)
int rows_gemm(const EncRun& x, const void* A, int K, const DevBuf& W, const DevBuf& bias, int N, void* Cout, int out_f32, int act,
              unsigned short* planes = nullptr, int c_pairs = 0) {
  const int rows = (int)x.p.rows;
  GemmArgs g;
  g.A = A; g.W = W.p; g.C = Cout; g.bias = bias.as<float>();
  g.M = rows; g.N = N; g.K = K; g.a_rpb = rows; g.a_rstride = K; g.ldw = K; g.ldc = N;
  g.out_f32 = out_f32; g.act = act;
  g.planes = planes; g.plane_stride = (long)rows * N;
  g.a_pairs = x.pk_enc ? 1 : 0; g.c_pairs = c_pairs;
  return launch_gemm(x.p.gp, g, x.s);
}

// QKV projection -> attention -> out-projection: w.xb -> the attention branch in w.hF
int attention_block(const EncRun& x, const EncLayerW& Lw, const LayerForm& f, int l) {
  const EncPlan& p = x.p;
  const EncWs& w = x.w;
  const int D = p.D;
  // split-operand modes with the fused attention: the QKV projection's epilogue writes the planes the attention reads
  const bool x3 = p.attn.path == ATTN_FUSED_X3;
  if (int r = rows_gemm(x, w.xb, D, Lw.wqkv, Lw.bqkv, 3 * D, w.qkv, 0, ACT_NONE, x3 ? (unsigned short*)w.ab.pl_qkv : nullptr)) return r;
  const float* gate = nullptr;
  if (p.rel) {
    // WavLM: the gate of the relative position bias is a function of the attention INPUT (w.xb, operand type)
    if (int r = launch_relpos_gate(p.sp, w.xb, p.rows, (int)p.T, p.H, p.dh, Lw.g_wab.as<float>(), Lw.g_bab.as<float>(),
                                   Lw.g_const.as<float>(), w.gate, x.s)) return r;
    gate = w.gate;
  }
  DropSpec ad;   // site 2
  if (p.attn_drop) ad = make_drop_spec(x.drop->attention_dropout, x.drop->seed, x.drop->step, 2, l);
  AttnArgs a;
  a.prec = p.sp; a.gp = p.gp;
  a.Q = w.qkv; a.K = (const char*)w.qkv + (size_t)D * esize(p.sp); a.V = (const char*)w.qkv + (size_t)2 * D * esize(p.sp);
  a.ldq = a.ldkv = 3L * D;
  a.out = w.attn_o; a.ldo = D; a.o_pairs = x.pk_enc ? 1 : 0;
  a.B = p.B; a.T = (int)p.T; a.H = p.H; a.dh = p.dh; a.scale = 1.0f / std::sqrt((float)p.dh);
  a.gate = gate; a.relpb = w.relpb;
  a.drop = p.attn_drop ? &ad : nullptr; a.fused_drop = x.e->drop.fused_attention != 0;
  a.kv_ready = x3;   // the planes are there already
  if (int r = launch_attention(a, w.ab, x.s)) return r;
  // (rounds 1-2 fused this projection with the residual add and the LayerNorm in one row-complete kernel, 44 us against 29 + 23; with
  //  the projection on gemm_pps_kernel the pair costs 20.6 + 23.9 us and the fused kernel -- every workgroup streaming all of W,
  //  0.16 of the matrix pipe -- is gone: C2 6 093-6 110 against 6 066-6 074 clips/s on one box)
  if (int r = rows_gemm(x, w.attn_o, D, Lw.wo, Lw.bo, D, w.hF, f.branch_f32, ACT_NONE)) return r;
  if (!x.drop) return SVT_OK;
  return drop_rows(x, 3, l, x.drop->hidden_dropout, w.hF, f.branch_f32 ? 0 : (p.sp ? 1 : 0), p.rows * D);   // site 3: the branch, before the LayerNorm adds it
}

// FFN-1 (GELU) -> FFN-2: w.xb -> the feed-forward branch in w.hF (K-split form: in w.ksplit)
int ffn_block(const EncRun& x, const EncLayerW& Lw, const LayerForm& f, int l) {
  const EncWs& w = x.w;
  const int D = x.p.D, F = x.p.F, rows = (int)x.p.rows;
  if (int r = rows_gemm(x, w.xb, D, Lw.w1, Lw.b1, F, w.ffn, f.ffn1_f32, ACT_GELU, nullptr, f.ffn1_pairs)) return r;
  if (x.drop)   // site 4, behind GELU
    if (int r = drop_rows(x, 4, l, x.drop->activation_dropout, w.ffn, f.ffn1_f32 ? 0 : (x.p.sp ? 1 : 0), x.p.rows * F)) return r;
  if (!f.ffn2_ksplit) {
    if (int r = rows_gemm(x, w.ffn, F, Lw.w2, Lw.b2, D, w.hF, f.branch_f32, ACT_NONE)) return r;
    if (!x.drop) return SVT_OK;
    return drop_rows(x, 5, l, x.drop->hidden_dropout, w.hF, f.branch_f32 ? 0 : (x.p.sp ? 1 : 0), x.p.rows * D);   // site 5, behind FFN-2
  }
  // a few utterances: K = F split four ways over workgroups, raw fp32 partial tiles, summed (+ bias, rounded to the operand type
  // like the un-split product's stored result) by the LayerNorm that reads them
  GemmArgs g;
  g.A = w.ffn; g.W = Lw.w2.p; g.C = w.ksplit; g.M = rows; g.N = D; g.K = F; g.a_rpb = rows; g.a_rstride = F; g.ldw = F; g.ldc = D;
  g.out_f32 = 1; g.ksplit = 4; g.ksplit_stride = (long)rows * D;
  return launch_gemm_skinny(g, x.s);
}

// Post-LN: x = LN0(pre); per layer x = LN1(x + attention(x)), x = LN2(x + ffn(x)).  ln0() is the family's first LayerNorm,
// ln(Lw, second, last) the one behind a branch: the residual add lives in the LayerNorm kernel (LN(x + branch)), not in the GEMM
// epilogue, which is then store-only (fire-and-forget under the next tile's MFMAs in the persistent kernel).  The branch sits in w.hF,
// free after the positional conv.  The last LayerNorm also leaves the fp32 result in x.resid for the whole-batch output norm.
template <class Ln0, class Ln>
int post_ln_layers(const EncRun& x, const LayerForm& f, Ln0&& ln0, Ln&& ln) {
  if (int r = ln0()) return r;
  const int last = x.last_active();   // (the plain forward: num_layers - 1)
  for (int l = 0; l < x.c.num_layers; ++l) {
    if (x.skipped(l)) continue;       // layerdrop: a skipped layer launches nothing
    const EncLayerW& Lw = x.e->layers[l];
    if (int r = attention_block(x, Lw, f, l)) return r;
    if (int r = ln(Lw, false, false)) return r;
    if (int r = ffn_block(x, Lw, f, l)) return r;
    if (int r = ln(Lw, true, l == last)) return r;
  }
  return SVT_OK;
}

// FFN-2 as a K-split small GEMM: when the one-utterance kernel would serve it with less than one workgroup per CU (gemm_skinny.hip)
bool ffn2_ksplit_ok(const EncRun& x) {
  const int D = x.p.D, F = x.p.F, rows = (int)x.p.rows;
  if (!(g_ffn2_ksplit && x.w.ksplit && x.p.gp == 1 && F % 256 == 0 && F >= 2048 && g_ln_two_rows)) return false;
  GemmArgs g;
  g.A = x.w.ffn; g.W = x.e->layers[0].w2.p; g.C = x.w.hF; g.M = rows; g.N = D; g.K = F; g.a_rpb = rows; g.a_rstride = F; g.ldw = F; g.ldc = D;
  return g_gemm_skinny && gemm_skinny_eligible(g) && (long)((x.p.rows + 31) / 32) * (D / 32) <= 256;
}

// throughput mode: the residual stream lives as a bf16 (hi, lo) pair -- hi IS the operand copy the next GEMM
// reads -- so a LayerNorm moves 10 bytes per element instead of 12 (see layernorm.hip, layernorm_hilo_kernel)
int post_ln_hilo(const EncRun& x) {
  const EncWs& w = x.w;
  const int64_t rows = x.p.rows;
  const int D = x.p.D;
  const float eps = x.c.layer_norm_eps;
  bf16_t* const xh = (bf16_t*)w.xb;
  bf16_t* const xl = (bf16_t*)w.xlo;
  LayerForm f;
  // branch outputs (out-proj / FFN-2) are stored in the operand type (bf16: half the store burst of the GEMM epilogue and half the
  // read of the LayerNorm) and widened when added to the residual stream
  f.branch_f32 = 0;
  // (hidden_dropout > 0: the un-split FFN-2 -- the K-split form hands raw partials to the LayerNorm, and there is no tensor to drop)
  f.ffn2_ksplit = ffn2_ksplit_ok(x) && !(x.drop && x.drop->hidden_dropout > 0);
  return post_ln_layers(x, f,
    [&]() -> int {
      if (int r = launch_layernorm_hilo(nullptr, nullptr, nullptr, w.preF, rows, D, x.e->enc_g.as<float>(), x.e->enc_b.as<float>(), eps, xh, xl, nullptr, x.s)) return r;
      if (!x.drop || !(x.drop->hidden_dropout > 0)) return SVT_OK;
      // site 1 on the stream as this family stores it: the value hi + lo, cut again
      return launch_dropout_hilo(xh, xl, rows * D, 0, make_drop_spec(x.drop->hidden_dropout, x.drop->seed, x.drop->step, 1, 0), x.s) ? SVT_ERR_HIP : SVT_OK;
    },
    [&](const EncLayerW& Lw, bool second, bool last) {
      const float *g = (second ? Lw.ln2g : Lw.ln1g).as<float>(), *b = (second ? Lw.ln2b : Lw.ln1b).as<float>();
      float* const yF = last ? x.resid : nullptr;
      if (second && f.ffn2_ksplit)
        return launch_layernorm_hilo_parts(w.ksplit, 4, (long)rows * D, Lw.b2.as<float>(), xh, xl, rows, D, g, b, eps, xh, xl, yF, x.s);
      return launch_layernorm_hilo((const bf16_t*)w.hF, xh, xl, nullptr, rows, D, g, b, eps, xh, xl, yF, x.s);
    });
}

// split modes on pair rows.  fp16 pieces (kind 3): the layer input w.xb (pair rows) IS the residual stream -- LN(branch + (hi + lo))
// -> (hi', lo') in place, 12 bytes per element and pass instead of 16 with an fp32 copy beside it: hi + lo of two IEEE halves
// carries 22 of fp32's 24 mantissa bits.  bf16 pieces (kind 2) carry 16: there the residual stream stays fp32 (x.resid, updated in
// place) beside the pair rows the products read, as in round 3.  The products see exactly the same pieces either way; the last
// layer also leaves the fp32 result for the whole-batch output norm.
int post_ln_pairs(const EncRun& x) {
  const EncWs& w = x.w;
  const bool pair_resid = x.pk_enc == 3;
  LayerForm f;
  f.branch_f32 = 1; f.ffn1_f32 = 1; f.ffn1_pairs = 1;
  return post_ln_layers(x, f,
    [&] {
      LnArgs n = ln_f32(x, w.preF, x.p.rows, x.p.D, x.e->enc_g, x.e->enc_b, x.c.layer_norm_eps);
      // (every layer skipped: the first LayerNorm is also the last, and leaves the fp32 result.  Element dropouts are refused in the
      //  split modes -- svt_encoder_set_dropout -- so site 1 never reaches pair rows)
      n.yP = w.xb; n.pair_kind = x.pk_enc; n.yF = (pair_resid && x.last_active() >= 0) ? nullptr : x.resid;
      return launch_layernorm(n, x.s);
    },
    [&](const EncLayerW& Lw, bool second, bool last) {
      LnArgs n = ln_f32(x, w.hF, x.p.rows, x.p.D, second ? Lw.ln2g : Lw.ln1g, second ? Lw.ln2b : Lw.ln1b, x.c.layer_norm_eps);
      n.yP = w.xb; n.pair_kind = x.pk_enc;
      if (pair_resid) { n.addP = w.xb; n.yF = last ? x.resid : nullptr; }
      // every lane holds its part of the row in registers before anything is stored: add and yF may be the same buffer
      else { n.add = x.resid; n.yF = x.resid; }
      return launch_layernorm(n, x.s);
    });
}

// plain post-LN: operand copy in w.xb, fp32 residual stream in x.resid (fp32 storage: the same buffer, written once as yT)
int post_ln_plain(const EncRun& x, int branch_f32) {
  const EncWs& w = x.w;
  LayerForm f;
  f.branch_f32 = branch_f32;
  auto out = [&](LnArgs n) { n.yT = w.xb; n.yF = x.p.sp ? x.resid : nullptr; return launch_layernorm(n, x.s); };
  return post_ln_layers(x, f,
    [&]() -> int {
      if (int r = out(ln_f32(x, w.preF, x.p.rows, x.p.D, x.e->enc_g, x.e->enc_b, x.c.layer_norm_eps))) return r;
      if (!x.drop) return SVT_OK;
      // site 1: the operand copy and, where it is a buffer of its own, the fp32 residual stream beside it -- the same mask
      const int64_t n = x.p.rows * x.p.D;
      if (int r = drop_rows(x, 1, 0, x.drop->hidden_dropout, w.xb, x.p.sp ? 1 : 0, n)) return r;
      return (void*)x.resid != w.xb ? drop_rows(x, 1, 0, x.drop->hidden_dropout, x.resid, 0, n) : SVT_OK;
    },
    [&](const EncLayerW& Lw, bool second, bool) {
      LnArgs n = ln_f32(x, w.hF, x.p.rows, x.p.D, second ? Lw.ln2g : Lw.ln1g, second ? Lw.ln2b : Lw.ln1b, x.c.layer_norm_eps);
      n.x_is_f32 = branch_f32; n.add = x.resid;
      return out(n);
    });
}

// Pre-LN (stable_layer_norm): h = pre; per layer h += attention(LN1(h)), h += ffn(LN2(h)); result LN(h) in fp32 (*final_x).  Each
// branch is added by the LayerNorm that follows it: the fp32 residual stream h (w.preF) is updated in place (sumF) and the
// products' operand copy of LN(h) goes to w.xb.
int pre_ln_layers(const EncRun& x, int branch_f32, float** final_x) {
  const EncWs& w = x.w;
  float* const h = w.preF;
  LayerForm f;
  f.branch_f32 = branch_f32; f.ffn1_pairs = x.pk_enc ? 1 : 0;
  // y = LN(h + branch) with h += branch, to the operand copy y_op or (the last one) to fp32 y_f32
  auto ln_add = [&](const DevBuf& g_, const DevBuf& b_, const void* branch, void* y_op, float* y_f32) -> int {
    LnArgs n = ln_f32(x, h, x.p.rows, x.p.D, g_, b_, x.c.layer_norm_eps);
    n.sumF = (branch && y_op) ? h : nullptr;
    if (x.pk_enc && y_op) {   // pair rows for the products; h (fp32) += branch in place
      n.add = (const float*)branch; n.yP = y_op; n.pair_kind = x.pk_enc;
    } else if (!branch) {
      if (y_op) { n.yT = y_op; n.yF = y_f32; }
      else { n.prec = 0; n.yT = y_f32; }   // every layer skipped: the final LayerNorm of the untouched stream, in fp32
    } else if (!branch_f32) {  // x = bf16 branch, add = fp32 residual, sumF = residual updated in place
      n.x = branch; n.x_is_f32 = 0; n.add = h; n.yT = y_op; n.yF = y_f32;
    } else {
      n.add = (const float*)branch;
      if (y_op) n.yT = y_op; else { n.prec = 0; n.yT = y_f32; }
    }
    return launch_layernorm(n, x.s);
  };
  if (x.drop)   // site 1: in this family in front of the layers, on the fp32 stream
    if (int r = drop_rows(x, 1, 0, x.drop->hidden_dropout, h, 0, x.p.rows * x.p.D)) return r;
  const void* pending = nullptr;  // branch output not yet added to h
  for (int l = 0; l < x.c.num_layers; ++l) {
    if (x.skipped(l)) continue;   // layerdrop: a skipped layer launches nothing
    const EncLayerW& Lw = x.e->layers[l];
    if (int r = ln_add(Lw.ln1g, Lw.ln1b, pending, w.xb, nullptr)) return r;
    if (int r = attention_block(x, Lw, f, l)) return r;
    if (int r = ln_add(Lw.ln2g, Lw.ln2b, w.hF, w.xb, nullptr)) return r;
    if (int r = ffn_block(x, Lw, f, l)) return r;
    pending = w.hF;
  }
  // final LN(h + last FFN branch) -> fp32 (xF is unused in this family when prec == 0 it aliases xb: use qkv space)
  *final_x = (float*)w.qkv;
  return ln_add(x.e->enc_g, x.e->enc_b, pending, nullptr, *final_x);
}

// the transformer layers, w.preF -> *final_x (fp32, un-normalised encoder output)
int encoder_layers(const EncRun& x, float** final_x) {
  const EncPlan& p = x.p;
  if (p.rel)
    if (int r = launch_relpos_table(x.e->rel_embed.as<float>(), p.H, (int)p.T, x.c.rel_pos_buckets, x.c.rel_pos_max_distance, x.w.relpb, x.s)) return r;
  // branch outputs (out-proj / FFN-2) are stored in the operand type (bf16 in throughput mode: half the store burst of
  // the GEMM epilogue and 2 of the 14 bytes per element the LayerNorm moves) and widened when added to the fp32 residual stream
  const bool vecD = (p.D == 512 || p.D == 768 || p.D == 1024);
  const int branch_f32 = (p.sp && vecD) ? 0 : 1;
  if (x.c.stable_layer_norm) return pre_ln_layers(x, branch_f32, final_x);
  *final_x = x.resid;
  // (every layer skipped: no product reads the (hi, lo) pair, and its first LayerNorm -- layernorm_f32_to_hilo_kernel -- leaves no
  //  fp32 result; the plain form's does)
  if (p.hilo && x.last_active() >= 0) return post_ln_hilo(x);
  if (x.pk_enc) return post_ln_pairs(x);
  return post_ln_plain(x, branch_f32);
}

// the wrapper's whole-batch output LayerNorm (+ frame head + decode when a head was given)
int forward_tail(EncRun& x, float* final_x, const TailSpec& tail) {
  const svt_encoder_config& c = x.c;
  const EncWs& w = x.w;
  const int64_t rows = x.p.rows, n_out = rows * x.p.D;
  const double n_out_stat = x.global_norm ? (double)x.e->reduce_global_clips * (double)x.p.T * (double)x.p.D : 0.0;
  x.rctx.mom = x.out_mom;
  if (tail.head) {
    static_assert(sizeof(svt_frame) == sizeof(FrameOut), "frame layout");
    if (launch_head_fused(final_x, rows, x.p.D, tail.head->w.as<float>(), tail.head->wsum.as<float>(),
                          tail.head->has_bias ? tail.head->b.as<float>() : nullptr, tail.head->out_f, w.dots,
                          c.output_norm ? x.out_mom : nullptr, rows / x.groups, 1e-5f, tail.logits, (FrameOut*)tail.frames, tail.n_oct,
                          tail.n_cls, x.s, n_out_stat, x.global_norm && c.output_norm ? reduce_now : nullptr, &x.rctx,
                          (char*)w.mom + w.mom_scr[3])) return SVT_ERR_HIP;
    return SVT_OK;
  }
  if (c.output_norm) {
    if (int r = launch_moments(final_x, n_out / x.groups, x.out_mom, (char*)w.mom + w.mom_scr[1], x.p.B, x.s, x.groups)) return r;
    if (x.global_norm) { if (int r = reduce_now(&x.rctx)) return r; }
    return launch_global_norm(final_x, tail.feats, n_out / x.groups, x.out_mom, 1e-5f, x.s, x.groups, n_out_stat);
  }
  return launch_copy_f32(final_x, tail.feats, n_out, x.s) ? SVT_ERR_HIP : SVT_OK;
}

int encoder_forward_impl(svt_encoder* e, const float* wav, int32_t B, int64_t L, const TailSpec& tail, void* workspace,
                         size_t workspace_bytes, void* stream, int32_t clips_per_norm_group) {
  if (!e || !wav || !workspace) { set_error("encoder_forward: null argument"); return SVT_ERR_INVALID; }
  if (!e->finalized) { set_error("encoder_forward: parameters not finalized"); return SVT_ERR_STATE; }
  if (B < 1) { set_error("encoder_forward: batch < 1"); return SVT_ERR_INVALID; }
  EncPlan plan;
  if (!plan_encoder(e, B, L, &plan)) { set_error("encoder_forward: waveform shorter than the receptive field"); return SVT_ERR_INVALID; }
  EncRun x{e, e->cfg, plan, carve_encoder(e, plan, workspace), (hipStream_t)stream};
  x.drop = e->drop_on ? &e->drop : nullptr;
  const bool masks = e->sa_time || e->sa_feat;
  if (masks && (e->sa_B != B || e->sa_T != plan.T)) {
    set_error("encoder_forward: the SpecAugment masks were set for (" + std::to_string(e->sa_B) + ", " + std::to_string(e->sa_T) + ") clips x frames, this call has (" +
              std::to_string(B) + ", " + std::to_string(plan.T) + ")");
    return SVT_ERR_INVALID;
  }
  if (e->sa_time && !e->spec_embed.p) { set_error("encoder_forward: a time mask is set but masked_spec_embed was not loaded before finalize"); return SVT_ERR_STATE; }
  if (x.w.total > workspace_bytes) { set_error("encoder_forward: workspace too small (" + std::to_string(workspace_bytes) + " < " + std::to_string(x.w.total) + ")"); return SVT_ERR_WORKSPACE; }
  SVT_HIP(hipSetDevice(e->device));
  if (int r = check_norm_groups(x, clips_per_norm_group)) return r;
  if (int r = input_statistics(x, wav)) return r;
  choose_pair_rows(x);
  int cur = 0;
  if (e->cfg.num_conv_layers == 0) {   // features-in mode: `wav` is the (B, T, C) fp32 feature tensor
    const int64_t n = plan.rows * e->cfg.conv_dim[0];
    if (plan.sp) { if (int r = launch_f32_to_bf16(wav, (bf16_t*)x.w.act[0], n, x.s)) return r; }
    else if (launch_copy_f32(wav, (float*)x.w.act[0], n, x.s)) return SVT_ERR_HIP;
  } else {
    if (int r = conv_layer0(x, wav)) return r;
    if (int r = conv_stack(x, &cur)) return r;
  }
  if (int r = feature_projection(x, cur)) return r;
  if (x.drop)    // site 0, in front of SpecAugment as in HF's feature projection
    if (int r = drop_rows(x, 0, 0, x.drop->feat_proj_dropout, x.w.hF, 0, plan.rows * plan.D)) return r;
  if (masks)
    if (int r = spec_augment(x)) return r;
  if (int r = positional_conv(x)) return r;
  float* final_x = nullptr;
  if (int r = encoder_layers(x, &final_x)) return r;
  return forward_tail(x, final_x, tail);
}

}  // namespace

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

// One step of a finalized encoder on the caller's device buffers (include/svt_mi355.h documents the steps, buffers and refusals)
int svt_debug_encoder_step(svt_encoder* e, const svt_debug_encoder_desc* d, void* stream) {
  auto refuse = [](const char* why) { set_error(std::string("svt_debug_encoder_step: ") + why); return (int)SVT_ERR_INVALID; };
  auto aligned16 = [](auto... p) { return !((... | (uintptr_t)p) & 15); };   // a null pointer passes
  if (!d || d->struct_size != (int32_t)sizeof(svt_debug_encoder_desc)) return refuse("struct_size");
  if (!e) return refuse("null handle");
  if (!e->finalized) return refuse("call svt_encoder_finalize first");
  const int step = d->step;
  if (step < 1 || step > 3) return refuse("step is 1 .. 3");
  if (!aligned16(d->x, d->out, d->workspace)) return refuse("every buffer 16-byte aligned");
  if (!d->out || (step != 2 && !d->x) || (step == 1 && !d->workspace)) return refuse("null buffer");
  if (d->B < 1 || d->T < 1) return refuse("B and T must be positive");
  const svt_encoder_config& c = e->cfg;
  if (step != 1 && !c.rel_pos_buckets) return refuse("steps 2 and 3 need an encoder with rel_pos_buckets");
  if (step == 3 && (d->layer < 0 || d->layer >= c.num_layers)) return refuse("layer out of range");
  if ((int64_t)d->B * d->T > 2147483647LL / (c.hidden_size > 2 * c.num_heads ? c.hidden_size : 2 * c.num_heads))
    return refuse("too many frames for one call");
  hipStream_t s = (hipStream_t)stream;
  const int H = c.num_heads, D = c.hidden_size;
  int rc = SVT_OK;
  if (step == 1) {
    EncPlan plan;
    if (!plan_encoder(e, d->B, d->n_samples, &plan)) return refuse("n_samples is shorter than the receptive field");
    if (plan.T != d->T) return refuse("the plan of (B, n_samples) has another frame count than T");
    const EncWs w = carve_encoder(e, plan, d->workspace);
    if (w.total > d->workspace_bytes) return refuse("workspace smaller than svt_encoder_workspace_bytes");
    SVT_HIP(hipSetDevice(e->device));
    // the whole workspace 0xFF first: whatever the step reads without having written it is NaN
    if (hipMemsetAsync(d->workspace, 0xFF, w.total, s) != hipSuccess) { set_error("svt_debug_encoder_step: hipMemsetAsync"); rc = SVT_ERR_HIP; }
    const int64_t n = plan.rows * D;
    if (!rc && launch_copy_f32((const float*)d->x, w.hF, n, s)) rc = SVT_ERR_HIP;
    if (!rc) {
      const EncRun x{e, e->cfg, plan, w, s};
      rc = positional_conv(x);
    }
    if (!rc && launch_copy_f32(w.preF, (float*)d->out, n, s)) rc = SVT_ERR_HIP;
  } else {
    SVT_HIP(hipSetDevice(e->device));
    if (step == 2) {
      rc = launch_relpos_table(e->rel_embed.as<float>(), H, d->T, c.rel_pos_buckets, c.rel_pos_max_distance, (float*)d->out, s);
    } else {
      const EncLayerW& L = e->layers[d->layer];
      rc = launch_relpos_gate(storage_prec(c.precision), d->x, (int64_t)d->B * d->T, d->T, H, D / H, L.g_wab.as<float>(), L.g_bab.as<float>(),
                              L.g_const.as<float>(), (float*)d->out, s);
    }
  }
  if (rc && rc != SVT_ERR_HIP) rc = SVT_ERR_INVALID;   // a launcher's own refusal
  if (hipStreamSynchronize(s) != hipSuccess && !rc) { set_error("svt_debug_encoder_step: hipStreamSynchronize"); rc = SVT_ERR_HIP; }
  return rc;
}

}  // extern "C"
