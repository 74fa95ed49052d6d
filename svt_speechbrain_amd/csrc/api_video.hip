// C ABI of the AV-HuBERT lip front-end: ResNet-18 over the mouth ROI + projection.  The BatchNorm / conv folds
// and re-posed weight images of finalize, and the launch sequence of a forward.  Host code only.
#include "../../include/svt_mi355.h"
#include "api.h"
#include "common.h"
#include "host.h"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

using namespace svt;

int svt::g_conv_down_fused = 1;   // svt_debug_set key 27: 0 = stage 2's stride-2 conv1 and its 1x1 downsample as two products (A/B, tests)

struct VConv {
  DevBuf w, bias, slope;  // w: operand type [Cout][k*k*Cin] tap-major with the BN scale folded; bias / slope fp32
};
struct svt_video {
  int E = 0, prec = 0, gp = 0, device = 0;  // prec: storage type, gp: product engine
  bool finalized = false;
  bool uploaded = false;   // device buffers exist: the next finalize is a RE-upload into live buffers
  ParamMap params;
  DevBuf stem_w, stem_bias, stem_slope;
  VConv conv1[4][2], conv2[4][2], down[4];
  // stage 1 (64 channels) with G = 2 / 4 output pixels per GEMM row (bf16 mode): index [g][block], g = 0: G = 2, 1: G = 4
  VConv grp1[2][2], grp2[2][2];
  DevBuf gslope1[2][2], gslope2[2][2];
  DevBuf slope2[4][2];
  DevBuf frag1[2], frag2[2];  // stage 1, 16-bit storage: the 3x3 kernels as MFMA fragment images (conv3x3_c64.hip)
  VConv comb2;                // stage 2, block 0: conv1 (3x3 / 2) and the 1x1 / 2 downsample as ONE 256-column product (see svt_video_finalize)
  DevBuf frag128[3];          // stage 2's stride-1 convolutions: block 0 conv2, block 1 conv1 / conv2 (conv3x3_c128_kernel)
  DevBuf proj_w, proj_b;
  // svt_video_keep_workspace: the zero halos of the stage buffers are written by no kernel but zero_halo_kernel, so a caller who owns
  // the workspace (nobody writes it between two calls) needs them written ONCE per (workspace, geometry, stream)
  bool keep_ws = false;
  const void* halo_ws = nullptr;
  void* halo_stream = nullptr;
  int halo_geom[4] = {0, 0, 0, 0};
};

namespace {
struct VGeom {
  int H, W, Hp0, Wp0, H0, W0, Hs[4], Ws[4];
};
VGeom video_geom(int H, int W) {
  VGeom g;
  g.H = H; g.W = W;
  g.Hp0 = H + 6; g.Wp0 = round_up_int(W + 8, 8);
  g.H0 = (H - 1) / 2 + 1; g.W0 = (W - 1) / 2 + 1;
  int h = (g.H0 - 1) / 2 + 1, w = (g.W0 - 1) / 2 + 1;   // 3x3 / 2 max-pool, pad 1
  for (int i = 0; i < 4; ++i) {
    if (i > 0) { h = (h - 1) / 2 + 1; w = (w - 1) / 2 + 1; }  // 3x3 / 2 conv, pad 1
    g.Hs[i] = h; g.Ws[i] = w;
  }
  return g;
}
const int kVC[4] = {64, 128, 256, 512};

struct VWs {
  void *vp, *o0, *buf[4][3], *pooled;
};
size_t video_carve(const svt_video* v, int B, int T, const VGeom& g, void* base, VWs* out) {
  Carver c(base);
  const size_t es = esize(v->prec);
  const size_t F = (size_t)B * T;
  VWs w;
  w.vp = c.take((size_t)B * (T + 4) * g.Hp0 * g.Wp0 * es);
  w.o0 = c.take(F * g.H0 * g.W0 * 64 * es);
  for (int i = 0; i < 4; ++i)
    // stage 1: one tail pixel behind the last frame, zeroed with the halos -- the four-pixel grouped product's window reads it (video_group_width)
    for (int j = 0; j < 3; ++j) w.buf[i][j] = c.take((F * (g.Hs[i] + 2) * (g.Ws[i] + 2) + (i == 0 ? 1 : 0)) * kVC[i] * es);
  w.pooled = c.take(F * 512 * es);
  if (out) *out = w;
  return c.off;
}

// eval-mode BatchNorm -> per-channel scale / bias (eps 1e-5, torch.nn.BatchNorm2d/3d default)
int bn_fold(const ParamMap& P, const std::string& pre, int C, std::vector<float>* scale, std::vector<float>* bias) {
  const Param *g = nullptr, *b = nullptr, *m = nullptr, *var = nullptr;
  if (int r = need(P, pre + ".weight", {C}, &g)) return r;
  if (int r = need(P, pre + ".bias", {C}, &b)) return r;
  if (int r = need(P, pre + ".running_mean", {C}, &m)) return r;
  if (int r = need(P, pre + ".running_var", {C}, &var)) return r;
  batch_norm_fold(g->v.data(), b->v.data(), m->v.data(), var->v.data(), C, scale, bias);
  return SVT_OK;
}
// conv weight (Cout, Cin, k, k) -> [Cout][(ky*k + kx)*Cin + ci] with the BN scale folded
int fold_conv(int prec, const ParamMap& P, const std::string& wkey, const std::string& bnkey, int Cout, int Cin, int k, VConv* out) {
  const Param* w = nullptr;
  if (int r = need(P, wkey, {Cout, Cin, k, k}, &w)) return r;
  std::vector<float> sc, bi;
  if (int r = bn_fold(P, bnkey, Cout, &sc, &bi)) return r;
  std::vector<float> t((size_t)Cout * k * k * Cin);
  for (int co = 0; co < Cout; ++co)
    for (int ci = 0; ci < Cin; ++ci)
      for (int ky = 0; ky < k; ++ky)
        for (int kx = 0; kx < k; ++kx)
          t[(size_t)co * k * k * Cin + (size_t)(ky * k + kx) * Cin + ci] = w->v[(((size_t)co * Cin + ci) * k + ky) * k + kx] * sc[co];
  if (int r = upload_operand(prec, out->w, t.data(), t.size())) return r;
  return upload_f32(out->bias, bi.data(), bi.size());
}
// 3x3 stride-1 conv with 64 output channels re-posed for G (2 or 4) horizontally adjacent output pixels at once: the
// A row is the 3 x (G+2) pixel window they share (K = 3 (G+2) Cin), the weight matrix has G * Cout rows, row j*Cout + co
// holding the 3x3 kernel of pixel j shifted to taps kx' = j..j+2 (zeros elsewhere).  (G+2)/3 of the MACs, but the product
// is G*64 wide and runs on the LDS-DMA kernel, which is LDS / fill bound on narrow tiles: multiplying the structural
// zeros on a 256-wide tile is cheaper than a 64-wide tile without them (measured).
int fold_conv_group(const ParamMap& P, const std::string& wkey, const std::string& bnkey, int Cout, int Cin, int G, VConv* out) {
  const Param* w = nullptr;
  if (int r = need(P, wkey, {Cout, Cin, 3, 3}, &w)) return r;
  std::vector<float> sc, bi;
  if (int r = bn_fold(P, bnkey, Cout, &sc, &bi)) return r;
  const size_t K = (size_t)3 * (G + 2) * Cin;
  std::vector<float> t((size_t)G * Cout * K, 0.f), b2((size_t)G * Cout);
  for (int j = 0; j < G; ++j)
    for (int co = 0; co < Cout; ++co) {
      b2[(size_t)j * Cout + co] = bi[co];
      for (int ci = 0; ci < Cin; ++ci)
        for (int ky = 0; ky < 3; ++ky)
          for (int kx = 0; kx < 3; ++kx)
            t[((size_t)j * Cout + co) * K + (size_t)(ky * (G + 2) + kx + j) * Cin + ci] = w->v[(((size_t)co * Cin + ci) * 3 + ky) * 3 + kx] * sc[co];
    }
  if (int r = upload_operand(1, out->w, t.data(), t.size())) return r;
  return upload_f32(out->bias, b2.data(), b2.size());
}
// 64 -> 64 channel 3x3 kernel + BN scale as conv3x3_c64_kernel's LDS image: [tap ky*3+kx][k-step][channel block nb][lane] x 8 values,
// lane (i = lane & 15, kq = lane >> 4) = A-operand row i of block nb = output channel (nb>>1)*32 + (i>>2)*8 + (nb&1)*4 + (i&3), input
// channels ks*32 + kq*8 .. +7: a wave takes the two blocks of one channel half (nb>>1), a lane of its result then holds 8 consecutive
// channels and the four lanes of a pixel 32 consecutive ones (whole 64-byte segments per store instruction)
int fold_conv_frag64(const ParamMap& P, const std::string& wkey, const std::string& bnkey, DevBuf* out) {
  const Param* w = nullptr;
  if (int r = need(P, wkey, {64, 64, 3, 3}, &w)) return r;
  std::vector<float> sc, bi;
  if (int r = bn_fold(P, bnkey, 64, &sc, &bi)) return r;
  std::vector<float> t((size_t)9 * 2 * 4 * 64 * 8);
  for (int tap = 0; tap < 9; ++tap)
    for (int ks = 0; ks < 2; ++ks)
      for (int nb = 0; nb < 4; ++nb)
        for (int lane = 0; lane < 64; ++lane) {
          const int i = lane & 15, kq = lane >> 4, co = (nb >> 1) * 32 + (i >> 2) * 8 + (nb & 1) * 4 + (i & 3);
          for (int e = 0; e < 8; ++e) {
            const int ci = ks * 32 + kq * 8 + e;
            t[((((size_t)tap * 2 + ks) * 4 + nb) * 64 + lane) * 8 + e] = w->v[(((size_t)co * 64 + ci) * 3 + tap / 3) * 3 + tap % 3] * sc[co];
          }
        }
  return upload_operand(1, *out, t.data(), t.size());
}
// 128 -> 128 channel 3x3 kernel + BN scale as conv3x3_c128_kernel's register image: [wave = cq*2 + kh][tap][k-step][nb][lane] x 8
// values; lane (i = lane & 15, kq = lane >> 4) = A-operand row i of block nb = output channel cq*32 + (i>>2)*8 + nb*4 + (i&3) (a lane of
// the result holds 8 consecutive channels), input channels kh*64 + ks*32 + kq*8 .. +7
int fold_conv_frag128(const ParamMap& P, const std::string& wkey, const std::string& bnkey, DevBuf* out) {
  const Param* w = nullptr;
  if (int r = need(P, wkey, {128, 128, 3, 3}, &w)) return r;
  std::vector<float> sc, bi;
  if (int r = bn_fold(P, bnkey, 128, &sc, &bi)) return r;
  std::vector<float> t((size_t)8 * 36 * 64 * 8);
  for (int wv = 0; wv < 8; ++wv)
    for (int tap = 0; tap < 9; ++tap)
      for (int ks = 0; ks < 2; ++ks)
        for (int nb = 0; nb < 2; ++nb)
          for (int lane = 0; lane < 64; ++lane) {
            const int i = lane & 15, kq = lane >> 4, co = (wv >> 1) * 32 + (i >> 2) * 8 + nb * 4 + (i & 3);
            for (int e = 0; e < 8; ++e) {
              const int ci = (wv & 1) * 64 + ks * 32 + kq * 8 + e;
              t[(((size_t)wv * 36 + (tap * 2 + ks) * 2 + nb) * 64 + lane) * 8 + e] = w->v[(((size_t)co * 128 + ci) * 3 + tap / 3) * 3 + tap % 3] * sc[co];
            }
          }
  return upload_operand(1, *out, t.data(), t.size());
}
int upload_vec_rep(const ParamMap& P, const std::string& key, int C, int G, DevBuf* out) {
  const Param* p = nullptr;
  if (int r = need(P, key, {C}, &p)) return r;
  std::vector<float> t;
  for (int j = 0; j < G; ++j) t.insert(t.end(), p->v.begin(), p->v.end());
  return upload_f32(*out, t.data(), t.size());
}

// ---- the steps of a forward: video_forward_impl and svt_debug_video_step (one step on the caller's buffers) call the same functions ----
// what every step needs: the finalized handle, the frame count and the stream
struct VRun {
  const svt_video* v;
  long F;
  hipStream_t s;
};
// svt_debug_set key 43: codes of a block's convolutions (include/svt_mi355.h)
enum { VK_NONE = 0, VK_C64 = 1, VK_C128 = 2, VK_G2 = 3, VK_G4 = 4, VK_PLAIN = 5, VK_COMB = 6 };

// stem alone (the fused stem + pool does not apply): padded operand -> [F][H0][W0][64]
int video_stem(const VRun& r, const void* vp, int t, const VGeom& g, void* o0) {
  const svt_video* v = r.v;
  return launch_conv3d_front(v->prec, vp, v->stem_w.p, v->stem_bias.as<float>(), v->stem_slope.as<float>(), r.F, t, g.Hp0, g.Wp0, g.H0, g.W0, o0,
                             r.s) ? SVT_ERR_HIP : SVT_OK;
}
// stem + max-pool in one kernel -> interior of the zero-haloed stage-1 input
int video_stem_pool(const VRun& r, const void* vp, int t, const VGeom& g, void* out, int max_workgroups = 0) {
  const svt_video* v = r.v;
  return launch_conv3d_front_pool(vp, v->stem_w.p, v->stem_bias.as<float>(), v->stem_slope.as<float>(), r.F, t, g.Hp0, g.Wp0, g.H0, g.W0, g.Hs[0],
                                  g.Ws[0], out, r.s, max_workgroups) ? SVT_ERR_HIP : SVT_OK;
}
// 3x3 / 2 max-pool of the stem's output -> interior of the zero-haloed stage-1 input
int video_pool(const VRun& r, const void* o0, int H0, int W0, void* out) {
  return launch_maxpool_3x3s2(r.v->prec, o0, r.F, H0, W0, 64, (H0 - 1) / 2 + 1, (W0 - 1) / 2 + 1, out, r.s) ? SVT_ERR_HIP : SVT_OK;
}
// one k x k convolution (k = 3: pad 1; k = 1: no pad) over the zero-haloed channels-last tensor `in`
int video_conv(const VRun& r, const void* in, int Hin, int Win, int Cin, void* out, int Ho, int Wo, int Cout, int stride, int k, const VConv& cw,
               const float* slope, const void* resid, long second_out = 0) {
  const size_t es = esize(r.v->prec);
  const long F = r.F;
  GemmArgs a;
  const long Wpi = Win + 2, Hpi = Hin + 2, Wpo = Wo + 2, Hpo = Ho + 2;
  a.gen = 1;
  a.A = (const char*)in + (k == 1 ? (size_t)(Wpi + 1) * Cin * es : 0);
  a.W = cw.w.p; a.C = out; a.bias = cw.bias.as<float>();
  a.M = (int)(F * Ho * Wo); a.N = second_out ? 2 * Cout : Cout; a.K = k * k * Cin;
  a.c_nsplit = second_out ? Cout : 0; a.c_nstride = second_out;   // columns >= Cout: the tensor second_out elements behind `out`
  a.a_rstride = (long)stride * Cin;
  a.a_d1 = Wo; a.a_e1 = (long)stride * Wpi * Cin - (long)Wo * stride * Cin;
  a.a_d2 = Wo * Ho; a.a_e2 = Hpi * Wpi * Cin - (long)Ho * stride * Wpi * Cin;
  if (k == 3) { a.kseg = 3 * Cin; a.kseg_stride = Wpi * Cin; }
  a.ldw = (long)k * k * Cin; a.ldc = Cout;
  a.c_d1 = Wo; a.c_e1 = 2L * Cout;
  a.c_d2 = Wo * Ho; a.c_e2 = (Hpo * Wpo - (long)Ho * Wpo) * Cout;
  a.c_base = (Wpo + 1) * Cout;
  a.act = slope ? ACT_PRELU : ACT_NONE; a.slope = slope;
  a.resid = (const float*)resid; a.resid_first = 1; a.resid_op_type = 1;
  return launch_gemm(r.v->gp, a, r.s);
}
// stage 1 in the 16-bit modes: G output pixels per GEMM row (see fold_conv_group).  G = 4 computes one pixel past the end of a row of
// width 4 n + 3 (it lands on the right halo, re-zeroed afterwards, and its window reads one pixel past the row's right halo: the next
// row's left halo, or, behind the last row of the last frame, the tail pixel video_carve keeps behind every stage-1 buffer); G = 2 needs
// an even width; otherwise (0) the plain 64-wide product is used.
int video_group_width(int prec, long F, int Hs, int Ws) {
  int grp = 0;
  if (prec) {
    if (Ws % 2 == 0) grp = 2;                        // measured on 22 x 22 x 64: G = 2 794 us, G = 4 871 us, plain 901 us per conv
    else if ((Ws + 3) / 4 * 4 - Ws <= 2) grp = 4;
    if (grp && F * Hs * ((Ws + grp - 1) / grp) < 128) grp = 0;
  }
  return grp;
}
int video_conv_group(const VRun& r, int grp, const void* in, int Hh, int Ww, void* out, const VConv& cw, const float* slope_rep, const void* resid) {
  GemmArgs a;
  const long F = r.F;
  const long Wp = Ww + 2, Hp = Hh + 2, Wq = (Ww + grp - 1) / grp;
  a.gen = 1;
  a.A = in; a.W = cw.w.p; a.C = out; a.bias = cw.bias.as<float>();
  a.M = (int)(F * Hh * Wq); a.N = grp * 64; a.K = 3 * (grp + 2) * 64;
  a.a_rstride = (long)grp * 64;
  a.a_d1 = (int)Wq; a.a_e1 = (Wp - Wq * grp) * 64;
  a.a_d2 = (int)(Wq * Hh); a.a_e2 = (Hp * Wp - (long)Hh * Wp) * 64;
  a.kseg = (grp + 2) * 64; a.kseg_stride = Wp * 64;
  a.ldw = a.K; a.ldc = (long)grp * 64;
  a.c_d1 = (int)Wq; a.c_e1 = (Wp - Wq * grp) * 64;
  a.c_d2 = (int)(Wq * Hh); a.c_e2 = (Hp * Wp - (long)Hh * Wp) * 64;
  a.c_base = (Wp + 1) * 64;
  a.act = ACT_PRELU; a.slope = slope_rep;
  a.resid = (const float*)resid; a.resid_first = 1; a.resid_op_type = 1;
  if (int rc = launch_gemm(r.v->gp, a, r.s)) return rc;
  if (Wq * grp != Ww) return launch_zero_halo(r.v->prec, out, F, (int)Hp, (int)Wp, 64, r.s);
  return 0;
}
// BasicBlock b of stage li over the zero-haloed block input x (Hin x Win interior; it is also the identity residual and survives).
// fr: the stage's buffers the block may write -- fr[0] receives conv1, and a block with a downsample (b == 0, li > 0) puts it into fr[1]
// and its output into fr[2], every other block its output into fr[1].  *xout = the buffer that holds the block's output.
int video_block(const VRun& r, int li, int b, int Hin, int Win, const void* x, void* const fr[3], void** xout, int max_workgroups = 0) {
  const svt_video* v = r.v;
  const int prec = v->prec;
  const size_t es = esize(prec);
  const long F = r.F;
  const int C = kVC[li], stride = (b == 0 && li > 0) ? 2 : 1, cin = stride == 2 ? kVC[li - 1] : C;
  const int Ho = stride == 2 ? (Hin - 1) / 2 + 1 : Hin, Wo = stride == 2 ? (Win - 1) / 2 + 1 : Win;
  void* t1 = fr[0];
  void* outb = fr[1];
  const void* res = x;
  int k1 = VK_PLAIN, kd = VK_NONE, k2 = VK_PLAIN;
  auto done = [&]() { g_vstep_kernel_id = 5000 + 100 * k1 + 10 * kd + k2; *xout = outb; return (int)SVT_OK; };
  if (li == 0 && v->gp == 1 && conv3x3_c64_ok(prec, Ho, Wo)) {
    // frame-resident direct convolution (conv3x3_c64.hip): every input pixel fetched once, weights resident in LDS
    if (launch_conv3x3_c64(x, v->frag1[b].p, v->conv1[0][b].bias.as<float>(), v->conv1[0][b].slope.as<float>(), nullptr, t1, F, Ho, Wo, r.s,
                           max_workgroups)) return SVT_ERR_HIP;
    if (launch_conv3x3_c64(t1, v->frag2[b].p, v->conv2[0][b].bias.as<float>(), v->slope2[0][b].as<float>(), x, outb, F, Ho, Wo, r.s,
                           max_workgroups)) return SVT_ERR_HIP;
    k1 = k2 = VK_C64;
    return done();
  }
  const int grp = li == 0 ? video_group_width(prec, F, Ho, Wo) : 0;
  if (grp) {
    const int gi = grp == 4 ? 1 : 0;
    if (int rc = video_conv_group(r, grp, x, Ho, Wo, t1, v->grp1[gi][b], v->gslope1[gi][b].as<float>(), nullptr)) return rc;
    if (int rc = video_conv_group(r, grp, t1, Ho, Wo, outb, v->grp2[gi][b], v->gslope2[gi][b].as<float>(), x)) return rc;
    k1 = k2 = grp == 4 ? VK_G4 : VK_G2;
    return done();
  }
  const bool direct128 = li == 1 && v->gp == 1 && conv3x3_c128_ok(prec, Ho, Wo);
  if (direct128 && stride == 1) {
    if (launch_conv3x3_c128(x, v->frag128[1].p, v->conv1[1][b].bias.as<float>(), v->conv1[1][b].slope.as<float>(), nullptr, t1, F, Ho, Wo, r.s,
                            max_workgroups)) return SVT_ERR_HIP;
    k1 = VK_C128;
  } else if (li == 1 && stride == 2 && v->gp == 1 && g_conv_down_fused && (const char*)fr[1] > (const char*)t1 &&
             ((const char*)fr[1] - (const char*)t1) % (16 * es) == 0) {
    // conv1 + downsample as one 256-column product (svt_video_finalize): t1 <- columns 0..127, fr[1] <- columns 128..255
    if (int rc = video_conv(r, x, Hin, Win, cin, t1, Ho, Wo, C, 2, 3, v->comb2, v->comb2.slope.as<float>(), nullptr,
                            (long)(((const char*)fr[1] - (const char*)t1) / es))) return rc;
    res = fr[1];
    outb = fr[2];
    k1 = kd = VK_COMB;
  } else {
    if (int rc = video_conv(r, x, Hin, Win, cin, t1, Ho, Wo, C, stride, 3, v->conv1[li][b], v->conv1[li][b].slope.as<float>(), nullptr)) return rc;
    if (stride == 2) {  // first block of stages 2-4: the residual is the 1x1 stride-2 conv + BN of the block input
      if (int rc = video_conv(r, x, Hin, Win, cin, fr[1], Ho, Wo, C, 2, 1, v->down[li], nullptr, nullptr)) return rc;
      res = fr[1];
      outb = fr[2];
      kd = VK_PLAIN;
    }
  }
  if (direct128) {
    if (launch_conv3x3_c128(t1, v->frag128[b == 0 ? 0 : 2].p, v->conv2[1][b].bias.as<float>(), v->slope2[1][b].as<float>(), res, outb, F, Ho, Wo,
                            r.s, max_workgroups)) return SVT_ERR_HIP;
    k2 = VK_C128;
  } else if (int rc = video_conv(r, t1, Ho, Wo, C, outb, Ho, Wo, C, 1, 3, v->conv2[li][b], v->slope2[li][b].as<float>(), res)) return rc;
  return done();
}
// mean over the last stage's interior -> [F][512], the projection's operand
int video_avgpool(const VRun& r, const void* x, int H, int W, void* pooled) {
  return launch_avgpool_interior(r.v->prec, x, r.F, H, W, 512, pooled, r.s) ? SVT_ERR_HIP : SVT_OK;
}
int video_project(const VRun& r, const void* pooled, float* out_dev, int64_t out_ld) {
  const svt_video* v = r.v;
  GemmArgs pj;
  pj.A = pooled; pj.W = v->proj_w.p; pj.C = out_dev; pj.bias = v->proj_b.as<float>();
  pj.M = (int)r.F; pj.N = v->E; pj.K = 512; pj.a_rpb = (int)r.F; pj.a_rstride = 512; pj.ldw = 512; pj.ldc = out_ld; pj.out_f32 = 1;
  return launch_gemm(v->gp, pj, r.s) ? SVT_ERR_HIP : SVT_OK;
}
}  // namespace

extern "C" {

int svt_video_create(int32_t embed_dim, int32_t precision, int device, svt_video** out) {
  if (!out || embed_dim < 8 || embed_dim % 8) { set_error("svt_video_create: embed_dim must be a positive multiple of 8"); return SVT_ERR_INVALID; }
  if (!valid_precision(precision)) { set_error("svt_video_create: precision"); return SVT_ERR_INVALID; }
  if (int r = check_device(device)) return r;
  svt_video* v = new svt_video();
  v->E = embed_dim; v->prec = storage_prec(precision); v->gp = precision; v->device = device;
  *out = v;
  return SVT_OK;
}
void svt_video_destroy(svt_video* v) {
  if (!v) return;
  (void)hipSetDevice(v->device);
  delete v;
}
int svt_video_load_param(svt_video* v, const char* key, const void* data_host, int dtype, const int64_t* shape, int ndim) {
  if (!v) { set_error("null video front-end"); return SVT_ERR_INVALID; }
  v->finalized = false;
  return load_param_into(v->params, key, data_host, dtype, shape, ndim);
}
int svt_video_finalize(svt_video* v) {
  if (!v) { set_error("null video front-end"); return SVT_ERR_INVALID; }
  SVT_HIP(hipSetDevice(v->device));
  if (int r = begin_upload(v->uploaded)) return r;
  const ParamMap& P = v->params;
  const Param* p = nullptr;
  // ---- stem: (64,1,5,7,7) + BatchNorm3d + PReLU(64) ----
  if (int r = need(P, "resnet.frontend3D.0.weight", {64, 1, 5, 7, 7}, &p)) return r;
  std::vector<float> sc, bi;
  if (int r = bn_fold(P, "resnet.frontend3D.1", 64, &sc, &bi)) return r;
  auto wat = [&](int c, int dt, int dy, int dx) { return p->v[(((size_t)c * 5 + dt) * 7 + dy) * 7 + dx] * sc[c]; };
  if (v->prec) {
    // MFMA A-operand fragments [10 k-steps][4 channel blocks][64 lanes][8]: lane (i = lane & 15, cq = lane >> 4) holds
    // channel (i>>2)*16 + nb*4 + (i&3), k chunk s = ks*4 + cq = (dt, dy) row, element e = x tap e-1 (e = 0: alignment pad)
    std::vector<float> t((size_t)10 * 4 * 64 * 8, 0.f);
    for (int ks = 0; ks < 10; ++ks)
      for (int nb = 0; nb < 4; ++nb)
        for (int lane = 0; lane < 64; ++lane) {
          const int i = lane & 15, cq = lane >> 4, c = (i >> 2) * 16 + nb * 4 + (i & 3), sidx = ks * 4 + cq;
          if (sidx >= 35) continue;
          for (int e = 1; e < 8; ++e) t[(((size_t)ks * 4 + nb) * 64 + lane) * 8 + e] = wat(c, sidx / 7, sidx % 7, e - 1);
        }
    if (int r = upload_operand(1, v->stem_w, t.data(), t.size())) return r;
  } else {
    std::vector<float> t((size_t)280 * 64, 0.f);  // [(dt*7+dy)*8 + j][c]
    for (int c = 0; c < 64; ++c)
      for (int dt = 0; dt < 5; ++dt)
        for (int dy = 0; dy < 7; ++dy)
          for (int j = 1; j < 8; ++j) t[(size_t)((dt * 7 + dy) * 8 + j) * 64 + c] = wat(c, dt, dy, j - 1);
    if (int r = upload_f32(v->stem_w, t.data(), t.size())) return r;
  }
  if (int r = upload_f32(v->stem_bias, bi.data(), bi.size())) return r;
  if (int r = upload_vec(P, "resnet.frontend3D.2.weight", 64, &v->stem_slope)) return r;
  // ---- trunk ----
  int cin = 64;
  for (int li = 0; li < 4; ++li) {
    const int C = kVC[li];
    for (int b = 0; b < 2; ++b) {
      const std::string pre = "resnet.trunk.layer" + std::to_string(li + 1) + "." + std::to_string(b);
      if (int r = fold_conv(v->prec, P, pre + ".conv1.weight", pre + ".bn1", C, b == 0 ? cin : C, 3, &v->conv1[li][b])) return r;
      if (int r = upload_vec(P, pre + ".relu1.weight", C, &v->conv1[li][b].slope)) return r;
      if (int r = fold_conv(v->prec, P, pre + ".conv2.weight", pre + ".bn2", C, C, 3, &v->conv2[li][b])) return r;
      if (int r = upload_vec(P, pre + ".relu2.weight", C, &v->slope2[li][b])) return r;
      if (b == 0 && li > 0)
        if (int r = fold_conv(v->prec, P, pre + ".downsample.0.weight", pre + ".downsample.1", C, cin, 1, &v->down[li])) return r;
      if (li == 1 && b == 0 && v->prec) {
        // The 1x1 stride-2 downsample reads exactly the centre tap of conv1's 3x3 stride-2 window: as 128 more output columns of the
        // same product (weights zero outside the centre tap's 64 input channels, slope 1 = no activation) it rides in the half of the
        // 256-column tile that conv1 alone leaves empty, and the separate 168 us launch disappears.  Columns >= 128 go to the next
        // stage buffer (GemmArgs::c_nsplit).
        const Param *w1 = nullptr, *wd = nullptr, *sl = nullptr;
        if (int r = need(P, pre + ".conv1.weight", {128, 64, 3, 3}, &w1)) return r;
        if (int r = need(P, pre + ".downsample.0.weight", {128, 64, 1, 1}, &wd)) return r;
        if (int r = need(P, pre + ".relu1.weight", {128}, &sl)) return r;
        std::vector<float> s1, b1, sd, bd;
        if (int r = bn_fold(P, pre + ".bn1", 128, &s1, &b1)) return r;
        if (int r = bn_fold(P, pre + ".downsample.1", 128, &sd, &bd)) return r;
        std::vector<float> t((size_t)256 * 576, 0.f), bb(256), ss(256);
        for (int co = 0; co < 128; ++co) {
          bb[co] = b1[co]; ss[co] = sl->v[co];
          bb[128 + co] = bd[co]; ss[128 + co] = 1.0f;
          for (int ci = 0; ci < 64; ++ci) {
            for (int ky = 0; ky < 3; ++ky)
              for (int kx = 0; kx < 3; ++kx)
                t[(size_t)co * 576 + (size_t)(ky * 3 + kx) * 64 + ci] = w1->v[(((size_t)co * 64 + ci) * 3 + ky) * 3 + kx] * s1[co];
            t[(size_t)(128 + co) * 576 + (size_t)4 * 64 + ci] = wd->v[(size_t)co * 64 + ci] * sd[co];
          }
        }
        if (int r = upload_operand(v->prec, v->comb2.w, t.data(), t.size())) return r;
        if (int r = upload_f32(v->comb2.bias, bb.data(), bb.size())) return r;
        if (int r = upload_f32(v->comb2.slope, ss.data(), ss.size())) return r;
      }
      if (li == 1 && v->prec) {
        if (b == 1)
          if (int r = fold_conv_frag128(P, pre + ".conv1.weight", pre + ".bn1", &v->frag128[1])) return r;
        if (int r = fold_conv_frag128(P, pre + ".conv2.weight", pre + ".bn2", &v->frag128[b == 0 ? 0 : 2])) return r;
      }
      if (li == 0 && v->prec) {
        if (int r = fold_conv_frag64(P, pre + ".conv1.weight", pre + ".bn1", &v->frag1[b])) return r;
        if (int r = fold_conv_frag64(P, pre + ".conv2.weight", pre + ".bn2", &v->frag2[b])) return r;
        for (int gi = 0; gi < 2; ++gi) {
          const int G = gi ? 4 : 2;
          if (int r = fold_conv_group(P, pre + ".conv1.weight", pre + ".bn1", 64, 64, G, &v->grp1[gi][b])) return r;
          if (int r = upload_vec_rep(P, pre + ".relu1.weight", 64, G, &v->gslope1[gi][b])) return r;
          if (int r = fold_conv_group(P, pre + ".conv2.weight", pre + ".bn2", 64, 64, G, &v->grp2[gi][b])) return r;
          if (int r = upload_vec_rep(P, pre + ".relu2.weight", 64, G, &v->gslope2[gi][b])) return r;
        }
      }
    }
    cin = C;
  }
  if (int r = need(P, "proj.weight", {v->E, 512}, &p)) return r;
  if (int r = upload_weight(v->gp, v->proj_w, p->v.data(), (size_t)v->E, (size_t)512)) return r;
  if (int r = upload_vec(P, "proj.bias", v->E, &v->proj_b)) return r;
  v->finalized = true;
  return SVT_OK;
}

int64_t svt_video_workspace_bytes(const svt_video* v, int32_t batch, int32_t t, int32_t h, int32_t w) {
  if (!v || batch < 1 || t < 1 || h < 8 || w < 8) return -1;
  return (int64_t)video_carve(v, batch, t, video_geom(h, w), nullptr, nullptr);
}

int svt_video_keep_workspace(svt_video* v, int keep) {
  if (!v) { set_error("svt_video_keep_workspace: null handle"); return SVT_ERR_INVALID; }
  v->keep_ws = keep != 0;
  v->halo_ws = nullptr;
  return SVT_OK;
}

// One body for the four entry points: `video_dev` fp32 (B,1,T,h,w) already normalised, or `roi_dev` uint8 (B,T,h_in,w_in) with the
// recipe's transform `tf` and crop offsets (dy, dx) fused into the padding pass -- with `clips` (a host array of `batch` entries, already
// validated) every clip's own offsets, flip and length instead of (dy, dx); only the padding launch differs; out rows with pitch out_ld,
// `zero_left` columns to the left of every row zeroed by a kernel of the library (zero_cols_kernel: no torch kernel, no memset node --
// capturable)
static int video_forward_impl(svt_video* v, const float* video_dev, const unsigned char* roi_dev, int h_in, int w_in, int dy, int dx,
                              const VideoTransform* tf, const VideoClip* clips, int32_t batch, int32_t t, int32_t h, int32_t w, float* out_dev,
                              int64_t out_ld, int32_t zero_left, void* workspace_dev, size_t workspace_bytes, void* stream) {
  if (!v || (!video_dev && !roi_dev) || !out_dev || !workspace_dev) { set_error("svt_video_forward: null argument"); return SVT_ERR_INVALID; }
  if (!v->finalized) { set_error("svt_video_forward: call svt_video_finalize first"); return SVT_ERR_STATE; }
  if (batch < 1 || t < 1 || h < 8 || w < 8) { set_error("svt_video_forward: bad geometry"); return SVT_ERR_INVALID; }
  if (out_ld < v->E || zero_left < 0 || (zero_left > 0 && out_ld < (int64_t)v->E + zero_left)) {
    set_error("svt_video_forward: out_ld must hold embed_dim (+ zero_left) columns"); return SVT_ERR_INVALID; }
  const VGeom g = video_geom(h, w);
  VWs ws;
  if (video_carve(v, batch, t, g, workspace_dev, &ws) > workspace_bytes) { set_error("svt_video_forward: workspace too small"); return SVT_ERR_WORKSPACE; }
  if ((long)batch * t * g.Hs[0] * g.Ws[0] > 2000000000L) { set_error("svt_video_forward: too many frames for one call"); return SVT_ERR_INVALID; }
  SVT_HIP(hipSetDevice(v->device));
  hipStream_t s = (hipStream_t)stream;
  const int prec = v->prec;
  const long F = (long)batch * t;
  if (roi_dev && clips) {
    if (launch_video_pad_u8_clips(prec, roi_dev, batch, t, h_in, w_in, h, w, g.Hp0, g.Wp0, *tf, clips, ws.vp, s)) return SVT_ERR_HIP;
  } else if (roi_dev) {
    if (launch_video_pad_u8(prec, roi_dev, batch, t, h_in, w_in, dy, dx, h, w, g.Hp0, g.Wp0, *tf, ws.vp, s)) return SVT_ERR_HIP;
  } else if (launch_video_pad(prec, video_dev, batch, t, h, w, g.Hp0, g.Wp0, ws.vp, s)) return SVT_ERR_HIP;
  if (zero_left > 0)
    if (launch_zero_cols(out_dev - zero_left, F, zero_left, out_ld, s)) return SVT_ERR_HIP;
  const VRun run{v, F, s};
  const bool fused_stem = v->gp == 1 && conv3d_front_pool_ok(prec, g.Hp0, g.Wp0, g.W0);
  if (!fused_stem)
    if (int r = video_stem(run, ws.vp, t, g, ws.o0)) return r;
  // zero halos: the padded stage buffers are written in their interior only (12 launches, 1.3 GB of stores per 16 x 500 frames of
  // 88 x 88: 0.25 ms) -- skipped when the caller keeps the workspace to this object and the halos of this geometry are still there
  const bool halos_there = v->keep_ws && v->halo_ws == workspace_dev && v->halo_stream == stream && v->halo_geom[0] == batch &&
                           v->halo_geom[1] == t && v->halo_geom[2] == h && v->halo_geom[3] == w;
  if (!halos_there) {
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 3; ++j)
        if (launch_zero_halo(prec, ws.buf[i][j], F, g.Hs[i] + 2, g.Ws[i] + 2, kVC[i], s, i == 0 ? 1 : 0)) return SVT_ERR_HIP;
    v->halo_ws = v->keep_ws ? workspace_dev : nullptr;
    v->halo_stream = stream;
    v->halo_geom[0] = batch; v->halo_geom[1] = t; v->halo_geom[2] = h; v->halo_geom[3] = w;
  }
  if (fused_stem) {
    if (int r = video_stem_pool(run, ws.vp, t, g, ws.buf[0][0])) return r;
  } else if (int r = video_pool(run, ws.o0, g.H0, g.W0, ws.buf[0][0])) return r;

  const void* x = ws.buf[0][0];
  for (int li = 0; li < 4; ++li)
    for (int b = 0; b < 2; ++b) {
      // the stage's three buffers minus the block input (which is also the identity residual and must survive)
      void* fr[3] = {nullptr, nullptr, nullptr}; int nf = 0;
      for (int j = 0; j < 3; ++j) if (ws.buf[li][j] != x) fr[nf++] = ws.buf[li][j];
      const int pl = (b == 0 && li > 0) ? li - 1 : li;   // the stage whose geometry the block input has
      void* xo = nullptr;
      if (int r = video_block(run, li, b, g.Hs[pl], g.Ws[pl], x, fr, &xo)) return r;
      x = xo;
    }
  if (int r = video_avgpool(run, x, g.Hs[3], g.Ws[3], ws.pooled)) return r;
  return video_project(run, ws.pooled, out_dev, out_ld);
}

int svt_video_forward(svt_video* v, const float* video_dev, int32_t batch, int32_t t, int32_t h, int32_t w, float* out_dev,
                      void* workspace_dev, size_t workspace_bytes, void* stream) {
  return video_forward_impl(v, video_dev, nullptr, 0, 0, 0, 0, nullptr, nullptr, batch, t, h, w, out_dev, v ? v->E : 0, 0, workspace_dev, workspace_bytes, stream);
}
int svt_video_forward_ex(svt_video* v, const float* video_dev, int32_t batch, int32_t t, int32_t h, int32_t w, float* out_dev, int64_t out_ld,
                         int32_t zero_left, void* workspace_dev, size_t workspace_bytes, void* stream) {
  return video_forward_impl(v, video_dev, nullptr, 0, 0, 0, 0, nullptr, nullptr, batch, t, h, w, out_dev, out_ld, zero_left, workspace_dev, workspace_bytes, stream);
}
int svt_video_forward_u8(svt_video* v, const uint8_t* roi_dev, int32_t batch, int32_t t, int32_t h_in, int32_t w_in,
                         const svt_video_transform* tf, float* out_dev, int64_t out_ld, int32_t zero_left, void* workspace_dev,
                         size_t workspace_bytes, void* stream) {
  if (!tf || !roi_dev) { set_error("svt_video_forward_u8: null argument"); return SVT_ERR_INVALID; }
  if (tf->crop_h < 8 || tf->crop_w < 8 || tf->crop_h > h_in || tf->crop_w > w_in) {
    set_error("svt_video_forward_u8: the crop must lie inside the ROI (CenterCrop of a smaller frame is not defined by the reference)"); return SVT_ERR_INVALID; }
  if (tf->div0 == 0.0 || tf->std == 0.0) { set_error("svt_video_forward_u8: zero divisor in the transform"); return SVT_ERR_INVALID; }
  // CenterCrop (N20EMv2/video_only/utils.py:79-83): delta = int(round(w - tw) / 2.) -- truncation of a non-negative half
  const int dx = (w_in - tf->crop_w) / 2, dy = (h_in - tf->crop_h) / 2;
  const VideoTransform vt{tf->sub0, tf->div0, tf->mean, tf->std};
  return video_forward_impl(v, nullptr, roi_dev, h_in, w_in, dy, dx, &vt, nullptr, batch, t, tf->crop_h, tf->crop_w, out_dev, out_ld, zero_left, workspace_dev,
                            workspace_bytes, stream);
}
int svt_video_forward_u8_clips(svt_video* v, const uint8_t* roi_dev, int32_t batch, int32_t t, int32_t h_in, int32_t w_in,
                               const svt_video_transform* tf, const svt_video_clip* clips_host, float* out_dev, int64_t out_ld,
                               int32_t zero_left, void* workspace_dev, size_t workspace_bytes, void* stream) {
  static_assert(sizeof(svt_video_clip) == sizeof(VideoClip), "svt_video_clip and svt::VideoClip are the same four int32");
  if (!tf || !roi_dev || !clips_host) { set_error("svt_video_forward_u8_clips: null argument"); return SVT_ERR_INVALID; }
  if (batch < 1 || t < 1) { set_error("svt_video_forward_u8_clips: bad geometry"); return SVT_ERR_INVALID; }
  if (tf->crop_h < 8 || tf->crop_w < 8 || tf->crop_h > h_in || tf->crop_w > w_in) {
    set_error("svt_video_forward_u8_clips: the crop must lie inside the ROI"); return SVT_ERR_INVALID; }
  if (tf->div0 == 0.0 || tf->std == 0.0) { set_error("svt_video_forward_u8_clips: zero divisor in the transform"); return SVT_ERR_INVALID; }
  // every clip before any launch: an offset outside the ROI would read outside the caller's buffer
  for (int32_t b = 0; b < batch; ++b) {
    const svt_video_clip& c = clips_host[b];
    const char* field = nullptr;
    int32_t val = 0, lo = 0, hi = 0;
    if (c.dy < 0 || c.dy > h_in - tf->crop_h) { field = "dy"; val = c.dy; hi = h_in - tf->crop_h; }
    else if (c.dx < 0 || c.dx > w_in - tf->crop_w) { field = "dx"; val = c.dx; hi = w_in - tf->crop_w; }
    else if (c.flip != 0 && c.flip != 1) { field = "flip"; val = c.flip; hi = 1; }
    else if (c.n_frames < 1 || c.n_frames > t) { field = "n_frames"; val = c.n_frames; lo = 1; hi = t; }
    if (field) {
      set_error("svt_video_forward_u8_clips: clip " + std::to_string(b) + ": " + field + " = " + std::to_string(val) + " is outside " +
                std::to_string(lo) + " .. " + std::to_string(hi));
      return SVT_ERR_INVALID;
    }
  }
  const VideoTransform vt{tf->sub0, tf->div0, tf->mean, tf->std};
  return video_forward_impl(v, nullptr, roi_dev, h_in, w_in, 0, 0, &vt, reinterpret_cast<const VideoClip*>(clips_host), batch, t, tf->crop_h,
                            tf->crop_w, out_dev, out_ld, zero_left, workspace_dev, workspace_bytes, stream);
}

// One step of a finalized front-end on the caller's device buffers (include/svt_mi355.h documents the steps, buffers and refusals)
int svt_debug_video_step(svt_video* v, const svt_debug_video_desc* d, void* stream) {
  auto refuse = [](const char* why) { set_error(std::string("svt_debug_video_step: ") + why); return (int)SVT_ERR_INVALID; };
  auto aligned = [](auto... p) { return !((... | (uintptr_t)p) & 15); };   // a null pointer passes
  if (!d || d->struct_size != (int32_t)sizeof(svt_debug_video_desc)) return refuse("struct_size");
  if (!v) return refuse("null handle");
  if (!v->finalized) return refuse("call svt_video_finalize first");
  const int step = d->step;
  if (step < 1 || step > 6) return refuse("step is 1 .. 6");
  if (d->workgroups < 0) return refuse("workgroups must not be negative");
  if (!aligned(d->x, d->t1, d->ds, d->out)) return refuse("every buffer 16-byte aligned");
  if (!d->out || (step != 4 && !d->x)) return refuse("null buffer");
  const int prec = v->prec;
  const size_t es = esize(prec);
  VGeom g{};
  long F = d->F;
  if (step == 1 || step == 3) {
    if (d->B < 1 || d->T < 1 || d->h < 8 || d->w < 8) return refuse("B, T >= 1 and h, w >= 8");
    g = video_geom(d->h, d->w);
    F = (long)d->B * d->T;
    if ((double)F * g.Hp0 * g.Wp0 > 2.0e9) return refuse("too many frames for one call");
    if (step == 1 && prec && (size_t)5 * g.Hp0 * g.Wp0 * 2 > 160 * 1024) return refuse("the stem's five planes do not fit the LDS");
    if (step == 3 && !(v->gp == 1 && conv3d_front_pool_ok(prec, g.Hp0, g.Wp0, g.W0)))
      return refuse("the forward does not run the fused stem + pool at this geometry (conv3d_front_pool_ok; svt_debug_set key 26)");
  } else {
    if (F < 1 || d->H < 1 || d->W < 1) return refuse("F, H and W must be positive");
    if ((double)F * (d->H + 2) * (d->W + 2) > 2.0e9) return refuse("too many frames for one call");
  }
  if (step == 4 && (d->H < 3 || d->W < 3 || (d->C != 64 && d->C != 128 && d->C != 256 && d->C != 512)))
    return refuse("zero-halo: Hp, Wp >= 3 and C one of 64, 128, 256, 512");
  if (step == 5) {
    if (d->li < 0 || d->li > 3 || d->b < 0 || d->b > 1) return refuse("li is 0 .. 3 and b is 0 or 1");
    if (!d->t1 || (d->li > 0 && d->b == 0 && !d->ds)) return refuse("null buffer");
  }
  SVT_HIP(hipSetDevice(v->device));
  hipStream_t s = (hipStream_t)stream;
  const VRun run{v, F, s};
  void* vp = nullptr;
  int rc = SVT_OK;
  if (step == 1 || step == 3) {
    // the padded operand is the hook's own: 0xFF bytes first, so padding that the pad kernel does not write is NaN to the stem
    const size_t bytes = (size_t)d->B * (d->T + 4) * g.Hp0 * g.Wp0 * es;
    rc = dev_alloc(&vp, bytes);
    if (!rc && hipMemsetAsync(vp, 0xFF, bytes, s) != hipSuccess) { set_error("svt_debug_video_step: hipMemsetAsync"); rc = SVT_ERR_HIP; }
    if (!rc && launch_video_pad(prec, (const float*)d->x, d->B, d->T, d->h, d->w, g.Hp0, g.Wp0, vp, s)) rc = SVT_ERR_HIP;
    if (!rc) rc = step == 1 ? video_stem(run, vp, d->T, g, d->out) : video_stem_pool(run, vp, d->T, g, d->out, d->workgroups);
  } else if (step == 2) {
    rc = video_pool(run, d->x, d->H, d->W, d->out);
  } else if (step == 4) {
    rc = launch_zero_halo(prec, d->out, F, d->H, d->W, d->C, s) ? SVT_ERR_HIP : SVT_OK;
  } else if (step == 5) {
    const bool has_ds = d->li > 0 && d->b == 0;
    void* const fr[3] = {d->t1, has_ds ? d->ds : d->out, has_ds ? d->out : nullptr};
    void* xo = nullptr;
    rc = video_block(run, d->li, d->b, d->H, d->W, d->x, fr, &xo, d->workgroups);
  } else {
    rc = video_avgpool(run, d->x, d->H, d->W, d->out);
  }
  if (rc && rc != SVT_ERR_HIP) rc = SVT_ERR_INVALID;   // a launcher's own refusal
  if (hipStreamSynchronize(s) != hipSuccess && !rc) { set_error("svt_debug_video_step: hipStreamSynchronize"); rc = SVT_ERR_HIP; }
  if (vp) dev_free(vp);
  return rc;
}

}  // extern "C"
