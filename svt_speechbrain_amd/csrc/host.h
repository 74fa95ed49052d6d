// Host-only part of the library: routines that never touch the GPU -- the error string behind svt_last_error(), parameter intake by
// key (svt_*_load_param), configuration validation (svt_encoder_create), the weight re-layouts and folds of svt_*_finalize and the
// frames -> notes scan (svt_frames_to_notes), and the RIFF/WAVE header parser and writer (svt_wav_parse, svt_wav_header; `make san_wav`
// builds those two with tests/cabi/wav_san_driver.cpp).  Plain
// C++17 with no HIP header, so the same translation unit is compiled twice: by hipcc into libsvt_mi355*.so, and by g++ with
// -fsanitize=address,undefined into the CPU test binary of `make san` (tests/test_host_sanitizers.py drives it with the reference's
// frame2note fixture and hostile arguments).  Sanitizers run on the CPU build only.
#pragma once
#include "../../include/svt_mi355.h"

#include <cstdint>
#include <map>
#include <string>
#include <vector>

namespace svt {

void set_error(const std::string& msg);

struct Param {
  std::vector<float> v;
  std::vector<int64_t> shape;
  int64_t numel() const { int64_t n = 1; for (auto s : shape) n *= s; return n; }
};
typedef std::map<std::string, Param> ParamMap;

int load_param_into(ParamMap& m, const char* key, const void* data, int dtype, const int64_t* shape, int ndim);
const Param* find(const ParamMap& m, const std::string& k);
int need(const ParamMap& m, const std::string& k, std::vector<int64_t> shape, const Param** out);
int validate_cfg(const svt_encoder_config& c);

// ---- re-layouts and folds of the finalize step: pure index arithmetic on host floats (tests/test_host_sanitizers.py runs each) ----
// conv weight (Co, Ci, k) -> (Co, k*Ci) tap-major: the implicit-GEMM row of output frame t is then the contiguous channels-last slice
// x[t*s : t*s+k, :]
std::vector<float> tap_major(const float* w, int Co, int Ci, int k);
// a tap-major (Co, k*Ci) matrix with its K axis in TAP-MINOR slab order: slab g = tap g % k of channels [(g / k) * 64, + 64); Ci % 64 == 0
std::vector<float> tap_minor_slabs(const float* wt, int Co, int Ci, int k);
// weight-norm over dim 2 of v (.., kp), n elements: W[.., j] = g[j] v[.., j] / ||v[.., j]||_F, norms and quotient in fp64
std::vector<float> weight_norm_fold(const float* g, const float* v, size_t n, int kp);
// eval-mode BatchNorm (eps 1e-5, the torch.nn.BatchNorm*d default) -> y = scale x + shift per channel, folded in fp64
void batch_norm_fold(const float* weight, const float* bias, const float* mean, const float* var, int C, std::vector<float>* scale,
                     std::vector<float>* shift);
// WavLM gate: gate = a (b const - 1) + 2, a / b = sigmoid of the sums of rows 0-3 / 4-7 of gru_rel_pos_linear (w: 8 x dh, b: 8):
// the row sums, wab (2 x dh) and bab (2), added in fp32 in row order
void gate_rowsum_fold(const float* w, const float* b, int dh, std::vector<float>* wab, std::vector<float>* bab);
// multi-frame form of the grouped positional conv w (G*cg, cg, kp): Pf consecutive output frames per GEMM row.  wP is G x Pf*cg x
// (kp+Pf-1)*cg -- row j*cg+co of a group holds filter co shifted by j taps, zero elsewhere -- and bP (G x Pf*cg) repeats the bias
void posconv_multiframe(const float* w, const float* bias, int G, int cg, int kp, int Pf, std::vector<float>* wP, std::vector<float>* bP);

// ---- attention planner: which of the four attention paths a geometry takes and which workspace buffers that path needs.  A function of
// numbers and flags only (no pointer, no global): the workspace carves, the launcher (attention.hip launch_attention) and the debug hooks
// all read ONE AttnPlan, so a carve can never disagree with the launch behind it (`make san` runs its expectation table) ----
enum AttnPath {
  ATTN_FUSED16,        // fused 16-bit kernels (attention_bf16.hip), with WavLM's gated bias where the kernel has it
  ATTN_FUSED16_DROP,   // the same with the dropout mask of site 2 inside (attention_drop.hip)
  ATTN_FUSED_X3,       // split-operand fused kernel on 16-bit (hi, lo) planes (attention_x3.hip)
  ATTN_SCORES          // materialised scores: two batched products around bias add, softmax (with or without the mask) and V^T
};
struct AttnGeom {
  int prec = 0, gp = 0, dh = 0;   // storage type (0 fp32, 1 16-bit); product engine (svt_precision); head size
  int64_t T = 0;
  bool bias = false;              // gated relative position bias (WavLM)
  bool drop = false;              // a dropout mask on the probabilities ...
  bool fused_drop = false;        // ... and the caller opted into the masked fused kernel where it serves the geometry
  bool packed_kv = false;         // k | v are columns D.., 2D.. of ONE fp32 (rows, 3D) projection: the planes are cut from it whole
  bool q_packed = false;          // ... and q is its columns 0..
};
struct AttnPlan {
  AttnPath path = ATTN_SCORES;
  int Tp = 0;                  // padded key length the S / P / V^T buffers are carved with
  bool scores = false;         // needs S and P
  bool vt = false;             // needs V^T
  bool planes_qkv = false;     // needs the planes of the packed projection
  bool planes_q = false;       // needs planes for a query in a buffer of its own
};
AttnPlan plan_attention(const AttnGeom& g);
// The plan a WORKSPACE is carved from: `p` plus two buffers nothing reads, kept because dropping them changes svt_*_workspace_bytes
// (a follow-up): V^T on the fused paths, and (scores_with_planes: FusionRCA) S and P on the fused split path.
AttnPlan attn_workspace_plan(AttnPlan p, bool scores_with_planes);

#ifdef SVT_OPERAND_F16
// the IEEE-half build serves the exact fp32 mode and the 16-bit throughput mode; the split-operand engines live in the bf16 build
static inline bool valid_precision(int p) { return p == SVT_PREC_FP32 || p == SVT_PREC_BF16; }
#else
static inline bool valid_precision(int p) { return p >= SVT_PREC_FP32 && p <= SVT_PREC_FP16X3; }
#endif

}  // namespace svt
