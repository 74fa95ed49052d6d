// Host-side pieces shared by the C-ABI translation units (api.hip and api_*.hip): device buffers, workspace carving, uploads,
// the attention launcher's arguments (attention.hip) and the argument checks every entry point family uses.  Included by the api*.hip files only.
#pragma once
#include "common.h"
#include "host.h"
#include "philox.h"

#include <cstddef>
#include <cstdint>

namespace svt {

// the helpers below stay out of the library's dynamic symbol table: the C ABI (include/svt_mi355.h) is its interface
#pragma GCC visibility push(hidden)

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  ~DevBuf() { release(); }
  void release() { if (p) { split_weights_forget(p); dev_free(p); p = nullptr; } }
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
  int alloc(size_t n) {
    if (p && bytes == n) return 0;   // a re-upload of the same tensor keeps its buffer (no free / allocate pair: see upload_operand)
    release();
    bytes = n;
    return dev_alloc(&p, n);
  }
  template <typename T> T* as() const { return (T*)p; }
};

// upload fp32 host data as fp32 or (prec) bf16 operand
int upload_f32(DevBuf& b, const float* h, size_t n);
int upload_operand(int prec, DevBuf& b, const float* h, size_t n);
// weight matrix (rows x K, K contiguous): storage copy as upload_operand + in the split-operand modes the packed (hi, lo)
// pieces the LDS-DMA split kernels read (split_weights.hip); `precision` is the svt_precision of the object
int upload_weight(int precision, DevBuf& b, const float* h, size_t rows, size_t K);
// parameter intake of the svt_*_finalize steps: the loaded tensor `key`, which must have exactly the shape (C) / (rows, K) (need():
// SVT_ERR_KEY when it is missing, SVT_ERR_INVALID when mis-shaped), uploaded as upload_f32 / upload_weight do
int upload_vec(const ParamMap& P, const std::string& key, int C, DevBuf* out);
int upload_mat(int precision, const ParamMap& P, const std::string& key, int rows, int K, DevBuf* out);
// first step of every svt_*_finalize: waits for the forwards still in flight before a RE-upload changes live buffers
int begin_upload(bool& uploaded);

static inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }
static inline int round_up_int(int x, int a) { return (x + a - 1) / a * a; }

struct Carver {
  char* base;
  size_t off = 0;
  explicit Carver(void* b) : base((char*)b) {}
  void* take(size_t bytes) {
    void* p = base ? base + off : nullptr;
    off += align_up(bytes);
    return p;
  }
};

struct AttnBufs {
  float* S;   // (B,H,T,Tp) fp32
  void* P;    // operand type
  void* Vt;   // (B,H,dh,Tp)
  // split-operand modes: 16-bit (hi, lo) planes of the packed (rows, 3D) q/k/v projection, and of a separate (rows, D)
  // query projection (RCA cross attention); null in the other modes
  void* pl_qkv = nullptr;
  void* pl_q = nullptr;
};
static inline size_t esize(int prec) { return prec ? 2 : 4; }
// svt_precision -> storage type of activations / weights in HBM (0 = fp32, 1 = bf16).  The split-operand modes
// (SVT_PREC_BF16X3 / SVT_PREC_FP16X3) keep the fp32 parity pipeline and change only the engine of the dense products:
// launch_gemm(gp = precision) cuts the fp32 operands into 16-bit pieces on their way into LDS (gemm.hip).
static inline int storage_prec(int precision) { return precision >= 2 ? 0 : precision; }

// One attention (attention.hip): out[b,t,h*dh+d] = softmax(scale q k^T [+ gated bias]) v; q rows at Q + (b*T+t)*ldq + h*dh, likewise
// K and V (ldkv).  plan_attention (host.h) chooses among the fused kernels and the materialised scores.
struct AttnArgs {
  int prec = 0, gp = -1;     // storage type; product engine (-1: prec)
  const void *Q = nullptr, *K = nullptr, *V = nullptr; long ldq = 0, ldkv = 0;
  void* out = nullptr; long ldo = 0; int o_pairs = 0;   // o_pairs: out written as pair rows (the fused split path only)
  int B = 0, T = 0, H = 0, dh = 0; float scale = 1.f;
  const float *gate = nullptr, *relpb = nullptr;        // WavLM: gate (B,H,T), bias table (H, 2T-1); both or neither
  // training-mode attention dropout (site 2): the mask on the probabilities, element ((b*H + h)*T + i)*T + j; null: the plain paths.
  // fused_drop (svt_dropout.fused_attention): a geometry the plain fused 16-bit kernels serve runs their masked form, the rest the scores
  const DropSpec* drop = nullptr; bool fused_drop = false;
  bool kv_ready = false;     // the K/V side (V^T, or the planes) was prepared by an earlier call on the same k, v
};
AttnGeom attn_geom(const AttnArgs& a);   // the ONE place that infers packed_kv / q_packed from addresses and strides
// refuses (set_error, nothing launched) when a buffer the plan needs is null in `ab`
int launch_attention(const AttnArgs& a, const AttnBufs& ab, hipStream_t s);
// the buffers `plan` names, in the order S, P, Vt, pl_qkv, pl_q; the rest null.  es: esize of the storage type
AttnBufs carve_attention(Carver& cv, const AttnPlan& plan, size_t B, size_t H, size_t T, size_t dh, size_t es);

// The backward of one fused attention (attention_bwd.hip): dQ, dK, dV from q, k, v, the saved o and dO, all in the build's 16-bit operand
// type, rows addressed as AttnArgs' (q at Q + (b*T+t)*ldq + h*dh, ...); each gradient has its own row stride, so the three can land in
// one packed (B*T, 3D) buffer.  drop: the forward's site-2 mask (null: the plain kernels), e0 its first element index.  ws: the
// workspace, attention_backward_workspace_bytes (L and delta, (B, H, T) fp32 each).
struct AttnBwdArgs {
  int prec = 0;
  const void *Q = nullptr, *K = nullptr, *V = nullptr, *O = nullptr, *dO = nullptr;
  void *dQ = nullptr, *dK = nullptr, *dV = nullptr;
  long ldq = 0, ldkv = 0, ldo = 0, lddo = 0, lddq = 0, lddkv = 0;
  int B = 0, T = 0, H = 0, dh = 0; float scale = 1.f;
  const float *gate = nullptr, *relpb = nullptr;   // a position bias is refused
  const DropSpec* drop = nullptr; uint64_t e0 = 0;
  void* ws = nullptr;
};
size_t attention_backward_workspace_bytes(int B, int H, int T);
// refuses (set_error, nothing launched): head size other than 64, a precision other than the 16-bit one, a position bias, strides that
// are no multiples of 8 elements, a pointer the 16-byte accesses find misaligned
int launch_attention_backward(const AttnBwdArgs& a, hipStream_t s);

// a gfx950 device of this index exists; it becomes the current device
int check_device(int device);
// workspace_bytes is in / out: with workspace == NULL the size the call needs is stored and nothing else happens
int ws_query(const char* who, void* ws, size_t* ws_bytes, size_t need, bool* query);

#pragma GCC visibility pop

}  // namespace svt

struct svt_linear {
  int in_f = 0, out_f = 0, has_bias = 0, device = 0;
  bool loaded = false;
  svt::DevBuf w, b;
  svt::DevBuf wsum;  // sum_k w[j][k] per output (fp64 on the host): the fused out-norm + head tail needs it
};
