// C-ABI (include/svt_mi355.h) and host-side orchestration of the forward path.
// Host code only: parameter intake by HF key, one-time re-layout / fold / cast, workspace carving
// and the launch sequence.  No allocation, no synchronisation inside a forward call.
#include "../../include/svt_mi355.h"
#include "common.h"
#include "host.h"

#include <atomic>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

namespace svt {

int hip_fail(hipError_t e, const char* what, const char* file, int line) {
  set_error(std::string("HIP error ") + hipGetErrorName(e) + " (" + hipGetErrorString(e) + ") at " + file + ":" +
          std::to_string(line) + " in " + what);
  return SVT_ERR_HIP;
}

// ---------------------------------------------------------------- profiling (dominant kernel)
struct ProfState {
  bool on = false;
  int every = 1;        // record every `every`-th launch (sampling keeps the event pairs out of most launches of a timed region)
  unsigned tick = 0;
  bool armed = false;   // prof_begin recorded a start event for the launch in flight
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
  size_t used = 0;
  std::vector<int> kind;
  double flops[3] = {0, 0, 0}, bytes[3] = {0, 0, 0};
  static constexpr size_t kMax = 16384;
};
static ProfState g_prof;
void prof_begin(hipStream_t s) {
  g_prof.armed = false;
  if (!g_prof.on || g_prof.used >= ProfState::kMax) return;
  if (g_prof.every > 1 && (g_prof.tick++ % (unsigned)g_prof.every) != 0) return;
  g_prof.armed = true;
  if (g_prof.used == g_prof.ev.size()) {
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { g_prof.on = false; return; }
    g_prof.ev.emplace_back(a, b);
  }
  (void)hipEventRecord(g_prof.ev[g_prof.used].first, s);
}
void prof_end(hipStream_t s, double flops, double bytes, int kind) {
  if (!g_prof.on || !g_prof.armed || g_prof.used >= g_prof.ev.size()) return;
  g_prof.armed = false;
  (void)hipEventRecord(g_prof.ev[g_prof.used].second, s);
  if (g_prof.kind.size() <= g_prof.used) g_prof.kind.resize(g_prof.used + 1);
  g_prof.kind[g_prof.used] = kind;
  g_prof.used++;
  g_prof.flops[kind] += flops;
  g_prof.bytes[kind] += bytes;
}

// ---------------------------------------------------------------- small helpers
// ---- device allocations of the library (weights, packed pieces, scratch of the debug hooks) ----
// g_guard_alloc (svt_debug_set key 13, diagnostics): 0 = hipMalloc.  1 / 2 = every allocation gets its own mapping between two
// unmapped granules of reserved address space, the buffer flush against the END (1) or the START (2) of the mapping, so that a
// kernel reading or writing past that edge takes a page fault instead of touching a neighbour (this pool has no GPU sanitizer).
// 3 = hipMalloc with every byte set to 0xFF.
int g_guard_alloc = 0;
namespace {
struct GuardRec { void* va; size_t va_bytes; void* map; size_t map_bytes; hipMemGenericAllocationHandle_t h; };
std::map<void*, GuardRec> g_guard_recs;
std::mutex g_guard_mu;
}  // namespace
// per (kernel, device): the largest dynamic-LDS size already granted (see common.h)
int ensure_dyn_lds(const void* kernel, int bytes) {
  static std::mutex mu;
  static std::map<std::pair<const void*, int>, int> granted;
  int dev = 0;
  SVT_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(mu);
  int& have = granted[{kernel, dev}];
  if (bytes > have) {
    SVT_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    have = bytes;
  }
  return 0;
}

int dev_alloc(void** out, size_t n) {
  if (n == 0) n = 16;
  if (!g_guard_alloc) { SVT_HIP(hipMalloc(out, n)); return 0; }
  if (g_guard_alloc == 3) {   // plain allocation, every byte 0xFF (NaN in fp32 / bf16 / fp16): finds reads of bytes nobody wrote
    SVT_HIP(hipMalloc(out, n));
    SVT_HIP(hipMemset(*out, 0xFF, n));
    return 0;
  }
  int dev = 0;
  SVT_HIP(hipGetDevice(&dev));
  hipMemAllocationProp prop = {};
  prop.type = hipMemAllocationTypePinned;
  prop.location.type = hipMemLocationTypeDevice;
  prop.location.id = dev;
  size_t gran = 0;
  SVT_HIP(hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityMinimum));
  const size_t n16 = (n + 15) / 16 * 16, mapped = (n16 + gran - 1) / gran * gran;
  GuardRec r{};
  r.va_bytes = mapped + 2 * gran;
  r.map_bytes = mapped;
  SVT_HIP(hipMemAddressReserve(&r.va, r.va_bytes, gran, nullptr, 0));
  r.map = (char*)r.va + gran;
  SVT_HIP(hipMemCreate(&r.h, mapped, &prop, 0));
  SVT_HIP(hipMemMap(r.map, mapped, 0, r.h, 0));
  hipMemAccessDesc acc = {};
  acc.location = prop.location;
  acc.flags = hipMemAccessFlagsProtReadWrite;
  SVT_HIP(hipMemSetAccess(r.map, mapped, &acc, 1));
  *out = g_guard_alloc == 2 ? r.map : (char*)r.map + (mapped - n16);
  std::lock_guard<std::mutex> lk(g_guard_mu);
  g_guard_recs[*out] = r;
  return 0;
}
static std::atomic<int> g_dev_frees{0};   // svt_debug_set key 31 (query): device frees of this process so far (tests: none on an upload path)
void dev_free(void* p) {
  if (!p) return;
  g_dev_frees.fetch_add(1, std::memory_order_relaxed);
  GuardRec r{};
  {
    std::lock_guard<std::mutex> lk(g_guard_mu);
    auto it = g_guard_recs.find(p);
    if (it == g_guard_recs.end()) { (void)hipFree(p); return; }
    r = it->second;
    g_guard_recs.erase(it);
  }
  (void)hipDeviceSynchronize();
  (void)hipMemUnmap(r.map, r.map_bytes);
  (void)hipMemRelease(r.h);
  // the reservation is deliberately NOT returned (hipMemAddressFree): on this stack a later reservation that lands on the same
  // addresses is read through stale translations (measured: garbage weights after a free / allocate pair); address space is not
  // a scarce resource for a diagnostic run
}

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
static int upload_f32(DevBuf& b, const float* h, size_t n) {
  if (int r = b.alloc(n * 4)) return r;
  SVT_HIP(hipMemcpy(b.p, h, n * 4, hipMemcpyHostToDevice));
  return 0;
}
// fp32 staging of the 16-bit uploads: ONE grow-only buffer per device, kept for the life of the process.  Round 4 used a temporary per
// tensor (~75 hipMalloc / hipFree pairs per encoder object).  With eight processes uploading to one GPU at the same time that corrupted
// the weights of 12 of 1 152 objects (tools/determinism_stress.py --encoders 24 --procs 8: an object whose logits are off by O(1) for
// its whole life; seen first as a rank of `bench.py --gpus 8 --verify` on a shared GPU disagreeing with the other seven); with the
// staging buffer kept: 0 of 1 152.  An address range handed back by hipFree and out again by the next hipMalloc is, on this stack under
// that load, not always the same memory for the kernel that runs next (the guard allocator above met the same thing with the
// virtual-memory API).  Rule for this file: no free / allocate pair on a path that launches kernels -- buffers are kept and reused.
static std::mutex g_stage_mu;
static std::map<int, std::pair<void*, size_t>> g_stage;
static int upload_operand(int prec, DevBuf& b, const float* h, size_t n) {
  if (!prec) return upload_f32(b, h, n);
  int dev = 0;
  SVT_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_stage_mu);   // (held over the synchronous conversion: uploads are not a concurrent path)
  auto& st = g_stage[dev];
  if (st.second < n * 4) {
    if (st.first) { SVT_HIP(hipDeviceSynchronize()); dev_free(st.first); st.first = nullptr; st.second = 0; }
    const size_t want = std::max(n * 4, (size_t)32 << 20);
    if (int r = dev_alloc(&st.first, want)) return r;
    st.second = want;
  }
  SVT_HIP(hipMemcpy(st.first, h, n * 4, hipMemcpyHostToDevice));
  if (int r = b.alloc(n * 2)) return r;
  if (int r = launch_f32_to_bf16((const float*)st.first, b.as<bf16_t>(), (int64_t)n, 0)) return r;
  SVT_HIP(hipDeviceSynchronize());
  return 0;
}

// weight matrix (rows x K, K contiguous): storage copy as upload_operand + in the split-operand modes the packed (hi, lo)
// pieces the LDS-DMA split kernel reads (gemm_dma.hip); `precision` is the svt_precision of the object
static int upload_weight(int precision, DevBuf& b, const float* h, size_t rows, size_t K) {
  if (int r = upload_operand(precision >= 2 ? 0 : precision, b, h, rows * K)) return r;
  if (precision >= 2) {
    if (int r = split_weights_register(b.p, (long)rows, (int)K, precision, 0)) return r;
    SVT_HIP(hipDeviceSynchronize());
  }
  return 0;
}

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

// ---------------------------------------------------------------- attention (materialised scores)
struct AttnBufs {
  float* S;   // (B,H,T,Tp) fp32
  void* P;    // operand type
  void* Vt;   // (B,H,dh,Tp)
  // split-operand modes: 16-bit (hi, lo) planes of the packed (rows, 3D) q/k/v projection, and of a separate (rows, D)
  // query projection (RCA cross attention); null in the other modes
  void* pl_qkv = nullptr;
  void* pl_q = nullptr;
};
static size_t esize(int prec) { return prec ? 2 : 4; }
// svt_precision -> storage type of activations / weights in HBM (0 = fp32, 1 = bf16).  The split-operand modes
// (SVT_PREC_BF16X3 / SVT_PREC_FP16X3) keep the fp32 parity pipeline and change only the engine of the dense products:
// launch_gemm(gp = precision) cuts the fp32 operands into 16-bit pieces on their way into LDS (gemm.hip).
static inline int storage_prec(int precision) { return precision >= 2 ? 0 : precision; }

// out[b,t,h*dh+d] = softmax(scale * q k^T) v ; q rows at Q + (b*T+t)*ldq + h*dh, likewise K (ldkv), V (ldkv)
// fused attention: bf16, head_dim 64 / 128; its relative-position-bias variant (WavLM) exists for head_dim 64 with the
// (2T-1)-entry table of a head in LDS -- other WavLM geometries take the score-matrix path
static bool use_flash(int prec, int dh, bool bias = false, int64_t T = 0) {
  if (!(prec == 1 && (dh == 64 || dh == 128))) return false;
  return !bias || (dh == 64 && 2 * T - 1 <= 8192);
}
static int attn_tp(int prec, int dh, int T, bool bias = false) {
  return use_flash(prec, dh, bias, T) ? round_up_int(T, 64) : round_up_int(T, 8);
}

static int attention_scores_path(int prec, const void* Q, long ldq, const void* K, const void* V, long ldkv, int B,
                                 int T, int H, int dh, float scale, const AttnBufs& ab, bool vt_ready, void* out,
                                 long ldo, hipStream_t s, const float* gate = nullptr, const float* relpb = nullptr,
                                 int gp = -1, int o_pairs = 0) {
  if (gp < 0) gp = prec;
  if (gp >= 2 && !gate && flash_attention_x3_ok(dh) && ab.pl_qkv && ldkv == 3L * H * dh &&
      (const float*)V == (const float*)K + (long)H * dh) {
    // split-operand fused attention: cut the fp32 projections into 16-bit planes once, then three MFMAs per product
    // (attention.hip flash_attn_x3_kernel) -- no (B, H, T, T) score tensor
    const long D = (long)H * dh, rows = (long)B * T;
    const float* kv0 = (const float*)K - D;                     // start of the packed (rows, 3D) projection
    const long pl3 = rows * 3 * D;
    unsigned short* p3 = (unsigned short*)ab.pl_qkv;
    if (!vt_ready)
      if (int r = launch_split_planes(gp, kv0, 3 * D, rows, (int)(3 * D), p3, 3 * D, pl3, s)) return r;
    const unsigned short* qp;
    long qld, qpl;
    if ((const float*)Q == kv0 && ldq == 3 * D) { qp = p3; qld = 3 * D; qpl = pl3; }
    else {
      if (!ab.pl_q) { set_error("attention: no workspace for the query planes"); return -1; }
      if (int r = launch_split_planes(gp, (const float*)Q, ldq, rows, (int)D, ab.pl_q, D, rows * D, s)) return r;
      qp = (const unsigned short*)ab.pl_q; qld = D; qpl = rows * D;
    }
    return launch_flash_attention_x3(gp, qp, qld, (long)T * qld, qpl, p3 + D, p3 + 2 * D, 3 * D, (long)T * 3 * D, pl3, (float*)out, ldo,
                                     (long)T * ldo, B, T, H, dh, scale, s, o_pairs);
  }
  if (o_pairs) { set_error("attention: pair-row output is served by the fused split attention only"); return -1; }
  if (use_flash(prec, dh, gate != nullptr, T)) {
    (void)vt_ready;
    return launch_flash_attention(Q, ldq, (long)T * ldq, K, V, ldkv, (long)T * ldkv, out, ldo, (long)T * ldo, B, T, H, dh,
                                  scale, s, gate, gate ? relpb : nullptr);
  }
  const int Tp = round_up_int(T, 8);
  GemmArgs g;
  g.A = Q; g.W = K; g.C = ab.S;
  g.M = T; g.N = T; g.K = dh;
  g.a_rpb = T; g.a_bstride = 0; g.a_rstride = ldq;
  g.ldw = ldkv; g.ldc = Tp;
  g.nz = B * H; g.nz2 = H;
  g.a_z1 = (long)T * ldq; g.a_z2 = dh;
  g.w_z1 = (long)T * ldkv; g.w_z2 = dh;
  g.c_z1 = (long)H * T * Tp; g.c_z2 = (long)T * Tp;
  g.alpha = scale; g.out_f32 = 1;
  if (int r = launch_gemm(gp, g, s)) return r;
  if (gate)
    if (int r = launch_scores_add_relbias(ab.S, (int64_t)B * H, H, T, Tp, gate, relpb, s)) return r;
  if (int r = launch_softmax_rows(prec, ab.S, (int64_t)B * H * T, T, Tp, ab.P, s)) return r;
  if (!vt_ready)
    if (int r = launch_transpose_v(prec, V, B, T, H, dh, ldkv, 0, Tp, ab.Vt, s)) return r;
  GemmArgs o;
  o.A = ab.P; o.W = ab.Vt; o.C = out;
  o.M = T; o.N = dh; o.K = Tp;
  o.a_rpb = T; o.a_rstride = Tp;
  o.ldw = Tp; o.ldc = ldo;
  o.nz = B * H; o.nz2 = H;
  o.a_z1 = (long)H * T * Tp; o.a_z2 = (long)T * Tp;
  o.w_z1 = (long)H * dh * Tp; o.w_z2 = (long)dh * Tp;
  o.c_z1 = (long)T * ldo; o.c_z2 = dh;
  return launch_gemm(gp, o, s);
}

}  // namespace svt

using namespace svt;

static int g_debug_keep_split = 0;  // svt_debug_set(12, 1): svt_debug_gemm keeps the split copy of its weight operand between calls
static int g_conv_ln_bf16 = 1;     // svt_debug_set(9, 0): fp32 conv output + LayerNorm (A/B)

// =================================================================================================
// encoder
// =================================================================================================
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

struct svt_linear {
  int in_f = 0, out_f = 0, has_bias = 0, device = 0;
  bool loaded = false;
  DevBuf w, b;
  DevBuf wsum;  // sum_k w[j][k] per output (fp64 on the host): the fused out-norm + head tail needs it
};

static int check_device(int device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { set_error("no HIP device visible: the MI355X path cannot run (there is no CPU fallback)"); return SVT_ERR_NO_DEVICE; }
  if (device < 0 || device >= n) { set_error("device index out of range"); return SVT_ERR_INVALID; }
  hipDeviceProp_t prop;
  SVT_HIP(hipGetDeviceProperties(&prop, device));
  if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos) {
    set_error(std::string("device arch is ") + prop.gcnArchName + ", this library is built for gfx950 only");
    return SVT_ERR_NO_DEVICE;
  }
  SVT_HIP(hipSetDevice(device));
  return SVT_OK;
}

extern "C" {

int svt_abi_version(void) { return SVT_ABI_VERSION; }
int svt_operand_type(void) {
#ifdef SVT_OPERAND_F16
  return 1;
#else
  return 0;
#endif
}
int svt_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  int ok = 0;
  for (int i = 0; i < n; ++i) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, i) == hipSuccess && std::string(prop.gcnArchName).find("gfx950") != std::string::npos) ++ok;
  }
  return ok;
}

int svt_debug_gemm(int32_t precision, const void* a, const void* w, void* c, const float* bias, const float* resid,
                   int32_t m, int32_t n, int32_t k, int32_t a_rpb, int64_t a_bstride, int64_t a_rstride, int64_t ldw,
                   int32_t act, int32_t out_f32, int device, void* stream) {
  if (!a || !w || !c) { set_error("svt_debug_gemm: null argument"); return SVT_ERR_INVALID; }
  SVT_HIP(hipSetDevice(device));
  GemmArgs g;
  g.A = a; g.W = w; g.C = c; g.bias = bias; g.resid = resid;
  g.M = m; g.N = n; g.K = k; g.a_rpb = a_rpb; g.a_bstride = a_bstride; g.a_rstride = a_rstride;
  g.ldw = ldw; g.ldc = n; g.act = act; g.out_f32 = out_f32;
  // split-operand modes: the product path cuts weight matrices into (hi, lo) pieces once, at finalize; the hook does it per
  // call (or once per weight pointer with svt_debug_set(12, 1): micro-benchmarks)
  static const void* s_kept = nullptr;
  const bool split = precision >= 2 && ldw == k && k % 32 == 0;
  if (split && !(g_debug_keep_split && s_kept == w)) {
    if (split_weights_register(w, n, k, precision, (hipStream_t)stream)) return SVT_ERR_HIP;
    s_kept = w;
  }
  const int rc = launch_gemm(precision, g, (hipStream_t)stream);
  if (split && !g_debug_keep_split) {
    SVT_HIP(hipStreamSynchronize((hipStream_t)stream));
    split_weights_forget(w);
    s_kept = nullptr;
  }
  return rc ? SVT_ERR_INVALID : SVT_OK;
}

int svt_debug_gemm_pairs(int32_t precision, const float* a, int64_t a_elems, const float* w, float* c, const float* bias, int32_t m,
                         int32_t n, int32_t k, int32_t a_rpb, int64_t a_bstride, int64_t a_rstride, int32_t act, int32_t out_kind,
                         int device, void* stream, int32_t time_iters, float* ms_out) {
  if (!a || !w || !c) { set_error("svt_debug_gemm_pairs: null argument"); return SVT_ERR_INVALID; }
  if ((precision != SVT_PREC_BF16X3 && precision != SVT_PREC_FP16X3) || !valid_precision(precision)) {
    set_error("svt_debug_gemm_pairs: split-operand precisions only (they live in libsvt_mi355.so, not in the IEEE-half build)"); return SVT_ERR_INVALID; }
  if (out_kind < 0 || out_kind > 2 || a_elems % 32 || ((int64_t)m * n) % 32) { set_error("svt_debug_gemm_pairs: out_kind / sizes"); return SVT_ERR_INVALID; }
  SVT_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  void *ap = nullptr, *cp = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  // one exit: the staging buffers, the events and (unless svt_debug_set key 13 keeps it) the registered split weight are released on
  // every path, including a failed HIP call in the middle
  static std::mutex s_mu;          // s_kept is shared by every caller of this hook
  static const void* s_kept = nullptr;
  std::lock_guard<std::mutex> lock(s_mu);
  bool registered = false;
  auto hip_ok = [](hipError_t e, const char* what) -> int {
    if (e == hipSuccess) return 0;
    set_error(std::string(what) + ": " + hipGetErrorString(e));
    return 1;
  };
  int rc = dev_alloc(&ap, (size_t)a_elems * 4);
  if (!rc && out_kind) rc = dev_alloc(&cp, (size_t)m * n * 4);
  if (!rc) rc = launch_f32_to_pairs(precision, a, ap, a_elems, s);
  if (!rc && !(g_debug_keep_split && s_kept == w)) {
    rc = split_weights_register(w, n, k, precision, s);
    if (!rc) { s_kept = w; registered = true; }
  } else if (!rc) {
    registered = true;
  }
  if (!rc) {
    GemmArgs g;
    g.A = ap; g.W = w; g.C = out_kind == 1 ? cp : (void*)c; g.bias = bias;
    g.M = m; g.N = n; g.K = k; g.a_rpb = a_rpb; g.a_bstride = a_bstride; g.a_rstride = a_rstride;
    g.ldw = k; g.ldc = n; g.act = act; g.out_f32 = 1; g.a_pairs = 1; g.c_pairs = out_kind == 1;
    if (out_kind == 2) { g.planes = (unsigned short*)cp; g.plane_stride = (long)m * n; }
    rc = launch_gemm(precision, g, s);
    if (!rc && time_iters > 0 && ms_out) {   // micro-benchmark: HIP events around `time_iters` more launches of the product alone
      rc = hip_ok(hipEventCreate(&e0), "hipEventCreate") || hip_ok(hipEventCreate(&e1), "hipEventCreate") ||
           hip_ok(hipEventRecord(e0, s), "hipEventRecord");
      for (int i = 0; i < time_iters && !rc; ++i) rc = launch_gemm(precision, g, s);
      float ms = 0.f;
      if (!rc) rc = hip_ok(hipEventRecord(e1, s), "hipEventRecord") || hip_ok(hipEventSynchronize(e1), "hipEventSynchronize") ||
                    hip_ok(hipEventElapsedTime(&ms, e0, e1), "hipEventElapsedTime");
      if (!rc) *ms_out = ms / (float)time_iters;
    }
  }
  if (!rc && out_kind == 1) rc = launch_pairs_to_f32(precision, cp, nullptr, c, (int64_t)m * n, s);
  if (!rc && out_kind == 2) rc = launch_pairs_to_f32(precision, cp, (const unsigned short*)cp + (size_t)m * n, c, (int64_t)m * n, s);
  (void)hipStreamSynchronize(s);
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (registered && !g_debug_keep_split) { split_weights_forget(w); s_kept = nullptr; }
  if (ap) dev_free(ap);
  if (cp) dev_free(cp);
  return rc ? SVT_ERR_INVALID : SVT_OK;
}

int svt_debug_attention(int32_t precision, const void* q, const void* k, const void* v, void* o, int32_t batch, int32_t t,
                        int32_t heads, int32_t head_dim, int64_t ldq, int64_t ldkv, int64_t ldo, float scale, int device,
                        void* stream) {
  if (!q || !k || !v || !o) { set_error("svt_debug_attention: null argument"); return SVT_ERR_INVALID; }
  if (!(precision >= 1 && precision <= 3) || !(head_dim == 64 || head_dim == 128)) {
    set_error("svt_debug_attention: only the fused kernels (bf16, or the split-operand modes on fp32 inputs; head_dim 64 / 128) are exposed"); return SVT_ERR_INVALID; }
  if (int r = check_device(device)) return r;
  SVT_HIP(hipSetDevice(device));
  if (precision >= 2) {
    // q / k / v: fp32 slices of ONE packed (batch * t, 3 * heads * head_dim) projection; o: fp32
    const long D = (long)heads * head_dim, rows = (long)batch * t;
    if ((const float*)k != (const float*)q + D || (const float*)v != (const float*)q + 2 * D || ldq != 3 * D || ldkv != 3 * D) {
      set_error("svt_debug_attention: the split-operand kernel is exposed for a packed q|k|v projection"); return SVT_ERR_INVALID; }
    void* planes = nullptr;
    if (int r = dev_alloc(&planes, (size_t)rows * 3 * D * 4)) return r;
    AttnBufs ab{};
    ab.pl_qkv = planes;
    const int rc = attention_scores_path(0, q, ldq, k, v, ldkv, batch, t, heads, head_dim, scale, ab, false, o, ldo, (hipStream_t)stream,
                                         nullptr, nullptr, precision);
    (void)hipStreamSynchronize((hipStream_t)stream);
    dev_free(planes);
    return rc ? SVT_ERR_INVALID : SVT_OK;
  }
  if (launch_flash_attention(q, ldq, (long)t * ldq, k, v, ldkv, (long)t * ldkv, o, ldo, (long)t * ldo, batch, t, heads,
                             head_dim, scale, (hipStream_t)stream)) return SVT_ERR_INVALID;
  return SVT_OK;
}

static int g_conv_down_fused = 1;   // svt_debug_set key 27: 0 = stage 2's stride-2 conv1 and its 1x1 downsample as two products (A/B, tests)
int svt_debug_set(int key, int value) {
  if (key == 0) g_gemm_dbg = value;
  else if (key == 1) g_gemm_force_bm = value;
  else if (key == 2) g_gemm_ring = value;
  else if (key == 3) g_gemm_variant = value;
  else if (key == 5) { /* retired: the fused out-projection + LayerNorm kernel */ }
  else if (key == 6) g_gemm_skinny = value;
  else if (key == 7) g_gemm_skinny_max_tiles = value;
  else if (key == 8) g_flash_wide = value;
  else if (key == 9) g_conv_ln_bf16 = value;
  else if (key == 10) { /* retired: the whole-head attention experiment */ }
  else if (key == 11) g_gemm_x3 = value;
  else if (key == 12) g_debug_keep_split = value;
  else if (key == 13) g_guard_alloc = value;
  else if (key == 15) g_stamp_ends = value;
  else if (key == 16) { /* retired: the eight-barrier schedule of gemm_pps_kernel (profiles/r03_gemm_pps_slots.txt) */ }
  else if (key == 18) { /* retired: tile stamps of the lockstep eight-wave attention kernel */ }
  else if (key == 19) g_x3_pairs = value;
  else if (key == 20) g_ln_two_rows = value;
  else if (key == 21) {
    // retired: the A/B arms of the head_dim-64 attention (lockstep, software-pipelined, LDS-padded forms); 0 and 3 both name the
    // staggered kernel that ships
    if (value != 0 && value != 3) { set_error("svt_debug_set(21): the attention A/B arms are retired"); return SVT_ERR_INVALID; }
  }
  else if (key == 22) g_conv0_mfma = value;
  else if (key == 23) g_conv3x3_c64 = value;
  else if (key == 24) return g_conv3x3_c64_launches;
  else if (key == 25) g_conv3x3_c64_form = value;
  else if (key == 26) g_stem_pool_fused = value;
  else if (key == 27) g_conv_down_fused = value;
  else if (key == 28) {   // retired: the two-slot schedule of gemm_pps_kernel (profiles/r05_gemm_two_slot_ab.txt)
    if (value != 0) { set_error("svt_debug_set(28): the two-slot schedule is retired"); return SVT_ERR_INVALID; }
  }
  else if (key == 29) g_gemm_p1w = value;
  else if (key == 30) {
#ifndef SVT_DIAG
    // gemm_p1x_kernel is built by `make DIAG=1` only: the shipped library holds the kernels it dispatches
    if (value != 0) { set_error("svt_debug_set(30): gemm_p1x_kernel is built by `make DIAG=1` only"); return SVT_ERR_INVALID; }
#endif
    g_gemm_p1x = value;
  }
  else if (key == 31) return g_dev_frees.load(std::memory_order_relaxed);
  else if (key == 32) return set_ticket_fenced(value);
  else if (key == 33) g_gemm_skinny_small_tiles = value;
  else if (key == 34) g_gemm_walk = value;
  else if (key == 35) g_conv_kperm = value;
  else if (key == 36) g_ffn2_ksplit = value;
  else if (key == 37) { if (value < 8 || value > 256 || value % 8) { set_error("svt_debug_set(37): 8 .. 256, a multiple of 8"); return SVT_ERR_INVALID; } g_gemm_persist_wgs = value; }
  else { set_error("svt_debug_set: unknown key"); return SVT_ERR_INVALID; }
  return SVT_OK;
}

int svt_debug_alloc(void** out, size_t bytes, int device) {
  if (!out) { set_error("svt_debug_alloc: null argument"); return SVT_ERR_INVALID; }
  if (int r = check_device(device)) return r;
  SVT_HIP(hipSetDevice(device));
  return dev_alloc(out, bytes);
}
int svt_debug_free(void* p, int device) {
  if (int r = check_device(device)) return r;
  SVT_HIP(hipSetDevice(device));
  dev_free(p);
  return SVT_OK;
}

int svt_debug_clock(int64_t* out_dev, int device, void* stream) {
  if (!out_dev) { set_error("svt_debug_clock: null argument"); return SVT_ERR_INVALID; }
  SVT_HIP(hipSetDevice(device));
  return launch_clock_stamp((long long*)out_dev, (hipStream_t)stream) ? SVT_ERR_HIP : SVT_OK;
}

int svt_prof_enable(int on) { g_prof.on = on != 0; g_prof.every = on > 1 ? on : 1; g_prof.tick = 0; return SVT_OK; }
int svt_prof_reset(void) {
  g_prof.used = 0;
  for (int k = 0; k < 3; ++k) g_prof.flops[k] = g_prof.bytes[k] = 0;
  return SVT_OK;
}
int svt_prof_read(int kind, int64_t* launches, double* total_ms, double* total_flops, double* total_bytes) {
  if (kind < 0 || kind > 2) { set_error("svt_prof_read: kind must be 0..2"); return SVT_ERR_INVALID; }
  double ms = 0;
  int64_t n = 0;
  for (size_t i = 0; i < g_prof.used; ++i) {
    if (g_prof.kind[i] != kind) continue;
    SVT_HIP(hipEventSynchronize(g_prof.ev[i].second));
    float t = 0;
    SVT_HIP(hipEventElapsedTime(&t, g_prof.ev[i].first, g_prof.ev[i].second));
    ms += t;
    ++n;
  }
  if (launches) *launches = n;
  if (total_ms) *total_ms = ms;
  if (total_flops) *total_flops = g_prof.flops[kind];
  if (total_bytes) *total_bytes = g_prof.bytes[kind];
  return SVT_OK;
}

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
  // A RE-upload overwrites live weight buffers in place (DevBuf::alloc keeps a buffer of unchanged size; the uploads and conversions run
  // on the null stream, which does not order against the callers' non-blocking streams): wait for every forward still in flight on this
  // device -- replica() lanes share these buffers -- before the first byte changes (tests/test_gpu_uploads.py)
  if (e->uploaded) SVT_HIP(hipDeviceSynchronize());
  e->uploaded = true;
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
  // partials: kernels.hip, last_workgroup); the whole region is zeroed at the start of every forward (the tickets must be)
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

// Tail of a forward call: either the features (the wrapper's output) or, with a head, logits (+ decoded frames) straight
// from the un-normalised encoder output (fused out-norm + head + decode, kernels.hip head_dots_kernel).
struct TailSpec {
  float* feats = nullptr;
  const svt_linear* head = nullptr;
  float* logits = nullptr;
  svt_frame* frames = nullptr;
  int n_oct = 0, n_cls = 0;
};
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
  if (launch_zero_bytes(w.mom, w.mom_zero, s)) return SVT_ERR_HIP;   // (a kernel, not a memset node: see kernels.hip)
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
    // reads -- so a LayerNorm moves 10 bytes per element instead of 12 (see kernels.hip, layernorm_hilo_kernel)
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

// =================================================================================================
// frame head + decode
// =================================================================================================

extern "C" {

int svt_linear_create(int32_t in_features, int32_t out_features, int has_bias, int device, svt_linear** out) {
  if (!out || in_features < 1 || out_features < 1) { set_error("svt_linear_create: bad argument"); return SVT_ERR_INVALID; }
  if (int r = check_device(device)) return r;
  svt_linear* l = new svt_linear();
  l->in_f = in_features; l->out_f = out_features; l->has_bias = has_bias; l->device = device;
  *out = l;
  return SVT_OK;
}
void svt_linear_destroy(svt_linear* l) {
  if (!l) return;
  (void)hipSetDevice(l->device);
  delete l;
}
int svt_linear_load(svt_linear* l, const float* weight_host, const float* bias_host) {
  if (!l || !weight_host) { set_error("svt_linear_load: null argument"); return SVT_ERR_INVALID; }
  if (l->has_bias && !bias_host) { set_error("svt_linear_load: bias expected"); return SVT_ERR_INVALID; }
  SVT_HIP(hipSetDevice(l->device));
  if (int r = upload_f32(l->w, weight_host, (size_t)l->in_f * l->out_f)) return r;
  if (l->has_bias)
    if (int r = upload_f32(l->b, bias_host, (size_t)l->out_f)) return r;
  std::vector<float> ws((size_t)l->out_f);
  for (int j = 0; j < l->out_f; ++j) {
    double a = 0.0;
    for (int k = 0; k < l->in_f; ++k) a += (double)weight_host[(size_t)j * l->in_f + k];
    ws[j] = (float)a;
  }
  if (int r = upload_f32(l->wsum, ws.data(), ws.size())) return r;
  l->loaded = true;
  return SVT_OK;
}
int svt_linear_forward(svt_linear* l, const float* x, int64_t rows, float* y, void* stream) {
  if (!l || !x || !y) { set_error("svt_linear_forward: null argument"); return SVT_ERR_INVALID; }
  if (!l->loaded) { set_error("svt_linear_forward: weights not loaded"); return SVT_ERR_STATE; }
  if (rows < 1) return SVT_OK;
  hipStream_t s = (hipStream_t)stream;
  SVT_HIP(hipSetDevice(l->device));
  const float* b = l->has_bias ? l->b.as<float>() : nullptr;
  if (linear_head_eligible(l->in_f, l->out_f)) return launch_linear_head(x, rows, l->in_f, l->w.as<float>(), b, l->out_f, y, s);
  if (l->in_f % 4) {
    if (l->out_f <= 32) return launch_linear_f32(x, rows, l->in_f, l->w.as<float>(), b, l->out_f, y, s); set_error("svt_linear_forward: in_features must be a multiple of 4 for out_features > 32"); return SVT_ERR_INVALID; }
  if (rows > 2147483647LL) { set_error("svt_linear_forward: too many rows"); return SVT_ERR_INVALID; }
  GemmArgs g;
  g.A = x; g.W = l->w.p; g.C = y; g.bias = b;
  g.M = (int)rows; g.N = l->out_f; g.K = l->in_f; g.a_rpb = (int)rows; g.a_rstride = l->in_f; g.ldw = l->in_f;
  g.ldc = l->out_f; g.out_f32 = 1;
  return launch_gemm(0, g, s);
}

int svt_decode_frames(const float* logits, int64_t rows, int32_t n_out, int32_t n_octave, int32_t n_class,
                      svt_frame* frames, int device, void* stream) {
  if (!logits || !frames) { set_error("svt_decode_frames: null argument"); return SVT_ERR_INVALID; }
  if (n_out != 2 + n_octave + 1 + n_class + 1) { set_error("svt_decode_frames: n_out != 2 + (n_octave+1) + (n_class+1)"); return SVT_ERR_INVALID; }
  if (rows < 1) return SVT_OK;
  SVT_HIP(hipSetDevice(device));
  static_assert(sizeof(svt_frame) == sizeof(FrameOut), "frame layout");
  return launch_decode_frames(logits, rows, n_out, n_octave, n_class, (FrameOut*)frames, (hipStream_t)stream);
}

}  // extern "C"

// =================================================================================================
// RCA fusion
// =================================================================================================
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
  const int dh = r->D / r->H, Tp = attn_tp(r->prec, dh, T);
  const bool flash = use_flash(r->prec, dh);
  w.s1F = (float*)cv.take(rows * D * 4);
  w.s2F = (float*)cv.take(rows * D * 4);
  w.s1T = r->prec ? cv.take(rows * D * es) : (void*)w.s1F;
  w.s2T = r->prec ? cv.take(rows * D * es) : (void*)w.s2F;
  w.qkv = cv.take(rows * 3 * D * es);
  w.qc = cv.take(rows * D * es);
  w.ab.S = flash ? nullptr : (float*)cv.take((size_t)B * r->H * T * Tp * 4);
  w.ab.P = flash ? nullptr : cv.take((size_t)B * r->H * T * Tp * es);
  w.ab.Vt = cv.take((size_t)B * r->H * dh * Tp * es);
  if (r->gp >= 2 && flash_attention_x3_ok(dh)) {
    w.ab.pl_qkv = cv.take(rows * 3 * D * 4);
    w.ab.pl_q = cv.take(rows * D * 4);
  }
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
    if (int rc = attention_scores_path(prec, qkv, 3L * D, kp, vp, 3L * D, B, T, H, dh, scale, w.ab, false, att_s, D, s, nullptr, nullptr, r->gp)) return rc;
    if (int rc = attention_scores_path(prec, qc, D, kp, vp, 3L * D, B, T, H, dh, scale, w.ab, true, att_c, D, s, nullptr, nullptr, r->gp)) return rc;
    // out_proj is linear: alpha*Wo(a_s) + (1-alpha)*Wo(a_c) + bo = Wo(alpha*a_s + (1-alpha)*a_c) + bo
    if (int rc = launch_axpby(prec, att_s, att_c, r->alpha, 1.f - r->alpha, blend, rows * D, s)) return rc;
    if (int rc = gemm_rows(blend, D, L.wo.p, L.bo.as<float>(), D, pre1, 1, ACT_NONE, nullptr)) return rc;
    if (int rc = launch_layernorm(prec, pre1, 1, rows, D, L.n1g.as<float>(), L.n1b.as<float>(), 1e-6f, 0, xT,
                                  prec ? xF : nullptr, s, kvF)) return rc;
    if (int rc = gemm_rows(xT, D, L.w1.p, L.b1.as<float>(), F, ffn, 0, ACT_RELU, nullptr)) return rc;
    if (int rc = gemm_rows(ffn, F, L.w2.p, L.b2.as<float>(), D, pre2, 1, ACT_NONE, nullptr)) return rc;
    if (int rc = launch_layernorm(0, pre2, 1, rows, D, L.n2g.as<float>(), L.n2b.as<float>(), 1e-6f, 0, outF, nullptr, s, xF)) return rc;
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
  // A RE-upload overwrites live weight buffers in place (DevBuf::alloc keeps a buffer of unchanged size; the uploads and conversions run
  // on the null stream, which does not order against the callers' non-blocking streams): wait for every forward still in flight on this
  // device -- replica() lanes share these buffers -- before the first byte changes (tests/test_gpu_uploads.py)
  if (r->uploaded) SVT_HIP(hipDeviceSynchronize());
  r->uploaded = true;
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

// =================================================================================================
// CTC greedy, Fbank
// =================================================================================================
int svt_ctc_greedy(const float* probs, int32_t B, int32_t T, int32_t V, const float* rel_lens, int32_t blank,
                   int32_t* tokens, int32_t* out_lens, int device, void* stream) {
  if (!probs || !rel_lens || !tokens || !out_lens) { set_error("svt_ctc_greedy: null argument"); return SVT_ERR_INVALID; }
  if (B < 1 || T < 1 || V < 1) { set_error("svt_ctc_greedy: empty input"); return SVT_ERR_INVALID; }
  if (blank < 0) blank += V;
  SVT_HIP(hipSetDevice(device));
  return launch_ctc_greedy(probs, B, T, V, rel_lens, blank, tokens, out_lens, (hipStream_t)stream);
}

// =================================================================================================
// AV-HuBERT lip front-end: ResNet-18 over the mouth ROI + projection
// =================================================================================================
}  // extern "C"

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
    for (int j = 0; j < 3; ++j) w.buf[i][j] = c.take(F * (g.Hs[i] + 2) * (g.Ws[i] + 2) * kVC[i] * es);
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
  scale->resize(C); bias->resize(C);
  for (int c = 0; c < C; ++c) {
    const double sc = (double)g->v[c] / std::sqrt((double)var->v[c] + 1e-5);
    (*scale)[c] = (float)sc;
    (*bias)[c] = (float)((double)b->v[c] - (double)m->v[c] * sc);
  }
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
int upload_vec(const ParamMap& P, const std::string& key, int C, DevBuf* out) {
  const Param* p = nullptr;
  if (int r = need(P, key, {C}, &p)) return r;
  return upload_f32(*out, p->v.data(), p->v.size());
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
  // A RE-upload overwrites live weight buffers in place (DevBuf::alloc keeps a buffer of unchanged size; the uploads and conversions run
  // on the null stream, which does not order against the callers' non-blocking streams): wait for every forward still in flight on this
  // device -- replica() lanes share these buffers -- before the first byte changes (tests/test_gpu_uploads.py)
  if (v->uploaded) SVT_HIP(hipDeviceSynchronize());
  v->uploaded = true;
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

// One body for the three entry points: `video_dev` fp32 (B,1,T,h,w) already normalised, or `roi_dev` uint8 (B,T,h_in,w_in) with the
// recipe's transform `tf` and crop offsets (dy, dx) fused into the padding pass; out rows with pitch out_ld, `zero_left` columns to the
// left of every row zeroed by a kernel of the library (zero_cols_kernel: no torch kernel, no memset node -- capturable)
static int video_forward_impl(svt_video* v, const float* video_dev, const unsigned char* roi_dev, int h_in, int w_in, int dy, int dx,
                              const VideoTransform* tf, int32_t batch, int32_t t, int32_t h, int32_t w, float* out_dev, int64_t out_ld,
                              int32_t zero_left, void* workspace_dev, size_t workspace_bytes, void* stream) {
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
  const size_t es = esize(prec);
  const long F = (long)batch * t;
  if (roi_dev) {
    if (launch_video_pad_u8(prec, roi_dev, batch, t, h_in, w_in, dy, dx, h, w, g.Hp0, g.Wp0, *tf, ws.vp, s)) return SVT_ERR_HIP;
  } else if (launch_video_pad(prec, video_dev, batch, t, h, w, g.Hp0, g.Wp0, ws.vp, s)) return SVT_ERR_HIP;
  if (zero_left > 0)
    if (launch_zero_cols(out_dev - zero_left, F, zero_left, out_ld, s)) return SVT_ERR_HIP;
  const bool fused_stem = v->gp == 1 && conv3d_front_pool_ok(prec, g.Hp0, g.Wp0, g.W0);
  if (!fused_stem && launch_conv3d_front(prec, ws.vp, v->stem_w.p, v->stem_bias.as<float>(), v->stem_slope.as<float>(), F, t, g.Hp0, g.Wp0,
                                         g.H0, g.W0, ws.o0, s)) return SVT_ERR_HIP;
  // zero halos: the padded stage buffers are written in their interior only (12 launches, 1.3 GB of stores per 16 x 500 frames of
  // 88 x 88: 0.25 ms) -- skipped when the caller keeps the workspace to this object and the halos of this geometry are still there
  const bool halos_there = v->keep_ws && v->halo_ws == workspace_dev && v->halo_stream == stream && v->halo_geom[0] == batch &&
                           v->halo_geom[1] == t && v->halo_geom[2] == h && v->halo_geom[3] == w;
  if (!halos_there) {
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 3; ++j)
        if (launch_zero_halo(prec, ws.buf[i][j], F, g.Hs[i] + 2, g.Ws[i] + 2, kVC[i], s)) return SVT_ERR_HIP;
    v->halo_ws = v->keep_ws ? workspace_dev : nullptr;
    v->halo_stream = stream;
    v->halo_geom[0] = batch; v->halo_geom[1] = t; v->halo_geom[2] = h; v->halo_geom[3] = w;
  }
  if (fused_stem) {
    if (launch_conv3d_front_pool(ws.vp, v->stem_w.p, v->stem_bias.as<float>(), v->stem_slope.as<float>(), F, t, g.Hp0, g.Wp0, g.H0, g.W0,
                                 g.Hs[0], g.Ws[0], ws.buf[0][0], s)) return SVT_ERR_HIP;
  } else if (launch_maxpool_3x3s2(prec, ws.o0, F, g.H0, g.W0, 64, g.Hs[0], g.Ws[0], ws.buf[0][0], s)) return SVT_ERR_HIP;

  // one k x k convolution (k = 3: pad 1; k = 1: no pad) over the zero-haloed channels-last tensor `in`
  auto conv = [&](const void* in, int Hin, int Win, int Cin, void* out, int Ho, int Wo, int Cout, int stride, int k,
                  const VConv& cw, const float* slope, const void* resid, long second_out = 0) -> int {
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
    return launch_gemm(v->gp, a, s);
  };
  // stage 1 in bf16 mode: G output pixels per GEMM row (see fold_conv_group).  G = 4 may compute up to two pixels past the
  // end of a row (they land on the right halo and on the next row's left halo, re-zeroed afterwards); G = 2 needs an even
  // width; otherwise the plain 64-wide product is used.
  int grp = 0;
  if (prec) {
    const int Wd = g.Ws[0];
    if (Wd % 2 == 0) grp = 2;                        // measured on 22 x 22 x 64: G = 2 794 us, G = 4 871 us, plain 901 us per conv
    else if ((Wd + 3) / 4 * 4 - Wd <= 2) grp = 4;
    if (grp && F * g.Hs[0] * ((Wd + grp - 1) / grp) < 128) grp = 0;
  }
  auto conv_group = [&](const void* in, int Hh, int Ww, void* out, const VConv& cw, const float* slope_rep, const void* resid) -> int {
    GemmArgs a;
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
    if (int r = launch_gemm(v->gp, a, s)) return r;
    if (Wq * grp != Ww) return launch_zero_halo(prec, out, F, (int)Hp, (int)Wp, 64, s);
    return 0;
  };
  const void* x = ws.buf[0][0];
  int Hin = g.Hs[0], Win = g.Ws[0], cin = 64;
  for (int li = 0; li < 4; ++li) {
    const int C = kVC[li], Ho = g.Hs[li], Wo = g.Ws[li];
    for (int b = 0; b < 2; ++b) {
      const int stride = (b == 0 && li > 0) ? 2 : 1;
      // the stage's three buffers minus the block input (which is also the identity residual and must survive)
      void* fr[3]; int nf = 0;
      for (int j = 0; j < 3; ++j) if (ws.buf[li][j] != x) fr[nf++] = ws.buf[li][j];
      void* t1 = fr[0];
      void* outb = fr[1];
      const void* res = x;
      if (li == 0 && v->gp == 1 && conv3x3_c64_ok(prec, Ho, Wo)) {
        // frame-resident direct convolution (conv3x3_c64.hip): every input pixel fetched once, weights resident in LDS
        if (launch_conv3x3_c64(x, v->frag1[b].p, v->conv1[0][b].bias.as<float>(), v->conv1[0][b].slope.as<float>(), nullptr, t1, F, Ho, Wo, s))
          return SVT_ERR_HIP;
        if (launch_conv3x3_c64(t1, v->frag2[b].p, v->conv2[0][b].bias.as<float>(), v->slope2[0][b].as<float>(), x, outb, F, Ho, Wo, s))
          return SVT_ERR_HIP;
        x = outb;
        continue;
      }
      if (li == 0 && grp) {
        const int gi = grp == 4 ? 1 : 0;
        if (int r = conv_group(x, Ho, Wo, t1, v->grp1[gi][b], v->gslope1[gi][b].as<float>(), nullptr)) return r;
        if (int r = conv_group(t1, Ho, Wo, outb, v->grp2[gi][b], v->gslope2[gi][b].as<float>(), x)) return r;
        x = outb;
        continue;
      }
      const bool direct128 = li == 1 && v->gp == 1 && conv3x3_c128_ok(prec, Ho, Wo);
      if (direct128 && stride == 1) {
        if (launch_conv3x3_c128(x, v->frag128[1].p, v->conv1[1][b].bias.as<float>(), v->conv1[1][b].slope.as<float>(), nullptr, t1, F, Ho, Wo, s))
          return SVT_ERR_HIP;
      } else if (li == 1 && stride == 2 && v->gp == 1 && g_conv_down_fused && (const char*)fr[1] > (const char*)t1 &&
                 ((const char*)fr[1] - (const char*)t1) % (16 * es) == 0) {
        // conv1 + downsample as one 256-column product (svt_video_finalize): t1 <- columns 0..127, fr[1] <- columns 128..255
        if (int r = conv(x, Hin, Win, cin, t1, Ho, Wo, C, 2, 3, v->comb2, v->comb2.slope.as<float>(), nullptr,
                         (long)(((const char*)fr[1] - (const char*)t1) / es))) return r;
        res = fr[1];
        outb = fr[2];
      } else {
        if (int r = conv(x, Hin, Win, cin, t1, Ho, Wo, C, stride, 3, v->conv1[li][b], v->conv1[li][b].slope.as<float>(), nullptr)) return r;
        if (stride == 2) {  // first block of stages 2-4: the residual is the 1x1 stride-2 conv + BN of the block input
          if (int r = conv(x, Hin, Win, cin, fr[1], Ho, Wo, C, 2, 1, v->down[li], nullptr, nullptr)) return r;
          res = fr[1];
          outb = fr[2];
        }
      }
      if (direct128) {
        if (launch_conv3x3_c128(t1, v->frag128[b == 0 ? 0 : 2].p, v->conv2[1][b].bias.as<float>(), v->slope2[1][b].as<float>(), res, outb, F, Ho, Wo, s))
          return SVT_ERR_HIP;
      } else if (int r = conv(t1, Ho, Wo, C, outb, Ho, Wo, C, 1, 3, v->conv2[li][b], v->slope2[li][b].as<float>(), res)) return r;
      x = outb; Hin = Ho; Win = Wo; cin = C;
    }
  }
  if (launch_avgpool_interior(prec, x, F, g.Hs[3], g.Ws[3], 512, ws.pooled, s)) return SVT_ERR_HIP;
  GemmArgs pj;
  pj.A = ws.pooled; pj.W = v->proj_w.p; pj.C = out_dev; pj.bias = v->proj_b.as<float>();
  pj.M = (int)F; pj.N = v->E; pj.K = 512; pj.a_rpb = (int)F; pj.a_rstride = 512; pj.ldw = 512; pj.ldc = out_ld; pj.out_f32 = 1;
  if (launch_gemm(v->gp, pj, s)) return SVT_ERR_HIP;
  return SVT_OK;
}

int svt_video_forward(svt_video* v, const float* video_dev, int32_t batch, int32_t t, int32_t h, int32_t w, float* out_dev,
                      void* workspace_dev, size_t workspace_bytes, void* stream) {
  return video_forward_impl(v, video_dev, nullptr, 0, 0, 0, 0, nullptr, batch, t, h, w, out_dev, v ? v->E : 0, 0, workspace_dev, workspace_bytes, stream);
}
int svt_video_forward_ex(svt_video* v, const float* video_dev, int32_t batch, int32_t t, int32_t h, int32_t w, float* out_dev, int64_t out_ld,
                         int32_t zero_left, void* workspace_dev, size_t workspace_bytes, void* stream) {
  return video_forward_impl(v, video_dev, nullptr, 0, 0, 0, 0, nullptr, batch, t, h, w, out_dev, out_ld, zero_left, workspace_dev, workspace_bytes, stream);
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
  return video_forward_impl(v, nullptr, roi_dev, h_in, w_in, dy, dx, &vt, batch, t, tf->crop_h, tf->crop_w, out_dev, out_ld, zero_left, workspace_dev,
                            workspace_bytes, stream);
}

// ---- Fbank add-ons ----
int svt_deltas(const float* x, int64_t ldx, int32_t batch, int32_t t, int32_t c, int32_t window_length, float* out, int64_t ldo,
               int device, void* stream) {
  if (!x || !out) { set_error("svt_deltas: null argument"); return SVT_ERR_INVALID; }
  if (batch < 1 || t < 1 || c < 1 || window_length < 3 || ldx < c || ldo < c) { set_error("svt_deltas: bad geometry"); return SVT_ERR_INVALID; }
  if (int r = check_device(device)) return r;
  SVT_HIP(hipSetDevice(device));
  const int n = (window_length - 1) / 2;
  const float denom = (float)(n * (n + 1) * (2 * n + 1)) / 3.0f;
  if (launch_deltas(x, ldx, batch, t, c, n, 1.0f / denom, out, ldo, (hipStream_t)stream)) return SVT_ERR_HIP;
  return SVT_OK;
}
int svt_context_window(const float* x, int32_t batch, int32_t t, int32_t c, int32_t left_frames, int32_t right_frames, float* out,
                       int device, void* stream) {
  if (!x || !out) { set_error("svt_context_window: null argument"); return SVT_ERR_INVALID; }
  if (batch < 1 || t < 1 || c < 1 || left_frames < 0 || right_frames < 0) { set_error("svt_context_window: bad geometry"); return SVT_ERR_INVALID; }
  if (int r = check_device(device)) return r;
  SVT_HIP(hipSetDevice(device));
  const int ctx = left_frames + right_frames + 1, pad = left_frames > right_frames ? left_frames : right_frames;
  const int lag = right_frames > left_frames ? right_frames - left_frames : 0;
  if (launch_context_window(x, batch, t, c, ctx, lag, pad, out, (hipStream_t)stream)) return SVT_ERR_HIP;
  return SVT_OK;
}

// ---- validation losses ----
static int loss_common_checks(const char* who, int64_t batch, int64_t t_pred, int64_t t_tgt, int32_t allowed, int32_t reduction,
                              size_t ws_bytes, int64_t* T) {
  if (batch < 1 || t_pred < 1 || t_tgt < 1) { set_error(std::string(who) + ": empty input"); return SVT_ERR_INVALID; }
  if (reduction < 0 || reduction > 3) { set_error(std::string(who) + ": reduction must be 0 (mean), 1 (batchmean), 2 (batch) or 3 (none)"); return SVT_ERR_INVALID; }
  const int64_t diff = t_pred - t_tgt;
  if ((diff < 0 ? -diff : diff) > allowed) {
    // same condition and wording as speechbrain.nnet.losses.truncate (losses.py:608-613)
    set_error("Predictions and targets should be same length, but got " + std::to_string(t_pred) + " and " +
              std::to_string(t_tgt) + " respectively.");
    return SVT_ERR_INVALID;
  }
  *T = diff < 0 ? t_pred : t_tgt;
  if (ws_bytes < (size_t)batch * 24 + 8) { set_error(std::string(who) + ": workspace too small (need batch*24+8 bytes)"); return SVT_ERR_INVALID; }
  return SVT_OK;
}

int svt_bce_loss(const float* logits, int64_t batch, int64_t t_pred, const float* targets, int64_t t_tgt, const float* rel_len,
                 const float* pos_weight, int32_t allowed_len_diff, int32_t reduction, float* out, void* workspace,
                 size_t workspace_bytes, int device, void* stream) {
  if (!logits || !targets || !out || !workspace) { set_error("svt_bce_loss: null argument"); return SVT_ERR_INVALID; }
  int64_t T = 0;
  if (int r = loss_common_checks("svt_bce_loss", batch, t_pred, t_tgt, allowed_len_diff, reduction, workspace_bytes, &T)) return r;
  if (int r = check_device(device)) return r;
  SVT_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  double* sums = (double*)workspace;
  if (launch_bce_loss(logits, batch, t_pred, targets, t_tgt, T, rel_len, pos_weight, reduction == 3 ? out : nullptr, sums, s)) return SVT_ERR_HIP;
  if (reduction != 3 && launch_loss_reduce(sums, (int)batch, reduction, 0.f, out, s)) return SVT_ERR_HIP;
  return SVT_OK;
}

int svt_nll_loss(const float* log_probs, int64_t batch, int64_t t_pred, int32_t n_class, const int64_t* targets, int64_t t_tgt,
                 const float* rel_len, float label_smoothing, int32_t allowed_len_diff, int32_t reduction, float* out,
                 void* workspace, size_t workspace_bytes, int device, void* stream) {
  if (!log_probs || !targets || !out || !workspace) { set_error("svt_nll_loss: null argument"); return SVT_ERR_INVALID; }
  if (n_class < 1) { set_error("svt_nll_loss: n_class < 1"); return SVT_ERR_INVALID; }
  if (reduction == 3 && label_smoothing != 0.f) { set_error("svt_nll_loss: reduction none with label smoothing is not provided"); return SVT_ERR_INVALID; }
  int64_t T = 0;
  if (int r = loss_common_checks("svt_nll_loss", batch, t_pred, t_tgt, allowed_len_diff, reduction, workspace_bytes, &T)) return r;
  if (int r = check_device(device)) return r;
  SVT_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  double* sums = (double*)workspace;
  int* bad = (int*)((char*)workspace + (size_t)batch * 24);
  SVT_HIP(hipMemsetAsync(bad, 0, 4, s));
  if (launch_nll_loss(log_probs, batch, t_pred, n_class, targets, t_tgt, T, rel_len, reduction == 3 ? out : nullptr, sums, bad, s)) return SVT_ERR_HIP;
  if (reduction != 3 && launch_loss_reduce(sums, (int)batch, reduction, label_smoothing, out, s)) return SVT_ERR_HIP;
  return SVT_OK;
}

int svt_softmax(const float* x, int64_t rows, int32_t n, int32_t apply_log, float* y, int device, void* stream) {
  if (!x || !y) { set_error("svt_softmax: null argument"); return SVT_ERR_INVALID; }
  if (rows < 1) return SVT_OK;
  if (n < 1 || n > 4096) { set_error("svt_softmax: n must be in 1..4096"); return SVT_ERR_INVALID; }
  if (int r = check_device(device)) return r;
  SVT_HIP(hipSetDevice(device));
  if (launch_softmax_small(x, rows, n, apply_log, y, (hipStream_t)stream)) return SVT_ERR_HIP;
  return SVT_OK;
}

// ---- head-only training step (linear probe) ----
// workspace_bytes is in / out: with workspace == NULL the size the call needs is stored and nothing else happens
static int ws_query(const char* who, void* ws, size_t* ws_bytes, size_t need, bool* query) {
  *query = false;
  if (!ws_bytes) { set_error(std::string(who) + ": workspace_bytes is null"); return SVT_ERR_INVALID; }
  if (!ws) { *ws_bytes = need; *query = true; return SVT_OK; }
  if (*ws_bytes < need) {
    set_error(std::string(who) + ": workspace too small (need " + std::to_string(need) + " bytes)");
    return SVT_ERR_WORKSPACE;
  }
  return SVT_OK;
}

int svt_amt_objective_grad(const float* logits, int64_t batch, int64_t t_pred, int32_t n_out, int32_t pitch_octave_num,
                           const float* onset_targets, const float* offset_targets, const int64_t* octave_targets,
                           const int64_t* class_targets, int64_t t_tgt, const float* rel_len, float onset_pos_weight,
                           int32_t allowed_len_diff, float label_smoothing, float* terms, float* terms_host, float* dlogits,
                           void* workspace, size_t* workspace_bytes, int device, void* stream) {
  const char* who = "svt_amt_objective_grad";
  if (batch < 1 || t_pred < 1 || t_tgt < 1) { set_error(std::string(who) + ": empty input"); return SVT_ERR_INVALID; }
  bool query = false;
  if (int r = ws_query(who, workspace, workspace_bytes, amt_objective_workspace_bytes(batch), &query)) return r;
  if (query) return SVT_OK;
  if (!logits || !onset_targets || !offset_targets || !octave_targets || !class_targets || !terms || !dlogits) {
    set_error(std::string(who) + ": null argument"); return SVT_ERR_INVALID;
  }
  if (n_out < 4 || n_out > 32) { set_error(std::string(who) + ": n_out must be in 4..32"); return SVT_ERR_INVALID; }
  if (pitch_octave_num < 0 || n_out - 2 - (pitch_octave_num + 1) < 1) {
    set_error(std::string(who) + ": n_out leaves no pitch-class column after onset, offset and pitch_octave_num + 1 octave columns");
    return SVT_ERR_INVALID;
  }
  if (batch > 65535) { set_error(std::string(who) + ": batch must be <= 65535"); return SVT_ERR_INVALID; }
  if (!std::isfinite(onset_pos_weight) || !std::isfinite(label_smoothing)) { set_error(std::string(who) + ": non-finite pos_weight or label_smoothing"); return SVT_ERR_INVALID; }
  const int64_t diff = t_pred - t_tgt;
  if ((diff < 0 ? -diff : diff) > allowed_len_diff) {
    // same condition and wording as speechbrain.nnet.losses.truncate (losses.py:608-613)
    set_error("Predictions and targets should be same length, but got " + std::to_string(t_pred) + " and " +
              std::to_string(t_tgt) + " respectively.");
    return SVT_ERR_INVALID;
  }
  const int64_t T = diff < 0 ? t_pred : t_tgt;
  if (T > (int64_t(1) << 24)) { set_error(std::string(who) + ": more than 2^24 frames"); return SVT_ERR_INVALID; }
  if (int r = check_device(device)) return r;
  SVT_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  if (launch_amt_objective_grad(logits, batch, t_pred, n_out, pitch_octave_num + 1, onset_targets, offset_targets, octave_targets,
                                class_targets, t_tgt, T, rel_len, onset_pos_weight, label_smoothing, dlogits, terms, workspace, s))
    return SVT_ERR_HIP;
  // the one synchronisation of the training entry points: the target range is only known on the device
  struct { int32_t bad; float terms[5]; } st;
  SVT_HIP(hipMemcpyAsync(&st, (char*)workspace + amt_objective_status_offset(batch), sizeof(st), hipMemcpyDeviceToHost, s));
  SVT_HIP(hipStreamSynchronize(s));
  if (st.bad) {
    set_error(std::string(who) + ": an octave or class target is outside [0, n_classes) and is not -100");
    return SVT_ERR_INVALID;
  }
  if (terms_host) std::memcpy(terms_host, st.terms, sizeof(st.terms));
  return SVT_OK;
}

int svt_linear_backward(const float* x, const float* dy, int64_t rows, int32_t in_features, int32_t out_features, float* dweight,
                        float* dbias, void* workspace, size_t* workspace_bytes, int device, void* stream) {
  const char* who = "svt_linear_backward";
  if (out_features < 1 || out_features > 32) { set_error(std::string(who) + ": out_features must be in 1..32"); return SVT_ERR_INVALID; }
  if (in_features < 4 || in_features % 4 != 0) { set_error(std::string(who) + ": in_features must be a positive multiple of 4"); return SVT_ERR_INVALID; }
  if (rows < 1 || rows > 2147483647LL) { set_error(std::string(who) + ": rows must be in 1..2^31-1"); return SVT_ERR_INVALID; }
  bool query = false;
  if (int r = ws_query(who, workspace, workspace_bytes, linear_wgrad_workspace_bytes(rows, in_features, out_features), &query)) return r;
  if (query) return SVT_OK;
  if (!x || !dy || !dweight) { set_error(std::string(who) + ": null argument"); return SVT_ERR_INVALID; }
  if (((uintptr_t)x | (uintptr_t)dweight | (uintptr_t)workspace) & 15) {
    set_error(std::string(who) + ": x, dweight and workspace must be 16-byte aligned"); return SVT_ERR_INVALID;
  }
  if (int r = check_device(device)) return r;
  SVT_HIP(hipSetDevice(device));
  if (launch_linear_wgrad(x, dy, rows, in_features, out_features, dweight, dbias, workspace, (hipStream_t)stream)) return SVT_ERR_HIP;
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

int svt_linear_backward_data(const float* dy, const float* weight, int64_t rows, int32_t in_features, int32_t out_features, float* dx,
                             int device, void* stream) {
  const char* who = "svt_linear_backward_data";
  if (out_features < 1) { set_error(std::string(who) + ": out_features must be positive"); return SVT_ERR_INVALID; }
  if (in_features < 4 || in_features % 4 != 0) { set_error(std::string(who) + ": in_features must be a positive multiple of 4"); return SVT_ERR_INVALID; }
  if (rows < 0 || rows > 2147483647LL) { set_error(std::string(who) + ": rows must be in 0..2^31-1"); return SVT_ERR_INVALID; }
  if (!dy || !weight || !dx) { set_error(std::string(who) + ": null argument"); return SVT_ERR_INVALID; }
  if (((uintptr_t)weight | (uintptr_t)dx) & 15) { set_error(std::string(who) + ": weight and dx must be 16-byte aligned"); return SVT_ERR_INVALID; }
  if (int r = check_device(device)) return r;
  if (rows == 0) return SVT_OK;
  SVT_HIP(hipSetDevice(device));
  if (launch_linear_dgrad(dy, weight, rows, in_features, out_features, dx, (hipStream_t)stream)) return SVT_ERR_HIP;
  return SVT_OK;
}

int svt_clip_adadelta_step(int32_t n_tensors, float* const* params, float* const* grads, float* const* square_avg,
                           float* const* acc_delta, const int64_t* numels, float lr, double rho, float eps, float weight_decay,
                           int32_t maximize, float max_norm, float* total_norm, void* workspace, size_t* workspace_bytes, int device,
                           void* stream) {
  const char* who = "svt_clip_adadelta_step";
  if (n_tensors < 1 || n_tensors > kAdaMaxTensors) {
    set_error(std::string(who) + ": n_tensors must be in 1.." + std::to_string(kAdaMaxTensors)); return SVT_ERR_INVALID;
  }
  if (!numels) { set_error(std::string(who) + ": null argument"); return SVT_ERR_INVALID; }
  for (int i = 0; i < n_tensors; ++i)
    if (numels[i] < 0) { set_error(std::string(who) + ": negative numel"); return SVT_ERR_INVALID; }
  bool query = false;
  if (int r = ws_query(who, workspace, workspace_bytes, ada_workspace_bytes(numels, n_tensors), &query)) return r;
  if (query) return SVT_OK;
  if (!params || !grads || !square_avg || !acc_delta) { set_error(std::string(who) + ": null argument"); return SVT_ERR_INVALID; }
  for (int i = 0; i < n_tensors; ++i)
    if (numels[i] > 0 && (!params[i] || !grads[i] || !square_avg[i] || !acc_delta[i])) {
      set_error(std::string(who) + ": null tensor pointer"); return SVT_ERR_INVALID;
    }
  if (!(rho >= 0.0 && rho <= 1.0) || !(eps >= 0.f) || !(lr >= 0.f) || !(weight_decay >= 0.f) || std::isnan(max_norm)) {
    set_error(std::string(who) + ": lr, eps and weight_decay must be >= 0 and rho in [0, 1]"); return SVT_ERR_INVALID;
  }
  if (int r = check_device(device)) return r;
  SVT_HIP(hipSetDevice(device));
  // torch scales by (1 - rho) as a Python float, i.e. computed in double before the fp32 multiply
  if (launch_clip_adadelta(n_tensors, params, grads, square_avg, acc_delta, numels, lr, (float)rho, (float)(1.0 - rho), eps, weight_decay,
                           maximize ? 1 : 0, max_norm, total_norm, workspace, (hipStream_t)stream))
    return SVT_ERR_HIP;
  return SVT_OK;
}

}  // extern "C"

namespace {
struct FbankConst {
  DevBuf window, basis, mel;
  int nb = 0, nbp = 0;
};
std::mutex g_fb_mu;
std::map<std::string, FbankConst*> g_fb;

int fbank_consts(int device, int sr, int n_fft, int win, int n_mels, float f_min, float f_max, FbankConst** out) {
  const std::string key = std::to_string(device) + ":" + std::to_string(sr) + ":" + std::to_string(n_fft) + ":" +
                          std::to_string(win) + ":" + std::to_string(n_mels) + ":" + std::to_string(f_min) + ":" + std::to_string(f_max);
  std::lock_guard<std::mutex> lk(g_fb_mu);
  auto it = g_fb.find(key);
  if (it != g_fb.end()) { *out = it->second; return 0; }
  FbankConst* fc = new FbankConst();
  const int nb = n_fft / 2 + 1, nbp = round_up_int(nb, 8);
  fc->nb = nb; fc->nbp = nbp;
  // periodic hamming window of length win, centred in n_fft
  std::vector<float> window(n_fft, 0.f);
  const int left = (n_fft - win) / 2;
  for (int n = 0; n < win; ++n) window[left + n] = (float)(0.54 - 0.46 * std::cos(2.0 * M_PI * n / win));
  // DFT basis rows: [0,nb) cos, [nbp,nbp+nb) -sin, zero rows in between (keeps every row 16-byte aligned)
  std::vector<float> basis((size_t)2 * nbp * n_fft, 0.f);
  for (int k = 0; k < nb; ++k)
    for (int n = 0; n < n_fft; ++n) {
      const double a = 2.0 * M_PI * (double)((long)k * n % n_fft) / n_fft;
      basis[(size_t)k * n_fft + n] = (float)std::cos(a);
      basis[(size_t)(nbp + k) * n_fft + n] = (float)(-std::sin(a));
    }
  // triangular mel filters (speechbrain/processing/features.py:452-470,586-610), fp32 arithmetic like the reference
  std::vector<float> mel((size_t)n_mels * nbp, 0.f);
  {
    const double mlo = 2595.0 * std::log10(1.0 + f_min / 700.0), mhi = 2595.0 * std::log10(1.0 + f_max / 700.0);
    std::vector<float> hz(n_mels + 2);
    for (int i = 0; i < n_mels + 2; ++i) {
      // torch.linspace in fp32: start + i*step for the first half, end - (n-1-i)*step for the second
      const float start = (float)mlo, end = (float)mhi;
      const float step = (end - start) / (float)(n_mels + 1);
      const float m = (i < (n_mels + 2) / 2) ? start + step * (float)i : end - step * (float)(n_mels + 1 - i);
      hz[i] = 700.f * (std::pow(10.f, m / 2595.f) - 1.f);
    }
    for (int f = 0; f < n_mels; ++f) {
      const float fc_ = hz[f + 1], band = hz[f + 1] - hz[f];
      for (int k = 0; k < nb; ++k) {
        const float start = 0.f, end = (float)(sr / 2);
        const float step = (end - start) / (float)(nb - 1);
        const float fr = (k < nb / 2) ? start + step * (float)k : end - step * (float)(nb - 1 - k);
        const float slope = (fr - fc_) / band;
        const float v = std::fmax(0.f, std::fmin(slope + 1.f, -slope + 1.f));
        mel[(size_t)f * nbp + k] = v;
      }
    }
  }
  if (int r = upload_f32(fc->window, window.data(), window.size())) return r;
  if (int r = upload_f32(fc->basis, basis.data(), basis.size())) return r;
  if (int r = upload_f32(fc->mel, mel.data(), mel.size())) return r;
  g_fb[key] = fc;
  *out = fc;
  return 0;
}
}  // namespace

extern "C" {

int64_t svt_fbank_workspace_bytes(int32_t B, int64_t L, int32_t n_fft, int32_t hop, int32_t n_mels) {
  if (B < 1 || L < 1 || n_fft < 8 || hop < 1) return -1;
  const int64_t nf = 1 + L / hop;
  const int nb = n_fft / 2 + 1, nbp = round_up_int(nb, 8);
  const size_t rows = (size_t)B * nf;
  (void)n_mels;
  (void)nb;
  return (int64_t)(align_up(rows * n_fft * 4) + align_up(rows * 2 * nbp * 4) + align_up(rows * nbp * 4));
}

int svt_fbank(const float* wav, int32_t B, int64_t L, int32_t sr, int32_t n_fft, int32_t win_length, int32_t hop,
              int32_t n_mels, float f_min, float f_max, float top_db, float* out, void* workspace, size_t workspace_bytes,
              int device, void* stream) {
  if (!wav || !out || !workspace) { set_error("svt_fbank: null argument"); return SVT_ERR_INVALID; }
  if (n_fft % 4 || win_length > n_fft || n_mels < 1 || n_mels > 1024) { set_error("svt_fbank: unsupported geometry"); return SVT_ERR_INVALID; }
  const int64_t need_bytes = svt_fbank_workspace_bytes(B, L, n_fft, hop, n_mels);
  if (need_bytes < 0 || (size_t)need_bytes > workspace_bytes) { set_error("svt_fbank: workspace too small"); return SVT_ERR_WORKSPACE; }
  if (int r = check_device(device)) return r;
  FbankConst* fc = nullptr;
  if (int r = fbank_consts(device, sr, n_fft, win_length, n_mels, f_min, f_max, &fc)) return r;
  hipStream_t s = (hipStream_t)stream;
  const int64_t nf = 1 + L / hop;
  const int64_t rows = (int64_t)B * nf;
  Carver cv(workspace);
  float* frames = (float*)cv.take((size_t)rows * n_fft * 4);
  float* reim = (float*)cv.take((size_t)rows * 2 * fc->nbp * 4);
  float* power = (float*)cv.take((size_t)rows * fc->nbp * 4);
  if (int r = launch_fbank_frames(wav, B, L, n_fft, hop, nf, fc->window.as<float>(), frames, s)) return r;
  GemmArgs g;
  g.A = frames; g.W = fc->basis.p; g.C = reim;
  g.M = (int)rows; g.N = 2 * fc->nbp; g.K = n_fft; g.a_rpb = (int)rows; g.a_rstride = n_fft; g.ldw = n_fft; g.ldc = 2 * fc->nbp; g.out_f32 = 1;
  if (int r = launch_gemm(0, g, s)) return r;
  if (int r = launch_power_spectrum(reim, rows, fc->nb, fc->nbp, 2 * fc->nbp, power, fc->nbp, s)) return r;
  GemmArgs m;
  m.A = power; m.W = fc->mel.p; m.C = out;
  m.M = (int)rows; m.N = n_mels; m.K = fc->nbp; m.a_rpb = (int)rows; m.a_rstride = fc->nbp; m.ldw = fc->nbp; m.ldc = n_mels; m.out_f32 = 1;
  if (int r = launch_gemm(0, m, s)) return r;
  return launch_fbank_db(out, B, nf * n_mels, top_db, s);
}

}  // extern "C"
