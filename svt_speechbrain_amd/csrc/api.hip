// The library runtime behind the C ABI (include/svt_mi355.h): HIP errors, kernel profiling, device allocations, uploads and the
// attention score path that the api_*.hip entry point families share (api.h), plus the library-wide and debug entry points.
// Host code only.  The entry points of the encoder, FusionRCA, the lip front-end and the small ops live in api_<family>.hip.
#include "../../include/svt_mi355.h"
#include "api.h"
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

int upload_f32(DevBuf& b, const float* h, size_t n) {
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
// virtual-memory API).  Rule for the api*.hip files: no free / allocate pair on a path that launches kernels -- buffers are kept and reused.
static std::mutex g_stage_mu;
static std::map<int, std::pair<void*, size_t>> g_stage;
int upload_operand(int prec, DevBuf& b, const float* h, size_t n) {
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

int upload_weight(int precision, DevBuf& b, const float* h, size_t rows, size_t K) {
  if (int r = upload_operand(precision >= 2 ? 0 : precision, b, h, rows * K)) return r;
  if (precision >= 2) {
    if (int r = split_weights_register(b.p, (long)rows, (int)K, precision, 0)) return r;
    SVT_HIP(hipDeviceSynchronize());
  }
  return 0;
}

int upload_vec(const ParamMap& P, const std::string& key, int C, DevBuf* out) {
  const Param* p = nullptr;
  if (int r = need(P, key, {C}, &p)) return r;
  return upload_f32(*out, p->v.data(), p->v.size());
}
int upload_mat(int precision, const ParamMap& P, const std::string& key, int rows, int K, DevBuf* out) {
  const Param* p = nullptr;
  if (int r = need(P, key, {rows, K}, &p)) return r;
  return upload_weight(precision, *out, p->v.data(), (size_t)rows, (size_t)K);
}

// A RE-upload overwrites live weight buffers in place (DevBuf::alloc keeps a buffer of unchanged size; the uploads and conversions run
// on the null stream, which does not order against the callers' non-blocking streams): wait for every forward still in flight on this
// device -- replica() lanes share these buffers -- before the first byte changes (tests/test_gpu_uploads.py)
int begin_upload(bool& uploaded) {
  if (uploaded) SVT_HIP(hipDeviceSynchronize());
  uploaded = true;
  return SVT_OK;
}

int check_device(int device) {
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

int ws_query(const char* who, void* ws, size_t* ws_bytes, size_t need, bool* query) {
  *query = false;
  if (!ws_bytes) { set_error(std::string(who) + ": workspace_bytes is null"); return SVT_ERR_INVALID; }
  if (!ws) { *ws_bytes = need; *query = true; return SVT_OK; }
  if (*ws_bytes < need) {
    set_error(std::string(who) + ": workspace too small (need " + std::to_string(need) + " bytes)");
    return SVT_ERR_WORKSPACE;
  }
  return SVT_OK;
}

int g_debug_keep_split = 0;  // svt_debug_set(12, 1): svt_debug_gemm keeps the split copy of its weight operand between calls

}  // namespace svt

using namespace svt;

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

int svt_debug_gemm_batched(int32_t precision, const svt_debug_gemm_desc* d, int device, void* stream) {
  if (!d || d->struct_size != (int32_t)sizeof(svt_debug_gemm_desc)) { set_error("svt_debug_gemm_batched: struct_size"); return SVT_ERR_INVALID; }
  if (!d->a || !d->w || !d->c) { set_error("svt_debug_gemm_batched: null argument"); return SVT_ERR_INVALID; }
  if (!valid_precision(precision)) { set_error("svt_debug_gemm_batched: precision"); return SVT_ERR_INVALID; }
  if (d->nz < 1 || d->nz2 < 1 || d->k < 1) { set_error("svt_debug_gemm_batched: nz, nz2 and k must be positive"); return SVT_ERR_INVALID; }
  SVT_HIP(hipSetDevice(device));
  GemmArgs g;
  g.A = d->a; g.W = d->w; g.C = d->c; g.bias = d->bias; g.resid = d->resid;
  g.M = d->m; g.N = d->n; g.K = d->k; g.a_rpb = d->a_rpb; g.a_bstride = d->a_bstride; g.a_rstride = d->a_rstride;
  g.ldw = d->ldw; g.ldc = d->ldc;
  g.nz = d->nz; g.nz2 = d->nz2;
  g.a_z1 = d->a_z1; g.a_z2 = d->a_z2; g.w_z1 = d->w_z1; g.w_z2 = d->w_z2; g.c_z1 = d->c_z1; g.c_z2 = d->c_z2; g.bias_z2 = d->bias_z2;
  g.alpha = d->alpha; g.act = d->act; g.out_f32 = d->out_f32;
  // split-operand modes: the weight rows the batch spans, cut per call (the product path does it once, at finalize); the row count is
  // launch_x3's own (gemm_dispatch.hip, last_z_row)
  const bool split = precision >= 2 && d->ldw == d->k && d->k % 32 == 0 && d->w_z1 >= 0 && d->w_z2 >= 0;
  if (split) {
    const size_t last_z_row = d->nz > 1 ? ((size_t)(d->nz / d->nz2 - 1) * d->w_z1 + (size_t)(d->nz2 - 1) * d->w_z2) / (size_t)d->k : 0;
    if (split_weights_register(d->w, (long)last_z_row + d->n, d->k, precision, (hipStream_t)stream)) return SVT_ERR_HIP;
  }
  const int rc = launch_gemm(precision, g, (hipStream_t)stream);
  if (split) {
    SVT_HIP(hipStreamSynchronize((hipStream_t)stream));
    split_weights_forget(d->w);
  }
  return rc ? SVT_ERR_INVALID : SVT_OK;
}

int svt_debug_layernorm(const svt_debug_layernorm_desc* d, int device, void* stream) {
  auto refuse = [](const char* why) { set_error(std::string("svt_debug_layernorm: ") + why); return SVT_ERR_INVALID; };
  auto aligned = [](unsigned mask, auto... p) { return !((... | (uintptr_t)p) & mask); };   // a null pointer passes
  if (!d || d->struct_size != (int32_t)sizeof(svt_debug_layernorm_desc)) return refuse("struct_size");
  if (d->form < 0 || d->form > 2) return refuse("form is 0, 1 or 2");
  if (d->rows < 1 || d->D < 1) return refuse("rows and D must be positive");
  if (!d->gamma || !d->beta) return refuse("null gamma / beta");
  // what the launchers leave to their callers (the header says why the hook is narrower): decided here, before anything is launched
  const bool hilo_width = d->D == 512 || d->D == 768 || d->D == 1024;
  if (d->form == 0) {
    if (!d->x) return refuse("null x");
    if (!d->prec && !d->x_is_f32) return refuse("a 16-bit x needs prec 1");
    if (!aligned(15, d->gamma, d->beta, d->x, d->yT, d->yF, d->add, d->sumF) || !aligned(127, d->yP, d->addP))
      return refuse("every buffer 16-byte aligned, yP / addP 128-byte aligned");
  } else {
    if (!hilo_width) return refuse("the (hi, lo) forms need D in {512, 768, 1024}");
    if (!d->yh || !d->yl) return refuse("null yh / yl");
    if (!aligned(15, d->gamma, d->beta, d->branch, d->rh, d->rl, d->x32, d->yh, d->yl, d->yF, d->parts, d->pbias))
      return refuse("every buffer 16-byte aligned");
    if (d->form == 1 && !(d->x32 ? !d->rh && !d->rl : d->rh && d->rl)) return refuse("form 1 takes exactly one of x32 and (rh, rl)");
    if (d->form == 2 && (!d->rh || !d->rl)) return refuse("form 2 needs rh and rl");
    if (d->form == 2 && (d->nparts < 1 || (d->nparts > 1 && d->part_stride < d->rows * d->D))) return refuse("nparts >= 1, parts rows * D elements apart or more");
  }
  if (int r = check_device(device)) return r;
  SVT_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if (d->form == 0) {
    LnArgs a;
    a.prec = d->prec; a.x = d->x; a.x_is_f32 = d->x_is_f32; a.rows = d->rows; a.D = d->D; a.gamma = d->gamma; a.beta = d->beta;
    a.eps = d->eps; a.gelu = d->gelu; a.yT = d->yT; a.yF = d->yF; a.add = d->add; a.sumF = d->sumF; a.yP = d->yP;
    a.pair_kind = d->pair_kind; a.addP = d->addP;
    rc = launch_layernorm(a, s);
  } else if (d->form == 1) {
    rc = launch_layernorm_hilo((const bf16_t*)d->branch, (const bf16_t*)d->rh, (const bf16_t*)d->rl, d->x32, d->rows, d->D, d->gamma,
                               d->beta, d->eps, (bf16_t*)d->yh, (bf16_t*)d->yl, d->yF, s);
  } else {
    rc = launch_layernorm_hilo_parts(d->parts, d->nparts, (long)d->part_stride, d->pbias, (const bf16_t*)d->rh, (const bf16_t*)d->rl,
                                     d->rows, d->D, d->gamma, d->beta, d->eps, (bf16_t*)d->yh, (bf16_t*)d->yl, d->yF, s);
  }
  return rc ? SVT_ERR_INVALID : SVT_OK;
}

int svt_debug_dropout(const svt_debug_dropout_desc* d, int device, void* stream) {
  auto refuse = [](const char* why) { set_error(std::string("svt_debug_dropout: ") + why); return SVT_ERR_INVALID; };
  if (!d || d->struct_size != (int32_t)sizeof(svt_debug_dropout_desc)) return refuse("struct_size");
  if (d->form < 0 || d->form > 2) return refuse("form is 0, 1 or 2");
  if (!(d->p >= 0.0 && d->p < 1.0)) return refuse("p must lie in [0, 1)");
  if (d->site < 0 || d->site > 255 || d->layer < 0 || d->layer >= (1 << 24)) return refuse("site 0 .. 255, layer 0 .. 2^24 - 1");
  if (d->prec != 0 && d->prec != 1) return refuse("prec is 0 or 1");
  if (d->form == 2) {
    if (!d->S || !d->P || d->rows < 1 || d->T < 1 || d->Tp < d->T) return refuse("form 2 needs S, P, rows >= 1 and 1 <= T <= Tp");
    if (((uintptr_t)d->S & 3) || ((uintptr_t)d->P & (d->prec ? 1 : 3))) return refuse("misaligned pointer");
  } else {
    if (d->n < 1) return refuse("n must be positive");
    if (d->form == 0 ? !d->x : (!d->xh || !d->xl)) return refuse(d->form == 0 ? "null x" : "null xh / xl");
  }
  if (int r = check_device(device)) return r;
  SVT_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  const DropSpec spec = make_drop_spec(d->p, d->seed, d->step, d->site, d->layer);
  int rc;
  if (d->form == 0) rc = launch_dropout_rows(d->prec, d->x, d->n, d->e0, spec, s);
  else if (d->form == 1) rc = launch_dropout_hilo((bf16_t*)d->xh, (bf16_t*)d->xl, d->n, d->e0, spec, s);
  else rc = launch_softmax_dropout(d->prec, d->S, d->rows, d->T, d->Tp, d->P, d->e0, spec, s);
  return rc ? SVT_ERR_INVALID : SVT_OK;
}

int svt_debug_conv0(const svt_debug_conv0_desc* d, int device, void* stream) {
  auto refuse = [](const char* why) { set_error(std::string("svt_debug_conv0: ") + why); return SVT_ERR_INVALID; };
  auto aligned = [](unsigned mask, auto... p) { return !((... | (uintptr_t)p) & mask); };   // a null pointer passes
  if (!d || d->struct_size != (int32_t)sizeof(svt_debug_conv0_desc)) return refuse("struct_size");
  const int form = d->form;
  if (form < 0 || form > 6) return refuse("form is 0 .. 6");
  // what the launchers leave to their callers (the header says why the hook is narrower): decided here, before anything is launched
  if (d->k != 10 || d->stride < 1 || d->stride > 5) return refuse("k must be 10 and stride 1 .. 5");
  if (!aligned(15, d->x, d->wav, d->wav_mom, d->w0, d->b0, d->gamma, d->beta, d->mom, d->wm, d->coef, d->out))
    return refuse("every buffer 16-byte aligned");
  const bool pairs = d->pair_kind != 0, mfma = form >= 5;
  if (form == 0) {
    if (d->groups < 1 || d->groups > d->groups_max) return refuse("1 <= groups <= groups_max");
    if (d->n < 1 || (d->groups > 1 && d->n % 4)) return refuse("n >= 1, a multiple of 4 with more than one group");
    if (!d->x || !d->mom) return refuse("null x / mom");
  } else {
    if (d->B < 1 || d->T1 < 1) return refuse("B and T1 must be positive");
    if (d->L < 10 || (d->L - 10) / d->stride < d->T1 - 1) return refuse("L < (T1 - 1) * stride + 10");
    if (form == 2 ? !d->wm : !d->wav) return refuse(form == 2 ? "null wm" : "null wav");
  }
  if (form == 1 && !d->wm) return refuse("null wm");
  if (form >= 2) {
    if (d->C < 1 || d->C > 512 || (form > 2 && d->C % 8)) return refuse("C in 1 .. 512, a multiple of 8 for the forms that write rows");
    if (mfma && d->C != 512) return refuse("the matrix-pipe forms need C = 512");
    if (d->pair_kind != 0 && d->pair_kind != 2 && d->pair_kind != 3) return refuse("pair_kind is 0, 2 or 3");
  }
  if (form == 2 || form == 4 || form == 6) {
    if (d->cpg < 1 || d->B % d->cpg) return refuse("cpg >= 1 and a divisor of B");
    if (d->wav_mom && d->n_wav < 1) return refuse("wav_mom needs n_wav >= 1");
    if (!d->w0 || !d->gamma || !d->beta) return refuse("null w0 / gamma / beta");
  }
  if (form == 2 && !d->coef) return refuse("null coef");
  if (form >= 3) {
    if (!d->out) return refuse("null out");
    if ((form == 3 || form == 5) && !d->coef) return refuse("null coef");
    if (!mfma && (d->prec < 0 || d->prec > 1)) return refuse("prec is 0 or 1");
    if (!mfma && pairs && (d->prec || d->C % 32)) return refuse("pair rows need prec 0 and C % 32 == 0");
    if ((pairs || mfma) && !aligned(127, d->out)) return refuse("a pair-row out and every out of forms 5 and 6 128-byte aligned");
  }
  if (int r = check_device(device)) return r;
  SVT_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  // scratch: tickets (zeroed once) in front of the partials for forms 0 and 1, the table workspace for forms 5 and 6; the rest 0xFF
  const int n_tickets = form == 0 ? d->groups_max : form == 1 ? d->B : 0;
  const size_t bytes = form == 0 ? moments_scratch_bytes(d->groups_max) : form == 1 ? conv0_window_moments_scratch_bytes(d->B, d->T1)
                     : mfma ? conv0_mfma_table_bytes(d->B) : 0;
  void* scratch = nullptr;
  int rc = SVT_OK;
  if (bytes) {
    rc = dev_alloc(&scratch, bytes);
    if (!rc && (hipMemsetAsync(scratch, 0xFF, bytes, s) != hipSuccess ||
                (n_tickets && hipMemsetAsync(scratch, 0, moments_ticket_bytes(n_tickets), s) != hipSuccess))) {
      set_error("svt_debug_conv0: hipMemsetAsync"); rc = SVT_ERR_HIP;
    }
  }
  for (int it = 0; !rc && it < (d->repeat > 1 ? d->repeat : 1); ++it) {
    int lr;
    if (form == 0) lr = launch_moments(d->x, d->n, d->mom, scratch, d->groups_max, s, d->groups);
    else if (form == 1) lr = launch_conv0_window_moments(d->wav, d->B, d->L, d->k, d->stride, d->T1, d->wm, scratch, s);
    else if (form == 2) lr = launch_conv0_group_coef(d->wav_mom, d->n_wav, d->wm, d->B, d->T1, d->C, d->k, d->w0, d->b0, d->gamma, d->beta,
                                                     d->eps_wav, d->eps, d->coef, s, d->cpg);
    else if (form == 3) lr = launch_conv0_group_apply(d->prec, d->wav, d->B, d->L, d->k, d->stride, d->T1, d->C, d->coef, d->out, s, d->pair_kind);
    else if (form == 4) lr = launch_conv0_layer(d->prec, d->wav, d->B, d->L, d->k, d->stride, d->T1, d->C, d->wav_mom, d->n_wav, d->eps_wav, d->w0,
                                                d->b0, d->gamma, d->beta, d->eps, d->out, s, d->cpg, d->pair_kind);
    else if (form == 5) lr = launch_conv0_mfma_group(d->wav, d->B, d->L, d->stride, d->T1, d->coef, scratch, d->out, s, d->pair_kind);
    else lr = launch_conv0_mfma_layer(d->wav, d->B, d->L, d->stride, d->T1, d->wav_mom, d->n_wav, d->eps_wav, d->w0, d->b0, d->gamma, d->beta,
                                      d->eps, scratch, d->out, s, d->cpg, d->pair_kind);
    if (lr) rc = SVT_ERR_INVALID;
  }
  if (hipStreamSynchronize(s) != hipSuccess && !rc) { set_error("svt_debug_conv0: hipStreamSynchronize"); rc = SVT_ERR_HIP; }
  if (!rc && n_tickets && d->tickets_out &&
      hipMemcpy(d->tickets_out, scratch, (size_t)n_tickets * 4, hipMemcpyDeviceToHost) != hipSuccess) {
    set_error("svt_debug_conv0: hipMemcpy"); rc = SVT_ERR_HIP;
  }
  if (scratch) dev_free(scratch);
  return rc;
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
    AttnArgs a;
    a.gp = precision; a.Q = q; a.K = k; a.V = v; a.ldq = ldq; a.ldkv = ldkv; a.out = o; a.ldo = ldo;
    a.B = batch; a.T = t; a.H = heads; a.dh = head_dim; a.scale = scale;
    const AttnPlan plan = plan_attention(attn_geom(a));
    if (plan.path != ATTN_FUSED_X3 || plan.planes_q) {
      set_error("svt_debug_attention: the split-operand kernel is exposed for a packed q|k|v projection"); return SVT_ERR_INVALID; }
    AttnBufs ab{};   // the plan needs the planes of the packed projection and nothing else
    if (int r = dev_alloc(&ab.pl_qkv, (size_t)batch * t * 3 * heads * head_dim * 4)) return r;
    const int rc = launch_attention(a, ab, (hipStream_t)stream);
    (void)hipStreamSynchronize((hipStream_t)stream);
    dev_free(ab.pl_qkv);
    return rc ? SVT_ERR_INVALID : SVT_OK;
  }
  if (launch_flash_attention(q, ldq, (long)t * ldq, k, v, ldkv, (long)t * ldkv, o, ldo, (long)t * ldo, batch, t, heads,
                             head_dim, scale, (hipStream_t)stream)) return SVT_ERR_INVALID;
  return SVT_OK;
}

int svt_debug_attention_dropout(const svt_debug_attention_dropout_desc* d, int device, void* stream) {
  auto refuse = [](const char* why) { set_error(std::string("svt_debug_attention_dropout: ") + why); return SVT_ERR_INVALID; };
  if (!d) return refuse("null descriptor");
  if (d->struct_size != (int32_t)sizeof(svt_debug_attention_dropout_desc)) return refuse("struct_size");
  if (!d->q || !d->k || !d->v || !d->o) return refuse("null argument");
  if (d->batch < 1 || d->t < 1 || d->heads < 1) return refuse("batch, t and heads must be positive");
  AttnGeom g;
  g.prec = g.gp = d->precision; g.dh = d->head_dim; g.T = d->t; g.drop = g.fused_drop = true;
  if (plan_attention(g).path != ATTN_FUSED16_DROP)
    return refuse("the fused kernel serves precision SVT_PREC_BF16 (the build's 16-bit operand type) at head_dim 64 / 128 only");
  if (!(d->p >= 0.0 && d->p < 1.0)) return refuse("p must lie in [0, 1)");
  if (d->layer < 0 || d->layer > 0xFFFFFF) return refuse("layer");
  if (int r = check_device(device)) return r;
  SVT_HIP(hipSetDevice(device));
  const DropSpec spec = make_drop_spec(d->p, d->seed, d->step, 2, d->layer);
  if (launch_flash_attention_dropout(d->q, d->ldq, (long)d->t * d->ldq, d->k, d->v, d->ldkv, (long)d->t * d->ldkv, d->o, d->ldo,
                                     (long)d->t * d->ldo, d->batch, d->t, d->heads, d->head_dim, d->scale, d->e0, spec,
                                     (hipStream_t)stream)) return SVT_ERR_INVALID;
  return SVT_OK;
}

int svt_debug_attention_bias(const void* q, const void* k, const void* v, void* o, int32_t batch, int32_t t, int32_t heads, int64_t ldq,
                             int64_t ldkv, int64_t ldo, float scale, const float* gate_dev, const float* pos_bias_dev, int device,
                             void* stream) {
  if (!q || !k || !v || !o || !gate_dev || !pos_bias_dev) { set_error("svt_debug_attention_bias: null argument"); return SVT_ERR_INVALID; }
  if (batch < 1 || t < 1 || heads < 1) { set_error("svt_debug_attention_bias: batch, t and heads must be positive"); return SVT_ERR_INVALID; }
  if (int r = check_device(device)) return r;
  SVT_HIP(hipSetDevice(device));
  if (launch_flash_attention(q, ldq, (long)t * ldq, k, v, ldkv, (long)t * ldkv, o, ldo, (long)t * ldo, batch, t, heads, 64, scale,
                             (hipStream_t)stream, gate_dev, pos_bias_dev)) return SVT_ERR_INVALID;
  return SVT_OK;
}

int svt_debug_attention_scores(int32_t precision, const void* q, const void* k, const void* v, void* o, int32_t batch, int32_t t,
                               int32_t heads, int32_t head_dim, int64_t ldq, int64_t ldkv, int64_t ldo, float scale,
                               const float* gate_dev, const float* pos_bias_dev, int device, void* stream) {
  if (!q || !k || !v || !o) { set_error("svt_debug_attention_scores: null argument"); return SVT_ERR_INVALID; }
  if (!valid_precision(precision)) { set_error("svt_debug_attention_scores: precision"); return SVT_ERR_INVALID; }
  if (batch < 1 || t < 1 || heads < 1 || head_dim < 1) { set_error("svt_debug_attention_scores: batch, t, heads and head_dim must be positive"); return SVT_ERR_INVALID; }
  if (!gate_dev != !pos_bias_dev) { set_error("svt_debug_attention_scores: gate and pos_bias come together"); return SVT_ERR_INVALID; }
  const int prec = storage_prec(precision);
  AttnArgs a;
  a.prec = prec; a.gp = precision; a.Q = q; a.K = k; a.V = v; a.ldq = ldq; a.ldkv = ldkv; a.out = o; a.ldo = ldo;
  a.B = batch; a.T = t; a.H = heads; a.dh = head_dim; a.scale = scale; a.gate = gate_dev; a.relpb = pos_bias_dev;
  const AttnPlan plan = plan_attention(attn_geom(a));
  if (plan.path != ATTN_SCORES) {
    set_error("svt_debug_attention_scores: this geometry runs the fused kernel (svt_debug_attention / svt_debug_attention_bias)"); return SVT_ERR_INVALID; }
  if (int r = check_device(device)) return r;
  SVT_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  const int Tp = plan.Tp;
  const size_t bh = (size_t)batch * heads;
  const size_t bytes[3] = {bh * t * Tp * 4, bh * t * Tp * esize(prec), bh * head_dim * Tp * esize(prec)};
  void* buf[3] = {nullptr, nullptr, nullptr};
  int rc = 0;
  for (int i = 0; i < 3 && !rc; ++i) {
    rc = dev_alloc(&buf[i], bytes[i]);
    if (!rc && hipMemsetAsync(buf[i], 0xFF, bytes[i], s) != hipSuccess) { set_error("svt_debug_attention_scores: hipMemsetAsync"); rc = SVT_ERR_HIP; }
  }
  if (!rc) {
    AttnBufs ab{};
    ab.S = (float*)buf[0]; ab.P = buf[1]; ab.Vt = buf[2];
    rc = launch_attention(a, ab, s) ? SVT_ERR_INVALID : SVT_OK;
  }
  (void)hipStreamSynchronize(s);
  for (int i = 0; i < 3; ++i) dev_free(buf[i]);
  return rc;
}

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
  else if (key == 38) return g_flash_kernel_id;
  else if (key == 39) return g_gemm_kernel_id;
  else if (key == 40) return g_ln_kernel_id;
  else if (key == 41) return g_c0_kernel_id;
  else if (key == 42) return g_vpad_kernel_id;
  else if (key == 43) return g_vstep_kernel_id;
  else if (key == 44) return g_dropout_kernel_id;
  else if (key == 45) return g_glue_kernel_id;
  else if (key == 46) return g_attn_bwd_id;
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

}  // extern "C"
