// Split-operand modes (precision "bf16x3" / "fp16x3"): every weight matrix is cut ONCE (svt_*_finalize) into packed 16-bit (hi, lo)
// pieces, which the LDS-DMA split kernels (gemm_x3s / gemm_x3p / gemm_x3q / gemm_p1x) read in place of the fp32 rows.  This file packs
// them and keeps the registry fp32 device pointer -> packed image that the dispatcher (gemm_dispatch.hip) and api.hip look up.
#include "device_util.h"
#include <map>
#include <mutex>

namespace svt {
namespace {

// fp32 (N, K) -> per row and 32-deep K slab [32 hi pieces | 32 lo pieces] (16-bit): one thread per 8 consecutive k
template <bool F16>
__global__ void split_pack_kernel(const float* __restrict__ w, long n_rows, int K, unsigned short* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;   // index of an 8-element piece
  const long per_row = K / 8;
  if (i >= n_rows * per_row) return;
  const long n = i / per_row;
  const int k0 = (int)(i % per_row) * 8;
  const float* src = w + n * K + k0;
  // the IEEE-half build rejects the split modes but keeps this kernel's symbols, and has always cut its "bf16" pieces as bf16_t = halves
  constexpr bool CUT16 = F16 || std::is_same<bf16_t, _Float16>::value;
  unsigned short h[8], l[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) cut_piece<CUT16 ? 3 : 2>(src[j], h[j], l[j]);
  unsigned short* dst = out + n * (2L * K) + (long)(k0 / 32) * 64 + (k0 % 32);
#pragma unroll
  for (int j = 0; j < 8; ++j) { dst[j] = h[j]; dst[32 + j] = l[j]; }
}

// ---- registry of split weight matrices: fp32 device pointer -> packed (hi, lo) pieces ----
struct SplitW { void* packed; int N, K, kind; };
std::map<const void*, SplitW> g_split_w;
std::mutex g_split_mu;
}  // namespace

int split_weights_register(const void* w_f32, long n_rows, int K, int kind, hipStream_t s) {
  if (kind != 2 && kind != 3) return 0;
  if (K % 32 || n_rows < 1) return 0;   // K tails stay on the register-staged split kernel
  void* packed = nullptr;
  {
    // a re-upload of the same matrix packs into the buffer it already has (no free / allocate pair beside kernels: api.hip, upload_operand)
    std::lock_guard<std::mutex> lk(g_split_mu);
    auto it = g_split_w.find(w_f32);
    if (it != g_split_w.end() && it->second.N == (int)n_rows && it->second.K == K) packed = it->second.packed;
  }
  const bool reused = packed != nullptr;
  if (reused) SVT_HIP(hipDeviceSynchronize());   // products of a forward still in flight on another stream may be reading `packed`
  if (!reused)
    if (int r = dev_alloc(&packed, (size_t)n_rows * K * 4)) return r;
  const long pieces = n_rows * (K / 8);
  if (kind == 3) hipLaunchKernelGGL((split_pack_kernel<true>), dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, s, (const float*)w_f32, n_rows, K, (unsigned short*)packed);
  else hipLaunchKernelGGL((split_pack_kernel<false>), dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, s, (const float*)w_f32, n_rows, K, (unsigned short*)packed);
  SVT_LAUNCH_CHECK();
  std::lock_guard<std::mutex> lk(g_split_mu);
  auto it = g_split_w.find(w_f32);
  if (it != g_split_w.end() && !reused) dev_free(it->second.packed);
  g_split_w[w_f32] = SplitW{packed, (int)n_rows, K, kind};
  return 0;
}
void split_weights_forget(const void* w_f32) {
  std::lock_guard<std::mutex> lk(g_split_mu);
  auto it = g_split_w.find(w_f32);
  if (it == g_split_w.end()) return;
  dev_free(it->second.packed);
  g_split_w.erase(it);
}
const void* split_weights_find(const void* W, int kind, int K, long rows_needed) {
  std::lock_guard<std::mutex> lk(g_split_mu);
  // the weight pointer may point INTO a registered matrix (row offset): find the matrix that contains it
  auto it = g_split_w.upper_bound(W);
  if (it == g_split_w.begin()) return nullptr;
  --it;
  const size_t off = (const char*)W - (const char*)it->first, row_bytes = (size_t)K * 4;
  if (it->second.kind != kind || it->second.K != K || off % row_bytes != 0 || off / row_bytes + (size_t)rows_needed > (size_t)it->second.N)
    return nullptr;
  return (const char*)it->second.packed + off;
}

}  // namespace svt
