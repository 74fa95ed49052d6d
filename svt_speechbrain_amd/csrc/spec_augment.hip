// SpecAugment masks on the output of the feature projection (svt_spec_augment; HF modeling_wav2vec2.py _mask_hidden_states): for the
// fp32 tensor h (B, T, D) with row pitch ld, a byte per frame time[b][t] and a byte per column feat[b][c],
//     h[b][t][c] = 0          if feat[b][c]
//                = embed[c]   else if time[b][t]
//                = unchanged  otherwise
// in ONE launch, in place, where torch runs two index_puts (a nonzero with its host synchronisation and a (B, T, D) boolean temporary
// each).  The cost follows the masked rows, not B*T*D:
//   spec_augment_kernel   a workgroup of 256 threads (four waves) takes kSpecRows consecutive frames of ONE clip at a time; up to
//                         kSpecMaxBlocks jobs each has a workgroup of its own, beyond that the workgroups stride over them.  Per job:
//                         1. the clip's feature bytes, four at a time per lane, ORed over the workgroup: `any` says whether the clip has a
//                            masked column at all (D bytes per job against kSpecRows * D * 4 of h).
//                         2. a wave owns a frame at a time.  Its time byte is read at a wave-uniform address; with neither that byte nor
//                            `any` set the frame is left alone: no load, no store.
//                         3. otherwise a lane owns four consecutive columns (16 bytes of h, of embed and 4 feature bytes), the lanes of
//                            a wave 1 KiB of the row per trip.  A time-masked frame is WRITTEN from embed and zeros without being read;
//                            in any other frame of a clip with masked columns only the 16-byte pieces that hold one are touched: stored
//                            as zeros where all four are masked, read, zeroed and stored back where some are.
// Masked elements are replaced, not multiplied: whatever was there, NaN included, does not survive.  Offsets into h are 64-bit.
#include "device_util.h"

namespace svt {
namespace {
constexpr int kSpecRows = 16;              // frames per job: four per wave
constexpr int64_t kSpecMaxBlocks = 8192;

__global__ __launch_bounds__(256) void spec_augment_kernel(float* __restrict__ h, int T, int D, int64_t ld, const uint8_t* __restrict__ time_mask,
                                                            const uint8_t* __restrict__ feat_mask, const float* __restrict__ embed,
                                                            int tiles, int64_t jobs) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int64_t job = blockIdx.x; job < jobs; job += gridDim.x) {
    const int b = (int)(job / tiles);
    const int t0 = (int)(job - (int64_t)b * tiles) * kSpecRows;
    const int t1 = min(T, t0 + kSpecRows);
    const uint8_t* fm = feat_mask ? feat_mask + (int64_t)b * D : nullptr;   // D % 4 == 0: a multiple of four bytes from a 4-byte-aligned base
    int any = 0;
    if (fm) {
      unsigned acc = 0;
      for (int c = tid * 4; c < D; c += 1024) acc |= *(const unsigned*)(fm + c);
      any = __syncthreads_or(acc != 0);      // uniform over the workgroup: every wave of a job reaches it
    }
    for (int t = t0 + wave; t < t1; t += 4) {
      const int64_t row = (int64_t)b * T + t;
      const bool masked = time_mask && time_mask[row];                      // one address per wave
      if (!masked && !any) continue;
      float* y = h + row * ld;
      for (int c = lane * 4; c < D; c += 256) {
        const unsigned f = fm ? *(const unsigned*)(fm + c) : 0u;
        if (!masked && !f) continue;
        f32x4 v;
        if (masked) v = *(const f32x4*)(embed + c);
        else if ((f & 0xffu) && (f & 0xff00u) && (f & 0xff0000u) && (f & 0xff000000u)) v = f32x4{0.f, 0.f, 0.f, 0.f};
        else v = *(const f32x4*)(y + c);
        if (f & 0xffu) v.x = 0.f;
        if (f & 0xff00u) v.y = 0.f;
        if (f & 0xff0000u) v.z = 0.f;
        if (f & 0xff000000u) v.w = 0.f;
        *(f32x4*)(y + c) = v;
      }
    }
  }
}
}  // namespace

// h (B, T, D) fp32 with row pitch ld, in place; time_mask (B*T bytes) and feat_mask (B*D bytes) may each be null, embed (D) only without
// a time mask.  D and ld multiples of 4, h and embed 16-byte aligned, feat_mask 4-byte: the caller checks (svt_spec_augment does).
// Both masks null: nothing is launched
int launch_spec_augment(float* h, int B, int T, int D, int64_t ld, const uint8_t* time_mask, const uint8_t* feat_mask, const float* embed,
                        hipStream_t s) {
  if (B < 1 || T < 1 || D < 1 || (D & 3) || (ld & 3) || ld < D || !h) { set_error("spec_augment: bad geometry"); return -1; }
  if (time_mask && !embed) { set_error("spec_augment: a time mask without the embedding"); return -1; }
  if (!aligned(15, h, embed) || !aligned(3, feat_mask)) { set_error("spec_augment: misaligned pointer"); return -1; }
  if (!time_mask && !feat_mask) return 0;
  const int tiles = (T + kSpecRows - 1) / kSpecRows;
  const int64_t jobs = (int64_t)B * tiles;
  const unsigned grid = (unsigned)(jobs < kSpecMaxBlocks ? jobs : kSpecMaxBlocks);
  hipLaunchKernelGGL(spec_augment_kernel, dim3(grid), dim3(256), 0, s, h, T, D, ld, time_mask, feat_mask, embed, tiles, jobs);
  SVT_LAUNCH_CHECK();
  return 0;
}

}  // namespace svt
