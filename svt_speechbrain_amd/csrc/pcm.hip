// PCM <-> fp32 on the raw bytes of a wav file (svt_pcm_decode, svt_pcm_encode): interleaved little-endian frames at ANY byte address on one
// side, planar fp32 rows (4-byte aligned, any pitch >= frames) on the other.  Both kernels are bandwidth-bound: no LDS, no atomics, no
// workspace; a workgroup of 256 threads takes kPcmFrames consecutive frames at a time and the grid is capped at kPcmBlocks.
//   pcm_decode_kernel<F, C, DM>   a lane takes a group of K frames = NB = K * block_align bytes (K = 4, 8 or 16: NB is a multiple of 16).
//                                 With r = src & 3 -- the same for every group -- it reads the NB / 4 (+ 1 when r != 0) 4-byte-aligned
//                                 words that cover the group, as NB / 16 16-byte loads that promise 4-byte alignment, funnels
//                                 every pair down by r bytes (v_alignbyte_b32) and takes the samples apart with shifts and bit-field
//                                 extracts on registers; then K / 4 16-byte stores to each channel row.
//   pcm_encode_kernel<F, C, MIS>  the way back.  A lane reads K frames of every row (16-byte loads), packs them into NB / 4 words of the
//                                 interleaved stream and stores them.  MIS (dst & 3 = r != 0): the lane owns the aligned words that begin r
//                                 bytes in FRONT of its group, so it also encodes the 4 stream bytes before the group (one or two samples:
//                                 an L1 hit) and funnels by 4 - r; every store is then a whole aligned word and no two lanes share one.
// Addressing: a vector group g runs over [g_lo, g_hi).  Decode: g_lo = 1 when r != 0 (the first word would begin before src) and g_hi
// is the last group whose closing word, which reaches 4 - r bytes beyond the group, ends inside the source.  Encode: g_lo = 1 when r != 0,
// g_hi = frames / K, and the r bytes that the last vector group leaves to its successor belong to the byte-wise tail.  Everything else --
// at most three groups -- is done by workgroup 0 with byte loads (decode: one sample per thread) or byte stores (encode: one byte per
// thread).  So no access touches a byte outside [src, src + frames * block_align) or outside the frames elements of a row, all indices
// are 64-bit, and every vector access is typed with the 4-byte alignment it really has (global_load / store_dwordx4 ask for no more).
#include "../../include/svt_mi355.h"
#include "device_util.h"

namespace svt {
namespace {
constexpr int kPcmFrames = SVT_PCM_FRAMES_PER_WORKGROUP;
constexpr int kPcmBlocks = SVT_PCM_MAX_WORKGROUPS;
typedef unsigned u32x4u __attribute__((ext_vector_type(4), aligned(4)));   // 16 bytes at a 4-byte-aligned address
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));

constexpr int pcm_bytes(int F) { return F == SVT_PCM_U8 ? 1 : F == SVT_PCM_S16 ? 2 : F == SVT_PCM_S24 ? 3 : F == SVT_PCM_F64 ? 8 : 4; }
// frames per lane: the smallest multiple of 4 (16-byte stores to a row) whose frames are whole 16-byte words, so the body is 16-byte
// loads and nothing else: 4, 8 or 16 frames for a block_align that is a multiple of 4, even, or odd
constexpr int pcm_group(int block_align) { return block_align % 4 == 0 ? 4 : block_align % 2 == 0 ? 8 : 16; }

__device__ __forceinline__ unsigned f2u(float x) { return __builtin_bit_cast(unsigned, x); }
__device__ __forceinline__ float u2f(unsigned x) { return __builtin_bit_cast(float, x); }

// sample i of a stream of format F held in the words s (byte 0 of the stream = the low byte of s[0]), as fp32 bits
template <int F, int N>
__device__ __forceinline__ unsigned decode_bits(const unsigned (&s)[N], int i) {
  if constexpr (F == SVT_PCM_U8) {
    const int b = (int)((s[i >> 2] >> (8 * (i & 3))) & 0xffu);
    return f2u((float)(b - 128) * 0x1p-7f);
  } else if constexpr (F == SVT_PCM_S16) {
    const int x = (int)(s[i >> 1] << (16 * (1 - (i & 1)))) >> 16;
    return f2u((float)x * 0x1p-15f);
  } else if constexpr (F == SVT_PCM_S24) {
    const int o = 3 * i, j = o >> 2, k = o & 3;
    unsigned w;   // the sample in bits 8..31
    if (k == 0) w = s[j] << 8;
    else if (k == 1) w = s[j];
    else w = __builtin_amdgcn_alignbyte(s[j + 1 < N ? j + 1 : j], s[j], (unsigned)(k - 1));
    return f2u((float)((int)(w & 0xffffff00u) >> 8) * 0x1p-23f);
  } else if constexpr (F == SVT_PCM_S32) {
    return f2u((float)(int)s[i] * 0x1p-31f);
  } else if constexpr (F == SVT_PCM_F32) {
    return s[i];
  } else {
    const double d = __builtin_bit_cast(double, (unsigned long long)s[2 * i] | ((unsigned long long)s[2 * i + 1] << 32));
    return f2u((float)d);
  }
}

template <int F>
__device__ __forceinline__ unsigned decode_bytes(const unsigned char* p) {   // one sample from byte loads
  unsigned w[2] = {0u, 0u};
#pragma unroll
  for (int b = 0; b < pcm_bytes(F); ++b) w[b >> 2] |= (unsigned)p[b] << (8 * (b & 3));
  return decode_bits<F, 2>(w, 0);
}

struct PcmSpan { int64_t g_lo, g_hi; };
// the vector groups of a decode: NB bytes each, the source r bytes behind a 4-byte boundary, total bytes in all
__host__ __device__ inline PcmSpan decode_span(unsigned r, int64_t total, int NB) {
  PcmSpan s;
  s.g_lo = r ? 1 : 0;
  s.g_hi = (total - (r ? 4 - (int64_t)r : 0)) / NB;
  if (s.g_hi < s.g_lo) s.g_hi = s.g_lo;
  return s;
}
__host__ __device__ inline PcmSpan encode_span(unsigned r, int64_t frames, int K) {
  PcmSpan s;
  s.g_lo = r ? 1 : 0;
  s.g_hi = frames / K;
  if (s.g_hi < s.g_lo) s.g_hi = s.g_lo;
  return s;
}

template <int F, int C, bool DM>
__global__ __launch_bounds__(256) void pcm_decode_kernel(const unsigned char* __restrict__ src, int64_t frames, float* __restrict__ out,
                                                         int64_t ld) {
  constexpr int BPS = pcm_bytes(F), B = BPS * C, K = pcm_group(B), NB = K * B, ND = NB / 4, GPT = kPcmFrames / K;
  static_assert(NB % 16 == 0 && GPT % 256 == 0, "a group is whole 16-byte words; a tile is whole trips of the workgroup");
  const unsigned r = (unsigned)((uintptr_t)src & 3);
  const PcmSpan sp = decode_span(r, frames * B, NB);
  const int64_t n_tiles = (sp.g_hi - sp.g_lo + GPT - 1) / GPT;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
#pragma unroll
    for (int it = 0; it < GPT / 256; ++it) {
      const int64_t g = sp.g_lo + tile * GPT + it * 256 + threadIdx.x;
      if (g >= sp.g_hi) continue;
      const unsigned char* a4 = src + g * NB - r;   // 4-byte aligned, inside the source (g >= 1 when r != 0)
      unsigned d[ND + 1];
#pragma unroll
      for (int i = 0; i < ND / 4; ++i) {
        const u32x4u v = *(const u32x4u*)(a4 + 16 * i);
        d[4 * i] = v.x; d[4 * i + 1] = v.y; d[4 * i + 2] = v.z; d[4 * i + 3] = v.w;
      }
      d[ND] = r ? *(const unsigned*)(a4 + 4 * ND) : 0u;   // the closing word: only a misaligned source has bytes in it
      unsigned s[ND];
#pragma unroll
      for (int j = 0; j < ND; ++j) s[j] = __builtin_amdgcn_alignbyte(d[j + 1], d[j], r);
      float* o = out + g * K;
      if constexpr (DM) {
#pragma unroll
        for (int m = 0; m < K / 4; ++m) {
          u32x4u v;
#pragma unroll
          for (int e = 0; e < 4; ++e)
            v[e] = f2u(0.5f * (u2f(decode_bits<F, ND>(s, 2 * (4 * m + e))) + u2f(decode_bits<F, ND>(s, 2 * (4 * m + e) + 1))));
          *(u32x4u*)(o + 4 * m) = v;
        }
      } else {
#pragma unroll
        for (int c = 0; c < C; ++c) {
#pragma unroll
          for (int m = 0; m < K / 4; ++m) {
            u32x4u v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = decode_bits<F, ND>(s, (4 * m + e) * C + c);
            *(u32x4u*)(o + c * ld + 4 * m) = v;
          }
        }
      }
    }
  }
  if (blockIdx.x == 0) {   // the frames outside the vector groups, from byte loads: one sample (downmix: one frame) per thread
    constexpr int PER = DM ? 1 : C;
    const int64_t head_n = sp.g_lo * K < frames ? sp.g_lo * K : frames;
    const int64_t tail0 = sp.g_hi * K < frames ? sp.g_hi * K : frames;
    const int64_t n_rest = (head_n + (frames - tail0)) * PER;
    for (int64_t j = threadIdx.x; j < n_rest; j += 256) {
      const int64_t q = j / PER, c = j % PER;
      const int64_t f = q < head_n ? q : tail0 + (q - head_n);
      const unsigned char* p = src + f * B + c * BPS;
      if constexpr (DM) out[f] = 0.5f * (u2f(decode_bytes<F>(p)) + u2f(decode_bytes<F>(p + BPS)));
      else ((unsigned*)out)[c * ld + f] = decode_bytes<F>(p);
    }
  }
}

// q = clamp(rint(x * 32768), -32768, 32767): ties to even (v_rndne_f32), NaN -> 0, the scale exact
__device__ __forceinline__ unsigned s16_of(float x) {
  float y = rintf(x * 32768.f);
  y = fminf(fmaxf(y, -32768.f), 32767.f);
  return x != x ? 0u : (unsigned)(int)y & 0xffffu;
}
template <int F>
__device__ __forceinline__ unsigned encode_word(float x) { return F == SVT_PCM_F32 ? f2u(x) : s16_of(x); }

template <int F, int C, bool MIS>
__global__ __launch_bounds__(256) void pcm_encode_kernel(const float* __restrict__ in, int64_t ld, int64_t frames,
                                                         unsigned char* __restrict__ dst) {
  constexpr int BPS = pcm_bytes(F), B = BPS * C, K = pcm_group(B), NB = K * B, ND = NB / 4, GPT = kPcmFrames / K, SPW = 4 / BPS;
  static_assert(F == SVT_PCM_S16 || F == SVT_PCM_F32, "the two formats the reference writes");
  static_assert(NB % 16 == 0 && GPT % 256 == 0, "a group is whole 16-byte words; a tile is whole trips of the workgroup");
  const unsigned r = (unsigned)((uintptr_t)dst & 3);
  const PcmSpan sp = encode_span(r, frames, K);
  const int64_t n_tiles = (sp.g_hi - sp.g_lo + GPT - 1) / GPT;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
#pragma unroll
    for (int it = 0; it < GPT / 256; ++it) {
      const int64_t g = sp.g_lo + tile * GPT + it * 256 + threadIdx.x;
      if (g >= sp.g_hi) continue;
      const int64_t f0 = g * K;
      unsigned e[C][K];   // the encoded samples (S16: the low 16 bits)
#pragma unroll
      for (int c = 0; c < C; ++c) {
#pragma unroll
        for (int m = 0; m < K / 4; ++m) {
          const f32x4u x = *(const f32x4u*)(in + c * ld + f0 + 4 * m);
          e[c][4 * m] = encode_word<F>(x.x); e[c][4 * m + 1] = encode_word<F>(x.y);
          e[c][4 * m + 2] = encode_word<F>(x.z); e[c][4 * m + 3] = encode_word<F>(x.w);
        }
      }
      unsigned s[ND];   // the group's words of the interleaved stream
#pragma unroll
      for (int j = 0; j < ND; ++j) {
        if constexpr (F == SVT_PCM_F32) s[j] = e[j % C][j / C];
        else s[j] = e[(2 * j) % C][(2 * j) / C] | (e[(2 * j + 1) % C][(2 * j + 1) / C] << 16);
      }
      unsigned char* a = dst + g * NB;
      if constexpr (MIS) {
        // the 4 stream bytes in front of the group: samples f0 * C - SPW .. f0 * C - 1 of the interleaved order (g >= 1 here)
        unsigned prev = 0u;
#pragma unroll
        for (int q = 0; q < SPW; ++q) {
          const int64_t i = f0 * C - SPW + q;
          prev |= encode_word<F>(in[(i % C) * ld + i / C]) << (8 * BPS * q);
        }
        unsigned t[ND];
#pragma unroll
        for (int j = 0; j < ND; ++j) t[j] = __builtin_amdgcn_alignbyte(s[j], j ? s[j > 0 ? j - 1 : 0] : prev, 4u - r);
#pragma unroll
        for (int j = 0; j < ND; ++j) s[j] = t[j];
        a -= r;
      }
#pragma unroll
      for (int i = 0; i < ND / 4; ++i) *(u32x4u*)(a + 16 * i) = u32x4u{s[4 * i], s[4 * i + 1], s[4 * i + 2], s[4 * i + 3]};
    }
  }
  if (blockIdx.x == 0) {   // the bytes outside the vector groups' words: one byte per thread
    const int64_t total = frames * B;
    const int64_t lead = sp.g_hi > sp.g_lo ? r : 0;   // the vector groups' words begin and end r bytes in front of the groups
    const int64_t head_b = sp.g_lo * NB - lead < total ? sp.g_lo * NB - lead : total;
    int64_t tail0 = sp.g_hi * NB - lead;
    tail0 = tail0 < head_b ? head_b : tail0 > total ? total : tail0;
    const int64_t n_rest = head_b + (total - tail0);
    for (int64_t j = threadIdx.x; j < n_rest; j += 256) {
      const int64_t b = j < head_b ? j : tail0 + (j - head_b);
      const int64_t i = b / BPS;
      const unsigned w = encode_word<F>(in[(i % C) * ld + i / C]);
      dst[b] = (unsigned char)((w >> (8 * (int)(b % BPS))) & 0xffu);
    }
  }
}

template <int F, int C, bool DM>
int decode_go(const void* src, int64_t frames, float* out, int64_t ld, hipStream_t s) {
  constexpr int B = pcm_bytes(F) * C, K = pcm_group(B), GPT = kPcmFrames / K;
  const PcmSpan sp = decode_span((unsigned)((uintptr_t)src & 3), frames * B, K * B);
  const int64_t n_tiles = (sp.g_hi - sp.g_lo + GPT - 1) / GPT;
  const int grid = (int)(n_tiles < 1 ? 1 : n_tiles > kPcmBlocks ? kPcmBlocks : n_tiles);
  hipLaunchKernelGGL((pcm_decode_kernel<F, C, DM>), dim3(grid), dim3(256), 0, s, (const unsigned char*)src, frames, out, ld);
  SVT_LAUNCH_CHECK();
  return 0;
}
template <int F>
int decode_f(const void* src, int C, int64_t frames, float* out, int64_t ld, bool dm, hipStream_t s) {
  if (dm) return decode_go<F, 2, true>(src, frames, out, ld, s);
  switch (C) {
    case 1: return decode_go<F, 1, false>(src, frames, out, ld, s);
    case 2: return decode_go<F, 2, false>(src, frames, out, ld, s);
    case 3: return decode_go<F, 3, false>(src, frames, out, ld, s);
    case 4: return decode_go<F, 4, false>(src, frames, out, ld, s);
    case 5: return decode_go<F, 5, false>(src, frames, out, ld, s);
    case 6: return decode_go<F, 6, false>(src, frames, out, ld, s);
    case 7: return decode_go<F, 7, false>(src, frames, out, ld, s);
    default: return decode_go<F, 8, false>(src, frames, out, ld, s);
  }
}

template <int F, int C>
int encode_go(const float* in, int64_t ld, int64_t frames, void* dst, hipStream_t s) {
  constexpr int B = pcm_bytes(F) * C, K = pcm_group(B), GPT = kPcmFrames / K;
  const unsigned r = (unsigned)((uintptr_t)dst & 3);
  const PcmSpan sp = encode_span(r, frames, K);
  const int64_t n_tiles = (sp.g_hi - sp.g_lo + GPT - 1) / GPT;
  const int grid = (int)(n_tiles < 1 ? 1 : n_tiles > kPcmBlocks ? kPcmBlocks : n_tiles);
  if (r) hipLaunchKernelGGL((pcm_encode_kernel<F, C, true>), dim3(grid), dim3(256), 0, s, in, ld, frames, (unsigned char*)dst);
  else hipLaunchKernelGGL((pcm_encode_kernel<F, C, false>), dim3(grid), dim3(256), 0, s, in, ld, frames, (unsigned char*)dst);
  SVT_LAUNCH_CHECK();
  return 0;
}
template <int F>
int encode_f(const float* in, int64_t ld, int C, int64_t frames, void* dst, hipStream_t s) {
  switch (C) {
    case 1: return encode_go<F, 1>(in, ld, frames, dst, s);
    case 2: return encode_go<F, 2>(in, ld, frames, dst, s);
    case 3: return encode_go<F, 3>(in, ld, frames, dst, s);
    case 4: return encode_go<F, 4>(in, ld, frames, dst, s);
    case 5: return encode_go<F, 5>(in, ld, frames, dst, s);
    case 6: return encode_go<F, 6>(in, ld, frames, dst, s);
    case 7: return encode_go<F, 7>(in, ld, frames, dst, s);
    default: return encode_go<F, 8>(in, ld, frames, dst, s);
  }
}
}  // namespace

int launch_pcm_decode(const void* src, int format, int channels, int64_t frames, float* out, int64_t ld, bool downmix, hipStream_t s) {
  if (!src || !out || channels < 1 || channels > 8 || frames < 1 || ld < frames || (downmix && channels != 2) || !aligned(3, out)) {
    set_error("pcm_decode: bad geometry"); return -1; }
  switch (format) {
    case SVT_PCM_U8: return decode_f<SVT_PCM_U8>(src, channels, frames, out, ld, downmix, s);
    case SVT_PCM_S16: return decode_f<SVT_PCM_S16>(src, channels, frames, out, ld, downmix, s);
    case SVT_PCM_S24: return decode_f<SVT_PCM_S24>(src, channels, frames, out, ld, downmix, s);
    case SVT_PCM_S32: return decode_f<SVT_PCM_S32>(src, channels, frames, out, ld, downmix, s);
    case SVT_PCM_F32: return decode_f<SVT_PCM_F32>(src, channels, frames, out, ld, downmix, s);
    case SVT_PCM_F64: return decode_f<SVT_PCM_F64>(src, channels, frames, out, ld, downmix, s);
    default: set_error("pcm_decode: unknown format"); return -1;
  }
}

int launch_pcm_encode(const float* in, int64_t ld, int channels, int64_t frames, int format, void* dst, hipStream_t s) {
  if (!in || !dst || channels < 1 || channels > 8 || frames < 1 || ld < frames || !aligned(3, in)) {
    set_error("pcm_encode: bad geometry"); return -1; }
  switch (format) {
    case SVT_PCM_S16: return encode_f<SVT_PCM_S16>(in, ld, channels, frames, dst, s);
    case SVT_PCM_F32: return encode_f<SVT_PCM_F32>(in, ld, channels, frames, dst, s);
    default: set_error("pcm_encode: only S16 and F32 are written"); return -1;
  }
}

}  // namespace svt
