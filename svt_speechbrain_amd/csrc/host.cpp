// Host-only routines of the C-ABI (see host.h): no HIP call, no device pointer is dereferenced here.
#include "host.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace svt {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }

int load_param_into(ParamMap& m, const char* key, const void* data, int dtype, const int64_t* shape, int ndim) {
  if (!key || !data || (ndim > 0 && !shape) || ndim < 0 || ndim > 6) { set_error("load_param: bad argument"); return SVT_ERR_INVALID; }
  if (dtype != SVT_F32) { set_error("load_param: only SVT_F32 host tensors are accepted"); return SVT_ERR_INVALID; }
  Param p;
  int64_t n = 1;
  for (int i = 0; i < ndim; ++i) {   // no negative extent, no product beyond 2^40 elements (also keeps the multiplication from overflowing)
    if (shape[i] < 0 || (shape[i] > 0 && n > ((int64_t)1 << 40) / shape[i])) { set_error("load_param: bad shape"); return SVT_ERR_INVALID; }
    n *= shape[i];
  }
  if (ndim > 0) p.shape.assign(shape, shape + ndim);
  p.v.assign((const float*)data, (const float*)data + n);
  m[key] = std::move(p);
  return SVT_OK;
}

const Param* find(const ParamMap& m, const std::string& k) {
  auto it = m.find(k);
  return it == m.end() ? nullptr : &it->second;
}

int need(const ParamMap& m, const std::string& k, std::vector<int64_t> shape, const Param** out) {
  const Param* p = find(m, k);
  if (!p) { set_error("missing parameter: " + k); return SVT_ERR_KEY; }
  if (p->shape != shape) {
    std::string s = "parameter " + k + " has shape (";
    for (auto d : p->shape) s += std::to_string(d) + ",";
    s += ") expected (";
    for (auto d : shape) s += std::to_string(d) + ",";
    set_error(s + ")");
    return SVT_ERR_INVALID;
  }
  *out = p;
  return SVT_OK;
}

int validate_cfg(const svt_encoder_config& c) {
  if (c.struct_size != (int32_t)sizeof(svt_encoder_config)) { set_error("svt_encoder_config: struct_size mismatch (ABI)"); return SVT_ERR_INVALID; }
  if (c.num_conv_layers < 0 || c.num_conv_layers > SVT_MAX_CONV_LAYERS) { set_error("num_conv_layers out of range"); return SVT_ERR_INVALID; }
  if (c.num_conv_layers == 0) {
    // features-in mode (AV-HuBERT video branch): the input is a (B, T, conv_dim[0]) feature tensor, the path starts at
    // the feature projection
    if (c.conv_dim[0] < 8 || c.conv_dim[0] % 8) { set_error("features-in mode: conv_dim[0] (the feature width) must be a multiple of 8"); return SVT_ERR_INVALID; }
    if (c.normalize_wav) { set_error("features-in mode: normalize_wav does not apply"); return SVT_ERR_INVALID; }
  } else if (c.conv_kernel[0] != 10) { set_error("conv layer 0 must have kernel 10 (wav2vec2/HuBERT geometry)"); return SVT_ERR_INVALID; }
  if (c.num_conv_layers > 0 && (c.conv_stride[0] > 5 || c.conv_stride[0] < 1)) { set_error("conv layer 0 stride must be 1..5"); return SVT_ERR_INVALID; }
  for (int i = 0; i < c.num_conv_layers; ++i) {
    if (c.conv_dim[i] % 8 || c.conv_dim[i] < 8) { set_error("conv_dim must be a multiple of 8"); return SVT_ERR_INVALID; }
    if (c.conv_kernel[i] < 1 || c.conv_stride[i] < 1) { set_error("bad conv geometry"); return SVT_ERR_INVALID; }
  }
  if (c.num_conv_layers > 0 && c.conv_dim[0] > 512) { set_error("conv_dim[0] > 512 unsupported"); return SVT_ERR_INVALID; }
  if (c.hidden_size < 8 || c.num_heads < 1 || c.pos_conv_groups < 1 || c.intermediate_size < 8 || c.num_layers < 0 || c.pos_conv_kernel < 1) {
    set_error("hidden_size / num_heads / pos_conv_groups / intermediate_size / num_layers / pos_conv_kernel out of range"); return SVT_ERR_INVALID; }
  if (c.hidden_size % c.num_heads) { set_error("hidden_size % num_heads != 0"); return SVT_ERR_INVALID; }
  const int dh = c.hidden_size / c.num_heads;
  if (dh % 8) { set_error("head_dim must be a multiple of 8"); return SVT_ERR_INVALID; }
  if (c.hidden_size % c.pos_conv_groups || (c.hidden_size / c.pos_conv_groups) % 8) { set_error("hidden_size/pos_conv_groups must be a multiple of 8"); return SVT_ERR_INVALID; }
  if (c.intermediate_size % 8 || c.hidden_size % 8) { set_error("sizes must be multiples of 8"); return SVT_ERR_INVALID; }
  if (c.feat_extract_norm != SVT_NORM_GROUP && c.feat_extract_norm != SVT_NORM_LAYER) { set_error("feat_extract_norm"); return SVT_ERR_INVALID; }
  if (!valid_precision(c.precision)) { set_error("precision"); return SVT_ERR_INVALID; }
  if (c.pos_conv_depth < 1 || c.pos_conv_depth > 16) { set_error("pos_conv_depth must be 1..16"); return SVT_ERR_INVALID; }
  if (c.pos_conv_batch_norm && c.pos_conv_depth != 1) { set_error("pos_conv_batch_norm applies to the single positional conv only"); return SVT_ERR_INVALID; }
  if (c.rel_pos_buckets < 0 || c.rel_pos_buckets % 4 || (c.rel_pos_buckets > 0 && c.rel_pos_max_distance <= c.rel_pos_buckets / 4)) {
    set_error("rel_pos_buckets must be a multiple of 4 and rel_pos_max_distance > rel_pos_buckets / 4"); return SVT_ERR_INVALID; }
  return SVT_OK;
}

// ---- re-layouts and folds of the finalize step (host.h) ----

std::vector<float> tap_major(const float* w, int Co, int Ci, int k) {
  std::vector<float> wt((size_t)Co * k * Ci);
  for (int o = 0; o < Co; ++o)
    for (int ci = 0; ci < Ci; ++ci)
      for (int j = 0; j < k; ++j) wt[((size_t)o * k + j) * Ci + ci] = w[((size_t)o * Ci + ci) * k + j];
  return wt;
}

std::vector<float> tap_minor_slabs(const float* wt, int Co, int Ci, int k) {
  std::vector<float> wp((size_t)Co * k * Ci);
  const int nb = Ci / 64;
  for (int o = 0; o < Co; ++o)
    for (int cb = 0; cb < nb; ++cb)
      for (int j = 0; j < k; ++j)
        std::copy_n(&wt[((size_t)o * k + j) * Ci + (size_t)cb * 64], 64, &wp[((size_t)o * k * nb + (size_t)cb * k + j) * 64]);
  return wp;
}

std::vector<float> weight_norm_fold(const float* g, const float* v, size_t n, int kp) {
  std::vector<double> nrm(kp, 0.0);
  for (size_t i = 0; i < n; ++i) nrm[i % kp] += (double)v[i] * (double)v[i];
  for (int j = 0; j < kp; ++j) nrm[j] = std::sqrt(nrm[j]);
  std::vector<float> w(n);
  for (size_t i = 0; i < n; ++i) w[i] = (float)((double)g[i % kp] * (double)v[i] / nrm[i % kp]);
  return w;
}

void batch_norm_fold(const float* weight, const float* bias, const float* mean, const float* var, int C, std::vector<float>* scale,
                     std::vector<float>* shift) {
  scale->resize(C); shift->resize(C);
  for (int c = 0; c < C; ++c) {
    const double sc = (double)weight[c] / std::sqrt((double)var[c] + 1e-5);
    (*scale)[c] = (float)sc;
    (*shift)[c] = (float)((double)bias[c] - (double)mean[c] * sc);
  }
}

void gate_rowsum_fold(const float* w, const float* b, int dh, std::vector<float>* wab, std::vector<float>* bab) {
  wab->assign((size_t)2 * dh, 0.f); bab->assign(2, 0.f);
  for (int j = 0; j < 8; ++j) {
    for (int d = 0; d < dh; ++d) (*wab)[(size_t)(j / 4) * dh + d] += w[(size_t)j * dh + d];
    (*bab)[j / 4] += b[j];
  }
}

void posconv_multiframe(const float* w, const float* bias, int G, int cg, int kp, int Pf, std::vector<float>* wP, std::vector<float>* bP) {
  const size_t Np = (size_t)Pf * cg, Kp = (size_t)(kp + Pf - 1) * cg;
  wP->assign((size_t)G * Np * Kp, 0.f); bP->resize((size_t)G * Np);
  for (int g = 0; g < G; ++g)
    for (int j = 0; j < Pf; ++j)
      for (int co = 0; co < cg; ++co) {
        const int o = g * cg + co;
        (*bP)[(size_t)g * Np + (size_t)j * cg + co] = bias[o];
        float* row = wP->data() + ((size_t)g * Np + (size_t)j * cg + co) * Kp;
        for (int k = 0; k < kp; ++k)
          for (int ci = 0; ci < cg; ++ci) row[(size_t)(k + j) * cg + ci] = w[((size_t)o * cg + ci) * kp + k];
      }
}

// First match wins.  The fused kernels exist for head sizes 64 / 128; the 16-bit one has WavLM's bias for head
// size 64 with the (2T-1)-entry table of a head in LDS; the split one reads planes cut from one packed projection and has neither bias
// nor mask; a mask without the opt-in takes the materialised scores for every geometry.
AttnPlan plan_attention(const AttnGeom& g) {
  const bool dh_ok = g.dh == 64 || g.dh == 128;
  auto pad = [&](int a) { return (int)((g.T + a - 1) / a * a); };
  AttnPlan p;
  if (g.gp >= 2 && !g.drop && !g.bias && dh_ok && g.packed_kv) {
    p.path = ATTN_FUSED_X3; p.Tp = pad(8); p.planes_qkv = true; p.planes_q = !g.q_packed;
  } else if (!g.drop && g.prec == 1 && dh_ok && (!g.bias || (g.dh == 64 && 2 * g.T - 1 <= 8192))) {
    p.path = ATTN_FUSED16; p.Tp = pad(64);
  } else if (g.drop && g.fused_drop && !g.bias && g.prec == 1 && dh_ok) {
    p.path = ATTN_FUSED16_DROP; p.Tp = pad(64);
  } else {
    p.path = ATTN_SCORES; p.Tp = pad(8); p.scores = p.vt = true;
  }
  return p;
}

AttnPlan attn_workspace_plan(AttnPlan p, bool scores_with_planes) {
  p.vt = true;
  if (scores_with_planes && p.path == ATTN_FUSED_X3) p.scores = true;
  return p;
}

}  // namespace svt

using namespace svt;

// ---- RIFF/WAVE headers (svt_wav_parse, svt_wav_header): little-endian fields read and written byte by byte, so neither the host's byte
// order nor the alignment of the caller's buffer matters ----
namespace {
inline uint32_t rd16(const unsigned char* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
inline uint32_t rd32(const unsigned char* p) { return rd16(p) | (rd16(p + 2) << 16); }
inline void wr16(unsigned char* p, uint32_t v) { p[0] = (unsigned char)(v & 0xff); p[1] = (unsigned char)((v >> 8) & 0xff); }
inline void wr32(unsigned char* p, uint32_t v) { wr16(p, v & 0xffff); wr16(p + 2, v >> 16); }
inline bool tag_is(const unsigned char* p, const char* t) { return p[0] == (unsigned char)t[0] && p[1] == (unsigned char)t[1] && p[2] == (unsigned char)t[2] && p[3] == (unsigned char)t[3]; }
int wav_refuse(const char* why) { set_error(std::string("svt_wav_parse: ") + why); return SVT_ERR_INVALID; }
// bytes 2..15 of KSDATAFORMAT_SUBTYPE_PCM / _IEEE_FLOAT (bytes 0..1 are the format tag)
const unsigned char kSubFormatTail[14] = {0x00, 0x00, 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xAA, 0x00, 0x38, 0x9B, 0x71};

// 0 or the svt_pcm_format of a format tag at a sample size
int pcm_format_of(uint32_t tag, uint32_t bits) {
  if (tag == 1) return bits == 8 ? SVT_PCM_U8 : bits == 16 ? SVT_PCM_S16 : bits == 24 ? SVT_PCM_S24 : bits == 32 ? SVT_PCM_S32 : 0;
  if (tag == 3) return bits == 32 ? SVT_PCM_F32 : bits == 64 ? SVT_PCM_F64 : 0;
  return 0;
}
}  // namespace

extern "C" {

const char* svt_last_error(void) { return svt::g_err.c_str(); }

int svt_wav_parse(const void* head_host, int64_t head_bytes, int64_t file_bytes, svt_wav_info* out, int64_t* need_bytes) {
  const unsigned char* h = (const unsigned char*)head_host;
  if (!out || head_bytes < 0 || file_bytes < head_bytes || (!h && head_bytes > 0)) return wav_refuse("bad argument");
  // the prefix ends before byte `upto`: ask for it if the file has it, otherwise the file is cut short
#define SVT_WAV_WANT(upto, what)                                                            \
  do {                                                                                      \
    if ((upto) > file_bytes) return wav_refuse(what);                                       \
    if ((upto) > head_bytes) {                                                              \
      if (!need_bytes) return wav_refuse("need_bytes is null and the prefix is too short"); \
      *need_bytes = (upto);                                                                 \
      return SVT_WAV_NEED_MORE;                                                             \
    }                                                                                       \
  } while (0)
  SVT_WAV_WANT(12, "the file is shorter than a RIFF header");
  if (tag_is(h, "RIFX")) return wav_refuse("RIFX (big-endian) files are not supported");
  if (tag_is(h, "RF64") || tag_is(h, "BW64")) return wav_refuse("RF64 files are not supported");
  if (tag_is(h, "riff")) return wav_refuse("W64 files are not supported");
  if (!tag_is(h, "RIFF") || !tag_is(h + 8, "WAVE")) return wav_refuse("not a RIFF/WAVE file");
  svt_wav_info w = {};
  bool have_fmt = false;
  int64_t pos = 12;
  for (;;) {
    SVT_WAV_WANT(pos + 8, "the file ends before its data chunk");
    const unsigned char* c = h + pos;
    const int64_t size = (int64_t)rd32(c + 4);
    if (tag_is(c, "data")) {
      if (!have_fmt) return wav_refuse("data chunk before fmt chunk");
      w.data_offset = pos + 8;
      const int64_t avail = file_bytes - w.data_offset;
      const int64_t bytes = (size == 0 || size == 0xFFFFFFFFll || size > avail) ? avail : size;
      w.frames = bytes / w.block_align;
      *out = w;
      return SVT_OK;
    }
    if (tag_is(c, "fmt ")) {
      if (size < 16) return wav_refuse("fmt chunk shorter than 16 bytes");
      if (pos + 8 + size > file_bytes) return wav_refuse("the file ends inside its fmt chunk");
      SVT_WAV_WANT(pos + 8 + (size < 40 ? size : 40), "the file ends inside its fmt chunk");
      const unsigned char* f = c + 8;
      uint32_t tag = rd16(f);
      const uint32_t channels = rd16(f + 2), rate = rd32(f + 4), align = rd16(f + 12), bits = rd16(f + 14);
      if (tag == 0xFFFE) {
        if (size < 40 || rd16(f + 16) < 22) return wav_refuse("WAVE_FORMAT_EXTENSIBLE with a short fmt chunk");
        if (memcmp(f + 26, kSubFormatTail, sizeof(kSubFormatTail)) != 0) return wav_refuse("unknown sub-format GUID");
        if (rd16(f + 18) != bits) return wav_refuse("valid bits differ from the container size");
        tag = rd16(f + 24);
        if (tag != 1 && tag != 3) return wav_refuse("unsupported sub-format (PCM and IEEE float only)");
      }
      if (tag == 6 || tag == 7) return wav_refuse("A-law / mu-law files are not supported");
      if (tag == 2 || tag == 0x11) return wav_refuse("ADPCM files are not supported");
      if (tag != 1 && tag != 3) return wav_refuse("unsupported format tag (PCM and IEEE float only)");
      const int fmt = pcm_format_of(tag, bits);
      if (!fmt) return wav_refuse("unsupported sample size");
      if (channels < 1 || channels > 8) return wav_refuse("channels must be in 1..8");
      if (rate < 1 || rate > 0x7FFFFFFFu) return wav_refuse("bad sample rate");
      if (align != channels * bits / 8) return wav_refuse("block_align is not channels * bits / 8");
      w.format = fmt; w.channels = (int32_t)channels; w.sample_rate = (int32_t)rate; w.bits_per_sample = (int32_t)bits;
      w.block_align = (int32_t)align;
      have_fmt = true;
    }
    pos += 8 + size + (size & 1);
    if (pos > file_bytes) return wav_refuse("the file ends inside a chunk");
  }
#undef SVT_WAV_WANT
}

int svt_wav_header(int32_t format, int32_t channels, int32_t sample_rate, int64_t frames, void* out_host, int64_t capacity,
                   int64_t* header_bytes) {
  if (!out_host || !header_bytes) { set_error("svt_wav_header: null argument"); return SVT_ERR_INVALID; }
  if (format != SVT_PCM_S16 && format != SVT_PCM_F32) { set_error("svt_wav_header: only SVT_PCM_S16 and SVT_PCM_F32 are written"); return SVT_ERR_INVALID; }
  if (channels < 1 || channels > 8 || sample_rate < 1 || frames < 0) { set_error("svt_wav_header: bad channels, rate or frames"); return SVT_ERR_INVALID; }
  const bool flt = format == SVT_PCM_F32;
  const int64_t hb = flt ? 58 : 44, align = (int64_t)channels * (flt ? 4 : 2);
  if (capacity < hb) { set_error("svt_wav_header: capacity below the header's size"); return SVT_ERR_INVALID; }
  if (frames > (0xFFFFFFFFll - hb) / align) { set_error("svt_wav_header: more than 4 GiB - 1 - header of data"); return SVT_ERR_INVALID; }
  const int64_t data = frames * align;
  unsigned char* p = (unsigned char*)out_host;
  memcpy(p, "RIFF", 4); wr32(p + 4, (uint32_t)(hb - 8 + data)); memcpy(p + 8, "WAVEfmt ", 8);
  wr32(p + 16, flt ? 18 : 16);
  wr16(p + 20, flt ? 3 : 1); wr16(p + 22, (uint32_t)channels); wr32(p + 24, (uint32_t)sample_rate);
  wr32(p + 28, (uint32_t)((int64_t)sample_rate * align)); wr16(p + 32, (uint32_t)align); wr16(p + 34, flt ? 32 : 16);
  unsigned char* q = p + 36;
  if (flt) {
    wr16(q, 0);   // cbSize
    memcpy(q + 2, "fact", 4); wr32(q + 6, 4); wr32(q + 10, (uint32_t)frames);
    q += 14;
  }
  memcpy(q, "data", 4); wr32(q + 4, (uint32_t)data);
  *header_bytes = hb;
  return SVT_OK;
}

// frame2note (reference MIR_ST500/utils.py:82-149) over a batch of decoded frame sequences, on the HOST (no device call).
// Same scan as the reference's loop: float32 comparisons against the thresholds, onset = above threshold AND equal to the
// maximum of onset[i-3 : min(i+4, N-1)] (the last frame is never inside a window), times = frame_size * i in double.
// The pitch of a note is the mode of its bag; where the top count is tied the reference's answer depends on CPython's set
// iteration order, so the note is returned with pitch = -1 and its frame range [lo, hi) and the caller resolves it.
int svt_frames_to_notes(const svt_frame* frames, int32_t batch, int64_t frames_per_clip, const int64_t* n_frames,
                        float onset_thres, float offset_thres, double frame_size, int32_t n_octave, int32_t n_class,
                        double* t_on, double* t_off, int32_t* pitch, int32_t* lo, int32_t* hi, int64_t capacity_per_clip,
                        int64_t* n_notes) {
  if (!frames || !t_on || !t_off || !pitch || !lo || !hi || !n_notes || batch < 0 || frames_per_clip < 0) {
    set_error("svt_frames_to_notes: bad argument"); return SVT_ERR_INVALID; }
  if (n_octave < 1 || n_class < 1 || (long)n_octave * n_class + n_class > 4096) { set_error("svt_frames_to_notes: bad class counts"); return SVT_ERR_INVALID; }
  std::vector<int> counts((size_t)n_octave * n_class + n_class + 1);
  for (int32_t b = 0; b < batch; ++b) {
    const svt_frame* f = frames + (int64_t)b * frames_per_clip;
    const int64_t n = n_frames ? n_frames[b] : frames_per_clip;
    if (n < 0 || n > frames_per_clip) { set_error("svt_frames_to_notes: n_frames out of range"); return SVT_ERR_INVALID; }
    int64_t k = 0;
    const int64_t base = (int64_t)b * capacity_per_clip;
    bool open = false;
    int64_t on_i = 0, bag_n = 0;
    auto emit = [&](int64_t close_frame, int64_t hi_frame) -> int {   // the open note [on_i, hi_frame) closes at time frame_size * close_frame
      if (k >= capacity_per_clip) { set_error("svt_frames_to_notes: more notes than capacity_per_clip"); return SVT_ERR_INVALID; }
      int top = 0, arg = 0, ties = 0;
      for (size_t v = 0; v < counts.size(); ++v) {
        if (counts[v] > top) { top = counts[v]; arg = (int)v; ties = 1; }
        else if (counts[v] == top && top > 0) ++ties;
      }
      t_on[base + k] = frame_size * (double)on_i;
      t_off[base + k] = frame_size * (double)close_frame;
      pitch[base + k] = ties > 1 ? -1 : arg + 36;
      lo[base + k] = (int32_t)on_i;
      hi[base + k] = (int32_t)hi_frame;
      ++k;
      return 0;
    };
    for (int64_t i = 0; i < n; ++i) {
      const float p_on = f[i].p_on;
      bool is_on = false;
      if (p_on >= onset_thres) {
        const int64_t w0 = i - 3 > 0 ? i - 3 : 0, w1 = i + 4 < n - 1 ? i + 4 : n - 1;
        if (w1 <= w0) { set_error("frame2note: max() of an empty onset window (a one-frame sequence above the onset threshold), as in the reference"); return SVT_ERR_INVALID; }
        float m = f[w0].p_on;
        for (int64_t j = w0 + 1; j < w1; ++j) m = f[j].p_on > m ? f[j].p_on : m;
        is_on = p_on == m;
      }
      if (is_on) {
        if (open && bag_n) { if (int r = emit(i, i)) return r; }
        open = true; on_i = i; bag_n = 0;
        std::fill(counts.begin(), counts.end(), 0);
      } else if (f[i].p_off >= offset_thres) {
        if (open) {
          if (bag_n) { if (int r = emit(i, i)) return r; }
          open = false; bag_n = 0;
        }
      }
      if (open && f[i].octave != n_octave && f[i].pitch_class != n_class) {
        const long v = (long)f[i].octave * n_class + f[i].pitch_class;
        if (v < 0 || v >= (long)counts.size()) { set_error("svt_frames_to_notes: frame class out of range"); return SVT_ERR_INVALID; }
        ++counts[v];
        ++bag_n;
      }
    }
    if (open && bag_n) { if (int r = emit(n - 1, n)) return r; }
    n_notes[b] = k;
  }
  return SVT_OK;
}

}  // extern "C"
