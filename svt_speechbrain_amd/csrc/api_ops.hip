// C ABI of the small ops around the encoder: the frame head and its decode, CTC greedy decoding, Fbank with its deltas and context
// window, the validation losses and softmax, and the linear-probe training step (objective gradient, head backward, clipped Adadelta).
// Host code only.
#include "../../include/svt_mi355.h"
#include "api.h"
#include "common.h"
#include "host.h"

#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

using namespace svt;

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

// ---- noise mixing at several SNRs (noise_mix.hip) ----
int64_t svt_noise_mix_workspace_bytes(int64_t n_samples, int32_t n_snr) {
  if (n_samples < 1 || n_snr < 1 || n_snr > 8) return -1;
  return (int64_t)noise_mix_scratch_bytes();
}

int svt_noise_mix(const float* clean, const float* noise, int64_t n_samples, const float* snr_db, int32_t n_snr, float* out,
                  int64_t ld_out, double* amps_out, void* workspace, int64_t workspace_bytes, int device, void* stream) {
  if (n_samples < 1) { set_error("svt_noise_mix: empty track"); return SVT_ERR_INVALID; }
  if (n_snr < 1 || n_snr > 8) { set_error("svt_noise_mix: n_snr must be in 1..8"); return SVT_ERR_INVALID; }
  if (!clean || !noise || !snr_db || (!out && !amps_out) || !workspace) { set_error("svt_noise_mix: null argument"); return SVT_ERR_INVALID; }
  if (ld_out < n_samples) { set_error("svt_noise_mix: ld_out < n_samples"); return SVT_ERR_INVALID; }
  if (((uintptr_t)clean | (uintptr_t)noise | (uintptr_t)out) & 3) { set_error("svt_noise_mix: tracks must be 4-byte aligned"); return SVT_ERR_INVALID; }
  if (((uintptr_t)workspace | (uintptr_t)amps_out) & 7) { set_error("svt_noise_mix: workspace and amps_out must be 8-byte aligned"); return SVT_ERR_INVALID; }
  if (workspace_bytes < svt_noise_mix_workspace_bytes(n_samples, n_snr)) { set_error("svt_noise_mix: workspace too small"); return SVT_ERR_WORKSPACE; }
  double f[8];
  for (int i = 0; i < n_snr; ++i) {
    if (!std::isfinite(snr_db[i])) { set_error("svt_noise_mix: non-finite SNR"); return SVT_ERR_INVALID; }
    f[i] = 1.0 / (std::pow(10.0, (double)snr_db[i] / 20.0) + 1.0);   // dB_to_amplitude in Python floats (signal_processing.py:354-369)
  }
  if (int r = check_device(device)) return r;
  if (launch_noise_mix(clean, noise, n_samples, f, n_snr, out, ld_out, amps_out, workspace, (hipStream_t)stream)) return SVT_ERR_HIP;
  return SVT_OK;
}

// ---- polyphase resampling with an optional stereo downmix (resample.hip) ----
namespace {
int64_t gcd64(int64_t a, int64_t b) { while (b) { const int64_t t = a % b; a = b; b = t; } return a; }
// Resample._output_samples (LinearResample::GetNumOutputSamples): time in ticks of 1 / lcm(orig, new); an input period is new / g
// ticks, an output period orig / g; the outputs at ticks in [0, n_in * new / g)
int64_t tick_rule(int64_t n_in, int64_t orig, int64_t fresh) {
  const int64_t g = gcd64(orig, fresh), per_in = fresh / g, per_out = orig / g;
  const int64_t interval = n_in * per_in;
  if (interval <= 0) return 0;
  int64_t last = interval / per_out;
  if (last * per_out == interval) --last;
  return last + 1;
}
}  // namespace

int64_t svt_resample_output_samples(int64_t n_in, int32_t orig_freq, int32_t new_freq) {
  if (n_in < 0 || orig_freq < 1 || new_freq < 1) return -1;
  return tick_rule(n_in, orig_freq, new_freq);
}

int svt_resample(const float* in, int32_t rows, int64_t n_in, int64_t ld_in, const float* weights, const int32_t* first, int32_t P, int32_t W,
                 int32_t S, float* out, int64_t n_out, int64_t ld_out, int32_t downmix, int device, void* stream) {
  if (rows < 1 || n_in < 1) { set_error("svt_resample: empty input"); return SVT_ERR_INVALID; }
  if (P < 1 || W < 1 || S < 1) { set_error("svt_resample: P, W and S must be positive"); return SVT_ERR_INVALID; }
  if (P == S) { set_error("svt_resample: P == S, the rates are equal and there is nothing to resample"); return SVT_ERR_INVALID; }
  if (resample_units_per_tile(P, W, S, downmix != 0) < 1) { set_error("svt_resample: the filter table does not fit SVT_RESAMPLE_LDS_BYTES of LDS"); return SVT_ERR_INVALID; }
  if (downmix && (rows & 1)) { set_error("svt_resample: downmix takes channel pairs, rows must be even"); return SVT_ERR_INVALID; }
  if (ld_in < n_in) { set_error("svt_resample: ld_in < n_in"); return SVT_ERR_INVALID; }
  if (ld_out < n_out) { set_error("svt_resample: ld_out < n_out"); return SVT_ERR_INVALID; }
  if (!in || !weights || !first || !out) { set_error("svt_resample: null argument"); return SVT_ERR_INVALID; }
  if (((uintptr_t)in | (uintptr_t)weights | (uintptr_t)first | (uintptr_t)out) & 3) { set_error("svt_resample: pointers must be 4-byte aligned"); return SVT_ERR_INVALID; }
  if (n_out != tick_rule(n_in, S, P)) { set_error("svt_resample: n_out is not what svt_resample_output_samples gives for n_in"); return SVT_ERR_INVALID; }
  if (int r = check_device(device)) return r;
  const int rows_out = downmix ? rows / 2 : rows;
  if (launch_resample(in, rows_out, n_in, ld_in, weights, first, P, W, S, out, n_out, ld_out, downmix != 0, (hipStream_t)stream)) return SVT_ERR_HIP;
  return SVT_OK;
}

// ---- frequency and chunk dropping of a waveform batch (drop_freq_chunk.hip) ----
int svt_drop_freq_chunk(const float* in, int32_t rows, int64_t n, int64_t ld_in, const float* filter, int32_t taps, const int64_t* chunks,
                        int32_t max_chunks, float* out, int64_t ld_out, int device, void* stream) {
  if (rows < 1 || n < 1) { set_error("svt_drop_freq_chunk: empty input"); return SVT_ERR_INVALID; }
  if ((filter != nullptr) != (taps != 0)) { set_error("svt_drop_freq_chunk: filter_dev and taps go together (NULL / 0: no filtering)"); return SVT_ERR_INVALID; }
  if (taps && (taps < 1 || taps > SVT_DROP_MAX_TAPS || !(taps & 1))) { set_error("svt_drop_freq_chunk: taps must be odd and in 1..SVT_DROP_MAX_TAPS"); return SVT_ERR_INVALID; }
  if (max_chunks < 0) { set_error("svt_drop_freq_chunk: max_chunks < 0"); return SVT_ERR_INVALID; }
  if ((chunks != nullptr) != (max_chunks != 0)) { set_error("svt_drop_freq_chunk: chunks_dev and max_chunks go together (NULL / 0: no chunks)"); return SVT_ERR_INVALID; }
  if (ld_in < n) { set_error("svt_drop_freq_chunk: ld_in < n"); return SVT_ERR_INVALID; }
  if (ld_out < n) { set_error("svt_drop_freq_chunk: ld_out < n"); return SVT_ERR_INVALID; }
  if (!in || !out) { set_error("svt_drop_freq_chunk: null argument"); return SVT_ERR_INVALID; }
  if (((uintptr_t)in | (uintptr_t)filter | (uintptr_t)out) & 3) { set_error("svt_drop_freq_chunk: in_dev, filter_dev and out_dev must be 4-byte aligned"); return SVT_ERR_INVALID; }
  if ((uintptr_t)chunks & 7) { set_error("svt_drop_freq_chunk: chunks_dev must be 8-byte aligned"); return SVT_ERR_INVALID; }
  const int64_t most = (INT64_MAX / 8 - n) / rows;                  // the byte extents below stay inside 63 bits
  if (ld_in > most || ld_out > most) { set_error("svt_drop_freq_chunk: a row pitch too large to address"); return SVT_ERR_INVALID; }
  const uintptr_t in_lo = (uintptr_t)in, in_hi = in_lo + 4 * (uintptr_t)((rows - 1) * ld_in + n);
  const uintptr_t out_lo = (uintptr_t)out, out_hi = out_lo + 4 * (uintptr_t)((rows - 1) * ld_out + n);
  if (in_lo < out_hi && out_lo < in_hi) { set_error("svt_drop_freq_chunk: in_dev and out_dev overlap (the filter's halo makes in-place operation wrong)"); return SVT_ERR_INVALID; }
  if (int r = check_device(device)) return r;
  if (launch_drop_freq_chunk(in, rows, n, ld_in, filter, taps, chunks, max_chunks, out, ld_out, (hipStream_t)stream)) return SVT_ERR_HIP;
  return SVT_OK;
}

// ---- SpecAugment masks on a (B, T, D) fp32 tensor, in place (spec_augment.hip) ----
int svt_spec_augment(float* h, int32_t B, int32_t T, int32_t D, int64_t ld, const uint8_t* time_mask, const uint8_t* feature_mask,
                     const float* embed, int device, void* stream) {
  if (B < 1 || T < 1 || D < 1) { set_error("svt_spec_augment: empty tensor"); return SVT_ERR_INVALID; }
  if (D % 4) { set_error("svt_spec_augment: D must be a multiple of 4 (16-byte accesses)"); return SVT_ERR_INVALID; }
  if (ld % 4) { set_error("svt_spec_augment: ld must be a multiple of 4 (16-byte accesses)"); return SVT_ERR_INVALID; }
  if (ld < D) { set_error("svt_spec_augment: ld < D"); return SVT_ERR_INVALID; }
  if (!h) { set_error("svt_spec_augment: null argument"); return SVT_ERR_INVALID; }
  if (time_mask && !embed) { set_error("svt_spec_augment: a time mask needs embed_dev (masked_spec_embed)"); return SVT_ERR_INVALID; }
  if (((uintptr_t)h | (uintptr_t)embed) & 15) { set_error("svt_spec_augment: h_dev and embed_dev must be 16-byte aligned"); return SVT_ERR_INVALID; }
  if ((uintptr_t)feature_mask & 3) { set_error("svt_spec_augment: feature_mask_dev must be 4-byte aligned"); return SVT_ERR_INVALID; }
  if (ld > (INT64_MAX / 4 - D) / ((int64_t)B * T)) { set_error("svt_spec_augment: a row pitch too large to address"); return SVT_ERR_INVALID; }
  if (int r = check_device(device)) return r;
  if (launch_spec_augment(h, B, T, D, ld, time_mask, feature_mask, embed, (hipStream_t)stream)) return SVT_ERR_HIP;
  return SVT_OK;
}

// ---- PCM <-> fp32 on the bytes of a wav file (pcm.hip); the header's parser and writer are host.cpp's ----
int svt_pcm_decode(const void* src, int32_t format, int32_t channels, int64_t frames, float* out, int64_t ld_out, int32_t downmix,
                   int device, void* stream) {
  if (format < SVT_PCM_U8 || format > SVT_PCM_F64) { set_error("svt_pcm_decode: unknown format"); return SVT_ERR_INVALID; }
  if (channels < 1 || channels > 8) { set_error("svt_pcm_decode: channels must be in 1..8"); return SVT_ERR_INVALID; }
  if (frames < 1) { set_error("svt_pcm_decode: frames < 1"); return SVT_ERR_INVALID; }
  if (ld_out < frames) { set_error("svt_pcm_decode: ld_out < frames"); return SVT_ERR_INVALID; }
  if (downmix && channels != 2) { set_error("svt_pcm_decode: downmix takes 2 channels"); return SVT_ERR_INVALID; }
  if (!src || !out) { set_error("svt_pcm_decode: null argument"); return SVT_ERR_INVALID; }
  if ((uintptr_t)out & 3) { set_error("svt_pcm_decode: out_dev must be 4-byte aligned"); return SVT_ERR_INVALID; }
  if (int r = check_device(device)) return r;
  if (launch_pcm_decode(src, format, channels, frames, out, ld_out, downmix != 0, (hipStream_t)stream)) return SVT_ERR_HIP;
  return SVT_OK;
}

int svt_pcm_encode(const float* in, int64_t ld_in, int32_t channels, int64_t frames, int32_t format, void* dst, int device, void* stream) {
  if (format != SVT_PCM_S16 && format != SVT_PCM_F32) { set_error("svt_pcm_encode: only SVT_PCM_S16 and SVT_PCM_F32 are written"); return SVT_ERR_INVALID; }
  if (channels < 1 || channels > 8) { set_error("svt_pcm_encode: channels must be in 1..8"); return SVT_ERR_INVALID; }
  if (frames < 1) { set_error("svt_pcm_encode: frames < 1"); return SVT_ERR_INVALID; }
  if (ld_in < frames) { set_error("svt_pcm_encode: ld_in < frames"); return SVT_ERR_INVALID; }
  if (!in || !dst) { set_error("svt_pcm_encode: null argument"); return SVT_ERR_INVALID; }
  if ((uintptr_t)in & 3) { set_error("svt_pcm_encode: in_dev must be 4-byte aligned"); return SVT_ERR_INVALID; }
  if (int r = check_device(device)) return r;
  if (launch_pcm_encode(in, ld_in, channels, frames, format, dst, (hipStream_t)stream)) return SVT_ERR_HIP;
  return SVT_OK;
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
// the frames predictions and targets keep, or -1 after set_error: same condition and wording as speechbrain.nnet.losses.truncate
// (losses.py:608-613)
static int64_t truncated_frames(int64_t t_pred, int64_t t_tgt, int32_t allowed) {
  const int64_t diff = t_pred - t_tgt;
  if ((diff < 0 ? -diff : diff) > allowed) {
    set_error("Predictions and targets should be same length, but got " + std::to_string(t_pred) + " and " +
              std::to_string(t_tgt) + " respectively.");
    return -1;
  }
  return diff < 0 ? t_pred : t_tgt;
}

static int loss_common_checks(const char* who, int64_t batch, int64_t t_pred, int64_t t_tgt, int32_t allowed, int32_t reduction,
                              size_t ws_bytes, int64_t* T) {
  if (batch < 1 || t_pred < 1 || t_tgt < 1) { set_error(std::string(who) + ": empty input"); return SVT_ERR_INVALID; }
  if (reduction < 0 || reduction > 3) { set_error(std::string(who) + ": reduction must be 0 (mean), 1 (batchmean), 2 (batch) or 3 (none)"); return SVT_ERR_INVALID; }
  *T = truncated_frames(t_pred, t_tgt, allowed);
  if (*T < 0) return SVT_ERR_INVALID;
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
  const int64_t T = truncated_frames(t_pred, t_tgt, allowed_len_diff);
  if (T < 0) return SVT_ERR_INVALID;
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

int svt_clip_adam_step(int32_t n_tensors, float* const* params, float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                       float* const* max_exp_avg_sq, const int64_t* numels, const float* step_size, const float* bc2_sqrt, double lr,
                       double beta1, double beta2, double eps, double weight_decay, int32_t flags, float max_norm, float* total_norm,
                       void* workspace, size_t* workspace_bytes, int device, void* stream) {
  const char* who = "svt_clip_adam_step";
  if (n_tensors < 1) { set_error(std::string(who) + ": n_tensors must be at least 1"); return SVT_ERR_INVALID; }
  if (!numels) { set_error(std::string(who) + ": null argument"); return SVT_ERR_INVALID; }
  for (int i = 0; i < n_tensors; ++i)
    if (numels[i] < 0) { set_error(std::string(who) + ": negative numel"); return SVT_ERR_INVALID; }
  if (adam_chunks(numels, n_tensors) > 2147483647LL) { set_error(std::string(who) + ": more than 2^31 - 1 chunks of 4096 elements"); return SVT_ERR_INVALID; }
  bool query = false;
  if (int r = ws_query(who, workspace, workspace_bytes, adam_workspace_bytes(numels, n_tensors), &query)) return r;
  if (query) return SVT_OK;
  const bool ams = (flags & SVT_ADAM_AMSGRAD) != 0;
  if (flags & ~(SVT_ADAM_MAXIMIZE | SVT_ADAM_AMSGRAD | SVT_ADAM_DECOUPLED)) { set_error(std::string(who) + ": unknown flag"); return SVT_ERR_INVALID; }
  if (!params || !grads || !exp_avg || !exp_avg_sq || !step_size || !bc2_sqrt || (ams && !max_exp_avg_sq)) {
    set_error(std::string(who) + ": null argument"); return SVT_ERR_INVALID;
  }
  if (!ams && max_exp_avg_sq) { set_error(std::string(who) + ": max_exp_avg_sq given without SVT_ADAM_AMSGRAD"); return SVT_ERR_INVALID; }
  uintptr_t bits = (uintptr_t)total_norm;
  for (int i = 0; i < n_tensors; ++i) {
    if (numels[i] == 0) continue;
    if (!params[i] || !grads[i] || !exp_avg[i] || !exp_avg_sq[i] || (ams && !max_exp_avg_sq[i])) {
      set_error(std::string(who) + ": null tensor pointer"); return SVT_ERR_INVALID;
    }
    bits |= (uintptr_t)params[i] | (uintptr_t)grads[i] | (uintptr_t)exp_avg[i] | (uintptr_t)exp_avg_sq[i] | (ams ? (uintptr_t)max_exp_avg_sq[i] : 0);
  }
  if (bits & 3) { set_error(std::string(who) + ": tensors must be 4-byte aligned"); return SVT_ERR_INVALID; }
  if ((uintptr_t)workspace & 15) { set_error(std::string(who) + ": workspace must be 16-byte aligned"); return SVT_ERR_INVALID; }
  if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !(weight_decay >= 0.0) ||
      std::isnan(max_norm)) {
    set_error(std::string(who) + ": lr, eps and weight_decay must be >= 0 and the betas in [0, 1)"); return SVT_ERR_INVALID;
  }
  if (int r = check_device(device)) return r;
  SVT_HIP(hipSetDevice(device));
  // torch forms 1 - beta1, 1 - beta2 and 1 - lr * weight_decay as Python floats, i.e. in double before the fp32 operation
  AdamHyper h{};
  h.w1 = (float)(1.0 - beta1);
  h.one_minus_w1 = 1.f - h.w1;
  h.lerp_far = h.w1 >= 0.5f ? 1 : 0;
  h.beta2 = (float)beta2;
  h.one_minus_beta2 = (float)(1.0 - beta2);
  h.eps = (float)eps;
  h.weight_decay = (float)weight_decay;
  h.decay_mul = (float)(1.0 - lr * weight_decay);
  h.maximize = (flags & SVT_ADAM_MAXIMIZE) ? 1 : 0;
  h.decoupled = (flags & SVT_ADAM_DECOUPLED) ? 1 : 0;
  if (launch_clip_adam(n_tensors, params, grads, exp_avg, exp_avg_sq, ams ? max_exp_avg_sq : nullptr, numels, step_size, bc2_sqrt, h,
                       max_norm, total_norm, workspace, (hipStream_t)stream))
    return SVT_ERR_HIP;
  return SVT_OK;
}

// svt_attention_forward / svt_attention_backward: the checks both share; fills `spec` when p > 0
static int attention_desc_check(const char* who, const svt_attention_desc* d, bool backward, DropSpec* spec) {
  auto refuse = [who](const char* why) { set_error(std::string(who) + ": " + why); return SVT_ERR_INVALID; };
  if (!d) return refuse("null descriptor");
  if (d->struct_size != (int32_t)sizeof(svt_attention_desc)) return refuse("struct_size");
  if (!d->q || !d->k || !d->v || !d->o) return refuse("null argument");
  if (backward && (!d->d_o || !d->dq || !d->dk || !d->dv)) return refuse("null argument");
  if (d->batch < 1 || d->t < 1 || d->heads < 1) return refuse("batch, t and heads must be positive");
  if (d->precision != SVT_PREC_BF16) return refuse("precision must be SVT_PREC_BF16 (the build's 16-bit operand type)");
  if (backward ? d->head_dim != 64 : (d->head_dim != 64 && d->head_dim != 128))
    return refuse(backward ? "head_dim must be 64" : "head_dim must be 64 or 128");
  if (!(d->p >= 0.0 && d->p < 1.0)) return refuse("p must lie in [0, 1)");
  if (d->layer < 0 || d->layer > 0xFFFFFF) return refuse("layer");
  if (d->p > 0.0) *spec = make_drop_spec(d->p, d->seed, d->step, 2, d->layer);
  return SVT_OK;
}

int svt_attention_forward(const svt_attention_desc* d, int device, void* stream) {
  DropSpec spec;
  if (int r = attention_desc_check("svt_attention_forward", d, false, &spec)) return r;
  if (int r = check_device(device)) return r;
  SVT_HIP(hipSetDevice(device));
  const long t = d->t;
  const int rc = d->p > 0.0
      ? launch_flash_attention_dropout(d->q, d->ldq, t * d->ldq, d->k, d->v, d->ldkv, t * d->ldkv, d->o, d->ldo, t * d->ldo, d->batch, d->t,
                                       d->heads, d->head_dim, d->scale, d->e0, spec, (hipStream_t)stream)
      : launch_flash_attention(d->q, d->ldq, t * d->ldq, d->k, d->v, d->ldkv, t * d->ldkv, d->o, d->ldo, t * d->ldo, d->batch, d->t, d->heads,
                               d->head_dim, d->scale, (hipStream_t)stream);
  return rc ? SVT_ERR_INVALID : SVT_OK;
}

int svt_attention_backward(const svt_attention_desc* d, void* workspace, size_t* workspace_bytes, int device, void* stream) {
  const char* who = "svt_attention_backward";
  DropSpec spec;
  if (int r = attention_desc_check(who, d, true, &spec)) return r;
  bool query;
  if (int r = ws_query(who, workspace, workspace_bytes, attention_backward_workspace_bytes(d->batch, d->heads, d->t), &query)) return r;
  if (query) return SVT_OK;
  if (int r = check_device(device)) return r;
  SVT_HIP(hipSetDevice(device));
  AttnBwdArgs a;
  a.prec = 1; a.Q = d->q; a.K = d->k; a.V = d->v; a.O = d->o; a.dO = d->d_o; a.dQ = d->dq; a.dK = d->dk; a.dV = d->dv;
  a.ldq = d->ldq; a.ldkv = d->ldkv; a.ldo = d->ldo; a.lddo = d->lddo; a.lddq = d->lddq; a.lddkv = d->lddkv;
  a.B = d->batch; a.T = d->t; a.H = d->heads; a.dh = d->head_dim; a.scale = d->scale;
  a.drop = d->p > 0.0 ? &spec : nullptr; a.e0 = d->e0; a.ws = workspace;
  return launch_attention_backward(a, (hipStream_t)stream) ? SVT_ERR_INVALID : SVT_OK;
}

}  // extern "C"
