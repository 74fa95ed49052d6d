/*
 * svt_mi355.h — C-ABI of the MI355X-native singing-transcription hot path.
 *
 * This is the drop-in boundary.  The reference is 100 % Python; its "FFI" for this
 * path is the set of torch ops reached from
 *   MIR_ST500/huggingface_interface.py:263-297   (HuggingFaceWav2Vec2.forward / extract_features)
 *   speechbrain/nnet/linear.py:63-76             (Linear.forward, the 20-way frame head)
 *   MIR_ST500/train_audio_ssl.py:41-46,93-100    (logit slicing, sigmoid / argmax per frame)
 *   N20EMv2/audio_visual/fusion.py:192-210       (FusionRCA.forward)
 *   speechbrain/decoders/ctc.py:341-383          (ctc_greedy_decode)
 *   speechbrain/lobes/features.py:126-143        (Fbank.forward)
 * Each entry point below names the interface it replaces.  A maintainer binds them with ctypes
 * (INTEGRATION.md shows the stub); svt_speechbrain_amd/ does exactly that.
 *
 * Conventions
 *   - plain C types only: pointers + sizes, no torch / HIP types in signatures (`stream` is a
 *     hipStream_t passed as void*; NULL = the default stream).
 *   - every *_dev pointer is device memory on the object's device, caller-owned, never mutated when
 *     const.  Host pointers are named *_host.
 *   - all functions return 0 on success or a negative svt_status; svt_last_error() returns a
 *     thread-local text.  Nothing aborts, nothing synchronises the device or allocates inside a
 *     forward call (workspace is caller-supplied), so calls may be captured into a hipGraph.
 *   - one object per device; an object is NOT thread-safe.
 */
#ifndef SVT_MI355_H
#define SVT_MI355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVT_ABI_VERSION 1
#define SVT_MAX_CONV_LAYERS 8

typedef enum {
  SVT_OK = 0,
  SVT_ERR_INVALID = -1,     /* bad argument / config / shape              */
  SVT_ERR_KEY = -2,         /* unknown or missing parameter key           */
  SVT_ERR_STATE = -3,       /* call order (e.g. encode before finalize)   */
  SVT_ERR_WORKSPACE = -4,   /* workspace too small                        */
  SVT_ERR_HIP = -5,         /* HIP runtime error (text in last_error)     */
  SVT_ERR_NO_DEVICE = -6    /* no gfx950 device visible                   */
} svt_status;

/* Operand handling of the dense products (conv 1-6 as implicit GEMM, projections, attention, FFN; HF:254-802):
 *   SVT_PREC_FP32    fp32 operands, exact fp32 MFMA (v_mfma_f32_16x16x4_f32): the parity mode, 157 TFLOP/s peak
 *   SVT_PREC_BF16    bf16 operands and activations, fp32 accumulate: the throughput mode
 *   SVT_PREC_BF16X3  fp32 activations / weights in memory; inside the product kernels every operand is cut into bf16
 *                    (hi, lo) and Ah*Wh + Al*Wh + Ah*Wl is accumulated in fp32 on the bf16 matrix pipe (3 MFMAs of 16
 *                    cycles instead of 8 fp32 MFMAs of 32): ~2^-17 relative operand error, fp32 range
 *   SVT_PREC_FP16X3  the same with fp16 pieces: ~2^-22 relative for operands of magnitude 0.125 and above; below 0.125 the lo piece
 *                    is a subnormal half (the device keeps it: conversion and MFMA are exact on subnormals) and carries an ABSOLUTE
 *                    error of 2^-25 per operand instead (tests/test_gpu_gemm_split_kernels.py).  Operands must stay below 65504 in magnitude,
 *                    which holds for the fp16-trained wav2vec2 / HuBERT / WavLM checkpoints the wrapper loads */
typedef enum { SVT_PREC_FP32 = 0, SVT_PREC_BF16 = 1, SVT_PREC_BF16X3 = 2, SVT_PREC_FP16X3 = 3 } svt_precision;
typedef enum { SVT_NORM_GROUP = 0, SVT_NORM_LAYER = 1 } svt_feat_norm;
typedef enum { SVT_F32 = 0 } svt_dtype;

/* Mirrors the HF Wav2Vec2Config / HubertConfig fields the forward reads
 * (huggingface_interface.py:107-124,169-179) plus the wrapper's two flags (:99-100,130). */
typedef struct svt_encoder_config {
  int32_t struct_size;          /* = sizeof(svt_encoder_config) */
  int32_t hidden_size;
  int32_t num_layers;
  int32_t num_heads;
  int32_t intermediate_size;
  int32_t num_conv_layers;
  int32_t conv_dim[SVT_MAX_CONV_LAYERS];
  int32_t conv_kernel[SVT_MAX_CONV_LAYERS];
  int32_t conv_stride[SVT_MAX_CONV_LAYERS];
  int32_t feat_extract_norm;    /* svt_feat_norm */
  int32_t conv_bias;
  int32_t stable_layer_norm;    /* do_stable_layer_norm */
  int32_t feat_proj_layer_norm;
  int32_t pos_conv_kernel;      /* num_conv_pos_embeddings */
  int32_t pos_conv_groups;      /* num_conv_pos_embedding_groups */
  float layer_norm_eps;
  int32_t normalize_wav;        /* wrapper: F.layer_norm(wav, wav.shape) */
  int32_t output_norm;          /* wrapper: F.layer_norm(out, out.shape) */
  int32_t precision;            /* svt_precision: operand type of the MFMA contractions */
  int32_t pos_conv_depth;       /* 1: one weight-normed positional conv + GELU (wav2vec2 / HuBERT); n > 1: data2vec-audio's stack of
                                 * n plain grouped convs, each followed by LayerNorm(no affine) + GELU */
  int32_t rel_pos_buckets;      /* 0: none; > 0: WavLM's gated relative position bias with this many buckets */
  int32_t rel_pos_max_distance; /* WavLM max_bucket_distance */
  int32_t pos_conv_batch_norm;  /* HuBERT conv_pos_batch_norm (HF modeling_hubert.py HubertPositionalConvEmbedding): eval-mode BatchNorm1d in
                                   front of a plain (not weight-normed) positional conv; keys encoder.pos_conv_embed.batch_norm.* */
} svt_encoder_config;

typedef struct svt_encoder svt_encoder;
typedef struct svt_linear svt_linear;
typedef struct svt_rca svt_rca;

/* one decoded frame: what the reference's per-frame loop appends to song_pred
 * (MIR_ST500/train_audio_ssl.py:95-100) */
typedef struct svt_frame {
  float p_on;
  float p_off;
  int32_t octave;
  int32_t pitch_class;
} svt_frame;

const char* svt_last_error(void);
int svt_abi_version(void);
/* The 16-bit operand type of precision code SVT_PREC_BF16 in THIS build of the library: 0 = bf16 (libsvt_mi355.so), 1 = IEEE half
 * (libsvt_mi355_f16.so: the same sources compiled with -DSVT_OPERAND_F16 -- same MFMA rate, three more mantissa bits; serves
 * precision codes 0 and 1 only). */
int svt_operand_type(void);
/* number of visible HIP devices whose arch is gfx950 (0 => the product path must fail loudly) */
int svt_device_count(void);

/* ---- encoder: replaces HuggingFaceWav2Vec2 (huggingface_interface.py:47-297) + the HF model it wraps ---- */
int svt_encoder_create(const svt_encoder_config* cfg, int device, svt_encoder** out);
void svt_encoder_destroy(svt_encoder* e);

/* Optional "global-batch-equivalent" norms for a batch that is ONE SHARD of a larger one (the reference's
 * wrapper normalises over every element of the batch it is given: huggingface_interface.py:289-295).  With a function set, every
 * forward of this encoder calls it twice, in stream order on the forward's stream -- after the waveform moments and after the
 * moments of the encoder output -- with a DEVICE pointer to the (sum, sum of squares) pair in double precision; the function must
 * replace the pair by its sum over all ranks (an all-reduce of 16 bytes: dist.all_reduce on a tensor wrapping the pointer, or
 * ncclAllReduce on `stream`) and return 0.  The statistics are then taken over global_clips clips (the clip count of the whole
 * global batch, equal lengths), and N shards return what one device returns for the whole batch.  Whole-batch norms only
 * (clips_per_norm_group = 0).  fn = NULL restores the per-shard norms, which is what the reference's DataParallel / DDP runs do. */
typedef int (*svt_norm_reduce_fn)(double* sums_dev, int32_t n_doubles, void* stream, void* user);
int svt_encoder_set_norm_reduce(svt_encoder* enc, svt_norm_reduce_fn fn, void* user, int64_t global_clips);
/* SpecAugment inside the encoder (HF _mask_hidden_states; the wrapper's apply_spec_augment=True).  While masks are set, every
 * forward of this encoder (svt_encoder_forward, _ex and _forward_head) runs svt_spec_augment's one launch on the fp32 output of the
 * feature projection, in front of the positional conv, with the parameter "masked_spec_embed" as the embedding.  time_mask_dev:
 * batch * frames bytes or NULL; feature_mask_dev: batch * hidden_size bytes (4-byte aligned) or NULL; device buffers owned by the
 * caller, read in stream order by every forward until they are replaced or cleared.  batch / frames: the geometry the masks were made
 * for -- a forward with another batch or frame count fails with SVT_ERR_INVALID before it launches anything.  (NULL, NULL) clears the
 * masks (batch and frames are then ignored): the forward is the plain one, with no launch added and no kernel changed.
 * SVT_ERR_KEY: a time mask on an encoder that never received "masked_spec_embed" (shape (hidden_size,)). */
int svt_encoder_set_spec_augment(svt_encoder* enc, const uint8_t* time_mask_dev, const uint8_t* feature_mask_dev, int32_t batch,
                                 int32_t frames);
/* Training-mode dropouts and layerdrop inside the encoder (HF modeling_wav2vec2.py: the model in train() mode; the wrapper's
 * freeze=False).  While a state is set, every forward of this encoder (svt_encoder_forward, _ex and _forward_head) skips the layers of
 * skip_mask and applies the element dropouts whose rate is above 0.  The mask of an element is a function of its POSITION:
 *     word = Philox4x32-10(key = (seed_lo, seed_hi), counter = (q_lo, q_hi, site | layer << 8, step))[e & 3],   q = e >> 2
 *     e is kept iff word >= floor(p * 2^32); a kept value is multiplied by float(1 / (1 - p)), a dropped one becomes +0
 * with e the element's LOGICAL index -- (b*T + t)*W + c in a (B, T, W) tensor, ((b*H + h)*T + i)*T + j in the attention
 * probabilities -- never a padded or tiled one, seed_lo / seed_hi the halves of `seed`, and the sites
 *     0  output of the feature projection (feat_proj_dropout), in front of SpecAugment
 *     1  the encoder's own dropout (hidden_dropout): behind the positional conv and the first LayerNorm (post-LN), or behind the
 *        positional conv alone, in front of the layers (stable_layer_norm)
 *     2  attention probabilities (attention_dropout): softmax -> dropout -> P V, as HF's eager attention
 *     3  the attention branch behind the out-projection (hidden_dropout)
 *     4  behind FFN-1's GELU (activation_dropout)
 *     5  behind FFN-2 (hidden_dropout)
 * (sites 0 and 1: layer = 0).  No parity with the masks torch's device generator would draw is claimed: those depend on torch's launch
 * geometry.  Where the residual stream is stored twice (an fp32 copy beside the operand copy) both copies receive the same mask; the
 * bf16 (hi, lo) stream has its value float(hi) + float(lo) scaled or zeroed and is cut again (hi' = T(o), lo' = T(o - hi')).
 * With attention_dropout > 0 the attention takes the score-matrix path for every geometry by default, whose score and probability
 * buffers svt_encoder_workspace_bytes counts ONLY while such a state is set: set the state BEFORE the size query.  fused_attention != 0
 * opts in to the fused attention with the mask inside (csrc/attention_drop.hip, flash_attn_drop_kernel): where the plain forward runs a
 * fused 16-bit kernel (SVT_PREC_BF16, head size 64 or 128, no position bias) the masked forward then runs its masked form -- the same
 * mask bit for bit, the row sum over all keys, the scale folded into the final division -- and the workspace is the plain forward's (no
 * score or probability buffers); every other geometry and precision runs the score-matrix path exactly as with 0.  The default stays 0
 * so that a forward recorded at a (seed, step) replays bit for bit: the two forms round the probabilities in different places.
 * With hidden_dropout > 0 FFN-2 takes its un-split form.  skip_mask: bit l set = layer l is skipped and launches nothing (HF's
 * layerdrop; the caller draws -- torch.rand([]) < layerdrop per layer, in layer order); `layerdrop` itself is only recorded.
 * The state is sticky on the handle; NULL clears it, and the forward is then the plain one: no launch added, no kernel changed.
 * SVT_ERR_INVALID: a rate outside [0, 1), a bit of skip_mask at or above num_layers, more than 64 layers with a skip, an element
 * rate above 0 in a split-operand precision (SVT_PREC_BF16X3 / SVT_PREC_FP16X3 serve layerdrop only: their activations travel as
 * pair rows, which these kernels do not read), attention_dropout > 0 with a relative position bias (WavLM: the reference runs torch's
 * fused multi-head attention there, which offers no seam to pin a mask against), layer 0 of such an encoder skipped while a later layer runs (the
 * reference cannot: only layer 0 holds the position embedding).
 * struct_size: the size of this structure, or that of its form without fused_attention (the first 64 bytes: callers built before the
 * field existed), which means fused_attention = 0; every other size is refused. */
typedef struct svt_dropout {
  int32_t struct_size;
  uint32_t step;
  double feat_proj_dropout;
  double hidden_dropout;
  double attention_dropout;
  double activation_dropout;
  double layerdrop;
  uint64_t seed;
  uint64_t skip_mask;
  int32_t fused_attention;
  int32_t reserved;   /* padding; ignored */
} svt_dropout;
int svt_encoder_set_dropout(svt_encoder* enc, const svt_dropout* state);
/* copy one parameter by its HF state-dict key (without the wrapper's "model." prefix); both weight-norm
 * spellings of the positional conv are accepted (…conv.weight_g/_v and …parametrizations.weight.original0/1).
 * "masked_spec_embed" (hidden_size) is optional: kept in fp32 for svt_encoder_set_spec_augment.
 * replaces: Module.load_state_dict (speechbrain/utils/checkpoints.py:69-95, train_audio_ssl.py:232-234) */
int svt_encoder_load_param(svt_encoder* e, const char* key, const void* data_host, int dtype,
                           const int64_t* shape, int ndim);
/* fold weight-norm, pack q/k/v, reorder conv kernels for implicit GEMM, cast to the operand type,
 * upload.  Fails with SVT_ERR_KEY (naming the key) if a required parameter was never loaded. */
int svt_encoder_finalize(svt_encoder* e);
/* read a (possibly folded) parameter back as fp32 by HF key — for state_dict() round trips */
int svt_encoder_get_param(svt_encoder* e, const char* key, void* out_host, int64_t capacity_elems);
int64_t svt_encoder_num_frames(const svt_encoder* e, int64_t n_samples);
/* (the size follows the dropout state of the handle: svt_encoder_set_dropout, which must be called before this query) */
int64_t svt_encoder_workspace_bytes(const svt_encoder* e, int32_t batch, int64_t n_samples);
/* replaces: HuggingFaceWav2Vec2.extract_features (:279-297): wav f32 (B,L) -> feats f32 (B,T,D) */
int svt_encoder_forward(svt_encoder* e, const float* wav_dev, int32_t batch, int64_t n_samples,
                        float* feats_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
/* Same, with the wrapper's two whole-tensor layer norms (huggingface_interface.py:289-295) taken over groups of
 * `clips_per_norm_group` consecutive clips instead of the whole batch (0 = whole batch = svt_encoder_forward).  With 1, a batch
 * of B equal-length clips gives what B batch-1 calls give: the reference's evaluation loop (MIR_ST500/train_audio_ssl.py:90
 * asserts batch 1; utterances of a song are 5 s each) run as ONE batch.  batch must be a multiple of the group size. */
int svt_encoder_forward_ex(svt_encoder* e, const float* wav_dev, int32_t batch, int64_t n_samples,
                           float* feats_dev, void* workspace_dev, size_t workspace_bytes, void* stream,
                           int32_t clips_per_norm_group);

/* encoder + whole-batch output norm + frame head (+ per-frame decode) in one call, WITHOUT writing the (B, T, D) features:
 * what AMT.compute_forward computes (MIR_ST500/train_audio_ssl.py:28-48: feats = wav2vec2(wavs); logits = model(feats))
 * followed, when frames_out_dev is given, by the sigmoid / argmax of compute_objectives (:93-100).  The head is linear, so
 * the raw dots x.w are taken in the single pass over the un-normalised encoder output that also sums the two moments of
 * the output norm; a second pass over B*T*n_out values applies (dot - mean * sum(w)) * rstd + bias and decodes.
 * head: an svt_linear with in_features = hidden_size (512 / 768 / 1024) and out_features <= 32 on the same device.
 * logits_out_dev: (B, T, n_out) fp32.  frames_out_dev: B*T svt_frame or NULL (then n_octave / n_class are ignored). */
int svt_encoder_forward_head(svt_encoder* enc, const svt_linear* head, const float* wav_dev, int32_t batch,
                             int64_t n_samples, float* logits_out_dev, svt_frame* frames_out_dev, int32_t n_octave,
                             int32_t n_class, void* workspace_dev, size_t workspace_bytes, void* stream,
                             int32_t clips_per_norm_group);

/* ---- frame head + per-frame decode: replaces speechbrain.nnet.linear.Linear (linear.py:41-76)
 *      and the sigmoid/argmax loop (train_audio_ssl.py:41-46,93-100) ---- */
int svt_linear_create(int32_t in_features, int32_t out_features, int has_bias, int device, svt_linear** out);
void svt_linear_destroy(svt_linear* l);
int svt_linear_load(svt_linear* l, const float* weight_host /*out x in*/, const float* bias_host /*out or NULL*/);
/* y = x W^T + b, fp32 in / fp32 accumulate / fp32 out; rows = product of leading dims */
int svt_linear_forward(svt_linear* l, const float* x_dev, int64_t rows, float* y_dev, void* stream);
/* logits (rows, 2+n_octave+1+n_class+1) -> frames; argmax = first maximum, sigmoid in fp32 */
int svt_decode_frames(const float* logits_dev, int64_t rows, int32_t n_out, int32_t n_octave,
                      int32_t n_class, svt_frame* frames_dev, int device, void* stream);
/* frame2note (reference MIR_ST500/utils.py:82-149; called per song at train_audio_ssl.py:104-108) over a batch of decoded frame
 * sequences ON THE HOST: frames = batch x frames_per_clip records (host memory, as copied back from svt_decode_frames /
 * svt_encoder_forward_head), n_frames = valid frames per clip (NULL: all).  Outputs, per clip b at [b * capacity_per_clip ...]:
 * onset / offset times in seconds (frame_size * frame index, double like the reference's Python floats), pitch (MIDI number =
 * mode of the note's frames + 36), the note's frame range [lo, hi), and n_notes[b].  Where the top pitch count is tied the
 * reference's answer is CPython's max(set(bag), key=bag.count) -- set iteration order -- so pitch is -1 and the caller resolves it
 * from the frames in [lo, hi) (svt_speechbrain_amd/decode.py does).  A one-frame sequence above the onset threshold is the
 * reference's ValueError (max of an empty window): SVT_ERR_INVALID.  No device call is made. */
int svt_frames_to_notes(const svt_frame* frames_host, int32_t batch, int64_t frames_per_clip, const int64_t* n_frames,
                        float onset_thres, float offset_thres, double frame_size, int32_t n_octave, int32_t n_class,
                        double* t_on, double* t_off, int32_t* pitch, int32_t* lo, int32_t* hi, int64_t capacity_per_clip,
                        int64_t* n_notes);

/* ---- RCA fusion: replaces FusionRCA (N20EMv2/audio_visual/fusion.py:186-209) ---- */
int svt_rca_create(int32_t d_model, int32_t nhead, int32_t d_ffn, float alpha, int32_t max_len,
                   int32_t precision, int device, svt_rca** out);
void svt_rca_destroy(svt_rca* r);
/* keys as in the FusionRCA state dict: "fusion.layer1.self_att.att.in_proj_weight", … */
int svt_rca_load_param(svt_rca* r, const char* key, const void* data_host, int dtype,
                       const int64_t* shape, int ndim);
int svt_rca_finalize(svt_rca* r);
int64_t svt_rca_workspace_bytes(const svt_rca* r, int32_t batch, int32_t t_audio);
/* audio (B,T1,D), video (B,T2,D) f32 -> out (B,T1,D) f32; video is truncated / zero-padded to T1 */
int svt_rca_forward(svt_rca* r, const float* audio_dev, int32_t t_audio, const float* video_dev,
                    int32_t t_video, int32_t batch, float* out_dev, void* workspace_dev,
                    size_t workspace_bytes, void* stream);
/* Training step of FusionRCA + head on frozen features (N20EMv2/audio_visual/train_rca_av.py:174-185); precision fp32 or bf16, head
 * size 64 or 128 (otherwise SVT_ERR_INVALID).  The 24 fusion tensors are in this order, for layer1 then layer2: self_att.att.
 * in_proj_weight, in_proj_bias, out_proj.weight, out_proj.bias, pos_ffn.ffn.0.weight, .0.bias, .3.weight, .3.bias, norm1.norm.weight,
 * .bias, norm2.norm.weight, .bias (the positional table is not trainable).  No entry point below synchronises or copies.
 *
 * svt_rca_refresh_params: rewrites the handle's weights on `stream` from params_dev (24 device fp32 tensors) -- the operand-format
 * copies the forward reads, with the bits a fresh svt_rca_load_param + svt_rca_finalize gives, and the transposed copies the backward
 * needs.  Required once after every svt_rca_finalize before svt_rca_backward.  Unlike svt_rca_finalize it does not wait for forwards
 * in flight: the caller orders it after every forward on other streams that reads this handle (replica lanes included). */
int svt_rca_refresh_params(svt_rca* r, const float* const* params_dev, int32_t n, void* stream);
int64_t svt_rca_train_workspace_bytes(const svt_rca* r, int32_t batch, int32_t t_audio);
/* the kernels of svt_rca_forward (the same output bits), keeping in the workspace what svt_rca_backward reads */
int svt_rca_forward_train(svt_rca* r, const float* audio_dev, int32_t t_audio, const float* video_dev, int32_t t_video, int32_t batch,
                          float* out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
/* d(out) (B,T1,D) f32 -> the 24 gradients (overwritten, fp32, in the order above), from the workspace of the last
 * svt_rca_forward_train with the same batch / t_audio.  No float atomics: two calls give the same bits. */
int svt_rca_backward(svt_rca* r, const float* dout_dev, int32_t batch, int32_t t_audio, float* const* grads_dev, void* workspace_dev,
                     size_t workspace_bytes, void* stream);

/* ---- CTC greedy: replaces speechbrain.decoders.ctc.ctc_greedy_decode (ctc.py:341-383) ----
 * probs (B,T,V) f32, rel_lens (B,) f32 (device).  tokens_dev (B,T) i32 receives the collapsed, blank-free
 * ids left-aligned per row; out_lens_dev (B,) i32 their counts.  blank < 0 counts from V. */
int svt_ctc_greedy(const float* probs_dev, int32_t batch, int32_t t, int32_t v, const float* rel_lens_dev,
                   int32_t blank, int32_t* tokens_dev, int32_t* out_lens_dev, int device, void* stream);

/* ---- Fbank: replaces speechbrain.lobes.features.Fbank default chain (features.py:126-143) ----
 * wav (B,L) f32 -> (B, 1+L/hop, n_mels) f32; hamming win, centred, constant pad, power, triangular mel,
 * 10 log10 clamp 1e-10, per-sequence top_db clip. */
int64_t svt_fbank_workspace_bytes(int32_t batch, int64_t n_samples, int32_t n_fft, int32_t hop, int32_t n_mels);
int svt_fbank(const float* wav_dev, int32_t batch, int64_t n_samples, int32_t sample_rate, int32_t n_fft,
              int32_t win_length, int32_t hop_length, int32_t n_mels, float f_min, float f_max, float top_db,
              float* out_dev, void* workspace_dev, size_t workspace_bytes, int device, void* stream);

/* ---- noise mixing at several SNRs: replaces the per-SNR chain of N20EMv2/audio_visual/synthesis_noise.py:123-137 (clone, scale,
 * compute_amplitude, rescale the noise, add) over speechbrain.processing.signal_processing.compute_amplitude (mean |x| of the whole
 * track) and dB_to_amplitude ----
 * For clean a and noise v of n_samples each and the n_snr (1..8) ratios snr_db_host[s] (host memory, dB):
 *     f_s = 1 / (10^(snr_s / 20) + 1) in double;  out_dev[s * ld_out + i] = (1 - f_s) a[i] + (f_s mean|a| / (mean|v| + 1e-14)) v[i]
 * always from the ORIGINAL v (the reference rescales its noise tensor in place from one SNR to the next, which is the same formula
 * with a few ulps of drift per step).  Two launches on `stream`, no synchronisation and no host round trip: sum |a| and sum |v| in fp64
 * (per-workgroup partials added in workgroup order: reproducible bit for bit, no float atomics), then one pass that derives both
 * coefficients of every row in fp64 on the device, rounds each ONCE to fp32 and evaluates fma(c2, v, c1 * a) in fp32; every element is
 * within 3 * 2^-24 * (|a| (1 - f) + |v| f mean|a| / (mean|v| + 1e-14)) + 2^-149 of the formula in exact arithmetic.  mean|v| == 0
 * (a silent noise track) takes c2 = 0, so out = c1 a.  clean_dev, noise_dev and out_dev need 4-byte alignment only; ld_out >= n_samples,
 * and out_dev[s * ld_out + n_samples .. (s + 1) * ld_out) is not written.  amps_out_dev: NULL, or 2 doubles (8-byte aligned) that
 * receive mean|a|, mean|v|; with them out_dev may be NULL: the amplitudes alone, no row is written.  workspace_dev: as many bytes as the workspace query returns, 8-byte aligned, contents irrelevant.
 * n_samples < 1, n_snr outside 1..8, ld_out < n_samples or a non-finite ratio: SVT_ERR_INVALID; a smaller workspace: SVT_ERR_WORKSPACE.
 * The sums use SVT_NOISE_AMP_WORKGROUPS workgroups per track at most and the mix SVT_NOISE_MIX_MAX_WORKGROUPS, of 256 threads x 4
 * samples: longer tracks take further trips of the grid-stride loops. */
#define SVT_NOISE_AMP_WORKGROUPS 256
#define SVT_NOISE_MIX_MAX_WORKGROUPS 2048
int64_t svt_noise_mix_workspace_bytes(int64_t n_samples, int32_t n_snr);
int svt_noise_mix(const float* clean_dev, const float* noise_dev, int64_t n_samples, const float* snr_db_host, int32_t n_snr,
                  float* out_dev, int64_t ld_out, double* amps_out_dev, void* workspace_dev, int64_t workspace_bytes, int device,
                  void* stream);

/* ---- polyphase resampling with an optional stereo downmix: replaces speechbrain.processing.speech_augmentation.Resample (Kaldi's
 * LinearResample: a Python loop of conv1d / conv_transpose1d / pad / += over the P phases) and the `.mean(dim=0)` that follows it in
 * MIR_ST500/prepare_benchmarks.py:49-72 and N20EMv2/audio_visual/synthesis_noise.py:18-48 (resample_wav) ----
 * With g = gcd(orig, new), S = orig / g input samples per unit and P = new / g phases, and a host-built table of P filters of W taps
 * (weights_dev: P x W fp32, row pitch W; first_dev: P int32, the input offset of each filter's first tap within its unit):
 *     y[row][n * P + p] = sum_{j < W} x[row][n * S + first[p] + j] * weights[p][j]        x taken as 0 outside [0, n_in)
 * for the n_out outputs the reference's tick rule gives (svt_resample_output_samples: the outputs at times in [0, n_in / orig)).
 * downmix != 0: rows come in channel pairs (2 r, 2 r + 1) and output row r is 0.5 * (y[2 r] + y[2 r + 1]) of the two fp32 sums, which
 * is resample-then-mean (the halving is exact).  One launch on `stream` for any number of rows; no synchronisation, no allocation.
 * Each output is ONE fp32 sum over the W taps in ascending order (fused multiply-adds); two calls give the same bits.
 * in_dev: rows x n_in, row pitch ld_in >= n_in; out_dev: (downmix ? rows / 2 : rows) x n_out, row pitch ld_out >= n_out; nothing is
 * read outside a row's n_in samples and nothing is written at out_dev[r * ld_out + n_out .. (r + 1) * ld_out).  All pointers need
 * 4-byte alignment only.  The table stays in device memory and is not read by the host: entries of first_dev outside [-W, S] (which no
 * table of the reference's rule has) are taken at the nearer end of that range.
 * SVT_ERR_INVALID (nothing is written): rows < 1 or n_in < 1; P, W or S < 1; P == S (equal rates: nothing to do); a table and input
 * span that do not fit SVT_RESAMPLE_LDS_BYTES of LDS even at one unit per workgroup; downmix with an odd number of rows; ld_in < n_in
 * or ld_out < n_out; a null or misaligned pointer; n_out != the tick rule's value.
 * svt_resample_output_samples is host-only: the tick rule for n_in samples at orig_freq resampled to new_freq; -1 for n_in < 0 or a
 * rate < 1.
 * A workgroup of 256 threads takes G units = G * P consecutive outputs of a row at a time, G the smallest with
 * G * P >= SVT_RESAMPLE_TILE_OUTPUTS for which the table and the input span fit SVT_RESAMPLE_LDS_BYTES; the grid holds at most
 * SVT_RESAMPLE_MAX_WORKGROUPS workgroups, which stage the table once and take further tiles beyond that. */
#define SVT_RESAMPLE_LDS_BYTES 65536
#define SVT_RESAMPLE_TILE_OUTPUTS 1024
#define SVT_RESAMPLE_MAX_WORKGROUPS 768
int64_t svt_resample_output_samples(int64_t n_in, int32_t orig_freq, int32_t new_freq);
int svt_resample(const float* in_dev, int32_t rows, int64_t n_in, int64_t ld_in, const float* weights_dev, const int32_t* first_dev,
                 int32_t P, int32_t W, int32_t S, float* out_dev, int64_t n_out, int64_t ld_out, int32_t downmix, int device,
                 void* stream);

/* ---- frequency and chunk dropping of a waveform batch: replaces the DropFreq and DropChunk steps of
 * speechbrain.lobes.augment.TimeDomainSpecAugment (speechbrain/processing/speech_augmentation.py:876-1140: a conv1d with a 101-tap
 * band-reject filter between a transpose, a clone and a squeeze, then a Python loop over the batch with one slice assignment per
 * dropped chunk), the `augmentation:` block of the five training yamls ----
 * For every r < rows and t < n, with the host-built filter of `taps` fp32 coefficients and row r's max_chunks pairs {start, end}
 * (chunks_dev: rows x max_chunks x 2 int64):
 *     out[r][t] = 0.0f                                                   if start <= t < end for any chunk of row r
 *               = sum_{k < taps} filter[k] * x[r][t + k - taps / 2]      otherwise,      x taken as 0 outside [0, n)
 * The sum is a cross-correlation, as torch.nn.functional.conv1d computes it (the reference's compound filter is not symmetric: its
 * Blackman window is the periodic one).  A row's zero padding starts at the row's n samples, not at a clip's valid length: what the
 * reference does to a padded batch.  A dropped element is WRITTEN as zero, not multiplied by it: whatever the filter produced there,
 * NaN included, does not survive.  A chunk with end > n is cut at n (and start < 0 at 0), one with start >= end is empty, chunks may
 * overlap; a row with fewer chunks than max_chunks fills up with empty ones.  filter_dev == NULL with taps == 0: no filtering, the
 * elements outside the chunks are copied unchanged (DropChunk alone); chunks_dev == NULL with max_chunks == 0: no chunks (DropFreq alone).
 * Each output is ONE fp32 chain of fused multiply-adds over the taps in ascending order, started at 0: two calls give the same bits,
 * and a delta filter (1 at the centre tap) returns finite input exactly.  One launch on `stream` for any number of rows; no
 * synchronisation, no allocation, no workspace.  in_dev: rows x n, row pitch ld_in >= n; out_dev: rows x n, row pitch ld_out >= n;
 * nothing is read outside a row's n samples and nothing is written at out_dev[r * ld_out + n .. (r + 1) * ld_out).  in_dev, filter_dev
 * and out_dev need 4-byte alignment only, chunks_dev 8-byte; indices into the rows are 64-bit.
 * SVT_ERR_INVALID (nothing is written): rows < 1 or n < 1; taps even or outside 1..SVT_DROP_MAX_TAPS; filter_dev non-null with taps ==
 * 0 or null with taps != 0, and the same for chunks_dev and max_chunks; max_chunks < 0; ld_in < n or ld_out < n; in_dev or out_dev
 * null; a misaligned pointer; the rows x n extents of in_dev and out_dev (row pitches included) overlapping: the filter reads taps / 2
 * samples either side of an output, so in-place operation would be wrong.
 * A workgroup of 256 threads takes SVT_DROP_TILE_OUTPUTS consecutive outputs of a row at a time (four per lane) and stages their
 * SVT_DROP_TILE_OUTPUTS + taps - 1 input samples in LDS; a tile that lies wholly inside one chunk is zeroed without reading its input.
 * Up to SVT_DROP_MAX_WORKGROUPS (row, tile) pairs each has a workgroup of its own; beyond that the grid is cut to the pairs divided by
 * the trips they need, and every workgroup takes that many. */
#define SVT_DROP_MAX_TAPS 255
#define SVT_DROP_TILE_OUTPUTS 1024
#define SVT_DROP_MAX_WORKGROUPS 8192
int svt_drop_freq_chunk(const float* in_dev, int32_t rows, int64_t n, int64_t ld_in, const float* filter_dev, int32_t taps,
                        const int64_t* chunks_dev, int32_t max_chunks, float* out_dev, int64_t ld_out, int device, void* stream);

/* ---- SpecAugment masks on the output of the feature projection: replaces the two index_puts of HF's _mask_hidden_states
 * (transformers modeling_wav2vec2.py; reached through `apply_spec_augment=True` of MIR_ST500/huggingface_interface.py:97,126-127) ----
 * In place on h_dev, fp32 (B, T, D) with row pitch ld (elements) between frames:
 *     h[b][t][c] = 0.0f          if feature_mask[b][c] != 0
 *                = embed[c]      else if time_mask[b][t] != 0
 *                = unchanged     otherwise
 * which is HF's order: the time-masked frames take the learned masked_spec_embed, then the feature-masked columns are zeroed in
 * every frame of the clip.  time_mask_dev: B*T bytes or NULL; feature_mask_dev: B*D bytes or NULL (both NULL: nothing is launched);
 * embed_dev: D floats, needed with a time mask.  Masked elements are WRITTEN, not multiplied: a NaN there does not survive; every
 * other element keeps its bits.  One launch on `stream`, no synchronisation, no allocation, no workspace: a frame with nothing to do
 * is neither read nor written, a time-masked frame is written without being read, and of the other frames of a clip with masked
 * columns only the 16-byte pieces that hold one are touched -- the cost follows the masked rows, not B*T*D.  Accesses are 16 bytes
 * per lane: h_dev and embed_dev 16-byte aligned, feature_mask_dev 4-byte, D and ld multiples of 4, ld >= D.
 * SVT_ERR_INVALID (nothing is written): B, T or D < 1, D % 4 != 0, ld % 4 != 0, ld < D, h_dev NULL, a time mask without embed_dev,
 * a misaligned pointer. */
int svt_spec_augment(float* h_dev, int32_t B, int32_t T, int32_t D, int64_t ld, const uint8_t* time_mask_dev,
                     const uint8_t* feature_mask_dev, const float* embed_dev, int device, void* stream);

/* ---- wav files: replaces torchaudio.info / load / save and speechbrain.dataio.dataio.read_audio / write_audio for RIFF/WAVE files
 * (MIR_ST500/prepare_benchmarks.py:58, N20EMv2/audio_visual/synthesis_noise.py, MIR_ST500/train_audio_ssl.py:373-390) ----
 * The host parses and writes the header (no device call); the sample conversion runs on the GPU on the raw bytes of the file.
 *
 * svt_wav_parse walks the chunks of a file of file_bytes bytes of which head_host holds the first head_bytes (0 <= head_bytes <=
 * file_bytes; nothing past head_bytes is read).  LIST / JUNK / bext / fact and any other chunk before or after `fmt ` is skipped, with the pad
 * byte after an odd size.  Returns SVT_OK and fills *out once the header of the `data` chunk has been seen; SVT_WAV_NEED_MORE (positive)
 * with *need_bytes > head_bytes, a prefix length that gets further, when the prefix ends before that (out is not written; need_bytes
 * may be NULL otherwise); SVT_ERR_INVALID with a text that begins "svt_wav_parse" and out untouched for everything else.
 * Accepted: WAVE_FORMAT_PCM (1) at 8 / 16 / 24 / 32 bits, WAVE_FORMAT_IEEE_FLOAT (3) at 32 / 64 bits, WAVE_FORMAT_EXTENSIBLE (0xFFFE) whose
 * sub-format GUID is one of those two and whose valid bits equal the container size; 1..8 channels; block_align == channels * bits / 8.
 * frames = data bytes / block_align (a trailing partial frame is dropped); a data size of 0 or 0xFFFFFFFF (streamed writers) or one that
 * runs past file_bytes is taken as "to the end of the file".  Refused: RIFX, RF64, W64, A-law, mu-law, ADPCM and every other tag, `data`
 * before `fmt `, zero channels or rate, a chunk or header cut by the end of the file.
 *
 * svt_wav_header writes the header of a file of `frames` frames into out_host (capacity bytes) and its length into *header_bytes: for
 * SVT_PCM_S16 the canonical 44 bytes, for SVT_PCM_F32 tag 3 with an 18-byte `fmt ` (cbSize 0) and a `fact` chunk, 58 bytes (the RIFF
 * specification's form for non-PCM data).  Other formats, channels outside 1..8, sample_rate < 1, frames < 0, a smaller capacity and
 * data beyond 4 GiB - 1 - header: SVT_ERR_INVALID.  svt_wav_parse of its output returns its arguments. */
typedef enum { SVT_PCM_U8 = 1, SVT_PCM_S16 = 2, SVT_PCM_S24 = 3, SVT_PCM_S32 = 4, SVT_PCM_F32 = 5, SVT_PCM_F64 = 6 } svt_pcm_format;
#define SVT_WAV_NEED_MORE 1
typedef struct svt_wav_info {
  int32_t format;            /* svt_pcm_format */
  int32_t channels;
  int32_t sample_rate;
  int32_t bits_per_sample;
  int32_t block_align;       /* bytes per frame */
  int64_t data_offset;       /* byte offset of the first frame in the file */
  int64_t frames;
} svt_wav_info;
int svt_wav_parse(const void* head_host, int64_t head_bytes, int64_t file_bytes, svt_wav_info* out, int64_t* need_bytes);
int svt_wav_header(int32_t format, int32_t channels, int32_t sample_rate, int64_t frames, void* out_host, int64_t capacity,
                   int64_t* header_bytes);

/* svt_pcm_decode: `frames` interleaved little-endian frames of `channels` samples at src_dev, at ANY byte alignment (an offset into a
 * 24-bit stereo file is a multiple of 6), to planar fp32: row c of out_dev, at pitch ld_out >= frames, holds channel c; with downmix
 * != 0 (2 channels only) the one row 0.5f * (l + r), the `.mean(dim=0)` of the preparation scripts: one rounding for the sum and an
 * exact halving.  Every value is the fp32 nearest (ties to even) to the exact one: U8 (b - 128) / 128, S16 x / 2^15, S24 x / 2^23 (all
 * three exact), S32 x / 2^31 (the one rounding of the int -> float conversion, then an exact scale: INT32_MAX gives 1.0), F32 the bits
 * unchanged (NaN payloads and -0.0 included), F64 rounded once to fp32.  These are torchaudio's normalize=True conventions; no bit
 * parity with sox is claimed for S32 / F64.
 * svt_pcm_encode: the way back for the two formats the reference writes.  Row c of in_dev (pitch ld_in >= frames, 4-byte aligned) is
 * channel c; dst_dev, at any byte alignment, receives `frames` interleaved frames.  F32: the bits unchanged (torchaudio.save of a float32
 * tensor).  S16: q = clamp(rint(x * 32768), -32768, 32767) with ties to even, NaN -> 0, +-inf clamped; the scale is exact in fp32
 * (soundfile's PCM_16).  No parity with sox's rounding is claimed.
 * Both: one launch on `stream`, no synchronisation, no allocation, no workspace, no atomics; two calls give the same bytes.  Nothing
 * outside [src_dev, src_dev + frames * block_align) is read, nothing outside the `frames` elements of each row (decode) or the frames *
 * block_align bytes at dst_dev (encode) is written; the gaps of ld_out stay untouched.  A workgroup of 256 threads takes
 * SVT_PCM_FRAMES_PER_WORKGROUP consecutive frames at a time and the grid holds at most SVT_PCM_MAX_WORKGROUPS of them; longer inputs
 * take further trips of the grid-stride loop.
 * SVT_ERR_INVALID (nothing is written): a null pointer, out_dev / in_dev not 4-byte aligned, channels outside 1..8, frames < 1, ld <
 * frames, downmix with channels != 2, for decode a format that is none of the six, for encode one other than S16 / F32. */
#define SVT_PCM_FRAMES_PER_WORKGROUP 4096
#define SVT_PCM_MAX_WORKGROUPS 1024
int svt_pcm_decode(const void* src_dev, int32_t format, int32_t channels, int64_t frames, float* out_dev, int64_t ld_out, int32_t downmix,
                   int device, void* stream);
int svt_pcm_encode(const float* in_dev, int64_t ld_in, int32_t channels, int64_t frames, int32_t format, void* dst_dev, int device,
                   void* stream);

/* ======================================================================================================================
 * DIAGNOSTIC SURFACE: svt_debug_* and svt_prof_*.  These entry points exist for the unit tests of single kernels, the micro-benchmarks
 * under tools/ and the bench's per-launch timing.  They are the ONE exception to the conventions of the product entry points above:
 * a svt_debug_* call may allocate and free device memory and may synchronise its stream (hipMalloc / hipStreamSynchronize inside), and
 * svt_debug_set changes process-wide kernel selection.  No product entry point (svt_encoder_*, svt_linear_*, svt_rca_*, svt_video_*,
 * svt_decode_frames, svt_ctc_greedy, svt_fbank, svt_deltas, svt_context_window, svt_bce_loss, svt_nll_loss, svt_softmax and the
 * training step) calls them, and none of those allocates or synchronises, except svt_amt_objective_grad, which synchronises its
 * stream to report an out-of-range target.
 * ====================================================================================================================== */
/* ---- test / micro-benchmark hook: the dense contraction kernel on caller-supplied operands ----
 * C (M,N) = act(A W^T + bias) + resid with A (M,K) and W (N,K) in the operand type of `precision`
 * (fp32, or bf16 bits for SVT_PREC_BF16; the split-operand precisions take fp32 operands), C in the operand type unless out_f32.  a_rpb/a_bstride/a_rstride describe the
 * implicit-conv row addressing (row m starts at (m / a_rpb) * a_bstride + (m % a_rpb) * a_rstride elements);
 * pass a_rpb = M, a_bstride = 0, a_rstride = K for a plain row-major A; ldw = W row pitch (>= K). */
int svt_debug_gemm(int32_t precision, const void* a_dev, const void* w_dev, void* c_dev, const float* bias_dev,
                   const float* resid_dev, int32_t m, int32_t n, int32_t k, int32_t a_rpb, int64_t a_bstride,
                   int64_t a_rstride, int64_t ldw, int32_t act, int32_t out_f32, int device, void* stream);

/* The same hook for the split-operand modes' PAIR-ROW products (csrc/gemm_x3q.hip: both operands pre-cut into 16-bit (hi, lo) pieces,
 * 32 elements per 128-byte line): `a_dev` is the fp32 tensor (a_elems elements, a multiple of 32; rows addressed as above with strides
 * in multiples of 32 elements), converted to pair rows inside the hook; the product runs with the pair-row operand and writes
 * out_kind 0 = fp32 rows, 1 = pair rows, 2 = separate (hi, lo) planes -- 1 and 2 are converted back to fp32 (hi + lo) into c_dev, so
 * the caller always compares an fp32 (M, N) result.  precision = SVT_PREC_BF16X3 / SVT_PREC_FP16X3; act 0 / 1 (exact-erf GELU). */
int svt_debug_gemm_pairs(int32_t precision, const float* a_dev, int64_t a_elems, const float* w_dev, float* c_dev, const float* bias_dev,
                         int32_t m, int32_t n, int32_t k, int32_t a_rpb, int64_t a_bstride, int64_t a_rstride, int32_t act,
                         int32_t out_kind, int device, void* stream, int32_t time_iters, float* ms_out);
/* (time_iters > 0 with ms_out: after the checked launch the product alone is launched time_iters more times between two HIP events;
 *  *ms_out = milliseconds per launch -- tools/x3q_bench.py) */

/* The same hook for the BATCHED forms of the product (blockIdx.y = z; tests/test_gpu_gemm_batched.py): nz problems of one launch,
 * z = z1 * nz2 + z2, problem z reading A at a + z1 * a_z1 + z2 * a_z2, W at w + z1 * w_z1 + z2 * w_z2 and the bias at bias + z2 * bias_z2
 * and writing C (and reading resid, fp32, with C's indexing) at c + z1 * c_z1 + z2 * c_z2 with row pitch ldc:
 *     C[z][m][n] = act(alpha * sum_k A[z][m][k] W[z][n][k] + bias[z2][n]) + resid[z][m][n],
 * every stride in elements, rows of A addressed as for svt_debug_gemm.  These are the launches of the score-matrix attention
 * (alpha = scale, ldc > n, slices of one packed projection), of the grouped positional convolution (a column slice per group of a wider
 * row, a bias slice per group) and of its phase-folded form.  In the split-operand precisions with ldw == k and k % 32 == 0 the weight
 * rows the batch spans are cut into (hi, lo) pieces for the call and forgotten after a stream synchronise.  struct_size = the size of
 * the structure; act: 0 none, 1 GELU, 2 ReLU. */
typedef struct svt_debug_gemm_desc {
  int32_t struct_size;
  const void* a;
  const void* w;
  void* c;
  const float* bias;
  const float* resid;
  int32_t m, n, k;
  int32_t a_rpb;
  int64_t a_bstride, a_rstride;
  int64_t ldw, ldc;
  int32_t nz, nz2;
  int64_t a_z1, a_z2, w_z1, w_z2, c_z1, c_z2, bias_z2;
  float alpha;
  int32_t act, out_f32;
} svt_debug_gemm_desc;
int svt_debug_gemm_batched(int32_t precision, const svt_debug_gemm_desc* d, int device, void* stream);

/* ---- test hook: one launch of a row LayerNorm launcher (csrc/layernorm.hip) on caller-supplied device buffers; tests/test_gpu_layernorm.py ----
 * y = LN(t) gamma + beta [-> GELU] over the D columns of each of `rows` rows; the descriptor holds the union of the three launchers'
 * arguments, and `form` says which one runs (fields of another form are ignored):
 *   form 0  launch_layernorm: t = x [+ add] [+ addP].  prec 0 / 1 = fp32 / the build's 16-bit type for yT, and for x unless x_is_f32;
 *           every output is optional: yT (type of prec), yF (fp32), sumF (fp32, receives t), yP (pair rows: every 32 consecutive elements
 *           as 64 bytes of hi pieces then 64 bytes of lo pieces in the 128 bytes of the fp32 slab they replace; pair_kind 2 = bf16 pieces,
 *           3 = IEEE-half pieces; needs fp32 x, prec 0, no yT, D in {512, 768, 1024}); add fp32; addP pair rows (needs yP; may alias it).
 *   form 1  launch_layernorm_hilo: (yh, yl) = cut(LN(t)), 16-bit planes of the build's type, yF (optional) the fp32 result;
 *           t = x32 (fp32; rh, rl NULL), or t = (rh + rl) [+ branch] with rh, rl, branch 16-bit (x32 NULL).  D in {512, 768, 1024}.
 *   form 2  launch_layernorm_hilo_parts: t = (rh + rl) + rn16(parts[0] + ... + parts[nparts - 1] + pbias): `nparts` fp32 partial
 *           products (rows, D), part_stride elements apart, pbias (D) fp32.  D in {512, 768, 1024}.
 * gamma, beta (D) fp32.  In-place use as the callers have it is allowed: x == sumF, x == yT, add == yF, add == sumF, addP == yP,
 * yh == rh with yl == rl.
 * The hook is NARROWER than the launchers in one respect: it refuses (SVT_ERR_INVALID, nothing is launched) whatever they leave to their
 * callers, so that no argument can send a kernel outside the buffers it was given -- rows < 1, D < 1, a NULL gamma / beta / x, prec 0
 * with a 16-bit x, forms 1 / 2 with D outside {512, 768, 1024} or without yh / yl, form 1 without exactly one of {x32} and {rh, rl},
 * nparts < 1 or parts closer than rows * D elements, and ANY non-NULL pointer that is not 16-byte aligned (128-byte for yP / addP).
 * The unaligned fall-backs of launch_layernorm are therefore not reachable through it; the one-row (hi, lo) kernel is reached with
 * svt_debug_set key 20 = 0.  A launcher's own refusal comes back as SVT_ERR_INVALID too.  struct_size = the size of the structure.
 * svt_debug_set(40, 0) says which kernel the launch chose. */
typedef struct svt_debug_layernorm_desc {
  int32_t struct_size;
  int32_t form;
  int32_t prec, x_is_f32;
  int64_t rows;
  int32_t D, gelu;
  float eps;
  int32_t pair_kind;
  const float* gamma;
  const float* beta;
  const void* x;
  void* yT;
  float* yF;
  const float* add;
  float* sumF;
  void* yP;
  const void* addP;
  const void* branch;
  const void* rh;
  const void* rl;
  const float* x32;
  void* yh;
  void* yl;
  const float* parts;
  const float* pbias;
  int64_t part_stride;
  int32_t nparts;
} svt_debug_layernorm_desc;
int svt_debug_layernorm(const svt_debug_layernorm_desc* d, int device, void* stream);

/* ---- test hook: ONE launch of a dropout kernel (csrc/dropout.hip) on caller-supplied device buffers; tests/test_gpu_dropout_kernels.py ----
 * form 0: launch_dropout_rows, in place on x -- n elements of fp32 (prec 0) or of the build's 16-bit operand type (prec 1);
 * form 1: launch_dropout_hilo, in place on the 16-bit pair (xh, xl) of n elements each;
 * form 2: launch_softmax_dropout, S (rows, Tp) fp32 -> P (rows, Tp) fp32 (prec 0) or 16-bit (prec 1), T real columns (n is ignored).
 * The mask is svt_dropout's: rate p in [0, 1), seed, step, site, layer; element i of forms 0 / 1 has the logical index e0 + i, column j
 * of row r of form 2 the index e0 + r*T + j -- e0 lets a small tensor reach q_hi != 0 and every alignment of the four-word groups.
 * Pointers: element-aligned; 16-byte accesses are used when e0 % 4 == 0 and the pointers are 16-byte aligned, as in the encoder.
 * svt_debug_set(44, 0) says which kernel ran.  struct_size = the size of the structure. */
typedef struct svt_debug_dropout_desc {
  int32_t struct_size;
  int32_t form;
  int32_t prec;
  int32_t site;
  int32_t layer;
  uint32_t step;
  double p;
  uint64_t seed;
  uint64_t e0;
  int64_t n;
  int64_t rows;
  int32_t T;
  int32_t Tp;
  void* x;
  void* xh;
  void* xl;
  const float* S;
  void* P;
} svt_debug_dropout_desc;
int svt_debug_dropout(const svt_debug_dropout_desc* d, int device, void* stream);

/* ---- test hook: one launch of ONE launcher of the waveform front end (csrc/stats.hip, csrc/conv0.hip, csrc/conv0_mfma.hip) on
 * caller-supplied device buffers; tests/test_gpu_conv0.py ----
 * The descriptor holds the union of the seven launchers' arguments; `form` says which one runs (fields of another form are ignored):
 *   form 0  launch_moments: mom[2 g] = sum, mom[2 g + 1] = sum of squares of x[g n .. (g + 1) n), g < groups (fp64, written, not
 *           accumulated); scratch sized for groups_max groups.
 *   form 1  launch_conv0_window_moments: wm[65 b ..] = the 10 tap sums and 55 tap products (j <= j2, products rounded to fp32) over the T1
 *           windows of stride `stride` of clip b of wav (B, L).
 *   form 2  launch_conv0_group_coef: coef (B, C, 11) fp32 from wm (B, 65), the waveform moments wav_mom (2 per norm group of cpg clips,
 *           over n_wav samples; NULL = the waveform is not normalised), w0 (C, 10), b0 (C) or NULL, gamma, beta (C); eps_wav, eps.
 *   form 3  launch_conv0_group_apply: out (B, T1, C) = gelu(sum_j coef[b, c, j] wav[b, t stride + j] + coef[b, c, 10]); prec 0 = fp32
 *           rows, 1 = the build's 16-bit rows; pair_kind 2 / 3 (prec 0, C % 32 == 0) = pair rows of bf16 / IEEE-half pieces.
 *   form 4  launch_conv0_layer: out = gelu(LN_C(conv(w0, b0) of the normalised waveform) gamma + beta); prec / pair_kind as form 3.
 *   form 5  launch_conv0_mfma_group: form 3 on the matrix pipe, C = 512; pair_kind 0 = 16-bit rows, 2 / 3 = pair rows (prec is ignored).
 *   form 6  launch_conv0_mfma_layer: form 4 on the matrix pipe, C = 512; pair_kind as form 5.
 * Buffers (elements): x groups * n floats; mom 2 * groups doubles; wav B * L floats; wm 65 * B doubles; wav_mom 2 * (B / cpg) doubles;
 * coef B * C * 11 floats; w0 10 * C, b0 / gamma / beta C floats; out B * T1 * C elements of its type (4 bytes each for pair rows).
 * The hook allocates the launchers' scratch itself (tickets and per-workgroup partials for forms 0 and 1, the table workspace for forms
 * 5 and 6), zeroes ONLY the tickets and fills the rest with 0xFF bytes, launches `repeat` times (values below 1 count as 1) on the same
 * scratch without zeroing it again -- a ticket that is not put back to 0 shows in the second launch -- synchronises the stream and, for
 * forms 0 and 1 with tickets_out != NULL (a HOST pointer), copies the final value of the groups_max (form 0) / B (form 1) tickets there.
 * The hook is NARROWER than the launchers: it refuses (SVT_ERR_INVALID, nothing is launched) every argument that could send a kernel
 * outside these buffers -- k != 10 or stride outside 1 .. 5 (in every form); groups < 1, groups > groups_max, n < 1, groups > 1 with
 * n % 4 != 0 (form 0); B < 1, T1 < 1, L < (T1 - 1) * stride + 10 (forms 1 - 6); C < 1 or C > 512 (forms 2 - 6), C % 8 != 0 (forms 3 - 6: form 2's kernel
 * takes any C); C != 512 (forms 5, 6); cpg < 1 or B % cpg != 0 (forms 2, 4, 6); wav_mom with n_wav < 1; prec outside {0, 1}, pair_kind outside {0, 2, 3}, pair rows
 * without C % 32 == 0 and prec == 0 (forms 3, 4); a NULL pointer where the form needs one (b0 and wav_mom may be NULL); ANY non-NULL
 * pointer that is not 16-byte aligned (128-byte for a pair-row out and for every out of forms 5 and 6).  Forms 5 and 6 validate their
 * geometry here and do not consult svt_debug_set key 22.  struct_size = the size of the structure.  svt_debug_set(41, 0) says which
 * kernel the launch chose. */
typedef struct svt_debug_conv0_desc {
  int32_t struct_size;
  int32_t form;
  int32_t B, C;
  int64_t L, T1;
  int32_t k, stride;
  int32_t prec, pair_kind;
  int32_t cpg, groups;
  int32_t groups_max, repeat;
  int64_t n, n_wav;
  float eps_wav, eps;
  const float* x;
  const float* wav;
  const double* wav_mom;
  const float* w0;
  const float* b0;
  const float* gamma;
  const float* beta;
  double* mom;
  double* wm;
  float* coef;
  void* out;
  uint32_t* tickets_out;
} svt_debug_conv0_desc;
int svt_debug_conv0(const svt_debug_conv0_desc* d, int device, void* stream);

/* ---- AV-HuBERT lip front-end: replaces SubModel / ResEncoder of N20EMv2/video_only/resnet.py:134-187 (the
 * `feature_extractor_video` of the AV-HuBERT model, hubert.py:344-346): 3-D stem + ResNet-18 trunk (PReLU) + Linear(512,
 * embed_dim), eval mode.  Parameter keys are SubModel.state_dict() keys ("resnet.frontend3D.0.weight", "resnet.trunk.layer1.0.
 * bn1.running_mean", ..., "proj.weight"); num_batches_tracked entries are not needed. ---- */
typedef struct svt_video svt_video;
int svt_video_create(int32_t embed_dim, int32_t precision, int device, svt_video** out);
void svt_video_destroy(svt_video* v);
int svt_video_load_param(svt_video* v, const char* key, const void* data_host, int dtype, const int64_t* shape, int ndim);
/* folds the eval-mode batch norms into the conv weights, re-lays the weights out tap-major / as MFMA fragments, uploads */
int svt_video_finalize(svt_video* v);
int64_t svt_video_workspace_bytes(const svt_video* v, int32_t batch, int32_t t, int32_t h, int32_t w);
/* keep != 0: the caller OWNS the workspace it passes to svt_video_forward -- between two calls nothing else writes it.  The zero halos
 * of the padded stage buffers (which no kernel of the path overwrites) are then written once per (workspace pointer, geometry, stream)
 * instead of on every call: 12 launches, 1.3 GB of stores, 0.25 ms per 16 x 500 frames of 88 x 88.  Default 0: the workspace is scratch
 * and every call rewrites them.  A host-side setting: no device work. */
int svt_video_keep_workspace(svt_video* v, int keep);
/* video (B,1,T,H,W) f32 on the device -> out (B,T,embed_dim) f32 */
int svt_video_forward(svt_video* v, const float* video_dev, int32_t batch, int32_t t, int32_t h, int32_t w, float* out_dev,
                      void* workspace_dev, size_t workspace_bytes, void* stream);
/* the same with a row pitch: out row (b, t) starts at out_dev + (b * t_total + t) * out_ld (out_ld >= embed_dim); zero_left > 0 also zeroes
 * the `zero_left` columns to the LEFT of every row (out_dev - zero_left must be inside the caller's buffer, out_ld >= embed_dim +
 * zero_left; zero_left and out_ld multiples of 4, out_dev - zero_left 16-byte aligned): with out_dev = feats + E, out_ld = 2 E, zero_left = E this writes AV-HuBERT's concat fusion input
 * cat([zeros (absent audio), video], -1) in place (N20EMv2/video_only/hubert.py:700-712) */
int svt_video_forward_ex(svt_video* v, const float* video_dev, int32_t batch, int32_t t, int32_t h, int32_t w, float* out_dev, int64_t out_ld,
                         int32_t zero_left, void* workspace_dev, size_t workspace_bytes, void* stream);
/* ---- the recipe's input side, fused (round 6): replaces transform_eval of N20EMv2/video_only/train_video_ssl.py:445-457 + the
 * .astype(np.float32) of :530-533 in front of the lip front-end.  roi_dev: (B, T, h_in, w_in) uint8 gray frames as np.load returns them,
 * on the device.  Every pixel u becomes float32(((double(u) - sub0) / div0 - mean) / std) -- numpy's float64 arithmetic rounded once,
 * bit-identical -- of the centre crop_h x crop_w window (offsets int(round(h_in - crop_h) / 2.), utils.py:79-83).  The recipes use
 * {0.0, 255.0, 0.421, 0.165, 88, 88}.  Workspace: svt_video_workspace_bytes(v, batch, t, crop_h, crop_w).  out_ld / zero_left as above. */
typedef struct svt_video_transform { double sub0, div0, mean, std; int32_t crop_h, crop_w; } svt_video_transform;
int svt_video_forward_u8(svt_video* v, const uint8_t* roi_dev, int32_t batch, int32_t t, int32_t h_in, int32_t w_in,
                         const svt_video_transform* tf, float* out_dev, int64_t out_ld, int32_t zero_left, void* workspace_dev,
                         size_t workspace_bytes, void* stream);
/* ---- the TRAINING recipe's input side, fused: replaces transform_train of N20EMv2/video_only/train_video_ssl.py:448-452 --
 * Normalize(0, 255) -> RandomCrop((88, 88)) -> HorizontalFlip(0.5) -> Normalize(0.421, 0.165), utils.py:87-129 -- and PaddedBatch's zero
 * padding of a ragged batch.  As svt_video_forward_u8, but clip b of roi_dev (B, T, h_in, w_in) carries its own crop offsets, flip and
 * length: crop pixel (y, x) of frame t < n_frames is the pixel map of roi[b, t, y + dy, dx + (flip ? crop_w - 1 - x : x)]; frames
 * t >= n_frames are exact float zeros (what the reference pads the TRANSFORMED tensor with), whatever bytes roi_dev holds there -- they
 * are never read.  The random draws are the caller's (svt_speechbrain_amd.video.TrainTransform reproduces the reference's order).
 * clips_host: `batch` entries on the HOST, free for reuse when the call returns; they travel to the padding kernel inside its arguments,
 * 64 clips per launch (no device allocation, copy or memset: capturable).  Checked before anything is launched, SVT_ERR_INVALID with the
 * clip and the field named otherwise: 0 <= dy <= h_in - crop_h, 0 <= dx <= w_in - crop_w, flip 0 or 1, 1 <= n_frames <= t.
 * Workspace: svt_video_workspace_bytes(v, batch, t, crop_h, crop_w).  out_ld / zero_left as above. */
typedef struct svt_video_clip { int32_t dy, dx, flip, n_frames; } svt_video_clip;
int svt_video_forward_u8_clips(svt_video* v, const uint8_t* roi_dev, int32_t batch, int32_t t, int32_t h_in, int32_t w_in,
                               const svt_video_transform* tf, const svt_video_clip* clips_host, float* out_dev, int64_t out_ld,
                               int32_t zero_left, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- Fbank add-ons: replace speechbrain.processing.features.Deltas (features.py:788-850; replicate padding, kernel
 * -n..n, denominator n(n+1)(2n+1)/3) and ContextWindow (:853-940; out[..., c*ctx + j], zero padding).  x rows have pitch ldx
 * (so a delta can be written next to its source inside a wider feature tensor). ---- */
int svt_deltas(const float* x_dev, int64_t ldx, int32_t batch, int32_t t, int32_t c, int32_t window_length, float* out_dev,
               int64_t ldo, int device, void* stream);
int svt_context_window(const float* x_dev, int32_t batch, int32_t t, int32_t c, int32_t left_frames, int32_t right_frames,
                       float* out_dev, int device, void* stream);

/* ---- validation losses: replace speechbrain.nnet.losses.bce_loss / nll_loss (losses.py:402-519) over
 * compute_masked_loss (:624-684), truncate (:594-621) and length_to_mask (dataio/dataio.py:661-706); forward only ----
 * logits (B,t_pred) f32, targets (B,t_tgt) f32; the longer of the two is truncated when |t_pred - t_tgt| <=
 * allowed_len_diff, otherwise SVT_ERR_INVALID with the reference's message.  rel_len (B,) f32 relative lengths or
 * NULL; pos_weight: device pointer to ONE float or NULL.  reduction: 0 mean, 1 batchmean, 2 batch ((B,) outputs),
 * 3 none ((B,T) masked per-frame losses).  workspace: batch*24+8 bytes of device memory. */
int svt_bce_loss(const float* logits_dev, int64_t batch, int64_t t_pred, const float* targets_dev, int64_t t_tgt,
                 const float* rel_len_dev, const float* pos_weight_dev, int32_t allowed_len_diff, int32_t reduction,
                 float* out_dev, void* workspace_dev, size_t workspace_bytes, int device, void* stream);
/* log_probs (B,t_pred,n_class) f32, targets (B,t_tgt) i64 (-100 = ignored, as torch.nn.functional.nll_loss).  After the
 * call the int32 at workspace + batch*24 is non-zero if a target was outside [0, n_class). */
int svt_nll_loss(const float* log_probs_dev, int64_t batch, int64_t t_pred, int32_t n_class, const int64_t* targets_dev,
                 int64_t t_tgt, const float* rel_len_dev, float label_smoothing, int32_t allowed_len_diff,
                 int32_t reduction, float* out_dev, void* workspace_dev, size_t workspace_bytes, int device, void* stream);
/* y = softmax(x) or log_softmax(x) over the last axis of (rows, n): replaces speechbrain.nnet.activations.Softmax
 * (activations.py:22-75) as the recipes use it (hparams log_softmax, apply_log=True) */
int svt_softmax(const float* x_dev, int64_t rows, int32_t n, int32_t apply_log, float* y_dev, int device, void* stream);

/* ---- head-only training step: the linear-probe stage of the recipes (MIR_ST500/train_audio_ssl.py:192-199, encoder frozen) ----
 * Every reduction has a fixed order (no float atomics, no inter-workgroup flags): two calls on the same inputs give the same bits.
 * Workspace convention of these three: *workspace_bytes is in / out; with workspace_dev == NULL the call stores the size it needs
 * there and returns SVT_OK without touching the device; otherwise a smaller *workspace_bytes is SVT_ERR_WORKSPACE.
 *
 * The recipe's objective (train_audio_ssl.py:50-76) and its gradient in one pass over logits (B,t_pred,n_out) f32, columns
 * [onset, offset, octave x (pitch_octave_num+1), class x the rest], n_out <= 32: BCE with logits on onset (pos_weight
 * onset_pos_weight) and offset, log-softmax + NLL on octave and class (label_smoothing as compute_masked_loss), each reduced "mean"
 * under the mask (float)t < rel_len[b]*T after truncating to T = min(t_pred, t_tgt) (|t_pred - t_tgt| <= allowed_len_diff, else
 * SVT_ERR_INVALID with the reference's message).  Targets (B,t_tgt): onset / offset f32, octave / class i64 (-100 ignored);
 * rel_len (B,) f32 or NULL.  terms_dev[5] = {onset, offset, octave, class, their sum}, each equal to svt_bce_loss / svt_nll_loss
 * (reduction 0) on the same inputs; dlogits_dev (B,t_pred,n_out) = d(sum)/d(logits), exactly 0 on masked and truncated frames.
 * terms_host (5 floats, may be NULL) receives the terms too.  This call synchronises `stream` (the target range is checked on the
 * device): a target outside [0, n_classes) that is not -100 gives SVT_ERR_INVALID. */
int svt_amt_objective_grad(const float* logits_dev, int64_t batch, int64_t t_pred, int32_t n_out, int32_t pitch_octave_num,
                           const float* onset_targets_dev, const float* offset_targets_dev, const int64_t* octave_targets_dev,
                           const int64_t* class_targets_dev, int64_t t_tgt, const float* rel_len_dev, float onset_pos_weight,
                           int32_t allowed_len_diff, float label_smoothing, float* terms_dev, float* terms_host, float* dlogits_dev,
                           void* workspace_dev, size_t* workspace_bytes, int device, void* stream);
/* Weight gradient of a Linear layer whose input is frozen: dweight (out_features, in_features) = dy^T x and dbias (may be NULL) =
 * sum over rows of dy, x (rows, in_features) f32, dy (rows, out_features) f32; out_features in 1..32, in_features a multiple of 4,
 * x / dweight / workspace 16-byte aligned.  Overwrites (does not accumulate into) dweight / dbias.  No dx. */
int svt_linear_backward(const float* x_dev, const float* dy_dev, int64_t rows, int32_t in_features, int32_t out_features,
                        float* dweight_dev, float* dbias_dev, void* workspace_dev, size_t* workspace_bytes, int device, void* stream);
/* The data half of a Linear layer's backward: dx (rows, in_features) = dy (rows, out_features) weight (out_features, in_features), all
 * f32; in_features a multiple of 4, weight / dx 16-byte aligned.  Overwrites dx. */
int svt_linear_backward_data(const float* dy_dev, const float* weight_dev, int64_t rows, int32_t in_features, int32_t out_features,
                             float* dx_dev, int device, void* stream);
/* torch.nn.utils.clip_grad_norm_ over n_tensors (<= 32) f32 gradient tensors -- total = ||[||g_i||]||, every g_i *= min(max_norm /
 * (total + 1e-6), 1) in place -- when max_norm > 0, then torch.optim.Adadelta's update of each parameter (single-tensor form, torch's
 * order of operations; maximize / weight_decay as torch).  All pointer arrays are HOST arrays of device pointers, numels a host array.
 * total_norm_dev (one float, may be NULL) receives the pre-clip total norm. */
int svt_clip_adadelta_step(int32_t n_tensors, float* const* params_dev, float* const* grads_dev, float* const* square_avg_dev,
                           float* const* acc_delta_dev, const int64_t* numels, float lr, double rho, float eps, float weight_decay,
                           int32_t maximize, float max_norm, float* total_norm_dev, void* workspace_dev, size_t* workspace_bytes,
                           int device, void* stream);
/* clip_grad_norm_ (when max_norm > 0, as svt_clip_adadelta_step: total_norm_dev, may be NULL, receives the pre-clip norm and every
 * gradient is scaled in place) then torch.optim.Adam's single-tensor update of n_tensors >= 1 contiguous f32 tensors -- any number: the
 * tensor table travels in the workspace, not in kernel arguments.  flags: SVT_ADAM_MAXIMIZE | SVT_ADAM_AMSGRAD (max_exp_avg_sq_dev is
 * then required, else it must be NULL) | SVT_ADAM_DECOUPLED (AdamW: p *= 1 - lr * weight_decay, nothing added to the gradient).  The
 * pointer arrays, numels, step_size (lr / (1 - beta1^step) per tensor) and bc2_sqrt (sqrt(1 - beta2^step) per tensor) are HOST arrays;
 * the bias corrections are per tensor because a parameter whose gradient was None in some step has a smaller step.  Alignment: every
 * tensor pointer may be ANY 4-byte-aligned address (a view into a flat buffer); 16-byte accesses are used where the arrays of a tensor
 * share one offset from a 16-byte boundary.  A tensor of 0 elements is skipped (its pointers may be NULL).  Workspace: the size-query
 * convention (workspace_dev NULL -> *workspace_bytes), 16-byte aligned.  No host-device synchronisation, no copy on the stream; two
 * calls on equal inputs at equal addresses give equal bits. */
#define SVT_ADAM_MAXIMIZE 1
#define SVT_ADAM_AMSGRAD 2
#define SVT_ADAM_DECOUPLED 4
int svt_clip_adam_step(int32_t n_tensors, float* const* params_dev, float* const* grads_dev, float* const* exp_avg_dev,
                       float* const* exp_avg_sq_dev, float* const* max_exp_avg_sq_dev, const int64_t* numels, const float* step_size,
                       const float* bc2_sqrt, double lr, double beta1, double beta2, double eps, double weight_decay, int32_t flags,
                       float max_norm, float* total_norm_dev, void* workspace_dev, size_t* workspace_bytes, int device, void* stream);

/* Fused attention kernel alone (bf16, head_dim 64 or 128): o[b,t,h*dh+d] = softmax(scale q k^T) v with q rows at
 * q + (b*t_len + t)*ldq + h*dh, k / v rows likewise with ldkv, o with ldo (element strides).  Replaces the eager
 * attention of transformers' Wav2Vec2Attention / torch.nn.MultiheadAttention inside the encoder and the RCA layers
 * (N20EMv2/audio_visual/fusion.py:102-117); exposed for the parity tests and tools/attn_bench.py. */
int svt_debug_attention(int32_t precision, const void* q, const void* k, const void* v, void* o, int32_t batch, int32_t t,
                        int32_t heads, int32_t head_dim, int64_t ldq, int64_t ldkv, int64_t ldo, float scale, int device,
                        void* stream);
/* The same kernel with WavLM's gated relative position bias (operand-type q / k / v / o, head_dim 64):
 * score(b, h, q, key) = scale q.k + gate[b, h, q] * pos_bias[h, key - q + t - 1], gate_dev (batch, heads, t) f32, pos_bias_dev
 * (heads, 2 t - 1) f32.  The bias row of a head stays in LDS: a t with 2 t - 1 > 8192 is refused (SVT_ERR_INVALID, nothing is launched).
 * Exposed for tests/test_gpu_attention.py: the encoder reaches these kernels only through a whole WavLM forward. */
int svt_debug_attention_bias(const void* q, const void* k, const void* v, void* o, int32_t batch, int32_t t, int32_t heads, int64_t ldq,
                             int64_t ldkv, int64_t ldo, float scale, const float* gate_dev, const float* pos_bias_dev, int device,
                             void* stream);
/* The fused attention with the dropout mask inside (csrc/attention_drop.hip), ONE launch of launch_flash_attention_dropout on caller
 * buffers: o = (keep * float(1 / (1 - p)) * softmax(scale q k^T)) v in HF's eager order (softmax -> dropout -> . v; the row sum runs
 * over all keys), operands and strides as for svt_debug_attention (16-bit q / k / v / o of the build's operand type).  Element
 * (b, h, i, j) of the probabilities has the logical index e0 + ((b*heads + h)*t + i)*t + j and is kept by svt_dropout's rule for site 2
 * of `layer` at (seed, step); e0 lets a small case reach q_hi != 0 and every alignment of the four-word groups.  precision must be
 * SVT_PREC_BF16 and head_dim 64 or 128, p in [0, 1): anything else is refused (SVT_ERR_INVALID) and nothing is launched.
 * svt_debug_set(38, 0) says which kernel ran.  struct_size = the size of the structure.  tests/test_gpu_attention_dropout.py */
typedef struct svt_debug_attention_dropout_desc {
  int32_t struct_size;
  int32_t precision;
  const void* q;
  const void* k;
  const void* v;
  void* o;
  int64_t ldq;
  int64_t ldkv;
  int64_t ldo;
  int32_t batch;
  int32_t t;
  int32_t heads;
  int32_t head_dim;
  float scale;
  uint32_t step;
  double p;
  uint64_t seed;
  int32_t layer;
  int32_t reserved;
  uint64_t e0;
} svt_debug_attention_dropout_desc;
int svt_debug_attention_dropout(const svt_debug_attention_dropout_desc* d, int device, void* stream);
/* The fused attention in both directions on caller buffers (csrc/attention_bf16.hip, attention_drop.hip, attention_bwd.hip), for a
 * caller that trains through it (svt_speechbrain_amd/attention.py wraps the pair in a torch.autograd.Function).  All tensors are in the
 * build's 16-bit operand type; precision must be SVT_PREC_BF16 and head_dim 64.  Rows: q at q + (b*t + i)*ldq + h*head_dim, k / v with
 * ldkv, o with ldo, d_o (the gradient of o; `do` is a C keyword) with lddo, dq with lddq, dk / dv with lddkv (element strides, multiples
 * of 8; every pointer 16-byte aligned).  dq / dk / dv have row strides of their own so that the three can land in one packed
 * (batch*t, 3*heads*head_dim) buffer, the dY operand of a packed q|k|v projection's backward.
 *   o = (keep * s * softmax(scale q k^T)) v, s = float(1 / (1 - p)), keep = svt_dropout's mask of site 2 in `layer` at (seed, step),
 *   element e0 + ((b*heads + h)*t + i)*t + j (HF eager order: softmax -> dropout -> . v).  p == 0: no mask is drawn, the plain kernels.
 * svt_attention_forward reads q, k, v and writes o (d_o, dq, dk, dv are ignored): launch_flash_attention at p == 0,
 * launch_flash_attention_dropout at p > 0.  svt_attention_backward reads q, k, v, o (as the forward stored it), d_o and writes dq, dk, dv:
 * three launches (row log-sum-exp and delta_i = d_o_i . o_i into the workspace, then dq, then dk and dv), deterministic -- no atomics, two
 * calls give the same bytes -- and without any (batch, heads, t, t) tensor.  workspace convention of svt_amt_objective_grad (workspace_dev
 * NULL: the size is stored in *workspace_bytes and nothing else happens).  Refused with SVT_ERR_INVALID and a message, nothing launched:
 * a struct_size other than the structure's, a precision other than SVT_PREC_BF16, head_dim other than 64 (the forward: 64 or 128), p
 * outside [0, 1), strides that are no multiples of 8, misaligned pointers.  svt_debug_set(46, 0) says which form the last backward ran. */
typedef struct svt_attention_desc {
  int32_t struct_size;
  int32_t precision;
  const void* q;
  const void* k;
  const void* v;
  void* o;
  const void* d_o;
  void* dq;
  void* dk;
  void* dv;
  int64_t ldq;
  int64_t ldkv;
  int64_t ldo;
  int64_t lddo;
  int64_t lddq;
  int64_t lddkv;
  int32_t batch;
  int32_t t;
  int32_t heads;
  int32_t head_dim;
  float scale;
  uint32_t step;
  double p;
  uint64_t seed;
  int32_t layer;
  int32_t reserved;
  uint64_t e0;
} svt_attention_desc;
int svt_attention_forward(const svt_attention_desc* d, int device, void* stream);
int svt_attention_backward(const svt_attention_desc* d, void* workspace_dev, size_t* workspace_bytes, int device, void* stream);
/* The score-matrix attention alone (tests/test_gpu_attention_scores.py): what every attention outside the fused kernels' reach runs --
 * the fp32 parity mode, 16-bit head sizes other than 64 / 128, WavLM's biased attention at head size 128 or 2 t - 1 > 8192, WavLM in the
 * split-operand modes.  Two batched products (scale q k^T into fp32 scores with rows padded to a multiple of 8 keys, P V) around the
 * bias add, the row softmax and the transpose of V.  precision 0 .. 3; q / k / v / o in the storage type of the precision (16-bit for
 * SVT_PREC_BF16, fp32 otherwise), addressed as for svt_debug_attention; gate_dev (batch, heads, t) / pos_bias_dev (heads, 2 t - 1) f32 as
 * for svt_debug_attention_bias, or both NULL.  The hook allocates the scores, the probabilities and V^T, fills them with 0xFF bytes (the
 * encoder's workspace is uninitialised: a pad the kernels fail to write shows up as NaN), synchronises and frees.  A geometry the fused
 * kernels serve is refused (SVT_ERR_INVALID, nothing is launched): this hook reaches the score-matrix path only. */
int svt_debug_attention_scores(int32_t precision, const void* q, const void* k, const void* v, void* o, int32_t batch, int32_t t,
                               int32_t heads, int32_t head_dim, int64_t ldq, int64_t ldkv, int64_t ldo, float scale,
                               const float* gate_dev, const float* pos_bias_dev, int device, void* stream);
/* The RCA training kernels alone (tests/test_gpu_fusion_train.py), precision 0 (fp32) or 1 (bf16 operands); workspace convention of
 * svt_linear_backward.  svt_debug_rca_wgrad: dw (n_out, n_in) = sum over the rows of one or two segments of dy_s^T x_s (dy f32 with row
 * strides ldy_s, x operand type (rows, n_in); dy1 / x1 NULL for one segment), db (may be NULL) = the column sums of dy.
 * svt_debug_rca_attn_bwd: for qkv (B*t, 3D) = [q_s | k | v] and qc (B*t, D) in the operand type, the attention outputs o_self / o_cross
 * and d(blend) (B*t, D) f32 with d o_self = alpha d blend, d o_cross = (1 - alpha) d blend: dqkv (B*t, 3D) = [dq_s | dk | dv] and
 * dqc (B*t, D), f32; head_dim 64 or 128. */
int svt_debug_rca_wgrad(int32_t precision, const float* dy0, int64_t ldy0, const void* x0, const float* dy1, int64_t ldy1, const void* x1,
                        int64_t rows, int32_t n_out, int32_t n_in, float* dw, float* db, void* workspace_dev, size_t* workspace_bytes,
                        int device, void* stream);
int svt_debug_rca_attn_bwd(int32_t precision, const void* qkv, const void* qc, const void* o_self, const void* o_cross,
                           const float* dblend, float alpha, int32_t batch, int32_t t, int32_t heads, int32_t head_dim, float* dqkv,
                           float* dqc, void* workspace_dev, size_t* workspace_bytes, int device, void* stream);
/* Diagnostics switches of the contraction kernels (tools/gemm_bench.py, tools/gemm_trace.py; never needed in production), by key:
 * 0 = kernel ablation variant, 1 = force the tile height (64/128/192/256), 2 = force the one-tile (2) / persistent (4) scheduler,
 * 3 = ablation variant while tracing (50-79: force gemm_pps_kernel), 5 = retired (the fused out-projection + LayerNorm kernel of
 * rounds 1-2), 6 = small-problem kernel (gemm_skinny.hip) on/off, 7 = its eligibility threshold in 128x256 tiles, 8 = 8-wave
 * fused-attention workgroups on/off, 9 = bf16 (1) or fp32 (0) convolution output in front of the conv-stack LayerNorm in bf16 mode,
 * 10 = retired (the whole-head fused attention kernel), 11 = LDS-DMA split-operand GEMM kernel on/off (off: the register-staged one),
 * 12 = svt_debug_gemm keeps the split copy of its weight between calls, 13 = page-guarded device allocations (see svt_debug_alloc),
 * 15 = slot-stamp form of the split-operand GEMM kernels (DIAG builds, tools/gemm_trace.py --x3-slots), 16 = retired (the eight-barrier
 * schedule of gemm_pps_kernel), 18 = retired (tile stamps of the lockstep attention kernel), 19 = split-operand modes keep product
 * operands as pair rows written by their producers (1, default) or as fp32 cut inside the product kernels (0: the round-2/3 path, A/B),
 * 20 = (hi, lo) LayerNorm with two rows per wave (1, default) or one (0), 21 = retired (A/B arms of the fused attention: only 0 and 3,
 * the staggered kernel, are accepted), 22 = conv layer 0 on the matrix pipe in the 16-bit modes (1, default) or on the vector ALU (0),
 * 23 = stage 1 of the lip front-end on the frame-resident direct convolution (1, default; conv3x3_c64.hip) or on the GEMM kernels (0),
 * 24 = query: returns the number of direct-convolution launches of this process so far (value ignored), 25 = timing-ablation bits of the
 * direct convolution (DIAG builds), 26 = stem + max-pool of the lip front-end as one persistent kernel (1, default) or as two kernels (0),
 * 27 = stage 2's 1x1 stride-2 downsample inside conv1's product (1, default) or as its own product (0), 28 = retired (the two-slot
 * schedule of gemm_pps_kernel: only 0 is accepted), 29 = gemm_p1w_kernel (one wave per SIMD) for the 16-bit products it measured faster
 * on (1, default), everywhere (2) or never (0), 30 = gemm_p1x_kernel (the same loop for the split-operand products on pair rows: 1; DIAG
 * builds only) or gemm_x3q_kernel (0, default: same bits, same speed), 31 = query: returns the number of device buffers this process has
 * FREED so far (value ignored; uploads and re-uploads must not free: tests/test_gpu_uploads.py), 32 = the tickets of the three ordered
 * cross-workgroup sums as acquire-release atomics (1) or relaxed ones behind write-through stores (0, default: stats.hip,
 * last_workgroup; same bits, tests/test_gpu_statistics.py), 33 = the small-problem GEMM uses 32 x 32 tiles while its 64 x 64 tiling has
 * at most this many workgroups (96, default; swept on the one-utterance forward: 150 / 200 / 1000 are 1.5-4.5 % slower), 34 = the
 * persistent 16-bit GEMM kernels' tile walk: -1 (default) chosen per launch, 0 = n fastest, n > 0 = panels of n tile rows (common.h,
 * tile_walk; same bits), 35 = the kernel-3 convolutions' K slabs tap-minor (1, default: the frame two neighbouring output rows share is
 * re-read out of L2) or tap-major (0) on gemm_p1w_kernel, 36 = FFN-2 of a small batch (<= 2048 rows) as a K-split small GEMM whose
 * partial products the following LayerNorm adds (1, default) or as one product (0), 37 = workgroups of a persistent GEMM launch (8 .. 256,
 * a multiple of 8; 256 = one per CU, default) of gemm_pps_kernel, gemm_p1w_kernel, gemm_x3p_kernel, gemm_x3q_kernel and gemm_p1x_kernel
 * (gemm_pers_kernel always launches one per CU): with few workgroups a small product gives each of them several tiles, 38 = query:
 * returns the id of the fused attention kernel the last attention launch of
 * this process chose (value ignored; 0 = none yet): 1 = flash_attn_kernel<64>, 2 = flash_attn_kernel<128>, 3 = flash_attn_stag_kernel<64>
 * (head_dim 64, "wide" launches), 4 = flash_attn_kernel<64, true> (position bias), 5 = flash_attn_kernel<64, true, 8> (position bias,
 * wide), 6 = flash_attn_x3_kernel<64, .>, 7 = flash_attn_x3_kernel<128, .>, 8 = flash_attn_x3_stag_kernel<.> (split-operand modes;
 * tests/test_gpu_attention.py asserts the id of every case), 9 = flash_attn_drop_kernel<64, 4>, 10 = flash_attn_drop_kernel<128, 4>
 * (the dropout mask inside; tests/test_gpu_attention_dropout.py), 11 = not assigned (kept for an eight-wave flash_attn_drop_kernel<64, 8>,
 * which is not built: DESIGN.md section 4.51), 39 = query: svt_debug_set(39, 0) returns which kernel the last dense product of this
 * process ran on (value ignored; 0 = none yet) as 1000 * family + tile rows: family 1 = gemm_skinny_kernel (32 / 64), 2 = the register-staged
 * gemm_kernel (128, or 256 for its 256 x 64 form; + 10000 for a split-operand instantiation), 3 = gemm_pp8_kernel (64 / 128 / 192 /
 * 256), 4 = gemm_pers_kernel, 5 = gemm_pps_kernel, 6 = gemm_p1w_kernel, 7 = gemm_x3s_kernel (256; 192 names its 192-column form),
 * 8 = gemm_x3p_kernel, 9 = gemm_x3q_kernel, 10 = gemm_p1x_kernel (tests/test_gpu_gemm_kernels.py and tests/test_gpu_gemm.py assert
 * the id of every case), 40 = query: returns which kernel the last row LayerNorm launch of this process chose (value ignored; 0 = none
 * yet; set on the host by every branch of the three launchers of csrc/layernorm.hip) as 1000 * kernel + instantiation:
 * 1000 + 10 * (16-bit x) + (16-bit yT) = layernorm_kernel<float, float> 1000, <float, 16-bit> 1001, <16-bit, 16-bit> 1011;
 * 2000 + 100 * PK + 10 * (16-bit x) + (16-bit yT) = layernorm_f32_vec_kernel<VPT, float> 2000, <VPT, 16-bit> 2001, <VPT, 16-bit, 16-bit>
 * 2011, <VPT, float, float, 2> 2200 (pair rows, bf16 pieces), <VPT, float, float, 3> 2300 (pair rows, IEEE-half pieces);
 * 3000 = layernorm_op16_rows2_kernel; 4000 = layernorm_hilo_kernel; 5000 = layernorm_hilo2_kernel, 5001 = its PARTS instantiation;
 * 6000 = layernorm_f32_to_hilo_kernel (tests/test_gpu_layernorm.py asserts the id of every case), 41 = query: returns which kernel of
 * the waveform front end the last launch of this process chose (value ignored; 0 = none yet; set on the host by every branch of the seven
 * launchers of csrc/stats.hip, csrc/conv0.hip and csrc/conv0_mfma.hip) as 100 * kernel + 10 * PK + (16-bit rows out):
 * 100 = moments_kernel; 200 = conv0_window_moments_kernel; 300 = conv0_group_coef_kernel; conv0_group_apply_kernel<float> 400,
 * <16-bit> 401, <float, 2> 420, <float, 3> 430; conv0_layer_kernel<float> 500, <16-bit> 501, <float, 2> 520, <float, 3> 530;
 * conv0_mfma_kernel<0, 0> 601 (with conv0_coef_exp_kernel and conv0_table_kernel<0> in front of it), <0, 2> 620, <0, 3> 630;
 * conv0_mfma_kernel<1, 0> 701 (with conv0_table_kernel<0>), <1, 2> 720, <1, 3> 730 (tests/test_gpu_conv0.py asserts the id of every case),
 * 42 = query: returns which padding kernel the last lip front-end call of this process launched (value ignored; 0 = none yet; set on the
 * host by every branch of the three launchers of csrc/video.hip) as 100 * family + form: family 1 = video_pad*_kernel (float input),
 * 2 = video_pad*_u8_kernel (svt_video_forward_u8), 3 = video_pad*_u8_clips_kernel (svt_video_forward_u8_clips); form 0 = the generic
 * kernel writing fp32, 1 = the generic kernel writing 16-bit, 2 = the 8-pixels-per-16-byte-store kernel of the 16-bit modes
 * (tests/test_gpu_video_train.py asserts the id of every case), 43 = query: returns which kernels the last step of the lip front-end
 * launched in this process (value ignored; 0 = none yet; set on the host by every branch of the launchers of csrc/video.hip and, for a
 * BasicBlock, by video_block of csrc/api_video.hip; a forward leaves its last block's or pooling launch's id): 100 =
 * conv3d_front_f32_kernel, 101 = conv3d_front_bf16_kernel (the 16-bit stem alone), 300 = conv3d_front_pool_kernel (stem + max-pool);
 * 200 = maxpool_3x3s2_kernel<float>, 201 = maxpool_3x3s2_kernel<16-bit>, 202 = maxpool_3x3s2_bf16x8_kernel; 400 = zero_halo_kernel;
 * 600 = avgpool_interior_kernel<float>, 601 = <16-bit>; a BasicBlock 5000 + 100 * conv1 + 10 * downsample + conv2 with the codes
 * 0 = none (downsample of a block that has none), 1 = conv3x3_c64_kernel, 2 = conv3x3_c128_kernel, 3 = grouped product G = 2,
 * 4 = grouped product G = 4, 5 = plain product, 6 = the combined conv1 + downsample product (conv1 and downsample both 6); for the
 * product launches key 39 names the GEMM kernel of the block's last product (tests/test_gpu_video_kernels.py asserts the id of every
 * case), 44 = query: returns which dropout kernel the last launch of csrc/dropout.hip in this process chose (value ignored; 0 = none
 * yet): 1 = dropout_rows_kernel<float>, 2 = dropout_rows_kernel<16-bit>, 3 = dropout_hilo_kernel, each + 10 for its element-by-element
 * instantiation (e0 % 4 != 0 or a pointer that is not 16-byte aligned); 4 = softmax_dropout_kernel<float>, 5 = <16-bit>
 * (tests/test_gpu_dropout_kernels.py asserts the id of every case), 45 = query: returns which kernel the last launch of the encoder's
 * glue chose in this process (value ignored; 0 = none yet; set on the host by every branch of five launchers of csrc/encoder_ops.hip
 * and by positional_conv of csrc/api_encoder.hip): launch_posconv_gather 11 = posconv_gather_kernel<float>, 12 = posconv_gather_kernel<16-bit>
 * (element by element), 13 = posconv_gather_bf16x8_kernel (8 channels per thread); launch_posconv_scatter_add 21 =
 * posconv_scatter_add_kernel<float> (split modes), 22 = <16-bit>; launch_relpos_table 30 = relpos_table_kernel; launch_relpos_gate 41 =
 * relpos_gate_vec_kernel<float>, 42 = <16-bit>, 43 = relpos_gate_kernel<float> (one thread per head: head sizes whose eighth is no power of
 * two), 44 = <16-bit>; a whole positional conv 1000 * form + 100 * gather + 10 * scatter with form 1 = plain (one grouped product with the
 * residual in its epilogue), 2 = multi-frame, 3 = the data2vec stack, gather 1 .. 3 and scatter 0 (none) .. 2 the last digits above; key 39
 * names the product's kernel (tests/test_gpu_encoder_glue.py asserts the id of every case), 46 = query: returns which form the last
 * attention backward of this process launched (value ignored; 0 = none yet; csrc/attention_bwd.hip): 1 = plain (attn_bwd_prep_kernel,
 * attn_bwd_dq_kernel<false>, attn_bwd_dkv_kernel<false>), 2 = masked (attn_bwd_prep_kernel, attn_bwd_dq_kernel<true>,
 * attn_bwd_dkv_kernel<true>: p > 0) (tests/test_gpu_attention_backward.py asserts the id of every case).
 * Returns 0 (keys 24, 31: the count; keys 38, 39, 40, 41, 42, 43, 44, 45, 46: the id), SVT_ERR_INVALID for an unknown key or a value a key does not accept (21, 28, 30, 37 above). */
int svt_debug_set(int key, int value);

/* ---- test hook: ONE step of a finalized lip front-end on caller-supplied device buffers; tests/test_gpu_video_kernels.py ----
 * The step runs with the handle's own uploaded weights (the BatchNorm folds, grouped matrices, fragment images and the combined
 * conv1 + downsample matrix of svt_video_finalize are inside the tested unit), through the same functions the forward calls, with the
 * forward's own choice of kernel; the stream is synchronised before the call returns.  Elements are fp32 for an fp32 / split-operand
 * handle and the build's 16-bit type otherwise; "haloed" = channels-last [F][H + 2][W + 2][C] with a one-pixel halo that the CALLER zeroes
 * (the kernels write interiors only).  H0 = (h - 1) / 2 + 1, H1 = (H0 - 1) / 2 + 1, likewise for widths.  `step`:
 *   1  the stem alone: launch_video_pad of the fp32 video `x` (B, 1, T, h, w) into scratch of the hook, then launch_conv3d_front ->
 *      out [B T][H0][W0][64].
 *   2  launch_maxpool_3x3s2: x [F][H][W][64] (H, W = H0, W0) -> the interior of the haloed out [F][H1 + 2][W1 + 2][64].
 *   3  pad as in step 1, then the fused launch_conv3d_front_pool -> the interior of the haloed out [B T][H1 + 2][W1 + 2][64].
 *   4  launch_zero_halo of out [F][H][W][C] (H, W = the PADDED sizes here).
 *   5  BasicBlock `b` of stage `li` over the haloed block input `x` [F][H + 2][W + 2][Cin]: conv1 -> t1, the 1x1 / 2 downsample of the first
 *      block of stages 1 .. 3 -> ds, the block's output -> out (all haloed, at the block's output size: (H - 1) / 2 + 1 where the block
 *      has stride 2).  svt_debug_set(43, 0) afterwards says which of them were written and by what.  As in the workspace, the combined
 *      conv1 + downsample product runs only when ds lies behind t1 at a multiple of 32 bytes (16-bit) -- carve both from one
 *      allocation.  The grouped product G = 4 reads ONE pixel (64 elements) behind the last frame of `x` and of t1, which the forward
 *      keeps zero behind its stage-1 buffers: the caller provides and zeroes it.
 *   6  launch_avgpool_interior: haloed x [F][H + 2][W + 2][512] -> out [F][512].
 * The padded operand of steps 1 and 3 is filled with 0xFF bytes before the pad launch: padding a pad kernel does not write is NaN.
 * workgroups: 0 = the launcher's choice; n > 0 caps the persistent grid of conv3x3_c64_kernel, conv3x3_c128_kernel and
 * conv3d_front_pool_kernel, so that a few frames give each workgroup several (ignored by the other kernels).
 * The hook never forces a path the forward would not take: svt_debug_set keys 23, 26 and 27 select the other arms, and step 3 refuses
 * where conv3d_front_pool_ok is false.  It is NARROWER than the launchers: it refuses (SVT_ERR_INVALID, nothing is launched) a wrong
 * struct_size, a NULL or unfinalized handle, step outside 1 .. 6, workgroups < 0, a NULL pointer where the step needs one (x, out; t1
 * for step 5; ds for a block with a downsample), ANY non-NULL pointer that is not 16-byte aligned, B < 1, T < 1, h < 8 or w < 8 (steps
 * 1, 3), a 16-bit stem whose five padded planes do not fit 160 KB of LDS (step 1), a geometry the fused kernel is not eligible for (step
 * 3), F < 1, H < 1 or W < 1 (steps 2, 4, 5, 6), H < 3, W < 3 or C outside {64, 128, 256, 512} (step 4), li outside 0 .. 3 or b outside
 * 0 .. 1 (step 5), more than 2e9 pixels.  A launcher's own refusal comes back as SVT_ERR_INVALID too.  struct_size = the size of the
 * structure. */
typedef struct svt_debug_video_desc {
  int32_t struct_size;
  int32_t step;
  int32_t B, T;
  int32_t h, w;
  int64_t F;
  int32_t H, W;
  int32_t C, li;
  int32_t b, workgroups;
  const void* x;
  void* t1;
  void* ds;
  void* out;
} svt_debug_video_desc;
int svt_debug_video_step(svt_video* v, const svt_debug_video_desc* d, void* stream);

/* ---- test hook: ONE step of a finalized encoder's glue on caller-supplied device buffers; tests/test_gpu_encoder_glue.py ----
 * The step runs with the handle's own uploaded weights (the weight-norm fold, the tap-major relayout, the multi-frame weight image, the
 * BatchNorm fold and the gate's row-sum fold of svt_encoder_finalize are inside the tested unit), through the same functions the forward
 * calls, with the forward's own choice of form and kernel; the stream is synchronised before the call returns.  `step`:
 *   1  positional_conv: `x` = h (B, T, D) fp32 -> `out` = h + pos_conv(h) (B, T, D) fp32.  The hook plans (B, n_samples) as a forward
 *      does and refuses unless the planned frame count is T (features-in mode, num_conv_layers = 0: n_samples = T); it fills the first
 *      svt_encoder_workspace_bytes(e, B, n_samples) bytes of `workspace` with 0xFF bytes (whatever the step reads without having written
 *      it is NaN), copies h into the plan's projection output, runs the step and copies its result out.  Which of the three forms ran --
 *      plain, multi-frame (B * ceil(T / Pf) >= 128 rows in the reduced modes), the data2vec stack -- is the plan's decision.
 *   2  launch_relpos_table: `out` = pb (heads, 2 T - 1) fp32 from the handle's rel_attn_embed, rel_pos_buckets and rel_pos_max_distance.
 *   3  launch_relpos_gate of layer `layer`: `x` = u (B T, D) in the handle's storage type (fp32 for an fp32 / split-operand handle, the
 *      build's 16-bit type otherwise) -> `out` = gate (B, heads, T) fp32.
 * svt_debug_set(45, 0) afterwards names the kernels, and for step 1 key 39 names the product's.  The hook never forces a form the forward
 * would not take.  It is NARROWER than the launchers: it refuses (SVT_ERR_INVALID, nothing is launched) a wrong struct_size, a NULL or
 * unfinalized handle, step outside 1 .. 3, a NULL pointer where the step needs one (out; x for steps 1 and 3; workspace for step 1),
 * ANY non-NULL pointer that is not 16-byte aligned, B < 1 or T < 1, a layer outside 0 .. num_layers - 1 (step 3), steps 2 and 3 on a
 * handle without rel_pos_buckets, a plan whose frame count is not T or a workspace_bytes below the plan's (step 1), more than 2^31
 * elements.  A launcher's own refusal comes back as SVT_ERR_INVALID too.  struct_size = the size of the structure. */
typedef struct svt_debug_encoder_desc {
  int32_t struct_size;
  int32_t step;
  int32_t B, T;
  int32_t layer, reserved;
  int64_t n_samples;
  const void* x;
  void* out;
  void* workspace;
  uint64_t workspace_bytes;
} svt_debug_encoder_desc;
int svt_debug_encoder_step(svt_encoder* e, const svt_debug_encoder_desc* d, void* stream);

/* ---- measurement hook: HIP-event timing of the dominant kernel on the stream it runs on ----
 * When enabled, forward calls bracket every launch of the dense contraction kernel with hipEvents on
 * the launch stream; svt_prof_read returns accumulated launches / milliseconds / algorithmic flops. */
/* on = 0: off; 1: a HIP-event pair around every dense-contraction / attention launch; n > 1: around every n-th one */
int svt_prof_enable(int on);
int svt_prof_reset(void);
/* kind: 0 = the dominant kernel family (svt::gemm_pps_kernel / gemm_pers_kernel / gemm_pp8_kernel: every large bf16
 * dense contraction; in the split-operand modes the split form of svt::gemm_kernel), 1 = the other dense contraction
 * kernels (exact-fp32 / small-shape GEMM), 2 = fused attention */
int svt_prof_read(int kind, int64_t* launches, double* total_ms, double* total_flops, double* total_bytes);
/* Clock stamps for a sustained-rate measurement (bench.py): enqueues a tiny kernel on `stream` that stores, per XCD x
 * (0..7), out_dev[2x] = s_memtime (shader-clock ticks) and out_dev[2x + 1] = s_memrealtime (100 MHz ticks) as int64.
 * Two calls around a region give the clock the chip HELD over it: d(memtime) / d(memrealtime) * 100 MHz, per XCD.
 * out_dev: 16 x int64, zeroed by the caller (an XCD that ran no block of the kernel leaves its pair untouched). */
int svt_debug_clock(int64_t* out_dev, int device, void* stream);
/* Diagnostics: a device buffer from the library's own allocator.  With svt_debug_set(13, 1 | 2) every allocation of the library
 * (these included) is its own mapping between two unmapped granules of address space, flush against the end (1) or the start (2)
 * of the mapping: an out-of-bounds access by a kernel on that side faults instead of landing in a neighbour
 * (tests/test_gpu_guard.py runs the forward passes with weights, workspace and inputs placed this way). */
int svt_debug_alloc(void** out, size_t bytes, int device);
/* Diagnostics (tools/determinism_stress.py): byte offsets of the regions svt_encoder_forward* carves out of the caller's workspace for
 * (batch, n_samples), in carve order -- 0 moments + ordered-sum scratch, 1 conv0 coefficients, 2 conv0 tables, 3 / 4 conv activations
 * (ping-pong), 5 fp32 conv output (layer-norm extractors), 6 projection input, 7 hF, 8 preF, 9 layer input, 10 fp32 residual, 11 low half
 * of the residual, 12 / 13 positional-conv operand / result, 14 QKV, 15 / 16 scores / probabilities (non-fused attention), 17 V transposed,
 * 18 QKV planes (split modes), 19 attention output, 20 FFN hidden, 21 gate, 22 relative-position bias, 23 head dots, 24 total.  A region the
 * configuration does not use has offset -1.  Writes min(n, 25) entries; returns the number written or a negative svt_status. */
int svt_debug_encoder_layout(const svt_encoder* e, int32_t batch, int64_t n_samples, int64_t* offsets, int n);
int svt_debug_free(void* p, int device);

#ifdef __cplusplus
}
#endif
#endif /* SVT_MI355_H */
