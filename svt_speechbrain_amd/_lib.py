"""ctypes binding of ``libsvt_mi355.so`` (C-ABI: ``include/svt_mi355.h``).

The HIP library is the product; there is NO CPU fallback.  Importing this module never touches the GPU,
but every compute entry point raises ``SvtError`` when the library is missing or no gfx950 device is
visible (SURVEY.md §8b error conventions: Python exceptions, never an abort).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
# SVT_LIB_PATH: load another build of the bf16 library (kernel experiments: tools/*_bench.py, bench.py); default = the in-tree one
LIB_PATH = os.environ.get("SVT_LIB_PATH") or os.path.join(_HERE, "libsvt_mi355.so")
MAX_CONV = 8


class SvtError(RuntimeError):
    pass


class EncoderConfigC(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32),
        ("hidden_size", C.c_int32),
        ("num_layers", C.c_int32),
        ("num_heads", C.c_int32),
        ("intermediate_size", C.c_int32),
        ("num_conv_layers", C.c_int32),
        ("conv_dim", C.c_int32 * MAX_CONV),
        ("conv_kernel", C.c_int32 * MAX_CONV),
        ("conv_stride", C.c_int32 * MAX_CONV),
        ("feat_extract_norm", C.c_int32),
        ("conv_bias", C.c_int32),
        ("stable_layer_norm", C.c_int32),
        ("feat_proj_layer_norm", C.c_int32),
        ("pos_conv_kernel", C.c_int32),
        ("pos_conv_groups", C.c_int32),
        ("layer_norm_eps", C.c_float),
        ("normalize_wav", C.c_int32),
        ("output_norm", C.c_int32),
        ("precision", C.c_int32),
        ("pos_conv_depth", C.c_int32),
        ("rel_pos_buckets", C.c_int32),
        ("rel_pos_max_distance", C.c_int32),
        ("pos_conv_batch_norm", C.c_int32),
    ]


class VideoTransformC(C.Structure):
    """svt_video_transform: ((u - sub0) / div0 - mean) / std in float64 on the centre crop_h x crop_w window of a uint8 lip ROI."""
    _fields_ = [("sub0", C.c_double), ("div0", C.c_double), ("mean", C.c_double), ("std", C.c_double), ("crop_h", C.c_int32), ("crop_w", C.c_int32)]


class VideoClipC(C.Structure):
    """svt_video_clip: one clip of svt_video_forward_u8_clips -- crop offsets, horizontal flip (0 / 1) and its number of real frames."""
    _fields_ = [("dy", C.c_int32), ("dx", C.c_int32), ("flip", C.c_int32), ("n_frames", C.c_int32)]


class GemmDescC(C.Structure):
    """svt_debug_gemm_desc: one batched launch of the dense product (svt_debug_gemm_batched); strides in elements."""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("a", C.c_void_p), ("w", C.c_void_p), ("c", C.c_void_p), ("bias", C.c_void_p), ("resid", C.c_void_p),
        ("m", C.c_int32), ("n", C.c_int32), ("k", C.c_int32),
        ("a_rpb", C.c_int32),
        ("a_bstride", C.c_int64), ("a_rstride", C.c_int64),
        ("ldw", C.c_int64), ("ldc", C.c_int64),
        ("nz", C.c_int32), ("nz2", C.c_int32),
        ("a_z1", C.c_int64), ("a_z2", C.c_int64), ("w_z1", C.c_int64), ("w_z2", C.c_int64), ("c_z1", C.c_int64), ("c_z2", C.c_int64),
        ("bias_z2", C.c_int64),
        ("alpha", C.c_float),
        ("act", C.c_int32), ("out_f32", C.c_int32),
    ]


class LayerNormDescC(C.Structure):
    """svt_debug_layernorm_desc: one launch of a row LayerNorm launcher (svt_debug_layernorm); form 0 / 1 / 2, device pointers."""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("form", C.c_int32),
        ("prec", C.c_int32), ("x_is_f32", C.c_int32),
        ("rows", C.c_int64),
        ("D", C.c_int32), ("gelu", C.c_int32),
        ("eps", C.c_float),
        ("pair_kind", C.c_int32),
        ("gamma", C.c_void_p), ("beta", C.c_void_p),
        ("x", C.c_void_p), ("yT", C.c_void_p), ("yF", C.c_void_p), ("add", C.c_void_p), ("sumF", C.c_void_p), ("yP", C.c_void_p), ("addP", C.c_void_p),
        ("branch", C.c_void_p), ("rh", C.c_void_p), ("rl", C.c_void_p), ("x32", C.c_void_p), ("yh", C.c_void_p), ("yl", C.c_void_p),
        ("parts", C.c_void_p), ("pbias", C.c_void_p),
        ("part_stride", C.c_int64),
        ("nparts", C.c_int32),
    ]


class DropoutC(C.Structure):
    """svt_dropout: the training-mode state of svt_encoder_set_dropout -- five rates, (seed, step) of the mask function, skipped layers,
    and the opt-in to the fused attention with the mask inside (fused_attention; the structure without its last 8 bytes is accepted
    and means 0)."""
    _fields_ = [
        ("struct_size", C.c_int32), ("step", C.c_uint32),
        ("feat_proj_dropout", C.c_double), ("hidden_dropout", C.c_double), ("attention_dropout", C.c_double),
        ("activation_dropout", C.c_double), ("layerdrop", C.c_double),
        ("seed", C.c_uint64), ("skip_mask", C.c_uint64),
        ("fused_attention", C.c_int32), ("reserved", C.c_int32),
    ]


class AttentionDropoutDescC(C.Structure):
    """svt_debug_attention_dropout_desc: one launch of the fused attention with the dropout mask inside (svt_debug_attention_dropout)."""
    _fields_ = [
        ("struct_size", C.c_int32), ("precision", C.c_int32),
        ("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("o", C.c_void_p),
        ("ldq", C.c_int64), ("ldkv", C.c_int64), ("ldo", C.c_int64),
        ("batch", C.c_int32), ("t", C.c_int32), ("heads", C.c_int32), ("head_dim", C.c_int32),
        ("scale", C.c_float), ("step", C.c_uint32),
        ("p", C.c_double), ("seed", C.c_uint64),
        ("layer", C.c_int32), ("reserved", C.c_int32),
        ("e0", C.c_uint64),
    ]


class AttentionDescC(C.Structure):
    """svt_attention_desc: the fused attention in both directions on caller buffers (svt_attention_forward / svt_attention_backward);
    d_o is the gradient of o (``do`` is a keyword in C)."""
    _fields_ = [
        ("struct_size", C.c_int32), ("precision", C.c_int32),
        ("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("o", C.c_void_p),
        ("d_o", C.c_void_p), ("dq", C.c_void_p), ("dk", C.c_void_p), ("dv", C.c_void_p),
        ("ldq", C.c_int64), ("ldkv", C.c_int64), ("ldo", C.c_int64), ("lddo", C.c_int64), ("lddq", C.c_int64), ("lddkv", C.c_int64),
        ("batch", C.c_int32), ("t", C.c_int32), ("heads", C.c_int32), ("head_dim", C.c_int32),
        ("scale", C.c_float), ("step", C.c_uint32),
        ("p", C.c_double), ("seed", C.c_uint64),
        ("layer", C.c_int32), ("reserved", C.c_int32),
        ("e0", C.c_uint64),
    ]


class DropoutDescC(C.Structure):
    """svt_debug_dropout_desc: one launch of a dropout kernel (svt_debug_dropout); form 0 / 1 / 2, device pointers."""
    _fields_ = [
        ("struct_size", C.c_int32), ("form", C.c_int32), ("prec", C.c_int32), ("site", C.c_int32), ("layer", C.c_int32), ("step", C.c_uint32),
        ("p", C.c_double), ("seed", C.c_uint64), ("e0", C.c_uint64), ("n", C.c_int64), ("rows", C.c_int64),
        ("T", C.c_int32), ("Tp", C.c_int32),
        ("x", C.c_void_p), ("xh", C.c_void_p), ("xl", C.c_void_p), ("S", C.c_void_p), ("P", C.c_void_p),
    ]


class Conv0DescC(C.Structure):
    """svt_debug_conv0_desc: one launch of a launcher of the waveform front end (svt_debug_conv0); form 0 .. 6, device pointers
    (tickets_out: a host pointer)."""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("form", C.c_int32),
        ("B", C.c_int32), ("C", C.c_int32),
        ("L", C.c_int64), ("T1", C.c_int64),
        ("k", C.c_int32), ("stride", C.c_int32),
        ("prec", C.c_int32), ("pair_kind", C.c_int32),
        ("cpg", C.c_int32), ("groups", C.c_int32),
        ("groups_max", C.c_int32), ("repeat", C.c_int32),
        ("n", C.c_int64), ("n_wav", C.c_int64),
        ("eps_wav", C.c_float), ("eps", C.c_float),
        ("x", C.c_void_p), ("wav", C.c_void_p), ("wav_mom", C.c_void_p), ("w0", C.c_void_p), ("b0", C.c_void_p), ("gamma", C.c_void_p),
        ("beta", C.c_void_p), ("mom", C.c_void_p), ("wm", C.c_void_p), ("coef", C.c_void_p), ("out", C.c_void_p),
        ("tickets_out", C.c_void_p),
    ]


class VideoStepDescC(C.Structure):
    """svt_debug_video_desc: one step of a finalized lip front-end on caller-supplied device buffers (svt_debug_video_step); step 1 .. 6."""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("step", C.c_int32),
        ("B", C.c_int32), ("T", C.c_int32),
        ("h", C.c_int32), ("w", C.c_int32),
        ("F", C.c_int64),
        ("H", C.c_int32), ("W", C.c_int32),
        ("C", C.c_int32), ("li", C.c_int32),
        ("b", C.c_int32), ("workgroups", C.c_int32),
        ("x", C.c_void_p), ("t1", C.c_void_p), ("ds", C.c_void_p), ("out", C.c_void_p),
    ]


class EncoderStepDescC(C.Structure):
    """svt_debug_encoder_desc: one step of a finalized encoder's glue on caller-supplied device buffers (svt_debug_encoder_step); step 1 .. 3."""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("step", C.c_int32),
        ("B", C.c_int32), ("T", C.c_int32),
        ("layer", C.c_int32), ("reserved", C.c_int32),
        ("n_samples", C.c_int64),
        ("x", C.c_void_p), ("out", C.c_void_p), ("workspace", C.c_void_p),
        ("workspace_bytes", C.c_uint64),
    ]


class WavInfoC(C.Structure):
    """svt_wav_info: what svt_wav_parse reads from a RIFF/WAVE header; format is a svt_pcm_format (U8 = 1 .. F64 = 6)."""
    _fields_ = [("format", C.c_int32), ("channels", C.c_int32), ("sample_rate", C.c_int32), ("bits_per_sample", C.c_int32),
                ("block_align", C.c_int32), ("data_offset", C.c_int64), ("frames", C.c_int64)]


class FrameC(C.Structure):
    _fields_ = [("p_on", C.c_float), ("p_off", C.c_float), ("octave", C.c_int32), ("pitch_class", C.c_int32)]


# every symbol include/svt_mi355.h declares: name -> (restype, argtypes)
_P = C.c_void_p
_I64P = C.POINTER(C.c_int64)
# svt_norm_reduce_fn (include/svt_mi355.h): int fn(double* sums_dev, int32_t n_doubles, void* stream, void* user)
NORM_REDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p)

SYMBOLS = {
    "svt_last_error": (C.c_char_p, []),
    "svt_abi_version": (C.c_int, []),
    "svt_device_count": (C.c_int, []),
    "svt_encoder_create": (C.c_int, [C.POINTER(EncoderConfigC), C.c_int, C.POINTER(_P)]),
    "svt_encoder_destroy": (None, [_P]),
    "svt_encoder_load_param": (C.c_int, [_P, C.c_char_p, _P, C.c_int, _I64P, C.c_int]),
    "svt_encoder_finalize": (C.c_int, [_P]),
    "svt_encoder_get_param": (C.c_int, [_P, C.c_char_p, _P, C.c_int64]),
    "svt_encoder_num_frames": (C.c_int64, [_P, C.c_int64]),
    "svt_encoder_workspace_bytes": (C.c_int64, [_P, C.c_int32, C.c_int64]),
    "svt_encoder_forward": (C.c_int, [_P, _P, C.c_int32, C.c_int64, _P, _P, C.c_size_t, _P]),
    "svt_encoder_forward_ex": (C.c_int, [_P, _P, C.c_int32, C.c_int64, _P, _P, C.c_size_t, _P, C.c_int32]),
    "svt_encoder_forward_head": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int64, _P, _P, C.c_int32, C.c_int32, _P, C.c_size_t, _P, C.c_int32]),
    "svt_linear_create": (C.c_int, [C.c_int32, C.c_int32, C.c_int, C.c_int, C.POINTER(_P)]),
    "svt_linear_destroy": (None, [_P]),
    "svt_linear_load": (C.c_int, [_P, _P, _P]),
    "svt_linear_forward": (C.c_int, [_P, _P, C.c_int64, _P, _P]),
    "svt_decode_frames": (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int, _P]),
    "svt_rca_create": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int32, C.c_int, C.POINTER(_P)]),
    "svt_rca_destroy": (None, [_P]),
    "svt_rca_load_param": (C.c_int, [_P, C.c_char_p, _P, C.c_int, _I64P, C.c_int]),
    "svt_rca_finalize": (C.c_int, [_P]),
    "svt_rca_workspace_bytes": (C.c_int64, [_P, C.c_int32, C.c_int32]),
    "svt_rca_forward": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, C.c_int32, _P, _P, C.c_size_t, _P]),
    "svt_rca_refresh_params": (C.c_int, [_P, C.POINTER(_P), C.c_int32, _P]),
    "svt_rca_train_workspace_bytes": (C.c_int64, [_P, C.c_int32, C.c_int32]),
    "svt_rca_forward_train": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, C.c_int32, _P, _P, C.c_size_t, _P]),
    "svt_rca_backward": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.POINTER(_P), _P, C.c_size_t, _P]),
    "svt_ctc_greedy": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, C.c_int, _P]),
    "svt_fbank_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "svt_fbank": (C.c_int, [_P, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                            C.c_float, C.c_float, C.c_float, _P, _P, C.c_size_t, C.c_int, _P]),
    "svt_noise_mix_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int32]),
    "svt_noise_mix": (C.c_int, [_P, _P, C.c_int64, C.POINTER(C.c_float), C.c_int32, _P, C.c_int64, _P, _P, C.c_int64, C.c_int, _P]),
    "svt_resample_output_samples": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    "svt_resample": (C.c_int, [_P, C.c_int32, C.c_int64, C.c_int64, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int64, C.c_int64,
                               C.c_int32, C.c_int, _P]),
    "svt_drop_freq_chunk": (C.c_int, [_P, C.c_int32, C.c_int64, C.c_int64, _P, C.c_int32, _P, C.c_int32, _P, C.c_int64, C.c_int, _P]),
    "svt_spec_augment": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int64, _P, _P, _P, C.c_int, _P]),
    "svt_encoder_set_spec_augment": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32]),
    "svt_encoder_set_dropout": (C.c_int, [_P, C.POINTER(DropoutC)]),
    "svt_debug_dropout": (C.c_int, [C.POINTER(DropoutDescC), C.c_int, _P]),
    "svt_debug_attention_dropout": (C.c_int, [C.POINTER(AttentionDropoutDescC), C.c_int, _P]),
    "svt_attention_forward": (C.c_int, [C.POINTER(AttentionDescC), C.c_int, _P]),
    "svt_attention_backward": (C.c_int, [C.POINTER(AttentionDescC), _P, C.POINTER(C.c_size_t), C.c_int, _P]),
    "svt_wav_parse": (C.c_int, [_P, C.c_int64, C.c_int64, C.POINTER(WavInfoC), _I64P]),
    "svt_wav_header": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int64, _P, C.c_int64, _I64P]),
    "svt_pcm_decode": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int64, _P, C.c_int64, C.c_int32, C.c_int, _P]),
    "svt_pcm_encode": (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int64, C.c_int32, _P, C.c_int, _P]),
    "svt_debug_gemm": (C.c_int, [C.c_int32, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64,
                                 C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int, _P]),
    "svt_debug_gemm_batched": (C.c_int, [C.c_int32, C.POINTER(GemmDescC), C.c_int, _P]),
    "svt_debug_layernorm": (C.c_int, [C.POINTER(LayerNormDescC), C.c_int, _P]),
    "svt_debug_conv0": (C.c_int, [C.POINTER(Conv0DescC), C.c_int, _P]),
    "svt_debug_video_step": (C.c_int, [_P, C.POINTER(VideoStepDescC), _P]),
    "svt_debug_encoder_step": (C.c_int, [_P, C.POINTER(EncoderStepDescC), _P]),
    "svt_debug_attention_scores": (C.c_int, [C.c_int32, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64,
                                             C.c_int64, C.c_float, _P, _P, C.c_int, _P]),
    "svt_debug_gemm_pairs": (C.c_int, [C.c_int32, _P, C.c_int64, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64,
                                       C.c_int64, C.c_int32, C.c_int32, C.c_int, _P, C.c_int32, C.POINTER(C.c_float)]),
    "svt_video_create": (C.c_int, [C.c_int32, C.c_int32, C.c_int, C.POINTER(C.c_void_p)]),
    "svt_video_destroy": (None, [C.c_void_p]),
    "svt_video_load_param": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.c_int]),
    "svt_video_finalize": (C.c_int, [C.c_void_p]),
    "svt_video_keep_workspace": (C.c_int, [C.c_void_p, C.c_int]),
    "svt_video_workspace_bytes": (C.c_int64, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "svt_video_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                    C.c_size_t, C.c_void_p]),
    "svt_video_forward_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int32,
                                       C.c_void_p, C.c_size_t, C.c_void_p]),
    "svt_video_forward_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(VideoTransformC),
                                       C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "svt_video_forward_u8_clips": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(VideoTransformC),
                                             C.POINTER(VideoClipC), C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "svt_deltas": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "svt_context_window": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int, C.c_void_p]),
    "svt_bce_loss": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                               C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
    "svt_nll_loss": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_float,
                               C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
    "svt_softmax": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int, C.c_void_p]),
    "svt_amt_objective_grad": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int64, _P, C.c_float,
                                         C.c_int32, C.c_float, _P, C.POINTER(C.c_float), _P, _P, C.POINTER(C.c_size_t), C.c_int, _P]),
    "svt_linear_backward": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, _P, _P, _P, C.POINTER(C.c_size_t), C.c_int, _P]),
    "svt_linear_backward_data": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, _P, C.c_int, _P]),
    "svt_clip_adadelta_step": (C.c_int, [C.c_int32, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), _I64P, C.c_float,
                                         C.c_double, C.c_float, C.c_float, C.c_int32, C.c_float, _P, _P, C.POINTER(C.c_size_t), C.c_int,
                                         _P]),
    "svt_clip_adam_step": (C.c_int, [C.c_int32, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), _I64P,
                                     C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_double, C.c_double, C.c_double, C.c_double,
                                     C.c_double, C.c_int32, C.c_float, _P, _P, C.POINTER(C.c_size_t), C.c_int, _P]),
    "svt_debug_attention": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                      C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_float, C.c_int, C.c_void_p]),
    "svt_debug_attention_bias": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64,
                                           C.c_int64, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "svt_debug_rca_wgrad": (C.c_int, [C.c_int32, _P, C.c_int64, _P, _P, C.c_int64, _P, C.c_int64, C.c_int32, C.c_int32, _P, _P, _P,
                                      C.POINTER(C.c_size_t), C.c_int, _P]),
    "svt_debug_rca_attn_bwd": (C.c_int, [C.c_int32, _P, _P, _P, _P, _P, C.c_float, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P,
                                         _P, C.POINTER(C.c_size_t), C.c_int, _P]),
    "svt_debug_set": (C.c_int, [C.c_int, C.c_int]),
    "svt_debug_clock": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "svt_debug_encoder_layout": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.POINTER(C.c_int64), C.c_int]),
    "svt_operand_type": (C.c_int, []),
    "svt_encoder_set_norm_reduce": (C.c_int, [_P, C.c_void_p, C.c_void_p, C.c_int64]),
    "svt_frames_to_notes": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_float, C.c_float, C.c_double, C.c_int32, C.c_int32,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "svt_debug_alloc": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t, C.c_int]),
    "svt_debug_free": (C.c_int, [C.c_void_p, C.c_int]),
    "svt_prof_enable": (C.c_int, [C.c_int]),
    "svt_prof_reset": (C.c_int, []),
    "svt_prof_read": (C.c_int, [C.c_int, _I64P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
}

_lib: Optional[C.CDLL] = None
_libs: dict = {}   # one handle per build of the library ("" = bf16 operands, "f16" = IEEE-half operands)


def load(variant: str = None) -> C.CDLL:
    """dlopen the in-tree library and bind every declared symbol; raises SvtError if it is missing.
    ``variant="f16"``: the IEEE-half build of the same sources (``libsvt_mi355_f16.so``, precision="fp16" of the modules)."""
    global _lib
    key = variant or ""
    if key in _libs:
        return _libs[key]
    if not variant and os.environ.get("SVT_LIB_SUFFIX"):   # diagnostics: an experimental build of the bf16 library (csrc/Makefile, XNAME)
        variant_path = LIB_PATH.replace("libsvt_mi355.so", f"libsvt_mi355_{os.environ['SVT_LIB_SUFFIX']}.so")
        if not os.path.exists(variant_path):
            raise SvtError(f"SVT_LIB_SUFFIX: {variant_path} not found")
        globals()["LIB_PATH"] = variant_path
    root, ext = os.path.splitext(LIB_PATH)   # only the file's suffix: the checkout may live under a directory with ".so" in its name
    path = LIB_PATH if not variant else f"{root}_{variant}{ext}"
    if not os.path.exists(path):
        raise SvtError(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C svt_speechbrain_amd/csrc`). The MI355X path has no CPU fallback.")
    lib = C.CDLL(path)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    if lib.svt_abi_version() != 1:
        raise SvtError(f"{os.path.basename(path)} ABI version mismatch")
    if lib.svt_operand_type() != (1 if variant == "f16" else 0):
        raise SvtError(f"{os.path.basename(path)} was built for another operand type")
    _libs[key] = lib
    if not variant:
        _lib = lib
    return lib


def last_error(lib: C.CDLL = None) -> str:
    return ((lib or load()).svt_last_error() or b"").decode("utf-8", "replace")


def check(rc: int, what: str = "", lib: C.CDLL = None) -> None:
    if rc != 0:
        raise SvtError(f"{what}: {last_error(lib)} (status {rc})")


def require_gpu() -> None:
    lib = load()
    if lib.svt_device_count() < 1:
        raise SvtError("no gfx950 (MI355X) device is visible: the HIP path cannot run and there is no CPU fallback")


def stream_ptr(device) -> int:
    import torch
    return int(torch.cuda.current_stream(device).cuda_stream)


def dev_index(device) -> int:
    import torch
    d = torch.device(device)
    if d.type != "cuda":
        raise SvtError(f"tensors must live on a ROCm device ('cuda:N'), got {d}")
    return d.index if d.index is not None else torch.cuda.current_device()


def ptr(t) -> int:
    return int(t.data_ptr())
