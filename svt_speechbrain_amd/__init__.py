"""svt_speechbrain_amd — MI355X-native singing-transcription forward path (drop-in for the hot path of
guxm2021/SVT_SpeechBrain; see DESIGN.md / INTEGRATION.md).  Importing the package never touches the GPU."""
from .config import EncoderConfig, PRESETS, config_from_source  # noqa: F401
from .huggingface_interface import HuggingFaceWav2Vec2  # noqa: F401
from .linear import Linear  # noqa: F401
from .fusion import FusionRCA  # noqa: F401
from .features import Fbank  # noqa: F401
from .decode import decode_frames, frame2note, frames2note, frames2note_batch, frames_to_info, ctc_greedy_decode, filter_ctc_output  # noqa: F401
from .amt import AMTForward  # noqa: F401
from . import losses  # noqa: F401
from . import checkpoints  # noqa: F401
from .checkpoints import Checkpointer  # noqa: F401
from .losses import bce_loss, nll_loss, Softmax  # noqa: F401
from . import video  # noqa: F401
from . import dataio, scoring  # noqa: F401
from .video import FairseqAVHubertPretrain, EvalTransform, TrainTransform, VideoClip, pad_roi_batch  # noqa: F401
from .song import (SongTranscriber, utterance_bounds, save_song_features, feature_path, song_video_features,  # noqa: F401
                   save_song_video_features, video_feature_path, noisy_wav_path, NoiseSweep)
from . import noise  # noqa: F401
from .noise import (SNRS_DB, compute_amplitude, mix_at_snrs, assemble_noise_track, split_natural_files, natural_keep,  # noqa: F401
                    babble_keep, babble_split, noise_pools, natural_pools, babble_pools)
from . import resample  # noqa: F401
from .resample import Resample, SpeedPerturb, resample_table, resample_to_mono  # noqa: F401
from . import augment  # noqa: F401
from .augment import notch_filter, drop_filter, DropFreq, DropChunk, TimeDomainSpecAugment  # noqa: F401
from . import spec_augment  # noqa: F401
from .spec_augment import compute_mask_indices  # noqa: F401
from . import dropout  # noqa: F401
from .dropout import draw_layerdrop  # noqa: F401
from . import audio_io  # noqa: F401
from .audio_io import info, load, save, read_audio, write_audio  # noqa: F401
from .dataio import read_utterance  # noqa: F401
from . import training  # noqa: F401
from .training import Adadelta, Adam, AdamW, LinearProbe, FusionTrainer, VideoProbe  # noqa: F401
from . import attention  # noqa: F401
from .attention import fused_attention, FusedSelfAttention  # noqa: F401

__all__ = ["EncoderConfig", "PRESETS", "config_from_source", "HuggingFaceWav2Vec2", "Linear", "FusionRCA", "Fbank",
           "decode_frames", "frame2note", "frames2note", "frames2note_batch", "frames_to_info", "ctc_greedy_decode", "filter_ctc_output", "AMTForward",
           "SongTranscriber", "utterance_bounds", "save_song_features", "feature_path", "song_video_features",
           "save_song_video_features", "video_feature_path", "EvalTransform", "TrainTransform", "VideoClip", "pad_roi_batch", "FairseqAVHubertPretrain",
           "Adadelta", "Adam", "AdamW", "LinearProbe", "FusionTrainer", "VideoProbe",
           "SNRS_DB", "compute_amplitude", "mix_at_snrs", "assemble_noise_track", "split_natural_files", "natural_keep", "babble_keep",
           "babble_split", "noise_pools", "natural_pools", "babble_pools", "noisy_wav_path", "NoiseSweep",
           "Resample", "SpeedPerturb", "resample_table", "resample_to_mono",
           "notch_filter", "drop_filter", "DropFreq", "DropChunk", "TimeDomainSpecAugment",
           "fused_attention", "FusedSelfAttention", "audio_io", "info", "load", "save", "read_audio", "write_audio", "read_utterance"]
