"""What tests/golden/make_golden_spec_augment.py and the SpecAugment tests share: the fixture's cases, its seeded input and digests.

The cases are the issue's: per HF tiny directory of tests/golden/local_ckpt/ a time mask alone (p 0.3, length 3), a feature mask alone
(p 0.2, length 2), both together, and HF's default fields on a waveform short enough for the span clamp.  B = 2 everywhere.  The clamp
(``num_masked_span * mask_length > sequence_length`` with length 10 and min_masks 2) needs fewer than 20 frames, i.e. fewer than 6 500
samples through the 320-sample hop: that case uses the 4 000 samples (12 frames) of the other tiny goldens, the rest 8 000 / 16 000.
The feature cases write ``mask_feature_min_masks`` (HF's default, 0) into config.json: transformers' WavLMConfig does not define the
field its own WavLMModel._mask_hidden_states reads, so without it the reference cannot draw a feature mask for WavLM at all.
"""
from __future__ import annotations

import hashlib

import torch

FAMILIES = ("tiny-wav2vec2-hf", "tiny-hubert-bn-hf", "tiny-wavlm-hf", "tiny-data2vec-hf")

# name -> (config.json fields, samples per clip, seed of numpy's generator and of the input)
CASES = {
    "time": (dict(mask_time_prob=0.3, mask_time_length=3, mask_feature_prob=0.0), 8000, 101),
    "feature": (dict(mask_time_prob=0.0, mask_feature_prob=0.2, mask_feature_length=2, mask_feature_min_masks=0), 8000, 102),
    "both": (dict(mask_time_prob=0.3, mask_time_length=3, mask_feature_prob=0.2, mask_feature_length=2, mask_feature_min_masks=0), 16000, 103),
    "clamp": (dict(), 4000, 104),   # HF's defaults: p 0.05, length 10, min_masks 2 -> 2 * 10 > 12 frames -> one span
}

# (shape, mask_prob, mask_length, min_masks, seed) of the mask-only table
MASK_ROWS = [
    ((2, 24), 0.0, 10, 0, 1),       # zero spans: all False, one draw (the epsilon) consumed
    ((2, 24), 0.05, 10, 0, 23),     # 0.12 + epsilon: zero or one span by the rounding
    ((2, 24), 0.05, 10, 0, 24),
    ((2, 12), 0.05, 10, 2, 3),      # the clamp: 2 * 10 > 12 -> 12 // 10 = 1
    ((2, 19), 0.65, 10, 2, 4),      # the clamp from the probability side
    ((2, 49), 0.05, 3, 4, 5),       # min_masks above the computed span count
    ((1, 49), 0.3, 3, 0, 7),        # B = 1
    ((2, 64), 0.2, 2, 0, 9),        # the (B, D) form, D = 64
    ((2, 64), 0.2, 2, 0, 21),
    ((2, 768), 0.2, 2, 0, 11),      # D = 768
    ((3, 768), 0.05, 10, 0, 12),
    ((2, 499), 0.05, 10, 2, 13),    # the 10 s clip, HF's defaults
    ((32, 499), 0.65, 10, 2, 14),   # ... and the pre-training probability on a full batch
    ((4, 24), 0.3, 3, 2, 15),
    ((2, 24), 1.0, 3, 0, 16),       # as many spans as fit
    ((2, 10), 0.5, 10, 1, 17),      # mask_length == sequence_length: one start to choose from
    ((3, 5), 0.9, 1, 0, 18),        # length 1
    ((2, 49), 0.3, 3, 2, 19),
    ((2, 12), 0.3, 3, 2, 20),
    ((5, 33), 0.4, 4, 1, 22),
]


def synth_wav(B: int, L: int, seed: int) -> torch.Tensor:
    """The seeded input of a case (tests/golden/make_golden.py synth_wav)."""
    g = torch.Generator().manual_seed(seed)
    return (0.1 * torch.randn(B, L, generator=g)).clamp_(-1, 1)


def wav_digest(wav: torch.Tensor) -> str:
    return hashlib.sha256(wav.detach().contiguous().numpy().tobytes()).hexdigest()
