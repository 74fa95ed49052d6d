"""What tests/golden/make_golden_encoder_dropout.py and the dropout tests share: a numpy restatement of the mask function of
include/svt_mi355.h ("svt_dropout") and the fixture's case tables.

The mask function.  Element ``e`` (its logical index in the tensor: ``(b*T + t)*W + c`` in a (B, T, W) tensor, ``((b*H + h)*T + i)*T + j``
in the attention probabilities) of site ``s`` in layer ``l`` is kept iff

    Philox4x32-10(key = (seed_lo, seed_hi), counter = (q_lo, q_hi, s | l << 8, step))[e & 3] >= floor(p * 2**32),   q = e >> 2;

a kept value is multiplied by ``float32(1 / (1 - p))`` (one fp32 rounding), a dropped one becomes +0.  Sites: 0 feature projection,
1 the encoder's own dropout, 2 attention probabilities, 3 attention branch, 4 behind GELU, 5 behind FFN-2; sites 0 and 1 use layer 0.

The cases.  Per family the issue's list: each rate alone, all together, one layerdrop case that skips exactly one layer, one that skips
all, and one with SpecAugment on as well.  B = 2, 16 000 samples (49 frames).  ``seed`` seeds the input, torch's host generator (the
layerdrop draws) and numpy's (the SpecAugment draws); ``mask_seed`` / ``step`` are the two words of the mask function.
"""
from __future__ import annotations

import hashlib
import math

import numpy as np
import torch

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
U32 = 0xFFFFFFFF

SITE_FEAT_PROJ, SITE_ENCODER, SITE_ATTN_PROBS, SITE_ATTN_OUT, SITE_ACTIVATION, SITE_FFN_OUT = range(6)


def philox4x32_10(counter, key):
    """counter: (..., 4) integers below 2**32, key: (k0, k1).  Returns (..., 4) uint64 holding the four 32-bit output words."""
    c = np.asarray(counter, dtype=np.uint64)
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    k0, k1 = int(key[0]) & U32, int(key[1]) & U32
    m32 = np.uint64(U32)
    for _ in range(10):
        p0 = np.uint64(M0) * c0
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)), (p1 & m32), ((p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)), (p0 & m32)
        k0, k1 = (k0 + W0) & U32, (k1 + W1) & U32
    return np.stack([c0, c1, c2, c3], axis=-1)


def threshold(p: float) -> int:
    return int(math.floor(p * 4294967296.0))


def scale(p: float) -> np.float32:
    return np.float32(1.0 / (1.0 - p))


def words(seed: int, step: int, site: int, layer: int, n: int, e0: int = 0) -> np.ndarray:
    """The mask word of each of the n elements e0 .. e0 + n - 1 (uint64 array holding 32-bit values)."""
    e = np.arange(n, dtype=np.uint64) + np.uint64(e0)
    q = e >> np.uint64(2)
    qs, inv = np.unique(q, return_inverse=True)
    ctr = np.stack([qs & np.uint64(U32), qs >> np.uint64(32), np.full_like(qs, (site | (layer << 8)) & U32), np.full_like(qs, step & U32)], -1)
    w = philox4x32_10(ctr, (seed & U32, (seed >> 32) & U32))
    return w[inv, (e & np.uint64(3)).astype(np.int64)]


def keep(p: float, seed: int, step: int, site: int, layer: int, n: int, e0: int = 0) -> np.ndarray:
    return words(seed, step, site, layer, n, e0) >= np.uint64(threshold(p))


def apply(x: np.ndarray, p: float, seed: int, step: int, site: int, layer: int, e0: int = 0) -> np.ndarray:
    """x: float32 array in logical order.  Kept: x * float32(1 / (1 - p)) in fp32; dropped: +0."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    k = keep(p, seed, step, site, layer, x.size, e0).reshape(x.shape)
    return np.where(k, x * scale(p), np.float32(0.0)).astype(np.float32)


def apply_torch(x: torch.Tensor, p: float, seed: int, step: int, site: int, layer: int) -> torch.Tensor:
    k = torch.from_numpy(keep(p, seed, step, site, layer, x.numel()).reshape(tuple(x.shape)))
    return torch.where(k, x * torch.tensor(float(scale(p)), dtype=x.dtype), torch.zeros((), dtype=x.dtype))


# ---------------------------------------------------------------------------------------------------------------- the fixture's cases
LOCAL = "local_ckpt"
# family -> (directory under tests/golden/local_ckpt, config.json fields on top of the case's, WavLM-like: no attention dropout)
FAMILIES = {
    "wav2vec2": ("tiny-wav2vec2-hf", {}, False),
    "stable": ("tiny-wav2vec2-hf", dict(do_stable_layer_norm=True), False),
    "hubert": ("tiny-hubert-bn-hf", {}, False),
    "data2vec": ("tiny-data2vec-hf", {}, False),
    "wavlm": ("tiny-wavlm-hf", {}, True),
    "dh64": ("tiny-wav2vec2-dh64-hf", {}, False),   # hidden 128, 2 heads: head dim 64, which the 16-bit modes serve with the fused attention
}
# family -> the fixture file (tests/golden/<name>.pt) that holds its cases: two files, each under the 1 MiB a committed file may have
FIXTURE_OF = {"wav2vec2": "encoder_dropout", "stable": "encoder_dropout", "hubert": "encoder_dropout", "dh64": "encoder_dropout",
              "data2vec": "encoder_dropout_2", "wavlm": "encoder_dropout_2"}
ZERO = dict(hidden_dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, feat_proj_dropout=0.0, layerdrop=0.0)
N_SAMPLES = 16000
STEP = 3

# name -> (config.json fields, seed, expected skipped layers or None = whatever the seed draws (recorded))
CASES = {
    "feat_proj": (dict(feat_proj_dropout=0.1), 201, (False, False)),
    "hidden": (dict(hidden_dropout=0.1), 202, (False, False)),
    "attention": (dict(attention_dropout=0.1), 203, (False, False)),
    "activation": (dict(activation_dropout=0.1), 204, (False, False)),
    "all": (dict(hidden_dropout=0.1, attention_dropout=0.1, activation_dropout=0.1, feat_proj_dropout=0.1, layerdrop=0.1), 205, (False, False)),
    "skip_one": (dict(layerdrop=0.5), 207, (False, True)),
    "skip_all": (dict(layerdrop=0.9), 206, (True, True)),
    "spec": (dict(hidden_dropout=0.1, feat_proj_dropout=0.1, apply_spec_augment=True, mask_time_prob=0.3, mask_time_length=3,
                  mask_feature_prob=0.0), 208, (False, False)),
}
DH64_CASES = ("all",)   # the head-dim-64 model: the one seeded case of the issue


def case_list():
    """(family, case) of every fixture entry.  WavLM: no attention-dropout case (refused: its reference attention is torch's fused one),
    "all" runs with attention_dropout 0, and there is no case that skips every layer: HF's WavLM encoder draws for layer 0 like for the
    others but never skips it (``i > 0``), because only that layer holds the position embedding."""
    out = []
    for fam, (_, _, wavlm_like) in FAMILIES.items():
        for name in CASES:
            if fam == "dh64" and name not in DH64_CASES:
                continue
            if wavlm_like and name in ("attention", "skip_all"):
                continue
            out.append((fam, name))
    return out


def case_fields(fam: str, name: str) -> dict:
    f = dict(ZERO)
    f.update(CASES[name][0])
    f.update(FAMILIES[fam][1])
    if FAMILIES[fam][2]:
        f["attention_dropout"] = 0.0
    return f


def mask_seed(fam: str, name: str) -> int:
    """The 64-bit seed word of a case: both halves nonzero."""
    return (0x9E3779B97F4A7C15 * (1 + list(FAMILIES).index(fam)) + 0xD1B54A32D192ED03 * (1 + list(CASES).index(name))) & 0xFFFFFFFFFFFFFFFF


def site_tensors(fields: dict, B: int, T: int, D: int, F: int, H: int, layers: int):
    """(site, layer, rate, element count) of every tensor a case's forward drops."""
    out = []
    if fields["feat_proj_dropout"] > 0:
        out.append((SITE_FEAT_PROJ, 0, fields["feat_proj_dropout"], B * T * D))
    if fields["hidden_dropout"] > 0:
        out.append((SITE_ENCODER, 0, fields["hidden_dropout"], B * T * D))
    for l in range(layers):
        if fields["attention_dropout"] > 0:
            out.append((SITE_ATTN_PROBS, l, fields["attention_dropout"], B * H * T * T))
        if fields["hidden_dropout"] > 0:
            out.append((SITE_ATTN_OUT, l, fields["hidden_dropout"], B * T * D))
            out.append((SITE_FFN_OUT, l, fields["hidden_dropout"], B * T * D))
        if fields["activation_dropout"] > 0:
            out.append((SITE_ACTIVATION, l, fields["activation_dropout"], B * T * F))
    return out


def synth_wav(B: int, L: int, seed: int) -> torch.Tensor:
    """The seeded input of a case (tests/golden/make_golden.py synth_wav)."""
    g = torch.Generator().manual_seed(seed)
    return (0.1 * torch.randn(B, L, generator=g)).clamp_(-1, 1)


def wav_digest(wav: torch.Tensor) -> str:
    return hashlib.sha256(wav.detach().contiguous().numpy().tobytes()).hexdigest()


def host_rng_digest() -> str:
    """A digest of torch's HOST default generator state: equal after two runs that made the same draws."""
    return hashlib.sha256(torch.get_rng_state().numpy().tobytes()).hexdigest()
