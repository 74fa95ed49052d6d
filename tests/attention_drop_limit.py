"""What tests/test_gpu_attention_dropout.py and tests/test_attention_drop_limit.py share: the value cases of the fused attention with the
dropout mask inside (csrc/attention_drop.hip), their fp64 reference and per-element limit, and a numpy / torch model of the kernel's
arithmetic with the mistakes a kernel of this kind can make (MUTANTS).

Reference (HF eager order, softmax -> dropout -> . v), from the inputs as rounded to the operand type:

    ref[i, d] = sum_j keep_ij s P_ij v_jd,      P = fp64 softmax(scale q k^T),  s = float32(1 / (1 - p)),
    keep_ij = the mask of include/svt_mi355.h "svt_dropout" at site 2, element e0 + ((b H + h) T + i) T + j   (tests/dropout_cases.py)

Limit, per element, from the number formats (u = 2^-8 for bf16, 2^-11 for IEEE half), tests/test_gpu_attention.py's limit taken over the
kept keys with no factor on top:

    |got - ref| <= u (A + |ref|) + s T 2^-24 max|v|,      A = s sum_j keep_ij P_ij |v_jd|

(P is rounded to the operand type before P V: <= u A; the output is rounded once: <= u |ref|; fp32 row sums and accumulators over T keys in
any order, and the one fp32 rounding of s: the last term).

The shapes.  Every mutant must break the limit at EVERY case, so every case has T % 64 != 0 (the padded row stride differs from T), more
than one head, a layer and a step other than 0, and p large enough that a wrong mask moves many elements.  T = 65: a one-key tail tile;
129: two query blocks of the four-wave kernel; 499 (odd): every alignment of a row's first element in its four-word group, eight tiles;
130 at head size 128.  One peaked case (gain 8: rows with one dominant key, the deferred rescale under a mask) and one in the "separate"
layout (q in its own buffer, k | v packed, padded output rows)."""
from __future__ import annotations

import collections

import numpy as np
import torch

import dropout_cases as DC

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}

ValueCase = collections.namedtuple("ValueCase", "B T H dh gain layout p seed step layer e0")


def V(B, T, H, dh=64, gain=1.5, layout="packed", p=0.1, seed=0x9E3779B97F4A7C15, step=3, layer=1, e0=0):
    return ValueCase(B, T, H, dh, gain, layout, p, seed, step, layer, e0)


VALUE_CASES = [
    V(2, 65, 3),
    V(1, 129, 2, p=0.5, e0=1),
    V(2, 499, 2),
    V(1, 499, 4, gain=8.0, e0=2 ** 32 - 2),
    V(2, 499, 2, layout="separate", p=0.5, layer=11, step=7, e0=2 ** 34 + 1),
    V(2, 65, 2, dh=128),
    V(1, 130, 2, dh=128, p=0.5, e0=1),
]


def case_id(c):
    return (f"B{c.B}-T{c.T}-H{c.H}-dh{c.dh}-g{c.gain}-p{c.p}-e{c.e0 % 1000}" + ("" if c.layout == "packed" else "-" + c.layout))


def scale_of(dh):
    return float(np.float32(dh ** -0.5))   # what the C ABI's float argument holds


def make_inputs(c, dtype):
    """x (B, T, 3 D) rounded to `dtype` on the CPU: q | k | v of every head."""
    D = c.H * c.dh
    g = torch.Generator().manual_seed(c.B * 100003 + c.T * 101 + c.H)
    return (torch.randn(c.B, c.T, 3 * D, generator=g) * c.gain).to(dtype)


# ---------------------------------------------------------------------------------------------------------------- the mask
def keep_at(e, p, seed, step, layer, word_shift=0):
    """The keep bit of site 2 at the element indices e (any shape, uint64): word (e + word_shift) & 3 of group e >> 2."""
    e = np.asarray(e, dtype=np.uint64)
    q = e >> np.uint64(2)
    qs, inv = np.unique(q.ravel(), return_inverse=True)
    site_layer = (DC.SITE_ATTN_PROBS | (layer << 8)) & DC.U32
    ctr = np.stack([qs & np.uint64(DC.U32), qs >> np.uint64(32), np.full_like(qs, site_layer), np.full_like(qs, step & DC.U32)], -1)
    w = DC.philox4x32_10(ctr, (seed & DC.U32, (seed >> 32) & DC.U32))
    word = w[inv.ravel(), ((e.ravel() + np.uint64(word_shift)) & np.uint64(3)).astype(np.int64)]
    return (word >= np.uint64(DC.threshold(p))).reshape(e.shape)


MUTANTS = ("transposed", "stride_tp", "word_shift", "key_map_r", "head_ignored", "layer_ignored", "step_ignored", "renormalised",
           "scale_omitted")


def keep_mask(c, mutant=None):
    """keep (B, H, T, T) bool as the kernel (or a mutant of it) lays it on the probabilities."""
    B, T, H = c.B, c.T, c.H
    b = np.arange(B, dtype=np.uint64)[:, None, None, None]
    h = np.arange(H, dtype=np.uint64)[None, :, None, None]
    i = np.arange(T, dtype=np.uint64)[None, None, :, None]
    j = np.arange(T, dtype=np.uint64)[None, None, None, :]
    stride = np.uint64(T)
    layer, step, shift = c.layer, c.step, 0
    if mutant == "stride_tp":
        stride = np.uint64((T + 63) // 64 * 64)          # the padded key length of the fused path's buffers
    if mutant == "head_ignored":
        h = h * np.uint64(0)
    if mutant == "layer_ignored":
        layer = 0
    if mutant == "step_ignored":
        step = 0
    if mutant == "word_shift":
        shift = 1
    if mutant == "key_map_r":
        # the lane's register r of a 32-key block holds key 4 hh + (r & 3) + 8 (r >> 2); the mutant looks up key 4 hh + r
        jj = np.arange(T, dtype=np.int64)
        in32 = jj % 32
        hh, rest = (in32 // 4) % 2, in32 - 4 * ((in32 // 4) % 2)
        r = (rest % 4) + 4 * (rest // 8)
        j = (jj - in32 + 4 * hh + r).astype(np.uint64)[None, None, None, :]
    e = np.uint64(c.e0) + ((b * np.uint64(H) + h) * np.uint64(T) + i) * stride + j
    k = keep_at(e, c.p, c.seed, step, layer, shift)
    if mutant == "transposed":
        k = np.ascontiguousarray(np.swapaxes(k, -1, -2))
    return k


# ---------------------------------------------------------------------------------------------------------------- reference and limit
def split_heads(x, c):
    D = c.H * c.dh
    return [t.reshape(c.B, c.T, c.H, c.dh).permute(0, 2, 1, 3) for t in x.split(D, dim=-1)]   # (B, H, T, dh)


def reference(c, x, keep):
    """(ref, A) as (B, T, H dh) float64 from the rounded inputs x and the keep mask."""
    q, k, v = (t.double() for t in split_heads(x, c))
    s = float(DC.scale(c.p))
    P = torch.softmax(q @ k.transpose(-1, -2) * scale_of(c.dh), -1) * torch.from_numpy(keep).double() * s
    D = c.H * c.dh
    ref = (P @ v).permute(0, 2, 1, 3).reshape(c.B, c.T, D)
    A = (P @ v.abs()).permute(0, 2, 1, 3).reshape(c.B, c.T, D)
    return ref, A


def limit(c, x, ref, A, dtype):
    D = c.H * c.dh
    vmax = x[..., 2 * D:].double().abs().max().item()
    return U[dtype] * (A + ref.abs()) + float(DC.scale(c.p)) * c.T * 2.0 ** -24 * vmax


# ---------------------------------------------------------------------------------------------------------------- model of the kernel
def model(c, x, dtype, mutant=None):
    """The kernel's arithmetic on the CPU: fp32 scores, unnormalised p = exp(s - max) in fp32, the row sum over ALL keys in fp32, p rounded
    to the operand type, the mask, an fp32 product with v, one multiplication by scale / l, the output rounded to the operand type."""
    q, k, v = (t.float() for t in split_heads(x, c))
    keep = torch.from_numpy(keep_mask(c, mutant))
    s = (q @ k.transpose(-1, -2)) * np.float32(scale_of(c.dh))
    pu = torch.exp(s - s.amax(-1, keepdim=True))
    l = (pu * keep if mutant == "renormalised" else pu).sum(-1, keepdim=True)
    pk = pu.to(dtype).float() * keep
    o = pk @ v
    sc = np.float32(1.0) if mutant == "scale_omitted" else DC.scale(c.p)
    out = (o * (torch.tensor(sc) / l)).to(dtype)
    return out.permute(0, 2, 1, 3).reshape(c.B, c.T, c.H * c.dh)
