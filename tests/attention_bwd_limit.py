"""What tests/test_gpu_attention_backward.py and tests/test_attention_bwd_limit.py share: the value cases of the fused attention backward
(csrc/attention_bwd.hip), their fp64 reference, a per-element limit for each of dQ, dK and dV, and a torch model of the kernels' arithmetic
with the mistakes a kernel of this kind can make (MUTANTS).

Reference, in fp64 from the inputs q, k, v, dO as rounded to the operand type (HF eager order, softmax -> dropout -> . v):

    P = softmax(scale q k^T)            keep_ij = the mask of "svt_dropout" site 2 at element e0 + ((b H + h) T + i) T + j
    Pt = s keep P                       s = float32(1 / (1 - p))                      (tests/dropout_cases.py)
    O  = Pt v, rounded to the operand type: what the op saved and the kernels read
    dV = Pt^T dO      dP = s keep (dO v^T)      delta_i = sum_j P_ij dP_ij  (= dO_i . O_i before O's rounding)
    dS = P (dP - delta)       dQ = scale dS k       dK = scale dS^T q

Limit, per element, first order in u (u = 2^-8 for bf16, 2^-11 for IEEE half) and w = 2^-24 (fp32), with no fitted factor.  What the
kernels round, and the term each rounding gives:

  * P in fp32.  The exponent x_ij = c S_ij - L_i (c = scale log2 e) carries: S_ij, an fp32 sum of 64 exact products (<= 64 w a_ij,
    a_ij = sum_d |q_id k_jd|), the roundings of c, of the product and of the fma (3 w c a_ij), and L_i = m_i + log2 l_i: the same errors
    of the row's dominant scores (<= 66 w c max_j a_ij), l's fp32 sum of T terms and exp2 / log2 / the add (<= (1.5 T + 6) w), its own
    magnitude (2 w log2 T; the c max a part is counted).  So P is off by the RELATIVE amount
        E_ij = ln 2 * w * (67 c a_ij + 66 c max_j a_ij + 2 log2 T + 1.5 T + 6) + 2^-22        (2^-22: v_exp_f32 itself).
  * dV: P~ = keep P is cut to 16 bits before the product (u), the fp32 accumulator sums T terms ((T + 2) w with s), one output rounding:
        lim_dV_jd = u (A + |dV_jd|) + sum_i E_ij Pt_ij |dO_id| + (T + 2) w A,          A = sum_i Pt_ij |dO_id|.
  * dS is cut to 16 bits before the dQ and dK products (u |dS|); before that it inherits P's error (E |dS|), dP's (an fp32 sum of 64
    exact products times s: 66 w s keep sum_d |dO_id v_jd|), the two fp32 operations on dP - delta (3 w (|dP| + |delta|)) and delta's:
    delta_i is read from the ROUNDED O, at most u G_i with G_i = sum_d |dO_id O_id|, plus its fp32 sum (64 w G_i), carried through P_ij:
        D_ij = (u + E_ij) |dS_ij| + P_ij (66 w s keep_ij sum_d |dO_id v_jd| + (u + 64 w) G_i + 3 w (|dP_ij| + |delta_i|))
        lim_dQ_id = scale sum_j D_ij |k_jd| + (T + 2) w scale sum_j |dS_ij| |k_jd| + u |dQ_id|
        lim_dK_jd = scale sum_i D_ij |q_id| + (T + 2) w scale sum_i |dS_ij| |q_id| + u |dK_jd|
    (the fp32 sums over T in any order, the multiplication by scale, one output rounding).
  * Every cut to 16 bits is relative only above the format's smallest normal number: below it the spacing is the subnormal one, so each
    cut adds at most half of it, h = 2^-25 for IEEE half (2^-134 for bf16), as an ABSOLUTE term: h s sum_i |dO_id| + h on dV, h on every
    D_ij and on the outputs dQ and dK.  Peaked rows put most of P and dS there.

The cases.  Every case has T % 64 != 0 (the padded row stride differs from T and the last tile has padded rows), more than one head, a
layer and a step other than 0.  T = 65: a one-row tail tile; 129: two blocks of either kernel; 499 (odd): every alignment of a row's
first element, eight tiles.  One peaked case (gain 8), one in the "separate" layout (q in its own buffer, k | v packed, padded gradient
rows), one with e0 = 2^34 + 1, p in {0, 0.1, 0.5}.  Every mutant must break the limit at every case it can touch: the mask mutants
change nothing where no mask is drawn, so they are held to the cases with p > 0 (MASK_MUTANTS); the rest to every case."""
from __future__ import annotations

import collections
import math

import numpy as np
import torch

import attention_drop_limit as AD
import dropout_cases as DC

U = AD.U
HALF_SUBNORMAL = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}   # half the spacing below the smallest normal number
W = 2.0 ** -24
DH = 64

ValueCase = collections.namedtuple("ValueCase", "B T H gain layout p seed step layer e0")


def V(B, T, H, gain=1.5, layout="packed", p=0.1, seed=0x9E3779B97F4A7C15, step=3, layer=1, e0=0):
    return ValueCase(B, T, H, gain, layout, p, seed, step, layer, e0)


VALUE_CASES = [
    V(2, 65, 3),
    V(1, 129, 2, p=0.5, e0=1),
    V(2, 499, 2),
    V(1, 499, 2, gain=8.0, e0=2 ** 32 - 2),
    V(2, 129, 2, layout="separate", p=0.5, layer=11, step=7, e0=2 ** 34 + 1),
    V(2, 65, 2, p=0.0),
]

MASK_MUTANTS = ("transposed_dkv", "dp_unmasked", "scale_once", "delta_kept_only", "stride_tp", "layer_ignored", "step_ignored",
                "head_ignored")
MUTANTS = MASK_MUTANTS + ("scale_omitted_dk", "l_natural", "padded_rows_counted", "padded_keys_counted")


def case_id(c):
    return f"B{c.B}-T{c.T}-H{c.H}-g{c.gain}-p{c.p}-e{c.e0 % 1000}" + ("" if c.layout == "packed" else "-" + c.layout)


def touches(mutant, c):
    return c.p > 0 or mutant not in MASK_MUTANTS


SCALE = AD.scale_of(DH)                                          # what the C ABI's float argument holds
C32 = float(np.float32(SCALE) * np.float32(1.44269504088896340736))   # the launcher's c = scale * log2 e, in fp32


def make_inputs(c, dtype):
    """(x, do): x (B, T, 3 D) = q | k | v of every head and do (B, T, D), rounded to `dtype` on the CPU."""
    D = c.H * DH
    g = torch.Generator().manual_seed(c.B * 100003 + c.T * 101 + c.H)
    x = (torch.randn(c.B, c.T, 3 * D, generator=g) * c.gain).to(dtype)
    do = torch.randn(c.B, c.T, D, generator=g).to(dtype)
    return x, do


def _dc(c):
    """the case as tests/attention_drop_limit.py's helpers read it (head size 64)"""
    return AD.ValueCase(c.B, c.T, c.H, DH, c.gain, c.layout, c.p, c.seed, c.step, c.layer, c.e0)


_mask_cache = {}


def keep_mask(c, mutant=None):
    """keep (B, H, T, T) bool; p == 0: all ones (no mask is drawn).  Mask mutants of the index: stride_tp, *_ignored."""
    if c.p == 0:
        return np.ones((c.B, c.H, c.T, c.T), dtype=bool)
    m = mutant if mutant in ("stride_tp", "layer_ignored", "step_ignored", "head_ignored") else None
    key = (c, m)
    if key not in _mask_cache:
        _mask_cache[key] = AD.keep_mask(_dc(c), m)
    return _mask_cache[key]


def heads(t, c):
    """(B, T, H 64) -> (B, H, T, 64)"""
    return t.reshape(c.B, c.T, c.H, DH).permute(0, 2, 1, 3)


def unheads(t, c):
    return t.permute(0, 2, 1, 3).reshape(c.B, c.T, c.H * DH)


# ---------------------------------------------------------------------------------------------------------------- reference and limit
def reference(c, x, do, dtype):
    """dict: o (the saved output, rounded to dtype), dq, dk, dv (fp64, (B, T, D)) and their limits lim_dq, lim_dk, lim_dv."""
    u, eta, T = U[dtype], HALF_SUBNORMAL[dtype], c.T
    q, k, v = (t.double() for t in AD.split_heads(x, _dc(c)))
    g = heads(do, c).double()
    keep = torch.from_numpy(keep_mask(c)).double()
    s = float(DC.scale(c.p)) if c.p > 0 else 1.0
    P = torch.softmax(q @ k.transpose(-1, -2) * SCALE, -1)
    Pt = P * keep * s
    o = (Pt @ v).to(dtype)
    dV = Pt.transpose(-1, -2) @ g
    dP = (g @ v.transpose(-1, -2)) * keep * s
    delta = (P * dP).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    dQ = SCALE * (dS @ k)
    dK = SCALE * (dS.transpose(-1, -2) @ q)

    a = q.abs() @ k.abs().transpose(-1, -2)
    E = math.log(2.0) * W * (67 * C32 * a + 66 * C32 * a.amax(-1, keepdim=True) + 2 * math.log2(T) + 1.5 * T + 6) + 2.0 ** -22
    A = Pt.transpose(-1, -2) @ g.abs()
    lim_dv = u * (A + dV.abs()) + (E * Pt).transpose(-1, -2) @ g.abs() + (T + 2) * W * A + eta * (s * g.abs().sum(-2, keepdim=True) + 1)
    G = (g * o.double()).abs().sum(-1, keepdim=True)
    adp = (g.abs() @ v.abs().transpose(-1, -2)) * keep * s
    Dm = (u + E) * dS.abs() + P * (66 * W * adp + (u + 64 * W) * G + 3 * W * (dP.abs() + delta.abs())) + eta
    lim_dq = SCALE * (Dm @ k.abs()) + (T + 2) * W * SCALE * (dS.abs() @ k.abs()) + u * dQ.abs() + eta
    lim_dk = SCALE * (Dm.transpose(-1, -2) @ q.abs()) + (T + 2) * W * SCALE * (dS.abs().transpose(-1, -2) @ q.abs()) + u * dK.abs() + eta
    out = dict(o=unheads(o, c), dq=dQ, dk=dK, dv=dV, lim_dq=lim_dq, lim_dk=lim_dk, lim_dv=lim_dv)
    return {n: (t if n == "o" else unheads(t, c)) for n, t in out.items()}


# ---------------------------------------------------------------------------------------------------------------- model of the kernels
def model(c, x, do, o, dtype, mutant=None):
    """The three kernels' arithmetic on the CPU: fp32 scores and dP, L = m + log2 l in fp32, P = exp2(c S - L), delta from the rounded
    O in fp32, the mask on P~ and dP, dS and P~ cut to the operand type, fp32 products, one output rounding.  Returns (dq, dk, dv)."""
    T, Tp = c.T, (c.T + 63) // 64 * 64
    q, k, v = (t.float() for t in AD.split_heads(x, _dc(c)))
    g, of = heads(do, c).float(), heads(o, c).float()
    keep = torch.from_numpy(keep_mask(c, mutant)).float()
    s = float(DC.scale(c.p)) if c.p > 0 else 1.0
    xs = (q @ k.transpose(-1, -2)) * np.float32(C32)
    m = xs.amax(-1, keepdim=True)
    L = m + torch.log2(torch.exp2(xs - m).sum(-1, keepdim=True))
    if mutant == "l_natural":
        L = L * math.log(2.0)
    P = torch.exp2(xs - L)
    delta = (g * of).sum(-1, keepdim=True)
    dpr = g @ v.transpose(-1, -2)
    if mutant == "delta_kept_only":
        delta = (P * keep * dpr).sum(-1, keepdim=True)          # the sum over the kept keys without their scale
    dp_b = dpr * (1.0 if mutant == "dp_unmasked" else keep) * (1.0 if mutant == "scale_once" else s)   # kernel (b)
    dS_b = (P * (dp_b - delta)).to(dtype).float()
    keep_c = keep.transpose(-1, -2) if mutant == "transposed_dkv" else keep
    dp_c = dpr * (1.0 if mutant == "dp_unmasked" else keep_c) * (1.0 if mutant == "scale_once" else s)   # kernel (c)
    dS_c = (P * (dp_c - delta)).to(dtype).float()
    Pk = (P * keep_c).to(dtype).float()
    dq = dS_b @ k
    dk = dS_c.transpose(-1, -2) @ q
    dv = Pk.transpose(-1, -2) @ g
    if mutant == "padded_rows_counted":      # rows T .. Tp - 1 of the last query tile are copies of row T - 1 (the clamped source row)
        dk = dk + (Tp - T) * dS_c[..., T - 1, :, None] * q[..., T - 1:T, :]
        dv = dv + (Tp - T) * Pk[..., T - 1, :, None] * g[..., T - 1:T, :]
    if mutant == "padded_keys_counted":      # keys T .. Tp - 1 of the last key tile are copies of key T - 1
        dq = dq + (Tp - T) * dS_b[..., :, T - 1:T] * k[..., T - 1:T, :]
    sc = np.float32(SCALE)
    dq, dk, dv = dq * sc, dk * (np.float32(1.0) if mutant == "scale_omitted_dk" else sc), dv * np.float32(s)
    return tuple(unheads(t.to(dtype), c) for t in (dq, dk, dv))
