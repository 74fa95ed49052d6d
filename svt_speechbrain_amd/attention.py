"""The fused attention of the 16-bit modes as a torch op that trains: ``fused_attention`` (a ``torch.autograd.Function`` over
``svt_attention_forward`` / ``svt_attention_backward``) and ``FusedSelfAttention``, an ``nn.Module`` with the parameter names of
transformers' ``Wav2Vec2Attention`` around it.

Both directions are HIP kernels (csrc/attention_bf16.hip, attention_drop.hip, attention_bwd.hip); no (B, H, T, T) tensor exists in either.
The dropout mask on the probabilities is a function of the element's position, (seed, step) and the layer (include/svt_mi355.h,
"svt_dropout", site 2), so the backward redraws the forward's mask from the same five numbers instead of storing it.  There is no eager
fall-back: what the kernels refuse raises ``SvtError`` with the library's message.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch
from torch import nn

from . import _lib
from ._lib import SvtError

HEAD_DIM = 64
_VARIANT = {torch.bfloat16: None, torch.float16: "f16"}


def _check_inputs(q, k, v):
    for name, t in (("q", q), ("k", k), ("v", v)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise ValueError(f"fused_attention: {name} must be a (B, T, H, {HEAD_DIM}) tensor")
        if t.device.type != "cuda":
            raise SvtError(f"fused_attention: {name} must live on a ROCm device ('cuda:N'), got {t.device}: there is no CPU path")
        if t.dtype not in _VARIANT:
            raise SvtError(f"fused_attention: {name} is {t.dtype}; the kernels take torch.bfloat16 or torch.float16")
        if t.shape[-1] != HEAD_DIM:
            raise SvtError(f"fused_attention: head size {t.shape[-1]}; the backward kernels serve head size {HEAD_DIM}")
    if not (q.shape == k.shape == v.shape and q.dtype == k.dtype == v.dtype and q.device == k.device == v.device):
        raise ValueError("fused_attention: q, k and v must agree in shape, dtype and device")


def _rows(t):
    """t (B, T, H, 64) as the kernels address it -- heads contiguous in a row, clips T rows apart -- or a contiguous copy."""
    B, T, H, dh = t.shape
    s = t.stride()
    ok = s[3] == 1 and s[2] == dh and s[1] % 8 == 0 and s[1] >= H * dh and (B == 1 or s[0] == T * s[1]) and t.data_ptr() % 16 == 0
    return t if ok else t.contiguous()


def _desc(q, k, v, o, scale, p, seed, step, layer, e0):
    B, T, H, dh = q.shape
    d = _lib.AttentionDescC()
    d.struct_size = C.sizeof(_lib.AttentionDescC)
    d.precision = 1
    d.q, d.k, d.v, d.o = q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr()
    d.ldq, d.ldkv, d.ldo = q.stride(1), k.stride(1), o.stride(1)
    d.batch, d.t, d.heads, d.head_dim = B, T, H, dh
    d.scale, d.p, d.seed, d.step, d.layer, d.e0 = scale, p, seed, step, layer, e0
    return d


class _FusedAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, scale, p, seed, step, layer, e0):
        lib = _lib.load(_VARIANT[q.dtype])
        q, k, v = _rows(q), _rows(k), _rows(v)
        if k.stride(1) != v.stride(1):   # the kernels take one row stride for k and v
            k, v = k.contiguous(), v.contiguous()
        B, T, H, dh = q.shape
        o = torch.empty(B, T, H, dh, device=q.device, dtype=q.dtype)
        d = _desc(q, k, v, o, scale, p, seed, step, layer, e0)
        dev = _lib.dev_index(q.device)
        _lib.check(lib.svt_attention_forward(C.byref(d), dev, _lib.stream_ptr(q.device)), "svt_attention_forward", lib)
        ctx.save_for_backward(q, k, v, o)
        ctx.mask = (scale, p, seed, step, layer, e0)
        return o

    @staticmethod
    def backward(ctx, d_o):
        q, k, v, o = ctx.saved_tensors
        lib = _lib.load(_VARIANT[q.dtype])
        B, T, H, dh = q.shape
        d_o = _rows(d_o)
        g = torch.empty(B, T, 3, H, dh, device=q.device, dtype=q.dtype)   # dq | dk | dv of a row side by side: one packed gradient
        d = _desc(q, k, v, o, *ctx.mask)
        d.d_o, d.lddo = d_o.data_ptr(), d_o.stride(1)
        d.dq, d.dk, d.dv = g[:, :, 0].data_ptr(), g[:, :, 1].data_ptr(), g[:, :, 2].data_ptr()
        d.lddq = d.lddkv = 3 * H * dh
        dev, stream = _lib.dev_index(q.device), _lib.stream_ptr(q.device)
        need = C.c_size_t(0)
        _lib.check(lib.svt_attention_backward(C.byref(d), None, C.byref(need), dev, stream), "svt_attention_backward", lib)
        ws = torch.empty(max(int(need.value), 16), device=q.device, dtype=torch.uint8)
        _lib.check(lib.svt_attention_backward(C.byref(d), ws.data_ptr(), C.byref(need), dev, stream), "svt_attention_backward", lib)
        return g[:, :, 0], g[:, :, 1], g[:, :, 2], None, None, None, None, None, None


def fused_attention(q, k, v, *, scale: Optional[float] = None, dropout_p: float = 0.0, seed: Optional[int] = None, step: int = 0,
                    layer: int = 0, e0: int = 0):
    """softmax(scale q k^T) -> dropout -> . v on (B, T, H, 64) bf16 / fp16 ROCm tensors; returns (B, T, H, 64).  Differentiable.

    bf16 runs ``libsvt_mi355.so``, fp16 ``libsvt_mi355_f16.so``.  Rows may be strided (heads contiguous within a row, a row stride that
    is a multiple of 8 elements, 16-byte aligned): the three chunks of a packed projection pass without a copy; any other layout is
    copied once.  ``scale`` defaults to 64 ** -0.5.  ``dropout_p`` > 0 draws the position-defined mask of site 2 in ``layer`` at
    (``seed``, ``step``), first element ``e0``; ``seed=None`` takes ``torch.cuda.initial_seed()``.  ``dropout_p == 0`` runs the plain
    kernels.  The backward returns three views of one packed (B, T, 3, H, 64) gradient."""
    _check_inputs(q, k, v)
    p = float(dropout_p)
    if not 0.0 <= p < 1.0:
        raise SvtError(f"fused_attention: dropout_p must lie in [0, 1), got {dropout_p}")
    if seed is None:
        seed = torch.cuda.initial_seed()
    scale = float(HEAD_DIM ** -0.5 if scale is None else scale)
    return _FusedAttention.apply(q, k, v, scale, p, int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFF, int(layer), int(e0))


class FusedSelfAttention(nn.Module):
    """Self-attention with the parameter names of transformers' ``Wav2Vec2Attention`` (``q_proj``, ``k_proj``, ``v_proj``, ``out_proj``: its
    ``state_dict`` loads) and ``fused_attention`` between the projections, which torch runs.  In ``train()`` with ``dropout`` > 0 every
    forward draws the mask at (``torch.cuda.initial_seed()``, ``dropout_step``) for ``layer`` and advances ``dropout_step``; in
    ``eval()`` no mask is drawn and the counter stands still.  ``forward`` returns ``(out, None, None)`` as HF's module does."""

    def __init__(self, embed_dim: int, num_heads: int, dropout: float = 0.0, bias: bool = True, layer: int = 0):
        super().__init__()
        if embed_dim != num_heads * HEAD_DIM:
            raise SvtError(f"FusedSelfAttention: embed_dim {embed_dim} / num_heads {num_heads} is not head size {HEAD_DIM}")
        self.embed_dim, self.num_heads, self.dropout, self.layer = embed_dim, num_heads, float(dropout), int(layer)
        self.scaling = HEAD_DIM ** -0.5
        self.k_proj = nn.Linear(embed_dim, embed_dim, bias=bias)
        self.v_proj = nn.Linear(embed_dim, embed_dim, bias=bias)
        self.q_proj = nn.Linear(embed_dim, embed_dim, bias=bias)
        self.out_proj = nn.Linear(embed_dim, embed_dim, bias=bias)
        self.dropout_step = 0

    @classmethod
    def from_module(cls, attn: nn.Module, layer: int = 0) -> "FusedSelfAttention":
        """A FusedSelfAttention that SHARES the four projections of an HF attention module (``Wav2Vec2Attention`` and its kin)."""
        self = cls(attn.embed_dim, attn.num_heads, dropout=float(attn.dropout), bias=attn.q_proj.bias is not None, layer=layer)
        self.q_proj, self.k_proj, self.v_proj, self.out_proj = attn.q_proj, attn.k_proj, attn.v_proj, attn.out_proj
        return self

    def forward(self, hidden_states, attention_mask=None, **_):
        if attention_mask is not None:
            raise SvtError("FusedSelfAttention: an attention mask is not served (the reference passes none)")
        B, T, _D = hidden_states.shape
        shape = (B, T, self.num_heads, HEAD_DIM)
        q, k, v = (proj(hidden_states).view(shape) for proj in (self.q_proj, self.k_proj, self.v_proj))
        if self.training and self.dropout > 0:
            step = self.dropout_step
            self.dropout_step = (step + 1) & 0xFFFFFFFF
            o = fused_attention(q, k, v, scale=self.scaling, dropout_p=self.dropout, step=step, layer=self.layer)
        else:
            o = fused_attention(q, k, v, scale=self.scaling)
        return self.out_proj(o.reshape(B, T, self.embed_dim)), None, None
