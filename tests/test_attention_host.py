"""Host-side checks of the fused attention's public surface (no GPU): the C ABI's new symbols are declared in the header and bound, the
module carries the parameter names of transformers' Wav2Vec2Attention, and what the kernels do not serve is refused before any library
call."""
import ctypes as C
import os
import re

import pytest
import torch

from svt_speechbrain_amd import _lib
from svt_speechbrain_amd import attention as ATT
import svt_speechbrain_amd as S

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "svt_mi355.h")


def test_symbols_are_declared_and_bound():
    with open(HEADER) as fh:
        text = fh.read()
    for name in ("svt_attention_forward", "svt_attention_backward"):
        assert re.search(r"\bint " + name + r"\(const svt_attention_desc\* d,", text), name
        assert name in _lib.SYMBOLS
    body = re.search(r"typedef struct svt_attention_desc \{(.*?)\} svt_attention_desc;", text, re.S).group(1)
    fields = re.findall(r"(\w+);", body)
    assert fields == [f[0] for f in _lib.AttentionDescC._fields_]
    assert fields[0] == "struct_size" and C.sizeof(_lib.AttentionDescC) == 176
    assert re.search(r"\b46 = query", text), "svt_debug_set key 46 is not documented"
    assert S.fused_attention is ATT.fused_attention and S.FusedSelfAttention is ATT.FusedSelfAttention


def test_state_dict_is_wav2vec2_attentions():
    w2v = pytest.importorskip("transformers.models.wav2vec2.modeling_wav2vec2")
    hf = w2v.Wav2Vec2Attention(128, 2, dropout=0.1)
    ours = ATT.FusedSelfAttention(128, 2, dropout=0.1)
    want = {k: tuple(v.shape) for k, v in hf.state_dict().items()}
    assert {k: tuple(v.shape) for k, v in ours.state_dict().items()} == want
    ours.load_state_dict(hf.state_dict())
    shared = ATT.FusedSelfAttention.from_module(hf, layer=4)
    assert shared.q_proj is hf.q_proj and shared.out_proj is hf.out_proj and shared.dropout == 0.1 and shared.layer == 4
    assert shared.dropout_step == 0
    nobias = ATT.FusedSelfAttention(128, 2, bias=False)
    assert sorted(nobias.state_dict()) == ["k_proj.weight", "out_proj.weight", "q_proj.weight", "v_proj.weight"]


def test_refusals_come_before_any_library_call(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_library)
    mod = ATT.FusedSelfAttention(128, 2)
    x = torch.zeros(1, 8, 128)
    with pytest.raises(_lib.SvtError, match="mask"):
        mod(x, attention_mask=torch.ones(1, 1, 8, 8))
    with pytest.raises(_lib.SvtError, match="ROCm device"):
        mod(x)                                                       # a CPU tensor
    q = torch.zeros(1, 8, 2, 64, dtype=torch.bfloat16)
    with pytest.raises(_lib.SvtError, match="ROCm device"):
        ATT.fused_attention(q, q, q)
    meta = torch.zeros(1, 8, 2, 64, device="meta")                   # fp32: the dtype check needs no device
    with pytest.raises(_lib.SvtError):
        ATT.fused_attention(meta, meta, meta)
    with pytest.raises(_lib.SvtError, match="head size"):
        ATT.FusedSelfAttention(256, 2)
    with pytest.raises(_lib.SvtError, match="head size 128"):
        ATT._check_inputs(*[_Fake((1, 8, 2, 128), torch.bfloat16)] * 3)
    with pytest.raises(_lib.SvtError, match="float32"):
        ATT._check_inputs(*[_Fake((1, 8, 2, 64), torch.float32)] * 3)


class _Fake(torch.Tensor):
    """A tensor that says it lives on a ROCm device: the checks behind the device check run without one."""
    @staticmethod
    def __new__(cls, shape, dtype):
        return torch.Tensor._make_subclass(cls, torch.zeros(shape, dtype=dtype))

    @property
    def device(self):
        return torch.device("cuda:0")
