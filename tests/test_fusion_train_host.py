"""Host-side checks of the FusionRCA training step (no GPU needed): the C-ABI additions are declared and bound, the optimizer takes
the recipe's 26 tensors in one call, and the trainer refuses CPU parameters loudly."""
import hashlib
import os
import re

import pytest
import torch

import svt_speechbrain_amd as S
from svt_speechbrain_amd import _lib
from svt_speechbrain_amd import training as TR
from svt_speechbrain_amd import weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("svt_rca_refresh_params", "svt_rca_train_workspace_bytes", "svt_rca_forward_train", "svt_rca_backward",
               "svt_linear_backward_data", "svt_debug_rca_wgrad", "svt_debug_rca_attn_bwd")


def test_training_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "svt_mi355.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.SYMBOLS, name


def test_one_optimizer_call_takes_the_recipes_26_tensors():
    assert TR._MAX_TENSORS == 32
    assert len(TR.RCA_KEYS) == 24 and len(set(TR.RCA_KEYS)) == 24
    f = S.FusionRCA(nhead=2, d_ffn=64, d_model=32, max_length=16, precision="fp32")
    names = dict(f.named_parameters())
    assert set(TR.RCA_KEYS) == set(names)
    head = S.Linear(20, input_size=32)
    assert len(list(f.parameters())) + len(list(head.parameters())) == 26


def test_fusion_trainer_refuses_cpu_parameters():
    f = S.FusionRCA(nhead=2, d_ffn=64, d_model=32, max_length=16, precision="fp32")
    head = S.Linear(20, input_size=32)
    with pytest.raises(_lib.SvtError):
        TR.FusionTrainer({"fusion": f, "head": head})


def test_fusion_trainer_refuses_untrainable_precisions():
    for prec in ("fp16", "bf16x3", "fp16x3"):
        f = S.FusionRCA(nhead=2, d_ffn=64, d_model=32, max_length=16, precision=prec)
        with pytest.raises(_lib.SvtError):
            TR.FusionTrainer({"fusion": f, "head": S.Linear(20, input_size=32)})


def test_fusion_trainer_is_exported():
    assert S.FusionTrainer is TR.FusionTrainer
    assert "FusionTrainer" in S.__all__


def fixture_inputs(fx):
    """Features and the initial head of tests/golden/fusion_train.pt, rebuilt from their seeds (the fixture keeps digests)."""
    g = torch.Generator().manual_seed(fx["feat_seed"])
    a = torch.randn(fx["B"], fx["T1"], fx["D"], generator=g)
    v = torch.randn(fx["B"], fx["T2"], fx["D"], generator=g)
    v[1, fx["pad_from"]:] = 0.0
    g = torch.Generator().manual_seed(fx["head_seed"])
    hd = {"w.weight": torch.randn(20, fx["D"], generator=g) * 0.03, "w.bias": torch.randn(20, generator=g) * 0.03}
    return a, v, hd


def sampled(t):
    """A tensor cut down to the entries the fixture records: D-sized vectors whole, the rest at 512 fixed positions."""
    t = t.detach().cpu().reshape(-1)
    if t.numel() <= 1024:
        return t.clone()
    idx = torch.randperm(t.numel(), generator=torch.Generator().manual_seed(99))[:512].sort().values
    return t[idx]


def _digest(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(v.detach().contiguous().numpy().tobytes())
    return h.hexdigest()


def test_fusion_fixture_rebuilds_from_its_seeds(golden):
    fx = golden("fusion_train")
    a, v, hd = fixture_inputs(fx)
    assert hashlib.sha256(a.contiguous().numpy().tobytes()).hexdigest() == fx["audio_sha256"]
    assert hashlib.sha256(v.contiguous().numpy().tobytes()).hexdigest() == fx["video_sha256"]
    assert _digest(hd) == fx["head_sha256"]
    assert _digest(W.seeded_fusion_state_dict(fx["D"], fx["F"], seed=fx["fusion_seed"])) == fx["sd_sha256"]
    assert fx["T2"] < fx["T1"] and float(fx["wav_lens"].min()) < 1
    for c in fx["cases"].values():
        assert len(c["params"]) == 5 and set(c["grad0_clipped"]) == set(c["params"][0])
        assert len(c["grad0_clipped"]) == 26
