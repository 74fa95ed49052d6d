"""Host behaviour of svt_speechbrain_amd.Adam / AdamW without a GPU: the installed torch's constructor, validation messages,
param_groups and state_dict; checkpoints load both ways; CPU parameters are refused loudly; the three trainers take the new classes
and still refuse torch's own."""
import copy

import pytest
import torch

import svt_speechbrain_amd as S
from svt_speechbrain_amd import _lib
from svt_speechbrain_amd import training as TR

PAIRS = [(TR.Adam, torch.optim.Adam), (TR.AdamW, torch.optim.AdamW)]

BAD = [dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(weight_decay=-0.1), dict(betas=(0.9, 1)),
       dict(lr=torch.tensor([1.0, 2.0])), dict(lr=torch.tensor(1e-3), foreach=True), dict(betas=(torch.tensor(0.9), 0.999)),
       dict(betas=(torch.tensor([0.9, 0.9]), torch.tensor(0.999))), dict(betas=(torch.tensor(0.9), torch.tensor(0.999)), foreach=True),
       dict(fused=True, foreach=True)]


@pytest.mark.parametrize("ours,theirs", PAIRS)
def test_constructor_errors_equal_torch(ours, theirs):
    p = torch.nn.Parameter(torch.zeros(3))
    for bad in BAD:
        with pytest.raises((ValueError, RuntimeError)) as want:
            theirs([p], **bad)
        with pytest.raises(type(want.value)) as got:
            ours([p], **bad)
        assert str(got.value) == str(want.value), bad
    with pytest.raises(NotImplementedError, match="differentiable"):
        ours([p], differentiable=True)


@pytest.mark.parametrize("ours,theirs", PAIRS)
def test_defaults_param_groups_and_state_dict_equal_torch(ours, theirs):
    p = torch.nn.Parameter(torch.zeros(3))
    for kw in (dict(), dict(lr=3e-4, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.02, amsgrad=True, maximize=True),
               dict(foreach=False, capturable=True), dict(fused=True), dict(betas=(torch.tensor(0.9), torch.tensor(0.999)))):
        a, b = ours([p], **kw), theirs([p], **kw)
        assert a.defaults == b.defaults, kw
        assert a.state_dict() == b.state_dict(), kw
        assert list(a.param_groups[0]) == list(b.param_groups[0])
    assert ours([p]).defaults["decoupled_weight_decay"] is (ours is TR.AdamW)
    assert TR.Adam([p], decoupled_weight_decay=True).defaults == torch.optim.Adam([p], decoupled_weight_decay=True).defaults
    assert S.Adam is TR.Adam and S.AdamW is TR.AdamW and issubclass(TR.AdamW, TR.Adam) and issubclass(TR.Adam, torch.optim.Optimizer)


@pytest.mark.parametrize("amsgrad", [False, True])
def test_a_torch_adam_state_loads_and_ours_loads_into_torch(amsgrad):
    g = torch.Generator().manual_seed(2)
    ps = [torch.nn.Parameter(torch.randn(4, 3, generator=g)), torch.nn.Parameter(torch.randn(5, generator=g)),
          torch.nn.Parameter(torch.randn(2, generator=g))]
    theirs = torch.optim.Adam(ps, lr=3e-4, amsgrad=amsgrad, weight_decay=0.01)
    for _ in range(3):
        for p in ps[:2]:   # the third parameter never has a gradient: no state
            p.grad = torch.randn(p.shape, generator=g)
        theirs.step()
    sd = theirs.state_dict()
    ours = TR.Adam([torch.nn.Parameter(p.detach().clone()) for p in ps], lr=1.0)
    ours.load_state_dict(copy.deepcopy(sd))
    got = ours.state_dict()
    keys = {"step", "exp_avg", "exp_avg_sq"} | ({"max_exp_avg_sq"} if amsgrad else set())
    assert set(got["state"]) == {0, 1} and all(set(got["state"][i]) == keys for i in (0, 1))
    assert got["param_groups"] == sd["param_groups"] and ours.param_groups[0]["lr"] == 3e-4
    for i in (0, 1):
        st = got["state"][i]
        assert st["step"].dtype == torch.float32 and st["step"].dim() == 0 and st["step"].device.type == "cpu" and float(st["step"]) == 3.0
        for k in keys - {"step"}:
            assert torch.equal(st[k], sd["state"][i][k])
    back = torch.optim.Adam([torch.nn.Parameter(p.detach().clone()) for p in ps], lr=1.0)
    back.load_state_dict(copy.deepcopy(got))
    for p in back.param_groups[0]["params"][:2]:
        p.grad = torch.ones_like(p)
    back.step()   # torch steps on from the state that went through ours
    assert float(back.state_dict()["state"][0]["step"]) == 4.0
    ours.param_groups[0]["lr"] = 1e-5   # what NewBobScheduler does between epochs
    assert ours.state_dict()["param_groups"][0]["lr"] == 1e-5


def test_a_pre_tensor_step_is_converted_as_torch_does():
    p = torch.nn.Parameter(torch.zeros(3))
    ours = TR.Adam([p])
    sd = ours.state_dict()
    sd["state"] = {0: {"step": 7, "exp_avg": torch.zeros(3), "exp_avg_sq": torch.zeros(3)}}
    for k in ("amsgrad", "maximize", "foreach", "capturable", "differentiable", "fused", "decoupled_weight_decay"):
        del sd["param_groups"][0][k]   # a checkpoint older than these keys
    ours.load_state_dict(sd)
    ours.__setstate__({"state": ours.state, "param_groups": ours.param_groups, "defaults": ours.defaults})
    st = ours.state[p]["step"]
    assert torch.is_tensor(st) and st.dtype == torch.float32 and float(st) == 7.0
    assert ours.param_groups[0]["amsgrad"] is False and ours.param_groups[0]["fused"] is None


@pytest.mark.parametrize("ours", [TR.Adam, TR.AdamW])
def test_cpu_parameters_raise(ours):
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    opt = ours([p])
    with pytest.raises(_lib.SvtError, match="no CPU fallback"):
        opt.step()
    assert torch.equal(p.detach(), torch.zeros(4)) and len(opt.state) == 0
    q = torch.nn.Parameter(torch.zeros(4))
    assert ours([q]).step() is None   # no gradient anywhere: nothing to do, nothing raised
    with pytest.raises(_lib.SvtError, match="no CPU fallback"):
        TR.clip_adam_step([p.detach()], [p.grad], [torch.zeros(4)], [torch.zeros(4)], None, [1e-3], [1.0], 1e-3, 0.9, 0.999, 1e-8)


def test_step_refuses_a_clip_over_two_param_groups():
    a, b = torch.nn.Parameter(torch.zeros(2)), torch.nn.Parameter(torch.zeros(2))
    opt = TR.Adam([{"params": [a]}, {"params": [b], "lr": 1e-4}])
    with pytest.raises(NotImplementedError, match="one param group"):
        opt.step(max_norm=1.0)


def test_the_trainers_take_the_new_classes_and_still_refuse_torch_adam():
    head = S.Linear(20, input_size=64)
    for cls in (TR.Adam, TR.AdamW):
        opt = cls(head.parameters(), lr=3e-4)
        assert S.LinearProbe({"wav2vec2": None, "model": head}, optimizer=opt).optimizer is opt
        assert S.VideoProbe({"encoder": None, "head": head}, optimizer=opt).optimizer is opt
    assert isinstance(S.LinearProbe({"wav2vec2": None, "model": head}).optimizer, TR.Adadelta)   # the default is what it was
    for bad in (torch.optim.Adam(head.parameters()), torch.optim.AdamW(head.parameters())):
        with pytest.raises(TypeError):
            S.LinearProbe({"wav2vec2": None, "model": head}, optimizer=bad)
        with pytest.raises(TypeError):
            S.VideoProbe({"encoder": None, "head": head}, optimizer=bad)


def test_the_adam_fixture_rebuilds_from_the_seeds_of_the_adadelta_fixture(golden):
    from test_fusion_train_host import _digest, fixture_inputs
    fx, base = golden("fusion_train_adam"), golden("fusion_train")
    a, v, hd = fixture_inputs(fx)
    for k in ("D", "F", "nhead", "alpha", "fusion_seed", "head_seed", "feat_seed", "B", "T1", "T2", "pad_from", "sd_sha256", "head_sha256",
              "audio_sha256", "video_sha256", "max_grad_norm"):
        assert fx[k] == base[k], k   # the same seeded inputs and the same reduced geometry
    assert _digest(hd) == fx["head_sha256"] and torch.equal(fx["anno"], base["cases"]["lr3e-4"]["anno"])
    assert fx["lr"] == 3e-4 and len(fx["params"]) == 5 and len(fx["params"][0]) == 26 and fx["terms"].shape == (5, 5)
    assert fx["opt_steps"] == [5.0] * 26 and max(fx["grad_norms"]) > fx["max_grad_norm"]   # the clip acts at every step
    assert set(fx["fp32_vs_fp64"]) == {"terms", "norm", "param"} and all(0 < x < 1e-3 for x in fx["fp32_vs_fp64"].values())


def test_the_library_declares_exports_and_binds_the_step():
    assert "svt_clip_adam_step" in _lib.SYMBOLS
    import os
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "svt_mi355.h")).read()
    assert "int svt_clip_adam_step(" in header and "4-byte-aligned" in header
    assert (TR.ADAM_MAXIMIZE, TR.ADAM_AMSGRAD, TR.ADAM_DECOUPLED) == (1, 2, 4)
    for name, value in (("SVT_ADAM_MAXIMIZE", 1), ("SVT_ADAM_AMSGRAD", 2), ("SVT_ADAM_DECOUPLED", 4)):
        assert f"#define {name} {value}" in header
