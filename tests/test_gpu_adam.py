"""clip_grad_norm_ + Adam on the MI355X (csrc/adam.hip, svt_clip_adam_step, svt_speechbrain_amd.Adam / AdamW): the kernels alone under
the per-element limits of tests/adam_limit.py, 20-step trajectories against torch on the CPU in fp32 and fp64, checkpoints both ways,
and the trainers with the new optimizer (tests/golden/linear_probe.pt, tests/golden/fusion_train_adam.pt)."""
import copy
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch

import adam_limit as AL
import svt_speechbrain_amd as S
from svt_speechbrain_amd import _lib
from svt_speechbrain_amd import training as TR
from test_linear_probe_host import _objective, fixture_inputs, sampled

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KEYS = ("p", "g", "m", "v", "x")
SENTINEL = 1234.5
CYCLE = (1, 2, 10, 1000)


# ---------------------------------------------------------------- the kernels alone
class Flat:
    """The five arrays of a tensor list as views into five flat device buffers whose other elements hold a sentinel.  offsets[i][k]: the
    element offset (mod 4) from a 16-byte boundary at which array k of tensor i starts."""

    def __init__(self, tensors, offsets):
        self.tensors, self.spans, host = tensors, {}, {}
        for ki, k in enumerate(KEYS):
            pos, spans = 4, []
            for t, off in zip(tensors, offsets):
                while pos % 4 != off[ki]:
                    pos += 1
                spans.append((pos, pos + t[k].size))
                pos += t[k].size + 1
            buf = np.full(pos + 4, SENTINEL, np.float32)
            for t, (a, b) in zip(tensors, spans):
                buf[a:b] = t[k]
            self.spans[k], host[k] = spans, buf
        self.dev = {k: torch.from_numpy(host[k]).to(DEV) for k in KEYS}
        assert all(self.dev[k].data_ptr() % 16 == 0 for k in KEYS)

    def views(self, k):
        return [self.dev[k][a:b] for a, b in self.spans[k]]

    def read(self):
        """([{array: values} per tensor], sentinels untouched)."""
        host = {k: self.dev[k].cpu().numpy() for k in KEYS}
        out, clean = [dict() for _ in self.tensors], True
        for k in KEYS:
            mask = np.ones(host[k].size, bool)
            for i, (a, b) in enumerate(self.spans[k]):
                out[i][k] = host[k][a:b].copy()
                mask[a:b] = False
            clean = clean and bool((host[k][mask].view(np.uint32) == np.float32(SENTINEL).view(np.uint32)).all())
        return out, clean


def _offsets(n, kind):
    if kind == "mixed":   # the arrays of one tensor disagree: that tensor takes 4-byte accesses
        return [[(i + k) % 4 for k in range(5)] for i in range(n)]
    if kind == "cycle":   # every tensor vectorises behind a head of its own
        return [[i % 4] * 5 for i in range(n)]
    return [[int(kind)] * 5 for _ in range(n)]


def _step(numels, steps, h, clip, offsets="0", seed=3, max_norm=None):
    """One call of svt_clip_adam_step on seeded inputs.  Returns what the checks need."""
    tensors, steps = AL.list_inputs(numels, seed, steps)
    flat = Flat(tensors, _offsets(len(tensors), offsets))
    total64 = AL.clip_coef64(tensors, 1.0)[0]
    if clip and max_norm is None:
        max_norm = 0.5 * total64   # a coefficient near 0.5: the clip acts
    total = torch.full((), -1.0, device=DEV)
    bias = [AL.bias(k, h) for k in steps]
    TR.clip_adam_step(flat.views("p"), flat.views("g"), flat.views("m"), flat.views("v"), flat.views("x") if h["amsgrad"] else None,
                      [b[0] for b in bias], [b[1] for b in bias], h["lr"], h["beta1"], h["beta2"], h["eps"], h["wd"], h["maximize"],
                      h["decoupled"], max_norm if clip else 0.0, total)
    torch.cuda.synchronize()
    got, clean = flat.read()
    return dict(tensors=tensors, steps=steps, got=got, clean=clean, total=float(total), total64=total64, max_norm=max_norm, flat=flat)


def _check(r, h, clip, what):
    """Every element of every array inside its limit; the sentinels untouched; the norm and the stored gradients as stated."""
    assert r["clean"], f"{what}: an element outside the tensors was written"
    coef64 = AL.clip_coef64(r["tensors"], r["max_norm"])[1] if clip else 1.0
    worst = dict.fromkeys(KEYS, 0.0)
    for t, k, got in zip(r["tensors"], r["steps"], r["got"]):
        w = AL.worst(got, t, k, h, coef64, clip)
        worst = {a: max(worst[a], w[a]) for a in worst}
    # total_norm: per-tensor norms rounded to fp32 (u each, so u of the total) and the total's own rounding: 2 u
    assert abs(r["total"] - r["total64"]) <= 2 * AL.U * r["total64"] + AL.TINY, (what, r["total"], r["total64"])
    coef32 = AL.coef_from_total(np.float32(r["total"]), r["max_norm"]) if clip else np.float32(1.0)
    for t, got in zip(r["tensors"], r["got"]):
        want = t["g"] * coef32 if clip else t["g"]
        assert np.array_equal(got["g"].view(np.uint32), want.astype(np.float32).view(np.uint32)), f"{what}: stored gradient is not g * coef"
    print(f"{what}: worst |got - fp64| / limit " + " ".join(f"{a}={worst[a]:.3f}" for a in KEYS))
    assert max(worst.values()) <= 1.0, (what, worst)
    return worst


LISTS = {
    "1 tensor, every size": [(n,) for n in AL.NUMELS],
    "2 tensors": [(4099, 0), (AL.CHUNK + 1, 3), (0, 0)],
    "33 tensors": [AL.NUMELS * 3],
    "300 tensors of 1-700": [tuple(int(v) for v in np.random.default_rng(300).integers(1, 701, 300))],
    "512 x 512 beside 1-element tensors": [(1, 512 * 512, 1, 1)],
}


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("name", list(LISTS))
def test_every_element_inside_the_limits_at_every_size_and_list_length(name, clip):
    h = AL.hyper(weight_decay=0.01, amsgrad=True)
    for numels in LISTS[name]:
        steps = [CYCLE[i % 4] for i in range(len(numels))]   # the per-tensor step differs inside one call
        if sum(numels) == 0 and clip:
            continue   # no gradient at all: total 0, nothing to scale (the unclipped call covers the empty list)
        r = _step(numels, steps, h, clip, seed=len(numels))
        _check(r, h, clip, f"{name} {numels if len(numels) < 5 else len(numels)} clip={clip}")


@pytest.mark.parametrize("index", range(24))
def test_every_flag_combination(index):
    clip, h = AL.flag_cases()[index]
    steps = (1, 2, 10, 1000, 2)
    r = _step(AL.MID_LIST, steps, h, clip)
    _check(r, h, clip, f"clip={clip} wd={h['wd']} decoupled={h['decoupled']} amsgrad={h['amsgrad']} maximize={h['maximize']}")
    if not h["amsgrad"]:   # the fifth array is not part of the call
        assert all(np.array_equal(got["x"], t["x"]) for got, t in zip(r["got"], r["tensors"]))


@pytest.mark.parametrize("step", AL.STEPS)
def test_every_step_of_the_cpu_study(step):
    for clip in (False, True):
        h = AL.hyper()
        _check(_step(AL.MID_LIST, step, h, clip), h, clip, f"step {step} clip={clip}")


@pytest.mark.parametrize("offsets", ["0", "1", "2", "3", "cycle", "mixed"])
def test_views_at_every_element_offset_leave_their_neighbours_alone(offsets):
    numels = AL.NUMELS + AL.MID_LIST
    steps = [CYCLE[i % 4] for i in range(len(numels))]
    for clip, h in ((True, AL.hyper(weight_decay=0.01, amsgrad=True)), (False, AL.hyper())):
        r = _step(numels, steps, h, clip, offsets=offsets, seed=9)
        _check(r, h, clip, f"offsets {offsets} clip={clip}")


def test_the_same_call_twice_gives_the_same_bits_and_a_coefficient_of_one_changes_no_gradient():
    numels = AL.NUMELS + (3 * AL.CHUNK + 7,)
    h = AL.hyper(weight_decay=0.01, amsgrad=True)
    first = _step(numels, 2, h, True, offsets="cycle")
    second = _step(numels, 2, h, True, offsets="cycle")
    assert first["total"] == second["total"]
    for a, b in zip(first["got"], second["got"]):
        for k in KEYS:
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    loose = _step(numels, 2, h, True, max_norm=1e6)
    _check(loose, h, True, "max_norm above the norm")
    assert all(np.array_equal(got["g"], t["g"]) for got, t in zip(loose["got"], loose["tensors"]))


def test_the_entry_point_refuses_what_the_header_says_it_refuses():
    lib = _lib.load()
    t = [torch.zeros(8, device=DEV) for _ in range(4)]
    arr = lambda x: (C.c_void_p * 1)(x)  # noqa: E731
    one, nb = (C.c_float * 1)(1.0), C.c_size_t(0)

    def call(n, ptrs, numel, ws=None, nbytes=None, flags=0, vmax=None):
        return lib.svt_clip_adam_step(n, ptrs[0], ptrs[1], ptrs[2], ptrs[3], vmax, (C.c_int64 * 1)(numel), one, one, 1e-3, 0.9, 0.999, 1e-8,
                                      0.0, flags, 0.0, None, ws, nbytes if nbytes is not None else C.byref(nb), 0, _lib.stream_ptr(DEV))

    good = [arr(_lib.ptr(x)) for x in t]
    assert call(1, good, 8) == 0 and nb.value > 0
    ws = torch.empty(int(nb.value), dtype=torch.uint8, device=DEV)
    size = C.c_size_t(ws.numel())
    assert call(0, good, 8) != 0 and "n_tensors" in _lib.last_error()
    assert call(1, good, -1) != 0 and "negative" in _lib.last_error()
    assert call(1, good[:3] + [None], 8, _lib.ptr(ws), C.byref(size)) != 0 and "null" in _lib.last_error()
    assert call(1, good[:3] + [arr(None)], 8, _lib.ptr(ws), C.byref(size)) != 0 and "null" in _lib.last_error()
    assert call(1, good, 8, _lib.ptr(ws), C.byref(size), flags=TR.ADAM_AMSGRAD) != 0 and "null" in _lib.last_error()
    assert call(1, good[:3] + [arr(_lib.ptr(t[3]) + 2)], 8, _lib.ptr(ws), C.byref(size)) != 0 and "aligned" in _lib.last_error()
    small = C.c_size_t(8)
    assert call(1, good, 8, _lib.ptr(ws), C.byref(small)) != 0 and "workspace" in _lib.last_error()
    assert call(1, good[:3] + [arr(None)], 0, _lib.ptr(ws), C.byref(size)) == 0   # a 0-element tensor is skipped, its pointers unread
    torch.cuda.synchronize()
    assert all(float(x.abs().sum()) == 0.0 for x in t)


# ---------------------------------------------------------------- 20-step trajectories against torch on the CPU
# G: the fp32 CPU run's largest deviation from the fp64 CPU run, relative to each tensor's largest magnitude, over parameters and all
# state; the GPU run is held to 4 G (both round the same quantities once per operation, in orders that differ by a fused multiply-add at
# most).  Measured on the MI355X (G / GPU vs fp64): plain 3.27e-7 / 2.98e-7, clip 5.23e-7 / 3.42e-7, wd 4.20e-7 / 3.65e-7, clip+wd
# 3.89e-7 / 3.56e-7, amsgrad 4.26e-7 / 4.01e-7, adamw 7.26e-7 / 6.50e-7.
TRAJ = {"plain": dict(), "clip": dict(clip=0.5), "wd": dict(wd=0.01), "clip+wd": dict(clip=0.5, wd=0.01),
        "amsgrad": dict(clip=0.5, wd=0.01, amsgrad=True), "adamw": dict(clip=0.5, wd=0.01, adamw=True)}


def _deviation(opt, params, ref_opt, ref_params):
    worst = 0.0
    for a, b in zip(params, ref_params):
        pairs = [(a.detach(), b.detach())] + [(opt.state[a][k], ref_opt.state[b][k]) for k in ref_opt.state[b] if k != "step"]
        for ta, tb in pairs:
            worst = max(worst, (ta.cpu().double() - tb).abs().max().item() / max(tb.abs().max().item(), 1e-300))
    return worst


@pytest.mark.parametrize("case", list(TRAJ))
def test_twenty_steps_stay_within_four_times_torchs_own_fp32_error(case):
    cfg = TRAJ[case]
    clip, wd, ams = cfg.get("clip"), cfg.get("wd", 0.0), cfg.get("amsgrad", False)
    g = torch.Generator().manual_seed(len(case) * 7 + int(wd * 100))
    w0, b0 = torch.randn(20, 768, generator=g) * 0.05, torch.randn(20, generator=g) * 0.05
    grads = [(torch.randn(20, 768, generator=g) * 0.01, torch.randn(20, generator=g) * 0.01) for _ in range(20)]
    ours_cls, torch_cls = (TR.AdamW, torch.optim.AdamW) if cfg.get("adamw") else (TR.Adam, torch.optim.Adam)
    runs = {}
    for name, dtype, dev in (("gpu", torch.float32, DEV), ("cpu32", torch.float32, "cpu"), ("cpu64", torch.float64, "cpu")):
        ps = [torch.nn.Parameter(w0.clone().to(device=dev, dtype=dtype)), torch.nn.Parameter(b0.clone().to(device=dev, dtype=dtype))]
        opt = ours_cls(ps, lr=1e-3, weight_decay=wd, amsgrad=ams) if name == "gpu" else \
            torch_cls(ps, lr=1e-3, weight_decay=wd, amsgrad=ams, foreach=False)
        for gw, gb in grads:
            for p, gr in zip(ps, (gw, gb)):
                p.grad = gr.clone().to(device=dev, dtype=dtype)
            if name == "gpu":
                opt.step(max_norm=clip or 0.0)
            else:
                if clip:
                    torch.nn.utils.clip_grad_norm_(ps, clip)
                opt.step()
        runs[name] = (opt, ps)
    torch.cuda.synchronize()
    G = _deviation(*runs["cpu32"], *runs["cpu64"])
    dev_gpu = _deviation(*runs["gpu"], *runs["cpu64"])
    print(f"{case}: G (torch fp32 vs fp64) {G:.3e}, GPU vs fp64 {dev_gpu:.3e}, ratio {dev_gpu / G:.2f}")
    for a, b, c in zip(runs["gpu"][1], runs["cpu32"][1], runs["cpu64"][1]):
        assert float(runs["gpu"][0].state[a]["step"]) == float(runs["cpu32"][0].state[b]["step"]) == \
            float(runs["cpu64"][0].state[c]["step"]) == 20.0
        assert set(runs["gpu"][0].state[a]) == set(runs["cpu32"][0].state[b])
    assert dev_gpu <= 4 * G, (dev_gpu, G)


# ---------------------------------------------------------------- checkpoints, lr = 0, a parameter without a gradient
@pytest.mark.parametrize("amsgrad", [False, True])
def test_state_dict_moves_both_ways_with_torch_adam(amsgrad):
    g = torch.Generator().manual_seed(5)
    w = torch.randn(20, 64, generator=g)
    pc = [torch.nn.Parameter(w.clone())]
    pg = [torch.nn.Parameter(w.clone().to(DEV))]
    oc = torch.optim.Adam(pc, lr=0.01, amsgrad=amsgrad)
    og = TR.Adam(pg, lr=0.01, amsgrad=amsgrad)
    for _ in range(3):
        gr = torch.randn(20, 64, generator=g)
        pc[0].grad, pg[0].grad = gr.clone(), gr.clone().to(DEV)
        oc.step()
        og.step()
    sd = og.state_dict()
    assert sd["param_groups"][0].keys() == oc.state_dict()["param_groups"][0].keys()
    assert set(sd["state"][0]) == set(oc.state_dict()["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} | ({"max_exp_avg_sq"} if amsgrad else set())
    assert sd["state"][0]["step"].device.type == "cpu" and sd["state"][0]["step"].dtype == torch.float32 and sd["state"][0]["step"].dim() == 0
    # ours -> torch (on CPU parameters) and torch -> ours (on GPU parameters)
    pc2 = [torch.nn.Parameter(pg[0].detach().cpu().clone())]
    oc2 = torch.optim.Adam(pc2, lr=0.5)
    oc2.load_state_dict(copy.deepcopy(sd))
    pg2 = [torch.nn.Parameter(pc[0].detach().clone().to(DEV))]
    og2 = TR.Adam(pg2, lr=0.5)
    og2.load_state_dict(copy.deepcopy(oc.state_dict()))
    assert og2.param_groups[0]["lr"] == 0.01 and og2.param_groups[0]["amsgrad"] is amsgrad
    assert og2.state[pg2[0]]["exp_avg"].is_cuda and float(og2.state[pg2[0]]["step"]) == 3.0
    gr = torch.randn(20, 64, generator=g)
    pc2[0].grad, pg2[0].grad = gr.clone(), gr.clone().to(DEV)
    oc2.step()
    og2.step()
    assert (pg2[0].detach().cpu() - pc2[0].detach()).abs().max().item() <= 1e-5 * pc2[0].abs().max().item()
    assert float(og2.state[pg2[0]]["step"]) == float(oc2.state[pc2[0]]["step"]) == 4.0
    og2.param_groups[0]["lr"] = 0.0   # what NewBobScheduler does between epochs, taken to its end
    before = pg2[0].detach().clone()
    moments = {k: v.clone() for k, v in og2.state[pg2[0]].items() if k != "step"}
    pg2[0].grad = (3 * gr).clone().to(DEV)
    og2.step()
    assert torch.equal(pg2[0].detach(), before)
    assert not torch.equal(og2.state[pg2[0]]["exp_avg"], moments["exp_avg"])
    assert not torch.equal(og2.state[pg2[0]]["exp_avg_sq"], moments["exp_avg_sq"])


def test_a_parameter_without_a_gradient_keeps_its_values_and_its_step():
    g = torch.Generator().manual_seed(6)
    init = [torch.randn(33, generator=g), torch.randn(7, 5, generator=g), torch.randn(4100, generator=g)]
    pc = [torch.nn.Parameter(t.clone()) for t in init]
    pg = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    oc, og = torch.optim.Adam(pc, lr=0.01), TR.Adam(pg, lr=0.01)
    for step in range(4):
        for i, (a, b) in enumerate(zip(pc, pg)):
            gr = torch.randn(a.shape, generator=g)
            skip = i == 1 and step in (1, 2)   # the second parameter misses two steps
            a.grad, b.grad = (None, None) if skip else (gr.clone(), gr.clone().to(DEV))
        held = pg[1].detach().clone()
        oc.step()
        og.step()
        if step in (1, 2):
            assert torch.equal(pg[1].detach(), held) and float(og.state[pg[1]]["step"]) == 1.0
        for a, b in zip(pc, pg):
            assert (b.detach().cpu() - a.detach()).abs().max().item() <= 1e-5 * a.detach().abs().max().item()
    assert [float(og.state[p]["step"]) for p in pg] == [float(oc.state[p]["step"]) for p in pc] == [4.0, 2.0, 4.0]


def test_more_tensors_than_the_adadelta_call_takes_with_the_clip():
    g = torch.Generator().manual_seed(40)
    shapes = [(int(n),) for n in torch.randint(1, 300, (40,), generator=g)]
    init = [torch.randn(s, generator=g) * 0.05 for s in shapes]
    pc = [torch.nn.Parameter(t.clone()) for t in init]
    pg = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    oc, og = torch.optim.Adam(pc, lr=1e-3), TR.Adam(pg, lr=1e-3)
    norm = torch.empty((), device=DEV)
    for _ in range(3):
        gr = [torch.randn(s, generator=g) for s in shapes]
        for a, b, x in zip(pc, pg, gr):
            a.grad, b.grad = x.clone(), x.clone().to(DEV)
        want = torch.nn.utils.clip_grad_norm_(pc, 5.0)
        og.step(max_norm=5.0, total_norm=norm)
        oc.step()
        assert abs(float(norm) - float(want)) <= 1e-6 * float(want)
        for a, b in zip(pc, pg):
            assert (b.grad.cpu() - a.grad).abs().max().item() <= 1e-6 * a.grad.abs().max().item()
    for a, b in zip(pc, pg):
        assert (b.detach().cpu() - a.detach()).abs().max().item() <= 1e-5 * a.detach().abs().max().item()


# ---------------------------------------------------------------- the trainers
def _head(fx):
    head = S.Linear(20, input_size=fx["feats"].shape[-1])
    head.load_state_dict(fixture_inputs(fx)[1])
    return head.to(DEV)


def test_linear_probe_with_adam_follows_torch_autograd_and_torch_adam(golden):
    from test_gpu_linear_probe import FEATS_PARAM_ABS, FEATS_TERMS_REL   # the bounds of the Adadelta run from the same features
    fx = golden("linear_probe")
    c = fx["cases"]["lr3e-4"]
    feats, lens, anno, idx = fx["feats"], fx["wav_lens"], c["anno"], fx["sampled_index"]
    hd = fixture_inputs(fx)[1]
    lin = torch.nn.Linear(feats.shape[-1], 20)
    lin.load_state_dict({"weight": hd["w.weight"], "bias": hd["w.bias"]})
    ref_opt = torch.optim.Adam(lin.parameters(), lr=3e-4)
    head = _head(fx)
    probe = S.LinearProbe({"wav2vec2": None, "model": head}, optimizer=S.Adam(head.parameters(), lr=3e-4),
                          onset_positive_weight=fx["onset_positive_weight"], max_grad_norm=fx["max_grad_norm"])
    worst_t = worst_p = 0.0
    for step in range(5):
        terms = _objective(lin(feats), anno, lens, fx["onset_positive_weight"])
        sum(terms).backward()
        want_norm = float(torch.nn.utils.clip_grad_norm_(lin.parameters(), fx["max_grad_norm"]))
        ref_opt.step()
        ref_opt.zero_grad()
        probe.fit_features(feats.to(DEV), lens.to(DEV), anno.to(DEV))
        got = torch.tensor([probe.last_terms[k] for k in TR.TERMS])
        want = torch.tensor([float(t.detach()) for t in terms])
        worst_t = max(worst_t, ((got - want).abs() / want.abs()).max().item())
        assert abs(float(probe.last_grad_norm) - want_norm) <= 1e-5 * want_norm
        sd = head.state_dict()
        worst_p = max(worst_p, (sampled(sd["w.weight"], idx) - sampled(lin.weight, idx)).abs().max().item(),
                      (sd["w.bias"].cpu() - lin.bias.detach()).abs().max().item())
    print(f"LinearProbe + Adam: max relative term deviation {worst_t:.3e} (bound {FEATS_TERMS_REL}), max |param| deviation {worst_p:.3e} "
          f"(bound {FEATS_PARAM_ABS})")
    assert worst_t <= FEATS_TERMS_REL and worst_p <= FEATS_PARAM_ABS
    assert [float(s["step"]) for s in probe.optimizer.state_dict()["state"].values()] == [5.0, 5.0]


def test_fusion_trainer_with_adam_reproduces_the_reference_trajectory(golden):
    from test_fusion_train_host import fixture_inputs as fusion_inputs, sampled as fusion_sampled
    fx = golden("fusion_train_adam")
    a, v, hd = fusion_inputs(fx)
    fusion = S.FusionRCA(alpha=fx["alpha"], nhead=fx["nhead"], d_ffn=fx["F"], d_model=fx["D"], precision="fp32",
                         seed=fx["fusion_seed"]).to(DEV)
    head = S.Linear(20, input_size=fx["D"])
    head.load_state_dict(hd)
    head = head.to(DEV)
    with pytest.raises(TypeError):
        TR.FusionTrainer({"fusion": fusion, "head": head}, optimizer=torch.optim.Adam(head.parameters()))
    opt = S.Adam(list(fusion.parameters()) + list(head.parameters()), lr=fx["lr"], betas=fx["betas"], eps=fx["eps"])
    tr = TR.FusionTrainer({"fusion": fusion, "head": head}, optimizer=opt, max_grad_norm=fx["max_grad_norm"])
    assert tr.optimizer is opt
    named = {"fusion." + k: p for k, p in fusion.named_parameters()}
    named.update({"head." + k: p for k, p in head.named_parameters()})
    worst = dict(terms=0.0, norm=0.0, param=0.0)
    for step in range(len(fx["params"])):
        tr.fit_batch(a.to(DEV), v.to(DEV), fx["wav_lens"].to(DEV), fx["anno"].to(DEV))
        got = torch.tensor([tr.last_terms[k] for k in TR.TERMS])
        ref = fx["terms"][step][:4]
        worst["terms"] = max(worst["terms"], ((got - ref).abs() / ref.abs()).max().item())
        norm, rnorm = float(tr.last_grad_norm), fx["grad_norms"][step]
        worst["norm"] = max(worst["norm"], abs(norm - rnorm) / rnorm)
        for k, r in fx["params"][step].items():
            worst["param"] = max(worst["param"], (fusion_sampled(named[k]) - r).abs().max().item())
    gap = fx["fp32_vs_fp64"]
    # the relative bounds tests/test_gpu_fusion_train.py applies to fusion_train.pt at lr 3e-4; where torch's own fp32 run is further than
    # a quarter of one from its fp64 run on the generator's machine, 4 x that distance (recorded in the fixture) instead
    bound = dict(terms=max(1e-4, 4 * gap["terms"]), norm=max(1e-4, 4 * gap["norm"]), param=max(1e-5, 4 * gap["param"]))
    print(f"FusionTrainer + Adam: terms {worst['terms']:.2e} rel (bound {bound['terms']:.2e}), pre-clip norm {worst['norm']:.2e} rel (bound "
          f"{bound['norm']:.2e}), parameters {worst['param']:.2e} abs (bound {bound['param']:.2e}); torch fp32 vs fp64: {gap}")
    for k in worst:
        assert worst[k] <= bound[k], (k, worst, bound)
    assert [float(opt.state[p]["step"]) for p in opt.param_groups[0]["params"]] == fx["opt_steps"]


# sha256 of the head's weight and bias after ONE LinearProbe.fit_features step with optimizer=None on the features of
# tests/golden/linear_probe.pt (case lr3e-4), taken on the MI355X when Adam was added: the head forward, the objective, the weight gradient
# and svt_clip_adadelta_step (csrc/train.hip, training.Adadelta) are the files of the commit before it, byte for byte
DEFAULT_STEP_SHA256 = "fa92db092c3126628bfa91cbd7e3cdb605d2bb8782e5989082a02d272d2ffc8b"


def _digest(head):
    h = hashlib.sha256()
    for k in ("w.weight", "w.bias"):
        h.update(head.state_dict()[k].detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def test_the_default_optimizer_is_the_adadelta_it_was(golden):
    fx = golden("linear_probe")
    c = fx["cases"]["lr3e-4"]
    digests = []
    for explicit in (False, True):
        head = _head(fx)
        opt = TR.Adadelta(head.parameters(), lr=3e-4, rho=0.95, eps=1e-8) if explicit else None
        probe = S.LinearProbe({"wav2vec2": None, "model": head}, optimizer=opt, onset_positive_weight=fx["onset_positive_weight"],
                              max_grad_norm=fx["max_grad_norm"])
        assert type(probe.optimizer) is TR.Adadelta
        assert (probe.optimizer.defaults["lr"], probe.optimizer.defaults["rho"], probe.optimizer.defaults["eps"]) == (3e-4, 0.95, 1e-8)
        probe.fit_features(fx["feats"].to(DEV), fx["wav_lens"].to(DEV), c["anno"].to(DEV))
        torch.cuda.synchronize()
        digests.append(_digest(head))
    print(f"default optimizer, one step: sha256 {digests[0]}")
    assert digests[0] == digests[1]
    assert digests[0] == DEFAULT_STEP_SHA256
