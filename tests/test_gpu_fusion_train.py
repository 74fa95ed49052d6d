"""The audio-visual recipe's training step on the GPU (train_rca_av.py:174-185): FusionRCA + head on frozen features.  Gradients
are checked against fp64 autograd of the oracle's FusionRCA forward + head + objective; the forward of the training path against
the inference forward bit for bit; the step's weights against a freshly built module."""
import ctypes as C

import pytest
import torch

import svt_speechbrain_amd as S
from svt_speechbrain_amd import _lib
from svt_speechbrain_amd import training as TR
from oracle import svt_oracle as O
from test_gpu_linear_probe import _reference_terms, _targets

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
D_SMALL, F_SMALL = 256, 512


def _modules(precision, nhead, seed=7, D=D_SMALL, F=F_SMALL, max_len=256):  # noqa: N803
    fusion = S.FusionRCA(nhead=nhead, d_ffn=F, d_model=D, precision=precision, max_length=max_len, seed=seed)
    g = torch.Generator().manual_seed(seed + 1000)
    head = S.Linear(20, input_size=D)
    with torch.no_grad():
        head.w.weight.copy_(torch.randn(20, D, generator=g) * 0.05)
        head.w.bias.copy_(torch.randn(20, generator=g) * 0.05)
    return fusion.to(DEV), head.to(DEV)


def _batch(B, T1, T2, D=D_SMALL, seed=3):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(B, T1, D, generator=g)
    v = torch.randn(B, T2, D, generator=g)
    if B > 1 and T2 > 3:
        v[1, T2 - 3:] = 0.0   # the second clip zero-padded, as PaddedBatch does
    on, off, octv, cls = _targets(B, T1, seed + 1)
    anno = torch.stack([on, off, octv.float(), cls.float()], dim=-1)
    lens = torch.tensor([1.0, 0.6][:B]) if B > 1 else torch.tensor([1.0])
    return a, v, anno, lens


def _fp64_grads(fusion, head, a, v, anno, lens):
    sd = {k: t.detach().cpu().double().requires_grad_(k in TR.RCA_KEYS) for k, t in fusion.state_dict().items()}
    w = head.w.weight.detach().cpu().double().requires_grad_(True)
    b = head.w.bias.detach().cpu().double().requires_grad_(True)
    feats = O.fusion_forward(sd, a.double(), v.double(), alpha=fusion.alpha, nhead=fusion.nhead)
    logits = torch.nn.functional.linear(feats, w, b)
    terms = _reference_terms(logits, anno[..., 0], anno[..., 1], anno[..., 2].long(), anno[..., 3].long(), lens, 15.0, 0.0,
                             torch.float64)
    loss = sum(terms)
    loss.backward()
    out = {k: sd[k].grad for k in TR.RCA_KEYS}
    out["w"], out["b"] = w.grad, b.grad
    return out, [float(t.detach()) for t in terms]


def _gpu_grads(fusion, head, a, v, anno, lens):
    tr = TR.FusionTrainer({"fusion": fusion, "head": head}, lr=0.0, max_grad_norm=0.0)
    tr.fit_batch(a.to(DEV), v.to(DEV), lens.to(DEV), anno.to(DEV))
    named = dict(fusion.named_parameters())
    out = {k: named[k].grad.detach().cpu().clone() for k in TR.RCA_KEYS}
    out["w"], out["b"] = head.w.weight.grad.detach().cpu().clone(), head.w.bias.grad.detach().cpu().clone()
    return out, tr


# ---------------------------------------------------------------- forward of the training path
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("T2", [33, 40, 47])
def test_forward_train_is_bit_identical_to_the_forward(precision, T2):
    fusion, _ = _modules(precision, 2)
    a, v, _, _ = _batch(2, 40, T2)
    a, v = a.to(DEV), v.to(DEV)
    ref = fusion(a, v)
    lib = _lib.load()
    slot = fusion._sync(DEV)
    need = lib.svt_rca_train_workspace_bytes(slot.handle, 2, 40)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = torch.empty_like(ref)
    _lib.check(lib.svt_rca_forward_train(slot.handle, _lib.ptr(a), 40, _lib.ptr(v), T2, 2, _lib.ptr(out), _lib.ptr(ws), need,
                                         _lib.stream_ptr(DEV)), "svt_rca_forward_train")
    torch.cuda.synchronize()
    assert torch.equal(out, ref)


# ---------------------------------------------------------------- gradients
@pytest.mark.parametrize("nhead", [2, 4])   # head size 128 / 64
@pytest.mark.parametrize("T,T2", [(1, 1), (7, 9), (129, 131), (129, 118)])   # T2 < T1: the video zero-padded to T1
def test_fp32_gradients_match_fp64_autograd(nhead, T, T2):
    fusion, head = _modules("fp32", nhead)
    a, v, anno, lens = _batch(2, T, T2)
    ref, _ = _fp64_grads(fusion, head, a, v, anno, lens)
    got, tr = _gpu_grads(fusion, head, a, v, anno, lens)
    worst = 0.0
    for k, r in ref.items():
        err = (got[k].double() - r).abs().max().item() / max(r.abs().max().item(), 1e-30)
        worst = max(worst, err)
        assert err <= 1e-4, (k, err)
    print(f"nhead={nhead} T={T} T2={T2}: worst per-tensor error / max|g| = {worst:.3e}")


def test_bf16_gradients_follow_fp32():
    grads = {}
    a, v, anno, lens = _batch(2, 129, 131)
    for prec in ("fp32", "bf16"):
        fusion, head = _modules(prec, 2)
        grads[prec], _ = _gpu_grads(fusion, head, a, v, anno, lens)
    worst = 1.0
    for k in grads["fp32"]:
        x, y = grads["fp32"][k].double().flatten(), grads["bf16"][k].double().flatten()
        cos = float(torch.dot(x, y) / (x.norm() * y.norm()).clamp_min(1e-300))
        worst = min(worst, cos)
        assert cos >= 0.999, (k, cos)   # measured 0.99976 on the first run
    print(f"bf16 vs fp32 step-1 gradients: worst per-tensor cosine {worst:.5f}")


def test_gradients_are_bit_identical_across_calls_and_streams():
    fusion, head = _modules("bf16", 4)
    a, v, anno, lens = _batch(2, 70, 66)
    first, _ = _gpu_grads(fusion, head, a, v, anno, lens)
    second, _ = _gpu_grads(fusion, head, a, v, anno, lens)
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        third, _ = _gpu_grads(fusion, head, a, v, anno, lens)
    side.synchronize()
    for k in first:
        assert torch.equal(first[k], second[k]), k
        assert torch.equal(first[k], third[k]), k


# ---------------------------------------------------------------- the data half of the head's backward
def test_linear_backward_data_against_fp64():
    g = torch.Generator().manual_seed(11)
    dy, w = torch.randn(301, 20, generator=g), torch.randn(20, 1024, generator=g)
    dx = TR.linear_backward_data(dy.to(DEV), w.to(DEV)).cpu()
    ref = dy.double() @ w.double()
    assert (dx.double() - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()


# ---------------------------------------------------------------- clip + Adadelta over the recipe's 26 tensors
def test_clip_adadelta_over_26_tensors_matches_torch():
    g = torch.Generator().manual_seed(26)
    shapes = [(48, 16), (48,), (16, 16), (16,), (64, 16), (64,), (16, 64), (16,)] + [(16,)] * 4
    shapes = shapes * 2 + [(20, 16), (20,)]
    assert len(shapes) == 26
    init = [torch.randn(s, generator=g) * 0.05 for s in shapes]
    pc = [torch.nn.Parameter(t.clone()) for t in init]
    pg = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    oc = torch.optim.Adadelta(pc, lr=1.0, rho=0.95, eps=1e-8)
    og = TR.Adadelta(pg, lr=1.0, rho=0.95, eps=1e-8)
    worst = 0.0
    for _ in range(10):
        gr = [torch.randn(s, generator=g) * 0.5 for s in shapes]
        for p, x in zip(pc, gr):
            p.grad = x.clone()
        for p, x in zip(pg, gr):
            p.grad = x.clone().to(DEV)
        torch.nn.utils.clip_grad_norm_(pc, 5.0)
        og.step(max_norm=5.0)
        oc.step()
    for a, b in zip(pg, pc):
        worst = max(worst, (a.detach().cpu() - b.detach()).abs().max().item() / b.detach().abs().max().item())
    print(f"26 tensors: max relative deviation from torch after 10 steps {worst:.3e}")
    assert worst <= 1e-5, worst


# ---------------------------------------------------------------- the step's weights reach the next forward
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_no_stale_weights_after_a_step(precision):
    fusion, head = _modules(precision, 2)
    a, v, anno, lens = _batch(2, 40, 38)
    a, v = a.to(DEV), v.to(DEV)
    tr = TR.FusionTrainer({"fusion": fusion, "head": head}, lr=1.0)
    tr.fit_batch(a, v, lens.to(DEV), anno.to(DEV))
    lib = _lib.load()
    calls = []
    orig = lib.svt_rca_finalize
    lib.svt_rca_finalize = lambda h: calls.append(h) or orig(h)
    try:
        got = fusion(a, v)
    finally:
        lib.svt_rca_finalize = orig
    assert not calls, "the forward after a step re-uploaded the fusion weights through the host"
    fresh = S.FusionRCA(nhead=2, d_ffn=F_SMALL, d_model=D_SMALL, precision=precision, max_length=256)
    fresh.load_state_dict({k: t.detach().cpu() for k, t in fusion.state_dict().items()})
    fresh = fresh.to(DEV)
    ref = fresh(a, v)
    torch.cuda.synchronize()
    assert torch.equal(got, ref)
    head2 = S.Linear(20, input_size=D_SMALL)
    head2.load_state_dict({k: t.detach().cpu() for k, t in head.state_dict().items()})
    assert torch.equal(head(got), head2.to(DEV)(got))


# ---------------------------------------------------------------- learning and the non-finite skip
def test_loss_falls_over_30_steps_on_synthetic_singing():
    from svt_speechbrain_amd import synth
    cfg = S.PRESETS["wav2vec2-base"]
    enc = S.HuggingFaceWav2Vec2("wav2vec2-base", None, config=cfg, precision="bf16", seed=1986).to(DEV)
    wav, lab, _ = synth.synth_singing(4, 5.0, seed=300)
    with torch.no_grad():
        feats = enc(torch.from_numpy(wav).to(DEV))
    T = feats.shape[1]
    anno = torch.from_numpy(lab[:, :T]).float().to(DEV)
    video = feats[:, 1:].contiguous()   # a second, shifted stream stands in for the lip features (T2 = T1 - 1)
    fusion, head = _modules("bf16", 12, D=768, F=1536, max_len=512)
    tr = TR.FusionTrainer({"fusion": fusion, "head": head}, lr=1.0)
    losses = [float(tr.fit_batch(feats, video, None, anno)) for _ in range(30)]
    first, last = sum(losses[:5]) / 5, sum(losses[-5:]) / 5
    print(f"synthetic singing: mean loss {first:.4f} (first 5 steps) -> {last:.4f} (last 5)")
    assert last < 0.9 * first


def test_nonfinite_loss_skips_the_step_and_patience_raises():
    fusion, head = _modules("fp32", 2)
    a, v, anno, lens = _batch(2, 20, 20)
    anno[0, 0, 0] = float("nan")
    tr = TR.FusionTrainer({"fusion": fusion, "head": head}, lr=1.0, nonfinite_patience=3)
    before = {k: t.detach().clone() for k, t in list(fusion.state_dict().items()) + list(head.state_dict().items())}
    for _ in range(3):
        loss = tr.fit_batch(a.to(DEV), v.to(DEV), lens.to(DEV), anno.to(DEV))
        assert not torch.isfinite(loss)
    after = {k: t.detach() for k, t in list(fusion.state_dict().items()) + list(head.state_dict().items())}
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert all(p.grad is None for p in list(fusion.parameters()) + list(head.parameters()))
    with pytest.raises(ValueError):
        tr.fit_batch(a.to(DEV), v.to(DEV), lens.to(DEV), anno.to(DEV))


# ---------------------------------------------------------------- units: the weight gradient and the attention backward alone
def _wgrad(prec, dys, xs, n_out, n_in, stream=None):
    lib = _lib.load()
    dev_stream = stream.cuda_stream if stream is not None else _lib.stream_ptr(DEV)
    rows = dys[0].shape[0]
    dw = torch.empty(n_out, n_in, device=DEV)
    db = torch.empty(n_out, device=DEV)
    two = len(dys) == 2
    args = lambda ws, nb: (1 if prec == "bf16" else 0, _lib.ptr(dys[0]), dys[0].stride(0), _lib.ptr(xs[0]),  # noqa: E731
                           _lib.ptr(dys[1]) if two else None, dys[1].stride(0) if two else 0, _lib.ptr(xs[1]) if two else None,
                           rows, n_out, n_in, _lib.ptr(dw), _lib.ptr(db), ws, nb, 0, dev_stream)
    nb = C.c_size_t(0)
    _lib.check(lib.svt_debug_rca_wgrad(*args(None, C.byref(nb))), "svt_debug_rca_wgrad")
    ws = torch.empty(int(nb.value), dtype=torch.uint8, device=DEV)
    _lib.check(lib.svt_debug_rca_wgrad(*args(_lib.ptr(ws), C.byref(nb))), "svt_debug_rca_wgrad")
    return dw, db


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("rows,n_out,n_in,segs,ld_extra", [(301, 200, 72, 2, 3), (77, 520, 136, 1, 0), (2049, 1024, 256, 2, 0),
                                                           (5, 33, 8, 1, 5)])
def test_weight_gradient_against_fp64(prec, rows, n_out, n_in, segs, ld_extra):
    g = torch.Generator().manual_seed(rows + n_out)
    pads = [torch.randn(rows, n_out + ld_extra, generator=g) for _ in range(segs)]   # dY rows with a stride wider than N
    dys = [p[:, :n_out] for p in pads]
    dt = torch.bfloat16 if prec == "bf16" else torch.float32
    xs = [torch.randn(rows, n_in, generator=g).to(dt) for _ in range(segs)]
    dys_d = [p.to(DEV)[:, :n_out] for p in pads]
    xs_d = [x.to(DEV).contiguous() for x in xs]
    dw, db = _wgrad(prec, dys_d, xs_d, n_out, n_in)
    ref_w = sum(d.double().t() @ x.double() for d, x in zip(dys, xs))
    ref_b = sum(d.double().sum(0) for d in dys)
    ew = (dw.cpu().double() - ref_w).abs().max().item() / ref_w.abs().max().item()
    eb = (db.cpu().double() - ref_b).abs().max().item() / ref_b.abs().max().item()
    print(f"{prec} rows={rows} N={n_out} C={n_in} segments={segs}: dW {ew:.2e}, db {eb:.2e} of max")
    assert ew <= 1e-5 and eb <= 1e-5, (ew, eb)
    again = _wgrad(prec, dys_d, xs_d, n_out, n_in)
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        other = _wgrad(prec, dys_d, xs_d, n_out, n_in, side)
    side.synchronize()
    assert torch.equal(again[0], dw) and torch.equal(other[0], dw) and torch.equal(again[1], db) and torch.equal(other[1], db)


def _attn_bwd(prec, qkv, qc, os_, oc, dbl, alpha, B, T, H, dh, stream=None):
    lib = _lib.load()
    st = stream.cuda_stream if stream is not None else _lib.stream_ptr(DEV)
    D = H * dh
    dqkv = torch.empty(B * T, 3 * D, device=DEV)
    dqc = torch.empty(B * T, D, device=DEV)
    args = lambda ws, nb: (1 if prec == "bf16" else 0, _lib.ptr(qkv), _lib.ptr(qc), _lib.ptr(os_), _lib.ptr(oc), _lib.ptr(dbl),  # noqa: E731
                           float(alpha), B, T, H, dh, _lib.ptr(dqkv), _lib.ptr(dqc), ws, nb, 0, st)
    nb = C.c_size_t(0)
    _lib.check(lib.svt_debug_rca_attn_bwd(*args(None, C.byref(nb))), "svt_debug_rca_attn_bwd")
    ws = torch.empty(int(nb.value), dtype=torch.uint8, device=DEV)
    _lib.check(lib.svt_debug_rca_attn_bwd(*args(_lib.ptr(ws), C.byref(nb))), "svt_debug_rca_attn_bwd")
    return dqkv, dqc


def _mha(q, k, v, B, T, H, dh):
    sh = lambda x: x.view(B, T, H, dh).transpose(1, 2)  # noqa: E731
    p = torch.softmax(sh(q) @ sh(k).transpose(-1, -2) / dh ** 0.5, dim=-1)
    return (p @ sh(v)).transpose(1, 2).reshape(B * T, H * dh)


@pytest.mark.parametrize("B,T,H,dh,alpha", [(2, 37, 2, 64, 0.5), (1, 130, 1, 128, 0.3), (2, 1, 2, 64, 0.5)])
def test_attention_backward_against_fp64(B, T, H, dh, alpha):
    D = H * dh
    g = torch.Generator().manual_seed(T * 7 + H)
    qkv = torch.randn(B * T, 3 * D, generator=g)
    qc = torch.randn(B * T, D, generator=g)
    dbl = torch.randn(B * T, D, generator=g)
    x = qkv.double().requires_grad_(True)
    y = qc.double().requires_grad_(True)
    o_s = _mha(x[:, :D], x[:, D:2 * D], x[:, 2 * D:], B, T, H, dh)
    o_c = _mha(y, x[:, D:2 * D], x[:, 2 * D:], B, T, H, dh)
    (dbl.double() * (alpha * o_s + (1 - alpha) * o_c)).sum().backward()
    dev = [t.to(DEV).contiguous() for t in (qkv, qc, o_s.detach().float(), o_c.detach().float(), dbl)]
    dqkv, dqc = _attn_bwd("fp32", *dev, alpha, B, T, H, dh)
    for name, got, ref in (("dq_s", dqkv[:, :D], x.grad[:, :D]), ("dk", dqkv[:, D:2 * D], x.grad[:, D:2 * D]),
                           ("dv", dqkv[:, 2 * D:], x.grad[:, 2 * D:]), ("dq_c", dqc, y.grad)):
        err = (got.cpu().double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)
        print(f"B={B} T={T} H={H} dh={dh}: {name} {err:.2e} of max")
        assert err <= 1e-4, (name, err)
    for prec in ("fp32", "bf16"):
        args = dev if prec == "fp32" else [t.to(torch.bfloat16) for t in dev[:4]] + [dev[4]]
        first = _attn_bwd(prec, *args, alpha, B, T, H, dh)
        second = _attn_bwd(prec, *args, alpha, B, T, H, dh)
        side = torch.cuda.Stream(DEV)
        with torch.cuda.stream(side):
            third = _attn_bwd(prec, *args, alpha, B, T, H, dh, side)
        side.synchronize()
        for a_, b_, c_ in zip(first, second, third):
            assert torch.equal(a_, b_) and torch.equal(a_, c_), prec


# ---------------------------------------------------------------- the reference's own trajectory (tests/golden/fusion_train.pt)
@pytest.mark.parametrize("case", ["lr1", "lr3e-4"])
def test_fusion_trainer_reproduces_the_reference_trajectory(golden, case):
    from test_fusion_train_host import fixture_inputs, sampled
    fx = golden("fusion_train")
    c = fx["cases"][case]
    a, v, hd = fixture_inputs(fx)
    fusion = S.FusionRCA(alpha=fx["alpha"], nhead=fx["nhead"], d_ffn=fx["F"], d_model=fx["D"], precision="fp32",
                         seed=fx["fusion_seed"]).to(DEV)
    head = S.Linear(20, input_size=fx["D"])
    head.load_state_dict(hd)
    head = head.to(DEV)
    tr = TR.FusionTrainer({"fusion": fusion, "head": head}, lr=c["lr"], rho=fx["rho"], eps=fx["eps"], max_grad_norm=fx["max_grad_norm"])
    named = {"fusion." + k: p for k, p in fusion.named_parameters()}
    named.update({"head." + k: p for k, p in head.named_parameters()})
    worst = dict(terms=0.0, norm=0.0, grad=0.0, param=0.0)
    for step in range(len(c["params"])):
        tr.fit_batch(a.to(DEV), v.to(DEV), fx["wav_lens"].to(DEV), c["anno"].to(DEV))
        got = torch.tensor([tr.last_terms[k] for k in TR.TERMS])
        ref = c["terms"][step][:4]
        worst["terms"] = max(worst["terms"], ((got - ref).abs() / ref.abs()).max().item())
        norm, rnorm = float(tr.last_grad_norm), c["grad_norms"][step]
        worst["norm"] = max(worst["norm"], abs(norm - rnorm) / rnorm)
        if step == 0:
            for k, r in c["grad0_clipped"].items():
                err = (sampled(named[k].grad) - r).abs().max().item() / max(r.abs().max().item(), 1e-30)
                worst["grad"] = max(worst["grad"], err)
        for k, r in c["params"][step].items():
            worst["param"] = max(worst["param"], (sampled(named[k]) - r).abs().max().item())
    print(f"{case}: terms {worst['terms']:.2e} rel, pre-clip norm {worst['norm']:.2e} rel, step-1 gradients {worst['grad']:.2e} of max, "
          f"parameters {worst['param']:.2e} abs")
    # lr 1.0 diverges in the reference itself (loss 8.3 -> 24.0, pre-clip norms 56 -> 162): a 1e-4 difference at step 1 grows along
    # it, so that case has wider bounds for the later steps' terms and parameters (DESIGN §4.41 records the measured figures)
    terms_bound, param_bound = (1e-3, 1e-4) if case == "lr1" else (1e-4, 1e-5)
    assert worst["terms"] <= terms_bound and worst["norm"] <= 1e-4, worst
    assert worst["grad"] <= 1e-3, worst
    assert worst["param"] <= param_bound, worst
