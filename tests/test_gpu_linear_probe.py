"""The linear-probe training step on the MI355X (svt_speechbrain_amd/training.py, csrc/train.hip): the recipe's objective and its
gradient, the head's weight gradient, clip + Adadelta, and LinearProbe end to end against the reference's own trajectory
(tests/golden/linear_probe.pt, tests/golden/make_golden_linear_probe.py)."""
import copy

import pytest
import torch

import svt_speechbrain_amd as S
from svt_speechbrain_amd import _lib
from svt_speechbrain_amd import training as TR
from svt_speechbrain_amd import weights as W
from test_linear_probe_host import fixture_inputs, sampled

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


# ---------------------------------------------------------------- objective
def _targets(B, tt, seed, ignore=True):
    g = torch.Generator().manual_seed(seed)
    on = (torch.rand(B, tt, generator=g) < 0.2).float()
    off = (torch.rand(B, tt, generator=g) < 0.2).float()
    octv = torch.randint(0, 5, (B, tt), generator=g)
    cls = torch.randint(0, 13, (B, tt), generator=g)
    if ignore:
        octv[0, min(1, tt - 1)] = -100
        cls[-1, tt // 2] = -100
    return on, off, octv, cls


def _reference_terms(logits, on, off, octv, cls, rel_len, pw, smoothing, dtype):
    """compute_objectives in plain torch on the CPU (compute_masked_loss / truncate / length_to_mask semantics)."""
    x = logits.to(dtype)
    T = min(x.shape[1], on.shape[1])
    x, on, off, octv, cls = x[:, :T], on[:, :T].to(dtype), off[:, :T].to(dtype), octv[:, :T], cls[:, :T]
    if rel_len is None:
        m = torch.ones(x.shape[0], T, dtype=dtype)
    else:
        lim = (rel_len.float() * T)   # fp32 product, as length_to_mask
        m = (torch.arange(T, dtype=torch.float32)[None, :] < lim[:, None]).to(dtype)
    den = m.sum()
    f = torch.nn.functional
    l_on = (f.binary_cross_entropy_with_logits(x[:, :, 0], on, pos_weight=torch.tensor([pw], dtype=dtype), reduction="none") * m).sum() / den
    l_off = (f.binary_cross_entropy_with_logits(x[:, :, 1], off, reduction="none") * m).sum() / den

    def nll(z, k):
        lp = torch.log_softmax(z, dim=-1)
        loss = (f.nll_loss(lp.transpose(1, 2), k, reduction="none") * m).sum() / den
        if smoothing == 0:
            return loss
        reg = (lp.mean(dim=-1) * m).sum() / den
        return -smoothing * reg + (1 - smoothing) * loss

    return [l_on, l_off, nll(x[:, :, 2:7], octv), nll(x[:, :, 7:], cls)]


CASES = [  # (B, t_pred, t_tgt, rel_len, smoothing)
    (2, 49, 49, None, 0.0),
    (3, 301, 298, [1.0, 0.77, 0.5], 0.0),        # predictions truncated
    (3, 257, 260, [0.93, 1.0, 0.31], 0.1),       # targets truncated, label smoothing
    (1, 1, 1, None, 0.0),
    (4, 513, 514, [0.999, 0.2, 0.6, 1.0], 0.1),
]


@pytest.mark.parametrize("B,tp,tt,rel,ls", CASES)
def test_objective_matches_the_validation_losses_and_fp64_autograd(B, tp, tt, rel, ls):
    g = torch.Generator().manual_seed(B * 1000 + tp)
    logits = 3.0 * torch.randn(B, tp, 20, generator=g)
    on, off, octv, cls = _targets(B, tt, tp)
    rl = torch.tensor(rel) if rel is not None else None
    terms, dlog, host = TR.amt_objective_grad(logits.to(DEV), on, off, octv, cls, rl.to(DEV) if rl is not None else None, 15.0, 4, 3, ls)
    terms = terms.cpu()
    assert host == terms.tolist()
    # the existing validation losses on the same inputs (svt_bce_loss / svt_softmax + svt_nll_loss), within 2e-6 relative
    xd = logits.to(DEV)
    lsm = S.Softmax(apply_log=True)
    rld = rl.to(DEV) if rl is not None else None
    ref = [S.bce_loss(xd[:, :, 0], on.to(DEV), length=rld, pos_weight=torch.tensor([15.0], device=DEV)),
           S.bce_loss(xd[:, :, 1], off.to(DEV), length=rld),
           S.nll_loss(lsm(xd[:, :, 2:7]), octv.to(DEV), length=rld, label_smoothing=ls),
           S.nll_loss(lsm(xd[:, :, 7:]), cls.to(DEV), length=rld, label_smoothing=ls)]
    for i, r in enumerate(ref):
        r = float(r)
        assert abs(float(terms[i]) - r) <= 2e-6 * abs(r), (i, float(terms[i]), r)
    assert float(terms[4]) == float(((terms[0] + terms[1]) + terms[2]) + terms[3])
    # the gradient against fp64 autograd of the same losses
    x64 = logits.double().requires_grad_(True)
    sum(_reference_terms(x64, on, off, octv, cls, rl, 15.0, ls, torch.float64)).backward()
    want = x64.grad
    err = (dlog.cpu().double() - want).abs().max().item()
    assert err <= 1e-5 * want.abs().max().item(), (err, want.abs().max().item())
    # masked and truncated frames are exactly 0
    T = min(tp, tt)
    d = dlog.cpu()
    assert torch.all(d[:, T:] == 0)
    if rl is not None:
        lim = rl.float() * T
        for b in range(B):
            masked = torch.arange(T, dtype=torch.float32) >= lim[b]
            assert torch.all(d[b, :T][masked] == 0)


def test_objective_refusals():
    x = torch.randn(2, 10, 20, device=DEV)
    on, off, octv, cls = _targets(2, 10, 1, ignore=False)
    with pytest.raises(ValueError, match="same length"):
        TR.amt_objective_grad(x, on[:, :6], off[:, :6], octv[:, :6], cls[:, :6])
    with pytest.raises(_lib.SvtError, match="n_out"):
        TR.amt_objective_grad(torch.randn(2, 10, 33, device=DEV), on, off, octv, cls)
    bad = octv.clone()
    bad[1, 4] = 5
    with pytest.raises(_lib.SvtError, match="outside"):
        TR.amt_objective_grad(x, on, off, bad, cls)
    bad = cls.clone()
    bad[0, 0] = -1
    with pytest.raises(_lib.SvtError, match="outside"):
        TR.amt_objective_grad(x, on, off, octv, bad)


def test_objective_is_deterministic():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(16, 499, 20, generator=g).to(DEV)
    on, off, octv, cls = _targets(16, 497, 9)
    rl = torch.rand(16, generator=g).clamp_min(0.3).to(DEV)
    a = TR.amt_objective_grad(x, on, off, octv, cls, rl)
    b = TR.amt_objective_grad(x, on, off, octv, cls, rl)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---------------------------------------------------------------- weight gradient
@pytest.mark.parametrize("D", [512, 768, 1024])
@pytest.mark.parametrize("N", [1, 20, 32])
@pytest.mark.parametrize("rows", [1, 77, 4099, 16001])
def test_weight_gradient_against_fp64(D, N, rows):
    g = torch.Generator().manual_seed(D + N + rows)
    x = torch.randn(rows, D, generator=g)
    dy = torch.randn(rows, N, generator=g) * 1e-3
    dw, db = TR.linear_backward(x.to(DEV), dy.to(DEV))
    want_w = dy.double().t() @ x.double()
    want_b = dy.double().sum(0)
    ew = (dw.cpu().double() - want_w).abs().max().item()
    eb = (db.cpu().double() - want_b).abs().max().item()
    # fp32 sums of `rows` products: error ~ sqrt(rows) * 2^-24 * scale
    tol = 4e-7 * (rows ** 0.5 + 8) * (dy.abs().max().item() * x.abs().max().item())
    assert ew <= tol, (ew, tol)
    assert eb <= 4e-7 * (rows ** 0.5 + 8) * dy.abs().max().item(), eb


def test_weight_gradient_is_bit_identical_across_calls_and_streams():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(15968, 768, generator=g).to(DEV)
    dy = torch.randn(15968, 20, generator=g).to(DEV)
    w0, b0 = TR.linear_backward(x, dy)
    w1, b1 = TR.linear_backward(x, dy)
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        w2, b2 = TR.linear_backward(x, dy)
    with torch.cuda.stream(s2):
        w3, b3 = TR.linear_backward(x, dy)
    torch.cuda.synchronize()
    for w, b in ((w1, b1), (w2, b2), (w3, b3)):
        assert torch.equal(w, w0) and torch.equal(b, b0)


def test_weight_gradient_refusals():
    x = torch.randn(10, 768, device=DEV)
    with pytest.raises(_lib.SvtError, match="out_features"):
        TR.linear_backward(x, torch.randn(10, 33, device=DEV))
    with pytest.raises(_lib.SvtError, match="multiple of 4"):
        TR.linear_backward(torch.randn(10, 766, device=DEV), torch.randn(10, 20, device=DEV))


# ---------------------------------------------------------------- clip + Adadelta
# fp32 agreement with torch's CPU Adadelta + clip_grad_norm_ after 20 steps, max |ours - torch| relative to max |torch| of each tensor
# (parameters, square_avg, acc_delta).  First MI355X run: 3.7e-7 / 5.5e-7 / 4.1e-7 / 5.9e-7 for the four cases -> bound 2e-6.
ADADELTA_BOUND = 2e-6


@pytest.mark.parametrize("clip", [None, 0.5])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_clip_adadelta_matches_torch(clip, wd):
    g = torch.Generator().manual_seed(int(wd * 100) + (1 if clip else 0))
    w0, b0 = torch.randn(20, 768, generator=g) * 0.05, torch.randn(20, generator=g) * 0.05
    grads = [(torch.randn(20, 768, generator=g) * 0.01, torch.randn(20, generator=g) * 0.01) for _ in range(20)]
    pc = [torch.nn.Parameter(w0.clone()), torch.nn.Parameter(b0.clone())]
    pg = [torch.nn.Parameter(w0.clone().to(DEV)), torch.nn.Parameter(b0.clone().to(DEV))]
    oc = torch.optim.Adadelta(pc, lr=1.0, rho=0.95, eps=1e-8, weight_decay=wd)
    og = TR.Adadelta(pg, lr=1.0, rho=0.95, eps=1e-8, weight_decay=wd)
    worst = 0.0
    for gw, gb in grads:
        for p, gr in zip(pc, (gw, gb)):
            p.grad = gr.clone()
        for p, gr in zip(pg, (gw, gb)):
            p.grad = gr.clone().to(DEV)
        if clip:
            torch.nn.utils.clip_grad_norm_(pc, clip)
            og.step(max_norm=clip)
        else:
            og.step()
        oc.step()
    for a, b in zip(pg, pc):
        for ta, tb in ((a.detach(), b.detach()), (og.state[a]["square_avg"], oc.state[b]["square_avg"]),
                       (og.state[a]["acc_delta"], oc.state[b]["acc_delta"])):
            rel = (ta.cpu() - tb).abs().max().item() / max(tb.abs().max().item(), 1e-30)
            worst = max(worst, rel)
        assert float(og.state[a]["step"]) == float(oc.state[b]["step"]) == 20.0
    print(f"clip={clip} wd={wd}: max relative deviation from torch after 20 steps {worst:.3e}")
    assert worst <= ADADELTA_BOUND, worst


def test_state_dict_moves_both_ways_with_torch_adadelta():
    g = torch.Generator().manual_seed(5)
    w = torch.randn(20, 64, generator=g)
    pc = [torch.nn.Parameter(w.clone())]
    pg = [torch.nn.Parameter(w.clone().to(DEV))]
    oc = torch.optim.Adadelta(pc, lr=0.5, rho=0.95, eps=1e-8)
    og = TR.Adadelta(pg, lr=0.5, rho=0.95, eps=1e-8)
    for _ in range(3):
        gr = torch.randn(20, 64, generator=g)
        pc[0].grad, pg[0].grad = gr.clone(), gr.clone().to(DEV)
        oc.step()
        og.step()
    sd = og.state_dict()
    assert sd["param_groups"][0].keys() == oc.state_dict()["param_groups"][0].keys()
    assert set(sd["state"][0]) == {"step", "square_avg", "acc_delta"}
    # ours -> torch (on CPU parameters) and torch -> ours (on GPU parameters)
    pc2 = [torch.nn.Parameter(pg[0].detach().cpu().clone())]
    oc2 = torch.optim.Adadelta(pc2, lr=0.1)
    oc2.load_state_dict(copy.deepcopy(sd))
    pg2 = [torch.nn.Parameter(pc[0].detach().clone().to(DEV))]
    og2 = TR.Adadelta(pg2, lr=0.1)
    og2.load_state_dict(copy.deepcopy(oc.state_dict()))
    assert og2.param_groups[0]["lr"] == 0.5 and og2.param_groups[0]["rho"] == 0.95
    assert og2.state[pg2[0]]["square_avg"].is_cuda
    gr = torch.randn(20, 64, generator=g)
    pc2[0].grad, pg2[0].grad = gr.clone(), gr.clone().to(DEV)
    oc2.step()
    og2.step()
    assert (pg2[0].detach().cpu() - pc2[0].detach()).abs().max().item() <= 1e-5 * pc2[0].abs().max().item()
    og2.param_groups[0]["lr"] = 0.0   # what NewBobScheduler does between epochs
    before = pg2[0].detach().clone()
    pg2[0].grad = gr.clone().to(DEV)
    og2.step()
    assert torch.equal(pg2[0].detach(), before)


def test_adadelta_refuses_cpu_parameters():
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    with pytest.raises(_lib.SvtError):
        TR.Adadelta([p]).step()


# ---------------------------------------------------------------- LinearProbe end to end
def _probe_from_fixture(fx, lr, precision="fp32"):
    cfg = S.PRESETS[fx["cfg"]]
    enc = S.HuggingFaceWav2Vec2(fx["cfg"], None, config=cfg, precision=precision, seed=fx["weight_seed"]).to(DEV)
    head = S.Linear(20, input_size=cfg.hidden_size)
    head.load_state_dict(fixture_inputs(fx)[1])
    head = head.to(DEV)
    probe = S.LinearProbe({"wav2vec2": enc, "model": head}, lr=lr, rho=fx["rho"], eps=fx["eps"],
                          onset_positive_weight=fx["onset_positive_weight"], max_grad_norm=fx["max_grad_norm"])
    return probe, head, enc


# Bounds from the first MI355X run (max over the 5 steps of both cases).  From the waveform (fp32 encoder, whose logits are <= 1e-3 from the
# reference's): terms 1.5e-5 relative, head parameters 1.4e-6 absolute -> bounds 2e-4 / 2e-5, a 13x / 14x margin (Adadelta's first
# steps move a weight by ~lr * 4.5e-4 whatever the gradient's size, so feature error reaches the parameters only through near-zero
# gradients).  From the reference's own features (the head side alone): 2.7e-7 relative, 3.0e-8 absolute -> bounds 2e-6 / 2e-6.  The
# parameters are compared at the fixture's 512 recorded weight entries and the whole bias.
TRAJ_TERMS_REL = 2e-4
TRAJ_PARAM_ABS = 2e-5
FEATS_TERMS_REL = 2e-6
FEATS_PARAM_ABS = 2e-6


@pytest.mark.parametrize("case", ["lr1", "lr3e-4"])
@pytest.mark.parametrize("source", ["wav", "feats"])
def test_linear_probe_reproduces_the_reference_trajectory(golden, case, source):
    fx = golden("linear_probe")
    c = fx["cases"][case]
    probe, head, _ = _probe_from_fixture(fx, c["lr"])
    wav, lens, anno = fixture_inputs(fx)[0].to(DEV), fx["wav_lens"].to(DEV), c["anno"].to(DEV)
    idx = fx["sampled_index"]
    tr, pr = (TRAJ_TERMS_REL, TRAJ_PARAM_ABS) if source == "wav" else (FEATS_TERMS_REL, FEATS_PARAM_ABS)
    worst_t = worst_p = 0.0
    for step in range(len(c["params"])):
        if source == "wav":
            loss = probe.fit_batch(wav, lens, anno)
        else:
            loss = probe.fit_features(fx["feats"].to(DEV), lens, anno)
        got = torch.tensor([probe.last_terms[k] for k in TR.TERMS] + [float(loss)])
        want = c["terms"][step]
        worst_t = max(worst_t, ((got - want).abs() / want.abs()).max().item())
        if step == 0:
            gw = sampled(head.w.weight.grad, idx)
            ref = c["grad0_clipped"]["w.weight"]
            assert (gw - ref).abs().max().item() <= 50 * tr * ref.abs().max().item()
        for k, v in head.state_dict().items():
            worst_p = max(worst_p, (sampled(v, idx) - c["params"][step][k]).abs().max().item())
    print(f"{case}/{source}: max relative term deviation {worst_t:.3e} (bound {tr}), max |param| deviation {worst_p:.3e} (bound {pr})")
    assert worst_t <= tr and worst_p <= pr
    st = probe.optimizer.state_dict()["state"]
    ref_st = c["opt_state"]
    for i in (0, 1):
        for k in ("square_avg", "acc_delta"):
            assert (sampled(st[i][k], idx) - ref_st[i][k]).abs().max().item() <= 0.05 * ref_st[i][k].abs().max().item() + 1e-12
        assert float(st[i]["step"]) == float(ref_st[i]["step"])


def test_no_stale_head_after_a_step_plain_and_fused_tail():
    fx_cfg = S.PRESETS["wav2vec2-base"]
    g = torch.Generator().manual_seed(8)
    wav = (0.1 * torch.randn(2, 16000, generator=g)).clamp_(-1, 1).to(DEV)
    anno = torch.stack([(torch.rand(2, 49, generator=g) < 0.2).float(), (torch.rand(2, 49, generator=g) < 0.2).float(),
                        torch.randint(0, 5, (2, 49), generator=g).float(), torch.randint(0, 13, (2, 49), generator=g).float()], -1)
    enc = S.HuggingFaceWav2Vec2("wav2vec2-base", None, config=fx_cfg, precision="bf16", seed=3).to(DEV)
    head = S.Linear(20, input_size=768)
    head.load_state_dict(W.seeded_head_state_dict(768, 20, seed=4))
    head = head.to(DEV)
    amt = S.AMTForward({"wav2vec2": enc, "model": head})
    for fuse in (False, True):
        amt.fuse_tail = fuse
        amt.compute_forward(wav)   # uploads (and caches) the head's current parameters
    probe = S.LinearProbe({"wav2vec2": enc, "model": head}, lr=1.0)
    probe.fit_batch(wav, None, anno.to(DEV))
    fresh = S.Linear(20, input_size=768)
    fresh.load_state_dict(head.state_dict())
    fresh = fresh.to(DEV)
    assert not torch.equal(head.state_dict()["w.weight"].cpu(), W.seeded_head_state_dict(768, 20, seed=4)["w.weight"])
    for fuse in (False, True):
        amt.fuse_tail = fuse
        amt.compute_forward(wav)
        got = amt.last_logits.clone()
        amt_fresh = S.AMTForward({"wav2vec2": enc, "model": fresh})
        amt_fresh.fuse_tail = fuse
        amt_fresh.compute_forward(wav)
        assert torch.equal(got, amt_fresh.last_logits), fuse


def test_it_learns_on_synthetic_singing():
    from svt_speechbrain_amd import synth
    cfg = S.PRESETS["wav2vec2-base"]
    enc = S.HuggingFaceWav2Vec2("wav2vec2-base", None, config=cfg, precision="bf16", seed=1986).to(DEV)
    head = S.Linear(20, input_size=768)
    head.load_state_dict(W.seeded_head_state_dict(768, 20, seed=77))
    head = head.to(DEV)
    init = copy.deepcopy(head.state_dict())
    probe = S.LinearProbe({"wav2vec2": enc, "model": head}, lr=1.0)
    train, held = _synth_batches(synth, enc, 6, seed=100), _synth_batches(synth, enc, 2, seed=900)
    losses = []
    for step in range(50):
        feats, anno = train[step % len(train)]
        losses.append(float(probe.fit_features(feats, None, anno)))
    first, last = sum(losses[:10]) / 10, sum(losses[-10:]) / 10
    trained = _frame_accuracy(head, held)
    rand = S.Linear(20, input_size=768)
    rand.load_state_dict(init)
    rand = rand.to(DEV)
    base = _frame_accuracy(rand, held)
    print(f"mean loss {first:.4f} (first 10 steps) -> {last:.4f} (last 10); held-out octave / class accuracy {base} -> {trained}")
    assert last < first
    assert trained[0] > base[0] and trained[1] > base[1]


def _synth_batches(synth, enc, n, seed):
    """n batches of 4 clips of 5 s synthetic singing through the frozen encoder: (features, labels) on the GPU."""
    out = []
    for i in range(n):
        wav, lab, _ = synth.synth_singing(4, 5.0, seed=seed + i)
        with torch.no_grad():
            feats = enc(torch.from_numpy(wav).to(DEV))
        out.append((feats, torch.from_numpy(lab[:, :feats.shape[1]]).float().to(DEV)))
    return out


def _frame_accuracy(head, batches):
    hit_o = hit_c = n = 0
    for feats, anno in batches:
        lg = head(feats)
        T = min(lg.shape[1], anno.shape[1])
        o = lg[:, :T, 2:7].argmax(-1)
        c = lg[:, :T, 7:].argmax(-1)
        hit_o += int((o == anno[:, :T, 2].long()).sum())
        hit_c += int((c == anno[:, :T, 3].long()).sum())
        n += o.numel()
    return round(hit_o / n, 4), round(hit_c / n, 4)


def test_nonfinite_loss_skips_the_step_and_patience_raises():
    cfg = S.PRESETS["wav2vec2-base"]
    enc = S.HuggingFaceWav2Vec2("wav2vec2-base", None, config=cfg, precision="bf16", seed=1).to(DEV)
    head = S.Linear(20, input_size=768)
    head.load_state_dict(W.seeded_head_state_dict(768, 20, seed=2))
    head = head.to(DEV)
    probe = S.LinearProbe({"wav2vec2": enc, "model": head}, lr=1.0, nonfinite_patience=3)
    g = torch.Generator().manual_seed(1)
    feats = torch.randn(2, 30, 768, generator=g).to(DEV)
    anno = torch.stack([torch.zeros(2, 30), torch.zeros(2, 30), torch.ones(2, 30), torch.ones(2, 30)], -1).to(DEV)
    probe.fit_features(feats, None, anno)
    bad = feats.clone()
    bad[1, 7, 100] = float("nan")
    before = {k: v.clone() for k, v in head.state_dict().items()}
    st_before = copy.deepcopy(probe.optimizer.state_dict())
    for _ in range(3):
        loss = probe.fit_features(bad, None, anno)
        assert not torch.isfinite(loss)
        for k, v in head.state_dict().items():
            assert torch.equal(v, before[k])
        assert head.w.weight.grad is None
    assert probe.optimizer.state_dict()["state"][0]["step"] == st_before["state"][0]["step"]
    with pytest.raises(ValueError, match="patience"):
        probe.fit_features(bad, None, anno)
    probe.on_epoch_start()
    probe.fit_features(bad, None, anno)   # the count restarts with the epoch
    probe.fit_features(feats, None, anno)
    assert not torch.equal(head.state_dict()["w.weight"], before["w.weight"])
