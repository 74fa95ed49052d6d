"""Generate tests/golden/fusion_train.pt: the audio-visual recipe's step (N20EMv2/audio_visual/train_rca_av.py:174-185) run by the
REFERENCE ITSELF on the CPU.

    python tests/golden/make_golden_fusion_train.py

What runs: the reference's ``fusion.FusionRCA`` (imported by ``make_golden.import_reference``) loaded with
``weights.seeded_fusion_state_dict(1024, 3072, seed=3986)``, ``speechbrain.nnet.linear.Linear`` (20 outputs, seeded), the recipe's
``compute_objectives`` (``bce_loss`` with pos_weight 15 / 1, ``Softmax(apply_log=True)`` + ``nll_loss`` twice, ``length=wav_lens``),
``loss.backward()``, ``check_gradients``' ``clip_grad_norm_(..., 5.0)`` and ``torch.optim.Adadelta(rho=0.95, eps=1e-8)`` over
``ModuleList([fusion, head])``: 5 steps at lr 1.0 and 5 at the recipe's 3e-4, each from the same initial weights.  The fixture holds
data only: seeds and digests of the initial weights and features (rebuilt by the tests), targets, per-step terms and pre-clip norms,
the step-1 (clipped) gradients and every step's parameters at 512 fixed entries of each matrix and of the 3 072-long biases, and every
D-sized vector whole.
"""
from __future__ import annotations

import hashlib
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402
from make_golden import W  # noqa: E402

STEPS = 5
MAX_GRAD_NORM = 5.0
N_SAMPLED = 512
D, F, FUSION_SEED, HEAD_SEED, FEAT_SEED = 1024, 3072, 3986, 4986, 77
B, T1, T2, PAD_FROM = 2, 40, 37, 31


def features():
    """Seeded audio (B, T1, D) and video (B, T2, D) features; clip 1's video zero from PAD_FROM on (PaddedBatch)."""
    g = torch.Generator().manual_seed(FEAT_SEED)
    a = torch.randn(B, T1, D, generator=g)
    v = torch.randn(B, T2, D, generator=g)
    v[1, PAD_FROM:] = 0.0
    return a, v


def head_state():
    g = torch.Generator().manual_seed(HEAD_SEED)
    return {"w.weight": torch.randn(20, D, generator=g) * 0.03, "w.bias": torch.randn(20, generator=g) * 0.03}


def digest(t: torch.Tensor) -> str:
    return hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()


def sample_index(n: int, seed: int) -> torch.Tensor:
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed))[:N_SAMPLED].sort().values


def sampled(k, t):
    """A tensor cut down to the recorded entries: D-sized vectors whole, the rest at sample_index(numel)."""
    t = t.detach().reshape(-1)
    if t.numel() <= D:
        return t.clone()
    return t[sample_index(t.numel(), 99)].clone()


def make_targets(t_tgt, seed):
    g = torch.Generator().manual_seed(seed)
    anno = torch.zeros(B, t_tgt, 4)
    anno[:, :, 0] = (torch.rand(B, t_tgt, generator=g) < 0.15).float()
    anno[:, :, 1] = (torch.rand(B, t_tgt, generator=g) < 0.15).float()
    anno[:, :, 2] = torch.randint(0, 5, (B, t_tgt), generator=g).float()
    anno[:, :, 3] = torch.randint(0, 13, (B, t_tgt), generator=g).float()
    anno[0, 3, 2] = -100.0
    return anno


def run_case(sb, fusion_mod, sd, a, v, wav_lens, anno, lr):
    fusion = fusion_mod.FusionRCA(alpha=0.5, nhead=8, d_ffn=F, d_model=D)
    fusion.load_state_dict({k: t for k, t in sd.items()}, strict=True)
    head = sb.nnet.linear.Linear(n_neurons=20, input_size=D)
    head.load_state_dict(head_state(), strict=True)
    modules = torch.nn.ModuleList([fusion, head])
    opt = torch.optim.Adadelta(modules.parameters(), lr=lr, rho=0.95, eps=1e-8)
    log_softmax = sb.nnet.activations.Softmax(apply_log=True)
    names = [("fusion." + k) for k, _ in fusion.named_parameters()] + [("head." + k) for k, _ in head.named_parameters()]
    terms, norms, params, grad0 = [], [], [], None
    for step in range(STEPS):
        logits = head(fusion(a, v))
        po = logits[:, :, 2:]
        l_on = sb.nnet.losses.bce_loss(logits[:, :, 0], anno[:, :, 0].float(), length=wav_lens, pos_weight=torch.tensor([15.0]))
        l_off = sb.nnet.losses.bce_loss(logits[:, :, 1], anno[:, :, 1].float(), length=wav_lens, pos_weight=torch.tensor([1.0]))
        l_oct = sb.nnet.losses.nll_loss(log_softmax(po[:, :, 0:5]), anno[:, :, 2].long(), length=wav_lens)
        l_cls = sb.nnet.losses.nll_loss(log_softmax(po[:, :, 5:]), anno[:, :, 3].long(), length=wav_lens)
        loss = l_on + l_off + l_oct + l_cls
        loss.backward()
        assert torch.isfinite(loss)
        norms.append(float(torch.nn.utils.clip_grad_norm_(modules.parameters(), MAX_GRAD_NORM)))
        if step == 0:
            grad0 = {n: sampled(n, p.grad) for n, p in zip(names, modules.parameters())}
        opt.step()
        opt.zero_grad()
        terms.append(torch.tensor([l_on.item(), l_off.item(), l_oct.item(), l_cls.item(), loss.item()]))
        params.append({n: sampled(n, p) for n, p in zip(names, modules.parameters())})
    return dict(lr=lr, terms=torch.stack(terms), grad_norms=norms, grad0_clipped=grad0, params=params)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    _, fusion_mod, _ = MG.import_reference()
    import speechbrain as sb
    sd = W.seeded_fusion_state_dict(D, F, seed=FUSION_SEED)
    a, v = features()
    wav_lens = torch.tensor([1.0, 0.8])
    cases = {}
    for key, lr, t_tgt, tseed in (("lr1", 1.0, T1 + 2, 50), ("lr3e-4", 3e-4, T1 - 1, 51)):
        anno = make_targets(t_tgt, tseed)
        c = run_case(sb, fusion_mod, sd, a, v, wav_lens, anno, lr)
        c.update(anno=anno, target_seed=tseed)
        cases[key] = c
        print(key, "terms", c["terms"][0].tolist(), "->", c["terms"][-1].tolist(), "norms", [round(n, 4) for n in c["grad_norms"]])
    fx = dict(D=D, F=F, nhead=8, alpha=0.5, fusion_seed=FUSION_SEED, head_seed=HEAD_SEED, feat_seed=FEAT_SEED, B=B, T1=T1, T2=T2,
              pad_from=PAD_FROM, sd_sha256=MG.sd_digest(sd), head_sha256=MG.sd_digest(head_state()), audio_sha256=digest(a),
              video_sha256=digest(v), wav_lens=wav_lens, rho=0.95, eps=1e-8, max_grad_norm=MAX_GRAD_NORM, cases=cases)
    torch.save(fx, os.path.join(HERE, "fusion_train.pt"))


if __name__ == "__main__":
    main()
