"""Generate tests/golden/fusion_train_adam.pt: the audio-visual recipe's step (N20EMv2/audio_visual/train_rca_av.py:174-185) run by the
REFERENCE ITSELF on the CPU under the recipes' second optimizer class, ``torch.optim.Adam`` (``wav2vec_opt_class`` / ``encoder_opt_class``).

    python tests/golden/make_golden_fusion_train_adam.py

What runs: everything ``make_golden_fusion_train.py`` runs -- the reference's ``fusion.FusionRCA`` with the same seeded weights, features,
head and reduced geometry, the recipe's ``compute_objectives``, ``loss.backward()``, ``check_gradients``' ``clip_grad_norm_(..., 5.0)`` --
with ``torch.optim.Adam(lr=3e-4)`` over ``ModuleList([fusion, head])`` in place of Adadelta: 5 steps on the targets of that fixture's
``lr3e-4`` case.  The same 5 steps then run in fp64 (modules, features and targets cast to double), and the fixture records the distance
between the two runs: Adam's first steps move every weight by about lr whatever its gradient's size, so an entry whose gradient is
within rounding of zero may step the other way, and that distance is the scale a second fp32 implementation is held to
(tests/test_gpu_adam.py allows 4 x it where it exceeds the Adadelta fixture's bounds).  The fixture holds data only: seeds and digests,
targets, per-step terms and pre-clip norms, every step's parameters at the entries ``make_golden_fusion_train.sampled`` keeps, and the
fp32-to-fp64 distances.
"""
from __future__ import annotations

import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402
import make_golden_fusion_train as FT  # noqa: E402
from make_golden import W  # noqa: E402

LR = 3e-4
TARGET_LEN, TARGET_SEED = FT.T1 - 1, 51   # the Adadelta fixture's lr3e-4 case


def run(sb, fusion_mod, sd, a, v, wav_lens, anno, dtype):
    fusion = fusion_mod.FusionRCA(alpha=0.5, nhead=8, d_ffn=FT.F, d_model=FT.D)
    fusion.load_state_dict({k: t for k, t in sd.items()}, strict=True)
    head = sb.nnet.linear.Linear(n_neurons=20, input_size=FT.D)
    head.load_state_dict(FT.head_state(), strict=True)
    modules = torch.nn.ModuleList([fusion, head]).to(dtype)
    a, v, wav_lens = a.to(dtype), v.to(dtype), wav_lens.to(dtype)
    opt = torch.optim.Adam(modules.parameters(), lr=LR)
    log_softmax = sb.nnet.activations.Softmax(apply_log=True)
    names = [("fusion." + k) for k, _ in fusion.named_parameters()] + [("head." + k) for k, _ in head.named_parameters()]
    terms, norms, params = [], [], []
    for step in range(FT.STEPS):
        logits = head(fusion(a, v))
        po = logits[:, :, 2:]
        l_on = sb.nnet.losses.bce_loss(logits[:, :, 0], anno[:, :, 0].to(dtype), length=wav_lens, pos_weight=torch.tensor([15.0], dtype=dtype))
        l_off = sb.nnet.losses.bce_loss(logits[:, :, 1], anno[:, :, 1].to(dtype), length=wav_lens, pos_weight=torch.tensor([1.0], dtype=dtype))
        l_oct = sb.nnet.losses.nll_loss(log_softmax(po[:, :, 0:5]), anno[:, :, 2].long(), length=wav_lens)
        l_cls = sb.nnet.losses.nll_loss(log_softmax(po[:, :, 5:]), anno[:, :, 3].long(), length=wav_lens)
        loss = l_on + l_off + l_oct + l_cls
        loss.backward()
        assert torch.isfinite(loss)
        norms.append(float(torch.nn.utils.clip_grad_norm_(modules.parameters(), FT.MAX_GRAD_NORM)))
        opt.step()
        opt.zero_grad()
        terms.append(torch.tensor([l_on.item(), l_off.item(), l_oct.item(), l_cls.item(), loss.item()], dtype=torch.float64))
        params.append({n: FT.sampled(n, p) for n, p in zip(names, modules.parameters())})
    steps = [float(opt.state[p]["step"]) for p in modules.parameters()]
    return dict(terms=torch.stack(terms), grad_norms=norms, params=params, opt_steps=steps)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    _, fusion_mod, _ = MG.import_reference()
    import speechbrain as sb
    sd = W.seeded_fusion_state_dict(FT.D, FT.F, seed=FT.FUSION_SEED)
    a, v = FT.features()
    wav_lens = torch.tensor([1.0, 0.8])
    anno = FT.make_targets(TARGET_LEN, TARGET_SEED)
    r32 = run(sb, fusion_mod, sd, a, v, wav_lens, anno, torch.float32)
    r64 = run(sb, fusion_mod, sd, a, v, wav_lens, anno, torch.float64)
    gap = dict(terms=0.0, norm=0.0, param=0.0)
    for step in range(FT.STEPS):
        t32, t64 = r32["terms"][step][:4], r64["terms"][step][:4]
        gap["terms"] = max(gap["terms"], ((t32 - t64).abs() / t64.abs()).max().item())
        gap["norm"] = max(gap["norm"], abs(r32["grad_norms"][step] - r64["grad_norms"][step]) / r64["grad_norms"][step])
        for k, p64 in r64["params"][step].items():
            gap["param"] = max(gap["param"], (r32["params"][step][k].double() - p64).abs().max().item())
    print("terms", r32["terms"][0].tolist(), "->", r32["terms"][-1].tolist(), "norms", [round(n, 4) for n in r32["grad_norms"]])
    print("fp32 vs fp64 over the 5 steps:", gap)
    fx = dict(D=FT.D, F=FT.F, nhead=8, alpha=0.5, fusion_seed=FT.FUSION_SEED, head_seed=FT.HEAD_SEED, feat_seed=FT.FEAT_SEED, B=FT.B,
              T1=FT.T1, T2=FT.T2, pad_from=FT.PAD_FROM, sd_sha256=MG.sd_digest(sd), head_sha256=MG.sd_digest(FT.head_state()),
              audio_sha256=FT.digest(a), video_sha256=FT.digest(v), wav_lens=wav_lens, max_grad_norm=FT.MAX_GRAD_NORM, lr=LR,
              betas=(0.9, 0.999), eps=1e-8, anno=anno, target_seed=TARGET_SEED, terms=r32["terms"].float(), grad_norms=r32["grad_norms"],
              params=r32["params"], opt_steps=r32["opt_steps"], fp32_vs_fp64=gap)
    torch.save(fx, os.path.join(HERE, "fusion_train_adam.pt"))


if __name__ == "__main__":
    main()
