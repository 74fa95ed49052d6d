"""Generate tests/golden/linear_probe.pt: the recipe's linear-probe stage run by the REFERENCE ITSELF.

Runs only where the reference and HF transformers are importable (as make_golden.py, whose helpers it imports); the fixture it
writes holds data only: seeds and digests of the waveform and the initial head (rebuilt by the tests), the reference encoder's
features, targets, per-step loss terms, and the gradients, parameters and optimizer state at 512 fixed entries of the weight
(`sampled_index`) plus the whole bias.

    python tests/golden/make_golden_linear_probe.py

What runs: the reference's ``HuggingFaceWav2Vec2`` (freeze=True, eval) over HF ``Wav2Vec2Model`` with seeded wav2vec2-base weights on a
ragged batch of two 0.625 s clips,
``speechbrain.nnet.linear.Linear``, ``compute_objectives`` of MIR_ST500/train_audio_ssl.py:50-76 (``bce_loss`` with pos_weight 15,
``bce_loss``, ``Softmax(apply_log=True)`` + ``nll_loss`` twice, all with ``length=wav_lens``), ``loss.backward()``,
``Brain.check_gradients``' ``clip_grad_norm_(..., 5.0)`` and ``torch.optim.Adadelta(rho=0.95, eps=1e-8)``: 5 steps at lr 1.0 and 5 at
the recipe's 3e-4, each from the same seeded head.
"""
from __future__ import annotations

import hashlib
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402
from make_golden import PRESETS, W  # noqa: E402

STEPS = 5
MAX_GRAD_NORM = 5.0
N_SAMPLED = 512    # head weights recorded per tensor and step (of 20 x 768); the bias is recorded whole


def synth_wav(B, L, seed, pad_from):
    """MG.synth_wav with clip 1 zero from `pad_from` on (a ragged batch); the tests rebuild it from these numbers."""
    wav = MG.synth_wav(B, L, seed=seed)
    wav[1, pad_from:] = 0.0
    return wav


def sampled(t, idx):
    """A weight-shaped tensor cut down to the recorded entries (flattened, at `idx`); a bias passes whole."""
    return t.detach().reshape(-1)[idx].clone() if t.dim() == 2 else t.detach().clone()


def make_targets(B, t_tgt, seed):
    g = torch.Generator().manual_seed(seed)
    anno = torch.zeros(B, t_tgt, 4)
    anno[:, :, 0] = (torch.rand(B, t_tgt, generator=g) < 0.15).float()
    anno[:, :, 1] = (torch.rand(B, t_tgt, generator=g) < 0.15).float()
    anno[:, :, 2] = torch.randint(0, 5, (B, t_tgt), generator=g).float()
    anno[:, :, 3] = torch.randint(0, 13, (B, t_tgt), generator=g).float()
    anno[0, 3, 2] = -100.0   # torch's ignore_index reaches nll_loss unchanged
    return anno


def run_case(sb, feats, wav_lens, anno, hd, lr, idx):
    head = sb.nnet.linear.Linear(n_neurons=20, input_size=feats.shape[-1])
    head.load_state_dict(hd, strict=True)
    opt = torch.optim.Adadelta(head.parameters(), lr=lr, rho=0.95, eps=1e-8)
    log_softmax = sb.nnet.activations.Softmax(apply_log=True)
    terms, params, grad0_clipped, norms = [], [], None, []
    for step in range(STEPS):
        logits = head(feats)
        on_l, off_l = logits[:, :, 0], logits[:, :, 1]
        po = logits[:, :, 2:]
        oct_l, cls_l = po[:, :, 0:5], po[:, :, 5:]
        pw = torch.tensor([15.0])
        l_on = sb.nnet.losses.bce_loss(on_l, anno[:, :, 0].float(), length=wav_lens, pos_weight=pw, reduction="mean",
                                       allowed_len_diff=3)
        l_off = sb.nnet.losses.bce_loss(off_l, anno[:, :, 1].float(), length=wav_lens, reduction="mean", allowed_len_diff=3)
        l_oct = sb.nnet.losses.nll_loss(log_softmax(oct_l), anno[:, :, 2].long(), length=wav_lens, reduction="mean", allowed_len_diff=3)
        l_cls = sb.nnet.losses.nll_loss(log_softmax(cls_l), anno[:, :, 3].long(), length=wav_lens, reduction="mean", allowed_len_diff=3)
        loss = l_on + l_off + l_oct + l_cls
        loss.backward()
        assert torch.isfinite(loss)
        norms.append(float(torch.nn.utils.clip_grad_norm_(head.parameters(), MAX_GRAD_NORM)))
        if step == 0:
            grad0_clipped = {k: p.grad.clone() for k, p in head.named_parameters()}
        opt.step()
        opt.zero_grad()
        terms.append(torch.tensor([l_on.item(), l_off.item(), l_oct.item(), l_cls.item(), loss.item()]))
        params.append({k: sampled(v, idx) for k, v in head.state_dict().items()})
    grad0_clipped = {k: sampled(v, idx) for k, v in grad0_clipped.items()}
    st = opt.state_dict()
    opt_state = {i: {"step": v["step"].clone(), "square_avg": sampled(v["square_avg"], idx), "acc_delta": sampled(v["acc_delta"], idx)}
                 for i, v in st["state"].items()}
    return dict(lr=lr, terms=torch.stack(terms), params=params, grad0_clipped=grad0_clipped, grad_norms=norms,
                opt_state=opt_state)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    hi, _, _ = MG.import_reference()
    import speechbrain as sb
    cfg_name, seed, B, L = "wav2vec2-base", 31, 2, 10000
    cfg = PRESETS[cfg_name]
    sd = W.seeded_encoder_state_dict(cfg, seed=seed)
    hd = W.seeded_head_state_dict(cfg.hidden_size, 20, seed=seed + 1000)
    enc = MG.reference_encoder(hi, cfg, sd)
    pad_from = 8000
    wav = synth_wav(B, L, seed + 7, pad_from)
    idx = torch.randperm(20 * cfg.hidden_size, generator=torch.Generator().manual_seed(seed + 99))[:N_SAMPLED].sort().values
    wav_lens = torch.tensor([1.0, 0.8])
    with torch.no_grad():
        feats = enc(wav)
    T = feats.shape[1]
    cases = {}
    for key, lr, t_tgt, tseed in (("lr1", 1.0, T + 2, seed + 50), ("lr3e-4", 3e-4, T - 1, seed + 51)):
        anno = make_targets(B, t_tgt, tseed)
        c = run_case(sb, feats, wav_lens, anno, hd, lr, idx)
        c.update(anno=anno, target_seed=tseed)
        cases[key] = c
        print(key, "terms", c["terms"][0].tolist(), "->", c["terms"][-1].tolist(), "norms", [round(n, 4) for n in c["grad_norms"]])
    # the waveform and the initial head are rebuilt from their seeds by the tests (digests recorded); the feature tensor, the
    # reference encoder's output, is the one input kept whole
    fx = dict(cfg=cfg_name, weight_seed=seed, head_seed=seed + 1000, wav_seed=seed + 7, pad_from=pad_from, B=B, L=L, T=T,
              sd_sha256=MG.sd_digest(sd), wav_sha256=hashlib.sha256(wav.numpy().tobytes()).hexdigest(), head_sha256=MG.sd_digest(hd),
              wav_lens=wav_lens, feats=feats.clone(), sampled_index=idx.to(torch.int32), rho=0.95, eps=1e-8,
              max_grad_norm=MAX_GRAD_NORM, onset_positive_weight=15.0, cases=cases)
    torch.save(fx, os.path.join(HERE, "linear_probe.pt"))
    print("linear_probe", tuple(feats.shape))


if __name__ == "__main__":
    main()
