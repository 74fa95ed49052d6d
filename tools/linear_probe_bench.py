"""Steps/s of the linear-probe training step (LinearProbe.fit_batch: frozen encoder + head side) against the forward alone
(AMTForward.compute_forward) at the same batch, and HIP-event times of each part of the step:

    encoder | head forward | objective (+ its one stream sync) | weight gradient | clip + Adadelta

plus the weight-gradient kernel's effective bandwidth (bytes of X, dY and the slab partials moved / time).

    python tools/linear_probe_bench.py [--steps 20] [--warmup 3] [--configs c2-bf16,c2-fp16x3,recipe-bf16] [--json OUT]

c2-*: 32 clips x 10 s, wav2vec2-base (feat_dim 768); recipe-bf16: the recipe's own shape, 8 x 5 s, wav2vec2-large (feat_dim 1024).
One line of text per configuration and, with --json, the numbers."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import svt_speechbrain_amd as S  # noqa: E402
from svt_speechbrain_amd import training as TR  # noqa: E402
from svt_speechbrain_amd import weights as W  # noqa: E402

CONFIGS = {
    "c2-bf16": ("wav2vec2-base", "bf16", 32, 160000),
    "c2-fp16x3": ("wav2vec2-base", "fp16x3", 32, 160000),
    "recipe-bf16": ("wav2vec2-large-lv60", "bf16", 8, 80000),
}
PARTS = ("encoder", "head_forward", "objective", "weight_grad", "clip_update")


def run(name, steps, warmup, dev):
    model, prec, B, L = CONFIGS[name]
    cfg = S.PRESETS[model]
    enc = S.HuggingFaceWav2Vec2(model, None, config=cfg, precision=prec, seed=1986).to(dev)
    head = S.Linear(20, input_size=cfg.hidden_size)
    head.load_state_dict(W.seeded_head_state_dict(cfg.hidden_size, 20, seed=7))
    head = head.to(dev)
    modules = {"wav2vec2": enc, "model": head}
    probe = S.LinearProbe(modules, lr=3e-4, rho=0.95, eps=1e-8)
    amt = S.AMTForward(modules)
    g = torch.Generator().manual_seed(0)
    wav = (0.1 * torch.randn(B, L, generator=g)).clamp_(-1, 1).to(dev)
    with torch.no_grad():
        T = enc(wav).shape[1]
    anno = torch.stack([(torch.rand(B, T, generator=g) < 0.1).float(), (torch.rand(B, T, generator=g) < 0.1).float(),
                        torch.randint(0, 5, (B, T), generator=g).float(), torch.randint(0, 13, (B, T), generator=g).float()], -1).to(dev)
    lens = torch.ones(B, device=dev)

    def timed(fn, n):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / n

    fwd_s = timed(lambda: amt.compute_forward(wav, lens), steps)
    fit_s = timed(lambda: probe.fit_batch(wav, lens, anno), steps)

    # the parts of one step, each between a pair of HIP events on the current stream
    ev = {p: [] for p in PARTS}
    w, b = head.w.weight, head.w.bias
    for i in range(warmup + steps):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(len(PARTS) + 1)]
        e[0].record()
        with torch.no_grad():
            feats = enc(wav)
        e[1].record()
        logits = head(feats)
        e[2].record()
        terms, dlog, host = TR.amt_objective_grad(logits, anno[:, :, 0], anno[:, :, 1], anno[:, :, 2].long(), anno[:, :, 3].long(), lens)
        e[3].record()
        if w.grad is None:
            w.grad, b.grad = torch.empty_like(w), torch.empty_like(b)
        TR.linear_backward(feats.reshape(-1, feats.shape[-1]), dlog.reshape(-1, dlog.shape[-1]), w.grad, b.grad)
        e[4].record()
        probe.optimizer.step(max_norm=5.0)
        e[5].record()
        torch.cuda.synchronize()
        if i >= warmup:
            for k, p in enumerate(PARTS):
                ev[p].append(e[k].elapsed_time(e[k + 1]) * 1e3)
    med = {p: sorted(v)[len(v) // 2] for p, v in ev.items()}
    # the weight-gradient kernels alone: back-to-back calls between one pair of events (the per-part times above include the host
    # time of each call, as the step does)
    xf, dl = feats.reshape(-1, feats.shape[-1]), dlog.reshape(-1, dlog.shape[-1])
    ws = {}
    wsq = lambda q: ws.setdefault("w", TR._workspace(q, dev))  # noqa: E731
    for _ in range(warmup):
        TR.linear_backward(xf, dl, w.grad, b.grad, workspace=wsq)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        TR.linear_backward(xf, dl, w.grad, b.grad, workspace=wsq)
    e1.record()
    torch.cuda.synchronize()
    wg_us = e0.elapsed_time(e1) * 1e3 / steps
    rows, D = B * T, cfg.hidden_size
    tiles = -(-D // 256)
    slabs = max(1, min(-(-256 // tiles), -(-rows // 64)))   # csrc/train.hip linear_wgrad_slabs
    x_bytes = rows * D * 4
    moved = x_bytes + rows * 20 * 4 + 2 * slabs * 20 * D * 4
    head_side = med["head_forward"] + med["objective"] + med["weight_grad"] + med["clip_update"]
    step_us = sum(med.values())
    out = dict(config=name, model=model, precision=prec, batch=B, seconds=L / 16000, frames=T, feat_dim=D,
               fit_batch_steps_per_s=1.0 / fit_s, compute_forward_steps_per_s=1.0 / fwd_s,
               parts_us_median=med, head_side_us=head_side, head_side_share=head_side / step_us,
               weight_grad_kernels_us=wg_us, weight_grad_x_gb_per_s=x_bytes / (wg_us * 1e-6) / 1e9,
               weight_grad_all_bytes_gb_per_s=moved / (wg_us * 1e-6) / 1e9, x_mb=x_bytes / 1e6)
    print(f"{name}: fit_batch {out['fit_batch_steps_per_s']:.2f} steps/s vs compute_forward {out['compute_forward_steps_per_s']:.2f}; "
          + ", ".join(f"{p} {med[p]:.1f} us" for p in PARTS)
          + f"; head side {head_side:.1f} us = {100 * out['head_side_share']:.2f} % of the step; weight-gradient kernels alone {wg_us:.1f} us, {x_bytes / 1e6:.1f} MB of X at "
          f"{out['weight_grad_x_gb_per_s']:.0f} GB/s ({out['weight_grad_all_bytes_gb_per_s']:.0f} GB/s counting dY and the partials)",
          flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = [run(c, a.steps, a.warmup, dev) for c in a.configs.split(",")]
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
