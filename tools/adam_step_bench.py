"""Time of one clip + Adam step (svt_speechbrain_amd.Adam.step: csrc/adam.hip) for four parameter lists, beside the bytes the step must
move and beside torch's own clip_grad_norm_(foreach=True) + torch.optim.Adam(fused=True) on clones of the same tensors:

    head            the 20-way head of wav2vec2-large features (2 tensors)
    fusion+head     FusionRCA (d_model 1024, d_ffn 3072) + head (26 tensors)
    wav2vec2-base   every parameter shape of the preset (config.PRESETS; random values, no encoder object)
    wav2vec2-large  likewise

    python tools/adam_step_bench.py [--rounds 7] [--lists head,fusion+head,wav2vec2-base,wav2vec2-large] [--out profiles/adam_step.txt]

Each figure is the median over the rounds of (HIP-event time around `inner` back-to-back steps) / inner; the two implementations alternate
inside every round, on the same device in the same process.  The event span holds the host's work per step too (the Python of either
optimizer), as a training loop's does.  Bytes: 28 per parameter (read p, g, m, v; write p, m, v), +4 with the clip (the sum of squares reads
g once more), +8 with amsgrad; the fraction is bytes / time over the 8 TB/s peak of HBM3E."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import svt_speechbrain_amd as S  # noqa: E402
from svt_speechbrain_amd import weights as W  # noqa: E402

PEAK = 8e12   # bytes/s (MI355X HBM3E)


def shapes_of(name):
    if name == "head":
        return [(20, 1024), (20,)]
    if name == "fusion+head":
        sh = [s for k, s in W.fusion_param_shapes(1024, 3072).items() if not k.endswith("positional_encoding.pe")]
        return sh + [(20, 1024), (20,)]
    return list(W.encoder_param_shapes(S.PRESETS[name], False).values())


def step_bytes(numel, clip, amsgrad):
    """Bytes the step must move: read p, g, m, v and write p, m, v; the clip's sum of squares reads g once more; amsgrad reads and writes one
    more array.  (The scaled gradient the clip writes back is not counted: a step need not keep it.)"""
    return numel * (28 + (4 if clip else 0) + (8 if amsgrad else 0))


def torch_optimizer(params, amsgrad, dev):
    """torch.optim.Adam(fused=True) where this torch build has it (probed on a throwaway parameter), else foreach=True."""
    try:
        probe = torch.nn.Parameter(torch.zeros(8, device=dev))
        probe.grad = torch.zeros_like(probe)
        torch.optim.Adam([probe], fused=True).step()
        return torch.optim.Adam(params, lr=3e-4, amsgrad=amsgrad, fused=True), "fused"
    except (RuntimeError, ValueError):
        return torch.optim.Adam(params, lr=3e-4, amsgrad=amsgrad, foreach=True), "foreach"


def bench(name, clip, amsgrad, rounds, dev):
    shapes = shapes_of(name)
    numel = sum(int(torch.Size(s).numel()) for s in shapes)
    g = torch.Generator(device=dev).manual_seed(1)
    init = [torch.randn(s, generator=g, device=dev) * 0.05 for s in shapes]
    grads = [torch.randn(s, generator=g, device=dev) * 0.01 for s in shapes]
    ours_p = [torch.nn.Parameter(t.clone()) for t in init]
    torch_p = [torch.nn.Parameter(t.clone()) for t in init]
    ours = S.Adam(ours_p, lr=3e-4, amsgrad=amsgrad)
    theirs, kind = torch_optimizer(torch_p, amsgrad, dev)
    norm = torch.empty((), device=dev)
    max_norm = 5.0 if clip else 0.0

    def ours_step():
        ours.step(max_norm=max_norm, total_norm=norm if clip else None)

    def torch_step():
        if clip:
            torch.nn.utils.clip_grad_norm_(torch_p, 5.0, foreach=True)
        theirs.step()

    inner = 50 if numel < 50_000_000 else 10
    times = {"ours": [], "torch": []}
    for r in range(rounds + 1):   # round 0 warms both up
        for p, q, x in zip(ours_p, torch_p, grads):
            p.grad, q.grad = x.clone(), x.clone()
        for key, fn in (("ours", ours_step), ("torch", torch_step)):
            fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if r > 0:
                times[key].append(e0.elapsed_time(e1) * 1e-3 / inner)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    spread = {k: (min(v), max(v)) for k, v in times.items()}
    dev_max = max((a.detach() - b.detach()).abs().max().item() for a, b in zip(ours_p, torch_p))
    must = step_bytes(numel, clip, amsgrad)
    return dict(list=name, tensors=len(shapes), numel=numel, clip=clip, amsgrad=amsgrad, torch_kind=kind, ours_s=med["ours"], torch_s=med["torch"],
                ours_spread=spread["ours"], torch_spread=spread["torch"], must_bytes=must,
                ours_frac=must / med["ours"] / PEAK, torch_frac=must / med["torch"] / PEAK, max_param_diff=dev_max, inner=inner)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--lists", default="head,fusion+head,wav2vec2-base,wav2vec2-large")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adam_step_bench needs the GPU: there is nothing to time without it")
    dev = torch.device("cuda:0")
    lines = [f"# tools/adam_step_bench.py --rounds {args.rounds} --lists {args.lists}",
             f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; median of {args.rounds} rounds of HIP-event time / inner steps; peak 8 TB/s",
             "# must: bytes the step has to move (28 B/param, +4 clip, +8 amsgrad); frac: must / time / 8 TB/s; (min..max) over the rounds",
             f"{'list':15s} {'tensors':>7s} {'params':>11s} {'clip':>4s} {'ams':>3s} {'must MB':>9s} {'ours us':>10s} {'(min..max)':>19s} {'frac':>6s} "
             f"{'torch us':>10s} {'(min..max)':>19s} {'frac':>6s} {'torch':>7s} {'ours/torch':>10s} {'max|dp|':>9s}"]
    for name in args.lists.split(","):
        for amsgrad in (False, True):
            for clip in (False, True):
                r = bench(name, clip, amsgrad, args.rounds, dev)
                lines.append(f"{r['list']:15s} {r['tensors']:7d} {r['numel']:11d} {str(r['clip'])[0]:>4s} {str(r['amsgrad'])[0]:>3s} {r['must_bytes'] / 1e6:9.2f} "
                             f"{r['ours_s'] * 1e6:10.1f} {'(%.1f..%.1f)' % (r['ours_spread'][0] * 1e6, r['ours_spread'][1] * 1e6):>19s} {r['ours_frac']:6.3f} "
                             f"{r['torch_s'] * 1e6:10.1f} {'(%.1f..%.1f)' % (r['torch_spread'][0] * 1e6, r['torch_spread'][1] * 1e6):>19s} {r['torch_frac']:6.3f} "
                             f"{r['torch_kind']:>7s} {r['ours_s'] / r['torch_s']:10.2f} {r['max_param_diff']:9.2e}")
                print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
