"""The video recipe's training input side: the per-clip padding pass (svt_video_forward_u8_clips) against the one-crop pass
(svt_video_forward_u8), the frozen-encoder step on top of it, and the reference's op sequence for the same batch.

    python tools/video_train_input_bench.py [--paths u8,clips,probe,reference] [--batch 8] [--frames 250] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -o NAME --output-format csv -- python tools/video_train_input_bench.py --paths clips --trace-only
    python tools/video_train_input_bench.py --summarise DIR/.../NAME_kernel_trace.csv [--launches 20]

Default batch: 8 clips of 250 frames, 96 x 96 -> 88 x 88, bf16, half the clips flipped, every length 250, offsets drawn from a seeded
generator.  Paths:
  u8         SubModel.forward_into(roi): the centre crop of transform_eval (video_pad8_u8_kernel in the 16-bit modes)
  clips      SubModel.forward_into(roi, clips=plan): per-clip crop / flip / length (video_pad8_u8_clips_kernel)
  probe      VideoProbe.fit_batch on the padded uint8 batch (--config, frozen AV-HuBERT encoder + 20-way head)
  reference  the reference's op sequence: numpy transform_train per clip on the host (TrainTransform.__call__), zero padding, the fp32
             upload, then the float entry point
Each path is timed as a whole call: a host clock around `--launches` calls that end in a device synchronise, after `--warmup` calls,
`--rounds` rounds alternating between the paths; median and extremes.  --trace-only runs warm-up + launches of the chosen paths once
and times nothing (for a rocprofv3 kernel trace, which slows the host); --summarise reads such a trace and prints, per padding kernel,
the LAST `--launches` launches' durations: median, min, max.  --root imports the package from another built checkout (the parent
commit's, for an A/B on the same box in the same session).  No assertion on the timings: the tool reports."""
import argparse
import csv
import os
import random
import statistics
import sys
import time

HERE_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def summarise(path, launches, say):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = {}
    for r in rows:
        n = r["Kernel_Name"]
        if "video_pad" not in n:
            continue
        n = n.replace("void svt::(anonymous namespace)::", "").replace("svt::(anonymous namespace)::", "").split("(")[0]
        per.setdefault(n, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    say(f"{path}: {len(rows)} kernel launches")
    for n, d in per.items():
        last = d[-launches:]
        say(f"  {n}: last {len(last)} of {len(d)} launches: median {statistics.median(last):.2f} us, min {min(last):.2f}, max {max(last):.2f} "
            f"(max - min {max(last) - min(last):.2f})")
        say("    " + " ".join(f"{v:.2f}" for v in last))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", default="u8,clips,probe,reference")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=250)
    ap.add_argument("--roi", type=int, default=96)
    ap.add_argument("--crop", type=int, default=88)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--config", default="avhubert-large-video")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--summarise", nargs="*", default=None)
    ap.add_argument("--root", default=HERE_ROOT)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def finish():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write("\n".join(lines) + "\n")

    if args.summarise is not None:
        for p in args.summarise:
            summarise(p, args.launches, say)
        return finish()

    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import svt_speechbrain_amd as S
    from svt_speechbrain_amd import _lib
    from svt_speechbrain_amd.video import SubModel

    _lib.require_gpu()
    paths = [p for p in args.paths.split(",") if p]
    B, T, R, crop = args.batch, args.frames, args.roi, args.crop
    g = torch.Generator().manual_seed(0)
    roi_host = torch.randint(0, 256, (B, T, R, R), generator=g, dtype=torch.uint8)
    roi = roi_host.to(DEV)
    cfg = S.PRESETS[args.config]
    fns = {}
    fe = SubModel(512, cfg.hidden_size, "prelu", precision=args.precision, seed=1).to(DEV)
    say(f"{B} clips x {T} frames, {R} x {R} -> {crop} x {crop}, {args.precision}, package {os.path.abspath(args.root)}")
    if "u8" in paths:
        tf_eval = S.EvalTransform(crop=(crop, crop))
        fns["u8"] = lambda: fe.forward_into(roi, transform=tf_eval)
    if "clips" in paths or "reference" in paths or "probe" in paths:
        rng = random.Random(0)
        tf = S.TrainTransform(crop=(crop, crop), rng=rng)
        plan = [c._replace(flip=b % 2) for b, c in enumerate(tf.plan([T] * B, R, R))]   # exactly half the clips flipped
        say("clips (dy, dx, flip, n_frames): " + " ".join(str(tuple(c)) for c in plan))
    if "clips" in paths:
        fns["clips"] = lambda: fe.forward_into(roi, transform=tf, clips=plan)
    if "reference" in paths:
        def reference():
            x = torch.zeros((B, 1, T, crop, crop), dtype=torch.float32)
            for b, c in enumerate(plan):
                x[b, 0, :c.n_frames] = torch.from_numpy(tf(roi_host[b, :c.n_frames].numpy(), draw=(c.dy, c.dx, bool(c.flip))))
            return fe.forward_into(x.to(DEV))
        fns["reference"] = reference
    if "probe" in paths:
        from svt_speechbrain_amd import weights as W
        enc = S.FairseqAVHubertPretrain(config=cfg, precision=args.precision, seed=1, output_norm=True).to(DEV)
        head = S.Linear(20, input_size=cfg.hidden_size)
        head.load_state_dict(W.seeded_head_state_dict(cfg.hidden_size, 20, seed=2))
        probe = S.VideoProbe({"encoder": enc, "head": head.to(DEV)}, transform=tf)
        anno = torch.stack([(torch.rand(B, T, generator=g) < 0.1).float(), (torch.rand(B, T, generator=g) < 0.1).float(),
                            torch.randint(0, 5, (B, T), generator=g).float(), torch.randint(0, 13, (B, T), generator=g).float()], -1).to(DEV)
        lens = torch.ones(B)
        fns["probe"] = lambda: probe.fit_batch(roi, lens, anno)
    if "clips" in fns and "reference" in fns:
        a, b = fns["clips"]().clone(), fns["reference"]()
        say(f"clips path == reference op sequence, bit for bit: {torch.equal(a, b)}")
        assert torch.equal(a, b), "the two paths disagree"
    for fn in fns.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    if args.trace_only:
        for name, fn in fns.items():
            for _ in range(args.launches):
                fn()
            torch.cuda.synchronize()
            say(f"{name}: {args.warmup} warm-up + {args.launches} calls, not timed")
        return finish()
    times = {k: [] for k in fns}
    for _ in range(args.rounds):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.launches):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / args.launches)
    for name, t in times.items():
        say(f"{name:10s} {statistics.median(t):9.3f} ms per call   (rounds {min(t):.3f} .. {max(t):.3f}; {args.launches} calls per round, {args.rounds} rounds)")
    finish()


if __name__ == "__main__":
    main()
