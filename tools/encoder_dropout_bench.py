"""The encoder in training mode: what the checkpoint's dropouts and layerdrop cost on top of a plain forward.

    python tools/encoder_dropout_bench.py [--out profiles/encoder_dropout.txt]
    python tools/encoder_dropout_bench.py --precisions bf16,fp16 --out profiles/encoder_dropout_fused.txt      (the fused masked attention)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR_N -- python tools/encoder_dropout_bench.py --count-forwards N   (N = 1, 3;
                                                          --count-parse reads the csv statistics, not the rocpd database)
    python tools/encoder_dropout_bench.py --count-parse DIR_1 DIR_3 [--out ...]                                 (appends the launch table)

wav2vec2-base at 8 x 5 s (the recipe's training batch) and 32 x 10 s, bf16 and fp32.  One encoder per precision; the rates are fields
of its config, read per forward, so the variants below share one upload and alternate inside every round (HIP events around ITERS
forwards, median of the rounds).  Layerdrop is held off (skip_layers all False) so that every variant runs the same layers:

    plain            eval(): no state set, the forward of the parent commit
    HF defaults      hidden 0.1, attention 0.1, activation 0.1, feat_proj 0.0 (Wav2Vec2Config's defaults)
    hidden alone     sites 1, 3, 5 and the un-split FFN-2
    activation alone site 4 (the widest tensor: rows x 3072)
    attention alone  site 2, which takes the score-matrix attention
    attention ~ 0    attention_dropout 2^-33: threshold 0, nothing dropped -- what FORCING the score-matrix path costs by itself
    one layer fewer  HF defaults with the last layer skipped: what a skipped layer saves
    ..., fused       HF defaults / attention alone with fused_attention_dropout=True: the mask inside the fused attention kernel
                     (csrc/attention_drop.hip) in place of the score-matrix path; in fp32 the flag changes nothing

The host cost of the draws is taken by the host clock around draw_layerdrop + torch.cuda.initial_seed().  No assertion on the timings:
the tool reports."""
import argparse
import csv
import dataclasses
import glob
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import svt_speechbrain_amd as S  # noqa: E402
from svt_speechbrain_amd import _lib  # noqa: E402
from svt_speechbrain_amd.dropout import draw_layerdrop  # noqa: E402

DEV = "cuda:0"
ZERO = dict(hidden_dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, feat_proj_dropout=0.0, layerdrop=0.0)
VARIANTS = [
    ("HF defaults", dict(hidden_dropout=0.1, attention_dropout=0.1, activation_dropout=0.1), None),
    ("hidden alone", dict(hidden_dropout=0.1), None),
    ("activation alone", dict(activation_dropout=0.1), None),
    ("attention alone", dict(attention_dropout=0.1), None),
    ("attention ~ 0 (score path forced)", dict(attention_dropout=2.0 ** -33), None),
    ("HF defaults, last layer skipped", dict(hidden_dropout=0.1, attention_dropout=0.1, activation_dropout=0.1), "last"),
    ("HF defaults, fused attention", dict(hidden_dropout=0.1, attention_dropout=0.1, activation_dropout=0.1), "fused"),
    ("attention alone, fused attention", dict(attention_dropout=0.1), "fused"),
]


def added_launches(rates, layers, skipped_layers=0):
    """Launches a training-mode forward adds to the plain one (fp32 and bf16 alike at this geometry): site 1 once, sites 3, 4, 5 per
    layer that runs; the attention's own launches change with the path and are not counted here."""
    n = 0
    run = layers - skipped_layers
    if rates.get("hidden_dropout", 0) > 0:
        n += 1 + 2 * run
    if rates.get("activation_dropout", 0) > 0:
        n += run
    return n


def time_rounds(fns, iters, rounds):
    times = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) * 1e3 / iters)
    return [statistics.median(t) for t in times], [(min(t), max(t)) for t in times]


def kernel_calls(d):
    """name -> calls from the kernel statistics rocprofv3 --stats wrote under d."""
    out = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                out[row["Name"]] = out.get(row["Name"], 0) + int(row["Calls"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--precisions", default="bf16,fp32", help="comma-separated precisions of the timed encoders")
    ap.add_argument("--count-forwards", type=int, default=0)
    ap.add_argument("--count-parse", nargs=2, default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def flush(mode):
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, mode) as f:
                f.write("\n".join(lines) + "\n")

    if args.count_parse:
        one, three = (kernel_calls(d) for d in args.count_parse)
        say("launches per plain forward (calls of a 3-forward run minus calls of a 1-forward run, halved; bf16, 32 x 10 s, nothing set):")
        total = 0.0
        for name in sorted(set(one) | set(three)):
            per = (three.get(name, 0) - one.get(name, 0)) / 2
            if per:
                say(f"  {per:6.1f}   {name[:150]}")
                total += per
        say(f"total {total:.1f}" if one and three else "not measured: no kernel statistics found")
        flush("a")
        return

    _lib.require_gpu()
    cfg = S.PRESETS["wav2vec2-base"]
    g = torch.Generator().manual_seed(0)
    if args.count_forwards:
        enc = S.HuggingFaceWav2Vec2("wav2vec2-base", None, config=cfg, precision="bf16", seed=3).to(DEV)
        wav = (0.1 * torch.randn(32, 160000, generator=g)).clamp_(-1, 1).to(DEV)
        with torch.no_grad():
            for _ in range(args.count_forwards):
                enc(wav)
        torch.cuda.synchronize()
        return

    layers = cfg.num_hidden_layers
    none = (False,) * layers
    last = (False,) * (layers - 1) + (True,)
    for prec in args.precisions.split(","):
        enc = S.HuggingFaceWav2Vec2("wav2vec2-base", None, config=cfg, precision=prec, seed=3, freeze=False).to(DEV)
        for B, secs in ((8, 5), (32, 10)):
            L = secs * 16000
            wav = (0.1 * torch.randn(B, L, generator=g)).clamp_(-1, 1).to(DEV)

            def plain():
                enc.eval()
                return enc(wav)

            def variant(rates, skip):
                def run():
                    enc.train()
                    enc.config = dataclasses.replace(cfg, **dict(ZERO, **rates))
                    enc.fused_attention_dropout = skip == "fused"
                    return enc(wav, dropout_seed=1234, dropout_step=0, skip_layers=last if skip == "last" else none)
                return run

            fns = [plain] + [variant(r, s) for _, r, s in VARIANTS]
            iters = (10 if B == 8 else 4) if prec != "fp32" else (4 if B == 8 else 2)
            with torch.no_grad():
                for fn in fns:
                    for _ in range(2):
                        fn()
                torch.cuda.synchronize()
                t, spread = time_rounds(fns, iters, args.rounds)
            enc.config = cfg
            enc.fused_attention_dropout = False
            say(f"encoder forward, wav2vec2-base, {prec}, {B} x {secs} s ({B * cfg.frames(L)} rows), us per forward (median of {args.rounds} rounds of {iters}):")
            say(f"    {'plain (eval mode)':36s} {t[0]:10.1f}   (rounds {spread[0][0]:.1f} .. {spread[0][1]:.1f})")
            for k, (name, rates, skip) in enumerate(VARIANTS, start=1):
                n = added_launches(rates, layers, 1 if skip == "last" else 0)
                extra = t[k] - t[0]
                per = f"; {n} dropout launches outside the attention: {extra / n:6.1f} us each" if n and "attention_dropout" not in rates else ""
                say(f"    {name:36s} {t[k]:10.1f}   (rounds {spread[k][0]:.1f} .. {spread[k][1]:.1f})   {extra:+9.1f} us  {100 * (t[k] / t[0] - 1):+6.2f} %{per}")
        del enc
        torch.cuda.empty_cache()

    draws = []
    for _ in range(200):
        t0 = time.perf_counter()
        draw_layerdrop(layers, 0.1)
        torch.cuda.initial_seed()
        draws.append((time.perf_counter() - t0) * 1e6)
    say(f"host: {layers} layerdrop draws + the device generator's seed: {statistics.median(draws):.1f} us per forward (median of 200)")
    flush("w")


if __name__ == "__main__":
    main()
