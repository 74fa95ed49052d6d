"""SpecAugment inside the encoder: svt_spec_augment against torch's two index_puts, the host draw + upload, and its share of a forward.

    python tools/spec_augment_bench.py [--batch 32] [--samples 160000] [--out profiles/spec_augment.txt]

Default: the C2 shape, 32 clips of 10 s through wav2vec2-base, so the masked tensor is (32, 499, 768) fp32 (49 MB).  Three measurements:

1. the kernel alone with masks drawn at HF's defaults (p 0.05, length 10, min_masks 2) and at the pre-training setting (p 0.65, length
   10), each with and without a feature mask (p 0.2, length 2; HF's default leaves it at 0), against what HF's
   _mask_hidden_states launches on the same buffer: ``h[time] = embed`` and ``h[feature[:, None].expand(-1, T, -1)] = 0`` with boolean
   device masks (a nonzero with its host synchronisation and, for the feature mask, a (B, T, D) boolean temporary each).  Timed with HIP
   events around ITERS back-to-back calls, the paths alternating, after a warm-up; the figure is the median of the rounds.  The bytes the
   kernel has to move are counted from the masks: 4 D per time-masked frame written, and per other frame of a clip with masked columns
   the 16-byte pieces that hold one (read unless wholly masked, written).
2. the host side of one step: the draws (numpy) and the pinned staging + asynchronous copy, by the host clock, the copy's end awaited.
3. one encoder forward (bf16 mode, the benchmark's precision) with the masks drawn per call in training mode, with explicit masks
   already on the device, and plain, alternating, by HIP events around ITERS forwards.

No assertion on the timings: the tool reports.  The two paths' outputs are compared bit for bit before anything is timed."""
import argparse
import dataclasses
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import svt_speechbrain_amd as S  # noqa: E402
from svt_speechbrain_amd import _lib, spec_augment as SA  # noqa: E402

DEV = "cuda:0"
STREAM_TBS = 6.0  # what the project's streaming kernels reach, TB/s


def time_rounds(fns, iters, rounds):
    """Median over `rounds` of the event time per call, in us, of each function; the functions alternate inside a round."""
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


def kernel_bytes(tm, fm, D):
    """Bytes svt_spec_augment reads and writes for these masks (h and embed; the mask bytes themselves are B T + B D per job more)."""
    B, T = tm.shape if tm is not None else (fm.shape[0], 0)
    rd = wr = 0
    for b in range(fm.shape[0] if fm is not None else B):
        n_t = int(tm[b].sum()) if tm is not None else 0
        rd += n_t * D * 4          # embed (L2-resident after the first frame)
        wr += n_t * D * 4
        if fm is not None and fm[b].any():
            pieces = fm[b].reshape(-1, 4)
            touched, whole = int(pieces.any(1).sum()), int(pieces.all(1).sum())
            other = (tm.shape[1] if tm is not None else T) - n_t
            wr += other * touched * 16
            rd += other * (touched - whole) * 16
    return rd, wr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=int, default=160000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    _lib.require_gpu()
    lib = _lib.load()
    cfg = S.PRESETS["wav2vec2-base"]
    B, L, D = args.batch, args.samples, cfg.hidden_size
    T = cfg.frames(L)
    stream = _lib.stream_ptr(DEV)
    g = torch.Generator().manual_seed(0)
    h0 = torch.randn(B, T, D, generator=g).to(DEV)
    embed = torch.rand(D, generator=g).to(DEV)
    say(f"masked tensor ({B}, {T}, {D}) fp32 = {h0.numel() * 4 / 1e6:.1f} MB; a pass over all of it at {STREAM_TBS:g} TB/s would take "
        f"{2 * h0.numel() * 4 / STREAM_TBS * 1e-6:.1f} us (read + write)")

    # ---- 1. the kernel against torch's index_puts
    np.random.seed(0)
    settings = [("HF defaults: time p 0.05 / 10 / min 2", (0.05, 10, 2), None), ("time p 0.65 / 10", (0.65, 10, 2), None),
                ("HF defaults + feature p 0.2 / 2", (0.05, 10, 2), (0.2, 2, 0)), ("time p 0.65 / 10 + feature p 0.2 / 2", (0.65, 10, 2), (0.2, 2, 0))]
    with torch.no_grad():
        for name, tp, fp in settings:
            tm = SA.compute_mask_indices((B, T), *tp)
            fm = SA.compute_mask_indices((B, D), *fp) if fp else None
            tm_d = torch.from_numpy(tm).to(DEV)
            fm_d = torch.from_numpy(fm).to(DEV) if fm is not None else None
            tm_u = tm_d.to(torch.uint8)
            fm_u = fm_d.to(torch.uint8) if fm is not None else None
            h = h0.clone()

            def ours():
                rc = lib.svt_spec_augment(_lib.ptr(h), B, T, D, D, _lib.ptr(tm_u), _lib.ptr(fm_u) if fm_u is not None else None,
                                          _lib.ptr(embed), 0, stream)
                assert rc == 0, _lib.last_error()

            def index_puts():
                h[tm_d] = embed
                if fm_d is not None:
                    h[fm_d[:, None].expand(-1, T, -1)] = 0

            ours()
            a = h.clone()
            h.copy_(h0)
            index_puts()
            torch.cuda.synchronize()
            assert torch.equal(a.view(torch.int32), h.view(torch.int32)), "the two paths disagree"
            for fn in (ours, index_puts):
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            (t_k, t_t), spread = time_rounds([ours, index_puts], args.iters, args.rounds)
            rd, wr = kernel_bytes(tm, fm, D)
            say(f"{name}: {int(tm.sum())} of {B * T} frames time-masked"
                + (f", {int(fm.sum())} of {B * D} columns feature-masked" if fm is not None else ""))
            say(f"    svt_spec_augment (1 launch):        {t_k:9.1f} us per call   (rounds {spread[0][0]:.1f} .. {spread[0][1]:.1f});  "
                f"{(rd + wr) / 1e6:.2f} MB to move -> {(rd + wr) / t_k * 1e-3:.0f} GB/s")
            say(f"    torch index_put{'s (2)' if fm is not None else ' (1)  '}:              {t_t:9.1f} us per call   (rounds {spread[1][0]:.1f} .. {spread[1][1]:.1f});  "
                f"ratio {t_t / t_k:.1f} x")

    # ---- 2. the host side of a step
    stg = SA.MaskStaging()
    cfg_d = cfg   # HF's defaults
    for name, c in (("HF defaults", cfg_d), ("time p 0.65 / 10", dataclasses.replace(cfg, mask_time_prob=0.65))):
        draws, ups = [], []
        for _ in range(50):
            t0 = time.perf_counter()
            tm, fm = SA.draw_masks(c, B, T)
            t1 = time.perf_counter()
            stg.upload(torch.device(DEV), tm, fm)
            torch.cuda.current_stream().synchronize()
            t2 = time.perf_counter()
            draws.append((t1 - t0) * 1e6)
            ups.append((t2 - t1) * 1e6)
        say(f"host, {name}: draw {statistics.median(draws):.0f} us, staging + copy (awaited) {statistics.median(ups):.0f} us per step (medians of 50)")

    # ---- 3. one forward with and without the masks
    wav = (0.1 * torch.randn(B, L, generator=g)).clamp_(-1, 1).to(DEV)
    enc = S.HuggingFaceWav2Vec2("wav2vec2-base", None, config=cfg, precision=args.precision, seed=3, apply_spec_augment=True, freeze=False).to(DEV)
    np.random.seed(1)
    tm_x = torch.from_numpy(SA.compute_mask_indices((B, T), 0.05, 10, 2)).to(DEV)

    def plain():
        enc.model.eval()
        return enc(wav)

    def drawn():
        enc.model.train()
        return enc(wav)

    def explicit():
        enc.model.eval()
        return enc(wav, mask_time_indices=tm_x)

    with torch.no_grad():
        fns = [plain, drawn, explicit]
        for fn in fns:
            for _ in range(max(2, args.warmup // 2)):
                fn()
        torch.cuda.synchronize()
        (t_p, t_d, t_e), spread = time_rounds(fns, max(4, args.iters // 4), args.rounds)
        say(f"encoder forward, {args.precision}, {B} x {L / 16000:g} s:")
        say(f"    plain (eval mode):                  {t_p:9.1f} us   (rounds {spread[0][0]:.1f} .. {spread[0][1]:.1f})")
        say(f"    masks drawn per call (HF defaults): {t_d:9.1f} us   (rounds {spread[1][0]:.1f} .. {spread[1][1]:.1f})   {100 * (t_d / t_p - 1):+.2f} %")
        say(f"    explicit device mask:               {t_e:9.1f} us   (rounds {spread[2][0]:.1f} .. {spread[2][1]:.1f})   {100 * (t_e / t_p - 1):+.2f} %")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
