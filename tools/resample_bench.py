"""Resample + downmix of a whole song: svt_resample against the dense polyphase form as ONE torch conv1d, on the same device and stream.

    python tools/resample_bench.py [--seconds 240] [--orig 44100] [--new 16000] [--out profiles/resample_bandwidth.txt]

Default: a 240 s stereo 44.1 kHz track to mono 16 kHz.  Both paths are timed with HIP events around ITERS back-to-back calls, alternating
between the two, after a warm-up; the figure per path is the median of the rounds.  The yardstick is written here from the table alone: the P
filters laid into one (P, 1, K) kernel -- row p holds w[p] behind first[p] - min(first) zeros, K = max(first) - min(first) + W -- applied
at stride S to the zero-padded channels, the (C, P, units) result read unit by unit, cut to n_out, and averaged over the channels.  Dense:
it multiplies the zeros too (K = 472 taps where 34 are non-zero at 44.1 -> 16 kHz), which is what one library call costs.  Bytes: the algorithm
needs to read every input row once and write every output row once, 4 * (rows * n_in + rows_out * n_out).  The two paths' outputs are compared
before anything is timed; the one assertion is that svt_resample is the faster."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import svt_speechbrain_amd as S  # noqa: E402
from svt_speechbrain_amd import _lib, resample as R  # noqa: E402

DEV = "cuda:0"
HBM_TBS = 8.0   # MI355X peak HBM bandwidth, TB/s


def dense_kernel(first, weights):
    """(P, 1, K) conv1d kernel of the whole table and the left padding it wants."""
    P, W = weights.shape
    lo, hi = int(first.min()), int(first.max())
    k = torch.zeros(P, 1, hi - lo + W)
    for p in range(P):
        k[p, 0, int(first[p]) - lo:int(first[p]) - lo + W] = weights[p]
    return k, -lo


def conv_yardstick(x, kernel, left, S_, n_out):
    """x (C, n) -> (n_out,): pad, one conv1d at stride S, interleave the phases, cut, channel mean."""
    P, K = kernel.shape[0], kernel.shape[2]
    units = -(-n_out // P)
    right = max(0, (units - 1) * S_ + K - left - x.shape[1])
    xp = torch.nn.functional.pad(x, (left, right) if left >= 0 else (0, right))
    if left < 0:
        xp = xp[:, -left:]
    y = torch.nn.functional.conv1d(xp.unsqueeze(1), kernel, stride=S_)[:, :, :units]      # (C, P, units)
    return y.transpose(1, 2).reshape(x.shape[0], -1)[:, :n_out].mean(dim=0)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--orig", type=int, default=44100)
    ap.add_argument("--new", type=int, default=16000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    _lib.require_gpu()
    lib = _lib.load()
    n_in = round(args.seconds * args.orig)
    x = (0.1 * torch.randn(2, n_in, generator=torch.Generator().manual_seed(0))).clamp_(-1, 1).to(DEV)
    rs = S.Resample(args.orig, args.new)
    first, weights, S_ = rs.table()
    first_d, weights_d, _ = rs.table(DEV)
    P, W = weights.shape
    n_out = R.output_samples(n_in, args.orig, args.new)
    out = torch.empty(n_out, dtype=torch.float32, device=DEV)
    kernel, left = dense_kernel(first, weights)
    kernel = kernel.to(DEV)
    stream = _lib.stream_ptr(DEV)

    def ours():
        rc = lib.svt_resample(_lib.ptr(x), 2, n_in, n_in, _lib.ptr(weights_d), _lib.ptr(first_d), P, W, S_, _lib.ptr(out), n_out, n_out, 1, 0, stream)
        assert rc == 0, _lib.last_error()

    def yardstick():
        return conv_yardstick(x, kernel, left, S_, n_out)

    ours()
    ref = yardstick()
    torch.cuda.synchronize()
    diff, scale = (out - ref).abs().max().item(), ref.abs().max().item()
    say(f"{args.seconds:g} s stereo at {args.orig} Hz -> mono at {args.new} Hz: 2 x {n_in} -> {n_out} samples; P = {P}, S = {S_}, W = {W}, "
        f"G = {R.units_per_tile(P, W, S_, True)} units per workgroup; the dense kernel has {kernel.shape[2]} taps per phase")
    say(f"largest |svt_resample - conv1d yardstick| = {diff:.3e} (outputs up to {scale:.3f})")
    assert diff <= 1e-5 * scale, "the two paths disagree"
    fns = [ours, yardstick]
    for fn in fns:
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    (t_svt, t_conv), spread = time_rounds(fns, args.iters, args.rounds)
    need = 4 * (2 * n_in + n_out)
    gbs = need / t_svt * 1e-3
    say(f"svt_resample (1 launch, downmix fused):   {t_svt:9.1f} us per call   (rounds {spread[0][0]:.1f} .. {spread[0][1]:.1f})")
    say(f"conv1d yardstick (pad, conv, mean):       {t_conv:9.1f} us per call   (rounds {spread[1][0]:.1f} .. {spread[1][1]:.1f})")
    say(f"ratio yardstick / svt_resample:           {t_conv / t_svt:9.2f} x")
    say(f"bytes the algorithm needs:                4 * (2 * n_in + n_out) = {need / 1e6:.1f} MB -> {gbs:.0f} GB/s achieved by svt_resample = "
        f"{gbs / (HBM_TBS * 1e3) * 100:.0f} % of the {HBM_TBS:g} TB/s peak")
    say(f"LDS reads of the sums:                    3 * W = {3 * W} per output, {3 * W * n_out * 4 / 1e9:.2f} GB per call")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    assert t_svt < t_conv, "svt_resample is not faster than the conv1d yardstick"


if __name__ == "__main__":
    main()
