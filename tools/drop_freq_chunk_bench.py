"""DropFreq + DropChunk of a training batch: svt_drop_freq_chunk against the reference's own op sequence, on the same device and stream.

    python tools/drop_freq_chunk_bench.py [--batch 32] [--samples 160000] [--out profiles/drop_freq_chunk_bandwidth.txt]

Default: 32 clips of 10 s at 16 kHz, 2 notches, 5 chunks of 1 000 - 2 000 samples per clip (the lobe's top count).  The paths are timed with
HIP events around ITERS back-to-back calls, alternating between them, after a warm-up; the figure per path is the median of the rounds.  The
yardstick is what the reference launches: a conv1d of the (B, 1, T) batch with the (1, 1, 101) filter at padding 50, then one slice
assignment per chunk (B x 5 launches; their host-side index reads are left out: the spans are Python ints here), and the conv1d alone is
timed as a third path.  Two ceilings: HBM bytes -- every sample read once and written once, 8 B T -- and fp32 fused multiply-adds, 101 B T,
at the plain (v_fma_f32: 256 CUs x 4 SIMDs x 16 lanes per clock) and the packed (v_pk_fma_f32: twice that) rate of the shader clock
measured around the timed calls.  The two paths' outputs are compared before anything is timed.  No assertion on the timings: the tool
reports."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import svt_speechbrain_amd as S  # noqa: E402
from svt_speechbrain_amd import _lib, augment as A  # noqa: E402

DEV = "cuda:0"
HBM_TBS = 8.0     # MI355X peak HBM bandwidth, TB/s
STREAM_TBS = 6.0  # what the project's streaming kernels reach
LANES = 256 * 4 * 16   # fp32 lanes per clock: CUs x SIMDs x lanes


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


def shader_ghz(lib, stamps):
    st = stamps.cpu().view(2, 8, 2)
    ghz = [float(st[1, x, 0] - st[0, x, 0]) / float(st[1, x, 1] - st[0, x, 1]) * 0.1 for x in range(8)
           if st[0, x, 1] > 0 and st[1, x, 1] > st[0, x, 1]]
    return statistics.median(ghz) if ghz else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=int, default=160000)
    ap.add_argument("--chunks", type=int, default=5)
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
    B, T = args.batch, args.samples
    g = torch.Generator().manual_seed(0)
    x = (0.1 * torch.randn(B, T, generator=g)).clamp_(-1, 1).to(DEV)
    taps = S.drop_filter(torch.tensor([0.21, 0.63]))
    length = torch.randint(1000, 2001, (B, args.chunks), generator=g)
    start = (torch.rand(B, args.chunks, generator=g) * (T - 2000)).long()
    table = torch.stack([start, start + length], dim=-1).contiguous()
    spans = table.tolist()
    f_d, c_d = taps.to(DEV), table.to(DEV)
    w_d = f_d.view(1, 1, -1)
    out = torch.empty_like(x)
    stream = _lib.stream_ptr(DEV)

    def ours():
        rc = lib.svt_drop_freq_chunk(_lib.ptr(x), B, T, T, _lib.ptr(f_d), taps.numel(), _lib.ptr(c_d), args.chunks, _lib.ptr(out), T, 0, stream)
        assert rc == 0, _lib.last_error()

    def conv_alone():
        return torch.nn.functional.conv1d(x.unsqueeze(1), w_d, padding=taps.numel() // 2)

    def yardstick():
        y = conv_alone()[:, 0]
        for i in range(B):
            for s, e in spans[i]:
                y[i, s:e] = 0.0
        return y

    with torch.no_grad():
        ours()
        ref = yardstick()
        torch.cuda.synchronize()
        diff, scale = (out - ref).abs().max().item(), ref.abs().max().item()
        say(f"{B} x {T} samples, {taps.numel()} taps (2 notches), {args.chunks} chunks of 1000 - 2000 samples per clip "
            f"({int((ref == 0).sum())} dropped samples)")
        say(f"largest |svt_drop_freq_chunk - reference ops| = {diff:.3e} (outputs up to {scale:.3f}); zero masks "
            f"{'equal' if torch.equal(out == 0, ref == 0) else 'DIFFER'}")
        assert diff <= 1e-5 * scale and torch.equal(out == 0, ref == 0), "the two paths disagree"
        fns = [ours, yardstick, conv_alone]
        for fn in fns:
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        stamps = torch.zeros((2, 16), dtype=torch.int64, device=DEV)
        _lib.check(lib.svt_debug_clock(_lib.ptr(stamps[0]), 0, stream), "svt_debug_clock")
        (t_svt, t_ref, t_conv), spread = time_rounds(fns, args.iters, args.rounds)
        _lib.check(lib.svt_debug_clock(_lib.ptr(stamps[1]), 0, stream), "svt_debug_clock")
        torch.cuda.synchronize()
    ghz = shader_ghz(lib, stamps)
    need = 8 * B * T
    fmas = taps.numel() * B * T
    say(f"svt_drop_freq_chunk (1 launch):                  {t_svt:9.1f} us per call   (rounds {spread[0][0]:.1f} .. {spread[0][1]:.1f})")
    say(f"reference ops (conv1d + {B * args.chunks} slice assignments): {t_ref:9.1f} us per call   (rounds {spread[1][0]:.1f} .. {spread[1][1]:.1f})")
    say(f"conv1d alone:                                    {t_conv:9.1f} us per call   (rounds {spread[2][0]:.1f} .. {spread[2][1]:.1f})")
    say(f"ratio reference ops / svt_drop_freq_chunk:       {t_ref / t_svt:9.2f} x;   conv1d alone / svt_drop_freq_chunk: {t_conv / t_svt:.2f} x")
    gbs = need / t_svt * 1e-3
    say(f"HBM ceiling: 8 B T = {need / 1e6:.1f} MB -> {gbs:.0f} GB/s achieved = {gbs / (STREAM_TBS * 1e3) * 100:.0f} % of the {STREAM_TBS:g} TB/s "
        f"streaming rate ({need / STREAM_TBS * 1e-6:.1f} us), {gbs / (HBM_TBS * 1e3) * 100:.0f} % of the {HBM_TBS:g} TB/s peak")
    clock = ghz or 2.4
    plain = fmas / (LANES * clock * 1e3)
    say(f"FMA ceiling: {taps.numel()} B T = {fmas / 1e6:.0f} M fused multiply-adds at {clock:.2f} GHz"
        f"{' (measured around the timed calls, all paths)' if ghz else ' (nominal: no clock stamps)'}: {plain:.1f} us plain = "
        f"{plain / t_svt * 100:.0f} % reached, {plain / 2:.1f} us packed = {plain / 2 / t_svt * 100:.0f} % reached")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
