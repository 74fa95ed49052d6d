"""Noise mixing at the recipes' five SNRs: svt_noise_mix against the reference's chain of elementwise torch ops on the same device and stream.

    python tools/noise_sweep_bench.py [--n 3840000] [--snrs -10 -5 0 5 10] [--out profiles/noise_mix_bandwidth.txt]
    python tools/noise_sweep_bench.py --table [--clips 32] [--held-out] [--out profiles/noise_sweep_f1_by_snr.txt]

Default: a 4-minute song (n = 3 840 000 samples), S = 5.  Both paths are timed with HIP events around ITERS back-to-back calls, alternating
between the two, after a warm-up; the figure per path is the median of the rounds.  The torch chain does what synthesis_noise.py:123-137 does
per SNR on the GPU -- clone, in-place scale, compute_amplitude of the clean track and of the (already rescaled) noise, in-place rescale
of the noise, in-place add -- without a host round trip.  Bytes: the algorithm needs to read both tracks twice (amplitudes, mix) and write S
rows: (2 + 2 + S) * 4 * n.  The two paths' outputs are compared before anything is timed.

--table: white noise on seeded synthetic singing (svt_speechbrain_amd/synth.py: `clips` 10 s clips as one song, utterances of 10 s) through
NoiseSweep with the trained-like head of tests/golden/trained_like_head.pt: COn / COnP / COnPOff F1 against the clips' ground-truth notes
per SNR and precision mode, beside the clean song."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import svt_speechbrain_amd as S  # noqa: E402
from svt_speechbrain_amd import _lib, scoring  # noqa: E402

DEV = "cuda:0"
HBM_TBS = 8.0   # MI355X peak HBM bandwidth, TB/s


def torch_chain(clean, noise, snrs, out):
    """The reference's steps, SNR after SNR, on (1, n) GPU tensors; the noise tensor is rescaled in place like the reference's."""
    noise = noise.clone()
    for s, snr in enumerate(snrs):
        sig = out[s:s + 1]
        sig.copy_(clean)                        # the reference's audio.clone(), into the row it is saved from
        clean_amplitude = torch.mean(torch.abs(clean), dim=1, keepdim=True)
        f = 1 / (10 ** (snr / 20) + 1)
        new_noise_amplitude = f * clean_amplitude
        sig *= 1 - f
        noise_amplitude = torch.mean(torch.abs(noise), dim=1, keepdim=True)
        noise *= new_noise_amplitude / (noise_amplitude + 1e-14)
        sig += noise
    return out


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


def bandwidth(args, say):
    _lib.require_gpu()
    n, snrs = args.n, tuple(args.snrs)
    g = torch.Generator().manual_seed(0)
    clean = (0.1 * torch.randn(n, generator=g)).clamp_(-1, 1).to(DEV)
    noise = torch.randn(n, generator=g).to(DEV)
    out = torch.empty((len(snrs), n), dtype=torch.float32, device=DEV)
    out_t = torch.empty_like(out)
    S.mix_at_snrs(clean, noise, snrs, out=out)
    torch_chain(clean[None], noise[None], snrs, out_t)
    torch.cuda.synchronize()
    diff = (out - out_t).abs().max().item()
    scale = out_t.abs().max().item()
    say(f"n = {n} samples ({n / 16000:.0f} s at 16 kHz), S = {len(snrs)} SNRs {list(snrs)} dB")
    say(f"largest |svt_noise_mix - torch chain| = {diff:.3e} (rows up to {scale:.3f}: the chain takes its amplitudes in fp32 and rescales the noise in place)")
    assert diff <= 1e-5 * scale, "the two paths disagree"
    fns = [lambda: S.mix_at_snrs(clean, noise, snrs, out=out), lambda: torch_chain(clean[None], noise[None], snrs, out_t)]
    for fn in fns:
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    (t_svt, t_torch), spread = time_rounds(fns, args.iters, args.rounds)
    need = (2 + 2 + len(snrs)) * 4 * n
    say(f"svt_noise_mix (2 launches):       {t_svt:9.1f} us per call   (rounds {spread[0][0]:.1f} .. {spread[0][1]:.1f})")
    say(f"torch elementwise chain:          {t_torch:9.1f} us per call   (rounds {spread[1][0]:.1f} .. {spread[1][1]:.1f})")
    say(f"ratio torch / svt_noise_mix:      {t_torch / t_svt:9.2f} x")
    gbs = need / t_svt * 1e-3
    say(f"bytes the algorithm needs:        (2 + 2 + {len(snrs)}) * 4 * n = {need / 1e6:.1f} MB -> {gbs:.0f} GB/s achieved by svt_noise_mix = "
        f"{gbs / (HBM_TBS * 1e3) * 100:.0f} % of the {HBM_TBS:g} TB/s peak")
    # per SNR: clone r+w, scale r+w, abs r+w and mean r for each of the two amplitudes, noise rescale r+w, add 2r+w
    passes_torch = len(snrs) * (2 + 2 + 3 + 3 + 2 + 3)
    say(f"track passes: svt_noise_mix {4 + len(snrs)}, torch chain {passes_torch} (byte ratio {passes_torch / (4 + len(snrs)):.1f})")
    if t_torch / t_svt < 0.5 * passes_torch / (4 + len(snrs)):
        say("the time ratio is below half the byte ratio: see the note at the end of the file")
    assert t_svt < t_torch, "svt_noise_mix is not faster than the torch chain"


def table(args, say):
    from svt_speechbrain_amd.synth import synth_singing
    _lib.require_gpu()
    fx = torch.load(os.path.join(ROOT, "tests", "golden", "trained_like_head.pt"), weights_only=False)
    cfg = S.PRESETS[fx["model"]]
    wav, _, notes = synth_singing(args.clips, fx["seconds"], seed=fx["held_out_seed"] if args.held_out else fx["train_seed"])
    # frame2note puts frame k of the song at k / 49.8 s (the recipes' frame_size), and a 10 s clip is cfg.frames(L) = 499 frames: clip i starts at
    # 499 i / 49.8 = 10.02 i s on that axis, not at 10 i -- the ground truth is laid on the same axis
    start = cfg.frames(wav.shape[1]) / 49.8
    truth = [[float(a) + i * start, float(b) + i * start, int(m)] for i, clip in enumerate(notes) for a, b, m in clip]
    song = torch.from_numpy(wav).reshape(-1).to(DEV)
    white = torch.randn(song.shape, generator=torch.Generator().manual_seed(1234)).to(DEV)
    head = S.Linear(20, input_size=cfg.hidden_size)
    head.load_state_dict({"w.weight": fx["w.weight"], "w.bias": fx["w.bias"]})
    head = head.to(DEV)
    say(f"{args.clips} x {fx['seconds']:g} s of seeded synthetic singing ({'held-out clips' if args.held_out else 'the clips the head was fitted on'}) as one song ({len(truth)} ground-truth notes), white noise, "
        f"{fx['model']} (seeded) + the trained-like head; F1 against the ground truth: COn / COnP / COnPOff")
    say(f"{'mode':6s} {'SNR dB':>7s} {'notes':>6s} {'COn':>7s} {'COnP':>7s} {'COnPOff':>8s}")
    for mode in args.modes:
        enc = S.HuggingFaceWav2Vec2(fx["model"], None, config=cfg, precision=mode, normalize_wav=True, seed=fx["encoder_seed"]).to(DEV)
        tr = S.SongTranscriber(enc, head, dur_threshold=fx["seconds"])
        rows = [("clean", tr.transcribe(song))]
        rows += [(str(snr), notes_s) for snr, (notes_s, _) in S.NoiseSweep(tr).run(song, white).items()]
        for name, est in rows:
            m = scoring.score_song(est, truth) if est else {"Onset_F-measure": 0.0, "F-measure_no_offset": 0.0, "F-measure": 0.0}
            say(f"{mode:6s} {name:>7s} {len(est):6d} {m['Onset_F-measure']:7.3f} {m['F-measure_no_offset']:7.3f} {m['F-measure']:8.3f}")
        del enc, tr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=3840000)
    ap.add_argument("--snrs", type=float, nargs="+", default=[-10, -5, 0, 5, 10])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--table", action="store_true")
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--held-out", action="store_true", help="--table: the fixture's second seed (clips the head was not fitted on)")
    ap.add_argument("--modes", nargs="+", default=["fp32", "bf16", "fp16"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    (table if args.table else bandwidth)(args, say)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
