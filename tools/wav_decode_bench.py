"""PCM -> planar fp32 of a whole song: svt_pcm_decode against the same conversion as torch ops on the same device and stream, and the
file-to-GPU time of audio_io.load against decoding on the host with numpy and uploading fp32.

    python tools/wav_decode_bench.py [--seconds 240] [--rate 44100] [--out profiles/pcm_decode_bandwidth.txt]

Default: a 240 s stereo 44.1 kHz track, once as a 16-bit and once as a 24-bit file.  Kernel paths are timed with HIP events around ITERS
back-to-back calls, alternating between svt_pcm_decode and the yardstick, after a warm-up; the figure per path is the median of the rounds.
The yardstick for 16 bits: view the bytes as int16, `.to(float32)`, scale, transpose, `.contiguous()`; for 24 bits: the three byte planes
widened to int32, shifted together and sign-extended from bit 23, `.to(float32)`, scale, transpose, `.contiguous()`.  Both paths' outputs
are compared bit for bit before anything is timed.  Bytes: the algorithm reads every source byte once and writes every fp32 once,
frames * channels * (bytes per sample + 4).  The source and the output of one call together (127 MB at 16 bits) fit the 256 MiB Infinity
Cache, as they do for a song in production; the share of the HBM peak is the usual yardstick of this repository's bandwidth tables, not a
claim about where the bytes came from.

File to GPU: the file is written to --dir (default: the system's temporary directory) and read back through the page cache by both
paths, so this is the CPU and PCIe side, not a disk.  Host clock around a call that ends in a device synchronise; medians.  No assertion
on speed."""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from svt_speechbrain_amd import _lib, audio_io  # noqa: E402

DEV = "cuda:0"
HBM_TBS = 8.0   # MI355X peak HBM bandwidth, TB/s


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


def host_rounds(fns, rounds):
    """Median host time per call, in ms; every function ends in a synchronise; the functions alternate."""
    times = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    return [statistics.median(t) for t in times], [(min(t), max(t)) for t in times]


def torch_s16(raw, channels):
    return (raw.view(torch.int16).to(torch.float32) * (2.0 ** -15)).view(-1, channels).t().contiguous()


def torch_s24(raw, channels):
    b = raw.view(-1, 3)
    x = b[:, 0].to(torch.int32) | (b[:, 1].to(torch.int32) << 8) | (b[:, 2].to(torch.int32) << 16)
    x = (x ^ 0x800000) - 0x800000   # the sign of the top byte
    return (x.to(torch.float32) * (2.0 ** -23)).view(-1, channels).t().contiguous()


def numpy_decode(path, info):
    """The host's way: read the data chunk, convert with numpy, upload fp32 (channels first)."""
    with open(path, "rb") as fh:
        fh.seek(info["offset"])
        raw = np.frombuffer(fh.read(info["frames"] * info["align"]), dtype=np.uint8)
    if info["fmt"] == audio_io.PCM_S16:
        x = raw.view("<i2").astype(np.float32) * np.float32(2.0 ** -15)
    else:
        t = raw.reshape(-1, 3)
        v = t[:, 0].astype(np.int32) | (t[:, 1].astype(np.int32) << 8) | (t[:, 2].astype(np.int32) << 16)
        v = (v ^ 0x800000) - 0x800000
        x = v.astype(np.float32) * np.float32(2.0 ** -23)
    return torch.from_numpy(np.ascontiguousarray(x.reshape(-1, info["channels"]).T)).to(DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--file-rounds", type=int, default=7)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    _lib.require_gpu()
    lib = _lib.load()
    frames, C = round(args.seconds * args.rate), args.channels
    stream = _lib.stream_ptr(DEV)
    say(f"{args.seconds:g} s, {C} channels at {args.rate} Hz: {frames} frames; svt_pcm_decode takes {audio_io.FRAMES_PER_WORKGROUP} frames per "
        f"workgroup, {audio_io.MAX_WORKGROUPS} workgroups at most")
    rng = np.random.RandomState(0)
    with tempfile.TemporaryDirectory(dir=args.dir) as tmp:
        for name, fmt, width, yardstick in (("S16", audio_io.PCM_S16, 2, torch_s16), ("S24", audio_io.PCM_S24, 3, torch_s24)):
            host = rng.randint(0, 256, frames * C * width, dtype=np.int64).astype(np.uint8)
            raw = torch.from_numpy(host).to(DEV)
            out = torch.empty((C, frames), dtype=torch.float32, device=DEV)

            def ours():
                rc = lib.svt_pcm_decode(_lib.ptr(raw), fmt, C, frames, _lib.ptr(out), frames, 0, 0, stream)
                assert rc == 0, _lib.last_error()

            def theirs():
                return yardstick(raw, C)

            ours()
            ref = theirs()
            torch.cuda.synchronize()
            assert torch.equal(out.view(torch.int32), ref.view(torch.int32)), "the two paths disagree"
            del ref
            for fn in (ours, theirs):
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            (t_svt, t_torch), spread = time_rounds([ours, theirs], args.iters, args.rounds)
            need = frames * C * (width + 4)
            tbs = need / t_svt * 1e-6
            say(f"--- {name}: {frames * C * width / 1e6:.1f} MB of PCM -> {frames * C * 4 / 1e6:.1f} MB of fp32, outputs equal bit for bit ---")
            say(f"svt_pcm_decode (1 launch):                {t_svt:9.1f} us per call   (rounds {spread[0][0]:.1f} .. {spread[0][1]:.1f})")
            say(f"torch ops (view, to, scale, transpose):   {t_torch:9.1f} us per call   (rounds {spread[1][0]:.1f} .. {spread[1][1]:.1f})")
            say(f"ratio torch / svt_pcm_decode:             {t_torch / t_svt:9.2f} x")
            say(f"bytes the algorithm needs:                frames * channels * ({width} + 4) = {need / 1e6:.1f} MB -> {tbs:.2f} TB/s = "
                f"{tbs / HBM_TBS * 100:.0f} % of the {HBM_TBS:g} TB/s peak")
            # file to GPU
            path = os.path.join(tmp, f"{name}.wav")
            head = (b"RIFF" + (36 + host.size).to_bytes(4, "little") + b"WAVEfmt " + (16).to_bytes(4, "little") + (1).to_bytes(2, "little") +
                    C.to_bytes(2, "little") + args.rate.to_bytes(4, "little") + (args.rate * C * width).to_bytes(4, "little") +
                    (C * width).to_bytes(2, "little") + (8 * width).to_bytes(2, "little") + b"data" + host.size.to_bytes(4, "little"))
            with open(path, "wb") as fh:
                fh.write(head)
                fh.write(host.tobytes())
            info = dict(offset=44, frames=frames, align=C * width, channels=C, fmt=fmt)
            a, _ = audio_io.load(path, device=DEV)
            b = numpy_decode(path, info)
            torch.cuda.synchronize()
            assert torch.equal(a.view(torch.int32), out.view(torch.int32)) and torch.equal(b.view(torch.int32), out.view(torch.int32))
            del a, b
            (t_load, t_np), fs = host_rounds([lambda: audio_io.load(path, device=DEV), lambda: numpy_decode(path, info)], args.file_rounds)
            utt = 5 * args.rate
            (t_utt, t_whole_utt), _ = host_rounds([lambda: audio_io.load(path, frame_offset=frames // 2, num_frames=utt, device=DEV),
                                                   lambda: numpy_decode(path, info)[:, frames // 2:frames // 2 + utt]], args.file_rounds)
            say(f"file -> GPU, whole song:   audio_io.load {t_load:8.2f} ms ({fs[0][0]:.2f} .. {fs[0][1]:.2f}), {host.size / 1e6:.1f} MB over PCIe;   "
                f"numpy decode + fp32 upload {t_np:8.2f} ms ({fs[1][0]:.2f} .. {fs[1][1]:.2f}), {frames * C * 4 / 1e6:.1f} MB over PCIe;   ratio {t_np / t_load:.2f} x")
            say(f"file -> GPU, one 5 s utterance:   audio_io.load(frame_offset, num_frames) {t_utt:8.2f} ms;   whole-song numpy decode, upload, slice "
                f"{t_whole_utt:8.2f} ms;   ratio {t_whole_utt / t_utt:.1f} x")
            del raw, out
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
