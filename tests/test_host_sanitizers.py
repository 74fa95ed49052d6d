"""CPU: the host-only routines of the C-ABI (svt_speechbrain_amd/csrc/host.cpp: error string, parameter intake, configuration
validation, the frames -> notes scan) built with AddressSanitizer + UndefinedBehaviorSanitizer (`make -C svt_speechbrain_amd/csrc san`)
and driven by tests/cabi/host_san_driver.cpp: the reference's frame2note fixture, random sequences against the Python frame loop,
exact-size output arrays, every refusal path with hostile arguments, and the weight re-layouts / folds of the finalize step against
numpy restatements of their formulas.  A sanitizer finding aborts the binary (non-zero exit).
SURVEY.md §5 (sanitizers): CPU build only -- the GPU pool has no sanitizer runs, and this code has no GPU part."""
import os
import subprocess

import numpy as np
import pytest

import svt_speechbrain_amd as S
from svt_speechbrain_amd.decode import FRAME_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svt_speechbrain_amd", "csrc")
BIN = os.path.join(CSRC, "build_san", "host_san_test")


@pytest.fixture(scope="module")
def san_bin():
    r = subprocess.run(["make", "-C", CSRC, "san"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return BIN


def run(binary, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([binary, *map(str, args)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout}\n{r.stderr}"
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    return r.stdout


def pack(p_on, p_off, octv, pc):
    fr = np.zeros(len(p_on), dtype=FRAME_DTYPE)
    fr["p_on"], fr["p_off"], fr["octave"], fr["pitch_class"] = p_on, p_off, octv, pc
    return fr


def notes_via_binary(binary, tmp_path, frames, cap=None):
    """frames: structured (B, T) -> per clip [[t_on, t_off, pitch or -1, lo, hi], ...] as the sanitized routine returned them"""
    B, T = frames.shape
    path = tmp_path / "frames.bin"
    np.ascontiguousarray(frames).tofile(path)
    args = ["notes", path, B, T, repr(float(np.float32(0.4))), repr(float(np.float32(0.5))), repr(1 / 49.8)]
    if cap is not None:
        args.append(cap)
    out = run(binary, *args)
    if out.startswith("error"):
        return out.strip()
    clips = [[] for _ in range(B)]
    for line in out.splitlines():
        b, t_on, t_off, pitch, lo, hi = line.split()
        clips[int(b)].append([float(t_on), float(t_off), int(pitch), int(lo), int(hi)])
    return clips


def resolve(clip_notes, fr_row):
    """tied pitch histograms come back as -1 with their frame range: the reference's own expression on the reference's own list"""
    out = []
    for t_on, t_off, pitch, lo, hi in clip_notes:
        if pitch < 0:
            bag = [int(o) * 12 + int(p) for o, p in zip(fr_row["octave"][lo:hi], fr_row["pitch_class"][lo:hi]) if o != 4 and p != 12]
            pitch = max(set(bag), key=bag.count) + 36
        out.append([t_on, t_off, pitch])
    return out


def fold_via_binary(binary, tmp_path, op, dims, inputs, out_shapes):
    """one `fold` command of the driver: float32 arrays in (raw files), the routine's results out, in the given shapes"""
    paths = []
    for i, a in enumerate(inputs):
        assert a.dtype == np.float32
        paths.append(tmp_path / f"{op}_in{i}.bin")
        np.ascontiguousarray(a).tofile(paths[-1])
    out = tmp_path / f"{op}_out.bin"
    run(binary, "fold", op, out, *dims, *paths)
    flat = np.fromfile(out, dtype=np.float32)
    sizes = [int(np.prod(s)) for s in out_shapes]
    assert flat.size == sum(sizes), (flat.size, sizes)
    return [part.reshape(s) for part, s in zip(np.split(flat, np.cumsum(sizes)[:-1]), out_shapes)]


def ulps_apart(got, want64):
    """distance of float32 `got` from the float64 result rounded to float32, in float32 steps"""
    want = np.asarray(want64, dtype=np.float64).astype(np.float32)
    assert got.shape == want.shape and np.isfinite(got).all()
    key = lambda a: np.where(a.view(np.int32) < 0, np.int64(-2**31) - a.view(np.int32), a.view(np.int32)).astype(np.int64)
    return int(np.abs(key(got) - key(want)).max())


def distinct(shape):
    """a float32 tensor whose every element is a different, exactly representable value"""
    return (np.arange(1, int(np.prod(shape)) + 1, dtype=np.float32) * np.float32(0.25)).reshape(shape)


# positional-conv geometry of the fold cases: D = 16 channels in G = 2 groups of cg = 8, kernel kp = 9
POS_D, POS_G, POS_KP = 16, 2, 9
POS_CG = POS_D // POS_G


def test_tap_major_relayout_under_sanitizers(san_bin, tmp_path):
    Co, Ci, k = 3, 5, 3
    w = distinct((Co, Ci, k))
    got, = fold_via_binary(san_bin, tmp_path, "tap_major", [Co, Ci, k], [w], [(Co, k, Ci)])
    want = np.empty((Co, k, Ci), np.float32)
    for o in range(Co):
        for j in range(k):
            for ci in range(Ci):
                want[o, j, ci] = w[o, ci, j]          # column j*Ci + ci of row o: tap j, input channel ci
    assert np.array_equal(got, want)


def test_tap_minor_slab_order_under_sanitizers(san_bin, tmp_path):
    Co, Ci, k = 2, 128, 3
    w = distinct((Co, Ci, k))
    got, = fold_via_binary(san_bin, tmp_path, "tap_minor", [Co, Ci, k], [w], [(Co, k * Ci // 64, 64)])
    want = np.empty_like(got)
    for g in range(k * Ci // 64):                      # slab g = tap g % 3 of channel block g // 3, 64 channels per block
        want[:, g, :] = w[:, (g // 3) * 64:(g // 3) * 64 + 64, g % 3]
    assert np.array_equal(got, want)


def test_multi_frame_positional_conv_matrix_under_sanitizers(san_bin, tmp_path):
    G, cg, kp = POS_G, POS_CG, POS_KP
    Pf = 256 // cg
    K = (kp + Pf - 1) * cg
    assert (Pf, K) == (32, 320)
    w, bias = distinct((POS_D, cg, kp)), distinct((POS_D,)) + np.float32(1000)
    wP, bP = fold_via_binary(san_bin, tmp_path, "multiframe", [G, cg, kp, Pf], [w, bias], [(G, Pf, cg, kp + Pf - 1, cg), (G, Pf, cg)])
    want = np.zeros_like(wP)
    for j in range(Pf):                                # output frame j of a row: the filter shifted by j taps, zero elsewhere
        want[:, j, :, j:j + kp, :] = w.reshape(G, cg, cg, kp).transpose(0, 1, 3, 2)
    assert np.array_equal(wP, want)
    assert np.array_equal(bP, np.broadcast_to(bias.reshape(G, 1, cg), (G, Pf, cg)))


def test_weight_norm_fold_under_sanitizers(san_bin, tmp_path):
    rng = np.random.default_rng(0)
    g = rng.standard_normal(POS_KP).astype(np.float32)
    v = rng.standard_normal((POS_D, POS_CG, POS_KP)).astype(np.float32)
    got, = fold_via_binary(san_bin, tmp_path, "weight_norm", [v.size, POS_KP], [g, v], [v.shape])
    v64 = v.astype(np.float64)
    want = g.astype(np.float64) * v64 / np.sqrt((v64 * v64).sum(axis=(0, 1)))     # W[:,:,j] = g[j] v[:,:,j] / ||v[:,:,j]||_F
    assert ulps_apart(got, want) <= 1


def test_batch_norm_fold_under_sanitizers(san_bin, tmp_path):
    rng = np.random.default_rng(1)
    weight, bias, mean = (rng.standard_normal(POS_D).astype(np.float32) for _ in range(3))
    var = rng.uniform(0.1, 4.0, POS_D).astype(np.float32)
    scale, shift = fold_via_binary(san_bin, tmp_path, "batch_norm", [POS_D], [weight, bias, mean, var], [(POS_D,), (POS_D,)])
    k = weight.astype(np.float64) / np.sqrt(var.astype(np.float64) + 1e-5)         # y = (x - mean) / sqrt(var + eps) * weight + bias
    assert ulps_apart(scale, k) <= 1
    assert ulps_apart(shift, bias.astype(np.float64) - mean.astype(np.float64) * k) <= 1


def test_wavlm_gate_row_sum_fold_under_sanitizers(san_bin, tmp_path):
    """The fold adds its rows in float32, so the values are distinct ones on a 1/4 grid: every sum is exact in float32 and float64
    alike, a row in the wrong sum shows, and the result must equal the float64 row sums (on values whose sums cancel, float32
    addition keeps the rounding of the larger partial sums and no bound in steps of the result holds)."""
    dh = 8                                              # (H = 2 heads share the gate projection: the fold does not see H)
    w, b = distinct((8, dh)), distinct((8,)) + np.float32(100)
    wab, bab = fold_via_binary(san_bin, tmp_path, "gate", [dh], [w, b], [(2, dh), (2,)])
    assert ulps_apart(wab, w.astype(np.float64).reshape(2, 4, dh).sum(axis=1)) == 0    # rows 0-3 -> a, rows 4-7 -> b
    assert ulps_apart(bab, b.astype(np.float64).reshape(2, 4).sum(axis=1)) == 0


def test_hostile_arguments_under_sanitizers(san_bin):
    assert run(san_bin, "hostile").strip() == "hostile ok"


def test_attention_planner_table_under_sanitizers(san_bin):
    """plan_attention (the one place that chooses an attention path and the buffers it needs) against the driver's hand-written table:
    every path, every edge of a condition, the key pad at T = 1, 63, 64, 65, and what the encoder's and FusionRCA's workspaces hold."""
    assert run(san_bin, "attention").strip() == "attention ok"


def test_reference_frame2note_fixture_under_sanitizers(san_bin, tmp_path, golden):
    for k, c in golden("frame2note").items():
        fr = pack(c["p_on"].numpy(), c["p_off"].numpy(), c["oct"].numpy(), c["pc"].numpy())
        got = notes_via_binary(san_bin, tmp_path, fr[None])
        assert resolve(got[0], fr) == c["notes"], k


def test_random_sequences_under_sanitizers_match_the_frame_loop(san_bin, tmp_path):
    rng = np.random.default_rng(11)
    grid = np.array([0.0, 0.1, 0.4, 0.5, 0.7, 0.7, 0.9, 1.0], dtype=np.float32)
    for trial in range(12):
        B, T = int(rng.integers(1, 5)), int(rng.integers(2, 300))
        fr = np.zeros((B, T), dtype=FRAME_DTYPE)
        fr["p_on"] = grid[rng.integers(0, len(grid), (B, T))] * (rng.random((B, T)) < 0.3)
        fr["p_off"] = grid[rng.integers(0, len(grid), (B, T))] * (rng.random((B, T)) < 0.2)
        fr["octave"] = np.repeat(rng.integers(0, 5, (B, T // 7 + 1)), 7, axis=1)[:, :T]
        fr["pitch_class"] = np.repeat(rng.integers(0, 13, (B, T // 3 + 1)), 3, axis=1)[:, :T]
        want = [S.frame2note(S.frames_to_info(fr[b]), 0.4, 0.5, 1 / 49.8) for b in range(B)]
        most = max(1, max(len(w) for w in want))
        got = notes_via_binary(san_bin, tmp_path, fr, cap=most)       # output arrays of EXACTLY the size needed
        assert [resolve(got[b], fr[b]) for b in range(B)] == want, trial
        if most > 1:                                                  # one slot short: refused, nothing written past the arrays
            assert "more notes than capacity_per_clip" in notes_via_binary(san_bin, tmp_path, fr, cap=most - 1)
