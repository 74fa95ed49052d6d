"""bench.py's own N > 1 control flow on a one-GPU box: two ranks launched exactly like the driver launches them
(`python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 ... bench.py --gpus 2`), both on device 0
(SVT_SHARE_GPU=1) with the collectives on gloo, staged through the host (SVT_DIST_BACKEND=gloo; RCCL refuses two ranks on one
device).  Everything else is the real path: per-rank clip seeding, shard bounds, the lanes / streams, one gather per step from the
step's stream, max over ranks, per-rank rates, the JSON line -- and `--verify`: every rank recomputes all shards locally and
compares them with the rows the last step gathered.  Second case: compact-frames gather + the optional global-batch norms, whose
two 16-byte all-reduces then really cross a process boundary, verified against ONE forward of the whole global batch."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def launch(port, *extra, nproc=2, batch=3, share_gpu=True):
    env = dict(os.environ, SVT_DIST_BACKEND="gloo")
    env.pop("SVT_SHARE_GPU", None)
    if share_gpu:
        env["SVT_SHARE_GPU"] = "1"
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", str(nproc), "--steps", "3", "--warmup", "1", "--batch", str(batch),
           "--seconds", "2", "--no-cpu-baseline", "--no-extra-legs", "--verify", *extra]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    if r.returncode != 0 and ("address already in use" in r.stderr.lower() or "rendezvous" in r.stderr.lower()
                              or "connection" in r.stderr.lower()):
        # the rendezvous port of a fresh box can still be held for a moment (seen once in four sessions): one retry on another port
        cmd[cmd.index(str(port))] = str(port + 173)
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.stdout[-3000:], r.stderr[-3000:])
    return json.loads(lines[0])


def test_two_ranks_logits_gather():
    j = launch(29541)
    assert j["n_gpus"] == 2 and j["rccl_ranks"] == 2 and j["scaling"] == "weak" and j["verified"] is True
    assert len(j["per_rank_clips_per_s"]) == 2 and j["config"]["global_batch"] == 6 and j["config"]["per_gpu_batch"] == 3
    c = j["collective"]
    assert c["op"] == "all_gather_into_tensor" and c["payload"] == "logits" and c["backend"] == "gloo"
    assert c["bytes_per_rank_per_step"] == 3 * 99 * 20 * 4          # 3 clips x 99 frames (2 s) x 20 logits, fp32
    assert j["value"] > 0 and j["steps"] == 3 and j["warmup"] == 1


def test_two_ranks_frames_gather_with_global_norms():
    j = launch(29542, "--gather", "frames", "--global-norm", "--precision", "fp32")
    assert j["verified"] is True and j["rccl_ranks"] == 2
    c = j["collective"]
    assert c["payload"] == "frames" and c["bytes_per_rank_per_step"] == 3 * 99 * 16 and c["norm_all_reduce"]


def test_eight_ranks_dry_run_of_the_drivers_scaling_command():
    """`bench.py --gpus 8` exactly as the driver launches it for SCALE_rNN.json, one rank per device (collectives on gloo): rank count,
    weak scaling, per-rank rates, gather size and the verification of every gathered row.  What it cannot show is RCCL itself: the
    `nccl` branch of distributed._gather_into with more than one rank has never executed.  Eight ranks on ONE device are
    more processes than a shared GPU may hold at once, so on a box with fewer than eight GPUs the test skips before it starts anything."""
    import torch
    n_dev = torch.cuda.device_count()
    if n_dev < 8:
        pytest.skip(f"needs 8 GPUs (one rank per device), found {n_dev}")
    j = launch(29551, nproc=8, batch=2, share_gpu=False)
    assert j["n_gpus"] == 8 and j["rccl_ranks"] == 8 and j["scaling"] == "weak" and j["verified"] is True
    assert len(j["per_rank_clips_per_s"]) == 8 and j["config"]["global_batch"] == 16 and j["config"]["per_gpu_batch"] == 2
    assert j["collective"]["bytes_per_rank_per_step"] == 2 * 99 * 20 * 4 and j["collective"]["backend"] == "gloo"


def test_plain_launch_starts_its_own_ranks():
    """`python bench.py --gpus 2` WITHOUT a launcher (no WORLD_SIZE): bench.py starts two fresh ranks itself, before any GPU call,
    and relays rank 0's JSON line -- n_gpus == rccl_ranks == 2 (the driver's 8-GPU run must not silently time one rank)."""
    env = dict(os.environ, SVT_SHARE_GPU="1", SVT_DIST_BACKEND="gloo")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "2", "--seconds", "2",
           "--no-cpu-baseline", "--no-extra-legs", "--verify"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.stdout[-3000:], r.stderr[-3000:])
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["rccl_ranks"] == 2 and j["verified"] is True and j["config"]["global_batch"] == 4
    assert "launching 2 ranks" in r.stderr


def test_two_ranks_with_the_step_replayed_from_a_hip_graph():
    """`--graph` at N > 1 (opt-in; the default there is eager launches): every rank captures its lane's forward, replays it, and the
    collective stays outside the graph on the lane's stream; the gathered rows still equal a local recomputation of every shard."""
    j = launch(29561, "--graph")
    assert j["n_gpus"] == 2 and j["rccl_ranks"] == 2 and j["verified"] is True
    assert j["config"]["launch"].startswith("hipGraph replay"), j["config"]["launch"]


def test_one_rank_default_replays_a_checked_graph_and_no_graph_launches_eagerly():
    """N = 1: the default line replays a captured step that was compared bit for bit with the eager step; `--no-graph` is the mode of
    rounds 1-5.  Both report what they did in config.launch."""
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "SVT_SHARE_GPU", "SVT_DIST_BACKEND"):
        env.pop(k, None)
    seen = {}
    for flag in ((), ("--no-graph",)):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--batch", "2", "--seconds", "2", "--no-cpu-baseline",
               "--no-extra-legs", *flag]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert r.returncode == 0 and len(lines) == 1, (r.stdout[-2000:], r.stderr[-2000:])
        seen[flag] = json.loads(lines[0])
    assert seen[()]["config"]["launch"].startswith("hipGraph replay") and seen[("--no-graph",)]["config"]["launch"] == "eager"
    assert seen[()]["verified"] is None and seen[()]["n_gpus"] == 1


def test_one_rank_dump_outputs_of_the_last_timed_step(tmp_path):
    """`--dump-outputs DIR`: the last timed step's logits and decoded frames as .npy files; a graph-replayed run on two lanes and an
    eager run on one lane with another step count hand back the same bits (same seeded inputs), and `steps` / `ms_per_step` are the
    timed region's."""
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "SVT_SHARE_GPU", "SVT_DIST_BACKEND"):
        env.pop(k, None)
    import numpy as np
    dumps = []
    for steps, flags in (("3", ()), ("2", ("--no-graph", "--streams", "1"))):
        d = tmp_path / f"out{len(dumps)}"
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", steps, "--warmup", "1", "--batch", "2", "--seconds", "2",
               "--no-cpu-baseline", "--no-extra-legs", "--dump-outputs", str(d), *flags]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert r.returncode == 0 and len(lines) == 1, (r.stdout[-2000:], r.stderr[-2000:])
        j = json.loads(lines[0])
        assert j["steps"] == int(steps) and j["ms_per_step"] > 0
        files = sorted(os.listdir(d))
        assert files == ["frame_octave.npy", "frame_p_off.npy", "frame_p_on.npy", "frame_pitch_class.npy", "logits.npy"], files
        dumps.append({f[:-4]: np.load(d / f) for f in files})
    a, b = dumps
    assert a["logits"].shape == (2, 99, 20) and a["logits"].dtype == np.float32 and np.isfinite(a["logits"]).all()
    assert a["frame_octave"].shape == (2, 99) and a["frame_octave"].dtype == np.float64
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    # the frames are the decode of these logits: the octave field is the argmax over its five classes (20 = 2 + 5 + 13)
    assert np.array_equal(a["frame_octave"], a["logits"][..., 2:7].argmax(-1))


def test_one_rank_plain_run_is_lean_and_full_runs_the_legs():
    """A plain run prints the timed figures and none of the legs after the timed region; `--full` runs them (the CPU baseline is left
    out here, `--no-cpu-baseline`: it is the oracle on the host, minutes at this size)."""
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "SVT_SHARE_GPU", "SVT_DIST_BACKEND"):
        env.pop(k, None)
    seen = {}
    for flags in ((), ("--full", "--no-cpu-baseline")):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--batch", "2", "--seconds", "2", *flags]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert r.returncode == 0 and len(lines) == 1, (r.stdout[-2000:], r.stderr[-2000:])
        seen[flags] = json.loads(lines[0])
    plain, full = seen[()], seen[("--full", "--no-cpu-baseline")]
    for j in (plain, full):
        assert j["value"] > 0 and j["ms_per_step"] > 0 and j["steps"] == 2 and j["warmup"] == 1 and j["dtype"] == "bf16"
        assert j["unit"] == "clips/s" and j["higher_is_better"] is True and "cpu_baseline" not in j
    legs = ("sustained", "notes_out", "parity_grade", "trained_like")
    assert not any(k in plain for k in legs) and plain["parity"] is None and "achieved" not in plain["roofline"]
    assert all(k in full for k in legs) and full["parity"] is not None and full["roofline"]["launches"] > 0
