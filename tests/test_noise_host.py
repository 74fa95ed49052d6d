"""Host side of the noise synthesis (svt_speechbrain_amd/noise.py), no GPU: the babble / natural track assembly and the natural split
reproduce, bit for bit, what the reference's synthesis_noise.py produced for the fixture tests/golden/noise_mix.pt (copies and zeros: equality
is exact); the duration filters; the C ABI's new symbols; the errors of the Python entry points."""
import os
import random
import re

import pytest
import torch

import noise_limit as NL
import svt_speechbrain_amd as S
from svt_speechbrain_amd import _lib, noise as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return NL.load_fixture()


def test_assembly_and_split_reproduce_the_reference(fx):
    """Seeded like the reference and called in its order (babble: one choice per chunk and song; natural: two shuffles, then the
    choices), the picks, the splits and every sample of the four noise.wav tracks are the reference's."""
    inp = NL.fixture_inputs(fx)
    rng = random.Random(fx["inputs"]["random_seed"])
    pools, splits = N.babble_pools(inp["babble_files"])
    assert list(splits) == fx["babble"]["order"] and dict(splits) == fx["babble"]["splits"]
    assert fx["babble"]["pool_split"] == "train"   # the reference's leftover variable: the last file listed is us-gov/train-0002.wav
    tracks = {}
    for name, clean in inp["songs"].items():
        track, picks = N.assemble_noise_track(pools[fx["babble"]["pool_split"]], clean.shape[0], rng, return_picks=True)
        assert picks == fx["babble"]["tracks"][name]["picks"]
        assert track.dtype == torch.float32 and track.shape == clean.shape
        assert NL.sha256(track) == fx["babble"]["tracks"][name]["sha256"]
        tracks[name, "babble"] = track
    pools, splits = N.natural_pools(inp["natural_files"][0], inp["natural_files"][1], rng)
    assert list(splits) == fx["natural"]["order"] and dict(splits) == fx["natural"]["splits"]
    assert set(splits.values()) == {"train", "valid", "test"}
    for name, clean in inp["songs"].items():
        track, picks = N.assemble_noise_track(pools[fx["inputs"]["song_splits"][name]], clean.shape[0], rng, return_picks=True)
        assert picks == fx["natural"]["tracks"][name]["picks"]
        assert NL.sha256(track) == fx["natural"]["tracks"][name]["sha256"]
        tracks[name, "natural"] = track
    shared = NL.fixture_noise_tracks(fx)   # what the limit tests and the GPU test mix
    for key, t in tracks.items():
        assert torch.equal(shared[key], t)
    for name in inp["songs"]:
        assert NL.sha256(inp["white"][name]) == fx["white_sha256"][name]   # the white track the reference drew


def test_fixture_meets_both_last_chunk_branches(fx):
    inp = NL.fixture_inputs(fx)
    pools, _ = N.natural_pools(inp["natural_files"][0], inp["natural_files"][1], random.Random(0))   # pool CONTENT does not depend on the seed ...
    files = {k: t for pool in pools.values() for k, t in pool.items()}
    train = [files[k] for k, s in fx["natural"]["splits"].items() if s == "train"]                     # ... its split does: take the recorded one
    tracks = NL.fixture_noise_tracks(fx)
    rem = {"trunc": 40000, "pad": 150000}
    last = {name: train[fx["natural"]["tracks"][name]["picks"][-1]] for name in rem}
    assert last["trunc"].shape[0] > rem["trunc"]                               # cut to its first `rem` samples
    assert torch.equal(tracks["trunc", "natural"][-rem["trunc"]:], last["trunc"][:rem["trunc"]])
    n = last["pad"].shape[0]
    assert n < rem["pad"]                                                      # centred in the remainder
    tail, pad1 = tracks["pad", "natural"][-rem["pad"]:], (rem["pad"] - n) // 2
    assert torch.equal(tail[pad1:pad1 + n], last["pad"]) and tail[:pad1].abs().max() == 0 and tail[pad1 + n:].abs().max() == 0


def test_assemble_noise_track_small_cases():
    """sample_rate 2, chunks of 10 samples."""
    short, long_ = torch.arange(1.0, 4.0), torch.arange(1.0, 11.0)
    kw = dict(sample_rate=2, duration_thrd=5)
    # one full chunk (file of 3 centred: pad1 = 3, pad2 = 4), then a remainder of 5 (pad1 = 1, pad2 = 1)
    t = N.assemble_noise_track([short], 15, random.Random(0), **kw)
    assert t.tolist() == [0, 0, 0, 1, 2, 3, 0, 0, 0, 0, 0, 1, 2, 3, 0]
    # remainder of 4 < 10: the file's first 4 samples
    t = N.assemble_noise_track([long_], 14, random.Random(0), **kw)
    assert t.tolist() == list(range(1, 11)) + [1, 2, 3, 4]
    # a file exactly as long as the remainder takes the pad branch with no padding; a song of whole chunks has a full-chunk remainder
    assert N.assemble_noise_track([short], 3, random.Random(0), **kw).tolist() == [1, 2, 3]
    assert N.assemble_noise_track([long_], 20, random.Random(0), **kw).tolist() == 2 * list(range(1, 11))
    # (1, len) files as torchaudio loads them, a mapping as the pool, one rng.choice per chunk over list(pool)
    rng, twin = random.Random(5), random.Random(5)
    pool = {"a": short[None], "b": long_[None], "c": torch.ones(1, 2)}
    _, picks = N.assemble_noise_track(pool, 47, rng, return_picks=True, **kw)
    assert picks == [twin.choice(range(3)) for _ in range(5)] and rng.random() == twin.random()
    with pytest.raises(ValueError):
        N.assemble_noise_track([torch.ones(11)], 25, random.Random(0), **kw)   # longer than a full chunk: the reference's assert
    with pytest.raises(ValueError):
        N.assemble_noise_track([], 25, random.Random(0), **kw)


def test_split_natural_files_thresholds():
    """8 keys: i <= 6 train, i == 7 valid; 9 keys: i <= 6 train (6.75), i == 7 valid (7.875), i == 8 test; two shuffles, free-sound first."""
    a, b = [f"a{i}" for i in range(8)], [f"b{i}" for i in range(9)]
    rng, twin = random.Random(3), random.Random(3)
    got = N.split_natural_files(a, b, rng)
    sa, sb = list(a), list(b)
    twin.shuffle(sa)
    twin.shuffle(sb)
    assert list(got) == a + b and rng.random() == twin.random()
    assert [got[k] for k in sa] == ["train"] * 7 + ["valid"]
    assert [got[k] for k in sb] == ["train"] * 7 + ["valid", "test"]


def test_duration_filters(fx):
    assert N.natural_keep(16000) and N.natural_keep(160000) and not N.natural_keep(15999) and not N.natural_keep(160001)
    assert N.babble_keep(160000) and not N.babble_keep(159999) and not N.babble_keep(160001)
    assert N.babble_split("musan/speech/us-gov/train-0002-x.wav") == "train" and N.babble_split("valid-1.wav") == "valid"
    inp = NL.fixture_inputs(fx)
    pools, splits = N.natural_pools(inp["natural_files"][0], inp["natural_files"][1], random.Random(0))
    lengths = {k: n for folder in fx["inputs"]["natural_files"] for k, (n, _) in folder.items()}
    assert min(lengths.values()) < 16000 and max(lengths.values()) > 160000 and 16000 in lengths.values() and 160000 in lengths.values()
    assert sorted(splits) == sorted(k for k, n in lengths.items() if 16000 <= n <= 160000) and len(splits) < len(lengths)
    bpools, bsplits = N.babble_pools(inp["babble_files"])
    kept = [p.split("/")[-1] for p, (n, _) in fx["inputs"]["babble_files"].items() if n == 160000]
    assert list(bsplits) == kept and len(kept) == len(inp["babble_files"]) - 2
    assert {k: len(v) for k, v in bpools.items()} == {"train": 3, "valid": 2, "test": 1}


def test_new_symbols_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "svt_mi355.h")).read()
    for name in ("svt_noise_mix", "svt_noise_mix_workspace_bytes"):
        assert re.search(r"\b" + name + r"\s*\(", hdr) and name in _lib.SYMBOLS
    assert int(re.search(r"#define SVT_NOISE_AMP_WORKGROUPS (\d+)", hdr).group(1)) == N.AMP_WORKGROUPS
    assert int(re.search(r"#define SVT_NOISE_MIX_MAX_WORKGROUPS (\d+)", hdr).group(1)) == N.MIX_MAX_WORKGROUPS
    lib = _lib.load()
    assert lib.svt_noise_mix_workspace_bytes(1000, 5) == 2 * N.AMP_WORKGROUPS * 8
    assert lib.svt_noise_mix_workspace_bytes(0, 5) == -1 and lib.svt_noise_mix_workspace_bytes(1000, 9) == -1
    assert lib.svt_noise_mix_workspace_bytes(1000, 0) == -1
    for name in ("SNRS_DB", "compute_amplitude", "mix_at_snrs", "assemble_noise_track", "split_natural_files", "noisy_wav_path", "NoiseSweep"):
        assert name in S.__all__ and hasattr(S, name)
    assert S.SNRS_DB == (-10, -5, 0, 5, 10)


def test_errors_and_paths():
    a = torch.zeros(100)
    with pytest.raises(_lib.SvtError):
        S.mix_at_snrs(a, a)                       # CPU tensors: no CPU fallback
    with pytest.raises(_lib.SvtError):
        S.compute_amplitude(a)
    with pytest.raises(ValueError):
        S.mix_at_snrs(a, torch.zeros(101))        # the reference asserts equal lengths
    with pytest.raises(ValueError):
        S.mix_at_snrs(a[None], torch.zeros(1, 99))
    for kw in (dict(amp_type="peak"), dict(scale="dB"), dict(lengths=torch.ones(1))):
        with pytest.raises(NotImplementedError):
            S.compute_amplitude(a, **kw)
    assert S.noisy_wav_path("data/s1", "natural", -10) == os.path.join("data/s1", "noise_data", "natural", "SNR_-10dB.wav")
    assert os.path.dirname(S.noisy_wav_path("data/s1", "babble", 5)) == os.path.dirname(S.feature_path("data/s1", True, "babble", 5))
    with pytest.raises(ValueError):
        S.NoiseSweep(None).run(a, a, song_folder="x")   # a folder without a noise type
