"""What tests/test_noise_limit.py, tests/test_noise_host.py (CPU) and tests/test_gpu_noise_mix.py (GPU) share: the fp64 formula of the noise
mixture, the per-element limit a correct kernel stays inside, a correct fp32 evaluation and its mutants, and the inputs of the fixture
tests/golden/noise_mix.pt rebuilt from the seeds it records (tests/golden/make_golden_noise_mix.py wrote it from the reference's own
synthesis_noise.py; no test reads the reference).

The formula (N20EMv2/audio_visual/synthesis_noise.py:123-137), for clean a, noise v, SNR s:

    f = 1 / (10 ** (s / 20) + 1)      A_a = mean|a|, A_v = mean|v|      out = (1 - f) a + (f A_a / (A_v + 1e-14)) v

The limit is a bound, not a fitted tolerance.  With M = |a| (1 - f) + |v| f A_a / (A_v + 1e-14) in fp64,

    limit = 3 * 2^-24 * M + 2^-149

counts the roundings of an evaluation whose two coefficients are computed in fp64 and rounded ONCE to fp32: each coefficient (2^-24 of its
term), each product (2^-24 of its term; an fma spares one of them), the sum (2^-24 |out| <= 2^-24 M) -- three half-ulp pairs of the
magnitude sum; 2^-149 is half the spacing of fp32's subnormals.  The reference itself is NOT inside it: it takes both amplitudes in fp32 and
rescales its noise tensor in place from one SNR to the next (1.6 - 2.2 of the limit); against the fixture's recorded reference samples the
kernel is therefore held to (1 + ref_vs_fp64) * limit by the triangle inequality, ref_vs_fp64 being the recorded distance of the reference
from the formula in units of the limit."""
import hashlib
import math
import os
import random

import torch

SNRS_DB = (-10, -5, 0, 5, 10)
STEP = 997   # every 997th sample of a mixture is recorded in the fixture
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "noise_mix.pt")


def factor(snr_db, exponent_div=20):
    return 1 / (10 ** (snr_db / exponent_div) + 1)


def mean_abs_exact(x):
    """mean|x| with an exactly rounded sum (math.fsum) and one division: the fp64 mean the device's amplitudes are held to."""
    return math.fsum(x.reshape(-1).double().abs().tolist()) / x.numel()


def amplitudes(a, v):
    return a.double().abs().mean().item(), v.double().abs().mean().item()


def coefficients(snrs_db, A_a, A_v):
    """(c1, c2) per SNR as Python doubles."""
    return [(1 - factor(s), factor(s) * A_a / (A_v + 1e-14)) for s in snrs_db]


def formula(a, v, snrs_db=SNRS_DB, amps=None):
    """(out, M): the fp64 formula and the magnitude sum, (S, n) each, of fp32 tracks a, v (1-D).  amps: (A_a, A_v) of the WHOLE tracks when
    a, v are samples of them."""
    A_a, A_v = amps if amps is not None else amplitudes(a, v)
    a64, v64 = a.double(), v.double()
    out = torch.stack([c1 * a64 + c2 * v64 for c1, c2 in coefficients(snrs_db, A_a, A_v)])
    M = torch.stack([abs(c1) * a64.abs() + abs(c2) * v64.abs() for c1, c2 in coefficients(snrs_db, A_a, A_v)])
    return out, M


def limit(M):
    return 3 * 2.0 ** -24 * M + 2.0 ** -149


def worst(got, ref, lim):
    """Largest |got - ref| / limit; a NaN or an infinity anywhere counts as infinite."""
    r = (got.double() - ref).abs() / lim
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))
    return r.max().item()


MUTANTS = ("rms", "clean_unscaled", "db10", "short_amplitude", "noise_amp_from_clean", "next_snr_row")


def direct_fp32(a, v, snrs_db=SNRS_DB, mutant=None, amps=None, index=None):
    """A correct evaluation -- amplitudes and coefficients in fp64, each coefficient rounded once, c1 * a + c2 * v in fp32 -- or a mutant:
    rms (root mean square in place of mean|x|), clean_unscaled (clean not scaled by 1 - f), db10 (10 ** (s / 10)), short_amplitude (the
    amplitudes over the first n - 4 samples), noise_amp_from_clean (A_v taken from the clean track), next_snr_row (row s written with the
    coefficients of SNR s + 1, the last row with the first's).  index: evaluate these samples only (the amplitudes are the whole tracks')."""
    assert mutant is None or mutant in MUTANTS
    if amps is not None:
        A_a, A_v = amps
    elif mutant == "rms":
        A_a, A_v = a.double().pow(2).mean().sqrt().item(), v.double().pow(2).mean().sqrt().item()
    elif mutant == "short_amplitude":
        A_a, A_v = amplitudes(a[:-4], v[:-4])
    else:
        A_a, A_v = amplitudes(a, v)
    if mutant == "noise_amp_from_clean":
        A_v = A_a
    snrs = list(snrs_db)
    if mutant == "next_snr_row":
        snrs = snrs[1:] + snrs[:1]
    if index is not None:
        a, v = a[index], v[index]
    rows = []
    for s in snrs:
        f = factor(s, 10 if mutant == "db10" else 20)
        c1 = torch.tensor(1.0 if mutant == "clean_unscaled" else 1 - f, dtype=torch.float64).float()
        c2 = torch.tensor(0.0 if A_v == 0 else f * A_a / (A_v + 1e-14), dtype=torch.float64).float()
        rows.append(c1 * a + c2 * v)
    return torch.stack(rows)


# ---- the fixture's inputs, rebuilt from its seeds ----

def sha256(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def seeded_track(n, seed, kind="song"):
    """song: a vibrato tone under a slow envelope plus a little noise, in [-1, 1]; noise: Gaussian at 0.05."""
    g = torch.Generator().manual_seed(seed)
    if kind == "noise":
        return 0.05 * torch.randn(n, generator=g)
    t = torch.arange(n, dtype=torch.float64) / 16000
    tone = torch.sin(2 * math.pi * (220.0 + seed % 7 * 20) * t + 3.0 * torch.sin(2 * math.pi * 5.5 * t))
    env = 0.25 + 0.2 * torch.sin(2 * math.pi * 0.31 * t)
    return ((env * tone).float() + 0.01 * torch.randn(n, generator=g)).clamp_(-1, 1)


def load_fixture():
    return torch.load(GOLDEN, weights_only=False)


_inputs = {}


def fixture_inputs(fx=None):
    """{"songs": {name: clean (n,)}, "accomp": {name: (n,)}, "white": {name: (n,)}, "natural_files": ({key: track}, {key: track}),
    "babble_files": {path: track}} -- CPU fp32 tensors from the recorded seeds, built once."""
    if _inputs:
        return _inputs
    fx = fx or load_fixture()
    m = fx["inputs"]
    _inputs["songs"] = {name: seeded_track(n, seed) for name, (n, seed) in m["songs"].items()}
    _inputs["accomp"] = {name: seeded_track(m["songs"][name][0], seed, "noise") for name, seed in m["accomp_seeds"].items()}
    state = torch.random.get_rng_state()
    torch.manual_seed(m["white_seed"])          # the reference draws torch.randn_like(audio) from the global generator, song after song
    _inputs["white"] = {name: torch.randn_like(_inputs["songs"][name][None])[0] for name in m["songs"]}
    torch.random.set_rng_state(state)
    _inputs["natural_files"] = tuple({key: seeded_track(n, seed, "noise") for key, (n, seed) in folder.items()} for folder in m["natural_files"])
    _inputs["babble_files"] = {path: seeded_track(n, seed, "noise") for path, (n, seed) in m["babble_files"].items()}
    return _inputs


def fixture_noise_tracks(fx=None):
    """{(song, type): noise track (n,)} of the fixture: accomp and white from their seeds; natural and babble assembled by
    svt_speechbrain_amd.noise from the recorded pool order, split and seed (tests/test_noise_host.py holds them to the reference's digests)."""
    if "tracks" in _inputs:
        return _inputs["tracks"]
    from svt_speechbrain_amd import noise as N
    fx = fx or load_fixture()
    inp = fixture_inputs(fx)
    tracks = {}
    for name in inp["songs"]:
        tracks[name, "accomp"] = inp["accomp"][name]
        tracks[name, "white"] = inp["white"][name]
    rng = random.Random(fx["inputs"]["random_seed"])
    # the reference's call order (synthesis_noise.py:482-486): babble (one choice per chunk and song), then natural (two shuffles, then choices)
    pools, _ = N.babble_pools(inp["babble_files"])
    for name, clean in inp["songs"].items():
        tracks[name, "babble"] = N.assemble_noise_track(pools[fx["babble"]["pool_split"]], clean.shape[0], rng)
    pools, _ = N.natural_pools(inp["natural_files"][0], inp["natural_files"][1], rng)
    for name, clean in inp["songs"].items():
        tracks[name, "natural"] = N.assemble_noise_track(pools[fx["inputs"]["song_splits"][name]], clean.shape[0], rng)
    _inputs["tracks"] = tracks
    return tracks
