"""Generate tests/golden/noise_mix.pt by running the REFERENCE's own N20EMv2/audio_visual/synthesis_noise.py, unmodified.

Runs only where the reference checkout is present (REF below); the fixture it writes holds data only -- seeds, file lengths, digests, strided
samples -- and the reference itself is never committed.

    python tests/golden/make_golden_noise_mix.py

synthesis_noise.py is imported by file path with permissive stubs for hyperpyyaml / ruamel (as make_golden.py does) and a torchaudio stub
whose load / save go to an in-memory dict; empty files in a temporary folder satisfy its glob calls, glob.glob is wrapped in sorted() (the
listing order decides the picks), random.choice and torch.randn_like are wrapped to RECORD what they return.  Its four synthesis_* functions
then run in the order of its __main__ (random.seed(1234); accomp, white, babble, natural) on two songs:

    trunc   2 x 160 000 + 40 000 samples: a remainder of 2.5 s, shorter than most noise files (the last chunk is cut)
    pad     160 000 + 150 000 samples: a remainder of 9.375 s (the last chunk is centred in zeros, for natural)

Inputs are recorded by seed (tests/noise_limit.py rebuilds them).  Per (song, type, SNR): the sha256 of the saved mixture, every 997th
sample of it, and ref_vs_fp64 = the largest |reference - fp64 formula| / limit over those samples (tests/noise_limit.py: formula, limit).
Per (song, babble | natural): the sha256 of the saved noise.wav track and the pool indices the reference picked; per type the pool order
and splits the reference saw."""
import glob
import importlib.util
import json
import os
import random
import sys
import tempfile
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import noise_limit as NL  # noqa: E402

REF = "/root/reference"
SEED = 1234   # synthesis_noise.py:478
SR = 16000
SONGS = {"trunc": (2 * 160000 + 40000, 7101), "pad": (160000 + 150000, 7102)}
SONG_SPLITS = {"trunc": "train", "pad": "train"}
ACCOMP_SEEDS = {"trunc": 7201, "pad": 7202}
WHITE_SEED = 7301
# seconds of the noise files: both ends of the natural filter (1 <= d <= 10) and of babble's (d == 10) are met from both sides
NATURAL_SECONDS = ([0.5, 1.0, 1.5, 2.25, 3.0, 4.7, 6.0, 8.2, 9.375, 10.0, 10.0001, 12.0],
                   [0.99, 1.2, 2.0, 2.5, 3.3, 5.0, 7.7, 9.0, 9.99, 10.5, 11.0])
BABBLE_FILES = [("us-gov", "test-0000.wav", 10.0), ("us-gov", "train-0000.wav", 10.0), ("us-gov", "train-0001.wav", 10.0),
                ("us-gov", "train-0002.wav", 9.0), ("librivox", "valid-0000.wav", 10.0), ("librivox", "valid-0001.wav", 10.0),
                ("librivox", "valid-0002.wav", 10.5), ("librivox", "train-0003.wav", 10.0)]


class Stub(types.ModuleType):
    __path__ = []

    def __getattr__(self, n):
        if n.startswith("__"):
            raise AttributeError(n)
        return Stub(self.__name__ + "." + n)

    def __call__(self, *a, **k):
        return None


def main():
    store = {}   # path -> (1, n) tensor: the "files" torchaudio.load reads and torchaudio.save writes

    ta = types.ModuleType("torchaudio")
    ta.load = lambda path: (store[path].clone(), SR)
    ta.save = lambda path, wav, sr: store.__setitem__(path, wav.clone())   # a copy: the reference goes on rescaling the tensor in place
    ta.transforms = Stub("torchaudio.transforms")
    sys.modules["torchaudio"] = ta
    for m in ["hyperpyyaml", "ruamel", "ruamel.yaml"]:
        sys.modules.setdefault(m, Stub(m))
    sys.path.append(REF)
    spec = importlib.util.spec_from_file_location("ref_synthesis_noise", REF + "/N20EMv2/audio_visual/synthesis_noise.py")
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    inputs = {"songs": SONGS, "song_splits": SONG_SPLITS, "accomp_seeds": ACCOMP_SEEDS, "white_seed": WHITE_SEED, "random_seed": SEED,
              "natural_files": ({}, {}), "babble_files": {}}
    with tempfile.TemporaryDirectory() as tmp:
        folder, musan, babble = (os.path.join(tmp, d) for d in ("n20emv2", "musan", "babble"))
        os.makedirs(os.path.join(folder, "data"))
        with open(os.path.join(folder, "annotations.json"), "w") as f:
            json.dump({name: {"split": SONG_SPLITS[name]} for name in SONGS}, f)
        for name, (n, seed) in SONGS.items():
            os.makedirs(os.path.join(folder, "data", name))
            store[os.path.join(folder, "data", name, "vocals.wav")] = NL.seeded_track(n, seed)[None]
            store[os.path.join(folder, "data", name, "accomp.wav")] = NL.seeded_track(n, ACCOMP_SEEDS[name], "noise")[None]
        seed = 7400
        for k, (sub, seconds) in enumerate(zip(("free-sound", "sound-bible"), NATURAL_SECONDS)):
            os.makedirs(os.path.join(musan, sub))
            for i, sec in enumerate(seconds):
                path = os.path.join(musan, sub, f"noise-{sub}-{i:04d}.wav")
                open(path, "w").close()
                seed += 1
                inputs["natural_files"][k][f"{sub}/noise-{sub}-{i:04d}.wav"] = (round(sec * SR), seed)
                store[path] = NL.seeded_track(round(sec * SR), seed, "noise")[None]
        made = {}
        for sub, fname, sec in BABBLE_FILES:
            os.makedirs(os.path.join(babble, sub), exist_ok=True)
            path = os.path.join(babble, sub, fname)
            open(path, "w").close()
            seed += 1
            made[path] = (round(sec * SR), seed)
            store[path] = NL.seeded_track(round(sec * SR), seed, "noise")[None]
        # sorted listing; the fixture records the files in the order the reference saw them, relative to the noise folder
        real_glob = glob.glob
        glob.glob = lambda *a, **k: sorted(real_glob(*a, **k))
        for path in glob.glob(babble + "/*/*wav"):
            inputs["babble_files"][os.path.relpath(path, babble)] = made[path]

        picks, whites = [], []
        real_choice, real_randn_like = random.choice, torch.randn_like

        def choice(seq):
            got = real_choice(seq)
            picks.append(next(i for i, t in enumerate(seq) if t is got))
            return got

        def randn_like(x, *a, **k):
            got = real_randn_like(x, *a, **k)
            whites.append(got.clone())
            return got

        random.choice, torch.randn_like = choice, randn_like
        try:
            random.seed(SEED)
            torch.manual_seed(WHITE_SEED)
            ref.synthesis_accomp(folder=folder)
            ref.synthesis_white(folder=folder)
            ref.synthesis_babble(folder=folder, noise_folder=babble, save_json_file=os.path.join(tmp, "babble.json"))
            n_babble = len(picks)
            ref.synthesis_natural(folder=folder, noise_folder=musan, save_json_file=os.path.join(tmp, "natural.json"))
        finally:
            random.choice, torch.randn_like, glob.glob = real_choice, real_randn_like, real_glob
        babble_json = json.load(open(os.path.join(tmp, "babble.json")))
        natural_json = json.load(open(os.path.join(tmp, "natural.json")))

    # the noise track of every (song, type) as the reference had it BEFORE its first in-place rescale
    noise = {}
    for k, name in enumerate(SONGS):
        d = os.path.join(folder, "data", name)
        noise[name, "accomp"] = NL.seeded_track(SONGS[name][0], ACCOMP_SEEDS[name], "noise")
        noise[name, "white"] = whites[k][0]
        noise[name, "babble"] = store[os.path.join(d, "noise_data", "babble", "noise.wav")][0]
        noise[name, "natural"] = store[os.path.join(d, "noise_data", "natural", "noise.wav")][0]

    def chunks(n):
        return round(-(-n // (SR * 10)))

    fx = {"inputs": inputs, "step": NL.STEP, "snrs_db": list(NL.SNRS_DB), "mix": {}, "white_sha256": {},
          "babble": {"order": list(babble_json), "splits": {k: v["split"] for k, v in babble_json.items()},
                     # synthesis_babble never reads the song's split: every song draws from the pool named by the last file LISTED
                     "pool_split": list(inputs["babble_files"])[-1].split("/")[-1].split("-")[0], "tracks": {}},
          "natural": {"order": list(natural_json), "splits": {k: v["split"] for k, v in natural_json.items()}, "tracks": {}}}
    for typ, lo in (("babble", 0), ("natural", n_babble)):
        at = lo
        for name, (n, _) in SONGS.items():
            fx[typ]["tracks"][name] = {"sha256": NL.sha256(noise[name, typ]), "picks": picks[at:at + chunks(n)]}
            at += chunks(n)
    assert at == len(picks), (at, len(picks))
    for name, (n, seed) in SONGS.items():
        clean = NL.seeded_track(n, seed)
        fx["white_sha256"][name] = NL.sha256(noise[name, "white"])
        idx = torch.arange(0, n, NL.STEP)
        for typ in ("accomp", "white", "babble", "natural"):
            v = noise[name, typ]
            amps = (NL.mean_abs_exact(clean), NL.mean_abs_exact(v))
            want, M = NL.formula(clean[idx], v[idx], NL.SNRS_DB, amps)
            for s, snr in enumerate(NL.SNRS_DB):
                got = store[os.path.join(folder, "data", name, "noise_data", typ, f"SNR_{snr}dB.wav")][0]
                assert got.shape[0] == n
                fx["mix"][name, typ, snr] = {"sha256": NL.sha256(got), "samples": got[idx].clone(),
                                            "ref_vs_fp64": NL.worst(got[idx], want[s], NL.limit(M[s]))}
    out = os.path.join(HERE, "noise_mix.pt")
    torch.save(fx, out)
    print("wrote", out, os.path.getsize(out), "bytes")
    print("ref_vs_fp64:", {k: round(v["ref_vs_fp64"], 2) for k, v in fx["mix"].items()})
    print("babble", fx["babble"]["pool_split"], fx["babble"]["tracks"], "\nnatural", fx["natural"]["splits"], fx["natural"]["tracks"])


if __name__ == "__main__":
    main()
