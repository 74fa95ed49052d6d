"""Generate tests/golden/spec_augment.pt by running the REFERENCE's wrapper with apply_spec_augment=True.

Runs only in the build container (needs the reference checkout and HF transformers); the fixture it writes holds data only.

    python tests/golden/make_golden_spec_augment.py

Two tables:

``cases``: the reference's real constructor (``HuggingFaceWav2Vec2(source=<dir>, save_path=..., apply_spec_augment=True, freeze=False)``,
MIR_ST500/huggingface_interface.py:89-150) on a copy of each HF tiny directory of ``local_ckpt/`` whose config.json carries the case's
``mask_*`` fields, and its forward in ``train()`` mode on the CPU.  The directories' dropouts and layerdrop are 0 (make_golden.hf_model),
and the HuBERT directory's positional BatchNorm1d is put back into ``eval()`` (running statistics: a training-mode BatchNorm would
normalise with the batch's own and move them, which this project's forward-only encoder does not do any more than dropout).  numpy is
seeded before each call; per case the fixture holds the seed, the input's digest (``spec_augment_cases.synth_wav`` regenerates it), the
two masks HF drew (captured from its ``_compute_mask_indices``), a digest of numpy's generator state after the call, the output, and
the same model's output with the flag off.

``masks``: rows of (shape, prob, length, min_masks, seed) -> mask and generator-state digest from HF's ``_compute_mask_indices`` alone.
"""
from __future__ import annotations

import hashlib
import json
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from make_golden import import_reference  # noqa: E402
from spec_augment_cases import CASES, FAMILIES, MASK_ROWS, synth_wav, wav_digest  # noqa: E402
from svt_speechbrain_amd.spec_augment import generator_digest  # noqa: E402


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    hi, _, _ = import_reference()
    out = {"cases": {}, "masks": []}
    for fam in FAMILIES:
        src = os.path.join(HERE, "local_ckpt", fam)
        for name, (fields, n_samples, seed) in CASES.items():
            with tempfile.TemporaryDirectory() as tmp:
                d = os.path.join(tmp, fam)   # the reference picks the model class by substring of the path
                shutil.copytree(src, d)
                with open(os.path.join(d, "config.json")) as fh:
                    cj = json.load(fh)
                cj.update(fields)
                with open(os.path.join(d, "config.json"), "w") as fh:
                    json.dump(cj, fh)
                ref = hi.HuggingFaceWav2Vec2(source=d, save_path=os.path.join(tmp, "cache"), apply_spec_augment=True, freeze=False)
            assert ref.model.training and ref.model.config.apply_spec_augment
            for m in ref.model.modules():
                if isinstance(m, torch.nn.BatchNorm1d):
                    m.eval()
            mod = sys.modules[type(ref.model).__module__]
            real = mod._compute_mask_indices
            drawn = []

            def capture(*a, **k):
                m = real(*a, **k)
                drawn.append(np.array(m, copy=True))
                return m

            wav = synth_wav(2, n_samples, seed)
            mod._compute_mask_indices = capture
            try:
                np.random.seed(seed)
                with torch.no_grad():
                    y = ref(wav).clone()
                digest = generator_digest()
            finally:
                mod._compute_mask_indices = real
            want_t, want_f = cj["mask_time_prob"] > 0, cj["mask_feature_prob"] > 0
            assert len(drawn) == int(want_t) + int(want_f), (fam, name, len(drawn))
            tm = drawn[0] if want_t else None
            fm = drawn[-1] if want_f else None
            ref.model.config.apply_spec_augment = False
            state = np.random.get_state()
            with torch.no_grad():
                y_off = ref(wav).clone()
            assert generator_digest() == digest and state[2] == np.random.get_state()[2]   # the flag off draws nothing
            T, D = y.shape[1], y.shape[2]
            if tm is not None:
                assert tm.shape == (2, T)
                if name != "clamp":
                    assert all(0 < int(r.sum()) < T for r in tm), (fam, name, tm.sum(1))
                assert tm.any()
            if fm is not None:
                assert fm.shape == (2, D) and all(0 < int(r.sum()) < D for r in fm), (fam, name)
            diff = (y - y_off).abs().max().item()
            assert diff > 1e-2, (fam, name, diff)   # ten times the parity bar: a case below that shows nothing
            out["cases"][f"{fam}/{name}"] = dict(
                family=fam, case=name, fields=dict(fields), n_samples=n_samples, seed=seed, wav_sha256=wav_digest(wav),
                time_mask=None if tm is None else torch.from_numpy(tm), feature_mask=None if fm is None else torch.from_numpy(fm),
                rng_digest=digest, out=y, out_off=y_off, normalize_wav=bool(ref.normalize_wav))
            print(f"{fam}/{name}: T={T} time {None if tm is None else tm.sum(1).tolist()} feature "
                  f"{None if fm is None else fm.sum(1).tolist()} max|on - off| = {diff:.3f}")
    from transformers.models.wav2vec2.modeling_wav2vec2 import _compute_mask_indices
    for shape, prob, length, min_masks, seed in MASK_ROWS:
        np.random.seed(seed)
        m = _compute_mask_indices(tuple(shape), prob, length, min_masks=min_masks)
        out["masks"].append(dict(shape=tuple(shape), prob=prob, length=length, min_masks=min_masks, seed=seed,
                                 mask=torch.from_numpy(np.array(m, copy=True)), rng_digest=generator_digest()))
        print(shape, prob, length, min_masks, seed, "->", m.sum(1).tolist())
    path = os.path.join(HERE, "spec_augment.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path), "bytes", hashlib.sha256(open(path, "rb").read()).hexdigest()[:16])


if __name__ == "__main__":
    main()
