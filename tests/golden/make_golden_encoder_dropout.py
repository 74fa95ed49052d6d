"""Generate tests/golden/encoder_dropout.pt and encoder_dropout_2.pt (and the model directory tests/golden/local_ckpt/tiny-wav2vec2-dh64-hf) by running the REFERENCE's
wrapper in training mode with the dropout masks of tests/dropout_cases.py injected into it.

Runs only in the build container (needs the reference checkout and HF transformers); what it writes holds data only.

    python tests/golden/make_golden_encoder_dropout.py

Per case (``dropout_cases.case_list``): the reference's real constructor (``HuggingFaceWav2Vec2(source=<dir>, save_path=...,
apply_spec_augment=<case>, freeze=False)``, MIR_ST500/huggingface_interface.py:89-150) on a copy of the family's tiny directory whose
config.json carries the case's rates, and its forward in ``train()`` mode on the CPU, with HuBERT's positional BatchNorm1d back in
``eval()`` and the attention in HF's eager form.  torch draws its dropout masks from a generator whose offsets depend on its launch
geometry, so no parity with ITS masks is claimed: ``nn.Dropout.forward`` and ``nn.functional.dropout`` are replaced by a function that
multiplies by the mask ``dropout_cases`` computes for that site, layer and step.  The site is known from the MODULE -- every
``nn.Dropout`` of the model is labelled by its qualified name, and a forward pre-hook on each layer's attention names the layer whose
probabilities ``nn.functional.dropout`` is about to see -- not from the call order, which layerdrop changes.  Layerdrop itself is HF's
own: its ``torch.rand([])`` per layer from torch's host generator, seeded by the case; the fixture records which layers ran and a
digest of the generator state afterwards.  The same model's output with every rate at 0 is computed per case and must differ by more
than 1e-2 (ten times the parity bar); it is not stored.  The cases are split over two files by family (``dropout_cases.FIXTURE_OF``)
to keep each under the repository's 1 MiB per file.
"""
from __future__ import annotations

import dataclasses
import hashlib
import json
import os
import re
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

from make_golden import hf_model, import_reference  # noqa: E402
import dropout_cases as DC  # noqa: E402

SITE_OF = [(re.compile(r"^feature_projection\.dropout$"), DC.SITE_FEAT_PROJ), (re.compile(r"^encoder\.dropout$"), DC.SITE_ENCODER),
           (re.compile(r"^encoder\.layers\.(\d+)\.dropout$"), DC.SITE_ATTN_OUT),
           (re.compile(r"^encoder\.layers\.(\d+)\.feed_forward\.intermediate_dropout$"), DC.SITE_ACTIVATION),
           (re.compile(r"^encoder\.layers\.(\d+)\.feed_forward\.output_dropout$"), DC.SITE_FFN_OUT)]


def make_dh64_dir():
    """The head-dim-64 model of the fixture: tiny-group's front end with hidden 128, 2 heads, 2 layers, seeded weights of this project's
    own initialiser, written as a HuggingFace directory (config.json, preprocessor_config.json, pytorch_model.bin: data only)."""
    import svt_speechbrain_amd as S
    from svt_speechbrain_amd.weights import seeded_encoder_state_dict
    cfg = dataclasses.replace(S.PRESETS["tiny-group"], name="tiny-dh64", hidden_size=128, num_attention_heads=2, intermediate_size=128,
                              num_conv_pos_embedding_groups=16)   # (sized to stay under the repository's 1 MiB per file)
    d = os.path.join(HERE, DC.LOCAL, DC.FAMILIES["dh64"][0])
    os.makedirs(d, exist_ok=True)
    m = hf_model(cfg)
    sd = {k: v for k, v in seeded_encoder_state_dict(cfg, seed=64).items()}
    own = m.state_dict()
    for k in own:
        if k not in sd:
            assert k == "masked_spec_embed", k
            sd[k] = torch.zeros_like(own[k])
    m.load_state_dict(sd, strict=True)
    torch.save({k: v.clone() for k, v in m.state_dict().items()}, os.path.join(d, "pytorch_model.bin"))
    cj = m.config.to_dict()
    cj.pop("_name_or_path", None)
    with open(os.path.join(d, "config.json"), "w") as fh:
        json.dump(cj, fh, indent=1, sort_keys=True)
    shutil.copy(os.path.join(HERE, DC.LOCAL, "tiny-wav2vec2-hf", "preprocessor_config.json"), os.path.join(d, "preprocessor_config.json"))
    print(d, {f: os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)})


class Injector:
    """Replaces torch's two dropout entry points while a reference forward runs."""

    def __init__(self, model, seed, step):
        self.seed, self.step, self.on = seed, step, True
        self.attn_layer = None
        self.used = []
        self.ran = []
        self.hooks = []
        for name, m in model.named_modules():
            if isinstance(m, torch.nn.Dropout):
                for rx, site in SITE_OF:
                    mt = rx.match(name)
                    if mt:
                        m._svt_site = (site, int(mt.group(1)) if mt.groups() else 0)
                        break
                else:
                    assert m.p == 0, f"an nn.Dropout this fixture does not know: {name} (p = {m.p})"
            mt = re.match(r"^encoder\.layers\.(\d+)$", name)
            if mt:
                l = int(mt.group(1))
                self.hooks.append(m.register_forward_pre_hook(lambda mod, a, l=l: self.ran.append(l)))
                self.hooks.append(m.attention.register_forward_pre_hook(lambda mod, a, l=l: setattr(self, "attn_layer", l), with_kwargs=False))

    def __enter__(self):
        inj = self
        self.real_fwd, self.real_fn = torch.nn.Dropout.forward, torch.nn.functional.dropout

        def fwd(mod, x):
            if not mod.training or mod.p == 0 or not inj.on:
                return x
            site, layer = mod._svt_site
            inj.used.append((site, layer, mod.p, x.numel()))
            return DC.apply_torch(x, mod.p, inj.seed, inj.step, site, layer)

        def fn(x, p=0.5, training=True, inplace=False):
            if not training or p == 0 or not inj.on:
                return x
            assert x.dim() == 4 and inj.attn_layer is not None, "functional dropout outside the eager attention"
            inj.used.append((DC.SITE_ATTN_PROBS, inj.attn_layer, p, x.numel()))
            return DC.apply_torch(x, p, inj.seed, inj.step, DC.SITE_ATTN_PROBS, inj.attn_layer)

        torch.nn.Dropout.forward, torch.nn.functional.dropout = fwd, fn
        return self

    def __exit__(self, *a):
        torch.nn.Dropout.forward, torch.nn.functional.dropout = self.real_fwd, self.real_fn
        for h in self.hooks:
            h.remove()


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    make_dh64_dir()
    hi, _, _ = import_reference()
    out = {f: {"cases": {}} for f in sorted(set(DC.FIXTURE_OF.values()))}
    for fam, name in DC.case_list():
        sub, _, wavlm_like = DC.FAMILIES[fam]
        fields = DC.case_fields(fam, name)
        _, seed, want_skip = DC.CASES[name]
        mseed = DC.mask_seed(fam, name)
        spec = bool(fields.get("apply_spec_augment", False))
        with tempfile.TemporaryDirectory() as tmp:
            d = os.path.join(tmp, sub)   # the reference picks the model class by substring of the path
            shutil.copytree(os.path.join(HERE, DC.LOCAL, sub), d)
            with open(os.path.join(d, "config.json")) as fh:
                cj = json.load(fh)
            cj.update(fields)
            with open(os.path.join(d, "config.json"), "w") as fh:
                json.dump(cj, fh)
            ref = hi.HuggingFaceWav2Vec2(source=d, save_path=os.path.join(tmp, "cache"), apply_spec_augment=spec, freeze=False)
        model = ref.model
        assert model.training
        if not wavlm_like:
            model.config._attn_implementation = "eager"
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.eval()
        hc = model.config
        for k in DC.ZERO:
            assert abs(getattr(hc, k) - fields[k]) < 1e-12, (fam, name, k)
        wav = DC.synth_wav(2, DC.N_SAMPLES, seed)
        with Injector(model, mseed, DC.STEP) as inj:
            torch.manual_seed(seed)
            np.random.seed(seed)
            with torch.no_grad():
                y = ref(wav).clone()
            digest = DC.host_rng_digest()
            ran = sorted(set(inj.ran))
            skipped = tuple(l not in ran for l in range(hc.num_hidden_layers))
            used = list(inj.used)
            # the same model with every rate at 0: nothing injected, no layer skipped, no SpecAugment
            inj.on = False
            ld, hc.layerdrop = hc.layerdrop, 0.0
            sa, hc.apply_spec_augment = hc.apply_spec_augment, False
            with torch.no_grad():
                y_off = ref(wav).clone()
            hc.layerdrop, hc.apply_spec_augment = ld, sa
        assert skipped == tuple(want_skip), (fam, name, skipped)
        # every site the rates switch on was applied, in the layers that ran, on tensors of the expected size -- and nothing else
        B, T, D = y.shape
        want = [t for t in DC.site_tensors(fields, B, T, D, hc.intermediate_size, hc.num_attention_heads, hc.num_hidden_layers)
                if t[0] < 2 or not skipped[t[1]]]
        assert sorted(used) == sorted(want), (fam, name, sorted(used), sorted(want))
        diff = (y - y_off).abs().max().item()
        assert diff > 1e-2, (fam, name, diff)   # ten times the parity bar: a smaller effect shows nothing
        out[DC.FIXTURE_OF[fam]]["cases"][f"{fam}/{name}"] = dict(
            family=fam, case=name, dir=sub, fields=fields, n_samples=DC.N_SAMPLES, seed=seed, mask_seed=mseed, step=DC.STEP,
            wav_sha256=DC.wav_digest(wav), skipped=skipped, rng_digest=digest, out=y, on_off_gap=diff, normalize_wav=bool(ref.normalize_wav))
        print(f"{fam}/{name}: T={T} skipped {skipped} sites {sorted(set((s, l) for s, l, _, _ in used))} max|on - off| = {diff:.3f}")
    for f, table in out.items():
        path = os.path.join(HERE, f + ".pt")
        torch.save(table, path)
        print(path, os.path.getsize(path), "bytes", hashlib.sha256(open(path, "rb").read()).hexdigest()[:16])


if __name__ == "__main__":
    main()
