"""The host side of apply_spec_augment=True (svt_speechbrain_amd/spec_augment.py, HuggingFaceWav2Vec2's constructor): no GPU needed.

The mask-only table of tests/golden/spec_augment.pt was recorded from transformers' own ``_compute_mask_indices`` (numpy's global
generator seeded per row): ``compute_mask_indices`` must give the same mask AND leave the generator in the same state, which pins the
number, order and arguments of its draws.
"""
import os

import numpy as np
import pytest
import torch

import svt_speechbrain_amd as S
from svt_speechbrain_amd import spec_augment as SA
from svt_speechbrain_amd.huggingface_interface import _config_from_dir

from spec_augment_cases import CASES, FAMILIES, MASK_ROWS, synth_wav, wav_digest

HERE = os.path.dirname(os.path.abspath(__file__))
LOCAL = os.path.join(HERE, "golden", "local_ckpt")


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("spec_augment")


def test_fixture_covers_the_cases(fixture):
    assert sorted(fixture["cases"]) == sorted(f"{f}/{c}" for f in FAMILIES for c in CASES)
    assert [(r["shape"], r["prob"], r["length"], r["min_masks"], r["seed"]) for r in fixture["masks"]] == [tuple(r) for r in MASK_ROWS]
    for key, c in fixture["cases"].items():
        fields, n, seed = CASES[c["case"]]
        assert (c["fields"], c["n_samples"], c["seed"]) == (fields, n, seed), key
        assert wav_digest(synth_wav(2, n, seed)) == c["wav_sha256"], key   # the input the tests regenerate is the recorded one


@pytest.mark.parametrize("i", range(len(MASK_ROWS)))
def test_mask_table_row(fixture, i):
    row = fixture["masks"][i]
    np.random.seed(row["seed"])
    m = SA.compute_mask_indices(row["shape"], row["prob"], row["length"], row["min_masks"])
    assert m.dtype == np.bool_ and m.shape == tuple(row["shape"])
    assert np.array_equal(m, row["mask"].numpy()), MASK_ROWS[i]
    assert SA.generator_digest() == row["rng_digest"], MASK_ROWS[i]


def test_zero_span_row_is_all_false_and_consumes_the_epsilon(fixture):
    np.random.seed(1)
    before = SA.generator_digest()
    m = SA.compute_mask_indices((2, 24), 0.0, 10, 0)
    assert not m.any() and SA.generator_digest() != before
    np.random.seed(1)
    np.random.rand(1)
    assert SA.generator_digest() == fixture["masks"][0]["rng_digest"]


def test_value_errors():
    state = SA.generator_digest()
    with pytest.raises(ValueError, match="`mask_length` has to be bigger than 0."):
        SA.compute_mask_indices((2, 24), 0.3, 0)
    with pytest.raises(ValueError, match="`mask_length` has to be smaller than `sequence_length`"):
        SA.compute_mask_indices((2, 9), 0.3, 10)
    assert SA.generator_digest() == state   # refused before any draw, as in HF


@pytest.mark.parametrize("family", FAMILIES)
def test_case_masks_from_the_config(fixture, family, tmp_path):
    """draw_masks on the fields of each case = the two masks the reference's model drew, in its order, with its generator state."""
    cfg0 = _config_from_dir(os.path.join(LOCAL, family))
    assert (cfg0.mask_time_prob, cfg0.mask_time_length, cfg0.mask_time_min_masks) == (0.05, 10, 2)
    assert (cfg0.mask_feature_prob, cfg0.mask_feature_length, cfg0.mask_feature_min_masks) == (0.0, 10, 0)
    import dataclasses
    for name, (fields, n, seed) in CASES.items():
        c = fixture["cases"][f"{family}/{name}"]
        cfg = dataclasses.replace(cfg0, **fields)
        np.random.seed(seed)
        tm, fm = SA.draw_masks(cfg, 2, cfg.frames(n))
        for got, want in ((tm, c["time_mask"]), (fm, c["feature_mask"])):
            assert (got is None) == (want is None), (family, name)
            if got is not None:
                assert np.array_equal(got, want.numpy()), (family, name)
        assert SA.generator_digest() == c["rng_digest"], (family, name)


def test_config_defaults_are_hfs():
    c = S.PRESETS["wav2vec2-base"]
    assert (c.mask_time_prob, c.mask_time_length, c.mask_time_min_masks, c.mask_feature_prob, c.mask_feature_length,
            c.mask_feature_min_masks) == (0.05, 10, 2, 0.0, 10, 0)


def test_constructor_accepts_the_flag(golden):
    d = os.path.join(LOCAL, "tiny-wav2vec2-hf")
    enc = S.HuggingFaceWav2Vec2(d, None, apply_spec_augment=True, freeze=False)
    assert enc.apply_spec_augment and enc.model.training
    ck = torch.load(os.path.join(d, "pytorch_model.bin"), map_location="cpu")
    assert torch.equal(enc.model.masked_spec_embed.detach(), ck["masked_spec_embed"])   # loaded, not seeded
    keys = list(enc.state_dict().keys())
    assert "model.masked_spec_embed" in keys
    # the flag adds that one key and nothing else
    rec = golden("local_ckpt")["tiny-wav2vec2-hf"]["keys"]
    assert sorted(k[len("model."):] for k in keys) == sorted(rec)
    # freeze=True is eval(): the flag is accepted, the parameter exists, nothing will be drawn
    frozen = S.HuggingFaceWav2Vec2(d, None, apply_spec_augment=True)
    assert not frozen.model.training and not frozen.model.masked_spec_embed.requires_grad


def test_seeded_embed_leaves_the_other_weights_alone():
    cfg = S.PRESETS["tiny-group"]
    a = S.HuggingFaceWav2Vec2("tiny-group", None, config=cfg, seed=11)
    b = S.HuggingFaceWav2Vec2("tiny-group", None, config=cfg, seed=11, apply_spec_augment=True)
    sa, sb = a.state_dict(), b.state_dict()
    assert [k for k in sb if k not in sa] == ["model.masked_spec_embed"]
    for k, v in sa.items():
        assert torch.equal(v, sb[k]), k
    e = sb["model.masked_spec_embed"]
    assert e.shape == (cfg.hidden_size,) and 0.0 <= float(e.min()) and float(e.max()) < 1.0 and float(e.std()) > 0.1   # uniform_()
    c = S.HuggingFaceWav2Vec2("tiny-group", None, config=cfg, seed=11, apply_spec_augment=True)
    assert torch.equal(c.state_dict()["model.masked_spec_embed"], e)                      # from the seed
    d = S.HuggingFaceWav2Vec2("tiny-group", None, config=cfg, seed=12, apply_spec_augment=True)
    assert not torch.equal(d.state_dict()["model.masked_spec_embed"], e)


@pytest.mark.parametrize("family", FAMILIES)
def test_flag_off_keeps_the_key_list(golden, family):
    rec = golden("local_ckpt")[family]["keys"]
    enc = S.HuggingFaceWav2Vec2(os.path.join(LOCAL, family), None)
    keys = sorted(k[len("model."):] for k in enc.state_dict().keys())
    assert keys == sorted(k for k in rec if k != "masked_spec_embed")
    # and a state dict that carries the key still loads, the key dropped
    sd = dict(enc.state_dict())
    sd["model.masked_spec_embed"] = torch.zeros(enc.config.hidden_size)
    enc.load_state_dict(sd, strict=True)
    assert "model.masked_spec_embed" not in enc.state_dict()


def test_flag_on_state_dict_round_trip():
    d = os.path.join(LOCAL, "tiny-wav2vec2-hf")
    a = S.HuggingFaceWav2Vec2(d, None, apply_spec_augment=True)
    b = S.HuggingFaceWav2Vec2("tiny-group", None, config=a.config, seed=3, apply_spec_augment=True)
    b.load_state_dict(a.state_dict(), strict=True)
    assert torch.equal(b.model.masked_spec_embed.detach(), a.model.masked_spec_embed.detach())


def test_explicit_masks_need_the_flag():
    enc = S.HuggingFaceWav2Vec2("tiny-group", None, config=S.PRESETS["tiny-group"], seed=11)
    with pytest.raises(ValueError, match="apply_spec_augment=True"):
        enc._set_spec_masks(None, None, torch.device("cpu"), 2, 12, np.zeros((2, 12), bool), None)


def test_eval_mode_and_flag_off_leave_numpys_generator_alone():
    """The decision to draw is made on the host before any device call: eval mode, or the flag off, draws nothing."""

    class Slot:
        masks = None

    np.random.seed(5)
    before = SA.generator_digest()
    for kw in (dict(apply_spec_augment=True), dict(apply_spec_augment=False), dict(apply_spec_augment=False, freeze=False)):
        enc = S.HuggingFaceWav2Vec2("tiny-group", None, config=S.PRESETS["tiny-group"], seed=11, **kw)
        enc._set_spec_masks(None, Slot(), torch.device("cpu"), 2, 24, None, None)   # nothing set before: no library call either
        assert enc.last_spec_masks == (None, None)
        assert SA.generator_digest() == before, kw
