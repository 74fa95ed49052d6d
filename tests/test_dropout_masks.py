"""The dropout mask function and the layerdrop draws on the CPU (no GPU, no library).

tests/dropout_cases.py restates the mask function of include/svt_mi355.h in numpy; here it is checked against the Philox generator's
published known answers and its keep rule at the edge rates, the seeds the GPU cases use are checked to give tensors whose dropped share
is unremarkable (a condition on the INPUTS of those tests, not a measurement), and ``draw_layerdrop`` is run against HF's encoder loops
themselves: the same skipped layers and the same host generator state afterwards.
"""
import dataclasses
import json
import math
import os

import numpy as np
import pytest
import torch

import dropout_cases as DC
import svt_speechbrain_amd as S
from svt_speechbrain_amd.dropout import draw_layerdrop

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def hexwords(w):
    return " ".join("%08x" % int(v) for v in w)


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10."""
    assert hexwords(DC.philox4x32_10([0, 0, 0, 0], (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    ones = 0xFFFFFFFF
    assert hexwords(DC.philox4x32_10([ones] * 4, (ones, ones))) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert hexwords(DC.philox4x32_10([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], (0xA4093822, 0x299F31D0))) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"
    # the vectorised form gives the same words as one counter at a time
    ctr = np.array([[0, 0, 0, 0], [ones] * 4, [5, 1, 2 | 3 << 8, 7]], dtype=np.uint64)
    both = DC.philox4x32_10(ctr, (11, 12))
    for i in range(3):
        assert np.array_equal(both[i], DC.philox4x32_10(ctr[i], (11, 12)))


def test_counter_layout():
    """counter = (q_lo, q_hi, site | layer << 8, step), key = (seed_lo, seed_hi), word e & 3, q = e >> 2."""
    seed, step, site, layer = 0x0123456789ABCDEF, 9, 4, 7
    for e in (0, 1, 5, 2 ** 32 - 2, 2 ** 34 + 1, 2 ** 34 + 3):
        q = e >> 2
        w = DC.philox4x32_10([q & 0xFFFFFFFF, q >> 32, site | layer << 8, step], (seed & 0xFFFFFFFF, seed >> 32))
        assert int(DC.words(seed, step, site, layer, 1, e0=e)[0]) == int(w[e & 3])
    # a run of elements crossing group boundaries equals the elements one by one
    run = DC.words(seed, step, site, layer, 11, e0=2 ** 34 + 1)
    assert [int(v) for v in run] == [int(DC.words(seed, step, site, layer, 1, e0=2 ** 34 + 1 + i)[0]) for i in range(11)]


def test_keep_rule_at_the_edge_rates():
    below = math.nextafter(2.0 ** -32, 0.0)
    assert [DC.threshold(p) for p in (0.0, below, 2.0 ** -32, 0.1, 0.5, 1 - 2.0 ** -24)] == [0, 0, 1, 429496729, 2 ** 31, 2 ** 32 - 256]
    assert DC.scale(0.0) == 1 and DC.scale(below) == 1 and DC.scale(0.5) == 2 and DC.scale(1 - 2.0 ** -24) == 2.0 ** 24
    assert DC.scale(0.1) == np.float32(1.0 / 0.9) and DC.scale(0.1).dtype == np.float32
    seed, step = 77, 1
    n = 4096
    w = DC.words(seed, step, 0, 0, n)
    x = np.linspace(-2, 2, n, dtype=np.float32)
    for p in (0.0, below):               # nothing can be dropped: a word is never below 0
        assert DC.keep(p, seed, step, 0, 0, n).all()
        assert np.array_equal(DC.apply(x, p, seed, step, 0, 0).view(np.uint32), x.view(np.uint32))
    assert np.array_equal(DC.keep(2.0 ** -32, seed, step, 0, 0, n), w != 0)      # only the word 0 is dropped
    for p in (0.1, 0.5, 1 - 2.0 ** -24):
        k = DC.keep(p, seed, step, 0, 0, n)
        assert np.array_equal(k, w >= DC.threshold(p))
        y = DC.apply(x, p, seed, step, 0, 0)
        assert np.array_equal(y[k].view(np.uint32), (x[k] * DC.scale(p)).astype(np.float32).view(np.uint32))
        assert not y[~k].view(np.uint32).any()                                   # +0, whatever the sign of the input
    assert DC.keep(1 - 2.0 ** -24, seed, step, 0, 0, n).sum() <= 2               # about n / 2^24 survive


def test_masks_of_different_sites_layers_and_steps_differ():
    seed, n, p = 0xFEEDFACE12345678, 2048, 0.5
    base = DC.keep(p, seed, 0, 0, 0, n)
    seen = {base.tobytes()}
    for site, layer, step, sd in ((1, 0, 0, seed), (0, 1, 0, seed), (0, 0, 1, seed), (2, 1, 0, seed), (0, 0, 0, seed + 1), (0, 0, 0, seed ^ (1 << 32)),
                                  (0, 256, 0, seed)):
        m = DC.keep(p, sd, step, site, layer, n)
        assert abs(float((m != base).mean()) - 0.5) < 0.1     # not merely different: uncorrelated
        seen.add(m.tobytes())
    assert len(seen) == 8
    assert np.array_equal(DC.keep(p, seed, 0, 0, 0, n), base)   # and a function: the same words give the same mask


def geometry(fam):
    with open(os.path.join(GOLDEN, DC.LOCAL, DC.FAMILIES[fam][0], "config.json")) as fh:
        j = json.load(fh)
    return j["hidden_size"], j["intermediate_size"], j["num_attention_heads"], j["num_hidden_layers"]


# the (seed, step) pairs tests/test_gpu_encoder_dropout.py uses on the wav2vec2-base geometry (B = 2, 1 s: T = 49)
BASE_SEEDS = [(0xA5A5A5A55A5A5A5A, 0), (0xA5A5A5A55A5A5A5A, 1), (0x1234567887654321, 5)]


def test_the_seeds_of_the_gpu_cases_give_unremarkable_masks():
    """Dropped share of every tensor within 5 sqrt(p (1 - p) / n) of p."""
    T, B = 49, 2
    checked = 0
    for fam, name in DC.case_list():
        D, F, H, L = geometry(fam)
        fields = DC.case_fields(fam, name)
        for site, layer, p, n in DC.site_tensors(fields, B, T, D, F, H, L):
            share = 1.0 - float(DC.keep(p, DC.mask_seed(fam, name), DC.STEP, site, layer, n).mean())
            assert abs(share - p) <= 5 * math.sqrt(p * (1 - p) / n), (fam, name, site, layer, share)
            checked += 1
    fields = dict(DC.ZERO, hidden_dropout=0.1, attention_dropout=0.1, activation_dropout=0.1, feat_proj_dropout=0.1)
    for seed, step in BASE_SEEDS:
        for site, layer, p, n in DC.site_tensors(fields, B, T, 768, 3072, 12, 2):
            share = 1.0 - float(DC.keep(p, seed, step, site, layer, n).mean())
            assert abs(share - p) <= 5 * math.sqrt(p * (1 - p) / n), (seed, step, site, layer, share)
            checked += 1
    assert checked > 100


def hf_encoder(kind, layerdrop, layers=6):
    from transformers import Wav2Vec2Config, WavLMConfig
    from transformers.models.wav2vec2.modeling_wav2vec2 import Wav2Vec2Encoder, Wav2Vec2EncoderStableLayerNorm
    from transformers.models.wavlm.modeling_wavlm import WavLMEncoder
    kw = dict(hidden_size=16, num_hidden_layers=layers, num_attention_heads=2, intermediate_size=16, num_conv_pos_embeddings=4,
              num_conv_pos_embedding_groups=2, hidden_dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, feat_proj_dropout=0.0,
              layerdrop=layerdrop, attn_implementation="eager")
    torch.manual_seed(1)
    if kind == "wavlm":
        return WavLMEncoder(WavLMConfig(num_buckets=8, max_bucket_distance=16, **kw))
    if kind == "stable":
        return Wav2Vec2EncoderStableLayerNorm(Wav2Vec2Config(do_stable_layer_norm=True, **kw))
    return Wav2Vec2Encoder(Wav2Vec2Config(**kw))


@pytest.mark.parametrize("kind", ["wav2vec2", "stable", "wavlm"])
@pytest.mark.parametrize("layerdrop", [0.0, 0.1, 0.5, 0.9])
def test_layerdrop_draws_match_hf_encoder_loop(kind, layerdrop):
    enc = hf_encoder(kind, layerdrop).train()
    ran = []
    for l, layer in enumerate(enc.layers):
        layer.register_forward_pre_hook(lambda m, a, l=l: ran.append(l))
    x = torch.zeros(1, 5, 16)
    patterns = set()
    for seed in range(8):
        ran.clear()
        torch.manual_seed(seed)
        with torch.no_grad():
            enc(x)
        want = tuple(l not in ran for l in range(len(enc.layers)))
        want_digest = DC.host_rng_digest()
        torch.manual_seed(seed)
        got = draw_layerdrop(len(enc.layers), layerdrop, "wavlm" if kind == "wavlm" else "wav2vec2")
        assert got == want, (seed, got, want)
        assert DC.host_rng_digest() == want_digest          # as many draws, of the same kind
        patterns.add(got)
    if layerdrop == 0.0:
        assert patterns == {(False,) * 6}                    # drawn all the same (the digests above), never skipped
    if layerdrop == 0.5:
        assert len(patterns) > 4
    if kind == "wavlm":
        assert not any(p[0] for p in patterns)               # HF's WavLM never skips layer 0


def test_the_fixture_seeds_skip_what_the_case_table_says():
    for name, (fields, seed, want) in DC.CASES.items():
        torch.manual_seed(seed)
        assert draw_layerdrop(2, fields.get("layerdrop", 0.0)) == tuple(want), name


def test_config_intake_of_the_five_rates(tmp_path):
    from svt_speechbrain_amd.huggingface_interface import _config_from_dir
    for preset in S.PRESETS.values():
        assert all(getattr(preset, k) == 0.0 for k in DC.ZERO), preset.name
    src = os.path.join(GOLDEN, DC.LOCAL, "tiny-wav2vec2-hf", "config.json")
    with open(src) as fh:
        j = json.load(fh)
    assert all(getattr(_config_from_dir(os.path.dirname(src)), k) == 0.0 for k in DC.ZERO)
    j.update(hidden_dropout=0.05, attention_dropout=0.06, activation_dropout=0.07, feat_proj_dropout=0.08, layerdrop=0.09)
    (tmp_path / "config.json").write_text(json.dumps(j))
    c = _config_from_dir(str(tmp_path))
    assert (c.hidden_dropout, c.attention_dropout, c.activation_dropout, c.feat_proj_dropout, c.layerdrop) == (0.05, 0.06, 0.07, 0.08, 0.09)
    for k in DC.ZERO:     # a config.json written with use_diff=True omits what equals the class default
        j.pop(k)
    (tmp_path / "config.json").write_text(json.dumps(j))
    c = _config_from_dir(str(tmp_path))
    assert (c.hidden_dropout, c.attention_dropout, c.activation_dropout, c.feat_proj_dropout, c.layerdrop) == (0.1, 0.1, 0.1, 0.0, 0.1)
    assert dataclasses.replace(c, layerdrop=0.0).layerdrop == 0.0
