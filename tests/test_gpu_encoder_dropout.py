"""The encoder in training mode: the checkpoint's dropouts and layerdrop through HuggingFaceWav2Vec2 (svt_encoder_set_dropout).

References: tests/golden/encoder_dropout.pt and encoder_dropout_2.pt -- the reference's wrapper in train() mode with the masks of
tests/dropout_cases.py injected into torch's dropout entry points and HF's own layerdrop draws (tests/golden/
make_golden_encoder_dropout.py) -- under the project's parity bar of 1e-3 in fp32, with equal skipped layers and an equal host
generator state; the fp32-mode output for the 16-bit modes (same seeds, so the masks are identical by construction); and the plain
forward, bit for bit, wherever no rate applies.
"""
import dataclasses
import json
import os
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import svt_speechbrain_amd as S  # noqa: E402
from svt_speechbrain_amd import _lib, weights as W  # noqa: E402
import dropout_cases as DC  # noqa: E402

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RATES = dict(hidden_dropout=0.1, attention_dropout=0.1, activation_dropout=0.1, feat_proj_dropout=0.1, layerdrop=0.1)
BASE_SEED, BASE_SEED_2 = 0xA5A5A5A55A5A5A5A, 0x1234567887654321     # tests/test_dropout_masks.py checks the masks these give

_built = {}


def fixture_case(golden, fam, name):
    return golden(DC.FIXTURE_OF[fam])["cases"][f"{fam}/{name}"]


def case_encoder(golden, tmp_path_factory, fam, name, prec):
    """Our constructor on a copy of the case's directory with its config.json fields; built once per (family, case, precision)."""
    key = (fam, name, prec)
    if key not in _built:
        fx = fixture_case(golden, fam, name)
        d = str(tmp_path_factory.mktemp("drop") / fx["dir"])
        shutil.copytree(os.path.join(GOLDEN, DC.LOCAL, fx["dir"]), d)
        with open(os.path.join(d, "config.json")) as fh:
            cj = json.load(fh)
        cj.update(fx["fields"])
        with open(os.path.join(d, "config.json"), "w") as fh:
            json.dump(cj, fh)
        enc = S.HuggingFaceWav2Vec2(d, None, apply_spec_augment=bool(fx["fields"].get("apply_spec_augment", False)), freeze=False,
                                    precision=prec).to(DEV)
        assert enc.model.training and enc.training and enc.normalize_wav == fx["normalize_wav"]
        for k in DC.ZERO:
            assert getattr(enc.config, k) == fx["fields"][k]
        wav = DC.synth_wav(2, fx["n_samples"], fx["seed"])
        assert DC.wav_digest(wav) == fx["wav_sha256"]
        _built[key] = dict(fx=fx, enc=enc, wav=wav.to(DEV))
    return _built[key]


def drawn_forward(r):
    """The case's forward as the generator ran the reference's: torch's host generator and numpy's seeded by the case, the mask
    function's two words from the fixture.  Returns (output, last_dropout, host generator digest afterwards)."""
    fx, enc = r["fx"], r["enc"]
    torch.manual_seed(fx["seed"])
    np.random.seed(fx["seed"])
    with torch.no_grad():
        y = enc(r["wav"], dropout_seed=fx["mask_seed"], dropout_step=fx["step"]).clone()
    return y, dict(enc.last_dropout), DC.host_rng_digest()


@pytest.mark.parametrize("fam,name", DC.case_list())
def test_fp32_parity_with_the_reference(golden, tmp_path_factory, fam, name):
    r = case_encoder(golden, tmp_path_factory, fam, name, "fp32")
    fx = r["fx"]
    y, last, digest = drawn_forward(r)
    assert last["skipped"] == tuple(fx["skipped"]) and last["seed"] == fx["mask_seed"] and last["step"] == fx["step"]
    assert digest == fx["rng_digest"]                       # as many host draws as HF made, of the same kind
    err = (y.cpu() - fx["out"]).abs().max().item()
    print(f"{fam}/{name} fp32: max |y - reference| = {err:.3e} (the reference moves by {fx['on_off_gap']:.3f} against all rates 0)")
    assert y.shape == fx["out"].shape
    assert err < 1e-3, err


@pytest.mark.parametrize("fam,name", [(f, n) for f, n in DC.case_list() if n.startswith("skip")])
def test_split_modes_serve_layerdrop(golden, tmp_path_factory, fam, name, prec="fp16x3"):
    r = case_encoder(golden, tmp_path_factory, fam, name, prec)
    fx = r["fx"]
    y, last, digest = drawn_forward(r)
    assert last["skipped"] == tuple(fx["skipped"]) and digest == fx["rng_digest"]
    err = (y.cpu() - fx["out"]).abs().max().item()
    print(f"{fam}/{name} {prec}: max |y - reference| = {err:.3e}")
    assert err < 1e-3, err     # the parity bar, as the SpecAugment cases hold fp16x3 to it


def gap_pair(enc32, enc16, wav, **kw):
    """(gap with the dropouts on, gap of the plain forward) between a 16-bit mode and the fp32 mode of one model."""
    with torch.no_grad():
        on = (enc16(wav, **kw) - enc32(wav, **kw)).abs().max().item()
        enc32.eval(), enc16.eval()
        try:
            off = (enc16(wav) - enc32(wav)).abs().max().item()      # eval(): the plain path, the parent commit's behaviour
        finally:
            enc32.train(), enc16.train()
    return on, off


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("fam", list(DC.FAMILIES))
def test_16_bit_modes_stay_near_the_fp32_mode(golden, tmp_path_factory, fam, prec):
    """Same seeds, so the masks are identical by construction: the gap to the fp32-mode output is at most 3 x the gap of the plain
    forward measured here (the margin covers 1 / (1 - p) <= 1.25 and the move from the fused to the score-matrix attention)."""
    r32 = case_encoder(golden, tmp_path_factory, fam, "all", "fp32")
    r16 = case_encoder(golden, tmp_path_factory, fam, "all", prec)
    fx = r32["fx"]
    on, off = gap_pair(r32["enc"], r16["enc"], r32["wav"], dropout_seed=fx["mask_seed"], dropout_step=fx["step"], skip_layers=(False, False))
    print(f"{fam}/all {prec}: gap to the fp32 mode {on:.3e} with the dropouts, {off:.3e} plain")
    assert on <= 3 * off, (on, off)


def small_base(**rates):
    """wav2vec2-base's geometry (hidden 768, head dim 64: the (hi, lo) residual stream, 16-bit branches and the fused attention of the
    16-bit modes; what the fused head serves) with two transformer layers."""
    return dataclasses.replace(S.PRESETS["wav2vec2-base"], name="wav2vec2-base-2l", num_hidden_layers=2, **rates)


def base_encoder(prec="fp32", rates=RATES, **kw):
    cfg = small_base(**rates)
    kw.setdefault("freeze", False)
    return cfg, S.HuggingFaceWav2Vec2("wav2vec2-base", None, config=cfg, precision=prec, seed=13, **kw).to(DEV)


@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp16x3"])
def test_16_bit_modes_stay_near_the_fp32_mode_at_the_base_geometry(prec):
    """... and with layers skipped, the last one and all of them (the families' first LayerNorm is then also the last).  The split mode
    runs the same skips with layerdrop alone, which is what it serves."""
    rates = RATES if prec != "fp16x3" else dict(layerdrop=0.1)
    _, e32 = base_encoder("fp32", rates=rates)
    _, e16 = base_encoder(prec, rates=rates)
    wav = DC.synth_wav(2, 16000, 41).to(DEV)
    for skip in ((False, False), (False, True), (True, True)):
        on, off = gap_pair(e32, e16, wav, dropout_seed=BASE_SEED, dropout_step=0, skip_layers=skip)
        print(f"base geometry {prec} skipped {skip}: gap to the fp32 mode {on:.3e} with the dropouts, {off:.3e} plain")
        assert on <= 3 * off, (skip, on, off)


@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16", "fp16x3"])
def test_eval_and_zero_rates_are_the_plain_forward_bit_for_bit(prec):
    wav = DC.synth_wav(2, 16000, 43).to(DEV)
    rates = RATES if prec != "fp16x3" else dict(layerdrop=0.5)
    with torch.no_grad():
        _, never = base_encoder(prec, rates={}, freeze=True)
        plain = never(wav).clone()
        _, zero = base_encoder(prec, rates={})                   # training mode, every rate 0: nothing is drawn, nothing is called
        torch.manual_seed(5)
        before = DC.host_rng_digest()
        assert torch.equal(zero(wav), plain) and zero.last_dropout is None and zero.dropout_step == 0
        assert DC.host_rng_digest() == before
        _, enc = base_encoder(prec, rates=rates)
        a = enc(wav, dropout_seed=BASE_SEED, skip_layers=(False, True)).clone()
        assert not torch.equal(a, plain)
        assert enc.last_dropout == dict(seed=BASE_SEED, step=0, skipped=(False, True)) and enc.dropout_step == 1
        enc.eval()                                               # eval(): the state is dropped, the forward is the plain one again
        before = DC.host_rng_digest()
        assert torch.equal(enc(wav), plain) and enc.last_dropout is None and enc.dropout_step == 1
        assert DC.host_rng_digest() == before
        enc.train()
        assert torch.equal(enc(wav, dropout_seed=BASE_SEED, dropout_step=0, skip_layers=(False, True)), a)
        _, frozen = base_encoder(prec, rates=rates, freeze=True)  # freeze=True is eval()
        assert torch.equal(frozen(wav), plain) and frozen.last_dropout is None
        with pytest.raises(ValueError, match="training-mode forward"):
            frozen(wav, dropout_step=3)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_seed_and_step_decide_the_forward(prec):
    _, enc = base_encoder(prec)
    wav = DC.synth_wav(2, 16000, 45).to(DEV)
    skip = (False, False)
    with torch.no_grad():
        a = enc(wav, dropout_seed=BASE_SEED, dropout_step=0, skip_layers=skip).clone()
        assert enc.last_dropout == dict(seed=BASE_SEED, step=0, skipped=skip) and enc.dropout_step == 0   # an explicit step leaves the counter
        b = enc(wav, dropout_seed=BASE_SEED, dropout_step=0, skip_layers=skip).clone()
        c = enc(wav, dropout_seed=BASE_SEED, dropout_step=1, skip_layers=skip).clone()
        d = enc(wav, dropout_seed=BASE_SEED_2, dropout_step=0, skip_layers=skip).clone()
        assert torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(a, d)
        assert (a - c).abs().max().item() > 1e-2
        # the module's counter: step 0, then 1 -- the two forwards above
        torch.manual_seed(3)
        enc.dropout_step = 0
        e0 = enc(wav, dropout_seed=BASE_SEED).clone()
        s0 = enc.last_dropout
        e1 = enc(wav, dropout_seed=BASE_SEED).clone()
        s1 = enc.last_dropout
        assert (s0["step"], s1["step"], enc.dropout_step) == (0, 1, 2)
        assert torch.equal(e0, enc(wav, dropout_seed=BASE_SEED, dropout_step=0, skip_layers=s0["skipped"]))
        assert torch.equal(e1, enc(wav, dropout_seed=BASE_SEED, dropout_step=1, skip_layers=s1["skipped"]))
        # the seed defaults to the device generator's
        torch.manual_seed(77)
        enc(wav)
        assert enc.last_dropout["seed"] == torch.cuda.initial_seed() == 77
        with pytest.raises(ValueError, match="one bool per layer"):
            enc(wav, skip_layers=(True,))


def test_forward_head_equals_head_of_forward():
    cfg, enc = base_encoder("fp32")
    head = S.Linear(20, input_size=cfg.hidden_size)
    head.load_state_dict(W.seeded_head_state_dict(cfg.hidden_size, 20, seed=14))
    head = head.to(DEV)
    wav = DC.synth_wav(2, 16000, 47).to(DEV)
    kw = dict(dropout_seed=BASE_SEED, dropout_step=1, skip_layers=(False, False))
    with torch.no_grad():
        enc.eval()
        plain = head(enc(wav))
        enc.train()
        ref = head(enc(wav, **kw))
        got = enc.forward_head(wav, head, **kw)
        assert (ref - plain).abs().max().item() > 1e-2          # the dropouts matter
        err = (got - ref).abs().max().item()
        assert err < 2e-4, err                                  # the bound of tests/test_gpu_parity.py's fused-tail comparison
        torch.manual_seed(9)
        a = enc.forward_head(wav, head, dropout_seed=BASE_SEED)  # drawn layerdrop and the module's step reach the fused call as well
        last = enc.last_dropout
        assert torch.equal(a, enc.forward_head(wav, head, dropout_seed=BASE_SEED, dropout_step=last["step"], skip_layers=last["skipped"]))


def test_linear_probe_trains_on_the_dropped_features():
    cfg, enc = base_encoder("fp32")
    B, L = 2, 16000
    T = cfg.frames(L)
    wav = DC.synth_wav(B, L, 49).to(DEV)
    g = torch.Generator().manual_seed(8)
    anno = torch.stack([(torch.rand(B, T, generator=g) < 0.2).float(), (torch.rand(B, T, generator=g) < 0.2).float(),
                        torch.randint(0, 5, (B, T), generator=g).float(), torch.randint(0, 13, (B, T), generator=g).float()], -1).to(DEV)

    def head():
        h = S.Linear(20, input_size=cfg.hidden_size)
        h.load_state_dict(W.seeded_head_state_dict(cfg.hidden_size, 20, seed=14))
        return h.to(DEV)

    probe = S.LinearProbe({"wav2vec2": enc, "model": head()}, lr=1.0)
    probe2 = S.LinearProbe({"wav2vec2": enc, "model": head()}, lr=1.0)
    torch.manual_seed(123)
    enc.dropout_step = 5
    for i in range(2):
        loss = probe.fit_batch(wav, None, anno)
        last = dict(enc.last_dropout)
        assert last["step"] == 5 + i and last["seed"] == 123        # one training-mode forward per step
        with torch.no_grad():
            feats = enc(wav, dropout_seed=last["seed"], dropout_step=last["step"], skip_layers=last["skipped"])
        assert enc.dropout_step == 6 + i                             # ... and the explicit step did not move the counter
        loss2 = probe2.fit_features(feats, None, anno)
        assert torch.equal(loss, loss2) and probe.last_terms == probe2.last_terms, i


def test_refused_combinations_say_why(golden, tmp_path_factory):
    wav = DC.synth_wav(2, 16000, 51).to(DEV)
    for prec in ("fp16x3", "bf16x3"):
        for field in ("hidden_dropout", "attention_dropout", "activation_dropout", "feat_proj_dropout"):
            _, enc = base_encoder(prec, rates={field: 0.1})
            with pytest.raises(_lib.SvtError, match=f"precision {prec} serves layerdrop only"):
                enc(wav)
            enc.eval()
            with torch.no_grad():
                enc(wav)                                             # the refused call left nothing behind
    r = case_encoder(golden, tmp_path_factory, "wavlm", "hidden", "fp32")
    enc = r["enc"]
    cfg = enc.config
    try:
        enc.config = dataclasses.replace(cfg, attention_dropout=0.1)
        with pytest.raises(_lib.SvtError, match="WavLM"):
            enc(r["wav"])
        enc.config = cfg
        with pytest.raises(_lib.SvtError, match="layer 0"):
            enc(r["wav"], skip_layers=(True, False))
    finally:
        enc.config = cfg
    lib = _lib.load()
    h = enc._dev.slot(0, (enc.normalize_wav, enc.output_norm, enc.precision)).handle
    st = _lib.DropoutC()
    st.struct_size = 8
    assert lib.svt_encoder_set_dropout(h, st) == -1 and "struct_size" in _lib.last_error(lib)
    import ctypes
    st.struct_size = ctypes.sizeof(_lib.DropoutC)
    st.hidden_dropout = 1.0
    assert lib.svt_encoder_set_dropout(h, st) == -1 and "[0, 1)" in _lib.last_error(lib)
    st.hidden_dropout = 0.0
    st.skip_mask = 4
    assert lib.svt_encoder_set_dropout(h, st) == -1 and "num_layers" in _lib.last_error(lib)
    assert lib.svt_encoder_set_dropout(h, None) == 0


def test_workspace_follows_the_state():
    """svt_encoder_workspace_bytes counts the score and probability buffers only while a state with attention_dropout > 0 is set."""
    import ctypes
    _, enc = base_encoder("bf16")
    wav = DC.synth_wav(2, 16000, 53).to(DEV)
    lib = enc._lib()
    with torch.no_grad():
        enc(wav, dropout_seed=BASE_SEED)
    h = enc._dev.slot(0, (enc.normalize_wav, enc.output_norm, enc.precision)).handle
    with_state = lib.svt_encoder_workspace_bytes(h, 2, 16000)
    assert lib.svt_encoder_set_dropout(h, None) == 0
    plain = lib.svt_encoder_workspace_bytes(h, 2, 16000)
    st = _lib.DropoutC()
    st.struct_size = ctypes.sizeof(_lib.DropoutC)
    st.hidden_dropout = 0.1
    assert lib.svt_encoder_set_dropout(h, st) == 0
    assert lib.svt_encoder_workspace_bytes(h, 2, 16000) == plain      # no attention dropout: the fused attention, no score buffers
    assert lib.svt_encoder_set_dropout(h, None) == 0
    # S (fp32) and P (16-bit) of 2 clips x 12 heads x 49 x 56 are 395 136 bytes; V^T shrinks from 64 to 56 padded keys (24 576 bytes)
    assert 350000 < with_state - plain < 400000, with_state - plain
    _, e2 = base_encoder("bf16", rates={}, freeze=True)
    with torch.no_grad():
        e2(wav)
    h2 = e2._dev.slot(0, (e2.normalize_wav, e2.output_norm, e2.precision)).handle
    assert lib.svt_encoder_workspace_bytes(h2, 2, 16000) == plain      # ... which is what a handle that never had a state asks for
