"""svt_spec_augment on the GPU (csrc/spec_augment.hip) and apply_spec_augment=True through the encoder.

The kernel is a copy and a zero, so every check of it is bit for bit: the buffer is filled with seeded random BIT patterns (NaNs with
payloads, infinities and subnormals among them, and a few planted ones) between poisoned guard rows, the expected image is built on the
host from the three-way rule of include/svt_mi355.h, and the whole buffer -- guards and row padding included -- is compared as integers.

Through the encoder the references are tests/golden/spec_augment.pt (the reference's wrapper with apply_spec_augment=True, in train()
mode with dropouts and layerdrop at 0; tests/golden/make_golden_spec_augment.py) under the project's parity bar of 1e-3, and the plain
forward, bit for bit, wherever nothing is masked.
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
from svt_speechbrain_amd import _lib, spec_augment as SA, weights as W  # noqa: E402
from spec_augment_cases import CASES, FAMILIES, synth_wav, wav_digest  # noqa: E402

DEV = "cuda:0"
POISON = 0x7FC0DEAD   # a NaN with a payload: a write of any value, NaN included, changes the bits
GUARD = 2             # guard rows in front of and behind the tensor
INVALID, KEY = -1, -2
LOCAL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "local_ckpt")


# ---------------------------------------------------------------------------------------------------------------- the kernel alone
def bits(n, seed):
    """n seeded int32 bit patterns: uniform over all 2^32, so about 1 in 256 is a NaN or an infinity; four planted on top."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=g, dtype=torch.int64).to(torch.int32)
    planted = torch.tensor([0x7FC00001, 0x7F800000, -0x7FFFFF, 0x00000001], dtype=torch.int64).to(torch.int32)   # NaN, inf, -NaN payload, subnormal
    v[:min(4, n)] = planted[:min(4, n)]
    return v


def run(B, T, D, ld, tm, fm, embed=True, seed=0, expect=0, over=None):
    """One svt_spec_augment call.  tm (B, T) / fm (B, D) bool or None.  Returns (buffer after, expected buffer), both int32 on the CPU,
    guard rows and row padding included."""
    lib = _lib.load()
    rows = B * T
    host = torch.full(((rows + 2 * GUARD) * ld,), POISON, dtype=torch.int32)
    body = host[GUARD * ld:(GUARD + rows) * ld].view(rows, ld)
    body[:, :D] = bits(rows * D, 1000 + seed).view(rows, D)
    e = bits(D, 2000 + seed)
    want = host.clone()
    wb = want[GUARD * ld:(GUARD + rows) * ld].view(B, T, ld)
    if tm is not None:
        wb[:, :, :D][tm] = e
    if fm is not None:
        wb[:, :, :D][fm[:, None, :].expand(B, T, D)] = 0
    buf = host.to(DEV)
    e_d = e.to(DEV)
    tm_d = tm.to(torch.uint8).to(DEV).contiguous() if tm is not None else None
    fm_d = fm.to(torch.uint8).to(DEV).contiguous() if fm is not None else None
    a = dict(h=_lib.ptr(buf) + 4 * GUARD * ld, B=B, T=T, D=D, ld=ld, tm=_lib.ptr(tm_d) if tm_d is not None else None,
             fm=_lib.ptr(fm_d) if fm_d is not None else None, e=_lib.ptr(e_d) if embed else None)
    a.update(over or {})   # arguments passed instead of the true ones (the refusals)
    rc = lib.svt_spec_augment(a["h"], a["B"], a["T"], a["D"], a["ld"], a["tm"], a["fm"], a["e"], 0, _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert rc == expect, (rc, _lib.last_error())
    return buf.cpu(), want if expect == 0 else host


def same(got, want):
    return bool(torch.equal(got, want))


def zeros(*shape):
    return torch.zeros(shape, dtype=torch.bool)


@pytest.mark.parametrize("pad", [0, 4])
@pytest.mark.parametrize("D", [64, 768, 1024])
@pytest.mark.parametrize("T", [1, 5, 12])
def test_kernel_bit_exact(T, D, pad):
    B, ld = 3, D + pad
    g = torch.Generator().manual_seed(T * 7 + D + pad)
    cases = {}
    cases["both NULL"] = (None, None)
    cases["all-zero masks"] = (zeros(B, T), zeros(B, D))
    cases["all-zero time mask alone"] = (zeros(B, T), None)
    cases["every row"] = (~zeros(B, T), None)
    first = zeros(B, T); first[1, 0] = True
    last = zeros(B, T); last[1, T - 1] = True; last[2, T - 1] = True
    cases["first row of a clip"] = (first, None)
    cases["last row of a clip"] = (last, None)
    c0 = zeros(B, D); c0[:, 0] = True
    c1 = zeros(B, D); c1[:, D - 1] = True
    cases["first column"] = (None, c0)
    cases["last column"] = (None, c1)
    one = zeros(B, D); one[1] = torch.rand(D, generator=g) < 0.2
    cases["feature mask on one clip of three"] = (None, one)
    full4 = zeros(B, D); full4[0, 4:8] = True; full4[2, D - 8:D - 3] = True    # a whole 16-byte piece, and one and a bit
    cases["whole 16-byte pieces"] = (None, full4)
    tm = torch.rand(B, T, generator=g) < 0.4
    tm[0, 0] = True
    fm = torch.rand(B, D, generator=g) < 0.2
    fm[2] = False
    cases["time and feature together"] = (tm, fm)
    cases["every row and every column"] = (~zeros(B, T), ~zeros(B, D))
    for i, (name, (t, f)) in enumerate(cases.items()):
        got, want = run(B, T, D, ld, t, f, seed=i)
        assert same(got, want), (name, int((got != want).sum()))
        if name == "time and feature together":   # masked rows hold embed with the columns zeroed: spelled out once, not only via `want`
            e = bits(D, 2000 + i)
            body = got[GUARD * ld:(GUARD + B * T) * ld].view(B, T, ld)
            b, tt = 0, 0
            assert torch.equal(body[b, tt, :D], torch.where(fm[b], torch.zeros_like(e), e))
            assert body[:, :, :D][fm[:, None, :].expand(B, T, D)].abs().sum() == 0


@pytest.mark.parametrize("B,T,D", [(2, 37, 64), (1, 16, 128), (1, 17, 128), (8200, 1, 64)])
def test_kernel_more_than_one_tile_and_the_grid_stride(B, T, D):
    """16 frames per workgroup: 37 = two tiles and a ragged third, 16 / 17 = the tile exactly and one more; 8 200 clips of one frame are more
    jobs than the grid's cap of 8 192 workgroups, so some workgroups take a second one."""
    g = torch.Generator().manual_seed(B + T)
    tm = torch.rand(B, T, generator=g) < 0.3
    tm[B - 1, T - 1] = True
    fm = torch.rand(B, D, generator=g) < 0.1
    fm[B // 2] = False
    for t, f in ((tm, fm), (tm, None), (None, fm)):
        got, want = run(B, T, D, D, t, f, seed=5)
        assert same(got, want)


def test_kernel_refusals():
    t, f = ~zeros(3, 5), ~zeros(3, 64)
    for kw, text in ((dict(D=66), "D must be a multiple of 4"), (dict(ld=70), "ld must be a multiple of 4"), (dict(ld=60), "ld < D"),
                     (dict(B=0), "empty"), (dict(T=0), "empty"), (dict(h=None), "null")):
        got, want = run(3, 5, 64, 64, t, f, expect=INVALID, over=kw)
        assert text in _lib.last_error(), (kw, _lib.last_error())
        assert same(got, want), kw                    # nothing was written
    got, want = run(3, 5, 64, 64, t, None, embed=False, expect=INVALID)
    assert "embed" in _lib.last_error() and same(got, want)
    got, want = run(3, 5, 64, 64, None, f, embed=False)   # a feature mask alone needs no embedding
    assert same(got, want)
    # misaligned pointers: h 4 bytes off, the feature mask 1 byte off
    buf = torch.zeros(3 * 5 * 64 + 8, dtype=torch.float32, device=DEV)
    m = torch.zeros(3 * 64 + 8, dtype=torch.uint8, device=DEV)
    lib = _lib.load()
    assert lib.svt_spec_augment(_lib.ptr(buf) + 4, 3, 5, 64, 64, None, _lib.ptr(m), None, 0, _lib.stream_ptr(DEV)) == INVALID
    assert "aligned" in _lib.last_error()
    assert lib.svt_spec_augment(_lib.ptr(buf), 3, 5, 64, 64, None, _lib.ptr(m) + 1, None, 0, _lib.stream_ptr(DEV)) == INVALID
    assert "aligned" in _lib.last_error()
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0


# ---------------------------------------------------------------------------------------------------------------- through the encoder
MODES = ["fp32", "bf16", "bf16x3", "fp16x3", "fp16"]   # the four precision codes of libsvt_mi355.so and the IEEE-half build's 16-bit mode


def tiny(prec, **kw):
    return S.HuggingFaceWav2Vec2("tiny-group", None, config=S.PRESETS["tiny-group"], precision=prec, seed=11, **kw).to(DEV)


@pytest.mark.parametrize("prec", MODES)
def test_nothing_masked_is_the_plain_forward_bit_for_bit(prec):
    wav = synth_wav(2, 8000, 7).to(DEV)
    T, D = 24, 64
    with torch.no_grad():
        plain = tiny(prec)(wav).clone()                                   # the flag off: today's forward
        assert torch.equal(tiny(prec, freeze=False)(wav), plain)          # ... in training mode too
        on_eval = tiny(prec, apply_spec_augment=True)                     # freeze=True is eval(): nothing is drawn
        np.random.seed(3)
        before = SA.generator_digest()
        assert torch.equal(on_eval(wav), plain)
        assert SA.generator_digest() == before and on_eval.last_spec_masks == (None, None)
        # all-False masks SET: the pass runs and changes nothing
        for tm, fm in ((np.zeros((2, T), bool), np.zeros((2, D), bool)), (torch.zeros(2, T, dtype=torch.bool, device=DEV), None),
                       (None, torch.zeros(2, D, dtype=torch.bool))):
            assert torch.equal(on_eval(wav, mask_time_indices=tm, mask_feature_indices=fm), plain)
        # and a forward after a masked one is the plain one again: the masks do not outlive their call
        tm = np.zeros((2, T), bool)
        tm[0, 3:9] = True
        assert not torch.equal(on_eval(wav, mask_time_indices=tm), plain)
        assert torch.equal(on_eval(wav), plain)
        # a training-mode encoder whose probabilities are both 0 draws nothing and is the plain forward
        on_train = tiny(prec, apply_spec_augment=True, freeze=False)
        on_train.config = dataclasses.replace(on_train.config, mask_time_prob=0.0, mask_feature_prob=0.0)
        assert torch.equal(on_train(wav), plain) and SA.generator_digest() == before


_built = {}


def case_run(golden, tmp_path_factory, family, name, prec):
    """The encoder of a fixture case -- our constructor on a copy of the directory with the case's config.json fields -- and its drawn
    forward, built once per (family, case, precision)."""
    key = (family, name, prec)
    if key not in _built:
        fx = golden("spec_augment")["cases"][f"{family}/{name}"]
        d = str(tmp_path_factory.mktemp("sa") / family)
        shutil.copytree(os.path.join(LOCAL, family), d)
        with open(os.path.join(d, "config.json")) as fh:
            cj = json.load(fh)
        cj.update(fx["fields"])
        with open(os.path.join(d, "config.json"), "w") as fh:
            json.dump(cj, fh)
        enc = S.HuggingFaceWav2Vec2(d, None, apply_spec_augment=True, freeze=False, precision=prec).to(DEV)
        assert enc.model.training and enc.normalize_wav == fx["normalize_wav"]
        wav = synth_wav(2, fx["n_samples"], fx["seed"])
        assert wav_digest(wav) == fx["wav_sha256"]
        wav = wav.to(DEV)
        np.random.seed(fx["seed"])
        with torch.no_grad():
            y = enc(wav).clone()
        _built[key] = dict(fx=fx, enc=enc, wav=wav, y=y, masks=enc.last_spec_masks, digest=SA.generator_digest())
    return _built[key]


ALL_CASES = [(f, c) for f in FAMILIES for c in CASES]


@pytest.mark.parametrize("prec", ["fp32", "fp16x3"])
@pytest.mark.parametrize("family,name", ALL_CASES)
def test_parity_with_the_reference(golden, tmp_path_factory, family, name, prec):
    r = case_run(golden, tmp_path_factory, family, name, prec)
    fx = r["fx"]
    for got, want in zip(r["masks"], (fx["time_mask"], fx["feature_mask"])):
        assert (got is None) == (want is None)
        if got is not None:
            assert np.array_equal(got, want.numpy())
    assert r["digest"] == fx["rng_digest"]
    err = (r["y"].cpu() - fx["out"]).abs().max().item()
    off = (r["y"].cpu() - fx["out_off"]).abs().max().item()
    print(f"{family}/{name} {prec}: max |y - reference| = {err:.3e}; against the reference with the flag off {off:.3f}")
    assert r["y"].shape == fx["out"].shape
    assert err < 1e-3, err


@pytest.mark.parametrize("prec", ["fp32", "fp16x3"])
@pytest.mark.parametrize("family,name", ALL_CASES)
def test_explicit_masks_equal_the_drawn_run(golden, tmp_path_factory, family, name, prec):
    r = case_run(golden, tmp_path_factory, family, name, prec)
    enc, wav, (tm, fm) = r["enc"], r["wav"], r["masks"]
    np.random.seed(1)
    before = SA.generator_digest()
    with torch.no_grad():
        assert torch.equal(enc(wav, mask_time_indices=tm, mask_feature_indices=fm), r["y"])          # host masks
        dev = [None if m is None else torch.from_numpy(m).to(DEV) for m in (tm, fm)]
        assert torch.equal(enc.extract_features(wav, mask_time_indices=dev[0], mask_feature_indices=dev[1]), r["y"])   # device masks
        enc.model.eval()
        try:
            assert torch.equal(enc(wav, mask_time_indices=tm, mask_feature_indices=fm), r["y"])      # any mode
        finally:
            enc.model.train()
    assert SA.generator_digest() == before   # explicit masks bypass the draw


def small_base():
    """wav2vec2-base's geometry (hidden size 768: what the fused head and the head's backward serve) with two transformer layers."""
    return dataclasses.replace(S.PRESETS["wav2vec2-base"], name="wav2vec2-base-2l", num_hidden_layers=2)


def base_encoder(**kw):
    cfg = small_base()
    enc = S.HuggingFaceWav2Vec2("wav2vec2-base", None, config=cfg, precision="fp32", seed=13, apply_spec_augment=True, **kw).to(DEV)
    head = S.Linear(20, input_size=cfg.hidden_size)
    head.load_state_dict(W.seeded_head_state_dict(cfg.hidden_size, 20, seed=14))
    return cfg, enc, head.to(DEV)


def test_forward_head_with_masks_equals_head_of_forward():
    cfg, enc, head = base_encoder()
    B, L = 2, 16000
    T = cfg.frames(L)
    wav = synth_wav(B, L, 15).to(DEV)
    np.random.seed(21)
    tm = SA.compute_mask_indices((B, T), 0.3, 3, 2)
    fm = SA.compute_mask_indices((B, cfg.hidden_size), 0.2, 2, 0)
    with torch.no_grad():
        plain = head(enc(wav))
        ref = head(enc(wav, mask_time_indices=tm, mask_feature_indices=fm))
        got = enc.forward_head(wav, head, mask_time_indices=tm, mask_feature_indices=fm)
        assert (ref - plain).abs().max().item() > 1e-2      # the masks matter
        err = (got - ref).abs().max().item()
        assert err < 2e-4, err          # the bound of tests/test_gpu_parity.py's fused-tail comparison
        assert (enc.forward_head(wav, head) - plain).abs().max().item() < 2e-4   # and cleared again
        # drawn masks in training mode reach the fused call as well
        enc.model.train()
        np.random.seed(21)
        a = enc.forward_head(wav, head)
        drawn = enc.last_spec_masks
        assert drawn[0] is not None and drawn[1] is None    # HF's defaults: a time mask only
        assert torch.equal(a, enc.forward_head(wav, head, mask_time_indices=drawn[0]))


def test_geometry_mismatch_is_an_error():
    enc = tiny("fp32", apply_spec_augment=True)
    wav = synth_wav(2, 8000, 7).to(DEV)   # (B, T) = (2, 24)
    with torch.no_grad():
        for shape in ((2, 25), (2, 23), (3, 24), (1, 24)):
            with pytest.raises(_lib.SvtError, match="SpecAugment masks were set for"):
                enc(wav, mask_time_indices=np.zeros(shape, bool))
        with pytest.raises(_lib.SvtError, match="SpecAugment masks were set for"):
            enc(wav, mask_feature_indices=np.zeros((3, 64), bool))
        with pytest.raises(ValueError):
            enc(wav, mask_feature_indices=np.zeros((2, 60), bool))
        with pytest.raises(ValueError, match="batch size"):
            enc(wav, mask_time_indices=np.zeros((2, 24), bool), mask_feature_indices=np.zeros((3, 64), bool))
        y = enc(wav)   # the refused calls left no mask behind
        assert torch.equal(y, tiny("fp32")(wav))
    with pytest.raises(ValueError, match="apply_spec_augment=True"):
        tiny("fp32")(wav, mask_time_indices=np.zeros((2, 24), bool))


def test_time_mask_needs_the_embedding_and_the_c_abi_checks_the_geometry():
    lib = _lib.load()
    wav = synth_wav(2, 8000, 7).to(DEV)
    off = tiny("fp32")
    with torch.no_grad():
        off(wav)
    h = off._dev.slot(0, (off.normalize_wav, off.output_norm, off.precision)).handle
    m = torch.zeros(2 * 64, dtype=torch.uint8, device=DEV)
    assert lib.svt_encoder_set_spec_augment(h, _lib.ptr(m), None, 2, 24) == KEY and "masked_spec_embed" in _lib.last_error()
    assert lib.svt_encoder_set_spec_augment(h, None, _lib.ptr(m), 0, 24) == INVALID
    assert lib.svt_encoder_set_spec_augment(h, None, _lib.ptr(m) + 1, 2, 24) == INVALID
    assert lib.svt_encoder_set_spec_augment(h, None, _lib.ptr(m), 2, 24) == 0      # a feature mask alone needs no embedding
    assert lib.svt_encoder_set_spec_augment(h, None, None, 0, 0) == 0
    on = tiny("fp32", apply_spec_augment=True)
    with torch.no_grad():
        on(wav)
    buf = torch.empty(64)
    assert lib.svt_encoder_get_param(on._dev.slot(0, (on.normalize_wav, on.output_norm, on.precision)).handle, b"masked_spec_embed",
                                     buf.data_ptr(), 64) == 0
    assert torch.equal(buf, on.model.masked_spec_embed.detach().cpu())


def test_linear_probe_draws_once_per_step_and_trains_on_the_masked_features():
    cfg, enc, head = base_encoder(freeze=False)
    B, L = 2, 16000
    T = cfg.frames(L)
    wav = synth_wav(B, L, 31).to(DEV)
    g = torch.Generator().manual_seed(8)
    anno = torch.stack([(torch.rand(B, T, generator=g) < 0.2).float(), (torch.rand(B, T, generator=g) < 0.2).float(),
                        torch.randint(0, 5, (B, T), generator=g).float(), torch.randint(0, 13, (B, T), generator=g).float()], -1).to(DEV)
    probe = S.LinearProbe({"wav2vec2": enc, "model": head}, lr=1.0)
    np.random.seed(77)
    terms, losses, drawn = [], [], []
    for _ in range(2):
        losses.append(probe.fit_batch(wav, None, anno))
        terms.append(dict(probe.last_terms))
        drawn.append(enc.last_spec_masks)
    after = SA.generator_digest()
    # exactly two time-mask draws (HF's defaults: the feature probability is 0), by hand
    c = enc.config
    np.random.seed(77)
    hand = [SA.compute_mask_indices((B, T), c.mask_time_prob, c.mask_time_length, c.mask_time_min_masks) for _ in range(2)]
    assert SA.generator_digest() == after
    for d, m in zip(drawn, hand):
        assert d[1] is None and np.array_equal(d[0], m) and m.any()
    # the same two steps from the explicitly masked features, on a head that starts alike
    head2 = S.Linear(20, input_size=cfg.hidden_size)
    head2.load_state_dict(W.seeded_head_state_dict(cfg.hidden_size, 20, seed=14))
    head2 = head2.to(DEV)
    probe2 = S.LinearProbe({"wav2vec2": enc, "model": head2}, lr=1.0)
    for i in range(2):
        with torch.no_grad():
            feats = enc(wav, mask_time_indices=hand[i])
        loss = probe2.fit_features(feats, None, anno)
        assert probe2.last_terms == terms[i] and torch.equal(loss, losses[i]), i
    assert SA.generator_digest() == after
    for k, v in head.state_dict().items():
        assert torch.equal(v, head2.state_dict()[k]), k
