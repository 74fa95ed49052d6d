"""The encoder in training mode with ``fused_attention_dropout=True``: the attention of the 16-bit modes keeps its fused kernel and
computes the dropout mask inside it (csrc/attention_drop.hip) instead of materialising the (B, H, T, T) scores.

The mask is the same function of position, so the yardsticks are those of tests/test_gpu_encoder_dropout.py: the fp32-mode output at
the same (seed, step, skipped layers) under that file's bar (the gap is at most 3 x the plain forward's gap measured in the same test),
the plain forward bit for bit wherever no attention dropout applies, and the flag-off forward bit for bit wherever the fused kernels do
not serve the geometry.  The helpers (the two-layer wav2vec2-base geometry, the golden families' encoders) are that file's."""
import ctypes
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

import svt_speechbrain_amd as S  # noqa: E402
from svt_speechbrain_amd import _lib, weights as W  # noqa: E402
import dropout_cases as DC  # noqa: E402
import test_gpu_encoder_dropout as ED  # noqa: E402

DEV = ED.DEV
SEED = ED.BASE_SEED
NEW_IDS = {9, 10}     # svt_debug_set key 38: flash_attn_drop_kernel<64, 4>, <128, 4>
NONE = (False, False)


def handle(enc):
    return enc._dev.slot(0, (enc.normalize_wav, enc.output_norm, enc.precision)).handle


@pytest.mark.parametrize("n_samples,frames", [(16000, 49), (48000, 149)])   # one key tile; three tiles and two query blocks
@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_base_geometry_stays_near_the_fp32_mode(prec, n_samples, frames):
    cfg, e32 = ED.base_encoder("fp32")
    _, e16 = ED.base_encoder(prec, fused_attention_dropout=True)
    assert e16.fused_attention_dropout is True and cfg.frames(n_samples) == frames
    wav = DC.synth_wav(2, n_samples, 41).to(DEV)
    kw = dict(dropout_seed=SEED, dropout_step=0, skip_layers=NONE)
    lib = e16._lib()
    with torch.no_grad():
        a = e16(wav, **kw).clone()
        assert lib.svt_debug_set(38, 0) in NEW_IDS, lib.svt_debug_set(38, 0)
        assert torch.equal(e16(wav, **kw), a)                                   # the same (seed, step) twice
        assert not torch.equal(e16(wav, **dict(kw, dropout_step=1)), a)         # step + 1
        on, off = ED.gap_pair(e32, e16, wav, **kw)
        e16.fused_attention_dropout = False
        b = e16(wav, **kw).clone()
        assert lib.svt_debug_set(38, 0) not in NEW_IDS                          # eval() in gap_pair ran the plain fused kernel last
        score_gap = (b - e32(wav, **kw)).abs().max().item()
    print(f"base geometry {prec} T={frames}: gap to the fp32 mode {on:.3e} with the fused masked attention, {score_gap:.3e} with the "
          f"score-matrix path, {off:.3e} plain; flag on against flag off {(a - b).abs().max().item():.3e}")
    assert on <= 3 * off, (on, off)
    assert not torch.equal(a, b)          # the two forms round the probabilities in different places


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("rates", ["all", "attention"])
def test_head_dim_64_family_stays_near_the_fp32_mode(golden, tmp_path_factory, rates, prec):
    r32 = ED.case_encoder(golden, tmp_path_factory, "dh64", "all", "fp32")
    r16 = ED.case_encoder(golden, tmp_path_factory, "dh64", "all", prec)
    fx, e32, e16 = r32["fx"], r32["enc"], r16["enc"]
    cfg32, cfg16 = e32.config, e16.config
    kw = dict(dropout_seed=fx["mask_seed"], dropout_step=fx["step"], skip_layers=NONE)
    try:
        if rates == "attention":
            only = dict(DC.ZERO, attention_dropout=0.1)
            e32.config, e16.config = dataclasses.replace(cfg32, **only), dataclasses.replace(cfg16, **only)
        e16.fused_attention_dropout = True
        with torch.no_grad():
            e16(r32["wav"], **kw)
            assert e16._lib().svt_debug_set(38, 0) in NEW_IDS
            on, off = ED.gap_pair(e32, e16, r32["wav"], **kw)
    finally:
        e16.fused_attention_dropout = False
        e32.config, e16.config = cfg32, cfg16
    print(f"dh64/{rates} {prec}: gap to the fp32 mode {on:.3e} with the fused masked attention, {off:.3e} plain")
    assert on <= 3 * off, (on, off)


@pytest.mark.parametrize("fam,prec", [("wav2vec2", "bf16"), ("hubert", "fp16"), ("dh64", "fp32")])
def test_unserved_geometries_ignore_the_flag(golden, tmp_path_factory, fam, prec):
    """Head sizes other than 64 / 128 in the 16-bit modes, and the fp32 mode at any head size: flag on is flag off, bit for bit."""
    r = ED.case_encoder(golden, tmp_path_factory, fam, "all", prec)
    enc, fx = r["enc"], r["fx"]
    kw = dict(dropout_seed=fx["mask_seed"], dropout_step=fx["step"], skip_layers=NONE)
    try:
        with torch.no_grad():
            off = enc(r["wav"], **kw).clone()
            enc.fused_attention_dropout = True
            on = enc(r["wav"], **kw).clone()
            assert enc._lib().svt_debug_set(38, 0) not in NEW_IDS
    finally:
        enc.fused_attention_dropout = False
    assert torch.equal(on, off)


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_flag_without_attention_dropout_is_the_plain_forward(prec):
    wav = DC.synth_wav(2, 16000, 43).to(DEV)
    with torch.no_grad():
        _, never = ED.base_encoder(prec, rates={}, freeze=True)
        plain = never(wav).clone()
        _, enc = ED.base_encoder(prec, fused_attention_dropout=True)
        a = enc(wav, dropout_seed=SEED, dropout_step=0, skip_layers=NONE).clone()
        assert not torch.equal(a, plain)
        torch.manual_seed(5)
        before = DC.host_rng_digest()
        enc.eval()                                                   # eval(): the plain forward, the host generator untouched
        assert torch.equal(enc(wav), plain) and enc.last_dropout is None
        enc.train()
        _, frozen = ED.base_encoder(prec, freeze=True, fused_attention_dropout=True)    # freeze=True is eval()
        assert torch.equal(frozen(wav), plain) and frozen.last_dropout is None
        _, zero = ED.base_encoder(prec, rates={}, fused_attention_dropout=True)          # every rate 0: nothing is set
        assert torch.equal(zero(wav), plain) and zero.last_dropout is None
        assert DC.host_rng_digest() == before
        # attention_dropout == 0 beside other rates: the flag changes nothing
        rates = dict(ED.RATES, attention_dropout=0.0)
        _, off = ED.base_encoder(prec, rates=rates)
        _, on = ED.base_encoder(prec, rates=rates, fused_attention_dropout=True)
        kw = dict(dropout_seed=SEED, dropout_step=2, skip_layers=NONE)
        assert torch.equal(on(wav, **kw), off(wav, **kw))
        assert on._lib().svt_debug_set(38, 0) not in NEW_IDS


def test_workspace_and_the_old_structure_size():
    """With the flag on and the state set the workspace is the plain forward's; with the flag off it is what it was; a svt_dropout of the
    size it had before fused_attention was appended is accepted and means flag off."""
    _, enc = ED.base_encoder("bf16")
    wav = DC.synth_wav(2, 16000, 53).to(DEV)
    lib = enc._lib()
    with torch.no_grad():
        enc(wav, dropout_seed=SEED)
    h = handle(enc)
    with_state = lib.svt_encoder_workspace_bytes(h, 2, 16000)
    assert lib.svt_encoder_set_dropout(h, None) == 0
    plain = lib.svt_encoder_workspace_bytes(h, 2, 16000)
    assert 350000 < with_state - plain < 400000, with_state - plain      # tests/test_gpu_encoder_dropout.py's figure: flag off is what it was
    st = _lib.DropoutC()
    st.struct_size = ctypes.sizeof(_lib.DropoutC)
    st.attention_dropout = st.hidden_dropout = 0.1
    st.fused_attention = 1
    assert lib.svt_encoder_set_dropout(h, st) == 0
    assert lib.svt_encoder_workspace_bytes(h, 2, 16000) == plain          # no score or probability buffers
    st.fused_attention = 0
    assert lib.svt_encoder_set_dropout(h, st) == 0
    assert lib.svt_encoder_workspace_bytes(h, 2, 16000) == with_state
    old = _lib.DropoutC.fused_attention.offset
    assert old == 64 and ctypes.sizeof(_lib.DropoutC) == 72
    st.fused_attention = 1                                                # bytes past the old size: not read
    st.struct_size = old
    assert lib.svt_encoder_set_dropout(h, st) == 0
    assert lib.svt_encoder_workspace_bytes(h, 2, 16000) == with_state     # the old size means flag off
    for bad in (old - 8, old + 4, ctypes.sizeof(_lib.DropoutC) + 8):
        st.struct_size = bad
        assert lib.svt_encoder_set_dropout(h, st) == -1 and "struct_size" in _lib.last_error(lib)
    assert lib.svt_encoder_set_dropout(h, None) == 0
    enc.fused_attention_dropout = True                                    # the wrapper passes the attribute on
    with torch.no_grad():
        enc(wav, dropout_seed=SEED)
    assert lib.svt_debug_set(38, 0) in NEW_IDS
    assert lib.svt_encoder_workspace_bytes(handle(enc), 2, 16000) == plain


def test_linear_probe_trains_on_a_flagged_encoder():
    cfg, enc = ED.base_encoder("bf16", fused_attention_dropout=True)
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
        assert enc._lib().svt_debug_set(38, 0) in NEW_IDS
        last = dict(enc.last_dropout)
        assert last["step"] == 5 + i and last["seed"] == 123
        with torch.no_grad():
            feats = enc(wav, dropout_seed=last["seed"], dropout_step=last["step"], skip_layers=last["skipped"])
        loss2 = probe2.fit_features(feats, None, anno)
        assert torch.equal(loss, loss2) and probe.last_terms == probe2.last_terms, i
