"""GPU unit tests of the fused attention with the dropout mask inside (csrc/attention_drop.hip) through svt_debug_attention_dropout, in
both library builds.  Every case NaN-poisons its output and asserts the kernel id svt_debug_set(38, 0) reports.

1. The mask, read back bit for bit.  With Q = 0 every unnormalised probability is exactly 1 and the row sum is T.  V is laid out so
   that the output spells the mask: V[b, j, h, d] = 2^((j // dh) mod G) where d == j % dh and key block j // dh lies in the current
   group of G blocks, 0 elsewhere.  Then N = O T / s (s = float32(1 / (1 - p))) is an integer whose bit g says whether element
   (b, h, i, j = dh (G group + g) + d) was kept; G <= 6 keeps the decode exact in bf16 (N < 64 carries six bits, the output's rounding
   moves N by at most 64 * 2^-9 = 1/8), and the test asserts |O T / s - N| < 1/4 before it reads a bit.  One launch per group covers all
   key blocks.  Every bit is compared with tests/dropout_cases.py's keep().  Every shape runs the whole product e0 x p except
   (2, 499, 2), where each e0 runs two of the four p (the product there is partial, for run time; every p is still reached).
2. Values against fp64 under the per-element limit of tests/attention_drop_limit.py (derived there; tests/test_attention_drop_limit.py
   shows on the CPU that a model of the kernel passes it and that each of nine mutants breaks it at every case).
3. The cases reach every kernel id the header lists for this family, and the hook refuses what the kernel does not serve."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from svt_speechbrain_amd import _lib  # noqa: E402

import attention_drop_limit as AD  # noqa: E402
import dropout_cases as DC  # noqa: E402

DEV = "cuda:0"
BUILDS = {"bf16": (None, torch.bfloat16), "f16": ("f16", torch.float16)}
# kernel ids (include/svt_mi355.h, svt_debug_set key 38): 9 flash_attn_drop_kernel<64, 4>, 10 flash_attn_drop_kernel<128, 4>
KID = {64: 9, 128: 10}
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "svt_mi355.h")


def header_family_ids():
    """{id: (head_dim, waves)} of every `N = flash_attn_drop_kernel<DH, NW>` the header's key-38 paragraph assigns."""
    with open(HEADER) as fh:
        text = re.sub(r"\s*\n \*\s*", " ", fh.read())
    return {int(m.group(1)): (int(m.group(2)), int(m.group(3))) for m in re.finditer(r"(\d+) = flash_attn_drop_kernel<(\d+), (\d+)>", text)}


SEED = 0xD1B54A32D192ED03


def launch(lib, q, k, v, out, B, T, H, dh, ldq, ldkv, ldo, p, seed, step, layer, e0, scale, precision=1, struct_size=None):
    """One call of the hook on device pointers; returns (rc, kernel id reported afterwards)."""
    d = _lib.AttentionDropoutDescC()
    d.struct_size = C.sizeof(_lib.AttentionDropoutDescC) if struct_size is None else struct_size
    d.precision = precision
    d.q, d.k, d.v, d.o = q, k, v, out
    d.ldq, d.ldkv, d.ldo = ldq, ldkv, ldo
    d.batch, d.t, d.heads, d.head_dim = B, T, H, dh
    d.scale, d.step, d.p, d.seed, d.layer, d.e0 = scale, step, p, seed, layer, e0
    rc = lib.svt_debug_attention_dropout(C.byref(d), 0, torch.cuda.current_stream().cuda_stream)
    return rc, lib.svt_debug_set(38, 0)


# ---------------------------------------------------------------------------------------------------------------- 1. the mask
def read_mask(lib, dtype, B, T, H, dh, p, seed, step, layer, e0, G=6):
    """keep (B, H, T, T) bool as the kernel applied it, decoded from the outputs of ceil(blocks / G) launches."""
    D = H * dh
    nblk = (T + dh - 1) // dh
    s = float(DC.scale(p))
    j = torch.arange(T)
    kept = torch.zeros(B, H, T, T, dtype=torch.bool)
    for g0 in range(0, nblk, G):
        x = torch.zeros(B, T, 3 * D, dtype=torch.float32)
        x[..., D:2 * D] = 1.0                                   # K: anything finite (Q = 0 makes every score 0)
        v = x[..., 2 * D:].view(B, T, H, dh)
        blk = j // dh
        sel = (blk >= g0) & (blk < g0 + G)
        v[:, j[sel], :, (j % dh)[sel]] = (2.0 ** (blk[sel] - g0).float())[:, None, None]   # indexed dims first: (keys, B, H)
        xd = x.to(dtype).to(DEV)
        out = torch.full((B, T, D), float("nan"), device=DEV, dtype=dtype)
        es = xd.element_size()
        rc, kid = launch(lib, xd.data_ptr(), xd.data_ptr() + es * D, xd.data_ptr() + 2 * es * D, out.data_ptr(), B, T, H, dh,
                         3 * D, 3 * D, D, p, seed, step, layer, e0, 1.0)
        _lib.check(rc, "svt_debug_attention_dropout", lib)
        assert kid == KID[dh], f"kernel {kid} ran, the case is written for kernel {KID[dh]}"
        torch.cuda.synchronize()
        o = out.double().cpu()
        assert torch.isfinite(o).all(), "unwritten (NaN-poisoned) outputs"
        n = o * T / s
        N = n.round()
        assert (n - N).abs().max().item() < 0.25, (n - N).abs().max().item()
        N = N.long().view(B, T, H, dh).permute(0, 2, 1, 3)      # (B, H, i, d)
        for g in range(min(G, nblk - g0)):
            lo = (g0 + g) * dh
            w = min(dh, T - lo)
            kept[:, :, :, lo:lo + w] = ((N[..., :w] >> g) & 1).bool()
            assert not ((N[..., w:] >> g) & 1).any(), "a column past the last key received a value"
        assert not (N >> min(G, nblk - g0)).any()
    return kept.numpy()


MASK_SHAPES = [(3, 1, 2, 64), (2, 64, 2, 64), (2, 65, 3, 64), (1, 129, 2, 64), (2, 499, 2, 64), (2, 65, 2, 128), (1, 130, 2, 128)]
E0S = [0, 1, 2 ** 32 - 2, 2 ** 34 + 1]
PS = [0.1, 0.5, 0.9, 2.0 ** -33]


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("e0", E0S)
@pytest.mark.parametrize("B,T,H,dh", MASK_SHAPES)
def test_mask_is_read_back_bit_for_bit(B, T, H, dh, e0, build):
    variant, dtype = BUILDS[build]
    lib = _lib.load(variant)
    # the long shape runs the full product over two parameters in turn, the short ones all of it
    ps = PS if T < 499 else [PS[E0S.index(e0)], PS[(E0S.index(e0) + 1) % 4]]
    for p in ps:
        got = read_mask(lib, dtype, B, T, H, dh, p, SEED, 5, 3, e0)
        want = DC.keep(p, SEED, 5, DC.SITE_ATTN_PROBS, 3, B * H * T * T, e0).reshape(B, H, T, T)
        bad = np.argwhere(got != want)
        print(f"mask [{build}] B={B} T={T} H={H} dh={dh} e0={e0} p={p}: kept {got.mean():.4f}, {len(bad)} bits differ")
        assert len(bad) == 0, (build, (B, T, H, dh), e0, p, bad[:8].tolist())
        if p == 2.0 ** -33:
            assert got.all(), "p = 2^-33 has threshold 0: nothing is dropped"


@pytest.mark.parametrize("build", list(BUILDS))
def test_layer_step_and_seed_change_the_mask(build):
    variant, dtype = BUILDS[build]
    lib = _lib.load(variant)
    B, T, H, dh, p = 1, 129, 2, 64, 0.5
    base = read_mask(lib, dtype, B, T, H, dh, p, SEED, 5, 3, 0)
    for what, (seed, step, layer) in {"layer": (SEED, 5, 4), "step": (SEED, 6, 3), "seed": (SEED + 1, 5, 3),
                                       "seed_hi": (SEED ^ (1 << 40), 5, 3)}.items():
        other = read_mask(lib, dtype, B, T, H, dh, p, seed, step, layer, 0)
        want = DC.keep(p, seed, step, DC.SITE_ATTN_PROBS, layer, B * H * T * T, 0).reshape(B, H, T, T)
        assert np.array_equal(other, want), what
        differ = (other != base).mean()
        print(f"mask [{build}] another {what}: {differ:.3f} of the bits differ")
        assert 0.4 < differ < 0.6, (what, differ)


# ---------------------------------------------------------------------------------------------------------------- 2. values
_ref_cache = {}


def _reference(c, dtype):
    key = (c, dtype)
    if key not in _ref_cache:
        x = AD.make_inputs(c, dtype)
        ref, A = AD.reference(c, x, AD.keep_mask(c))
        _ref_cache[key] = (x, ref, AD.limit(c, x, ref, A, dtype))
    return _ref_cache[key]


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("c", AD.VALUE_CASES, ids=AD.case_id)
def test_values_against_fp64(c, build):
    """|got - ref| <= u (A + |ref|) + s T 2^-24 max|v| on every element (tests/attention_drop_limit.py)."""
    variant, dtype = BUILDS[build]
    lib = _lib.load(variant)
    x, ref, lim = _reference(c, dtype)
    B, T, H, dh = c.B, c.T, c.H, c.dh
    D, es = H * dh, x.element_size()
    if c.layout == "packed":
        xd = x.to(DEV)
        qp, kp, vp, ldq, ldkv, ldo = xd.data_ptr(), xd.data_ptr() + es * D, xd.data_ptr() + 2 * es * D, 3 * D, 3 * D, D
    else:   # q in its own buffer, k | v packed, output rows padded by 64 columns: the RCA layers' call
        qd, kvd = x[..., :D].contiguous().to(DEV), x[..., D:].contiguous().to(DEV)
        qp, kp, vp, ldq, ldkv, ldo = qd.data_ptr(), kvd.data_ptr(), kvd.data_ptr() + es * D, D, 2 * D, D + 64
    out = torch.full((B, T, ldo), float("nan"), device=DEV, dtype=dtype)
    before = out.view(torch.int16).clone()
    rc, kid = launch(lib, qp, kp, vp, out.data_ptr(), B, T, H, dh, ldq, ldkv, ldo, c.p, c.seed, c.step, c.layer, c.e0, AD.scale_of(dh))
    _lib.check(rc, "svt_debug_attention_dropout", lib)
    assert kid == KID[dh], f"kernel {kid} ran, the case is written for kernel {KID[dh]}"
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16)[..., D:], before[..., D:]), "columns past D of a padded output row were written"
    got = out[..., :D].cpu()
    assert torch.isfinite(got).all(), "unwritten (NaN-poisoned) outputs"
    err = (got.double() - ref).abs()
    ratio = err / lim
    worst = ratio.max().item()
    b, t, col = np.unravel_index(int(ratio.argmax()), ratio.shape)
    print(f"masked attention [{build}] {AD.case_id(c)}: worst err / limit {worst:.3f} at clip {b} query {t} (block {t // 128}, wave "
          f"{t % 128 // 32}) head {col // dh} column {col % dh}; max|err| {err.max().item():.3e}")
    assert worst <= 1.0, (build, AD.case_id(c), worst, (int(b), int(t), int(col)))


# ---------------------------------------------------------------------------------------------------------------- 3. coverage, refusals
def test_cases_cover_every_kernel_of_the_family():
    ids = header_family_ids()
    assert ids, "the header lists no flash_attn_drop_kernel id under svt_debug_set key 38"
    assert {k: dh for k, (dh, _) in ids.items()} == {v: k for k, v in KID.items()}, ids     # the header's ids are the ones the cases assert
    assert {KID[s[3]] for s in MASK_SHAPES} == set(ids)
    assert {KID[c.dh] for c in AD.VALUE_CASES} == set(ids)
    assert any(c.gain == 8.0 for c in AD.VALUE_CASES) and any(c.layout == "separate" for c in AD.VALUE_CASES)


@pytest.mark.parametrize("build", list(BUILDS))
def test_refusals_launch_nothing(build):
    variant, dtype = BUILDS[build]
    lib = _lib.load(variant)
    x = torch.zeros(1, 8, 3 * 128, device=DEV, dtype=dtype)
    out = torch.full((1, 8, 128), float("nan"), device=DEV, dtype=dtype)
    before = out.view(torch.int16).clone()
    good = dict(B=1, T=8, H=2, dh=64, ldq=384, ldkv=384, ldo=128, p=0.1, seed=1, step=0, layer=0, e0=0, scale=0.125)

    def call(**kw):
        a = dict(good, **kw)
        return launch(lib, x.data_ptr(), x.data_ptr() + 256, x.data_ptr() + 512, out.data_ptr(), **a)[0]

    assert call(dh=48, ldq=288, ldkv=288, ldo=96) == -1 and b"head_dim" in lib.svt_last_error()
    assert call(precision=0) == -1 and b"precision" in lib.svt_last_error()
    assert call(p=1.0) == -1 and b"[0, 1)" in lib.svt_last_error()
    assert call(p=1.5) == -1
    assert call(struct_size=C.sizeof(_lib.AttentionDropoutDescC) - 8) == -1 and b"struct_size" in lib.svt_last_error()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), before), "a refused call wrote to the output"
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
