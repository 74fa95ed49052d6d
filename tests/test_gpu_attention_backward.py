"""GPU tests of the fused attention backward (csrc/attention_bwd.hip) through svt_attention_backward and the torch op around it
(svt_speechbrain_amd/attention.py), in both library builds.  Every case NaN-poisons its gradient buffers and asserts the form
svt_debug_set(46, 0) reports (1 = plain, 2 = masked).

1. The mask of each kernel, read back bit for bit (the trick of tests/test_gpu_attention_dropout.py, done three ways).  With all scores 0,
   P = 1 / T.  G = 5 blocks of 64 per launch: N < 32 carries five bits and the two 16-bit roundings on the way (P~ or dS as an MFMA operand,
   the output) move it by at most 2 * 32 * 2^-9 = 1/8 in bf16; the test asserts |N - round(N)| < 1/4 before it reads a bit.
     * Q = 0 and dO[i, d] = 2^g at d == i % 64 for query block i // 64 = g0 + g: dV[j, d] T / s spells keep[i, j] -- (c)'s mask on P~.
     * Q = 0, O = 0 (delta = 0), dO = V = e_0 (dP = s keep), K[j, d] = 2^g at d == j % 64: dQ[i, d] T / s spells keep[i, j] -- (b)'s mask.
     * K = 0, O = 0, dO = V = e_0, Q[i, d] = 2^g at d == i % 64: dK[j, d] T / s spells keep[i, j] -- (c)'s mask on dP.
   Every shape runs the whole product e0 x p except (2, 499, 2), where each e0 runs two of the four p.
2. Values against fp64 under the derived per-element limits of tests/attention_bwd_limit.py.
3. Gradient rows with a padded stride keep the bytes past D; three gradients in one packed buffer equal three separate ones bit for bit.
4. Two calls give the same bytes; p = 2^-33 (threshold 0: the masked form, nothing dropped, s = 1) equals the plain form bit for bit.
5. fused_attention on the three chunks of a packed leaf: .backward() equals the C-level call bit for bit and fp64 autograd of the eager
   expression (mask injected) under the same limits; FusedSelfAttention in train() and eval().
6. What the kernels do not serve is refused with SVT_ERR_INVALID and writes nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from svt_speechbrain_amd import _lib  # noqa: E402
from svt_speechbrain_amd import attention as ATT  # noqa: E402

import attention_bwd_limit as AB  # noqa: E402
import dropout_cases as DC  # noqa: E402

DEV = "cuda:0"
BUILDS = {"bf16": (None, torch.bfloat16), "f16": ("f16", torch.float16)}
SEED = 0xD1B54A32D192ED03
DH = 64


def backward(lib, q, k, v, o, do, dq, dk, dv, *, scale, p=0.0, seed=0, step=0, layer=0, e0=0, precision=1, head_dim=DH,
             struct_size=None, want_rc=0):
    """One svt_attention_backward on (B, T, H, 64) device tensors (views with a row stride); returns the form key 46 reports."""
    B, T, H, _ = q.shape
    d = _lib.AttentionDescC()
    d.struct_size = C.sizeof(_lib.AttentionDescC) if struct_size is None else struct_size
    d.precision = precision
    d.q, d.k, d.v, d.o, d.d_o = q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr()
    d.dq, d.dk, d.dv = dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    assert k.stride(1) == v.stride(1) and dk.stride(1) == dv.stride(1)
    d.ldq, d.ldkv, d.ldo, d.lddo, d.lddq, d.lddkv = q.stride(1), k.stride(1), o.stride(1), do.stride(1), dq.stride(1), dk.stride(1)
    d.batch, d.t, d.heads, d.head_dim = B, T, H, head_dim
    d.scale, d.p, d.seed, d.step, d.layer, d.e0 = scale, p, seed, step, layer, e0
    stream = torch.cuda.current_stream().cuda_stream
    need = C.c_size_t(0)
    rc = lib.svt_attention_backward(C.byref(d), None, C.byref(need), 0, stream)
    if rc == 0:
        ws = torch.full((max(int(need.value), 16),), 0xFF, device=DEV, dtype=torch.uint8)   # NaN bytes: L and delta must be written
        rc = lib.svt_attention_backward(C.byref(d), ws.data_ptr(), C.byref(need), 0, stream)
        torch.cuda.synchronize()
    assert rc == want_rc, (rc, _lib.last_error(lib))
    return lib.svt_debug_set(46, 0)


def poisoned(B, T, H, dtype, pad=0):
    """A NaN-filled (B, T, H * 64 + pad) buffer and its (B, T, H, 64) view."""
    ld = H * DH + pad
    buf = torch.full((B, T, ld), float("nan"), device=DEV, dtype=dtype)
    return buf, buf.as_strided((B, T, H, DH), (T * ld, ld, DH, 1))


# ---------------------------------------------------------------------------------------------------------------- 1. the masks
G = 5


def onehot_blocks(B, T, H, g0):
    """x[b, i, h, d] = 2^g at d == i % 64 for block i // 64 = g0 + g (g < G), 0 elsewhere."""
    x = torch.zeros(B, T, H, DH)
    i = torch.arange(T)
    blk = i // DH
    sel = (blk >= g0) & (blk < g0 + G)
    x[:, i[sel], :, (i % DH)[sel]] = (2.0 ** (blk[sel] - g0).float())[:, None, None]
    return x


def decode(out, T, s, nb):
    """out (B, T, H, 64) with out[x, d] T / s = sum_g 2^g bit_g[x, d]; returns the bits, (nb, B, H, T, 64) bool."""
    o = out.double().cpu()
    assert torch.isfinite(o).all(), "unwritten (NaN-poisoned) outputs"
    n = o * T / s
    N = n.round()
    assert (n - N).abs().max().item() < 0.25, (n - N).abs().max().item()
    N = N.long().permute(0, 2, 1, 3)      # (B, H, x, d)
    assert not (N >> nb).any() and (N >= 0).all()
    return torch.stack([((N >> g) & 1).bool() for g in range(nb)])


def read_masks(lib, dtype, B, T, H, p, seed, step, layer, e0):
    """{"dv", "dq", "dk"}: keep (B, H, T, T) bool as each kernel applied it."""
    nblk = (T + DH - 1) // DH
    s = float(DC.scale(p))
    kept = {n: torch.zeros(B, H, T, T, dtype=torch.bool) for n in ("dv", "dq", "dk")}
    zero = torch.zeros(B, T, H, DH, device=DEV, dtype=dtype)
    e_0 = torch.zeros(B, T, H, DH)
    e_0[..., 0] = 1.0
    e_0 = e_0.to(dtype).to(DEV)
    kw = dict(scale=1.0, p=p, seed=seed, step=step, layer=layer, e0=e0)
    for g0 in range(0, nblk, G):
        nb = min(G, nblk - g0)
        hot = onehot_blocks(B, T, H, g0).to(dtype).to(DEV)
        for which, (q, k, v, do) in {"dv": (zero, zero, zero, hot), "dq": (zero, hot, e_0, e_0), "dk": (hot, zero, e_0, e_0)}.items():
            bufs = [poisoned(B, T, H, dtype) for _ in range(3)]
            kid = backward(lib, q, k, v, zero, do, bufs[0][1], bufs[1][1], bufs[2][1], **kw)
            assert kid == 2, f"form {kid} ran, the case is written for the masked form"
            out = bufs[("dq", "dk", "dv").index(which)][1]
            bits = decode(out, T, s, nb)
            for g in range(nb):
                lo = (g0 + g) * DH
                w = min(DH, T - lo)
                assert not bits[g][..., w:].any(), "a column past the last row of the block received a value"
                if which == "dq":
                    kept[which][:, :, :, lo:lo + w] = bits[g][..., :w]                       # [b, h, i, d] -> keep[i, lo + d]
                else:
                    kept[which][:, :, lo:lo + w, :] = bits[g][..., :w].transpose(-1, -2)   # [b, h, j, d] -> keep[lo + d, j]
    return {n: t.numpy() for n, t in kept.items()}


MASK_SHAPES = [(3, 1, 2), (2, 64, 2), (2, 65, 3), (1, 129, 2), (2, 499, 2)]
E0S = [0, 1, 2 ** 32 - 2, 2 ** 34 + 1]
PS = [0.1, 0.5, 0.9, 2.0 ** -33]


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("e0", E0S)
@pytest.mark.parametrize("B,T,H", MASK_SHAPES)
def test_masks_are_read_back_bit_for_bit(B, T, H, e0, build):
    variant, dtype = BUILDS[build]
    lib = _lib.load(variant)
    ps = PS if T < 499 else [PS[E0S.index(e0)], PS[(E0S.index(e0) + 1) % 4]]
    for p in ps:
        got = read_masks(lib, dtype, B, T, H, p, SEED, 5, 3, e0)
        want = DC.keep(p, SEED, 5, DC.SITE_ATTN_PROBS, 3, B * H * T * T, e0).reshape(B, H, T, T)
        for which, m in got.items():
            bad = np.argwhere(m != want)
            print(f"mask of {which} [{build}] B={B} T={T} H={H} e0={e0} p={p}: kept {m.mean():.4f}, {len(bad)} bits differ")
            assert len(bad) == 0, (which, build, (B, T, H), e0, p, bad[:8].tolist())
            if p == 2.0 ** -33:
                assert m.all(), "p = 2^-33 has threshold 0: nothing is dropped"


# ---------------------------------------------------------------------------------------------------------------- 2. values
_ref_cache = {}


def _reference(c, dtype):
    key = (c, dtype)
    if key not in _ref_cache:
        x, do = AB.make_inputs(c, dtype)
        _ref_cache[key] = (x, do, AB.reference(c, x, do, dtype))
    return _ref_cache[key]


def _device_case(c, x, do, ref, dtype, pad):
    """q, k, v, o, do views on the device in the case's layout and three poisoned gradient buffers (rows padded by `pad`)."""
    B, T, H = c.B, c.T, c.H
    D = H * DH
    shape = (B, T, H, DH)
    if c.layout == "packed":
        xd = x.to(DEV)
        q, k, v = (xd[..., i * D:(i + 1) * D].unflatten(-1, (H, DH)) for i in range(3))
    else:   # q in its own buffer, k | v packed
        qd, kvd = x[..., :D].contiguous().to(DEV), x[..., D:].contiguous().to(DEV)
        q, k, v = qd.view(shape), kvd[..., :D].unflatten(-1, (H, DH)), kvd[..., D:].unflatten(-1, (H, DH))
    o, g = ref["o"].to(DEV).view(shape), do.to(DEV).view(shape)
    return q, k, v, o, g, [poisoned(B, T, H, dtype, pad) for _ in range(3)]


def _check_values(tag, c, got, ref, build):
    D = c.H * DH
    for name, t in zip(("dq", "dk", "dv"), got):
        t = t.reshape(c.B, c.T, D).cpu()
        assert torch.isfinite(t).all(), f"{name}: unwritten (NaN-poisoned) outputs"
        err = (t.double() - ref[name]).abs()
        ratio = err / ref["lim_" + name]
        worst = ratio.max().item()
        b, t_, col = np.unravel_index(int(ratio.argmax()), ratio.shape)
        print(f"{tag} {name} [{build}] {AB.case_id(c)}: worst err / limit {worst:.3f} at clip {b} row {t_} (block {t_ // 128}, wave "
              f"{t_ % 128 // 32}) head {col // DH} column {col % DH}; max|err| {err.max().item():.3e}")
        assert worst <= 1.0, (tag, name, build, AB.case_id(c), worst, (int(b), int(t_), int(col)))


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("c", AB.VALUE_CASES, ids=AB.case_id)
def test_values_against_fp64(c, build):
    variant, dtype = BUILDS[build]
    lib = _lib.load(variant)
    x, do, ref = _reference(c, dtype)
    pad = 64 if c.layout == "separate" else 0
    q, k, v, o, g, bufs = _device_case(c, x, do, ref, dtype, pad)
    before = [b[0].view(torch.int16).clone() for b in bufs]
    kid = backward(lib, q, k, v, o, g, bufs[0][1], bufs[1][1], bufs[2][1], scale=AB.SCALE, p=c.p, seed=c.seed, step=c.step,
                   layer=c.layer, e0=c.e0)
    assert kid == (2 if c.p > 0 else 1), kid
    D = c.H * DH
    for b, b0 in zip(bufs, before):
        assert torch.equal(b[0].view(torch.int16)[..., D:], b0[..., D:]), "columns past D of a padded gradient row were written"
    _check_values("backward", c, [b[1] for b in bufs], ref, build)


# ---------------------------------------------------------------------------------------------------------------- 3, 4. layouts, determinism
@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_packed_equals_separate_and_two_calls_agree(p, build):
    variant, dtype = BUILDS[build]
    lib = _lib.load(variant)
    c = AB.V(2, 129, 2, p=p, e0=3)
    x, do, ref = _reference(c, dtype)
    q, k, v, o, g, bufs = _device_case(c, x, do, ref, dtype, 0)
    kw = dict(scale=AB.SCALE, p=c.p, seed=c.seed, step=c.step, layer=c.layer, e0=c.e0)
    form = 2 if p > 0 else 1
    assert backward(lib, q, k, v, o, g, bufs[0][1], bufs[1][1], bufs[2][1], **kw) == form
    D = c.H * DH
    for _ in range(2):   # one packed (B, T, 3 D) gradient buffer, twice
        pk = torch.full((c.B, c.T, 3, c.H, DH), float("nan"), device=DEV, dtype=dtype)
        assert backward(lib, q, k, v, o, g, pk[:, :, 0], pk[:, :, 1], pk[:, :, 2], **kw) == form
        for i in range(3):
            assert torch.equal(pk[:, :, i].reshape(c.B, c.T, D).view(torch.int16), bufs[i][0].view(torch.int16)), ("dq", "dk", "dv")[i]


@pytest.mark.parametrize("build", list(BUILDS))
def test_masked_form_that_drops_nothing_equals_the_plain_form(build):
    variant, dtype = BUILDS[build]
    lib = _lib.load(variant)
    c = AB.V(2, 129, 2, p=0.0)
    x, do, ref = _reference(c, dtype)
    q, k, v, o, g, plain = _device_case(c, x, do, ref, dtype, 0)
    assert backward(lib, q, k, v, o, g, plain[0][1], plain[1][1], plain[2][1], scale=AB.SCALE) == 1
    masked = [poisoned(c.B, c.T, c.H, dtype) for _ in range(3)]
    assert backward(lib, q, k, v, o, g, masked[0][1], masked[1][1], masked[2][1], scale=AB.SCALE, p=2.0 ** -33, seed=SEED, step=5,
                    layer=3, e0=7) == 2
    for a, b, name in zip(plain, masked, ("dq", "dk", "dv")):
        assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)), name


# ---------------------------------------------------------------------------------------------------------------- 5. autograd
@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_autograd_op_on_a_packed_leaf(p, build):
    variant, dtype = BUILDS[build]
    lib = _lib.load(variant)
    c = AB.V(2, 129, 2, p=p, e0=3)
    x, do, ref = _reference(c, dtype)
    B, T, H, D = c.B, c.T, c.H, c.H * DH
    leaf = x.to(DEV).requires_grad_(True)                       # (2, 129, 3 * 128)
    q, k, v = (t.unflatten(-1, (H, DH)) for t in leaf.split(D, dim=-1))
    out = ATT.fused_attention(q, k, v, scale=AB.SCALE, dropout_p=c.p, seed=c.seed, step=c.step, layer=c.layer, e0=c.e0)
    assert out.shape == (B, T, H, DH)
    g = do.to(DEV).view(B, T, H, DH)
    out.backward(g)
    assert lib.svt_debug_set(46, 0) == (2 if p > 0 else 1)
    grad = leaf.grad
    assert grad.shape == leaf.shape and torch.isfinite(grad).all()
    # the C-level call on the op's own saved output: bit for bit
    bufs = [poisoned(B, T, H, dtype) for _ in range(3)]
    backward(lib, q.detach(), k.detach(), v.detach(), out.detach(), g, bufs[0][1], bufs[1][1], bufs[2][1], scale=AB.SCALE, p=c.p,
             seed=c.seed, step=c.step, layer=c.layer, e0=c.e0)
    for i, name in enumerate(("dq", "dk", "dv")):
        assert torch.equal(grad[..., i * D:(i + 1) * D].contiguous().view(torch.int16), bufs[i][0].view(torch.int16)), name
    # fp64 autograd of the eager expression HF runs, the mask injected
    xr = x.double().requires_grad_(True)
    qr, kr, vr = (t.unflatten(-1, (H, DH)).permute(0, 2, 1, 3) for t in xr.split(D, dim=-1))
    keep = torch.from_numpy(AB.keep_mask(c)).double()
    s = float(DC.scale(c.p)) if c.p > 0 else 1.0
    probs = torch.softmax(qr @ kr.transpose(-1, -2) * AB.SCALE, -1) * keep * s
    (probs @ vr).permute(0, 2, 1, 3).backward(do.double().view(B, T, H, DH))
    auto = {n: xr.grad[..., i * D:(i + 1) * D] for i, n in enumerate(("dq", "dk", "dv"))}
    for n in auto:
        assert (auto[n] - ref[n]).abs().max().item() <= 1e-9 * (1 + ref[n].abs().max().item()), n   # the reference IS that autograd
    _check_values("autograd", c, [grad[..., i * D:(i + 1) * D].detach() for i in range(3)], ref, build)


@pytest.mark.parametrize("build", list(BUILDS))
def test_module_train_and_eval_steps(build):
    variant, dtype = BUILDS[build]
    lib = _lib.load(variant)
    torch.manual_seed(3)
    mod = ATT.FusedSelfAttention(128, 2, dropout=0.1).to(DEV).to(dtype)
    x = torch.randn(2, 65, 128, device=DEV, dtype=dtype)
    mod.train()
    out, w, pkv = mod(x)
    assert w is None and pkv is None and out.shape == x.shape and mod.dropout_step == 1
    out.float().square().mean().backward()
    assert lib.svt_debug_set(46, 0) == 2
    for name, prm in mod.named_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all() and prm.grad.abs().max() > 0, name
    mod.zero_grad()
    mod.eval()
    out_e, _, _ = mod(x)
    assert mod.dropout_step == 1, "eval() draws no mask and leaves the counter alone"
    out_e.float().square().mean().backward()
    assert lib.svt_debug_set(46, 0) == 1
    # eval: the plain attention, against eager torch in fp32 on the same 16-bit projections
    with torch.no_grad():
        q, k, v = (p_(x).view(2, 65, 2, DH).permute(0, 2, 1, 3).float() for p_ in (mod.q_proj, mod.k_proj, mod.v_proj))
        eager = (torch.softmax(q @ k.transpose(-1, -2) * DH ** -0.5, -1) @ v).permute(0, 2, 1, 3).reshape(2, 65, 128)
        want = mod.out_proj(eager.to(dtype))
    assert (out_e.float() - want.float()).abs().max().item() <= 8 * AB.U[dtype] * (1 + want.float().abs().max().item())
    with pytest.raises(_lib.SvtError):
        mod(x, attention_mask=torch.ones(2, 1, 65, 65, device=DEV))


# ---------------------------------------------------------------------------------------------------------------- 6. refusals
@pytest.mark.parametrize("build", list(BUILDS))
def test_refusals_write_nothing(build):
    variant, dtype = BUILDS[build]
    lib = _lib.load(variant)
    B, T, H = 1, 8, 2
    z = torch.zeros(B, T, H, DH, device=DEV, dtype=dtype)
    bufs = [poisoned(B, T, H, dtype) for _ in range(3)]
    before = [b[0].view(torch.int16).clone() for b in bufs]

    def call(want_rc=-1, **kw):
        return backward(lib, z, z, z, z, z, bufs[0][1], bufs[1][1], bufs[2][1], **dict(dict(scale=0.125, p=0.1, seed=1), **kw), want_rc=want_rc)

    call(head_dim=48)
    assert b"head_dim" in lib.svt_last_error()
    call(head_dim=128)
    assert b"head_dim" in lib.svt_last_error()
    call(precision=0)
    assert b"precision" in lib.svt_last_error()
    call(p=1.0)
    assert b"[0, 1)" in lib.svt_last_error()
    call(struct_size=C.sizeof(_lib.AttentionDescC) - 8)
    assert b"struct_size" in lib.svt_last_error()
    torch.cuda.synchronize()
    for b, b0 in zip(bufs, before):
        assert torch.equal(b[0].view(torch.int16), b0), "a refused call wrote to a gradient"
    assert call(want_rc=0) == 2
    for b in bufs:
        assert torch.isfinite(b[0]).all()
    # the op refuses before any library call what the kernels do not serve
    with pytest.raises(_lib.SvtError):
        ATT.fused_attention(z.float(), z.float(), z.float())
