"""GPU unit tests of the fused attention kernels through the C-ABI test hooks (svt_debug_attention, svt_debug_attention_bias).

Two layers.  The first (test_attention_vs_torch ... test_split_operand_attention_vs_torch) compares with a torch softmax(q k^T) v on the
same inputs under flat bounds: the encoder shapes (T = 499 / 249, head_dim 64), the RCA shape (head_dim 128) and the edge lengths around
the 64-key / 128-query tiles (1, 63, 64, 65, 127, 128, 129).  None of its launches is "wide", so it only ever runs kernels 1, 2, 6, 7.

The second (CASES_16 / CASES_BIAS / CASES_SPLIT below) runs EVERY kernel the launchers can choose, at the launch sizes that choose it:
each case names the kernel id it expects and asserts that svt_debug_set(38, 0) reports it after the launch, so a moved threshold fails a
case instead of silently moving it to another kernel, and test_case_tables_cover_every_kernel requires the tables to reach ids 1..8.
The reference is fp64 on the CPU from the same rounded inputs, every output element is compared, the output is NaN-poisoned first.

Limit of the 16-bit kernels, per element, from the number formats (u = 2^-8 for bf16, 2^-11 for IEEE half; the kernels round P to the
operand type before P V and the output once; scores, row sums and accumulators are fp32):

    |got - ref| <= u (A + |ref|) + T 2^-24 max|v|,      A = softmax(...) |v|

(P rounding <= u A, output rounding <= u |ref|, fp32 accumulation over T keys in any order).  No factor on top.  The test prints the
worst ratio err / limit of every case and where it sits (clip, query, head, column; query block and wave of the 256-query workgroup)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from svt_speechbrain_amd import _lib  # noqa: E402

DEV = "cuda:0"


def run_attention(B, T, H, dh, seed=0, gain=1.5):
    lib = _lib.load()
    D = H * dh
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(B, T, 3 * D, generator=g) * gain).to(DEV, torch.bfloat16)
    out = torch.full((B, T, D), float("nan"), device=DEV, dtype=torch.bfloat16)
    scale = dh ** -0.5
    _lib.check(lib.svt_debug_attention(1, qkv.data_ptr(), qkv.data_ptr() + 2 * D, qkv.data_ptr() + 4 * D, out.data_ptr(),
                                       B, T, H, dh, 3 * D, 3 * D, D, scale, 0, torch.cuda.current_stream().cuda_stream),
               "svt_debug_attention")
    torch.cuda.synchronize()
    q, k, v = [x.float().cpu().view(B, T, H, dh).transpose(1, 2) for x in qkv.split(D, dim=-1)]
    ref = (torch.softmax(q @ k.transpose(-1, -2) * scale, -1) @ v).transpose(1, 2).reshape(B, T, D)
    return out.float().cpu(), ref


@pytest.mark.parametrize("B,T,H,dh", [(2, 499, 12, 64), (1, 249, 12, 64), (2, 499, 16, 64), (2, 499, 8, 128), (1, 500, 8, 128),
                                      (3, 1, 2, 64), (2, 63, 2, 64), (2, 64, 2, 64), (2, 65, 3, 64), (1, 127, 2, 64),
                                      (1, 128, 2, 128), (1, 129, 2, 64), (1, 1000, 2, 64)])
def test_attention_vs_torch(B, T, H, dh):
    got, ref = run_attention(B, T, H, dh)
    assert torch.isfinite(got).all(), "unwritten (NaN-poisoned) outputs"
    err = (got - ref).abs().max().item()
    # P and the output are rounded to bf16 (2^-9 relative); |o| <= max|v| ~ 6
    assert err < 4e-2, (B, T, H, dh, err)
    assert (got - ref).abs().mean().item() < 2e-3


def test_attention_peaked_rows_do_not_overflow():
    # one dominant key per row (scores ~ +-60 after scaling): exercises the deferred-rescale path of the running max
    got, ref = run_attention(1, 499, 4, 64, seed=5, gain=8.0)
    assert torch.isfinite(got).all()
    assert (got - ref).abs().max().item() < 0.25  # |v| ~ 30 here; bf16 output rounding alone is 0.12


def test_attention_rejects_other_head_dims():
    lib = _lib.load()
    x = torch.zeros(1, 8, 3 * 96, device=DEV, dtype=torch.bfloat16)
    o = torch.zeros(1, 8, 96, device=DEV, dtype=torch.bfloat16)
    rc = lib.svt_debug_attention(1, x.data_ptr(), x.data_ptr(), x.data_ptr(), o.data_ptr(), 1, 8, 2, 48, 288, 288, 96, 1.0, 0, None)
    assert rc != 0 and b"head_dim" in lib.svt_last_error()


@pytest.mark.parametrize("prec,tol", [(3, 2e-5), (2, 4e-4)])
@pytest.mark.parametrize("B,T,H,dh", [(2, 499, 12, 64), (1, 249, 3, 64), (2, 499, 8, 128), (2, 65, 2, 64), (1, 1, 2, 64), (3, 130, 2, 128)])
def test_split_operand_attention_vs_torch(prec, tol, B, T, H, dh):
    """The fused attention of the split-operand modes (fp32 q|k|v cut into 16-bit (hi, lo) planes, three MFMAs per product,
    fp32 output) against fp64 softmax(q k^T) v on the same fp32 inputs: fp16 pieces to ~1e-6, bf16 pieces to ~1e-4."""
    lib = _lib.load()
    D = H * dh
    g = torch.Generator().manual_seed(B * 1000 + T)
    qkv = (torch.randn(B, T, 3 * D, generator=g) * 1.5).to(DEV)
    out = torch.full((B, T, D), float("nan"), device=DEV)
    scale = dh ** -0.5
    _lib.check(lib.svt_debug_attention(prec, qkv.data_ptr(), qkv.data_ptr() + 4 * D, qkv.data_ptr() + 8 * D, out.data_ptr(), B, T, H, dh,
                                       3 * D, 3 * D, D, scale, 0, torch.cuda.current_stream().cuda_stream), "svt_debug_attention")
    torch.cuda.synchronize()
    q, k, v = [x.double().cpu().view(B, T, H, dh).transpose(1, 2) for x in qkv.split(D, dim=-1)]
    ref = (torch.softmax(q @ k.transpose(-1, -2) * scale, -1) @ v).transpose(1, 2).reshape(B, T, D).float()
    got = out.cpu()
    assert torch.isfinite(got).all()
    err = (got - ref).abs().max().item()
    print(f"split attention prec={prec} B={B} T={T} H={H} dh={dh}: max|err| {err:.3e}")
    assert err < tol, err


# ---------------------------------------------------------------------------------------------------------------------
# Every kernel at the launch sizes that select it.  Kernel ids (include/svt_mi355.h, svt_debug_set key 38):
#   1 flash_attn_kernel<64>   2 flash_attn_kernel<128>   3 flash_attn_stag_kernel<64>   4 flash_attn_kernel<64, true>
#   5 flash_attn_kernel<64, true, 8>   6 flash_attn_x3_kernel<64, .>   7 flash_attn_x3_kernel<128, .>   8 flash_attn_x3_stag_kernel<.>
import collections  # noqa: E402

import numpy as np  # noqa: E402

BUILDS = {"bf16": (None, torch.bfloat16, 2.0 ** -8), "f16": ("f16", torch.float16, 2.0 ** -11)}

Case = collections.namedtuple("Case", "kid B T H dh gain layout")


def C(kid, B, T, H, dh=64, gain=1.5, layout="packed"):
    return Case(kid, B, T, H, dh, gain, layout)


def _id(c):
    return f"k{c.kid}-B{c.B}-T{c.T}-H{c.H}-dh{c.dh}-g{c.gain}" + ("" if c.layout == "packed" else "-" + c.layout)


# A launch is "wide" (256-query workgroups) when B H ceil(T / 256) reaches a threshold the tests do NOT restate: the shapes below
# sit on both sides of the present one (512) at equal T and the reported kernel id decides.  nqb = ceil(T / 256) query blocks:
# nqb = 1: T = 129 .. 256 (waves 4-7, the late group of the staggered schedule, own one query at T = 129), 2: 257 .. 512 (T = 257: the
# last query block holds one query), 3: 513, 700, 4: 999.  B H = 516, 258, 172, 129 are no multiples of 8 (the remainder branch of the
# staggered kernels' block map: 4, 2, 4 heads and 1 head), 512, 256, 176 are.  T % 64 != 0 everywhere but 192, 256, 320, 512.
WIDE_SHAPES = [(43, 129, 12), (43, 192, 12), (43, 249, 12), (43, 255, 12), (32, 256, 16),
               (43, 257, 6), (43, 320, 6), (43, 499, 6), (16, 512, 16),
               (22, 513, 8), (43, 700, 4),
               (43, 999, 3)]
# the same T with B H nqb = 504
NARROW_SHAPES = [(42, 129, 12), (42, 192, 12), (42, 249, 12), (42, 255, 12), (42, 256, 12),
                 (21, 257, 12), (21, 320, 12), (21, 499, 12), (21, 512, 12),
                 (14, 513, 12), (14, 700, 12),
                 (21, 999, 6)]

CASES_16 = ([C(3, *s) for s in WIDE_SHAPES] + [C(1, *s) for s in NARROW_SHAPES] +
            [C(3, 43, 499, 6, gain=8.0),                       # peaked rows: the deferred rescale in the staggered schedule
             C(2, 2, 499, 8, dh=128), C(2, 43, 129, 12, dh=128),   # head_dim 128 is never wide
             # q in its own buffer (ldq = D), k|v packed (ldkv = 2 D), output rows padded by 64 columns (ldo = D + 64): the RCA layers' call
             C(3, 43, 499, 6, layout="separate"), C(3, 43, 129, 12, layout="separate"), C(1, 2, 499, 12, layout="separate"),
             C(2, 2, 499, 8, dh=128, layout="separate")])
CASES_BIAS = ([C(4, 3, 1, 2), C(4, 2, 65, 3), C(4, 2, 249, 12), C(4, 2, 499, 12), C(4, 42, 249, 12), C(4, 21, 499, 12)] +
              [C(5, 43, 249, 12), C(5, 32, 257, 8), C(5, 43, 499, 6), C(5, 43, 499, 6, gain=8.0)])
CASES_SPLIT = ([C(8, *s) for s in WIDE_SHAPES] + [C(6, *s) for s in NARROW_SHAPES] +
               [C(8, 43, 499, 6, gain=8.0), C(7, 2, 499, 8, dh=128), C(7, 43, 129, 12, dh=128)])


def _scale(dh):
    return float(np.float32(dh ** -0.5))   # what the C ABI's float argument holds


def reference(q, k, v, scale, gate=None, pb=None):
    """fp64 softmax(scale q k^T [+ gate pb]) v and A = softmax(...) |v| for q, k, v (B, T, H, dh); one clip at a time, so the
    (H, T, T) scores of a clip are the largest tensor.  Returns (o, A) as (B, T, H * dh) float64."""
    B, T, H, dh = q.shape
    o = torch.empty(B, T, H * dh, dtype=torch.float64)
    A = torch.empty(B, T, H * dh, dtype=torch.float64)
    rel = None
    if pb is not None:
        idx = torch.arange(T)[None, :] - torch.arange(T)[:, None] + (T - 1)   # [query, key]
        rel = pb.double()[:, idx]                                                  # (H, T, T)
    for b in range(B):
        qb, kb, vb = (x[b].double().transpose(0, 1) for x in (q, k, v))           # (H, T, dh)
        s = torch.bmm(qb, kb.transpose(1, 2)).mul_(scale)
        if rel is not None:
            s.addcmul_(gate[b].double()[:, :, None], rel)
        p = torch.softmax(s, -1)
        both = torch.bmm(p, torch.cat([vb, vb.abs()], -1))                         # (H, T, 2 dh)
        o[b] = both[..., :dh].transpose(0, 1).reshape(T, H * dh)
        A[b] = both[..., dh:].transpose(0, 1).reshape(T, H * dh)
    return o, A


_ref_cache = collections.OrderedDict()   # test speed only: neighbouring cases share inputs (two split precisions, key 8 on / off)


def make_case(c, dtype, bias=False):
    """The rounded inputs of a case (CPU, `dtype`) and their fp64 reference: (x (B, T, 3 D), gate, pb, o, A)."""
    key = (c.B, c.T, c.H, c.dh, c.gain, dtype, bias)
    if key not in _ref_cache:
        D = c.H * c.dh
        g = torch.Generator().manual_seed(c.B * 100003 + c.T * 101 + c.H)
        x = (torch.randn(c.B, c.T, 3 * D, generator=g) * c.gain).to(dtype)
        gate = pb = None
        if bias:
            gate = torch.rand(c.B, c.H, c.T, generator=g) * 1.98 + 0.01   # in (0, 2)
            pb = torch.randn(c.H, 2 * c.T - 1, generator=g)
        q, k, v = (t.reshape(c.B, c.T, c.H, c.dh) for t in x.split(D, dim=-1))
        o, A = reference(q, k, v, _scale(c.dh), gate, pb)
        _ref_cache[key] = (x, gate, pb, o, A)
        while len(_ref_cache) > 2:
            _ref_cache.popitem(last=False)
    return _ref_cache[key]


def launch_16(lib, c, x, gate=None, pb=None):
    """Run the 16-bit hook on inputs x (B, T, 3 D) in the build's operand type; returns (out (B, T, D) on the CPU, kernel id)."""
    B, T, H, dh = c.B, c.T, c.H, c.dh
    D, es = H * dh, x.element_size()
    st = torch.cuda.current_stream().cuda_stream
    if c.layout == "packed":
        xd = x.to(DEV)
        qp, kp, vp, ldq, ldkv, ldo = xd.data_ptr(), xd.data_ptr() + es * D, xd.data_ptr() + 2 * es * D, 3 * D, 3 * D, D
    else:
        qd, kvd = x[..., :D].contiguous().to(DEV), x[..., D:].contiguous().to(DEV)
        qp, kp, vp, ldq, ldkv, ldo = qd.data_ptr(), kvd.data_ptr(), kvd.data_ptr() + es * D, D, 2 * D, D + 64
    out = torch.full((B, T, ldo), float("nan"), device=DEV, dtype=x.dtype)
    before = out.view(torch.int16).clone()
    if gate is None:
        rc = lib.svt_debug_attention(1, qp, kp, vp, out.data_ptr(), B, T, H, dh, ldq, ldkv, ldo, _scale(dh), 0, st)
    else:
        gd, pd = gate.to(DEV), pb.to(DEV)
        rc = lib.svt_debug_attention_bias(qp, kp, vp, out.data_ptr(), B, T, H, ldq, ldkv, ldo, _scale(dh), gd.data_ptr(), pd.data_ptr(), 0, st)
    _lib.check(rc, "svt_debug_attention", lib)
    kid = lib.svt_debug_set(38, 0)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16)[..., D:], before[..., D:]), "columns past D of a padded output row were written"
    return out[..., :D].cpu(), kid


def check_16(c, build, got, o, A, x, what):
    """|got - ref| <= u (A + |ref|) + T 2^-24 max|v| on every element (module docstring)."""
    u = BUILDS[build][2]
    D = c.H * c.dh
    assert torch.isfinite(got).all(), "unwritten (NaN-poisoned) outputs"
    vmax = x[..., 2 * D:].double().abs().max().item()
    err = (got.double() - o).abs()
    ratio = err / (u * (A + o.abs()) + c.T * 2.0 ** -24 * vmax)
    worst = ratio.max().item()
    b, t, col = np.unravel_index(int(ratio.argmax()), ratio.shape)
    print(f"{what} [{build}] {_id(c)}: worst err / limit {worst:.3f} at clip {b} query {t} (block {t // 256}, wave {t % 256 // 32}) "
          f"head {col // c.dh} column {col % c.dh}; max|err| {err.max().item():.3e}")
    assert worst <= 1.0, (what, build, _id(c), worst, (int(b), int(t), int(col)))


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("c", CASES_16, ids=_id)
def test_16bit_kernel_at_its_launch_sizes(c, build):
    variant, dtype, _ = BUILDS[build]
    lib = _lib.load(variant)
    x, _, _, o, A = make_case(c, dtype)
    got, kid = launch_16(lib, c, x)
    assert kid == c.kid, f"kernel {kid} ran, the case is written for kernel {c.kid}"
    check_16(c, build, got, o, A, x, "attention")


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("c", [C(1, 43, 499, 6), C(1, 43, 129, 12)], ids=_id)
def test_four_wave_kernel_at_a_wide_shape(c, build):
    """svt_debug_set key 8 = 0 sends a wide launch to the four-wave kernel: same limit."""
    variant, dtype, _ = BUILDS[build]
    lib = _lib.load(variant)
    x, _, _, o, A = make_case(c, dtype)
    try:
        _lib.check(lib.svt_debug_set(8, 0), "svt_debug_set", lib)
        got, kid = launch_16(lib, c, x)
    finally:
        lib.svt_debug_set(8, 1)
    assert kid == 1
    check_16(c, build, got, o, A, x, "attention, key 8 = 0")


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("c", CASES_BIAS, ids=_id)
def test_position_bias_kernel_at_its_launch_sizes(c, build):
    """score = scale q.k + gate[b, h, q] pos_bias[h, key - q + T - 1] (WavLM), gate in (0, 2), pos_bias ~ N(0, 1)."""
    variant, dtype, _ = BUILDS[build]
    lib = _lib.load(variant)
    x, gate, pb, o, A = make_case(c, dtype, bias=True)
    got, kid = launch_16(lib, c, x, gate, pb)
    assert kid == c.kid, f"kernel {kid} ran, the case is written for kernel {c.kid}"
    check_16(c, build, got, o, A, x, "position-bias attention")


@pytest.mark.parametrize("build", list(BUILDS))
def test_position_bias_refuses_a_row_longer_than_lds(build):
    """2 T - 1 = 8193 bias values do not fit the 32 KiB row: the launcher's error, nothing launched, the output untouched."""
    variant, dtype, _ = BUILDS[build]
    lib = _lib.load(variant)
    T = 4097
    x = torch.zeros(1, T, 192, device=DEV, dtype=dtype)
    out = torch.full((1, T, 64), float("nan"), device=DEV, dtype=dtype)
    before = out.view(torch.int16).clone()
    gate = torch.ones(1, 1, T, device=DEV)
    pb = torch.zeros(1, 2 * T - 1, device=DEV)
    rc = lib.svt_debug_attention_bias(x.data_ptr(), x.data_ptr() + 128, x.data_ptr() + 256, out.data_ptr(), 1, T, 1, 192, 192, 64, 0.125,
                                      gate.data_ptr(), pb.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
    assert rc == -1 and b"sequence too long" in lib.svt_last_error(), (rc, lib.svt_last_error())   # SVT_ERR_INVALID
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), before)


# max|got - ref| of the split-operand kernels against fp64: the figures of test_split_operand_attention_vs_torch at gain 1.5.  At gain g
# the operands' cut errors move the scores by an amount proportional to |q| |k| ~ g^2 and the output answers with the spread of v ~ g
# (P and V cut errors are relative to an output ~ g), so the gain-8 case is held to (8 / 1.5)^3 times the same figures.
SPLIT_TOL = {3: 2e-5, 2: 4e-4}


@pytest.mark.parametrize("c,prec", [(c, prec) for c in CASES_SPLIT for prec in (3, 2)], ids=lambda v: _id(v) if isinstance(v, Case) else f"prec{v}")
def test_split_operand_kernel_at_its_launch_sizes(c, prec):
    lib = _lib.load()
    B, T, H, dh = c.B, c.T, c.H, c.dh
    D = H * dh
    x, _, _, o, _ = make_case(c, torch.float32)
    xd = x.to(DEV)
    out = torch.full((B, T, D), float("nan"), device=DEV)
    _lib.check(lib.svt_debug_attention(prec, xd.data_ptr(), xd.data_ptr() + 4 * D, xd.data_ptr() + 8 * D, out.data_ptr(), B, T, H, dh,
                                       3 * D, 3 * D, D, _scale(dh), 0, torch.cuda.current_stream().cuda_stream), "svt_debug_attention")
    kid = lib.svt_debug_set(38, 0)
    torch.cuda.synchronize()
    assert kid == c.kid, f"kernel {kid} ran, the case is written for kernel {c.kid}"
    got = out.cpu()
    assert torch.isfinite(got).all(), "unwritten (NaN-poisoned) outputs"
    err = (got.double() - o).abs()
    tol = SPLIT_TOL[prec] * (c.gain / 1.5) ** 3
    b, t, col = np.unravel_index(int(err.argmax()), err.shape)
    print(f"split attention prec={prec} {_id(c)}: max|err| {err.max().item():.3e} (limit {tol:.1e}) at clip {b} query {t} head {col // dh}")
    assert err.max().item() < tol, (prec, _id(c), err.max().item())


def test_case_tables_cover_every_kernel():
    """Removing the only case that reaches a kernel fails here: the tables must name every id the launchers can report."""
    assert {c.kid for c in CASES_16} == {1, 2, 3}
    assert {c.kid for c in CASES_BIAS} == {4, 5}
    assert {c.kid for c in CASES_SPLIT} == {6, 7, 8}
    for kid, cases in ((3, CASES_16), (5, CASES_BIAS), (8, CASES_SPLIT)):   # the wide kernels: both branches of the block map, peaked rows
        wide = [c for c in cases if c.kid == kid]
        assert any(c.B * c.H % 8 for c in wide) and any(c.B * c.H % 8 == 0 for c in wide) and any(c.gain == 8.0 for c in wide)
    for kid in (3, 8):
        assert {(c.T + 255) // 256 for c in CASES_16 + CASES_SPLIT if c.kid == kid} == {1, 2, 3, 4}
