"""GPU unit tests of the split-operand GEMM kernels -- gemm_x3s_kernel (family 7), gemm_x3p_kernel (8), gemm_x3q_kernel (9), gemm_p1x_kernel
(10) and the split instantiation of the register-staged kernel (12) -- and of the register-staged kernel's fp32 parity mode (family 2 at
precision 0), at the smallest shapes that select each, through svt_debug_gemm and svt_debug_gemm_pairs.

Every case names the kernel id svt_debug_set(39, 0) must report behind the launch and asserts it; the thresholds of csrc/gemm_dispatch.hip
are not restated here.  Every touched debug key is restored in a `finally`.  The reference of every test is the three-term value
T = Ah Wh^T + Al Wh^T + Ah Wl^T (+ bias) in fp64 (tests/gemm_split.py), NOT the fp64 product of the operands.

  test_exact_cases     operands whose arithmetic is exact in fp32 in any order: bit equality, up to the longest K the exactness budget
                       allows, several tiles per workgroup (key 37 = 8), integer bias / residual, ReLU, pair and plane outputs.  THE SHARP TEST.
  test_random_cases    random operands under the derived per-element limit, NaN poison inside and 64 poisoned guard rows on each side of the
                       output; GELU, fractional biases, N tails, conv rows.  The limit cannot see a single lost term (tests/gemm_split.py,
                       tests/test_gemm_limit.py): do not mistake these cases for the sharp ones.
  test_cut             one operand one-hot: C = hi(x) + lo(x) over the whole magnitude range of the piece type, bit for bit -- the grid in W
                       (split_pack_kernel) and in A (the kernels' own cut; f32_to_pairs for the pair-row kernels).
  test_gelu_alone      the GELU epilogue without accumulation error."""
import pytest
import torch

import gemm_limit as G
import gemm_split as X

pytestmark = pytest.mark.gpu

from svt_speechbrain_amd import _lib  # noqa: E402

DEV = "cuda:0"
GUARD = 64   # poisoned rows in front of row 0 and behind row M - 1 of the buffer the hook is given


def launch(c, prec, A, W, bias, resid, addr):
    """The case's product under its debug keys, every touched key restored.  Returns (C (M, N) fp32 on the CPU, kernel id).  The buffer handed to
    the hook is NaN-poisoned between 64 poisoned guard rows; with pair / plane output the kernel writes a buffer of the hook's own and the
    guards surround what the hook reads back from it."""
    lib = _lib.load(X.library(c))
    rpb, bstr, rstr = addr
    Ad, Wd = A.to(DEV), W.to(DEV)
    bd = bias.to(DEV) if bias is not None else None
    rd = resid.to(DEV) if resid is not None else None
    buf = torch.full((c.M + 2 * GUARD, c.N), float("nan"), device=DEV)
    before = buf.view(torch.int32).clone()
    out = buf.data_ptr() + GUARD * c.N * 4
    stream = torch.cuda.current_stream().cuda_stream
    keys = dict(c.keys)
    assert set(keys) <= set(G.KEY_DEFAULTS)
    try:
        for k, v in keys.items():
            _lib.check(lib.svt_debug_set(k, v), f"svt_debug_set({k}, {v})", lib)
        if c.out_kind is None:
            rc = lib.svt_debug_gemm(prec, Ad.data_ptr(), Wd.data_ptr(), out, bd.data_ptr() if bd is not None else None,
                                    rd.data_ptr() if rd is not None else None, c.M, c.N, c.K, rpb, bstr, rstr, c.K, c.act, 0, 0, stream)
            _lib.check(rc, "svt_debug_gemm", lib)
        else:
            assert rd is None
            rc = lib.svt_debug_gemm_pairs(prec, Ad.data_ptr(), Ad.numel(), Wd.data_ptr(), out, bd.data_ptr() if bd is not None else None,
                                          c.M, c.N, c.K, rpb, bstr, rstr, c.act, c.out_kind, 0, stream, 0, None)
            _lib.check(rc, "svt_debug_gemm_pairs", lib)
        kid = lib.svt_debug_set(39, 0)
        torch.cuda.synchronize()
    finally:
        for k in keys:
            lib.svt_debug_set(k, G.KEY_DEFAULTS[k])
    after = buf.view(torch.int32)
    assert torch.equal(after[:GUARD], before[:GUARD]), "rows in front of row 0 were written"
    assert torch.equal(after[GUARD + c.M:], before[GUARD + c.M:]), "rows behind row M - 1 were written"
    return buf[GUARD:GUARD + c.M].cpu(), kid


def _params(table):
    return [pytest.param(c, p, id=f"{X.case_id(c)}-prec{p}") for c in table for p in X.precisions(c)]


@pytest.mark.parametrize("c,prec", _params(X.EXACT))
def test_exact_cases(c, prec):
    inp = X.exact_inputs(c, prec)
    exp = X.exact_expected(c, inp, prec)
    got, kid = launch(c, prec, inp["A"], inp["W"], inp["bias"], inp["resid"], inp["addr"])
    assert kid == c.kid, f"kernel {kid} ran, the case is written for kernel {c.kid}"
    assert bool((got == exp).all()), X.first_mismatch(c, got, exp)   # (every bit but the sign of a zero; a NaN equals nothing)


_cache = {}   # test speed only: the two pair-row families and their tile heights share operands and references


def _random_data(c, prec):
    key = (c.M, c.N, c.K, c.conv, c.act, c.resid, c.bias, prec)
    if key not in _cache:
        if len(_cache) >= 6:
            _cache.pop(next(iter(_cache)))
        inp = G.make_inputs(c, torch.float32)
        _cache[key] = (inp,) + X.reference(c, inp, prec)
    return _cache[key]


@pytest.mark.parametrize("c,prec", _params(X.RANDOM))
def test_random_cases(c, prec):
    inp, z, S3, ref = _random_data(c, prec)
    got, kid = launch(c, prec, inp["A"], inp["W"], inp["bias"], inp["resid"], inp["addr"])
    assert kid == c.kid, f"kernel {kid} ran, the case is written for kernel {c.kid}"
    assert not torch.isnan(got).any(), "unwritten (NaN-poisoned) outputs"
    ratio, where = X.worst(c, got, ref, X.limit(c, prec, z, S3, ref, inp["resid"]))
    print(f"split gemm [prec {prec}] {X.case_id(c)}: worst err / limit {ratio:.4f} at {where}")
    assert ratio <= 1.0, (prec, X.case_id(c), ratio, where)


def _one_hot(rows, K):
    H = torch.zeros(rows, K)
    H[torch.arange(rows), torch.arange(rows) % 64] = 1.0
    return H


@pytest.mark.parametrize("side", ["W", "A"])
@pytest.mark.parametrize("c,prec", _params(X.ALONE))
def test_cut(c, prec, side):
    """C[m, n] = hi(x) + lo(x), bit for bit, over the piece type's whole range (X.cut_grid: every binade, +-0, one ulp below the powers of two, the
    ties of the hi rounding, and for IEEE-half pieces subnormal lo pieces, hi = 0 and 65504 .. 65519).  side W: the grid is the weight matrix
    (split_pack_kernel cuts it) and A is one-hot; side A: the grid is the activation (cut inside gemm_x3s_kernel / gemm_x3p_kernel / the
    register-staged kernel; by f32_to_pairs in front of the pair-row kernels) and W is one-hot.  With pair output the stored value is cut once more
    (cut8 in the epilogue): the expectation is the cut of hi + lo."""
    dtype = X.PIECE[prec][0]
    A, W = torch.zeros(c.M, c.K), torch.zeros(c.N, c.K)

    def grid_of(n):
        g = X.cut_grid(prec, n)
        if c.out_kind and prec == 3:
            # hi + lo of 65519.996 is 65520: as a STORED value it would leave the contract of the second cut.  65519 = 65504 + 15 stays inside
            g = torch.where(X.recombine(g, dtype).abs() >= 65520.0, torch.copysign(torch.tensor(65519.0), g), g)
        return g

    if side == "W":
        grid = grid_of(c.N * 64).reshape(c.N, 64)
        W[:, :64] = grid
        A = _one_hot(c.M, c.K)
        x = grid.t()[torch.arange(c.M) % 64]                 # C[m, n] <- W[n, m % 64]
    else:
        grid = grid_of(c.M * 64).reshape(c.M, 64)
        A[:, :64] = grid
        W = _one_hot(c.N, c.K)
        x = grid[:, torch.arange(c.N) % 64]                  # C[m, n] <- A[m, n % 64]
    exp = X.recombine(x.contiguous(), dtype)
    if c.out_kind:
        exp = X.recombine(exp, dtype)
    c0 = c._replace(bias=False)
    got, kid = launch(c0, prec, A, W, None, None, (c.M, 0, c.K))
    assert kid == c.kid, f"kernel {kid} ran, the case is written for kernel {c.kid}"
    bad = got != exp   # every bit but the sign of a zero (x = -2^-26 cuts into two negative zeros, an accumulator that started at +0 ends at +0)
    if bad.any():
        i = int(bad.flatten().float().argmax())
        m, n = i // c.N, i % c.N
        hi, lo = X.cut(x[m, n], dtype)
        raise AssertionError(f"{int(bad.sum())} of {bad.numel()} differ; first at row {m} column {n}: x = {x[m, n].item():.9g} "
                             f"(hi {hi.item():.9g} lo {lo.item():.9g}) got {got[m, n].item():.9g} expected {exp[m, n].item():.9g}")


def gelu_grids():
    """The W grids (512 x 64 fp32 values) and their biases: dense [-8, 8] in 32768 steps with bias 0, and the same under a fractional bias."""
    dense = torch.linspace(-8.0, 8.0, 512 * 64, dtype=torch.float64).float().reshape(512, 64)
    frac = torch.rand(512, generator=torch.Generator().manual_seed(1)) - 0.5
    return [("dense", dense, torch.zeros(512)), ("frac", dense, frac)]


@pytest.mark.parametrize("c,prec", _params(X.ALONE))
def test_gelu_alone(c, prec):
    """The GELU epilogue of every split family without accumulation error: A is one-hot, so z = hi + lo of W[n, m % 64] (+ bias[n]) and the limit
    is 2^-24 |ref| + 5e-7 |z| / 2 -- the store's rounding and the documented bound of gelu_erf / gelu_fast (csrc/common.h) -- plus
    1.13 2^-24 |z| under the fractional bias (z itself is rounded) and, for pair output, the cut of the stored value."""
    dtype = X.PIECE[prec][0]
    c1 = c._replace(act=1)
    A = _one_hot(c.M, c.K)
    for name, grid, bias in gelu_grids():
        W = torch.zeros(c.N, c.K)
        W[:, :64] = grid
        got, kid = launch(c1, prec, A, W, bias, None, (c.M, 0, c.K))
        assert kid == c.kid, f"kernel {kid} ran, the case is written for kernel {c.kid}"
        assert not torch.isnan(got).any(), "unwritten (NaN-poisoned) outputs"
        z = (X.recombine(grid, dtype).double().t() + bias.double()[None, :])[torch.arange(c.M) % 64]   # (M, N)
        ref = G.gelu64(z)
        lim = 2.0 ** -24 * ref.abs() + G.g_act("fast", None, z)
        if name == "frac":
            lim += 1.13 * 2.0 ** -24 * z.abs()
        if c.out_kind:
            lim += X.cut_term(prec, ref)
        ratio = (got.double() - ref).abs() / lim.clamp_min(1e-300)
        ratio = torch.where(got.double() == ref, torch.zeros_like(ratio), ratio)   # 0 / 0 at z = +-0
        i = int(ratio.argmax())
        m, n = i // c.N, i % c.N
        print(f"split gelu [prec {prec}] {X.case_id(c)} {name}: worst err / limit {ratio.max().item():.4f} at z = {z[m, n].item():.6g}: "
              f"got {got[m, n].item():.9g} ref {ref[m, n].item():.9g} (row {m} column {n})")
        assert ratio.max().item() <= 1.0, (prec, X.case_id(c), name, z[m, n].item(), got[m, n].item(), ref[m, n].item())
