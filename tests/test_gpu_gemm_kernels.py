"""GPU unit tests of every 16-bit GEMM kernel, in both builds (libsvt_mi355.so: bf16 operands, libsvt_mi355_f16.so: IEEE half), at the
smallest shapes that select it, through the C-ABI test hook svt_debug_gemm.

Every case names the kernel it is written for -- the id svt_debug_set(39, 0) reports after the launch, 1000 * family + tile rows
(include/svt_mi355.h) -- and asserts it, so a moved threshold in csrc/gemm_dispatch.hip fails a case instead of silently moving it to
another kernel.  The tests do not restate the thresholds (100 tiles, K >= 192, GELU with K < 1024, 512 tiles): the shapes sit on both
sides of them and the id decides.  Families 5 and 6 are reached both by force (keys 3 / 29) and by the dispatcher's own choice.

Every output element is compared with an fp64 reference of the same rounded operands under the per-element limit of tests/gemm_limit.py
(its docstring derives it; tests/test_gemm_limit.py shows on the CPU that a correct kernel passes it and that a truncating store or a lost
K block does not).  The output is NaN-poisoned with 64 poisoned guard rows before row 0 and behind row M - 1 in the same allocation: the
guards must come back bit-unchanged (M-tail overruns) and no NaN may be left inside.  The worst err / limit of a case is printed with its
tile, its row inside the tile and its column.

The edges, per kernel (tests/gemm_limit.py holds the tables): K at the contract minimum (one slab for gemm_skinny_kernel with three of
its four waves idle and for gemm_pp8_kernel, two for gemm_pers_kernel / gemm_pps_kernel, three for gemm_p1w_kernel), a workgroup that owns
many tiles (key 37 = 8), a last tile with one valid row, N tails down to the scalar-store path, implicit-conv rows, every tile height."""
import pytest
import torch

import gemm_limit as G

pytestmark = pytest.mark.gpu

from svt_speechbrain_amd import _lib  # noqa: E402

DEV = "cuda:0"
GUARD = 64   # poisoned rows in front of row 0 and behind row M - 1


def launch(lib, c, A, W, bias, resid, addr, dtype):
    """svt_debug_gemm(1, ...) under the case's debug keys, every touched key restored.  Returns (C (M, N) on the CPU, kernel id)."""
    rpb, bstr, rstr = addr
    out_dtype = torch.float32 if c.out_f32 else dtype
    Ad, Wd = A.to(DEV), W.to(DEV)
    bd = bias.to(DEV) if bias is not None else None
    rd = resid.to(DEV) if resid is not None else None
    buf = torch.full((c.M + 2 * GUARD, c.N), float("nan"), device=DEV, dtype=out_dtype)
    ints = torch.int32 if c.out_f32 else torch.int16
    before = buf.view(ints).clone()
    keys = dict(c.keys)
    assert set(keys) <= set(G.KEY_DEFAULTS)
    try:
        for k, v in keys.items():
            _lib.check(lib.svt_debug_set(k, v), f"svt_debug_set({k}, {v})", lib)
        rc = lib.svt_debug_gemm(1, Ad.data_ptr(), Wd.data_ptr(), buf.data_ptr() + GUARD * c.N * buf.element_size(),
                                bd.data_ptr() if bd is not None else None, rd.data_ptr() if rd is not None else None,
                                c.M, c.N, c.K, rpb, bstr, rstr, c.K, c.act, c.out_f32, 0, torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "svt_debug_gemm", lib)
        kid = lib.svt_debug_set(39, 0)
        torch.cuda.synchronize()
    finally:
        for k in keys:
            lib.svt_debug_set(k, G.KEY_DEFAULTS[k])
    after = buf.view(ints)
    assert torch.equal(after[:GUARD], before[:GUARD]), "rows in front of row 0 were written"
    assert torch.equal(after[GUARD + c.M:], before[GUARD + c.M:]), "rows behind row M - 1 were written"
    return buf[GUARD:GUARD + c.M].cpu(), kid


@pytest.mark.parametrize("build", list(G.BUILDS))
@pytest.mark.parametrize("c", G.CASES, ids=G.case_id)
def test_kernel_at_the_shapes_that_select_it(c, build):
    variant, dtype, _ = G.BUILDS[build]
    lib = _lib.load(variant)
    inp, z, S, ref = G.case_data(c, build)
    got, kid = launch(lib, c, inp["A"], inp["W"], inp["bias"], inp["resid"], inp["addr"], dtype)
    assert kid == c.kid, f"kernel {kid} ran, the case is written for kernel {c.kid}"
    assert not torch.isnan(got).any(), "unwritten (NaN-poisoned) outputs"
    ratio, where = G.worst(c, got, ref, G.limit(c, build, z, S, ref, inp["resid"]))
    print(f"gemm [{build}] {G.case_id(c)}: worst err / limit {ratio:.3f} at {where}")
    assert ratio <= 1.0, (build, G.case_id(c), ratio, where)


def _bits(dtype):
    return torch.arange(-2 ** 15, 2 ** 15, dtype=torch.int32).to(torch.int16).view(dtype)


def gelu_grids(dtype):
    """The W grids (512 x 64 values of the build's 16-bit type, C[m, n] = act(W[n, m % 64] + bias[n])) and their biases:
    dense: [-8, 8] in 32768 steps (2^-11: every IEEE-half value from 1 up, every bf16 value and 15 repeats of it), bias 0;
    edges: +-3 and +-3.8 (where the two polynomials saturate) with their neighbours, +-6, +-100, +-0, the smallest normals, bias 0;
    frac:  the dense grid under a fractional fp32 bias, which fills the low mantissa bits of z."""
    dense = torch.linspace(-8.0, 8.0, 512 * 64, dtype=torch.float64).to(dtype).reshape(512, 64)
    allv = _bits(dtype)
    allv = allv[torch.isfinite(allv.float())]
    tiny = float(torch.finfo(dtype).tiny)
    near = [allv[(allv.float() - x).abs().argsort()[:8]] for x in (3.0, -3.0, 3.8, -3.8)]
    edge = torch.cat(near + [torch.tensor([6.0, -6.0, 100.0, -100.0, 0.0, -0.0, tiny, -tiny, 2 * tiny, -2 * tiny], dtype=torch.float64).to(dtype)])
    edges = edge.repeat(512 * 64 // edge.numel() + 1)[:512 * 64].reshape(512, 64)
    g = torch.Generator().manual_seed(1)
    frac = torch.rand(512, generator=g) - 0.5
    return [("dense", dense, torch.zeros(512)), ("edges", edges, torch.zeros(512)), ("frac", dense, frac)]


@pytest.mark.parametrize("build", list(G.BUILDS))
@pytest.mark.parametrize("c", G.GELU_ALONE, ids=G.case_id)
def test_gelu_alone(c, build):
    """The GELU epilogue of every kernel family that has one, without accumulation error: A is one-hot (A[m, m % 64] = 1, K padded with zero
    columns to the kernel's minimum), so C[m, n] = gelu(W[n, m % 64] + bias[n]) and the limit is u_out |ref| + eta_out + g_act(z), the rounding
    of the store and the documented bound of the form the kernel calls alone (under the fractional bias also the one fp32 rounding of z,
    1.13 2^-24 |z|): gemm_skinny_kernel and the register-staged kernel call gelu_fast, the four LDS-DMA kernels
    gelu_bf16x2 for 16-bit output and gelu_erf (= gelu_fast) for fp32 output, which two of them have (csrc/common.h; G.gelu_form)."""
    variant, dtype, u = G.BUILDS[build]
    lib = _lib.load(variant)
    A = torch.zeros(c.M, c.K, dtype=dtype)
    A[torch.arange(c.M), torch.arange(c.M) % 64] = 1.0
    for name, grid, bias in gelu_grids(dtype):
        W = torch.zeros(c.N, c.K, dtype=dtype)
        W[:, :64] = grid
        got, kid = launch(lib, c, A, W, bias, None, (c.M, 0, c.K), dtype)
        assert kid == c.kid, f"kernel {kid} ran, the case is written for kernel {c.kid}"
        assert not torch.isnan(got).any(), "unwritten (NaN-poisoned) outputs"
        z = (grid.double().t() + bias.double()[None, :])[torch.arange(c.M) % 64]   # (M, N)
        ref = G.gelu64(z)
        lim = (2.0 ** -24 * ref.abs() if c.out_f32 else u * ref.abs() + G.ETA[build]) + G.g_act(G.gelu_form(c), build, z)
        if name == "frac":
            lim += 1.13 * 2.0 ** -24 * z.abs()   # z itself is rounded once: W + bias in fp32
        ratio = (got.double() - ref).abs() / lim.clamp_min(1e-300)
        ratio = torch.where((got.double() == ref), torch.zeros_like(ratio), ratio)   # 0 / 0 at z = +-0
        i = int(ratio.argmax())
        m, n = i // c.N, i % c.N
        print(f"gelu [{build}] {G.case_id(c)} {name} ({G.gelu_form(c)}): worst err / limit {ratio.max().item():.3f} at z = {z[m, n].item():.6g}: "
              f"got {got[m, n].item():.6g} ref {ref[m, n].item():.6g} (row {m} column {n})")
        assert ratio.max().item() <= 1.0, (build, G.case_id(c), name, z[m, n].item(), got[m, n].item(), ref[m, n].item())

