"""GPU unit tests of the BATCHED forms of the dense product, in both 16-bit builds, the fp32 parity mode and the split-operand modes, through
the C-ABI test hook svt_debug_gemm_batched: everything of a launch that svt_debug_gemm cannot express -- nz > 1 (blockIdx.y = z), the z
strides of A, W, C and the bias, alpha, ldc != N -- in the four forms the product callers use (tests/gemm_limit.py, BATCHED: the grouped
positional conv plain and phase-folded, scale q k^T and P V of the score-matrix attention).

Every case names the kernel it is written for (svt_debug_set(39, 0) after the launch) and asserts it.  Every element of every z is compared with
the fp64 reference of the same rounded operands under the per-element limit of tests/gemm_limit.py (one Case per z; tests/test_gemm_limit.py
shows on the CPU that a correct kernel passes and that a wrong z stride on the last clip's heads, a dropped bias_z2 and alpha applied after the
bias do not).  The C buffer is NaN-poisoned with 64 poisoned rows in front of it and behind it in the same allocation: the guards and every element
of the buffer that no z owns -- the columns [N, ldc) of the score rows -- must keep their bits, and no NaN may be left inside.  The worst
err / limit of a case is printed with its z1, z2, tile, row and column."""
import ctypes

import pytest
import torch

import gemm_limit as G

pytestmark = pytest.mark.gpu

from svt_speechbrain_amd import _lib  # noqa: E402

DEV = "cuda:0"
GUARD = 64   # poisoned rows of ldc elements in front of the C buffer and behind it


def describe(b, prec, ptrs, es):
    g = b.geom
    d = _lib.GemmDescC()
    d.struct_size = ctypes.sizeof(_lib.GemmDescC)
    d.a, d.c, d.bias, d.resid = ptrs["A"], ptrs["C"], ptrs["bias"], ptrs["resid"]
    d.w = ptrs["A"] + g.w_off * es if g.w_off is not None else ptrs["W"]
    d.m, d.n, d.k, d.a_rpb, d.a_bstride, d.a_rstride, d.ldw, d.ldc = g.M, g.N, g.K, g.a_rpb, g.a_bstride, g.a_rstride, g.ldw, g.ldc
    d.nz, d.nz2 = g.nz, g.nz2
    d.a_z1, d.a_z2, d.w_z1, d.w_z2, d.c_z1, d.c_z2, d.bias_z2 = g.a_z1, g.a_z2, g.w_z1, g.w_z2, g.c_z1, g.c_z2, g.bias_z2
    d.alpha, d.act, d.out_f32 = b.alpha, b.act, 0 if (prec == 1 and b.out16) else 1
    return d


def launch(lib, b, prec, dtype, bufs, edit=None):
    """The hook under the case's debug keys, every touched key restored.  Returns (rc, C buffer on the CPU (c_elems,), kernel id); asserts that the
    guards and every element no z owns kept their poison bits.  edit(desc): a change to the descriptor before the call (the refusals)."""
    g = b.geom
    assert G.batched_in_bounds(b), "the case addresses memory outside its buffers"
    out_dtype = dtype if (prec == 1 and b.out16) else torch.float32
    # (operands and residual with a zeroed tail behind them: a read past the end -- which tests/test_gpu_guard.py hunts with page guards --
    # would change a result here instead of faulting a GPU that other work shares)
    dev = {k: (torch.cat([v, v.new_zeros(4096)]).to(DEV) if v is not None else None) for k, v in bufs.items()}
    guard = GUARD * g.ldc
    buf = torch.full((g.c_elems + 2 * guard,), float("nan"), device=DEV, dtype=out_dtype)
    ints = torch.int32 if out_dtype == torch.float32 else torch.int16
    poison = int(buf.view(ints)[0].item())
    ptrs = {k: (v.data_ptr() if v is not None else None) for k, v in dev.items()}
    ptrs["C"] = buf.data_ptr() + guard * buf.element_size()
    d = describe(b, prec, ptrs, dev["A"].element_size())
    if edit:
        edit(d)
    keys = dict(b.keys)
    try:
        for k, v in keys.items():
            _lib.check(lib.svt_debug_set(k, v), f"svt_debug_set({k}, {v})", lib)
        rc = lib.svt_debug_gemm_batched(prec, ctypes.byref(d), 0, torch.cuda.current_stream().cuda_stream)
        kid = lib.svt_debug_set(39, 0)
        torch.cuda.synchronize()
    finally:
        for k in keys:
            lib.svt_debug_set(k, G.KEY_DEFAULTS[k])
    after = buf.view(ints)
    assert bool((after[:guard] == poison).all()), "elements in front of the C buffer were written"
    assert bool((after[guard + g.c_elems:] == poison).all()), "elements behind the C buffer were written"
    if rc == 0:
        own = torch.zeros(g.c_elems, dtype=torch.bool)
        for z in range(g.nz):
            own[G.batched_index(g, z)[2].flatten()] = True
        assert bool((after[guard:guard + g.c_elems][~own.to(DEV)] == poison).all()), "an element of the C buffer that no z owns was written"
    else:
        assert bool((after == poison).all()), "a refused launch wrote to C"
    return rc, buf[guard:guard + g.c_elems].cpu(), kid


RUNS = [(b, run) for b in G.BATCHED for run in G.batched_runs(b)]


@pytest.mark.parametrize("b,run", RUNS, ids=[f"{G.bcase_id(b)}-{run[3]}" for b, run in RUNS])
def test_batched_kernel_at_the_shapes_that_select_it(b, run):
    variant, dtype, prec, tag = run
    lib = _lib.load(variant)
    bufs = G.batched_inputs(b, dtype)
    rc, got, kid = launch(lib, b, prec, dtype, bufs)
    _lib.check(rc, "svt_debug_gemm_batched", lib)
    own = torch.cat([G.batched_index(b.geom, z)[2].flatten() for z in range(b.geom.nz)])
    ratio, where = G.batched_worst(b, prec, tag, bufs, lambda z, ci: got[ci])
    print(f"batched gemm [{tag}] {G.bcase_id(b)}: kernel {kid}, worst err / limit {ratio:.3f} at {where}")
    assert kid == b.kid, f"kernel {kid} ran, the case is written for kernel {b.kid}"
    assert not torch.isnan(got[own]).any(), "unwritten (NaN-poisoned) outputs"
    assert ratio <= 1.0, (tag, G.bcase_id(b), ratio, where)


def _folded16():
    return next(b for b in G.BATCHED if b.geom.form == "folded" and b.precs == "16" and not b.keys)


@pytest.mark.parametrize("field", ["a_z2", "w_z2"])
@pytest.mark.parametrize("build", list(G.BUILDS))
def test_a_z_stride_off_the_16_byte_piece_is_refused(build, field):
    """Operand rows are read in 16-byte pieces: a z stride that is not a multiple of 8 16-bit elements is an error, nothing is launched, C untouched."""
    variant, dtype, _ = G.BUILDS[build]
    lib = _lib.load(variant)
    b = _folded16()
    rc, _, _ = launch(lib, b, 1, dtype, G.batched_inputs(b, dtype), edit=lambda d: setattr(d, field, getattr(d, field) - 4))
    assert rc == -1 and b"16-byte aligned" in lib.svt_last_error(), (rc, lib.svt_last_error())   # SVT_ERR_INVALID


def test_the_hook_refuses_a_descriptor_of_another_size():
    lib = _lib.load()
    b = _folded16()
    rc, _, _ = launch(lib, b, 1, torch.bfloat16, G.batched_inputs(b, torch.bfloat16), edit=lambda d: setattr(d, "struct_size", d.struct_size - 8))
    assert rc == -1 and b"struct_size" in lib.svt_last_error()


def test_table_reaches_the_batched_arms():
    """Families 1, 2, 3, 7 and 12 each with nz > 1, and the refusal of the split batched arm (nz % nz2 != 0: the register-staged split kernel, same limit)."""
    assert {b.kid // 1000 for b in G.BATCHED if b.geom.nz > 1} >= {1, 2, 3, 7, 12}
    assert any(b.geom.nz % b.geom.nz2 and b.kid == 12128 and b.precs == (2, 3) for b in G.BATCHED)
