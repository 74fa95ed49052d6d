"""CPU test of the per-element limit that tests/test_gpu_gemm_kernels.py holds the 16-bit GEMM kernels to (tests/gemm_limit.py): a correct
kernel, simulated -- fp32 accumulation in 32-wide K chunks, fp32 activation, one round-to-nearest store -- stays inside it on every case
shape in both builds, and the two defects the flat max-abs tolerances let through do not: a 16-bit store that truncates, and one row that
misses one 32-element K block."""
import pytest
import torch

import gemm_limit as G


def _shapes():
    seen, out = set(), []
    for c in G.CASES:
        key = (c.M, c.N, c.K, c.conv, c.act, c.out_f32, c.resid, c.bias)
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


SHAPES = _shapes()


@pytest.mark.parametrize("build", list(G.BUILDS))
@pytest.mark.parametrize("c", SHAPES, ids=G.case_id)
def test_limit_on_a_simulated_kernel(c, build):
    dtype = G.BUILDS[build][1]
    inp, z, S, ref = G.case_data(c, build)
    lim = G.limit(c, build, z, S, ref, inp["resid"])
    ok, where = G.worst(c, G.simulate(c, inp, dtype).double(), ref, lim)
    print(f"[{build}] {G.case_id(c)}: correct kernel {ok:.3f} at {where}")
    assert ok <= 1.0, (ok, where)
    row = c.M - 1                                                      # (a tail row: the one a wrong M-tail clamp would hit)
    short, where = G.worst(c, G.simulate(c, inp, dtype, drop=(row, (c.K // 32) // 2)).double(), ref, lim)
    print(f"[{build}] {G.case_id(c)}: row {row} without one K block {short:.3g}")
    assert short > 1.0, "a row that misses 32 of its K products passes the limit"
    if not c.out_f32:
        trunc, _ = G.worst(c, G.simulate(c, inp, dtype, truncate=True).double(), ref, lim)
        print(f"[{build}] {G.case_id(c)}: truncating store {trunc:.3f}")
        assert trunc > 1.0, "a truncating 16-bit store passes the limit"


def test_truncation_helper_truncates():
    x = torch.tensor([1.0 + 2.0 ** -7 + 2.0 ** -9, -(1.0 + 2.0 ** -7 + 2.0 ** -9), 3.0, -0.0, 1.0 + 2.0 ** -10 + 2.0 ** -12])
    assert G.truncate_to(x, torch.bfloat16).float().tolist() == [1.0 + 2.0 ** -7, -(1.0 + 2.0 ** -7), 3.0, -0.0, 1.0]
    assert G.truncate_to(x, torch.float16).float().tolist() == [1.0 + 2.0 ** -7 + 2.0 ** -9, -(1.0 + 2.0 ** -7 + 2.0 ** -9), 3.0, -0.0, 1.0 + 2.0 ** -10]


def test_case_tables_reach_every_kernel_and_both_sides_of_the_thresholds():
    """Removing the only case that reaches a kernel, a tile height or an epilogue fails here."""
    ids = {c.kid for c in G.CASES}
    assert ids >= {1032, 1064, 2128, 2256} | {f * 1000 + bm for f in (3, 4) for bm in (64, 128, 192, 256)} | {f * 1000 + bm for f in (5, 6) for bm in (128, 192, 256)}
    for fam in (5, 6):   # forced and chosen by the dispatcher
        mine = [c for c in G.CASES if c.kid // 1000 == fam]
        assert any(dict(c.keys).get(3) == 70 or dict(c.keys).get(29) == 2 for c in mine) and any(set(dict(c.keys)) <= {1} for c in mine)
    assert {G.gelu_form(c) for c in G.CASES if c.act == 1} == {"fast", "poly"}
    assert {c.kid // 1000 for c in G.GELU_ALONE} == {1, 2, 3, 4, 5, 6}
