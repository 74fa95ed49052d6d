"""CPU proof for tests/test_gpu_video_kernels.py (no GPU): on the exact inputs the GPU test uses, a simulated correct kernel -- fp32
arithmetic, K in chunks of 32, one rounding to the output type -- stays inside every limit of tests/video_limit.py, each of sixteen
mutants breaks the check of a named case, and the direct convolutions' float row formula is exact at every geometry they accept."""
import pytest
import torch

import video_limit as V

BUILDS16 = ("bf16", "f16")


def _builds(c):
    return ("fp32",) if c.fp32 else BUILDS16


# ---- the row formula, exhaustively -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ok", [("c64", V.conv3x3_c64_ok), ("c128", V.conv3x3_c128_ok)])
def test_row_formula_is_exact_at_every_eligible_geometry(name, ok):
    """y = (int)((p + 0.5f) * (1.0f / Wp)) of conv3x3_c64_kernel / conv3x3_c128_kernel equals p // Wp for every position p < Hs (Ws + 2) of
    every (Hs, Ws) the kernel's predicate accepts: raising the LDS budget or the eligibility re-runs the proof over the new geometries."""
    geoms = V.direct_geometries(ok)
    assert len(geoms) > 300
    bad = [(Hs, Ws, int(f[0])) for (Hs, Ws) in geoms for f in (V.row_formula_failures(Hs, Ws),) if f.size]
    print(f"{name}: {len(geoms)} geometries, widest row Wp = {max(w for _, w in geoms) + 2}, most positions {max(h * (w + 2) for h, w in geoms)}")
    assert not bad, bad[:5]


def test_block_table_names_the_path_the_forward_takes():
    """The kernel id of every block case against the forward's path choice restated (video_block of csrc/api_video.hip): a case that names
    a direct kernel at a geometry its predicate refuses would never run it."""
    for c in V.BLOCKS:
        stride, _, _, Ho, Wo = V.block_dims(c)
        keys = dict(c.keys)
        direct = not c.fp32 and keys.get(23, 1) == 1
        if c.li == 0 and direct and V.conv3x3_c64_ok(Ho, Wo):
            want = V.block_kid(V.VK_C64, 0, V.VK_C64)
        elif c.li == 0 and V.group_width("fp32" if c.fp32 else "bf16", c.F, Ho, Wo):
            g = V.VK_G4 if V.group_width("bf16", c.F, Ho, Wo) == 4 else V.VK_G2
            want = V.block_kid(g, 0, g)
        else:
            d128 = c.li == 1 and direct and V.conv3x3_c128_ok(Ho, Wo)
            if d128 and stride == 1:
                k1, kd = V.VK_C128, 0
            elif c.li == 1 and stride == 2 and not c.fp32 and keys.get(27, 1) == 1:
                k1 = kd = V.VK_COMB
            else:
                k1, kd = V.VK_PLAIN, (V.VK_PLAIN if stride == 2 else 0)
            want = V.block_kid(k1, kd, V.VK_C128 if d128 else V.VK_PLAIN)
        assert c.kid == want, (c.name, c.kid, want)
    assert not V.conv3x3_c128_ok(3, 57) and V.conv3x3_c128_ok(1, 57) and not V.conv3x3_c128_ok(1, 58)
    assert all(V.conv3d_front_pool_ok(h, w) for h, w in V.FUSED_HW) and not V.conv3d_front_pool_ok(*V.FUSED_REFUSED)


# ---- a correct kernel stays inside every limit ----------------------------------------------------------------------------------
@pytest.mark.parametrize("build", ("bf16", "f16", "fp32"))
def test_correct_stem_pool_and_average_are_inside_their_limits(build):
    for c in V.STEM:
        video = V.video_input(c, build)
        ref, lim = V.stem_reference(build, video)
        r, at = V.check_plain(V.sim_stem(build, video), ref, lim, f"stem {c}")
        assert 0 < r
    for c in V.POOL:
        x = V.pool_input(c, build)
        V.check_exact_haloed(V.sim_pool(x), V.maxpool_reference(x), f"pool {c}")
    for c in V.AVG:
        xh = V.avg_input(c, build)
        V.check_plain(V.sim_avg(build, xh), *V.avg_reference(build, xh), f"avgpool {c}")
    if build != "fp32":
        for c in V.FUSED:
            video = V.video_input(c, build)
            ref, lim = V.fused_reference(build, video)
            V.check_haloed(V.sim_pool(V.sim_stem(build, video)), ref, lim, f"stem + pool {c}")


@pytest.mark.parametrize("name", [c.name for c in V.BLOCKS])
def test_correct_block_is_inside_its_limits(name):
    c = V.BLOCK_BY_NAME[name]
    for build in _builds(c):
        xh = V.block_input(c, build)
        res = V.check_block(c, build, xh, *V.sim_block(c, build, xh))
        assert all(0 < r <= 1 for r, _ in res.values()), res


# ---- every mutant is killed by a named case ---------------------------------------------------------------------------------------
# mutant -> (family, case, build): the case whose check the mutant breaks
KILLS = {
    "trunc_store": ("block", "c64-12x14-F1-wg0", "bf16"),
    "drop_tap": ("block", "c64-12x14-F1-wg0", "bf16"),
    "no_resid": ("block", "c64-12x14-F1-wg0", "f16"),
    "resid_after": ("block", "c128-7x7-F1-wg0", "bf16"),
    "slope_neighbour": ("block", "c128-4x10-F1-wg0", "bf16"),
    "swap_channels": ("block", "c64-13x13-F1-wg0", "bf16"),
    "frag_perm": ("block", "c64-12x14-F1-wg0", "bf16"),
    "garbage_col": ("block", "c64-13x13-F3-wg1", "bf16"),
    "shift_out": ("block", "c128-11x11-F1-wg0", "f16"),
    "group_no_rezero": ("block", "g4-7x7-F10", "bf16"),
    "comb_down_tap": ("block", "s2b0-13x13-F3", "bf16"),
    "time_pad_clip": ("stem", V.StemCase(9, 11, 2, 2), "bf16"),
    "stem_x_off": ("stem", V.StemCase(8, 8, 1, 2), "bf16"),
    "pool_pad0": ("pool", V.PoolCase(4, 4, 2), "bf16"),
    "pool_no_first_row": ("pool", V.PoolCase(5, 6, 2), "f16"),
    "avg_over_halo": ("avg", V.AvgCase(3, 3, 1), "fp32"),
}


def test_every_mutant_has_a_killing_case():
    assert set(KILLS) == set(V.MUTANTS)


@pytest.mark.parametrize("mutant", V.MUTANTS)
def test_mutant_breaks_the_check_of_its_named_case(mutant):
    family, c, build = KILLS[mutant]
    if family == "block":
        c = V.BLOCK_BY_NAME[c]
        xh = V.block_input(c, build)
        V.check_block(c, build, xh, *V.sim_block(c, build, xh))                  # the correct kernel passes this very case
        with pytest.raises(AssertionError):
            V.check_block(c, build, xh, *V.sim_block(c, build, xh, mutant))
    elif family == "stem":
        assert c in V.STEM
        video = V.video_input(c, build)
        ref, lim = V.stem_reference(build, video)
        V.check_plain(V.sim_stem(build, video), ref, lim, "stem")
        with pytest.raises(AssertionError):
            V.check_plain(V.sim_stem(build, video, mutant), ref, lim, "stem")
        # the fused kernel pools the same stem outputs: its check sees the mutant too
        fc = V.FusedCase(16, 18, 2, 3, 0)
        assert fc in V.FUSED
        fv = V.video_input(fc, build)
        with pytest.raises(AssertionError):
            V.check_haloed(V.sim_pool(V.sim_stem(build, fv, mutant)), *V.fused_reference(build, fv), "stem + pool")
    elif family == "pool":
        assert c in V.POOL
        x = V.pool_input(c, build)
        with pytest.raises(AssertionError):
            V.check_exact_haloed(V.sim_pool(x, mutant), V.maxpool_reference(x), "pool")
    else:
        assert c in V.AVG
        xh = V.avg_input(c, build)
        V.check_plain(V.sim_avg(build, xh), *V.avg_reference(build, xh), "avgpool")
        with pytest.raises(AssertionError):
            V.check_plain(V.sim_avg(build, xh, mutant), *V.avg_reference(build, xh), "avgpool")


def test_zero_halo_check_sees_a_missed_corner_and_a_written_interior():
    for c in V.HALO:
        t = torch.full((c.F, c.Hp, c.Wp, c.C), float("nan"), dtype=torch.bfloat16)
        poison = V._bits(t)[0, 0, 0, 0].item()
        good = t.clone()
        good[:, 0], good[:, -1], good[:, :, 0], good[:, :, -1] = 0, 0, 0, 0
        V.check_zero_halo(good, poison, str(c))
        for bad in (t.clone(), torch.zeros_like(t)):
            with pytest.raises(AssertionError):
                V.check_zero_halo(bad, poison, str(c))
        corner = good.clone()
        corner[-1, -1, -1, -1] = float("nan")
        with pytest.raises(AssertionError):
            V.check_zero_halo(corner, poison, str(c))
