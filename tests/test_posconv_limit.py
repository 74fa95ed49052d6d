"""CPU proof of the checks tests/test_gpu_encoder_glue.py applies to the encoder's glue (tests/posconv_limit.py derives them): a correct
positional conv, simulated in fp32 with the kernels' own indexing (gather, shifted-filter rows, q = t / Pf and j = t % Pf, scatter), stays
inside the per-element limit in every case and mode of the GPU table, and each of twelve mutants falls outside in at least one; HF's bucket
formula, the kernel's arithmetic and the fp64 floor agree at every distance and the edge sets are as small as the GPU test relies on; an fp32
evaluation of the gate in both summation orders stays inside its limit and five mutants do not.  Needs no GPU."""
import collections

import numpy as np
import pytest
import torch

import gemm_limit as G
import layernorm_limit as L
import posconv_limit as P


def test_the_table_reaches_every_form_mode_and_tail():
    forms = collections.defaultdict(set)
    tails = collections.defaultdict(set)
    for c, mode in P.RUNS:
        assert P.form_of(c, mode) == c.form, (P.pcase_id(c), mode)
        forms[c.form].add(mode)
        if c.form == "multi":
            Pf = P.pf_of(c)
            tails[(c.cg, c.kp)].add("0" if c.T % Pf == 0 else "1" if c.T % Pf == 1 else "Pf-1" if c.T % Pf == Pf - 1 else "other")
    assert forms["plain"] == set(P.MODES) and forms["multi"] == set(P.SIXTEEN + P.SPLIT) and forms["stack"] == {"fp32"} | set(P.SIXTEEN)
    assert tails[(64, 8)] >= {"0", "1", "Pf-1"} and tails[(48, 16)] >= {"0", "1", "Pf-1"} and tails[(16, 17)] >= {"0", "1"}, dict(tails)
    # the switch: 127 and 128 GEMM rows of one handle
    sw = [c for c in P.PCASES if c.tag == "switch"]
    assert sorted(c.B * ((c.T + 3) // 4) for c in sw) == [127, 128] and len({P.geometry_key(c) for c in sw}) == 1
    # eligibility: Pf = 10 frames per row would need (kp + 9) cg to be a multiple of 64
    ne = [c for c in P.PCASES if c.tag == "not-eligible"]
    assert ne and all(P.pf_of(c) == 0 and 256 // c.cg >= 2 and c.B * c.T // (256 // c.cg) >= 128 for c in ne)


def test_a_correct_step_stays_inside_the_limit():
    worst = collections.defaultdict(float)
    for c, mode in P.RUNS:
        params, h, ref, lim = P.case_data(c, mode)
        assert torch.isfinite(ref).all() and torch.isfinite(lim).all() and (lim > 0).all()
        w, where = P.worst(P.simulate(c, mode, params, h), ref, lim)
        assert w <= 1.0, (P.pcase_id(c), mode, w, where)
        worst[(c.form, mode)] = max(worst[(c.form, mode)], w)
    for (form, mode), w in sorted(worst.items()):
        print(f"simulated correct {form} form [{mode}]: worst err / limit {w:.4f}")


@pytest.mark.parametrize("mutant", P.PMUTANTS)
def test_a_positional_conv_mutant_falls_outside(mutant):
    shown, caught, ratios = 0, 0, []
    for c, mode in P.RUNS:
        if not P.papplies(mutant, c, mode):
            continue
        params, h, ref, lim = P.case_data(c, mode)
        w, _ = P.worst(P.simulate(c, mode, params, h, mutant), ref, lim)
        shown += 1
        caught += w > 1.0
        ratios.append(w)
    print(f"mutant {mutant!r}: outside the limit in {caught} of the {shown} runs it can show in; err / limit from {min(ratios):.3g} to {max(ratios):.3g}")
    assert caught >= 1


def test_the_stack_limit_is_layernorm_limit_without_an_input_error():
    """ln_limit with e_in = 0 is layernorm_limit.reference with gamma = 1, beta = 0: the composition adds no constant of its own."""
    c = next(c for c in L.CASES if c.unit and not c.gelu and c.prec == 0)
    inp, ref, lim = L.case_data(c, "bf16")
    t = inp["t32"].double()
    y, lim_y = P.ln_limit(t, torch.zeros_like(t), c.eps)
    assert torch.allclose(y, ref, rtol=0, atol=1e-12) and torch.allclose(lim_y, lim, rtol=1e-12, atol=0)


# ---- relative-position buckets
def test_the_three_bucket_evaluations_agree_at_every_distance():
    a = np.arange(8192)
    for nb, md in P.CONFIGS:
        hf = P.bucket_hf(torch.from_numpy(a), nb, md).numpy()
        kn = P.bucket_kernel_np(a, nb, md)
        f64 = P.bucket_f64(a, nb, md)
        assert np.array_equal(hf, kn), (nb, md, a[hf != kn][:8])
        assert np.array_equal(hf, f64), (nb, md, a[hf != f64][:8])
        assert hf.max() == nb // 2 - 1 and (np.diff(hf) >= 0).all()


def test_the_edge_sets_are_small():
    for nb, md in P.CONFIGS:
        e = P.edges(nb, md)
        print(f"buckets {nb} max distance {md}: edge distances {e}")
        assert len(e) <= 4, (nb, md, e)
        if (nb, md) == (320, 800):
            assert e == [80, 713]
        elif (nb, md) == (32, 128):
            assert e == [8, 16, 32, 64]
        else:
            assert e == [nb // 4], (nb, md, e)


def test_the_table_reference_takes_the_upper_half_for_keys_behind_the_query():
    pb = P.table_reference(2, 5, 8, 16)   # nb = 4, max_exact = 2
    assert pb.shape == (2, 9)
    assert pb[0].tolist() == [2 * b for b in (2, 2, 2, 1, 0, 5, 6, 6, 6)] and torch.equal(pb[1], pb[0] + 1)


# ---- the gate
def _gate_runs():
    for c in P.GCASES:
        for block in P.GBLOCKS:
            for dtype in (torch.float32, torch.bfloat16, torch.float16):
                yield c, block, dtype


def test_a_correct_gate_stays_inside_the_limit_in_both_orders():
    worst, beyond, inside = 0.0, 0, 0
    for c, block, dtype in _gate_runs():
        w, b, const = P.gate_params(c, block)
        u = P.gate_input(c, block, dtype)
        ref, lim, s = P.gate_reference(c, w, b, const, u)
        if block == "saturated":
            beyond += int((s.abs() > 90).sum())
            inside += int((s.abs() < 20).sum())
        for order in (("chain", "tree") if c.vec else ("chain",)):
            got = P.gate_simulate(c, w, b, const, u, order)
            assert torch.isfinite(got).all()
            r = ((got.double() - ref).abs() / lim).max().item()
            assert r <= 1.0, (P.gcase_id(c), block, dtype, order, r)
            worst = max(worst, r)
    print(f"simulated correct gate: worst err / limit {worst:.4f}; saturated block: {beyond} pre-activations beyond +-90, {inside} within +-20")
    assert beyond > 1000 and inside > 100, "the saturated block must reach beyond +-90 and keep ordinary rows"


@pytest.mark.parametrize("mutant", P.GMUTANTS)
def test_a_gate_mutant_falls_outside(mutant):
    shown = 0
    for c, block, dtype in _gate_runs():
        if not P.gapplies(mutant, c) or block != "ordinary":
            continue
        w, b, const = P.gate_params(c, block)
        u = P.gate_input(c, block, dtype)
        ref, lim, _ = P.gate_reference(c, w, b, const, u)
        got = P.gate_simulate(c, w, b, const, u, "tree" if c.vec else "chain", mutant)
        r = ((got.double() - ref).abs() / lim).max().item()
        assert r > 1.0, f"{mutant!r} passes the limit of {P.gcase_id(c)} [{dtype}]: err / limit {r:.3g}"
        shown += 1
    assert shown > 0


def test_the_gate_fold_is_the_hosts():
    """Rows 0-3 and 4-7 summed in fp32 from 0 in row order (csrc/host.cpp gate_rowsum_fold)."""
    w = torch.randn(8, 16, generator=torch.Generator().manual_seed(3))
    b = torch.randn(8, generator=torch.Generator().manual_seed(4))
    wab, bab = P.fold_gate(w, b)
    assert torch.equal(wab[0], ((w[0] + w[1]) + w[2]) + w[3]) and torch.equal(wab[1], ((w[4] + w[5]) + w[6]) + w[7])
    assert torch.equal(bab, torch.stack([((b[0] + b[1]) + b[2]) + b[3], ((b[4] + b[5]) + b[6]) + b[7]]))
    assert G.BUILDS["bf16"][1] is torch.bfloat16
