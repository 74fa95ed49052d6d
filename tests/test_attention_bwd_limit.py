"""CPU check of the limits tests/test_gpu_attention_backward.py holds the fused attention backward to (tests/attention_bwd_limit.py): a
model of the three kernels' arithmetic passes them at every value case in both operand types, and every mutant -- each a mistake a
kernel of this kind can make while still producing plausible numbers -- breaks one of them at every case it can touch (the mask mutants:
every case that draws a mask).  A mutant that slips under the limit at a case means the case list is too weak: change the cases, not
the limit."""
import numpy as np
import pytest
import torch

import attention_bwd_limit as AB
import dropout_cases as DC

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}

_cache = {}


def _case(c, dtype):
    """Inputs, reference and limits of a case, computed once and shared by the tests."""
    key = (c, dtype)
    if key not in _cache:
        x, do = AB.make_inputs(c, dtype)
        _cache[key] = (x, do, AB.reference(c, x, do, dtype))
    return _cache[key]


def _worst(c, dtype, mutant=None):
    """{gradient: worst err / limit} of the model (or a mutant of it)."""
    x, do, ref = _case(c, dtype)
    got = AB.model(c, x, do, ref["o"], dtype, mutant)
    out = {}
    for name, t in zip(("dq", "dk", "dv"), got):
        t = t.double()
        out[name] = ((t - ref[name]).abs() / ref["lim_" + name]).max().item() if torch.isfinite(t).all() else float("inf")
    return out


@pytest.mark.parametrize("build", list(DTYPES))
@pytest.mark.parametrize("c", AB.VALUE_CASES, ids=AB.case_id)
def test_model_of_the_kernels_passes_the_limits(c, build):
    worst = _worst(c, DTYPES[build])
    print(f"model [{build}] {AB.case_id(c)}: worst err / limit " + ", ".join(f"{n} {w:.3f}" for n, w in worst.items()))
    assert max(worst.values()) <= 1.0, (build, AB.case_id(c), worst)


@pytest.mark.parametrize("build", list(DTYPES))
@pytest.mark.parametrize("c", AB.VALUE_CASES, ids=AB.case_id)
def test_every_mutant_breaks_a_limit(c, build):
    for mutant in AB.MUTANTS:
        if not AB.touches(mutant, c):
            continue
        worst = _worst(c, DTYPES[build], mutant)
        print(f"mutant {mutant} [{build}] {AB.case_id(c)}: worst err / limit " + ", ".join(f"{n} {w:.1f}" for n, w in worst.items()))
        assert max(worst.values()) > 1.0, (mutant, build, AB.case_id(c), worst)


def test_the_mask_helper_is_the_fixture_mask():
    for c in AB.VALUE_CASES[:2] + AB.VALUE_CASES[4:5]:
        n = c.B * c.H * c.T * c.T
        want = DC.keep(c.p, c.seed, c.step, DC.SITE_ATTN_PROBS, c.layer, n, c.e0).reshape(c.B, c.H, c.T, c.T)
        assert np.array_equal(AB.keep_mask(c), want)


def test_cases_are_what_the_mutants_need():
    for c in AB.VALUE_CASES:
        assert c.T % 64 and c.H > 1 and c.layer and c.step
    assert {c.T for c in AB.VALUE_CASES} == {65, 129, 499}
    assert {c.p for c in AB.VALUE_CASES} == {0.0, 0.1, 0.5}
    assert any(c.gain == 8.0 for c in AB.VALUE_CASES) and any(c.layout == "separate" for c in AB.VALUE_CASES)
    assert any(c.e0 == 2 ** 34 + 1 for c in AB.VALUE_CASES)
    assert all(any(AB.touches(m, c) for c in AB.VALUE_CASES) for m in AB.MUTANTS)
