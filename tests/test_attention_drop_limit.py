"""CPU check of the limit tests/test_gpu_attention_dropout.py holds the fused masked attention to (tests/attention_drop_limit.py): a model
of the kernel's arithmetic passes it at every value case in both operand types, and every mutant -- each a mistake a kernel of this kind
can make while still producing plausible numbers -- breaks it at every case.  A mutant that slips under the limit at a case means the
case list is too weak: change the cases, not the limit."""
import numpy as np
import pytest
import torch

import attention_drop_limit as AD

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}

_cache = {}


def _case(c, dtype):
    """Inputs, reference and limit of a case, computed once and shared by the tests."""
    key = (c, dtype)
    if key not in _cache:
        x = AD.make_inputs(c, dtype)
        ref, A = AD.reference(c, x, AD.keep_mask(c))
        _cache[key] = (x, ref, AD.limit(c, x, ref, A, dtype))
    return _cache[key]


def _worst(c, dtype, mutant=None):
    x, ref, lim = _case(c, dtype)
    got = AD.model(c, x, dtype, mutant).double()
    if not torch.isfinite(got).all():   # a mutant may divide by a row sum of 0 (peaked rows whose dominant key is dropped): broken
        assert mutant is not None
        return float("inf")
    return ((got - ref).abs() / lim).max().item()


@pytest.mark.parametrize("build", list(DTYPES))
@pytest.mark.parametrize("c", AD.VALUE_CASES, ids=AD.case_id)
def test_model_of_the_kernel_passes_the_limit(c, build):
    worst = _worst(c, DTYPES[build])
    print(f"model [{build}] {AD.case_id(c)}: worst err / limit {worst:.3f}")
    assert worst <= 1.0, (build, AD.case_id(c), worst)


@pytest.mark.parametrize("build", list(DTYPES))
@pytest.mark.parametrize("c", AD.VALUE_CASES, ids=AD.case_id)
def test_every_mutant_breaks_the_limit(c, build):
    for mutant in AD.MUTANTS:
        worst = _worst(c, DTYPES[build], mutant)
        print(f"mutant {mutant} [{build}] {AD.case_id(c)}: worst err / limit {worst:.1f}")
        assert worst > 1.0, (mutant, build, AD.case_id(c), worst)


def test_the_mask_helper_is_the_fixture_mask():
    """keep_mask restates tests/dropout_cases.py's keep on the (B, H, T, T) index: equal bit for bit, e0 and q_hi != 0 included."""
    import dropout_cases as DC
    for c in AD.VALUE_CASES[:2] + AD.VALUE_CASES[3:4]:
        n = c.B * c.H * c.T * c.T
        want = DC.keep(c.p, c.seed, c.step, DC.SITE_ATTN_PROBS, c.layer, n, c.e0).reshape(c.B, c.H, c.T, c.T)
        assert np.array_equal(AD.keep_mask(c), want)


def test_cases_are_strong_enough_for_the_mutants():
    for c in AD.VALUE_CASES:
        assert c.T % 64 and c.H > 1 and c.layer and c.step and c.p >= 0.1
