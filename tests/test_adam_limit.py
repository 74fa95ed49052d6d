"""tests/adam_limit.py judged on the CPU: a numpy fp32 restatement of the kernel's order (csrc/adam.hip adam_element) stays inside the
derived limits on the GPU tests' inputs at steps 1, 2, 10 and 1000 -- steps 1 and 2 are where the bias corrections are far from 1 --, and
every mutant of it leaves them.  No GPU, no library."""
import numpy as np
import pytest

import adam_limit as AL

MIXED_STEPS = (1, 2, 10, 1000, 2)   # per tensor of MID_LIST: a parameter whose gradient was None in some steps is behind the others


def _run(numels, steps, clip, h, seed=3, mutant=None):
    """The largest |got - formula| / limit over a list, per array."""
    tensors, steps = AL.list_inputs(numels, seed, steps)
    coef64 = coef32 = None
    if clip:
        total, _ = AL.clip_coef64(tensors, 1.0)
        max_norm = 0.5 * total   # a coefficient near 0.5: the clip acts
        coef64 = AL.clip_coef64(tensors, max_norm)[1]
        coef32 = AL.clip_coef32(tensors, max_norm)[1]
        assert 0.4 < coef64 < 0.6
    out = dict.fromkeys(("g", "m", "v", "x", "p"), 0.0)
    for t, k in zip(tensors, steps):
        got = AL.restate_fp32(t, k, h, coef32, mutant=mutant, ss_step=steps[0] if mutant == "first_step_size" else None)
        w = AL.worst(got, t, k, h, coef64 if clip else 1.0, clip)
        out = {a: max(out[a], w[a]) for a in out}
    return out


def test_inputs_are_as_stated():
    for step in AL.STEPS:
        tensors, _ = AL.list_inputs(AL.NUMELS + AL.MID_LIST, 3, step)
        g = np.concatenate([np.abs(t["g"]) for t in tensors])
        assert g.min() >= 0.999e-3 and g.max() <= 1.0
        v = np.concatenate([t["v"] for t in tensors])
        assert (v == 0).all() if step == 1 else (v > 0).all()


@pytest.mark.parametrize("step", AL.STEPS)
def test_restatement_stays_inside_the_limits_for_every_flag_combination(step):
    worst = 0.0
    for clip, h in AL.flag_cases():
        w = _run(AL.MID_LIST, step, clip, h)
        worst = max(worst, max(w.values()))
        assert max(w.values()) <= 1.0, (clip, h, w)
    print(f"step {step}: largest |restatement - fp64| / limit over 24 flag combinations {worst:.3f}")


@pytest.mark.parametrize("step", AL.STEPS)
@pytest.mark.parametrize("clip", [False, True])
def test_restatement_stays_inside_the_limits_at_every_size(step, clip):
    for h in (AL.hyper(), AL.hyper(weight_decay=0.01, amsgrad=True)):
        w = _run(AL.NUMELS, step, clip, h, seed=5)
        assert max(w.values()) <= 1.0, (h, w)


def test_restatement_stays_inside_the_limits_with_a_step_per_tensor_and_other_betas():
    for clip, h in AL.flag_cases():
        w = _run(AL.MID_LIST, MIXED_STEPS, clip, h)
        assert max(w.values()) <= 1.0, (clip, h, w)
    for betas in ((0.3, 0.9), (0.5, 0.99), (0.0, 0.5)):   # both lerp branches
        w = _run(AL.MID_LIST, MIXED_STEPS, True, AL.hyper(betas=betas, weight_decay=0.01))
        assert max(w.values()) <= 1.0, (betas, w)


MUTANT_SETUPS = {   # mutant -> (steps, clip, hyper) at which it must show
    "no_bias_correction": [(s, False, AL.hyper()) for s in AL.STEPS],
    "bc2_without_sqrt": [(s, False, AL.hyper()) for s in AL.STEPS],
    "eps_inside_sqrt": [(s, False, AL.hyper()) for s in AL.STEPS],
    "clip_stored_only": [(s, True, AL.hyper()) for s in AL.STEPS],
    "decay_form_swapped": [(s, False, AL.hyper(weight_decay=0.01, decoupled=d)) for s in AL.STEPS for d in (False, True)],
    "amsgrad_max_before": [(s, False, AL.hyper(amsgrad=True)) for s in AL.STEPS],
    "skip_last_of_chunk": [(s, c, AL.hyper()) for s in AL.STEPS for c in (False, True)],
    "first_step_size": [(MIXED_STEPS, False, AL.hyper()), (MIXED_STEPS, True, AL.hyper(weight_decay=0.01, amsgrad=True))],
}


@pytest.mark.parametrize("mutant", AL.MUTANTS)
def test_every_mutant_leaves_the_limits(mutant):
    assert set(MUTANT_SETUPS) == set(AL.MUTANTS)
    for steps, clip, h in MUTANT_SETUPS[mutant]:
        good = _run(AL.MID_LIST, steps, clip, h)
        bad = _run(AL.MID_LIST, steps, clip, h, mutant=mutant)
        assert max(good.values()) <= 1.0
        print(f"{mutant} steps={steps} clip={clip}: worst / limit {max(bad.values()):.3g}")
        assert max(bad.values()) > 1.0, (mutant, steps, clip, h, bad)
