"""CPU proof of the checks tests/test_gpu_conv0.py applies to the kernels of the waveform front end (tests/conv0_limit.py derives them): a
correct kernel of every family, simulated in two summation orders with the piece arithmetic in the piece type and storing as the real
kernels store, stays inside every check in every case of the GPU tables and both builds; every mutant falls outside in every case it can
show in -- except a truncated lo piece, which the limits of these outputs cannot be relied on to see (conv0_limit.py says why; counted here).  Needs no GPU."""
import collections

import pytest

import conv0_limit as Z

RUNS = [(c, b) for c in Z.APPLY for b in Z.builds(c)]
FAMILY = {3: "vector, group", 4: "vector, layer", 5: "matrix pipe, group", 6: "matrix pipe, layer"}


def test_the_tables_reach_every_kernel_and_every_branch():
    assert {Z.kid_of(c.form, c.out) for c in Z.APPLY} | {Z.K_MOM, Z.K_WIN, Z.K_COEF} == set(Z.ALL_IDS)
    by = collections.defaultdict(set)
    for c in Z.APPLY:
        by[c.form].add(c.T1)
        assert Z.length(c) - ((c.T1 - 1) * c.stride + Z.K0) in (0, c.stride - 1) and c.B in (3, 4) and c.B % c.cpg == 0
    assert by[3] == {1, 31, 32, 33, 128, 129, 161} and by[4] == {1, 2, 15, 16, 17, 64, 65, 81}
    assert by[5] == by[6] == {1, 3, 4, 5, 16, 17, 63, 64, 65, 256, 257, 323}
    for form in (3, 4):
        assert {c.C for c in Z.APPLY if c.form == form and not c.out.startswith("pk")} == {8, 32, 264, 512}
        assert {c.C for c in Z.APPLY if c.form == form and c.out.startswith("pk")} == {32, 512}
        assert {c.stride for c in Z.APPLY if c.form == form} == {1, 3, 5}
    for form in (4, 6):
        assert any(not c.wav_mom for c in Z.APPLY if c.form == form) and {c.cpg == c.B for c in Z.APPLY if c.form == form} == {True, False}
    assert {c.n for c in Z.MOMENTS} == {3, 4099, 4 * 256 * 300 + 2, 4096} and {c.groups for c in Z.MOMENTS if c.n == 4096} == {1, 3, 64, 70}
    assert {c.T1 for c in Z.WINDOWS} == {1, 7, 8, 9, 2048, 2049, 8 * 2048 + 1}
    assert {c.C for c in Z.COEFS} == {8, 70, 512} and {c.cpg for c in Z.COEFS} == {4, 2, 1}
    assert any(not c.wav_mom for c in Z.COEFS) and any(not c.b0 for c in Z.COEFS) and {c.kind for c in Z.COEFS} == {"lowpass", "white"}
    # the matrix-pipe group cases reach the clamp of kx + ka (clip 3's strip of zeros) in every case, and an unclamped strip beside it
    for c in Z.APPLY:
        if c.form == 5:
            _, _, _, clamped, _ = Z.strip_scales(c, Z.apply_inputs(c))
            assert clamped[3, 0] and not clamped[:3].any(), Z.case_id(c)


def test_correct_ordered_sums_stay_inside_and_a_lost_partial_does_not():
    worst = 0.0
    for table, make in ((Z.MOMENTS, Z.moments_inputs), (Z.WINDOWS, Z.window_inputs)):
        for c in table:
            x, ref, lim = make(c)
            for order in (0, 1):
                fails, w = Z.check_sums(Z.simulate_sums(c, x, order), ref, lim)
                assert not fails, (Z.case_id(c), order, fails)
                worst = max(worst, w)
            fails, _ = Z.check_sums(Z.simulate_sums(c, x, 0, "partial lost"), ref, lim)
            assert fails, f"a lost partial passes {Z.case_id(c)}"
    print(f"simulated ordered sums: exact kinds bit-equal; random kinds worst err / limit {worst:.4f}")
    assert worst <= 1.0


def test_correct_coefficients_stay_inside_and_the_mutants_do_not():
    worst, kappa_max = 0.0, 0.0
    shown = collections.Counter()
    for c in Z.COEFS:
        inp = Z.coef_inputs(c)
        ref, lim, kappa = Z.coef_reference(c, inp)
        kappa_max = max(kappa_max, float(kappa.max()))
        for order in (0, 1):
            fails, w = Z.check_coef(Z.simulate_coef(c, inp, order), ref, lim)
            assert not fails, (Z.case_id(c), order, fails)
            worst = max(worst, w)
        for mutant in Z.COEF_MUTANTS:
            if mutant == Z.COEF_MUTANTS[0] and not (c.wav_mom and c.cpg < c.B):
                continue   # without moments nothing is indexed; with cpg == B the other groups lie outside the moments
            fails, w = Z.check_coef(Z.simulate_coef(c, inp, 0, mutant), ref, lim)
            assert fails, f"{mutant!r} passes {Z.case_id(c)}"
            shown[mutant] += 1
    print(f"simulated coefficient kernel: worst err / limit {worst:.4f}; cancellation factor A / (var + eps) up to {kappa_max:.3g}")
    assert worst <= 1.0 and all(shown[m] for m in Z.COEF_MUTANTS), shown


def test_a_correct_kernel_stays_inside_every_check():
    worst = collections.defaultdict(float)
    for c, build in RUNS:
        inp, ref, lim = Z.apply_data(c, build)
        for order in (0, 1):
            rows, guard = Z.simulate_apply(c, build, inp, order)
            fails, w = Z.check_apply(c, build, rows, ref, lim)
            assert not fails and not guard, (Z.case_id(c), build, order, fails)
            worst[(c.form, c.out, build)] = max(worst[(c.form, c.out, build)], w)
    for (form, out, build), w in sorted(worst.items()):
        print(f"simulated correct kernel, form {form} ({FAMILY[form]}), {out} rows [{build}]: worst err / limit {w:.4f}")
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize("mutant", Z.APPLY_MUTANTS)
def test_a_mutant_falls_outside(mutant):
    shown, passed = 0, 0
    for c, build in RUNS:
        if not Z.applies(mutant, c, build):
            continue
        inp, ref, lim = Z.apply_data(c, build)
        for order in (0, 1):
            rows, guard = Z.simulate_apply(c, build, inp, order, mutant)
            fails, w = Z.check_apply(c, build, rows, ref, lim)
            if mutant in Z.BLIND:
                passed += not (fails or guard)
            else:
                assert fails or guard, f"{mutant!r} passes every check of {Z.case_id(c)} [{build}] in order {order}"
            shown += 1
    assert shown > 0
    if mutant in Z.BLIND:
        print(f"mutant {mutant!r}: inside every check in {passed} of {shown} runs, as derived: these outputs cannot be relied on to show it")
        assert passed > shown // 2
    else:
        print(f"mutant {mutant!r}: caught in all {shown} runs it can show in")
