"""CPU proof of the checks tests/test_gpu_layernorm.py applies to the LayerNorm kernels (tests/layernorm_limit.py derives them): a
correct fp32 two-pass kernel, simulated in both reduction orders of the real kernels (a wave per row: 64 lanes, six exchange steps; half a
wave per row: 32 lanes, five) and storing as they store, stays inside every check in every case of the GPU table and both builds; each
of thirteen mutants falls outside at least one check in every case it can show in.  Needs no GPU."""
import collections

import pytest
import torch

import layernorm_limit as L

RUNS = [(c, b) for c in L.CASES for b in L.builds(c)]


def test_the_table_reaches_every_kernel_and_every_edge_of_the_row_blocking():
    seen = collections.defaultdict(set)
    widths = collections.defaultdict(set)
    for c in L.CASES:
        seen[c.kid].add(c.rows)
        widths[c.kid].add(c.D)
    assert set(seen) == set(L.ALL_IDS), set(seen) ^ set(L.ALL_IDS)
    for kid in L.ALL_IDS:
        print(f"kernel {kid}: rows {sorted(seen[kid])} widths {sorted(widths[kid])}")
        assert widths[kid] == set(L.NARROW if kid // 1000 == 1 else L.WIDE), (kid, widths[kid])
        if kid in L.TWO_ROW_IDS:
            assert seen[kid] == set(L.ROWS), (kid, seen[kid])   # 8 rows per workgroup, 2 per wave, an idle half-wave when odd
        else:
            # 4 rows per workgroup: fewer than a workgroup, exactly one, one more, and more than two
            assert seen[kid] & {1, 3} and seen[kid] & {4, 8} and seen[kid] & {5, 9, 13} and max(seen[kid]) >= 9, (kid, seen[kid])
    kinds = {k for c in L.CASES for k in L.kinds_of(c)}
    assert kinds == set(L.KINDS)


def test_a_correct_kernel_stays_inside_every_check():
    worst = collections.defaultdict(float)
    outside = 0
    for c, build in RUNS:
        inp, ref, lim = L.case_data(c, build)
        for order in L.orders(c):
            fails, report = L.check_outputs(c, build, inp, ref, lim, L.simulate(c, build, inp, order))
            assert not fails, (L.case_id(c), build, order, fails)
            for name, (w, _, _) in report.items():
                if name == "yT outside its interval":
                    outside += int(w)
                elif name != "yT (information)":
                    worst[(c.kid, build)] = max(worst[(c.kid, build)], w)
    for (kid, build), w in sorted(worst.items()):
        print(f"simulated correct kernel {kid} [{build}]: worst err / limit {w:.4f}")
    print(f"worst of all: {max(worst.values()):.4f} (the limit is a worst-case bound over summation orders; random roundings stay far inside it)")
    assert outside == 0 and max(worst.values()) <= 1.0


@pytest.mark.parametrize("mutant", L.MUTANTS)
def test_a_mutant_falls_outside(mutant):
    shown, factor = 0, []
    for c, build in RUNS:
        if not L.applies(mutant, c):
            continue
        inp, ref, lim = L.case_data(c, build)
        for order in L.orders(c):
            fails, report = L.check_outputs(c, build, inp, ref, lim, L.simulate(c, build, inp, order, mutant))
            assert fails, f"{mutant!r} passes every check of {L.case_id(c)} [{build}] in order {order!r}"
            shown += 1
            factor.append(max([w for name, (w, _, _) in report.items() if name not in ("yT outside its interval", "yT (information)")] + [0.0]))
    assert shown > 0
    over = [f for f in factor if 1.0 < f < float("inf")]   # runs a limit sees; the others are seen by an interval, an identity or a left-over NaN alone
    nan = sum(f == float("inf") for f in factor)
    print(f"mutant {mutant!r}: caught in all {shown} runs it can show in; {len(over)} by a limit, err / limit from {min(over, default=0):.3g} to "
          f"{max(over, default=0):.3g}; {nan} by a NaN left in the output; {shown - len(over) - nan} by a 16-bit interval or a bit-exact identity alone")


def test_pair_row_layout_matches_the_kernels():
    """Element e of a row sits at byte (e >> 5) * 128 + (e & 31) * 2, its lo piece 64 bytes further (csrc/device_util.h store_pairs)."""
    hi = torch.arange(2 * 64, dtype=torch.int16).reshape(2, 64)
    lo = hi + 1000
    img = L.pack_pairs(hi.view(torch.bfloat16), lo.view(torch.bfloat16)).view(torch.uint8).reshape(2, 64 * 4)
    for r in range(2):
        for e in (0, 1, 31, 32, 63):
            off = (e >> 5) * 128 + (e & 31) * 2
            assert int(img[r, off]) + 256 * int(img[r, off + 1]) == int(hi[r, e])
            assert int(img[r, off + 64]) + 256 * int(img[r, off + 65]) == int(lo[r, e])
    h2, l2 = L.unpack_pairs(L.pack_pairs(hi.view(torch.bfloat16), lo.view(torch.bfloat16)), torch.bfloat16)
    assert torch.equal(h2.view(torch.int16), hi) and torch.equal(l2.view(torch.int16), lo)
