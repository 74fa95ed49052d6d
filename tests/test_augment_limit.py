"""The yardstick of tests/test_gpu_augment.py, proven on the CPU (tests/augment_limit.py), and the host side of
svt_speechbrain_amd/augment.py against tests/golden/augment.pt (recorded from the reference's own DropFreq, DropChunk and
TimeDomainSpecAugment):

* the limit holds for a correct fp32 evaluation in either order and for torch's conv1d, and every mutant misses it -- window shifted,
  taps flipped, bf16 taps, edges clamped, first / last tap dropped, and a dropped span multiplied by zero with a NaN inside;
* drop_filter is within 2 x the fixture's filter_vs_fp64 of an fp64 evaluation of the same formulas (the reference's own distance: the
  ops and their order are the same, only the math library under sin and sum may differ between hosts);
* the draws, replayed without a GPU, give the fixture's frequencies, chunk pairs and generator state for every case;
* the constructors validate and clamp as the reference's do."""
import pytest
import torch

import augment_limit as AL
import svt_speechbrain_amd as S
from svt_speechbrain_amd import augment as A, resample as R

LENGTHS = (101, 441, 1500)


@pytest.fixture(scope="module")
def fx():
    return AL.load_fixture()


_cache = {}


def dense_case(n):
    if n not in _cache:
        x = AL.seeded_input(2, n, 500 + n % 97)
        f = AL.dense_taps(AL.TAPS, 40 + n % 7)
        want, M = AL.exact(x, f)
        _cache[n] = (x, f, want, AL.limit(M, AL.TAPS))
    return _cache[n]


@pytest.mark.parametrize("n", (3, 50) + LENGTHS)
def test_a_correct_evaluation_is_inside_the_limit(n):
    x, f, want, lim = dense_case(n)
    for descending in (False, True):
        r = AL.worst(AL.direct_fp32(x, f, descending=descending), want, lim)
        print(f"n = {n}, {'descending' if descending else 'ascending'}: {r:.4f} of the limit")
        assert r <= 1.0
    conv = torch.nn.functional.conv1d(x.unsqueeze(1), f.view(1, 1, -1), padding=AL.TAPS // 2)[:, 0]
    r = AL.worst(conv, want, lim)
    print(f"n = {n}, conv1d: {r:.4f} of the limit")
    assert r <= 1.0


@pytest.mark.parametrize("mutant", AL.MUTANTS)
@pytest.mark.parametrize("n", LENGTHS)
def test_every_mutant_misses_the_limit(n, mutant):
    x, f, want, lim = dense_case(n)
    r = AL.worst(AL.direct_fp32(x, f, mutant=mutant), want, lim)
    print(f"n = {n}, {mutant}: {r:.3g} of the limit")
    assert r > 1.0


def test_a_span_multiplied_by_zero_keeps_its_nan():
    """A dropped element is 0, whatever the filter gave: a NaN sample well inside the span makes the filtered value NaN, and a product
    with zero keeps it."""
    x, f, _, _ = dense_case(441)
    x = x.clone()
    x[0, 200] = float("nan")
    pairs = [[(100, 300)], []]
    mask = AL.chunk_mask(pairs, 2, 441)
    clean = torch.where(torch.isnan(x), torch.zeros(()), x)
    want, M = AL.exact(clean, f)
    want = torch.where(mask, torch.zeros((), dtype=torch.float64), want)
    lim = AL.limit(M, AL.TAPS)
    y = AL.direct_fp32(x, f)
    assert AL.worst(torch.where(mask, torch.zeros(()), y), want, lim) <= 1.0      # written as zero
    assert AL.worst(y * (~mask).float(), want, lim) == float("inf")                # multiplied by zero


def test_the_two_exact_sums_agree():
    """conv1d in fp64 against the terms written out: within 2^-50 M, far below the limit's 2^-24 M."""
    for n in (3, 50, 441):
        x, f, want, lim = dense_case(n)
        y2, M2 = AL.exact_by_windows(x, f)
        assert bool(((want - y2).abs() <= 2.0 ** -50 * M2 + 1e-300).all())
        assert bool(((lim - AL.limit(M2, AL.TAPS)).abs() <= 2.0 ** -50 * lim).all())
    x5 = AL.seeded_input(1, 7, 1)
    f5 = torch.tensor([1.0, 2.0, 4.0, 8.0, 16.0])
    y, _ = AL.exact(x5, f5)                                # the first tap meets the sample two to the LEFT: a correlation
    assert y[0, 3].item() == sum(float(f5[k]) * float(x5[0, 3 + k - 2]) for k in range(5))


def test_chunk_mask_rule():
    mask = AL.chunk_mask([[(2, 4), (3, 6)], [(8, 20)], [(5, 5), (7, 3)], []], 4, 10)
    assert mask.tolist() == [[False, False, True, True, True, True, False, False, False, False],
                             [False] * 8 + [True, True], [False] * 10, [False] * 10]


def test_drop_filter_against_fp64(fx):
    seen = 0
    for name, rec in fx["cases"].items():
        if rec["filter"] is None:
            continue
        seen += 1
        got = S.drop_filter(rec["frequencies"])
        assert got.shape == (AL.TAPS,) and got.dtype == torch.float32
        d = (got.double() - AL.drop_filter_fp64(rec["frequencies"])).abs().max().item()
        print(f"{name}: drop_filter is {d:.3g} from the fp64 build, the reference {rec['filter_vs_fp64']:.3g}; "
              f"from the reference's filter {(got - rec['filter']).abs().max().item():.3g}")
        assert d <= 2 * rec["filter_vs_fp64"]
    assert seen == 4


def test_the_filter_is_a_correlation_and_not_symmetric(fx):
    """Two notches: the flipped taps differ by more than 1e-3 (the periodic Blackman window), so the taps' order matters; composing by
    convolution (the first notch flipped) is another filter."""
    f = S.drop_filter(fx["cases"]["drop_freq_2"]["frequencies"])
    assert (f - f.flip(0)).abs().max() > 1e-3
    one = S.notch_filter(torch.tensor(0.25))            # a 0-dim fp32 tensor, as DropFreq passes it: frequency + width is an fp32 sum
    assert (one - S.notch_filter(0.25)).abs().max() < 1e-6
    assert one.shape == (1, 101, 1) and one.dtype == torch.float32
    assert torch.equal(S.drop_filter([0.25]), torch.nn.functional.conv1d(torch.eye(101)[50].view(1, 1, -1), one.view(1, 1, -1), padding=50).view(-1))
    # a tensor frequency is not changed by the call: frequency + notch_width is applied once, out of place
    fr = torch.tensor([0.25])
    S.drop_filter(fr)
    assert fr.item() == 0.25
    assert torch.equal(S.notch_filter(fr[0]), one)


def replay(name):
    """The case's draws without a GPU: (frequencies or None, chunk pairs or None, speed index or None)."""
    kind, kwargs, shape, lengths, seed = AL.CASES[name]
    module = getattr(S, kind)(**kwargs)
    torch.manual_seed(seed)
    freqs = chunks = speed = None
    n = shape[1]
    if kind == "TimeDomainSpecAugment":
        sp = module.speed_perturb                         # SpeedPerturb.forward's draws, which need the GPU only for what follows them
        assert not bool(torch.rand(1) > sp.perturb_prob)
        speed = int(torch.randint(len(sp.speeds), (1,))[0])
        new = sp.orig_freq * sp.speeds[speed] // 100
        n = n if new == sp.orig_freq else R.output_samples(n, sp.orig_freq, new)
        freqs = module.drop_freq.draw()
        module.drop_chunk.draw(AL.case_lengths(name), n)
        chunks = module.drop_chunk.chunks
    elif kind == "DropFreq":
        freqs = module.draw()
    else:
        module.draw(AL.case_lengths(name), n)
        chunks = module.chunks
    return freqs, chunks, speed, n


@pytest.mark.parametrize("name", list(AL.CASES))
def test_the_draws_are_the_references(fx, name):
    rec = fx["cases"][name]
    assert AL.sha256(AL.case_input(name)) == rec["sha256"]
    freqs, chunks, speed, n = replay(name)
    assert AL.rng_digest() == rec["rng"]
    assert speed == rec["speed"] and n == rec["out"].shape[1]
    if rec["frequencies"] is None:
        assert freqs is None or freqs.numel() == 0
    else:
        assert torch.equal(freqs, rec["frequencies"])
    assert chunks == rec["chunks"]
    if chunks is not None:      # the recorded output is zero exactly where the pairs say (a Gaussian input has no zeros of its own)
        assert torch.equal(rec["out"] == 0, AL.chunk_mask(chunks, *rec["out"].shape))


def test_the_fixture_holds_what_the_cases_need(fx):
    c = fx["cases"]
    assert len(c["drop_freq_1"]["frequencies"]) == 1 and len(c["drop_freq_2"]["frequencies"]) == 2
    short = c["drop_chunk"]["chunks"][2]                # a clip of 90 samples: every chunk starts at 0 and is longer than the clip
    assert short and all(s == 0 and e >= 100 for s, e in short)
    assert c["lobe_speeds"]["speed"] != 1 and c["lobe_speeds"]["out"].shape[1] != 6000 and c["lobe_100"]["out"].shape[1] == 6000
    for name in ("lobe_100", "lobe_speeds"):
        assert c[name]["filter"] is not None and any(c[name]["chunks"])


def test_slice_pairs_follow_the_slice_rules():
    table, most = A.slice_pairs([[(5, 10), (100, 300)], [], [(-5, 9), (190, 250), (7, 7)]], 200)
    assert most == 3 and table.shape == (3, 3, 2) and table.dtype == torch.int64
    assert table.tolist() == [[[5, 10], [100, 200], [0, 0]], [[0, 0]] * 3, [[195, 9], [190, 200], [7, 7]]]
    table, most = A.slice_pairs([[], []], 200)
    assert most == 0


def test_sample_lengths_are_an_fp32_product():
    lengths = torch.tensor([1.0, 0.5, 0.03, 0.7], dtype=torch.float32)
    assert A.sample_lengths(lengths, 3000).tolist() == (lengths * 3000).long().tolist() == [3000, 1500, 90, 2100]


def test_constructor_validation():
    for bad in (dict(drop_length_low=200, drop_length_high=100), dict(drop_count_low=3, drop_count_high=2), dict(drop_start=300, drop_end=200)):
        with pytest.raises(ValueError, match="Low limit must not be more than high limit"):
            S.DropChunk(**bad)
    d = S.DropChunk(drop_start=100, drop_end=350)           # the length limits are clamped to drop_end - drop_start
    assert (d.drop_length_low, d.drop_length_high) == (100, 250)
    d = S.DropChunk(drop_start=100, drop_end=150)
    assert (d.drop_length_low, d.drop_length_high) == (50, 50)
    d = S.DropChunk(drop_start=-300, drop_end=-100)         # a negative end: no clamping, as in the reference
    assert (d.drop_length_low, d.drop_length_high) == (100, 1000)
    with pytest.raises(NotImplementedError, match="device generator"):
        S.DropChunk(noise_factor=0.5)
    with pytest.raises(NotImplementedError):
        S.TimeDomainSpecAugment(drop_chunk_noise_factor=0.5)
    f = S.DropFreq()
    assert (f.drop_freq_low, f.drop_freq_high, f.drop_count_low, f.drop_count_high, f.drop_width, f.drop_prob) == (1e-14, 1, 1, 2, 0.05, 1)
    lobe = S.TimeDomainSpecAugment()
    assert lobe.speed_perturb.speeds == [95, 100, 105] and (lobe.drop_freq.drop_count_low, lobe.drop_freq.drop_count_high) == (0, 3)
    assert (lobe.drop_chunk.drop_count_low, lobe.drop_chunk.drop_count_high, lobe.drop_chunk.drop_length_low,
            lobe.drop_chunk.drop_length_high) == (0, 5, 1000, 2000)


def test_probability_misses_draw_nothing_more():
    torch.manual_seed(5)
    assert S.DropFreq(drop_prob=-1.0).draw() is None
    table, most = S.DropChunk(drop_prob=-1.0).draw(torch.ones(2), 1000)
    assert table is None and most == 0
    after = AL.rng_digest()
    torch.manual_seed(5)
    torch.rand(1)
    torch.rand(1)
    assert AL.rng_digest() == after


def test_cpu_waveforms_are_refused():
    for module, args in ((S.DropFreq(), ()), (S.DropChunk(), (torch.ones(2),)), (S.TimeDomainSpecAugment(speeds=[100]), (torch.ones(2),))):
        with pytest.raises(S._lib.SvtError, match="no CPU fallback"):
            module(torch.zeros(2, 300), *args)


def test_the_modules_constants_are_the_headers():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "svt_mi355.h")).read()
    defines = dict(re.findall(r"#define (SVT_DROP_\w+) (\d+)", header))
    assert defines == {"SVT_DROP_MAX_TAPS": str(A.MAX_TAPS), "SVT_DROP_TILE_OUTPUTS": str(A.TILE_OUTPUTS),
                       "SVT_DROP_MAX_WORKGROUPS": str(A.MAX_WORKGROUPS)}
    assert A.MAX_TAPS >= A.FILTER_LENGTH == AL.TAPS == 101 and A.MAX_TAPS % 2 == 1
