"""The limit of tests/noise_limit.py against a correct evaluation and against wrong ones, on the CPU, on the inputs of the fixture
tests/golden/noise_mix.pt: the direct fp32 evaluation of the formula (coefficients in fp64, rounded once) stays inside 1.0 x limit on every
element, and each mutant leaves it on at least one of the samples the fixture records -- so the GPU test that holds svt_noise_mix to the
same limit on the same samples can tell them apart."""
import pytest
import torch

import noise_limit as NL


@pytest.fixture(scope="module")
def cases():
    fx = NL.load_fixture()
    songs, tracks = NL.fixture_inputs(fx)["songs"], NL.fixture_noise_tracks(fx)
    return fx, {key: (songs[key[0]], v) for key, v in tracks.items()}


def test_fixture_holds_every_song_type_and_snr(cases):
    fx, data = cases
    assert sorted(data) == sorted((s, t) for s in ("trunc", "pad") for t in ("accomp", "white", "babble", "natural"))
    assert sorted(fx["mix"]) == sorted((s, t, snr) for (s, t) in data for snr in NL.SNRS_DB)
    assert tuple(fx["snrs_db"]) == NL.SNRS_DB and fx["step"] == NL.STEP


def test_direct_evaluation_stays_inside_the_limit(cases):
    _, data = cases
    for key, (a, v) in data.items():
        ref, M = NL.formula(a, v)
        r = NL.worst(NL.direct_fp32(a, v), ref, NL.limit(M))
        print(f"{key}: direct fp32 evaluation at {r:.3f} of the limit")
        assert r <= 1.0, (key, r)


def test_reference_samples_are_as_far_from_the_formula_as_recorded(cases):
    """ref_vs_fp64 is what the fixture says it is (the GPU test widens its limit by it), and the reference is not far off: below 4."""
    fx, data = cases
    for (song, typ), (a, v) in data.items():
        idx = torch.arange(0, a.shape[0], NL.STEP)
        ref, M = NL.formula(a[idx], v[idx], NL.SNRS_DB, (NL.mean_abs_exact(a), NL.mean_abs_exact(v)))
        for s, snr in enumerate(NL.SNRS_DB):
            rec = fx["mix"][song, typ, snr]
            assert rec["samples"].shape == idx.shape
            assert NL.worst(rec["samples"], ref[s], NL.limit(M[s])) == pytest.approx(rec["ref_vs_fp64"], rel=1e-6)
            assert 0.0 < rec["ref_vs_fp64"] < 4.0


@pytest.mark.parametrize("mutant", NL.MUTANTS)
def test_mutant_leaves_the_limit_on_a_recorded_sample(cases, mutant):
    _, data = cases
    for key, (a, v) in data.items():
        idx = torch.arange(0, a.shape[0], NL.STEP)
        ref, M = NL.formula(a[idx], v[idx], NL.SNRS_DB, NL.amplitudes(a, v))
        r = NL.worst(NL.direct_fp32(a, v, mutant=mutant, index=idx), ref, NL.limit(M))
        print(f"{key} {mutant}: {r:.3g} of the limit")
        assert r > 1.0, (key, mutant, r)


def test_silent_tracks():
    """A zero noise track gives c1 * a (c2 = 0, nothing non-finite); a zero clean track gives exactly 0."""
    a = NL.seeded_track(5003, 1)
    z = torch.zeros_like(a)
    got = NL.direct_fp32(a, z)
    ref, M = NL.formula(a, z)
    assert torch.isfinite(got).all() and NL.worst(got, ref, NL.limit(M)) <= 1.0
    assert torch.equal(ref, torch.stack([(1 - NL.factor(s)) * a.double() for s in NL.SNRS_DB]))
    assert NL.direct_fp32(z, a).abs().max() == 0
