"""svt_resample on the GPU (csrc/resample.hip): every output element against the fp64 sum over the fp32 filter table under the limit of
tests/resample_limit.py (a bound derived from the roundings, held by a correct fp32 evaluation and by the reference's own outputs and
missed by the mutants of tests/test_resample_limit.py), with unaligned rows, padded row pitches, poisoned gaps on BOTH sides (a NaN next to
the input would reach a sum if the kernel read outside [0, n_in)), the argument checks, bitwise reproducibility, the reference's outputs
recorded in tests/golden/resample.pt, and the Python layer up to SongTranscriber.transcribe(song, sample_rate=...).

Lengths at 44.1 -> 16 kHz (P = 160, S = 441, a tile of G = 7 units = 3 087 inputs = 1 120 outputs): 1 and 3 (fewer samples than taps), 440 /
441 / 442 (one unit: the tick rule drops the closing output at 441), one tile's span - 1 / + 0 / + 1 (the second workgroup appears at + 1, with
one output) and 88 237 (29 tiles, a ragged last one).  The other five ratios at 5 003 samples: P = 1, P > S, the largest table."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import resample_limit as RL  # noqa: E402
import svt_speechbrain_amd as S  # noqa: E402
from svt_speechbrain_amd import _lib, resample as R, weights as Wt  # noqa: E402
from svt_speechbrain_amd.config import PRESETS  # noqa: E402

DEV = "cuda:0"
POISON = 0x7FC0DEAD   # a NaN with a payload: a write of any value, NaN included, changes the bits
GUARD = 64
INVALID = -1
MAIN = (44100, 16000)
TILE_IN = R.units_per_tile(160, 34, 441) * 441
LENGTHS = (1, 3, 440, 441, 442, TILE_IN - 1, TILE_IN, TILE_IN + 1, 88237)

_tables = {}


def table(ratio):
    """(first, weights, S) on the CPU and on the GPU, built once (tests/test_resample_limit.py holds the CPU table to the reference's bits)."""
    if ratio not in _tables:
        first, weights, S_ = S.resample_table(*ratio)
        _tables[ratio] = (first, weights, S_, first.to(DEV), weights.contiguous().to(DEV))
    return _tables[ratio]


def resample(x, ratio, downmix=False, off=(1, 2), pad=(5, 3), expect=0, **over):
    """One svt_resample call through the C ABI.  x (rows, n_in) is copied into a NaN-filled buffer, rows n_in + pad[0] apart, the first
    one GUARD + off[0] floats behind a fresh allocation; the output rows are n_out + pad[1] apart, GUARD + off[1] floats behind another,
    in a buffer filled with POISON.  over: arguments passed instead of the true ones (the refusals).  Returns (rows (rows_out, n_out), the
    whole output buffer as int32, a mask of the elements the call may write)."""
    lib = _lib.load()
    first, weights, S_, first_d, weights_d = table(ratio)
    P, W = weights.shape
    rows, n_in = x.shape
    rows_out = rows // 2 if downmix else rows
    n_out = RL.tick_rule(n_in, P, S_)
    ld_in, ld_out = n_in + pad[0], n_out + pad[1]
    src = torch.full((GUARD + off[0] + rows * ld_in + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    src[GUARD + off[0]:GUARD + off[0] + rows * ld_in].view(rows, ld_in)[:, :n_in] = x.to(DEV)
    out = torch.full((GUARD + off[1] + max(rows_out, 1) * ld_out + GUARD,), POISON, dtype=torch.int32, device=DEV)
    lo = GUARD + off[1]
    a = dict(in_ptr=_lib.ptr(src) + 4 * (GUARD + off[0]), rows=rows, n_in=n_in, ld_in=ld_in, w_ptr=_lib.ptr(weights_d), f_ptr=_lib.ptr(first_d),
             P=P, W=W, S=S_, out_ptr=_lib.ptr(out) + 4 * lo, n_out=n_out, ld_out=ld_out, downmix=int(downmix))
    a.update(over)
    rc = lib.svt_resample(a["in_ptr"], a["rows"], a["n_in"], a["ld_in"], a["w_ptr"], a["f_ptr"], a["P"], a["W"], a["S"], a["out_ptr"],
                          a["n_out"], a["ld_out"], a["downmix"], 0, _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert rc == expect, (rc, _lib.last_error())
    may = torch.zeros(out.shape, dtype=torch.bool, device=DEV)
    may[lo:lo + rows_out * ld_out].view(rows_out, ld_out)[:, :n_out] = True
    got = out[lo:lo + rows_out * ld_out].view(rows_out, ld_out)[:, :n_out].view(torch.float32)
    return got, out, may


def untouched(out, may):
    return bool((out[~may] == POISON).all())


_cache = {}


def case(ratio, n, rows=2):
    """(x, exact fp64 sum, magnitude sum M) of a ratio, a length and a row count, computed once and never changed."""
    key = (ratio, n, rows)
    if key not in _cache:
        first, weights, S_ = table(ratio)[:3]
        x = RL.seeded_input(rows, n, 300 + n % 89 + rows)
        want, M = RL.exact(x, first, weights, S_, RL.tick_rule(n, weights.shape[0], S_))
        _cache[key] = (x, want, M)
    return _cache[key]


def check(got, want, M, W, downmix=False):
    if downmix:
        want, M = RL.downmix_exact(want, M)
    assert got.shape == want.shape
    return RL.worst(got.cpu(), want, RL.downmix_limit(M, W) if downmix else RL.limit(M, W))


@pytest.mark.parametrize("downmix", (False, True))
@pytest.mark.parametrize("n", LENGTHS)
def test_every_element_inside_the_limit(n, downmix):
    x, want, M = case(MAIN, n)
    got, out, may = resample(x, MAIN, downmix)
    r = check(got, want, M, 34, downmix)
    print(f"44100 -> 16000, n = {n} -> {got.shape[1]}{' downmix' if downmix else ''}: worst error {r:.3f} of the limit")
    assert r <= 1.0, (n, r)
    assert untouched(out, may)


def test_441_samples_give_160_outputs():
    assert [case(MAIN, n)[1].shape[1] for n in (440, 441, 442, TILE_IN, TILE_IN + 1)] == [160, 160, 161, 1120, 1121]


@pytest.mark.parametrize("downmix", (False, True))
@pytest.mark.parametrize("ratio", RL.RATIOS[1:])
def test_the_other_ratios(ratio, downmix):
    x, want, M = case(ratio, 5003)
    got, out, may = resample(x, ratio, downmix)
    r = check(got, want, M, table(ratio)[1].shape[1], downmix)
    print(f"{ratio[0]} -> {ratio[1]}, n = 5003 -> {got.shape[1]}{' downmix' if downmix else ''}: worst error {r:.3f} of the limit")
    assert r <= 1.0, (ratio, r)
    assert untouched(out, may)


@pytest.mark.parametrize("downmix", (False, True))
def test_more_tiles_than_workgroups(downmix):
    """16 -> 16.8 kHz (a tile of 49 units = 980 inputs = 1 029 outputs), 4 rows of 400 000 samples: 4 x 409 (row, tile) pairs (2 x 409 with
    the downmix), more than the grid's MAX_WORKGROUPS, so workgroups go on to a second tile with the table they staged for the first."""
    ratio, n, rows = (16000, 16800), 400000, 4
    P, W_ = table(ratio)[1].shape
    G = R.units_per_tile(P, W_, 20, downmix)
    x, want, M = case(ratio, n, rows)
    tiles = -(-want.shape[1] // (G * P))
    assert (G, tiles) == (49, 409) and R.MAX_WORKGROUPS < tiles * rows // 2 < 2 * R.MAX_WORKGROUPS
    got, out, may = resample(x, ratio, downmix)
    r = check(got, want, M, W_, downmix)
    print(f"16000 -> 16800, {rows} x {n} -> {got.shape[1]}{' downmix' if downmix else ''}: worst error {r:.3f} of the limit")
    assert r <= 1.0
    assert untouched(out, may)


@pytest.mark.parametrize("rows,downmix", ((1, False), (2, False), (3, False), (2, True), (4, True)))
def test_rows_and_channel_pairs(rows, downmix):
    x, want, M = case(MAIN, TILE_IN + 1, rows)
    got, out, may = resample(x, MAIN, downmix)
    assert got.shape[0] == (rows // 2 if downmix else rows)
    assert check(got, want, M, 34, downmix) <= 1.0
    assert untouched(out, may)


@pytest.mark.parametrize("off", ((0, 0), (1, 1), (2, 3), (3, 1), (3, 2)))
@pytest.mark.parametrize("downmix", (False, True))
def test_unaligned_rows_and_padded_pitches(off, downmix):
    """Input and output each 0-3 floats off a fresh allocation, rows n_in + 5 and n_out + 3 apart: the gaps between the output rows and the
    guards around them come back bit for bit, and the NaNs around the input rows reach no sum."""
    x, want, M = case(MAIN, TILE_IN + 1)
    got, out, may = resample(x, MAIN, downmix, off=off)
    assert (_lib.ptr(out) + 4 * (GUARD + off[1])) % 16 == 4 * off[1] % 16
    assert bool(torch.isfinite(got).all())
    assert check(got, want, M, 34, downmix) <= 1.0
    assert untouched(out, may)


@pytest.mark.parametrize("downmix", (False, True))
def test_two_calls_give_the_same_bits(downmix):
    x = case(MAIN, 88237)[0]
    r1 = resample(x, MAIN, downmix)[0]
    r2 = resample(x, MAIN, downmix)[0]
    assert torch.equal(r1.view(torch.int32), r2.view(torch.int32))


def test_refusals_write_nothing():
    x = case(MAIN, 442)[0]
    x3 = case(MAIN, TILE_IN + 1, 3)[0]
    first_d, weights_d = table(MAIN)[3:]
    refusals = [(x, dict(n_in=0)), (x, dict(rows=0)),                          # empty input
                (x, dict(P=20000)),                                          # a table of 20 000 x 35 words: over the LDS cap
                (x3, dict(downmix=1)),                                       # channel pairs: an odd number of rows
                (x, dict(ld_in=441)), (x, dict(ld_out=160)),                 # a pitch below the row's length
                (x, dict(n_out=160)), (x, dict(n_out=162)),                  # not the tick rule's value (161)
                (x, dict(P=441)),                                            # P == S: equal rates
                (x, dict(w_ptr=_lib.ptr(weights_d) + 2)), (x, dict(f_ptr=_lib.ptr(first_d) + 2)),
                (x, dict(w_ptr=None)), (x, dict(f_ptr=None)), (x, dict(in_ptr=None)), (x, dict(out_ptr=None))]
    for xx, over in refusals:
        got, out, may = resample(xx, MAIN, expect=INVALID, **over)
        assert bool((out == POISON).all()), over
        assert _lib.last_error().startswith("svt_resample"), (over, _lib.last_error())
    # in / out two bytes off: the pointers are made here, the call must refuse them before anything runs
    for key in ("in_ptr", "out_ptr"):
        probe = torch.full((2048,), POISON, dtype=torch.int32, device=DEV)
        over = {key: _lib.ptr(probe) + 2}
        got, out, may = resample(x, MAIN, expect=INVALID, **over)
        assert bool((out == POISON).all()) and bool((probe == POISON).all()), key
        assert _lib.last_error().startswith("svt_resample")


def test_fixture_outputs_of_the_reference():
    """Every (ratio, length) of tests/golden/resample.pt: the kernel's output is within (1 + ref_vs_fp64) limit of what the reference's
    Resample.forward returned -- its own distance from the exact sum, read from the fixture, added by the triangle inequality -- and the
    downmix within the same of the mean of the reference's two rows."""
    fx = RL.load_fixture()
    for ratio in RL.RATIOS:
        t = fx["tables"][ratio]
        first, weights, S_ = table(ratio)[:3]
        for n in RL.LENGTHS:
            rec = t["cases"][n]
            x = RL.seeded_input(2, n, rec["seed"])
            assert RL.sha256(x) == rec["sha256"]
            _, M = RL.exact(x, first, weights, S_, rec["out"].shape[1])
            got = resample(x, ratio)[0]
            r = RL.worst(got.cpu(), rec["out"].double(), (1 + rec["ref_vs_fp64"]) * RL.limit(M, t["W"]))
            assert r <= 1.0, (ratio, n, r, rec["ref_vs_fp64"])
            # the mean of the reference's rows: both rows are within ref_vs_fp64 of their limits, and limit_0 + limit_1 over two <= the
            # downmix limit; the reference's own addition costs at most one more unit of it
            got = resample(x, ratio, downmix=True)[0]
            M2 = RL.downmix_exact(M, M)[1]
            r = RL.worst(got.cpu(), rec["out"].double().mean(dim=0, keepdim=True), (2 + rec["ref_vs_fp64"]) * RL.downmix_limit(M2, t["W"]))
            assert r <= 1.0, (ratio, n, r)


def test_resample_module_shapes_and_limit():
    x, want, M = case(MAIN, TILE_IN + 1, 4)
    rs = S.Resample(44100, 16000)
    y = rs(x.to(DEV))                                              # [batch, time]
    assert y.shape == want.shape and y.dtype == torch.float32 and y.is_cuda and RL.worst(y.cpu(), want, RL.limit(M, 34)) <= 1.0
    x3 = x.view(2, 2, -1).transpose(1, 2).contiguous()             # [batch, time, channels]: batch b, channel c is row 2 b + c
    y3 = rs(x3.to(DEV))
    assert y3.shape == (2, want.shape[1], 2)
    assert torch.equal(y3.transpose(1, 2).reshape(4, -1), y)
    assert len(rs._tables) == 1 and rs(x.to(DEV)) is not None and len(rs._tables) == 1    # one upload per device
    same = S.Resample(16000, 16000)
    xd = x.to(DEV)
    assert same(xd) is xd
    with pytest.raises(ValueError):
        rs(xd[0])


def test_resample_to_mono():
    x, want, M = case(MAIN, TILE_IN + 1)
    xd = x.to(DEV)
    mono = S.resample_to_mono(xd, 44100)
    want2, M2 = RL.downmix_exact(want, M)
    assert mono.shape == (want.shape[1],) and mono.is_cuda and RL.worst(mono.cpu()[None], want2, RL.downmix_limit(M2, 34)) <= 1.0
    # Resample followed by the mean: the same two fp32 sums, added and halved -- the same bits
    assert torch.equal(mono, S.Resample(44100, 16000)(xd).mean(dim=0))
    one = S.resample_to_mono(xd[0], 44100)
    assert torch.equal(one, S.resample_to_mono(xd[:1], 44100)) and RL.worst(one.cpu()[None], want[:1], RL.limit(M[:1], 34)) <= 1.0
    assert S.resample_to_mono(xd[0], 16000).data_ptr() == xd.data_ptr()
    assert torch.equal(S.resample_to_mono(xd, 16000), xd.mean(dim=0))


def test_speed_perturb_makes_the_reference_draws():
    """Seeded alike, the module picks the speed the same draws dictate: torch.rand(1) against perturb_prob, then torch.randint."""
    speeds = [95, 100, 105]
    sp = S.SpeedPerturb(16000, speeds=speeds)
    x = case((16000, 15200), 5003)[0].to(DEV)
    torch.manual_seed(1234)
    lengths, picks = [], []
    for _ in range(6):
        y = sp(x)
        lengths.append(y.shape[1])
        picks.append(int(sp.samp_index))
    torch.manual_seed(1234)
    want = []
    for _ in range(6):
        assert not bool(torch.rand(1) > 1.0)
        want.append(int(torch.randint(len(speeds), (1,))[0]))
    assert picks == want and len(set(picks)) == 3
    assert lengths == [R.output_samples(5003, 16000, 16000 * speeds[k] // 100) if speeds[k] != 100 else 5003 for k in want]
    x_, want_, M_ = case((16000, 15200), 5003)
    torch.manual_seed(1234)
    k = want.index(0)
    for _ in range(k + 1):
        y = sp(x)
    assert RL.worst(y.cpu(), want_, RL.limit(M_, 13)) <= 1.0
    never = S.SpeedPerturb(16000, speeds=speeds, perturb_prob=-1.0)   # rand(1) > -1 always: the early return, a copy
    y = never(x)
    assert torch.equal(y, x) and y.data_ptr() != x.data_ptr()


def test_transcribe_at_a_sample_rate():
    """0.3 s of stereo 44.1 kHz audio: transcribe(song, sample_rate=44100) is transcribe(resample_to_mono(song, 44100)) -- equal notes,
    equal feature bits -- and without the argument nothing changes."""
    cfg = PRESETS["tiny-group"]
    hd = Wt.seeded_head_state_dict(cfg.hidden_size, 20, seed=32)
    enc = S.HuggingFaceWav2Vec2("tiny-group", None, config=cfg, precision="fp32", seed=31).to(DEV)
    head = S.Linear(20, input_size=cfg.hidden_size)
    head.load_state_dict(hd)
    head = head.to(DEV)
    tr = S.SongTranscriber(enc, head, sample_rate=16000, dur_threshold=0.25)
    stereo = RL.seeded_input(2, 13230, 77).to(DEV)
    mono = S.resample_to_mono(stereo, 44100)
    assert mono.shape == (4800,)
    notes, feats = tr.transcribe(stereo, return_feats=True, sample_rate=44100)
    notes2, feats2 = tr.transcribe(mono, return_feats=True)
    assert notes == notes2 and torch.equal(feats, feats2) and feats.shape[0] > 0
    assert tr.transcribe(stereo, sample_rate=44100) == notes
    notes3, feats3 = tr.transcribe(mono, True)                     # positional, as before
    assert notes3 == notes2 and torch.equal(feats3, feats2)
    notes4, feats4 = tr.transcribe(stereo[0], return_feats=True, sample_rate=44100)   # (n,) at a rate
    notes5, feats5 = tr.transcribe(S.resample_to_mono(stereo[0], 44100), return_feats=True)
    assert notes4 == notes5 and torch.equal(feats4, feats5)
    with pytest.raises(ValueError):
        tr.transcribe(stereo)                                      # two rows and no rate: refused, as ever
