"""svt_drop_freq_chunk on the GPU (csrc/drop_freq_chunk.hip) and the modules over it (svt_speechbrain_amd/augment.py): every filtered
element against the fp64 correlation under the limit of tests/augment_limit.py (a bound derived from the roundings, held by a correct fp32
evaluation and by the reference's own outputs and missed by the mutants of tests/test_augment_limit.py), dropped spans exactly, with
unaligned rows, padded row pitches, poisoned gaps on BOTH sides of every row (a NaN next to the input would reach a sum if the kernel read
outside [0, n)), the argument checks, bitwise reproducibility, and the reference's outputs recorded in tests/golden/augment.pt.

Lengths against the tile of SVT_DROP_TILE_OUTPUTS = 1024 outputs and the 101 taps (a halo of 50): 3, 50 and 51 (shorter than the halo, the
halo, one more), 101, 441, 1023 / 1025 (the second workgroup appears at 1025, with one output) and 2051 (three tiles, a ragged last one)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import augment_limit as AL  # noqa: E402
import svt_speechbrain_amd as S  # noqa: E402
from svt_speechbrain_amd import _lib, augment as A  # noqa: E402

DEV = "cuda:0"
POISON = 0x7FC0DEAD   # a NaN with a payload: a write of any value, NaN included, changes the bits
GUARD = 64
INVALID = -1
TILE = A.TILE_OUTPUTS
LENGTHS = (3, 50, 51, 101, 441, TILE - 1, TILE + 1, 2 * TILE + 3)


def call(x, taps=None, table=None, off=(1, 2), pad=(5, 3), expect=0, **over):
    """One svt_drop_freq_chunk call through the C ABI.  x (rows, n) is copied into a NaN-filled buffer, rows n + pad[0] apart, the first
    one GUARD + off[0] floats behind a fresh allocation; the output rows are n + pad[1] apart, GUARD + off[1] floats behind another, in a
    buffer filled with POISON.  taps: (k,) fp32 or None; table: (rows, max_chunks, 2) int64 or None.  over: arguments passed instead of
    the true ones (the refusals).  Returns (rows (rows, n), the whole output buffer as int32, a mask of the elements the call may write)."""
    lib = _lib.load()
    rows, n = x.shape
    ld_in, ld_out = n + pad[0], n + pad[1]
    src = torch.full((GUARD + off[0] + rows * ld_in + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    src[GUARD + off[0]:GUARD + off[0] + rows * ld_in].view(rows, ld_in)[:, :n] = x.to(DEV)
    out = torch.full((GUARD + off[1] + rows * ld_out + GUARD,), POISON, dtype=torch.int32, device=DEV)
    lo = GUARD + off[1]
    f_d = taps.to(DEV).contiguous() if taps is not None else None
    c_d = table.to(DEV).contiguous() if table is not None else None
    a = dict(in_ptr=_lib.ptr(src) + 4 * (GUARD + off[0]), rows=rows, n=n, ld_in=ld_in, f_ptr=_lib.ptr(f_d) if f_d is not None else None,
             n_taps=taps.numel() if taps is not None else 0, c_ptr=_lib.ptr(c_d) if c_d is not None else None,
             max_chunks=table.shape[1] if table is not None else 0, out_ptr=_lib.ptr(out) + 4 * lo, ld_out=ld_out)
    a.update(over)
    rc = lib.svt_drop_freq_chunk(a["in_ptr"], a["rows"], a["n"], a["ld_in"], a["f_ptr"], a["n_taps"], a["c_ptr"], a["max_chunks"], a["out_ptr"],
                                 a["ld_out"], 0, _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert rc == expect, (rc, _lib.last_error())
    may = torch.zeros(out.shape, dtype=torch.bool, device=DEV)
    may[lo:lo + rows * ld_out].view(rows, ld_out)[:, :n] = True
    got = out[lo:lo + rows * ld_out].view(rows, ld_out)[:, :n].view(torch.float32)
    return got, out, may


def untouched(out, may):
    return bool((out[~may] == POISON).all())


def table_of(pairs, max_chunks=None):
    """(rows, max_chunks, 2) int64 of per-row (start, end) lists, as given (no clipping: that is the kernel's), filled up with (0, 0)."""
    most = max_chunks or max(len(p) for p in pairs)
    t = torch.zeros((len(pairs), most, 2), dtype=torch.int64)
    for r, row in enumerate(pairs):
        for j, (s, e) in enumerate(row):
            t[r, j, 0], t[r, j, 1] = s, e
    return t


_cache = {}


def case(n, rows, taps=AL.TAPS):
    """(x, f, exact fp64 correlation, limit) of a length, a row count and a tap count, computed once and never changed."""
    key = (n, rows, taps)
    if key not in _cache:
        x = AL.seeded_input(rows, n, 600 + n % 89 + rows)
        f = AL.dense_taps(taps, 50 + taps)
        want, M = AL.exact(x, f)
        _cache[key] = (x, f, want, AL.limit(M, taps))
    return _cache[key]


@pytest.mark.parametrize("n", LENGTHS)
def test_fir_dense_taps_inside_the_limit(n):
    rows = 1 + LENGTHS.index(n) % 3
    x, f, want, lim = case(n, rows)
    got, out, may = call(x, f)
    r = AL.worst(got.cpu(), want, lim)
    print(f"101 dense taps, {rows} x {n}: worst error {r:.4f} of the limit")
    assert r <= 1.0, (n, r)
    assert untouched(out, may)


@pytest.mark.parametrize("taps", (1, 5))
@pytest.mark.parametrize("n", LENGTHS)
def test_fir_short_filters(n, taps):
    x, f, want, lim = case(n, 2, taps)
    got, out, may = call(x, f)
    r = AL.worst(got.cpu(), want, lim)
    print(f"{taps} dense taps, 2 x {n}: worst error {r:.4f} of the limit")
    assert r <= 1.0, (n, taps, r)
    assert untouched(out, may)


def test_fir_the_longest_filter():
    x, f, want, lim = case(2 * TILE + 3, 2, A.MAX_TAPS)
    got, out, may = call(x, f)
    r = AL.worst(got.cpu(), want, lim)
    print(f"{A.MAX_TAPS} dense taps, 2 x {2 * TILE + 3}: worst error {r:.4f} of the limit")
    assert r <= 1.0
    assert untouched(out, may)


@pytest.mark.parametrize("off", ((0, 0), (1, 1), (2, 3), (3, 1), (3, 2)))
def test_fir_unaligned_rows_and_padded_pitches(off):
    x, f, want, lim = case(2 * TILE + 3, 3)
    got, out, may = call(x, f, off=off)
    assert (_lib.ptr(out) + 4 * (GUARD + off[1])) % 16 == 4 * off[1] % 16
    assert bool(torch.isfinite(got).all())
    assert AL.worst(got.cpu(), want, lim) <= 1.0
    assert untouched(out, may)


@pytest.mark.parametrize("n", LENGTHS)
def test_fir_delta_filter_returns_the_input(n):
    x = case(n, 2)[0]
    f = torch.zeros(AL.TAPS)
    f[AL.TAPS // 2] = 1
    got, out, may = call(x, f)
    assert torch.equal(got.cpu(), x)
    assert untouched(out, may)


def test_fir_two_calls_give_the_same_bits():
    x, f = case(2 * TILE + 3, 3)[:2]
    r1 = call(x, f)[0]
    r2 = call(x, f)[0]
    assert torch.equal(r1.view(torch.int32), r2.view(torch.int32))


# rows of 2 * TILE + 3 samples: a span across a tile boundary, one ending exactly on one, two overlapping, one with end > n, an empty and
# a reversed one, one covering the whole row (its middle tile lies wholly inside it: the kernel's shortcut), a row with no chunks
N_CHUNK = 2 * TILE + 3
CHUNK_ROWS = [[(TILE - 7, TILE + 9)],
              [(TILE - 30, TILE)],
              [(100, 300), (250, 400)],
              [(2 * TILE - 5, N_CHUNK + 100)],
              [(500, 500), (900, 700)],
              [(0, N_CHUNK)],
              [],
              [(5, 9), (TILE, 2 * TILE), (2 * TILE + 1, 2 * TILE + 2), (-4, 2), (40, 41), (N_CHUNK - 1, N_CHUNK)]]   # max_chunks of them


def test_chunks_alone():
    x = AL.seeded_input(len(CHUNK_ROWS), N_CHUNK, 77)
    mask = AL.chunk_mask(CHUNK_ROWS, *x.shape)
    assert bool(mask[5].all()) and not bool(mask[6].any()) and bool(mask[0, TILE - 7:TILE + 9].all()) and int(mask[0].sum()) == 16
    got, out, may = call(x, None, table_of(CHUNK_ROWS))
    got = got.cpu()
    assert torch.equal(got[~mask].view(torch.int32), x[~mask].view(torch.int32))     # bit for bit
    assert torch.equal(got[mask].view(torch.int32), torch.zeros(int(mask.sum()), dtype=torch.int32))   # +0.0 exactly
    assert untouched(out, may)


@pytest.mark.parametrize("n", (3, 441, TILE - 1, TILE + 1))
def test_chunks_alone_short_rows(n):
    pairs = [[(1, 2)], [], [(0, n + 5)]]
    x = AL.seeded_input(3, n, 78)
    mask = AL.chunk_mask(pairs, 3, n)
    got, out, may = call(x, None, table_of(pairs))
    assert torch.equal(got.cpu(), torch.where(mask, torch.zeros(()), x))
    assert untouched(out, may)


def test_more_chunks_than_one_batch():
    """300 chunks per row: the kernel takes a row's table 256 pairs at a time."""
    n = TILE + 1
    pairs = [[(3 * j, 3 * j + 1) for j in range(300)], [(n - 2 - j, n - 1 - j) for j in range(0, 600, 2)]]
    x = AL.seeded_input(2, n, 79)
    mask = AL.chunk_mask(pairs, 2, n)
    got, out, may = call(x, None, table_of(pairs))
    assert torch.equal(got.cpu(), torch.where(mask, torch.zeros(()), x))
    assert untouched(out, may)


def test_both_together_with_nans_inside_the_spans():
    """Filter and chunks in one call; NaN samples at least 50 samples inside a dropped span reach no output outside it, and inside it the
    output is written as zero."""
    x, f, _, _ = case(N_CHUNK, len(CHUNK_ROWS))
    x = x.clone()
    mask = AL.chunk_mask(CHUNK_ROWS, *x.shape)
    nans = [(2, 175), (2, 330), (5, 0), (5, 1000), (5, N_CHUNK - 1), (7, TILE + 50), (7, TILE + 512), (7, 2 * TILE - 51)]
    for r, t in nans:
        assert bool(mask[r, max(0, t - 50):t + 51].all())
        x[r, t] = float("nan")
    clean = torch.where(torch.isnan(x), torch.zeros(()), x)
    want, M = AL.exact(clean, f)
    want = torch.where(mask, torch.zeros((), dtype=torch.float64), want)
    got, out, may = call(x, f, table_of(CHUNK_ROWS))
    got = got.cpu()
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got[mask].view(torch.int32), torch.zeros(int(mask.sum()), dtype=torch.int32))
    r = AL.worst(got[~mask], want[~mask], AL.limit(M, AL.TAPS)[~mask])
    print(f"filter and chunks, {len(CHUNK_ROWS)} x {N_CHUNK}: worst error {r:.4f} of the limit outside the spans")
    assert r <= 1.0
    assert untouched(out, may)


def test_more_rows_than_workgroups():
    """MAX_WORKGROUPS + 3 rows of one tile each: the grid is cut to half as many workgroups, which go on to a second job.  Five taps:
    the job loop is under test here, the long filter above."""
    rows = A.MAX_WORKGROUPS + 3
    x, f, want, lim = case(TILE, rows, 5)
    pairs = [[(r % TILE, r % TILE + 3)] if r % 2 else [] for r in range(rows)]
    mask = AL.chunk_mask(pairs, rows, TILE)
    got, out, may = call(x, f, table_of(pairs))
    got = got.cpu()
    assert bool((got[mask] == 0).all())
    assert AL.worst(got[~mask], want[~mask], lim[~mask]) <= 1.0
    assert untouched(out, may)
    # and without a filter: the copy path's job loop
    got, out, may = call(x, None, table_of(pairs))
    assert torch.equal(got.cpu(), torch.where(mask, torch.zeros(()), x))
    assert untouched(out, may)


def test_refusals_write_nothing():
    x, f = case(441, 2)[:2]
    table = table_of([[(5, 9)], []])
    f_d, c_d = f.to(DEV), table.to(DEV)
    refusals = [dict(rows=0), dict(n=0),
                dict(n_taps=100), dict(n_taps=A.MAX_TAPS + 2), dict(n_taps=-1),               # even, too long, negative
                dict(n_taps=0), dict(f_ptr=None),                                         # a filter without its count, a count without its filter
                dict(max_chunks=0), dict(c_ptr=None), dict(max_chunks=-1),
                dict(ld_in=440), dict(ld_out=440),
                dict(in_ptr=None), dict(out_ptr=None),
                dict(f_ptr=_lib.ptr(f_d) + 2), dict(c_ptr=_lib.ptr(c_d) + 4)]
    for over in refusals:
        got, out, may = call(x, f, table, expect=INVALID, **over)
        assert bool((out == POISON).all()), over
        assert _lib.last_error().startswith("svt_drop_freq_chunk"), (over, _lib.last_error())
    # in / out two bytes off, and overlapping ranges: the pointers are made here, the call must refuse them before anything runs
    for key in ("in_ptr", "out_ptr"):
        probe = torch.full((2048,), POISON, dtype=torch.int32, device=DEV)
        got, out, may = call(x, f, table, expect=INVALID, **{key: _lib.ptr(probe) + 2})
        assert bool((out == POISON).all()) and bool((probe == POISON).all()), key
        assert _lib.last_error().startswith("svt_drop_freq_chunk")
    probe = torch.full((4096,), POISON, dtype=torch.int32, device=DEV)
    rows, n = x.shape
    extent = 4 * ((rows - 1) * (n + 5) + n)               # bytes of the input's rows at call()'s pitch
    for in_off, out_off in ((0, 0), (0, extent - 4), (4 * 500, 0)):
        got, out, may = call(x, f, table, expect=INVALID, in_ptr=_lib.ptr(probe) + in_off, out_ptr=_lib.ptr(probe) + out_off)
        assert bool((probe == POISON).all()), (in_off, out_off)
        assert "overlap" in _lib.last_error() and _lib.last_error().startswith("svt_drop_freq_chunk")
    # ranges that touch without overlapping are taken
    ok = torch.zeros((8192,), dtype=torch.float32, device=DEV)
    got, out, may = call(x, f, table, in_ptr=_lib.ptr(ok), out_ptr=_lib.ptr(ok) + extent)


# ---- the modules against the reference's recorded outputs ----

@pytest.fixture(scope="module")
def fx():
    return AL.load_fixture()


def run_case(name, device_lengths=False):
    kind, kwargs, shape, lengths, seed = AL.CASES[name]
    module = getattr(S, kind)(**kwargs)
    x = AL.case_input(name).to(DEV)
    torch.manual_seed(seed)
    if lengths is None:
        y = module(x)
    else:
        ln = AL.case_lengths(name)
        y = module(x, ln.to(DEV) if device_lengths else ln)
    return module, x, y, AL.rng_digest()


@pytest.mark.parametrize("name", ("drop_freq_1", "drop_freq_2"))
def test_drop_freq_module_against_the_fixture(fx, name):
    rec = fx["cases"][name]
    module, x, y, rng = run_case(name)
    assert rng == rec["rng"] and torch.equal(module.frequencies, rec["frequencies"])
    assert y.shape == rec["out"].shape and y.is_cuda and y.dtype == torch.float32
    _, M = AL.exact(x.cpu(), rec["filter"])
    r = AL.worst(y.cpu(), rec["out"].double(), (1 + rec["ref_vs_fp64"]) * AL.limit(M, AL.TAPS))
    print(f"{name}: {r:.4f} of (1 + {rec['ref_vs_fp64']:.3f}) limit from the reference's output")
    assert r <= 1.0


@pytest.mark.parametrize("device_lengths", (False, True))
@pytest.mark.parametrize("name", ("drop_chunk", "drop_chunk_negative"))
def test_drop_chunk_module_against_the_fixture(fx, name, device_lengths):
    rec = fx["cases"][name]
    module, x, y, rng = run_case(name, device_lengths)
    assert rng == rec["rng"] and module.chunks == rec["chunks"]
    assert torch.equal(y.cpu(), rec["out"])
    assert torch.equal(x.cpu(), AL.case_input(name))      # the input is left alone


def test_drop_chunk_keeps_a_channel_axis(fx):
    rec = fx["cases"]["drop_chunk"]
    module = S.DropChunk()
    x = AL.case_input("drop_chunk").to(DEV).unsqueeze(-1)
    torch.manual_seed(rec["seed"])
    y = module(x, AL.case_lengths("drop_chunk"))
    assert y.shape == x.shape and torch.equal(y[:, :, 0].cpu(), rec["out"])


def test_lobe_at_speed_100(fx, monkeypatch):
    rec = fx["cases"]["lobe_100"]
    launches = []
    real = A._launch
    monkeypatch.setattr(A, "_launch", lambda *a: launches.append(a) or real(*a))
    module, x, y, rng = run_case("lobe_100")
    assert rng == rec["rng"]
    assert len(launches) == 1 and launches[0][1] is not None and launches[0][2] is not None     # ONE launch, filter and chunks in it
    assert module.drop_chunk.chunks == rec["chunks"] and torch.equal(module.drop_freq.frequencies, rec["frequencies"])
    y = y.cpu()
    assert y.shape == rec["out"].shape
    mask = AL.chunk_mask(rec["chunks"], *y.shape)
    assert torch.equal(y == 0, rec["out"] == 0) and torch.equal(y == 0, mask)
    _, M = AL.exact(x.cpu(), rec["filter"])
    r = AL.worst(y[~mask], rec["out"].double()[~mask], ((1 + rec["ref_vs_fp64"]) * AL.limit(M, AL.TAPS))[~mask])
    print(f"lobe, speeds = [100]: {r:.4f} of (1 + {rec['ref_vs_fp64']:.3f}) limit from the reference's output")
    assert r <= 1.0


def test_lobe_with_speed_perturbation(fx):
    rec = fx["cases"]["lobe_speeds"]
    module, x, y, rng = run_case("lobe_speeds", device_lengths=True)
    assert rng == rec["rng"]
    assert int(module.speed_perturb.samp_index) == rec["speed"]
    y = y.cpu()
    assert y.shape == rec["out"].shape and y.shape[1] != x.shape[1]
    assert module.drop_chunk.chunks == rec["chunks"]
    mask = AL.chunk_mask(rec["chunks"], *y.shape)
    assert torch.equal(y == 0, rec["out"] == 0) and torch.equal(y == 0, mask)
    # the filter step against fp64 on the product's OWN SpeedPerturb output (the resampler has its test: tests/test_gpu_resample.py)
    taps = module.drop_freq.filter
    # both filters against the fp64 build: the reference's at filter_vs_fp64, this one at up to twice that (tests/test_augment_limit.py)
    assert (taps - rec["filter"]).abs().max().item() <= 3 * rec["filter_vs_fp64"]
    want, M = AL.exact(module.perturbed.cpu(), taps)
    r = AL.worst(y[~mask], want[~mask], AL.limit(M, AL.TAPS)[~mask])
    print(f"lobe, speeds = [95, 100, 105]: {r:.4f} of the limit on its own SpeedPerturb output")
    assert r <= 1.0


def test_no_op_paths_launch_nothing(monkeypatch):
    launches = []
    real = A._launch
    monkeypatch.setattr(A, "_launch", lambda *a: launches.append(a) or real(*a))
    x = AL.seeded_input(2, 700, 5).to(DEV)
    keep = x.clone()
    ones = torch.ones(2)
    modules = [(S.DropFreq(drop_prob=0), ()), (S.DropFreq(drop_count_low=0, drop_count_high=0), ()),
               (S.DropChunk(drop_prob=0), (ones,)), (S.DropChunk(drop_count_low=0, drop_count_high=0), (ones,)),
               (S.TimeDomainSpecAugment(speeds=[100], drop_freq_prob=0, drop_chunk_prob=0), (ones,)),
               (S.TimeDomainSpecAugment(speeds=[100], drop_freq_count_high=0, drop_chunk_count_high=0), (ones,)),
               (S.TimeDomainSpecAugment(perturb_prob=0, drop_freq_prob=0, drop_chunk_prob=0), (ones,))]
    torch.manual_seed(8)     # rand(1) > 0 always but for an exact 0.0
    for module, args in modules:
        y = module(x, *args)
        assert torch.equal(y, keep) and y.data_ptr() != x.data_ptr() and torch.equal(x, keep), module
    assert launches == []
    S.DropChunk()(x, ones)
    assert len(launches) == 1


def test_error_paths():
    with pytest.raises(NotImplementedError):
        S.DropChunk(noise_factor=0.5)
    x = torch.zeros(2, 300)
    with pytest.raises(_lib.SvtError):
        S.DropFreq()(x)
    with pytest.raises(_lib.SvtError):
        S.DropChunk()(x, torch.ones(2))
    with pytest.raises(_lib.SvtError):
        S.TimeDomainSpecAugment()(x, torch.ones(2))
    x3 = torch.zeros(2, 300, 3, device=DEV)
    for module, args in ((S.DropFreq(), ()), (S.DropChunk(), (torch.ones(2),)), (S.TimeDomainSpecAugment(), (torch.ones(2),))):
        before = AL.rng_digest()
        with pytest.raises(ValueError):
            module(x3, *args)
        assert AL.rng_digest() == before     # refused before anything is drawn
