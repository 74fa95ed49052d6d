"""CPU test of the per-element limit that tests/test_gpu_gemm_kernels.py holds the 16-bit GEMM kernels to (tests/gemm_limit.py): a correct
kernel, simulated -- fp32 accumulation in 32-wide K chunks, fp32 activation, one round-to-nearest store -- stays inside it on every case
shape in both builds, and the two defects the flat max-abs tolerances let through do not: a 16-bit store that truncates, and one row that
misses one 32-element K block.

The second half does the same for the split-operand kernels (tests/gemm_split.py, tests/test_gpu_gemm_split_kernels.py): a correct simulated
split kernel is bit-equal to the three-term value T on the exact operands and inside the random limit; four mutants fail the exact test, and
the first of them -- one row loses Al Wh of one 32-block -- PASSES the random limit, which is why the exact cases exist; and T itself is
within the mode's documented distance of the fp64 product."""
import pytest
import torch

import gemm_limit as G
import gemm_split as X


def _shapes():
    seen, out = set(), []
    for c in G.CASES:
        key = (c.M, c.N, c.K, c.conv, c.act, c.out_f32, c.resid, c.bias)
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


SHAPES = _shapes()


@pytest.mark.parametrize("build", list(G.BUILDS))
@pytest.mark.parametrize("c", SHAPES, ids=G.case_id)
def test_limit_on_a_simulated_kernel(c, build):
    dtype = G.BUILDS[build][1]
    inp, z, S, ref = G.case_data(c, build)
    lim = G.limit(c, build, z, S, ref, inp["resid"])
    ok, where = G.worst(c, G.simulate(c, inp, dtype).double(), ref, lim)
    print(f"[{build}] {G.case_id(c)}: correct kernel {ok:.3f} at {where}")
    assert ok <= 1.0, (ok, where)
    row = c.M - 1                                                      # (a tail row: the one a wrong M-tail clamp would hit)
    short, where = G.worst(c, G.simulate(c, inp, dtype, drop=(row, (c.K // 32) // 2)).double(), ref, lim)
    print(f"[{build}] {G.case_id(c)}: row {row} without one K block {short:.3g}")
    assert short > 1.0, "a row that misses 32 of its K products passes the limit"
    if not c.out_f32:
        trunc, _ = G.worst(c, G.simulate(c, inp, dtype, truncate=True).double(), ref, lim)
        print(f"[{build}] {G.case_id(c)}: truncating store {trunc:.3f}")
        assert trunc > 1.0, "a truncating 16-bit store passes the limit"


def test_truncation_helper_truncates():
    x = torch.tensor([1.0 + 2.0 ** -7 + 2.0 ** -9, -(1.0 + 2.0 ** -7 + 2.0 ** -9), 3.0, -0.0, 1.0 + 2.0 ** -10 + 2.0 ** -12])
    assert G.truncate_to(x, torch.bfloat16).float().tolist() == [1.0 + 2.0 ** -7, -(1.0 + 2.0 ** -7), 3.0, -0.0, 1.0]
    assert G.truncate_to(x, torch.float16).float().tolist() == [1.0 + 2.0 ** -7 + 2.0 ** -9, -(1.0 + 2.0 ** -7 + 2.0 ** -9), 3.0, -0.0, 1.0 + 2.0 ** -10]


def test_case_tables_reach_every_kernel_and_both_sides_of_the_thresholds():
    """Removing the only case that reaches a kernel, a tile height or an epilogue fails here."""
    ids = {c.kid for c in G.CASES}
    assert ids >= {1032, 1064, 2128, 2256} | {f * 1000 + bm for f in (3, 4) for bm in (64, 128, 192, 256)} | {f * 1000 + bm for f in (5, 6) for bm in (128, 192, 256)}
    for fam in (5, 6):   # forced and chosen by the dispatcher
        mine = [c for c in G.CASES if c.kid // 1000 == fam]
        assert any(dict(c.keys).get(3) == 70 or dict(c.keys).get(29) == 2 for c in mine) and any(set(dict(c.keys)) <= {1} for c in mine)
    assert {G.gelu_form(c) for c in G.CASES if c.act == 1} == {"fast", "poly"}
    assert {c.kid // 1000 for c in G.GELU_ALONE} == {1, 2, 3, 4, 5, 6}


# ---------------- the split-operand kernels (tests/gemm_split.py) ----------------
@pytest.mark.parametrize("prec,K", [(2, 512), (3, 512), (3, 192), (2, 192)])
def test_split_exact_operands_on_a_simulated_kernel(prec, K):
    """The longest K of the exact tables (IEEE-half pieces: P restricted to +-1 there; K = 192 is the longest with P from +-1, +-2): fp32 accumulation of
    the three piece products in shuffled 32-block order is bit-equal to T, T differs from the fp64 product nearly everywhere, and every mutant is seen."""
    c = X.S(7256, 128, 128, K)
    inp = X.exact_inputs(c, prec)
    exp = X.exact_expected(c, inp, prec)
    rows = inp["rows"].float()
    for seed in (0, 1):
        assert torch.equal(X.simulate(rows, inp["W"], inp["bias"], prec, seed=seed), exp)
    full = inp["rows"] @ inp["W"].double().t() + inp["bias"].double()
    assert (exp.double() != full).float().mean().item() > 0.9, "T equals the fp64 product: the exact operands would not show a fourth term"
    for mutant in X.MUTANTS:
        got = X.simulate(rows, inp["W"], inp["bias"], prec, mutant=mutant)
        assert not torch.equal(got, exp), f"the mutant {mutant} is bit-equal to T on the exact operands"
    # pair / plane output: the cut of T read back is T itself only where T has few enough bits -- the expectation is the emulated cut
    cp = X.S(9128, 128, 256, K, out_kind=1)
    inp = X.exact_inputs(cp, prec)
    exp = X.exact_expected(cp, inp, prec)
    assert torch.equal(X.recombine(X.simulate(inp["rows"].float(), inp["W"], inp["bias"], prec), X.PIECE[prec][0]), exp)


def test_split_exact_operands_refuse_a_k_that_is_too_long():
    X.exact_inputs(X.S(12256, 24, 64, 772), 3)       # P from +-1: 772 (1 + 8 2^-14) 2^14 < 2^24
    with pytest.raises(AssertionError, match="too long"):
        X.exact_inputs(X.S(7256, 128, 128, 1024), 3)
    with pytest.raises(AssertionError, match="too long"):
        X.exact_inputs(X.S(7256, 128, 128, 4096), 2)


@pytest.mark.parametrize("prec", [2, 3])
@pytest.mark.parametrize("K", [64, 192, 768])
def test_split_limit_on_a_simulated_kernel(K, prec):
    """Random operands: the correct simulated kernel stays inside the limit; a lost K block does not.  A single lost term (Al Wh of one
    32-block of one row) PASSES at K = 768 -- the limit's documented blindness."""
    c = X.S(7256, 256, 256, K)
    inp = G.make_inputs(c, torch.float32)
    z, S3, ref = X.reference(c, inp, prec)
    lim = X.limit(c, prec, z, S3, ref, None)
    rows = inp["rows"].float()
    ok, where = X.worst(c, X.simulate(rows, inp["W"], inp["bias"], prec), ref, lim)
    print(f"[prec {prec}] K = {K}: correct kernel {ok:.4f} at {where}")
    assert ok <= 1.0, (ok, where)
    block, _ = X.worst(c, X.simulate(rows, inp["W"], inp["bias"], prec, mutant="lost_block"), ref, lim)
    assert block > 1.0, "a row that misses a whole K block passes the limit"
    term, _ = X.worst(c, X.simulate(rows, inp["W"], inp["bias"], prec, mutant="lost_term"), ref, lim)
    print(f"[prec {prec}] K = {K}: one lost Al Wh term {term:.4f}")
    if K == 768:
        assert term <= 1.0, "the random limit sees a single lost term after all: say so in tests/gemm_split.py"


@pytest.mark.parametrize("prec", [2, 3])
@pytest.mark.parametrize("K", [64, 768])
@pytest.mark.parametrize("wscale", ["sqrtK", 0.02])
def test_split_mode_precision(wscale, K, prec):
    """|T - fp64 product| stays inside X.mode_bound: on U(-1, 1) / sqrt K weights, and on weights scaled to 0.02, every one of which has a
    subnormal IEEE-half lo piece (|w| < 0.125), so that the eta term dominates for that piece type."""
    g = torch.Generator().manual_seed(2)
    A = torch.rand(256, K, generator=g) * 2 - 1
    W = (torch.rand(256, K, generator=g) * 2 - 1) * (K ** -0.5 if wscale == "sqrtK" else wscale)
    T, _ = X.three_term(A, W, prec)
    err = (T - A.double() @ W.double().t()).abs()
    ratio = (err / X.mode_bound(A, W, prec)).max().item()
    print(f"[prec {prec}] K = {K} weights {wscale}: |T - product| / bound {ratio:.3f}")
    assert 0.0 < ratio <= 1.0
    if prec == 3:
        _, wl = X.cut(W, torch.float16)
        assert (wl.float().abs() < 2.0 ** -14).all(), "these weights were meant to have subnormal lo pieces"


def test_split_tables_reach_every_kernel():
    """Removing the only case that reaches a kernel, a tile height, an output form or an epilogue fails here."""
    want = {7256, 7192, 8256, 12128, 12256, 2128, 2256} | {f * 1000 + bm for f in (9, 10) for bm in (128, 192, 256)}
    for table in (X.EXACT, X.RANDOM):
        assert {c.kid for c in table} == want
        for fam in (9, 10):
            assert {(c.kid, c.out_kind) for c in table if c.kid // 1000 == fam} == {(fam * 1000 + bm, ok) for bm in (128, 192, 256) for ok in (0, 1, 2)}
        for fam in (8, 9, 10):   # a workgroup that walks several tiles
            assert any(dict(c.keys).get(37) == 8 for c in table if c.kid // 1000 == fam)
    assert any(c.kid == 8256 and not c.keys for c in X.RANDOM), "gemm_x3p_kernel as the dispatcher's own choice"
    assert any(c.kid // 1000 == 9 and 1 not in dict(c.keys) for c in X.RANDOM), "gemm_x3q_kernel at the cost model's own height"
    assert {c.kid // 1000 for c in X.RANDOM if c.act == 1} >= {2, 7, 8, 9, 10, 12}
    assert {c.kid // 1000 for c in X.ALONE} == {7, 8, 9, 10, 12}
    assert max(c.K for c in X.EXACT if c.kid // 1000 in (7, 8, 9, 10)) == 512
    for c in X.EXACT + X.RANDOM + X.ALONE:
        assert set(dict(c.keys)) <= set(G.KEY_DEFAULTS), c
    assert X.tile_shape(7192) == (256, 192) and X.tile_shape(12128) == (128, 128) and X.tile_shape(10192) == (192, 256)


# ---------------- batched launches and the score-matrix attention (tests/test_gpu_gemm_batched.py, tests/test_gpu_attention_scores.py) ----------------
def _batched_ratio(b, prec, build, dtype, bufs, mutant=None):
    return G.batched_worst(b, prec, build, bufs, lambda z, ci: G.batched_simulate(b, bufs, z, prec, dtype, mutant).double())


@pytest.mark.parametrize("b", G.BATCHED, ids=G.bcase_id)
def test_batched_limit_on_a_simulated_kernel(b):
    """Every z of every batched case: the launch stays inside its buffers, and a correct simulated kernel stays inside the limit."""
    assert G.batched_in_bounds(b), "the case addresses memory outside its buffers"
    _, dtype, prec, tag = G.batched_runs(b)[-1]   # (the IEEE-half build, or the last split precision)
    bufs = G.batched_inputs(b, dtype)
    ok, where = _batched_ratio(b, prec, tag, dtype, bufs)
    print(f"[{tag}] {G.bcase_id(b)}: correct kernel {ok:.3f} at {where}")
    assert ok <= 1.0, (ok, where)


def _bcase(form, precs, alpha=False):
    return next(b for b in G.BATCHED if b.geom.form == form and b.precs == precs and (b.alpha != 1.0) == alpha and b.geom.M < 1000)


@pytest.mark.parametrize("form,precs,alpha,mutant", [("qk", "16", True, "prev_head"), ("qk", (0,), True, "prev_head"),
                                                     ("posconv", "16", False, "no_bias_z2"), ("posconv", (2, 3), False, "no_bias_z2"),
                                                     ("posconv", "16", True, "alpha_last"), ("posconv", (0,), True, "alpha_last"),
                                                     ("posconv", (2, 3), True, "alpha_last")])
def test_batched_mutants_fall_outside_the_limit(form, precs, alpha, mutant):
    """A wrong z stride on the last clip's heads, a dropped bias_z2 and alpha applied after the bias are each seen on a case of the table."""
    b = _bcase(form, precs, alpha)
    for _, dtype, prec, tag in G.batched_runs(b):
        bufs = G.batched_inputs(b, dtype)
        good, _ = _batched_ratio(b, prec, tag, dtype, bufs)
        bad, where = _batched_ratio(b, prec, tag, dtype, bufs, mutant)
        print(f"[{tag}] {G.bcase_id(b)} {mutant}: {bad:.3g} at {where} (correct kernel {good:.3f})")
        assert good <= 1.0 < bad


def test_batched_table_reaches_the_batched_arms():
    """Families 1, 2, 3, 7 and 12 (include/svt_mi355.h, svt_debug_set key 39) each with nz > 1; every form in every precision class it is served in."""
    assert {b.kid // 1000 for b in G.BATCHED if b.geom.nz > 1} >= {1, 2, 3, 7, 12}
    assert {b.kid for b in G.BATCHED} >= {1032, 2128, 2256, 3064, 3192, 7256, 7192, 12128, 12256}
    assert {(b.geom.form, b.precs) for b in G.BATCHED} >= {(f, p) for f in ("posconv", "folded") for p in ("16", (0,), (2, 3))} | {
        ("qk", "16"), ("qk", (0,)), ("pv", "16"), ("pv", (0,))}
    assert any(b.geom.form == "qk" and b.geom.ldc > b.geom.N for b in G.BATCHED) and any(b.geom.form == "qk" and b.geom.ldc == b.geom.N for b in G.BATCHED)
    assert any(b.geom.nz % b.geom.nz2 for b in G.BATCHED) and any(b.alpha != 1.0 and b.bias for b in G.BATCHED)
    for b in G.BATCHED:
        assert set(dict(b.keys)) <= set(G.KEY_DEFAULTS), b


def _attn_ratio(c, prec, tag, dtype, parts, mutant=None):
    x, gate, pb, q, k, v, o, A, delta, spread = parts
    got = G.attn_simulate(c, prec, dtype, q, k, v, gate, pb, mutant).double()
    ratio = (got - o).abs() / G.attn_limit(c, prec, tag if prec == 1 else None, v, o, A, delta, spread)
    return torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio).max().item()


def _attn_parts(c, dtype, prec):
    x, gate, pb = G.attn_inputs(c, dtype)
    q, k, v = (t.reshape(c.B, c.T, c.H, c.dh) for t in x.split(c.H * c.dh, dim=-1))
    o, A = G.attn_reference(q, k, v, G.attn_scale(c.dh), gate, pb)
    return (x, gate, pb, q, k, v, o, A) + G.attn_row_terms(q, k, G.attn_scale(c.dh), gate, pb, prec)


@pytest.mark.parametrize("c", [c for c in G.ATTN if c.layout == "packed"], ids=G.acase_id)
def test_attention_limit_on_a_simulated_pipeline(c):
    for _, dtype, prec, tag in G.attn_runs(c):
        ok = _attn_ratio(c, prec, tag, dtype, _attn_parts(c, dtype, prec))
        print(f"[{tag}] {G.acase_id(c)}: correct pipeline {ok:.3f}")
        assert ok <= 1.0, (tag, ok)


@pytest.mark.parametrize("c,mutant", [(G.AC(2256, 0, 2, 67, 3, 32), "pad_ones"), (G.AC(2256, 0, 2, 9, 2, 64), "pad_ones"), (G.AC(2128, "16", 2, 67, 3, 96), "pad_ones"),
                                      (G.AC(2128, "16", 2, 65, 2, 128, bias=True), "rel_off_by_one"), (G.AC(12256, 3, 2, 65, 3, 64, bias=True), "rel_off_by_one"),
                                      (G.AC(2128, "16", 2, 65, 2, 128, bias=True), "gate_next"), (G.AC(12256, 2, 2, 65, 3, 64, bias=True), "gate_next")],
                         ids=lambda v: G.acase_id(v) if isinstance(v, G.ACase) else v)
def test_attention_mutants_fall_outside_the_limit(c, mutant):
    assert c in G.ATTN, "the mutant is shown on a case the GPU test runs"
    for _, dtype, prec, tag in G.attn_runs(c):
        bad = _attn_ratio(c, prec, tag, dtype, _attn_parts(c, dtype, prec), mutant)
        print(f"[{tag}] {G.acase_id(c)} {mutant}: {bad:.3g}")
        assert bad > 1.0


def test_attention_table_reaches_every_route():
    """fp32: every T % 8 class and both sides of the wave's 64-key stride; 16-bit: head sizes the fused kernels do not serve, and the biased geometries
    they refuse; split modes: WavLM's route; the separate-q layout once per precision; no case is one the fused kernels would take."""
    f32 = [c for c in G.ATTN if c.prec == 0]
    assert {c.T % 8 for c in f32} >= {0, 1, 7} and {c.T for c in f32} >= {1, 63, 64, 65} and any(c.gain == 8.0 for c in f32)
    assert {c.prec for c in G.ATTN if c.layout == "separate"} == {0, "16", 2, 3}
    for c in G.ATTN:
        if c.prec == "16":
            assert c.dh not in (64, 128) or (c.bias and (c.dh == 128 or 2 * c.T - 1 > 8192)), c
        if c.prec in (2, 3):
            assert c.bias or c.layout == "separate"
    assert any(c.prec == "16" and c.dh == 64 and c.bias and 2 * c.T - 1 == 8199 for c in G.ATTN)
