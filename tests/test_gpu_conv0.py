"""GPU tests of each kernel of the waveform front end alone (csrc/stats.hip: moments_kernel, conv0_window_moments_kernel,
conv0_group_coef_kernel; csrc/conv0.hip: conv0_group_apply_kernel, conv0_layer_kernel; csrc/conv0_mfma.hip: conv0_mfma_kernel behind its
table and exponent kernels), in both 16-bit builds, through the C-ABI test hook svt_debug_conv0.

Every case names the kernel and instantiation it is written for (the id svt_debug_set(41, 0) reports, include/svt_mi355.h) and asserts it.
Every output is allocated filled with 0xFF bytes (NaN in every type) between 8 such guard rows in the same allocation; the guards must
come back bit-unchanged and no NaN may be left inside.  Every element is held to the checks tests/conv0_limit.py derives: bit equality
with integer arithmetic for the ordered sums of exact inputs, and limits derived from the number formats and the operation counts for
everything else; tests/test_conv0_limit.py shows on the CPU that a correct kernel passes them and which mutants do not.  The refusals
are decided on the host: each must return SVT_ERR_INVALID and leave the poisoned outputs untouched."""
import ctypes
import dataclasses

import pytest
import torch

import conv0_limit as Z
import gemm_limit as G
import gemm_split as GS

pytestmark = pytest.mark.gpu

from svt_speechbrain_amd import _lib  # noqa: E402

DEV = "cuda:0"
SVT_ERR_INVALID = -1
EPS = 1e-5


class Buf:
    """(rows + 2 GUARD, D) elements of `dtype`, every byte 0xFF: an output between its guard rows."""

    def __init__(self, rows, D, dtype):
        self.rows, self.D = rows, D
        es = torch.empty((), dtype=dtype).element_size()
        raw = torch.full(((rows + 2 * Z.GUARD) * D * es,), 0xFF, dtype=torch.uint8, device=DEV)
        self.t = raw.view(dtype).view(rows + 2 * Z.GUARD, D)
        self.ptr = self.t.data_ptr() + Z.GUARD * D * es
        self.before = raw.clone()

    def guards_intact(self):
        now, n = self.t.view(torch.uint8).flatten(), Z.GUARD * self.D * self.t.element_size()
        return torch.equal(now[:n], self.before[:n]) and torch.equal(now[-n:], self.before[-n:])

    def untouched(self):
        return torch.equal(self.t.view(torch.uint8).flatten(), self.before)

    def rows_cpu(self):
        return self.t[Z.GUARD:Z.GUARD + self.rows].cpu()


def desc(form, **kw):
    d = _lib.Conv0DescC()
    d.struct_size = ctypes.sizeof(d)
    d.form, d.k, d.stride, d.eps_wav, d.eps = form, Z.K0, 5, EPS, EPS
    for n, v in kw.items():
        setattr(d, n, v)
    return d


def dev(t):
    return None if t is None else t.contiguous().to(DEV)


def ptr(t):
    return None if t is None else t.data_ptr()


def launch(lib, d, fenced=0):
    """svt_debug_conv0 under key 32, the key restored.  Returns (rc, kernel id)."""
    try:
        assert lib.svt_debug_set(32, fenced) == 0
        rc = lib.svt_debug_conv0(ctypes.byref(d), 0, torch.cuda.current_stream().cuda_stream)
        kid = lib.svt_debug_set(41, 0)
        torch.cuda.synchronize()
    finally:
        lib.svt_debug_set(32, 0)
    return rc, kid


# ---- forms 0, 1: the ordered sums --------------------------------------------------------------------------------------------------
SUMS = [(c, b) for c in Z.MOMENTS + Z.WINDOWS for b in G.BUILDS]


@pytest.mark.parametrize("c,build", SUMS, ids=[f"{Z.case_id(c)}-{b}" for c, b in SUMS])
def test_ordered_sums(c, build):
    lib = _lib.load(G.BUILDS[build][0])
    form = 0 if isinstance(c, Z.MCase) else 1
    x, ref, lim = (Z.moments_inputs if form == 0 else Z.window_inputs)(c)
    xd = dev(x)
    seen = []
    for fenced, repeat in ((0, 1), (1, 1), (0, 3)):
        out = Buf(c.groups, 2, torch.float64) if form == 0 else Buf(c.B, Z.NWM, torch.float64)   # NaN-filled: the sums are written, not accumulated
        n_t = c.groups_max if form == 0 else c.B
        tickets = (ctypes.c_uint32 * n_t)(*([0xFFFFFFFF] * n_t))
        if form == 0:
            d = desc(0, x=xd.data_ptr(), n=c.n, groups=c.groups, groups_max=c.groups_max, mom=out.ptr)
        else:
            d = desc(1, wav=xd.data_ptr(), B=c.B, L=x.shape[1], stride=c.stride, T1=c.T1, wm=out.ptr)
        d.repeat, d.tickets_out = repeat, ctypes.addressof(tickets)
        rc, kid = launch(lib, d, fenced)
        _lib.check(rc, "svt_debug_conv0", lib)
        assert kid == (Z.K_MOM, Z.K_WIN)[form]
        assert out.guards_intact()
        assert not any(tickets), f"tickets left at {list(tickets)} (key 32 = {fenced}, repeat {repeat})"
        got = out.rows_cpu()
        fails, w = Z.check_sums(got, ref, lim)
        print(f"front end [{build}] kernel {kid} {Z.case_id(c)} key32={fenced} repeat={repeat}: " + ("bit-equal" if lim is None else f"worst err / limit {w:.3g}"))
        assert not fails, (Z.case_id(c), fenced, repeat, fails)
        seen.append(got)
    assert torch.equal(seen[0].view(torch.int64), seen[1].view(torch.int64)), "the two ticket arms differ"
    assert torch.equal(seen[0].view(torch.int64), seen[2].view(torch.int64)), "the third launch on the same scratch differs from the first"


# ---- form 2: the coefficients --------------------------------------------------------------------------------------------------------
COEF = [(c, b) for c in Z.COEFS for b in G.BUILDS]


@pytest.mark.parametrize("c,build", COEF, ids=[f"{Z.case_id(c)}-{b}" for c, b in COEF])
def test_group_coefficients(c, build):
    lib = _lib.load(G.BUILDS[build][0])
    inp = Z.coef_inputs(c)
    ref, lim, kappa = Z.coef_reference(c, inp)
    keep = {n: dev(inp[n]) for n in ("wm", "wav_mom", "w0", "b0", "gamma", "beta")}
    out = Buf(c.B * c.C, Z.K0 + 1, torch.float32)
    d = desc(2, B=c.B, C=c.C, L=Z.length(c), T1=c.T1, stride=c.stride, cpg=c.cpg, n_wav=inp["n_wav"], coef=out.ptr, **{n: ptr(t) for n, t in keep.items()})
    rc, kid = launch(lib, d)
    _lib.check(rc, "svt_debug_conv0", lib)
    assert kid == Z.K_COEF and out.guards_intact()
    fails, w = Z.check_coef(out.rows_cpu().reshape(c.B, c.C, Z.K0 + 1), ref, lim)
    print(f"front end [{build}] kernel {kid} {Z.case_id(c)}: worst err / limit {w:.4f}; cancellation factor up to {float(kappa.max()):.3g}")
    assert not fails, (Z.case_id(c), fails)


# ---- forms 3 .. 6 ----------------------------------------------------------------------------------------------------------------------
def run_apply(c, build, inp, out_kind=None):
    """One launch of a case (its output form replaced by out_kind if given).  Returns (rows as stored, kernel id)."""
    lib = _lib.load(G.BUILDS[build][0])
    if out_kind is not None:
        c = c._replace(out=out_kind)
    out = Buf(c.B * c.T1, c.C, Z.out_dtype(c, build))
    names = ("wav", "coef") if c.form in (3, 5) else ("wav", "wav_mom", "w0", "b0", "gamma", "beta")
    keep = {n: dev(inp[n]) for n in names}
    d = desc(c.form, B=c.B, C=c.C, L=Z.length(c), T1=c.T1, stride=c.stride, cpg=c.cpg, n_wav=inp.get("n_wav", 0), out=out.ptr,
             prec=int(c.out == "16"), pair_kind={"pk2": 2, "pk3": 3}.get(c.out, 0), **{n: ptr(t) for n, t in keep.items()})
    rc, kid = launch(lib, d)
    _lib.check(rc, "svt_debug_conv0", lib)
    assert out.guards_intact(), f"the guard rows in front of frame 0 or behind frame {c.T1 - 1} of the last clip were written"
    return out.rows_cpu(), kid


APPLY = [(c, b) for c in Z.APPLY for b in Z.builds(c)]


@pytest.mark.parametrize("c,build", APPLY, ids=[f"{Z.case_id(c)}-{b}" for c, b in APPLY])
def test_conv0_kernel_alone(c, build):
    inp, ref, lim = Z.apply_data(c, build)
    rows, kid = run_apply(c, build, inp)
    assert kid == Z.kid_of(c.form, c.out), f"kernel {kid} ran, the case is written for kernel {Z.kid_of(c.form, c.out)}"
    fails, w = Z.check_apply(c, build, rows, ref, lim)
    print(f"front end [{build}] kernel {kid} {Z.case_id(c)}: worst err / limit {w:.4f}" + (" (16-bit rows: for information, the interval decides)" if c.out == "16" else ""))
    assert not fails, (build, Z.case_id(c), fails)


PAIRS = [c for c in Z.APPLY if c.form in (3, 4) and c.out.startswith("pk")]


@pytest.mark.parametrize("c", PAIRS, ids=[Z.case_id(c) for c in PAIRS])
def test_pair_rows_are_the_cut_of_the_fp32_kernels_value(c):
    """hi + lo of a pair-row output lies within the cut term of what the fp32-output instantiation returns for the same case."""
    inp, _, _ = Z.apply_data(c, "bf16")
    got = Z.readback(c, "bf16", run_apply(c, "bf16", inp)[0]).double()
    full = run_apply(c, "bf16", inp, "f32")[0].double()
    bad = ~((got - full).abs() <= GS.cut_term(Z.piece_prec(c, "bf16"), full))
    assert not bad.any(), (Z.case_id(c), int(bad.sum()), float((got - full).abs().max()))


HALF = [c for c in Z.APPLY if c.form >= 5 and c.out == "pk3"]


@pytest.mark.parametrize("c", HALF, ids=[Z.case_id(c) for c in HALF])
def test_half_rows_and_half_pair_rows_agree_in_the_f16_build(c):
    """PK = 0 and PK = 3 use the same IEEE-half pieces there: the accumulators are the same, so the outputs differ by the two GELU forms and
    the two stores only."""
    inp = Z.apply_inputs(c)
    z = Z.apply_reference(c, inp, "f16")[2].reshape(-1, c.C)
    pairs = Z.readback(c, "f16", run_apply(c, "f16", inp)[0]).double()
    c16 = c._replace(out="16")
    rows16 = run_apply(c16, "f16", inp)[0].double()
    tol = (G.BUILDS["f16"][2] * pairs.abs() + G.ETA["f16"] + GS.cut_term(3, pairs) + G.g_act("poly", "f16", z) + G.g_act("fast", "f16", z))
    bad = ~((rows16 - pairs).abs() <= tol)
    assert not bad.any(), (Z.case_id(c), int(bad.sum()), float(((rows16 - pairs).abs() / tol).max()))


# ---- the product dispatch ------------------------------------------------------------------------------------------------------------
def _cfg(norm, wide):
    import svt_speechbrain_amd as S
    base = S.PRESETS["tiny-group" if norm == "group" else "tiny-layer"]
    # the matrix-pipe kernels need 512 channels; the split modes write pair rows only where every product of the conv stack and the feature
    # projection fits gemm_x3q_kernel (csrc/api_encoder.hip choose_pair_rows): N % 256 == 0, and 128 rows or more in the last conv layer
    return dataclasses.replace(base, name=base.name + "-wide", conv_dim=(512,) * 7, hidden_size=256) if wide else base


# (norm, conv_dim 512, precision, key 22) -> the id of the kernel that writes conv layer 0's output: the smallest configuration for each id
DISPATCH = [
    ("group", False, "fp32", 1, 400), ("layer", False, "fp32", 1, 500),
    ("group", False, "bf16", 1, 401), ("layer", False, "fp16", 1, 501),
    ("group", True, "bf16", 1, 601), ("group", True, "fp16", 0, 401), ("layer", True, "fp16", 1, 701), ("layer", True, "bf16", 0, 501),
    ("group", True, "bf16x3", 1, 620), ("group", True, "fp16x3", 1, 630), ("layer", True, "bf16x3", 1, 720), ("layer", True, "fp16x3", 1, 730),
    ("group", True, "bf16x3", 0, 420), ("group", True, "fp16x3", 0, 430), ("layer", True, "bf16x3", 0, 520), ("layer", True, "fp16x3", 0, 530),
]


@pytest.mark.parametrize("norm,wide,prec,key22,kid", DISPATCH, ids=[f"{n}-{'wide' if w else 'tiny'}-{p}-key22={k}-k{i}" for n, w, p, k, i in DISPATCH])
def test_the_product_dispatch_picks_the_kernel(norm, wide, prec, key22, kid):
    """A one-clip forward without the output norm: the last front-end launch is the kernel that writes conv layer 0's output."""
    import svt_speechbrain_amd as S
    cfg = _cfg(norm, wide)
    enc = S.HuggingFaceWav2Vec2(cfg.name, None, config=cfg, precision=prec, output_norm=False, normalize_wav=True, seed=5).to(DEV)
    lib = enc._lib()
    n = 129 * 320 + 120 if prec.endswith("x3") else 1600          # 129 frames behind the conv stack / 4
    wav = (0.1 * torch.randn(1, n, generator=torch.Generator().manual_seed(2))).to(DEV)
    try:
        assert lib.svt_debug_set(22, key22) == 0
        y = enc(wav)
        torch.cuda.synchronize()
        got = lib.svt_debug_set(41, 0)
    finally:
        lib.svt_debug_set(22, 1)
    assert torch.isfinite(y).all()
    assert got == kid, f"conv layer 0 ran on kernel {got}, expected {kid}"


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
RB, RT, RC, RS = 4, 20, 512, 5                      # the geometry of the refusal cases
RL = (RT - 1) * RS + Z.K0


def _base(form):
    """A descriptor the hook accepts, its outputs, and what must stay alive (every input zero: every buffer is large enough for every form)."""
    keep = {n: torch.zeros(RB * RL + 4096 * 11, dtype=torch.float32, device=DEV) for n in ("x", "wav", "w0", "b0", "gamma", "beta", "coef_in")}
    keep["wav_mom"] = torch.ones(64, dtype=torch.float64, device=DEV)
    keep["wm_in"] = torch.zeros(RB * Z.NWM, dtype=torch.float64, device=DEV)
    outs = {"mom": Buf(8, 2, torch.float64), "wm": Buf(RB, Z.NWM, torch.float64), "coef": Buf(RB * RC, 11, torch.float32),
            "out": Buf(RB * RT, RC, torch.float32)}
    d = desc(form, B=RB, C=RC, L=RL, T1=RT, stride=RS, cpg=2, n_wav=2 * RL, groups=2, groups_max=4, n=64)
    p = {n: t.data_ptr() for n, t in keep.items()}
    if form == 0:
        d.x, d.mom = p["x"], outs["mom"].ptr
    elif form == 1:
        d.wav, d.wm = p["wav"], outs["wm"].ptr
    elif form == 2:
        d.wm, d.coef = p["wm_in"], outs["coef"].ptr
    if form in (3, 5):
        d.wav, d.coef, d.out = p["wav"], p["coef_in"], outs["out"].ptr
    if form in (2, 4, 6):
        d.wav_mom, d.w0, d.b0, d.gamma, d.beta = p["wav_mom"], p["w0"], p["b0"], p["gamma"], p["beta"]
    if form in (4, 6):
        d.wav, d.out = p["wav"], outs["out"].ptr
    return d, outs, keep


def _set(**kw):
    def f(d, o, k):
        for n, v in kw.items():
            setattr(d, n, v)
    return f


def _shift(name, by):
    def f(d, o, k):
        setattr(d, name, getattr(d, name) + by)
    return f


ALL = tuple(range(7))
REFUSALS = [("struct_size", (0,), _set(struct_size=8)), ("form 7", (0,), _set(form=7)), ("form -1", (3,), _set(form=-1))]
REFUSALS += [(f"k 9, form {f}", (f,), _set(k=9)) for f in ALL] + [(f"stride 0, form {f}", (f,), _set(stride=0)) for f in ALL]
REFUSALS += [(f"stride 6, form {f}", (f,), _set(stride=6, L=(RT - 1) * 6 + Z.K0)) for f in ALL]
REFUSALS += [(f"B 0, form {f}", (f,), _set(B=0)) for f in ALL[1:]] + [(f"T1 0, form {f}", (f,), _set(T1=0)) for f in ALL[1:]]
REFUSALS += [(f"L one short, form {f}", (f,), _set(L=RL - 1)) for f in ALL[1:]]
REFUSALS += [(f"C 0, form {f}", (f,), _set(C=0)) for f in ALL[2:]] + [(f"C 520, form {f}", (f,), _set(C=520)) for f in ALL[2:]]
REFUSALS += [(f"C 12, form {f}", (f,), _set(C=12)) for f in (3, 4, 5, 6)] + [(f"C 256, form {f}", (f,), _set(C=256)) for f in (5, 6)]
REFUSALS += [(f"pair rows with C 40, form {f}", (f,), _set(C=40, pair_kind=2)) for f in (3, 4)]
REFUSALS += [(f"pair rows with prec 1, form {f}", (f,), _set(prec=1, pair_kind=3)) for f in (3, 4)]
REFUSALS += [(f"pair kind 1, form {f}", (f,), _set(pair_kind=1)) for f in (3, 4, 5, 6)] + [(f"prec 2, form {f}", (f,), _set(prec=2)) for f in (3, 4)]
REFUSALS += [(f"cpg 0, form {f}", (f,), _set(cpg=0)) for f in (2, 4, 6)] + [(f"cpg 3 with B 4, form {f}", (f,), _set(cpg=3)) for f in (2, 4, 6)]
REFUSALS += [(f"n_wav 0 with moments, form {f}", (f,), _set(n_wav=0)) for f in (2, 4, 6)]
REFUSALS += [("groups 0", (0,), _set(groups=0)), ("groups > groups_max", (0,), _set(groups=5)), ("n 0", (0,), _set(n=0)),
             ("two groups with n % 4 != 0", (0,), _set(n=66))]
REFUSALS += [(f"null {n}, form {f}", (f,), _set(**{n: None})) for f, names in
             ((0, ("x", "mom")), (1, ("wav", "wm")), (2, ("wm", "coef", "w0", "gamma", "beta")), (3, ("wav", "coef", "out")),
              (4, ("wav", "w0", "gamma", "beta", "out")), (5, ("wav", "coef", "out")), (6, ("wav", "w0", "gamma", "beta", "out"))) for n in names]
REFUSALS += [(f"{n} not 16-byte aligned, form {f}", (f,), _shift(n, 8)) for f, names in
             ((0, ("x", "mom")), (1, ("wav", "wm")), (2, ("wm", "wav_mom", "coef", "w0", "b0", "gamma", "beta")), (3, ("wav", "coef", "out")),
              (4, ("wav", "wav_mom", "w0", "b0", "gamma", "beta", "out")), (5, ("wav", "coef")), (6, ("wav", "wav_mom", "w0", "b0", "gamma", "beta"))) for n in names]
REFUSALS += [(f"pair-row out not 128-byte aligned, form {f}", (f,), lambda d, o, k: (_set(pair_kind=2)(d, o, k), _shift("out", 64)(d, o, k))) for f in (3, 4)]
REFUSALS += [(f"out not 128-byte aligned, form {f}", (f,), _shift("out", 64)) for f in (5, 6)]
REFUSALS = [(name, f, change) for name, forms, change in REFUSALS for f in forms]


@pytest.mark.parametrize("build", list(G.BUILDS))
@pytest.mark.parametrize("name,form,change", REFUSALS, ids=[r[0].replace(" ", "_") for r in REFUSALS])
def test_the_hook_refuses(name, form, change, build):
    lib = _lib.load(G.BUILDS[build][0])
    d, outs, keep = _base(form)
    change(d, outs, keep)
    rc, _ = launch(lib, d)
    assert rc == SVT_ERR_INVALID and b"svt_debug_conv0" in lib.svt_last_error(), (name, rc, lib.svt_last_error())
    for n, b in outs.items():
        assert b.untouched(), f"{name}: the refused call wrote to {n}"


@pytest.mark.parametrize("build", list(G.BUILDS))
@pytest.mark.parametrize("form", ALL)
def test_the_base_of_the_refusals_is_accepted(form, build):
    """The descriptor every refusal case changes in ONE respect runs, so each refusal is due to that one change."""
    lib = _lib.load(G.BUILDS[build][0])
    d, outs, keep = _base(form)
    rc, kid = launch(lib, d)
    _lib.check(rc, "svt_debug_conv0", lib)
    assert kid == (100, 200, 300, 400, 500, 601, 701)[form]
    written = {0: "mom", 1: "wm", 2: "coef"}.get(form, "out")
    for n, b in outs.items():
        assert b.guards_intact(), n
        if n != written:
            assert b.untouched(), n
    got = outs[written].t.view(torch.uint8).flatten()
    assert not torch.equal(got, outs[written].before)
