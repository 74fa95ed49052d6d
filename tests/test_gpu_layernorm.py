"""GPU tests of each row LayerNorm kernel alone (csrc/layernorm.hip: six kernels behind three launchers), in both 16-bit builds, through the
C-ABI test hook svt_debug_layernorm, in the forms the encoder and the RCA layers build -- with the buffer aliasing they use.

Every case names the kernel and instantiation it is written for (the id svt_debug_set(40, 0) reports, include/svt_mi355.h) and asserts it, so
a changed condition in a launcher fails a case instead of moving it to another kernel.  Every output is allocated filled with 0xFF bytes (NaN
in every type) with 8 such guard rows in front of and behind it in the same allocation; the guards must come back bit-unchanged and no NaN
may be left inside.  Every element of every output is held to the checks tests/layernorm_limit.py derives (fp64 reference from the bit-exact
fp32 input row; a per-element limit for fp32, an interval for 16-bit stores, the cut term for pair rows and (hi, lo) planes; bit-exact
identities between the outputs of a launch); tests/test_layernorm_limit.py shows on the CPU that a correct kernel passes them and that
thirteen mutants do not.  For the in-place cases the reference comes from the inputs as they were before the launch.

The refusals -- what the hook adds to the launchers' own checks, and every set_error branch of the launchers it can reach -- are decided on the
host: each must return SVT_ERR_INVALID and leave the poisoned outputs untouched.  Nothing here launches a kernel with arguments it cannot serve."""
import ctypes

import pytest
import torch

import gemm_limit as G
import layernorm_limit as L

pytestmark = pytest.mark.gpu

from svt_speechbrain_amd import _lib  # noqa: E402

DEV = "cuda:0"
SVT_ERR_INVALID = -1


class Buf:
    """(rows + 2 GUARD, D) elements of `dtype`, every byte 0xFF; `init` (rows, D) is copied into the middle (an input that is also an output)."""

    def __init__(self, rows, D, dtype, init=None):
        self.rows, self.D = rows, D
        es = torch.empty((), dtype=dtype).element_size()
        raw = torch.full(((rows + 2 * L.GUARD) * D * es,), 0xFF, dtype=torch.uint8, device=DEV)
        self.t = raw.view(dtype).view(rows + 2 * L.GUARD, D)
        if init is not None:
            assert init.dtype == dtype and tuple(init.shape) == (rows, D)
            self.t[L.GUARD:L.GUARD + rows] = init.to(DEV)
        self.ptr = self.t.data_ptr() + L.GUARD * D * es
        self.before = raw.clone()

    def guards_intact(self):
        now, n = self.t.view(torch.uint8).flatten(), L.GUARD * self.D * self.t.element_size()
        return torch.equal(now[:n], self.before[:n]) and torch.equal(now[-n:], self.before[-n:])

    def untouched(self):
        return torch.equal(self.t.view(torch.uint8).flatten(), self.before)

    def rows_cpu(self):
        return self.t[L.GUARD:L.GUARD + self.rows].cpu()


def out_dtype(c, name, dtype):
    if name == "yP":
        return torch.int32
    if name in ("yh", "yl") or (name == "yT" and c.prec):
        return dtype
    return torch.float32


def build_launch(c, build, inp):
    """(descriptor, outputs {name: Buf}, everything that must stay alive) of a case, with the caller's aliasing."""
    dtype = G.BUILDS[build][1]
    R, D = c.rows, c.D
    d = _lib.LayerNormDescC()
    d.struct_size = ctypes.sizeof(d)
    d.form, d.prec, d.x_is_f32, d.rows, d.D, d.gelu, d.eps, d.pair_kind = c.form, c.prec, int(c.x == "f32"), R, D, c.gelu, c.eps, c.pk
    keep, outs, ptr = [], {}, {}
    out_names = list(c.outs) + (["yh", "yl"] if c.form else [])
    alias = dict((o, i) for i, o in c.alias)          # output -> the input it shares its buffer with
    if c.form and c.src == "hilo":
        alias.update(yh="rh", yl="rl")                  # the residual stream is normalised in place
    for name in out_names:
        src = alias.get(name)
        outs[name] = Buf(R, D, out_dtype(c, name, dtype), None if src is None else inp[src])
        ptr[name] = outs[name].ptr
        if src is not None:
            ptr[src] = outs[name].ptr
    for name in ("x", "add", "addP", "branch", "rh", "rl", "x32", "pbias", "gamma", "beta"):
        if name in inp and name not in ptr:
            keep.append(inp[name].contiguous().to(DEV))
            ptr[name] = keep[-1].data_ptr()
    if c.form == 2:
        keep.append(inp["parts"].contiguous().to(DEV))
        ptr["parts"] = keep[-1].data_ptr()
        d.nparts, d.part_stride = c.nparts, R * D
    for name, p in ptr.items():
        setattr(d, name, p)
    return d, outs, keep


def launch(lib, d, key20=1):
    """svt_debug_layernorm under key 20, the key restored.  Returns (rc, kernel id)."""
    try:
        _lib.check(lib.svt_debug_set(20, key20), f"svt_debug_set(20, {key20})", lib)
        rc = lib.svt_debug_layernorm(ctypes.byref(d), 0, torch.cuda.current_stream().cuda_stream)
        kid = lib.svt_debug_set(40, 0)
        torch.cuda.synchronize()
    finally:
        lib.svt_debug_set(20, 1)
    return rc, kid


RUNS = [(c, b) for c in L.CASES for b in L.builds(c)]


@pytest.mark.parametrize("c,build", RUNS, ids=[f"{L.case_id(c)}-{b}" for c, b in RUNS])
def test_layernorm_kernel_alone(c, build):
    lib = _lib.load(G.BUILDS[build][0])
    inp, ref, lim = L.case_data(c, build)
    d, outs, keep = build_launch(c, build, inp)
    rc, kid = launch(lib, d, c.key20)
    _lib.check(rc, "svt_debug_layernorm", lib)
    assert kid == c.kid, f"kernel {kid} ran, the case is written for kernel {c.kid}"
    for name, b in outs.items():
        assert b.guards_intact(), f"{name}: the guard rows in front of row 0 or behind row {c.rows - 1} were written"
    fails, report = L.check_outputs(c, build, inp, ref, lim, {name: b.rows_cpu() for name, b in outs.items()})
    for name, (w, r, col) in report.items():
        if name == "yT outside its interval":
            print(f"layernorm [{build}] kernel {kid} {L.case_id(c)}: yT: {int(w)} of {c.rows * c.D} elements outside their interval")
        else:
            print(f"layernorm [{build}] kernel {kid} {L.case_id(c)}: {name}: worst err / limit {w:.4f} at row {r} column {col} of {c.rows * c.D} elements")
    assert not fails, (build, L.case_id(c), fails)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
RR, RD = 5, 512        # the shape of the refusal cases; every buffer is allocated for rows of 1280 fp32 elements, whatever a case says


def _base(form, dtype):
    """A descriptor the hook accepts, its outputs, and what must stay alive."""
    d = _lib.LayerNormDescC()
    d.struct_size = ctypes.sizeof(d)
    d.form, d.rows, d.D, d.eps, d.x_is_f32 = form, RR, RD, 1e-5, 1
    wide = lambda: torch.zeros(4 * RR * 1280, dtype=torch.float32, device=DEV)   # noqa: E731
    keep = {n: wide() for n in ("gamma", "beta", "x", "add", "addP", "branch", "rh", "rl", "x32", "parts", "pbias")}
    outs = {n: Buf(RR, 1280, torch.float32) for n in ("yT", "yF", "sumF", "yP", "yh", "yl")}
    d.gamma, d.beta = keep["gamma"].data_ptr(), keep["beta"].data_ptr()
    if form == 0:
        d.x, d.yT = keep["x"].data_ptr(), outs["yT"].ptr
    elif form == 1:
        d.rh, d.rl, d.branch, d.yh, d.yl = keep["rh"].data_ptr(), keep["rl"].data_ptr(), keep["branch"].data_ptr(), outs["yh"].ptr, outs["yl"].ptr
    else:
        d.rh, d.rl, d.yh, d.yl = keep["rh"].data_ptr(), keep["rl"].data_ptr(), outs["yh"].ptr, outs["yl"].ptr
        d.parts, d.pbias, d.nparts, d.part_stride = keep["parts"].data_ptr(), keep["pbias"].data_ptr(), 4, RR * RD
    return d, outs, keep


def _pairs(d, o, k):
    """form 0 writing pair rows (and nothing else)."""
    d.yT, d.yP, d.pair_kind = None, o["yP"].ptr, 2


def _set(**kw):
    def f(d, o, k):
        for n, v in kw.items():
            setattr(d, n, v(d, o, k) if callable(v) else v)
    return f


def _shift(name, by):
    """The pointer `name` (taken from the spare buffers where the base leaves it NULL) moved by `by` bytes."""
    def f(d, o, k):
        p = getattr(d, name) or (o[name].ptr if name in o else k[name].data_ptr())
        setattr(d, name, p + by)
    return f


def _both(*fs):
    def f(d, o, k):
        for g in fs:
            g(d, o, k)
    return f


REFUSALS = [
    # ---- what the hook adds
    ("struct_size", 0, _set(struct_size=8)), ("form 3", 0, _set(form=3)),
    ("rows 0", 0, _set(rows=0)), ("D 0", 0, _set(D=0)), ("rows 0, form 1", 1, _set(rows=0)), ("D 0, form 2", 2, _set(D=0)),
    ("null gamma", 0, _set(gamma=None)), ("null beta", 1, _set(beta=None)), ("null gamma, form 2", 2, _set(gamma=None)),
    ("null x", 0, _set(x=None)), ("16-bit x with prec 0", 0, _set(x_is_f32=0)),
    ("form 1, D 640", 1, _set(D=640)), ("form 2, D 640", 2, _set(D=640)), ("form 1, D 64", 1, _set(D=64)), ("form 2, D 1280", 2, _set(D=1280)),
    ("form 1, x32 and (rh, rl)", 1, _set(x32=lambda d, o, k: k["x32"].data_ptr())),
    ("form 1, neither x32 nor (rh, rl)", 1, _set(rh=None, rl=None)),
    ("form 1, rh without rl", 1, _set(rl=None)), ("form 1, x32 and rl", 1, _set(rh=None, x32=lambda d, o, k: k["x32"].data_ptr())),
    ("form 2 without rh", 2, _set(rh=None)),
    ("form 1 without yh", 1, _set(yh=None)), ("form 1 without yl", 1, _set(yl=None)), ("form 2 without yh", 2, _set(yh=None)), ("form 2 without yl", 2, _set(yl=None)),
    ("nparts 0", 2, _set(nparts=0)), ("nparts -1", 2, _set(nparts=-1)), ("overlapping parts", 2, _set(part_stride=RR * RD - 4)),
] + [(f"{n} not 16-byte aligned", 0, _shift(n, 8)) for n in ("x", "yT", "yF", "add", "sumF")] + [
    ("gamma not 16-byte aligned", 0, _shift("gamma", 4)), ("beta not 16-byte aligned", 0, _shift("beta", 8)),
    ("yP not 128-byte aligned", 0, _both(_pairs, _shift("yP", 64))), ("yP not 16-byte aligned", 0, _both(_pairs, _shift("yP", 8))),
    ("addP not 128-byte aligned", 0, _both(_pairs, _shift("addP", 64))),
] + [(f"{n} not 16-byte aligned, form 1", 1, _shift(n, 8)) for n in ("branch", "rh", "rl", "yh", "yl", "yF", "gamma", "beta")] + [
    ("x32 not 16-byte aligned", 1, _both(_set(rh=None, rl=None, branch=None), _shift("x32", 8))),
] + [(f"{n} not 16-byte aligned, form 2", 2, _shift(n, 8)) for n in ("parts", "pbias", "rh", "rl", "yh", "yl", "yF")] + [
    # ---- the launchers' own refusals, reached through the hook
    ("addP without yP", 0, _set(addP=lambda d, o, k: k["addP"].data_ptr())),
    ("pair rows with prec 1", 0, _both(_pairs, _set(prec=1))),
    ("pair rows with yT", 0, _both(_pairs, _set(yT=lambda d, o, k: o["yT"].ptr))),
    ("pair rows at D 64", 0, _both(_pairs, _set(D=64))), ("pair rows at D 1280", 0, _both(_pairs, _set(D=1280))),
    ("pair kind 1", 0, _both(_pairs, _set(pair_kind=1))), ("pair kind 0", 0, _both(_pairs, _set(pair_kind=0))),
    ("16-bit x with add at D 64", 0, _set(prec=1, x_is_f32=0, D=64, add=lambda d, o, k: k["add"].data_ptr())),
    ("16-bit x with add at D 1280", 0, _set(prec=1, x_is_f32=0, D=1280, add=lambda d, o, k: k["add"].data_ptr())),
    ("form 2 without parts", 2, _set(parts=None)), ("form 2 without pbias", 2, _set(pbias=None)),
    ("part_stride not a multiple of 4", 2, _set(part_stride=RR * RD + 2)),
]


@pytest.mark.parametrize("build", list(G.BUILDS))
@pytest.mark.parametrize("name,form,change", REFUSALS, ids=[r[0].replace(" ", "_") for r in REFUSALS])
def test_the_hook_refuses(name, form, change, build):
    variant, dtype, _ = G.BUILDS[build]
    lib = _lib.load(variant)
    d, outs, keep = _base(form, dtype)
    change(d, outs, keep)
    rc, _ = launch(lib, d)
    assert rc == SVT_ERR_INVALID and b"layernorm" in lib.svt_last_error(), (name, rc, lib.svt_last_error())
    for n, b in outs.items():
        assert b.untouched(), f"{name}: the refused call wrote to {n}"


@pytest.mark.parametrize("build", list(G.BUILDS))
@pytest.mark.parametrize("form", (0, 1, 2))
def test_the_base_of_the_refusals_is_accepted(form, build):
    """The descriptor every refusal case changes in ONE respect runs (all-zero inputs: every output row is beta = 0), so each refusal is due to that
    one change."""
    variant, dtype, _ = G.BUILDS[build]
    lib = _lib.load(variant)
    d, outs, keep = _base(form, dtype)
    rc, kid = launch(lib, d)
    _lib.check(rc, "svt_debug_layernorm", lib)
    assert kid == (L.K_VEC_F32, L.K_HILO2, L.K_HILO2_PARTS)[form]
    assert all(b.guards_intact() for b in outs.values())
    written = {"yT"} if form == 0 else {"yh", "yl"}
    for n, b in outs.items():
        if n in written:
            es = 4 if form == 0 else 2
            got = b.t.view(torch.uint8).flatten()[L.GUARD * 1280 * 4:][:RR * RD * es]
            assert not got.any(), f"{n}: LN of zero rows with beta = 0 is zero"
        else:
            assert b.untouched(), n
