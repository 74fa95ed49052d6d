"""What tests/test_gpu_layernorm.py (GPU) and tests/test_layernorm_limit.py (CPU) share for the six row LayerNorm kernels of
csrc/layernorm.hip: the case table, the inputs, the fp64 reference, the per-element limit and the checks of every storage form.

THE INPUT.  The row the kernel normalises, t, is built by every form with plain IEEE fp32 additions in a fixed order and no multiply
beside them (nothing for -ffp-contract to fuse), so the host reproduces it bit for bit with torch float32 operations in the same order:

    layernorm_kernel / layernorm_f32_vec_kernel     t = widen(x);  t += add;  t += (float(hi) + float(lo)) of addP
    the (hi, lo) kernels                             t = float(h) + float(l);  t += float(branch)
    PARTS                                            a = p0; a += p1; ...;  t = (float(h) + float(l)) + float(rn16(a + bias))

(t32 below).  Wherever sumF is written it must equal t32 bit for bit, and the reference starts from t32: the rounding point of the K-split
branch is part of the input, not an error term.

THE REFERENCE, in fp64 from t32:  mu = mean(t), d = t - mu, v = mean(d^2), r = (v + eps)^-1/2, z = d r, y = z gamma + beta,
ref = gelu(y) or y  (eps as the float the kernel is given).

THE LIMIT OF THE fp32 STAGE.  It is a bound for a kernel that takes both statistics in fp32, two-pass, in ANY summation order, not a fitted
tolerance.  With u = 2^-24 (every fp32 operation rounds to nearest: relative error u):

    e_mu  = (D + 1) u mean|t|                 the sum of D terms in any order (D - 1 adds, each at most u of a partial sum that is at most
                                              sum|t|, to first order) and the scaling by 1 / D (the constant and the multiply: 2 u)
    e_d   = e_mu + u |d|                      the subtraction of the computed mean
    rho_v = ((D + 2) u v + 2 mean(|d| e_d) + mean(e_d^2)) / (v + eps) + 2 u
                                              relative error of v + eps: summing the D squares (each squared with error u) and scaling by
                                              1 / D, the propagated error of d (d^2 moves by 2 |d| e_d + e_d^2), and the addition of eps
    rho_r = rho_v / 2 + 2 u                   x^-1/2 halves a relative error; rsqrtf is taken as accurate to 1 ulp = 2 u relative (the
                                              figure the HIP programming guide lists for rsqrtf; the build calls __ocml_rsqrt_f32, which is
                                              v_rsq_f32 on gfx950, documented to 1 ulp)
    e_z   = e_d r + |z| (rho_r + 2 u)         z = d r: the error of d scaled by r, the relative error of r, and the multiply
    lim_y = |gamma| e_z + 2 u (|z gamma| + |beta|)          the multiply by gamma and the addition of beta (or their fused form)

    lim32 = lim_y                              without GELU
    lim32 = 1.13 lim_y + g_act(form, build, y) with GELU: 1.13 bounds |GELU'|, g_act is the documented error of the GELU form the kernel
                                              calls (tests/gemm_limit.py): "poly" (gelu_bf16x2) exactly where the source says so -- 16-bit-only
                                              output with PK == 0 and no yF in layernorm_f32_vec_kernel, always in layernorm_op16_rows2_kernel --
                                              and "fast" (gelu_erf) everywhere else (gelu_form below)

THE CHECKS, per element (check_outputs):

    fp32 (yF, fp32 yT)       |got - ref| <= lim32 + u |ref|
    16-bit yT                rn16(ref - lim32) <= got <= rn16(ref + lim32): rounding is monotone, so a kernel whose fp32 value lies within lim32 of
                             ref stores a value inside that interval (rn16 = the build's type, round to nearest even; taken through fp32, which
                             keeps the interval sound: an fp32 value >= ref - lim32 is >= rn32(ref - lim32)).  Printed for information as
                             well: err / (lim32 + u_out |ref| + eta_out).
    pair rows (yP), (hi, lo) planes (yh, yl)    read back as hi + lo in fp32:  |got - ref| <= lim32 + cut_term (tests/gemm_split.py: u^2 |ref| of
                             the piece type, and half the subnormal spacing of an IEEE-half lo piece).  Pair rows are laid out as store_pairs
                             writes and the addP reader reads them: blocks of 32 elements in 128 bytes, 64 bytes of hi then 64 of lo.
    exact, bit for bit       sumF == t32;  yT == rn16(yF) and (hi, lo) == cut(yF) wherever yF is written beside them: a wrong lo piece is far
                             below lim32, this identity sees it.  A row of zeros returns beta exactly (without GELU): d = 0, so
                             y = fma(0, gamma, beta).

A missing (NaN-poisoned) element fails every comparison.  tests/test_layernorm_limit.py shows on the CPU that a correct fp32 two-pass kernel
in both reduction orders of the real kernels stays inside all of this, and that thirteen mutants do not.

ROWS OF A CASE.  Eight kinds, cycled over the case's rows starting at a kind that moves from case to case (KINDS): unit normal, mean 100
with spread 0.1, spread 1e-3 ~ sqrt(eps), constant, zeros, one outlier of 300, scale 1e4, a ramp.  Where t has several addends the row
kind is that of their sum; the constant and the zero row have zero addends, so t is exactly constant / zero.  gamma = 1 + 0.3 N(0, 1),
beta = 0.2 N(0, 1), or gamma = 1, beta = 0 (`unit`: the data2vec positional stack's form)."""
import collections

import torch

import gemm_limit as G
import gemm_split as GS

U = 2.0 ** -24
ROWS = (1, 3, 4, 5, 8, 9, 13)        # 4 rows per workgroup (one-row kernels); 8 per workgroup and 2 per wave, an idle half-wave when odd (two-row)
WIDE = (512, 768, 1024)              # the register-resident kernels
NARROW = (64, 80, 1280)              # layernorm_kernel: one pass of the lane loop, idle lanes in the second pass, hubert-xlarge's width
GUARD = 8                            # poisoned rows in front of and behind every output
KINDS = ("normal", "mean100", "tiny", "constant", "zeros", "outlier", "big", "ramp")
PIECE_PREC = {"bf16": 2, "f16": 3}   # the piece type of a build's (hi, lo) planes, as a gemm_split precision

# kernel ids (include/svt_mi355.h, svt_debug_set key 40)
K_ROW_F32, K_ROW_F32_16, K_ROW_16 = 1000, 1001, 1011
K_VEC_F32, K_VEC_F32_16, K_VEC_16, K_VEC_PK2, K_VEC_PK3 = 2000, 2001, 2011, 2200, 2300
K_ROWS2, K_HILO, K_HILO2, K_HILO2_PARTS, K_F32_HILO = 3000, 4000, 5000, 5001, 6000
ALL_IDS = (K_ROW_F32, K_ROW_F32_16, K_ROW_16, K_VEC_F32, K_VEC_F32_16, K_VEC_16, K_VEC_PK2, K_VEC_PK3, K_ROWS2, K_HILO, K_HILO2, K_HILO2_PARTS, K_F32_HILO)
TWO_ROW_IDS = (K_ROWS2, K_HILO2, K_HILO2_PARTS)

# form 0: x "f32" / "16"; outs of {"yT", "yF", "sumF", "yP"}; add / addP: the addends; pk: the pair kind; alias: pairs of buffers that are ONE
# buffer, as the caller has them.  form 1: src "x32" / "hilo", branch; outs of {"yF"} beside the planes, which are written in place over (rh, rl).
# form 2: nparts, grid (parts and bias on a 2^-10 grid: every partial sum exact).  key20: svt_debug_set key 20 for the launch.  idx: position in CASES.
LCase = collections.namedtuple("LCase", "name kid form D rows prec x outs add addP pk gelu eps alias src branch nparts grid key20 unit idx")
CASES = []


def _case(name, kid, form, D, rows, prec=0, x="f32", outs=(), add=False, addP=False, pk=0, gelu=0, eps=1e-5, alias=(), src=None, branch=False,
          nparts=0, grid=False, key20=1, unit=False):
    assert rows in ROWS and (D in WIDE or (D in NARROW and kid // 1000 == 1))
    CASES.append(LCase(name, kid, form, D, rows, prec, x, tuple(outs), add, addP, pk, gelu, eps, tuple(alias), src, branch, nparts, grid, key20, unit, len(CASES)))


def _rows(i):
    return ROWS[i % len(ROWS)]


def _build_table():
    n = 0   # walks ROWS so that every kernel meets every row count
    # fp32 -> fp32 yT: plain, + GELU, + add + sumF with x == sumF (the pre-LN residual update)
    for D in NARROW + WIDE:
        kid = K_VEC_F32 if D in WIDE else K_ROW_F32
        for tag, kw in (("plain", {}), ("gelu", dict(gelu=1)), ("add-sum", dict(add=True, outs=("yT", "sumF"), alias=(("x", "sumF"),)))):
            _case(f"f32-{tag}", kid, 0, D, _rows(n), **{"outs": ("yT",), **kw})
            n += 1
    # prec 1, fp32 x -> 16-bit yT (+ yF) (+ add, add == yF: post-LN plain)
    for D in NARROW + WIDE:
        kid = K_VEC_F32_16 if D in WIDE else K_ROW_F32_16
        for tag, kw in (("yT", dict(outs=("yT",))), ("yT-yF", dict(outs=("yT", "yF"))),
                        ("add-yT-yF", dict(add=True, outs=("yT", "yF"), alias=(("add", "yF"),)))):
            _case(f"f32to16-{tag}", kid, 0, D, _rows(n), prec=1, **kw)
            n += 1
    _case("f32to16-gelu-yT", K_VEC_F32_16, 0, 512, 5, prec=1, outs=("yT",), gelu=1)             # 16-bit only: the polynomial GELU
    _case("f32to16-gelu-yT", K_VEC_F32_16, 0, 1024, 9, prec=1, outs=("yT",), gelu=1)
    _case("f32to16-gelu-yT-yF", K_VEC_F32_16, 0, 768, 13, prec=1, outs=("yT", "yF"), gelu=1)    # yF beside it: gelu_erf
    _case("f32to16-gelu-yT", K_ROW_F32_16, 0, 80, 3, prec=1, outs=("yT",), gelu=1)              # layernorm_kernel: always gelu_erf
    # prec 1, 16-bit x -> 16-bit yT, narrow
    for D in NARROW:
        for gelu in (0, 1):
            _case("16to16" + ("-gelu" if gelu else ""), K_ROW_16, 0, D, _rows(n), prec=1, x="16", outs=("yT",), gelu=gelu)
            n += 1
    # prec 1, 16-bit x + fp32 add -> yT, yF (add == yF) / yT, sumF (add == sumF: pre-LN with a 16-bit branch), wide
    for D in WIDE:
        _case("16+add-yT-yF", K_VEC_16, 0, D, _rows(n), prec=1, x="16", add=True, outs=("yT", "yF"), alias=(("add", "yF"),))
        _case("16+add-yT-sumF", K_VEC_16, 0, D, _rows(n + 1), prec=1, x="16", add=True, outs=("yT", "sumF"), alias=(("add", "sumF"),))
        n += 2
    # prec 1, 16-bit rows in place: two rows per wave (key 20 = 1), and the one-row kernel with the polynomial GELU (key 20 = 0)
    for key20, kid in ((1, K_ROWS2), (0, K_VEC_16)):
        m = 0
        for D in WIDE:
            for gelu in (0, 1):
                _case("16-inplace" + ("-gelu" if gelu else ""), kid, 0, D, _rows(m), prec=1, x="16", outs=("yT",), gelu=gelu, alias=(("x", "yT"),), key20=key20)
                m += 1
        _case("16-inplace-gelu", kid, 0, 768, _rows(m), prec=1, x="16", outs=("yT",), gelu=1, alias=(("x", "yT"),), key20=key20)
    # pair rows
    for pk, kid in ((2, K_VEC_PK2), (3, K_VEC_PK3)):
        for D in WIDE:
            _case("pairs", kid, 0, D, _rows(n), outs=("yP",), pk=pk)                                                      # LN0
            _case("pairs-yF", kid, 0, D, _rows(n + 1), outs=("yP", "yF"), pk=pk)
            _case("pairs-add-sumF", kid, 0, D, _rows(n + 2), add=True, outs=("yP", "sumF"), pk=pk, alias=(("x", "sumF"),))  # pre-LN
            _case("pairs-gelu", kid, 0, D, _rows(n + 3), outs=("yP",), pk=pk, gelu=1)                                     # layer-norm conv stack
            n += 4
        _case("pairs-yF-eps1e-6", kid, 0, 768, 8, outs=("yP", "yF"), pk=pk, eps=1e-6)
    for D in WIDE:
        _case("pairs-add-yF", K_VEC_PK2, 0, D, _rows(n), add=True, outs=("yP", "yF"), pk=2, alias=(("add", "yF"),))       # fp32 residual beside the pairs
        _case("pairs-addP", K_VEC_PK3, 0, D, _rows(n + 1), addP=True, outs=("yP",), pk=3, alias=(("addP", "yP"),))        # in place
        _case("pairs-addP-yF", K_VEC_PK3, 0, D, _rows(n + 2), addP=True, outs=("yP", "yF"), pk=3, alias=(("addP", "yP"),))   # last layer
        n += 3
    _case("pairs-addP", K_VEC_PK2, 0, 768, 5, addP=True, outs=("yP",), pk=2, alias=(("addP", "yP"),))                    # the bf16-piece reader
    _case("pairs-addP-yF", K_VEC_PK2, 0, 512, 9, addP=True, outs=("yP", "yF"), pk=2, alias=(("addP", "yP"),))
    # form 1: x32 -> (yh, yl)
    m = 0
    for D in WIDE:
        for _ in range(2):
            _case("x32-hilo", K_F32_HILO, 1, D, _rows(m), src="x32")
            m += 1
    _case("x32-hilo", K_F32_HILO, 1, 768, _rows(m), src="x32")
    # form 1: branch + (rh, rl) -> (yh, yl) in place, with and without yF; two rows per wave and one
    for key20, kid in ((1, K_HILO2), (0, K_HILO)):
        m = 0
        for D in WIDE:
            for outs in ((), ("yF",)):
                _case("hilo-branch" + ("-yF" if outs else ""), kid, 1, D, _rows(m), src="hilo", branch=True, outs=outs, key20=key20)
                m += 1
        _case("hilo-branch-yF", kid, 1, 768, _rows(m), src="hilo", branch=True, outs=("yF",), key20=key20)
    # form 2: the K-split branch, nparts 4 and 1, with and without yF, in place; one case with every partial sum exact
    m = 0
    for D in WIDE:
        for nparts in (4, 1):
            _case(f"parts{nparts}" + ("-yF" if m % 2 else ""), K_HILO2_PARTS, 2, D, _rows(m), src="hilo", nparts=nparts, outs=("yF",) if m % 2 else ())
            m += 1
    _case("parts4-yF", K_HILO2_PARTS, 2, 768, _rows(m), src="hilo", nparts=4, outs=("yF",))
    _case("parts4-grid-yF", K_HILO2_PARTS, 2, 768, 9, src="hilo", nparts=4, grid=True, outs=("yF",))
    _case("parts1-yF", K_HILO2_PARTS, 2, 512, 5, src="hilo", nparts=1, outs=("yF",))
    # gamma = 1, beta = 0
    _case("f32-unit", K_VEC_F32, 0, 768, 8, outs=("yT",), unit=True)
    _case("16-inplace-gelu-unit", K_ROWS2, 0, 512, 9, prec=1, x="16", outs=("yT",), gelu=1, alias=(("x", "yT"),), unit=True)


_build_table()


def case_id(c):
    return f"{c.idx:03d}-k{c.kid}-{c.name}-D{c.D}-r{c.rows}"


def builds(c):
    """The builds a case runs in: both 16-bit builds, except the pair-row forms, which run in the library that serves the split modes."""
    if c.pk:
        assert GS.library(GS.S(7256, 128, 128, 32)) is None   # the split modes live in the bf16 library
        return ("bf16",)
    return tuple(G.BUILDS)


def gelu_form(c):
    """From csrc/layernorm.hip: gelu_bf16x2 in layernorm_op16_rows2_kernel, and in layernorm_f32_vec_kernel where the result is stored in 16 bits
    only (sizeof(TO) == 2 && PK == 0 && !yF); gelu_erf everywhere else."""
    if c.kid == K_ROWS2:
        return "poly"
    if c.kid in (K_VEC_F32_16, K_VEC_16) and "yF" not in c.outs:
        return "poly"
    return "fast"


def piece_prec(c, build):
    """The piece type of a case's pair rows / planes, as a gemm_split precision (2 = bf16, 3 = IEEE half)."""
    return c.pk if c.pk else PIECE_PREC[build]


# ---------------------------------------------------------------------------------------------------------------------------------
# pair rows: 32-element blocks of 128 bytes, 64 bytes of hi pieces then 64 of lo pieces (csrc/device_util.h store_pairs)
def pack_pairs(hi, lo):
    """(rows, D) 16-bit hi and lo -> (rows, D) int32: the image of the pair-row tensor over the fp32 tensor it replaces."""
    R, D = hi.shape
    h = hi.contiguous().view(torch.int16).reshape(R, D // 32, 1, 32)
    l_ = lo.contiguous().view(torch.int16).reshape(R, D // 32, 1, 32)
    return torch.cat([h, l_], dim=2).reshape(R, D // 32, 64).contiguous().view(torch.int32).reshape(R, D)


def unpack_pairs(buf, dtype):
    """(rows, D) int32 pair-row image -> (hi, lo), (rows, D) each, in the piece type."""
    R, D = buf.shape
    p = buf.contiguous().view(torch.int16).reshape(R, D // 32, 2, 32)
    return p[:, :, 0].reshape(R, D).contiguous().view(dtype), p[:, :, 1].reshape(R, D).contiguous().view(dtype)


# ---------------------------------------------------------------------------------------------------------------------------------
def _kind_rows(c, g):
    """(rows, D) fp32: the value each row's t is meant to have, and the spread of its addends."""
    R, D = c.rows, c.D
    w = torch.empty(R, D)
    spread = torch.empty(R)
    for r in range(R):
        kind = KINDS[(r + c.idx) % len(KINDS)]
        n = torch.randn(D, generator=g)
        if kind == "normal":
            w[r], spread[r] = n, 1.0
        elif kind == "mean100":
            w[r], spread[r] = 100.0 + 0.1 * n, 0.1
        elif kind == "tiny":
            w[r], spread[r] = 1e-3 * n, 1e-3
        elif kind == "constant":
            w[r], spread[r] = 0.7306, 0.0
        elif kind == "zeros":
            w[r], spread[r] = 0.0, 0.0
        elif kind == "outlier":
            n[int(torch.randint(0, D, (1,), generator=g))] = 300.0
            w[r], spread[r] = n, 1.0
        elif kind == "big":
            w[r], spread[r] = (1e4 * n).clamp(-4e4, 4e4), 1e4
        else:
            w[r], spread[r] = torch.linspace(-2.0, 3.0, D), 1.0
    return w, spread


def kinds_of(c):
    return [KINDS[(r + c.idx) % len(KINDS)] for r in range(c.rows)]


def make_inputs(c, build):
    """Every input buffer of a case as the kernel reads it (CPU tensors), gamma, beta, and t32 (module docstring)."""
    dtype = G.BUILDS[build][1]
    g = torch.Generator().manual_seed(1000 + c.idx)
    R, D = c.rows, c.D
    w, spread = _kind_rows(c, g)
    inp = {}
    addend = lambda s=0.25: s * spread[:, None] * torch.randn(R, D, generator=g)   # noqa: E731
    if c.form == 0:
        rest = w.clone()
        if c.add:
            inp["add"] = addend()
            rest = rest - inp["add"]
        if c.addP:   # the residual stream as pair rows carries the row, x is the branch added to it
            branch = addend()
            hi, lo = GS.cut(rest - branch, GS.PIECE[c.pk][0])
            inp["addP"] = pack_pairs(hi, lo)
            rest = branch
        inp["x"] = rest if c.x == "f32" else rest.to(dtype)
        t = inp["x"].float()
        if c.add:
            t = t + inp["add"]
        if c.addP:
            hi, lo = unpack_pairs(inp["addP"], GS.PIECE[c.pk][0])
            t = t + (hi.float() + lo.float())
    elif c.src == "x32":
        inp["x32"] = w
        t = w.clone()
    else:
        rest = w.clone()
        if c.form == 1 and c.branch:
            inp["branch"] = addend().to(dtype)
            rest = rest - inp["branch"].float()
        if c.form == 2:
            if c.grid:
                inp["parts"] = torch.randint(-512, 513, (c.nparts, R, D), generator=g).float() * 2.0 ** -10
                inp["pbias"] = torch.randint(-256, 257, (D,), generator=g).float() * 2.0 ** -10
            else:
                inp["parts"] = torch.randn(c.nparts, R, D, generator=g) * (0.5 / c.nparts ** 0.5)
                inp["pbias"] = 0.2 * torch.randn(D, generator=g)
            a = inp["parts"][0].clone()
            for k in range(1, c.nparts):
                a = a + inp["parts"][k]
            br = (a + inp["pbias"]).to(dtype).float()
            rest = rest - br
        inp["rh"], inp["rl"] = GS.cut(rest, dtype)
        t = inp["rh"].float() + inp["rl"].float()
        if c.form == 1 and c.branch:
            t = t + inp["branch"].float()
        if c.form == 2:
            t = t + br
    assert t.dtype == torch.float32 and torch.isfinite(t).all()
    if c.unit:
        inp["gamma"], inp["beta"] = torch.ones(D), torch.zeros(D)
    else:
        inp["gamma"], inp["beta"] = 1.0 + 0.3 * torch.randn(D, generator=g), 0.2 * torch.randn(D, generator=g)
    inp["t32"] = t
    return inp


def reference(c, build, inp):
    """(ref, lim32) in fp64, (rows, D) each (module docstring)."""
    D = c.D
    t = inp["t32"].double()
    gam, bet = inp["gamma"].double(), inp["beta"].double()
    eps = float(torch.tensor(c.eps, dtype=torch.float32))
    mu = t.mean(1, keepdim=True)
    d = t - mu
    v = (d * d).mean(1, keepdim=True)
    r = (v + eps) ** -0.5
    z = d * r
    y = z * gam + bet
    e_mu = (D + 1) * U * t.abs().mean(1, keepdim=True)
    e_d = e_mu + U * d.abs()
    rho_v = ((D + 2) * U * v + 2 * (d.abs() * e_d).mean(1, keepdim=True) + (e_d * e_d).mean(1, keepdim=True)) / (v + eps) + 2 * U
    rho_r = rho_v / 2 + 2 * U
    e_z = e_d * r + z.abs() * (rho_r + 2 * U)
    lim_y = gam.abs() * e_z + 2 * U * ((z * gam).abs() + bet.abs())
    if c.gelu:
        return G.gelu64(y), 1.13 * lim_y + G.g_act(gelu_form(c), build, y)
    return y, lim_y


_cache = collections.OrderedDict()


def case_data(c, build):
    """(inputs, ref, lim32) of a case in a build, computed once and shared (the CPU test and the GPU test of a case use the same tensors)."""
    key = (c.idx, build)
    if key not in _cache:
        inp = make_inputs(c, build)
        _cache[key] = (inp,) + reference(c, build, inp)
        while len(_cache) > 8:
            _cache.popitem(last=False)
    _cache.move_to_end(key)
    return _cache[key]


# ---------------------------------------------------------------------------------------------------------------------------------
def _bits(x):
    return x.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[x.element_size()])


def _worst(ratio):
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    i = int(ratio.argmax())
    return ratio.flatten()[i].item(), i // ratio.shape[1], i % ratio.shape[1]


def check_outputs(c, build, inp, ref, lim32, outs):
    """outs: what the kernel left in its output buffers, rows 0 .. rows - 1 (CPU tensors): "yT" in its type, "yF" / "sumF" fp32, "yP" the int32
    pair-row image, "yh" / "yl" 16-bit.  Returns (failures, report): failures is a list of texts, empty when every check of the module
    docstring holds; report maps a check's name to (worst err / limit, row, column)."""
    _, dtype, u_out = G.BUILDS[build]
    fails, report = [], {}
    want = set(c.outs) | ({"yh", "yl"} if c.form else set())
    assert set(outs) == want, (set(outs), want)

    def limit_check(name, got, lim):
        if torch.isnan(got).any():
            fails.append(f"{name}: {int(torch.isnan(got).sum())} NaN (unwritten) elements")
        err = (got.double() - ref).abs()
        w, r, col = _worst(torch.where(err == 0, torch.zeros_like(err), err / lim))   # (a zero row under gamma = 1, beta = 0: limit 0, met exactly)
        report[name] = (w, r, col)
        if not w <= 1.0:
            fails.append(f"{name}: err / limit {w:.3g} at row {r} column {col}")

    def same_bits(name, got, exp):
        bad = _bits(got) != _bits(exp)
        if bad.any():
            i = int(bad.flatten().float().argmax())
            fails.append(f"{name}: {int(bad.sum())} of {bad.numel()} elements differ, first at row {i // c.D} column {i % c.D}")

    zero_rows = (inp["t32"] == 0).all(1)
    yF = outs.get("yF")
    if yF is not None:
        limit_check("yF", yF, lim32 + U * ref.abs())
        if not c.gelu and zero_rows.any():
            same_bits("yF of a zero row == beta", yF[zero_rows], inp["beta"].expand(int(zero_rows.sum()), c.D))
    if "sumF" in outs:
        same_bits("sumF == t32", outs["sumF"], inp["t32"])
    if "yT" in outs:
        yT = outs["yT"]
        if yT.dtype == torch.float32:
            limit_check("yT", yT, lim32 + U * ref.abs())
            exp_zero = inp["beta"]
        else:
            if torch.isnan(yT.float()).any():
                fails.append(f"yT: {int(torch.isnan(yT.float()).sum())} NaN (unwritten) elements")
            lo, hi = (ref - lim32).float().to(dtype).double(), (ref + lim32).float().to(dtype).double()
            out = ~((yT.double() >= lo) & (yT.double() <= hi))
            if out.any():
                i = int(out.flatten().float().argmax())
                fails.append(f"yT: {int(out.sum())} elements outside [rn16(ref - lim32), rn16(ref + lim32)], first at row {i // c.D} column {i % c.D}")
            report["yT outside its interval"] = (float(out.sum()), 0, 0)
            report["yT (information)"] = _worst((yT.double() - ref).abs() / (lim32 + u_out * ref.abs() + G.ETA[build]))
            exp_zero = inp["beta"].to(dtype)
            if yF is not None:
                same_bits("yT == rn16(yF)", yT, yF.to(dtype))
        if not c.gelu and zero_rows.any():
            same_bits("yT of a zero row == beta", yT[zero_rows], exp_zero.expand(int(zero_rows.sum()), c.D))
    pieces = None
    if "yP" in outs:
        pieces = ("yP",) + unpack_pairs(outs["yP"], GS.PIECE[c.pk][0])
    elif c.form:
        pieces = ("(yh, yl)", outs["yh"], outs["yl"])
    if pieces is not None:
        name, hi, lo = pieces
        pp = piece_prec(c, build)
        got = hi.float() + lo.float()
        limit_check(name, got, lim32 + GS.cut_term(pp, ref))
        if yF is not None:
            eh, el = GS.cut(yF, GS.PIECE[pp][0])
            same_bits(f"hi of {name} == hi of cut(yF)", hi, eh)
            same_bits(f"lo of {name} == lo of cut(yF)", lo, el)
        if not c.gelu and zero_rows.any():
            n = int(zero_rows.sum())
            eh, el = GS.cut(inp["beta"].expand(n, c.D).contiguous(), GS.PIECE[pp][0])
            same_bits(f"{name} of a zero row == cut(beta)", torch.stack([hi[zero_rows], lo[zero_rows]]), torch.stack([eh, el]))
    return fails, report


# ---------------------------------------------------------------------------------------------------------------------------------
# A correct kernel, simulated on the CPU in fp32 (tests/test_layernorm_limit.py), and the mutants the checks must catch
MUTANTS = ("variance over D - 1", "mean misses the last element", "eps 1e-6 for 1e-5", "gamma shifted by one column", "lo of the input dropped",
           "yl written as zero", "yl not cut from o", "branch not added", "one part skipped", "bias added after the rounding",
           "half-waves read each other's rows", "last row skipped when rows is odd", "GELU in the wrong form")


def applies(mutant, c):
    """The cases a mutant must show in: the forms that have what it breaks, with at least one row of a kind on which the damage is larger
    than the limit.  The limit is a worst-case bound, so it is wide exactly where fp32 itself is inaccurate: a row of mean 100 and spread 0.1
    may move by (D + 1) u 100 / 0.1 = 0.06 of a standard deviation at D = 1024, and a row of scale 1e4 by 1e-4 of 1e4.  What each mutant
    changes, against that:
      variance over D - 1       z by |z| / 2 D = 4e-4 |z| at D = 1280: seen on rows whose limit is fp32-sized (normal, outlier, big, ramp)
      mean misses the last      mu by t_last / D: nothing on a zero row
      eps                       only where v is near eps: the rows of spread 1e-3
      gamma shifted             0.4 |z|: every row with z != 0
      lo of the input dropped   t by up to 2^-12 |t| (IEEE-half pieces); a constant row stays constant, a zero row zero
      yl zero                   y by up to 2^-12 |y|: not on a mean-100 row unless yF stands beside the planes (then cut(yF) sees it everywhere)
      yl not cut from o         one unit of lo's last place: only the identity with cut(yF) sees it
      branch not added          a quarter of the row's spread; the constant and the zero row have no branch
      one part skipped          t by a part, 0.25 N(0, 1): everywhere but on a row of scale 1e4
      bias after the rounding   t by 2^-12 of the branch (IEEE half): rows whose own t is small (spread 1e-3, zeros).  Not in the grid case,
                                where a and a + bias are multiples of 2^-10 below 4 and IEEE half holds both exactly
      half-waves swapped, last row skipped      every row
      GELU in the wrong form    the polynomial where gelu_erf is due: up to 1e-4 |y|, not on a mean-100 row, and not at D = 1280, where the
                                fp32 stage's own limit, 1e-4 (1 + |z|), is as wide as the polynomial's error; and only where an output keeps
                                more than 16 bits (fp32 rows, pair rows): under a 16-bit store alone the polynomial's error is below the store's
                                rounding, which is why the kernels use it there.  (gelu_erf where the polynomial is due
                                is inside the polynomial's documented error by construction: not a mutant the limit can or should see.)"""
    i = MUTANTS.index(mutant)
    kinds = set(kinds_of(c))
    planes = "yP" in c.outs or c.form != 0
    if i == 0:
        return bool(kinds & {"normal", "outlier", "big", "ramp"})
    if i == 1:
        return bool(kinds - {"zeros"})
    if i == 2:
        return "tiny" in kinds and c.eps == 1e-5
    if i == 3:
        return not c.unit and bool(kinds - {"constant", "zeros"})
    if i == 4:
        return (c.addP or c.src == "hilo") and bool(kinds - {"constant", "zeros"})
    if i == 5:
        return planes and ("yF" in c.outs or bool(kinds - {"mean100"}))
    if i == 6:
        return planes and "yF" in c.outs
    if i == 7:
        return (c.add or c.branch) and bool(kinds - {"constant", "zeros"})
    if i == 8:
        return c.form == 2 and c.nparts == 4 and bool(kinds - {"big"})
    if i == 9:
        return c.form == 2 and not c.grid and bool(kinds & {"tiny", "zeros"})
    if i == 10:
        return c.kid in TWO_ROW_IDS and c.rows >= 2
    if i == 11:
        return c.kid in TWO_ROW_IDS and c.rows % 2 == 1
    wide_out = c.prec == 0 or "yF" in c.outs or "yP" in c.outs
    return bool(c.gelu) and gelu_form(c) == "fast" and wide_out and c.D <= 1024 and bool(kinds & {"normal", "tiny", "outlier", "big", "ramp"})


def _sum_one_row(t):
    """Row sums in the one-row kernels' order: lane i of 64 adds elements i, i + 64, ... in turn, then six butterfly steps."""
    R, D = t.shape
    pad = torch.zeros(R, (D + 63) // 64 * 64)
    pad[:, :D] = t
    lanes = torch.zeros(R, 64)
    for j in range(pad.shape[1] // 64):
        lanes = lanes + pad[:, 64 * j:64 * j + 64]
    return _butterfly(lanes)


def _sum_two_rows(t):
    """Row sums in the two-row kernels' order: lane i of 32 holds 8 consecutive elements per chunk, added pairwise, then five exchange steps."""
    R, D = t.shape
    ch = t.reshape(R, D // 256, 32, 8)
    lanes = torch.zeros(R, 32)
    for j in range(D // 256):
        v = ch[:, j]
        lanes = lanes + (((v[..., 0] + v[..., 1]) + (v[..., 2] + v[..., 3])) + ((v[..., 4] + v[..., 5]) + (v[..., 6] + v[..., 7])))
    return _butterfly(lanes)


def _butterfly(lanes):
    n = lanes.shape[1]
    idx = torch.arange(n)
    o = n // 2
    while o:
        lanes = lanes + lanes[:, idx ^ o]
        o //= 2
    return lanes[:, :1]


def gelu_poly32(x, build):
    """gelu_bf16x2 of csrc/common.h in torch fp32, for the build."""
    if build == "bf16":
        t = x.clamp(-3.8, 3.8)
        u = t * t
        q = u * 3.6657791326e-08 + (-2.2724625145e-06)
        for coef in (6.0684808363e-05, -9.3154765044e-04, 9.3166354115e-03, -6.5719787820e-02, 3.9867674568e-01):
            q = q * u + coef
        return x * (t * q + 0.4999907314777374)
    z = (x * 0.70710678118654752440).clamp(-3.0, 3.0)
    u = z * z
    q = u * 4.074456683e-08 + (-1.944940095e-06)
    for coef in (4.106299457e-05, -5.110675702e-04, 4.235681612e-03, -2.510436811e-02, 1.110860035e-01, -3.753373921e-01, 1.128336072e+00):
        q = q * u + coef
    pe = (z * q).clamp(-1.0, 1.0)
    hx = x * 0.5
    return hx * pe + hx


def simulate(c, build, inp, order="one", mutant=None):
    """The outputs of a correct fp32 two-pass kernel (order "one": a wave per row, "two": half a wave per row -- D a multiple of 256), stored
    as the real kernels store, into NaN-poisoned buffers.  mutant: one of MUTANTS."""
    dtype = G.BUILDS[build][1]
    m = MUTANTS.index(mutant) if mutant else -1
    D, R = c.D, c.rows
    f = lambda x: x.float()   # noqa: E731
    # ---- t, in the kernels' order
    if c.form == 0:
        t = f(inp["x"])
        if c.add and m != 7:
            t = t + inp["add"]
        if c.addP:
            hi, lo = unpack_pairs(inp["addP"], GS.PIECE[c.pk][0])
            t = t + (f(hi) + (f(lo) if m != 4 else 0.0))
    elif c.src == "x32":
        t = inp["x32"].clone()
    else:
        t = f(inp["rh"]) + (f(inp["rl"]) if m != 4 else 0.0)
        if c.form == 1 and c.branch and m != 7:
            t = t + f(inp["branch"])
        if c.form == 2:
            parts = [inp["parts"][k] for k in range(c.nparts) if not (m == 8 and k == 2)]
            a = parts[0].clone()
            for p in parts[1:]:
                a = a + p
            t = t + (f((a + inp["pbias"]).to(dtype)) if m != 9 else f(a.to(dtype)) + inp["pbias"])
    if m == 10:   # the two half-waves of a wave swap rows; an odd last row has no partner
        perm = torch.arange(R)
        for r in range(0, R - 1, 2):
            perm[r], perm[r + 1] = r + 1, r
        t_in = t[perm]
    else:
        t_in = t
    # ---- statistics, fp32 two-pass
    rsum = _sum_one_row if order == "one" else _sum_two_rows
    inv_d = torch.tensor(1.0 / D, dtype=torch.float32)
    s = rsum(torch.cat([t_in[:, :D - 1], torch.zeros(R, 1)], 1)) if m == 1 else rsum(t_in)
    mean = s * inv_d
    d = t_in - mean
    q = rsum(d * d)
    var = q * (torch.tensor(1.0 / (D - 1), dtype=torch.float32) if m == 0 else inv_d)
    eps = torch.tensor(1e-6 if m == 2 else c.eps, dtype=torch.float32)
    rstd = (var + eps).double().rsqrt().float()
    gam = inp["gamma"].roll(1) if m == 3 else inp["gamma"]
    o = (d * rstd) * gam + inp["beta"]
    if c.gelu:
        form = gelu_form(c)
        if m == 12:
            form = "fast" if form == "poly" else "poly"
        o = gelu_poly32(o, build) if form == "poly" else torch.nn.functional.gelu(o.double()).float()
    if m == 11 and R % 2:
        o = o.clone()
        o[R - 1] = float("nan")   # never written: the poison stays
    # ---- stores
    outs = {}
    if "yT" in c.outs:
        outs["yT"] = o.clone() if c.prec == 0 else o.to(dtype)
    if "yF" in c.outs:
        outs["yF"] = o.clone()
    if "sumF" in c.outs:
        outs["sumF"] = t.clone()
    if "yP" in c.outs or c.form:
        pd = GS.PIECE[piece_prec(c, build)][0]
        hi = o.to(pd)
        if m == 5:
            lo = torch.zeros_like(hi)
        elif m == 6:
            lo = G.truncate_to(o - hi.float(), pd)   # cut, but not rounded to nearest: the piece is no longer that of cut(yF)
        else:
            lo = (o - hi.float()).to(pd)
        if m == 11 and R % 2:
            lo[R - 1] = float("nan")
        if "yP" in c.outs:
            outs["yP"] = pack_pairs(hi, lo)
        else:
            outs["yh"], outs["yl"] = hi, lo
    return outs


def orders(c):
    return ("one", "two") if c.D % 256 == 0 else ("one",)
