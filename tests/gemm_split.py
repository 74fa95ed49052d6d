"""What tests/test_gpu_gemm_split_kernels.py (GPU) and tests/test_gemm_limit.py (CPU) share for the split-operand GEMM kernels (precision
bf16x3 = 2 / fp16x3 = 3: fp32 operands cut into 16-bit (hi, lo) pieces, three MFMAs per K block) and for the fp32 parity mode of the
register-staged kernel: the case tables, the operand generators and the fp64 references.

The reference is the three-term value, not the fp64 product.  A piece type has unit roundoff u (2^-8 bf16, 2^-11 IEEE half); the cut is
deterministic, hi = rn(x), lo = rn(x - hi) (csrc/device_util.h cut_piece, csrc/gemm_ring.h cut8, csrc/gemm.hip split4), and
`x.to(dtype)`, `(x - hi.float()).to(dtype)` reproduce it.  In fp64

    T = Ah Wh^T + Al Wh^T + Ah Wl^T (+ bias)

is what a correct kernel computes up to its fp32 accumulation; it leaves out Al Wl^T, so it differs from the fp64 product of the
operands in nearly every element and a kernel that computes anything else is visible.  How far T is from the true product is a property
of the mode, not of a kernel: tests/test_gemm_limit.py checks that bound on the CPU (mode_bound below).

Three kinds of case:

EXACT   operands a = P + Q 2^-s, P and Q from {+-1, +-2}, s = 12 (bf16 pieces) / 14 (IEEE half): hi = P and lo = Q 2^-s exactly, every
        product and every partial sum in ANY order is an integer multiple of 2^-s, and fp32 accumulation is exact while
        (K (pmax^2 + 4 pmax 2^-s) + |bias| + |resid|) 2^s < 2^24 (exact_inputs asserts it and restricts P to +-1 where +-2 would break it).  got
        must equal T bit for bit.  The smallest term a kernel can lose is 2^-s: nothing can hide.
RANDOM  operands as gemm_limit.make_inputs draws them, under the per-element limit of gemm_limit.py with 3 K products:
            u_out |ref| + 1.13 (3 K + 2) 2^-23 S3 + g_act(z) + 2^-23 |resid|,   S3 = |Ah||Wh|^T + |Al||Wh|^T + |Ah||Wl|^T + |bias|
        (pair / plane output: + u^2 |ref|, + 2^-25 for IEEE-half pieces: the stored value is itself cut).  THIS LIMIT IS BLIND TO A SINGLE
        LOST TERM: Al Wh of one 32-element K block of one row is about 1.9e-3 / sqrt K (bf16) or 2.4e-4 / sqrt K (IEEE half), while the
        summation bound grows with K -- at K = 768 the lost term is 0.09 (bf16) / 0.01 (IEEE half) of the limit (tests/test_gemm_limit.py asserts
        that this mutant passes there; only at K = 64 is it seen in both piece types).  The random cases are here for the
        guard rows, the NaN poison, GELU, fractional biases, N tails and conv rows; the sharp check of the arithmetic is the EXACT table.
CUT     one operand one-hot with value 1 (hi = 1, lo = 0): C[m, n] = hi(x) + lo(x) of the other operand's grid, at most 24 bits, exact in
        fp32 -> bit equality over the whole magnitude range (cut_grid)."""
import collections

import torch

import gemm_limit as G

# piece type of a split precision: (dtype, u, s of the exact operands, eta = half the spacing of its subnormals)
PIECE = {2: (torch.bfloat16, 2.0 ** -8, 12, 2.0 ** -134), 3: (torch.float16, 2.0 ** -11, 14, 2.0 ** -25)}

# kid: the id svt_debug_set(39, 0) must report.  out_kind: None = svt_debug_gemm; 0 / 1 / 2 = svt_debug_gemm_pairs writing fp32 rows / pair rows /
# (hi, lo) planes.  keys as in gemm_limit.Case.  prec: None = both split precisions, 0 = the fp32 parity mode (family 2)
class SCase(collections.namedtuple("SCase", "kid M N K conv act resid bias out_kind prec keys")):
    __slots__ = ()
    out_f32 = 1   # every output here is fp32


def S(kid, M, N, K, conv=None, act=0, resid=False, bias=True, out_kind=None, prec=None, **keys):
    fam = kid // 1000
    if fam in (9, 10) and out_kind is None:
        out_kind = 0
    assert (out_kind is not None) == (fam in (9, 10)), "families 9 and 10 run through svt_debug_gemm_pairs, the others through svt_debug_gemm"
    return SCase(kid, M, N, K, conv, act, resid, bias, out_kind, prec, tuple(sorted((int(k[1:]), v) for k, v in keys.items())))


def case_id(c):
    s = f"k{c.kid}-{c.M}x{c.N}x{c.K}"
    if c.conv:
        s += "-conv"
    s += ("", "-gelu", "-relu")[c.act] + ("-resid" if c.resid else "") + ("" if c.bias else "-nobias")
    s += ("", "-rows", "-pairs", "-planes")[0 if c.out_kind is None else c.out_kind + 1]
    return s + "".join(f"-key{k}={v}" for k, v in c.keys)


def precisions(c):
    return (0,) if c.prec == 0 else (2, 3)


def library(c):
    """The build a case runs in: gemm_p1x_kernel (family 10) is an A/B arm that only the diagnostic build of the bf16 library holds."""
    return "diag" if c.kid // 1000 == 10 else None


CONV = G.CONV   # 60 overlapping rows per clip: M = 60 B


def _pair_family(fam, ks, k_long, extra):
    """gemm_x3q_kernel (9) / gemm_p1x_kernel (10): every tile height x every output, the contract minimum of K and the longest exact K; one valid
    row in the last tile (bm + 1); 22 tiles on 8 workgroups (two or three tiles per workgroup, both parities)."""
    exact, rand = [], []
    for bm in (128, 192, 256):
        kid = 1000 * fam + bm
        for ok in (0, 1, 2):
            exact += [S(kid, 300, 256, ks[0], out_kind=ok, k1=bm, **extra), S(kid, bm + 1, 512, k_long, out_kind=ok, bias=ok != 1, k1=bm, **extra)]
            rand += [S(kid, 300, 512, ks[1], out_kind=ok, k1=bm, **extra), S(kid, bm + 1, 256, ks[2], out_kind=ok, bias=ok != 2, k1=bm, **extra)]
        for ok in (0, 1):
            rand += [S(kid, 300, 256, ks[0], act=1, out_kind=ok, k1=bm, **extra)]
        exact += [S(kid, 2600, 512, ks[2], out_kind=0, k1=bm, k37=8, **extra)]
        rand += [S(kid, 300, 256, 192, conv=CONV, out_kind=0, k1=bm, **extra)]
    exact += [S(1000 * fam + 256, 2600, 512, k_long, out_kind=1, k1=256, k37=8, **extra), S(1000 * fam + 128, 2600, 512, ks[0], out_kind=2, k1=128, k37=8, **extra),
              S(1000 * fam + 128, 300, 256, 192, conv=CONV, out_kind=1, k1=128, **extra)]
    rand += [S(1000 * fam + 128, 2600, 512, ks[1], act=1, out_kind=1, k1=128, k37=8, **extra),
             S(1000 * fam + 128, 300, 256, ks[1], out_kind=0, **extra)]   # key 1 = 0: the cost model's own height
    return exact, rand


_X3Q_EXACT, _X3Q_RANDOM = _pair_family(9, (64, 96, 192), 512, {})
_P1X_EXACT, _P1X_RANDOM = _pair_family(10, (96, 128, 192), 512, {"k30": 1})

# ---- bit-equal cases.  K = 512: every slot of the five-slot LDS ring is used six times (IEEE-half pieces: P restricted to +-1 there)
EXACT = [
    # gemm_x3s_kernel: M at the contract minimum, one valid row in the last tile, one slab, N tails, the 192-column form, every exact epilogue
    S(7256, 128, 128, 32), S(7256, 257, 256, 192, act=2, resid=True), S(7256, 300, 260, 512), S(7256, 300, 200, 64, bias=False),
    S(7256, 128, 256, 96, resid=True), S(7192, 300, 192, 96), S(7192, 257, 384, 512, bias=False), S(7192, 128, 192, 32, act=2),
    S(7256, 180, 256, 192, conv=CONV),
    # gemm_x3p_kernel, forced (key 3 = 34): K at its minimum, several tiles per workgroup (key 37 = 8: 12 and 22 tiles)
    S(8256, 300, 256, 64, k3=34), S(8256, 300, 512, 96, bias=False, k3=34), S(8256, 300, 512, 512, k3=34), S(8256, 300, 256, 192, conv=CONV, k3=34),
    S(8256, 1500, 512, 192, k3=34, k37=8), S(8256, 2600, 512, 64, k3=34, k37=8), S(8256, 2600, 512, 512, bias=False, k3=34, k37=8),
    # the split instantiation of the register-staged kernel: below the LDS-DMA kernels' minimum, a K tail with scalar stores, forced (key 11 = 0)
    S(12256, 24, 64, 32), S(12256, 499, 20, 772), S(12128, 300, 256, 96, act=2, resid=True, k11=0), S(12128, 300, 200, 512, k11=0),
    # family 2 at precision 0 (the fp32 parity mode): plain small-integer operands
    S(2256, 24, 64, 32, prec=0), S(2256, 499, 20, 772, prec=0), S(2128, 300, 256, 96, act=2, resid=True, prec=0), S(2128, 300, 200, 512, prec=0),
] + _X3Q_EXACT + _P1X_EXACT

# ---- cases under the derived limit, with 64 poisoned guard rows on each side of the output
RANDOM = [
    S(7256, 128, 128, 32), S(7256, 257, 200, 64, act=1), S(7256, 300, 260, 96, act=2), S(7256, 300, 256, 192, resid=True), S(7256, 257, 128, 192, act=1, resid=True),
    S(7256, 128, 260, 64, bias=False), S(7192, 300, 192, 96, act=1), S(7192, 257, 384, 192, resid=True), S(7256, 180, 200, 192, conv=CONV, act=1),
    S(8256, 300, 256, 64, act=1, k3=34), S(8256, 300, 512, 96, k3=34), S(8256, 300, 512, 192, bias=False, k3=34), S(8256, 300, 256, 192, conv=CONV, act=1, k3=34),
    S(8256, 1500, 512, 96, act=1, k3=34, k37=8), S(8256, 2600, 512, 192, k3=34, k37=8),
    S(8256, 32769, 512, 64, act=1),   # 258 tiles with GELU: the dispatcher's own choice, one valid row in the last tile row
    S(12256, 24, 64, 32, act=1), S(12256, 499, 20, 772, resid=True), S(12128, 300, 256, 96, act=1, k11=0), S(12128, 300, 200, 96, resid=True, k11=0),
    S(2256, 24, 64, 32, act=1, prec=0), S(2256, 499, 20, 772, resid=True, prec=0), S(2128, 300, 256, 96, act=1, prec=0), S(2128, 300, 200, 72, resid=True, prec=0),
] + _X3Q_RANDOM + _P1X_RANDOM

# ---- the cut and GELU alone: one launch shape per family (the one-hot operand's K is padded with zero columns beyond the 64 in use)
ALONE = [
    S(7256, 128, 512, 64), S(8256, 128, 512, 64, k3=34), S(12128, 128, 512, 64, k11=0),
    S(9128, 128, 512, 64, out_kind=0, k1=128), S(9128, 128, 512, 64, out_kind=1, k1=128),
    S(10128, 128, 512, 96, out_kind=0, k1=128, k30=1), S(10128, 128, 512, 96, out_kind=1, k1=128, k30=1),
]


def tile_shape(kid):
    """(rows, columns) of a kernel id's output tile; 7192 names the 192-COLUMN form of gemm_x3s_kernel's 256-row tile."""
    if kid == 7192:
        return 256, 192
    return G.tile_shape(kid)


def cut(x, dtype):
    """(hi, lo) of fp32 x as the kernels cut it: hi = rn(x), lo = rn(x - hi), both in `dtype`."""
    hi = x.to(dtype)
    return hi, (x - hi.float()).to(dtype)


def recombine(x, dtype):
    """hi + lo of fp32 x in fp32, as the pair / plane outputs are read back; exact (the two pieces span at most 24 bits)."""
    hi, lo = cut(x, dtype)
    y = hi.float() + lo.float()
    assert torch.equal(y.double(), hi.double() + lo.double()), "hi + lo does not fit fp32"
    return y


def _conv_rows(A, c):
    T_in, T_out, st, cin = c.conv
    idx = (torch.arange(T_out) * st)[:, None] + torch.arange(c.K // cin)[None, :]
    return A[:, idx].reshape(c.M, c.K)


def exact_inputs(c, prec, seed=0):
    """Operands whose three-term arithmetic is exact in fp32 in any order (module docstring), as dict like gemm_limit.make_inputs: A, rows, W, bias,
    resid, addr.  Refuses (AssertionError) a case whose partial sums could leave fp32's 24 bits.  prec 0: plain integers from {-2 .. 2}."""
    g = torch.Generator().manual_seed(seed)
    M, N, K = c.M, c.N, c.K
    bmax, rmax = (3 if c.bias else 0), (4 if c.resid else 0)
    if prec == 0:
        s, pmax, q = 0, 2, 0.0
        assert K * 4 + bmax + rmax < 2 ** 24
    else:
        dtype, _, s, _ = PIECE[prec]
        q = 2.0 ** -s
        fits = [p for p in (2, 1) if (K * (p * p + 4 * p * q) + bmax + rmax) * 2 ** s < 2 ** 24]
        assert fits, f"K = {K} is too long for exact fp32 accumulation with {dtype} pieces"
        pmax = fits[0]

    def draw(shape):
        if prec == 0:
            return torch.randint(-2, 3, shape, generator=g).float()
        sign = lambda: (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()   # noqa: E731
        P = torch.randint(1, pmax + 1, shape, generator=g).float() * sign()
        Q = torch.randint(1, 3, shape, generator=g).float() * sign()
        x = P + Q * q
        hi, lo = cut(x, dtype)
        assert torch.equal(hi.float(), P) and torch.equal(lo.float(), Q * q), "the exact operands do not cut into (P, Q 2^-s)"
        return x

    if c.conv:
        T_in, T_out, st, cin = c.conv
        A = draw((M // T_out, T_in, cin))
        rows, addr = _conv_rows(A, c), (T_out, T_in * cin, st * cin)
    else:
        A = draw((M, K))
        rows, addr = A, (M, 0, K)
    W = draw((N, K))
    bias = torch.randint(-bmax, bmax + 1, (N,), generator=g).float() if c.bias else None
    resid = torch.randint(-rmax, rmax + 1, (M, N), generator=g).float() if c.resid else None
    return dict(A=A, rows=rows.double(), W=W, bias=bias, resid=resid, addr=addr)


def three_term(rows, W, prec):
    """(T, S3) in fp64 without the bias, from fp32 rows (M, K) and W (N, K).  prec 0: the plain product and |A||W|^T."""
    if prec == 0:
        return rows.double() @ W.double().t(), rows.double().abs() @ W.double().abs().t()
    dtype = PIECE[prec][0]
    ah, al = (t.double() for t in cut(rows, dtype))
    wh, wl = (t.double() for t in cut(W, dtype))
    # (ah + al is exact in fp64, so the two products below are the three terms)
    return (ah + al) @ wh.t() + ah @ wl.t(), (ah.abs() + al.abs()) @ wh.abs().t() + ah.abs() @ wl.abs().t()


def reference(c, inp, prec, alpha=1.0):
    """(z, S3, ref) in fp64: ref = act(alpha T + bias) + resid, and for pair / plane output its (hi, lo) cut read back as hi + lo."""
    z, S3 = three_term(inp["rows"].float(), inp["W"], prec)
    if alpha != 1.0:
        z, S3 = z * alpha, S3 * abs(alpha)
    if inp["bias"] is not None:
        z = z + inp["bias"].double()
        S3 = S3 + inp["bias"].double().abs()
    ref = G.gelu64(z) if c.act == 1 else torch.relu(z) if c.act == 2 else z.clone()
    if inp["resid"] is not None:
        ref = ref + inp["resid"].double()
    return z, S3, ref


def exact_expected(c, inp, prec):
    """The fp32 matrix an exact case must return bit for bit."""
    assert c.act != 1, "GELU is not exact"
    _, _, ref = reference(c, inp, prec)
    exp = ref.float()
    assert torch.equal(exp.double(), ref), "the exact case's value does not fit fp32"
    return recombine(exp, PIECE[prec][0]) if c.out_kind else exp


def limit(c, prec, z, S3, ref, resid, alpha=1.0):
    """The per-element limit of a random case (module docstring; gemm_limit.py derives the form, and the one more rounding of alpha != 1)."""
    terms = c.K if prec == 0 else 3 * c.K
    lim = 2.0 ** -24 * ref.abs() + 1.13 * (terms + 2 + (alpha != 1.0)) * 2.0 ** -23 * S3
    if c.act == 1:
        lim = lim + G.g_act("fast", None, z)   # every GELU of these kernels is gelu_erf / gelu_fast
    if resid is not None:
        lim = lim + 2.0 ** -23 * resid.double().abs()
    if c.out_kind:
        lim = lim + cut_term(prec, ref)
    return lim


def cut_term(prec, ref):
    """What the cut of a stored value adds: u^2 |ref|, and half the subnormal spacing of an IEEE-half lo piece."""
    u = PIECE[prec][1]
    return u * u * ref.abs() + (2.0 ** -25 if prec == 3 else 0.0)


def worst(c, got, ref, lim):
    tr, tc = tile_shape(c.kid)
    ratio = (got.double() - ref).abs() / lim
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    i = int(ratio.argmax())
    m, n = i // c.N, i % c.N
    return ratio.max().item(), (f"tile ({m // tr}, {n // tc}) row {m % tr} column {n} (row {m} of {c.M}); "
                                f"err {abs(got[m, n].item() - ref[m, n].item()):.3e} limit {lim[m, n].item():.3e}")


def first_mismatch(c, got, exp):
    """Text naming the first element of `got` that differs from `exp`, and how many do."""
    bad = got != exp
    i = int(bad.flatten().float().argmax())
    m, n = i // c.N, i % c.N
    tr, tc = tile_shape(c.kid)
    return (f"{int(bad.sum())} of {bad.numel()} elements differ; first at tile ({m // tr}, {n // tc}) row {m % tr} column {n} (row {m} of {c.M}): "
            f"got {got[m, n].item():.9g} expected {exp[m, n].item():.9g}")


def cut_grid(prec, n, seed=0):
    """n fp32 values over the piece type's whole range, inside the contract (nothing at or above 65520 for IEEE-half pieces, nothing that rounds
    to a bf16 infinity): every binade from 2^-100 to 2^100 (bf16) / from 2^-30 to just below 65520 (IEEE half: lo pieces that are subnormal --
    every |x| < 0.125 --, hi = 0 below 2^-25, and 65504 .. 65519) with random mantissas and both signs; +-0; one fp32 ulp below a power of two
    (hi rounds up, lo is negative); the halfway cases of the hi rounding and their fp32 neighbours."""
    g = torch.Generator().manual_seed(seed)
    dtype = PIECE[prec][0]
    lo_e, hi_e, keep = (-100, 100, 8) if prec == 2 else (-30, 15, 11)
    exps = torch.arange(lo_e, hi_e + 1, dtype=torch.float64)
    pw = 2.0 ** exps
    special = [torch.tensor([0.0, -0.0], dtype=torch.float64), pw, -pw, pw * (1 - 2.0 ** -24), -pw * (1 - 2.0 ** -24)]
    half = 2.0 ** -keep   # half an ulp of the piece type at 1: 1 + half and 1 + 3 half are the ties (to even: down, up)
    for m in (1 + half, 1 + 3 * half, 1 + half + 2.0 ** -23, 1 + half - 2.0 ** -23, 1 + 3 * half + 2.0 ** -23, 1 + 3 * half - 2.0 ** -23, 2 - half, 2 - half - 2.0 ** -23):
        special += [pw * m, -pw * m]
    if prec == 3:
        top = torch.arange(65504, 65520, dtype=torch.float64)
        sub = 2.0 ** -24 * torch.tensor([0.25, 0.5, 0.5 + 2.0 ** -20, 0.75, 1.0, 1.5, 2.5, 3.0, 1023.0, 1023.5, 1024.5], dtype=torch.float64)   # around the subnormal grid
        special += [top, -top, top + 0.5, sub, -sub, 0.125 * torch.tensor([1 - 2.0 ** -24, 1.0, 1 + 2.0 ** -11 + 2.0 ** -22], dtype=torch.float64)]
    special = torch.cat(special)
    k = n - special.numel()
    assert k >= exps.numel(), "the grid is too small for its special values and one value per binade"
    e = exps.repeat(k // exps.numel() + 1)[:k]
    mant = 1 + torch.rand(k, generator=g, dtype=torch.float64)
    sign = (torch.randint(0, 2, (k,), generator=g) * 2 - 1).double()
    x = torch.cat([special, sign * mant * 2.0 ** e]).float()
    if prec == 3:
        x = torch.where(x.abs() >= 65520.0, torch.copysign(torch.tensor(65519.996), x), x)
    assert torch.isfinite(x.to(dtype).float()).all(), "a grid value leaves the piece type's range"
    return x[torch.randperm(n, generator=g)]


def mode_bound(A, W, prec):
    """|T - fp64 product| <= 3 u^2 (1 + u)^2 |A||W|^T + eta (1 + u) (sum_k |a| + sum_k |w|): each piece pair (hi, lo) represents x to
    u^2 |x| + eta (eta: the lo piece's underflow, which dominates for IEEE-half pieces of values below 0.125, whose lo is subnormal), and the
    dropped Al Wl^T is at most u^2 (1 + u)^2 |A||W|^T.  The eta term charges every operand element an absolute eta against a partner of
    magnitude up to 1 + u -- operands in [-1, 1], as the tests draw them."""
    _, u, _, eta = PIECE[prec]
    A, W = A.double(), W.double()
    assert A.abs().max() <= 1 and W.abs().max() <= 1
    return 3 * u * u * (1 + u) ** 2 * (A.abs() @ W.abs().t()) + eta * (1 + u) * (A.abs().sum(1)[:, None] + W.abs().sum(1)[None, :])


# ---- a correct split kernel, simulated on the CPU (tests/test_gemm_limit.py), and the mutants the exact cases must catch ----
def simulate(rows, W, bias, prec, seed=0, mutant=None):
    """fp32 accumulation of the three piece products in 32-wide K blocks, in shuffled block order, from the bias.  mutant:
    "lost_term"  row 5 loses Al Wh of one 32-block        "shifted_lo"  A's lo plane is shifted by one element along K
    "fourth_term"  Al Wl is added                          "lost_block"  row 5 loses one whole K block"""
    dtype = PIECE[prec][0]
    ah, al = (t.float() for t in cut(rows, dtype))
    wh, wl = (t.float() for t in cut(W, dtype))
    if mutant == "shifted_lo":
        al = torch.roll(al, 1, dims=1)
    M, K = rows.shape
    acc = torch.zeros(M, W.shape[0]) if bias is None else bias.float().repeat(M, 1)
    order = torch.randperm(K // 32, generator=torch.Generator().manual_seed(seed)).tolist()
    for j, b in enumerate(order):
        sl = slice(32 * b, 32 * b + 32)
        terms = [(al, wh), (ah, wh), (ah, wl)] + ([(al, wl)] if mutant == "fourth_term" else [])
        for i, (x, y) in enumerate(terms):
            part = x[:, sl] @ y[:, sl].t()
            if j == len(order) // 2 and ((mutant == "lost_term" and i == 0) or mutant == "lost_block"):
                part[5] = 0.0
            acc = acc + part
    return acc


MUTANTS = ("lost_term", "shifted_lo", "fourth_term", "lost_block")
