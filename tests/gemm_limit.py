"""What tests/test_gpu_gemm_kernels.py (GPU) and tests/test_gemm_limit.py (CPU) share: the case tables of the 16-bit GEMM kernels, the
fp64 reference of a case and the per-element limit a correct kernel stays inside.  The second half of the file holds the same for the batched
launches (tests/test_gpu_gemm_batched.py) and for the score-matrix attention (tests/test_gpu_attention_scores.py), each under its own heading.

The limit is a bound, not a fitted tolerance.  With, in fp64 on the operands already rounded to the build's 16-bit type,

    z = A W^T + bias        S = |A| |W|^T + |bias|        ref = act(z) + resid

a kernel that accumulates in fp32 (in ANY order), applies the activation in fp32 and rounds the result once to the output type obeys

    |got - ref| <= u_out |ref| + eta_out + 1.13 (K + 2) 2^-23 S + g_act(z) + 2^-23 |resid|

u_out = the build's u for 16-bit output (2^-8 bf16, 2^-11 IEEE half), 2^-24 for fp32 output.  The middle term is the worst-case fp32
summation bound (K products + the bias, two roundings per add); 1.13 bounds |GELU'| and absorbs the (1 + u) of the final rounding.
ReLU is 1-Lipschitz and exact: no term of its own.  u_out |ref| is the rounding of a NORMAL result; a 16-bit result below the type's smallest
normal (6.1e-5 for IEEE half: the negative tail of GELU, a sum that cancels) lands on the subnormal grid, at most half its spacing away:
eta_out = 2^-25 (IEEE half) / 2^-134 (bf16) is added for 16-bit output -- the underflow term of the standard rounding model, 3e-8 at most.
g_act is the documented error of the GELU form the kernel calls (the comments above
the functions in csrc/common.h):

    "fast"  gelu_fast / gelu_erf: erf to 5e-7 absolute as evaluated in fp32   -> |z| / 2 * 5e-7
    "poly"  gelu_bf16x2, bf16 build: |y error| <= 1.0e-4 |x| (the positive tail's 1.9e-5 |x| lies inside it) -> 1.0e-4 |z| for z >= -3.8;
            the negative tail is flushed, |y| <= 6.3e-9 |x| for x < -3.8       -> |gelu(z)| + (1 + 2^-8) 6.3e-9 |z| for z < -3.8
            (the stored value is y rounded to bf16, hence the 1 + 2^-8 on |y|; x = -100 must return 6.4e-7 at most, where 1.0e-4 |x|
            would let the -9e-4 of the unflushed polynomial pass)
    "poly"  gelu_bf16x2, IEEE-half build: 1.5e-4 absolute                    -> 1.5e-4

Which form a kernel calls (read from its source) is gelu_form below."""
import collections

import numpy as np
import torch

BUILDS = {"bf16": (None, torch.bfloat16, 2.0 ** -8), "f16": ("f16", torch.float16, 2.0 ** -11)}
ETA = {"bf16": 2.0 ** -134, "f16": 2.0 ** -25}   # half the spacing of the 16-bit type's subnormals

# svt_debug_set keys a case may touch, and their defaults: 1 tile height, 2 one-tile / persistent scheduler, 3 kernel arm (70 = gemm_pps_kernel
# wherever eligible), 6 small-problem kernel on / off, 29 gemm_p1w_kernel (1 where it measured faster, 2 everywhere, 0 never), 33 the small-problem
# kernel's 32 x 32 threshold, 34 tile walk, 37 workgroups of a persistent launch; the split-operand cases (tests/gemm_split.py) also 3 = 34 (gemm_x3p_kernel
# wherever eligible), 11 the LDS-DMA split kernels on / off (off: the register-staged split kernel), 30 gemm_p1x_kernel in place of gemm_x3q_kernel
KEY_DEFAULTS = {1: 0, 2: 0, 3: 0, 6: 1, 11: 1, 29: 1, 30: 0, 33: 96, 34: -1, 37: 256}

# kid: the id svt_debug_set(39, 0) must report (1000 * family + tile rows; include/svt_mi355.h).  conv = (T_in, T_out, stride, cin): implicit-conv
# rows over a channels-last (B, T_in, cin) tensor, B = M / T_out, K = taps * cin.  keys: {debug key: value} in force for the launch.
Case = collections.namedtuple("Case", "kid M N K conv act out_f32 resid bias keys")


def C(kid, M, N, K, conv=None, act=0, out_f32=0, resid=False, bias=True, **keys):
    return Case(kid, M, N, K, conv, act, out_f32, resid, bias, tuple(sorted((int(k[1:]), v) for k, v in keys.items())))


def case_id(c):
    s = f"k{c.kid}-{c.M}x{c.N}x{c.K}"
    if c.conv:
        s += "-conv"
    s += ("", "-gelu", "-relu")[c.act] + ("-f32" if c.out_f32 else "") + ("-resid" if c.resid else "") + ("" if c.bias else "-nobias")
    return s + "".join(f"-key{k}={v}" for k, v in c.keys)


CONV = (122, 60, 2, 64)   # kernel 3 over 64 channels, stride 2: 60 overlapping rows per clip, row stride 2 x 64, clip stride 122 x 64

# ---- gemm_skinny_kernel (every activation through gelu_fast).  K = 64: one slab, three of the four waves idle; 320: five slabs, uneven quarters
SKINNY = [
    C(1032, 70, 48, 64), C(1032, 70, 48, 128), C(1032, 70, 48, 320),
    C(1032, 249, 48, 6144, act=1, out_f32=1, resid=True),            # the grouped positional-conv call
    C(1064, 249, 3072, 768, act=1), C(1064, 193, 2048, 192, act=2),
    C(1064, 130, 512, 3072, out_f32=1, resid=True, k33=0),
    C(1064, 120, 128, 192, conv=CONV, k33=0),
    C(1032, 120, 128, 192, conv=CONV),
]
# ---- register-staged gemm_kernel (gelu_erf = gelu_fast).  N = 20 with 16-bit output: rows are not 16-byte aligned -> scalar stores
STAGED = [
    C(2128, 300, 256, 96), C(2128, 300, 200, 72, act=1),
    C(2256, 499, 20, 768), C(2256, 499, 48, 104, out_f32=1, resid=True),
]
# ---- gemm_pp8_kernel (16-bit output without residual: gelu_bf16x2; fp32 output or residual: gelu_erf).  N = 200: not a small-problem shape
PP8 = ([C(3000 + bm, 777, 200, 128, k1=bm) for bm in (64, 128, 192, 256)] +
       [C(3064, 777, 200, 128),                                         # the cost model's own height
        C(3256, 777, 200, 128, out_f32=1, resid=True, k1=256), C(3128, 777, 200, 128, act=2, k1=128),
        C(3192, 777, 200, 128, act=1, k1=192), C(3064, 777, 200, 128, act=1, out_f32=1, k1=64),
        C(3256, 257, 200, 128, k1=256),                                 # the last tile holds one valid row
        C(3128, 180, 200, 192, conv=CONV, k1=128),
        C(3128, 777, 200, 64, k1=128), C(3064, 777, 200, 64)])          # a single slab
# ---- gemm_pers_kernel (fp32 output: gelu_erf; 16-bit: gelu_bf16x2), forced by key 2 = 4 with the small-problem kernel off, and once chosen
PERS = ([C(4000 + bm, M, N, K, k1=bm, k2=4, k6=0, **kw) for (M, N, K) in ((300, 256, 128), (1500, 512, 256)) for bm in (64, 128, 192, 256)
         for kw in (dict(out_f32=1), dict(act=2))] +
        [C(4064, 4100, 2048, 128, out_f32=1, k1=64)])                   # 520 tiles: the dispatcher's own choice
# ---- gemm_pps_kernel (gelu_bf16x2), forced by key 3 = 70, and chosen by the dispatcher
PPS = ([C(5000 + bm, 300, 256, 128, act=act, bias=bias, k1=bm, k3=70, k6=0) for bm in (128, 192, 256) for act in (0, 1) for bias in (True, False)] +
       [C(5128, 1500, 512, 192, k1=128, k3=70, k6=0, k37=8),            # 24 tiles on 8 workgroups: three tiles each
        C(5192, 1500, 512, 192, act=1, k1=192, k3=70, k6=0, k37=8),     # 16 tiles: two each
        C(5128, 300, 256, 192, conv=CONV, k1=128, k3=70, k6=0),
        C(5128, 6400, 512, 128, act=1, k1=128),                         # 100 tiles
        C(3128, 6272, 512, 128, act=1, k1=128),                         # 98 tiles: another family
        C(5128, 6400, 512, 192, k1=128, k29=0)])
# ---- gemm_p1w_kernel (gelu_bf16x2; K >= 192 = three slabs).  The 256-row GELU form finishes its tiles out of the accumulator registers
P1W = [
    C(6128, 6400, 512, 192, k1=128), C(6128, 6400, 512, 256, k1=128), C(6128, 6400, 512, 320, k1=128),
    C(6128, 6400, 512, 1024, act=1, k1=128),                            # GELU: the dispatcher's choice from K = 1024
    C(6128, 6400, 512, 192, act=1, k1=128, k29=2),
    C(6192, 2400, 2048, 192, k1=192), C(6256, 3200, 2048, 192, k1=256),
    C(6192, 2400, 2048, 192, act=1, k1=192, k29=2), C(6256, 3200, 2048, 192, act=1, k1=256, k29=2),
    C(6128, 6400, 512, 192, k1=128, k37=8), C(6128, 6400, 512, 192, act=1, k1=128, k29=2, k37=8),   # 12 - 13 tiles per workgroup: both parities
    C(6128, 6400, 512, 192, k1=128, k34=3),                             # 50 tile rows in panels of 3
    C(6128, 6273, 512, 192, k1=128),                                    # the last tile holds one valid row
    C(6128, 6400, 512, 192, conv=(129, 64, 2, 64), k1=128),
]
CASES = SKINNY + STAGED + PP8 + PERS + PPS + P1W

# GELU alone (one-hot A): kernel id, M, K padded with zero columns to the kernel's minimum, keys.  16-bit output for every family, and fp32
# output -- where nothing but gelu_fast's own error and one fp32 rounding is left -- for the kernels that have it
GELU_ALONE = [
    C(1032, 128, 512, 64, act=1), C(2128, 128, 512, 72, act=1),
    C(3128, 128, 512, 64, act=1, k1=128, k2=2, k6=0), C(4128, 128, 512, 128, act=1, k1=128, k2=4, k6=0),
    C(5128, 128, 512, 128, act=1, k1=128, k3=70, k6=0), C(6128, 6400, 512, 192, act=1, k1=128, k29=2),
    C(1032, 128, 512, 64, act=1, out_f32=1), C(2128, 128, 512, 72, act=1, out_f32=1),
    C(3128, 128, 512, 64, act=1, out_f32=1, k1=128, k2=2, k6=0), C(4128, 128, 512, 128, act=1, out_f32=1, k1=128, k2=4, k6=0),
]


def gelu_form(c):
    """The GELU a kernel calls, from its source: gemm_skinny.hip act_apply and gemm.hip apply_act -> gelu_fast; gemm_epilogue.h (gemm_pp8_kernel)
    gelu_bf16x2 for 16-bit output without residual, apply_act otherwise; gemm_pers.hip gelu_erf for fp32 output, gelu_bf16x2 for 16-bit;
    gemm_pps.hip / gemm_p1w.hip gelu_bf16x2."""
    family = c.kid // 1000
    if family in (1, 2):
        return "fast"
    if family == 3:
        return "fast" if (c.out_f32 or c.resid) else "poly"
    if family == 4:
        return "fast" if c.out_f32 else "poly"
    return "poly"


def g_act(form, build, z):
    if form == "fast":
        return z.abs() * (0.5 * 5e-7)
    if build == "bf16":
        return torch.where(z < -3.8, gelu64(z).abs() + (1.0 + 2.0 ** -8) * 6.3e-9 * z.abs(), 1.0e-4 * z.abs())
    return torch.full_like(z, 1.5e-4)


def gelu64(z):
    return 0.5 * z * (1.0 + torch.special.erf(z * 0.5 ** 0.5))


def tile_shape(kid):
    """(rows, columns) of the output tile of a kernel id."""
    family, rows = kid // 1000 % 10, kid % 1000
    if family == 1:
        return rows, rows
    if family == 2:
        return rows, 64 if rows == 256 else 128
    return rows, 256


def make_inputs(c, dtype, seed=0):
    """Operands as run_gemm of test_gpu_gemm.py draws them -- A U(-1, 1), W U(-1, 1) / sqrt K, bias and residual N(0, 1) -- rounded to `dtype`.
    Returns dict: A (what the kernel reads: (M, K), or (B, T_in, cin) for conv rows), rows (M, K) fp64, W, bias, resid, and the row addressing."""
    g = torch.Generator().manual_seed(seed)
    M, N, K = c.M, c.N, c.K
    if c.conv:
        T_in, T_out, st, cin = c.conv
        A = (torch.rand(M // T_out, T_in, cin, generator=g) * 2 - 1).to(dtype)
        idx = (torch.arange(T_out) * st)[:, None] + torch.arange(K // cin)[None, :]
        rows = A.double()[:, idx].reshape(M, K)
        addr = (T_out, T_in * cin, st * cin)
    else:
        A = (torch.rand(M, K, generator=g) * 2 - 1).to(dtype)
        rows = A.double()
        addr = (M, 0, K)
    W = ((torch.rand(N, K, generator=g) * 2 - 1) / K ** 0.5).to(dtype)
    bias = torch.randn(N, generator=g) if c.bias else None
    resid = torch.randn(M, N, generator=g) if c.resid else None
    return dict(A=A, rows=rows, W=W, bias=bias, resid=resid, addr=addr)


def reference(c, inp, alpha=1.0):
    """(z, S, ref) in fp64; alpha (a batched launch's GemmArgs::alpha, as the float the ABI holds): z = alpha A W^T + bias, S = |alpha| |A||W|^T + |bias|."""
    W = inp["W"].double()
    z = inp["rows"] @ W.t()
    S = inp["rows"].abs() @ W.abs().t()
    if alpha != 1.0:
        z *= alpha
        S *= abs(alpha)
    if inp["bias"] is not None:
        z += inp["bias"].double()
        S += inp["bias"].double().abs()
    ref = gelu64(z) if c.act == 1 else torch.relu(z) if c.act == 2 else z.clone()
    if inp["resid"] is not None:
        ref += inp["resid"].double()
    return z, S, ref


def limit(c, build, z, S, ref, resid, alpha=1.0):
    """alpha != 1: one more rounding per element, the multiply -> 1.13 (K + 3) 2^-23 S with S scaled by |alpha| (reference above)."""
    u_out = 2.0 ** -24 if c.out_f32 else BUILDS[build][2]
    lim = u_out * ref.abs() + 1.13 * (c.K + 2 + (alpha != 1.0)) * 2.0 ** -23 * S + (0.0 if c.out_f32 else ETA[build])
    if c.act == 1:
        lim += g_act(gelu_form(c), build, z)
    if resid is not None:
        lim += 2.0 ** -23 * resid.double().abs()
    return lim


def worst(c, got, ref, lim):
    """(worst err / limit, text saying where it sits: tile, row inside the tile, column)."""
    ratio = (got.double() - ref).abs() / lim
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    m, n = np.unravel_index(int(ratio.argmax()), ratio.shape)
    tr, tc = tile_shape(c.kid)
    return ratio.max().item(), (f"tile ({m // tr}, {n // tc}) row {m % tr} column {n} (row {m} of {c.M}); "
                                f"err {abs(got[m, n].item() - ref[m, n].item()):.3e} limit {lim[m, n].item():.3e}")


_cache = collections.OrderedDict()   # test speed only: neighbouring cases (the other build, another tile height) share operands and reference


def case_data(c, build):
    """(inputs, z, S, ref) of a case in a build; the last few are kept.  Nothing in the key but what the operands depend on."""
    key = (c.M, c.N, c.K, c.conv, c.act, c.resid, c.bias, build)
    if key not in _cache:
        inp = make_inputs(c, BUILDS[build][1])
        _cache[key] = (inp,) + reference(c, inp)
        while len(_cache) > 4:
            _cache.popitem(last=False)
    _cache.move_to_end(key)
    return _cache[key]


# ---- a correct kernel, simulated on the CPU (tests/test_gemm_limit.py): fp32 accumulation in 32-wide K chunks, fp32 activation, one rounding ----
def truncate_to(x, dtype):
    """fp32 -> 16-bit by truncation (toward zero) instead of round-to-nearest-even."""
    r = x.to(dtype)
    bits = r.view(torch.int16)
    mag = (bits & 0x7FFF) - (r.float().abs() > x.abs()).to(torch.int16)
    return ((bits & -0x8000) | mag).view(dtype)


def simulate(c, inp, dtype, truncate=False, drop=None, alpha=1.0, alpha_last=False):
    """drop = (row, chunk): that row misses the 32-element K block `chunk`.  alpha_last (a mutant): alpha multiplies the sum AND the bias."""
    rows, W = inp["rows"].float(), inp["W"].float()
    acc = torch.zeros(c.M, c.N)
    for k0 in range(0, c.K, 32):
        part = rows[:, k0:k0 + 32] @ W[:, k0:k0 + 32].t()
        if drop is not None and drop[1] * 32 == k0:
            part[drop[0]] = 0.0
        acc += part
    if alpha != 1.0 and not alpha_last:
        acc *= alpha
    if inp["bias"] is not None:
        acc += inp["bias"]
    if alpha != 1.0 and alpha_last:
        acc *= alpha
    if c.act == 1:
        acc = torch.nn.functional.gelu(acc)
    elif c.act == 2:
        acc = torch.relu(acc)
    if inp["resid"] is not None:
        acc += inp["resid"]
    if c.out_f32:
        return acc
    return truncate_to(acc, dtype) if truncate else acc.to(dtype)


# =====================================================================================================================
# Batched launches (svt_debug_gemm_batched; tests/test_gpu_gemm_batched.py): everything of GemmArgs that svt_debug_gemm cannot express --
# nz > 1 with z = z1 * nz2 + z2, the z strides of A / W / C / bias, alpha, ldc != N -- in the four forms the product callers use.
#
# A batched case is one Case per z: problem z is an ordinary (M, N, K) product on operands gathered from the launch's buffers by the
# strides the kernels are given (batched_problem), held to the same fp64 reference and the same per-element limit as an unbatched case.
# alpha != 1 adds one rounding, the multiply: z = alpha A W^T + bias, S = |alpha| |A||W|^T + |bias|, summation term 1.13 (K + 3) 2^-23 S
# (reference / limit above).  The split-operand precisions use the three-term reference and the random-case limit of tests/gemm_split.py.
#
#   posconv  grouped positional conv, plain form: z1 = clip, z2 = group; overlapping implicit-conv rows (row stride cg, K = kp cg) of a
#            (B, G, T + kp, cg) operand, w_z1 = 0, a cg-wide column slice of the (B T, D = G cg) output, bias slice and residual alike
#   folded   its phase-folded form: one z per group, M = B Tq rows in clips of Tq (a_rpb = Tq with a clip stride), N = Pf cg
#   qk       scale q k^T of the score-matrix attention: A and W are slices of ONE packed (B T, 3 D) tensor, a_z2 = w_z2 = dh, fp32 scores
#            with rows padded to Tp = T rounded up to 8 (ldc = Tp > N unless T % 8 == 0)
#   pv       P V: K = Tp, P row-stochastic with zero pad columns, V^T with zero pad columns, c_z2 = dh into (B T, D) rows
Geom = collections.namedtuple("Geom", "form M N K a_rpb a_bstride a_rstride ldw ldc nz nz2 a_z1 a_z2 w_z1 w_z2 c_z1 c_z2 bias_z2 a_elems w_off w_elems "
                                      "bias_elems c_elems dims")
# precs: "16" (both 16-bit builds), or a tuple of the precision codes 0 / 2 / 3 of the bf16 library.  out16: 16-bit output in the 16-bit builds
# (every other precision stores fp32).  name: a tag for the id.
BCase = collections.namedtuple("BCase", "kid precs geom alpha act out16 resid bias keys name")


def posconv_geom(B, G, T, cg, kp):
    K, D = kp * cg, G * cg
    return Geom("posconv", T, cg, K, T, 0, cg, K, D, B * G, G, G * (T + kp) * cg, (T + kp) * cg, 0, cg * K, T * D, cg, cg,
                B * G * (T + kp) * cg, None, G * cg * K, G * cg, B * T * D, (B, G, T, cg, kp))


def folded_geom(G, B, Tq, Pf, cg, kf, nz2=None):
    """nz2 != G (the refusal case): the same addresses with z1 strides of nz2 z2 strides."""
    N, K, Tp = Pf * cg, kf * cg, (Tq - 1) * Pf + kf + 3
    nz2 = nz2 or G
    az, wz, cz = Tp * cg, N * K, B * Tq * N
    return Geom("folded", B * Tq, N, K, Tq, G * Tp * cg, Pf * cg, K, N, G, nz2, nz2 * az, az, nz2 * wz, wz, nz2 * cz, cz, N,
                B * G * Tp * cg, None, G * N * K, G * N, G * B * Tq * N, (G, B, Tq, Pf, cg, kf))


def attn_tp(T):
    return (T + 7) // 8 * 8


def qk_geom(B, H, T, dh):
    D, Tp = H * dh, attn_tp(T)
    return Geom("qk", T, T, dh, T, 0, 3 * D, 3 * D, Tp, B * H, H, T * 3 * D, dh, T * 3 * D, dh, H * T * Tp, T * Tp, 0,
                B * T * 3 * D, D, 0, 0, B * H * T * Tp, (B, H, T, dh))


def pv_geom(B, H, T, dh):
    D, Tp = H * dh, attn_tp(T)
    return Geom("pv", T, dh, Tp, T, 0, Tp, Tp, D, B * H, H, H * T * Tp, T * Tp, H * dh * Tp, dh * Tp, T * D, dh, 0,
                B * H * T * Tp, None, B * H * dh * Tp, 0, B * T * D, (B, H, T, dh))


def BC(kid, precs, geom, alpha=1.0, act=0, out16=False, resid=False, bias=True, name="", **keys):
    if geom.form in ("qk", "pv"):
        bias = False
    return BCase(kid, precs, geom, float(np.float32(alpha)), act, out16, resid, bias, tuple(sorted((int(k[1:]), v) for k, v in keys.items())), name)


def bcase_id(b):
    g = b.geom
    s = f"k{b.kid}-{g.form}-" + "x".join(str(d) for d in g.dims) + f"-nz{g.nz}" + (f"of{g.nz2}" if g.nz2 != g.nz else "")
    s += ("", "-gelu", "-relu")[b.act] + ("-o16" if b.out16 else "") + ("-resid" if b.resid else "") + ("-alpha" if b.alpha != 1.0 else "")
    s += ("-" + b.name if b.name else "") + "-p" + (b.precs if isinstance(b.precs, str) else "".join(str(p) for p in b.precs))
    return s + "".join(f"-key{k}={v}" for k, v in b.keys)


_PC, _PC320, _PC300 = posconv_geom(2, 4, 70, 48, 8), posconv_geom(2, 4, 70, 64, 5), posconv_geom(2, 4, 300, 64, 8)
_PF, _PF192 = folded_geom(4, 3, 50, 4, 64, 5), folded_geom(4, 3, 50, 3, 64, 5)
_ATT = [(2, 3, 67, 32), (2, 2, 200, 128), (1, 2, 4160, 64)]
_SCALE = {dh: dh ** -0.5 for dh in (32, 64, 128)}
_pc = dict(act=1, resid=True)   # the plain positional conv: GELU, fp32 output, residual
BATCHED = [
    # ---- plain positional-conv form.  K = 384: six slabs; K = 320: five slabs over the small-problem kernel's four waves
    BC(1032, "16", _PC, **_pc), BC(1032, "16", _PC320, **_pc), BC(2256, (0,), _PC, **_pc), BC(12256, (2, 3), _PC, **_pc),
    BC(2256, "16", _PC300, k6=0, **_pc),                             # T = 300: two 256-row tiles per z, the second with 44 valid rows
    # alpha with a bias (no product caller has both: the epilogues' order alpha * sum + bias is checked here)
    BC(1032, "16", _PC, alpha=0.3, **_pc), BC(2256, (0,), _PC, alpha=0.3, **_pc), BC(12256, (2, 3), _PC, alpha=0.3, **_pc),
    # ---- phase-folded form: M = 150 rows in clips of 50, GELU, 16-bit output in the 16-bit builds
    BC(1032, "16", _PF, act=1, out16=True), BC(3064, "16", _PF, act=1, out16=True, k6=0),
    BC(7256, (2, 3), _PF, act=1), BC(7192, (2, 3), _PF192, act=1), BC(2128, (0,), _PF, act=1),
    # nz % nz2 != 0: the batched arm of gemm_x3s_kernel refuses, the register-staged split kernel computes the same
    BC(12128, (2, 3), folded_geom(4, 3, 50, 4, 64, 5, nz2=3), act=1, name="refused"),
    # ---- scale q k^T: fp32 scores, ldc = Tp
    BC(2128, "16", qk_geom(*_ATT[0]), alpha=_SCALE[32]), BC(2128, (0,), qk_geom(*_ATT[0]), alpha=_SCALE[32]),
    BC(3064, "16", qk_geom(*_ATT[1]), alpha=_SCALE[128]), BC(3192, "16", qk_geom(*_ATT[2]), alpha=_SCALE[64]),
    # ---- P V: 16-bit output in the 16-bit builds
    BC(2256, "16", pv_geom(*_ATT[0]), out16=True), BC(2256, (0,), pv_geom(*_ATT[0])),
    BC(2128, "16", pv_geom(*_ATT[1]), out16=True), BC(2256, "16", pv_geom(*_ATT[2]), out16=True),
]


def batched_runs(b):
    """(library variant, storage dtype, precision code, tag) of every run of a case."""
    if b.precs == "16":
        return [(BUILDS[n][0], BUILDS[n][1], 1, n) for n in BUILDS]
    return [(None, torch.float32, p, f"prec{p}") for p in b.precs]


def batched_inputs(b, dtype, seed=0):
    """The launch's buffers, flat, rounded to `dtype`: A, W (None where it lives inside A: the packed q | k | v), bias, resid (fp32, C's indexing)."""
    g = b.geom
    gen = torch.Generator().manual_seed(seed)
    if g.form == "pv":
        B, H, T, dh = g.dims
        Tp = g.K
        P = torch.zeros(B * H, T, Tp)
        P[..., :T] = torch.softmax(torch.randn(B * H, T, T, generator=gen) * 2.0, -1)
        Vt = torch.zeros(B * H, dh, Tp)
        Vt[..., :T] = torch.rand(B * H, dh, T, generator=gen) * 2 - 1
        A, W = P.to(dtype).flatten(), Vt.to(dtype).flatten()
    else:
        A = (torch.rand(g.a_elems, generator=gen) * 2 - 1).to(dtype)
        W = ((torch.rand(g.w_elems, generator=gen) * 2 - 1) / g.K ** 0.5).to(dtype) if g.w_off is None else None
    bias = torch.randn(g.bias_elems, generator=gen) if b.bias else None
    resid = torch.randn(g.c_elems, generator=gen) if b.resid else None
    return dict(A=A, W=W, bias=bias, resid=resid)


def batched_offsets(g, z):
    z1, z2 = divmod(z, g.nz2)
    return z1 * g.a_z1 + z2 * g.a_z2, (g.w_off or 0) + z1 * g.w_z1 + z2 * g.w_z2, z1 * g.c_z1 + z2 * g.c_z2, z2 * g.bias_z2


def batched_index(g, z):
    """Element indices of problem z: A rows (M, K) into the A buffer, W (N, K) into the W buffer (A's where the two share one), C (M, N)."""
    ao, wo, co, _ = batched_offsets(g, z)
    m, k, n = torch.arange(g.M), torch.arange(g.K), torch.arange(g.N)
    ai = ao + ((m // g.a_rpb) * g.a_bstride + (m % g.a_rpb) * g.a_rstride)[:, None] + k[None, :]
    return ai, wo + n[:, None] * g.ldw + k[None, :], co + m[:, None] * g.ldc + n[None, :]


def batched_in_bounds(b):
    """Every address the launch may touch lies inside its buffers (checked on the CPU before anything is launched)."""
    g = b.geom
    for z in range(g.nz):
        ai, wi, ci = batched_index(g, z)
        w_elems = g.a_elems if g.w_off is not None else g.w_elems
        if not (ai.min() >= 0 and ai.max() < g.a_elems and wi.min() >= 0 and wi.max() < w_elems and ci.min() >= 0 and ci.max() < g.c_elems):
            return False
        if b.bias and batched_offsets(g, z)[3] + g.N > g.bias_elems:
            return False
    return True


def batched_problem(b, bufs, z, prec, mutant=None):
    """Problem z as (Case, inputs) for reference / limit / simulate of this file (16-bit) or of gemm_split.py (precision 0 / 2 / 3), and its C indices.
    mutant "prev_head": head z2 > 0 of the last z1 reads head z2 - 1's W rows; "no_bias_z2": every z reads the first bias slice."""
    g = b.geom
    ai, wi, ci = batched_index(g, z)
    if mutant == "prev_head" and z // g.nz2 == (g.nz - 1) // g.nz2 and z % g.nz2 > 0:
        wi = wi - g.w_z2
    Wbuf = bufs["A"] if g.w_off is not None else bufs["W"]
    bo = 0 if mutant == "no_bias_z2" else batched_offsets(g, z)[3]
    inp = dict(rows=bufs["A"][ai].double(), W=Wbuf[wi], bias=bufs["bias"][bo:bo + g.N] if b.bias else None,
               resid=bufs["resid"][ci] if b.resid else None)
    if prec == 1:
        c = C(b.kid, g.M, g.N, g.K, act=b.act, out_f32=0 if b.out16 else 1, resid=b.resid, bias=b.bias)
    else:
        import gemm_split as X
        c = X.S(b.kid, g.M, g.N, g.K, act=b.act, resid=b.resid, bias=b.bias, out_kind=None if b.kid // 1000 not in (9, 10) else 0)
    return c, inp, ci


def batched_reference(b, bufs, z, prec, build):
    """(Case, z, S, ref, limit, C indices) of problem z."""
    c, inp, ci = batched_problem(b, bufs, z, prec)
    if prec == 1:
        zz, S, ref = reference(c, inp, b.alpha)
        return c, zz, S, ref, limit(c, build, zz, S, ref, inp["resid"], b.alpha), ci
    import gemm_split as X
    zz, S, ref = X.reference(c, inp, prec, b.alpha)
    return c, zz, S, ref, X.limit(c, prec, zz, S, ref, inp["resid"], b.alpha), ci


def batched_simulate(b, bufs, z, prec, dtype, mutant=None):
    """A correct kernel on problem z (fp32 torch arithmetic, 32-wide K chunks, one rounding), or one of the mutants of batched_problem / "alpha_last"."""
    c, inp, _ = batched_problem(b, bufs, z, prec, mutant)
    if prec in (0, 1):
        if g_pad := (-b.geom.K) % 32:   # (a K tail: zero columns change nothing)
            inp = dict(inp, rows=torch.nn.functional.pad(inp["rows"], (0, g_pad)), W=torch.nn.functional.pad(inp["W"], (0, g_pad)))
            c = c._replace(K=c.K + g_pad)
        return simulate(c, inp, dtype, alpha=b.alpha, alpha_last=mutant == "alpha_last")
    import gemm_split as X
    assert b.geom.K % 32 == 0
    acc = X.simulate(inp["rows"].float(), inp["W"], None, prec)
    acc = acc * b.alpha + inp["bias"] if mutant != "alpha_last" else (acc + inp["bias"]) * b.alpha
    if b.act == 1:
        acc = torch.nn.functional.gelu(acc)
    return acc + inp["resid"] if b.resid else acc


def batched_worst(b, prec, build, bufs, got_of_z):
    """Worst err / limit over every element of every z, and where it sits: (ratio, text).  got_of_z(z, C indices) -> (M, N) result of problem z."""
    best = (-1.0, "")
    for z in range(b.geom.nz):
        c, _, _, ref, lim, ci = batched_reference(b, bufs, z, prec, build)
        got = got_of_z(z, ci)
        if prec == 1:
            r, where = worst(c, got, ref, lim)
        else:
            import gemm_split as X
            r, where = X.worst(c, got, ref, lim)
        if r > best[0]:
            best = (r, f"z1 {z // b.geom.nz2} z2 {z % b.geom.nz2} {where}")
    return best


# =====================================================================================================================
# Score-matrix attention (svt_debug_attention_scores; tests/test_gpu_attention_scores.py): scale q k^T (+ gate pb) into fp32 scores, a row
# softmax in fp32 (one wave per row, lanes striding the keys by 64), P in the storage type with zero pad columns, P V against V^T with zero
# pad columns.  All in fp64 from the inputs already rounded to the storage type:
#
#     s_ij = scale q_i.k_j (+ gate_i pb_(j - i + T - 1))     sigma_ij = the same with absolute values     m_i = max_j s_ij
#     p = softmax(s)      ref = p v      A = p |v|
#
#     delta_i = (dh + 3) 2^-24 max_j sigma_ij          fp32 accumulation of the score in any order, the scale, the bias add
#     eps_i   = 2 delta_i                              s_ij and m_i each off by delta_i
#               + 2^-24 max_j |s_ij - m_i|             the rounding of s - max
#               + (T / 64 + 16) 2^-24                  expf to 1 ulp, the lane's T / 64 adds and the wave's 6, the reciprocal and the multiply
#     |got - ref| <= eps_i A + u_P A + (Tp + 2) 2^-23 A + u_out |ref| + eta_out
#
# u_P = 0 where P is stored in fp32, else the 16-bit type's u; u_out = 2^-24 for fp32 output, else u; eta_out as ETA above.  No factor on top.
# Split-operand modes (fp32 storage, both products through the split instantiation of the register-staged kernel): the two product terms are
# the split product's own (tests/gemm_split.py): its summation term with three products per element and its distance from the fp64 product
# (mode_bound there, written out here because these operands exceed 1):
#     delta_i = max_j [ |scale| (1.13 (3 dh + 3) 2^-23 S3_ij + 3 u^2 (1 + u)^2 |q_i|.|k_j| + eta (1 + u) (sum|q_i| + sum|k_j|)) + 2^-23 sigma_ij ]
#     P V     : (1.13 (3 Tp + 2) 2^-23 (1 + 4 u) + 3 u^2 (1 + u)^2) A + eta (1 + u) (1 + sum_j |v_jd|)
# (S3 of P V <= ((1 + u)^2 + u (1 + u)) A <= (1 + 4 u) A; sum_j p_ij = 1; 2^-23 sigma: the roundings of the scale and of the bias add.)
# kid: the id svt_debug_set(39, 0) must report after the call -- the kernel of the LAST product, P V (K = Tp, N = dh)
ACase = collections.namedtuple("ACase", "kid prec B T H dh gain bias layout")


def AC(kid, prec, B, T, H, dh=64, gain=1.5, bias=False, layout="packed"):
    return ACase(kid, prec, B, T, H, dh, gain, bias, layout)


def acase_id(c):
    return (f"k{c.kid}-p{c.prec}-B{c.B}-T{c.T}-H{c.H}-dh{c.dh}-g{c.gain}" + ("-bias" if c.bias else "") + ("" if c.layout == "packed" else "-" + c.layout))


ATTN = ([AC(2256, 0, *s) for s in ((2, 1, 2, 64), (2, 7, 3, 64), (2, 67, 3, 32), (1, 249, 12, 64))] + [AC(2128, 0, 2, 130, 2, 128)] +
        [AC(2256, 0, 2, T, 2, 64) for T in (8, 9, 63, 64, 65)] +    # T % 8 = 0, 1, 7; T just past the wave's 64-key stride; Tp = T
        [AC(2256, 0, 2, 65, 2, 64, gain=8.0),                        # peaked rows
         AC(2256, 0, 2, 67, 3, 32, layout="separate")] +
        # 16-bit: P V of T = 249 (K = Tp = 256, a slab multiple) runs the small-problem kernel, the others the register-staged one
        [AC(2256, "16", 2, 67, 3, 32), AC(1032, "16", 2, 249, 3, 32), AC(2128, "16", 2, 67, 3, 96), AC(1032, "16", 2, 249, 3, 96),
         AC(2128, "16", 2, 65, 2, 128, bias=True), AC(2128, "16", 2, 200, 2, 128, bias=True),
         AC(2256, "16", 1, 4100, 2, 64, bias=True),                  # the smallest length the fused bias kernel refuses
         AC(2128, "16", 2, 67, 3, 96, layout="separate")] +
        [AC(12256, p, 2, T, 3, 64, bias=True) for p in (2, 3) for T in (65, 249)] +   # WavLM's route in the split modes
        [AC(12256, p, 2, 65, 3, 64, layout="separate") for p in (2, 3)])


def attn_runs(c):
    """(library variant, storage dtype, precision code, tag) of every run of a case."""
    if c.prec == "16":
        return [(BUILDS[n][0], BUILDS[n][1], 1, n) for n in BUILDS]
    return [(None, torch.float32, c.prec, f"prec{c.prec}")]


def attn_scale(dh):
    return float(np.float32(dh ** -0.5))   # what the C ABI's float argument holds


def attn_inputs(c, dtype):
    """x (B, T, 3 D) rounded to `dtype`, gate (B, H, T) in (0, 2) and pb (H, 2 T - 1) ~ N(0, 1) or None: as tests/test_gpu_attention.py draws them."""
    D = c.H * c.dh
    g = torch.Generator().manual_seed(c.B * 100003 + c.T * 101 + c.H)
    x = (torch.randn(c.B, c.T, 3 * D, generator=g) * c.gain).to(dtype)
    gate = pb = None
    if c.bias:
        gate = torch.rand(c.B, c.H, c.T, generator=g) * 1.98 + 0.01
        pb = torch.randn(c.H, 2 * c.T - 1, generator=g)
    return x, gate, pb


def _rel_index(T, shift=0):
    return (torch.arange(T)[None, :] - torch.arange(T)[:, None] + (T - 1 + shift)).clamp_(0, 2 * T - 2)   # [query, key]


def attn_row_terms(q, k, scale, gate, pb, prec):
    """(delta, spread) per row, (B, H, T) fp64: delta_i as above for `prec` (0 / 1: the plain form; 2 / 3: the split form), spread_i = max_j |s_ij - m_i|."""
    B, T, H, dh = q.shape
    delta, spread = torch.empty(B, H, T, dtype=torch.float64), torch.empty(B, H, T, dtype=torch.float64)
    rel = pb.double()[:, _rel_index(T)] if pb is not None else None
    for b in range(B):
        qb, kb = (x[b].double().transpose(0, 1) for x in (q, k))
        s = torch.bmm(qb, kb.transpose(1, 2)).mul_(scale)
        sig = torch.bmm(qb.abs(), kb.abs().transpose(1, 2)).mul_(abs(scale))
        if prec >= 2:
            import gemm_split as X
            _, u, _, eta = X.PIECE[prec]
            S3 = torch.stack([X.three_term(q[b, :, h].float(), k[b, :, h].float(), prec)[1] for h in range(H)])
            d = abs(scale) * (1.13 * (3 * dh + 3) * 2.0 ** -23 * S3 + 3 * u * u * (1 + u) ** 2 * sig / abs(scale) +
                              eta * (1 + u) * (qb.abs().sum(-1)[:, :, None] + kb.abs().sum(-1)[:, None, :]))
        if rel is not None:
            s.addcmul_(gate[b].double()[:, :, None], rel)
            sig.addcmul_(gate[b].double()[:, :, None], rel.abs())
        delta[b] = (d + 2.0 ** -23 * sig).amax(-1) if prec >= 2 else (dh + 3) * 2.0 ** -24 * sig.amax(-1)
        spread[b] = (s.amax(-1, keepdim=True) - s).amax(-1)
    return delta, spread


def attn_limit(c, prec, build, v, o, A, delta, spread):
    """The per-element limit, (B, T, H * dh) fp64, from the reference o, A = p |v| and the row terms."""
    B, T, H, dh = c.B, c.T, c.H, c.dh
    Tp = attn_tp(T)
    eps = 2 * delta + 2.0 ** -24 * spread + (T / 64 + 16) * 2.0 ** -24               # (B, H, T)
    eps = eps.transpose(1, 2)[..., None].expand(B, T, H, dh).reshape(B, T, H * dh)
    u16 = BUILDS[build][2] if prec == 1 else 0.0
    lim = eps * A + u16 * A + (u16 if prec == 1 else 2.0 ** -24) * o.abs() + (ETA[build] if prec == 1 else 0.0)
    if prec >= 2:
        import gemm_split as X
        _, u, _, eta = X.PIECE[prec]
        vsum = v.double().abs().sum(1, keepdim=True).expand(B, T, H, dh).reshape(B, T, H * dh)
        return lim + (1.13 * (3 * Tp + 2) * 2.0 ** -23 * (1 + 4 * u) + 3 * u * u * (1 + u) ** 2) * A + eta * (1 + u) * (1 + vsum)
    return lim + (Tp + 2) * 2.0 ** -23 * A


def attn_reference(q, k, v, scale, gate=None, pb=None):
    """(o, A) in fp64, (B, T, H * dh): the same computation as reference() of tests/test_gpu_attention.py, for the CPU test (which must not import a
    module that needs the GPU library); tests/test_gpu_attention_scores.py uses that one and checks this one against it."""
    B, T, H, dh = q.shape
    o, A = torch.empty(B, T, H * dh, dtype=torch.float64), torch.empty(B, T, H * dh, dtype=torch.float64)
    rel = pb.double()[:, _rel_index(T)] if pb is not None else None
    for b in range(B):
        qb, kb, vb = (x[b].double().transpose(0, 1) for x in (q, k, v))
        s = torch.bmm(qb, kb.transpose(1, 2)).mul_(scale)
        if rel is not None:
            s.addcmul_(gate[b].double()[:, :, None], rel)
        both = torch.bmm(torch.softmax(s, -1), torch.cat([vb, vb.abs()], -1))
        o[b] = both[..., :dh].transpose(0, 1).reshape(T, H * dh)
        A[b] = both[..., dh:].transpose(0, 1).reshape(T, H * dh)
    return o, A


def _chunked(a, bt, prec):
    """a (T, K) @ bt (N, K)^T in fp32, 32-wide K chunks (K padded with zero columns); split precisions: three piece products per chunk."""
    pad = (-a.shape[1]) % 32
    a, bt = torch.nn.functional.pad(a.float(), (0, pad)), torch.nn.functional.pad(bt.float(), (0, pad))
    if prec >= 2:
        import gemm_split as X
        return X.simulate(a, bt, None, prec)
    acc = torch.zeros(a.shape[0], bt.shape[0])
    for k0 in range(0, a.shape[1], 32):
        acc += a[:, k0:k0 + 32] @ bt[:, k0:k0 + 32].t()
    return acc


def attn_simulate(c, prec, dtype, q, k, v, gate, pb, mutant=None):
    """A correct pipeline in fp32 torch arithmetic: chunked scores, the scale, the bias add, an fp32 softmax, P rounded to the storage type, a chunked
    P V over Tp keys, one rounding of the output.  Mutants: "pad_ones" (P's pad columns hold 1 while V^T's pad columns hold the last key's V),
    "rel_off_by_one" (key - q + T in place of key - q + T - 1), "gate_next" (the gate of [b, h, q + 1])."""
    B, T, H, dh = q.shape
    Tp, scale = attn_tp(T), torch.tensor(attn_scale(dh))
    out = torch.empty(B, T, H * dh)
    rel = pb[:, _rel_index(T, 1 if mutant == "rel_off_by_one" else 0)] if pb is not None else None
    for b in range(B):
        for h in range(H):
            s = _chunked(q[b, :, h], k[b, :, h], prec) * scale
            if rel is not None:
                gt = gate[b, h]
                if mutant == "gate_next":
                    gt = torch.cat([gt[1:], gt[-1:]])
                s = s + gt[:, None] * rel[h]
            e = torch.exp(s - s.amax(-1, keepdim=True))
            p = (e * (1.0 / e.sum(-1, keepdim=True))).to(dtype)
            P = torch.full((T, Tp), 1.0 if mutant == "pad_ones" else 0.0, dtype=dtype)
            P[:, :T] = p
            Vt = torch.zeros(dh, Tp, dtype=dtype)
            Vt[:, :T] = v[b, :, h].t()
            if mutant == "pad_ones":
                Vt[:, T:] = v[b, T - 1, h][:, None]
            out[b, :, h * dh:(h + 1) * dh] = _chunked(P, Vt, prec)
    return out.to(dtype)
