"""What tests/test_gpu_gemm_kernels.py (GPU) and tests/test_gemm_limit.py (CPU) share: the case tables of the 16-bit GEMM kernels, the
fp64 reference of a case and the per-element limit a correct kernel stays inside.

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


def reference(c, inp):
    """(z, S, ref) in fp64."""
    W = inp["W"].double()
    z = inp["rows"] @ W.t()
    S = inp["rows"].abs() @ W.abs().t()
    if inp["bias"] is not None:
        z += inp["bias"].double()
        S += inp["bias"].double().abs()
    ref = gelu64(z) if c.act == 1 else torch.relu(z) if c.act == 2 else z.clone()
    if inp["resid"] is not None:
        ref += inp["resid"].double()
    return z, S, ref


def limit(c, build, z, S, ref, resid):
    u_out = 2.0 ** -24 if c.out_f32 else BUILDS[build][2]
    lim = u_out * ref.abs() + 1.13 * (c.K + 2) * 2.0 ** -23 * S + (0.0 if c.out_f32 else ETA[build])
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


def simulate(c, inp, dtype, truncate=False, drop=None):
    """drop = (row, chunk): that row misses the 32-element K block `chunk`."""
    rows, W = inp["rows"].float(), inp["W"].float()
    acc = torch.zeros(c.M, c.N)
    for k0 in range(0, c.K, 32):
        part = rows[:, k0:k0 + 32] @ W[:, k0:k0 + 32].t()
        if drop is not None and drop[1] * 32 == k0:
            part[drop[0]] = 0.0
        acc += part
    if inp["bias"] is not None:
        acc += inp["bias"]
    if c.act == 1:
        acc = torch.nn.functional.gelu(acc)
    elif c.act == 2:
        acc = torch.relu(acc)
    if inp["resid"] is not None:
        acc += inp["resid"]
    if c.out_f32:
        return acc
    return truncate_to(acc, dtype) if truncate else acc.to(dtype)
