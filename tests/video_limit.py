"""What tests/test_gpu_video_kernels.py (GPU) and tests/test_video_limit.py (CPU) share for the kernels of the AV-HuBERT lip front-end
(csrc/video.hip: the stems, the max-pools, zero_halo_kernel, avgpool_interior_kernel; csrc/conv3x3_c64.hip: the two frame-resident direct
convolutions; the generalised 2-D addressing of the GEMM launches in csrc/api_video.hip): the case tables, the operands as svt_video_finalize
makes them, the fp64 references, the limits, a simulated correct kernel and the mutants the limits must catch.

OPERANDS.  Every operand is what the kernel reads, bit for bit: sc = float32(float64(gamma) / sqrt(float64(var) + 1e-5)), shift =
float32(float64(beta) - float64(mean) * sc) (batch_norm_fold of csrc/host.cpp), folded weight = float32(w) * sc in fp32 (one rounding), then
.to(the build's 16-bit type) (fp32 mode: kept); inputs N(0, 1) rounded to the storage type; parameters from
weights.seeded_video_frontend_state_dict, whose BatchNorm statistics are away from the identity.

REFERENCE.  torch conv2d / conv3d in fp64 on those operands (a haloed tensor is the already-padded input):
    z = conv(x, w) + bias        S = conv(|x|, |w|) + |bias|        ref = prelu(z + resid)
(the residual is added BEFORE the activation: resid_first = 1 of the products, and the direct kernels do the same).

THE CONVOLUTION LIMIT, derived (u = 2^-24; no number in it is fitted):
    1  a kernel that adds the K products and the bias in fp32 in ANY order computes a with |a - z| <= (K + 1) 2 u S: K + 1 additions, each
       result (and, where the matrix pipe rounds them, each product) within u of exact -- tests/gemm_limit.py's summation bound;
    2  the residual add is one more rounding of |z + resid| <= S + |resid|, PReLU's multiply one more of a value <= L (S + |resid|) with
       L = max(1, |slope_c|), PReLU's Lipschitz constant, which also carries the error of 1 to the result:
       |y - ref| <= L ((K + 3) 2^-23 S + 2^-23 |resid|);
    3  the store rounds once to the output type: u_out |ref| (u_out = 2^-8 bf16, 2^-11 IEEE half, 2^-24 fp32) + eta_out, half the spacing
       of the 16-bit type's subnormals (tests/gemm_limit.py ETA).
    |got - ref| <= u_out |ref| + eta_out + L ((K + 3) 2^-23 S + 2^-23 |resid|)
K is the number of accumulated products AS LAUNCHED: 320 for the 16-bit stem (245 taps padded to ten 32-deep k-steps; the pad weights are
zero), 280 for the fp32 stem (35 rows of 8), 9 Cin for a 3x3 and Cin for a 1x1 trunk convolution, 3 (G + 2) 64 for the grouped form, 576 for
the downsample columns of the combined conv1 + downsample product.

THE OTHER LIMITS.  Max-pool: exact -- bit for bit fp64 max_pool2d with -inf padding of the same stored values (channel 5 of every pool input
is all-negative, x - 4: zero padding would show).  Fused stem + pool: at a pooled element the maximum of the stem limits over its window
(max is 1-Lipschitz in the sup norm).  Average pool: u_out |ref| + eta_out + (H W + 1) 2^-24 mean|x| (H W - 1 fp32 additions and the division,
each within u of a value <= sum|x|).  Zero-halo: exact -- every halo byte 0, every interior byte the poison it held.

THE HALO INVARIANT, asserted in every block and pool case: the test zeroes the halos and fills the interiors of the buffers to be written
with NaN; afterwards every halo element of every written buffer is +0 bit for bit and every interior element is finite and inside its limit
(a stored garbage column, a shifted store and a grouped product that does not put the halo back all break it)."""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as Fn

import gemm_limit as G
from svt_speechbrain_amd import weights as W

BUILDS = dict(G.BUILDS)                      # "bf16" / "f16": (library variant, torch type, u_out)
BUILDS["fp32"] = (None, torch.float32, 2.0 ** -24)
ETA = dict(G.ETA)
ETA["fp32"] = 0.0
PRECISION = {"bf16": "bf16", "f16": "fp16", "fp32": "fp32"}   # the modules' precision name of a build
U23 = 2.0 ** -23
KVC = (64, 128, 256, 512)
EMBED, WEIGHT_SEED = 64, 4986

# kernel ids (include/svt_mi355.h, svt_debug_set key 43)
K_STEM_F32, K_STEM_16, K_STEM_POOL = 100, 101, 300
K_POOL_F32, K_POOL_X8 = 200, 202
K_HALO = 400
K_AVG_F32, K_AVG_16 = 600, 601
VK_NONE, VK_C64, VK_C128, VK_G2, VK_G4, VK_PLAIN, VK_COMB = 0, 1, 2, 3, 4, 5, 6


def block_kid(k1, kd, k2):
    return 5000 + 100 * k1 + 10 * kd + k2


# ---------------------------------------------------------------------------------------------------------------------------------
# the eligibility predicates of csrc/conv3x3_c64.hip and csrc/video.hip, restated: THEY MUST TRACK THE SOURCE (c3_lds_bytes, conv3x3_c64_ok,
# c128_ring_slots, c128_lds_bytes, conv3x3_c128_ok, stem_pool_lds, conv3d_front_pool_ok)
LDS_BUDGET = 160 * 1024
C3_SLACK = 56


def c3_lds_bytes(Hs, Ws):
    FP = (Hs + 2) * (Ws + 2)
    return 2 * ((FP + 7) // 8 * 8 + C3_SLACK) * 128 + 512


def conv3x3_c64_ok(Hs, Ws):
    return Hs >= 1 and Ws >= 1 and Hs * (Ws + 2) >= 12 * 16 and c3_lds_bytes(Hs, Ws) <= LDS_BUDGET


def c128_ring_slots(Hs, Ws):
    Wp = Ws + 2
    FP, MB = (Hs + 2) * Wp, (Hs * Wp + 15) // 16
    need = (MB + 2) // 3 * 48 + 2 * Wp + 2
    return (max(FP, need) + 7) // 8 * 8


def c128_lds_bytes(Hs, Ws):
    return 2 * c128_ring_slots(Hs, Ws) * 256 + 4 * 2 * 6 * 1024 + 1024


def conv3x3_c128_ok(Hs, Ws):
    return Hs >= 1 and Ws >= 1 and Hs * (Ws + 2) >= 48 and c128_lds_bytes(Hs, Ws) <= LDS_BUDGET


def stem_geom(h, w):
    """(Hp0, Wp0, H0, W0, H1, W1) of video_geom (csrc/api_video.hip)."""
    H0, W0 = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return h + 6, (w + 8 + 7) // 8 * 8, H0, W0, (H0 - 1) // 2 + 1, (W0 - 1) // 2 + 1


def conv3d_front_pool_ok(h, w):
    Hp, Wp, _, W0, _, _ = stem_geom(h, w)
    return W0 <= 64 and 6 * ((Hp * Wp * 2 + 1023) // 1024 * 1024) + 9 * W0 * 128 + 512 <= LDS_BUDGET


def direct_geometries(ok, bound=700):
    """Every (Hs, Ws) a direct convolution's predicate accepts (two padded frames of more than 700 pixels a side fit no budget near this one)."""
    return [(Hs, Ws) for Hs in range(1, bound) for Ws in range(1, bound) if ok(Hs, Ws)]


def row_formula_failures(Hs, Ws):
    """Positions p < Hs (Ws + 2) at which the kernels' row index, (int)((p + 0.5f) * (1.0f / Wp)) in float32, is not p // Wp."""
    Wp = Ws + 2
    p = np.arange(Hs * Wp, dtype=np.int64)
    r = np.float32(1.0) / np.float32(Wp)
    y = ((p.astype(np.float32) + np.float32(0.5)) * r).astype(np.int32)
    return p[y != p // Wp]


# ---------------------------------------------------------------------------------------------------------------------------------
# case tables
StemCase = collections.namedtuple("StemCase", "h w T B")
PoolCase = collections.namedtuple("PoolCase", "H0 W0 F")
FusedCase = collections.namedtuple("FusedCase", "h w B T wg")
HaloCase = collections.namedtuple("HaloCase", "Hp Wp C F")
AvgCase = collections.namedtuple("AvgCase", "H W F")
# li, b: the block; H, W: interior of the block INPUT; wg: the hook's workgroups; keys: ((debug key, value), ...) in force for the launch;
# kid: the key-43 id in a 16-bit build (fp32 cases: the id of the fp32 handle); fp32: a case of the fp32 handle alone
BlockCase = collections.namedtuple("BlockCase", "name li b H W F wg keys kid fp32")

# 16 pixels = one block with all four neighbour planes zero (T = 1); 30 pixels: masked tail block; non-square; 144 pixels = 9 blocks for 8
# waves and interior frames with five real planes
STEM = [StemCase(8, 8, 1, 2), StemCase(9, 11, 2, 2), StemCase(18, 12, 3, 2), StemCase(31, 17, 6, 2)]
# odd and even edges, clipped and whole last windows
POOL = [PoolCase(4, 4, 2), PoolCase(5, 6, 2), PoolCase(9, 8, 2), PoolCase(16, 9, 2)]
# h -> H0 = 4 (below one band), 8, 9 (last band of one row), 17; every h, every w, non-square pairs
FUSED_HW = [(8, 8), (16, 18), (17, 31), (33, 18), (16, 31), (33, 8)]
# one frame; the launcher's grid; runs of 8 and 7 frames on two workgroups, each crossing two clip boundaries (the plane-slot ring wraps,
# both band buffers are reused)
FUSED = [FusedCase(h, w, B, T, wg) for (h, w) in FUSED_HW for (B, T, wg) in ((1, 1, 0), (2, 3, 0), (3, 5, 2))]
FUSED_REFUSED = (8, 136)   # W0 = 68 > 64
HALO = [HaloCase(Hp, Wp, C, F) for (Hp, Wp, C) in ((3, 3, 64), (4, 9, 128), (24, 24, 64), (3, 4, 512)) for F in (1, 3)]
AVG = [AvgCase(H, Wd, F) for (H, Wd) in ((1, 1), (1, 2), (3, 3)) for F in (1, 5)]


def _blocks():
    out = []

    def add(name, li, b, H, Wd, F, wg=0, keys=(), kid=None, fp32=False):
        out.append(BlockCase(name, li, b, H, Wd, F, wg, tuple(keys), kid, fp32))

    c64 = block_kid(VK_C64, 0, VK_C64)
    # direct c64: NV = 192 = exactly one triple per position group; five triples, partial last one; the 88-pixel ROI, the largest frame that
    # fits; Wp = 96, the widest-row end of the row formula.  F = 3 on one workgroup: both LDS buffers reused; F = 5 on two: uneven runs
    for (H, Wd) in ((12, 14), (13, 13), (22, 22), (2, 94)):
        for (F, wg) in ((1, 0), (3, 1), (5, 2)):
            add(f"c64-{H}x{Wd}-F{F}-wg{wg}", 0, 0, H, Wd, F, wg, kid=c64)
    add("c64-13x13-F3-wg1-b1", 0, 1, 13, 13, 3, 1, kid=c64)
    # grouped and plain stage 1
    add("g2-8x8-F4", 0, 0, 8, 8, 4, kid=block_kid(VK_G2, 0, VK_G2))
    add("g4-7x7-F10", 0, 0, 7, 7, 10, kid=block_kid(VK_G4, 0, VK_G4))       # one pixel past the row end, re-zero
    add("g4-5x11-F10", 0, 1, 5, 11, 10, kid=block_kid(VK_G4, 0, VK_G4))
    add("plain-7x7-F1", 0, 0, 7, 7, 1, kid=block_kid(VK_PLAIN, 0, VK_PLAIN))
    add("plain-13x13-F2-key23", 0, 0, 13, 13, 2, keys=((23, 0),), kid=block_kid(VK_PLAIN, 0, VK_PLAIN))
    # stage 2, block 0 (stride 2): the combined 256-column product then direct c128; two products; conv2 on the GEMM path
    add("s2b0-13x13-F3", 1, 0, 13, 13, 3, kid=block_kid(VK_COMB, VK_COMB, VK_C128))
    add("s2b0-13x13-F3-key27", 1, 0, 13, 13, 3, keys=((27, 0),), kid=block_kid(VK_PLAIN, VK_PLAIN, VK_C128))
    add("s2b0-8x9-F3", 1, 0, 8, 9, 3, kid=block_kid(VK_COMB, VK_COMB, VK_PLAIN))
    # direct c128: one triple; two, the second partial; three; Wp = 59, the widest row the predicate admits -- at Hs = 1, a padded frame
    # of 3 x 59.  (Hs, Ws) = (3, 57) itself is NOT eligible (296 ring slots need 201 728 B of LDS): the forward runs it on the products, so
    # does the hook, and the case stays as one of the plain path.
    c128 = block_kid(VK_C128, 0, VK_C128)
    for (H, Wd) in ((4, 10), (7, 7), (11, 11), (1, 57)):
        for (F, wg) in ((1, 0), (3, 1), (5, 2)):
            add(f"c128-{H}x{Wd}-F{F}-wg{wg}", 1, 1, H, Wd, F, wg, kid=c128)
    for (F, wg) in ((1, 0), (3, 1), (5, 2)):
        add(f"c128-3x57-F{F}-wg{wg}", 1, 1, 3, 57, F, wg, kid=block_kid(VK_PLAIN, 0, VK_PLAIN))
    # stages 3 and 4: the product path only
    for (li, H, Wd) in ((2, 4, 5), (3, 2, 3)):
        add(f"s{li + 1}b0-{H}x{Wd}-F3", li, 0, H, Wd, 3, kid=block_kid(VK_PLAIN, VK_PLAIN, VK_PLAIN))
        Ho, Wo = (H - 1) // 2 + 1, (Wd - 1) // 2 + 1
        add(f"s{li + 1}b1-{Ho}x{Wo}-F3", li, 1, Ho, Wo, 3, kid=block_kid(VK_PLAIN, 0, VK_PLAIN))
    # fp32 handle: one case per stage and block
    for (li, H, Wd) in ((0, 7, 7), (1, 13, 13), (2, 4, 5), (3, 2, 3)):
        add(f"f32-s{li + 1}b0-{H}x{Wd}-F2", li, 0, H, Wd, 2, kid=block_kid(VK_PLAIN, VK_PLAIN if li else 0, VK_PLAIN), fp32=True)
        Ho, Wo = ((H - 1) // 2 + 1, (Wd - 1) // 2 + 1) if li else (H, Wd)
        add(f"f32-s{li + 1}b1-{Ho}x{Wo}-F2", li, 1, Ho, Wo, 2, kid=block_kid(VK_PLAIN, 0, VK_PLAIN), fp32=True)
    return out


BLOCKS = _blocks()
BLOCK_BY_NAME = {c.name: c for c in BLOCKS}


def block_dims(c):
    """(stride, Cin, C, Ho, Wo) of a block case."""
    stride = 2 if (c.b == 0 and c.li > 0) else 1
    C = KVC[c.li]
    cin = KVC[c.li - 1] if stride == 2 else C
    return stride, cin, C, (c.H - 1) // stride + 1, (c.W - 1) // stride + 1


def group_width(build, F, Hs, Ws):
    """video_group_width of csrc/api_video.hip: the grouped form a stage-1 block takes where the direct kernel does not apply."""
    if build == "fp32":
        return 0
    grp = 2 if Ws % 2 == 0 else (4 if (Ws + 3) // 4 * 4 - Ws <= 2 else 0)
    if grp and F * Hs * ((Ws + grp - 1) // grp) < 128:
        grp = 0
    return grp


def block_K(c, build):
    """(K of conv1, K of the downsample, K of conv2) as launched, from the case's kernel id."""
    kid = c.kid
    k1, kd, k2 = (kid - 5000) // 100, (kid // 10) % 10, kid % 10
    _, cin, C, _, _ = block_dims(c)

    def K(code, ci, one_by_one=False):
        if code in (VK_G2, VK_G4):
            return 3 * ((2 if code == VK_G2 else 4) + 2) * 64
        if code == VK_COMB:
            return 9 * ci
        return ci if one_by_one else 9 * ci
    return K(k1, cin), K(kd, cin, True), K(k2, C)


# ---------------------------------------------------------------------------------------------------------------------------------
# operands as svt_video_finalize uploads them
def _bn(sd, pre):
    g, b, m, v = (sd[f"{pre}.{k}"].to(torch.float32) for k in ("weight", "bias", "running_mean", "running_var"))
    sc = g.double() / torch.sqrt(v.double() + 1e-5)
    return sc.to(torch.float32), (b.double() - m.double() * sc).to(torch.float32)


def _fold(w, sc, dtype):
    return (w.to(torch.float32) * sc.view(-1, *([1] * (w.dim() - 1)))).to(dtype)


Conv = collections.namedtuple("Conv", "w bias slope")   # w: (Cout, Cin, k, k) folded, storage type; bias fp32; slope fp32 or None


@functools.lru_cache(maxsize=None)
def state_dict():
    return W.seeded_video_frontend_state_dict(EMBED, seed=WEIGHT_SEED)


@functools.lru_cache(maxsize=None)
def operands(build):
    """{"stem": Conv, (li, b, "conv1" | "conv2" | "down"): Conv}: what the handle of this build multiplies with."""
    dtype = BUILDS[build][1]
    sd = state_dict()
    ops = {}
    sc, sh = _bn(sd, "resnet.frontend3D.1")
    ops["stem"] = Conv(_fold(sd["resnet.frontend3D.0.weight"], sc, dtype), sh, sd["resnet.frontend3D.2.weight"].to(torch.float32))
    for li in range(4):
        for b in range(2):
            pre = f"resnet.trunk.layer{li + 1}.{b}"
            for n in (1, 2):
                sc, sh = _bn(sd, f"{pre}.bn{n}")
                ops[(li, b, f"conv{n}")] = Conv(_fold(sd[f"{pre}.conv{n}.weight"], sc, dtype), sh, sd[f"{pre}.relu{n}.weight"].to(torch.float32))
            if b == 0 and li > 0:
                sc, sh = _bn(sd, f"{pre}.downsample.1")
                ops[(li, b, "down")] = Conv(_fold(sd[f"{pre}.downsample.0.weight"], sc, dtype), sh, None)
    return ops


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs (the GPU test and the CPU proof draw the same ones)
def _seed(*key):
    return sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31)


def haloed(interior, dtype=None):
    """[F][H][W][C] -> zero-haloed [F][H + 2][W + 2][C]."""
    return Fn.pad(interior, (0, 0, 1, 1, 1, 1)).to(dtype or interior.dtype)


def interior(t):
    return t[:, 1:-1, 1:-1, :]


def video_input(c, build):
    """fp32 video (B, 1, T, h, w) whose values the build's storage type holds exactly (the pad kernel's rounding is then the identity)."""
    g = torch.Generator().manual_seed(_seed(1, c.h, c.w, c.T, c.B))
    return torch.randn(c.B, 1, c.T, c.h, c.w, generator=g).to(BUILDS[build][1]).to(torch.float32)


def pool_input(c, build):
    g = torch.Generator().manual_seed(_seed(2, c.H0, c.W0, c.F))
    x = torch.randn(c.F, c.H0, c.W0, 64, generator=g)
    x[..., 5] -= 4.0     # an all-negative channel: padding with 0 instead of -inf shows
    x[..., 5].clamp_(max=-0.25)
    return x.to(BUILDS[build][1])


def block_input(c, build):
    _, cin, _, _, _ = block_dims(c)
    g = torch.Generator().manual_seed(_seed(3, c.li, c.b, c.H, c.W, c.F))
    return haloed(torch.randn(c.F, c.H, c.W, cin, generator=g).to(BUILDS[build][1]))


def avg_input(c, build):
    g = torch.Generator().manual_seed(_seed(4, c.H, c.W, c.F))
    return haloed(torch.randn(c.F, c.H, c.W, 512, generator=g).to(BUILDS[build][1]))


def poisoned(F, H, Wd, C, dtype):
    """A zero-haloed output buffer whose interior is NaN."""
    t = torch.zeros(F, H + 2, Wd + 2, C, dtype=dtype)
    t[:, 1:-1, 1:-1, :] = float("nan")
    return t


# ---------------------------------------------------------------------------------------------------------------------------------
# references and limits
def _prelu(a, slope):
    return a if slope is None else torch.where(a > 0, a, a * slope.double())


def conv_limit(build, K, ref, S, slope, resid=None):
    u, eta = BUILDS[build][2], ETA[build]
    L = 1.0 if slope is None else slope.double().abs().clamp(min=1.0)
    r = 0.0 if resid is None else resid.abs()
    return u * ref.abs() + eta + L * ((K + 3) * U23 * S + U23 * r)


def conv_reference(build, xh, cv, K, stride=1, resid_h=None):
    """One trunk convolution over the zero-haloed channels-last xh [F][H + 2][W + 2][Cin] (stored values): (ref, limit), both fp64
    [F][Ho][Wo][Cout].  A 1x1 convolution reads the interior; resid_h is the haloed residual at the output size."""
    k = cv.w.shape[-1]
    x = xh.double().permute(0, 3, 1, 2)
    if k == 1:
        x = x[:, :, 1:-1, 1:-1]
    w = cv.w.double()
    z = Fn.conv2d(x, w, stride=stride) + cv.bias.double().view(1, -1, 1, 1)
    S = Fn.conv2d(x.abs(), w.abs(), stride=stride) + cv.bias.double().abs().view(1, -1, 1, 1)
    z, S = z.permute(0, 2, 3, 1), S.permute(0, 2, 3, 1)
    resid = None if resid_h is None else interior(resid_h).double()
    ref = _prelu(z if resid is None else z + resid, cv.slope)
    return ref, conv_limit(build, K, ref, S, cv.slope, resid)


def stem_reference(build, video, fp32_kernel=None):
    """The stem over the fp32 video (B, 1, T, h, w): (ref, limit) fp64 [B T][H0][W0][64]."""
    cv = operands(build)["stem"]
    K = 280 if build == "fp32" else 320
    x, w = video.double(), cv.w.double()
    z = Fn.conv3d(x, w, stride=(1, 2, 2), padding=(2, 3, 3)) + cv.bias.double().view(1, -1, 1, 1, 1)
    S = Fn.conv3d(x.abs(), w.abs(), stride=(1, 2, 2), padding=(2, 3, 3)) + cv.bias.double().abs().view(1, -1, 1, 1, 1)
    # (B, 64, T, H0, W0) -> [B T][H0][W0][64]
    z, S = (t.permute(0, 2, 3, 4, 1).reshape(-1, t.shape[3], t.shape[4], 64) for t in (z, S))
    ref = _prelu(z, cv.slope)
    return ref, conv_limit(build, K, ref, S, cv.slope)


def maxpool_reference(x):
    """3x3 / 2 max-pool, -inf padding, of the stored values [F][H0][W0][C]: fp64 [F][H1][W1][C] (exact: a maximum rounds nothing)."""
    return Fn.max_pool2d(x.double().permute(0, 3, 1, 2), 3, stride=2, padding=1).permute(0, 2, 3, 1)


def fused_reference(build, video):
    """Stem + pool: (ref, limit); the limit of a pooled element is the maximum of the stem limits over its window."""
    ref, lim = stem_reference(build, video)
    return maxpool_reference(ref), maxpool_reference(lim)


def avg_reference(build, xh):
    x = interior(xh).double()
    n = x.shape[1] * x.shape[2]
    ref = x.mean(dim=(1, 2))
    return ref, BUILDS[build][2] * ref.abs() + ETA[build] + (n + 1) * 2.0 ** -24 * x.abs().mean(dim=(1, 2))


# ---------------------------------------------------------------------------------------------------------------------------------
# checks: every function returns (worst err / limit, where) and raises AssertionError with the place of the first violation
def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def worst(got, ref, lim):
    """max over elements of |got - ref| / limit and its (frame, y, x, channel) / (frame, channel); non-finite got counts as infinite."""
    err = (got.double() - ref).abs()
    ratio = torch.where(torch.isfinite(got.double()), err / lim, torch.full_like(err, float("inf")))
    i = int(ratio.argmax())
    return float(ratio.flatten()[i]), tuple(int(v) for v in np.unravel_index(i, tuple(ratio.shape)))


def check_haloed(got_h, ref, lim, what):
    """The halo invariant and the limit for one written buffer: halo +0 bit for bit, interior finite and inside the limit."""
    halo = _bits(got_h).clone()
    halo[:, 1:-1, 1:-1, :] = 0
    bad = halo.nonzero()
    assert bad.numel() == 0, f"{what}: halo element (frame, y, x, channel) = {tuple(bad[0].tolist())} is not +0"
    r, at = worst(interior(got_h), ref, lim)
    assert r <= 1.0, f"{what}: err / limit = {r:.3g} at (frame, y, x, channel) = {at}"
    return r, at


def check_plain(got, ref, lim, what):
    r, at = worst(got, ref, lim)
    assert r <= 1.0, f"{what}: err / limit = {r:.3g} at {at}"
    return r, at


def check_exact_haloed(got_h, ref, what):
    """Max-pool: halo +0, interior equal to the fp64 reference bit for bit (every value is a stored value)."""
    halo = _bits(got_h).clone()
    halo[:, 1:-1, 1:-1, :] = 0
    bad = halo.nonzero()
    assert bad.numel() == 0, f"{what}: halo element {tuple(bad[0].tolist())} is not +0"
    g = interior(got_h)
    same = _bits(g) == _bits(ref.to(g.dtype))
    assert bool(same.all()), f"{what}: differs at (frame, y, x, channel) = {tuple((~same).nonzero()[0].tolist())}"
    return 0.0, (0, 0, 0, 0)


def check_zero_halo(got, poison_bits, what):
    """Zero-halo: every halo element 0, every interior element still the poison."""
    b = _bits(got)
    inner = b[:, 1:-1, 1:-1, :]
    assert bool((inner == poison_bits).all()), f"{what}: an interior element was written"
    halo = b.clone()
    halo[:, 1:-1, 1:-1, :] = 0
    assert not bool(halo.any()), f"{what}: halo element {tuple(halo.nonzero()[0].tolist())} is not 0"


def check_block(c, build, xh, t1, ds, out):
    """Every convolution of a block against a reference computed from the 16-bit values THAT convolution read: conv1 and the downsample
    from the block input, conv2 from the t1 (and the downsample) it was given.  Returns {"conv1" | "down" | "conv2": (ratio, where)}."""
    ops = operands(build)
    stride, _, _, _, _ = block_dims(c)
    K1, Kd, K2 = block_K(c, build)
    res = {}
    ref, lim = conv_reference(build, xh, ops[(c.li, c.b, "conv1")], K1, stride)
    res["conv1"] = check_haloed(t1, ref, lim, f"{c.name} conv1")
    resid = xh
    if stride == 2:
        ref, lim = conv_reference(build, xh, ops[(c.li, c.b, "down")], Kd, 2)
        res["down"] = check_haloed(ds, ref, lim, f"{c.name} downsample")
        resid = ds
    # t1 passed its own check: finite, zero halo -- it is a valid padded input
    ref, lim = conv_reference(build, t1, ops[(c.li, c.b, "conv2")], K2, 1, resid)
    res["conv2"] = check_haloed(out, ref, lim, f"{c.name} conv2")
    return res


# ---------------------------------------------------------------------------------------------------------------------------------
# a simulated correct kernel (fp32 torch arithmetic, K in chunks of 32, one rounding to the output type) and the mutants
MUTANTS = ("trunc_store", "drop_tap", "no_resid", "resid_after", "slope_neighbour", "swap_channels", "frag_perm", "garbage_col", "shift_out",
           "group_no_rezero", "time_pad_clip", "stem_x_off", "pool_pad0", "pool_no_first_row", "avg_over_halo", "comb_down_tap")


def _round_store(a, dtype, truncate=False):
    r = a.to(dtype)
    if truncate and dtype != torch.float32:
        over = r.to(torch.float32).abs() > a.abs()        # rounded away from zero: step the magnitude back by one ulp
        bits = r.view(torch.int16)
        r = torch.where(over, bits - 1, bits).view(dtype)
    return r


def _chunked(A, Wm):
    """A (M, K) x Wm (N, K)^T accumulated in fp32, 32 columns of K at a time."""
    acc = torch.zeros(A.shape[0], Wm.shape[0], dtype=torch.float32)
    for k0 in range(0, A.shape[1], 32):
        acc += A[:, k0:k0 + 32] @ Wm[:, k0:k0 + 32].t()
    return acc


def frag_perm():
    """Output channel whose weights channel c receives when the fragment image's two index fields are exchanged -- block-of-four major,
    (nb & 1) * 16 + (i >> 2) * 4, in place of (i >> 2) * 8 + (nb & 1) * 4 (fold_conv_frag64)."""
    perm = [0] * 64
    for nb in range(4):
        for i in range(16):
            good = (nb >> 1) * 32 + (i >> 2) * 8 + (nb & 1) * 4 + (i & 3)
            perm[good] = (nb >> 1) * 32 + (nb & 1) * 16 + (i >> 2) * 4 + (i & 3)
    return perm


def sim_conv(build, xh, cv, stride=1, resid_h=None, mutant=None, out_poison=True, tap=None):
    """One trunk convolution as a correct kernel computes it -> the zero-haloed output buffer (interior written, halo left +0).
    tap: read this tap of the 3x3 window in place of the centre (a 1x1 convolution; mutant comb_down_tap)."""
    dtype = BUILDS[build][1]
    k = cv.w.shape[-1]
    F, Hp, Wp, Cin = xh.shape
    H, Wd = Hp - 2, Wp - 2
    Ho, Wo = (H - 1) // stride + 1, (Wd - 1) // stride + 1
    x = xh.to(torch.float32).permute(0, 3, 1, 2)
    w = cv.w.to(torch.float32)
    if mutant == "frag_perm":
        w = w[frag_perm()]
    if k == 1:
        ty, tx = (1, 1) if tap is None else tap
        x = x[:, :, ty:ty + H, tx:tx + Wd]
    A = Fn.unfold(x, k, stride=stride).permute(0, 2, 1).reshape(F * Ho * Wo, Cin * k * k)      # columns (ci, ky, kx)
    if mutant == "drop_tap":
        A = A.clone()
        A[(F * Ho * Wo) // 2].view(Cin, k * k)[:, 4] = 0.0
    a = _chunked(A, w.reshape(w.shape[0], -1)) + cv.bias
    a = a.view(F, Ho, Wo, -1)
    slope = cv.slope
    if slope is not None and mutant == "slope_neighbour":
        slope = slope.roll(-1)
    act = (lambda t: t) if slope is None else (lambda t: torch.where(t > 0, t, t * slope))
    if resid_h is not None and mutant != "no_resid":
        r = interior(resid_h).to(torch.float32)
        a = act(a) + r if mutant == "resid_after" else act(a + r)
    else:
        a = act(a)
    o = _round_store(a, dtype, truncate=mutant == "trunc_store")
    if mutant == "swap_channels":
        o = o.clone()
        o[..., [2, 3]] = o[..., [3, 2]]
    out = poisoned(F, Ho, Wo, o.shape[-1], dtype) if out_poison else torch.zeros(F, Ho + 2, Wo + 2, o.shape[-1], dtype=dtype)
    if mutant == "shift_out":
        # stored at padded pixel p + Wp + 2: the interior moves one pixel right, its last column lands on the halo
        out[:, 1:-1, 2:, :] = o
    else:
        out[:, 1:-1, 1:-1, :] = o
    if mutant in ("garbage_col", "group_no_rezero"):
        # flat position x = Ws of every row is stored too: its 3x3 window starts at padded column Ws and wraps into the next row
        xf = xh.to(torch.float32).reshape(F, Hp * Wp, Cin)
        xf = torch.cat([xf, torch.zeros(F, 2 * Wp + 4, Cin)], 1)
        for y in range(Ho):
            p = y * Wp + Wd
            win = torch.stack([xf[:, p + ky * Wp + kx, :] for ky in range(3) for kx in range(3)], -1)      # (F, Cin, 9)
            g = act(win.reshape(F, -1) @ w.reshape(w.shape[0], -1).t() + cv.bias)
            out[:, y + 1, Wd + 1, :] = g.to(dtype)
    return out


def sim_block(c, build, xh, mutant=None):
    """A block as the forward runs it: (t1, ds or None, out), every buffer zero-haloed with its interior written."""
    ops = operands(build)
    stride, _, _, _, _ = block_dims(c)
    m1 = mutant if mutant in ("drop_tap", "frag_perm", "garbage_col", "shift_out", "swap_channels", "trunc_store") else None
    t1 = sim_conv(build, xh, ops[(c.li, c.b, "conv1")], stride, mutant=m1)
    ds, resid = None, xh
    if stride == 2:
        ds = sim_conv(build, xh, ops[(c.li, c.b, "down")], 2, tap=(0, 0) if mutant == "comb_down_tap" else None)
        resid = ds
    t1_read = t1
    if m1 in ("garbage_col", "shift_out"):       # conv2 of the simulation reads a clean t1: the mutant is conv1's store alone
        t1_read = sim_conv(build, xh, ops[(c.li, c.b, "conv1")], stride)
    m2 = mutant if mutant in ("no_resid", "resid_after", "slope_neighbour", "group_no_rezero") else None
    out = sim_conv(build, t1_read, ops[(c.li, c.b, "conv2")], 1, resid, mutant=m2)
    return t1, ds, out


def sim_stem(build, video, mutant=None):
    """The stem as a correct kernel computes it -> [B T][H0][W0][64] of the storage type."""
    cv = operands(build)["stem"]
    dtype = BUILDS[build][1]
    B, _, T, h, w = video.shape
    v = video.to(torch.float32)[:, 0]                                          # (B, T, h, w)
    left = 4 if mutant == "stem_x_off" else 3                                  # the alignment pad element taken for a tap
    vp = Fn.pad(v, (left, 6 - left, 3, 3))
    if mutant == "time_pad_clip":
        # the planes in front of and behind a clip are its neighbours' frames where it has neighbours (zero only at the batch's ends)
        flat = Fn.pad(vp.reshape(B * T, *vp.shape[2:]), (0, 0, 0, 0, 2, 2))
        vp = torch.stack([flat[b * T:b * T + T + 4] for b in range(B)])
    else:
        vp = Fn.pad(vp, (0, 0, 0, 0, 2, 2))
    win = vp.unfold(1, 5, 1).unfold(2, 7, 2).unfold(3, 7, 2)                   # (B, T, H0, W0, 5, 7, 7)
    H0, W0 = win.shape[2], win.shape[3]
    A = win.reshape(B * T * H0 * W0, 245)
    a = _chunked(A, cv.w.to(torch.float32).reshape(64, 245)) + cv.bias
    a = torch.where(a > 0, a, a * cv.slope)
    return _round_store(a, dtype).view(B * T, H0, W0, 64)


def sim_pool(x, mutant=None):
    """3x3 / 2 max-pool of [F][H0][W0][C] -> zero-haloed [F][H1 + 2][W1 + 2][C]."""
    xs = x.to(torch.float32).permute(0, 3, 1, 2)
    pad = 0.0 if mutant == "pool_pad0" else float("-inf")
    xp = Fn.pad(xs, (1, 1, 1, 1), value=pad)
    if mutant == "pool_no_first_row":
        xp = xp.clone()
        win = xp.unfold(2, 3, 2).unfold(3, 3, 2)[..., 1:, :]
    else:
        win = xp.unfold(2, 3, 2).unfold(3, 3, 2)
    o = win.amax(dim=(-1, -2)).permute(0, 2, 3, 1).to(x.dtype)
    out = poisoned(o.shape[0], o.shape[1], o.shape[2], o.shape[3], x.dtype)
    out[:, 1:-1, 1:-1, :] = o
    return out


def sim_avg(build, xh, mutant=None):
    x = (xh if mutant == "avg_over_halo" else interior(xh)).to(torch.float32)
    s = torch.zeros(x.shape[0], x.shape[3], dtype=torch.float32)
    for y in range(x.shape[1]):
        for xx in range(x.shape[2]):
            s = s + x[:, y, xx, :]
    return (s / float(x.shape[1] * x.shape[2])).to(BUILDS[build][1])
