"""What tests/test_gpu_conv0.py (GPU) and tests/test_conv0_limit.py (CPU) share for the kernels of the waveform front end (csrc/stats.hip:
moments_kernel, conv0_window_moments_kernel, conv0_group_coef_kernel; csrc/conv0.hip: conv0_group_apply_kernel, conv0_layer_kernel;
csrc/conv0_mfma.hip: conv0_mfma_kernel with its table and exponent kernels): the case tables, the inputs, the references and the limits.
Every limit is a bound derived from the number formats and the operation count (u = 2^-24 fp32, u64 = 2^-53 fp64, h = the unit roundoff of a
16-bit piece: 2^-9 bf16, 2^-12 IEEE half, eta = half the spacing of its subnormals); none is fitted to what a kernel returns.

ORDERED SUMS (forms 0, 1).  Exact inputs are multiples of 2^-6 in [-1, 1]: every fp32 four-term partial and every fp32 product is exact, so
are the fp64 sums in any order, and the result must equal integer arithmetic bit for bit.  Random audio:
    form 0   |ds| <= (2^-22 + n u64) sum|x|,  |dss| <= (2^-22 + n u64) sum x^2      three fp32 roundings per four-sum (contracted or not), then
                                                                                  fp64 additions in any order
    form 1   |d| <= T1 u64 sum|term|     terms = the samples and the fp32-ROUNDED tap products, which the host forms identically
A lost workgroup's share is at least 1 / workgroups of the sum: far outside.

COEFFICIENTS (form 2).  The kernel folds the waveform norm, the conv and the GroupNorm statistics into 11 coefficients per (clip, channel)
from 65 window moments: var = e2 - mean^2 with e2 a quadratic form of the moments -- heavy cancellation.  The reference takes ANOTHER route
in numpy.longdouble: the normalised waveform, y[c, t] = w_c . window_t + b for every frame, a two-pass mean and variance, then a, shift
and the coefficients.  The waveform lies on a 2^-11 grid, so every tap product is exact in fp32 and the moments the hook is fed (exact
sums of the fp32-rounded products) are the exact moments of the data the reference uses: only this kernel's arithmetic is under test.
    A      = sum_{j <= j2} f |w_j w_j2| r^2 (|m_jj2| / T + |mu| (|m_j| + |m_j2|) / T + mu^2) + 2 |b| D + b^2 + (D + |b|)^2,
             D = sum_j |w_j| r (|m_j| / T + |mu|)            the magnitude of what is added and subtracted to form var (f = 1 / 2)
    rho_a  = 75 u64 A / (2 (var + eps)) + 4 u64             each of the 55 terms carries at most 10 roundings and passes through at most 55
                                                            additions; e2, mean^2 and the subtraction add 7 more (75 in all, rounded up);
                                                            x^-1/2 halves the relative error; the sqrt, the division and gamma: 4 u64
    lim_j  = (u + rho_a + 4 u64) |coef_j|                   j < 10: the final rounding to fp32 and a r w_j
    lim_10 = u |coef_10| + (rho_a + 16 u64) |a| (|b| + r |mu| sum|w| + D + |b|) + 2 u64 |beta|
A / (var + eps) is the cancellation factor, computed per (clip, channel) from the data in extended precision.

VECTOR KERNELS.  Form 3: ref = gelu64(z), z = sum_j coef_j x_j + coef_10 in fp64 from the fp32 coefficients given, S = sum|coef_j x_j| +
|coef_10|;   lim32 = 1.13 * 12 * 2^-23 S + g_act(form, build, z)   (tests/gemm_limit.py: K + 2 = 12 for ten products and the bias; 1.13 bounds
|GELU'|; g_act the documented error of the GELU the source calls: gelu_bf16x2_x4 ("poly") for 16-bit rows, gelu_fast2 / gelu_erf ("fast")
for fp32 rows and pair rows).  Form 4: mu, r and the normalised samples xn = (x - mu) * r are reproduced bit for bit in fp32 (one
subtraction and one multiplication: nothing to contract); y = conv(xn) in fp64; the limit is tests/layernorm_limit.py's two-pass fp32
bound over the C channels with ONE more term: the computed row is y + delta, |delta| <= e_y = 12 * 2^-23 S_y, so d moves by at most
e_c = e_y + mean(e_y), which joins e_d (ln_limit below); then 1.13 lim_y + g_act.
The store: fp32 rows  |got - ref| <= lim32 + u |ref|;  16-bit rows  rn16(ref - lim32) <= got <= rn16(ref + lim32);  pair rows read back
as hi + lo  |got - ref| <= lim32 + cut_term (tests/gemm_split.py).

MATRIX-PIPE KERNELS (forms 5, 6).  Same references.  Both operands are cut into (hi, lo) pieces AFTER the kernel's power-of-two scalings,
which the host repeats (strip_scales: per wave strip of 64 frames 2^kx from max|x| of the strip, per clip 2^ka from max|coef|, the clamp of
kx + ka to [-14, 15]); with xs, cs the scaled operands, xs = xh + xl + rx, |xl| <= h (1 + h) |xs|, |rx| <= h^2 |xs| + eta, likewise cs, and
    xs cs - (xh ch + xl ch + xh cl) = xs rc + rx cs - rx rc + xl cl         (the dropped lo x lo product and the rounding of each lo piece)
    |.| <= 3.1 h^2 |xs| |cs| + 1.01 eta (|xs| + |cs|)      per tap;  the bias column: (h^2 |b| + eta) 2^tot
    taps = (sum over the ten taps + the bias term) / 2^tot                  in units of the output
    e_z  = taps + 34 * 2^-23 * 1.01 S                                       the fp32 accumulation of 32 products (K + 2 = 34)
Form 5: lim32 = 1.13 e_z + g_act; form 6: e_y = e_z enters ln_limit over the 512 accumulators, then 1.13 lim_y + g_act.  PK = 0 stores 16-bit
rows behind the polynomial GELU, PK = 2 / 3 pair rows behind gelu_fast2.

WHAT THE LIMITS CANNOT SEE.  A lo piece TRUNCATED instead of rounded moves a piece by at most 2 h^2 |x| where rounding leaves h^2 |x|: the same
order as the residual the limit must allow, and below the accumulation term (34 * 2^-23 S ~ 4e-6 S against 4 h^2 = 1.5e-5 / 2.4e-7 per
tap in the worst alignment).  No output of these kernels keeps enough bits to show it reliably: tests/test_conv0_limit.py counts the runs in
which it stays inside every check (most of them) and says so, as tests/test_gemm_limit.py does for a single lost term at K = 768."""
import collections

import numpy as np
import torch

import gemm_limit as G
import gemm_split as GS
import layernorm_limit as L

U = 2.0 ** -24
U64 = 2.0 ** -53
K0, NWM, GUARD = 10, 65, 8
EPS = float(np.float32(1e-5))                       # the float both norms are given, as the kernels widen it
H = {2: 2.0 ** -9, 3: 2.0 ** -12}                    # unit roundoff of a piece type
ETA_P = {2: 2.0 ** -134, 3: 2.0 ** -25}
PIECE_OF_BUILD = L.PIECE_PREC

# kernel ids (include/svt_mi355.h, svt_debug_set key 41)
K_MOM, K_WIN, K_COEF = 100, 200, 300
OUT_ID = {"f32": 0, "16": 1, "pk2": 20, "pk3": 30}
ALL_IDS = (100, 200, 300, 400, 401, 420, 430, 500, 501, 520, 530, 601, 620, 630, 701, 720, 730)


def kid_of(form, out):
    return {3: 400, 4: 500, 5: 600, 6: 700}[form] + OUT_ID[out]


# ---------------------------------------------------------------------------------------------------------------------------------
# case tables
MCase = collections.namedtuple("MCase", "n groups groups_max kind idx")                       # form 0
WCase = collections.namedtuple("WCase", "T1 stride slack B kind idx")                         # form 1
CCase = collections.namedtuple("CCase", "C cpg T1 stride wav_mom b0 kind B idx")              # form 2
ACase = collections.namedtuple("ACase", "form T1 C stride slack out cpg wav_mom b0 B idx")    # forms 3 .. 6
STRIDES = (5, 3, 1)

MOMENTS = []
for _kind in ("exact", "random"):
    # n % 4 != 0 with one group; 4 * 256 * 300 + 2: 301 workgroups, the final sum's second trip; both grid formulas (groups < 64, >= 64)
    for _n, _g, _gm in ((3, 1, 1), (4099, 1, 1), (4 * 256 * 300 + 2, 1, 2), (4096, 1, 1), (4096, 3, 5), (4096, 64, 64), (4096, 70, 70)):
        MOMENTS.append(MCase(_n, _g, _gm, _kind, len(MOMENTS)))

WINDOWS = []
for _kind in ("exact", "random"):
    # one thread's eight windows: 1, 7, 8, 9; one workgroup: 2048, two: 2049; nine workgroups: one eight-wide trip of the ordered add + the tail
    for _i, _t in enumerate((1, 7, 8, 9, 2048, 2049, 8 * 2048 + 1)):
        _st = 1 if _t > 4096 else STRIDES[_i % 3]
        WINDOWS.append(WCase(_t, _st, (0, _st - 1)[_i % 2], 3, _kind, len(WINDOWS)))

COEFS = []
for _i, (_C, _cpg) in enumerate(((8, 4), (8, 1), (70, 2), (70, 4), (512, 2), (512, 1), (512, 4))):
    # (C = 70: a part-filled second 64-thread workgroup; this kernel, alone of the seven, has no multiple-of-8 rule)
    for _kind in ("lowpass", "white"):
        COEFS.append(CCase(_C, _cpg, (57, 40, 33)[_i % 3], STRIDES[_i % 3], _i % 4 != 2, _i % 3 != 2, _kind, 4, len(COEFS)))

APPLY = []


def _acase(form, T1, C, stride, slack, out, cpg=1, wav_mom=True, b0=True, B=3):
    APPLY.append(ACase(form, T1, C, stride, slack, out, cpg, wav_mom, b0, B, len(APPLY)))


def _build_apply():
    """T1 x output form for each launcher; C, stride, slack, B, cpg, the moments and the bias walk their values along both axes."""
    for form, frames in ((3, (1, 31, 32, 33, 128, 129, 161)), (4, (1, 2, 15, 16, 17, 64, 65, 81))):
        for ti, T1 in enumerate(frames):
            for oi, out in enumerate(("f32", "16", "pk2", "pk3")):
                k = ti + oi
                C = (32, 512)[k % 2] if out.startswith("pk") else (8, 32, 264, 512)[k % 4]
                st = STRIDES[k % 3]
                B = 3 + ti % 2
                cpg = (B, 1, 2 if B == 4 else 1)[k % 3]
                _acase(form, T1, C, st, (0, st - 1)[k % 2], out, cpg, wav_mom=k % 5 != 4, b0=k % 4 != 3, B=B)
    for form in (5, 6):
        for ti, T1 in enumerate((1, 3, 4, 5, 16, 17, 63, 64, 65, 256, 257, 323)):
            for oi, out in enumerate(("16", "pk2", "pk3")):
                k = ti + oi
                st = 1 if T1 > 200 and k % 2 else STRIDES[k % 3]
                _acase(form, T1, 512, st, (0, st - 1)[k % 2], out, (4, 1)[k % 2], wav_mom=k % 5 != 4, b0=k % 4 != 3, B=4)


_build_apply()
MFMA_GAINS = (2.0 ** -10, 3e-4, 1.0, 2.0 ** 17)
VEC_GAINS = (1.0, 0.05, 0.5, 2.0)


def case_id(c):
    if isinstance(c, MCase):
        return f"f0-{c.idx:02d}-n{c.n}-g{c.groups}of{c.groups_max}-{c.kind}"
    if isinstance(c, WCase):
        return f"f1-{c.idx:02d}-T{c.T1}-s{c.stride}+{c.slack}-{c.kind}"
    if isinstance(c, CCase):
        return f"f2-{c.idx:02d}-C{c.C}-cpg{c.cpg}-T{c.T1}-s{c.stride}-{c.kind}" + ("" if c.wav_mom else "-nomom") + ("" if c.b0 else "-nobias")
    return (f"f{c.form}-{c.idx:03d}-k{kid_of(c.form, c.out)}-T{c.T1}-C{c.C}-s{c.stride}+{c.slack}-B{c.B}-cpg{c.cpg}" + ("" if c.wav_mom else "-nomom") +
            ("" if c.b0 else "-nobias"))


def length(c):
    return (c.T1 - 1) * c.stride + K0 + getattr(c, "slack", 0)


def builds(c):
    """fp32 rows and pair rows are served by the bf16 library (the split modes live there); 16-bit rows run in both builds, and the
    IEEE-half pair rows of the matrix-pipe kernels also in the f16 build (PK = 0 and PK = 3 use the same pieces there)."""
    if c.out == "16" or (c.form >= 5 and c.out == "pk3"):
        return tuple(G.BUILDS)
    return ("bf16",)


def gelu_form(c):
    """From the sources: conv0_group_apply_kernel / conv0_layer_kernel call gelu_bf16x2_x4 where sizeof(TO) == 2 and gelu_fast2 / gelu_erf
    otherwise (pair rows have TO = float); c0_store8 calls gelu_bf16x2_x4 for PK = 0 and gelu_fast2 for PK = 2 / 3."""
    return "poly" if c.out == "16" else "fast"


def piece_prec(c, build):
    """The piece type of a matrix-pipe case (and of any pair-row output) as a gemm_split precision."""
    return {"pk2": 2, "pk3": 3}.get(c.out) or PIECE_OF_BUILD[build]


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
def _gen(c, salt):
    return torch.Generator().manual_seed(7919 * salt + 31 * c.idx + 1)


def exact_samples(shape, g):
    return torch.randint(-64, 65, shape, generator=g)


def moments_inputs(c):
    """x (groups, n) fp32; (ref (groups, 2) fp64, lim (groups, 2) or None for the exact kind: bit equality)."""
    g = _gen(c, 1)
    if c.kind == "exact":
        k = exact_samples((c.groups, c.n), g)
        x = k.float() / 64.0
        ref = torch.stack([k.sum(1).double() / 64.0, (k * k).sum(1).double() / 4096.0], 1)
        return x, ref, None
    x = (0.1 * torch.randn(c.groups, c.n, generator=g) * (1.0 + torch.arange(c.groups)[:, None])).clamp_(-1, 1)
    xl = x.numpy().astype(np.longdouble)
    ref = torch.tensor(np.stack([xl.sum(1), (xl * xl).sum(1)], 1).astype(np.float64))
    mag = torch.tensor(np.stack([np.abs(xl).sum(1), (xl * xl).sum(1)], 1).astype(np.float64))
    return x, ref, (2.0 ** -22 + c.n * U64) * mag


def window_terms(wav, stride, T1):
    """(B, T1, 65) fp32: the ten samples of every window and the 55 products j <= j2, rounded to fp32 as the kernel forms them."""
    win = wav[:, :(T1 - 1) * stride + K0].unfold(-1, K0, stride)
    cols = [win[..., j] for j in range(K0)]
    for j in range(K0):
        for j2 in range(j, K0):
            cols.append(win[..., j] * win[..., j2])
    return torch.stack(cols, -1)


def window_inputs(c):
    """wav (B, L) fp32; ref (B, 65) fp64; lim or None (exact kind)."""
    g = _gen(c, 2)
    Lw = length(c)
    if c.kind == "exact":
        k = exact_samples((c.B, Lw), g)
        wav = k.float() / 64.0
        kw = k[:, :(c.T1 - 1) * c.stride + K0].unfold(-1, K0, c.stride)
        cols = [kw[..., j].sum(1).double() / 64.0 for j in range(K0)]
        for j in range(K0):
            for j2 in range(j, K0):
                cols.append((kw[..., j] * kw[..., j2]).sum(1).double() / 4096.0)
        return wav, torch.stack(cols, 1), None
    wav = (0.1 * torch.randn(c.B, Lw, generator=g) * torch.tensor([1.0, 0.01, 3.0])[:c.B, None]).clamp_(-1, 1)
    t = window_terms(wav, c.stride, c.T1).numpy().astype(np.longdouble)
    ref = torch.tensor(t.sum(1).astype(np.float64))
    return wav, ref, c.T1 * U64 * torch.tensor(np.abs(t).sum(1).astype(np.float64))


def check_sums(got, ref, lim):
    """(failures, worst err / limit or 0.0 for the exact kind)."""
    if torch.isnan(got).any():
        return [f"{int(torch.isnan(got).sum())} NaN (unwritten) values"], float("inf")
    if lim is None:
        bad = got.contiguous().view(torch.int64) != ref.contiguous().view(torch.int64)
        return ([f"{int(bad.sum())} of {bad.numel()} sums differ from integer arithmetic, first at {int(bad.flatten().float().argmax())}"] if bad.any() else []), 0.0
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / lim)
    w = float(ratio.max())
    return ([f"err / limit {w:.3g} at {int(ratio.flatten().argmax())}"] if not w <= 1.0 else []), w


def simulate_sums(c, x, order=0, mutant=None):
    """A correct kernel of form 0 (c an MCase, x (groups, n)) / form 1 (a WCase, x = wav): fp32 four-sums or fp32 products, fp64 sums in two
    orders.  mutant "partial lost": the first workgroup's share never arrives."""
    flip = (lambda t: t.flip(-1)) if order else (lambda t: t)
    if isinstance(c, MCase):
        n4 = c.n // 4 * 4
        drop = min(1024, c.n) if mutant else 0
        v = x[:, drop:n4].reshape(c.groups, -1, 4) if drop < n4 else x[:, :0].reshape(c.groups, 0, 4)
        a = (v[..., 0] + v[..., 1]) + (v[..., 2] + v[..., 3])
        b = (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + (v[..., 2] * v[..., 2] + v[..., 3] * v[..., 3])
        tail = x[:, max(n4, drop):].double()
        s = flip(torch.cat([a.double(), tail], 1)).cumsum(1)[:, -1] if a.shape[1] + tail.shape[1] else torch.zeros(c.groups, dtype=torch.float64)
        ss = flip(torch.cat([b.double(), tail * tail], 1)).cumsum(1)[:, -1] if a.shape[1] + tail.shape[1] else torch.zeros(c.groups, dtype=torch.float64)
        return torch.stack([s, ss], 1)
    t = window_terms(x, c.stride, c.T1).double()
    if mutant:
        t = t[:, min(2048, c.T1):]
    if t.shape[1] == 0:
        return torch.zeros(c.B, NWM, dtype=torch.float64)
    return flip(t.transpose(1, 2)).cumsum(-1)[..., -1]


# ---------------------------------------------------------------------------------------------------------------------------------
def group_moments(wav, cpg):
    """(B / cpg, 2) fp64: sum and sum of squares of each norm group of cpg clips, from extended precision."""
    xl = wav.reshape(wav.shape[0] // cpg, -1).numpy().astype(np.longdouble)
    return torch.tensor(np.stack([xl.sum(1), (xl * xl).sum(1)], 1).astype(np.float64))


def wave_norm32(mom, n_wav, cpg, B):
    """(mu, r) per clip as fp32 tensors (B, 1), computed as the kernels do: fp64 from the group's moments, rounded once."""
    if mom is None:
        return torch.zeros(B, 1), torch.ones(B, 1)
    m = mom[:, 0] / float(n_wav)
    var = mom[:, 1] / float(n_wav) - m * m
    r = 1.0 / torch.sqrt(var + EPS)
    idx = torch.arange(B) // cpg
    return m.float()[idx, None], r.float()[idx, None]


def coef_inputs(c):
    """Form 2: everything the hook is given, on the CPU."""
    g = _gen(c, 3)
    Lw = length(c)
    noise = torch.randn(c.B, Lw + 64, generator=g)
    if c.kind == "lowpass":
        cs = torch.cat([torch.zeros(c.B, 1), noise.cumsum(1)], 1)
        base = (cs[:, 33:33 + Lw] - cs[:, 1:1 + Lw]) / 32.0 * 1.5        # a 32-sample moving average: neighbouring taps nearly equal
    else:
        base = 0.2 * noise[:, :Lw]
    base = base * torch.tensor(VEC_GAINS)[:c.B, None] * 0.4
    base[2] = 0.0                                                         # digital silence: var clamps to 0
    k = (base.clamp(-1, 1) * 2048.0).round().to(torch.int64)              # the 2^-11 grid: every tap product exact in fp32
    wav = k.float() / 2048.0
    kw = k[:, :(c.T1 - 1) * c.stride + K0].unfold(-1, K0, c.stride)
    cols = [kw[..., j].sum(1).double() / 2048.0 for j in range(K0)]
    for j in range(K0):
        for j2 in range(j, K0):
            cols.append((kw[..., j] * kw[..., j2]).sum(1).double() / 2.0 ** 22)
    inp = dict(wav=wav, wm=torch.stack(cols, 1), n_wav=c.cpg * Lw)
    kg = k.reshape(c.B // c.cpg, -1)
    inp["wav_mom"] = torch.stack([kg.sum(1).double() / 2048.0, (kg * kg).sum(1).double() / 2.0 ** 22], 1) if c.wav_mom else None
    inp["w0"] = 0.5 * torch.randn(c.C, K0, generator=g)
    inp["b0"] = 0.2 * torch.randn(c.C, generator=g) if c.b0 else None
    inp["gamma"] = 1.0 + 0.3 * torch.randn(c.C, generator=g)
    inp["beta"] = 0.2 * torch.randn(c.C, generator=g)
    return inp


def coef_reference(c, inp):
    """(ref, lim) (B, C, 11) fp64, by the other route (module docstring)."""
    LD = np.longdouble
    B, C, T = c.B, c.C, c.T1
    x = inp["wav"].numpy().astype(LD)
    if inp["wav_mom"] is not None:
        mom = inp["wav_mom"].numpy().astype(LD)[np.arange(B) // c.cpg]
        mu = mom[:, 0] / LD(inp["n_wav"])
        r = 1 / np.sqrt(mom[:, 1] / LD(inp["n_wav"]) - mu * mu + LD(EPS))
    else:
        mu, r = np.zeros(B, LD), np.ones(B, LD)
    xn = (x - mu[:, None]) * r[:, None]
    idx = np.arange(T)[:, None] * c.stride + np.arange(K0)[None, :]
    win = xn[:, idx]                                                      # (B, T, 10)
    w = inp["w0"].numpy().astype(LD)
    b = inp["b0"].numpy().astype(LD) if inp["b0"] is not None else np.zeros(C, LD)
    gam, bet = inp["gamma"].numpy().astype(LD), inp["beta"].numpy().astype(LD)
    y = np.einsum("btj,cj->bct", win, w) + b[None, :, None]
    mean = y.mean(2)
    var = ((y - mean[..., None]) ** 2).mean(2)
    a = gam[None] / np.sqrt(var + LD(EPS))
    shift = bet[None] - mean * a
    ref = np.empty((B, C, K0 + 1), LD)
    ref[..., :K0] = a[..., None] * r[:, None, None] * w[None]
    ref[..., K0] = a * (b[None] - (r * mu)[:, None] * w.sum(1)[None]) + shift
    # the magnitude A of what the kernel adds and subtracts to form var
    m = inp["wm"].numpy().astype(LD)
    aw, amu = np.abs(w), np.abs(mu)[:, None]
    mj = np.abs(m[:, :K0]) / T
    D = np.einsum("cj,bj->bc", aw, r[:, None] * (mj + amu))
    A = np.zeros((B, C), LD)
    i = K0
    for j in range(K0):
        for j2 in range(j, K0):
            R = (r * r)[:, None] * (np.abs(m[:, i:i + 1]) / T + amu * (mj[:, j:j + 1] + mj[:, j2:j2 + 1]) + amu * amu)
            A += (1 if j == j2 else 2) * (aw[:, j] * aw[:, j2])[None] * R
            i += 1
    ab = np.abs(b)[None]
    A += 2 * ab * D + ab * ab + (D + ab) ** 2
    rho = 75 * U64 * A / (2 * (var + LD(EPS))) + 4 * U64
    lim = np.empty_like(ref)
    lim[..., :K0] = (U + rho[..., None] + 4 * U64) * np.abs(ref[..., :K0])
    lim[..., K0] = U * np.abs(ref[..., K0]) + (rho + 16 * U64) * np.abs(a) * (ab + (r * np.abs(mu))[:, None] * aw.sum(1)[None] + D + ab) + 2 * U64 * np.abs(bet)[None]
    return torch.tensor(ref.astype(np.float64)), torch.tensor(lim.astype(np.float64)), torch.tensor((A / (var + LD(EPS))).astype(np.float64))


COEF_MUTANTS = ("b % cpg for b / cpg", "factor 2 on the off-diagonal moments missing", "eps of the GroupNorm omitted")


def simulate_coef(c, inp, order=0, mutant=None):
    """conv0_group_coef_kernel in torch fp64, the 55 terms in ascending (0) or descending (1) order."""
    B, C, T = c.B, c.C, float(c.T1)
    m = inp["wm"]
    if inp["wav_mom"] is not None:
        gi = torch.arange(B) // c.cpg
        if mutant == COEF_MUTANTS[0]:
            gi = (torch.arange(B) % c.cpg).clamp(max=B // c.cpg - 1)
        mom = inp["wav_mom"][gi]
        mu = mom[:, 0] / float(inp["n_wav"])
        r = 1.0 / torch.sqrt(mom[:, 1] / float(inp["n_wav"]) - mu * mu + EPS)
    else:
        mu, r = torch.zeros(B, dtype=torch.float64), torch.ones(B, dtype=torch.float64)
    w = inp["w0"].double()
    bias = inp["b0"].double()[None] if inp["b0"] is not None else torch.zeros(1, C, dtype=torch.float64)
    invT = 1.0 / T
    mn = r[:, None] * (m[:, :K0] * invT - mu[:, None])
    dot = torch.zeros(B, C, dtype=torch.float64)
    for j in (range(K0 - 1, -1, -1) if order else range(K0)):
        dot = dot + w[None, :, j] * mn[:, j:j + 1]
    terms = []
    i = K0
    for j in range(K0):
        for j2 in range(j, K0):
            R = (r * r) * (m[:, i] * invT - mu * m[:, j] * invT - mu * m[:, j2] * invT + mu * mu)
            f = 1.0 if (j == j2 or mutant == COEF_MUTANTS[1]) else 2.0
            terms.append(f * (w[:, j] * w[:, j2])[None] * R[:, None])
            i += 1
    quad = torch.zeros(B, C, dtype=torch.float64)
    for t in (reversed(terms) if order else terms):
        quad = quad + t
    mean = dot + bias
    var = (quad + 2.0 * bias * dot + bias * bias - mean * mean).clamp(min=0.0)
    a = inp["gamma"].double()[None] / torch.sqrt(var + (0.0 if mutant == COEF_MUTANTS[2] else EPS))
    shift = inp["beta"].double()[None] - mean * a
    out = torch.empty(B, C, K0 + 1)
    out[..., :K0] = ((a * r[:, None])[..., None] * w[None]).float()
    out[..., K0] = (a * (bias - (r * mu)[:, None] * w.sum(1)[None]) + shift).float()
    return out


def check_coef(got, ref, lim):
    bad = ~torch.isfinite(got)
    err = (got.double() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / lim)
    ratio = torch.where(bad | torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    w = float(ratio.max())
    i = int(ratio.flatten().argmax())
    return ([f"coef: err / limit {w:.3g} at clip {i // (got.shape[1] * 11)} channel {i // 11 % got.shape[1]} coefficient {i % 11}"] if not w <= 1.0 else []), w


# ---------------------------------------------------------------------------------------------------------------------------------
# forms 3 .. 6
def apply_inputs(c):
    g = _gen(c, 4 + c.form)
    B, C, Lw = c.B, c.C, length(c)
    mf = c.form >= 5
    # (form 6 without the waveform norm: the LayerNorm form has no strip scaling -- the norm is what brings the samples to O(1) -- so raw
    #  samples reach the pieces as they are and IEEE-half pieces hold |x| < 65 504 only; un-normalised audio lies in [-1, 1]: moderate gains)
    gains = torch.tensor((MFMA_GAINS if mf and not (c.form == 6 and not c.wav_mom) else VEC_GAINS)[:B], dtype=torch.float64)
    wav = torch.randn(B, Lw, generator=g).double() * (1.0 if mf else 0.25)
    if mf:
        # clip 3 (2^17): its first strip is exact zeros: amax = 0, and kx + ka clamps at 15 (form 6 has no strips: half as many frames there)
        wav[3, :(min(c.T1, 64 if c.form == 5 else 32) - 1) * c.stride + K0] = 0.0
        if c.T1 > 64:
            wav[1, 64 * c.stride:64 * c.stride + 330] = 0.0   # clip 1 (3e-4): a 330-sample strip of exact zeros inside quiet audio (wave 1)
    wav = (wav * gains[:, None]).float()
    if mf:
        wav[0, Lw // 2] = 1.0                            # clip 0: quiet audio (2^-10) with ONE full-scale click
    inp = dict(wav=wav, gains=gains)
    if c.form in (3, 5):
        taps = torch.randn(C, K0, generator=g) * (0.25 if mf else 1.0)
        amp = 1.0 + 0.3 * torch.randn(B, C, generator=g)
        coef = torch.empty(B, C, K0 + 1)
        coef[..., :K0] = (taps[None].double() * amp[..., None].double() / gains[:, None, None]).float()
        coef[..., K0] = 0.3 * torch.randn(B, C, generator=g)
        inp["coef"] = coef
    else:
        inp["w0"] = 0.5 * torch.randn(C, K0, generator=g)
        inp["b0"] = 0.2 * torch.randn(C, generator=g) if c.b0 else None
        inp["gamma"] = 1.0 + 0.3 * torch.randn(C, generator=g)
        inp["beta"] = 0.2 * torch.randn(C, generator=g)
        inp["n_wav"] = c.cpg * Lw
        inp["wav_mom"] = group_moments(wav, c.cpg) if c.wav_mom else None
        mu, r = wave_norm32(inp["wav_mom"], inp["n_wav"], c.cpg, B)
        inp["xn"] = (wav - mu) * r                       # fp32, bit for bit what the kernels stage in LDS
    return inp


def frames(x, c):
    return x[:, :(c.T1 - 1) * c.stride + K0].unfold(-1, K0, c.stride)     # (B, T1, 10)


def strip_scales(c, inp):
    """Form 5: per (clip, frame) the exponents the kernel derives: (tot, xscale exponent, ka, clamped), as int tensors (B, T1) / (B,)."""
    B, T1 = c.B, c.T1
    cmax = inp["coef"][..., :K0].abs().amax((1, 2))
    ka = torch.where(cmax > 0, torch.frexp(cmax)[1], torch.zeros(B, dtype=torch.int32)).clamp(-100, 100).long()
    tot = torch.empty(B, T1, dtype=torch.long)
    clamped = torch.zeros(B, T1, dtype=torch.bool)
    e_all = torch.empty(B, T1, dtype=torch.long)
    for t0 in range(0, T1, 64):
        nfr = min(64, T1 - t0)
        strip = inp["wav"][:, t0 * c.stride:t0 * c.stride + (nfr - 1) * c.stride + K0]
        amax = strip.abs().amax(1)
        e = torch.where(amax > 0, torch.frexp(amax)[1], torch.zeros(B, dtype=torch.int32)).clamp(-100, 100).long()
        raw = -e - ka
        tot[:, t0:t0 + nfr] = raw.clamp(-14, 15)[:, None]
        clamped[:, t0:t0 + nfr] = ((raw < -14) | (raw > 15))[:, None]
        e_all[:, t0:t0 + nfr] = e[:, None]
    return tot, tot + ka[:, None], ka, clamped, e_all


def ln_limit(y, e_y, gam, bet):
    """tests/layernorm_limit.py's two-pass fp32 bound over the last axis of y (fp64), the computed row being y + delta, |delta| <= e_y."""
    D = y.shape[-1]
    mean = lambda t: t.mean(-1, keepdim=True)   # noqa: E731
    mu = mean(y)
    d = y - mu
    v = mean(d * d)
    r = (v + EPS) ** -0.5
    z = d * r
    o = z * gam + bet
    e_c = e_y + mean(e_y)
    e_d = (D + 1) * U * mean(y.abs()) + U * d.abs() + e_c
    rho_v = ((D + 2) * U * v + 2 * mean(d.abs() * e_d) + mean(e_d * e_d)) / (v + EPS) + 2 * U
    rho_r = rho_v / 2 + 2 * U
    e_z = e_d * r + z.abs() * (rho_r + 2 * U)
    return o, gam.abs() * e_z + 2 * U * ((z * gam).abs() + bet.abs())


def apply_reference(c, inp, build):
    """(ref, lim32, z) (B, T1, C) fp64: the reference, the limit of the fp32 value in front of the store, the GELU's argument."""
    mf = c.form >= 5
    if c.form in (3, 5):
        win = frames(inp["wav"], c).double()
        cf = inp["coef"].double()
        z = torch.einsum("btj,bcj->btc", win, cf[..., :K0]) + cf[:, None, :, K0]
        S = torch.einsum("btj,bcj->btc", win.abs(), cf[..., :K0].abs()) + cf[:, None, :, K0].abs()
        bias = cf[:, None, :, K0]
        xs_w, cs_w = win, cf[..., :K0]
    else:
        win = frames(inp["xn"], c).double()
        w = inp["w0"].double()
        b = inp["b0"].double() if inp["b0"] is not None else torch.zeros(c.C, dtype=torch.float64)
        y = torch.einsum("btj,cj->btc", win, w) + b
        S = torch.einsum("btj,cj->btc", win.abs(), w.abs()) + b.abs()
        bias = b.expand(c.B, 1, c.C)
        xs_w, cs_w = win, w[None].expand(c.B, c.C, K0)
    if not mf:
        e = 12 * 2.0 ** -23 * S
    else:
        pp = piece_prec(c, build)
        h, eta = H[pp], ETA_P[pp]
        if c.form == 5:
            tot, xe, ka, _, _ = strip_scales(c, inp)
            xs_w = xs_w * (2.0 ** xe.double())[..., None]
            cs_w = cs_w * (2.0 ** -ka.double())[:, None, None]
            scale = 2.0 ** tot.double()[..., None]
        else:
            scale = torch.ones(c.B, c.T1, 1, dtype=torch.float64)
        taps = 3.1 * h * h * torch.einsum("btj,bcj->btc", xs_w.abs(), cs_w.abs()) + 1.01 * eta * (xs_w.abs().sum(-1, keepdim=True) + cs_w.abs().sum(-1)[:, None, :])
        taps = (taps + (h * h * bias.abs() + eta) * scale) / scale
        e = taps + 34 * 2.0 ** -23 * 1.01 * S
    if c.form in (3, 5):
        lim_pre = e
    else:
        z, lim_pre = ln_limit(y, e, inp["gamma"].double(), inp["beta"].double())
    return G.gelu64(z), 1.13 * lim_pre + G.g_act(gelu_form(c), build, z), z


_cache = collections.OrderedDict()


def apply_data(c, build):
    """(inputs, ref, lim32) of a case of forms 3 .. 6 in a build, computed once and shared by the CPU and the GPU test."""
    mf = c.form >= 5
    key = (c.idx, build if (mf or c.out == "16") else "bf16")
    if key not in _cache:
        inp = apply_inputs(c)
        _cache[key] = (inp,) + apply_reference(c, inp, build)[:2]
        while len(_cache) > 6:
            _cache.popitem(last=False)
    _cache.move_to_end(key)
    return _cache[key]


def out_dtype(c, build):
    return {"f32": torch.float32, "16": G.BUILDS[build][1]}.get(c.out, torch.int32)


def store(c, build, o):
    """fp32 (B, T1, C) -> the rows as the kernel stores them, (B * T1, C) of out_dtype."""
    o2 = o.reshape(-1, c.C)
    if c.out == "f32":
        return o2.clone()
    if c.out == "16":
        return o2.to(G.BUILDS[build][1])
    return L.pack_pairs(*GS.cut(o2, GS.PIECE[piece_prec(c, build)][0]))


def readback(c, build, rows):
    """The stored rows as fp32 values (pair rows: hi + lo)."""
    if c.out.startswith("pk"):
        hi, lo = L.unpack_pairs(rows, GS.PIECE[piece_prec(c, build)][0])
        return hi.float() + lo.float()
    return rows.float()


def check_apply(c, build, rows, ref, lim32):
    """rows (B * T1, C) as stored.  (failures, worst err / limit -- for 16-bit rows err / (lim32 + u_out |ref| + eta), for information)."""
    ref2, lim2 = ref.reshape(-1, c.C), lim32.reshape(-1, c.C)
    got = readback(c, build, rows)
    fails = []
    if torch.isnan(got).any():
        fails.append(f"{int(torch.isnan(got).sum())} NaN (unwritten) elements")
    err = (got.double() - ref2).abs()
    if c.out == "16":
        dtype, u_out = G.BUILDS[build][1], G.BUILDS[build][2]
        lo, hi = (ref2 - lim2).float().to(dtype).double(), (ref2 + lim2).float().to(dtype).double()
        out = ~((got.double() >= lo) & (got.double() <= hi))
        if out.any():
            i = int(out.flatten().float().argmax())
            fails.append(f"{int(out.sum())} elements outside [rn16(ref - lim32), rn16(ref + lim32)], first at row {i // c.C} channel {i % c.C}")
        lim = lim2 + u_out * ref2.abs() + G.ETA[build]
    else:
        lim = lim2 + (U * ref2.abs() if c.out == "f32" else GS.cut_term(piece_prec(c, build), ref2))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / lim)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    w = float(ratio.max())
    if c.out != "16" and not w <= 1.0:
        i = int(ratio.flatten().argmax())
        fails.append(f"err / limit {w:.3g} at row {i // c.C} channel {i % c.C}")
    return fails, w


# ---------------------------------------------------------------------------------------------------------------------------------
# a correct kernel of forms 3 .. 6 on the CPU, and the mutants
APPLY_MUTANTS = ("x_lo w_hi dropped", "lo piece truncated", "two channels of the table permutation swapped", "bias column without the strip scale",
                 "unscale by 2^e instead of 2^tot in a clamped strip", "clamped frame nfr - 1 stored past the tail", "odd last frame of the layer kernel skipped",
                 "mean over 512 when C < 512", "b % cpg for b / cpg", "polynomial GELU where gelu_fast is due")
BLIND = ("lo piece truncated",)     # module docstring: WHAT THE LIMITS CANNOT SEE


def applies(mutant, c, build="bf16"):
    """The cases a mutant of forms 3 .. 6 can show in.
      x_lo w_hi dropped, swapped channels      every matrix-pipe case (distinct random weights per channel)
      bias without the strip scale             form 5 (form 6 has no scaling): every clip's 2^tot differs from 1
      unscale by 2^e                           form 5: clip 3's first strip is clamped in every case (apply_inputs)
      frame stored past the tail               forms 5, 6 with T1 % 16 != 0: the A fragment's clamped rows
      odd last frame skipped                   form 4 with T1 odd
      mean over 512                            form 4 with C < 512
      b % cpg                                  forms 4, 6 with waveform moments and cpg < B (with cpg == B both expressions name group 0
                                               for b = 0 only; the others read outside the moments: the hook's buffers end there)
      polynomial GELU                          fp32 rows and pair rows, in the bf16 build, whose polynomial is good to 1e-4 |x| only; forms 3, 5
                                               (behind a LayerNorm over 512 channels the fp32 bound itself reaches 1e-4 |z|: layernorm_limit.py)"""
    i = APPLY_MUTANTS.index(mutant)
    mf = c.form >= 5
    if i in (0, 1, 2):
        return mf
    if i in (3, 4):
        return c.form == 5
    if i == 5:
        return mf and c.T1 % 16 != 0
    if i == 6:
        return c.form == 4 and c.T1 % 2 == 1
    if i == 7:
        return c.form == 4 and c.C < 512
    if i == 8:
        return c.form in (4, 6) and c.wav_mom and c.cpg < c.B
    return c.out != "16" and build == "bf16" and c.form in (3, 5)


def _ordered_sum(terms, order):
    acc = torch.zeros_like(terms[0])
    for t in (reversed(terms) if order else terms):
        acc = acc + t
    return acc


def _row_sum(t, order):
    return (t.flip(-1) if order else t).cumsum(-1)[..., -1:]


def simulate_apply(c, build, inp, order=0, mutant=None):
    """(rows as stored with NaN where nothing was written, guard_written).  fp32 arithmetic in two summation orders, the piece arithmetic in
    the piece type."""
    m = APPLY_MUTANTS.index(mutant) if mutant else -1
    B, C, T1 = c.B, c.C, c.T1
    mf = c.form >= 5
    guard_written = False
    if c.form in (3, 5):
        x = inp["wav"]
        wt = inp["coef"][..., :K0]
        bias = inp["coef"][..., K0][:, None, :]
    else:
        if m == 8:
            gi = (torch.arange(B) % c.cpg).clamp(max=B // c.cpg - 1) * c.cpg
            mu, r = wave_norm32(inp["wav_mom"], inp["n_wav"], c.cpg, B)
            x = (inp["wav"] - mu[gi]) * r[gi]
        else:
            x = inp["xn"]
        wt = inp["w0"][None].expand(B, C, K0)
        bias = (inp["b0"] if inp["b0"] is not None else torch.zeros(C))[None, None, :].expand(B, 1, C)
    win = frames(x, c)                                                     # (B, T1, 10) fp32
    if not mf:
        terms = [bias.expand(B, T1, C)] + [win[..., j:j + 1] * wt[:, None, :, j] for j in range(K0)]
        acc = _ordered_sum(terms, order)
    else:
        pd = GS.PIECE[piece_prec(c, build)][0]
        if c.form == 5:
            tot, xe, ka, clamped, e_all = strip_scales(c, inp)
            xs = win * (2.0 ** xe.float())[..., None]
            cs = wt * (2.0 ** -ka.float())[:, None, None]
            one = 2.0 ** tot.float()[..., None]
            unscale = 1.0 / one
            if m == 4:
                unscale = torch.where(clamped[..., None], 2.0 ** (e_all + ka[:, None]).float()[..., None], unscale)
            if m == 3:
                one = torch.ones_like(one)
        else:
            xs, cs = win, wt
            one = unscale = torch.ones(B, T1, 1)
        cut = (lambda v: (v.to(pd), G.truncate_to(v - v.to(pd).float(), pd))) if m == 1 else (lambda v: GS.cut(v, pd))   # noqa: E731
        xh, xl = (t.float() for t in cut(xs))
        ch, cl = (t.float() for t in cut(cs))
        bh, bl = (t.float() for t in cut(bias.contiguous()))
        if m == 2:
            perm = torch.arange(C)
            perm[8], perm[9] = 9, 8
            ch, cl, bh, bl = ch[:, perm], cl[:, perm], bh[..., perm], bl[..., perm]
        terms = [xh[..., j:j + 1] * ch[:, None, :, j] for j in range(K0)]
        if m != 0:
            terms += [xl[..., j:j + 1] * ch[:, None, :, j] for j in range(K0)]
        terms += [xh[..., j:j + 1] * cl[:, None, :, j] for j in range(K0)] + [(bh * one).expand(B, T1, C), (bl * one).expand(B, T1, C)]
        acc = _ordered_sum(terms, order) * unscale
    if c.form in (4, 6):
        Cd = 512.0 if m == 7 else float(C)
        mean = _row_sum(acc, order) / Cd
        d = acc - mean
        var = _row_sum(d * d, order) / Cd
        rstd = (var + torch.tensor(1e-5)).double().rsqrt().float()
        acc = (d * rstd) * inp["gamma"] + inp["beta"]
    form = gelu_form(c)
    if m == 9:
        form = "poly"
    o = L.gelu_poly32(acc, build) if form == "poly" else torch.nn.functional.gelu(acc.double()).float()
    o = o.clone()
    if m == 6:
        o[:, T1 - 1] = float("nan")          # never written: the poison stays
    if m == 5:
        last = o[:, T1 - 1].clone()
        o[1:, 0] = last[:-1]                  # clip b's frame T1 is clip b + 1's frame 0; the last clip's is the guard row behind the output
        guard_written = True
    return store(c, build, o), guard_written
