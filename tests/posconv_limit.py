"""What tests/test_gpu_encoder_glue.py (GPU) and tests/test_posconv_limit.py (CPU) share for the glue of the transformer encoder: the three
forms of the positional conv (csrc/api_encoder.hip positional_conv with the gather / scatter kernels of csrc/encoder_ops.hip), WavLM's
relative-position table and its two gate kernels.  Case tables, inputs, fp64 references, per-element limits, and a simulation of every
form that follows the kernels' indexing, with the mutants the limits must catch.

POSITIONAL CONV.  reference(): F.conv1d in float64 with padding = kp // 2, groups = G and the last frame dropped for an even kp, on the
operands AS THE STEP ROUNDS THEM -- the weights after the host's folds (weight norm in double, rounded once to fp32) rounded to the storage
type at upload; the input after the fp32 fmaf of the BatchNorm fold (the zero padding stays zero) rounded to the 16-bit type by the gather;
in the split modes the three-term value of the (hi, lo) pieces (tests/gemm_split.py) -- then + bias, exact-erf GELU, + h.  With z the
pre-activation and S the same sum over absolute values, the limit composes what the other kernel tests already use and adds no constant:

    plain        the product's own limit with GELU, fp32 output and the residual in its epilogue: gemm_limit.limit (16-bit modes),
                 gemm_split.limit (fp32 and split modes), K = kp cg
    multi-frame  y = gelu(z) leaves the product in 16 bits (16-bit modes: gemm_limit.limit with 16-bit output, i.e. the store's interval
                 u |y| + eta on top of the fp32 stage) or in fp32 (split modes: gemm_split.limit), K = (kp + Pf - 1) cg of which kp cg terms are
                 non-zero; the scatter's fp32 add rounds once:  lim = lim_y + 2^-24 (|ref| + lim_y)
    stack        per layer: the conv without activation into fp32 (the product's limit, K = kp cg), then LayerNorm over D without affine, eps 1e-5,
                 + GELU in fp32 (tests/layernorm_limit.py, the GELU form of its fp32 output); a layer's input error e is carried forward
                 to first order, as layernorm_limit.py carries its own e_d: through the gather's rounding (16-bit modes: |rn(x + e) - rn(x)| <=
                 e + 2 u |x| + eta), the conv (|W| * e), the LayerNorm (ln_limit: e_d = e_mu + u |d| + e + mean e, the same formulas
                 after that) and GELU (slope 1.13); the final h + pos rounds once in fp32.

RELATIVE-POSITION TABLE.  HF's _relative_positions_bucket in torch fp32 on the CPU (bucket_hf), a NumPy fp32 transcription of the kernel
(bucket_kernel_np) and the floor of the same expression in fp64 (bucket_f64) with its edge distances (edges): |d| whose fp64 value lies
within 1e-4 of an integer below the clamp.  tests/test_posconv_limit.py asserts that the three agree at every distance below 8192 for every
configuration of CONFIGS and that no configuration has more than 4 edge distances; the GPU test demands equality with bucket_hf.

GATE.  gate = ga (gb c - 1) + 2, ga / gb = sigmoid(x . wa + ba), sigmoid(x . wb + bb), wa / wb the fp32 sums of rows 0-3 / 4-7 of
gru_rel_pos_linear in the host's order (fold_gate).  In fp64 from those: s, sigma = sum |x_d w_d| + |b|.  An fp32 FMA chain of dh terms --
and the vec kernel's tree: 8 terms per lane, log2(dh / 8) exchange steps, the bias: fewer roundings on every path -- obeys
|ds| <= (dh + 2) 2^-24 sigma.  The sigmoid's slope is at most 1/4; expf, the fp32 add and the division are allowed SIGMOID_ALLOW = 16 * 2^-24
relative, the constant part of the softmax allowance of the attention limit in tests/gemm_limit.py (expf to 1 ulp, the reciprocal, the
multiply).  Then, each fp32 operation rounding once (u = 2^-24):
    e_g  = ds / 4 + 16 u g                                  for ga and gb
    e_t  = |c| e_b + u (|gb c| + |t|)                       t = gb c - 1
    e_m  = |t| e_a + ga e_t + e_a e_t + u |ga t|            m = ga t
    lim  = e_m + u |gate|"""
import collections
import math

import numpy as np
import torch
import torch.nn.functional as F

import gemm_limit as G
import gemm_split as GS
import layernorm_limit as L

U = 2.0 ** -24
MODES = ("fp32", "bf16", "f16", "bf16x3", "fp16x3")
# mode -> (library variant, the modules' precision name, svt_precision code, storage dtype, gemm_limit build of a 16-bit mode, gemm_split precision)
MODE = {"fp32": (None, "fp32", 0, torch.float32, None, 0), "bf16": (None, "bf16", 1, torch.bfloat16, "bf16", None),
        "f16": ("f16", "fp16", 1, torch.float16, "f16", None), "bf16x3": (None, "bf16x3", 2, torch.float32, None, 2),
        "fp16x3": (None, "fp16x3", 3, torch.float32, None, 3)}
SIXTEEN = ("bf16", "f16")
SPLIT = ("bf16x3", "fp16x3")

# ---------------------------------------------------------------------------------------------------------------------------------
# the positional-conv cases.  form: the form the plan must choose ("plain" / "multi" / "stack"); bn: eval BatchNorm1d in front; depth: stacked
# layers (1 = the single weight-normed conv); tag: what the case is there for
PCase = collections.namedtuple("PCase", "form cg G kp B T bn depth modes tag")


def _p(form, cg, G, kp, B, T, modes, bn=False, depth=1, tag=""):
    return PCase(form, cg, G, kp, B, T, bn, depth, tuple(modes), tag)


def pf_of(c):
    """Frames per GEMM row of the multi-frame form the handle holds, 0: none (csrc/api_encoder.hip finalize_pos_conv)."""
    Pf = 256 // c.cg
    ok = c.depth == 1 and Pf >= 2 and c.cg % 8 == 0 and ((c.kp + Pf - 1) * c.cg) % 64 == 0
    return Pf if ok else 0


def form_of(c, mode):
    """The form plan_encoder chooses: the multi-frame one in the reduced modes from 128 GEMM rows up."""
    if c.depth > 1:
        return "stack"
    Pf = pf_of(c)
    return "multi" if (mode != "fp32" and Pf and c.B * ((c.T + Pf - 1) // Pf) >= 128) else "plain"


_R16 = SIXTEEN + SPLIT
PCASES = (
    # plain form, fp32: the float gather; one frame, fewer frames than half a kernel, more than one block of the gather
    [_p("plain", 8, 4, kp, B, T, ("fp32",)) for kp in (16, 5) for (B, T) in ((1, 1), (2, 7), (2, 33))] +
    # plain form, 16-bit: the 8-wide gather (the element-wise 16-bit gather needs cg % 8 != 0, which svt_encoder_create refuses);
    # T < kp / 2: every window is mostly padding
    [_p("plain", 16, 2, 16, 2, T, SIXTEEN) for T in (5, 33)] + [_p("plain", 16, 2, 16, 2, 33, SPLIT)] +
    # multi-frame form: T % Pf in {0, 1, Pf - 1}
    [_p("multi", 64, 2, 8, 2, T, _R16) for T in (256, 253, 255)] +
    [_p("multi", 48, 2, 16, 2, T, _R16) for T in (320, 321, 324)] +
    [_p("multi", 16, 2, 17, 1, T, _R16, tag="odd-kernel") for T in (2048, 2033)] +
    # the switch at 127 / 128 rows: two forms that must agree
    [_p("plain", 64, 2, 8, 1, 508, _R16, tag="switch"), _p("multi", 64, 2, 8, 1, 509, _R16, tag="switch")] +
    # BatchNorm in front, running means far from 0
    [_p("plain", 16, 2, 16, 2, 33, ("fp32",) + SIXTEEN, bn=True), _p("multi", 64, 2, 8, 2, 253, _R16, bn=True)] +
    # the data2vec stack
    [_p("stack", 16, 2, 19, 2, 40, ("fp32",) + SIXTEEN, depth=d) for d in (2, 5)] +
    # eligibility refused: Pf = 10 and (kp + 9) 24 % 64 != 0 -> plain however many rows
    [_p("plain", 24, 2, 16, 2, 700, _R16, tag="not-eligible")])
RUNS = [(c, m) for c in PCASES for m in c.modes]


def pcase_id(c):
    return (f"{c.form}-cg{c.cg}-G{c.G}-kp{c.kp}-B{c.B}-T{c.T}" + ("-bn" if c.bn else "") + (f"-depth{c.depth}" if c.depth > 1 else "") +
            (f"-{c.tag}" if c.tag else ""))


def geometry_key(c):
    """What a handle depends on: cases that differ in (B, T) only share one."""
    return (c.cg, c.G, c.kp, c.bn, c.depth)


def make_params(c):
    """The positional conv's parameters under their HF keys (fp32 CPU tensors), seeded by the geometry.  The single conv is weight-normed
    (g, v) unless a BatchNorm stands in front of it (HF: then a plain conv); the stack's layers are plain convs."""
    D = c.cg * c.G
    g = torch.Generator().manual_seed(7000 + 31 * c.cg + 7 * c.kp + c.G + 1000 * c.depth + (500 if c.bn else 0))
    fan = c.cg * c.kp
    p = collections.OrderedDict()
    pc = "encoder.pos_conv_embed."
    if c.depth > 1:
        # A worst-case bound carried through a layer grows by |W|_1 / std(z) (the conv spreads a uniform input error over a whole filter row,
        # the LayerNorm divides by the row's spread): small filters under a bias of spread 1 keep that factor below 1, so the
        # limit of depth 5 is as sharp as that of depth 2 (the LayerNorm's own bound passes a uniform error on about threefold: hence
        # |W|_1 ~ 0.25 behind layer 0, whose input carries no error).  Layer 0 has a bias of 1e-3 instead: with make_h's second clip its
        # variance is of the order of eps = 1e-5, where an eps of 1e-6 shows
        for i in range(c.depth):
            p[f"{pc}layers.{i}.conv.weight"] = torch.randn(D, c.cg, c.kp, generator=g) * ((1.0 if i == 0 else 0.3) / fan)
            p[f"{pc}layers.{i}.conv.bias"] = (1e-3 if i == 0 else 1.0) * torch.randn(D, generator=g)
        return p
    if c.bn:
        p[pc + "conv.weight"] = torch.randn(D, c.cg, c.kp, generator=g) * (2.0 / fan) ** 0.5
        p[pc + "batch_norm.weight"] = 1.0 + 0.3 * torch.randn(D, generator=g)
        p[pc + "batch_norm.bias"] = 0.5 * torch.randn(D, generator=g)
        p[pc + "batch_norm.running_mean"] = 3.0 + torch.randn(D, generator=g)      # far from 0: a shift leaking into the padding shows
        p[pc + "batch_norm.running_var"] = 0.5 + torch.rand(D, generator=g)
    else:
        p[pc + "conv.parametrizations.weight.original0"] = (0.6 + 0.1 * torch.randn(1, 1, c.kp, generator=g).abs()) * (D * c.cg / fan) ** 0.5 * 2.0 ** 0.5
        p[pc + "conv.parametrizations.weight.original1"] = torch.randn(D, c.cg, c.kp, generator=g)
    p[pc + "conv.bias"] = 0.5 * torch.randn(D, generator=g)
    return p


def make_h(c):
    """h (B, T, D) fp32.  The stack's second clip is scaled to 0.05, where the first LayerNorm's variance is of the order of its eps (make_params)."""
    D = c.cg * c.G
    T = max(x.T for x in PCASES if x.tag == "switch") if c.tag == "switch" else c.T   # the two sides of the switch share their frames
    g = torch.Generator().manual_seed(9000 + c.B * 10007 + T * 13 + D)
    h = torch.randn(c.B, T, D, generator=g)[:, :c.T].contiguous()
    if c.depth > 1:
        h[1] *= 0.05
    return h


def folded(c, p):
    """The host's folds in its arithmetic: (list of (weight (D, cg, kp) fp32, bias (D) fp32) per layer, BatchNorm (scale, shift) fp32 or None)."""
    pc = "encoder.pos_conv_embed."
    if c.depth > 1:
        return [(p[f"{pc}layers.{i}.conv.weight"], p[f"{pc}layers.{i}.conv.bias"]) for i in range(c.depth)], None
    if c.bn:
        sc = p[pc + "batch_norm.weight"].double() / (p[pc + "batch_norm.running_var"].double() + 1e-5).sqrt()
        sh = p[pc + "batch_norm.bias"].double() - p[pc + "batch_norm.running_mean"].double() * sc
        return [(p[pc + "conv.weight"], p[pc + "conv.bias"])], (sc.float(), sh.float())
    gg, v = p[pc + "conv.parametrizations.weight.original0"].double(), p[pc + "conv.parametrizations.weight.original1"].double()
    w = (gg * v / (v * v).sum((0, 1), keepdim=True).sqrt()).float()   # weight norm over dim 2: one norm per tap (host.cpp weight_norm_fold)
    return [(w, p[pc + "conv.bias"])], None


def bn_apply(h, bn):
    """The gather's fp32 fmaf(h, scale, shift): the exact product and sum in fp64 (48 + a few bits), rounded once to fp32."""
    return h if bn is None else (h.double() * bn[0].double() + bn[1].double()).float()


def _conv64(x, w, c):
    """(B, T, D) x (D, cg, kp) -> (B, T, D) in fp64: SamePad conv of HF (padding kp // 2, the last frame dropped for an even kernel)."""
    y = F.conv1d(x.double().transpose(1, 2), w.double(), padding=c.kp // 2, groups=c.G)
    return y[..., :x.shape[1]].transpose(1, 2)


def _z_and_s(c, mode, x, w, bias):
    """(z, S) of one conv layer on the fp32 input x (already BatchNorm-folded) and the fp32 weight w, operands rounded as `mode` rounds them."""
    dtype, sp = MODE[mode][3], MODE[mode][5]
    if mode in SIXTEEN:
        xr, wr = x.to(dtype), w.to(dtype)
        z, S = _conv64(xr, wr, c), _conv64(xr.abs(), wr.abs(), c)
    elif sp:
        pd = GS.PIECE[sp][0]
        (xh, xl), (wh, wl) = GS.cut(x, pd), GS.cut(w, pd)
        z = _conv64(xh.double() + xl.double(), wh, c) + _conv64(xh, wl, c)
        S = _conv64(xh.double().abs() + xl.double().abs(), wh.abs(), c) + _conv64(xh.abs(), wl.abs(), c)
    else:
        z, S = _conv64(x, w, c), _conv64(x.abs(), w.abs(), c)
    return z + bias.double(), S + bias.double().abs()


def _product_limit(c, mode, K, z, S, ref, act, out16, resid, gelu_form):
    """The product's own per-element limit: gemm_limit.limit (16-bit modes; gelu_form "fast" / "poly" as the kernel that ran calls it) or
    gemm_split.limit (fp32: K terms, split modes: 3 K)."""
    if mode in SIXTEEN:
        kid = 1032 if gelu_form == "fast" else 5128   # a family whose gemm_limit.gelu_form is the requested one
        gc = G.C(kid, 1, 1, K, act=act, out_f32=0 if out16 else 1, resid=resid is not None)
        assert act != 1 or G.gelu_form(gc) == gelu_form
        return G.limit(gc, MODE[mode][4], z, S, ref, resid)
    sc = GS.S(2128, 1, 1, K, act=act, resid=resid is not None, prec=0)
    return GS.limit(sc, MODE[mode][5], z, S, ref, resid)


def ln_limit(t, e_in, eps):
    """(y, lim_y) of LayerNorm over the last axis without affine in fp64, for an fp32 two-pass kernel whose input is within e_in of t: the
    formulas of layernorm_limit.reference with gamma = 1, beta = 0 and e_d = e_mu + u |d| + e_in + mean(e_in)."""
    D = t.shape[-1]
    eps = float(torch.tensor(eps, dtype=torch.float32))
    mu = t.mean(-1, keepdim=True)
    d = t - mu
    v = (d * d).mean(-1, keepdim=True)
    r = (v + eps) ** -0.5
    z = d * r
    e_mu = (D + 1) * U * t.abs().mean(-1, keepdim=True)
    e_d = e_mu + U * d.abs() + e_in + e_in.mean(-1, keepdim=True)
    rho_v = ((D + 2) * U * v + 2 * (d.abs() * e_d).mean(-1, keepdim=True) + (e_d * e_d).mean(-1, keepdim=True)) / (v + eps) + 2 * U
    rho_r = rho_v / 2 + 2 * U
    e_z = e_d * r + z.abs() * (rho_r + 2 * U)
    return z, e_z + 2 * U * z.abs()


def reference(c, mode, gelu_form="fast", params=None, h=None):
    """(ref, lim) in fp64, (B, T, D) each, of the case in a mode (module docstring).  gelu_form: the GELU the product kernel that ran calls
    (16-bit modes; tests/gemm_limit.py gelu_form of its key-39 id)."""
    params = make_params(c) if params is None else params
    h = make_h(c) if h is None else h
    layers, bn = folded(c, params)
    form = form_of(c, mode)
    K = c.kp * c.cg
    if form == "stack":
        assert mode not in SPLIT, "the stack's carried error is derived for fp32 and 16-bit storage"
        cur, e = h.double(), torch.zeros_like(h, dtype=torch.float64)
        dtype = MODE[mode][3]
        for i, (w, b) in enumerate(layers):
            x32 = cur.float()   # layer 0: h itself; later layers: the kernel holds an fp32 value within e of cur
            if i > 0:
                e = e + U * cur.abs()
                if mode in SIXTEEN:   # |rn(a) - rn(b)| <= |a - b| (1 + u) + 2 u |b| + eta
                    u16 = G.BUILDS[MODE[mode][4]][2]
                    e = e * (1 + u16) + 2 * u16 * cur.abs() + G.ETA[MODE[mode][4]]
            z, S = _z_and_s(c, mode, x32, w, b)
            wr = w.to(dtype).double().abs() if mode in SIXTEEN else w.double().abs()
            lim_z = _product_limit(c, mode, K, z, S, z, 0, False, None, "fast") + _conv64(e, wr, c)
            y, lim_y = ln_limit(z, lim_z, 1e-5)
            cur = G.gelu64(y)
            e = 1.13 * lim_y + G.g_act("fast", None, y) + U * cur.abs()   # gelu_erf into fp32 (layernorm_limit.gelu_form: yF is written)
        ref = h.double() + cur
        return ref, e + U * (ref.abs() + e)
    (w, b), = layers
    z, S = _z_and_s(c, mode, bn_apply(h, bn), w, b)
    if form == "plain":
        ref = h.double() + G.gelu64(z)
        return ref, _product_limit(c, mode, K, z, S, ref, 1, False, h, gelu_form)
    Pf = pf_of(c)
    y = G.gelu64(z)
    lim_y = _product_limit(c, mode, (c.kp + Pf - 1) * c.cg, z, S, y, 1, mode in SIXTEEN, None, gelu_form)
    ref = h.double() + y
    return ref, lim_y + U * (ref.abs() + lim_y)


_cache = collections.OrderedDict()


def case_data(c, mode, gelu_form="fast"):
    """(params, h, ref, lim) of a run, computed once and shared between the tests that need it; never written to."""
    key = (c, mode, gelu_form)
    if key not in _cache:
        params, h = make_params(c), make_h(c)
        _cache[key] = (params, h) + reference(c, mode, gelu_form, params, h)
        while len(_cache) > 6:
            _cache.popitem(last=False)
    _cache.move_to_end(key)
    return _cache[key]


def worst(got, ref, lim):
    """(worst err / limit, text saying where): a NaN counts as infinitely far."""
    ratio = (got.double() - ref).abs() / lim
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    i = int(ratio.argmax())
    b, t, d = np.unravel_index(i, ratio.shape)
    return ratio.flatten()[i].item(), (f"clip {b} frame {t} channel {d}: got {got[b, t, d].item():.9g} ref {ref[b, t, d].item():.9g} "
                                      f"limit {lim[b, t, d].item():.3e}")


# ---------------------------------------------------------------------------------------------------------------------------------
# the step simulated in fp32 with the kernels' indexing (csrc/encoder_ops.hip, csrc/host.cpp posconv_multiframe, csrc/api_encoder.hip)
PMUTANTS = ("gather centred on kp/2 - 1", "filter of row j shifted by j - 1", "tail frames from row Tq - 2", "bias only in rows j = 0",
            "BatchNorm shift leaks into the padding", "group and clip swapped in the scatter", "groups reversed", "GELU in front of the bias",
            "residual missing", "stack: eps 1e-6", "stack: final + h missing", "stack: layer 0's weight in every layer")


def papplies(mutant, c, mode):
    """The runs a mutant can show in."""
    i, form = PMUTANTS.index(mutant), form_of(c, mode)
    Pf = pf_of(c)
    if i == 0:
        return form != "stack"
    if i in (1, 3):
        return form == "multi"
    if i == 5:
        return form == "multi" and c.B > 1   # one clip: [group][clip] and [clip][group] are the same index
    if i == 6:
        return form != "stack"
    if i == 2:
        return form == "multi" and c.T % Pf != 0 and (c.T + Pf - 1) // Pf >= 2
    if i == 4:
        return c.bn
    if i in (7, 8):
        return form != "stack"
    return form == "stack"


def _store(x, mode):
    return x.to(MODE[mode][3]) if mode in SIXTEEN else x


def _gather(h, c, Tp, bn, mode, m):
    """posconv_gather_*: (B, G, Tp, cg) in the storage type; frame tp holds h[tp - kp // 2], zero outside [0, T)."""
    B, T, D = h.shape
    t = torch.arange(Tp) - (c.kp // 2 - 1 if m == 0 else c.kp // 2)
    ok = (t >= 0) & (t < T)
    v = torch.zeros(B, Tp, D)
    v[:, ok] = h[:, t[ok]]
    if bn is not None:
        f = bn_apply(v, bn)
        v = f if m == 4 else torch.where(ok[None, :, None], f, v)
    return _store(v.reshape(B, Tp, c.G, c.cg).permute(0, 2, 1, 3).contiguous(), mode)


def _matmul(A, W, mode):
    """A (M, K) x W (N, K)^T in fp32 from operands in the storage type; split modes: the three piece products."""
    sp = MODE[mode][5]
    if sp:
        return GS.simulate(A, W, None, sp) if A.shape[1] % 32 == 0 else _three(A, W, sp)
    return A.float() @ W.float().t()


def _three(A, W, sp):
    pd = GS.PIECE[sp][0]
    (ah, al), (wh, wl) = (tuple(t.float() for t in GS.cut(x, pd)) for x in (A, W))
    return al @ wh.t() + ah @ wh.t() + ah @ wl.t()


def _tap_major(w, c):
    """(D, cg, kp) -> (G, cg_out, kp * cg_in): host.cpp tap_major."""
    return w.permute(0, 2, 1).reshape(c.G, c.cg, c.kp * c.cg)


def _plain_product(posg, w, bias, c, T, mode):
    """z (B, T, D) fp32: one product per (clip, group), row t = frames t .. t + kp - 1 of the gathered operand."""
    B = posg.shape[0]
    wt = _store(_tap_major(w, c), mode)
    idx = torch.arange(T)[:, None] + torch.arange(c.kp)[None, :]
    z = torch.empty(B, T, c.G * c.cg)
    for b in range(B):
        for g in range(c.G):
            A = posg[b, g][idx].reshape(T, c.kp * c.cg)
            z[b, :, g * c.cg:(g + 1) * c.cg] = _matmul(A, wt[g], mode)
    return z


def simulate(c, mode, params, h, mutant=None):
    """The step's output (B, T, D) fp32 from a correct kernel chain in fp32 torch arithmetic, or from one of PMUTANTS."""
    m = PMUTANTS.index(mutant) if mutant else -1
    layers, bn = folded(c, params)
    form = form_of(c, mode)
    B, T, D = h.shape
    gelu = lambda x: F.gelu(x.double()).float()   # noqa: E731  (erf GELU evaluated exactly, rounded once)
    if form == "stack":
        cur = h
        for i, (w, b) in enumerate(layers):
            if m == 11:
                w = layers[0][0]
            z = _plain_product(_gather(cur, c, T + c.kp, None, mode, -1), w, b, c, T, mode) + b
            mean = z.mean(-1, keepdim=True)
            d = z - mean
            var = (d * d).mean(-1, keepdim=True)
            rstd = (var + torch.tensor(1e-6 if m == 9 else 1e-5)).double().rsqrt().float()
            cur = gelu(d * rstd)
        return cur.clone() if m == 10 else h + cur
    (w, b), = layers
    if form == "plain":
        posg = _gather(h, c, T + c.kp, bn, mode, m)
        if m == 6:
            posg = posg.flip(1)
        z = _plain_product(posg, w, b, c, T, mode)
        y = gelu(z) + b if m == 7 else gelu(z + b)
        return y if m == 8 else h + y
    Pf = pf_of(c)
    Tq = (T + Pf - 1) // Pf
    Tp = Tq * Pf + c.kp
    posg = _gather(h, c, Tp, bn, mode, m)
    # posconv_multiframe: row j * cg + co of a group holds the filter shifted by j taps
    Kp = (c.kp + Pf - 1) * c.cg
    wt = _tap_major(w, c)
    wP = torch.zeros(c.G, Pf, c.cg, Kp)
    for j in range(Pf):
        s = max(j - 1, 0) if m == 1 else j
        wP[:, j, :, s * c.cg:(s + c.kp) * c.cg] = wt
    wP = _store(wP.reshape(c.G, Pf * c.cg, Kp), mode)
    bP = b.reshape(c.G, 1, c.cg).expand(c.G, Pf, c.cg).clone()
    if m == 3:
        bP[:, 1:] = 0.0
    bP = bP.reshape(c.G, Pf * c.cg)
    idx = (torch.arange(Tq) * Pf)[:, None] + torch.arange(c.kp + Pf - 1)[None, :]
    y = torch.empty(c.G, B, Tq, Pf, c.cg)
    for g in range(c.G):
        for bb in range(B):
            A = posg[bb, g][idx].reshape(Tq, Kp)
            acc = _matmul(A, wP[g], mode)
            yy = gelu(acc) + bP[g] if m == 7 else gelu(acc + bP[g])
            y[g, bb] = _store(yy, mode).float().reshape(Tq, Pf, c.cg)
    # posconv_scatter_add_kernel: frame t = q Pf + j of group g reads y[g][b Tq + q][j cg + c]
    t = torch.arange(T)
    q, j = t // Pf, t % Pf
    if m == 2:
        q = torch.where(t >= T - T % Pf, torch.full_like(q, Tq - 2), q)
    flat = y.reshape(c.G * B, Tq, Pf, c.cg)
    pos = torch.empty(B, T, D)
    for bb in range(B):
        for g in range(c.G):
            gi = c.G - 1 - g if m == 6 else g
            z1 = bb * c.G + gi if m == 5 else gi * B + bb
            pos[bb, :, g * c.cg:(g + 1) * c.cg] = flat[z1, q, j]
    return pos if m == 8 else h + pos


# ---------------------------------------------------------------------------------------------------------------------------------
# WavLM's relative-position buckets
CONFIGS = ((320, 800), (320, 1000), (8, 16), (16, 40), (32, 40), (64, 40), (16, 128), (32, 128), (64, 128), (32, 64))   # (num_buckets, max_distance)
TABLE_T = lambda me: (1, 2, me + 1, 400, 900, 4097)   # noqa: E731


def bucket_hf(a, num_buckets, max_distance):
    """HF modeling_wavlm.py _relative_positions_bucket for |d| = a (int64 tensor), in torch fp32 on the CPU, op for op; without the sign's half."""
    nb = num_buckets // 2
    max_exact = nb // 2
    is_small = a < max_exact
    big = torch.log(a.float() / max_exact)
    big = big / math.log(max_distance / max_exact)
    big = big * (nb - max_exact)
    big = (max_exact + big).to(torch.long)
    big = torch.min(big, torch.full_like(big, nb - 1))
    return torch.where(is_small, a, big)


def bucket_kernel_np(a, num_buckets, max_distance):
    """relpos_table_kernel's arithmetic in NumPy fp32, statement by statement."""
    nb = num_buckets // 2
    me = nb // 2
    a = np.asarray(a)
    with np.errstate(divide="ignore"):
        v = np.log(a.astype(np.float32) / np.float32(me))
    v = v / np.float32(math.log(float(max_distance) / float(me)))
    v = v * np.float32(nb - me)
    s = np.float32(me) + v
    lb = np.where(np.isfinite(s), s, 0).astype(np.int64)
    return np.where(a < me, a, np.minimum(lb, nb - 1))


def _bucket_value64(a, num_buckets, max_distance):
    nb = num_buckets // 2
    me = nb // 2
    with np.errstate(divide="ignore"):
        return me + np.log(np.asarray(a, dtype=np.float64) / me) / math.log(max_distance / me) * (nb - me)


def bucket_f64(a, num_buckets, max_distance):
    nb = num_buckets // 2
    me = nb // 2
    a = np.asarray(a)
    v = _bucket_value64(np.maximum(a, 1), num_buckets, max_distance)
    return np.where(a < me, a, np.minimum(np.floor(v).astype(np.int64), nb - 1))


def edges(num_buckets, max_distance, limit=8192):
    """Distances a in [max_exact, limit) whose fp64 bucket value lies within 1e-4 of an integer below the clamp."""
    nb = num_buckets // 2
    me = nb // 2
    a = np.arange(me, limit)
    v = _bucket_value64(a, num_buckets, max_distance)
    near = np.abs(v - np.round(v)) < 1e-4
    return [int(x) for x in a[near & (np.round(v) <= nb - 1)]]


def table_reference(H, T, num_buckets, max_distance):
    """pb (H, 2 T - 1) for rel_attn_embed[bucket][h] = bucket H + h: key - query = d > 0 takes the upper half of the buckets."""
    d = torch.arange(-(T - 1), T)
    bucket = bucket_hf(d.abs(), num_buckets, max_distance) + (d > 0).long() * (num_buckets // 2)
    return (bucket[None, :] * H + torch.arange(H)[:, None]).float()


# ---------------------------------------------------------------------------------------------------------------------------------
# the gate
SIGMOID_ALLOW = 16 * U   # expf to 1 ulp, the add, the division: the constant part of tests/gemm_limit.py attn_limit's softmax allowance
GCase = collections.namedtuple("GCase", "dh H B T vec")
GCASES = ([GCase(dh, H, B, T, True) for (dh, H) in ((64, 3), (8, 4), (128, 2)) for (B, T) in ((1, 1), (2, 5), (3, 43))] +
          # one thread per head: head sizes whose eighth is no power of two (a head size that is no multiple of 8 is refused at create)
          [GCase(dh, 2, B, T, False) for dh in (48, 24) for (B, T) in ((2, 5), (3, 43))])
GBLOCKS = ("ordinary", "saturated")


def gcase_id(c):
    return f"dh{c.dh}-H{c.H}-B{c.B}-T{c.T}-" + ("vec" if c.vec else "scalar")


def gate_params(c, block):
    """gru_rel_pos_linear (8, dh), its bias (8) and gru_rel_pos_const (1, H, 1, 1): constants that differ by head.  "saturated": weights
    that carry the pre-activations beyond +-90."""
    g = torch.Generator().manual_seed(4000 + c.dh * 17 + c.H)
    w = torch.randn(8, c.dh, generator=g) * (0.5 / c.dh ** 0.5)
    b = 0.3 * torch.randn(8, generator=g)
    if block == "saturated":
        w = w * 400.0
    const = 1.0 + 0.25 * torch.arange(c.H).float() + 0.1 * torch.randn(c.H, generator=g)
    return w, b, const.reshape(1, c.H, 1, 1)


def gate_input(c, block, dtype):
    g = torch.Generator().manual_seed(4100 + c.B * 1009 + c.T * 7 + c.dh)
    u = torch.randn(c.B * c.T, c.H * c.dh, generator=g)
    return u.to(dtype)


def fold_gate(w, b):
    """host.cpp gate_rowsum_fold in its order: fp32 sums of rows 0-3 and 4-7, from 0."""
    wab, bab = torch.zeros(2, w.shape[1]), torch.zeros(2)
    for j in range(8):
        wab[j // 4] = wab[j // 4] + w[j]
        bab[j // 4] = bab[j // 4] + b[j]
    return wab, bab


def gate_reference(c, w, b, const, u):
    """(ref, lim, s) in fp64: ref / lim (B, H, T); s (2, rows, H) the two pre-activations."""
    wab, bab = fold_gate(w, b)
    x = u.double().reshape(c.B * c.T, c.H, c.dh)
    s = torch.einsum("rhd,kd->krh", x, wab.double()) + bab.double()[:, None, None]
    sig = torch.einsum("rhd,kd->krh", x.abs(), wab.double().abs()) + bab.double().abs()[:, None, None]
    ds = (c.dh + 2) * U * sig
    ga, gb = torch.sigmoid(s[0]), torch.sigmoid(s[1])
    e_a, e_b = ds[0] / 4 + SIGMOID_ALLOW * ga, ds[1] / 4 + SIGMOID_ALLOW * gb
    cc = const.double().reshape(1, c.H)
    t = gb * cc - 1.0
    e_t = cc.abs() * e_b + U * ((gb * cc).abs() + t.abs())
    mm = ga * t
    e_m = t.abs() * e_a + ga * e_t + e_a * e_t + U * mm.abs()
    ref = mm + 2.0
    lim = e_m + U * ref.abs()
    to_bht = lambda x: x.reshape(c.B, c.T, c.H).permute(0, 2, 1).contiguous()   # noqa: E731
    return to_bht(ref), to_bht(lim), s


GMUTANTS = ("rows 0-3 and 4-7 swapped", "const of head h + 1", "const of head h - 1", "gate written as (B, T, H)", "bias once per lane")


def gate_simulate(c, w, b, const, u, order, mutant=None):
    """The kernels' fp32 arithmetic in NumPy: order "chain" = relpos_gate_kernel's FMA chain from the bias, "tree" = relpos_gate_vec_kernel's 8
    terms per lane, exchange steps, then the bias.  (NumPy has no fma: each product is rounded, which the limit's dh + 2 roundings cover.)"""
    m = GMUTANTS.index(mutant) if mutant else -1
    wab, bab = (t.numpy().astype(np.float32) for t in fold_gate(w, b))
    if m == 0:
        wab, bab = wab[::-1].copy(), bab[::-1].copy()
    x = u.float().numpy().reshape(c.B * c.T, c.H, c.dh)
    lph = c.dh // 8
    s = []
    for k in range(2):
        if order == "chain":
            acc = np.full(x.shape[:2], bab[k], dtype=np.float32)
            for d in range(c.dh):
                acc = acc + x[..., d] * wab[k, d]
        else:
            lanes = np.zeros(x.shape[:2] + (lph,), dtype=np.float32)
            for j in range(8):
                lanes = lanes + x.reshape(x.shape[:2] + (lph, 8))[..., j] * wab[k].reshape(lph, 8)[:, j]
            if m == 4:
                lanes = lanes + bab[k]
            o = lph // 2
            idx = np.arange(lph)
            while o:
                lanes = lanes + lanes[..., idx ^ o]
                o //= 2
            acc = lanes[..., 0] + (np.float32(0) if m == 4 else bab[k])
        s.append(acc)
    one = np.float32(1)
    with np.errstate(over="ignore"):
        ga, gb = one / (one + np.exp(-s[0])), one / (one + np.exp(-s[1]))
    cst = const.numpy().astype(np.float32).reshape(c.H)
    if m == 1:
        cst = np.roll(cst, -1)
    if m == 2:
        cst = np.roll(cst, 1)
    gate = ga * (gb * cst[None, :] - one) + np.float32(2)             # (rows, H)
    gate = torch.from_numpy(gate.astype(np.float32)).reshape(c.B, c.T, c.H)
    if m == 3:
        return gate.reshape(c.B, c.H, c.T).clone()                    # (B, T, H) bytes read as (B, H, T)
    return gate.permute(0, 2, 1).contiguous()


def gapplies(mutant, c):
    i = GMUTANTS.index(mutant)
    if i in (1, 2):
        return c.H >= 2
    if i == 3:
        return c.H >= 2 and c.T >= 2
    if i == 4:
        return c.vec and c.dh >= 16
    return True
