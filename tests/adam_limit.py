"""What tests/test_adam_limit.py (CPU) and tests/test_gpu_adam.py (GPU) share: the fp64 formula of one clip + Adam step, the per-element
limits a correct fp32 evaluation in the kernel's order stays inside, a numpy fp32 restatement of that order with its mutants, and the seeded
inputs.

The step (torch/optim/adam.py ``_single_tensor_adam``; csrc/adam.hip states the same order), for one element with clip coefficient c,
sign s = -1 with maximize, w = 1 - beta1, step size ss = lr / (1 - beta1^k) and b = sqrt(1 - beta2^k) at the tensor's step k:

    G = c g (stored)      g' = s G [+ wd p, coupled]      p0 = p [(1 - lr wd), decoupled]
    m' = m + w (g' - m)   v' = beta2 v + (1 - beta2) g'^2   x' = max(x, v') [amsgrad]
    D = sqrt(v' or x') / b + eps                            p' = p0 - ss m' / D

The limits are bounds, not fitted tolerances: u = 2^-24 (half an ulp, relative) times the magnitudes that enter the element, one u per
fp32 rounding of the order above, errors carried forward to first order.  Every scalar (w, beta2, 1 - beta2, wd, 1 - lr wd, eps, ss, b) is
a double rounded ONCE to fp32 (1 u of its term).  The terms of two roundings multiplied (<= 2^-46 relative) are covered by counting the
final rounding of each array against the magnitude SUM (M_m, M_v, |p| + ss M_m / D) instead of the result, and 2^-149 is half the
spacing of fp32's subnormals.

  clip     the kernel's coefficient is min(max_norm / (total + 1e-6), 1) from fp32 per-tensor norms: 5 u (norms 1, sqrt of their sum 1,
           the addition 1, max_norm's rounding 1, the division 1), and the product g * coef 1 more:   E_G = 6 u |G|      (0 without clip)
  g'       coupled decay is one fma(p, wd, s G): wd's rounding u |wd p|, the fma's u M_g, M_g = |G| + |wd p|:
           E_g = E_G + u (|wd p| + M_g)                                                             (E_g = E_G without it)
  m'       d = g' - m: E_g + u (M_g + |m|); fma(w, d, m): w's rounding u w (M_g + |m|) and the result's u M_m, M_m = |m| + w (M_g + |m|):
           E_m = w E_g + 2 u w (M_g + |m|) + u M_m
           (w >= 0.5, torch's other lerp branch g' - d (1 - w), 1 - w formed in fp32: E_g + (1 - w) (E_g + u (M_g + |m|)) + 3 u (1 - w) (M_g + |m|)
            + u (M_g + (1 - w) (M_g + |m|)))
  v'       v beta2: 2 u beta2 v; ((1 - beta2) g') g': (1 - beta2) (3 u M_g^2 + 2 M_g E_g); the sum: u M_v, M_v = beta2 v + (1 - beta2) M_g^2:
           E_v = 2 u beta2 v + (1 - beta2) (3 u M_g^2 + 2 M_g E_g) + u M_v
  x'       max is 1-Lipschitz:  E_x = E_v
  p'       r = v' or x' with error E_r; |sqrt(a) - sqrt(r)| <= |a - r| / sqrt(r), the root's rounding u sqrt(r); / b: b's rounding and the
           quotient's, 2 u sqrt(r) / b; + eps: u eps and u D:       E_D = E_r / (sqrt(r) b) + 3 u sqrt(r) / b + u eps + u D
           -ss m': 2 u ss M_m + ss E_m; / D: u ss M_m / D and ss M_m E_D / D^2; p0: 2 u |p| when decoupled; the sum: u (|p| + ss M_m / D):
           E_p = [2 u |p|] + (ss E_m + 3 u ss M_m) / D + ss M_m E_D / D^2 + u (|p| + ss M_m / D)
"""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149
CHUNK = 4096          # csrc/common.h kAdaChunk
MUTANTS = ("no_bias_correction", "bc2_without_sqrt", "eps_inside_sqrt", "clip_stored_only", "decay_form_swapped", "amsgrad_max_before",
           "skip_last_of_chunk", "first_step_size")
STEPS = (1, 2, 10, 1000)
# the GPU tests' lists (elements per tensor)
NUMELS = (0, 1, 3, 4, 5, 255, 256, 257, 1023, 4099, CHUNK + 1)
MID_LIST = (257, 1023, 5, CHUNK + 1, 64)   # the list every flag combination runs on


def hyper(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, maximize=False, decoupled=False):
    return dict(lr=float(lr), beta1=float(betas[0]), beta2=float(betas[1]), eps=float(eps), wd=float(weight_decay), amsgrad=bool(amsgrad),
                maximize=bool(maximize), decoupled=bool(decoupled))


def flag_cases():
    """Every combination of clip on / off, weight decay 0 / 0.01 coupled / 0.01 decoupled, amsgrad and maximize: (clip, hyper)."""
    out = []
    for clip in (False, True):
        for wd, dec in ((0.0, False), (0.01, False), (0.01, True)):
            for ams in (False, True):
                for mx in (False, True):
                    out.append((clip, hyper(weight_decay=wd, decoupled=dec, amsgrad=ams, maximize=mx)))
    return out


def bias(step, h):
    """(lr / bias_correction1, sqrt(bias_correction2)) as torch's single-tensor path forms them: Python doubles."""
    step = float(step)
    return h["lr"] / (1 - h["beta1"] ** step), (1 - h["beta2"] ** step) ** 0.5


def tensor_inputs(n, seed, step):
    """One tensor's five fp32 arrays: |g| log-uniform in [1e-3, 1] with random signs (not near 0, where m / (sqrt(v) + eps) magnifies a
    rounding), p ~ N(0, 0.5); before the first step the state is zero, later m ~ U(-0.5, 0.5), v log-uniform in [1e-8, 1] (small v is
    where an eps in the wrong place shows) and x = v * U(0.5, 2) so that amsgrad's max takes either side."""
    r = np.random.default_rng(seed)
    g = (10.0 ** r.uniform(-3, 0, n) * r.choice([-1.0, 1.0], n)).astype(np.float32)
    p = (0.5 * r.standard_normal(n)).astype(np.float32)
    if step == 1:
        m, v, x = (np.zeros(n, np.float32) for _ in range(3))
    else:
        m = r.uniform(-0.5, 0.5, n).astype(np.float32)
        v = (10.0 ** r.uniform(-8, 0, n)).astype(np.float32)
        x = (v * r.uniform(0.5, 2.0, n)).astype(np.float32)
    return dict(p=p, g=g, m=m, v=v, x=x)


def list_inputs(numels, seed, steps):
    """A list of tensors; ``steps`` one step for all or one per tensor."""
    steps = [steps] * len(numels) if np.isscalar(steps) else list(steps)
    return [tensor_inputs(n, seed * 1000 + i, k) for i, (n, k) in enumerate(zip(numels, steps))], steps


def clip_coef64(tensors, max_norm):
    """clip_grad_norm_ in fp64: (total norm, coefficient)."""
    total = float(np.sqrt(sum(float(np.sum(t["g"].astype(np.float64) ** 2)) for t in tensors)))
    return total, min(max_norm / (total + 1e-6), 1.0)


def clip_coef32(tensors, max_norm):
    """The kernel's fp32 path: per-tensor norms rounded to fp32, the total rounded to fp32, the coefficient in fp32."""
    norms = [np.float32(np.sqrt(np.sum(t["g"].astype(np.float64) ** 2))) for t in tensors]
    total = np.float32(np.sqrt(sum(float(x) * float(x) for x in norms)))
    return total, coef_from_total(total, max_norm)


def coef_from_total(total, max_norm):
    c = np.float32(max_norm) / (np.float32(total) + np.float32(1e-6))
    return np.float32(min(c, np.float32(1.0)))


def formula(t, step, h, coef=1.0):
    """The fp64 step of one tensor: {"g" (stored), "m", "v", "x", "p"} and the magnitudes the limits need."""
    p, g, m, v, x = (t[k].astype(np.float64) for k in ("p", "g", "m", "v", "x"))
    ss, b = bias(step, h)
    w = 1 - h["beta1"]
    G = coef * g
    gu = -G if h["maximize"] else G
    coupled = h["wd"] != 0 and not h["decoupled"]
    p0 = p * (1 - h["lr"] * h["wd"]) if (h["wd"] != 0 and h["decoupled"]) else p
    if coupled:
        gu = gu + h["wd"] * p
    m1 = m + w * (gu - m)
    v1 = h["beta2"] * v + (1 - h["beta2"]) * gu * gu
    x1 = np.maximum(x, v1)
    r = x1 if h["amsgrad"] else v1
    D = np.sqrt(r) / b + h["eps"]
    p1 = p0 - ss * m1 / D
    Mg = np.abs(G) + (np.abs(h["wd"] * p) if coupled else 0.0)
    return dict(g=G, m=m1, v=v1, x=x1, p=p1, Mg=Mg, r=r, D=D, ss=ss, b=b, w=w, coupled=coupled, absG=np.abs(G), absm=np.abs(m), v0=v,
                absp=np.abs(p))


def limits(t, step, h, coef=1.0, clip=False):
    """Per-element limits {"g", "m", "v", "x", "p"} of one tensor (the derivation is this module's docstring)."""
    f = formula(t, step, h, coef)
    w, ss, b, Mg, D, r = f["w"], f["ss"], f["b"], f["Mg"], f["D"], f["r"]
    beta2, eps = h["beta2"], h["eps"]
    E_G = 6 * U * f["absG"] if clip else 0.0 * f["absG"]
    E_g = E_G + (U * (np.abs(h["wd"]) * f["absp"] + Mg) if f["coupled"] else 0.0)
    span = Mg + f["absm"]
    if w < 0.5:
        M_m = f["absm"] + w * span
        E_m = w * E_g + 2 * U * w * span + U * M_m
    else:
        M_m = Mg + (1 - w) * span
        E_m = E_g + (1 - w) * (E_g + U * span) + 3 * U * (1 - w) * span + U * M_m
    M_v = beta2 * f["v0"] + (1 - beta2) * Mg * Mg
    E_v = 2 * U * beta2 * f["v0"] + (1 - beta2) * (3 * U * Mg * Mg + 2 * Mg * E_g) + U * M_v
    root = np.sqrt(r)
    with np.errstate(divide="ignore", invalid="ignore"):
        E_root = np.where(r > 0, E_v / np.where(r > 0, root, 1.0), np.sqrt(E_v))
    E_D = E_root / b + 3 * U * root / b + U * eps + U * D
    E_p0 = 2 * U * f["absp"] if (h["wd"] != 0 and h["decoupled"]) else 0.0
    E_p = E_p0 + (ss * E_m + 3 * U * ss * M_m) / D + ss * M_m * E_D / (D * D) + U * (f["absp"] + ss * M_m / D)
    return dict(g=E_G + TINY, m=E_m + TINY, v=E_v + TINY, x=E_v + TINY, p=E_p + TINY)


def _f32(x):
    return np.asarray(x, dtype=np.float32)


def _fma(a, b, c):
    """fma on fp32 arrays: the product of two fp32 numbers is exact in fp64."""
    return (a.astype(np.float64) * np.asarray(b, dtype=np.float64) + c.astype(np.float64)).astype(np.float32)


def restate_fp32(t, step, h, coef32=None, mutant=None, ss_step=None):
    """The kernel's order in numpy fp32, one rounding per operation (csrc/adam.hip adam_element), or a mutant of it.  ``coef32``: the fp32
    clip coefficient, None without clip.  ``ss_step``: the step the step size is taken from (mutant first_step_size passes the first tensor's)."""
    assert mutant is None or mutant in MUTANTS
    p, g, m, v, x = (t[k].copy() for k in ("p", "g", "m", "v", "x"))
    dec, wd = h["decoupled"], h["wd"]
    if mutant == "decay_form_swapped":
        dec = not dec
    ss, b = bias(step, h)
    if ss_step is not None:
        ss = bias(ss_step, h)[0]
    if mutant == "no_bias_correction":
        ss, b = h["lr"], 1.0
    if mutant == "bc2_without_sqrt":
        b = b * b
    neg_ss, b32, eps32 = np.float32(-np.float32(ss)), np.float32(b), np.float32(h["eps"])
    w1 = np.float32(1.0 - h["beta1"])
    beta2, omb2 = np.float32(h["beta2"]), np.float32(1.0 - h["beta2"])
    g_st = g * np.float32(coef32) if coef32 is not None else g
    gu = g if mutant == "clip_stored_only" else g_st
    gu = -gu if h["maximize"] else gu
    p0 = p
    if wd != 0:
        if dec:
            p0 = p * np.float32(1.0 - h["lr"] * wd)
        else:
            gu = _fma(p, np.float32(wd), gu)
    d = gu - m
    if w1 >= np.float32(0.5):
        m1 = gu - d * (np.float32(1.0) - w1)
    else:
        m1 = _fma(d, w1, m)
    v1 = v * beta2 + (omb2 * gu) * gu
    x1 = np.maximum(x, v if mutant == "amsgrad_max_before" else v1)
    r = x1 if h["amsgrad"] else v1
    if mutant == "eps_inside_sqrt":
        D = np.sqrt(r + eps32) / b32
    else:
        D = np.sqrt(r) / b32 + eps32
    p1 = p0 + (neg_ss * m1) / D
    out = dict(g=_f32(g_st), m=_f32(m1), v=_f32(v1), x=_f32(x1) if h["amsgrad"] else x.copy(), p=_f32(p1))
    if mutant == "skip_last_of_chunk" and p.size:
        last = [i for i in range(CHUNK - 1, p.size, CHUNK)] + [p.size - 1]
        for k in ("g", "m", "v", "x", "p"):
            out[k][last] = t[k][last]
    for k in out:
        assert out[k].dtype == np.float32
    return out


def worst(got, t, step, h, coef=1.0, clip=False):
    """{"g", "m", "v", "x", "p"}: the largest |got - formula| / limit of one tensor (0 for an empty one); a NaN or an infinity counts as
    infinite.  Without amsgrad "x" is held to stay what it was."""
    f, lim = formula(t, step, h, coef), limits(t, step, h, coef, clip)
    out = {}
    for k in ("g", "m", "v", "x", "p"):
        ref = f[k] if (k != "x" or h["amsgrad"]) else t["x"].astype(np.float64)
        if ref.size == 0:
            out[k] = 0.0
            continue
        r = np.abs(np.asarray(got[k], dtype=np.float64) - ref) / lim[k]
        out[k] = float(np.max(np.where(np.isfinite(r), r, np.inf)))
    return out
