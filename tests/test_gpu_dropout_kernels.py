"""Every kernel of csrc/dropout.hip alone, through the C-ABI test hook svt_debug_dropout, against the numpy restatement of the mask
function in tests/dropout_cases.py.

The row kernels multiply by one fp32 constant or write +0, so every check of them is bit for bit: the tensor sits between poisoned guard
elements, the expected image is built on the host from the rule of include/svt_mi355.h, and the whole buffer, guards included, is
compared as integers.  The (hi, lo) form is compared the same way against its stated value rule: o = keep ? fl(fl(hi + lo) * scale) : +0,
hi' = T(o), lo' = T(fl(o - hi')).  The softmax form must reproduce the mask exactly (a probability is +0 iff its element is dropped) and
keep every kept probability inside the limit tests/gemm_limit.py states for the row softmax (tests/test_gpu_attention_scores.py):
relative error 2^-24 max_j |s_ij - m_i| + (T / 64 + 16) 2^-24 + u_P, plus 2^-24 for the one multiplication by float(1 / (1 - p)) where
p > 0 (exact at p = 0, where the limit is the plain kernel's), plus half the storage type's smallest subnormal as an absolute term.
Shapes are the smallest that can go wrong: widths around the 4-element Philox group and the 8-element 16-byte piece, element counts that leave a partial last wave, a partial last piece and more than one
workgroup, first logical indices e0 that are no multiple of 4 and that carry into the high counter word.  Both builds of the library run
(bf16 and IEEE-half operands).
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from svt_speechbrain_amd import _lib  # noqa: E402
import dropout_cases as DC  # noqa: E402

DEV = "cuda:0"
GUARD = 8            # guard elements in front of and behind a tensor: the body stays 16-byte aligned
INVALID = -1
SEED = 0x0123456789ABCDEF
WIDTHS = (1, 3, 4, 5, 7, 8, 9, 64)
ROWS = (1, 5, 37, 261)     # 261 * 3 = 783 elements: three waves and a bit of 4-element pieces; 261 * 64: seventeen workgroups
E0S = (0, 2 ** 32 - 2, 2 ** 34 + 1)
RATES = (0.0, 0.1, 0.5)
# build -> (library variant, operand type, its unit roundoff u, half its smallest subnormal: the absolute error of a rounding below the normal range)
BUILDS = {"bf16": (None, torch.bfloat16, 2.0 ** -8, 2.0 ** -134), "f16": ("f16", torch.float16, 2.0 ** -11, 2.0 ** -25)}


def ints(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def poison(n, dtype):
    t = torch.empty(n, dtype=dtype)
    ints(t).fill_(0x7FC0DEAD if dtype == torch.float32 else 0x7FC1)   # NaNs with a payload
    return t


def values(n, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g) * 3
    if n > 3:
        x[0], x[1], x[2] = -0.0, 1e-30, -65000.0    # a negative zero (must become +0 when dropped), a tiny and a large value
    return x.to(dtype)


def call(lib, **kw):
    d = _lib.DropoutDescC()
    d.struct_size = C.sizeof(_lib.DropoutDescC)
    for k, v in kw.items():
        setattr(d, k, v)
    rc = lib.svt_debug_dropout(C.byref(d), 0, _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    return rc


def rows_case(lib, dtype, n, e0, p, step, site, layer, shift=0):
    """One form-0 launch on n elements (shift: elements the body starts past a 16-byte boundary).  Returns (got, want) as integers."""
    host = poison(n + 2 * GUARD + shift, dtype)
    body = slice(GUARD + shift, GUARD + shift + n)
    host[body] = values(n, dtype, n + step)
    want = host.clone()
    k = torch.from_numpy(DC.keep(p, SEED, step, site, layer, n, e0))
    prod = (host[body].float() * torch.tensor(float(DC.scale(p)))).to(dtype)       # one fp32 product, one rounding to the storage type
    want[body] = torch.where(k, prod, torch.zeros((), dtype=dtype))
    buf = host.to(DEV)
    rc = call(lib, form=0, prec=0 if dtype == torch.float32 else 1, site=site, layer=layer, step=step, p=p, seed=SEED, e0=e0, n=n,
              x=_lib.ptr(buf) + (GUARD + shift) * buf.element_size())
    assert rc == 0, _lib.last_error(lib)
    return ints(buf.cpu()), ints(want)


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("kind", ["fp32", "op16"])
def test_row_dropout_bit_for_bit(build, kind):
    variant, op = BUILDS[build][:2]
    lib = _lib.load(variant)
    dtype = torch.float32 if kind == "fp32" else op
    base = 1 if kind == "fp32" else 2
    step = 0
    for W in WIDTHS:
        for rows in ROWS:
            for e0 in E0S:
                for p in RATES:
                    step += 1
                    got, want = rows_case(lib, dtype, rows * W, e0, p, step, site=step % 6, layer=step % 3)
                    assert torch.equal(got, want), (W, rows, e0, p, int((got != want).sum()))
                    assert lib.svt_debug_set(44, 0) == base + (0 if e0 % 4 == 0 else 10)
    # a body that starts past a 16-byte boundary takes the element-by-element instantiation and gives the same image
    got, want = rows_case(lib, dtype, 777, 0, 0.5, 1, 3, 1, shift=1)
    assert torch.equal(got, want) and lib.svt_debug_set(44, 0) == base + 10
    # p = 0 changes no bit of a finite value; the rate just below 2^-32 has threshold 0 as well
    for p in (0.0, float(np.nextafter(2.0 ** -32, 0.0))):
        got, want = rows_case(lib, dtype, 333, 0, p, 2, 0, 0)
        host = poison(333 + 2 * GUARD, dtype)
        host[GUARD:GUARD + 333] = values(333, dtype, 333 + 2)
        assert torch.equal(got, want) and torch.equal(got, ints(host))
    # the largest rate a float32 scale serves: about one element in 2^24 survives, scaled by 2^24
    got, want = rows_case(lib, dtype, 4096, 0, 1 - 2.0 ** -24, 4, 5, 2)
    assert torch.equal(got, want)


def test_row_dropout_past_the_grid_cap():
    """More 16-byte pieces than 16 384 workgroups of 256 threads hold: some threads take a second piece."""
    lib = _lib.load()
    n = 16384 * 256 * 4 + 4 * 300 + 3
    got, want = rows_case(lib, torch.float32, n, 0, 0.1, 7, 4, 1)
    assert torch.equal(got, want)
    k = DC.keep(0.1, SEED, 7, 4, 1, n)
    assert abs(1 - k.mean() - 0.1) < 5 * (0.09 / n) ** 0.5


@pytest.mark.parametrize("build", list(BUILDS))
def test_hilo_dropout_against_its_value_rule(build):
    variant, op = BUILDS[build][:2]
    lib = _lib.load(variant)
    step = 100
    for W, rows in ((1, 1), (3, 5), (5, 37), (7, 261), (8, 37), (9, 5), (64, 261), (768, 3)):
        for e0 in E0S:
            for p in RATES:
                step += 1
                n = W * rows
                hi = poison(n + 2 * GUARD, op)
                lo = poison(n + 2 * GUARD, op)
                body = slice(GUARD, GUARD + n)
                v = values(n, torch.float32, n + step)
                hi[body] = v.to(op)
                lo[body] = (v - hi[body].float()).to(op)        # a stream as layernorm_hilo_kernel leaves it
                wh, wl = hi.clone(), lo.clone()
                k = torch.from_numpy(DC.keep(p, SEED, step, 1, 0, n, e0))
                val = hi[body].float() + lo[body].float()
                o = torch.where(k, val * torch.tensor(float(DC.scale(p))), torch.zeros(()))
                wh[body] = o.to(op)
                wl[body] = (o - wh[body].float()).to(op)
                dh, dl = hi.to(DEV), lo.to(DEV)
                rc = call(lib, form=1, prec=1, site=1, layer=0, step=step, p=p, seed=SEED, e0=e0, n=n,
                          xh=_lib.ptr(dh) + GUARD * 2, xl=_lib.ptr(dl) + GUARD * 2)
                assert rc == 0, _lib.last_error(lib)
                assert torch.equal(ints(dh.cpu()), ints(wh)) and torch.equal(ints(dl.cpu()), ints(wl)), (W, rows, e0, p)
                assert lib.svt_debug_set(44, 0) == 3 + (0 if e0 % 4 == 0 else 10)


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("kind", ["fp32", "op16"])
def test_softmax_dropout(build, kind):
    variant, op, u16, eta16 = BUILDS[build]
    lib = _lib.load(variant)
    dtype, uP, eta = (torch.float32, 0.0, 2.0 ** -150) if kind == "fp32" else (op, u16, eta16)
    rows = 13      # four rows per workgroup: three full workgroups and one row
    step = 200
    for T in (1, 7, 8, 9, 65):
        Tp = (T + 7) // 8 * 8
        for e0 in E0S:
            for p in RATES:
                step += 1
                g = torch.Generator().manual_seed(step)
                S = poison((rows + 2) * Tp, torch.float32).view(rows + 2, Tp)      # a guard row on each side, poisoned pad columns
                S[1:rows + 1, :T] = torch.randn(rows, T, generator=g) * 1.5
                Pb = poison((rows + 2) * Tp, dtype).view(rows + 2, Tp)
                Sd, Pd = S.to(DEV), Pb.to(DEV)
                rc = call(lib, form=2, prec=0 if kind == "fp32" else 1, site=2, layer=1, step=step, p=p, seed=SEED, e0=e0, rows=rows, T=T,
                          Tp=Tp, S=_lib.ptr(Sd) + Tp * 4, P=_lib.ptr(Pd) + Tp * Pd.element_size())
                assert rc == 0, _lib.last_error(lib)
                assert lib.svt_debug_set(44, 0) == (4 if kind == "fp32" else 5)
                got = Pd.cpu()
                assert torch.equal(ints(Sd.cpu()), ints(S))                                             # S is read only
                assert torch.equal(ints(got[0]), ints(Pb[0])) and torch.equal(ints(got[-1]), ints(Pb[-1]))   # the guard rows
                assert not ints(got[1:rows + 1, T:]).any()                                              # pad columns: zero, as the plain kernel leaves them
                k = torch.from_numpy(DC.keep(p, SEED, step, 2, 1, rows * T, e0).reshape(rows, T))
                body = got[1:rows + 1, :T]
                s64 = S[1:rows + 1, :T].double()
                ref = torch.softmax(s64, -1)
                assert float(ref.min()) > 2.0 ** -20      # (the inputs: no probability so small that its storage type rounds it to zero)
                assert torch.equal(ints(body.contiguous()) == 0, ~k), (T, e0, p)                         # the mask, exactly (dropped: +0)
                spread = (s64 - s64.max(-1, keepdim=True).values).abs().max(-1, keepdim=True).values
                rel = 2.0 ** -24 * spread + (T / 64 + 16) * 2.0 ** -24 + uP + (2.0 ** -24 if p > 0 else 0.0)
                want = ref * float(DC.scale(p))
                err = ((body.double() - want).abs() / (rel * want + eta))[k]
                print(f"softmax dropout {build} {kind} T={T} e0={e0} p={p}: worst err / limit {float(err.max()) if err.numel() else 0:.3f}")
                assert err.numel() == 0 or float(err.max()) <= 1.0, (T, e0, p, float(err.max()))


def test_refusals():
    lib = _lib.load()
    buf = torch.zeros(64, device=DEV)
    ok = dict(form=0, prec=0, site=0, layer=0, step=0, p=0.1, seed=1, e0=0, n=64, x=_lib.ptr(buf))
    for over, text in ((dict(p=1.0), "p must lie"), (dict(p=-0.1), "p must lie"), (dict(form=3), "form"), (dict(n=0), "n must"),
                       (dict(x=None), "null x"), (dict(site=256), "site"), (dict(prec=2), "prec"),
                       (dict(form=1), "null xh"), (dict(form=2), "form 2 needs")):
        assert call(lib, **dict(ok, **over)) == INVALID and text in _lib.last_error(lib), (over, _lib.last_error(lib))
    d = _lib.DropoutDescC()
    assert lib.svt_debug_dropout(C.byref(d), 0, _lib.stream_ptr(DEV)) == INVALID and "struct_size" in _lib.last_error(lib)
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0
