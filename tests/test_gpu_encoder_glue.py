"""GPU: the glue of the transformer encoder ALONE -- one step of a finalized handle on the test's own buffers through the C-ABI hook
svt_debug_encoder_step, with the handle's own uploaded weights (weight-norm fold, tap-major relayout, multi-frame weight image, BatchNorm
fold, gate row-sum fold are inside the tested unit) -- against the fp64 references and the derived limits of tests/posconv_limit.py: the
three forms of the positional conv in every mode that reaches them, WavLM's relative-position table entry by entry against HF's CPU formula,
and the two gate kernels.  The kernel ids of svt_debug_set keys 45 and 39 are asserted in every case.  tests/test_posconv_limit.py proves on
the CPU, for these very inputs, that a correct step stays inside the limits and that the mutants do not.

Every encoder is a tiny features-in one (num_conv_layers = 0: n_samples = T) with seeded weights and 0 or 1 layers.  Each case prints its
worst err / limit and where it sits."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_limit as G  # noqa: E402
import posconv_limit as P  # noqa: E402
from svt_speechbrain_amd import _lib  # noqa: E402
from svt_speechbrain_amd import weights as W  # noqa: E402
from svt_speechbrain_amd.config import EncoderConfig  # noqa: E402
from svt_speechbrain_amd.huggingface_interface import _config_to_c  # noqa: E402

DEV = "cuda:0"
SVT_ERR_INVALID = -1
GUARD = 4096   # bytes of 0xA5 behind the workspace: the step must not write past svt_encoder_workspace_bytes

# svt_debug_set key 45 after step 1: 1000 * form + 100 * gather kernel + 10 * scatter kernel (include/svt_mi355.h)
GLUE_ID = {("plain", "fp32"): 1100, ("plain", "16"): 1300, ("plain", "x3"): 1100, ("multi", "16"): 2320, ("multi", "x3"): 2110,
           ("stack", "fp32"): 3100, ("stack", "16"): 3300}


def gemm_id(c, mode):
    """... and key 39, the product's kernel as the dispatcher chooses it for these launches (csrc/gemm_dispatch.hip): 2256 / 12256 the
    register-staged kernel's 256 x 64 tiles (N = cg <= 64) in its exact-fp32 / split instantiation -- the plain form's weight is not
    registered as split --, 7256 gemm_x3s_kernel's batched arm, 1032 the small-problem kernel with 32 x 32 tiles, which every 16-bit launch
    here is small enough for, unless K is no multiple of 64 (the stack: 19 * 16) or N no multiple of 16 (cg = 24)."""
    form, kind = P.form_of(c, mode), _kind(mode)
    if kind == "fp32":
        return 2256
    if kind == "x3":
        return 7256 if form == "multi" else 12256
    return 2256 if (form == "stack" or c.cg % 16) else 1032


def _kind(mode):
    return "fp32" if mode == "fp32" else "16" if mode in P.SIXTEEN else "x3"


def _base_cfg(**kw):
    return EncoderConfig(name="glue", conv_dim=(8,), conv_kernel=(), conv_stride=(), feat_proj_layer_norm=False, intermediate_size=8, **kw)


def _make_handle(lib, cfg, precision_name, overrides, finalize=True):
    """A finalized encoder handle of `cfg` with seeded weights, `overrides` (HF key -> tensor) on top."""
    sd = W.seeded_encoder_state_dict(cfg, seed=77)
    for k, v in overrides.items():
        assert k in sd and sd[k].shape == v.shape, (k, v.shape)
        sd[k] = v
    h = ctypes.c_void_p()
    cc = _config_to_c(cfg, False, False, precision_name)
    _lib.check(lib.svt_encoder_create(ctypes.byref(cc), 0, ctypes.byref(h)), "svt_encoder_create", lib)
    for name, p in sd.items():
        if not p.is_floating_point():
            continue
        t = p.detach().to(torch.float32).contiguous()
        shape = (ctypes.c_int64 * t.dim())(*t.shape)
        _lib.check(lib.svt_encoder_load_param(h, name.encode(), ctypes.c_void_p(t.data_ptr()), 0, shape, t.dim()), f"load_param({name})", lib)
    if finalize:
        _lib.check(lib.svt_encoder_finalize(h), "svt_encoder_finalize", lib)
    return h


@functools.lru_cache(maxsize=None)
def _posconv_handle(key, mode):
    cg, Gr, kp, bn, depth = key
    c = P.PCase("", cg, Gr, kp, 1, 1, bn, depth, (), "")
    lib = _lib.load(P.MODE[mode][0])
    cfg = _base_cfg(family="data2vec" if depth > 1 else "hubert", hidden_size=cg * Gr, num_hidden_layers=0, num_attention_heads=1,
                    num_conv_pos_embeddings=kp, num_conv_pos_embedding_groups=Gr, pos_conv_depth=depth, conv_pos_batch_norm=bn)
    return lib, _make_handle(lib, cfg, P.MODE[mode][1], P.make_params(c))


def _step(lib, handle, **fields):
    """One svt_debug_encoder_step call.  Returns (rc, key-45 id, key-39 id)."""
    d = _lib.EncoderStepDescC()
    d.struct_size = ctypes.sizeof(d)
    for k, v in fields.items():
        setattr(d, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    torch.cuda.synchronize()
    rc = lib.svt_debug_encoder_step(handle, ctypes.byref(d), torch.cuda.current_stream().cuda_stream)
    return rc, lib.svt_debug_set(45, 0), lib.svt_debug_set(39, 0)


def _run_posconv(c, mode, h):
    """The step on h (B, T, D): (output on the CPU, key-45 id, key-39 id)."""
    lib, handle = _posconv_handle(P.geometry_key(c), mode)
    need = lib.svt_encoder_workspace_bytes(handle, c.B, c.T)
    assert need > 0, _lib.last_error(lib)
    ws = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    x = h.to(DEV)
    out = torch.full_like(x, float("nan"))
    rc, glue, gemm = _step(lib, handle, step=1, B=c.B, T=c.T, n_samples=c.T, x=x, out=out, workspace=ws, workspace_bytes=need)
    _lib.check(rc, "svt_debug_encoder_step", lib)
    assert bool((ws[need:] == 0xA5).all()), "the step wrote behind svt_encoder_workspace_bytes"
    return out.cpu(), glue, gemm


def _gelu_form(gemm_id, mode):
    """The GELU the product kernel that ran calls (tests/gemm_limit.py gelu_form), for the limit of a 16-bit mode."""
    if mode not in P.SIXTEEN:
        return "fast"
    multi16 = G.C(gemm_id, 1, 1, 64, act=1, out_f32=0)
    return G.gelu_form(multi16)


def _check_posconv(c, mode):
    params, h = P.make_params(c), P.make_h(c)
    got, glue, gemm = _run_posconv(c, mode, h)
    form = P.form_of(c, mode)
    # the plain form's product writes fp32 with the residual in its epilogue: gelu_erf in every family that serves it
    gform = _gelu_form(gemm, mode) if form == "multi" else "fast"
    _, _, ref, lim = P.case_data(c, mode, gform)
    w, where = P.worst(got, ref, lim)
    print(f"encoder-glue posconv {P.pcase_id(c)} [{mode}]: form {form}, key 45 = {glue}, key 39 = {gemm}, worst err / limit {w:.4f} at {where}")
    assert glue == GLUE_ID[(form, _kind(mode))], (glue, form, mode)
    assert gemm == gemm_id(c, mode), (gemm, gemm_id(c, mode))
    assert torch.isfinite(got).all(), "a frame of the output is not finite: the step read workspace it had not written"
    assert w <= 1.0, (w, where)
    return got, ref, lim, gemm


_POS_RUNS = [(c, m) for c, m in P.RUNS if c.tag != "switch"]


@pytest.mark.parametrize("c,mode", _POS_RUNS, ids=[f"{P.pcase_id(c)}-{m}" for c, m in _POS_RUNS])
def test_positional_conv(c, mode):
    assert P.form_of(c, mode) == c.form
    _check_posconv(c, mode)


@pytest.mark.parametrize("mode", P.SIXTEEN + P.SPLIT)
def test_the_two_forms_agree_across_the_switch(mode):
    """127 GEMM rows run the plain form, 128 the multi-frame one; on the frames whose windows the two clips share they differ by no more than
    the sum of their limits."""
    lo, hi = sorted((c for c in P.PCASES if c.tag == "switch"), key=lambda c: c.T)
    assert (P.form_of(lo, mode), P.form_of(hi, mode)) == ("plain", "multi")
    got_lo, ref_lo, lim_lo, _ = _check_posconv(lo, mode)
    got_hi, ref_hi, lim_hi, _ = _check_posconv(hi, mode)
    n = lo.T - (lo.kp - 1 - lo.kp // 2)   # frames whose window ends inside the shorter clip
    assert torch.equal(P.make_h(lo)[:, :n], P.make_h(hi)[:, :n]) and torch.allclose(ref_lo[:, :n], ref_hi[:, :n], rtol=0, atol=1e-12)
    r = ((got_lo[:, :n].double() - got_hi[:, :n].double()).abs() / (lim_lo[:, :n] + lim_hi[:, :n])).max().item()
    print(f"encoder-glue switch [{mode}]: plain against multi-frame on {n} shared frames, worst difference / (sum of the limits) {r:.4f}")
    assert r <= 1.0


def test_geometries_the_issue_names_but_no_handle_can_have():
    """Channels per group and a head size must be multiples of 8 (validate_cfg): cg = 12 -- the only way to the element-by-element 16-bit
    gather, key-45 id 12 -- and a head size of 12 are refused when the handle is created."""
    lib = _lib.load()
    for kw in (dict(hidden_size=24, num_attention_heads=1, num_conv_pos_embedding_groups=2), dict(hidden_size=24, num_attention_heads=2, num_conv_pos_embedding_groups=1)):
        cfg = _base_cfg(family="hubert", num_hidden_layers=0, num_conv_pos_embeddings=16, **kw)
        h = ctypes.c_void_p()
        cc = _config_to_c(cfg, False, False, "bf16")
        assert lib.svt_encoder_create(ctypes.byref(cc), 0, ctypes.byref(h)) == SVT_ERR_INVALID, kw


# ---------------------------------------------------------------------------------------------------------------------------------
# the relative-position table
@functools.lru_cache(maxsize=None)
def _table_handle(nb, md, H=2):
    lib = _lib.load()
    cfg = _base_cfg(family="wavlm", hidden_size=8 * H, num_hidden_layers=1, num_attention_heads=H, num_conv_pos_embeddings=3,
                    num_conv_pos_embedding_groups=1, rel_pos_buckets=nb, rel_pos_max_distance=md)
    embed = (torch.arange(nb)[:, None] * H + torch.arange(H)[None, :]).float()
    return lib, _make_handle(lib, cfg, "fp32", {"encoder.layers.0.attention.rel_attn_embed.weight": embed})


@pytest.mark.parametrize("nb,md", P.CONFIGS, ids=[f"buckets{nb}-max{md}" for nb, md in P.CONFIGS])
def test_relative_position_table_equals_hf(nb, md):
    """rel_attn_embed[bucket][h] = bucket H + h reads the bucket back exactly: every entry is HF's CPU bucket, at the edge distances too."""
    H = 2
    lib, handle = _table_handle(nb, md)
    for T in P.TABLE_T(nb // 4):
        pb = torch.full((H * (2 * T - 1) + 64,), float("nan"), device=DEV)
        rc, glue, _ = _step(lib, handle, step=2, B=1, T=T, out=pb)
        _lib.check(rc, "svt_debug_encoder_step", lib)
        assert glue == 30
        got = pb.cpu()
        assert torch.isnan(got[H * (2 * T - 1):]).all(), "the table kernel wrote behind (H, 2 T - 1)"
        got = got[:H * (2 * T - 1)].reshape(H, 2 * T - 1)
        ref = P.table_reference(H, T, nb, md)
        bad = (got != ref).nonzero()
        d_bad = sorted({int(i[1]) - (T - 1) for i in bad})
        print(f"encoder-glue table buckets {nb} max {md} T {T}: {len(bad)} of {ref.numel()} entries differ from HF" +
              (f", at key - query = {d_bad[:8]} (edge distances {P.edges(nb, md)})" if len(bad) else ""))
        assert len(bad) == 0, (d_bad[:8], got[tuple(bad[0])].item(), ref[tuple(bad[0])].item())


# ---------------------------------------------------------------------------------------------------------------------------------
# the gate
GATE_RUNS = ((None, "fp32", torch.float32), (None, "bf16", torch.bfloat16), ("f16", "fp32", torch.float32), ("f16", "fp16", torch.float16))
GROWS = 8   # NaN rows in front of and behind u


@functools.lru_cache(maxsize=None)
def _gate_handle(dh, H, block, variant, precision_name):
    lib = _lib.load(variant)
    c = P.GCase(dh, H, 1, 1, True)
    w, b, const = P.gate_params(c, block)
    cfg = _base_cfg(family="wavlm", hidden_size=dh * H, num_hidden_layers=1, num_attention_heads=H, num_conv_pos_embeddings=3,
                    num_conv_pos_embedding_groups=H, rel_pos_buckets=8, rel_pos_max_distance=16)
    ov = {"encoder.layers.0.attention.gru_rel_pos_linear.weight": w, "encoder.layers.0.attention.gru_rel_pos_linear.bias": b,
          "encoder.layers.0.attention.gru_rel_pos_const": const}
    return lib, _make_handle(lib, cfg, precision_name, ov)


@pytest.mark.parametrize("variant,precision_name,dtype", GATE_RUNS, ids=[f"{v or 'bf16'}lib-{p}" for v, p, _ in GATE_RUNS])
@pytest.mark.parametrize("c", P.GCASES, ids=[P.gcase_id(c) for c in P.GCASES])
def test_gate(c, variant, precision_name, dtype):
    for block in P.GBLOCKS:
        lib, handle = _gate_handle(c.dh, c.H, block, variant, precision_name)
        w, b, const = P.gate_params(c, block)
        u = P.gate_input(c, block, dtype)
        rows, D = u.shape
        buf = torch.full((rows + 2 * GROWS, D), float("nan"), dtype=dtype, device=DEV)   # u between guard rows of NaN
        buf[GROWS:GROWS + rows] = u.to(DEV)
        n = c.B * c.H * c.T
        out = torch.full((n + 2 * 64,), float("nan"), device=DEV)
        rc, glue, _ = _step(lib, handle, step=3, B=c.B, T=c.T, layer=0, x=buf[GROWS:], out=out[64:])
        _lib.check(rc, "svt_debug_encoder_step", lib)
        assert glue == (41 if c.vec else 43) + (dtype != torch.float32), glue
        res = out.cpu()
        assert torch.isnan(res[:64]).all() and torch.isnan(res[64 + n:]).all(), "the gate kernel wrote outside (B, H, T)"
        got = res[64:64 + n].reshape(c.B, c.H, c.T)
        assert torch.isfinite(got).all(), "NaN in the gate: a guard row was read, an element was not written, or saturation gave NaN"
        ref, lim, s = P.gate_reference(c, w, b, const, u)
        ratio = (got.double() - ref).abs() / lim
        i = int(ratio.argmax())
        print(f"encoder-glue gate {P.gcase_id(c)} [{variant or 'bf16'} library, {precision_name}] {block}: key 45 = {glue}, worst err / limit "
              f"{ratio.max().item():.4f} at flat index {i}")
        assert ratio.max().item() <= 1.0
        if block == "saturated":
            # beyond +-90 the sigmoids are exactly 0 or 1 in fp32: gate = 2, 1, or fl(fl(c - 1) + 2)
            sa, sb = (x.reshape(c.B, c.T, c.H).permute(0, 2, 1) for x in s)
            cst = const.reshape(1, c.H, 1).expand(c.B, c.H, c.T)
            assert (got[sa < -90] == 2.0).all()
            assert (got[(sa > 90) & (sb < -90)] == 1.0).all()
            both = (sa > 90) & (sb > 90)
            assert torch.equal(got[both], (cst[both] - 1.0) + 2.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# the hook's refusals: SVT_ERR_INVALID, the error names the hook, nothing is launched
def _refusal_setup():
    c = next(c for c in P.PCASES if c.form == "plain" and "bf16" in c.modes and not c.bn)
    lib, handle = _posconv_handle(P.geometry_key(c), "bf16")
    need = lib.svt_encoder_workspace_bytes(handle, c.B, c.T)
    ws = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    x = P.make_h(c).to(DEV)
    out = torch.full((x.numel() + 16,), float("nan"), device=DEV)
    good = dict(step=1, B=c.B, T=c.T, n_samples=c.T, x=x.data_ptr(), out=out.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=need)
    return lib, handle, good, (ws, x, out)


def _gate_good():
    """A descriptor the gate handle (head size 8, 4 heads) accepts, and the buffers it points to."""
    u = torch.zeros(4, 32, device=DEV)
    out = torch.full((64,), float("nan"), device=DEV)
    return dict(step=3, B=1, T=4, layer=0, x=u.data_ptr(), out=out.data_ptr()), (u, out)


REFUSALS = {
    "struct_size": lambda g: dict(g, struct_size=ctypes.sizeof(_lib.EncoderStepDescC) - 8),
    "step 0": lambda g: dict(g, step=0),
    "step 4": lambda g: dict(g, step=4),
    "null x": lambda g: dict(g, x=0),
    "null out": lambda g: dict(g, out=0),
    "null workspace": lambda g: dict(g, workspace=0),
    "x not 16-byte aligned": lambda g: dict(g, x=g["x"] + 4),
    "out not 16-byte aligned": lambda g: dict(g, out=g["out"] + 8),
    "workspace not 16-byte aligned": lambda g: dict(g, workspace=g["workspace"] + 4),
    "B = 0": lambda g: dict(g, B=0),
    "T = 0": lambda g: dict(g, T=0, n_samples=0),
    "T is not the plan's frame count": lambda g: dict(g, T=g["T"] + 1),
    "workspace one byte short": lambda g: dict(g, workspace_bytes=g["workspace_bytes"] - 1),
    "step 2 without rel_pos_buckets": lambda g: dict(g, step=2),
    "step 3 without rel_pos_buckets": lambda g: dict(g, step=3, layer=0),
}


def _call(lib, handle, fields):
    d = _lib.EncoderStepDescC()
    d.struct_size = ctypes.sizeof(d)
    for k, v in fields.items():
        setattr(d, k, v)
    torch.cuda.synchronize()
    return lib.svt_debug_encoder_step(handle, ctypes.byref(d), torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("name", list(REFUSALS))
def test_the_hook_refuses(name):
    lib, handle, good, (ws, x, out) = _refusal_setup()
    before = lib.svt_debug_set(45, 0)
    rc = _call(lib, handle, REFUSALS[name](good))
    assert rc == SVT_ERR_INVALID and b"svt_debug_encoder_step" in lib.svt_last_error(), (name, rc, lib.svt_last_error())
    torch.cuda.synchronize()
    assert lib.svt_debug_set(45, 0) == before and torch.isnan(out).all() and bool((ws == 0xA5).all()), f"{name}: something was launched"
    _lib.check(_call(lib, handle, good), "svt_debug_encoder_step", lib)   # and the unchanged descriptor is accepted
    assert torch.isfinite(out[:x.numel()]).all() and torch.isnan(out[x.numel():]).all()


@pytest.mark.parametrize("layer", (-1, 1))
def test_the_hook_refuses_a_layer_out_of_range(layer):
    lib, handle = _gate_handle(8, 4, "ordinary", None, "fp32")
    good, keep = _gate_good()
    rc = _call(lib, handle, dict(good, layer=layer))
    assert rc == SVT_ERR_INVALID and b"svt_debug_encoder_step" in lib.svt_last_error(), (rc, lib.svt_last_error())
    assert torch.isnan(keep[1]).all()
    _lib.check(_call(lib, handle, good), "svt_debug_encoder_step", lib)


def test_the_hook_refuses_null_and_unfinalized_handles():
    lib, handle, good, keep = _refusal_setup()
    assert _call(lib, None, good) == SVT_ERR_INVALID and b"svt_debug_encoder_step" in lib.svt_last_error()
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.svt_debug_encoder_step(handle, None, stream) == SVT_ERR_INVALID
    c = next(c for c in P.PCASES if c.form == "plain" and "bf16" in c.modes and not c.bn)
    cfg = _base_cfg(family="hubert", hidden_size=c.cg * c.G, num_hidden_layers=0, num_attention_heads=1, num_conv_pos_embeddings=c.kp,
                    num_conv_pos_embedding_groups=c.G)
    raw = _make_handle(lib, cfg, "bf16", P.make_params(c), finalize=False)
    try:
        assert _call(lib, raw, good) == SVT_ERR_INVALID and b"svt_encoder_finalize" in lib.svt_last_error(), lib.svt_last_error()
        assert torch.isnan(keep[2]).all()
    finally:
        lib.svt_encoder_destroy(raw)
