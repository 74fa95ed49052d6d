"""GPU: every kernel of the AV-HuBERT lip front-end ALONE -- one step of a finalized handle on the test's own buffers through the C-ABI hook
svt_debug_video_step, with the handle's own uploaded weights (the folds and fragment images of svt_video_finalize are inside the tested unit)
-- against the fp64 references and the derived limits of tests/video_limit.py, in both 16-bit builds and the fp32 mode, with the kernel id of
svt_debug_set key 43 asserted in every case.  tests/test_video_limit.py proves on the CPU, for these very inputs, that a correct kernel stays
inside the limits and that sixteen mutants do not.

Every buffer lives in one arena of 0xFF bytes (NaN in every type): what a kernel reads outside its operands is NaN, and after every case the
bytes between the buffers must still be 0xFF.  A stage-1 block input and its t1 are followed by the one zero pixel the forward keeps behind
its stage-1 workspace buffers (the grouped G = 4 product's last window reads it).  Each case prints its worst err / limit, where it sits, and
the GEMM kernel id of key 39 for the product launches."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import video_limit as V  # noqa: E402
from svt_speechbrain_amd import _lib  # noqa: E402
from svt_speechbrain_amd.video import SubModel  # noqa: E402

DEV = "cuda:0"
SVT_ERR_INVALID = -1
BUILDS16 = ("bf16", "f16")
KEY_DEFAULTS = {23: 1, 26: 1, 27: 1}


@functools.lru_cache(maxsize=None)
def _ctx(build):
    """(library, finalized handle, module that owns it) of a build, with the seeded parameters of tests/video_limit.py."""
    m = SubModel(512, V.EMBED, "prelu", precision=V.PRECISION[build], seed=1)
    m.load_state_dict(V.state_dict(), strict=True)
    m = m.to(DEV)
    slot = m._sync(torch.device(DEV))
    return _lib.load(V.BUILDS[build][0]), slot.handle, m


class Arena:
    """One device allocation of 0xFF bytes; buffers 256-byte aligned with at least 256 guard bytes between them."""

    def __init__(self, nbytes):
        self.buf = torch.full((nbytes + 4096,), 0xFF, dtype=torch.uint8, device=DEV)
        self.off = 0
        self.mask = torch.zeros(nbytes + 4096, dtype=torch.bool)

    def put(self, t, tail_zero_bytes=0):
        n = t.numel() * t.element_size()
        off = (self.off + 255) // 256 * 256
        view = self.buf[off:off + n].view(t.dtype).view(t.shape)
        view.copy_(t)
        if tail_zero_bytes:
            self.buf[off + n:off + n + tail_zero_bytes] = 0
        self.mask[off:off + n + tail_zero_bytes] = True
        self.off = off + n + tail_zero_bytes + 256
        assert self.off <= self.buf.numel() - 256
        return view

    def check_guards(self, what):
        torch.cuda.synchronize()
        outside = self.buf.cpu()[~self.mask]
        assert bool((outside == 0xFF).all()), f"{what}: a byte outside the buffers was written"


def _one_frame_per_workgroup(F, wg):
    """With workgroups = 0 the persistent launchers size their grid by the CU count: the cases that rely on one frame per workgroup say so."""
    return wg > 0 or F <= torch.cuda.get_device_properties(0).multi_processor_count


def _nbytes(*tensors):
    return sum(t.numel() * t.element_size() + 1024 for t in tensors)


def _step(build, keys=(), **fields):
    """One svt_debug_video_step call under the case's debug keys (restored).  Returns (rc, key-43 id, key-39 id)."""
    lib, handle, _ = _ctx(build)
    d = _lib.VideoStepDescC()
    d.struct_size = ctypes.sizeof(d)
    for k, v in fields.items():
        setattr(d, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    torch.cuda.synchronize()
    try:
        for k, v in keys:
            lib.svt_debug_set(k, v)
        rc = lib.svt_debug_video_step(handle, ctypes.byref(d), torch.cuda.current_stream().cuda_stream)
    finally:
        for k, _ in keys:
            lib.svt_debug_set(k, KEY_DEFAULTS[k])
    return rc, lib.svt_debug_set(43, 0), lib.svt_debug_set(39, 0)


def _ok(rc, build):
    _lib.check(rc, "svt_debug_video_step", _ctx(build)[0])


def _report(family, build, name, results, gemm_id=None):
    for part, (r, at) in results.items():
        print(f"video-kernel {family} {build} {name} {part}: worst err / limit {r:.4f} at {at}" + (f", key 39 = {gemm_id}" if gemm_id else ""))


# ---- stem alone (step 1) --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", ("bf16", "f16", "fp32"))
@pytest.mark.parametrize("c", V.STEM, ids=lambda c: f"{c.h}x{c.w}-T{c.T}")
def test_stem_alone(c, build):
    dtype = V.BUILDS[build][1]
    video = V.video_input(c, build)
    _, _, H0, W0, _, _ = V.stem_geom(c.h, c.w)
    out0 = torch.full((c.B * c.T, H0, W0, 64), float("nan"), dtype=dtype)
    ar = Arena(_nbytes(video, out0))
    x, out = ar.put(video), ar.put(out0)
    rc, kid, _ = _step(build, step=1, B=c.B, T=c.T, h=c.h, w=c.w, x=x, out=out)
    _ok(rc, build)
    assert kid == (V.K_STEM_F32 if build == "fp32" else V.K_STEM_16)
    ref, lim = V.stem_reference(build, video)
    _report("stem", build, f"{c.h}x{c.w}-T{c.T}", {"out": V.check_plain(out.cpu(), ref, lim, f"stem {c}")})
    ar.check_guards(f"stem {c}")


# ---- max-pool alone (step 2) ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", ("bf16", "f16", "fp32"))
@pytest.mark.parametrize("c", V.POOL, ids=lambda c: f"{c.H0}x{c.W0}")
def test_maxpool_alone(c, build):
    dtype = V.BUILDS[build][1]
    x0 = V.pool_input(c, build)
    H1, W1 = (c.H0 - 1) // 2 + 1, (c.W0 - 1) // 2 + 1
    out0 = V.poisoned(c.F, H1, W1, 64, dtype)
    ar = Arena(_nbytes(x0, out0))
    x, out = ar.put(x0), ar.put(out0)
    rc, kid, _ = _step(build, step=2, F=c.F, H=c.H0, W=c.W0, x=x, out=out)
    _ok(rc, build)
    assert kid == (V.K_POOL_F32 if build == "fp32" else V.K_POOL_X8)
    V.check_exact_haloed(out.cpu(), V.maxpool_reference(x0), f"max-pool {c}")
    ar.check_guards(f"max-pool {c}")


# ---- fused stem + pool (step 3) -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", BUILDS16)
@pytest.mark.parametrize("c", V.FUSED, ids=lambda c: f"{c.h}x{c.w}-B{c.B}-T{c.T}-wg{c.wg}")
def test_fused_stem_and_pool(c, build):
    dtype = V.BUILDS[build][1]
    assert _one_frame_per_workgroup(c.B * c.T, c.wg)
    video = V.video_input(c, build)
    _, _, _, _, H1, W1 = V.stem_geom(c.h, c.w)
    out0 = V.poisoned(c.B * c.T, H1, W1, 64, dtype)
    ar = Arena(_nbytes(video, out0))
    x, out = ar.put(video), ar.put(out0)
    rc, kid, _ = _step(build, step=3, B=c.B, T=c.T, h=c.h, w=c.w, workgroups=c.wg, x=x, out=out)
    _ok(rc, build)
    assert kid == V.K_STEM_POOL
    ref, lim = V.fused_reference(build, video)
    _report("stem+pool", build, f"{c.h}x{c.w}-B{c.B}-T{c.T}-wg{c.wg}", {"out": V.check_haloed(out.cpu(), ref, lim, f"stem + pool {c}")})
    ar.check_guards(f"stem + pool {c}")


@pytest.mark.parametrize("build", BUILDS16)
def test_fused_stem_refuses_what_the_forward_would_not_run(build):
    """W0 = 68 > 64 pooled-item columns: conv3d_front_pool_ok is false, the step refuses and the output stays untouched; under key 26 = 0
    every geometry is refused."""
    dtype = V.BUILDS[build][1]
    lib = _ctx(build)[0]
    for (h, w), keys in ((V.FUSED_REFUSED, ()), ((16, 18), ((26, 0),))):
        video = torch.zeros(1, 1, 1, h, w)
        _, _, _, _, H1, W1 = V.stem_geom(h, w)
        out0 = V.poisoned(1, H1, W1, 64, dtype)
        ar = Arena(_nbytes(video, out0))
        x, out = ar.put(video), ar.put(out0)
        rc, _, _ = _step(build, keys=keys, step=3, B=1, T=1, h=h, w=w, x=x, out=out)
        assert rc == SVT_ERR_INVALID and b"svt_debug_video_step" in lib.svt_last_error(), (rc, lib.svt_last_error())
        assert torch.equal(V._bits(out.cpu()), V._bits(out0))
        ar.check_guards("refused stem + pool")


# ---- zero-halo (step 4) ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", ("bf16", "fp32"))
@pytest.mark.parametrize("c", V.HALO, ids=lambda c: f"{c.Hp}x{c.Wp}x{c.C}-F{c.F}")
def test_zero_halo_alone(c, build):
    dtype = V.BUILDS[build][1]
    n = c.F * c.Hp * c.Wp * c.C
    raw = torch.full((n * torch.empty(0, dtype=dtype).element_size(),), 0xFF, dtype=torch.uint8).view(dtype).view(c.F, c.Hp, c.Wp, c.C)
    ar = Arena(_nbytes(raw))
    out = ar.put(raw)
    rc, kid, _ = _step(build, step=4, F=c.F, H=c.Hp, W=c.Wp, C=c.C, out=out)
    _ok(rc, build)
    assert kid == V.K_HALO
    V.check_zero_halo(out.cpu(), -1, f"zero-halo {c}")
    ar.check_guards(f"zero-halo {c}")


# ---- BasicBlocks (step 5) -------------------------------------------------------------------------------------------------------
def _block_builds():
    return [pytest.param(c, b, id=f"{c.name}-{b}") for c in V.BLOCKS for b in (("fp32",) if c.fp32 else BUILDS16)]


@pytest.mark.parametrize("c,build", _block_builds())
def test_block_alone(c, build):
    dtype = V.BUILDS[build][1]
    assert _one_frame_per_workgroup(c.F, c.wg)
    stride, cin, C, Ho, Wo = V.block_dims(c)
    x0 = V.block_input(c, build)
    o0 = V.poisoned(c.F, Ho, Wo, C, dtype)
    ar = Arena(_nbytes(x0, o0, o0, o0))
    tail = 64 * x0.element_size() if c.li == 0 else 0
    x, t1 = ar.put(x0, tail), ar.put(o0, tail)
    ds = ar.put(o0) if stride == 2 else None          # behind t1 in one allocation, as in the workspace
    out = ar.put(o0)
    rc, kid, gid = _step(build, keys=c.keys, step=5, F=c.F, H=c.H, W=c.W, li=c.li, b=c.b, workgroups=c.wg, x=x, t1=t1,
                         ds=ds if ds is not None else 0, out=out)
    _ok(rc, build)
    assert kid == c.kid, (c.name, kid, c.kid)
    res = V.check_block(c, build, x0, t1.cpu(), None if ds is None else ds.cpu(), out.cpu())
    assert torch.equal(V._bits(x.cpu()), V._bits(x0)), "the block input must survive"
    direct = kid % 10 in (V.VK_C64, V.VK_C128)
    _report("block", build, c.name, res, None if direct else gid)
    ar.check_guards(c.name)


# ---- average pool (step 6) ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", ("bf16", "f16", "fp32"))
@pytest.mark.parametrize("c", V.AVG, ids=lambda c: f"{c.H}x{c.W}-F{c.F}")
def test_average_pool_alone(c, build):
    dtype = V.BUILDS[build][1]
    x0 = V.avg_input(c, build)
    out0 = torch.full((c.F, 512), float("nan"), dtype=dtype)
    ar = Arena(_nbytes(x0, out0))
    x, out = ar.put(x0), ar.put(out0)
    rc, kid, _ = _step(build, step=6, F=c.F, H=c.H, W=c.W, x=x, out=out)
    _ok(rc, build)
    assert kid == (V.K_AVG_F32 if build == "fp32" else V.K_AVG_16)
    _report("avgpool", build, f"{c.H}x{c.W}-F{c.F}", {"out": V.check_plain(out.cpu(), *V.avg_reference(build, x0), f"average pool {c}")})
    ar.check_guards(f"average pool {c}")


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_hook_refuses_what_the_header_says_it_refuses():
    """Every documented refusal: SVT_ERR_INVALID, the hook named in the error text, every output buffer untouched."""
    build = "bf16"
    lib, handle, _ = _ctx(build)
    dtype = V.BUILDS[build][1]
    video = torch.zeros(1, 1, 2, 160, 160)
    o0 = V.poisoned(2, 8, 8, 128, dtype)
    ar = Arena(_nbytes(video, o0, o0, o0, o0))
    x, t1, ds, out = ar.put(video), ar.put(o0), ar.put(o0), ar.put(o0)
    stem = dict(step=1, B=1, T=2, h=8, w=8, x=x, out=out)
    block = dict(step=5, F=2, H=8, W=8, li=1, b=1, x=x, t1=t1, ds=ds, out=out)
    halo = dict(step=4, F=2, H=10, W=10, C=128, out=out)
    cases = [
        ("struct_size", dict(stem, struct_size=8)),
        ("step 0", dict(stem, step=0)), ("step 7", dict(stem, step=7)),
        ("null x", dict(stem, x=0)), ("null out", dict(stem, out=0)), ("null t1", dict(block, t1=0)),
        ("null ds of a block with a downsample", dict(block, b=0, ds=0)),
        ("unaligned x", dict(stem, x=x.data_ptr() + 4)), ("unaligned out", dict(block, out=out.data_ptr() + 8)),
        ("unaligned t1", dict(block, t1=t1.data_ptr() + 2)), ("unaligned ds", dict(block, ds=ds.data_ptr() + 2)),
        ("B = 0", dict(stem, B=0)), ("T = 0", dict(stem, T=0)), ("h = 7", dict(stem, h=7)), ("w = 7", dict(stem, w=7)),
        ("fused: B = 0", dict(stem, step=3, B=0)), ("fused: w = 7", dict(stem, step=3, w=7)),
        ("li = 4", dict(block, li=4)), ("li = -1", dict(block, li=-1)), ("b = 2", dict(block, b=2)), ("b = -1", dict(block, b=-1)),
        ("block H = 0", dict(block, H=0)), ("block W = 0", dict(block, W=0)), ("block F = 0", dict(block, F=0)),
        ("pool H = 0", dict(step=2, F=2, H=0, W=8, x=x, out=out)), ("average F = 0", dict(step=6, F=0, H=1, W=1, x=x, out=out)),
        ("halo Hp = 2", dict(halo, H=2)), ("halo C = 96", dict(halo, C=96)),
        ("stem too large for the LDS", dict(stem, h=160, w=160)),
        ("workgroups < 0", dict(block, workgroups=-1)), ("fused: workgroups < 0", dict(stem, step=3, workgroups=-1)),
    ]
    stream = torch.cuda.current_stream().cuda_stream

    def call(h, fields):
        d = _lib.VideoStepDescC()
        d.struct_size = ctypes.sizeof(d)
        for k, v in fields.items():
            setattr(d, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
        return lib.svt_debug_video_step(h, ctypes.byref(d), stream)

    def untouched(name):
        torch.cuda.synchronize()
        for buf in (t1, ds, out):
            assert torch.equal(V._bits(buf.cpu()), V._bits(o0)), name
        ar.check_guards(name)

    for name, fields in cases:
        rc = call(handle, fields)
        assert rc == SVT_ERR_INVALID and b"svt_debug_video_step" in lib.svt_last_error(), (name, rc, lib.svt_last_error())
        untouched(name)
    assert lib.svt_debug_video_step(handle, None, stream) == SVT_ERR_INVALID
    assert lib.svt_debug_video_step(None, ctypes.byref(_lib.VideoStepDescC(struct_size=ctypes.sizeof(_lib.VideoStepDescC))), stream) == SVT_ERR_INVALID
    # an unfinalized handle
    h2 = ctypes.c_void_p()
    _lib.check(lib.svt_video_create(V.EMBED, 1, 0, ctypes.byref(h2)), "svt_video_create", lib)
    try:
        rc = call(h2, stem)
        assert rc == SVT_ERR_INVALID and b"svt_debug_video_step" in lib.svt_last_error(), (rc, lib.svt_last_error())
        untouched("unfinalized handle")
    finally:
        lib.svt_video_destroy(h2)
    # and the same descriptors, valid, run
    _lib.check(call(handle, halo), "svt_debug_video_step", lib)
    assert lib.svt_debug_set(43, 0) == V.K_HALO


# ---- the forward's own workspace ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", BUILDS16)
def test_forward_reads_nothing_unwritten_behind_a_stage1_buffer(build):
    """26 x 26 pixels, 11 frames: stage 1 is 7 x 7 on the grouped G = 4 product, whose last window reads the pixel BEHIND the last frame of
    its input.  With 11 x 81 pixels that was 128 bytes of alignment padding no kernel writes; video_carve now keeps a tail pixel there and
    zero_halo_kernel zeroes it.  A workspace of NaN patterns in front of the call changes nothing."""
    lib, _, m = _ctx(build)
    g = torch.Generator().manual_seed(26)
    video = torch.randn(1, 1, 11, 26, 26, generator=g).to(DEV)
    slot = m._sync(torch.device(DEV))
    _lib.check(lib.svt_video_keep_workspace(slot.handle, 0), "svt_video_keep_workspace", lib)
    try:
        want = m(video).clone()
        assert lib.svt_debug_set(43, 0) == V.K_AVG_16
        assert torch.isfinite(want).all()
        slot.ws.zero_()
        clean = m(video).clone()
        slot.ws.fill_(0xFF)
        assert torch.equal(m(video), clean) and torch.equal(want, clean)
    finally:
        _lib.check(lib.svt_video_keep_workspace(slot.handle, 1), "svt_video_keep_workspace", lib)
