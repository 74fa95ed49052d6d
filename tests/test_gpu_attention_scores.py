"""GPU tests of the score-matrix attention alone, through the C-ABI test hook svt_debug_attention_scores: the path every attention outside the
fused kernels' reach takes (the fp32 parity mode, 16-bit head sizes other than 64 / 128, WavLM's biased attention at head size 128 or
2 T - 1 > 8192, WavLM in the split-operand modes) -- two batched products around scores_add_relbias_kernel, softmax_rows_kernel and
transpose_v_kernel (csrc/encoder_ops.hip), which no other test runs outside a whole model forward.

The hook fills the scores, the probabilities and V^T with 0xFF bytes first (the encoder's workspace is uninitialised), so a pad column the
kernels fail to write reaches the output as NaN.  The reference is reference() of tests/test_gpu_attention.py (fp64 on the CPU from the same
rounded inputs), every case asserts the kernel id of its last product (P V), every output element is compared under the per-element limit tests/gemm_limit.py derives (tests/test_gemm_limit.py shows on
the CPU that a correct pipeline passes it and that P pad columns of 1, a relative-position index off by one and the neighbouring query's gate
do not).  The output is NaN-poisoned and its rows are padded by 64 columns, which must keep their bits."""
import numpy as np
import pytest
import torch

import gemm_limit as G
import test_gpu_attention as TA

pytestmark = pytest.mark.gpu

from svt_speechbrain_amd import _lib  # noqa: E402

DEV = "cuda:0"


def launch(lib, c, prec, x, gate, pb):
    """Returns (rc, out (B, T, D) on the CPU, id of the last product's kernel); asserts that the 64 pad columns of every output row kept their bits."""
    B, T, H, dh = c.B, c.T, c.H, c.dh
    D, es = H * dh, x.element_size()
    if c.layout == "packed":
        xd = x.to(DEV)
        qp, kp, vp, ldq, ldkv = xd.data_ptr(), xd.data_ptr() + es * D, xd.data_ptr() + 2 * es * D, 3 * D, 3 * D
    else:   # q in its own buffer, k | v packed: the RCA layers' cross-attention call
        qd, kvd = x[..., :D].contiguous().to(DEV), x[..., D:].contiguous().to(DEV)
        qp, kp, vp, ldq, ldkv = qd.data_ptr(), kvd.data_ptr(), kvd.data_ptr() + es * D, D, 2 * D
    ldo = D + 64
    out = torch.full((B, T, ldo), float("nan"), device=DEV, dtype=x.dtype)
    ints = torch.int16 if es == 2 else torch.int32
    before = out.view(ints).clone()
    gd, pd = (gate.to(DEV), pb.to(DEV)) if gate is not None else (None, None)
    rc = lib.svt_debug_attention_scores(prec, qp, kp, vp, out.data_ptr(), B, T, H, dh, ldq, ldkv, ldo, G.attn_scale(dh),
                                        gd.data_ptr() if gd is not None else None, pd.data_ptr() if pd is not None else None, 0,
                                        torch.cuda.current_stream().cuda_stream)
    kid = lib.svt_debug_set(39, 0)
    torch.cuda.synchronize()
    assert torch.equal(out.view(ints)[..., D:], before[..., D:]), "columns past D of a padded output row were written"
    if rc != 0:
        assert torch.equal(out.view(ints), before), "a refused call wrote to the output"
    return rc, out[..., :D].cpu(), kid


RUNS = [(c, run) for c in G.ATTN for run in G.attn_runs(c)]


@pytest.mark.parametrize("c,run", RUNS, ids=[f"{G.acase_id(c)}-{run[3]}" for c, run in RUNS])
def test_score_matrix_attention(c, run):
    variant, dtype, prec, tag = run
    lib = _lib.load(variant)
    x, gate, pb, o, A = TA.make_case(c, dtype, bias=c.bias)
    x2, gate2, pb2 = G.attn_inputs(c, dtype)
    assert torch.equal(x, x2) and (gate is None or (torch.equal(gate, gate2) and torch.equal(pb, pb2))), "the two files draw different inputs"
    rc, got, kid = launch(lib, c, prec, x, gate, pb)
    _lib.check(rc, "svt_debug_attention_scores", lib)
    assert kid == c.kid, f"the last product ran on kernel {kid}, the case is written for kernel {c.kid}"
    assert torch.isfinite(got).all(), "NaN in the output: an unwritten output element, or a pad of S / P / V^T that was read"
    q, k, v = (t.reshape(c.B, c.T, c.H, c.dh) for t in x.split(c.H * c.dh, dim=-1))
    delta, spread = G.attn_row_terms(q, k, G.attn_scale(c.dh), gate, pb, prec)
    err = (got.double() - o).abs()
    ratio = err / G.attn_limit(c, prec, tag if prec == 1 else None, v, o, A, delta, spread)
    worst = ratio.max().item()
    b, t, col = np.unravel_index(int(ratio.argmax()), ratio.shape)
    print(f"score-matrix attention [{tag}] {G.acase_id(c)}: worst err / limit {worst:.3f} at clip {b} query {t} head {col // c.dh} column {col % c.dh}; "
          f"max|err| {err.max().item():.3e}; last product on kernel {kid}")
    assert worst <= 1.0, (tag, G.acase_id(c), worst, (int(b), int(t), int(col)))


def test_reference_of_the_cpu_proof_is_the_reference_used_here():
    c = G.AC(2128, "16", 2, 65, 2, 128, bias=True)
    x, gate, pb, o, A = TA.make_case(c, torch.float16, bias=True)
    q, k, v = (t.reshape(c.B, c.T, c.H, c.dh) for t in x.split(c.H * c.dh, dim=-1))
    o2, A2 = G.attn_reference(q, k, v, G.attn_scale(c.dh), gate, pb)
    assert torch.equal(o, o2) and torch.equal(A, A2) and G.attn_scale(c.dh) == TA._scale(c.dh)


@pytest.mark.parametrize("build", list(G.BUILDS))
def test_the_hook_refuses_what_the_fused_kernel_serves(build):
    """16-bit, head size 64, no bias: the fused kernel's geometry.  SVT_ERR_INVALID, nothing launched, the output untouched."""
    variant, dtype, _ = G.BUILDS[build]
    lib = _lib.load(variant)
    c = G.AC(0, "16", 2, 65, 2, 64)
    x, _, _ = G.attn_inputs(c, dtype)
    rc, _, _ = launch(lib, c, 1, x, None, None)
    assert rc == -1 and b"fused kernel" in lib.svt_last_error(), (rc, lib.svt_last_error())
