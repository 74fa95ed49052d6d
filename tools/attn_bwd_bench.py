"""Micro-benchmark of the fused attention backward (csrc/attention_bwd.hip) on the encoder's shapes, against torch on the same device.
Usage: python tools/attn_bwd_bench.py [--build f16] [--only base] [--iters 50] [--reps 5]
       python tools/attn_bwd_bench.py --kernels-only      (a few backward calls and nothing else: the run to put under
                                                           `rocprofv3 --kernel-trace --stats` for the three kernels' own times)
       SVT_LIB_SUFFIX=bwddirect python tools/attn_bwd_bench.py   (an experimental build: make XNAME=bwddirect XDEFS=-DSVT_ATTN_BWD_DIRECT_MASK,
                                                                  attn_bwd_dkv_kernel with one Philox call per element)

Per shape and dropout rate, HIP events around `iters` calls after a warm-up, `reps` times, the candidates alternating within a repetition;
the median of the repetitions with their range:
  forward   svt_attention_forward (the plain kernel at p = 0, the masked one at p > 0)
  backward  svt_attention_backward: three launches (L / delta, dQ, dK and dV) -- the sum
  eager     torch autograd's backward of the expression HF runs, matmul -> softmax -> dropout -> matmul, same dtype   [yardstick (a)]
  sdpa      the backward of torch.nn.functional.scaled_dot_product_attention, where the installed torch runs it       [yardstick (b)]
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from svt_speechbrain_amd import _lib  # noqa: E402

SHAPES = [("base", 32, 499, 12), ("probe", 8, 249, 12)]
DH = 64


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", default=None, help="library build: f16 = the IEEE-half build (default: bf16)")
    ap.add_argument("--only", default=None)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rates", default="0,0.1")
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    lib = _lib.load(a.build)
    dev = torch.device("cuda:0")
    dtype = torch.float16 if a.build == "f16" else torch.bfloat16
    st = torch.cuda.current_stream().cuda_stream
    print(f"device: {torch.cuda.get_device_name(0)}; build {a.build or 'bf16'}"
          + (f"; library suffix {os.environ['SVT_LIB_SUFFIX']}" if os.environ.get("SVT_LIB_SUFFIX") else "")
          + f"; {a.iters} calls per window, {a.reps} windows, median [min .. max] in us", flush=True)
    for name, B, T, H in SHAPES:
        if a.only and a.only not in name:
            continue
        D = H * DH
        g = torch.Generator().manual_seed(3)
        qkv = (torch.randn(B, T, 3 * D, generator=g) * 1.5).to(dev, dtype)
        do = torch.randn(B, T, D, generator=g).to(dev, dtype)
        out = torch.empty(B, T, D, device=dev, dtype=dtype)
        grads = torch.empty(B, T, 3 * D, device=dev, dtype=dtype)
        scale = DH ** -0.5
        for p in [float(x) for x in a.rates.split(",")]:
            d = _lib.AttentionDescC()
            d.struct_size, d.precision = ctypes.sizeof(d), 1
            d.q, d.k, d.v, d.o, d.d_o = qkv.data_ptr(), qkv.data_ptr() + 2 * D, qkv.data_ptr() + 4 * D, out.data_ptr(), do.data_ptr()
            d.dq, d.dk, d.dv = grads.data_ptr(), grads.data_ptr() + 2 * D, grads.data_ptr() + 4 * D
            d.ldq, d.ldkv, d.ldo, d.lddo, d.lddq, d.lddkv = 3 * D, 3 * D, D, D, 3 * D, 3 * D
            d.batch, d.t, d.heads, d.head_dim = B, T, H, DH
            d.scale, d.step, d.p, d.seed, d.layer, d.e0 = scale, 5, p, 7, 3, 0
            need = ctypes.c_size_t(0)
            _lib.check(lib.svt_attention_backward(ctypes.byref(d), None, ctypes.byref(need), 0, st), "svt_attention_backward", lib)
            ws = torch.empty(need.value, device=dev, dtype=torch.uint8)

            def fwd():
                _lib.check(lib.svt_attention_forward(ctypes.byref(d), 0, st), "svt_attention_forward", lib)

            def bwd():
                _lib.check(lib.svt_attention_backward(ctypes.byref(d), ws.data_ptr(), ctypes.byref(need), 0, st), "svt_attention_backward", lib)

            fwd()
            bwd()
            torch.cuda.synchronize()
            form = lib.svt_debug_set(46, 0)
            if a.kernels_only:
                for _ in range(a.iters):
                    bwd()
                torch.cuda.synchronize()
                print(f"{name} B={B} T={T} H={H} p={p}: {a.iters + 1} backward calls (form {form})", flush=True)
                continue

            # the yardsticks: (B, H, T, 64) leaves of the same values
            q, k, v = (t.reshape(B, T, H, DH).transpose(1, 2).contiguous().requires_grad_(True) for t in qkv.split(D, dim=-1))
            gy = do.view(B, T, H, DH).transpose(1, 2).contiguous()
            w = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * scale, dim=-1)
            eager_out = torch.matmul(torch.nn.functional.dropout(w, p=p, training=True), v)
            cands = {"forward": fwd, "backward": bwd,
                     "eager": lambda: torch.autograd.grad(eager_out, (q, k, v), gy, retain_graph=True)}
            try:
                sdpa_out = torch.nn.functional.scaled_dot_product_attention(q, k, v, dropout_p=p, scale=scale)
                torch.autograd.grad(sdpa_out, (q, k, v), gy, retain_graph=True)
                cands["sdpa"] = lambda: torch.autograd.grad(sdpa_out, (q, k, v), gy, retain_graph=True)
            except Exception as e:   # report only
                print(f"  sdpa backward does not run here: {type(e).__name__}: {str(e)[:100]}")
            for fn in cands.values():   # warm-up of every candidate
                timed(fn, 3)
            times = {n: [] for n in cands}
            for _ in range(a.reps):
                for n, fn in cands.items():
                    times[n].append(timed(fn, a.iters))
            med = {n: statistics.median(t) for n, t in times.items()}
            print(f"{name} B={B} T={T} H={H} p={p} (backward form {form}):", flush=True)
            for n, t in times.items():
                print(f"  {n:9s} {med[n]:9.1f} [{min(t):9.1f} .. {max(t):9.1f}]", flush=True)
            flops = 14.0 * B * H * T * T * DH   # seven products
            print(f"  backward / forward {med['backward'] / med['forward']:.2f} (seven products against two: 3.5 is the arithmetic floor); "
                  f"backward {flops / med['backward'] / 1e6:.1f} TFLOP/s; eager / backward {med['eager'] / med['backward']:.2f}"
                  + (f"; sdpa / backward {med['sdpa'] / med['backward']:.2f}" if "sdpa" in med else ""), flush=True)
            print(f"  gate (backward faster than eager autograd): {'holds' if max(times['backward']) < min(times['eager']) else 'FAILS'}", flush=True)
            del w, eager_out, q, k, v
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
