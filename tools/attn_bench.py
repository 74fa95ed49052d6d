"""Micro-benchmark + check of the fused attention kernel on the encoder's shapes.
Usage: python tools/attn_bench.py [--check]
       python tools/attn_bench.py --dropout 0.1     (flash_attn_drop_kernel: the same shapes with the dropout mask inside)"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from svt_speechbrain_amd import _lib  # noqa: E402

SHAPES = [("base", 32, 499, 12, 64), ("large", 64, 499, 16, 64), ("c1", 1, 249, 12, 64), ("probe", 8, 249, 12, 64), ("rca", 16, 499, 8, 128)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--only", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--wide", type=int, default=None, help="svt_debug_set key 8 (workgroup shape / occupancy experiments of the fused attention)")
    ap.add_argument("--H", type=int, default=None, help="override the number of heads (workgroups per launch: occupancy / rounds experiments)")
    ap.add_argument("--T", type=int, default=None, help="override the sequence length of every shape (fixed cost vs per-key-tile cost)")
    ap.add_argument("--build", default=None, help="library build: f16 = the IEEE-half build (default: bf16)")
    ap.add_argument("--dropout", type=float, default=None, help="time svt_debug_attention_dropout at this rate instead (--check then "
                    "compares with the unmasked softmax only at a rate of 2^-33 or below, which drops nothing)")
    a = ap.parse_args()
    lib = _lib.load(a.build)
    if a.wide is not None:
        lib.svt_debug_set(8, a.wide)
    dev = torch.device("cuda:0")
    dtype = torch.float16 if a.build == "f16" else torch.bfloat16
    st = torch.cuda.current_stream().cuda_stream
    for name, B, T, H, dh in SHAPES:
        if a.only and a.only not in name:
            continue
        if a.T:
            T = a.T
        if a.H:
            H = a.H
        D = H * dh
        g = torch.Generator().manual_seed(3)
        qkv = (torch.randn(B, T, 3 * D, generator=g) * 1.5).to(dev, dtype)
        out = torch.empty(B, T, D, device=dev, dtype=dtype)
        scale = dh ** -0.5

        desc = None
        if a.dropout is not None:
            desc = _lib.AttentionDropoutDescC()
            desc.struct_size, desc.precision = ctypes.sizeof(desc), 1
            desc.q, desc.k, desc.v, desc.o = qkv.data_ptr(), qkv.data_ptr() + 2 * D, qkv.data_ptr() + 4 * D, out.data_ptr()
            desc.ldq, desc.ldkv, desc.ldo, desc.batch, desc.t, desc.heads, desc.head_dim = 3 * D, 3 * D, D, B, T, H, dh
            desc.scale, desc.step, desc.p, desc.seed, desc.layer, desc.e0 = scale, 5, a.dropout, 7, 3, 0

        def call():
            if desc is not None:
                _lib.check(lib.svt_debug_attention_dropout(ctypes.byref(desc), 0, st), "svt_debug_attention_dropout")
                return
            _lib.check(lib.svt_debug_attention(1, qkv.data_ptr(), qkv.data_ptr() + 2 * D, qkv.data_ptr() + 4 * D, out.data_ptr(),
                                               B, T, H, dh, 3 * D, 3 * D, D, scale, 0, st), "svt_debug_attention")
        call()
        torch.cuda.synchronize()
        err = None
        if a.check and (a.dropout is None or a.dropout <= 2.0 ** -33):   # a real rate has no unmasked reference here
            nb = min(B, 2)
            q, k, v = [x.float().view(nb, T, H, dh).transpose(1, 2) for x in qkv[:nb].split(D, dim=-1)]
            ref = torch.softmax(q @ k.transpose(-1, -2) * scale, -1) @ v
            err = (out[:nb].float().view(nb, T, H, dh).transpose(1, 2) - ref).abs().max().item()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            call()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / a.iters * 1e3
        tf = 4.0 * B * H * T * T * dh / us / 1e6
        print(f"{name:6s} B={B:3d} T={T} H={H:2d} dh={dh:3d}: kernel {lib.svt_debug_set(38, 0)} {us:8.1f} us  {tf:7.1f} TFLOP/s"
              + (f"  max|err|={err:.3e}" if err is not None else ""), flush=True)


if __name__ == "__main__":
    main()
