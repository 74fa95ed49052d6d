"""Steps/s of the audio-visual training step (FusionTrainer.fit_batch: FusionRCA + head on frozen features) against the fusion +
head forward alone, at the recipe's shape (8 clips x 5 s: T1 = 249 audio frames, T2 = 250 video frames, D = 1024); HIP-event times of
each part of the step called alone (forward_train / head forward / objective / head gradients / backward / clip + update / refresh;
the objective includes its one stream sync); and the weight-gradient kernel's TFLOP/s on the step's five products against the fp32
MFMA peak (157.3 TFLOP/s, v_mfma_f32_32x32x2_f32).

    python tools/fusion_train_bench.py [--precision fp32,bf16] [--steps 10] [--warmup 3] [--json OUT]

One line of text per precision and, with --json, the numbers."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import svt_speechbrain_amd as S  # noqa: E402
from svt_speechbrain_amd import _lib  # noqa: E402
from svt_speechbrain_amd import training as TR  # noqa: E402

B, T1, T2, D = 8, 249, 250, 1024


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / steps


def run(prec, steps, warmup, dev):
    fusion = S.FusionRCA(precision=prec).to(dev)
    head = S.Linear(20, input_size=D).to(dev)
    g = torch.Generator().manual_seed(0)
    a = torch.randn(B, T1, D, generator=g).to(dev)
    v = torch.randn(B, T2, D, generator=g).to(dev)
    anno = torch.zeros(B, T1, 4, device=dev)
    anno[..., 2] = 4
    anno[..., 3] = 12
    lens = torch.ones(B, device=dev)
    tr = TR.FusionTrainer({"fusion": fusion, "head": head})

    def fwd():
        with torch.no_grad():
            head(fusion(a, v))

    ms_fwd = _time(fwd, steps, warmup)
    ms_step = _time(lambda: tr.fit_batch(a, v, lens, anno), steps, warmup)
    lib = _lib.load()
    slot = fusion._sync(dev)
    need = lib.svt_rca_train_workspace_bytes(slot.handle, B, T1)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.empty(B, T1, D, device=dev)
    dout = torch.randn(B, T1, D, device=dev) * 1e-3
    grads = [torch.empty_like(p) for p in tr._params]
    gp = tr._ptrs(grads)
    stream = _lib.stream_ptr(dev)

    def ftrain():
        _lib.check(lib.svt_rca_forward_train(slot.handle, _lib.ptr(a), T1, _lib.ptr(v), T2, B, _lib.ptr(out), _lib.ptr(ws), need, stream))

    def bwd():
        _lib.check(lib.svt_rca_backward(slot.handle, _lib.ptr(dout), B, T1, gp, _lib.ptr(ws), need, stream))

    parts = {"forward_train": _time(ftrain, steps, warmup), "backward": _time(bwd, steps, warmup)}
    on_t, off_t = anno[..., 0].contiguous(), anno[..., 1].contiguous()
    oct_t, cls_t = anno[..., 2].long().contiguous(), anno[..., 3].long().contiguous()
    logits = head(out)
    parts["head_forward"] = _time(lambda: head(out), steps, warmup)
    _, dlogits, _ = TR.amt_objective_grad(logits, on_t, off_t, oct_t, cls_t, lens)
    parts["objective"] = _time(lambda: TR.amt_objective_grad(logits, on_t, off_t, oct_t, cls_t, lens), steps, warmup)
    x2, d2 = out.reshape(-1, D), dlogits.reshape(-1, 20)
    parts["head_grads"] = _time(lambda: (TR.linear_backward(x2, d2), TR.linear_backward_data(d2, head.w.weight)), steps, warmup)
    opt = tr.optimizer

    def update():
        opt.step(max_norm=5.0)

    parts["clip_update"] = _time(update, steps, warmup)
    parts["refresh"] = _time(lambda: tr._refresh(lib, slot, dev), steps, warmup)
    # the weight gradient alone on the step's products (per layer: in-proj q rows over two segments, in-proj k/v, out-proj, W1, W2)
    rows = B * T1
    dt = torch.bfloat16 if prec == "bf16" else torch.float32
    shapes = [(2, D, D), (1, 2 * D, D), (1, D, D), (1, 3072, D), (1, D, 3072)]
    flop, ms_wg = 0.0, 0.0
    for segs, n_out, n_in in shapes:
        dys = [torch.randn(rows, n_out, device=dev) for _ in range(segs)]
        xs = [torch.randn(rows, n_in, device=dev).to(dt) for _ in range(segs)]
        dw = torch.empty(n_out, n_in, device=dev)
        db = torch.empty(n_out, device=dev)
        nb = C.c_size_t(0)

        def call(ws_p, nbp, dys=dys, xs=xs, dw=dw, db=db, n_out=n_out, n_in=n_in):
            two = len(dys) == 2
            return lib.svt_debug_rca_wgrad(1 if prec == "bf16" else 0, _lib.ptr(dys[0]), n_out, _lib.ptr(xs[0]),
                                           _lib.ptr(dys[1]) if two else None, n_out, _lib.ptr(xs[1]) if two else None, rows, n_out, n_in,
                                           _lib.ptr(dw), _lib.ptr(db), ws_p, nbp, 0, stream)

        _lib.check(call(None, C.byref(nb)))
        wsw = torch.empty(int(nb.value), dtype=torch.uint8, device=dev)
        ms_wg += _time(lambda call=call, wsw=wsw, nb=nb: _lib.check(call(_lib.ptr(wsw), C.byref(nb))), steps, warmup)
        flop += 2.0 * segs * rows * n_out * n_in
    tflops = flop / (ms_wg * 1e-3) / 1e12
    r = {"precision": prec, "batch": B, "t_audio": T1, "t_video": T2, "steps_per_s": 1000.0 / ms_step,
         "forward_only_per_s": 1000.0 / ms_fwd, "ms_step": ms_step, "ms_forward_only": ms_fwd,
         "ms_parts": parts, "weight_grad": {"ms_per_layer": ms_wg, "tflops": tflops, "peak_tflops": 157.3, "frac": tflops / 157.3}}
    print(f"{prec}: step {ms_step:.2f} ms ({r['steps_per_s']:.1f} steps/s) vs fusion + head forward alone {ms_fwd:.2f} ms; "
          + ", ".join(f"{k} {v:.3f} ms" for k, v in parts.items())
          + f"; weight gradient {ms_wg:.3f} ms per layer at {tflops:.1f} TFLOP/s = {100 * tflops / 157.3:.1f} % of the fp32 MFMA peak",
          flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="fp32,bf16")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = [run(p, args.steps, args.warmup, dev) for p in args.precision.split(",")]
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
