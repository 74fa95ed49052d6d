"""The linear-probe stage of the recipes on the GPU: ``AMT.fit_batch`` with the wav2vec2 encoder frozen and only the 20-way
``Linear`` head learning (``MIR_ST500/train_audio_ssl.py:192-199``, the first ``linear_prob_epochs``; the whole run with
``freeze_wav2vec: True``).

One step is the frozen encoder forward (the existing hot path), the head forward, then three HIP kernels of ``csrc/train.hip``:
the recipe's objective and its gradient w.r.t. the logits in one pass (``compute_objectives``, ``train_audio_ssl.py:50-76``), the head's
weight gradient, and ``Brain.check_gradients``' clip (``speechbrain/core.py:882-923``) fused with ``torch.optim.Adadelta``'s update.
Nothing is computed by torch and there is no CPU fallback.  The encoder's backward (full fine-tuning) is out of scope.

``FusionTrainer`` is the audio-visual recipe's step (``N20EMv2/audio_visual/train_rca_av.py:174-185``): ``FusionRCA`` + the head on
precomputed, frozen audio and video features, with the RCA layers' backward of ``csrc/train_rca.hip``.

``VideoProbe`` is the video recipe's linear-probe step (``N20EMv2/video_only/train_video_ssl.py``): ``LinearProbe`` behind the frozen
AV-HuBERT encoder on raw uint8 lip ROIs, with the recipe's ``transform_train`` drawn on the host and applied in the padding kernel.

``Adam`` / ``AdamW`` are the recipes' second optimizer class (``wav2vec_opt_class`` / ``encoder_opt_class: torch.optim.Adam``): the
clip and torch's single-tensor update for a parameter list of any length in one call of ``svt_clip_adam_step`` (``csrc/adam.hip``).
The three trainers take one as ``optimizer=``; their default stays ``Adadelta``.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional

import torch

from . import _lib
from .amt import AMTForward

TERMS = ("onset", "offset", "octave", "pitch")
_MAX_TENSORS = 32   # tensors per svt_clip_adadelta_step call (csrc/common.h kAdaMaxTensors)
ADAM_MAXIMIZE, ADAM_AMSGRAD, ADAM_DECOUPLED = 1, 2, 4   # svt_clip_adam_step's flags (include/svt_mi355.h)


def _workspace(query, device) -> torch.Tensor:
    """Run a size query (a call with workspace NULL) and allocate that many bytes on ``device``."""
    n = C.c_size_t(0)
    query(n)
    return torch.empty(max(16, int(n.value)), dtype=torch.uint8, device=device)


def _bump(t) -> None:
    """A kernel wrote ``t`` (a tensor or a list of tensors) through its pointer: advance its version counter so every cached upload of
    it (``Linear._sync``, the fused tail) sees a change."""
    torch.autograd.graph.increment_version(t)


def clip_adadelta_step(params, grads, square_avgs, acc_deltas, lr: float, rho: float, eps: float, weight_decay: float = 0.0,
                       maximize: bool = False, max_norm: float = 0.0, total_norm: Optional[torch.Tensor] = None) -> None:
    """``clip_grad_norm_(grads, max_norm)`` (when ``max_norm > 0``) then one Adadelta update of every parameter, in one call of
    ``svt_clip_adadelta_step``.  All tensors contiguous fp32 on one GPU; ``total_norm`` (0-d fp32 on that GPU) receives the pre-clip
    norm."""
    if len(params) > _MAX_TENSORS:
        raise _lib.SvtError(f"clip_adadelta_step: at most {_MAX_TENSORS} tensors per call")
    dev = params[0].device
    for group in (params, grads, square_avgs, acc_deltas):
        for t in group:
            if not t.is_cuda:
                raise _lib.SvtError("Adadelta needs its parameters on the GPU; there is no CPU fallback")
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
                raise _lib.SvtError("Adadelta: parameters, gradients and state must be contiguous fp32 tensors on one device")
    lib = _lib.load()
    n = len(params)
    arr = C.c_void_p * n
    pp, gg, ss, aa = (arr(*[_lib.ptr(t) for t in g]) for g in (params, grads, square_avgs, acc_deltas))
    numels = (C.c_int64 * n)(*[t.numel() for t in params])
    idx, stream = _lib.dev_index(dev), _lib.stream_ptr(dev)

    def call(ws, nbytes):
        return lib.svt_clip_adadelta_step(n, pp, gg, ss, aa, numels, float(lr), float(rho), float(eps), float(weight_decay), int(maximize),
                                          float(max_norm), _lib.ptr(total_norm) if total_norm is not None else None, ws, nbytes, idx,
                                          stream)

    ws = _workspace(lambda nb: _lib.check(call(None, nb), "svt_clip_adadelta_step"), dev)
    nbytes = C.c_size_t(ws.numel())
    _lib.check(call(_lib.ptr(ws), C.byref(nbytes)), "svt_clip_adadelta_step")
    for t in params:
        _bump(t)
    if max_norm > 0:
        for t in grads:
            _bump(t)


def clip_adam_step(params, grads, exp_avgs, exp_avg_sqs, max_exp_avg_sqs, step_sizes, bc2_sqrts, lr: float, beta1: float, beta2: float,
                   eps: float, weight_decay: float = 0.0, maximize: bool = False, decoupled_weight_decay: bool = False,
                   max_norm: float = 0.0, total_norm: Optional[torch.Tensor] = None, workspace=None, validate: bool = True) -> None:
    """``clip_grad_norm_(grads, max_norm)`` (when ``max_norm > 0``) then one ``torch.optim.Adam`` update of every parameter, in one call
    of ``svt_clip_adam_step`` (``csrc/adam.hip``) -- any number of tensors.  ``max_exp_avg_sqs`` is None without amsgrad; ``step_sizes``
    (``lr / (1 - beta1**step)``) and ``bc2_sqrts`` (``sqrt(1 - beta2**step)``) are Python floats per tensor.  All tensors contiguous fp32
    on one GPU (views into a flat buffer are fine: any 4-byte-aligned address); ``total_norm`` (0-d fp32 on that GPU) receives the
    pre-clip norm.  ``workspace`` (a callable ``query -> uint8 tensor``) lets the caller keep the scratch between steps;
    ``validate=False`` is for a caller that has checked the tensors itself (``Adam.step``: the checks cost host time per tensor)."""
    dev = params[0].device
    groups = [params, grads, exp_avgs, exp_avg_sqs] + ([max_exp_avg_sqs] if max_exp_avg_sqs is not None else [])
    n = len(params)
    for group in groups if validate else ():
        if len(group) != n:
            raise ValueError("clip_adam_step: the tensor lists differ in length")
        for t, p in zip(group, params):
            if not t.is_cuda:
                raise _lib.SvtError("Adam needs its parameters on the GPU; there is no CPU fallback")
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
                raise _lib.SvtError("Adam: parameters, gradients and state must be contiguous fp32 tensors on one device")
            if t.numel() != p.numel():
                raise ValueError("clip_adam_step: a gradient or state tensor differs in size from its parameter")
    lib = _lib.load()
    arr = C.c_void_p * n
    ptrs = [arr(*[t.data_ptr() for t in g]) for g in groups]
    vmax = ptrs[4] if max_exp_avg_sqs is not None else None
    numels = (C.c_int64 * n)(*[t.numel() for t in params])
    ss = (C.c_float * n)(*step_sizes)
    bc = (C.c_float * n)(*bc2_sqrts)
    flags = (ADAM_MAXIMIZE if maximize else 0) | (ADAM_AMSGRAD if max_exp_avg_sqs is not None else 0) | \
        (ADAM_DECOUPLED if decoupled_weight_decay else 0)
    idx, stream = _lib.dev_index(dev), _lib.stream_ptr(dev)

    def call(ws, nbytes):
        return lib.svt_clip_adam_step(n, ptrs[0], ptrs[1], ptrs[2], ptrs[3], vmax, numels, ss, bc, float(lr), float(beta1), float(beta2),
                                      float(eps), float(weight_decay), flags, float(max_norm),
                                      _lib.ptr(total_norm) if total_norm is not None else None, ws, nbytes, idx, stream)

    def query(nb):
        _lib.check(call(None, nb), "svt_clip_adam_step")

    ws = workspace(query) if workspace is not None else _workspace(query, dev)
    nbytes = C.c_size_t(ws.numel())
    _lib.check(call(_lib.ptr(ws), C.byref(nbytes)), "svt_clip_adam_step")
    _bump(params)
    if max_norm > 0:
        _bump(grads)


def amt_objective_grad(logits, onset, offset, octave, pitch_class, rel_len=None, onset_pos_weight: float = 15.0,
                       pitch_octave_num: int = 4, allowed_len_diff: int = 3, label_smoothing: float = 0.0, workspace=None):
    """The recipe's objective and its gradient (``svt_amt_objective_grad``): ``logits`` (B, T, n_out) fp32 on the GPU, targets
    (B, T') -- onset / offset float, octave / class int64 (-100 ignored) -- and relative lengths (B,) or None.  Returns
    ``(terms, dlogits, host)``: ``terms`` the device (5,) {onset, offset, octave, pitch, sum}, ``dlogits`` d(sum)/d(logits), ``host``
    the five terms as Python floats.  Raises ``ValueError`` for a length difference beyond ``allowed_len_diff`` (the reference's
    message) and ``SvtError`` for every other refusal (n_out > 32, a target out of range, ...)."""
    if not logits.is_cuda:
        raise _lib.SvtError("amt_objective_grad needs GPU tensors; there is no CPU fallback")
    lib = _lib.load()
    dev = logits.device
    idx, stream = _lib.dev_index(dev), _lib.stream_ptr(dev)
    x = logits.detach().to(torch.float32).contiguous()
    if x.dim() != 3:
        raise ValueError(f"logits must be (batch, frames, n_out), got {tuple(x.shape)}")
    B, tp, n_out = x.shape
    on_t = onset.detach().to(device=dev, dtype=torch.float32).contiguous()
    off_t = offset.detach().to(device=dev, dtype=torch.float32).contiguous()
    oct_t = octave.detach().to(device=dev, dtype=torch.int64).contiguous()
    cls_t = pitch_class.detach().to(device=dev, dtype=torch.int64).contiguous()
    tt = on_t.shape[1]
    for t in (on_t, off_t, oct_t, cls_t):
        if t.shape != (B, tt):
            raise ValueError(f"targets must all be (batch, frames) = ({B}, {tt}), got {tuple(t.shape)}")
    ln = None
    if rel_len is not None:
        ln = torch.as_tensor(rel_len, dtype=torch.float32, device=dev).reshape(-1).contiguous()
        if ln.numel() != B:
            raise ValueError(f"rel_len has {ln.numel()} entries for a batch of {B}")
    terms = torch.empty(5, dtype=torch.float32, device=dev)
    dlogits = torch.empty_like(x)
    host = (C.c_float * 5)()

    def call(ws, nbytes):
        return lib.svt_amt_objective_grad(_lib.ptr(x), B, tp, n_out, int(pitch_octave_num), _lib.ptr(on_t), _lib.ptr(off_t),
                                          _lib.ptr(oct_t), _lib.ptr(cls_t), tt, _lib.ptr(ln) if ln is not None else None,
                                          float(onset_pos_weight), int(allowed_len_diff), float(label_smoothing), _lib.ptr(terms), host,
                                          _lib.ptr(dlogits), ws, nbytes, idx, stream)

    def query(nb):
        _lib.check(call(None, nb), "svt_amt_objective_grad")

    ws = workspace(query) if workspace is not None else _workspace(query, dev)
    nb = C.c_size_t(ws.numel())
    rc = call(_lib.ptr(ws), C.byref(nb))
    if rc != 0:
        msg = _lib.last_error()
        if "same length" in msg:
            raise ValueError(msg)   # speechbrain.nnet.losses.truncate's error
        _lib.check(rc, "svt_amt_objective_grad")
    return terms, dlogits, [float(v) for v in host]


def linear_backward(x: torch.Tensor, dy: torch.Tensor, dweight: Optional[torch.Tensor] = None, dbias: Optional[torch.Tensor] = None,
                    with_bias: bool = True, workspace=None):
    """``svt_linear_backward``: dweight = dy^T x (out, in) and dbias = dy summed over rows, for x (rows, in) and dy (rows, out)
    fp32 on the GPU.  Writes into ``dweight`` / ``dbias`` when given (contiguous fp32), else allocates; returns both."""
    if not x.is_cuda:
        raise _lib.SvtError("linear_backward needs GPU tensors; there is no CPU fallback")
    lib = _lib.load()
    dev = x.device
    xx = x.detach().to(torch.float32).contiguous()
    dd = dy.detach().to(device=dev, dtype=torch.float32).contiguous()
    rows, d_in = xx.shape
    d_out = dd.shape[1]
    if dd.shape[0] != rows:
        raise ValueError(f"x has {rows} rows, dy {dd.shape[0]}")
    if dweight is None:
        dweight = torch.empty((d_out, d_in), dtype=torch.float32, device=dev)
    if dbias is None and with_bias:
        dbias = torch.empty((d_out,), dtype=torch.float32, device=dev)
    idx, stream = _lib.dev_index(dev), _lib.stream_ptr(dev)

    def call(ws, nbytes):
        return lib.svt_linear_backward(_lib.ptr(xx), _lib.ptr(dd), rows, d_in, d_out, _lib.ptr(dweight),
                                       _lib.ptr(dbias) if dbias is not None else None, ws, nbytes, idx, stream)

    def query(nb):
        _lib.check(call(None, nb), "svt_linear_backward")

    ws = workspace(query) if workspace is not None else _workspace(query, dev)
    nb = C.c_size_t(ws.numel())
    _lib.check(call(_lib.ptr(ws), C.byref(nb)), "svt_linear_backward")
    return dweight, dbias


def linear_backward_data(dy: torch.Tensor, weight: torch.Tensor, dx: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``svt_linear_backward_data``: dx (rows, in) = dy (rows, out) weight (out, in), fp32 on the GPU."""
    if not (dy.is_cuda and weight.is_cuda):
        raise _lib.SvtError("linear_backward_data needs GPU tensors; there is no CPU fallback")
    lib = _lib.load()
    dev = dy.device
    dd = dy.detach().to(torch.float32).contiguous()
    w = weight.detach().to(device=dev, dtype=torch.float32).contiguous()
    rows, d_out = dd.shape
    if w.shape[0] != d_out:
        raise ValueError(f"dy has {d_out} columns, weight {w.shape[0]} rows")
    if dx is None:
        dx = torch.empty((rows, w.shape[1]), dtype=torch.float32, device=dev)
    _lib.check(lib.svt_linear_backward_data(_lib.ptr(dd), _lib.ptr(w), rows, w.shape[1], d_out, _lib.ptr(dx), _lib.dev_index(dev),
                                            _lib.stream_ptr(dev)), "svt_linear_backward_data")
    return dx


class Adadelta(torch.optim.Optimizer):
    """``torch.optim.Adadelta`` on GPU parameters, updated by a HIP kernel: same constructor, same ``param_groups`` and the same
    ``state_dict()`` (per parameter ``step``, ``square_avg``, ``acc_delta``), so a checkpoint moves both ways and a scheduler that sets
    ``param_groups[i]["lr"]`` (SpeechBrain's ``NewBobScheduler``) works unchanged.  fp32 parameters only; CPU parameters raise
    ``SvtError``."""

    def __init__(self, params, lr=1.0, rho=0.9, eps=1e-6, weight_decay=0, foreach=None, *, capturable=False, maximize=False,
                 differentiable=False):
        if isinstance(lr, torch.Tensor) and lr.numel() != 1:
            raise ValueError("Tensor lr must be 1-element")
        if not 0.0 <= float(lr):
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= rho <= 1.0:
            raise ValueError(f"Invalid rho value: {rho}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if differentiable:
            raise NotImplementedError("Adadelta: differentiable=True is not provided (the update is a HIP kernel)")
        defaults = dict(lr=lr, rho=rho, eps=eps, weight_decay=weight_decay, maximize=maximize, capturable=capturable, foreach=foreach,
                        differentiable=differentiable)
        super().__init__(params, defaults)

    def _group_tensors(self, group):
        params, grads, sqs, accs = [], [], [], []
        for p in group["params"]:
            if p.grad is None:
                continue
            if p.grad.is_sparse:
                raise RuntimeError("Adadelta does not support sparse gradients")
            if not p.is_cuda:
                raise _lib.SvtError("svt_speechbrain_amd.Adadelta needs its parameters on the GPU; there is no CPU fallback")
            state = self.state[p]
            if len(state) == 0:
                state["step"] = torch.tensor(0.0, dtype=torch.float32)
                state["square_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                state["acc_delta"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            params.append(p)
            grads.append(p.grad if p.grad.is_contiguous() else p.grad.contiguous())
            sqs.append(state["square_avg"])
            accs.append(state["acc_delta"])
        return params, grads, sqs, accs

    @torch.no_grad()
    def step(self, closure=None, max_norm: float = 0.0, total_norm: Optional[torch.Tensor] = None):
        """One Adadelta update.  ``max_norm > 0`` (extension) first clips the gradients of ALL parameters of the optimizer by their
        global norm as ``clip_grad_norm_`` does, in the same kernel call (one param group of at most 32 tensors)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if max_norm > 0 and len(self.param_groups) != 1:
            raise NotImplementedError("Adadelta.step(max_norm=...): one param group only")
        for group in self.param_groups:
            params, grads, sqs, accs = self._group_tensors(group)
            if not params:
                continue
            if max_norm > 0 and len(params) > _MAX_TENSORS:
                raise NotImplementedError(f"Adadelta.step(max_norm=...): at most {_MAX_TENSORS} parameters")
            for p in params:
                self.state[p]["step"] += 1
            lr = float(group["lr"])
            for i in range(0, len(params), _MAX_TENSORS):
                sl = slice(i, i + _MAX_TENSORS)
                clip_adadelta_step(params[sl], grads[sl], sqs[sl], accs[sl], lr, group["rho"], group["eps"], group["weight_decay"],
                                   group["maximize"], max_norm, total_norm)
        return loss


class Adam(torch.optim.Optimizer):
    """``torch.optim.Adam`` on GPU parameters, updated by the HIP kernels of ``csrc/adam.hip``: the installed torch's constructor,
    validation and messages, the same ``param_groups`` keys and the same ``state_dict()`` (per parameter ``step`` -- a 0-d fp32 CPU tensor
    --, ``exp_avg``, ``exp_avg_sq`` and, with amsgrad, ``max_exp_avg_sq``), so a checkpoint moves both ways and a scheduler that sets
    ``param_groups[i]["lr"]`` works unchanged.  Any number of parameters per call.  ``foreach`` / ``fused`` / ``capturable`` are accepted
    and stored, and change nothing: there is one implementation.  fp32 parameters only; CPU parameters raise ``SvtError``."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None, maximize=False,
                 capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        Tensor = torch.Tensor
        if isinstance(lr, Tensor):
            if foreach and not capturable:
                raise ValueError("lr as a Tensor is not supported for capturable=False and foreach=True")
            if lr.numel() != 1:
                raise ValueError("Tensor lr must be 1-element")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if not ((isinstance(betas[0], float) and isinstance(betas[1], float))
                or (isinstance(betas[0], Tensor) and isinstance(betas[1], Tensor))):
            raise ValueError("betas must be either both floats or both Tensors")
        for i in (0, 1):
            if isinstance(betas[i], Tensor):
                if not capturable and foreach:
                    raise ValueError(f"betas[{i}] as a Tensor is not supported for capturable=False and foreach=True")
                if betas[i].numel() != 1:
                    raise ValueError(f"Tensor betas[{i}] must be 1-element")
        betas = tuple(b.item() if isinstance(b, Tensor) else b for b in betas)
        if differentiable:
            raise NotImplementedError(f"{type(self).__name__}: differentiable=True is not provided (the update is a HIP kernel)")
        if fused and foreach:
            raise RuntimeError("`fused` and `foreach` cannot be `True` together.")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=foreach,
                        capturable=capturable, differentiable=differentiable, fused=fused, decoupled_weight_decay=decoupled_weight_decay)
        super().__init__(params, defaults)
        self._ws: Dict[torch.device, torch.Tensor] = {}
        self._seen: dict = {}         # parameter -> the state tensors that were checked (_group_tensors)
        self._step_views: dict = {}   # id(step tensor) -> (the tensor, its numpy view) (_advance)

    def __setstate__(self, state):
        super().__setstate__(state)
        for name in ("_ws", "_seen", "_step_views"):   # not part of the pickled state
            self.__dict__[name] = {}
        for group in self.param_groups:
            group.setdefault("amsgrad", False)
            group.setdefault("maximize", False)
            group.setdefault("foreach", None)
            group.setdefault("capturable", False)
            group.setdefault("differentiable", False)
            group.setdefault("decoupled_weight_decay", False)
            group.setdefault("fused", None)
            for p in group["params"]:
                p_state = self.state.get(p, [])
                if len(p_state) != 0 and not torch.is_tensor(p_state["step"]):
                    p_state["step"] = torch.tensor(float(p_state["step"]), dtype=torch.float32)

    def _scratch(self, query, device) -> torch.Tensor:
        n = C.c_size_t(0)
        query(n)
        ws = self._ws.get(device)
        if ws is None or ws.numel() < int(n.value):
            ws = torch.empty(max(16, int(n.value)), dtype=torch.uint8, device=device)
            self._ws[device] = ws
        return ws

    def _group_tensors(self, group):
        """The tensors of the parameters that have a gradient, checked: parameters and gradients at every step, the state tensors when
        they are first seen (``_seen`` keeps them by identity, so a state replaced by ``load_state_dict`` or by hand is checked again)."""
        params, grads, avgs, sqs, maxs, steps = [], [], [], [], [], []
        name, ams, seen, dev, f32 = type(self).__name__, group["amsgrad"], self._seen, None, torch.float32
        for p in group["params"]:
            g = p.grad
            if g is None:
                continue
            if g.is_sparse:
                raise RuntimeError("Adam does not support sparse gradients, please consider SparseAdam instead")
            if not p.is_cuda:
                raise _lib.SvtError(f"svt_speechbrain_amd.{name} needs its parameters on the GPU; there is no CPU fallback")
            if dev is None:
                dev = p.device
            if not g.is_contiguous():
                g = g.contiguous()
            if p.dtype is not f32 or g.dtype is not f32 or not p.is_contiguous() or p.device != dev or g.device != dev or g.numel() != p.numel():
                raise _lib.SvtError(f"{name}: parameters and gradients must be contiguous fp32 tensors of equal size on one device")
            state = self.state[p]
            if len(state) == 0:
                state["step"] = torch.tensor(0.0, dtype=torch.float32)
                state["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                if ams:
                    state["max_exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            m, v, x = state["exp_avg"], state["exp_avg_sq"], state["max_exp_avg_sq"] if ams else None
            was = seen.get(p)
            if was is None or was[0] is not m or was[1] is not v or was[2] is not x:
                for t in (m, v) + ((x,) if ams else ()):
                    if t.dtype is not f32 or not t.is_contiguous() or t.device != dev or t.numel() != p.numel():
                        raise _lib.SvtError(f"{name}: the state of a parameter must be contiguous fp32 tensors of its size on its device")
                seen[p] = (m, v, x)
            params.append(p)
            grads.append(g)
            avgs.append(m)
            sqs.append(v)
            if ams:
                maxs.append(x)
            steps.append(state["step"])
        return params, grads, avgs, sqs, maxs, steps

    def _advance(self, steps):
        """``step += 1`` of every 0-d fp32 step tensor and its new value as a Python float.  A CPU step tensor is written through a numpy
        view kept by identity: 400 tensor operations a step cost more host time than the kernels take."""
        views, out = self._step_views, []
        for st in steps:
            v = views.get(id(st))
            if v is None or v[0] is not st:
                if st.device.type != "cpu" or st.dtype is not torch.float32:   # a state loaded from a fused / capturable torch optimizer
                    st += 1
                    out.append(float(st))
                    continue
                v = views[id(st)] = (st, st.numpy())
            k = float(v[1]) + 1.0
            v[1][()] = k
            out.append(k)
        return out

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._seen.clear()
        self._step_views.clear()

    @torch.no_grad()
    def step(self, closure=None, max_norm: float = 0.0, total_norm: Optional[torch.Tensor] = None):
        """One Adam update.  ``max_norm > 0`` (extension) first clips the gradients of ALL parameters of the optimizer by their global
        norm as ``clip_grad_norm_`` does, in the same kernel call (one param group, any number of tensors).  Parameters whose ``grad``
        is None are skipped and keep their ``step``; the bias corrections are therefore formed per parameter, in double, as torch's
        single-tensor path forms them."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if max_norm > 0 and len(self.param_groups) != 1:
            raise NotImplementedError(f"{type(self).__name__}.step(max_norm=...): one param group only")
        for group in self.param_groups:
            params, grads, avgs, sqs, maxs, steps = self._group_tensors(group)
            if not params:
                continue
            beta1, beta2 = (float(b) for b in group["betas"])
            lr = float(group["lr"])
            ks = self._advance(steps)
            bias = {k: (lr / (1 - beta1 ** k), (1 - beta2 ** k) ** 0.5) for k in set(ks)}
            dev = params[0].device
            clip_adam_step(params, grads, avgs, sqs, maxs if group["amsgrad"] else None, [bias[k][0] for k in ks], [bias[k][1] for k in ks],
                           lr, beta1, beta2, group["eps"], group["weight_decay"], group["maximize"], group["decoupled_weight_decay"],
                           max_norm, total_norm, workspace=lambda q: self._scratch(q, dev), validate=False)
        return loss


class AdamW(Adam):
    """``torch.optim.AdamW``: ``Adam`` with ``decoupled_weight_decay=True`` and torch's default ``weight_decay=1e-2``."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False, foreach=None,
                 capturable=False, differentiable=False, fused=None):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, foreach=foreach, maximize=maximize, capturable=capturable,
                         differentiable=differentiable, fused=fused, decoupled_weight_decay=True)

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            group["decoupled_weight_decay"] = True


class LinearProbe:
    """``AMT.fit_batch`` of the linear-probe stage with the encoder frozen (``train_audio_ssl.py:28-76`` + ``Brain.fit_batch`` /
    ``check_gradients``, ``speechbrain/core.py:850-923``).  ``modules`` is the recipe's mapping (``wav2vec2`` + ``model``, as for
    ``AMTForward``); the hparams carry the recipe's names.  The head, its gradients and the optimizer state are fp32 whatever the
    encoder's ``precision``.

    After ``fit_batch`` / ``fit_features``: ``head.w.weight.grad`` / ``.bias.grad`` hold the (clipped) gradients the step used,
    ``last_terms`` the four loss terms, ``last_grad_norm`` the pre-clip norm, and ``head.state_dict()`` the new parameters (every later
    ``head(...)`` or fused tail uploads them).  A non-finite loss skips the step (gradients set to None, parameters untouched); the
    ``nonfinite_patience + 1``-th skip since ``on_epoch_start()`` raises ``ValueError``, as ``check_gradients`` does."""

    def __init__(self, modules, optimizer: Optional[torch.optim.Optimizer] = None, lr: float = 3e-4, rho: float = 0.95, eps: float = 1e-8,
                 onset_positive_weight: float = 15.0, pitch_octave_num: int = 4, pitch_class_num: int = 12, max_grad_norm: float = 5.0,
                 nonfinite_patience: int = 3, allowed_len_diff: int = 3, label_smoothing: float = 0.0):
        self.amt = AMTForward(modules, pitch_octave_num=pitch_octave_num, pitch_class_num=pitch_class_num)
        self.head = self.amt._head(False)
        self.onset_positive_weight = float(onset_positive_weight)
        self.pitch_octave_num = int(pitch_octave_num)
        self.pitch_class_num = int(pitch_class_num)
        self.max_grad_norm = float(max_grad_norm)
        self.nonfinite_patience = int(nonfinite_patience)
        self.allowed_len_diff = int(allowed_len_diff)
        self.label_smoothing = float(label_smoothing)
        if optimizer is None:
            optimizer = Adadelta(self.head.parameters(), lr=lr, rho=rho, eps=eps)
        if not isinstance(optimizer, (Adadelta, Adam)):
            raise TypeError("LinearProbe needs svt_speechbrain_amd.training.Adadelta, Adam or AdamW (the clip is fused into their kernels)")
        self.optimizer = optimizer
        self.nonfinite_count = 0
        self.last_terms: Dict[str, float] = {}
        self.last_grad_norm: Optional[torch.Tensor] = None
        self._ws: Dict[tuple, torch.Tensor] = {}

    def on_epoch_start(self) -> None:
        """Reset the non-finite counter, as ``Brain`` does at the start of every epoch (``core.py`` ``_fit_train``)."""
        self.nonfinite_count = 0

    def _scratch(self, key, query, device) -> torch.Tensor:
        n = C.c_size_t(0)
        query(n)
        ws = self._ws.get(key)
        if ws is None or ws.numel() < int(n.value) or ws.device != device:
            ws = torch.empty(max(16, int(n.value)), dtype=torch.uint8, device=device)
            self._ws[key] = ws
        return ws

    def fit_batch(self, wavs: torch.Tensor, wav_lens: Optional[torch.Tensor], anno: torch.Tensor,
                  anno_lens: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One training step from waveforms: the frozen encoder, then ``fit_features``.  An encoder built with
        ``apply_spec_augment=True, freeze=False`` (weights untouched by this step, model in training mode) draws and applies its
        SpecAugment masks inside that call -- one time-mask draw (and one feature-mask draw when its probability is above 0) per
        step, nothing to do here (tests/test_gpu_spec_augment.py checks the draws and the loss terms).  The same holds for the
        checkpoint's dropouts and layerdrop of a ``freeze=False`` encoder: they run inside the module's forward, one layerdrop draw per
        layer and one ``dropout_step`` per step (tests/test_gpu_encoder_dropout.py checks the loss against ``encoder.forward`` at the
        same seed and step)."""
        with torch.no_grad():
            feats = self.amt._get("wav2vec2")(wavs)
        return self.fit_features(feats, wav_lens, anno, anno_lens)

    def fit_features(self, feats: torch.Tensor, wav_lens: Optional[torch.Tensor], anno: torch.Tensor,
                     anno_lens: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One training step from the frozen encoder's output (B, T, D), e.g. features saved by ``song.save_song_features``.
        ``anno`` (B, T', 4): onset, offset, octave, pitch class per frame (``batch.anno``); the mask is ``wav_lens`` as in
        ``compute_objectives`` (``anno_lens`` is accepted for the recipe's signature and not used there either).  Returns the
        detached 0-d loss on the CPU, as ``Brain.fit_batch``."""
        if not feats.is_cuda:
            raise _lib.SvtError("LinearProbe needs its features on the GPU; there is no CPU fallback")
        head = self.head
        dev = feats.device
        x = feats.detach().to(torch.float32).contiguous()
        if x.dim() != 3 or x.shape[-1] != head.w.in_features:
            raise ValueError(f"features must be (batch, frames, {head.w.in_features}), got {tuple(x.shape)}")
        B, tp, D = x.shape
        logits = head(x)
        n_out = logits.shape[-1]
        a = anno.to(dev)
        if a.dim() != 3 or a.shape[0] != B or a.shape[2] < 4:
            raise ValueError(f"anno must be (batch, frames, 4), got {tuple(anno.shape)}")
        on_t = a[:, :, 0].to(torch.float32).contiguous()
        off_t = a[:, :, 1].to(torch.float32).contiguous()
        oct_t = a[:, :, 2].to(torch.int64).contiguous()
        cls_t = a[:, :, 3].to(torch.int64).contiguous()
        tt = a.shape[1]
        ln = None
        if wav_lens is not None:
            ln = torch.as_tensor(wav_lens, dtype=torch.float32, device=dev).reshape(-1).contiguous()
            if ln.numel() != B:
                raise ValueError(f"wav_lens has {ln.numel()} entries for a batch of {B}")
        terms, dlogits, host = amt_objective_grad(logits, on_t, off_t, oct_t, cls_t, ln, self.onset_positive_weight,
                                                  self.pitch_octave_num, self.allowed_len_diff, self.label_smoothing,
                                                  workspace=lambda q: self._scratch("obj", q, dev))
        self.last_terms = dict(zip(TERMS, host[:4]))
        loss = terms[4]
        if not math.isfinite(float(host[4])):
            # Brain.check_gradients: skip the step, count it, raise once the patience is spent
            self.nonfinite_count += 1
            head.w.weight.grad = None
            if head.w.bias is not None:
                head.w.bias.grad = None
            if self.nonfinite_count > self.nonfinite_patience:
                raise ValueError("Loss is not finite and patience is exhausted. To debug, wrap `fit()` with autograd's "
                                 "`detect_anomaly()`, e.g.\n\nwith torch.autograd.detect_anomaly():\n\tbrain.fit(...)")
            return loss.detach().cpu()
        w, b = head.w.weight, head.w.bias
        if w.grad is None or w.grad.shape != w.shape or not w.grad.is_contiguous():
            w.grad = torch.empty_like(w, memory_format=torch.contiguous_format)
        if b is not None and (b.grad is None or b.grad.shape != b.shape):
            b.grad = torch.empty_like(b)

        linear_backward(x.reshape(B * tp, D), dlogits.reshape(B * tp, n_out), w.grad, b.grad if b is not None else None,
                        workspace=lambda q: self._scratch("wgrad", q, dev))
        _bump(w.grad)
        if b is not None:
            _bump(b.grad)
        self.last_grad_norm = torch.empty((), dtype=torch.float32, device=dev)
        self.optimizer.step(max_norm=self.max_grad_norm, total_norm=self.last_grad_norm)
        return loss.detach().cpu()


class VideoProbe(LinearProbe):
    """``AMT.fit_batch`` of the video recipe with the AV-HuBERT encoder frozen (``N20EMv2/video_only/train_video_ssl.py:27-49``: the
    ``linear_prob_epochs`` stage, or ``freeze_encoder: True``): ``modules`` is the recipe's mapping, ``encoder``
    (``FairseqAVHubertPretrain``) + ``head``.  A step draws the batch's ``transform_train`` parameters on the host in the reference's
    order (``TrainTransform.plan``), runs the frozen encoder on the RAW uint8 lip ROIs -- crop, flip, pixel map and the zero padding of
    the ragged batch inside the front-end's padding kernel -- and then ``LinearProbe.fit_features``.  ``last_clips`` keeps the draws of
    the last step.  The offset term carries no positive weight (the recipe's ``offset_positive_weight: 1.0``)."""

    def __init__(self, modules, transform=None, **hparams):
        super().__init__(modules, **hparams)
        from .video import TrainTransform
        self.transform = transform if transform is not None else TrainTransform()
        self.last_clips = []

    def fit_batch(self, rois, lens: Optional[torch.Tensor], anno: torch.Tensor, anno_lens: Optional[torch.Tensor] = None,
                  transform=None) -> torch.Tensor:
        """One training step from lip ROIs: ``rois`` a list of ``(T_i, H, W)`` uint8 clips (padded here; ``lens`` None takes
        ``T_i / max T``, the relative lengths ``PaddedBatch`` would give) or an already padded ``(B, T, H, W)`` uint8 tensor with the
        relative ``lens`` (clip ``b`` has ``round(lens[b] * T)`` real frames; None: all ``T``).  ``lens`` also masks the objective, as
        ``video_lens`` does in ``compute_objectives``."""
        from .video import pad_roi_batch
        tf = transform if transform is not None else self.transform
        if isinstance(rois, (list, tuple)):
            roi, n_frames = pad_roi_batch(list(rois))
            if lens is None:
                lens = torch.tensor([n / roi.shape[1] for n in n_frames], dtype=torch.float32)
        else:
            roi = rois
            if roi.dtype != torch.uint8 or roi.dim() != 4:
                raise ValueError(f"expected a list of (T, H, W) uint8 clips or a padded (B, T, H, W) uint8 tensor, got {tuple(roi.shape)} {roi.dtype}")
            T = roi.shape[1]
            if lens is None:
                n_frames = [T] * roi.shape[0]
            else:
                n_frames = [int(round(float(l) * T)) for l in torch.as_tensor(lens).reshape(-1).tolist()]
        if not roi.is_cuda:
            raise _lib.SvtError("VideoProbe needs its lip ROIs on the GPU; there is no CPU fallback")
        self.last_clips = tf.plan(n_frames, roi.shape[-2], roi.shape[-1])
        with torch.no_grad():
            feats = self.amt._get("encoder")({"video": roi, "audio": None, "transform": tf, "clips": self.last_clips})
        return self.fit_features(feats, lens, anno, anno_lens)


# the 24 fusion tensors in the order of svt_rca_refresh_params / svt_rca_backward (include/svt_mi355.h)
RCA_LAYER_KEYS = ("self_att.att.in_proj_weight", "self_att.att.in_proj_bias", "self_att.att.out_proj.weight", "self_att.att.out_proj.bias",
                  "pos_ffn.ffn.0.weight", "pos_ffn.ffn.0.bias", "pos_ffn.ffn.3.weight", "pos_ffn.ffn.3.bias",
                  "norm1.norm.weight", "norm1.norm.bias", "norm2.norm.weight", "norm2.norm.bias")
RCA_KEYS = tuple(f"fusion.layer{l}.{k}" for l in (1, 2) for k in RCA_LAYER_KEYS)


class FusionTrainer:
    """``fit_batch`` of the audio-visual recipe (``train_rca_av.py:174-185``): ``FusionRCA`` + the 20-way ``Linear`` head trained on
    precomputed, frozen audio and video features -- forward, ``compute_objectives``, backward, ``check_gradients`` (non-finite skip +
    ``clip_grad_norm_``) and one Adadelta step over ``ModuleList[fusion, head]``, all HIP.  ``modules`` is the recipe's mapping
    (``fusion`` + ``head``).  Fusion precision fp32 (parity) or bf16 (throughput); master weights, gradients and the optimizer state are
    fp32 in both.  The fusion's parameters must be on the GPU.

    After ``fit_batch``: every parameter's ``.grad`` holds the (clipped) gradient the step used, ``last_terms`` the four loss terms,
    ``last_grad_norm`` the pre-clip norm.  The fusion's device weights are refreshed on the device from the new parameters, so the next
    ``fusion(a, v)`` uploads nothing through the host.  A non-finite loss skips the step (gradients set to None, parameters
    untouched); the ``nonfinite_patience + 1``-th skip since ``on_epoch_start()`` raises ``ValueError``."""

    def __init__(self, modules, optimizer: Optional[torch.optim.Optimizer] = None, lr: float = 3e-4, rho: float = 0.95, eps: float = 1e-8,
                 onset_positive_weight: float = 15.0, pitch_octave_num: int = 4, pitch_class_num: int = 12, max_grad_norm: float = 5.0,
                 nonfinite_patience: int = 3, allowed_len_diff: int = 3, label_smoothing: float = 0.0):
        from .fusion import FusionRCA
        from .linear import Linear
        self.fusion = modules["fusion"]
        self.head = modules["head"]
        if not isinstance(self.fusion, FusionRCA) or not isinstance(self.head, Linear):
            raise TypeError("FusionTrainer needs modules {'fusion': FusionRCA, 'head': Linear} of svt_speechbrain_amd")
        if self.fusion.precision not in ("fp32", "bf16"):
            raise _lib.SvtError(f"FusionTrainer: training takes precision fp32 or bf16, not {self.fusion.precision!r}")
        named = dict(self.fusion.named_parameters())
        self._params = [named[k] for k in RCA_KEYS]
        for p in self._params:
            if not p.is_cuda:
                raise _lib.SvtError("FusionTrainer needs the fusion's parameters on the GPU; there is no CPU fallback")
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise _lib.SvtError("FusionTrainer: the fusion's parameters must be contiguous fp32")
        self.onset_positive_weight = float(onset_positive_weight)
        self.pitch_octave_num = int(pitch_octave_num)
        self.pitch_class_num = int(pitch_class_num)
        self.max_grad_norm = float(max_grad_norm)
        self.nonfinite_patience = int(nonfinite_patience)
        self.allowed_len_diff = int(allowed_len_diff)
        self.label_smoothing = float(label_smoothing)
        if optimizer is None:
            optimizer = Adadelta(list(self.fusion.parameters()) + list(self.head.parameters()), lr=lr, rho=rho, eps=eps)
        if not isinstance(optimizer, (Adadelta, Adam)):
            raise TypeError("FusionTrainer needs svt_speechbrain_amd.training.Adadelta, Adam or AdamW (the clip is fused into their kernels)")
        self.optimizer = optimizer
        self.nonfinite_count = 0
        self.last_terms: Dict[str, float] = {}
        self.last_grad_norm: Optional[torch.Tensor] = None
        self._ws: Dict[tuple, torch.Tensor] = {}
        self._refreshed = None   # (handle, signature) the transposed weights were written for

    def on_epoch_start(self) -> None:
        self.nonfinite_count = 0

    def _scratch(self, key, nbytes: int, device) -> torch.Tensor:
        ws = self._ws.get(key)
        if ws is None or ws.numel() < nbytes or ws.device != device:
            ws = torch.empty(max(16, nbytes), dtype=torch.uint8, device=device)
            self._ws[key] = ws
        return ws

    def _ptrs(self, tensors):
        return (C.c_void_p * len(tensors))(*[_lib.ptr(t) for t in tensors])

    def _signature(self):
        return tuple((t.data_ptr(), t._version) for _, t in self.fusion._param_owner()._tensors())

    def _refresh(self, lib, slot, dev) -> None:
        """Rewrite the handle's weights (and the transposes the backward reads) from the fp32 parameters, on the device."""
        _lib.check(lib.svt_rca_refresh_params(slot.handle, self._ptrs(self._params), len(self._params), _lib.stream_ptr(dev)),
                   "svt_rca_refresh_params", lib)
        slot.sig = self._signature()
        self._refreshed = (slot.handle.value, slot.sig)

    def fit_batch(self, audio_feats: torch.Tensor, video_feats: torch.Tensor, wav_lens: Optional[torch.Tensor], anno: torch.Tensor,
                  anno_lens: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One step on audio (B, T1, D) and video (B, T2, D) features; ``anno`` (B, T', 4) as ``LinearProbe.fit_features``, masked by
        ``wav_lens``.  Returns the detached 0-d loss on the CPU, as ``Brain.fit_batch``."""
        if not (audio_feats.is_cuda and video_feats.is_cuda):
            raise _lib.SvtError("FusionTrainer needs its features on the GPU; there is no CPU fallback")
        fusion, head = self.fusion, self.head
        lib = _lib.load()
        dev = audio_feats.device
        a = audio_feats.detach().to(torch.float32).contiguous()
        v = video_feats.detach().to(torch.float32).contiguous()
        if a.dim() != 3 or v.dim() != 3 or a.shape[0] != v.shape[0] or a.shape[2] != fusion.d_model or v.shape[2] != fusion.d_model:
            raise ValueError(f"expected (B, T, {fusion.d_model}) features with equal batch, got {tuple(a.shape)} and {tuple(v.shape)}")
        B, T1, D = a.shape
        T2 = v.shape[1]
        if abs(T1 - T2) > 15:
            print("Alignment is wrong")  # the reference's diagnostic (fusion.py:204-205)
        slot = fusion._sync(dev)
        if self._refreshed != (slot.handle.value, slot.sig):
            self._refresh(lib, slot, dev)
        need = lib.svt_rca_train_workspace_bytes(slot.handle, B, T1)
        if need < 0:
            raise _lib.SvtError(_lib.last_error(lib))
        ws = self._scratch("rca", int(need), dev)
        stream = _lib.stream_ptr(dev)
        feats = torch.empty((B, T1, D), dtype=torch.float32, device=dev)
        _lib.check(lib.svt_rca_forward_train(slot.handle, _lib.ptr(a), T1, _lib.ptr(v), T2, B, _lib.ptr(feats), _lib.ptr(ws), ws.numel(),
                                             stream), "svt_rca_forward_train", lib)
        logits = head(feats)
        n_out = logits.shape[-1]
        an = anno.to(dev)
        if an.dim() != 3 or an.shape[0] != B or an.shape[2] < 4:
            raise ValueError(f"anno must be (batch, frames, 4), got {tuple(anno.shape)}")
        on_t = an[:, :, 0].to(torch.float32).contiguous()
        off_t = an[:, :, 1].to(torch.float32).contiguous()
        oct_t = an[:, :, 2].to(torch.int64).contiguous()
        cls_t = an[:, :, 3].to(torch.int64).contiguous()
        ln = None
        if wav_lens is not None:
            ln = torch.as_tensor(wav_lens, dtype=torch.float32, device=dev).reshape(-1).contiguous()
            if ln.numel() != B:
                raise ValueError(f"wav_lens has {ln.numel()} entries for a batch of {B}")

        def obj_ws(query):
            n = C.c_size_t(0)
            query(n)
            return self._scratch("obj", int(n.value), dev)

        terms, dlogits, host = amt_objective_grad(logits, on_t, off_t, oct_t, cls_t, ln, self.onset_positive_weight,
                                                  self.pitch_octave_num, self.allowed_len_diff, self.label_smoothing, workspace=obj_ws)
        self.last_terms = dict(zip(TERMS, host[:4]))
        loss = terms[4]
        all_params = self._params + [head.w.weight] + ([head.w.bias] if head.w.bias is not None else [])
        if not math.isfinite(float(host[4])):
            self.nonfinite_count += 1
            for p in all_params:
                p.grad = None
            if self.nonfinite_count > self.nonfinite_patience:
                raise ValueError("Loss is not finite and patience is exhausted. To debug, wrap `fit()` with autograd's "
                                 "`detect_anomaly()`, e.g.\n\nwith torch.autograd.detect_anomaly():\n\tbrain.fit(...)")
            return loss.detach().cpu()
        for p in all_params:
            if p.grad is None or p.grad.shape != p.shape or not p.grad.is_contiguous() or p.grad.device != p.device:
                p.grad = torch.empty_like(p, memory_format=torch.contiguous_format)
        w, b = head.w.weight, head.w.bias
        rows = B * T1
        x2, d2 = feats.reshape(rows, D), dlogits.reshape(rows, n_out)

        def wg_ws(query):
            n = C.c_size_t(0)
            query(n)
            return self._scratch("wgrad", int(n.value), dev)

        linear_backward(x2, d2, w.grad, b.grad if b is not None else None, workspace=wg_ws)
        dfeats = linear_backward_data(d2, w)
        grads = [p.grad for p in self._params]
        _lib.check(lib.svt_rca_backward(slot.handle, _lib.ptr(dfeats), B, T1, self._ptrs(grads), _lib.ptr(ws), ws.numel(), stream),
                   "svt_rca_backward", lib)
        for p in all_params:
            _bump(p.grad)
        self.last_grad_norm = torch.empty((), dtype=torch.float32, device=dev)
        self.optimizer.step(max_norm=self.max_grad_norm, total_norm=self.last_grad_norm)
        self._refresh(lib, slot, dev)
        return loss.detach().cpu()
