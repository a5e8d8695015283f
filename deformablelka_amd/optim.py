"""The step every reference trainer ends its iteration with, on the multi-tensor HIP kernels of ``csrc/cl_optim.hip`` (include/dlka.h:
``dlka_optim_*``): ``clip_grad_norm_(parameters, 12)`` followed by SGD with momentum, Nesterov and weight decay
(3D/d_lka_former/training/network_training/d_lka_former_trainer_synapse.py:197-205, :291-309; 2D/trainer_MaxViT_deform_LKA.py:114;
3D/train_pancreas.py:127), or by Adam / AdamW (3D/d_lka_former/training/network_training/Trainer_synapse.py:270-273, Trainer_acdc.py:269-272:
``Adam(3e-4, weight_decay=3e-5, amsgrad=True)``; 2D/trainer_MaxViT_LKA.py:114: ``AdamW(lr, weight_decay=1e-4)``).

  ``SGD``               ``torch.optim.SGD``'s arguments and state (``'momentum_buffer'``), so its ``state_dict`` loads into this class and back.
                        One fixed-order norm pass over the gradients of all groups, then per group ONE pass that applies the clip factor,
                        weight decay, momentum, Nesterov and the parameter write.  The learning rates live in a device tensor
                        (``lr_tensor``): ``param_groups[i]['lr'] = x`` keeps working, and a captured iteration follows the schedule.
  ``Adam``, ``AdamW``   ``torch.optim.Adam``'s / ``AdamW``'s arguments and state (``'step'``, ``'exp_avg'``, ``'exp_avg_sq'``, ``'max_exp_avg_sq'``),
                        the same norm pass, learning-rate tensor and ``step(max_grad_norm=...)``.  The step counts live on the device (one
                        float32 per parameter, torch's ``capturable`` convention): a captured step advances them at every replay.
  ``clip_grad_norm_``   ``torch.nn.utils.clip_grad_norm_`` for callers who keep their own optimizer.
  ``poly_lr``           nnU-Net's schedule (3D/d_lka_former/training/learning_rate/poly_lr.py:16-17; called at trainer_synapse.py:451).

Float32 parameters that are dense in memory; what is not covered raises ``NotImplementedError`` naming the argument.  There is no fall-back to
torch's implementation.  Deviation from the reference: ``step`` does not leave the scaled gradients behind (nothing in a trainer reads
them after the step); ``clip_grad_norm_`` does."""
from __future__ import annotations

import ctypes

import torch

from . import _lib as L

_CTOR = object()   # step(max_grad_norm=...): "what the constructor was given"


def poly_lr(epoch, max_epochs, initial_lr, exponent=0.9):
    return initial_lr * (1 - epoch / max_epochs) ** exponent


def _dense(t: torch.Tensor) -> bool:
    """Every element of the tensor's memory span belongs to exactly one index: the kernels walk numel() consecutive elements."""
    if t.is_contiguous():
        return True
    expect = 1
    for size, stride in sorted(((s, st) for s, st in zip(t.shape, t.stride()) if s != 1), key=lambda x: x[1]):
        if stride != expect:
            return False
        expect *= size
    return True


def _check_grad(g: torch.Tensor, what: str) -> None:
    if g.is_sparse:
        raise NotImplementedError(f"{what}: sparse gradients are not covered by the HIP optimizer kernels")
    if g.dtype != torch.float32:
        raise NotImplementedError(f"{what}: gradients must be float32, got {g.dtype}")


def _arrays(n: int):
    return (ctypes.c_void_p * max(n, 1))(), (ctypes.c_int64 * max(n, 1))()


def _at(arr, offset: int, ctype):
    return ctypes.cast(ctypes.addressof(arr) + ctypes.sizeof(ctype) * offset, ctypes.POINTER(ctype))


def _grad_norm(g_arr, counts, n: int, like: torch.Tensor, ws, norm: torch.Tensor):
    """norm[0] = the 2-norm of the n listed gradients; returns the workspace (grown when needed) for the caller to keep."""
    lib = L.get_lib()
    need = lib.dlka_optim_workspace_bytes(counts, n)
    if ws is None or ws.numel() < need:
        ws = L.scratch(need, like)
    L.check(lib.dlka_optim_grad_norm(g_arr, counts, n, L.DLKA_F32, L.ptr(ws), ws.numel(), L.ptr(norm), L.stream_ptr(like)), "optim_grad_norm")
    return ws


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """``torch.nn.utils.clip_grad_norm_``: scales the gradients in place by ``min(1, max_norm / (norm + 1e-6))`` and returns the norm (a device
    tensor).  Two passes over the gradients, no host read; the norm is bitwise reproducible.  ``foreach`` is accepted and has no meaning here."""
    if float(norm_type) != 2.0:
        raise NotImplementedError(f"norm_type: only the 2-norm is implemented on the HIP kernels, got {norm_type!r}")
    if error_if_nonfinite:
        raise NotImplementedError("error_if_nonfinite=True needs a host read of the norm; check torch.isfinite() of the returned norm instead")
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.tensor(0.0)
    for g in grads:
        _check_grad(g, "clip_grad_norm_")
        if not _dense(g):
            raise NotImplementedError("clip_grad_norm_: a gradient that is not dense in memory (an expanded or strided view) is not covered")
        if g.device != grads[0].device:
            raise NotImplementedError("clip_grad_norm_: gradients on more than one device")
    L.require_device(*grads)
    n = len(grads)
    g_arr, counts = _arrays(n)
    for i, g in enumerate(grads):
        g_arr[i], counts[i] = g.data_ptr(), g.numel()
    norm = torch.empty(1, dtype=torch.float32, device=grads[0].device)
    _grad_norm(g_arr, counts, n, grads[0], None, norm)
    L.check(L.get_lib().dlka_optim_scale(g_arr, counts, n, L.DLKA_F32, L.ptr(norm), float(max_norm), L.stream_ptr(grads[0])), "optim_scale")
    return norm.reshape(())


class _MultiTensorOptimizer(torch.optim.Optimizer):
    """What the classes below share: the learning rates in a device tensor, the address tables cached per set of parameters that have
    gradients, the gradients relaid into their parameter's layout, the norm pass, and the checks of what the kernels cover.  A subclass adds
    its state's address columns (``_state_columns``) and its launch (``_launch``)."""

    lr_on_device = True     # training.GraphedIteration: a changed learning rate is uploaded before the replay instead of refused
    clips_in_step = True    # training.run_iteration: step(max_grad_norm=clip_norm) replaces clip_grad_norm_ + step()

    def __init__(self, params, defaults, max_grad_norm):
        self.max_grad_norm = max_grad_norm
        self.last_grad_norm = None
        self.lr_tensor = None
        self._uploaded_lrs = None
        self._tables = {}
        self._ws = None
        self._norm = None
        super().__init__(params, defaults)
        self._check_groups()

    # ---- what is covered ------------------------------------------------------------------------------------------------------------------------------
    def _check_group(self, group):
        """The subclass's own arguments."""

    def _check_groups(self):
        for group in self.param_groups:
            self._check_group(group)
            if group.get("maximize", False):
                raise NotImplementedError("maximize=True is not implemented on the HIP kernels")
            if group.get("differentiable", False):
                raise NotImplementedError("differentiable=True is not implemented on the HIP kernels")
            for p in group["params"]:
                if p.dtype != torch.float32:
                    raise NotImplementedError(f"params: non-float32 parameters are not implemented on the HIP kernels, got {p.dtype}")
                if p.is_sparse or not _dense(p):
                    raise NotImplementedError("params: a parameter that is not dense in memory (a strided view) is not covered")

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self.invalidate_tables()
        self._check_groups()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self.invalidate_tables()
        self._check_groups()

    def invalidate_tables(self):
        self._tables = {}

    # ---- learning rates ---------------------------------------------------------------------------------------------------------------------------
    def _device(self):
        for group in self.param_groups:
            for p in group["params"]:
                return p.device
        return torch.device("cpu")

    def sync_lr(self):
        lrs = [float(g["lr"]) for g in self.param_groups]
        if self.lr_tensor is not None and lrs == self._uploaded_lrs:
            return
        dev = self._device()
        if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"optim.{type(self).__name__}: the learning rate changed ({self._uploaded_lrs} -> {lrs}) inside a stream capture; set "
                               "it, and call sync_lr() or step(), outside the capture — the captured step reads lr_tensor at replay")
        host = torch.tensor(lrs, dtype=torch.float32)
        if self.lr_tensor is None or self.lr_tensor.numel() != len(lrs):
            self.lr_tensor = host.to(dev)
        else:
            self.lr_tensor.copy_(host)   # a few floats, on the current stream
        self._uploaded_lrs = lrs

    # ---- address tables ---------------------------------------------------------------------------------------------------------------------------
    def _laid_like(self, p, buf, key):
        """The state tensor ``buf`` in the parameter's dtype and layout (one copy where it is not), or zeros where there is none yet."""
        if buf is None:
            return torch.zeros_like(p, memory_format=torch.preserve_format)
        if buf.dtype != torch.float32:
            raise NotImplementedError(f"{key}: non-float32 state is not implemented on the HIP kernels, got {buf.dtype}")
        if buf.stride() != p.stride() or buf.shape != p.shape:
            new = torch.empty_like(p, memory_format=torch.preserve_format)
            new.copy_(buf)
            return new
        return buf

    def _state_columns(self, group, params):
        """(dict of extra entries of the group's table, the tensors the table's addresses point into)"""
        raise NotImplementedError

    def _build_tables(self, key):
        groups, n_all = [], sum(len(k) for k in key)
        g_all, c_all = _arrays(n_all)
        off = 0
        for gi, (group, idx) in enumerate(zip(self.param_groups, key)):
            params = [group["params"][i] for i in idx]
            n = len(params)
            p_arr, _ = _arrays(n)
            for k, p in enumerate(params):
                p_arr[k], c_all[off + k] = p.data_ptr(), p.numel()
            columns, held = self._state_columns(group, params)
            groups.append(dict(index=gi, params=params, strides=[p.stride() for p in params], n=n, p_arr=p_arr,
                               keep=(held, [p.data for p in params]),   # the tabled memory stays allocated as long as the table
                               g_ptr=_at(g_all, off, ctypes.c_void_p), c_ptr=_at(c_all, off, ctypes.c_int64), offset=off, **columns))
            off += n
        return dict(groups=groups, n=n_all, g_all=g_all, c_all=c_all)

    # ---- the step -----------------------------------------------------------------------------------------------------------------------------------
    def _launch(self, lib, g, group, clip, stream):
        raise NotImplementedError

    @torch.no_grad()
    def step(self, closure=None, max_grad_norm=_CTOR):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        clip = self.max_grad_norm if max_grad_norm is _CTOR else max_grad_norm
        self.sync_lr()
        key = tuple(tuple(i for i, p in enumerate(group["params"]) if p.grad is not None) for group in self.param_groups)
        tab = self._tables.get(key)
        if tab is None:
            tab = self._tables[key] = self._build_tables(key)
        self.last_grad_norm = None
        if tab["n"] == 0:
            if clip is not None:
                self.last_grad_norm = torch.zeros((), dtype=torch.float32, device=self._device())
            return loss
        g_all, first, held = tab["g_all"], None, []
        for g in tab["groups"]:
            off = g["offset"]
            for k, (p, stride) in enumerate(zip(g["params"], g["strides"])):
                grad = p.grad
                _check_grad(grad, "step")
                if grad.stride() != stride:   # plumbing: into the parameter's layout, one copy
                    relaid = torch.empty_like(p, memory_format=torch.preserve_format)
                    relaid.copy_(grad)
                    grad = relaid
                    held.append(relaid)
                if first is None:
                    first = grad
                g_all[off + k] = grad.data_ptr()
        L.require_device(first, self.lr_tensor)
        lib, stream = L.get_lib(), L.stream_ptr(first)
        if self._norm is None:
            self._norm = torch.zeros(1, dtype=torch.float32, device=first.device)
        if clip is not None:
            self._ws = _grad_norm(g_all, tab["c_all"], tab["n"], first, self._ws, self._norm)
            self.last_grad_norm = self._norm.reshape(())
        for g in tab["groups"]:
            if g["n"] == 0:
                continue
            self._launch(lib, g, self.param_groups[g["index"]], clip, stream)
        del held   # (stream-ordered: the allocator hands the memory out again behind the launches that read it)
        return loss


class SGD(_MultiTensorOptimizer):
    """``torch.optim.SGD(params, lr, momentum, dampening, weight_decay, nesterov)`` with the clip of ``clip_grad_norm_(max_grad_norm)`` folded into
    the step.  ``step(max_grad_norm=x)`` overrides the constructor's value for that call (``None``: no clipping).  ``last_grad_norm``: the norm
    the last step clipped by (a device tensor that the next step overwrites), or ``None``.

    ``lr_tensor`` (device, float32, one entry per group) is what the kernels read.  ``sync_lr()`` uploads the groups' ``'lr'`` values when they
    differ from the last upload; ``step()`` calls it.  Inside a stream capture a changed value raises (an upload cannot be captured); an
    unchanged one copies nothing, so the captured step reads whatever ``lr_tensor`` holds at replay.

    The address tables of parameters and momentum buffers are built once per set of parameters that have gradients and kept;
    ``load_state_dict`` and ``add_param_group`` drop them, and so must ``invalidate_tables()`` after replacing a parameter's ``.data`` or a
    buffer in ``state`` by hand.  Only the gradients' addresses are read again at every eager step."""

    def __init__(self, params, lr, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, max_grad_norm=None, maximize=False,
                 differentiable=False):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        # torch.optim.SGD's keys, so that either class reads the other's state_dict
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, maximize=maximize,
                        foreach=None, differentiable=differentiable, fused=None)
        super().__init__(params, defaults, max_grad_norm)

    def _check_group(self, group):
        if group.get("dampening", 0) != 0:
            raise NotImplementedError(f"dampening: only 0 is implemented on the HIP kernels, got {group['dampening']!r}")

    def _state_columns(self, group, params):
        if group["momentum"] == 0:
            return dict(b_arr=None), []
        b_arr, _ = _arrays(len(params))
        bufs = []
        for k, p in enumerate(params):
            st = self.state[p]
            buf = st["momentum_buffer"] = self._laid_like(p, st.get("momentum_buffer"), "momentum_buffer")   # zeros: torch's first-step buf = d
            bufs.append(buf)
            b_arr[k] = buf.data_ptr()
        return dict(b_arr=b_arr), bufs

    def _launch(self, lib, g, group, clip, stream):
        d = L.OptimDesc(n_tensors=g["n"], dtype=L.DLKA_F32, nesterov=int(bool(group["nesterov"])), has_momentum=int(g["b_arr"] is not None),
                        clip=int(clip is not None), momentum=float(group["momentum"]), weight_decay=float(group["weight_decay"]),
                        max_norm=float(clip if clip is not None else 0.0), lr_index=g["index"])
        L.check(lib.dlka_optim_sgd_step(g["p_arr"], g["g_ptr"], g["b_arr"], g["c_ptr"], ctypes.byref(d), L.ptr(self.lr_tensor),
                                        L.ptr(self._norm), stream), "optim_sgd_step")


class Adam(_MultiTensorOptimizer):
    """``torch.optim.Adam(params, lr, betas, eps, weight_decay, amsgrad)`` with the clip of ``clip_grad_norm_(max_grad_norm)`` folded into the step:
    ``step(max_grad_norm=...)``, ``last_grad_norm``, ``lr_tensor``, ``sync_lr()`` and ``invalidate_tables()`` as in ``SGD``.

    The step counts are one float32 per parameter in ONE device tensor that the kernels advance (a parameter without a gradient does not
    advance); ``state[p]['step']`` is a 0-dim view of it, so a captured step counts at every replay and nothing reads the host.  That is
    torch's ``capturable=True`` convention and what ``param_groups`` say; ``capturable=False`` (a count on the host) is not offered.
    ``load_state_dict`` takes torch's dicts of either kind and moves the counts into that tensor.  ``foreach`` and ``fused`` are accepted and
    ignored."""

    _decoupled_default = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, max_grad_norm=None, foreach=None,
                 maximize=False, capturable=True, differentiable=False, fused=None, decoupled_weight_decay=None):
        if isinstance(lr, torch.Tensor):
            raise NotImplementedError("lr: a tensor learning rate is not implemented; the rate already lives on the device (lr_tensor)")
        if any(isinstance(b, torch.Tensor) for b in betas):
            raise NotImplementedError("betas: tensor betas are not implemented on the HIP kernels")
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
        if decoupled_weight_decay is None:
            decoupled_weight_decay = self._decoupled_default
        # torch.optim.Adam's keys, so that either class reads the other's state_dict
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=foreach,
                        capturable=capturable, differentiable=differentiable, fused=fused, decoupled_weight_decay=decoupled_weight_decay)
        self._steps = None   # float32 [parameters of all groups]: the counts
        self._bias = None    # float32 [2 * parameters]: the kernels' 1 - beta1^t, sqrt(1 - beta2^t) of the current step
        super().__init__(params, defaults, max_grad_norm)

    def _check_group(self, group):
        if not group.get("capturable", True):
            raise NotImplementedError("capturable=False keeps the step counts on the host, which the update would have to read; the HIP kernels "
                                      "keep them on the device (capturable=True)")
        if isinstance(group["lr"], torch.Tensor):
            raise NotImplementedError("lr: a tensor learning rate is not implemented; the rate already lives on the device (lr_tensor)")
        if any(isinstance(b, torch.Tensor) for b in group["betas"]):
            raise NotImplementedError("betas: tensor betas are not implemented on the HIP kernels")

    def load_state_dict(self, state_dict):
        torch.optim.Optimizer.load_state_dict(self, state_dict)
        for group in self.param_groups:   # torch's dicts say capturable=False and may predate the newer keys
            group["capturable"] = True
            for k, v in (("amsgrad", False), ("maximize", False), ("foreach", None), ("differentiable", False), ("fused", None)):
                group.setdefault(k, v)
            if self._decoupled_default:
                group["decoupled_weight_decay"] = True   # (as torch.optim.AdamW.__setstate__)
            else:
                group.setdefault("decoupled_weight_decay", False)
        self._steps = None
        self.invalidate_tables()
        self._check_groups()
        self._count_tensor()

    # ---- the counts ---------------------------------------------------------------------------------------------------------------------------------
    def _count_tensor(self):
        """The count tensor sized for the parameters of all groups, ``state[p]['step']`` of every parameter that has state a view of it.  Counts
        that live elsewhere (a loaded dict, parameters added since) are copied in."""
        params = [p for group in self.param_groups for p in group["params"]]
        if self._steps is not None and self._steps.numel() == len(params):
            return self._steps
        dev = self._device()
        host = torch.zeros(len(params), dtype=torch.float32)
        for i, p in enumerate(params):
            st = self.state.get(p)
            if st is not None and "step" in st:
                host[i] = float(st["step"])   # (not during a capture: tables are built in the warm-up)
        self._steps = host.to(dev)
        self._bias = torch.zeros(2 * len(params), dtype=torch.float32, device=dev)
        self._slot = {id(p): i for i, p in enumerate(params)}
        for i, p in enumerate(params):
            st = self.state.get(p)
            if st is not None and "step" in st:
                st["step"] = self._steps[i]
        return self._steps

    def _state_columns(self, group, params):
        steps = self._count_tensor()
        n, ams = len(params), bool(group["amsgrad"])
        cols = {k: _arrays(n)[0] for k in ("m_arr", "v_arr", "s_arr")}
        cols["x_arr"] = _arrays(n)[0] if ams else None
        held = [steps, self._bias]
        for k, p in enumerate(params):
            st = self.state[p]
            if "step" not in st:
                st["step"] = steps[self._slot[id(p)]]
            cols["s_arr"][k] = steps.data_ptr() + 4 * self._slot[id(p)]
            for name, arr in (("exp_avg", "m_arr"), ("exp_avg_sq", "v_arr"), ("max_exp_avg_sq", "x_arr")):
                if cols[arr] is None:
                    continue
                buf = st[name] = self._laid_like(p, st.get(name), name)
                held.append(buf)
                cols[arr][k] = buf.data_ptr()
        return cols, held

    def _launch(self, lib, g, group, clip, stream):
        d = L.OptimAdamDesc(n_tensors=g["n"], dtype=L.DLKA_F32, decoupled=int(bool(group["decoupled_weight_decay"])), amsgrad=int(g["x_arr"] is not None),
                            clip=int(clip is not None), beta1=float(group["betas"][0]), beta2=float(group["betas"][1]), eps=float(group["eps"]),
                            weight_decay=float(group["weight_decay"]), max_norm=float(clip if clip is not None else 0.0), lr_index=g["index"])
        ws = ctypes.c_void_p(self._bias.data_ptr() + 8 * g["offset"])   # this group's slots, behind the groups before it
        L.check(lib.dlka_optim_adam_step(g["p_arr"], g["g_ptr"], g["m_arr"], g["v_arr"], g["x_arr"], g["s_arr"], g["c_ptr"], ctypes.byref(d),
                                         L.ptr(self.lr_tensor), L.ptr(self._norm), ws, 8 * g["n"], stream), "optim_adam_step")


class AdamW(Adam):
    """``torch.optim.AdamW``: ``Adam`` with the weight decay applied to the parameter (``p *= 1 - lr * weight_decay``) instead of added to the
    gradient, and torch's default ``weight_decay=1e-2``."""

    _decoupled_default = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, max_grad_norm=None, maximize=False,
                 foreach=None, capturable=True, differentiable=False, fused=None):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, max_grad_norm=max_grad_norm, foreach=foreach, maximize=maximize,
                         capturable=capturable, differentiable=differentiable, fused=fused, decoupled_weight_decay=True)
