"""The planar (NCDHW) operators besides the deformable convs: plain conv3d, GELU, and the full net's plumbing (BatchNorm3d, 1x1x1 convs)."""
from __future__ import annotations

from ctypes import byref

import torch

from .. import _lib as L
from ._call import WS, _geom, _out_dims, _require_input_dtype, _triple, call, call_ws, grads_like


# ---- plain conv --------------------------------------------------------------------------------------------------------------------------
def conv3d_forward(input, weight, bias=None, stride=1, padding=0, dilation=1, groups=1):
    L.require_device(input, weight, bias)
    _require_input_dtype(input, weight=weight, bias=bias)
    s, p, d = _triple(stride), _triple(padding), _triple(dilation)
    input, weight = input.contiguous(), weight.contiguous()
    bias = None if bias is None else bias.contiguous()
    g = _geom(input.shape, weight.shape[0], tuple(weight.shape[2:5]), s, p, d, groups)
    dt = L.dtype_code(input, allow_f64=True)
    Do, Ho, Wo = _out_dims(g)
    out = torch.empty((g.B, g.Cout, Do, Ho, Wo), dtype=input.dtype, device=input.device)
    call_ws("conv3d_forward", ("conv3d_forward_workspace", byref(g), dt), input, L.ptr(input), L.ptr(weight), L.ptr(bias), L.ptr(out), WS, byref(g), dt,
            L.stream_ptr(input), label="conv3d")
    return out


def conv3d_backward(input, weight, grad_output, stride=1, padding=0, dilation=1, groups=1, need=(True, True, True)):
    L.require_device(input, weight, grad_output)
    _require_input_dtype(input, weight=weight, grad_output=grad_output)
    s, p, d = _triple(stride), _triple(padding), _triple(dilation)
    input, weight, grad_output = input.contiguous(), weight.contiguous(), grad_output.contiguous()
    g = _geom(input.shape, weight.shape[0], tuple(weight.shape[2:5]), s, p, d, groups)
    dt = L.dtype_code(input, allow_f64=True)
    gi, gw = grads_like((input, weight), need)
    gb = torch.empty((g.Cout,), dtype=input.dtype, device=input.device) if need[2] else None
    call_ws("conv3d_backward", ("conv3d_backward_workspace", byref(g), dt), input, L.ptr(input), L.ptr(weight), L.ptr(grad_output), L.ptr(gi), L.ptr(gw),
            L.ptr(gb), WS, byref(g), dt, L.stream_ptr(input), label="conv3d backward")
    return gi, gw, gb


def gelu_forward(x):
    L.require_device(x)
    x = x.contiguous()
    y = torch.empty_like(x)
    call("gelu_forward", L.ptr(x), L.ptr(y), x.numel(), L.dtype_code(x), L.stream_ptr(x), label="gelu")
    return y


def gelu_backward(x, gy):
    L.require_device(x, gy)
    x, gy = x.contiguous(), gy.contiguous()
    gx = torch.empty_like(x)
    call("gelu_backward", L.ptr(x), L.ptr(gy), L.ptr(gx), x.numel(), L.dtype_code(x), L.stream_ptr(x), label="gelu bwd")
    return gx


# ---- planar (NCDHW) plumbing of the full net: BatchNorm3d in training mode, 1x1x1 convs on few channels (csrc/planar_ops.hip) ------------
PLANAR_PW_CIN = (1, 2, 4, 8, 14, 16, 32)
PLANAR_BN_STATS_ROWS = 5   # rows of the BatchNorm statistics tensor (include/dlka.h: dlka_batchnorm_planar_forward)


def _planar_f32(name, *tensors):
    """The planar BatchNorm kernels read fp32 contiguous memory: anything else is refused (dtype) or made contiguous (layout)."""
    for t in tensors:
        if t is not None and t.dtype != torch.float32:
            raise RuntimeError(f"{name}: float32 tensors only, got {t.dtype}")
    return [None if t is None else t.contiguous() for t in tensors]


def batchnorm_planar_forward(x, weight, bias, eps=1e-5, out=None):
    """x (B, C, *spatial) fp32 -> y, stats (PLANAR_BN_STATS_ROWS, C) = mean, rstd, unbiased variance, mean - pivot, pivot (batch statistics; the pivot is the
    value the kernels centre on, see csrc/planar_ops.hip).
    out: a contiguous fp32 tensor of x's element count (any shape) that receives y instead of a fresh tensor of x's shape."""
    L.require_device(x, weight, bias)
    x, weight, bias = _planar_f32("batchnorm_planar_forward", x, weight, bias)
    B, C = x.shape[:2]
    N = x[0, 0].numel()
    if out is None:
        y = torch.empty_like(x)
    else:
        assert out.is_contiguous() and out.numel() == x.numel() and out.dtype == x.dtype and out.device == x.device
        y = out
    stats = torch.empty(PLANAR_BN_STATS_ROWS, C, dtype=torch.float32, device=x.device)
    scratch = torch.empty(2 * C, dtype=torch.float32, device=x.device)
    call("batchnorm_planar_forward", L.ptr(x), L.ptr(weight), L.ptr(bias), L.ptr(stats), L.ptr(y), L.ptr(scratch), B, C, N, float(eps), L.stream_ptr(x))
    return y, stats


def batchnorm_planar_backward(g, x, weight, stats, affine=True):
    """g, x (B, C, *spatial) fp32, stats as batchnorm_planar_forward returned it for this x -> gx, gw, gb (the latter two None without affine)."""
    L.require_device(x, g, weight, stats)
    g, x, weight, stats = _planar_f32("batchnorm_planar_backward", g, x, weight, stats)
    B, C = x.shape[:2]
    N = x[0, 0].numel()
    if g.shape != x.shape or tuple(stats.shape) != (PLANAR_BN_STATS_ROWS, C):
        raise RuntimeError(f"batchnorm_planar_backward: grad_out {tuple(g.shape)} / stats {tuple(stats.shape)} do not belong to x {tuple(x.shape)}")
    gx = torch.empty_like(x)
    gw = torch.empty(C, dtype=torch.float32, device=x.device) if affine else None
    gb = torch.empty(C, dtype=torch.float32, device=x.device) if affine else None
    scratch = torch.empty(2 * C, dtype=torch.float32, device=x.device)
    call("batchnorm_planar_backward", L.ptr(g), L.ptr(x), L.ptr(weight), L.ptr(stats), L.ptr(gx), L.ptr(gw), L.ptr(gb), L.ptr(scratch), B, C, N,
         L.stream_ptr(x))
    return gx, gw, gb


def pointwise_planar_supported(x, weight, need_weight_grad=True, need_input_grad=None) -> bool:
    """Whether the planar 1x1x1 kernels cover this call INCLUDING the backward pass it may need.  The forward kernel is instantiated on Cin (the
    channel count it holds in registers), the data-gradient kernel on Cout (``pl_pw_bwd_data_kernel<CO>``, planar_ops.hip: the same menu), the weight
    gradient takes Cout <= 16.  need_input_grad: None = ``x.requires_grad`` under grad mode."""
    Cout, Cin = weight.shape[:2]
    if need_input_grad is None:
        need_input_grad = bool(x.requires_grad and torch.is_grad_enabled())
    if not (x.dtype == torch.float32 and weight.dtype == torch.float32 and Cin in PLANAR_PW_CIN and x[0, 0].numel() % 4 == 0 and x.shape[0] <= 65535):
        return False
    if need_weight_grad:
        return Cout <= 16 and Cout in PLANAR_PW_CIN
    if need_input_grad:
        return Cout in PLANAR_PW_CIN
    return Cout <= 64


def pointwise_planar_forward(x, weight, bias=None):
    """1x1x1 conv: x (B, Cin, *spatial) fp32 contiguous, weight (Cout, Cin, 1, 1, 1)."""
    L.require_device(x, weight)
    B, Cin = x.shape[:2]
    Cout = weight.shape[0]
    y = torch.empty((B, Cout) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
    call("pointwise_planar_forward", L.ptr(x), L.ptr(weight), L.ptr(bias), L.ptr(y), B, Cin, Cout, x[0, 0].numel(), L.stream_ptr(x))
    return y


def pointwise_planar_backward(x, weight, g, need=(True, True, True)):
    L.require_device(x, weight, g)
    B, Cin = x.shape[:2]
    Cout = weight.shape[0]
    gx, gw = grads_like((x, weight), need)
    gb = torch.empty(Cout, dtype=torch.float32, device=x.device) if (need[1] and need[2]) else None
    if need[0] or need[1]:
        call("pointwise_planar_backward", L.ptr(x), L.ptr(weight), L.ptr(g), L.ptr(gx), L.ptr(gw), L.ptr(gb), B, Cin, Cout, x[0, 0].numel(),
             L.stream_ptr(x))
    if need[2] and gb is None:   # frozen weight, trainable bias (fine-tuning a head): the bias gradient rides in the weight-gradient kernel, which did
        gb = g.sum(dim=[0] + list(range(2, g.dim())))   # not run — a plain reduction of grad_out (not hot: a Cout-length result)
    return gx, gw, gb
