"""Tensor-level wrappers over the C-ABI.  PyTorch is used for device memory and streams only."""
from __future__ import annotations

import ctypes
import math
from ctypes import byref
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L


def _triple(v) -> Tuple[int, int, int]:
    if isinstance(v, int):
        return (v, v, v)
    v = tuple(int(x) for x in v)
    if len(v) != 3:
        raise ValueError(f"expected an int or a 3-tuple, got {v}")
    return v


def _pair(v) -> Tuple[int, int]:
    if isinstance(v, int):
        return (v, v)
    v = tuple(int(x) for x in v)
    if len(v) != 2:
        raise ValueError(f"expected an int or a 2-tuple, got {v}")
    return v


def _require_input_dtype(input, **named):
    """The general operators hand EVERY pointer to the library as the type of `input` (float32, bfloat16 or float64): a tensor of another dtype would be read at
    the wrong element size — past its end when it is the narrower one.  The reference's op raises a scalar-type mismatch there; so does this, before any launch."""
    for name, t in named.items():
        if t is not None and t.dtype != input.dtype:
            raise RuntimeError(f"expected `{name}` to have the dtype of `input` ({input.dtype}), got {t.dtype}")


def _geom(x_shape, cout, k, s, p, d, group, dg=1, im2col_step=64) -> L.ConvGeom:
    B, C, D, H, W = (int(v) for v in x_shape)
    return L.ConvGeom(B, C, D, H, W, int(cout), *k, *s, *p, *d, int(group), int(dg), int(im2col_step))


def _out_dims(g: L.ConvGeom):
    f = L.get_lib().dlka_conv_out_size
    return (f(g.D, g.pd, g.dd, g.kd, g.sd), f(g.H, g.ph, g.dh, g.kh, g.sh), f(g.W, g.pw, g.dw, g.kw, g.sw))


# ------------------------------------------------------------------------------------------------------------
# 3-D deformable conv
# ------------------------------------------------------------------------------------------------------------
def deform_conv3d_forward(input, weight, bias, offset, kernel_size, stride, padding, dilation, group, deformable_groups,
                          im2col_step=64):
    """``D3D.deform_conv_forward`` (3D/dcn/src/deform_conv.h:10-47)."""
    # deform_conv_cuda.cu:41-47
    if not input.is_contiguous():
        raise RuntimeError("input tensor has to be contiguous")
    if not weight.is_contiguous():
        raise RuntimeError("weight tensor has to be contiguous")
    L.require_device(input, weight, bias, offset)
    _require_input_dtype(input, weight=weight, bias=bias, offset=offset)
    k, s, p, d = _triple(kernel_size), _triple(stride), _triple(padding), _triple(dilation)
    if tuple(weight.shape[2:5]) != k:  # deform_conv_cuda.cu:72-73
        raise RuntimeError(f"Input shape and kernel shape wont match: ({k} vs {tuple(weight.shape[2:5])}).")
    if input.shape[1] != weight.shape[1] * group:  # :75-76
        raise RuntimeError(f"Input shape and kernel channels wont match: ({input.shape[1]} vs {weight.shape[1] * group}).")
    offset = offset.contiguous()  # the reference does not check offset; a strided view would be misread
    bias = bias.contiguous()
    lib = L.get_lib()
    g = _geom(input.shape, weight.shape[0], k, s, p, d, group, deformable_groups, im2col_step)
    dt = L.dtype_code(input, allow_f64=True)
    Do, Ho, Wo = _out_dims(g)
    if min(Do, Ho, Wo) <= 0:
        L.check(-4, "deform_conv_forward")
    K = k[0] * k[1] * k[2]
    if tuple(offset.shape) != (g.B, deformable_groups * 3 * K, Do, Ho, Wo):
        raise RuntimeError(f"offset shape {tuple(offset.shape)} does not match {(g.B, deformable_groups * 3 * K, Do, Ho, Wo)}")
    out = torch.empty((g.B, g.Cout, Do, Ho, Wo), dtype=input.dtype, device=input.device)
    wsb = lib.dlka_deform_conv3d_forward_workspace(byref(g), dt)
    ws = L.scratch(wsb, input)
    rc = lib.dlka_deform_conv3d_forward(L.ptr(input), L.ptr(offset), L.ptr(weight), L.ptr(bias), L.ptr(out), L.ptr(ws), wsb,
                                        byref(g), dt, L.stream_ptr(input))
    L.check(rc, "deform_conv_forward")
    return out


def deform_conv3d_backward(input, weight, bias, offset, grad_output, kernel_size, stride, padding, dilation, group,
                           deformable_groups, im2col_step=64, need=(True, True, True, True)):
    """``D3D.deform_conv_backward`` (3D/dcn/src/deform_conv.h:49-91) -> (grad_input, grad_offset, grad_weight, grad_bias)."""
    if not input.is_contiguous():
        raise RuntimeError("input tensor has to be contiguous")
    if not weight.is_contiguous():
        raise RuntimeError("weight tensor has to be contiguous")
    L.require_device(input, weight, bias, offset, grad_output)
    _require_input_dtype(input, weight=weight, bias=bias, offset=offset, grad_output=grad_output)
    k, s, p, d = _triple(kernel_size), _triple(stride), _triple(padding), _triple(dilation)
    offset = offset.contiguous()
    grad_output = grad_output.contiguous()  # reference: permute(...).contiguous() copies, deform_conv_cuda.cu:228
    lib = L.get_lib()
    g = _geom(input.shape, weight.shape[0], k, s, p, d, group, deformable_groups, im2col_step)
    dt = L.dtype_code(input, allow_f64=True)
    Do, Ho, Wo = _out_dims(g)
    if tuple(grad_output.shape) != (g.B, g.Cout, Do, Ho, Wo):  # deform_conv_cuda.cu:193-200
        raise RuntimeError(f"Input shape and grad_out shape wont match: ({(g.B, g.Cout, Do, Ho, Wo)} vs {tuple(grad_output.shape)}).")
    gi = torch.empty_like(input) if need[0] else None
    go = torch.empty_like(offset) if need[1] else None
    gw = torch.empty_like(weight) if need[2] else None
    gb = torch.empty_like(bias, memory_format=torch.contiguous_format) if need[3] else None
    wsb = lib.dlka_deform_conv3d_backward_workspace(byref(g), dt)
    ws = L.scratch(wsb, input)
    rc = lib.dlka_deform_conv3d_backward(L.ptr(input), L.ptr(offset), L.ptr(weight), L.ptr(grad_output), L.ptr(gi), L.ptr(go),
                                         L.ptr(gw), L.ptr(gb), L.ptr(ws), wsb, byref(g), dt, L.stream_ptr(input))
    L.check(rc, "deform_conv_backward")
    return gi, go, gw, gb


def deform_conv3d_sample_index(offset, in_size: Sequence[int], kernel_size, stride, padding, dilation, deformable_groups=1, path=0):
    """floor() indices [B,dg,K,Do,Ho,Wo,3] (int32) and guard mask [B,dg,K,Do,Ho,Wo] (uint8).
    ``path``: 0 = ``sample_cell3`` on its own (the one rule every kernel calls; the fixed-point grad_input kernel calls it directly),
    1 = through ``setup_tap`` (general kernels), 2 = through ``gather_describe3`` (channels-last gathers), 3 = through ``lane_tap``
    (grad_input window kernels); idx = 0 where the mask is 0."""
    L.require_device(offset)
    k, s, p, d = _triple(kernel_size), _triple(stride), _triple(padding), _triple(dilation)
    offset = offset.contiguous()
    B = offset.shape[0]
    g = _geom((B, deformable_groups, *in_size), deformable_groups, k, s, p, d, 1, deformable_groups, 64)
    Do, Ho, Wo = _out_dims(g)
    K = k[0] * k[1] * k[2]
    idx = torch.empty((B, deformable_groups, K, Do, Ho, Wo, 3), dtype=torch.int32, device=offset.device)
    mask = torch.empty((B, deformable_groups, K, Do, Ho, Wo), dtype=torch.uint8, device=offset.device)
    rc = L.get_lib().dlka_deform_conv3d_sample_index_path(L.ptr(offset), L.ptr(idx), L.ptr(mask), byref(g), L.dtype_code(offset),
                                                          int(path), L.stream_ptr(offset))
    L.check(rc, "deform_conv3d_sample_index")
    return idx, mask


# ------------------------------------------------------------------------------------------------------------
# 2-D deformable conv (torchvision semantics)
# ------------------------------------------------------------------------------------------------------------
def _geom2d(x_shape, weight_shape, s, p, d, offset_channels):
    B, C, H, W = (int(v) for v in x_shape)
    Cout, Cg, kh, kw = (int(v) for v in weight_shape)
    if C % Cg != 0:
        raise RuntimeError("input channels must be divisible by weight.shape[1]")
    og = offset_channels // (2 * kh * kw)
    if og == 0 or offset_channels != og * 2 * kh * kw:
        raise RuntimeError(f"offset.shape[1] = {offset_channels} is not a multiple of 2*kh*kw = {2 * kh * kw}")
    return L.ConvGeom(B, C, 1, H, W, Cout, 1, kh, kw, 1, s[0], s[1], 0, p[0], p[1], 1, d[0], d[1], C // Cg, og, 64)


def deform_conv2d_forward(input, offset, weight, bias=None, stride=1, padding=0, dilation=1):
    L.require_device(input, offset, weight, bias)
    _require_input_dtype(input, offset=offset, weight=weight, bias=bias)
    s, p, d = _pair(stride), _pair(padding), _pair(dilation)
    input, offset, weight = input.contiguous(), offset.contiguous(), weight.contiguous()
    bias = None if bias is None else bias.contiguous()
    g = _geom2d(input.shape, weight.shape, s, p, d, offset.shape[1])
    lib = L.get_lib()
    dt = L.dtype_code(input, allow_f64=True)
    _, Ho, Wo = _out_dims(g)
    if tuple(offset.shape[2:]) != (Ho, Wo):
        raise RuntimeError(f"offset spatial size {tuple(offset.shape[2:])} does not match output {(Ho, Wo)}")
    out = torch.empty((g.B, g.Cout, Ho, Wo), dtype=input.dtype, device=input.device)
    wsb = lib.dlka_deform_conv2d_forward_workspace(byref(g), dt)
    ws = L.scratch(wsb, input)
    rc = lib.dlka_deform_conv2d_forward(L.ptr(input), L.ptr(offset), L.ptr(weight), L.ptr(bias), L.ptr(out), L.ptr(ws), wsb,
                                        byref(g), dt, L.stream_ptr(input))
    L.check(rc, "deform_conv2d")
    return out


def deform_conv2d_backward(input, offset, weight, grad_output, stride=1, padding=0, dilation=1, with_bias=False,
                           need=(True, True, True)):
    L.require_device(input, offset, weight, grad_output)
    _require_input_dtype(input, offset=offset, weight=weight, grad_output=grad_output)
    s, p, d = _pair(stride), _pair(padding), _pair(dilation)
    input, offset, weight, grad_output = input.contiguous(), offset.contiguous(), weight.contiguous(), grad_output.contiguous()
    g = _geom2d(input.shape, weight.shape, s, p, d, offset.shape[1])
    lib = L.get_lib()
    dt = L.dtype_code(input, allow_f64=True)
    gi = torch.empty_like(input) if need[0] else None
    go = torch.empty_like(offset) if need[1] else None
    gw = torch.empty_like(weight) if need[2] else None
    gb = torch.empty((g.Cout,), dtype=input.dtype, device=input.device) if with_bias else None
    wsb = lib.dlka_deform_conv2d_backward_workspace(byref(g), dt)
    ws = L.scratch(wsb, input)
    rc = lib.dlka_deform_conv2d_backward(L.ptr(input), L.ptr(offset), L.ptr(weight), L.ptr(grad_output), L.ptr(gi), L.ptr(go),
                                         L.ptr(gw), L.ptr(gb), L.ptr(ws), wsb, byref(g), dt, L.stream_ptr(input))
    L.check(rc, "deform_conv2d backward")
    return gi, go, gw, gb


def deform_conv2d_sample_index(offset, in_size: Sequence[int], kernel_size, stride=1, padding=0, dilation=1, offset_groups=1, path=0):
    """2-D index-parity entry: floor cell [B,og,K,Ho,Wo,2] (int32; 0 outside `reach`) and mask [B,og,K,Ho,Wo] (uint8: bit 0 = sample inside
    the guard, bit 1 = reach).  ``path``: 0 = ``sample_cell2`` on its own, 1 = ``setup_tap<2>`` (general kernels), 2 = ``describe2``
    (channels-last depthwise kernels)."""
    L.require_device(offset)
    k, s, p, d = _pair(kernel_size), _pair(stride), _pair(padding), _pair(dilation)
    offset = offset.contiguous()
    B, H, W = int(offset.shape[0]), int(in_size[0]), int(in_size[1])
    g = L.ConvGeom(B, offset_groups, 1, H, W, offset_groups, 1, k[0], k[1], 1, s[0], s[1], 0, p[0], p[1], 1, d[0], d[1], 1, offset_groups, 64)
    _, Ho, Wo = _out_dims(g)
    K = k[0] * k[1]
    if tuple(offset.shape) != (B, offset_groups * 2 * K, Ho, Wo):
        raise RuntimeError(f"offset shape {tuple(offset.shape)} does not match {(B, offset_groups * 2 * K, Ho, Wo)}")
    idx = torch.empty((B, offset_groups, K, Ho, Wo, 2), dtype=torch.int32, device=offset.device)
    mask = torch.empty((B, offset_groups, K, Ho, Wo), dtype=torch.uint8, device=offset.device)
    rc = L.get_lib().dlka_deform_conv2d_sample_index_path(L.ptr(offset), L.ptr(idx), L.ptr(mask), byref(g), L.dtype_code(offset), int(path),
                                                          L.stream_ptr(offset))
    L.check(rc, "deform_conv2d_sample_index")
    return idx, mask


def _geom_dw2d_cl(x, weight, padding, dilation):
    B, H, W, C = (int(v) for v in x.shape)
    p, d = _pair(padding), _pair(dilation)
    if tuple(weight.shape[:2]) != (C, 1):
        raise RuntimeError(f"depthwise weight [C][1][kh][kw] expected, got {tuple(weight.shape)}")
    kh, kw = int(weight.shape[2]), int(weight.shape[3])
    return L.ConvGeom(B, C, 1, H, W, C, 1, kh, kw, 1, 1, 1, 0, p[0], p[1], 1, d[0], d[1], C, 1, 64)


def deform_dwconv2d_forward_cl(x, offset, weight, padding, dilation=1):
    """The 2-D D-LKA block's depthwise deformable conv on its own, channels-last (cl_ddw2d.hip): x [B,H,W,C], offset [B,2K,H,W] planar
    ((dy, dx) per tap, torchvision layout), weight [C,1,kh,kw] -> out [B,H,W,C]."""
    L.require_device(x, offset, weight)
    x, offset, weight = x.contiguous(), offset.contiguous(), weight.contiguous()
    g = _geom_dw2d_cl(x, weight, padding, dilation)
    lib, dt = L.get_lib(), L.dtype_code(x)
    out = torch.empty_like(x)
    wsb = lib.dlka_deform_dwconv2d_cl_workspace(byref(g), dt, 0)
    ws = L.scratch(wsb, x)
    rc = lib.dlka_deform_dwconv2d_forward_cl(L.ptr(x), L.ptr(offset), L.ptr(weight), L.ptr(out), L.ptr(ws), wsb, byref(g), dt, L.stream_ptr(x))
    L.check(rc, "deform_dwconv2d_forward_cl")
    return out


def deform_dwconv2d_backward_cl(x, offset, weight, grad_out, padding, dilation=1):
    """-> (grad_x [B,H,W,C], grad_offset [B,2K,H,W], grad_weight [C,1,kh,kw])."""
    L.require_device(x, offset, weight, grad_out)
    x, offset, weight, grad_out = x.contiguous(), offset.contiguous(), weight.contiguous(), grad_out.contiguous()
    g = _geom_dw2d_cl(x, weight, padding, dilation)
    lib, dt = L.get_lib(), L.dtype_code(x)
    gx, go, gw = torch.empty_like(x), torch.empty_like(offset), torch.empty_like(weight)
    wsb = lib.dlka_deform_dwconv2d_cl_workspace(byref(g), dt, 1)
    ws = L.scratch(wsb, x)
    rc = lib.dlka_deform_dwconv2d_backward_cl(L.ptr(x), L.ptr(offset), L.ptr(weight), L.ptr(grad_out), L.ptr(gx), L.ptr(go), L.ptr(gw), L.ptr(ws),
                                              wsb, byref(g), dt, L.stream_ptr(x))
    L.check(rc, "deform_dwconv2d_backward_cl")
    return gx, go, gw


# ------------------------------------------------------------------------------------------------------------
# plain conv
# ------------------------------------------------------------------------------------------------------------
def conv3d_forward(input, weight, bias=None, stride=1, padding=0, dilation=1, groups=1):
    L.require_device(input, weight, bias)
    _require_input_dtype(input, weight=weight, bias=bias)
    s, p, d = _triple(stride), _triple(padding), _triple(dilation)
    input, weight = input.contiguous(), weight.contiguous()
    bias = None if bias is None else bias.contiguous()
    g = _geom(input.shape, weight.shape[0], tuple(weight.shape[2:5]), s, p, d, groups)
    lib = L.get_lib()
    dt = L.dtype_code(input, allow_f64=True)
    Do, Ho, Wo = _out_dims(g)
    out = torch.empty((g.B, g.Cout, Do, Ho, Wo), dtype=input.dtype, device=input.device)
    wsb = lib.dlka_conv3d_forward_workspace(byref(g), dt)
    ws = L.scratch(wsb, input)
    rc = lib.dlka_conv3d_forward(L.ptr(input), L.ptr(weight), L.ptr(bias), L.ptr(out), L.ptr(ws), wsb, byref(g), dt,
                                 L.stream_ptr(input))
    L.check(rc, "conv3d")
    return out


def conv3d_backward(input, weight, grad_output, stride=1, padding=0, dilation=1, groups=1, need=(True, True, True)):
    L.require_device(input, weight, grad_output)
    _require_input_dtype(input, weight=weight, grad_output=grad_output)
    s, p, d = _triple(stride), _triple(padding), _triple(dilation)
    input, weight, grad_output = input.contiguous(), weight.contiguous(), grad_output.contiguous()
    g = _geom(input.shape, weight.shape[0], tuple(weight.shape[2:5]), s, p, d, groups)
    lib = L.get_lib()
    dt = L.dtype_code(input, allow_f64=True)
    gi = torch.empty_like(input) if need[0] else None
    gw = torch.empty_like(weight) if need[1] else None
    gb = torch.empty((g.Cout,), dtype=input.dtype, device=input.device) if need[2] else None
    wsb = lib.dlka_conv3d_backward_workspace(byref(g), dt)
    ws = L.scratch(wsb, input)
    rc = lib.dlka_conv3d_backward(L.ptr(input), L.ptr(weight), L.ptr(grad_output), L.ptr(gi), L.ptr(gw), L.ptr(gb), L.ptr(ws), wsb,
                                  byref(g), dt, L.stream_ptr(input))
    L.check(rc, "conv3d backward")
    return gi, gw, gb


def gelu_forward(x):
    L.require_device(x)
    x = x.contiguous()
    y = torch.empty_like(x)
    L.check(L.get_lib().dlka_gelu_forward(L.ptr(x), L.ptr(y), x.numel(), L.dtype_code(x), L.stream_ptr(x)), "gelu")
    return y


def gelu_backward(x, gy):
    L.require_device(x, gy)
    x, gy = x.contiguous(), gy.contiguous()
    gx = torch.empty_like(x)
    L.check(L.get_lib().dlka_gelu_backward(L.ptr(x), L.ptr(gy), L.ptr(gx), x.numel(), L.dtype_code(x), L.stream_ptr(x)), "gelu bwd")
    return gx


# ------------------------------------------------------------------------------------------------------------
# planar (NCDHW) plumbing of the full net: BatchNorm3d in training mode, 1x1x1 convs on few channels (csrc/planar_ops.hip)
# ------------------------------------------------------------------------------------------------------------
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
    L.check(L.get_lib().dlka_batchnorm_planar_forward(L.ptr(x), L.ptr(weight), L.ptr(bias), L.ptr(stats), L.ptr(y), L.ptr(scratch), B, C, N, float(eps),
                                                      L.stream_ptr(x)), "batchnorm_planar_forward")
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
    L.check(L.get_lib().dlka_batchnorm_planar_backward(L.ptr(g), L.ptr(x), L.ptr(weight), L.ptr(stats), L.ptr(gx), L.ptr(gw), L.ptr(gb), L.ptr(scratch), B, C, N,
                                                       L.stream_ptr(x)), "batchnorm_planar_backward")
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
    L.check(L.get_lib().dlka_pointwise_planar_forward(L.ptr(x), L.ptr(weight), L.ptr(bias), L.ptr(y), B, Cin, Cout, x[0, 0].numel(), L.stream_ptr(x)),
            "pointwise_planar_forward")
    return y


def pointwise_planar_backward(x, weight, g, need=(True, True, True)):
    L.require_device(x, weight, g)
    B, Cin = x.shape[:2]
    Cout = weight.shape[0]
    gx = torch.empty_like(x) if need[0] else None
    gw = torch.empty_like(weight) if need[1] else None
    gb = torch.empty(Cout, dtype=torch.float32, device=x.device) if (need[1] and need[2]) else None
    if need[0] or need[1]:
        L.check(L.get_lib().dlka_pointwise_planar_backward(L.ptr(x), L.ptr(weight), L.ptr(g), L.ptr(gx), L.ptr(gw), L.ptr(gb), B, Cin, Cout, x[0, 0].numel(),
                                                           L.stream_ptr(x)), "pointwise_planar_backward")
    if need[2] and gb is None:   # frozen weight, trainable bias (fine-tuning a head): the bias gradient rides in the weight-gradient kernel, which did
        gb = g.sum(dim=[0] + list(range(2, g.dim())))   # not run — a plain reduction of grad_out (not hot: a Cout-length result)
    return gx, gw, gb


# ------------------------------------------------------------------------------------------------------------
# whole blocks
# ------------------------------------------------------------------------------------------------------------
def _ptr_struct(cls, fields, tensors):
    st = cls()
    for n, t in zip(fields, tensors):
        setattr(st, n, t.data_ptr())
    return st


def lka3d_attention_forward(x, params: Sequence[torch.Tensor]):
    """x: [B,C,D,H,W]; params: the 14 tensors in ``_lib.LKA3D_FIELDS`` order. Returns (y, saved)."""
    L.require_device(x, *params)
    x = x.contiguous()
    params = [t.contiguous() for t in params]
    B, C, D, H, W = (int(v) for v in x.shape)
    lib = L.get_lib()
    dt = L.dtype_code(x)
    sb, wb = lib.dlka_lka3d_saved_bytes(B, C, D, H, W, dt), lib.dlka_lka3d_workspace_bytes(B, C, D, H, W, dt)
    if sb == 0:
        L.check(-4, "lka3d_attention_forward")
    saved, ws = L.scratch(sb, x), L.scratch(wb, x)
    y = torch.empty_like(x)
    ps = _ptr_struct(L.Lka3dPtrs, L.LKA3D_FIELDS, params)
    rc = lib.dlka_lka3d_attention_forward(L.ptr(x), byref(ps), L.ptr(y), L.ptr(saved), sb, L.ptr(ws), wb, B, C, D, H, W, dt,
                                          L.stream_ptr(x))
    L.check(rc, "lka3d_attention_forward")
    return y, saved


def lka3d_attention_backward(x, params, grad_y, saved):
    L.require_device(x, grad_y, saved, *params)
    x, grad_y = x.contiguous(), grad_y.contiguous()
    params = [t.contiguous() for t in params]
    B, C, D, H, W = (int(v) for v in x.shape)
    lib = L.get_lib()
    dt = L.dtype_code(x)
    wb = lib.dlka_lka3d_workspace_bytes(B, C, D, H, W, dt)
    ws = L.scratch(wb, x)
    gx = torch.empty_like(x)
    grads = [torch.empty_like(t) for t in params]
    ps = _ptr_struct(L.Lka3dPtrs, L.LKA3D_FIELDS, params)
    gs = _ptr_struct(L.Lka3dPtrs, L.LKA3D_FIELDS, grads)
    rc = lib.dlka_lka3d_attention_backward(L.ptr(x), byref(ps), L.ptr(grad_y), L.ptr(saved), saved.numel(), L.ptr(gx), byref(gs),
                                           L.ptr(ws), wb, B, C, D, H, W, dt, L.stream_ptr(x))
    L.check(rc, "lka3d_attention_backward")
    return gx, grads


def lka2d_bf16_supported(C: int) -> bool:
    """Widths the DLKA_BF16 2-D block covers (channels-last fast path: C / 32 in {1, 2, 3, 4, 6, 8, 12})."""
    return C % 32 == 0 and C // 32 in (1, 2, 3, 4, 6, 8, 12)


def _lka2d_params(x, params):
    if x.dtype == torch.bfloat16:   # DLKA_BF16: bf16 ACTIVATIONS, fp32 master parameters (include/dlka.h)
        if not lka2d_bf16_supported(int(x.shape[1])):
            raise RuntimeError(f"deformable_LKA_Attention with bfloat16 activations needs C / 32 in {{1,2,3,4,6,8,12}}, got C={int(x.shape[1])}")
        return [_fp32_param(t) for t in params]
    return [t.contiguous() for t in params]


def lka2d_attention_forward(x, params: Sequence[torch.Tensor]):
    L.require_device(x, *params)
    x = x.contiguous()
    params = _lka2d_params(x, params)
    B, C, H, W = (int(v) for v in x.shape)
    lib = L.get_lib()
    dt = L.dtype_code(x)
    sb, wb = lib.dlka_lka2d_saved_bytes(B, C, H, W, dt), lib.dlka_lka2d_workspace_bytes(B, C, H, W, dt)
    if sb == 0:
        L.check(-4, "lka2d_attention_forward")
    saved, ws = L.scratch(sb, x), L.scratch(wb, x)
    y = torch.empty_like(x)
    ps = _ptr_struct(L.Lka2dPtrs, L.LKA2D_FIELDS, params)
    rc = lib.dlka_lka2d_attention_forward(L.ptr(x), byref(ps), L.ptr(y), L.ptr(saved), sb, L.ptr(ws), wb, B, C, H, W, dt,
                                          L.stream_ptr(x))
    L.check(rc, "lka2d_attention_forward")
    return y, saved


def lka2d_saved_offsets(saved, x):
    """The two predicted offset tensors ([B, 50, H, W] of conv0, [B, 98, H, W] of conv_spatial; torchvision's planar layout) inside the opaque
    ``saved`` buffer of ``lka2d_attention_forward(x, ...)`` — for the path such a call takes now (``dlka_lka2d_saved_offsets``).  Diagnostics:
    the parity tests' cell-flip analysis reads them."""
    B, C, H, W = (int(v) for v in x.shape)
    lib = L.get_lib()
    offs = (ctypes.c_size_t * 2)()
    eb = ctypes.c_int(0)
    L.check(lib.dlka_lka2d_saved_offsets(B, C, H, W, L.dtype_code(x), offs, byref(eb)), "lka2d_saved_offsets")
    dt = torch.float32 if eb.value == 4 else torch.bfloat16
    out = []
    for o, ch in zip(offs, (50, 98)):
        n = B * ch * H * W * eb.value
        out.append(saved[int(o):int(o) + n].view(dt).view(B, ch, H, W))
    return out


def lka2d_attention_backward(x, params, grad_y, saved):
    L.require_device(x, grad_y, saved, *params)
    x, grad_y = x.contiguous(), grad_y.to(x.dtype).contiguous()
    params = _lka2d_params(x, params)
    B, C, H, W = (int(v) for v in x.shape)
    lib = L.get_lib()
    dt = L.dtype_code(x)
    wb = lib.dlka_lka2d_workspace_bytes(B, C, H, W, dt)
    ws = L.scratch(wb, x)
    gx = torch.empty_like(x)
    grads = [torch.empty_like(t) for t in params]
    ps = _ptr_struct(L.Lka2dPtrs, L.LKA2D_FIELDS, params)
    gs = _ptr_struct(L.Lka2dPtrs, L.LKA2D_FIELDS, grads)
    rc = lib.dlka_lka2d_attention_backward(L.ptr(x), byref(ps), L.ptr(grad_y), L.ptr(saved), saved.numel(), L.ptr(gx), byref(gs),
                                           L.ptr(ws), wb, B, C, H, W, dt, L.stream_ptr(x))
    L.check(rc, "lka2d_attention_backward")
    return gx, grads


# ------------------------------------------------------------------------------------------------------------
# channels-last fast path (fp32): x [B, D, H, W, C]
# ------------------------------------------------------------------------------------------------------------
def _geom_cl(x_shape, cout, k, p, d, group, dg=1):
    B, D, H, W, C = (int(v) for v in x_shape)
    return L.ConvGeom(B, C, D, H, W, int(cout), *k, 1, 1, 1, *p, *d, int(group), int(dg), 64)


def conv3d_forward_cl(x, weight, bias=None, padding=0, dilation=1, groups=1, out_planar=False):
    L.require_device(x, weight, bias)
    p, d = _triple(padding), _triple(dilation)
    x, weight = x.contiguous(), weight.contiguous()
    bias = None if bias is None else bias.contiguous()
    g = _geom_cl(x.shape, weight.shape[0], tuple(weight.shape[2:5]), p, d, groups)
    lib = L.get_lib()
    dt = L.dtype_code(x)
    B, D, H, W, _ = x.shape
    shape = (B, g.Cout, D, H, W) if out_planar else (B, D, H, W, g.Cout)
    out = torch.empty(shape, dtype=x.dtype, device=x.device)
    wsb = lib.dlka_conv3d_cl_workspace(byref(g), dt, 0)
    ws = L.scratch(wsb, x)
    rc = lib.dlka_conv3d_forward_cl(L.ptr(x), L.ptr(weight), L.ptr(bias), L.ptr(out), int(out_planar), L.ptr(ws), wsb, byref(g), dt,
                                    L.stream_ptr(x))
    L.check(rc, "conv3d_forward_cl")
    return out


def conv3d_backward_cl(x, weight, grad_out, padding=0, dilation=1, groups=1, grad_out_planar=False, need=(True, True, True)):
    """-> (grad_x, grad_weight, grad_bias); a gradient ``need`` does not ask for is passed to the library as null and returned as None (no gradient asked
    for: no library call)."""
    L.require_device(x, weight, grad_out)
    p, d = _triple(padding), _triple(dilation)
    x, weight, grad_out = x.contiguous(), weight.contiguous(), grad_out.contiguous()
    g = _geom_cl(x.shape, weight.shape[0], tuple(weight.shape[2:5]), p, d, groups)
    lib = L.get_lib()
    dt = L.dtype_code(x)
    if not any(need):
        return None, None, None
    gi = torch.empty_like(x) if need[0] else None
    gw = torch.empty_like(weight) if need[1] else None
    gb = torch.empty((g.Cout,), dtype=x.dtype, device=x.device) if need[2] else None
    wsb = lib.dlka_conv3d_cl_workspace(byref(g), dt, 1)
    ws = L.scratch(wsb, x)
    rc = lib.dlka_conv3d_backward_cl(L.ptr(x), L.ptr(weight), L.ptr(grad_out), int(grad_out_planar), L.ptr(gi), L.ptr(gw), L.ptr(gb),
                                     L.ptr(ws), wsb, byref(g), dt, L.stream_ptr(x))
    L.check(rc, "conv3d_backward_cl")
    return gi, gw, gb


def deform_cl_grad_dtype(x):
    """Element type of the four gradients ``dlka_deform_conv3d_backward_cl`` writes: x's for float32; float32 for bfloat16 activations too (DLKA_BF16 there
    is mixed storage — x / out / grad_out bf16; offsets, weight, bias and ALL FOUR gradients fp32: grad_x is the fp32 accumulation target of the window
    scatter, cl_deform_bwd2.hip, grad_offset one fp32 store per element, the parameter gradients come out of ``launch_cl_wgrad<float>``, cl_wgrad.hip)."""
    return torch.float32 if x.dtype == torch.bfloat16 else x.dtype


def _deform_cl_fp32_operands(x, **named):
    """DLKA_BF16 on the channels-last deformable conv is an ACTIVATION dtype: the library reads offsets, weight and bias as fp32 whatever x is."""
    for name, t in named.items():
        if t is not None and t.dtype != (torch.float32 if x.dtype == torch.bfloat16 else x.dtype):
            raise RuntimeError(f"channels-last deformable conv: {name} must be float32 (bfloat16 is the storage of x / out / grad_out only); got {t.dtype}")


def deform_conv3d_forward_cl(x, offset, weight, bias, padding=1, dilation=1):
    """x [B,D,H,W,C] channels-last, offset [B,3K,D,H,W] planar -> out [B,D,H,W,Cout] (x's dtype; with bfloat16 x the offsets, weight and bias stay float32)."""
    L.require_device(x, offset, weight, bias)
    _deform_cl_fp32_operands(x, offset=offset, weight=weight, bias=bias)
    p, d = _triple(padding), _triple(dilation)
    x, offset, weight, bias = x.contiguous(), offset.contiguous(), weight.contiguous(), bias.contiguous()
    g = _geom_cl(x.shape, weight.shape[0], tuple(weight.shape[2:5]), p, d, 1)
    lib = L.get_lib()
    dt = L.dtype_code(x)
    B, D, H, W, _ = x.shape
    out = torch.empty((B, D, H, W, g.Cout), dtype=x.dtype, device=x.device)
    wsb = lib.dlka_deform_conv3d_cl_workspace(byref(g), dt, 0)
    ws = L.scratch(wsb, x)
    rc = lib.dlka_deform_conv3d_forward_cl(L.ptr(x), L.ptr(offset), L.ptr(weight), L.ptr(bias), L.ptr(out), L.ptr(ws), wsb, byref(g), dt,
                                           L.stream_ptr(x))
    L.check(rc, "deform_conv3d_forward_cl")
    return out


def deform_conv3d_backward_cl(x, offset, weight, grad_out, padding=1, dilation=1, need=(True, True, True, True)):
    """-> (grad_x [B,D,H,W,C], grad_offset, grad_weight, grad_bias), each of ``deform_cl_grad_dtype(x)``; a gradient ``need`` does not ask for is passed to
    the library as null and returned as None (no gradient asked for: no library call).  With bfloat16 x the library refuses grad_bias without grad_weight."""
    L.require_device(x, offset, weight, grad_out)
    _deform_cl_fp32_operands(x, offset=offset, weight=weight)
    if grad_out.dtype != x.dtype:
        raise RuntimeError(f"channels-last deformable conv: grad_out must have x's dtype ({x.dtype}), got {grad_out.dtype}")
    p, d = _triple(padding), _triple(dilation)
    x, offset, weight, grad_out = x.contiguous(), offset.contiguous(), weight.contiguous(), grad_out.contiguous()
    g = _geom_cl(x.shape, weight.shape[0], tuple(weight.shape[2:5]), p, d, 1)
    lib = L.get_lib()
    dt = L.dtype_code(x)
    if not any(need):
        return None, None, None, None
    gdt = deform_cl_grad_dtype(x)
    gi = torch.empty(x.shape, dtype=gdt, device=x.device) if need[0] else None
    go = torch.empty(offset.shape, dtype=gdt, device=x.device) if need[1] else None
    gw = torch.empty(weight.shape, dtype=gdt, device=x.device) if need[2] else None
    gb = torch.empty((g.Cout,), dtype=gdt, device=x.device) if need[3] else None
    wsb = lib.dlka_deform_conv3d_cl_workspace(byref(g), dt, 1)
    ws = L.scratch(wsb, x)
    rc = lib.dlka_deform_conv3d_backward_cl(L.ptr(x), L.ptr(offset), L.ptr(weight), L.ptr(grad_out), L.ptr(gi), L.ptr(go), L.ptr(gw),
                                            L.ptr(gb), L.ptr(ws), wsb, byref(g), dt, L.stream_ptr(x))
    L.check(rc, "deform_conv3d_backward_cl")
    return gi, go, gw, gb


def lka3d_tokens_supported(x, B, C, D, H, W, variant=0) -> bool:
    """x: a tensor or a torch dtype; variant: 0 = Synapse depthwise pair, 1 = ACDC (include/dlka.h: dlka_lka3d_variant).  float32, or bfloat16 activations (DLKA_BF16: bf16 storage of x / y / saved activations, fp32 parameters,
    offsets and accumulation)."""
    dt = x if isinstance(x, torch.dtype) else x.dtype
    if dt not in (torch.float32, torch.bfloat16):
        return False
    return bool(L.get_lib().dlka_lka3d_tokens_supported_v(B, C, D, H, W, L.DLKA_F32 if dt == torch.float32 else L.DLKA_BF16, int(variant)))


def autocast_activation_dtype(x):
    """The autocast policy of the token-layout D-LKA block (the reference registers none): inside ``torch.autocast(dtype=
    torch.bfloat16)`` the block runs on bf16 activations with fp32 parameters / accumulation; anything else keeps x's dtype."""
    try:
        on = torch.is_autocast_enabled(x.device.type)
        dt = torch.get_autocast_dtype(x.device.type) if on else None
    except (TypeError, RuntimeError):
        return x.dtype
    return torch.bfloat16 if (on and dt == torch.bfloat16 and x.dtype in (torch.float32, torch.bfloat16)) else x.dtype



def _fp32_param(t):
    """Parameters of the token-layout block are fp32 masters whatever the activation dtype is."""
    if t.dtype != torch.float32:
        raise RuntimeError(f"the token-layout D-LKA block keeps its parameters in float32 (bf16 is an ACTIVATION dtype); got {t.dtype}")
    return t.contiguous()


def lka3d_attention_tokens_forward(x, params, dims, variant=0):
    """x: [B, N, C] tokens, dims = (D, H, W) spatial extents (the reference's H, W, D). Returns (y, saved)."""
    L.require_device(x, *params)
    x = x.contiguous()
    params = [_fp32_param(t) for t in params]
    B, N, C = (int(v) for v in x.shape)
    D, H, W = (int(v) for v in dims)
    assert N == D * H * W
    lib = L.get_lib()
    dt = L.dtype_code(x)
    v = int(variant)
    sb, wb = lib.dlka_lka3d_tokens_saved_bytes_v(B, C, D, H, W, dt, v), lib.dlka_lka3d_tokens_workspace_bytes_v(B, C, D, H, W, dt, v)
    if sb == 0:
        L.check(-8, "lka3d_attention_tokens_forward")
    saved, ws = L.scratch(sb, x), L.scratch(wb, x)
    y = torch.empty_like(x)
    ps = _ptr_struct(L.Lka3dPtrs, L.LKA3D_FIELDS, params)
    rc = lib.dlka_lka3d_attention_tokens_forward_v(L.ptr(x), byref(ps), L.ptr(y), L.ptr(saved), sb, L.ptr(ws), wb, B, C, D, H, W, dt, v,
                                                   L.stream_ptr(x))
    L.check(rc, "lka3d_attention_tokens_forward")
    return y, saved


def lka3d_tokens_saved_offsets(saved, B, C, dims, act_dtype=torch.float32, variant=0):
    """The predicted sampling offsets [B, 81, D, H, W] (fp32, the reference's planar layout) inside the opaque ``saved`` buffer of a token-layout
    forward call (``dlka_lka3d_tokens_saved_offsets_v``; the NCDHW entry point's fp32 ``saved`` starts with the same four tensors).  Diagnostics:
    bench.py's health check and the cell-flip analysis of the parity tests read them."""
    D, H, W = (int(v) for v in dims)
    off = ctypes.c_size_t(0)
    dt = L.DLKA_F32 if act_dtype == torch.float32 else L.DLKA_BF16
    lib = L.get_lib()
    if lib.dlka_lka3d_tokens_saved_offsets_v(B, C, D, H, W, dt, int(variant), byref(off)) != 0:   # widths outside the token path (general NCDHW entry)
        sb = 4 if act_dtype == torch.float32 else 2
        off = ctypes.c_size_t(4 * ((B * C * D * H * W * sb + 255) & ~255))
    o = int(off.value)
    return saved[o:o + B * 81 * D * H * W * 4].view(torch.float32).view(B, 81, D, H, W)


def tblock3d_saved_offsets(saved, B, C, dims, variant=0, lka_bf16=False):
    """The same tensor inside the ``saved`` buffer of a wrapper-block forward call (``tblock3d_forward``)."""
    D, H, W = (int(v) for v in dims)
    off = ctypes.c_size_t(0)
    L.check(L.get_lib().dlka_tblock3d_saved_offsets_v(B, C, D, H, W, L.DLKA_BF16 if lka_bf16 else L.DLKA_F32, int(variant), byref(off)), "tblock3d_saved_offsets")
    o = int(off.value)
    return saved[o:o + B * 81 * D * H * W * 4].view(torch.float32).view(B, 81, D, H, W)


def tblock3d_saved_activation_signs(saved, B, C, dims, variant=0, lka_bf16=False):
    """(a1 > 0, rd > 0, rd != 0) as bool tensors [B, N, C]: the activation pattern of UnetResBlock's two LeakyReLUs in the forward call that wrote ``saved``
    (``dlka_tblock3d_saved_activations_v``; rd carries the Dropout3d multipliers: a dropped channel is all zeros, hence the third tensor).  Diagnostics for
    the parity tests' kink analysis."""
    D, H, W = (int(v) for v in dims)
    offs = (ctypes.c_size_t * 2)()
    L.check(L.get_lib().dlka_tblock3d_saved_activations_v(B, C, D, H, W, L.DLKA_BF16 if lka_bf16 else L.DLKA_F32, int(variant), offs), "tblock3d_saved_activations")
    n = B * D * H * W * C
    a1 = saved[int(offs[0]):int(offs[0]) + n * 4].view(torch.float32).view(B, D * H * W, C)
    rd = saved[int(offs[1]):int(offs[1]) + n * 4].view(torch.float32).view(B, D * H * W, C)
    return a1 > 0, rd > 0, rd != 0


def lka3d_attention_tokens_backward(x, params, grad_y, saved, dims, variant=0, side_stream=None):
    """side_stream (a torch.cuda.Stream, optional): the pass in two parts (``dlka_lka3d_attention_tokens_backward_phase_v``) — the data-gradient chain on the current
    stream, the five weight-gradient launches and the fold of their partial sums on ``side_stream`` behind an event — and NOT joined: the returned parameter gradients are
    complete only once the current stream has waited for ``side_stream`` (``transformerblock.WgradOverlap`` joins once per backward pass).  Returns (gx, grads, keep):
    ``keep`` = what the side stream still reads, to be held until the join.  "inline": both parts on the current stream (tests)."""
    L.require_device(x, grad_y, saved, *params)
    x, grad_y = x.contiguous(), grad_y.to(x.dtype).contiguous()
    params = [_fp32_param(t) for t in params]
    B, N, C = (int(v) for v in x.shape)
    D, H, W = (int(v) for v in dims)
    lib = L.get_lib()
    dt = L.dtype_code(x)
    wb = lib.dlka_lka3d_tokens_workspace_bytes_v(B, C, D, H, W, dt, int(variant))
    ws = L.scratch(wb, x)
    gx = torch.empty_like(x)
    grads = [torch.empty_like(t) for t in params]
    ps = _ptr_struct(L.Lka3dPtrs, L.LKA3D_FIELDS, params)
    gs = _ptr_struct(L.Lka3dPtrs, L.LKA3D_FIELDS, grads)
    if side_stream is not None:
        pb = lib.dlka_lka3d_tokens_partials_bytes_v(B, C, D, H, W, dt, int(variant))
        part = L.scratch(pb, x)
        nplan = lib.dlka_wgrad_finalize_plan_bytes(1)
        plan = torch.zeros(nplan, dtype=torch.uint8)   # host job table of ONE block (its folds are launched per slot: no device copy is needed)
        planp = ctypes.c_void_p(plan.data_ptr())
        L.check(lib.dlka_wgrad_finalize_plan_init(planp, nplan, 1), "wgrad_finalize_plan_init")
        args = (L.ptr(x), byref(ps), L.ptr(grad_y), L.ptr(saved), saved.numel(), L.ptr(gx), byref(gs), L.ptr(ws), wb, L.ptr(part), pb)
        tail = (B, C, D, H, W, dt, int(variant))
        cur_ptr = L.stream_ptr(x)
        L.check(lib.dlka_lka3d_attention_tokens_backward_phase_v(*args, None, 0, 1, *tail, cur_ptr), "lka3d_attention_tokens_backward (data chain)")
        if isinstance(side_stream, str):
            sp = cur_ptr
        else:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(x.device))
            side_stream.wait_event(ev)
            sp = ctypes.c_void_p(side_stream.cuda_stream)
        L.check(lib.dlka_lka3d_attention_tokens_backward_phase_v(*args, planp, 0, 2, *tail, sp), "lka3d_attention_tokens_backward (weight gradients)")
        L.check(lib.dlka_wgrad_finalize_run_slot(planp, 0, sp), "wgrad_finalize_run_slot")
        return gx, grads, [ws, part, grad_y, saved, x]
    rc = lib.dlka_lka3d_attention_tokens_backward_v(L.ptr(x), byref(ps), L.ptr(grad_y), L.ptr(saved), saved.numel(), L.ptr(gx), byref(gs),
                                                  L.ptr(ws), wb, B, C, D, H, W, dt, int(variant), L.stream_ptr(x))
    L.check(rc, "lka3d_attention_tokens_backward")
    return gx, grads


# ------------------------------------------------------------------------------------------------------------
# TransformerBlock_3D_single_deform_LKA (transformerblock.py:570-630): the wrapper around the D-LKA block
# ------------------------------------------------------------------------------------------------------------
def tblock3d_supported(x, B, C, D, H, W, variant=0) -> bool:
    if x.dtype != torch.float32:
        return False
    return bool(L.get_lib().dlka_tblock3d_supported_v(B, C, D, H, W, L.DLKA_F32, int(variant)))


def tblock3d_lka_bf16_supported(B, C, D, H, W, variant=0) -> bool:
    """The wrapper block's MIXED mode (include/dlka.h: dtype = DLKA_BF16 on dlka_tblock3d_*): fp32 wrapper tensors, the D-LKA attention inside on bf16 activations."""
    return bool(L.get_lib().dlka_tblock3d_supported_v(B, C, D, H, W, L.DLKA_BF16, int(variant)))


def _opt_ptr_struct(cls, fields, tensors):
    st = cls()
    for f, t in zip(fields, tensors):
        setattr(st, f, None if t is None else L.ptr(t))
    return st


def tblock3d_forward(x, x_planar, tparams, lka_params, drop_mask, training, bn_stats, dims, ln_eps=1e-5, bn_eps=1e-5, variant=0, lka_bf16=False):
    """x: [B, C, N...] contiguous NCDHW (x_planar) or [B, N, C] tokens (fp32); dims = the reference's (H, W, D).
    Returns (y tokens [B, N, C], saved).  bn_stats [6*C] is written (training) or read (eval).
    lka_bf16: the MIXED mode — the D-LKA attention inside runs on bf16 activations (DLKA_BF16), the wrapper's own tensors stay fp32."""
    L.require_device(x, bn_stats, drop_mask, *[t for t in tparams if t is not None], *lka_params)
    assert x.is_contiguous() and bn_stats.is_contiguous()
    tparams = [None if t is None else t.contiguous() for t in tparams]
    lka_params = [t.contiguous() for t in lka_params]
    D, H, W = (int(v) for v in dims)
    N = D * H * W
    B = int(x.shape[0])
    C = int(x.shape[1] if x_planar else x.shape[-1])
    assert x.numel() == B * N * C
    lib = L.get_lib()
    if x.dtype != torch.float32:
        raise RuntimeError("tblock3d_forward: the wrapper block takes float32 tensors (lka_bf16 selects bf16 activations for the D-LKA attention inside)")
    dt = L.DLKA_BF16 if lka_bf16 else L.DLKA_F32
    v = int(variant)
    sb, wb = lib.dlka_tblock3d_saved_bytes_v(B, C, D, H, W, dt, v), lib.dlka_tblock3d_workspace_bytes_v(B, C, D, H, W, dt, v)
    if sb == 0:
        L.check(-8, "tblock3d_forward")
    saved, ws = L.scratch(sb, x), L.scratch(wb, x)
    y = torch.empty((B, N, C), dtype=x.dtype, device=x.device)
    ps = _opt_ptr_struct(L.TBlock3dPtrs, L.TBLOCK3D_FIELDS, tparams)
    lk = _ptr_struct(L.Lka3dPtrs, L.LKA3D_FIELDS, lka_params)
    rc = lib.dlka_tblock3d_forward_v(L.ptr(x), int(bool(x_planar)), byref(ps), byref(lk), L.ptr(drop_mask), int(bool(training)), L.ptr(bn_stats),
                                     L.ptr(y), L.ptr(saved), sb, L.ptr(ws), wb, B, C, D, H, W, float(ln_eps), float(bn_eps), dt, v, L.stream_ptr(x))
    L.check(rc, "tblock3d_forward")
    return y, saved


def tblock3d_backward(tparams, lka_params, drop_mask, training, bn_stats, grad_y, saved, dims, variant=0, lka_bf16=False, side_stream=None):
    """Returns (grad_x tokens [B, N, C], grads of tparams (None where the parameter is None), grads of lka_params).

    side_stream (a torch.cuda.Stream, optional): the pass is issued in two parts (``dlka_tblock3d_backward_phase_v``) — the data-gradient chain on the current stream,
    the weight gradients on ``side_stream`` behind an event — and NOT joined: every returned tensor that phase 2 writes is then complete only once the current stream has
    waited for ``side_stream`` (the caller's job: ``transformerblock.WgradOverlap`` joins once per backward pass).  The returned fourth element is the list of tensors
    that must stay alive until that join."""
    L.require_device(grad_y, saved, bn_stats)
    grad_y = grad_y.contiguous()
    tparams = [None if t is None else t.contiguous() for t in tparams]
    lka_params = [t.contiguous() for t in lka_params]
    B, N, C = (int(v) for v in grad_y.shape)
    D, H, W = (int(v) for v in dims)
    lib = L.get_lib()
    dt = L.DLKA_BF16 if lka_bf16 else L.DLKA_F32
    grad_y = grad_y.float()
    wb = lib.dlka_tblock3d_workspace_bytes_v(B, C, D, H, W, dt, int(variant))
    ws = L.scratch(wb, grad_y)
    gx = torch.empty_like(grad_y)
    tg = [None if t is None else torch.empty_like(t) for t in tparams]
    lg = [torch.empty_like(t) for t in lka_params]
    ps = _opt_ptr_struct(L.TBlock3dPtrs, L.TBLOCK3D_FIELDS, tparams)
    lk = _ptr_struct(L.Lka3dPtrs, L.LKA3D_FIELDS, lka_params)
    gs = _opt_ptr_struct(L.TBlock3dPtrs, L.TBLOCK3D_FIELDS, tg)
    gl = _ptr_struct(L.Lka3dPtrs, L.LKA3D_FIELDS, lg)
    args = (byref(ps), byref(lk), L.ptr(drop_mask), int(bool(training)), L.ptr(bn_stats), L.ptr(grad_y), L.ptr(saved),
            saved.numel(), L.ptr(gx), byref(gs), byref(gl), L.ptr(ws), wb, B, C, D, H, W, dt, int(variant))
    if side_stream is None:
        L.check(lib.dlka_tblock3d_backward_v(*args, L.stream_ptr(grad_y)), "tblock3d_backward")
        return gx, tg, lg
    if isinstance(side_stream, str):   # "inline": both parts back to back on the current stream (tests: the split pass equals the whole one)
        L.check(lib.dlka_tblock3d_backward_phase_v(*args, 1, L.stream_ptr(grad_y)), "tblock3d_backward (data chain)")
        L.check(lib.dlka_tblock3d_backward_phase_v(*args, 2, L.stream_ptr(grad_y)), "tblock3d_backward (weight gradients)")
        return gx, tg, lg
    cur = torch.cuda.current_stream(grad_y.device)
    L.check(lib.dlka_tblock3d_backward_phase_v(*args, 1, L.stream_ptr(grad_y)), "tblock3d_backward (data chain)")
    ev = torch.cuda.Event()
    ev.record(cur)
    side_stream.wait_event(ev)
    L.check(lib.dlka_tblock3d_backward_phase_v(*args, 2, ctypes.c_void_p(side_stream.cuda_stream)), "tblock3d_backward (weight gradients)")
    # What phase 2 READS stays referenced until the caller's join: memory released after the join is reused by work that is ordered behind it, so no
    # record_stream() is needed.  What it WRITES — the parameter gradients — must NOT be referenced: autograd's AccumulateGrad takes ownership of a returned
    # gradient only while nobody else holds it, and would otherwise COPY it on the current stream, i.e. before the side stream has written it (seen as garbage
    # gradients, profiles/r08_notes.md); as `.grad` they outlive the join by themselves.
    keep = [ws, grad_y, saved, bn_stats, drop_mask]
    return gx, tg, lg, keep


# ---- the wrapper's pieces, one by one (used by UnetResBlock standalone and by the parity tests) ---------------------------
def layernorm_tokens_forward(x, x_planar, pos, weight, bias, eps=1e-5):
    """x: NCDHW-contiguous [B, C, ...] (x_planar) or tokens [B, N, C].  Returns (xt, xn, stats[M, 2])."""
    L.require_device(x, pos, weight, bias)
    x = x.contiguous()
    B = int(x.shape[0])
    C = int(x.shape[1] if x_planar else x.shape[-1])
    N = x.numel() // (B * C)
    xt = torch.empty((B, N, C), dtype=x.dtype, device=x.device)
    xn = torch.empty_like(xt)
    stats = torch.empty((B * N, 2), dtype=torch.float32, device=x.device)
    rc = L.get_lib().dlka_layernorm_tokens_forward(L.ptr(x), int(bool(x_planar)), L.ptr(None if pos is None else pos.contiguous()), L.ptr(weight.contiguous()),
                                                   L.ptr(bias.contiguous()), L.ptr(xt), L.ptr(xn), L.ptr(stats), B, N, C, float(eps), L.dtype_code(x),
                                                   L.stream_ptr(x))
    L.check(rc, "layernorm_tokens_forward")
    return xt, xn, stats


def layernorm_tokens_backward(g_xn, g_res, xt, stats, weight, with_pos=False):
    L.require_device(g_xn, g_res, xt, stats, weight)
    B, N, C = (int(v) for v in xt.shape)
    g_xn = g_xn.contiguous()
    g_res = None if g_res is None else g_res.contiguous()
    gxt = torch.empty_like(xt)
    gw, gb = torch.empty_like(weight), torch.empty_like(weight)
    gpos = torch.empty((1, N, C), dtype=xt.dtype, device=xt.device) if with_pos else None
    rc = L.get_lib().dlka_layernorm_tokens_backward(L.ptr(g_xn), L.ptr(g_res), L.ptr(xt), L.ptr(stats), L.ptr(weight.contiguous()), L.ptr(gxt), L.ptr(gw),
                                                    L.ptr(gb), L.ptr(gpos), B, N, C, L.dtype_code(xt), L.stream_ptr(xt))
    L.check(rc, "layernorm_tokens_backward")
    return gxt, gw, gb, gpos


def scale_residual_forward(xt, e, gamma):
    L.require_device(xt, e, gamma)
    xt, e = xt.contiguous(), e.contiguous()
    out = torch.empty_like(xt)
    C = int(xt.shape[-1])
    rc = L.get_lib().dlka_scale_residual_forward(L.ptr(xt), L.ptr(e), L.ptr(gamma.contiguous()), L.ptr(out), xt.numel() // C, C, L.dtype_code(xt),
                                                 L.stream_ptr(xt))
    L.check(rc, "scale_residual_forward")
    return out


def scale_residual_backward(g, e, gamma):
    L.require_device(g, e, gamma)
    g, e = g.contiguous(), e.contiguous()
    ge, gg = torch.empty_like(e), torch.empty_like(gamma)
    C = int(e.shape[-1])
    rc = L.get_lib().dlka_scale_residual_backward(L.ptr(g), L.ptr(e), L.ptr(gamma.contiguous()), L.ptr(ge), L.ptr(gg), e.numel() // C, C, L.dtype_code(e),
                                                  L.stream_ptr(e))
    L.check(rc, "scale_residual_backward")
    return ge, gg


def batchnorm_cl_forward(x, res, weight, bias, stats, training, eps=1e-5, slope=0.01):
    """x: channels-last [..., C].  y = LeakyReLU(BN(x) (+ res)).  stats [3*C] written (training) or read (eval: {mean, rstd})."""
    L.require_device(x, res, weight, bias, stats)
    x = x.contiguous()
    res = None if res is None else res.contiguous()
    C = int(x.shape[-1])
    y = torch.empty_like(x)
    scr = torch.empty(2 * C, dtype=torch.float32, device=x.device)
    rc = L.get_lib().dlka_batchnorm_cl_forward(L.ptr(x), L.ptr(res), L.ptr(weight.contiguous()), L.ptr(bias.contiguous()), L.ptr(stats), int(bool(training)),
                                               L.ptr(y), L.ptr(scr), x.numel() // C, C, float(eps), float(slope), L.dtype_code(x), L.stream_ptr(x))
    L.check(rc, "batchnorm_cl_forward")
    return y


def batchnorm_cl_backward(g, x, y, weight, stats, training, with_res=False, slope=0.01):
    L.require_device(g, x, y, weight, stats)
    g, x, y = g.contiguous(), x.contiguous(), y.contiguous()
    C = int(x.shape[-1])
    gx = torch.empty_like(x)
    gres = torch.empty_like(x) if with_res else None
    gw, gb = torch.empty_like(weight), torch.empty_like(weight)
    scr = torch.empty(2 * C, dtype=torch.float32, device=x.device)
    rc = L.get_lib().dlka_batchnorm_cl_backward(L.ptr(g), L.ptr(x), L.ptr(y), L.ptr(weight.contiguous()), L.ptr(stats), int(bool(training)), L.ptr(gx),
                                                L.ptr(gres), L.ptr(gw), L.ptr(gb), L.ptr(scr), x.numel() // C, C, float(slope), L.dtype_code(x),
                                                L.stream_ptr(x))
    L.check(rc, "batchnorm_cl_backward")
    return gx, gres, gw, gb


def channel_scale(x, mask):
    """x [B, ..., C] channels-last, mask [B, C]."""
    L.require_device(x, mask)
    x, mask = x.contiguous(), mask.contiguous()
    B, C = int(x.shape[0]), int(x.shape[-1])
    y = torch.empty_like(x)
    rc = L.get_lib().dlka_channel_scale(L.ptr(x), L.ptr(mask), L.ptr(y), B, x.numel() // (B * C), C, L.dtype_code(x), L.stream_ptr(x))
    L.check(rc, "channel_scale")
    return y


def ncdhw_to_ndhwc(x):
    """[B, C, *S] contiguous -> [B, *S, C] contiguous (HIP transpose)."""
    L.require_device(x)
    x = x.contiguous()
    B, C = int(x.shape[0]), int(x.shape[1])
    out = torch.empty((B, *x.shape[2:], C), dtype=x.dtype, device=x.device)
    L.check(L.get_lib().dlka_ncdhw_to_ndhwc(L.ptr(x), L.ptr(out), B, C, x.numel() // (B * C), L.dtype_code(x), L.stream_ptr(x)), "ncdhw_to_ndhwc")
    return out


def ndhwc_to_ncdhw(x):
    L.require_device(x)
    x = x.contiguous()
    B, C = int(x.shape[0]), int(x.shape[-1])
    out = torch.empty((B, C, *x.shape[1:-1]), dtype=x.dtype, device=x.device)
    L.check(L.get_lib().dlka_ndhwc_to_ncdhw(L.ptr(x), L.ptr(out), B, C, x.numel() // (B * C), L.dtype_code(x), L.stream_ptr(x)), "ndhwc_to_ncdhw")
    return out


# ---- sliding-window prediction with test-time mirroring (include/dlka.h: dlka_tiles_*) ---------------------------------------------------
def _int_array(vals):
    vals = [int(v) for v in vals]
    return (ctypes.c_int * max(len(vals), 1))(*vals)


def tiles_gather(x, origins, masks, patch, pad_lo, pad_value=0.0):
    """x (C, X, Y, Z) fp32, unpadded; origins [(x, y, z)] in padded coordinates; masks: mirror masks (bit 0 = x, 1 = y, 2 = z).
    Returns the network input [T*M, C, pd, ph, pw] (b = t*M + m) = torch.flip of the constant-padded slice."""
    L.require_device(x)
    if x.dtype != torch.float32 or x.ndim != 4:
        raise RuntimeError(f"tiles_gather: x must be a (C, X, Y, Z) float32 tensor, got {tuple(x.shape)} {x.dtype}")
    x = x.contiguous()
    T, M = len(origins), len(masks)
    pd, ph, pw = (int(v) for v in patch)
    out = torch.empty((T * M, x.shape[0], pd, ph, pw), dtype=torch.float32, device=x.device)
    L.check(L.get_lib().dlka_tiles_gather(L.ptr(x), *x.shape, _int_array(v for o in origins for v in o), T, _int_array(masks), M, pd, ph, pw,
                                          *(int(v) for v in pad_lo), float(pad_value), L.ptr(out), L.stream_ptr(x)), "tiles_gather")
    return out


def tiles_blend(logits, nonlin: int, mirror_scale: float, gauss, score, weight, origins, masks):
    """score [K, X', Y', Z'] / weight [X', Y', Z'] (fp32, in place) += the chunk's blended prediction; logits [T*M, K, pd, ph, pw] fp32 or bf16;
    nonlin: L.DLKA_TILES_*; gauss [pd, ph, pw] fp32 or None."""
    L.require_device(logits, gauss, score, weight)
    if score.dtype != torch.float32 or weight.dtype != torch.float32 or not score.is_contiguous() or not weight.is_contiguous():
        raise RuntimeError("tiles_blend: score and weight must be contiguous float32 tensors (updated in place)")
    logits = logits.contiguous()
    T, M = len(origins), len(masks)
    K = logits.shape[1]
    if logits.ndim != 5 or logits.shape[0] != T * M or score.shape != (K,) + tuple(weight.shape):
        raise RuntimeError(f"tiles_blend: logits {tuple(logits.shape)} / score {tuple(score.shape)} / weight {tuple(weight.shape)} do not fit T={T}, M={M}")
    if gauss is not None:
        gauss = gauss.contiguous().float()
        if tuple(gauss.shape) != tuple(logits.shape[2:]):
            raise RuntimeError(f"tiles_blend: importance map {tuple(gauss.shape)} is not the patch {tuple(logits.shape[2:])}")
    L.check(L.get_lib().dlka_tiles_blend(L.ptr(logits), L.dtype_code(logits), K, int(nonlin), float(mirror_scale), L.ptr(gauss), L.ptr(score),
                                         L.ptr(weight), *weight.shape, _int_array(v for o in origins for v in o), T, _int_array(masks), M,
                                         *logits.shape[2:], L.stream_ptr(logits)), "tiles_blend")


def tiles_finalize(score, weight, pad_lo, shape):
    """The kept region [pad_lo, pad_lo + shape): (seg (X, Y, Z) int64 = argmax, probs (K, X, Y, Z) fp32 = score / weight)."""
    L.require_device(score, weight)
    score, weight = score.contiguous(), weight.contiguous()
    K = score.shape[0]
    probs = torch.empty((K,) + tuple(shape), dtype=torch.float32, device=score.device)
    seg = torch.empty(tuple(shape), dtype=torch.int64, device=score.device)
    L.check(L.get_lib().dlka_tiles_finalize(L.ptr(score), L.ptr(weight), K, *weight.shape, *(int(v) for v in pad_lo), *(int(v) for v in shape),
                                            L.ptr(probs), L.ptr(seg), L.stream_ptr(score)), "tiles_finalize")
    return seg, probs


def tiles_launch_count() -> int:
    return int(L.get_lib().dlka_tiles_launch_count())


# ---- the trainers' segmentation losses (include/dlka.h: dlka_seg_loss_*, dlka_seg_eval_counts) ---------------------------------------------
def _seg_desc(logits, labels, mode=L.DLKA_SEG_LOSS_NNUNET, batch_dice=False, do_bg=True, smooth=1.0, weight_ce=1.0, weight_dice=1.0, class_weight=None):
    """Checks of the planar pair (logits (B, K, *), labels (B, 1, *) or (B, *) float32 / int64, read as they are) and the description of the call."""
    L.require_device(logits, labels)
    if logits.ndim < 3:
        raise RuntimeError(f"seg_loss: logits must be (B, K, *spatial), got {tuple(logits.shape)}")
    B, K = int(logits.shape[0]), int(logits.shape[1])
    N = logits[0, 0].numel()
    if K > L.DLKA_SEG_LOSS_K_MAX:
        raise NotImplementedError(f"seg_loss: K = {K} classes (the kernels keep at most {L.DLKA_SEG_LOSS_K_MAX} in registers)")
    spatial = tuple(logits.shape[2:])
    if tuple(labels.shape) not in ((B, 1) + spatial, (B,) + spatial):
        raise RuntimeError(f"seg_loss: labels {tuple(labels.shape)} are not a label map of logits {tuple(logits.shape)}")
    if labels.device != logits.device:
        raise RuntimeError("seg_loss: logits and labels live on different devices")
    if labels.dtype not in (torch.float32, torch.int64):
        labels = labels.float() if labels.is_floating_point() else labels.long()
    d = L.SegLossDesc()
    d.B, d.K, d.N = B, K, N
    d.dtype, d.label_dtype = L.dtype_code(logits), (L.DLKA_LABEL_F32 if labels.dtype == torch.float32 else L.DLKA_LABEL_I64)
    d.mode, d.batch_dice, d.do_bg = int(mode), int(bool(batch_dice)), int(bool(do_bg))
    d.smooth, d.weight_ce, d.weight_dice = float(smooth), float(weight_ce), float(weight_dice)
    for k in range(K):
        d.class_weight[k] = 1.0 if class_weight is None else float(class_weight[k])
    return d, logits.contiguous(), labels.contiguous()


def seg_loss_forward(logits, labels, **kw):
    """Returns (loss (), dc (B, K), stats (B, 4K + 2), coef (3BK + 1,), desc, logits, labels): the last three are what ``seg_loss_backward`` takes."""
    d, logits, labels = _seg_desc(logits, labels, **kw)
    lib = L.get_lib()
    B, K = d.B, d.K
    ws = L.scratch(lib.dlka_seg_loss_workspace_bytes(ctypes.byref(d)), logits)
    out = torch.empty(1 + B * K + B * (4 * K + 2) + 3 * B * K + 1, dtype=torch.float32, device=logits.device)
    loss, dc, stats, coef = out[0:1], out[1:1 + B * K], out[1 + B * K:1 + B * K + B * (4 * K + 2)], out[1 + B * K + B * (4 * K + 2):]
    L.check(lib.dlka_seg_loss_forward(L.ptr(logits), L.ptr(labels), ctypes.byref(d), L.ptr(ws), ws.numel(), L.ptr(loss), L.ptr(dc), L.ptr(stats),
                                      L.ptr(coef), L.stream_ptr(logits)), "seg_loss_forward")
    return loss.reshape(()), dc.view(B, K), stats.view(B, 4 * K + 2), coef, d, logits, labels


def seg_loss_backward(logits, labels, d, coef, grad_output):
    """The logits' gradient, in their dtype; ``grad_output`` is read on the device (one float32 value)."""
    grad_output = grad_output.to(torch.float32).contiguous()
    L.require_device(logits, labels, coef, grad_output)
    gx = torch.empty_like(logits)
    L.check(L.get_lib().dlka_seg_loss_backward(L.ptr(logits), L.ptr(labels), ctypes.byref(d), L.ptr(coef), L.ptr(grad_output), L.ptr(gx),
                                               L.stream_ptr(logits)), "seg_loss_backward")
    return gx


def seg_eval_counts(logits, labels):
    """(tp, fp, fn), each (K - 1,) int64: hard counts of the foreground classes over the batch (argmax: first maximum)."""
    d, logits, labels = _seg_desc(logits, labels)
    lib = L.get_lib()
    ws = L.scratch(lib.dlka_seg_loss_workspace_bytes(ctypes.byref(d)), logits)
    counts = torch.empty((3, d.K - 1), dtype=torch.int64, device=logits.device)
    L.check(lib.dlka_seg_eval_counts(L.ptr(logits), L.ptr(labels), ctypes.byref(d), L.ptr(ws), ws.numel(), L.ptr(counts), L.stream_ptr(logits)),
            "seg_eval_counts")
    return counts[0], counts[1], counts[2]


def seg_loss_launch_count() -> int:
    return int(L.get_lib().dlka_seg_loss_launch_count())


# ---- overlap counts and surface distances of label maps (include/dlka.h: dlka_sd_*) ----------------------------------------------------------
_SD_DTYPES = {torch.uint8: L.DLKA_SD_U8, torch.bool: L.DLKA_SD_U8, torch.int16: L.DLKA_SD_I16, torch.int32: L.DLKA_SD_I32, torch.int64: L.DLKA_SD_I64}


def _rank_padded_ext(d, shape):
    """d.rank and d.ext of a description whose kernels always see three axes: the leading extents of a lower rank are 1."""
    d.rank = len(shape)
    for ax in range(3):
        d.ext[ax] = 1 if ax < 3 - d.rank else int(shape[ax - (3 - d.rank)])


def _sd_desc(prediction, label, class_ids=None, voxelspacing=None, connectivity=1):
    """Checks of the pair of maps and the description of the call; ``class_ids=None``: the maps are masks (value != 0)."""
    L.require_device(prediction, label)
    rank = prediction.ndim
    if rank not in (2, 3):
        raise RuntimeError(f"surface distances: the maps must have rank 2 or 3, got {tuple(prediction.shape)}")
    if tuple(prediction.shape) != tuple(label.shape):
        raise RuntimeError(f"surface distances: the two maps differ in extents, {tuple(prediction.shape)} against {tuple(label.shape)}")
    if prediction.numel() == 0:
        raise RuntimeError(f"surface distances: empty extents {tuple(prediction.shape)}")
    if prediction.device != label.device:
        raise RuntimeError("surface distances: the two maps live on different devices")
    for t in (prediction, label):
        if t.dtype not in _SD_DTYPES:
            raise RuntimeError(f"surface distances: label maps are uint8, int16, int32, int64 or bool, got {t.dtype}")
    if prediction.dtype != label.dtype:
        common = torch.promote_types(prediction.dtype, label.dtype)
        common = common if common in _SD_DTYPES else torch.int64
        prediction, label = prediction.to(common), label.to(common)
    if voxelspacing is None:
        spacing = [1.0] * rank
    else:
        spacing = [float(s) for s in voxelspacing]
        if len(spacing) != rank:
            raise RuntimeError(f"surface distances: voxelspacing has {len(spacing)} entries for rank {rank}")
        if not all(0.0 < s < 1e100 for s in spacing):
            raise RuntimeError(f"surface distances: voxelspacing must be positive, got {spacing}")
    connectivity = int(connectivity)
    if not 1 <= connectivity <= rank:
        raise RuntimeError(f"surface distances: connectivity must be between 1 and the rank ({rank}), got {connectivity}")
    ids = [0] if class_ids is None else [int(c) for c in class_ids]
    if not 1 <= len(ids) <= L.DLKA_SD_K_MAX:
        raise RuntimeError(f"surface distances: between 1 and {L.DLKA_SD_K_MAX} classes per call, got {len(ids)}")
    d = L.SurfaceDistDesc()
    d.connectivity, d.label_dtype, d.K, d.mask_mode = connectivity, _SD_DTYPES[prediction.dtype], len(ids), int(class_ids is None)
    _rank_padded_ext(d, prediction.shape)
    for ax in range(3):
        d.spacing[ax] = 1.0 if ax < 3 - rank else spacing[ax - (3 - rank)]
    for k, c in enumerate(ids):
        d.class_id[k] = c
    return d, prediction.contiguous(), label.contiguous()


def sd_label_stats(prediction, label, class_ids=None, voxelspacing=None, connectivity=1):
    """Returns (stats (K, 9) int64 on the device = |a & b|, |a|, |b|, box lo d h w, box hi d h w per class; desc, prediction, label): the last
    three are what ``sd_distances`` takes."""
    d, prediction, label = _sd_desc(prediction, label, class_ids, voxelspacing, connectivity)
    lib = L.get_lib()
    ws = L.scratch(lib.dlka_sd_stats_workspace_bytes(ctypes.byref(d)), prediction)
    stats = torch.empty((d.K, 9), dtype=torch.int64, device=prediction.device)
    L.check(lib.dlka_sd_label_stats(L.ptr(prediction), L.ptr(label), ctypes.byref(d), L.ptr(ws), ws.numel(), L.ptr(stats), L.stream_ptr(prediction)),
            "sd_label_stats")
    return stats, d, prediction, label


def sd_distances(prediction, label, d, boxes):
    """boxes: K rows (lo d, h, w, extent d, h, w) on the host, an extent of 0 skips the class.  Returns (sqdist float64 on the device, offsets):
    class c with n_c box cells has the squared distances prediction -> label at sqdist[offsets[c] : offsets[c] + n_c] and label -> prediction in
    the n_c cells behind them, -1 off the border."""
    L.require_device(prediction, label)
    flat = [int(v) for row in boxes for v in row]
    if len(flat) != 6 * d.K:
        raise RuntimeError(f"sd_distances: {d.K} boxes of 6 integers expected")
    arr = (ctypes.c_int64 * len(flat))(*flat)
    lib = L.get_lib()
    total = int(lib.dlka_sd_distance_cells(ctypes.byref(d), arr))
    if total < 0:
        raise RuntimeError("sd_distances: a box lies outside the maps")
    offsets, off = [], 0
    for k in range(d.K):
        offsets.append(off)
        n = flat[6 * k + 3] * flat[6 * k + 4] * flat[6 * k + 5]
        off += 2 * n
    sq = torch.empty(total, dtype=torch.float64, device=prediction.device)
    ws = L.scratch(12 * total, prediction)
    if total:
        L.check(lib.dlka_sd_distances(L.ptr(prediction), L.ptr(label), ctypes.byref(d), arr, L.ptr(ws), ws.numel(), L.ptr(sq), total,
                                      L.stream_ptr(prediction)), "sd_distances")
    return sq, offsets


def sd_launch_count() -> int:
    return int(L.get_lib().dlka_sd_launch_count())


# ---- connected components of label maps and the largest-component filter (include/dlka.h: dlka_cc_*) -----------------------------------------
def _cc_desc(image, entries=None, connectivity=1, min_counts=None):
    """Checks of the map and the description of one pass; ``entries``: sequences of class ids, pairwise disjoint; None: the mask (value != 0)."""
    L.require_device(image)
    rank = image.ndim
    if rank not in (1, 2, 3):
        raise RuntimeError(f"connected components: the map must have rank 1, 2 or 3, got {tuple(image.shape)}")
    if image.numel() == 0:
        raise RuntimeError(f"connected components: empty extents {tuple(image.shape)}")
    if image.numel() >= 2 ** 31:
        raise RuntimeError(f"connected components: fewer than 2^31 cells per map, got {image.numel()}")
    if image.dtype not in _SD_DTYPES:
        raise RuntimeError(f"connected components: label maps are uint8, int16, int32, int64 or bool, got {image.dtype}")
    connectivity = int(connectivity)
    if not 1 <= connectivity <= rank:
        raise RuntimeError(f"connected components: connectivity must be between 1 and the rank ({rank}), got {connectivity}")
    d = L.ConnCompDesc()
    d.connectivity, d.label_dtype, d.mask_mode = connectivity, _SD_DTYPES[image.dtype], int(entries is None)
    _rank_padded_ext(d, image.shape)
    if entries is None:
        d.K, d.n_ids = 1, 0
    else:
        pairs = [(int(c), k) for k, ids in enumerate(entries) for c in ids]
        if not 1 <= len(entries) <= L.DLKA_CC_K_MAX or not 1 <= len(pairs) <= L.DLKA_CC_IDS_MAX:
            raise RuntimeError(f"connected components: between 1 and {L.DLKA_CC_K_MAX} entries and at most {L.DLKA_CC_IDS_MAX} class ids per pass, "
                               f"got {len(entries)} and {len(pairs)}")
        if len({c for c, _ in pairs}) != len(pairs):
            raise RuntimeError("connected components: the entries of one pass must not share a class id")
        d.K, d.n_ids = len(entries), len(pairs)
        for j, (c, k) in enumerate(pairs):
            d.class_id[j], d.entry_of[j] = c, k
    if min_counts is not None:
        if len(min_counts) != d.K:
            raise RuntimeError(f"connected components: {d.K} minimum counts expected, got {len(min_counts)}")
        d.has_min = 1
        for k, t in enumerate(min_counts):
            d.min_count[k] = int(t)
    return d, image.contiguous()


def cc_components(image, entries=None, connectivity=1, min_counts=None, want_filtered=True):
    """One pass.  Returns (labels int32 like the map, filtered (dtype of the map) or None, summary int32 (DLKA_CC_SUMMARY,) on the device =
    [components, largest size per entry ..., largest removed size per entry ...], state): ``state`` is what ``cc_component_table`` takes."""
    d, image = _cc_desc(image, entries, connectivity, min_counts)
    lib = L.get_lib()
    ws = L.scratch(lib.dlka_cc_workspace_bytes(ctypes.byref(d)), image)
    labels = torch.empty(image.shape, dtype=torch.int32, device=image.device)
    filtered = torch.empty_like(image) if want_filtered else None
    summary = torch.empty(L.DLKA_CC_SUMMARY, dtype=torch.int32, device=image.device)
    L.check(lib.dlka_cc_components(L.ptr(image), ctypes.byref(d), L.ptr(ws), ws.numel(), L.ptr(labels), L.ptr(filtered), L.ptr(summary),
                                   L.stream_ptr(image)), "cc_components")
    return labels, filtered, summary, (d, ws)


def cc_component_table(state, n):
    """(sizes int64 (n,), owner int32 (n,)) of the components 1..n of the pass that returned ``state``."""
    d, ws = state
    sizes = torch.empty(n, dtype=torch.int64, device=ws.device)
    owner = torch.empty(n, dtype=torch.int32, device=ws.device)
    L.check(L.get_lib().dlka_cc_component_table(ctypes.byref(d), L.ptr(ws), ws.numel(), n, L.ptr(sizes), L.ptr(owner), L.stream_ptr(ws)),
            "cc_component_table")
    return sizes, owner


def cc_launch_count() -> int:
    return int(L.get_lib().dlka_cc_launch_count())


# ---- resampling of probabilities, images and label maps (include/dlka.h: dlka_resample_*) ---------------------------------------------------
_RS_DTYPES = {torch.float32: L.DLKA_F32, torch.float64: L.DLKA_F64}
_I3 = ctypes.c_int64 * 3   # three extents, as the entries below take them


def _rs_desc(x, out, taps, tap_hi, dtype=None):
    L.require_device(x)
    if x.ndim != 4 or x.numel() == 0:
        raise RuntimeError(f"resample: volumes are (c, x, y, z) with no empty axis, got {tuple(x.shape)}")
    out = tuple(int(v) for v in out)
    if len(out) != 3 or min(out) < 1:
        raise RuntimeError(f"resample: three positive target extents, got {out}")
    if x[0].numel() >= 2 ** 31 or out[0] * out[1] * out[2] >= 2 ** 31:
        raise RuntimeError("resample: fewer than 2^31 cells per channel")
    d = L.ResampleDesc()
    d.C, d.dtype = int(x.shape[0]), L.DLKA_F32 if dtype is None else dtype
    for ax in range(3):
        if taps[ax] not in (1, tap_hi):
            raise RuntimeError(f"resample: {taps[ax]} taps on axis {ax}")
        d.taps[ax], d.in_[ax], d.out[ax] = int(taps[ax]), int(x.shape[1 + ax]), out[ax]
    return d, out


def _rs_tables(x, tables, out, width, first_cells):
    """The per-axis tables [(cells int (n_out, k), weights float64 (n_out, k)) ...] as two device arrays of ``width`` entries per row.  The
    kernels trust the cells: they are checked here, on the host."""
    cells, weights = [], []
    for ax, (c, w) in enumerate(tables):
        c, w = np.asarray(c), np.asarray(w, dtype=np.float64)
        k, n = w.shape[1], int(x.shape[1 + ax])
        if w.shape[0] != out[ax] or c.shape[0] != out[ax] or c.min() < 0 or (c.max() + (k - 1 if first_cells else 0)) >= n:
            raise RuntimeError(f"resample: the table of axis {ax} does not fit extents {n} -> {out[ax]}")
        cells.append(np.pad(c.reshape(out[ax], -1), ((0, 0), (0, (1 if first_cells else width) - c.reshape(out[ax], -1).shape[1]))))
        weights.append(np.pad(w, ((0, 0), (0, width - k))))
    ci = torch.from_numpy(np.ascontiguousarray(np.concatenate(cells).astype(np.int32))).to(x.device)
    wi = torch.from_numpy(np.ascontiguousarray(np.concatenate(weights))).to(x.device)
    return ci, wi


def resample_argmax(x, out, tables, region_class=None):
    """uint8 ``out`` map: per cell the first maximum over the channels of ``x`` (c, x, y, z; float32 / float64) resampled by the per-axis
    linear ``tables``, or with ``region_class`` the value of the last channel above 0.5.  The resampled channels are not materialised."""
    taps = [np.asarray(w).shape[1] for _, w in tables]
    d, out = _rs_desc(x, out, taps, 2, _RS_DTYPES.get(x.dtype))
    if x.dtype not in _RS_DTYPES:
        raise RuntimeError(f"resample: float32 or float64 volumes, got {x.dtype}")
    if d.C > 256:
        raise RuntimeError(f"resample: at most 256 channels for a uint8 label map, got {d.C}")
    x = x.contiguous()
    ci, wi = _rs_tables(x, tables, out, 2, False)
    region = None
    if region_class is not None:
        if len(region_class) != d.C:
            raise RuntimeError(f"resample: {d.C} region values expected, got {len(region_class)}")
        region = torch.tensor([int(v) for v in region_class], dtype=torch.int32).to(x.device)
    labels = torch.empty(out, dtype=torch.uint8, device=x.device)
    L.check(L.get_lib().dlka_resample_argmax(L.ptr(x), L.ptr(labels), ctypes.byref(d), L.ptr(ci), L.ptr(wi), L.ptr(region), L.stream_ptr(x)),
            "resample_argmax")
    return labels


def resample_linear(x, out, tables):
    """``x`` (c, x, y, z; float32 / float64) resampled by the per-axis linear tables, every channel stored."""
    taps = [np.asarray(w).shape[1] for _, w in tables]
    d, out = _rs_desc(x, out, taps, 2, _RS_DTYPES.get(x.dtype))
    if x.dtype not in _RS_DTYPES:
        raise RuntimeError(f"resample: float32 or float64 volumes, got {x.dtype}")
    x = x.contiguous()
    ci, wi = _rs_tables(x, tables, out, 2, False)
    y = torch.empty((d.C,) + out, dtype=x.dtype, device=x.device)
    L.check(L.get_lib().dlka_resample_linear(L.ptr(x), L.ptr(y), ctypes.byref(d), L.ptr(ci), L.ptr(wi), L.stream_ptr(x)), "resample_linear")
    return y


def resample_labels(seg, out, tables, strict=False):
    """int32 label maps (c, x, y, z) resampled by the per-axis linear tables: the largest label whose summed weight is >= 0.5 (``strict``:
    > 0.5), else 0."""
    taps = [np.asarray(w).shape[1] for _, w in tables]
    d, out = _rs_desc(seg, out, taps, 2)
    if seg.dtype != torch.int32:
        raise RuntimeError(f"resample: int32 label maps, got {seg.dtype}")
    if d.C * out[0] * out[1] * out[2] >= 2 ** 31:
        raise RuntimeError("resample: fewer than 2^31 cells per label volume")
    seg = seg.contiguous()
    ci, wi = _rs_tables(seg, tables, out, 2, False)
    y = torch.empty((d.C,) + out, dtype=torch.int32, device=seg.device)
    L.check(L.get_lib().dlka_resample_labels(L.ptr(seg), L.ptr(y), ctypes.byref(d), L.ptr(ci), L.ptr(wi), int(bool(strict)), L.stream_ptr(seg)),
            "resample_labels")
    return y


def spline_coefficients(x, pad, boundary, axes, out=None):
    """float64 cubic B-spline coefficients of ONE volume ``x`` (x, y, z; float32 / float64) as scipy.ndimage.spline_filter prepares them:
    ``pad[ax]`` edge samples on both sides (all 0: the cast alone) in one launch, then ``spline_prefilter``.  ``out``: where to write."""
    L.require_device(x, out)
    x, ext = x.contiguous(), [int(n) + 2 * int(p) for n, p in zip(x.shape, pad)]
    out = torch.empty(ext, dtype=torch.float64, device=x.device) if out is None else out
    if x.ndim != 3 or x.dtype not in _RS_DTYPES or list(out.shape) != ext or out.device != x.device:
        raise RuntimeError(f"spline: one float32 / float64 volume (x, y, z) and room for {ext}, got {tuple(x.shape)} {x.dtype}, {tuple(out.shape)}")
    L.check(L.get_lib().dlka_spline_pad(L.ptr(x), L.ptr(out), _RS_DTYPES[x.dtype], _I3(*x.shape), _I3(*pad), L.stream_ptr(x)), "spline_pad")
    return spline_prefilter(out, boundary, axes)


def spline_prefilter(coef, boundary, axes):
    """In place: one launch per axis in ``axes`` with the start values of ``boundary`` (DLKA_SPLINE_REFLECT / DLKA_SPLINE_MIRROR)."""
    L.require_device(coef)
    if coef.ndim != 3 or coef.dtype != torch.float64 or not coef.is_contiguous():
        raise RuntimeError(f"spline: a contiguous float64 volume (x, y, z), got {tuple(coef.shape)} {coef.dtype}")
    for ax in axes:
        L.check(L.get_lib().dlka_spline_prefilter(L.ptr(coef), _I3(*coef.shape), int(ax), int(boundary), L.stream_ptr(coef)), "spline_prefilter")
    return coef


def resample_spline(x, out, tables, pad, lo, hi, clip_axis=-1):
    """One channel ``x`` (x, y, z; float32 / float64) through the cubic B-spline: ``pad[ax]`` edge samples on both sides and the prefilter on
    every axis with pad[ax] > 0, then the evaluation by the per-axis tables (first cell in the padded array, 4 weights; or 1 weight on an
    axis that is not filtered), clipped to [lo[s], hi[s]] (float64 device arrays; s: the index along ``clip_axis``, 0 when it is -1).
    float64 (x', y', z')."""
    L.require_device(x, lo, hi)
    if x.ndim != 3 or x.dtype not in _RS_DTYPES:
        raise RuntimeError(f"resample: one float32 / float64 channel (x, y, z), got {tuple(x.shape)} {x.dtype}")
    pad = [int(p) for p in pad]
    ext = [int(n) + 2 * p for n, p in zip(x.shape, pad)]
    if ext[0] * ext[1] * ext[2] >= 2 ** 31:
        raise RuntimeError("resample: fewer than 2^31 cells per padded channel")
    coef = spline_coefficients(x, pad, L.DLKA_SPLINE_REFLECT, [ax for ax in range(3) if pad[ax] > 0])
    taps = [np.asarray(w).shape[1] for _, w in tables]
    d, out = _rs_desc(coef[None], out, taps, 4)
    n_clip = 1 if clip_axis < 0 else out[clip_axis]
    if lo.dtype != torch.float64 or hi.dtype != torch.float64 or lo.numel() != n_clip or hi.numel() != n_clip:
        raise RuntimeError(f"resample: {n_clip} float64 clip bounds expected")
    ci, wi = _rs_tables(coef[None], tables, out, 4, True)
    y = torch.empty(out, dtype=torch.float64, device=x.device)
    L.check(L.get_lib().dlka_resample_spline_eval(L.ptr(coef), L.ptr(y), ctypes.byref(d), L.ptr(ci), L.ptr(wi), L.ptr(lo.contiguous()),
                                                  L.ptr(hi.contiguous()), int(clip_axis), L.stream_ptr(x)), "resample_spline_eval")
    return y


def resample_launch_count() -> int:
    return int(L.get_lib().dlka_resample_launch_count())


# ---- train-time augmentation (include/dlka.h: dlka_augment_*) -----------------------------------------------------------------------------
_AUG_DTYPES = {torch.float32: L.DLKA_F32, torch.bfloat16: L.DLKA_BF16, torch.float64: L.DLKA_F64, torch.int16: L.DLKA_AUG_I16}


# rank 3: volumes (b, c, x, y, z).  rank 2, the dummy-2D branch: (b, p, y, z), p the planes of a sample (channels x depth slices); the
# description's third extents are 0.  The words the messages of a rank use:
_AUG_WORDS = {3: ("(b, c, x, y, z)", "channel", "three", "volumes"), 2: ("(b, p, y, z)", "plane", "two", "planes")}


def _aug_volume(x, what, rank=3):
    L.require_device(x)
    if x.ndim != 2 + rank or x.numel() == 0:
        raise RuntimeError(f"augment: {what} is {_AUG_WORDS[rank][0]} with no empty axis, got {tuple(x.shape)}")
    if x[0, 0].numel() >= 2 ** 31:
        raise RuntimeError(f"augment: fewer than 2^31 cells per {_AUG_WORDS[rank][1]}")
    return x.contiguous()


def _aug_data(x, rank=3):
    x = _aug_volume(x, "data", rank)
    if x.dtype not in _AUG_DTYPES:
        raise RuntimeError(f"augment: float32, bfloat16, float64 or int16 {_AUG_WORDS[rank][3]}, got {x.dtype}")
    return x


def _aug_desc(x, out, order, mode, cval, pad=0, dtype=L.DLKA_F32):
    rank = x.ndim - 2
    out = tuple(int(v) for v in out)
    if len(out) != rank or min(out) < 1 or math.prod(out) >= 2 ** 31:
        raise RuntimeError(f"augment: {_AUG_WORDS[rank][2]} positive patch extents below 2^31 cells, got {out}")
    d = L.AugmentDesc()
    d.B, d.C, d.dtype, d.order, d.mode, d.pad, d.cval = int(x.shape[0]), int(x.shape[1]), dtype, int(order), int(mode), int(pad), float(cval)
    for ax in range(3):
        d.src[ax], d.out[ax] = (int(x.shape[2 + ax]), out[ax]) if ax < rank else (0, 0)
    return d, out


def _aug_sample_tables(x, out, maps, plain):
    """maps (B, rank, rank + 1) float64 and plain (B, 1 + rank) int (flag, lower bound per axis) on the device.  The kernels trust the boxes:
    checked here."""
    rank = x.ndim - 2
    maps = np.ascontiguousarray(np.asarray(maps, dtype=np.float64).reshape(-1, rank * (rank + 1)))
    plain = np.ascontiguousarray(np.asarray(plain, dtype=np.int32).reshape(-1, 1 + rank))
    if maps.shape[0] != x.shape[0] or plain.shape[0] != x.shape[0]:
        raise RuntimeError(f"augment: one map and one crop record per sample ({x.shape[0]})")
    for b in range(plain.shape[0]):
        if plain[b, 0] and any(plain[b, 1 + ax] < 0 or plain[b, 1 + ax] + out[ax] > x.shape[2 + ax] for ax in range(rank)):
            raise RuntimeError(f"augment: the crop of sample {b} at {plain[b, 1:].tolist()} leaves the source {tuple(x.shape[2:])}")
    return torch.from_numpy(maps).to(x.device), torch.from_numpy(plain).to(x.device)


def _aug_spline_source(x, mode):
    """What the prefilter reads (float32 / float64), and scipy's padding and start values for ``mode``."""
    src = x if x.dtype in _RS_DTYPES else x.to(torch.float64 if x.dtype == torch.int16 else torch.float32)
    return (src, L.DLKA_RESAMPLE_SPLINE_PAD, L.DLKA_SPLINE_REFLECT) if mode == L.DLKA_AUG_NEAREST else (src, 0, L.DLKA_SPLINE_MIRROR)


def _aug_spatial(x, out, maps, plain, order, mode, cval, rank):
    x = _aug_data(x, rank)
    coefficients, entry = ((augment_spline_coefficients, "augment_spatial") if rank == 3
                           else (augment_spline_coefficients2d, "augment_spatial2d"))
    coef, pad = (coefficients(x, mode) if order == 3 and not all(int(p[0]) for p in np.asarray(plain).reshape(-1, 1 + rank)) else (None, 0))
    if order == 3 and coef is None:
        order = 0                                            # every sample is a plain crop: nothing is interpolated
    d, out = _aug_desc(x, out, order, mode, cval, pad, _AUG_DTYPES[x.dtype])
    m, p = _aug_sample_tables(x, out, maps, plain)
    y = torch.empty(tuple(x.shape[:2]) + out, dtype=x.dtype, device=x.device)
    L.check(getattr(L.get_lib(), "dlka_" + entry)(L.ptr(x), L.ptr(coef), L.ptr(y), ctypes.byref(d), L.ptr(m), L.ptr(p), L.stream_ptr(x)), entry)
    return y


def _aug_spatial_labels(seg, out, maps, plain, order, mode, cval, rank):
    seg = _aug_volume(seg, "seg", rank)
    if seg.dtype != torch.int32:
        raise RuntimeError(f"augment: int32 label maps, got {seg.dtype}")
    d, out = _aug_desc(seg, out, order, mode, cval)
    m, p = _aug_sample_tables(seg, out, maps, plain)
    y = torch.empty(tuple(seg.shape[:2]) + out, dtype=torch.int32, device=seg.device)
    entry = "augment_spatial_labels" if rank == 3 else "augment_spatial2d_labels"
    L.check(getattr(L.get_lib(), "dlka_" + entry)(L.ptr(seg), L.ptr(y), ctypes.byref(d), L.ptr(m), L.ptr(p), L.stream_ptr(seg)), entry)
    return y


def augment_spline_coefficients(x, mode):
    """float64 cubic B-spline coefficients of every channel of ``x`` (b, c, x, y, z), as scipy.ndimage.map_coordinates prepares them: mode
    'nearest' pads DLKA_RESAMPLE_SPLINE_PAD edge samples and filters with the 'reflect' start values, 'constant' filters the array itself
    with the 'mirror' ones.  Returns (coefficients (b, c, x + 2 pad, ...), pad)."""
    x = _aug_volume(x, "data")
    src, pad, boundary = _aug_spline_source(x, mode)
    ext = [int(n) + 2 * pad for n in x.shape[2:]]
    if ext[0] * ext[1] * ext[2] >= 2 ** 31:
        raise RuntimeError("augment: fewer than 2^31 cells per padded channel")
    coef = torch.empty([x.shape[0], x.shape[1]] + ext, dtype=torch.float64, device=x.device)
    for b in range(x.shape[0]):
        for c in range(x.shape[1]):
            spline_coefficients(src[b, c], (pad, pad, pad), boundary, range(3), out=coef[b, c])
    return coef, pad


def augment_spatial(x, out, maps, plain, order, mode, cval):
    """``x`` (b, c, x, y, z; float32, bfloat16, float64, int16) sampled at the per-sample affine ``maps`` with scipy's map_coordinates rules
    (orders 0, 1, 3; mode DLKA_AUG_CONSTANT / DLKA_AUG_NEAREST); samples whose ``plain`` flag is set are copied boxes."""
    return _aug_spatial(x, out, maps, plain, order, mode, cval, 3)


def augment_spatial_labels(seg, out, maps, plain, order, mode, cval):
    """int32 label maps (b, c, x, y, z) at the same coordinates: order 0 the nearest cell, order 1 the largest label whose trilinear weight is
    >= 0.5, else 0."""
    return _aug_spatial_labels(seg, out, maps, plain, order, mode, cval, 3)


def augment_spline_coefficients2d(x, mode):
    """float64 cubic B-spline coefficients of every plane of ``x`` (b, p, y, z), as scipy.ndimage.map_coordinates prepares them for a 2-D
    array: the in-plane axes alone are padded (mode 'nearest': DLKA_RESAMPLE_SPLINE_PAD edge samples, 'reflect' start values; 'constant': no
    padding, 'mirror') and filtered.  The batch's stack of planes is ONE volume (b p, y, z) filtered along its axes 1 and 2: three launches
    whatever b and p are; a stack of 2^31 padded cells or more goes sample by sample.  Returns (coefficients (b, p, y + 2 pad, z + 2 pad), pad)."""
    x = _aug_volume(x, "data", 2)
    src, pad, boundary = _aug_spline_source(x, mode)
    B, P = int(x.shape[0]), int(x.shape[1])
    ext = [int(n) + 2 * pad for n in x.shape[2:]]
    if P * ext[0] * ext[1] >= 2 ** 31:
        raise RuntimeError("augment: fewer than 2^31 cells per padded sample")
    coef = torch.empty([B, P] + ext, dtype=torch.float64, device=x.device)
    if B * P * ext[0] * ext[1] < 2 ** 31:
        spline_coefficients(src.reshape(B * P, *x.shape[2:]), (0, pad, pad), boundary, (1, 2), out=coef.reshape(B * P, *ext))
    else:
        for b in range(B):
            spline_coefficients(src[b], (0, pad, pad), boundary, (1, 2), out=coef[b])
    return coef, pad


def augment_spatial2d(x, out, maps, plain, order, mode, cval):
    """``x`` (b, p, y, z; float32, bfloat16, float64, int16): every plane of sample b sampled at the in-plane affine ``maps[b]`` (2, 3) with
    scipy's 2-D map_coordinates rules (orders 0, 1, 3: 1 / 4 / 16 taps; mode DLKA_AUG_CONSTANT / DLKA_AUG_NEAREST); samples whose ``plain``
    flag is set are copied in-plane boxes.  batchgenerators' augment_spatial with dim == 2 on the planes the dummy-2D branch makes."""
    return _aug_spatial(x, out, maps, plain, order, mode, cval, 2)


def augment_spatial2d_labels(seg, out, maps, plain, order, mode, cval):
    """int32 label planes (b, p, y, z) at the same coordinates: order 0 the nearest cell, order 1 the largest label whose bilinear weight over
    the 4 in-plane neighbours is >= 0.5, else 0."""
    return _aug_spatial_labels(seg, out, maps, plain, order, mode, cval, 2)


def augment_gaussian(x, radius, weights):
    """scipy.ndimage.gaussian_filter of every channel of ``x`` (b, c, x, y, z), one launch per axis: ``radius`` (b * c,) int, < 0 = the channel
    is copied; ``weights`` (b * c, DLKA_AUG_RADIUS_MAX + 1) float64, centre first."""
    x = _aug_data(x)
    n = x.shape[0] * x.shape[1]
    radius = np.ascontiguousarray(np.asarray(radius, dtype=np.int32).reshape(-1))
    weights = np.ascontiguousarray(np.asarray(weights, dtype=np.float64))
    if radius.shape != (n,) or weights.shape != (n, L.DLKA_AUG_RADIUS_MAX + 1) or radius.max() > L.DLKA_AUG_RADIUS_MAX:
        raise RuntimeError(f"augment: {n} radii of at most {L.DLKA_AUG_RADIUS_MAX} and their weight rows expected")
    r, w = torch.from_numpy(radius).to(x.device), torch.from_numpy(weights).to(x.device)
    for ax in range(3):
        y = torch.empty_like(x)
        L.check(L.get_lib().dlka_augment_gaussian(L.ptr(x), L.ptr(y), _AUG_DTYPES[x.dtype], n, _I3(*x.shape[2:]), ax, L.ptr(r), L.ptr(w),
                                                  L.stream_ptr(x)), "augment_gaussian")
        x = y
    return x


def augment_channel_stats(x):
    """(b * c, 4) float64 on the device: sum, sum of squares about the mean, min, max of every channel of ``x`` (b, c, x, y, z)."""
    x = _aug_data(x)
    n, cells = x.shape[0] * x.shape[1], x[0, 0].numel()
    if n > 65535:
        raise RuntimeError("augment: at most 65535 channels in a batch")
    lib = L.get_lib()
    nbytes = lib.dlka_augment_stats_workspace_bytes(n, cells)
    ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=x.device)
    stats = torch.empty((n, 4), dtype=torch.float64, device=x.device)
    L.check(lib.dlka_augment_channel_stats(L.ptr(x), L.ptr(stats), L.ptr(ws), nbytes, _AUG_DTYPES[x.dtype], n, cells, L.stream_ptr(x)),
            "augment_channel_stats")
    return stats


def augment_pointwise(x, steps, noise=None, stats0=None, stats1=None, flip=None):
    """One streaming pass over ``x`` (b, c, x, y, z): ``steps`` (b * c, k <= DLKA_AUG_OPS_MAX, 6) float64 rows (code, p0 .. p4) applied in turn
    per channel; ``flip`` (b,) int, bit a reverses spatial axis a of the stored result."""
    x = _aug_data(x)
    n = x.shape[0] * x.shape[1]
    steps = np.asarray(steps, dtype=np.float64)
    if steps.ndim != 3 or steps.shape[0] != n or steps.shape[1] > L.DLKA_AUG_OPS_MAX or steps.shape[2] != 6:
        raise RuntimeError(f"augment: steps are ({n}, <= {L.DLKA_AUG_OPS_MAX}, 6), got {steps.shape}")
    table = np.zeros((n, L.DLKA_AUG_OPS_MAX, 6))
    table[:, :steps.shape[1]] = steps
    codes = set(table[:, :, 0].reshape(-1).tolist())
    if not codes <= set(float(c) for c in range(7)):
        raise RuntimeError(f"augment: unknown step codes {sorted(codes)}")
    if float(L.DLKA_AUG_OP_NOISE) in codes:
        if noise is None or noise.shape != x.shape or noise.dtype != x.dtype or noise.device != x.device:
            raise RuntimeError("augment: the noise step takes a field of the data's shape, dtype and device")
        noise = noise.contiguous()
    need0 = codes & {float(L.DLKA_AUG_OP_CONTRAST), float(L.DLKA_AUG_OP_GAMMA), float(L.DLKA_AUG_OP_RETAIN)}
    for s, need in ((stats0, bool(need0)), (stats1, float(L.DLKA_AUG_OP_RETAIN) in codes)):
        if need and (s is None or tuple(s.shape) != (n, 4) or s.dtype != torch.float64 or s.device != x.device or not s.is_contiguous()):
            raise RuntimeError(f"augment: ({n}, 4) float64 channel statistics on the data's device expected")
    f = None
    if flip is not None:
        flip = np.ascontiguousarray(np.asarray(flip, dtype=np.int32).reshape(-1))
        if flip.shape != (x.shape[0],) or flip.min() < 0 or flip.max() > 7:
            raise RuntimeError(f"augment: one flip mask 0..7 per sample ({x.shape[0]})")
        f = torch.from_numpy(flip).to(x.device)
    t = torch.from_numpy(table).to(x.device)
    y = torch.empty_like(x)
    L.check(L.get_lib().dlka_augment_pointwise(L.ptr(x), L.ptr(noise), L.ptr(y), _AUG_DTYPES[x.dtype], x.shape[0], x.shape[1], _I3(*x.shape[2:]),
                                               L.ptr(t), L.ptr(stats0), L.ptr(stats1), L.ptr(f), L.stream_ptr(x)), "augment_pointwise")
    return y


def augment_launch_count() -> int:
    return int(L.get_lib().dlka_augment_launch_count())


# ---- case preprocessing: nonzero mask, crop, normalisation (include/dlka.h: dlka_prep_*) --------------------------------------------------------
PREP_SCHEMES = {"CT": L.DLKA_PREP_CT, "CT2": L.DLKA_PREP_CT2}     # every other name is the reference's "nonCT" branch


def _prep_desc(data, what="data"):
    """Checks of a (c, *spatial) float32 volume and its description."""
    L.require_device(data)
    if data.ndim not in (3, 4):
        raise NotImplementedError(f"preprocessing: {what} of shape (C, X, Y, Z) or (C, X, Y), got {tuple(data.shape)}")
    if data.dtype != torch.float32:
        raise RuntimeError(f"preprocessing: the kernels take float32 {what}, got {data.dtype}")
    if data.numel() == 0:
        raise RuntimeError(f"preprocessing: empty extents {tuple(data.shape)}")
    if data[0].numel() >= 2 ** 31:
        raise RuntimeError(f"preprocessing: fewer than 2^31 cells per channel, got {data[0].numel()}")
    if data.shape[0] > L.DLKA_PREP_C_MAX:
        raise RuntimeError(f"preprocessing: at most {L.DLKA_PREP_C_MAX} channels, got {data.shape[0]}")
    d = L.PrepDesc()
    d.C = data.shape[0]
    _rank_padded_ext(d, data.shape[1:])
    return d, data.contiguous()


def _prep_seg(seg, like, what="seg"):
    L.require_device(seg)
    if seg.dtype != torch.int32 or seg.device != like.device or tuple(seg.shape[1:]) != tuple(like.shape[1:]) or seg.ndim != like.ndim:
        raise RuntimeError(f"preprocessing: {what} is int32 (c, *spatial) with the data's extents and device, got {seg.dtype} {tuple(seg.shape)}")
    return seg.contiguous()


def prep_nonzero_mask(data):
    """cropping.py:23-42 on the device: (mask uint8 like one channel, box int32 (8,) on the device = per-axis minima, per-axis maxima (left-padded
    to three axes), the number of set cells, unused)."""
    d, data = _prep_desc(data)
    lib = L.get_lib()
    bg = torch.empty(data.shape[1:], dtype=torch.uint8, device=data.device)
    L.check(lib.dlka_prep_background(L.ptr(data), ctypes.byref(d), L.ptr(bg), L.stream_ptr(data)), "prep_background")
    labels, _, _, _ = cc_components(bg, None, 1, want_filtered=False)
    ws = L.scratch(lib.dlka_prep_fill_workspace_bytes(ctypes.byref(d)), data)
    mask = torch.empty_like(bg)
    box = torch.empty(8, dtype=torch.int32, device=data.device)
    L.check(lib.dlka_prep_fill_bbox(L.ptr(bg), L.ptr(labels), ctypes.byref(d), L.ptr(ws), ws.numel(), L.ptr(mask), L.ptr(box),
                                    L.stream_ptr(data)), "prep_fill_bbox")
    return mask, box


def prep_mask_bbox(mask):
    """The box (as ``prep_nonzero_mask`` returns it) of a uint8 map's nonzero cells."""
    L.require_device(mask)
    if mask.dtype != torch.uint8 or mask.ndim not in (2, 3) or mask.numel() == 0 or mask.numel() >= 2 ** 31:
        raise RuntimeError(f"preprocessing: a uint8 mask of rank 2 or 3 with fewer than 2^31 cells, got {mask.dtype} {tuple(mask.shape)}")
    mask = mask.contiguous()
    d = L.PrepDesc()
    d.C = 1
    _rank_padded_ext(d, mask.shape)
    box = torch.empty(8, dtype=torch.int32, device=mask.device)
    L.check(L.get_lib().dlka_prep_mask_bbox(L.ptr(mask), ctypes.byref(d), L.ptr(box), L.stream_ptr(mask)), "prep_mask_bbox")
    return box


def prep_crop(data, seg, mask, bbox, nonzero_label=-1, nan_to_zero=False, want_seg=True):
    """cropping.py:95-115: (data inside ``bbox`` = [[lo, hi], ...] per spatial axis, int32 label map or None).  ``seg`` int32 (c, *spatial) or
    None; ``mask`` the uint8 nonzero mask (needed for the label map only)."""
    d, data = _prep_desc(data)
    if len(bbox) != d.rank:
        raise RuntimeError(f"preprocessing: one [lo, hi] per spatial axis ({d.rank}), got {bbox}")
    pad = 3 - d.rank
    for ax in range(3):
        d.lo[ax], d.hi[ax] = (0, 1) if ax < pad else (int(bbox[ax - pad][0]), int(bbox[ax - pad][1]))
        if not 0 <= d.lo[ax] < d.hi[ax] <= d.ext[ax]:
            raise RuntimeError(f"preprocessing: the box {bbox} does not lie inside {tuple(data.shape[1:])}")
    d.nan_to_zero, d.nonzero_label = int(bool(nan_to_zero)), int(nonzero_label)
    cshape = tuple(int(b[1]) - int(b[0]) for b in bbox)
    out = torch.empty((data.shape[0],) + cshape, dtype=torch.float32, device=data.device)
    seg_out = None
    if want_seg:
        if mask is None or mask.dtype != torch.uint8 or tuple(mask.shape) != tuple(data.shape[1:]) or mask.device != data.device:
            raise RuntimeError("preprocessing: the label map needs the uint8 nonzero mask of the data's extents")
        mask = mask.contiguous()
        if seg is not None:
            seg = _prep_seg(seg, data)
            if not 1 <= seg.shape[0] <= L.DLKA_PREP_C_MAX:
                raise RuntimeError(f"preprocessing: between 1 and {L.DLKA_PREP_C_MAX} seg channels, got {seg.shape[0]}")
            d.seg_channels = seg.shape[0]
        seg_out = torch.empty((max(d.seg_channels, 1),) + cshape, dtype=torch.int32, device=data.device)
    L.check(L.get_lib().dlka_prep_crop(L.ptr(data), L.ptr(seg), L.ptr(mask), ctypes.byref(d), L.ptr(out), L.ptr(seg_out), L.stream_ptr(data)),
            "prep_crop")
    return out, seg_out


def prep_normalize(data, seg_last, records):
    """preprocessing.py:274-305.  ``records``: per channel (scheme name, lower, upper, mean, sd, use_mask); ``seg_last`` int32 (*spatial), the
    reference's seg[-1].  Returns (normalised data, table float64 (c, DLKA_PREP_REC) on the device: scheme, lower, upper, mean, sd, use_mask,
    count, unused), the mean, sd and count of the CT2 and nonCT channels being those the kernels computed and used."""
    d, data = _prep_desc(data)
    seg_last = _prep_seg(seg_last[None], data, "seg[-1]")
    if len(records) != data.shape[0]:
        raise RuntimeError(f"preprocessing: one record per channel ({data.shape[0]}), got {len(records)}")
    host = np.zeros((data.shape[0], L.DLKA_PREP_REC), dtype=np.float64)
    for c, (scheme, lower, upper, mean, sd, use_mask) in enumerate(records):
        host[c, :6] = (PREP_SCHEMES.get(scheme, L.DLKA_PREP_NONCT), lower, upper, mean, sd, float(bool(use_mask)))
    table = torch.from_numpy(host).to(data.device)
    lib = L.get_lib()
    if (host[:, 0] != L.DLKA_PREP_CT).any():
        nbytes = lib.dlka_prep_stats_workspace_bytes(ctypes.byref(d))
        ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=data.device)
        L.check(lib.dlka_prep_channel_stats(L.ptr(data), L.ptr(seg_last), ctypes.byref(d), L.ptr(table), L.ptr(ws), nbytes, L.stream_ptr(data)),
                "prep_channel_stats")
    out = torch.empty_like(data)
    L.check(lib.dlka_prep_normalize(L.ptr(data), L.ptr(seg_last), ctypes.byref(d), L.ptr(table), L.ptr(out), L.stream_ptr(data)), "prep_normalize")
    return out, table


def prep_launch_count() -> int:
    return int(L.get_lib().dlka_prep_launch_count())


# ---- the 2-D evaluator's slice resampling (include/dlka.h: dlka_zoom2d_*) -----------------------------------------------------------------------
_ZM_DTYPES = {torch.float32: L.DLKA_F32, torch.bfloat16: L.DLKA_BF16, torch.float64: L.DLKA_F64, torch.int16: L.DLKA_ZOOM2D_I16}


def _zm_stack(x, what="slices"):
    L.require_device(x)
    if x.ndim != 3 or x.numel() == 0:
        raise RuntimeError(f"zoom2d: {what} are (n, h, w) with no empty axis, got {tuple(x.shape)}")
    if x.numel() >= 2 ** 31:
        raise RuntimeError("zoom2d: fewer than 2^31 cells per stack")
    return x.contiguous()


def _zm_desc(n, in_hw, out_hw):
    out_hw = tuple(int(v) for v in out_hw)
    if len(out_hw) != 2 or min(out_hw) < 1 or int(n) * out_hw[0] * out_hw[1] >= 2 ** 31:
        raise RuntimeError(f"zoom2d: two positive output extents and fewer than 2^31 output cells, got {out_hw} for {int(n)} slices")
    d = L.Zoom2dDesc()
    d.N = int(n)
    for ax in range(2):
        d.in_[ax], d.out[ax] = int(in_hw[ax]), out_hw[ax]
    return d, out_hw


def zoom2d_spline_tables(starts, weights, in_hw, taps, device):
    """Per-axis (rows, then columns) first taps and weights of the spline kernel as two device arrays.  ``starts[ax]``: int, -1 .. n - 1 (the
    kernel mirrors the taps beyond the slice) or DLKA_ZOOM2D_OUTSIDE; ``weights[ax]``: float64 (m, taps)."""
    s_all, w_all = [], []
    for ax in range(2):
        s, w = np.asarray(starts[ax], dtype=np.int64), np.asarray(weights[ax], dtype=np.float64)
        inside = s != L.DLKA_ZOOM2D_OUTSIDE
        if w.shape != (s.shape[0], taps) or (inside & ((s < (-1 if taps == 4 else 0)) | (s > int(in_hw[ax]) - 1))).any():
            raise RuntimeError(f"zoom2d: the table of axis {ax} does not fit an extent of {int(in_hw[ax])} with {taps} taps")
        s_all.append(s)
        w_all.append(np.pad(w, ((0, 0), (0, 4 - taps))))
    return (torch.from_numpy(np.concatenate(s_all).astype(np.int32)).to(device),
            torch.from_numpy(np.ascontiguousarray(np.concatenate(w_all))).to(device))


def zoom2d_index_tables(cells, in_hw, device):
    """Per-axis (rows, then columns) source indices of the order-0 kernels as one int32 device array; -1: outside the slice."""
    out = []
    for ax in range(2):
        c = np.asarray(cells[ax], dtype=np.int64)
        if c.ndim != 1 or c.min() < -1 or c.max() > int(in_hw[ax]) - 1:
            raise RuntimeError(f"zoom2d: the index table of axis {ax} does not fit an extent of {int(in_hw[ax])}")
        out.append(c)
    return torch.from_numpy(np.concatenate(out).astype(np.int32)).to(device)


def _zm_table(t, n, dtype, like, what):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.numel() != n or t.device != like.device or not t.is_contiguous():
        raise RuntimeError(f"zoom2d: {what} is a contiguous {dtype} device array of {n} entries (zoom2d_*_tables)")
    return t


def zoom2d_coefficients(x):
    """float64 cubic B-spline coefficients of every slice of ``x`` (n, h, w) as scipy.ndimage.zoom prepares them under mode 'constant': the
    'mirror' prefilter of the slice itself, no padding.  The stack is filtered as ONE volume along axes 1 and 2: three launches whatever n."""
    x = _zm_stack(x)
    if x.dtype in _RS_DTYPES:
        return spline_coefficients(x, (0, 0, 0), L.DLKA_SPLINE_MIRROR, (1, 2))
    if x.dtype in (torch.bfloat16, torch.int16):             # torch's cast: the pad kernel reads float32 / float64 only
        return spline_prefilter(x.to(torch.float64), L.DLKA_SPLINE_MIRROR, (1, 2))
    raise RuntimeError(f"zoom2d: float32, float64, bfloat16 or int16 slices, got {x.dtype}")


def zoom2d_spline(src, out_hw, start, w4, taps, out_dtype, mean=None, std=None):
    """The spline kernel: ``src`` (n, h, w) float64 coefficients (taps 4) or raw float32 / bfloat16 / int16 values (taps 2) evaluated through
    the device tables of ``zoom2d_spline_tables``; float32, bfloat16 or int16 result, float32 (v - mean) / std in between when given."""
    src = _zm_stack(src, "coefficients" if taps == 4 else "slices")
    if src.dtype not in _ZM_DTYPES or out_dtype not in _ZM_DTYPES or out_dtype == torch.float64:
        raise RuntimeError(f"zoom2d: {src.dtype} -> {out_dtype} is not a pair the spline kernel has")
    d, out_hw = _zm_desc(src.shape[0], src.shape[1:], out_hw)
    d.in_dtype, d.out_dtype, d.taps = _ZM_DTYPES[src.dtype], _ZM_DTYPES[out_dtype], int(taps)
    if (mean is None) != (std is None):
        raise RuntimeError("zoom2d: mean and std come together")
    if mean is not None:
        d.normalize, d.mean, d.std = 1, float(mean), float(std)
    rows = out_hw[0] + out_hw[1]
    start, w4 = _zm_table(start, rows, torch.int32, src, "start"), _zm_table(w4, 4 * rows, torch.float64, src, "w4")
    y = torch.empty((src.shape[0],) + out_hw, dtype=out_dtype, device=src.device)
    L.check(L.get_lib().dlka_zoom2d_spline(L.ptr(src), L.ptr(y), ctypes.byref(d), L.ptr(start), L.ptr(w4), L.stream_ptr(src)), "zoom2d_spline")
    return y


def zoom2d_nearest(x, out_hw, idx):
    """Order 0: ``x`` (n, h, w) of any 1, 2, 4 or 8 byte dtype gathered through the device table of ``zoom2d_index_tables``; outside: 0."""
    x = _zm_stack(x)
    if x.dtype == torch.bool or x.element_size() not in (1, 2, 4, 8) or x.is_complex():
        raise RuntimeError(f"zoom2d: a real dtype of 1, 2, 4 or 8 bytes, got {x.dtype}")
    d, out_hw = _zm_desc(x.shape[0], x.shape[1:], out_hw)
    idx = _zm_table(idx, out_hw[0] + out_hw[1], torch.int32, x, "idx")
    y = torch.empty((x.shape[0],) + out_hw, dtype=x.dtype, device=x.device)
    L.check(L.get_lib().dlka_zoom2d_nearest(L.ptr(x), L.ptr(y), ctypes.byref(d), x.element_size(), L.ptr(idx), L.stream_ptr(x)), "zoom2d_nearest")
    return y


def zoom2d_argmax(logits, out_hw, idx, out=None):
    """uint8 (n, x, y): the first maximum over the K planes of ``logits`` (n, K, h, w; float32 / bfloat16, finite) at the source pixel the
    device table of ``zoom2d_index_tables`` names for each output pixel, 0 outside.  ``out``: a contiguous uint8 (n, x, y) to write into."""
    L.require_device(logits)
    if logits.ndim != 4 or logits.numel() == 0 or logits.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"zoom2d: logits are float32 / bfloat16 (n, K, h, w) with no empty axis, got {logits.dtype} {tuple(logits.shape)}")
    if logits.shape[1] > L.DLKA_ZOOM2D_K_MAX:
        raise RuntimeError(f"zoom2d: at most {L.DLKA_ZOOM2D_K_MAX} classes for a uint8 label map, got {logits.shape[1]}")
    if logits.numel() >= 2 ** 31 * 64:
        raise RuntimeError("zoom2d: fewer than 2^37 logits per chunk")
    logits = logits.contiguous()
    d, out_hw = _zm_desc(logits.shape[0], logits.shape[2:], out_hw)
    if logits[:, 0].numel() >= 2 ** 31:
        raise RuntimeError("zoom2d: fewer than 2^31 cells per stack")
    d.in_dtype = _ZM_DTYPES[logits.dtype]
    idx = _zm_table(idx, out_hw[0] + out_hw[1], torch.int32, logits, "idx")
    shape = (logits.shape[0],) + out_hw
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=logits.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != shape or out.device != logits.device or not out.is_contiguous():
        raise RuntimeError(f"zoom2d: out is a contiguous uint8 {shape} on the logits' device")
    L.check(L.get_lib().dlka_zoom2d_argmax(L.ptr(logits), L.ptr(out), ctypes.byref(d), int(logits.shape[1]), L.ptr(idx), L.stream_ptr(logits)),
            "zoom2d_argmax")
    return out


def zoom2d_launch_count() -> int:
    return int(L.get_lib().dlka_zoom2d_launch_count())
