"""The deformable convolutions on their own: 3-D (the reference's D3D op), 2-D (torchvision semantics) and the 2-D block's channels-last depthwise one."""
from __future__ import annotations

from ctypes import byref
from typing import Sequence

import torch

from .. import _lib as L
from ._call import WS, _geom, _geom2d, _out_dims, _pair, _require_input_dtype, _triple, call, call_ws, grads_like


# ---- 3-D deformable conv -----------------------------------------------------------------------------------------------------------------
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
    g = _geom(input.shape, weight.shape[0], k, s, p, d, group, deformable_groups, im2col_step)
    dt = L.dtype_code(input, allow_f64=True)
    Do, Ho, Wo = _out_dims(g)
    if min(Do, Ho, Wo) <= 0:
        L.check(-4, "deform_conv_forward")
    K = k[0] * k[1] * k[2]
    if tuple(offset.shape) != (g.B, deformable_groups * 3 * K, Do, Ho, Wo):
        raise RuntimeError(f"offset shape {tuple(offset.shape)} does not match {(g.B, deformable_groups * 3 * K, Do, Ho, Wo)}")
    out = torch.empty((g.B, g.Cout, Do, Ho, Wo), dtype=input.dtype, device=input.device)
    call_ws("deform_conv3d_forward", ("deform_conv3d_forward_workspace", byref(g), dt), input, L.ptr(input), L.ptr(offset), L.ptr(weight), L.ptr(bias),
            L.ptr(out), WS, byref(g), dt, L.stream_ptr(input), label="deform_conv_forward")
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
    g = _geom(input.shape, weight.shape[0], k, s, p, d, group, deformable_groups, im2col_step)
    dt = L.dtype_code(input, allow_f64=True)
    Do, Ho, Wo = _out_dims(g)
    if tuple(grad_output.shape) != (g.B, g.Cout, Do, Ho, Wo):  # deform_conv_cuda.cu:193-200
        raise RuntimeError(f"Input shape and grad_out shape wont match: ({(g.B, g.Cout, Do, Ho, Wo)} vs {tuple(grad_output.shape)}).")
    gi, go, gw = grads_like((input, offset, weight), need)
    gb = torch.empty_like(bias, memory_format=torch.contiguous_format) if need[3] else None
    call_ws("deform_conv3d_backward", ("deform_conv3d_backward_workspace", byref(g), dt), input, L.ptr(input), L.ptr(offset), L.ptr(weight),
            L.ptr(grad_output), L.ptr(gi), L.ptr(go), L.ptr(gw), L.ptr(gb), WS, byref(g), dt, L.stream_ptr(input), label="deform_conv_backward")
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
    call("deform_conv3d_sample_index_path", L.ptr(offset), L.ptr(idx), L.ptr(mask), byref(g), L.dtype_code(offset), int(path), L.stream_ptr(offset),
         label="deform_conv3d_sample_index")
    return idx, mask


# ---- 2-D deformable conv (torchvision semantics) -----------------------------------------------------------------------------------------
def deform_conv2d_forward(input, offset, weight, bias=None, stride=1, padding=0, dilation=1):
    L.require_device(input, offset, weight, bias)
    _require_input_dtype(input, offset=offset, weight=weight, bias=bias)
    s, p, d = _pair(stride), _pair(padding), _pair(dilation)
    input, offset, weight = input.contiguous(), offset.contiguous(), weight.contiguous()
    bias = None if bias is None else bias.contiguous()
    g = _geom2d(input.shape, weight.shape, s, p, d, offset.shape[1])
    dt = L.dtype_code(input, allow_f64=True)
    _, Ho, Wo = _out_dims(g)
    if tuple(offset.shape[2:]) != (Ho, Wo):
        raise RuntimeError(f"offset spatial size {tuple(offset.shape[2:])} does not match output {(Ho, Wo)}")
    out = torch.empty((g.B, g.Cout, Ho, Wo), dtype=input.dtype, device=input.device)
    call_ws("deform_conv2d_forward", ("deform_conv2d_forward_workspace", byref(g), dt), input, L.ptr(input), L.ptr(offset), L.ptr(weight), L.ptr(bias),
            L.ptr(out), WS, byref(g), dt, L.stream_ptr(input), label="deform_conv2d")
    return out


def deform_conv2d_backward(input, offset, weight, grad_output, stride=1, padding=0, dilation=1, with_bias=False,
                           need=(True, True, True)):
    L.require_device(input, offset, weight, grad_output)
    _require_input_dtype(input, offset=offset, weight=weight, grad_output=grad_output)
    s, p, d = _pair(stride), _pair(padding), _pair(dilation)
    input, offset, weight, grad_output = input.contiguous(), offset.contiguous(), weight.contiguous(), grad_output.contiguous()
    g = _geom2d(input.shape, weight.shape, s, p, d, offset.shape[1])
    dt = L.dtype_code(input, allow_f64=True)
    gi, go, gw = grads_like((input, offset, weight), need)
    gb = torch.empty((g.Cout,), dtype=input.dtype, device=input.device) if with_bias else None
    call_ws("deform_conv2d_backward", ("deform_conv2d_backward_workspace", byref(g), dt), input, L.ptr(input), L.ptr(offset), L.ptr(weight),
            L.ptr(grad_output), L.ptr(gi), L.ptr(go), L.ptr(gw), L.ptr(gb), WS, byref(g), dt, L.stream_ptr(input), label="deform_conv2d backward")
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
    call("deform_conv2d_sample_index_path", L.ptr(offset), L.ptr(idx), L.ptr(mask), byref(g), L.dtype_code(offset), int(path), L.stream_ptr(offset),
         label="deform_conv2d_sample_index")
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
    dt = L.dtype_code(x)
    out = torch.empty_like(x)
    call_ws("deform_dwconv2d_forward_cl", ("deform_dwconv2d_cl_workspace", byref(g), dt, 0), x, L.ptr(x), L.ptr(offset), L.ptr(weight), L.ptr(out), WS,
            byref(g), dt, L.stream_ptr(x))
    return out


def deform_dwconv2d_backward_cl(x, offset, weight, grad_out, padding, dilation=1):
    """-> (grad_x [B,H,W,C], grad_offset [B,2K,H,W], grad_weight [C,1,kh,kw])."""
    L.require_device(x, offset, weight, grad_out)
    x, offset, weight, grad_out = x.contiguous(), offset.contiguous(), weight.contiguous(), grad_out.contiguous()
    g = _geom_dw2d_cl(x, weight, padding, dilation)
    dt = L.dtype_code(x)
    gx, go, gw = torch.empty_like(x), torch.empty_like(offset), torch.empty_like(weight)
    call_ws("deform_dwconv2d_backward_cl", ("deform_dwconv2d_cl_workspace", byref(g), dt, 1), x, L.ptr(x), L.ptr(offset), L.ptr(weight),
            L.ptr(grad_out), L.ptr(gx), L.ptr(go), L.ptr(gw), WS, byref(g), dt, L.stream_ptr(x))
    return gx, go, gw
