"""The plain (non-deformable) 2-D LKA block — ``dlka_lka2d_plain_attention_*`` — and its two depthwise convs on their own (``dlka_dwconv2d_*_cl``,
csrc/cl_dw2d.hip).  Reached as a submodule (``from deformablelka_amd.ops import lka2d_plain``); the package's public names stay as they are."""
from __future__ import annotations

from ctypes import byref
from typing import Sequence

import torch

from .. import _lib as L
from ._call import WS, Block, _pair, block_backward, block_forward, call_ws, require_fp32_params
from ._call import lka2d_width_ok as supported   # noqa: F401  (widths the fused block covers, in float32 and with bfloat16 activations alike)

ACTIVATION_DTYPES = (torch.float32, torch.bfloat16)


def _fp32_params(what, x, **named):
    """float32 or bfloat16 activations next to float32 parameters; anything else is refused before a launch."""
    if x.dtype not in ACTIVATION_DTYPES:
        raise RuntimeError(f"{what}: float32 or bfloat16 activations, got {x.dtype}")
    require_fp32_params(what, x, **named)


def _block_params(x, params):
    _fp32_params("LKA_Attention", x, **dict(zip(L.LKA2D_PLAIN_FIELDS, params)))
    return [t.contiguous() for t in params]


_PLAIN = Block("lka2d_plain_attention", "lka2d_plain", "", L.Lka2dPlainPtrs, L.LKA2D_PLAIN_FIELDS, _block_params,
               lambda x, dims: tuple(int(v) for v in x.shape), -8, True)


def attention_forward(x, params: Sequence[torch.Tensor]):
    """x: [B,C,H,W]; params: the 10 tensors in ``_lib.LKA2D_PLAIN_FIELDS`` order (float32).  Returns (y, saved).  A width or dtype outside the fused set
    raises (DLKA_ERR_UNSUPPORTED)."""
    return block_forward(_PLAIN, x, params)


def attention_backward(x, params, grad_y, saved):
    """-> (grad_x, the 10 parameter gradients)."""
    return block_backward(_PLAIN, x, params, grad_y, saved)


# ---- the depthwise convs on their own: x [B, H, W, C] ------------------------------------------------------------------------------------------
def _geom(x, weight, padding, dilation):
    B, H, W, C = (int(v) for v in x.shape)
    p, d = _pair(padding), _pair(dilation)
    if weight.ndim != 4 or tuple(weight.shape[:2]) != (C, 1):
        raise RuntimeError(f"depthwise weight [C][1][k][k] expected, got {tuple(weight.shape)}")
    kh, kw = int(weight.shape[2]), int(weight.shape[3])
    return L.ConvGeom(B, C, 1, H, W, C, 1, kh, kw, 1, 1, 1, 0, p[0], p[1], 1, d[0], d[1], C, 1, 64)


def dwconv2d_forward_cl(x, weight, bias, padding, dilation=1):
    """Channels-last depthwise conv with bias: x [B,H,W,C] (float32 or bfloat16), weight [C,1,k,k] and bias [C] (or None) float32 -> out [B,H,W,C]
    of x's dtype.  (k, dilation, padding) = (5, 1, 2) or (7, 3, 9), C a multiple of 32."""
    L.require_device(x, weight, bias)
    _fp32_params("dwconv2d_forward_cl", x, weight=weight, bias=bias)
    x, weight = x.contiguous(), weight.contiguous()
    bias = None if bias is None else bias.contiguous()
    g = _geom(x, weight, padding, dilation)
    dt = L.dtype_code(x)
    out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    call_ws("dwconv2d_forward_cl", ("dwconv2d_cl_workspace", byref(g), dt, 0), x, L.ptr(x), L.ptr(weight), L.ptr(bias), L.ptr(out), WS, byref(g), dt,
            L.stream_ptr(x))
    return out


def dwconv2d_backward_cl(x, weight, grad_out, padding, dilation=1):
    """-> (grad_x [B,H,W,C] of x's dtype, grad_weight [C,1,k,k] float32, grad_bias [C] float32)."""
    L.require_device(x, weight, grad_out)
    _fp32_params("dwconv2d_backward_cl", x, weight=weight)
    if grad_out.dtype != x.dtype:
        raise RuntimeError(f"dwconv2d_backward_cl: `grad_out` must have x's dtype ({x.dtype}), got {grad_out.dtype}")
    x, weight, grad_out = x.contiguous(), weight.contiguous(), grad_out.contiguous()
    g = _geom(x, weight, padding, dilation)
    dt = L.dtype_code(x)
    gx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    gw = torch.empty(weight.shape, dtype=torch.float32, device=x.device)
    gb = torch.empty((g.C,), dtype=torch.float32, device=x.device)
    call_ws("dwconv2d_backward_cl", ("dwconv2d_cl_workspace", byref(g), dt, 1), x, L.ptr(x), L.ptr(weight), L.ptr(grad_out), L.ptr(gx), L.ptr(gw),
            L.ptr(gb), WS, byref(g), dt, L.stream_ptr(x))
    return gx, gw, gb
