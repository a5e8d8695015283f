"""The channels-last operators on their own: the fast-path convs (x [B, D, H, W, C]) and the pieces of the wrapper block."""
from ctypes import byref

import torch

from .. import _lib as L
from ._call import WS, _geom_cl, _triple, call, call_ws, grads_like


# ---- channels-last fast path (fp32): x [B, D, H, W, C] -----------------------------------------------------------------------------------
def conv3d_forward_cl(x, weight, bias=None, padding=0, dilation=1, groups=1, out_planar=False):
    L.require_device(x, weight, bias)
    p, d = _triple(padding), _triple(dilation)
    x, weight = x.contiguous(), weight.contiguous()
    bias = None if bias is None else bias.contiguous()
    g = _geom_cl(x.shape, weight.shape[0], tuple(weight.shape[2:5]), p, d, groups)
    dt = L.dtype_code(x)
    B, D, H, W, _ = x.shape
    shape = (B, g.Cout, D, H, W) if out_planar else (B, D, H, W, g.Cout)
    out = torch.empty(shape, dtype=x.dtype, device=x.device)
    call_ws("conv3d_forward_cl", ("conv3d_cl_workspace", byref(g), dt, 0), x, L.ptr(x), L.ptr(weight), L.ptr(bias), L.ptr(out), int(out_planar), WS,
            byref(g), dt, L.stream_ptr(x))
    return out


def conv3d_backward_cl(x, weight, grad_out, padding=0, dilation=1, groups=1, grad_out_planar=False, need=(True, True, True)):
    """-> (grad_x, grad_weight, grad_bias); a gradient ``need`` does not ask for is passed to the library as null and returned as None (no gradient asked
    for: no library call)."""
    L.require_device(x, weight, grad_out)
    p, d = _triple(padding), _triple(dilation)
    x, weight, grad_out = x.contiguous(), weight.contiguous(), grad_out.contiguous()
    g = _geom_cl(x.shape, weight.shape[0], tuple(weight.shape[2:5]), p, d, groups)
    dt = L.dtype_code(x)
    if not any(need):
        return None, None, None
    gi, gw = grads_like((x, weight), need)
    gb = torch.empty((g.Cout,), dtype=x.dtype, device=x.device) if need[2] else None
    call_ws("conv3d_backward_cl", ("conv3d_cl_workspace", byref(g), dt, 1), x, L.ptr(x), L.ptr(weight), L.ptr(grad_out), int(grad_out_planar),
            L.ptr(gi), L.ptr(gw), L.ptr(gb), WS, byref(g), dt, L.stream_ptr(x))
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
    dt = L.dtype_code(x)
    B, D, H, W, _ = x.shape
    out = torch.empty((B, D, H, W, g.Cout), dtype=x.dtype, device=x.device)
    call_ws("deform_conv3d_forward_cl", ("deform_conv3d_cl_workspace", byref(g), dt, 0), x, L.ptr(x), L.ptr(offset), L.ptr(weight), L.ptr(bias),
            L.ptr(out), WS, byref(g), dt, L.stream_ptr(x))
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
    dt = L.dtype_code(x)
    if not any(need):
        return None, None, None, None
    gdt = deform_cl_grad_dtype(x)
    gi, go, gw, gb = (torch.empty(shape, dtype=gdt, device=x.device) if n else None
                      for shape, n in zip((x.shape, offset.shape, weight.shape, (g.Cout,)), need))
    call_ws("deform_conv3d_backward_cl", ("deform_conv3d_cl_workspace", byref(g), dt, 1), x, L.ptr(x), L.ptr(offset), L.ptr(weight), L.ptr(grad_out),
            L.ptr(gi), L.ptr(go), L.ptr(gw), L.ptr(gb), WS, byref(g), dt, L.stream_ptr(x))
    return gi, go, gw, gb


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
    call("layernorm_tokens_forward", L.ptr(x), int(bool(x_planar)), L.ptr(None if pos is None else pos.contiguous()), L.ptr(weight.contiguous()),
         L.ptr(bias.contiguous()), L.ptr(xt), L.ptr(xn), L.ptr(stats), B, N, C, float(eps), L.dtype_code(x), L.stream_ptr(x))
    return xt, xn, stats


def layernorm_tokens_backward(g_xn, g_res, xt, stats, weight, with_pos=False):
    L.require_device(g_xn, g_res, xt, stats, weight)
    B, N, C = (int(v) for v in xt.shape)
    g_xn = g_xn.contiguous()
    g_res = None if g_res is None else g_res.contiguous()
    gxt = torch.empty_like(xt)
    gw, gb = torch.empty_like(weight), torch.empty_like(weight)
    gpos = torch.empty((1, N, C), dtype=xt.dtype, device=xt.device) if with_pos else None
    call("layernorm_tokens_backward", L.ptr(g_xn), L.ptr(g_res), L.ptr(xt), L.ptr(stats), L.ptr(weight.contiguous()), L.ptr(gxt), L.ptr(gw), L.ptr(gb),
         L.ptr(gpos), B, N, C, L.dtype_code(xt), L.stream_ptr(xt))
    return gxt, gw, gb, gpos


def scale_residual_forward(xt, e, gamma):
    L.require_device(xt, e, gamma)
    xt, e = xt.contiguous(), e.contiguous()
    out = torch.empty_like(xt)
    C = int(xt.shape[-1])
    call("scale_residual_forward", L.ptr(xt), L.ptr(e), L.ptr(gamma.contiguous()), L.ptr(out), xt.numel() // C, C, L.dtype_code(xt), L.stream_ptr(xt))
    return out


def scale_residual_backward(g, e, gamma):
    L.require_device(g, e, gamma)
    g, e = g.contiguous(), e.contiguous()
    ge, gg = torch.empty_like(e), torch.empty_like(gamma)
    C = int(e.shape[-1])
    call("scale_residual_backward", L.ptr(g), L.ptr(e), L.ptr(gamma.contiguous()), L.ptr(ge), L.ptr(gg), e.numel() // C, C, L.dtype_code(e), L.stream_ptr(e))
    return ge, gg


def batchnorm_cl_forward(x, res, weight, bias, stats, training, eps=1e-5, slope=0.01):
    """x: channels-last [..., C].  y = LeakyReLU(BN(x) (+ res)).  stats [3*C] written (training) or read (eval: {mean, rstd})."""
    L.require_device(x, res, weight, bias, stats)
    x = x.contiguous()
    res = None if res is None else res.contiguous()
    C = int(x.shape[-1])
    y = torch.empty_like(x)
    scr = torch.empty(2 * C, dtype=torch.float32, device=x.device)
    call("batchnorm_cl_forward", L.ptr(x), L.ptr(res), L.ptr(weight.contiguous()), L.ptr(bias.contiguous()), L.ptr(stats), int(bool(training)), L.ptr(y),
         L.ptr(scr), x.numel() // C, C, float(eps), float(slope), L.dtype_code(x), L.stream_ptr(x))
    return y


def batchnorm_cl_backward(g, x, y, weight, stats, training, with_res=False, slope=0.01):
    L.require_device(g, x, y, weight, stats)
    g, x, y = g.contiguous(), x.contiguous(), y.contiguous()
    C = int(x.shape[-1])
    gx = torch.empty_like(x)
    gres = torch.empty_like(x) if with_res else None
    gw, gb = torch.empty_like(weight), torch.empty_like(weight)
    scr = torch.empty(2 * C, dtype=torch.float32, device=x.device)
    call("batchnorm_cl_backward", L.ptr(g), L.ptr(x), L.ptr(y), L.ptr(weight.contiguous()), L.ptr(stats), int(bool(training)), L.ptr(gx), L.ptr(gres),
         L.ptr(gw), L.ptr(gb), L.ptr(scr), x.numel() // C, C, float(slope), L.dtype_code(x), L.stream_ptr(x))
    return gx, gres, gw, gb


def channel_scale(x, mask):
    """x [B, ..., C] channels-last, mask [B, C]."""
    L.require_device(x, mask)
    x, mask = x.contiguous(), mask.contiguous()
    B, C = int(x.shape[0]), int(x.shape[-1])
    y = torch.empty_like(x)
    call("channel_scale", L.ptr(x), L.ptr(mask), L.ptr(y), B, x.numel() // (B * C), C, L.dtype_code(x), L.stream_ptr(x))
    return y


def ncdhw_to_ndhwc(x):
    """[B, C, *S] contiguous -> [B, *S, C] contiguous (HIP transpose)."""
    L.require_device(x)
    x = x.contiguous()
    B, C = int(x.shape[0]), int(x.shape[1])
    out = torch.empty((B, *x.shape[2:], C), dtype=x.dtype, device=x.device)
    call("ncdhw_to_ndhwc", L.ptr(x), L.ptr(out), B, C, x.numel() // (B * C), L.dtype_code(x), L.stream_ptr(x))
    return out


def ndhwc_to_ncdhw(x):
    L.require_device(x)
    x = x.contiguous()
    B, C = int(x.shape[0]), int(x.shape[-1])
    out = torch.empty((B, C, *x.shape[1:-1]), dtype=x.dtype, device=x.device)
    call("ndhwc_to_ncdhw", L.ptr(x), L.ptr(out), B, C, x.numel() // (B * C), L.dtype_code(x), L.stream_ptr(x))
    return out
