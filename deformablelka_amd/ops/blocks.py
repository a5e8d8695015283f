"""The fused blocks: the D-LKA attention (planar 3-D, 2-D, token layout) and TransformerBlock_3D_single_deform_LKA around it.

The three attention blocks go through ``_call.block_forward`` / ``block_backward``.  The wrapper block stays written out: it has two parameter structs, optional
parameters, its own inputs (drop mask, BatchNorm statistics, two epsilons) and takes its dtype from a flag, not from x."""
from __future__ import annotations

import ctypes
from ctypes import byref
from typing import Sequence

import torch

from .. import _lib as L
from ._call import (Block, block_backward, block_backward_args, block_forward, call, lka2d_width_ok, ptr_struct, require_fp32_params, saved_view,
                    side_stream_phases)

lka2d_bf16_supported = lka2d_width_ok   # widths the DLKA_BF16 2-D block covers: the channels-last fast path's


def _fp32_params(what, fields, x, params):
    """Parameters are fp32 masters whatever the activation dtype is."""
    require_fp32_params(what, x, **dict(zip(fields, params)))
    return [t.contiguous() for t in params]


def _lka2d_params(x, params):
    if x.dtype == torch.bfloat16:   # DLKA_BF16: bf16 ACTIVATIONS, fp32 master parameters (include/dlka.h)
        if not lka2d_bf16_supported(int(x.shape[1])):
            raise RuntimeError(f"deformable_LKA_Attention with bfloat16 activations needs C / 32 in {{1,2,3,4,6,8,12}}, got C={int(x.shape[1])}")
        return _fp32_params("deformable_LKA_Attention", L.LKA2D_FIELDS, x, params)
    return [t.contiguous() for t in params]


def _planar_extents(x, dims):
    return tuple(int(v) for v in x.shape)


_LKA3D = Block("lka3d_attention", "lka3d", "", L.Lka3dPtrs, L.LKA3D_FIELDS, lambda x, params: [t.contiguous() for t in params], _planar_extents, -4, False)
_LKA2D = Block("lka2d_attention", "lka2d", "", L.Lka2dPtrs, L.LKA2D_FIELDS, _lka2d_params, _planar_extents, -4, True)
_TOKENS = Block("lka3d_attention_tokens", "lka3d_tokens", "_v", L.Lka3dPtrs, L.LKA3D_FIELDS,
                lambda x, params: _fp32_params("the token-layout D-LKA block", L.LKA3D_FIELDS, x, params),
                lambda x, dims: (int(x.shape[0]), int(x.shape[2]), *(int(v) for v in dims)), -8, True)


# ---- the D-LKA attention, planar: x [B,C,D,H,W] / [B,C,H,W] ------------------------------------------------------------------------------
def lka3d_attention_forward(x, params: Sequence[torch.Tensor]):
    """x: [B,C,D,H,W]; params: the 14 tensors in ``_lib.LKA3D_FIELDS`` order. Returns (y, saved)."""
    return block_forward(_LKA3D, x, params)


def lka3d_attention_backward(x, params, grad_y, saved):
    return block_backward(_LKA3D, x, params, grad_y, saved)


def lka2d_attention_forward(x, params: Sequence[torch.Tensor]):
    return block_forward(_LKA2D, x, params)


def lka2d_saved_offsets(saved, x):
    """The two predicted offset tensors ([B, 50, H, W] of conv0, [B, 98, H, W] of conv_spatial; torchvision's planar layout) inside the opaque
    ``saved`` buffer of ``lka2d_attention_forward(x, ...)`` — for the path such a call takes now (``dlka_lka2d_saved_offsets``).  Diagnostics:
    the parity tests' cell-flip analysis reads them."""
    B, C, H, W = (int(v) for v in x.shape)
    offs = (ctypes.c_size_t * 2)()
    eb = ctypes.c_int(0)
    call("lka2d_saved_offsets", B, C, H, W, L.dtype_code(x), offs, byref(eb))
    dt = torch.float32 if eb.value == 4 else torch.bfloat16
    return [saved_view(saved, o, (B, ch, H, W), dt) for o, ch in zip(offs, (50, 98))]


def lka2d_attention_backward(x, params, grad_y, saved):
    return block_backward(_LKA2D, x, params, grad_y, saved)


# ---- the D-LKA attention in token layout: x [B, N, C] ------------------------------------------------------------------------------------
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


def lka3d_attention_tokens_forward(x, params, dims, variant=0):
    """x: [B, N, C] tokens, dims = (D, H, W) spatial extents (the reference's H, W, D). Returns (y, saved)."""
    assert x.shape[1] == int(dims[0]) * int(dims[1]) * int(dims[2])
    return block_forward(_TOKENS, x, params, dims, (int(variant),))


def lka3d_tokens_saved_offsets(saved, B, C, dims, act_dtype=torch.float32, variant=0):
    """The predicted sampling offsets [B, 81, D, H, W] (fp32, the reference's planar layout) inside the opaque ``saved`` buffer of a token-layout
    forward call (``dlka_lka3d_tokens_saved_offsets_v``; the NCDHW entry point's fp32 ``saved`` starts with the same four tensors).  Diagnostics:
    bench.py's health check and the cell-flip analysis of the parity tests read them."""
    D, H, W = (int(v) for v in dims)
    off = ctypes.c_size_t(0)
    dt = L.DLKA_F32 if act_dtype == torch.float32 else L.DLKA_BF16
    if L.get_lib().dlka_lka3d_tokens_saved_offsets_v(B, C, D, H, W, dt, int(variant), byref(off)) != 0:   # widths outside the token path (general NCDHW entry)
        sb = 4 if act_dtype == torch.float32 else 2
        off = ctypes.c_size_t(4 * ((B * C * D * H * W * sb + 255) & ~255))
    return saved_view(saved, off.value, (B, 81, D, H, W))


def lka3d_attention_tokens_backward(x, params, grad_y, saved, dims, variant=0, side_stream=None):
    """side_stream (a torch.cuda.Stream, optional): the pass in two parts (``dlka_lka3d_attention_tokens_backward_phase_v``) — the data-gradient chain on the current
    stream, the five weight-gradient launches and the fold of their partial sums on ``side_stream`` behind an event — and NOT joined: the returned parameter gradients are
    complete only once the current stream has waited for ``side_stream`` (``transformerblock.WgradOverlap`` joins once per backward pass).  Returns (gx, grads, keep):
    ``keep`` = what the side stream still reads, to be held until the join.  "inline": both parts on the current stream (tests)."""
    if side_stream is None:
        return block_backward(_TOKENS, x, params, grad_y, saved, dims, (int(variant),))
    args, tail, gx, grads, (ws, grad_y, saved, x) = block_backward_args(_TOKENS, x, params, grad_y, saved, dims, (int(variant),))
    lib = L.get_lib()
    pb = lib.dlka_lka3d_tokens_partials_bytes_v(*tail)
    part = L.scratch(pb, x)
    nplan = lib.dlka_wgrad_finalize_plan_bytes(1)
    plan = torch.zeros(nplan, dtype=torch.uint8)   # host job table of ONE block (its folds are launched per slot: no device copy is needed)
    planp = ctypes.c_void_p(plan.data_ptr())
    call("wgrad_finalize_plan_init", planp, nplan, 1)

    def run_phase(phase, stream):
        if phase == 1:
            call("lka3d_attention_tokens_backward_phase_v", *args, L.ptr(part), pb, None, 0, 1, *tail, stream,
                 label="lka3d_attention_tokens_backward (data chain)")
        else:
            call("lka3d_attention_tokens_backward_phase_v", *args, L.ptr(part), pb, planp, 0, 2, *tail, stream,
                 label="lka3d_attention_tokens_backward (weight gradients)")
            call("wgrad_finalize_run_slot", planp, 0, stream)

    side_stream_phases(run_phase, x, side_stream)
    return gx, grads, [ws, part, grad_y, saved, x]


# ---- TransformerBlock_3D_single_deform_LKA (transformerblock.py:570-630): the wrapper around the D-LKA block -----------------------------
def tblock3d_supported(x, B, C, D, H, W, variant=0) -> bool:
    if x.dtype != torch.float32:
        return False
    return bool(L.get_lib().dlka_tblock3d_supported_v(B, C, D, H, W, L.DLKA_F32, int(variant)))


def tblock3d_lka_bf16_supported(B, C, D, H, W, variant=0) -> bool:
    """The wrapper block's MIXED mode (include/dlka.h: dtype = DLKA_BF16 on dlka_tblock3d_*): fp32 wrapper tensors, the D-LKA attention inside on bf16 activations."""
    return bool(L.get_lib().dlka_tblock3d_supported_v(B, C, D, H, W, L.DLKA_BF16, int(variant)))


def tblock3d_saved_offsets(saved, B, C, dims, variant=0, lka_bf16=False):
    """The same tensor inside the ``saved`` buffer of a wrapper-block forward call (``tblock3d_forward``)."""
    D, H, W = (int(v) for v in dims)
    off = ctypes.c_size_t(0)
    call("tblock3d_saved_offsets_v", B, C, D, H, W, L.DLKA_BF16 if lka_bf16 else L.DLKA_F32, int(variant), byref(off), label="tblock3d_saved_offsets")
    return saved_view(saved, off.value, (B, 81, D, H, W))


def tblock3d_saved_activation_signs(saved, B, C, dims, variant=0, lka_bf16=False):
    """(a1 > 0, rd > 0, rd != 0) as bool tensors [B, N, C]: the activation pattern of UnetResBlock's two LeakyReLUs in the forward call that wrote ``saved``
    (``dlka_tblock3d_saved_activations_v``; rd carries the Dropout3d multipliers: a dropped channel is all zeros, hence the third tensor).  Diagnostics for
    the parity tests' kink analysis."""
    D, H, W = (int(v) for v in dims)
    offs = (ctypes.c_size_t * 2)()
    call("tblock3d_saved_activations_v", B, C, D, H, W, L.DLKA_BF16 if lka_bf16 else L.DLKA_F32, int(variant), offs, label="tblock3d_saved_activations")
    a1, rd = (saved_view(saved, o, (B, D * H * W, C)) for o in offs)
    return a1 > 0, rd > 0, rd != 0


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
    ps = ptr_struct(L.TBlock3dPtrs, L.TBLOCK3D_FIELDS, tparams)
    lk = ptr_struct(L.Lka3dPtrs, L.LKA3D_FIELDS, lka_params)
    call("tblock3d_forward_v", L.ptr(x), int(bool(x_planar)), byref(ps), byref(lk), L.ptr(drop_mask), int(bool(training)), L.ptr(bn_stats), L.ptr(y),
         L.ptr(saved), sb, L.ptr(ws), wb, B, C, D, H, W, float(ln_eps), float(bn_eps), dt, v, L.stream_ptr(x), label="tblock3d_forward")
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
    dt = L.DLKA_BF16 if lka_bf16 else L.DLKA_F32
    grad_y = grad_y.float()
    wb = L.get_lib().dlka_tblock3d_workspace_bytes_v(B, C, D, H, W, dt, int(variant))
    ws = L.scratch(wb, grad_y)
    gx = torch.empty_like(grad_y)
    tg = [None if t is None else torch.empty_like(t) for t in tparams]
    lg = [torch.empty_like(t) for t in lka_params]
    ps, gs = ptr_struct(L.TBlock3dPtrs, L.TBLOCK3D_FIELDS, tparams), ptr_struct(L.TBlock3dPtrs, L.TBLOCK3D_FIELDS, tg)
    lk, gl = ptr_struct(L.Lka3dPtrs, L.LKA3D_FIELDS, lka_params), ptr_struct(L.Lka3dPtrs, L.LKA3D_FIELDS, lg)
    args = (byref(ps), byref(lk), L.ptr(drop_mask), int(bool(training)), L.ptr(bn_stats), L.ptr(grad_y), L.ptr(saved),
            saved.numel(), L.ptr(gx), byref(gs), byref(gl), L.ptr(ws), wb, B, C, D, H, W, dt, int(variant))
    if side_stream is None:
        call("tblock3d_backward_v", *args, L.stream_ptr(grad_y), label="tblock3d_backward")
        return gx, tg, lg
    side_stream_phases(lambda phase, stream: call("tblock3d_backward_phase_v", *args, phase, stream,
                                                  label=f"tblock3d_backward ({'data chain' if phase == 1 else 'weight gradients'})"),
                       grad_y, side_stream)
    if isinstance(side_stream, str):
        return gx, tg, lg
    return gx, tg, lg, [ws, grad_y, saved, bn_stats, drop_mask]
