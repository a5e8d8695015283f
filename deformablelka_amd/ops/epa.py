"""The UNETR++ efficient paired attention — ``dlka_epa_attention_*`` (csrc/cl_epa.hip): everything of ``EPA.forward`` between the ``qkvv`` Linear and the two
output projections.  Reached as a submodule (``from deformablelka_amd.ops import epa``); the package's public names stay as they are."""
from __future__ import annotations

import torch

from .. import _lib as L
from ._call import call

HEAD_WIDTHS = (8, 16, 32, 64)
PROJ_SIZES = (32, 64)


def supported(C, heads, P, dtype) -> bool:
    """Whether the fused calls cover (hidden_size C, heads, proj_size P, dtype): float32, C / heads in HEAD_WIDTHS, P in PROJ_SIZES."""
    if dtype != torch.float32 or heads <= 0 or C % heads:
        return False
    return bool(L.get_lib().dlka_epa_supported(int(C), int(heads), int(P), L.DLKA_F32))


def _check(qkvv, kp, vp, temperature, temperature2, m1, m2):
    L.require_device(qkvv, kp, vp, temperature, temperature2, m1, m2)
    for name, t in (("qkvv", qkvv), ("kp", kp), ("vp", vp), ("temperature", temperature), ("temperature2", temperature2), ("m1", m1)):
        if t is not None and t.dtype != torch.float32:
            raise RuntimeError(f"epa attention: `{name}` must be float32, got {t.dtype}")
    if m2 is not None and m2.dtype not in (torch.uint8, torch.bool):
        raise RuntimeError(f"epa attention: `m2` is one keep byte per element (uint8 or bool), got {m2.dtype}")
    if qkvv.ndim != 3 or qkvv.shape[2] % 4:
        raise RuntimeError(f"epa attention: qkvv [B, N, 4 C] expected, got {tuple(qkvv.shape)}")
    B, N, C = int(qkvv.shape[0]), int(qkvv.shape[1]), int(qkvv.shape[2]) // 4
    heads = temperature.numel()
    if temperature2.numel() != heads or heads == 0 or C % heads:
        raise RuntimeError(f"epa attention: {temperature.numel()} / {temperature2.numel()} temperatures for C = {C}")
    if kp.ndim != 3 or tuple(kp.shape[:2]) != (B, C) or kp.shape != vp.shape:
        raise RuntimeError(f"epa attention: kp and vp [B, C, P] = [{B}, {C}, P] expected, got {tuple(kp.shape)} and {tuple(vp.shape)}")
    P, D = int(kp.shape[2]), C // heads
    if m1 is not None and m1.numel() != B * heads * D * D:
        raise RuntimeError(f"epa attention: m1 [B, heads, D, D] expected, got {tuple(m1.shape)}")
    if m2 is not None and m2.numel() != B * heads * N * P:
        raise RuntimeError(f"epa attention: m2 [B, heads, N, P] expected, got {tuple(m2.shape)}")
    return B, N, C, heads, P


def _contig(*ts):
    """Contiguous and 16-byte aligned, as the kernels' vector accesses need (a contiguous view at an odd storage offset is copied)."""
    out = []
    for t in ts:
        if t is not None:
            t = t.contiguous()
            if t.data_ptr() % 16:
                t = t.clone()
        out.append(t)
    return out


def attention_forward(qkvv, kp, vp, temperature, temperature2, m1=None, m2=None, m2_scale=1.0):
    """qkvv [B, N, 4 C] (the Linear's output), kp / vp [B, C, P], temperature / temperature2 [heads, 1, 1]; m1 float32 [B, heads, D, D] multipliers,
    m2 keep bytes [B, heads, N, P] (a kept element is multiplied by m2_scale).  Returns (x_sa, x_ca, saved): both [B, N, C], x_sa in the reference's
    permute-and-reshape order.  A width or dtype outside the fused set raises (DLKA_ERR_UNSUPPORTED)."""
    B, N, C, heads, P = _check(qkvv, kp, vp, temperature, temperature2, m1, m2)
    qkvv, kp, vp, temperature, temperature2, m1, m2 = _contig(qkvv, kp, vp, temperature, temperature2, m1, m2)
    lib = L.get_lib()
    wb = lib.dlka_epa_workspace_bytes(B, N, C, heads, P, 0)
    if wb == 0:
        L.check(-8, "epa_attention_forward")
    saved, ws = L.scratch(lib.dlka_epa_saved_bytes(B, C, heads), qkvv), L.scratch(wb, qkvv)
    x_sa = torch.empty((B, N, C), dtype=torch.float32, device=qkvv.device)
    x_ca = torch.empty_like(x_sa)
    call("epa_attention_forward", L.ptr(qkvv), L.ptr(kp), L.ptr(vp), L.ptr(temperature), L.ptr(temperature2), L.ptr(m1), L.ptr(m2), float(m2_scale),
         L.ptr(x_sa), L.ptr(x_ca), L.ptr(saved), L.ptr(ws), wb, B, N, C, heads, P, L.DLKA_F32, L.stream_ptr(qkvv))
    return x_sa, x_ca, saved


def attention_backward(qkvv, kp, vp, temperature, temperature2, g_x_sa, g_x_ca, saved, m1=None, m2=None, m2_scale=1.0):
    """-> (g_qkvv [B, N, 4 C], g_kp, g_vp [B, C, P], g_temperature, g_temperature2 [heads, 1, 1]).  g_qkvv holds the gradient through Q, the channel
    branch's K and Vc; K's and Vs's parts through kp / vp are the caller's GEMMs."""
    B, N, C, heads, P = _check(qkvv, kp, vp, temperature, temperature2, m1, m2)
    L.require_device(g_x_sa, g_x_ca, saved)
    qkvv, kp, vp, temperature, temperature2, m1, m2 = _contig(qkvv, kp, vp, temperature, temperature2, m1, m2)
    g_x_sa, g_x_ca = _contig(g_x_sa.to(torch.float32), g_x_ca.to(torch.float32))
    lib = L.get_lib()
    wb = lib.dlka_epa_workspace_bytes(B, N, C, heads, P, 1)
    if wb == 0:
        L.check(-8, "epa_attention_backward")
    ws = L.scratch(wb, qkvv)
    g_qkvv, g_kp, g_vp = torch.empty_like(qkvv), torch.empty_like(kp), torch.empty_like(vp)
    g_t = torch.empty((B, heads), dtype=torch.float32, device=qkvv.device)
    g_t2 = torch.empty_like(g_t)
    call("epa_attention_backward", L.ptr(qkvv), L.ptr(kp), L.ptr(vp), L.ptr(temperature), L.ptr(temperature2), L.ptr(m1), L.ptr(m2), float(m2_scale),
         L.ptr(saved), L.ptr(g_x_sa), L.ptr(g_x_ca), L.ptr(g_qkvv), L.ptr(g_kp), L.ptr(g_vp), L.ptr(g_t), L.ptr(g_t2), L.ptr(ws), wb, B, N, C, heads, P,
         L.DLKA_F32, L.stream_ptr(qkvv))
    return g_qkvv, g_kp, g_vp, g_t.sum(0).view_as(temperature), g_t2.sum(0).view_as(temperature2)
