"""Inference plumbing: sliding-window tiles with test-time mirroring, and the 2-D evaluator's slice resampling."""
from __future__ import annotations

import ctypes
from ctypes import byref

import numpy as np
import torch

from .. import _lib as L
from .. import ops as _ops   # another family's wrapper is called through the package, as the product modules call it
from ._call import _RS_DTYPES, _ZM_DTYPES, call


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
    call("tiles_gather", L.ptr(x), *x.shape, _int_array(v for o in origins for v in o), T, _int_array(masks), M, pd, ph, pw, *(int(v) for v in pad_lo),
         float(pad_value), L.ptr(out), L.stream_ptr(x))
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
    call("tiles_blend", L.ptr(logits), L.dtype_code(logits), K, int(nonlin), float(mirror_scale), L.ptr(gauss), L.ptr(score), L.ptr(weight), *weight.shape,
         _int_array(v for o in origins for v in o), T, _int_array(masks), M, *logits.shape[2:], L.stream_ptr(logits))


def tiles_finalize(score, weight, pad_lo, shape):
    """The kept region [pad_lo, pad_lo + shape): (seg (X, Y, Z) int64 = argmax, probs (K, X, Y, Z) fp32 = score / weight)."""
    L.require_device(score, weight)
    score, weight = score.contiguous(), weight.contiguous()
    K = score.shape[0]
    probs = torch.empty((K,) + tuple(shape), dtype=torch.float32, device=score.device)
    seg = torch.empty(tuple(shape), dtype=torch.int64, device=score.device)
    call("tiles_finalize", L.ptr(score), L.ptr(weight), K, *weight.shape, *(int(v) for v in pad_lo), *(int(v) for v in shape), L.ptr(probs), L.ptr(seg),
         L.stream_ptr(score))
    return seg, probs


# ---- the 2-D evaluator's slice resampling (include/dlka.h: dlka_zoom2d_*) -----------------------------------------------------------------------
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
        return _ops.spline_coefficients(x, (0, 0, 0), L.DLKA_SPLINE_MIRROR, (1, 2))
    if x.dtype in (torch.bfloat16, torch.int16):             # torch's cast: the pad kernel reads float32 / float64 only
        return _ops.spline_prefilter(x.to(torch.float64), L.DLKA_SPLINE_MIRROR, (1, 2))
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
    call("zoom2d_spline", L.ptr(src), L.ptr(y), byref(d), L.ptr(start), L.ptr(w4), L.stream_ptr(src))
    return y


def zoom2d_nearest(x, out_hw, idx):
    """Order 0: ``x`` (n, h, w) of any 1, 2, 4 or 8 byte dtype gathered through the device table of ``zoom2d_index_tables``; outside: 0."""
    x = _zm_stack(x)
    if x.dtype == torch.bool or x.element_size() not in (1, 2, 4, 8) or x.is_complex():
        raise RuntimeError(f"zoom2d: a real dtype of 1, 2, 4 or 8 bytes, got {x.dtype}")
    d, out_hw = _zm_desc(x.shape[0], x.shape[1:], out_hw)
    idx = _zm_table(idx, out_hw[0] + out_hw[1], torch.int32, x, "idx")
    y = torch.empty((x.shape[0],) + out_hw, dtype=x.dtype, device=x.device)
    call("zoom2d_nearest", L.ptr(x), L.ptr(y), byref(d), x.element_size(), L.ptr(idx), L.stream_ptr(x))
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
    call("zoom2d_argmax", L.ptr(logits), L.ptr(out), byref(d), int(logits.shape[1]), L.ptr(idx), L.stream_ptr(logits))
    return out
