"""Resampling of probabilities, images and label maps, and the cubic B-spline prefilter the pipeline modules share."""
from ctypes import byref

import numpy as np
import torch

from .. import _lib as L
from ._call import _I3, _RS_DTYPES, call, table_dtype


# ---- resampling of probabilities, images and label maps (include/dlka.h: dlka_resample_*) ---------------------------------------------------
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
    table_dtype(x, _RS_DTYPES, "resample", "float32 or float64 volumes")
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
    call("resample_argmax", L.ptr(x), L.ptr(labels), byref(d), L.ptr(ci), L.ptr(wi), L.ptr(region), L.stream_ptr(x))
    return labels


def resample_linear(x, out, tables):
    """``x`` (c, x, y, z; float32 / float64) resampled by the per-axis linear tables, every channel stored."""
    taps = [np.asarray(w).shape[1] for _, w in tables]
    d, out = _rs_desc(x, out, taps, 2, _RS_DTYPES.get(x.dtype))
    table_dtype(x, _RS_DTYPES, "resample", "float32 or float64 volumes")
    x = x.contiguous()
    ci, wi = _rs_tables(x, tables, out, 2, False)
    y = torch.empty((d.C,) + out, dtype=x.dtype, device=x.device)
    call("resample_linear", L.ptr(x), L.ptr(y), byref(d), L.ptr(ci), L.ptr(wi), L.stream_ptr(x))
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
    call("resample_labels", L.ptr(seg), L.ptr(y), byref(d), L.ptr(ci), L.ptr(wi), int(bool(strict)), L.stream_ptr(seg))
    return y


def spline_coefficients(x, pad, boundary, axes, out=None):
    """float64 cubic B-spline coefficients of ONE volume ``x`` (x, y, z; float32 / float64) as scipy.ndimage.spline_filter prepares them:
    ``pad[ax]`` edge samples on both sides (all 0: the cast alone) in one launch, then ``spline_prefilter``.  ``out``: where to write."""
    L.require_device(x, out)
    x, ext = x.contiguous(), [int(n) + 2 * int(p) for n, p in zip(x.shape, pad)]
    out = torch.empty(ext, dtype=torch.float64, device=x.device) if out is None else out
    if x.ndim != 3 or x.dtype not in _RS_DTYPES or list(out.shape) != ext or out.device != x.device:
        raise RuntimeError(f"spline: one float32 / float64 volume (x, y, z) and room for {ext}, got {tuple(x.shape)} {x.dtype}, {tuple(out.shape)}")
    call("spline_pad", L.ptr(x), L.ptr(out), _RS_DTYPES[x.dtype], _I3(*x.shape), _I3(*pad), L.stream_ptr(x))
    return spline_prefilter(out, boundary, axes)


def spline_prefilter(coef, boundary, axes):
    """In place: one launch per axis in ``axes`` with the start values of ``boundary`` (DLKA_SPLINE_REFLECT / DLKA_SPLINE_MIRROR)."""
    L.require_device(coef)
    if coef.ndim != 3 or coef.dtype != torch.float64 or not coef.is_contiguous():
        raise RuntimeError(f"spline: a contiguous float64 volume (x, y, z), got {tuple(coef.shape)} {coef.dtype}")
    for ax in axes:
        call("spline_prefilter", L.ptr(coef), _I3(*coef.shape), int(ax), int(boundary), L.stream_ptr(coef))
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
    call("resample_spline_eval", L.ptr(coef), L.ptr(y), byref(d), L.ptr(ci), L.ptr(wi), L.ptr(lo.contiguous()), L.ptr(hi.contiguous()), int(clip_axis),
         L.stream_ptr(x))
    return y
