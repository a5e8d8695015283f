"""Case preprocessing: nonzero mask, crop, normalisation."""
from ctypes import byref

import numpy as np
import torch

from .. import _lib as L
from .. import ops as _ops   # another family's wrapper is called through the package, as the product modules call it
from ._call import WS, _rank_padded_ext, call, call_ws


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
    bg = torch.empty(data.shape[1:], dtype=torch.uint8, device=data.device)
    call("prep_background", L.ptr(data), byref(d), L.ptr(bg), L.stream_ptr(data))
    labels, _, _, _ = _ops.cc_components(bg, None, 1, want_filtered=False)
    mask = torch.empty_like(bg)
    box = torch.empty(8, dtype=torch.int32, device=data.device)
    call_ws("prep_fill_bbox", ("prep_fill_workspace_bytes", byref(d)), data, L.ptr(bg), L.ptr(labels), byref(d), WS, L.ptr(mask), L.ptr(box),
            L.stream_ptr(data))
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
    call("prep_mask_bbox", L.ptr(mask), byref(d), L.ptr(box), L.stream_ptr(mask))
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
    call("prep_crop", L.ptr(data), L.ptr(seg), L.ptr(mask), byref(d), L.ptr(out), L.ptr(seg_out), L.stream_ptr(data))
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
    if (host[:, 0] != L.DLKA_PREP_CT).any():
        call_ws("prep_channel_stats", ("prep_stats_workspace_bytes", byref(d)), data, L.ptr(data), L.ptr(seg_last), byref(d), L.ptr(table), WS,
                L.stream_ptr(data))
    out = torch.empty_like(data)
    call("prep_normalize", L.ptr(data), L.ptr(seg_last), byref(d), L.ptr(table), L.ptr(out), L.stream_ptr(data))
    return out, table
