"""The dataset fingerprint: the foreground sample, its moments, exact order statistics and the labels of a map (include/dlka.h: dlka_dstats_*).

Reached as ``ops.dataset_stats.<name>`` (``from .ops import dataset_stats``): this family is not re-exported on the package."""
import ctypes
from ctypes import byref

import numpy as np
import torch

from .. import _lib as L
from ._call import WS, _rank_padded_ext, call, call_ws

_LABEL_DTYPES = {torch.float32: L.DLKA_DSTATS_F32, torch.int32: L.DLKA_DSTATS_I32}
LAUNCHES = {"fg_count": 2, "fg_sample": 1, "moments": 4, "select": 9, "unique_labels": 1}     # csrc/cl_dataset_stats.hip


def dstats_launch_count() -> int:
    """Kernels this family has launched in this process."""
    return int(L.get_lib().dlka_dstats_launch_count())


def _desc(seg, C=1, step=1):
    """Checks of a label map (*spatial), float32 or int32 as it is stored, and its description."""
    L.require_device(seg)
    if seg.dtype not in _LABEL_DTYPES:
        raise RuntimeError(f"dataset_analysis: the kernels read a float32 or int32 label map as it is stored, got {seg.dtype}")
    if seg.ndim not in (2, 3):
        raise RuntimeError(f"dataset_analysis: a label map of rank 2 or 3, got {tuple(seg.shape)}")
    if seg.numel() == 0:
        raise RuntimeError(f"dataset_analysis: empty extents {tuple(seg.shape)}")
    if seg.numel() >= 2 ** 31:
        raise RuntimeError(f"dataset_analysis: fewer than 2^31 cells, got {seg.numel()}")
    if isinstance(step, bool) or int(step) != step or not 1 <= int(step) < 2 ** 31:
        raise RuntimeError(f"dataset_analysis: step is a positive integer, got {step!r}")
    if not 1 <= C <= L.DLKA_PREP_C_MAX:
        raise RuntimeError(f"dataset_analysis: between 1 and {L.DLKA_PREP_C_MAX} modalities per call, got {C}")
    d = L.DatasetStatsDesc()
    d.C, d.label_dtype, d.step = int(C), _LABEL_DTYPES[seg.dtype], int(step)
    _rank_padded_ext(d, seg.shape)
    return d, seg.contiguous()


def dstats_fg_count(seg):
    """(count int64 (1,) on the device = cells of ``seg`` with a label > 0, the state ``dstats_fg_sample`` takes).  One read of the map."""
    d, seg = _desc(seg)
    count = torch.empty(1, dtype=torch.int64, device=seg.device)
    offsets = call_ws("dstats_fg_count", ("dstats_fg_workspace_bytes", byref(d)), seg, L.ptr(seg), byref(d), WS, L.ptr(count),
                      L.stream_ptr(seg))
    return count, (seg, offsets)


def dstats_fg_sample(data, state, count, step, out, out_offset=0):
    """out[c, out_offset + j] = data[c][seg > 0][::step][j] for the float32 volumes ``data`` (C, *spatial); ``state`` from ``dstats_fg_count``
    of the map, ``count`` its count as the host read it; ``out`` float32 (C, M) contiguous on the device.  Returns the number of samples per
    volume, ceil(count / step); nothing is launched for 0."""
    seg, offsets = state
    L.require_device(data, out)
    if data.dtype != torch.float32 or data.ndim != seg.ndim + 1 or tuple(data.shape[1:]) != tuple(seg.shape) or data.device != seg.device:
        raise RuntimeError(f"dataset_analysis: float32 volumes (C, *spatial) with the label map's extents {tuple(seg.shape)} and device, got "
                           f"{data.dtype} {tuple(data.shape)}")
    d, _ = _desc(seg, data.shape[0], step)
    m = -(-int(count) // int(step))
    if not 0 <= int(count) <= seg.numel():
        raise RuntimeError(f"dataset_analysis: the count {count} does not belong to a label map of {tuple(seg.shape)}")
    if (out.dtype != torch.float32 or out.ndim != 2 or out.shape[0] != data.shape[0] or not out.is_contiguous() or out.device != seg.device
            or out_offset < 0 or out_offset + m > out.shape[1]):
        raise RuntimeError(f"dataset_analysis: a contiguous float32 buffer ({data.shape[0]}, M) with room for {m} samples at {out_offset}, got "
                           f"{out.dtype} {tuple(out.shape)}")
    if m:
        data = data.contiguous()
        call("dstats_fg_sample", L.ptr(data), L.ptr(seg), byref(d), L.ptr(offsets), offsets.numel(), m, L.ptr(out), out.shape[1],
             int(out_offset), L.stream_ptr(seg))
    return m


def _sample(x, what):
    L.require_device(x)
    if x.dtype != torch.float32 or x.ndim != 1:
        raise RuntimeError(f"dataset_analysis: {what} takes a one-dimensional float32 buffer, got {x.dtype} {tuple(x.shape)}")
    if not 1 <= x.numel() < 2 ** 32:
        raise RuntimeError(f"dataset_analysis: {what} takes between 1 and 2^32 - 1 values, got {x.numel()}")
    return x.contiguous()


def dstats_moments(x):
    """float64 (4,) on the device: n, np.mean, np.std and the number of NaNs of the float32 buffer ``x``, summed in float64 in a fixed order."""
    x = _sample(x, "moments")
    result = torch.empty(4, dtype=torch.float64, device=x.device)
    call_ws("dstats_moments", ("dstats_moments_workspace_bytes", x.numel()), x, L.ptr(x), x.numel(), WS, L.ptr(result), L.stream_ptr(x))
    return result


def dstats_select(x, ranks):
    """(values float32 (len(ranks),), nan_count int64 (1,)) on the device: values[j] is the ranks[j]-th smallest of ``x`` (0-based; NaNs last,
    -0.0 as +0.0).  At most DLKA_DSTATS_RANKS_MAX ranks per call."""
    x = _sample(x, "order_statistics")
    ranks = [int(r) for r in ranks]
    if not 1 <= len(ranks) <= L.DLKA_DSTATS_RANKS_MAX:
        raise RuntimeError(f"dataset_analysis: between 1 and {L.DLKA_DSTATS_RANKS_MAX} ranks per call, got {len(ranks)}")
    if min(ranks) < 0 or max(ranks) >= x.numel():
        raise RuntimeError(f"dataset_analysis: ranks lie in 0 .. n - 1 = {x.numel() - 1}, got {ranks}")
    host = (ctypes.c_int64 * len(ranks))(*ranks)
    values = torch.empty(len(ranks), dtype=torch.float32, device=x.device)
    nans = torch.empty(1, dtype=torch.int64, device=x.device)
    call_ws("dstats_select", ("dstats_select_workspace_bytes",), x, L.ptr(x), x.numel(), host, len(ranks), WS, L.ptr(values), L.ptr(nans),
            L.stream_ptr(x))
    return values, nans


def dstats_unique_labels(seg):
    """int32 (DLKA_DSTATS_LABEL_WORDS,) on the device: the presence bitmap of the labels DLKA_DSTATS_LABEL_MIN .. DLKA_DSTATS_LABEL_MAX of
    ``seg``; the last word is nonzero for a label outside that range."""
    d, seg = _desc(seg)
    bitmap = torch.empty(L.DLKA_DSTATS_LABEL_WORDS, dtype=torch.int32, device=seg.device)
    call("dstats_unique_labels", L.ptr(seg), byref(d), L.ptr(bitmap), L.stream_ptr(seg))
    return bitmap


def labels_of_bitmap(words):
    """(sorted label values, outside flag) of a bitmap as the host read it."""
    w = np.asarray(words, dtype=np.int64) & 0xFFFFFFFF
    bits = [32 * i + b for i in range(L.DLKA_DSTATS_LABEL_WORDS - 1) for b in range(32) if (int(w[i]) >> b) & 1]
    return [b + L.DLKA_DSTATS_LABEL_MIN for b in bits], bool(w[-1])
