"""The 3-D trainer's batch loader: the batched crop with padding, and class locations (include/dlka.h: dlka_load_*).

Reached as ``ops.dataload.<name>`` (``from .ops import dataload``): this family is not re-exported on the package."""
import ctypes
from ctypes import byref

import numpy as np
import torch

from .. import _lib as L
from ._call import call

LOAD_MODES = {"constant": L.DLKA_LOAD_CONSTANT, "edge": L.DLKA_LOAD_EDGE}
_LABEL_DTYPES = {torch.float32: L.DLKA_LOAD_F32, torch.int32: L.DLKA_LOAD_I32}


def load_launch_count() -> int:
    """Kernels this family has launched in this process."""
    return int(L.get_lib().dlka_load_launch_count())


def load_crop_batch(cases, bbox_lb, patch_size, mode="constant", constant=0.0):
    """dataset_loading.py:331-368 for a whole batch: (data (B, C, *patch), seg (B, 1, *patch)) float32.  ``cases``: B float32 tensors
    (C + 1, X_b, Y_b, Z_b) on one device, the label map last; ``bbox_lb`` (B, 3) integers.  One launch per DLKA_LOAD_B_MAX samples."""
    cases = list(cases)
    if not cases:
        raise RuntimeError("dataloading: an empty batch")
    L.require_device(*cases)
    lb = np.asarray(bbox_lb, dtype=np.int64)
    patch = tuple(int(v) for v in patch_size)
    if lb.shape != (len(cases), 3) or len(patch) != 3:
        raise RuntimeError(f"dataloading: one lower corner (x, y, z) per case and three patch extents, got {lb.shape} for {len(cases)} cases and {patch}")
    if mode not in LOAD_MODES:
        raise NotImplementedError(f"dataloading: pad_mode={mode!r} (supported: 'constant', 'edge')")
    first = cases[0]
    for t in cases:
        if t.dtype != torch.float32 or t.ndim != 4 or t.shape[0] != first.shape[0] or t.shape[0] < 2 or t.device != first.device or t.numel() == 0:
            raise RuntimeError("dataloading: cases are float32 (C + 1, X, Y, Z) tensors on one device with the same number of channels, got "
                               f"{t.dtype} {tuple(t.shape)} on {t.device}")
        if t[0].numel() >= 2 ** 31:
            raise RuntimeError(f"dataloading: fewer than 2^31 cells per channel, got {t[0].numel()}")
    if min(patch) < 1:
        raise RuntimeError(f"dataloading: empty patch {patch}")
    cases = [t.contiguous() for t in cases]
    B, C = len(cases), first.shape[0] - 1
    data = torch.empty((B, C) + patch, dtype=torch.float32, device=first.device)
    seg = torch.empty((B, 1) + patch, dtype=torch.float32, device=first.device)
    for b0 in range(0, B, L.DLKA_LOAD_B_MAX):
        n = min(L.DLKA_LOAD_B_MAX, B - b0)
        d = L.LoadCropDesc()
        d.B, d.C, d.mode, d.constant = n, C, LOAD_MODES[mode], float(constant)
        for ax in range(3):
            d.patch[ax] = patch[ax]
        for j in range(n):
            s, t = d.sample[j], cases[b0 + j]
            s.data = t.data_ptr()
            for ax in range(3):
                s.ext[ax], s.lb[ax] = int(t.shape[1 + ax]), int(lb[b0 + j, ax])
        call("load_crop_batch", byref(d), L.ptr(data[b0:]), L.ptr(seg[b0:]), L.stream_ptr(first))
    return data, seg


def _classes_desc(seg, classes):
    L.require_device(seg)
    if seg.ndim != 3 or seg.numel() == 0 or seg.dtype not in _LABEL_DTYPES:
        raise RuntimeError(f"dataloading: a float32 or int32 label map (X, Y, Z), got {seg.dtype} {tuple(seg.shape)}")
    if seg.numel() >= 2 ** 31:
        raise RuntimeError(f"dataloading: fewer than 2^31 cells, got {seg.numel()}")
    classes = [int(c) for c in classes]
    if not 1 <= len(classes) <= L.DLKA_LOAD_K_MAX or len(set(classes)) != len(classes):
        raise RuntimeError(f"dataloading: between 1 and {L.DLKA_LOAD_K_MAX} distinct classes, got {classes}")
    d = L.LoadClassesDesc()
    d.K, d.dtype = len(classes), _LABEL_DTYPES[seg.dtype]
    for ax in range(3):
        d.ext[ax] = int(seg.shape[ax])
    for k, c in enumerate(classes):
        d.class_id[k] = c
    return d, seg.contiguous()


def load_class_counts(seg, classes):
    """(totals int32 (K,) on the device = cells of each of ``classes`` in the label map ``seg`` (X, Y, Z), the state ``load_class_select``
    takes).  One read of the map for all classes."""
    d, seg = _classes_desc(seg, classes)
    nbytes = L.get_lib().dlka_load_counts_workspace_bytes(byref(d))
    offsets = L.scratch(nbytes, seg)
    totals = torch.empty(d.K, dtype=torch.int32, device=seg.device)
    call("load_class_counts", L.ptr(seg), byref(d), L.ptr(offsets), nbytes, L.ptr(totals), L.stream_ptr(seg))
    return totals, (d, seg, offsets, nbytes)


def load_class_select(state, totals, sel_slot, sel_rank):
    """int32 (M, 3) on the device: row j = the (x, y, z) of cell number ``sel_rank[j]``, in numpy.argwhere's order, among the cells of class
    ``classes[sel_slot[j]]``.  ``state`` from ``load_class_counts``; ``totals`` its totals as the host read them."""
    d, seg, offsets, nbytes = state
    totals = [int(v) for v in totals]
    slot, rank = np.ascontiguousarray(sel_slot, dtype=np.int32), np.ascontiguousarray(sel_rank, dtype=np.int32)
    if len(totals) != d.K or slot.ndim != 1 or slot.shape != rank.shape or slot.size == 0:
        raise RuntimeError(f"dataloading: one total per class ({d.K}) and equally many slots and ranks (at least one), got {len(totals)}, "
                           f"{slot.shape}, {rank.shape}")
    if slot.min() < 0 or slot.max() >= d.K or rank.min() < 0 or bool((rank >= np.asarray(totals, dtype=np.int64)[slot]).any()):
        raise RuntimeError("dataloading: a selected rank lies outside its class")
    host = (ctypes.c_int64 * d.K)(*totals)
    wbytes = L.get_lib().dlka_load_select_workspace_bytes(byref(d), host)
    if wbytes == 0:
        raise RuntimeError(f"dataloading: the totals {totals} do not belong to a label map of {tuple(seg.shape)}")
    locs = L.scratch(wbytes, seg)
    slot_t, rank_t = torch.from_numpy(slot).to(seg.device), torch.from_numpy(rank).to(seg.device)
    out = torch.empty((slot.size, 3), dtype=torch.int32, device=seg.device)
    call("load_class_select", L.ptr(seg), byref(d), L.ptr(offsets), nbytes, host, L.ptr(locs), wbytes, L.ptr(slot_t), L.ptr(rank_t),
         slot.size, L.ptr(out), L.stream_ptr(seg))
    return out
