"""nnU-Net's connected-component post-processing on the HIP kernels of ``csrc/cl_conn_comp.hip`` (include/dlka.h: ``dlka_cc_*``): what the
reference runs on one CPU core with one ``scipy.ndimage.label`` per class and one full-volume comparison per object
(3D/d_lka_former/postprocessing/connected_components.py:48-105; called by ``determine_postprocessing`` at the end of both trainers'
``validate()`` and by ``load_remove_save`` for every case of inference/predict.py).

  ``label``                                            scipy.ndimage.label: nonzero cells, scipy's numbering, ``connectivity`` 1..rank
  ``component_sizes``                                  the same plus the cell count of every object
  ``remove_all_but_the_largest_connected_component``   connected_components.py:48-105, same name, arguments and return triple

Inputs are numpy arrays or torch tensors, on the host or the device; host data is moved to the device.  A tensor in gives a tensor out on the
same device, numpy in gives numpy out, the image in the dtype it came in.  The arguments are NOT written to (the reference edits ``image`` in
place and returns it).  All classes and regions whose id sets are disjoint are labelled, measured and filtered in ONE batched pass; the device is
read once per pass (the per-entry summary) and once more for the image when numpy was asked for.  Without a GPU the calls raise as every operator
of the package does: there is no host fall-back."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib as L
from . import ops
from .ops._call import _SD_DTYPES
from ._containers import load

__all__ = ["label", "component_sizes", "remove_all_but_the_largest_connected_component"]

_MAX_COUNT = 2 ** 31 - 1     # a map has fewer than 2^31 cells


def _as_classes(t):
    """The map in a dtype the kernels read.  Rule of this module: a floating value that is no integer is no class and becomes 0, background
    (metrics maps it to -1, resampling raises): keep the three apart."""
    if t.dtype in _SD_DTYPES:
        return t
    if t.dtype == torch.int8:
        return t.to(torch.int16)
    if t.is_floating_point():
        return torch.where(t == t.round(), t, torch.zeros_like(t)).to(torch.int64)
    raise RuntimeError(f"postprocessing: label maps are uint8, int16, int32, int64, bool, int8 or floating, got {t.dtype}")


def _as_object(t):
    """scipy.ndimage.label's input: nonzero cells."""
    if t.dtype in _SD_DTYPES:
        return t
    if t.dtype == torch.int8 or t.is_floating_point():
        return (t != 0).to(torch.uint8)
    raise RuntimeError(f"postprocessing: label maps are uint8, int16, int32, int64, bool, int8 or floating, got {t.dtype}")


def _label(input, connectivity):
    t, back = load(input, "postprocessing", "label maps", plural=True)
    labels, _, summary, state = ops.cc_components(_as_object(t), None, connectivity, want_filtered=False)
    return labels, int(summary[0].item()), state, back


def label(input, connectivity=1):
    """scipy.ndimage.label(input, generate_binary_structure(input.ndim, connectivity)): (labels int32, num_features int).  Objects are numbered in
    raster order of their first cell, as scipy numbers them."""
    labels, n, _, back = _label(input, connectivity)
    return back(labels, torch.int32), n


def component_sizes(input, connectivity=1):
    """(labels int32, sizes int64 (num_features,)): sizes[k] is the cell count of object k + 1."""
    labels, n, state, back = _label(input, connectivity)
    sizes, _ = ops.cc_component_table(state, n)
    return back(labels, torch.int32), back(sizes, torch.int64)


def _min_count(min_size, volume_per_voxel):
    """The smallest count T with float64(T) * volume_per_voxel >= min_size: ``count < T`` is the reference's ``size < minimum`` exactly, because
    the rounded product does not decrease with the count."""
    m = float(min_size)
    if not m > 0.0:                       # (a NaN minimum: no size is below it)
        return 0
    q = m / volume_per_voxel
    if not q < _MAX_COUNT:
        return _MAX_COUNT                 # above every possible count but that of an object filling the largest map, which is the largest
    t = int(math.ceil(q))
    while t > 0 and np.float64(t - 1) * volume_per_voxel >= m:
        t -= 1
    while t < _MAX_COUNT and np.float64(t) * volume_per_voxel < m:
        t += 1
    return t


def _groups(entries):
    """Consecutive entries, greedily, as long as their id sets are pairwise disjoint and one pass takes them."""
    groups, used, n_ids = [[]], set(), 0
    for e in entries:
        ids = e[1]
        if len(ids) > L.DLKA_CC_IDS_MAX:
            raise RuntimeError(f"postprocessing: a joint region of at most {L.DLKA_CC_IDS_MAX} classes, got {len(ids)}")
        if groups[-1] and (used & set(ids) or len(groups[-1]) == L.DLKA_CC_K_MAX or n_ids + len(ids) > L.DLKA_CC_IDS_MAX):
            groups.append([])
            used, n_ids = set(), 0
        groups[-1].append(e)
        used |= set(ids)
        n_ids += len(ids)
    return groups


def remove_all_but_the_largest_connected_component(image, for_which_classes, volume_per_voxel, minimum_valid_object_size=None):
    """connected_components.py:48-105.  Returns (image, largest_removed, kept_size): per class or joint region (a list or tuple entry; its key is
    the tuple) every object of the largest size is kept, every other object is removed when ``minimum_valid_object_size`` is None or its size
    ``count * volume_per_voxel`` is below ``minimum_valid_object_size[c]``.  ``kept_size[c]``: the largest size, None when the entry has no cell;
    ``largest_removed[c]``: the largest removed size, or None.  Entries are applied in order as the reference applies them; only entries that
    share a class id need more than one pass.  ``image`` is not written to: the filtered map is a new array or tensor."""
    vpv = float(volume_per_voxel)
    if not (vpv > 0.0 and math.isfinite(vpv)):
        raise ValueError(f"postprocessing: volume_per_voxel must be positive and finite, got {volume_per_voxel}")
    t, back = load(image, "postprocessing", "label maps", plural=True)
    work = _as_classes(t)
    if for_which_classes is None:
        for_which_classes = [int(v) for v in torch.unique(work).cpu().tolist() if v > 0]
    if 0 in for_which_classes:
        raise AssertionError("cannot remove background")   # connected_components.py:64
    entries = []
    for c in for_which_classes:
        if isinstance(c, (list, tuple)):
            c = tuple(c)   # otherwise it cant be used as key in the dict (connected_components.py:69)
            ids = tuple(dict.fromkeys(int(v) for v in c))
        else:
            ids = (int(c),)
        entries.append((c, ids))
    largest_removed, kept_size = {}, {}
    current = work
    for group in _groups(entries) if entries else []:
        mins = None
        if minimum_valid_object_size is not None:
            mins = [_min_count(minimum_valid_object_size[key], vpv) for key, _ in group]
        _, current, summary, _ = ops.cc_components(current, [ids for _, ids in group], 1, mins)
        s = summary.cpu().tolist()
        for k, (key, _) in enumerate(group):
            biggest, removed = s[1 + k], s[1 + L.DLKA_CC_K_MAX + k]
            kept_size[key] = float(np.float64(biggest) * vpv) if biggest else None
            largest_removed[key] = float(np.float64(removed) * vpv) if removed else None
    if current is work:
        out = t.clone()
    elif work is t:
        out = current
    else:   # the kernels saw a converted map: take the removed cells out of the caller's own
        out = torch.where((current == 0) & (work != 0), torch.zeros_like(t), t)
    return back(out), largest_removed, kept_size
