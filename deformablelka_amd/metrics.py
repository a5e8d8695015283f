"""The evaluators' metrics on the HIP kernels of ``csrc/cl_surface_dist.hip`` (include/dlka.h: ``dlka_sd_*``): what the reference computes with
``medpy.metric.binary`` (MedPy 0.4.0, pinned in both requirements.txt) on one CPU core per organ.

  ``dc``, ``hd``, ``hd95``, ``asd``, ``assd``   medpy.metric.binary, same signatures, semantics and errors
  ``calculate_metric_percase``               2D/utils.py:50-60
  ``evaluate_label_maps``                    the per-organ loops of 2D/utils.py:96-98 and 3D/d_lka_former/inference_synapse.py:11-21, 65-88, and
                                             nnU-Net's conventions (3D/d_lka_former/evaluation/metrics.py:105-120, :332-347), every class in one
                                             batched pass over the two label maps

Inputs are numpy arrays or torch tensors, on the host or the device; host data is moved to the device.  Results are Python floats and numpy
arrays.  One call reads the device twice: the per-class counts and bounding boxes (they size the transform), then the results.  The kernels
return exact squared distances; the order statistics (``torch.sort``) and sums run on the device, the square roots of the returned order
statistics on the host in IEEE float64.  Without a GPU the calls raise as every operator of the package does: there is no host fall-back."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib as L
from . import ops
from ._containers import to_working_device

__all__ = ["dc", "hd", "hd95", "asd", "assd", "surface_metrics", "surface_distances", "calculate_metric_percase", "evaluate_label_maps"]


def _as_tensor(x):
    return to_working_device(x, "metrics", "input", kinds=None)   # medpy takes whatever numpy.asarray takes: no dtype refusal here


def _as_mask(x):
    """medpy's ``astype(bool)``: nonzero, as uint8."""
    t = _as_tensor(x)
    return t if t.dtype in (torch.bool, torch.uint8) else (t != 0).to(torch.uint8)


def _as_labels(x):
    """Rule of this module: a floating value that is no integer becomes -1, which is no class (postprocessing maps it to 0, resampling
    raises): keep the three apart."""
    t = _as_tensor(x)
    if t.is_floating_point():
        t = torch.where(t == t.round(), t, torch.full_like(t, -1)).to(torch.int64)
    elif t.dtype == torch.int8:
        t = t.to(torch.int16)
    return t


def _spacing(voxelspacing, rank):
    if voxelspacing is None:
        return None
    if np.isscalar(voxelspacing):
        return [float(voxelspacing)] * rank
    return [float(s) for s in voxelspacing]


def _measure(p, q, class_ids, voxelspacing, connectivity, distances=True):
    """Per class: counts (inter, |a|, |b|, full size) and, where both masks exist, the device-side summary of the two directed distance sets."""
    spacing = _spacing(voxelspacing, p.ndim)
    ids = [0] if class_ids is None else [int(c) for c in class_ids]
    out = []
    for k0 in range(0, len(ids), L.DLKA_SD_K_MAX):
        chunk = None if class_ids is None else ids[k0:k0 + L.DLKA_SD_K_MAX]
        stats, d, pp, qq = ops.sd_label_stats(p, q, chunk, spacing, connectivity)
        st = stats.cpu().numpy()
        boxes = []
        for k in range(d.K):
            live = distances and st[k, 1] > 0 and st[k, 2] > 0
            boxes.append(list(st[k, 3:6]) + list(st[k, 6:9] - st[k, 3:6] + 1) if live else [0] * 6)
        sq, offsets = ops.sd_distances(pp, qq, d, boxes) if distances else (None, None)
        for k in range(d.K):
            n = int(boxes[k][3] * boxes[k][4] * boxes[k][5])
            seg = sq[offsets[k]:offsets[k] + 2 * n] if n else None
            out.append({"inter": int(st[k, 0]), "a": int(st[k, 1]), "b": int(st[k, 2]), "cells": int(pp.numel()), "n": n, "sq": seg})
    return out


def _summaries(entries):
    """One device -> host read for all classes: per class (count ab, count ba, sum ab, sum ba, sq at floor(0.95 (n - 1)), sq at that + 1,
    the interpolation weight, the largest sq)."""
    rows = []
    for e in entries:
        if e["sq"] is None:
            continue
        both, n = e["sq"], e["n"]
        on = both >= 0
        cnt = torch.stack((on[:n].sum(), on[n:].sum()))
        root = torch.where(on, both.clamp_min(0).sqrt(), torch.zeros_like(both))
        sums = torch.stack((root[:n].sum(), root[n:].sum()))
        srt = torch.sort(torch.where(on, both, torch.full_like(both, math.inf))).values
        tot = cnt.sum()
        v = 0.95 * (tot - 1).to(torch.float64)   # numpy.percentile, method 'linear'
        lo = v.floor().to(torch.int64)
        hi = torch.minimum(lo + 1, tot - 1)
        rows.append(torch.stack((cnt[0].double(), cnt[1].double(), sums[0], sums[1], srt[lo], srt[hi], v - lo.double(), srt[tot - 1])))
    if not rows:
        return []
    return torch.stack(rows).cpu().numpy().tolist()


def _finish(row):
    c0, c1, s0, s1, a2, b2, g, m2 = row
    a, b = math.sqrt(a2), math.sqrt(b2)
    p95 = a + (b - a) * g if g < 0.5 else b - (b - a) * (1.0 - g)   # (numpy's _lerp)
    return {"hd": math.sqrt(m2), "hd95": p95, "asd": s0 / c0, "asd_rev": s1 / c1}


def _pair(result, reference, voxelspacing, connectivity):
    p, q = _as_mask(result), _as_mask(reference)
    e = _measure(p, q, None, voxelspacing, connectivity)[0]
    if e["a"] == 0:
        raise RuntimeError("The first supplied array does not contain any binary object.")
    if e["b"] == 0:
        raise RuntimeError("The second supplied array does not contain any binary object.")
    return e


def dc(result, reference):
    """medpy.metric.binary.dc: 2 |a & b| / (|a| + |b|); two empty masks give 0.0."""
    e = _measure(_as_mask(result), _as_mask(reference), None, None, 1, distances=False)[0]
    return 2.0 * e["inter"] / float(e["a"] + e["b"]) if e["a"] + e["b"] else 0.0


def surface_distances(result, reference, voxelspacing=None, connectivity=1):
    """medpy's ``__surface_distances``: the distance of every border cell of ``result`` to the nearest border cell of ``reference``, in the
    array order of the cells (float64 numpy)."""
    e = _pair(result, reference, voxelspacing, connectivity)
    sq = e["sq"][:e["n"]].cpu().numpy()
    return np.sqrt(sq[sq >= 0])


def surface_metrics(result, reference, voxelspacing=None, connectivity=1):
    """{"hd", "hd95", "asd", "assd"} of one pair from one pass (the four functions below each run it)."""
    f = _finish(_summaries([_pair(result, reference, voxelspacing, connectivity)])[0])
    return {"hd": f["hd"], "hd95": f["hd95"], "asd": f["asd"], "assd": float(np.mean((f["asd"], f["asd_rev"])))}


def hd(result, reference, voxelspacing=None, connectivity=1):
    return surface_metrics(result, reference, voxelspacing, connectivity)["hd"]


def hd95(result, reference, voxelspacing=None, connectivity=1):
    return surface_metrics(result, reference, voxelspacing, connectivity)["hd95"]


def asd(result, reference, voxelspacing=None, connectivity=1):
    return surface_metrics(result, reference, voxelspacing, connectivity)["asd"]


def assd(result, reference, voxelspacing=None, connectivity=1):
    return surface_metrics(result, reference, voxelspacing, connectivity)["assd"]


def calculate_metric_percase(pred, gt):
    """2D/utils.py:50-60 on masks ``> 0``: (dice, hd95); (1, 0) when only ``gt`` is empty; (0, 0) when ``pred`` is.  The arguments are not
    written to (the reference binarises them in place)."""
    p, g = (_as_tensor(pred) > 0).to(torch.uint8), (_as_tensor(gt) > 0).to(torch.uint8)
    e = _measure(p, g, None, None, 1)[0]
    if e["a"] > 0 and e["b"] > 0:
        return 2.0 * e["inter"] / float(e["a"] + e["b"]), _finish(_summaries([e])[0])["hd95"]
    if e["a"] > 0 and e["b"] == 0:
        return 1, 0
    return 0, 0


def evaluate_label_maps(prediction, label, class_ids, voxelspacing=None, connectivity=1, nan_for_nonexisting=False):
    """{"dice": (K,), "hd95": (K,)} float64 for ``prediction == c`` against ``label == c``, every c of ``class_ids`` in one batched pass.
    Default, inference_synapse.py:11-21: dice 1 when both masks are empty, hd95 0 when either is.  ``nan_for_nonexisting``, nnU-Net's
    metrics.py:105-120 and :332-347: dice NaN when both are empty, hd95 NaN when either is empty or fills the map."""
    p, q = _as_labels(prediction), _as_labels(label)
    entries = _measure(p, q, list(class_ids), voxelspacing, connectivity)
    rows = iter(_summaries(entries))
    dice, h95 = [], []
    for e in entries:
        f = _finish(next(rows)) if e["sq"] is not None else None
        if e["a"] + e["b"] == 0:
            dice.append(math.nan if nan_for_nonexisting else 1.0)
        else:
            dice.append(2.0 * e["inter"] / float(e["a"] + e["b"]))
        if f is None:
            h95.append(math.nan if nan_for_nonexisting else 0.0)
        elif nan_for_nonexisting and (e["a"] == e["cells"] or e["b"] == e["cells"]):
            h95.append(math.nan)
        else:
            h95.append(f["hd95"])
    return {"dice": np.asarray(dice, dtype=np.float64), "hd95": np.asarray(h95, dtype=np.float64)}
