"""The 2-D evaluator on the HIP kernels of ``csrc/cl_zoom2d.hip`` (include/dlka.h: ``dlka_zoom2d_*``): what the 2-D trainer runs at every
evaluation interval, slice by slice on one host core with ``scipy.ndimage.zoom``, batch-1 forwards and eight ``medpy`` calls per case.

  ``zoom``                 scipy.ndimage.zoom, same signature; rank 2, orders 0 / 1 / 3, the other arguments at their defaults
  ``zoom_slices``          the same for a stack (N, H, W) in a number of launches that does not depend on N, optionally with the float32
                           Normalize and a bfloat16 result fused into the store
  ``resize_sample``        the deterministic tail of Synapse_dataset.__getitem__ (2D/datasets/dataset_synapse.py:109-126) for a batch
  ``predict_volume``       the slice loop of test_single_volume (2D/utils.py:64-95): every slice zoomed in one pass, the net on chunks of
                           ``slice_batch`` slices, each chunk's logits straight into the argmax fused with the order-0 zoom back
  ``test_single_volume``   2D/utils.py:63-110, same name, argument order and defaults; every class scored in one batched pass (metrics.py)
  ``inference``            2D/trainer_MaxViT_deform_LKA.py:25-47

scipy.ndimage.zoom's rules: the output extent is ``int(round(n * zoom))``; scipy then recomputes the step from the two extents,
``(n - 1) / (m - 1)``, and output index k reads the coordinate ``k * step``; under mode 'constant' a coordinate < 0 or > n - 1 gives cval = 0 at
every order.  For some pairs of extents the last coordinate exceeds n - 1 by one ulp and the whole last row or column is 0: 512 -> 224 (the
Synapse default: the reference network is fed slices whose last row and column are zero), 32 -> 16, 28 -> 24; not 224 -> 512, 19 -> 16,
21 -> 24.  This module reproduces that.  Coordinates, taps and weights are formed here in float64, as scipy forms them, and handed to the kernels as
per-axis tables.

Inputs are numpy arrays or torch tensors on the host or the device; host data is moved to the device and results come back in the caller's
container (``predict_volume``: always a device tensor).  Arguments are never written to.  Without a GPU the calls raise as every operator of
the package does: there is no host fall-back."""
from __future__ import annotations

import functools
import logging

import numpy as np
import torch

from . import _lib as L
from . import metrics as M
from . import ops
from ._containers import cubic_bspline_weights, to_working_device

__all__ = ["zoom", "zoom_slices", "resize_sample", "predict_volume", "test_single_volume", "inference"]

_SPLINE_DTYPES = (torch.float32, torch.bfloat16, torch.int16)


# ---- containers ------------------------------------------------------------------------------------------------------------------------------
def _load(x, what):
    """(tensor on the working device, function that gives a result tensor the container and device the caller expects).  Not the shared
    ``load``: a result whose dtype the call changed keeps it, and bfloat16 has no way back to numpy."""
    t = to_working_device(x, "inference2d", what, "iuf")
    if isinstance(x, torch.Tensor):
        def back(r):
            return r.to(device=x.device)
    else:
        a_dtype = np.asarray(x).dtype

        def back(r):
            if r.dtype == torch.bfloat16:
                raise RuntimeError("inference2d: numpy has no bfloat16; pass a tensor")
            return r.cpu().numpy().astype(a_dtype, copy=False) if r.dtype == t.dtype else r.cpu().numpy()
    return t, back


# ---- tables: float64 on the host, as scipy.ndimage.zoom computes them --------------------------------------------------------------------------
@functools.lru_cache(maxsize=64)
def _axis_table(n, m, order):
    """Axis n -> m.  order 0: (source index or -1,); orders 1 / 3: (first tap or DLKA_ZOOM2D_OUTSIDE, weights (m, taps))."""
    if m < 2:
        raise NotImplementedError("inference2d: an output axis of length 1 (scipy takes another path for it)")
    step = float(n - 1) / float(m - 1)
    cc = np.arange(m, dtype=np.float64) * step
    outside = (cc < 0.0) | (cc > float(n - 1))
    if order == 0:
        return (np.where(outside, -1, np.floor(cc + 0.5).astype(np.int64)),)
    lo = np.floor(cc)
    y = cc - lo
    if order == 1:
        w = np.stack([1.0 - y, y], 1)
        first = lo.astype(np.int64)
    else:
        w = cubic_bspline_weights(y)
        first = lo.astype(np.int64) - 1
    return np.where(outside, L.DLKA_ZOOM2D_OUTSIDE, first), w


def _identity_spline_tables(hw, device):
    """Two taps that return the value itself: what carries Normalize / the bfloat16 store when there is nothing to zoom."""
    starts = [np.arange(n, dtype=np.int64) for n in hw]
    weights = [np.stack([np.ones(n), np.zeros(n)], 1) for n in hw]
    return ops.zoom2d_spline_tables(starts, weights, hw, 2, device)


def _index_tables(in_hw, out_hw, device):
    return ops.zoom2d_index_tables([_axis_table(int(in_hw[ax]), int(out_hw[ax]), 0)[0] for ax in range(2)], in_hw, device)


def _output_size(shape, factors):
    return tuple(int(round(n * f)) for n, f in zip(shape, factors))


def _check_order(order):
    if order not in (0, 1, 3) or isinstance(order, bool):
        raise NotImplementedError(f"inference2d: order={order!r} (supported: 0, 1, 3)")


def _zoom_stack(t, out_hw, order, mean, std, dtype):
    """``t`` (N, H, W) on the working device -> (N, *out_hw)."""
    _check_order(order)
    out_hw = tuple(int(v) for v in out_hw)
    if len(out_hw) != 2:
        raise RuntimeError(f"inference2d: output_size is (rows, columns), got {out_hw}")
    if (mean is None) != (std is None):
        raise RuntimeError("inference2d: mean and std come together")
    dtype = t.dtype if dtype is None else dtype
    plain = mean is None and dtype == t.dtype
    if not plain and (t.dtype not in (torch.float32, torch.bfloat16) or dtype not in (torch.float32, torch.bfloat16)
                      or (t.dtype == torch.bfloat16 and dtype == torch.float32)):
        raise NotImplementedError(f"inference2d: mean / std / dtype={dtype} with {t.dtype} slices (float32 -> float32 / bfloat16, bfloat16 -> bfloat16)")
    in_hw = tuple(t.shape[1:])
    if in_hw == out_hw:
        if plain:
            return t.clone()                                  # the reference skips the call: the values, untouched
        start, w4 = _identity_spline_tables(in_hw, t.device)
        return ops.zoom2d_spline(t, out_hw, start, w4, 2, dtype, mean, std)
    if order == 0:
        if not plain:
            raise NotImplementedError("inference2d: mean / std / dtype with order=0")
        return ops.zoom2d_nearest(t, out_hw, _index_tables(in_hw, out_hw, t.device))
    if t.dtype not in _SPLINE_DTYPES:
        raise NotImplementedError(f"inference2d: orders 1 and 3 take float32, bfloat16 or int16 input, got {t.dtype}")
    tables = [_axis_table(in_hw[ax], out_hw[ax], order) for ax in range(2)]
    taps = 2 if order == 1 else 4
    start, w4 = ops.zoom2d_spline_tables([tb[0] for tb in tables], [tb[1] for tb in tables], in_hw, taps, t.device)
    src = t if order == 1 else ops.zoom2d_coefficients(t)
    return ops.zoom2d_spline(src, out_hw, start, w4, taps, dtype, mean, std)


# ---- scipy.ndimage.zoom --------------------------------------------------------------------------------------------------------------------------
def zoom(input, zoom, output=None, order=3, mode='constant', cval=0.0, prefilter=True, *, grid_mode=False):   # noqa: A002
    """scipy.ndimage.zoom for a rank-2 array at orders 0, 1 and 3; the result has the input's dtype and container."""
    for name, value, default in (("output", output, None), ("mode", mode, "constant"), ("cval", cval, 0.0), ("prefilter", prefilter, True),
                                 ("grid_mode", grid_mode, False)):
        if value is not default and value != default:
            raise NotImplementedError(f"inference2d.zoom: {name}={value!r} (only the default {default!r})")
    _check_order(order)
    t, back = _load(input, "input")
    if t.ndim != 2:
        raise NotImplementedError(f"inference2d.zoom: input of rank {t.ndim} (rank 2 only)")
    factors = [float(zoom)] * 2 if np.isscalar(zoom) else [float(z) for z in zoom]
    if len(factors) != 2:
        raise RuntimeError("inference2d.zoom: one zoom factor per axis")
    return back(_zoom_stack(t[None], _output_size(t.shape, factors), order, None, None, None)[0])


def zoom_slices(x, output_size, order=3, mean=None, std=None, dtype=None):
    """Every slice of ``x`` (N, H, W) through ``zoom`` to ``output_size``; the launch count does not depend on N.  ``mean`` / ``std``: the
    float32 result goes through ``(v - mean) / std`` in float32 (torchvision's Normalize); ``dtype=torch.bfloat16``: rounded once more.  An
    ``output_size`` equal to the input's returns the values untouched (the reference skips the call)."""
    t, back = _load(x, "x")
    if t.ndim != 3:
        raise RuntimeError(f"inference2d.zoom_slices: x is (N, H, W), got {tuple(t.shape)}")
    return back(_zoom_stack(t, output_size, order, mean, std, dtype))


def resize_sample(image, label, img_size, mean=0.5, std=0.5):
    """dataset_synapse.py:109-126 for a batch: image (B, H, W) zoomed at order 3 and label (B, H, W) at order 0 to ``img_size`` when the slice
    has another size, then ToTensor and Normalize([mean], [std]) for the image and ToTensor for the label:
    ``{'image': (B, 1, S, S) float32, 'label': (B, 1, S, S)}`` in the label's dtype."""
    size = (int(img_size),) * 2 if np.isscalar(img_size) else tuple(int(v) for v in img_size)
    ti, back_i = _load(image, "image")
    tl, back_l = _load(label, "label")
    if ti.ndim != 3 or tuple(tl.shape) != tuple(ti.shape):
        raise RuntimeError(f"inference2d.resize_sample: image and label are (B, H, W), got {tuple(ti.shape)} and {tuple(tl.shape)}")
    if ti.dtype != torch.float32:
        raise NotImplementedError(f"inference2d.resize_sample: a float32 image, got {ti.dtype}")
    # (the reference compares both extents with img_size and zooms both arrays or neither)
    img = _zoom_stack(ti, size, 3, mean, std, None)
    lab = _zoom_stack(tl, size, 0, None, None, None)
    return {"image": back_i(img[:, None]), "label": back_l(lab[:, None])}


# ---- test_single_volume ----------------------------------------------------------------------------------------------------------------------------
def _labels_of(logits, n, out_hw, idx, out=None, patch=None):
    """The logits of one chunk through the argmax fused with the order-0 zoom back."""
    if not isinstance(logits, torch.Tensor) or logits.ndim != 4 or logits.shape[0] != n:
        raise RuntimeError("inference2d: the net returns logits (n, classes, h, w)")
    if patch is not None and tuple(logits.shape[2:]) != patch:
        raise RuntimeError(f"inference2d: logits of extents {tuple(logits.shape[2:])} for patches of {patch}")
    if logits.dtype not in (torch.float32, torch.bfloat16):
        logits = logits.float()
    return ops.zoom2d_argmax(logits, out_hw, idx, out)


def predict_volume(image, net, patch_size, slice_batch=24, mean=0.5, std=0.5):
    """The prediction of test_single_volume (2D/utils.py:64-95) as a uint8 label map on the device.  ``image``: (S, x, y), every slice zoomed
    to ``patch_size`` at order 3 (when its size differs) and normalised in one pass, the net in ``eval()`` under ``no_grad`` on chunks of
    ``slice_batch`` slices, each chunk's logits reduced by the argmax fused with the order-0 zoom back to (x, y); or (x, y), the reference's
    2-D branch: no zoom and no Normalize.  The net's training flag is restored on return (the reference leaves the net in ``eval()``)."""
    t, _ = _load(image, "image")
    if t.ndim not in (2, 3) or t.numel() == 0:
        raise RuntimeError(f"inference2d.predict_volume: image is (S, x, y) or (x, y), got {tuple(t.shape)}")
    patch = tuple(int(v) for v in patch_size)
    slice_batch = int(slice_batch)
    if len(patch) != 2 or slice_batch < 1:
        raise RuntimeError("inference2d.predict_volume: patch_size is (rows, columns) and slice_batch >= 1")
    was_training = getattr(net, "training", None)
    if was_training is not None:
        net.eval()
    try:
        with torch.no_grad():
            if t.ndim == 2:
                logits = net(t[None, None].float())
                hw = tuple(logits.shape[2:]) if isinstance(logits, torch.Tensor) and logits.ndim == 4 else tuple(t.shape)
                idx = ops.zoom2d_index_tables([np.arange(n) for n in hw], hw, t.device)
                return _labels_of(logits, 1, hw, idx)[0]
            xy = tuple(t.shape[1:])
            if xy != patch and _output_size(patch, (xy[0] / patch[0], xy[1] / patch[1])) != xy:
                raise NotImplementedError(f"inference2d.predict_volume: zooming {patch} back does not give {xy}")
            inp = _zoom_stack(t.float(), patch, 3, mean, std, None)
            idx = (ops.zoom2d_index_tables([np.arange(n) for n in xy], xy, t.device) if xy == patch else _index_tables(patch, xy, t.device))
            out = torch.empty((t.shape[0],) + xy, dtype=torch.uint8, device=t.device)
            for s0 in range(0, t.shape[0], slice_batch):
                chunk = inp[s0:s0 + slice_batch, None]
                _labels_of(net(chunk), chunk.shape[0], xy, idx, out[s0:s0 + slice_batch], patch)
            return out
    finally:
        if was_training:
            net.train(True)


# NOTE for tests: pytest collects any module-level name that starts with ``test`` in a test module, so a test file must import this MODULE
# (``from deformablelka_amd import inference2d as I2``) and never this name.
def test_single_volume(image, label, net, classes, patch_size=[256, 256], test_save_path=None, case=None, z_spacing=1,   # noqa: B006
                       slice_batch=24, return_prediction=False):
    """2D/utils.py:63-110.  ``image`` and ``label`` carry the loader's leading batch axis of 1.  Returns the reference's list of (dice, hd95)
    per class 1 .. classes - 1 under calculate_metric_percase's convention: (1, 0) when only the label lacks the class, (0, 0) when the
    prediction does; with ``return_prediction`` also the label map, in the label's dtype and container."""
    if test_save_path is not None:
        raise NotImplementedError("inference2d.test_single_volume: test_save_path (writing NIfTI files needs SimpleITK and is out of scope)")
    img = image.detach() if isinstance(image, torch.Tensor) else np.asarray(image)
    lab, back = _load(label, "label")
    if img.shape[0] != 1 or lab.shape[0] != 1:
        raise RuntimeError("inference2d.test_single_volume: image and label carry a leading batch axis of 1")
    prediction = predict_volume(img[0], net, patch_size, slice_batch)
    lab = lab[0]
    if tuple(prediction.shape) != tuple(lab.shape):
        raise RuntimeError(f"inference2d.test_single_volume: a prediction of {tuple(prediction.shape)} for a label of {tuple(lab.shape)}")
    entries = M._measure(M._as_labels(prediction), M._as_labels(lab), list(range(1, int(classes))), None, 1)
    rows = iter(M._summaries(entries))                        # one device -> host read for all classes
    metric_list = []
    for e in entries:
        if e["a"] > 0 and e["b"] > 0:
            metric_list.append((2.0 * e["inter"] / float(e["a"] + e["b"]), M._finish(next(rows))["hd95"]))
        elif e["a"] > 0:
            metric_list.append((1, 0))
        else:
            metric_list.append((0, 0))
    if return_prediction:
        return metric_list, back(prediction.to(lab.dtype))
    return metric_list


def inference(model, testloader, args, test_save_path=None):
    """2D/trainer_MaxViT_deform_LKA.py:25-47: the mean over the cases of ``testloader`` (batches of one case: 'image', 'label', 'case_name'),
    logged per case and per class; returns (mean dice, mean hd95).  Reads ``args.num_classes``, ``args.img_size`` and ``args.z_spacing``."""
    was_training = getattr(model, "training", None)
    if was_training is not None:
        model.eval()
    try:
        total, cases = None, 0
        for i, batch in enumerate(testloader):
            name = batch["case_name"][0]
            scores = np.asarray(test_single_volume(batch["image"], batch["label"], model, classes=args.num_classes,
                                                   patch_size=[args.img_size, args.img_size], test_save_path=test_save_path, case=name,
                                                   z_spacing=args.z_spacing), dtype=np.float64)
            total = scores if total is None else total + scores
            cases += 1
            logging.info(" idx %d case %s mean_dice %f mean_hd95 %f", i, name, scores[:, 0].mean(), scores[:, 1].mean())
        n_cases = len(testloader.dataset) if hasattr(testloader, "dataset") else cases          # (the reference divides by the dataset's length)
        per_class = total / n_cases
        for c in range(1, args.num_classes):
            logging.info("Mean class %d mean_dice %f mean_hd95 %f", c, per_class[c - 1, 0], per_class[c - 1, 1])
        performance, mean_hd95 = per_class[:, 0].mean(), per_class[:, 1].mean()
        logging.info("Testing performance in best val model: mean_dice : %f mean_hd95 : %f", performance, mean_hd95)
        return performance, mean_hd95
    finally:
        if was_training:
            model.train(True)
