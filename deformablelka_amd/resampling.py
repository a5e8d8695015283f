"""The reference's resampling between a case's own grid and the network's grid on the HIP kernels of ``csrc/cl_resample.hip`` (include/dlka.h:
``dlka_resample_*``): what ``resample_data_or_seg`` (3D/d_lka_former/preprocessing/preprocessing.py:112-201) computes in float64 on one CPU
core, channel by channel and slice by slice, for ``save_segmentation_nifti_from_softmax`` (inference/segmentation_export.py:73-137; both
trainers' ``validate()`` and inference/predict.py) and for ``resample_patient`` (preprocessing.py:38-109).

  ``get_do_separate_z``, ``get_lowres_axis``, ``resample_patient``, ``resample_data_or_seg``   preprocessing.py:28-201, same names, arguments, defaults
  ``resample_and_argmax``          the resampling of the class probabilities and the argmax (or the region rule) of segmentation_export.py:104-125
                                   in ONE kernel: the C x D x H x W resampled probabilities are never stored
  ``segmentation_from_softmax``    segmentation_export.py:73-137 without the file writing: the label map in the case's original extents

skimage's ``resize(mode='edge', anti_aliasing=False)`` and batchgenerators' ``resize_segmentation`` are restated through
``scipy.ndimage.map_coordinates(mode='nearest')`` at the source coordinates ``(i + 0.5) * n_in / n_out - 0.5`` (what
``scipy.ndimage.zoom(grid_mode=True, mode='nearest')`` returns; the reference's own z step, :163-178, is this map).  The coordinates, source
cells and weights of every axis are computed here in float64, as scipy computes them, and handed to the kernels as tables.

Inputs are numpy arrays or torch tensors, on the host or the device; host data is moved to the device.  A tensor in gives a tensor out on the
same device, numpy in gives numpy out.  The arguments are NOT written to (the reference edits ``properties_dict['crop_bbox']`` in place).
Without a GPU the calls raise as every operator of the package does: there is no host fall-back."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from . import ops
from ._containers import cubic_bspline_weights, load

__all__ = ["RESAMPLING_SEPARATE_Z_ANISO_THRESHOLD", "get_do_separate_z", "get_lowres_axis", "resample_patient", "resample_data_or_seg",
           "resample_and_argmax", "segmentation_from_softmax"]

RESAMPLING_SEPARATE_Z_ANISO_THRESHOLD = 3   # d_lka_former/configuration.py:4


def get_do_separate_z(spacing, anisotropy_threshold=RESAMPLING_SEPARATE_Z_ANISO_THRESHOLD):
    """preprocessing.py:28-30."""
    return (np.max(spacing) / np.min(spacing)) > anisotropy_threshold


def get_lowres_axis(new_spacing):
    """preprocessing.py:33-35: the axes whose spacing is the largest."""
    return np.where(max(new_spacing) / np.array(new_spacing) == 1)[0]


# ---- tables: float64 on the host, as scipy.ndimage computes them ----------------------------------------------------------------------------
def _coordinates(n_in, n_out):
    return (np.arange(n_out, dtype=np.float64) + 0.5) * (float(n_in) / n_out) - 0.5


def _linear_table(n_in, n_out, order):
    """order 0: the cell floor(c + 0.5); order 1: cells floor(c), floor(c) + 1 with weights 1 - f, f.  Cells outside the array are the edge
    cells (mode 'edge' / 'nearest'); scipy keeps the weights of the unclamped coordinate and so does this, to the last bit."""
    c = _coordinates(n_in, n_out)
    if order == 0:
        return np.clip(np.floor(c + 0.5), 0, n_in - 1).astype(np.int64)[:, None], np.ones((n_out, 1))
    lo = np.floor(c)
    f = c - lo
    lo = lo.astype(np.int64)
    return np.stack([np.clip(lo, 0, n_in - 1), np.clip(lo + 1, 0, n_in - 1)], 1), np.stack([1.0 - f, f], 1)


def _cubic_table(n_in, n_out):
    """First of the four cells in the array padded by DLKA_RESAMPLE_SPLINE_PAD, and the cubic B-spline weights."""
    c = _coordinates(n_in, n_out) + float(L.DLKA_RESAMPLE_SPLINE_PAD)
    lo = np.floor(c)
    return lo.astype(np.int64) - 1, cubic_bspline_weights(c - lo)


def _identity_table(n, width):
    w = np.zeros((n, 1))
    w[:, 0] = 1.0
    return (np.arange(n, dtype=np.int64)[:, None] if width == 2 else np.arange(n, dtype=np.int64)), w


def _check_orders(order, order_z, is_seg, do_separate_z):
    allowed = (0, 1) if is_seg else (0, 1, 3)
    if order not in allowed:
        raise NotImplementedError(f"resampling: order={order!r} (is_seg={bool(is_seg)} supports {allowed})")
    if do_separate_z and order_z not in (0, 1):
        raise NotImplementedError(f"resampling: order_z={order_z!r} (supported: 0, 1)")


def _axis_orders(order, order_z, do_separate_z, axis):
    """The order along each of the three axes, and the separate axis or None."""
    if not do_separate_z:
        return [order] * 3, None
    assert axis is not None and len(axis) == 1, "only one anisotropic axis supported"   # preprocessing.py:139
    ax = int(axis[0])
    orders = [order] * 3
    orders[ax] = order_z
    return orders, ax


def _linear_tables(shape, new_shape, orders):
    return [_linear_table(shape[a], new_shape[a], orders[a]) for a in range(3)]


def _promote(tables):
    """Two taps on every axis but the first when all of them could do with one or two: the argmax kernel's two fixed patterns."""
    out = []
    for a, (c, w) in enumerate(tables):
        if a > 0 and w.shape[1] == 1:
            c, w = np.concatenate([c, c], 1), np.concatenate([w, np.zeros_like(w)], 1)
        out.append((c, w))
    return out


# ---- the three value paths ---------------------------------------------------------------------------------------------------------------------
def _compute_dtype(t):
    return t if t.dtype in (torch.float32, torch.float64) else t.to(torch.float32 if t.dtype in (torch.float16, torch.bfloat16) else torch.float64)


def _resample_values(t, new_shape, orders, sep_axis):
    """is_seg=False: (c, x', y', z') in float32 (float32, float16, bfloat16 in) or float64 (float64 and integers in)."""
    shape = tuple(t.shape[1:])
    x = _compute_dtype(t)
    cubic = [a for a in range(3) if orders[a] == 3]
    if not cubic:
        return ops.resample_linear(x, new_shape, _linear_tables(shape, new_shape, orders))
    # order 3 (in-plane when an axis is separate): float64, one channel at a time; the separate axis keeps its extent here and is resampled after
    mid = tuple(shape[a] if a == sep_axis else new_shape[a] for a in range(3))
    tables = [_cubic_table(shape[a], mid[a]) if a in cubic else _identity_table(shape[a], 4) for a in range(3)]
    pad = [L.DLKA_RESAMPLE_SPLINE_PAD if a in cubic else 0 for a in range(3)]
    out = torch.empty((x.shape[0],) + mid, dtype=torch.float64, device=x.device)
    for c in range(x.shape[0]):
        if sep_axis is None:     # resize clips to the range of its own input: the channel, or the slice
            lo, hi = x[c].amin().to(torch.float64).reshape(1), x[c].amax().to(torch.float64).reshape(1)
        else:
            dims = [a for a in range(3) if a != sep_axis]
            lo, hi = x[c].amin(dims).to(torch.float64), x[c].amax(dims).to(torch.float64)
        out[c] = ops.resample_spline(x[c], mid, tables, pad, lo, hi, -1 if sep_axis is None else sep_axis)
    if mid != tuple(new_shape):
        z_orders = [0] * 3
        z_orders[sep_axis] = orders[sep_axis]
        out = ops.resample_linear(out, new_shape, _linear_tables(mid, new_shape, z_orders))
    return out


def _as_labels(t):
    # rule of this module: a floating value that is no integer is an error (metrics maps it to -1, postprocessing to 0): keep the three apart
    if t.is_floating_point():
        if not bool((t == t.round()).all()):
            raise NotImplementedError("resampling: is_seg=True takes integer-valued label maps")
    elif t.dtype not in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64, torch.bool):
        raise RuntimeError(f"resampling: label maps are integer, bool or floating, got {t.dtype}")
    if t.numel() and (int(t.min()) < -2 ** 31 or int(t.max()) >= 2 ** 31):
        raise NotImplementedError("resampling: labels beyond 32 bits")
    return t.to(torch.int32)


def _resample_labels(t, new_shape, orders, sep_axis):
    """is_seg=True: int32 (c, x', y', z')."""
    shape = tuple(t.shape[1:])
    seg = _as_labels(t)
    if sep_axis is None or orders[sep_axis] == 0 or shape[sep_axis] == new_shape[sep_axis]:
        return ops.resample_labels(seg, new_shape, _linear_tables(shape, new_shape, orders))
    # preprocessing.py:149-188: the slices first (">= 0.5"), then the labels of that result along the separate axis ("round(.) > 0.5")
    mid = tuple(shape[a] if a == sep_axis else new_shape[a] for a in range(3))
    in_plane = [0 if a == sep_axis else orders[a] for a in range(3)]
    z_orders = [orders[a] if a == sep_axis else 0 for a in range(3)]
    seg = ops.resample_labels(seg, mid, _linear_tables(shape, mid, in_plane))
    return ops.resample_labels(seg, new_shape, _linear_tables(mid, new_shape, z_orders), strict=True)


# ---- public ---------------------------------------------------------------------------------------------------------------------------------
def _new_shape(new_shape):
    new_shape = tuple(int(v) for v in np.asarray(new_shape).reshape(-1))
    if len(new_shape) != 3 or min(new_shape) < 1:
        raise ValueError(f"resampling: new_shape must be three positive extents, got {new_shape}")
    return new_shape


def resample_data_or_seg(data, new_shape, is_seg, axis=None, order=3, do_separate_z=False, cval=0, order_z=0):
    """preprocessing.py:112-201.  ``data`` is (c, x, y, z); the result has the dtype of ``data`` (the reference's ``astype``: integers are
    truncated).  is_seg=False: order 0, 1 or 3; is_seg=True: order 0 or 1; order_z 0 or 1; anything else raises NotImplementedError.  ``cval``
    is accepted and, with edge mode, never used.  When the shapes agree nothing is resampled."""
    assert len(data.shape) == 4, "data must be (c, x, y, z)"
    _check_orders(order, order_z, is_seg, do_separate_z)
    new_shape = _new_shape(new_shape)
    t, back = load(data, "resampling", "data")
    if tuple(t.shape[1:]) == new_shape:
        return back(t)
    orders, sep_axis = _axis_orders(order, order_z, do_separate_z, axis)
    out = _resample_labels(t, new_shape, orders, sep_axis) if is_seg else _resample_values(t, new_shape, orders, sep_axis)
    if t.dtype == torch.bool:
        out = out != 0
    return back(out)


def resample_patient(data, seg, original_spacing, target_spacing, order_data=3, order_seg=0, force_separate_z=False, cval_data=0, cval_seg=-1,
                     order_z_data=0, order_z_seg=0, separate_z_anisotropy_threshold=RESAMPLING_SEPARATE_Z_ANISO_THRESHOLD):
    """preprocessing.py:38-109: (data, seg) at ``target_spacing``; either may be None."""
    assert not ((data is None) and (seg is None))
    if data is not None:
        assert len(data.shape) == 4, "data must be c x y z"
    if seg is not None:
        assert len(seg.shape) == 4, "seg must be c x y z"
    shape = np.array(tuple((data if data is not None else seg).shape[1:]))
    new_shape = np.round(((np.array(original_spacing) / np.array(target_spacing)).astype(float) * shape)).astype(int)
    if force_separate_z is not None:
        do_separate_z = force_separate_z
        axis = get_lowres_axis(original_spacing) if force_separate_z else None
    elif get_do_separate_z(original_spacing, separate_z_anisotropy_threshold):
        do_separate_z, axis = True, get_lowres_axis(original_spacing)
    elif get_do_separate_z(target_spacing, separate_z_anisotropy_threshold):
        do_separate_z, axis = True, get_lowres_axis(target_spacing)
    else:
        do_separate_z, axis = False, None
    if axis is not None and len(axis) != 1:    # every axis, or two of them (spacings like (0.24, 1.25, 1.25)), have the largest spacing
        do_separate_z = False
    data_reshaped = seg_reshaped = None
    if data is not None:
        data_reshaped = resample_data_or_seg(data, new_shape, False, axis, order_data, do_separate_z, cval=cval_data, order_z=order_z_data)
    if seg is not None:
        seg_reshaped = resample_data_or_seg(seg, new_shape, True, axis, order_seg, do_separate_z, cval=cval_seg, order_z=order_z_seg)
    return data_reshaped, seg_reshaped


def _argmax(t, new_shape, axis, order, do_separate_z, order_z, regions_class_order):
    if order not in (0, 1):
        raise NotImplementedError(f"resampling: order={order!r} (resample_and_argmax supports 0, 1)")
    _check_orders(order, order_z, False, do_separate_z)
    if regions_class_order is not None:
        regions_class_order = [int(c) for c in regions_class_order]
        if len(regions_class_order) != t.shape[0] or not all(0 <= c < 256 for c in regions_class_order):
            raise ValueError(f"resampling: one region value in 0..255 per channel ({t.shape[0]}), got {regions_class_order}")
    orders, _ = _axis_orders(order, order_z, do_separate_z, axis)
    tables = _promote(_linear_tables(tuple(t.shape[1:]), new_shape, orders))
    return ops.resample_argmax(_compute_dtype(t), new_shape, tables, regions_class_order)


def resample_and_argmax(probabilities, new_shape, axis=None, order=1, do_separate_z=False, order_z=0, regions_class_order=None):
    """``resample_data_or_seg(probabilities, new_shape, False, axis, order, do_separate_z, 0, order_z)`` followed by ``argmax(0)`` — or, with
    ``regions_class_order``, by the region rule of segmentation_export.py:119-125 (later entries overwrite earlier ones where the resampled
    channel is > 0.5) — as ONE kernel that keeps the running maximum in registers: uint8 (x', y', z').  Ties go to the first maximum, as in
    numpy.  order and order_z: 0 or 1."""
    assert len(probabilities.shape) == 4, "data must be (c, x, y, z)"
    t, _ = load(probabilities, "resampling", "probabilities")
    seg = _argmax(t, _new_shape(new_shape), axis, order, do_separate_z, order_z, regions_class_order)
    return seg.to(probabilities.device) if isinstance(probabilities, torch.Tensor) else seg.cpu().numpy()


def segmentation_from_softmax(segmentation_softmax, properties_dict, order=1, region_class_order=None, force_separate_z=None,
                              interpolation_order_z=0):
    """segmentation_export.py:73-137 without the files: the class probabilities (c, x, y, z) of the network's grid become the uint8 label map
    of the case's ``original_size_of_raw_data``: the separate-z decision from the spacings, ``resample_and_argmax`` to
    ``size_after_cropping``, and the placement into ``crop_bbox`` (upper bounds clamped to the volume as the reference clamps them).
    ``properties_dict`` is not modified."""
    assert len(segmentation_softmax.shape) == 4, "data must be (c, x, y, z)"
    t, _ = load(segmentation_softmax, "resampling", "segmentation_softmax")
    tensor = isinstance(segmentation_softmax, torch.Tensor)
    shape_after_cropping = tuple(int(v) for v in properties_dict.get('size_after_cropping'))
    do_separate_z, lowres_axis = False, None
    if tuple(t.shape[1:]) != shape_after_cropping:
        if force_separate_z is None:
            if get_do_separate_z(properties_dict.get('original_spacing')):
                do_separate_z, lowres_axis = True, get_lowres_axis(properties_dict.get('original_spacing'))
            elif get_do_separate_z(properties_dict.get('spacing_after_resampling')):
                do_separate_z, lowres_axis = True, get_lowres_axis(properties_dict.get('spacing_after_resampling'))
        else:
            do_separate_z = force_separate_z
            if do_separate_z:
                lowres_axis = get_lowres_axis(properties_dict.get('original_spacing'))
        if lowres_axis is not None and len(lowres_axis) != 1:
            do_separate_z = False
    # (equal shapes: the tables are identities and the kernel is the argmax alone)
    seg = _argmax(t, shape_after_cropping, lowres_axis, order, do_separate_z, interpolation_order_z, region_class_order)
    bbox = properties_dict.get('crop_bbox')
    if bbox is not None:
        full = tuple(int(v) for v in properties_dict.get('original_size_of_raw_data'))
        lo = [int(bbox[c][0]) for c in range(3)]
        hi = [min(lo[c] + seg.shape[c], full[c]) for c in range(3)]      # segmentation_export.py:132
        if any(hi[c] - lo[c] != seg.shape[c] for c in range(3)):
            raise ValueError(f"could not broadcast input array from shape {tuple(seg.shape)} into shape {tuple(h - l for l, h in zip(lo, hi))}")
        out = torch.zeros(full, dtype=torch.uint8, device=seg.device)
        out[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = seg
        seg = out
    return seg.to(segmentation_softmax.device) if tensor else seg.cpu().numpy()
