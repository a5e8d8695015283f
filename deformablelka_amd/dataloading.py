"""The 3-D trainer's batch loader on the HIP kernels of ``csrc/cl_dataload.hip`` (include/dlka.h: ``dlka_load_*``): what
``DataLoader3D.generate_train_batch`` (3D/d_lka_former/training/dataloading/dataset_loading.py:155-379) does on the host for every batch
between the preprocessed case and the augmentation, and the ``class_locations`` table its foreground oversampling reads
(preprocessing/preprocessing.py:333-348).  Names, argument order and defaults are the reference's.

  ``class_locations``      preprocessing.py:333-348: class -> int64 (n, 3) rows of ``np.argwhere(seg == c)``, chosen by ONE
                           ``RandomState(seed)`` consumed in the order of ``all_classes``
  ``get_patch_size``       default_data_augmentation.py:107-127 with batchgenerators' ``rotate_coords_3d`` / ``rotate_coords_2d`` beside it:
                           the trainer's ``basic_generator_patch_size``
  ``draw_batch``           the host half of ``generate_train_batch``: keys, forced-foreground flags, chosen class and voxel, box corners
  ``crop_batch``           the device half: every sample's box cut out of its resident case and padded, in one launch
  ``DataLoader3D``         the loader: every case is uploaded once and stays resident; ``training.augmented_batches(loader, augmentation)``
                           takes it as it is

As in ``augmentation``, ``draw_*`` runs on the host, takes a ``numpy.random.RandomState`` and returns a plain dict of numpy arrays;
the apply is a pure function of its input and that record.  With ``rs = np.random.RandomState(s)`` the draws are those of the reference
after ``np.random.seed(s)``.  Of a label map's content ``class_locations`` brings the counts per class to the host (``choice`` needs them)
and the selected rows, nothing else.  Inputs are not written to.  Without a GPU the device calls raise as every operator of the package
does: there is no host fall-back.

Not part of this module: ``unpack_dataset`` and the other file helpers, the worker processes, the cascade (``has_prev_stage``) and
``DataLoader2D``."""
from __future__ import annotations

import os
import pickle
import warnings
from collections import OrderedDict

import numpy as np
import torch

from ._containers import to_working_device
from .ops import dataload

__all__ = ["class_locations", "get_patch_size", "rotate_coords_3d", "rotate_coords_2d", "draw_batch", "crop_batch", "DataLoader3D",
           "launch_count"]


def launch_count() -> int:
    """Kernel launches of this module so far (this process)."""
    return dataload.load_launch_count()


# ---- preprocessing.py:333-348 ---------------------------------------------------------------------------------------------------------------------
def _label_map(seg):
    t = to_working_device(seg, "dataloading", "seg")
    if t.ndim != 3:
        raise NotImplementedError(f"dataloading: class_locations takes one label map (X, Y, Z), got {tuple(t.shape)}")
    if t.dtype == torch.float32 or t.dtype == torch.int32:
        return t
    return t.to(torch.float32 if t.is_floating_point() else torch.int32)


def class_locations(seg, all_classes, num_samples=10000, min_percent_coverage=0.01, seed=1234):
    """class -> int64 numpy (n, 3): ``np.argwhere(seg == c)[rndst.choice(len, target, replace=False)]`` with
    ``target = max(min(num_samples, len), ceil(len * min_percent_coverage))``; ``[]`` for a class that is absent.  ``seg``: one label map
    (X, Y, Z), numpy or a tensor on either side, float32 with integer values or an integer dtype; labels not in ``all_classes`` are ignored."""
    t = _label_map(seg)
    classes = list(all_classes)
    distinct = list(OrderedDict.fromkeys(int(c) for c in classes))
    if not classes:
        return {}
    totals_dev, state = dataload.load_class_counts(t, distinct)
    totals = totals_dev.cpu().tolist()                       # the one read the draw needs
    rndst = np.random.RandomState(seed)
    class_locs, slots, ranks, spans = {}, [], [], []
    for c in classes:
        slot = distinct.index(int(c))
        n = totals[slot]
        if n == 0:
            class_locs[c] = []
            continue
        target_num_samples = min(num_samples, n)
        target_num_samples = max(target_num_samples, int(np.ceil(n * min_percent_coverage)))
        chosen = rndst.choice(n, target_num_samples, replace=False)
        class_locs[c] = None                                 # (the reference's key order: that of all_classes)
        spans.append((c, len(chosen)))
        slots.append(np.full(len(chosen), slot, np.int32))
        ranks.append(chosen.astype(np.int32))
    if spans:
        rows = dataload.load_class_select(state, totals, np.concatenate(slots), np.concatenate(ranks)).cpu().numpy().astype(np.int64)
        at = 0
        for c, n in spans:
            class_locs[c] = rows[at:at + n]
            at += n
    return class_locs


# ---- default_data_augmentation.py:107-127 ---------------------------------------------------------------------------------------------------------
def _rotation_x(angle):
    return np.array([[1, 0, 0], [0, np.cos(angle), -np.sin(angle)], [0, np.sin(angle), np.cos(angle)]])


def _rotation_y(angle):
    return np.array([[np.cos(angle), 0, np.sin(angle)], [0, 1, 0], [-np.sin(angle), 0, np.cos(angle)]])


def _rotation_z(angle):
    return np.array([[np.cos(angle), -np.sin(angle), 0], [np.sin(angle), np.cos(angle), 0], [0, 0, 1]])


def rotate_coords_3d(coords, angle_x, angle_y, angle_z):
    """batchgenerators.augmentations.utils.rotate_coords_3d."""
    rot_matrix = np.identity(len(coords))
    rot_matrix = np.dot(rot_matrix, _rotation_x(angle_x))
    rot_matrix = np.dot(rot_matrix, _rotation_y(angle_y))
    rot_matrix = np.dot(rot_matrix, _rotation_z(angle_z))
    return np.dot(coords.reshape(len(coords), -1).transpose(), rot_matrix).transpose().reshape(coords.shape)


def rotate_coords_2d(coords, angle):
    """batchgenerators.augmentations.utils.rotate_coords_2d."""
    rot_matrix = np.array([[np.cos(angle), -np.sin(angle)], [np.sin(angle), np.cos(angle)]])
    return np.dot(coords.reshape(len(coords), -1).transpose(), rot_matrix).transpose().reshape(coords.shape)


def get_patch_size(final_patch_size, rot_x, rot_y, rot_z, scale_range):
    """The extents a loader has to deliver so that a rotation by up to ``rot_*`` (radians, a number or a range) and a zoom by
    ``min(scale_range)`` still fill ``final_patch_size``: an integer array."""
    if isinstance(rot_x, (tuple, list)):
        rot_x = max(np.abs(rot_x))
    if isinstance(rot_y, (tuple, list)):
        rot_y = max(np.abs(rot_y))
    if isinstance(rot_z, (tuple, list)):
        rot_z = max(np.abs(rot_z))
    rot_x = min(90 / 360 * 2. * np.pi, rot_x)
    rot_y = min(90 / 360 * 2. * np.pi, rot_y)
    rot_z = min(90 / 360 * 2. * np.pi, rot_z)
    coords = np.array(final_patch_size)
    final_shape = np.copy(coords)
    if len(coords) == 3:
        final_shape = np.max(np.vstack((np.abs(rotate_coords_3d(coords, rot_x, 0, 0)), final_shape)), 0)
        final_shape = np.max(np.vstack((np.abs(rotate_coords_3d(coords, 0, rot_y, 0)), final_shape)), 0)
        final_shape = np.max(np.vstack((np.abs(rotate_coords_3d(coords, 0, 0, rot_z)), final_shape)), 0)
    elif len(coords) == 2:
        final_shape = np.max(np.vstack((np.abs(rotate_coords_2d(coords, rot_x)), final_shape)), 0)
    final_shape = final_shape / min(scale_range)
    return final_shape.astype(int)


# ---- dataset_loading.py:204-205, 223-333 ----------------------------------------------------------------------------------------------------------
def _do_oversample(batch_idx, batch_size, oversample_foreground_percent):
    return not batch_idx < round(batch_size * (1 - oversample_foreground_percent))


def draw_batch(rs, cases, patch_size, need_to_pad, batch_size, oversample_foreground_percent):
    """The draws of one ``generate_train_batch`` in the reference's order: ``choice(keys, batch_size, True)``, then per sample three
    ``randint`` or, for a forced-foreground sample, ``choice(foreground_classes)`` and ``choice(len(voxels))``.

    ``cases``: key -> {'shape': the case's (X, Y, Z), 'properties': a dict with 'class_locations'} in the loader's order.  ``need_to_pad``
    is the LOADER'S array and is written to: a case smaller than the patch enlarges it for every later sample and batch (the reference
    aliases it, :275-280).  A forced sample is clamped from below only (:322-324).

    Returns numpy arrays: ``keys`` (B,), ``force_fg`` (B,) bool, ``selected_class`` (B,) int64 (-1: none), ``selected_voxel`` (B, 3) int64
    (-1: none), ``bbox_lb`` (B, 3) int64."""
    if not isinstance(need_to_pad, np.ndarray) or need_to_pad.shape != (3,) or need_to_pad.dtype.kind != "i":
        raise ValueError("dataloading: need_to_pad is the loader's integer array of three entries (it is updated in place)")
    patch_size = [int(v) for v in patch_size]
    list_of_keys = list(cases.keys())
    selected_keys = rs.choice(list_of_keys, batch_size, True, None)
    rec = {"keys": selected_keys, "force_fg": np.zeros(batch_size, bool), "selected_class": np.full(batch_size, -1, np.int64),
           "selected_voxel": np.full((batch_size, 3), -1, np.int64), "bbox_lb": np.zeros((batch_size, 3), np.int64)}
    for j, i in enumerate(selected_keys):
        force_fg = _do_oversample(j, batch_size, oversample_foreground_percent)
        properties = cases[i]["properties"]
        shape = tuple(int(v) for v in cases[i]["shape"])
        for d in range(3):
            if need_to_pad[d] + shape[d] < patch_size[d]:
                need_to_pad[d] = patch_size[d] - shape[d]
        lb = [-need_to_pad[d] // 2 for d in range(3)]
        ub = [shape[d] + need_to_pad[d] // 2 + need_to_pad[d] % 2 - patch_size[d] for d in range(3)]
        voxels_of_that_class = None
        if force_fg:
            if 'class_locations' not in properties.keys():
                raise RuntimeError("Please rerun the preprocessing with the newest version of nnU-Net!")
            foreground_classes = np.array([c for c in properties['class_locations'].keys() if len(properties['class_locations'][c]) != 0])
            foreground_classes = foreground_classes[foreground_classes > 0]
            if len(foreground_classes) == 0:
                warnings.warn(f"dataloading: case {i} does not contain any foreground classes")
            else:
                selected_class = rs.choice(foreground_classes)
                voxels_of_that_class = properties['class_locations'][selected_class]
                rec["selected_class"][j] = selected_class
        if voxels_of_that_class is not None:
            selected_voxel = voxels_of_that_class[rs.choice(len(voxels_of_that_class))]
            bbox_lb = [max(lb[d], selected_voxel[d] - patch_size[d] // 2) for d in range(3)]
            rec["selected_voxel"][j] = selected_voxel
        else:
            bbox_lb = [rs.randint(lb[d], ub[d] + 1) for d in range(3)]
        rec["force_fg"][j] = force_fg
        rec["bbox_lb"][j] = bbox_lb
    return rec


# ---- dataset_loading.py:331-368 -------------------------------------------------------------------------------------------------------------------
def _pad_arguments(pad_mode, pad_kwargs_data):
    kwargs = dict(pad_kwargs_data or {})
    if pad_mode == "constant":
        constant = kwargs.pop("constant_values", 0)
        if kwargs or np.ndim(constant) != 0:
            raise NotImplementedError(f"dataloading: pad_kwargs_data={pad_kwargs_data!r} (supported with 'constant': one scalar constant_values)")
        return float(constant)
    if pad_mode == "edge":
        if kwargs:
            raise NotImplementedError(f"dataloading: pad_kwargs_data={pad_kwargs_data!r} ('edge' takes none)")
        return 0.0
    raise NotImplementedError(f"dataloading: pad_mode={pad_mode!r} (supported: 'constant', 'edge')")


def crop_batch(cases, bbox_lb, patch_size, pad_mode="constant", pad_kwargs_data=None):
    """(data (B, C, *patch_size), seg (B, 1, *patch_size)) float32 on the device: sample b is the box of ``patch_size`` at ``bbox_lb[b]`` of
    ``cases[b]``, a resident float32 tensor (C + 1, X_b, Y_b, Z_b) whose last channel is the label map.  Data outside the case takes
    ``pad_mode`` ('constant' with ``pad_kwargs_data['constant_values']``, default 0, or 'edge'); the label map always takes -1."""
    constant = _pad_arguments(pad_mode, pad_kwargs_data)
    cases = list(cases)
    lb = np.asarray(bbox_lb, dtype=np.int64)
    if pad_mode == "edge" and lb.shape == (len(cases), 3):
        for t, corner in zip(cases, lb):
            if any(corner[d] >= t.shape[1 + d] or corner[d] + int(patch_size[d]) <= 0 for d in range(3)):
                raise ValueError(f"can't extend empty axis using modes other than 'constant' (the box at {corner.tolist()} misses the case "
                                 f"{tuple(t.shape[1:])})")
    return dataload.load_crop_batch(cases, lb, patch_size, pad_mode, constant)


# ---- dataset_loading.py:155-379 -------------------------------------------------------------------------------------------------------------------
def _load_entry(entry, memmap_mode):
    if "data" in entry:
        return entry["data"]
    data_file = entry["data_file"]
    if os.path.isfile(data_file[:-4] + ".npy"):
        return np.array(np.load(data_file[:-4] + ".npy", memmap_mode))    # (read once, here: the map is not kept)
    return np.load(data_file)['data']


def _load_properties(entry):
    if "properties" in entry:
        return entry["properties"]
    with open(entry["properties_file"], "rb") as f:
        return pickle.load(f)


class DataLoader3D(object):
    """``dataset_loading.DataLoader3D`` with every case resident on the device.  ``data``: key -> entry with 'data' (an array or tensor
    (C + 1, X, Y, Z), the label map last) or 'data_file' (.npy / .npz, read with numpy as the reference reads it) and 'properties' or
    'properties_file'.  Every case is uploaded once, here.  ``seed`` seeds the loader's own ``RandomState`` (the reference draws from
    numpy's global stream); ``generate_train_batch`` returns {'data', 'seg', 'properties', 'keys'} with 'data' and 'seg' on the device,
    and ``last_draw`` keeps the record of ``draw_batch`` it applied."""

    def __init__(self, data, patch_size, final_patch_size, batch_size, has_prev_stage=False, oversample_foreground_percent=0.0,
                 memmap_mode="r", pad_mode="edge", pad_kwargs_data=None, pad_sides=None, *, device=None, seed=None):
        if has_prev_stage:
            raise NotImplementedError("dataloading: has_prev_stage=True (the cascade)")
        if pad_kwargs_data is None:
            pad_kwargs_data = OrderedDict()
        _pad_arguments(pad_mode, pad_kwargs_data)
        self._data = data
        self.batch_size = batch_size
        self.pad_kwargs_data = pad_kwargs_data
        self.pad_mode = pad_mode
        self.oversample_foreground_percent = oversample_foreground_percent
        self.final_patch_size = final_patch_size
        self.has_prev_stage = has_prev_stage
        self.patch_size = patch_size
        self.list_of_keys = list(self._data.keys())
        self.need_to_pad = (np.array(patch_size) - np.array(final_patch_size)).astype(int)
        if pad_sides is not None:
            if not isinstance(pad_sides, np.ndarray):
                pad_sides = np.array(pad_sides)
            self.need_to_pad += pad_sides
        self.memmap_mode = memmap_mode
        self.num_channels = None
        self.pad_sides = pad_sides
        self.rs = np.random.RandomState(seed)
        self.last_draw = None
        self._resident, self._cases = {}, OrderedDict()
        for k in self.list_of_keys:
            t = to_working_device(_load_entry(self._data[k], memmap_mode), "dataloading", f"the data of case {k!r}")
            if device is not None:
                t = t.to(device)
            if t.ndim != 4 or t.shape[0] < 2:
                raise RuntimeError(f"dataloading: a case is (C + 1, X, Y, Z) with the label map last, got {tuple(t.shape)} for {k!r}")
            self._resident[k] = t.to(torch.float32).contiguous()
            self._cases[k] = {"shape": tuple(t.shape[1:]), "properties": _load_properties(self._data[k])}
        self.data_shape, self.seg_shape = self.determine_shapes()

    def get_do_oversample(self, batch_idx):
        return _do_oversample(batch_idx, self.batch_size, self.oversample_foreground_percent)

    def determine_shapes(self):
        num_seg = 1
        k = list(self._data.keys())[0]
        num_color_channels = self._resident[k].shape[0] - 1
        data_shape = (self.batch_size, num_color_channels, *self.patch_size)
        seg_shape = (self.batch_size, num_seg, *self.patch_size)
        return data_shape, seg_shape

    def generate_train_batch(self):
        rec = draw_batch(self.rs, self._cases, self.patch_size, self.need_to_pad, self.batch_size, self.oversample_foreground_percent)
        data, seg = crop_batch([self._resident[k] for k in rec["keys"]], rec["bbox_lb"], self.patch_size, self.pad_mode, self.pad_kwargs_data)
        self.last_draw = rec
        return {'data': data, 'seg': seg, 'properties': [self._cases[k]["properties"] for k in rec["keys"]], 'keys': rec["keys"]}

    def __iter__(self):
        return self

    def __next__(self):
        return self.generate_train_batch()


def __getattr__(name):
    if name == "DataLoader2D":
        raise NotImplementedError("dataloading: DataLoader2D is not implemented; DataLoader3D is")
    if name in ("unpack_dataset", "pack_dataset", "load_dataset", "delete_npy"):
        raise NotImplementedError(f"dataloading: {name} (the dataset's files) is not part of this module")
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
