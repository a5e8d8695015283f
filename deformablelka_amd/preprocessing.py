"""nnU-Net's case preprocessing on the HIP kernels of ``csrc/cl_preprocess.hip`` (include/dlka.h: ``dlka_prep_*``): what the reference runs on
one host core per case before either trainer or ``predict_simple`` sees it — ``ImageCropper.crop`` (3D/d_lka_former/preprocessing/cropping.py:
23-150: scipy's ``binary_fill_holes`` over the raw volume, two full-volume copies) and ``GenericPreprocessor.resample_and_normalize``
(preprocessing/preprocessing.py:228-306: order-3 resampling, one numpy pass per modality).

  ``create_nonzero_mask``, ``get_bbox_from_mask``, ``crop_to_bbox``, ``crop_to_nonzero``   cropping.py:23-116, same names, arguments, defaults
  ``ImageCropper.crop``                                          cropping.py:138-150
  ``GenericPreprocessor``                                        preprocessing.py:204-316: ``resample_and_normalize``, ``preprocess_test_case`` and
                                                                 ``preprocess_arrays``, which is ``preprocess_test_case`` from the point where the
                                                                 files have been read

Filling holes is "label the background (connectivity 1, ``dlka_cc_components``), keep the components that touch no face of the array".
Inputs are numpy arrays or torch tensors, on the host or the device; host data is moved to the device.  A tensor in gives a tensor out on the
same device, numpy in gives numpy out.  The arguments are NOT written to (the reference edits ``data``, ``seg`` and ``properties`` in place):
copies are returned.  Between the crop and the normalisation the volume stays on the device; of the volume's content the host reads the six
box integers with the cell count, and the ``classes`` list.  Without a GPU the calls raise as every operator of the package does: there is no
host fall-back."""
from __future__ import annotations

import copy

import numpy as np
import torch

from . import ops
from ._containers import load
from .resampling import RESAMPLING_SEPARATE_Z_ANISO_THRESHOLD, resample_patient

__all__ = ["create_nonzero_mask", "get_bbox_from_mask", "crop_to_bbox", "crop_to_nonzero", "ImageCropper", "GenericPreprocessor"]


def _spatial_rank(shape, what):
    if len(shape) not in (3, 4):
        raise NotImplementedError(f"preprocessing: {what} must have shape (C, X, Y, Z) or shape (C, X, Y), got {tuple(shape)}")
    return len(shape) - 1


def _box_list(box, rank):
    """[[lo, hi], ...] as Python ints from the device's eight integers (the ONE read of a crop); nothing set: numpy's error for min(empty)."""
    v = box.cpu().tolist()
    if v[6] == 0:
        raise ValueError("zero-size array to reduction operation minimum which has no identity (the mask has no cell to crop to)")
    return [[int(v[ax]), int(v[3 + ax]) + 1] for ax in range(3 - rank, 3)]


def _seg_to_device(seg, data_t):
    t, back = load(seg, "preprocessing", "seg")
    if tuple(t.shape[1:]) != tuple(data_t.shape[1:]) or t.ndim != data_t.ndim:
        raise ValueError(f"preprocessing: seg {tuple(t.shape)} does not have the extents of data {tuple(data_t.shape)}")
    return t.to(device=data_t.device, dtype=torch.int32), back


# ---- cropping.py -------------------------------------------------------------------------------------------------------------------------------
def create_nonzero_mask(data):
    """cropping.py:23-31: the cells that are nonzero in any channel, holes filled (scipy.ndimage.binary_fill_holes, default structure): bool."""
    _spatial_rank(data.shape, "data")
    t, back = load(data, "preprocessing", "data")
    if t.dtype != torch.float32:          # only "!= 0" matters, and a cast could round a small value to 0
        t = (t != 0).to(torch.float32)
    mask, _ = ops.prep_nonzero_mask(t)
    return back(mask, torch.bool)


def get_bbox_from_mask(mask, outside_value=0):
    """cropping.py:34-42: [[lo, hi], ...] per axis of the cells that differ from ``outside_value``, as Python ints."""
    if len(mask.shape) not in (2, 3):
        raise NotImplementedError(f"preprocessing: a mask of rank 2 or 3, got {tuple(mask.shape)}")
    t, _ = load(mask, "preprocessing", "mask")
    return _box_list(ops.prep_mask_bbox((t != outside_value).to(torch.uint8)), t.ndim)


def crop_to_bbox(image, bbox):
    """cropping.py:45-48: the box of one channel (a view, as in the reference)."""
    if len(image.shape) not in (2, 3) or len(bbox) != len(image.shape):
        raise NotImplementedError(f"preprocessing: an image of rank 2 or 3 and one [lo, hi] per axis, got {tuple(image.shape)} and {bbox}")
    return image[tuple(slice(int(b[0]), int(b[1])) for b in bbox)]


def _crop(t, seg_t, nonzero_label, nan_to_zero):
    """(data float32, seg int32, bbox) on the device from float32 data and an int32 seg or None."""
    mask, box = ops.prep_nonzero_mask(t)
    bbox = _box_list(box, t.ndim - 1)
    data, seg = ops.prep_crop(t, seg_t, mask, bbox, nonzero_label, nan_to_zero)
    return data, seg, bbox


def crop_to_nonzero(data, seg=None, nonzero_label=-1):
    """cropping.py:84-116: (data, seg, bbox).  Outside the nonzero mask the label map gets ``nonzero_label`` wherever it is 0; without a seg it is
    ``nonzero_label`` there and 0 inside (int64).  Data with nothing nonzero raises ValueError, as numpy's min of an empty array does."""
    _spatial_rank(data.shape, "data")
    t, back = load(data, "preprocessing", "data")
    seg_t, seg_back = (None, None) if seg is None else _seg_to_device(seg, t)
    out, seg_out, bbox = _crop(t.to(torch.float32), seg_t, nonzero_label, False)
    if seg is None:
        return back(out), back(seg_out, torch.int64), bbox
    return back(out), seg_back(seg_out), bbox


class ImageCropper(object):
    """cropping.py:123-150 without the files: ``crop`` only."""

    def __init__(self, num_threads=None, output_folder=None):
        if output_folder is not None:
            raise NotImplementedError("preprocessing: ImageCropper(output_folder=...) — writing .npz / .pkl files is not part of this module")
        self.num_threads, self.output_folder = num_threads, output_folder

    @staticmethod
    def crop(data, properties, seg=None):
        """(data, seg, properties): a copy of ``properties`` with ``crop_bbox``, ``classes`` (the sorted values of the cropped seg, a numpy array)
        and ``size_after_cropping``; labels below -1 become 0 (:148)."""
        data_out, seg_out, properties, _ = ImageCropper._crop(data, properties, seg, False)
        return data_out, seg_out, properties

    @staticmethod
    def _crop(data, properties, seg, nan_to_zero):
        """``crop`` that also hands on the device tensors (float32, int32) for the next stage."""
        _spatial_rank(data.shape, "data")
        t, back = load(data, "preprocessing", "data")
        seg_t, seg_back = (None, None) if seg is None else _seg_to_device(seg, t)
        out, seg_out, bbox = _crop(t.to(torch.float32), seg_t, -1, nan_to_zero)
        classes = torch.unique(seg_out).cpu().numpy()
        seg_out = torch.where(seg_out < -1, torch.zeros_like(seg_out), seg_out)
        properties = copy.copy(properties)
        properties["crop_bbox"] = bbox
        properties["classes"] = classes if seg is None or isinstance(seg, torch.Tensor) else classes.astype(np.asarray(seg).dtype)
        properties["size_after_cropping"] = tuple(out[0].shape)
        seg_ret = back(seg_out, torch.int64) if seg is None else seg_back(seg_out)
        return back(out), seg_ret, properties, (out, seg_out)

    def __getattr__(self, name):
        if name in ("crop_from_list_of_files", "load_crop_save", "run_cropping", "get_list_of_cropped_files", "load_properties", "save_properties"):
            raise NotImplementedError(f"preprocessing: ImageCropper.{name} (files and the worker pool) is not part of this module")
        raise AttributeError(name)


# ---- preprocessing.py ----------------------------------------------------------------------------------------------------------------------------
class GenericPreprocessor(object):
    """preprocessing.py:204-316.  ``normalization_scheme_per_modality`` {0: 'CT' | 'CT2' | anything else ("nonCT")}, ``use_nonzero_mask``
    {0: bool}, ``intensityproperties`` {0: {'mean', 'sd', 'percentile_00_5', 'percentile_99_5'}} for the CT schemes."""

    def __init__(self, normalization_scheme_per_modality, use_nonzero_mask, transpose_forward: (tuple, list), intensityproperties=None):
        self.transpose_forward = transpose_forward
        self.intensityproperties = intensityproperties
        self.normalization_scheme_per_modality = normalization_scheme_per_modality
        self.use_nonzero_mask = use_nonzero_mask
        self.resample_separate_z_anisotropy_threshold = RESAMPLING_SEPARATE_Z_ANISO_THRESHOLD

    def _records(self, channels):
        assert len(self.normalization_scheme_per_modality) == channels, "self.normalization_scheme_per_modality " \
                                                                        "must have as many entries as data has " \
                                                                        "modalities"
        assert len(self.use_nonzero_mask) == channels, "self.use_nonzero_mask must have as many entries as data" \
                                                       " has modalities"
        records = []
        for c in range(channels):
            scheme = self.normalization_scheme_per_modality[c]
            lower = upper = mean = sd = 0.0
            if scheme in ("CT", "CT2"):
                assert self.intensityproperties is not None, "ERROR: if there is a CT then we need intensity properties"
                lower = float(self.intensityproperties[c]['percentile_00_5'])
                upper = float(self.intensityproperties[c]['percentile_99_5'])
            if scheme == "CT":
                mean, sd = float(self.intensityproperties[c]['mean']), float(self.intensityproperties[c]['sd'])
            records.append((scheme, lower, upper, mean, sd, bool(self.use_nonzero_mask[c])))
        return records

    def _normalize(self, data, seg):
        """float32 data and int32 seg (or None) on the device -> (normalised data, the table of ``ops.prep_normalize``)."""
        records = self._records(data.shape[0])
        if seg is None:
            if any(r[5] for r in records):
                raise ValueError("preprocessing: use_nonzero_mask needs a seg (its last channel is < 0 outside the nonzero mask)")
            seg_last = torch.zeros(data.shape[1:], dtype=torch.int32, device=data.device)
        else:
            seg_last = seg[-1]
        return ops.prep_normalize(data, seg_last, records)

    def normalize(self, data, seg=None):
        """The loop of preprocessing.py:274-305 alone: (data, statistics).  ``statistics`` is float64 (c, 3) = (count, mean, sd) the kernels
        computed in float64 and used (rounded to float32) for the CT2 and nonCT channels; a CT channel has (0, given mean, given sd)."""
        if len(data.shape) != 4:
            raise NotImplementedError(f"preprocessing: normalize takes (C, X, Y, Z) data, got {tuple(data.shape)}")
        t, back = load(data, "preprocessing", "data")
        seg_t = None if seg is None else _seg_to_device(seg, t)[0]
        out, table = self._normalize(t.to(torch.float32), seg_t)
        return back(out), back(table[:, [6, 3, 4]], torch.float64)

    def _resample_and_normalize(self, t, seg_t, target_spacing, properties, force_separate_z, nan_done):
        original_spacing_transposed = np.array(properties["original_spacing"])[self.transpose_forward]
        if not nan_done:     # remove nans (:250): the crop kernel over the whole array, into a copy
            t, _ = ops.prep_crop(t, None, None, [[0, n] for n in t.shape[1:]], nan_to_zero=True, want_seg=False)
        t, seg_t = resample_patient(t, seg_t, np.array(original_spacing_transposed), target_spacing, 3, 1,
                                    force_separate_z=force_separate_z, order_z_data=0, order_z_seg=0,
                                    separate_z_anisotropy_threshold=self.resample_separate_z_anisotropy_threshold)
        if seg_t is not None:
            seg_t = torch.where(seg_t < -1, torch.zeros_like(seg_t), seg_t)
        properties = copy.copy(properties)
        properties["size_after_resampling"] = tuple(t[0].shape)
        properties["spacing_after_resampling"] = target_spacing
        out, _ = self._normalize(t, seg_t)
        return out, seg_t, properties

    def resample_and_normalize(self, data, target_spacing, properties, seg=None, force_separate_z=None):
        """preprocessing.py:228-306: data and seg must already have been transposed by transpose_forward, ``properties`` are the un-transposed
        values.  Returns (data, seg, properties); ``properties`` is a copy with ``size_after_resampling`` and ``spacing_after_resampling``."""
        if len(data.shape) != 4:
            raise NotImplementedError(f"preprocessing: resample_and_normalize takes (C, X, Y, Z) data, got {tuple(data.shape)}")
        t, back = load(data, "preprocessing", "data")
        seg_t, seg_back = (None, None) if seg is None else _seg_to_device(seg, t)
        out, seg_out, properties = self._resample_and_normalize(t.to(torch.float32), seg_t, target_spacing, properties, force_separate_z, False)
        return back(out), None if seg is None else seg_back(seg_out), properties

    def preprocess_arrays(self, data, target_spacing, properties, seg=None, force_separate_z=None, *, all_classes=None):
        """``preprocess_test_case`` (:308-316) from the point where the files have been read: crop to the nonzero region, ``transpose_forward``,
        resample to ``target_spacing`` (already transposed) and normalise.  ``properties`` needs ``original_spacing``.  Data comes back as
        float32; the volume does not leave the device between the stages.  With ``all_classes`` the returned properties carry
        ``class_locations`` of the returned seg's last channel, as ``_run_internal`` records them (:333-348, ``dataloading.class_locations``)."""
        if len(data.shape) != 4:
            raise NotImplementedError(f"preprocessing: preprocess_arrays takes (C, X, Y, Z) data, got {tuple(data.shape)}")
        _, _, properties, (t, seg_t) = ImageCropper._crop(data, properties, seg, True)
        perm = (0, *[i + 1 for i in self.transpose_forward])
        t, seg_t = t.permute(perm).contiguous(), seg_t.permute(perm).contiguous()
        out, seg_out, properties = self._resample_and_normalize(t, seg_t, target_spacing, properties, force_separate_z, True)
        if all_classes is not None:
            from .dataloading import class_locations
            properties["class_locations"] = class_locations(seg_out[-1], all_classes)
        _, back = load(data, "preprocessing", "data")
        if seg is None:
            return back(out, torch.float32), back(seg_out, torch.int64), properties
        return back(out, torch.float32), load(seg, "preprocessing", "seg")[1](seg_out), properties

    def preprocess_test_case(self, data_files, target_spacing, seg_file=None, force_separate_z=None):
        """preprocessing.py:308-316 with cropping.py:61-81: reads the files with SimpleITK, then ``preprocess_arrays``."""
        try:
            import SimpleITK as sitk
        except ImportError as e:
            raise ImportError("preprocessing: preprocess_test_case reads image files with SimpleITK, which is not installed; "
                              "read the case yourself and call preprocess_arrays") from e
        assert isinstance(data_files, list) or isinstance(data_files, tuple), "case must be either a list or a tuple"
        from collections import OrderedDict
        properties = OrderedDict()
        data_itk = [sitk.ReadImage(f) for f in data_files]
        properties["original_size_of_raw_data"] = np.array(data_itk[0].GetSize())[[2, 1, 0]]
        properties["original_spacing"] = np.array(data_itk[0].GetSpacing())[[2, 1, 0]]
        properties["list_of_data_files"] = data_files
        properties["seg_file"] = seg_file
        properties["itk_origin"] = data_itk[0].GetOrigin()
        properties["itk_spacing"] = data_itk[0].GetSpacing()
        properties["itk_direction"] = data_itk[0].GetDirection()
        data = np.vstack([sitk.GetArrayFromImage(d)[None] for d in data_itk]).astype(np.float32)
        seg = None if seg_file is None else sitk.GetArrayFromImage(sitk.ReadImage(seg_file))[None].astype(np.float32)
        return self.preprocess_arrays(data, target_spacing, properties, seg, force_separate_z)

    def __getattr__(self, name):
        if name in ("run", "_run_internal", "load_cropped"):
            raise NotImplementedError(f"preprocessing: GenericPreprocessor.{name} (.npz / .pkl files and the worker pool) is not part of this module; "
                                      "preprocess_arrays(..., all_classes=...) records class_locations")
        raise AttributeError(name)


def __getattr__(name):
    if name in ("PreprocessorFor2D", "GenericPreprocessor_linearResampling", "Preprocessor3DDifferentResampling", "Preprocessor3DBetterResampling",
                "PreprocessorFor3D_NoResampling", "PreprocessorFor3D_NoResampling_2D", "PreprocessorFor2D_noNormalization",
                "PreprocessorFor3D_LeaveOriginalZSpacing"):
        raise NotImplementedError(f"preprocessing: {name} is not implemented; GenericPreprocessor is")
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
