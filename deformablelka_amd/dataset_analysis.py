"""nnU-Net's dataset fingerprint on the HIP kernels of ``csrc/cl_dataset_stats.hip`` (include/dlka.h: ``dlka_dstats_*``): what the reference's
``DatasetAnalyzer`` (3D/d_lka_former/experiment_planning/DatasetAnalyzer.py) computes on host cores from the cropped cases of a dataset, and
what ``GenericPreprocessor(..., intensityproperties=...)`` needs for its CT schemes.  The reference's names, argument order and result keys;
its folder of ``.npz`` / ``.pkl`` files and its worker pool are replaced by cases in memory.

  ``foreground_voxels``              ``_get_voxels_in_foreground`` (:161-166): ``modality[seg > 0][::10]`` of one case, on the device
  ``order_statistics``               the k-th smallest values of a float32 buffer, exactly (a radix select: no sort)
  ``compute_stats``                  ``_compute_stats`` (:168-179): (median, mean, sd, mn, mx, percentile_99_5, percentile_00_5)
  ``collect_intensity_properties``   :181-223: per modality the seven values of the dataset and, under 'local_props', of every case
  ``unique_labels``                  ``np.unique`` of a label map with labels -1 .. 255 (:76-79)
  ``analyse_segmentations``          :113-132: (class_dct, props_per_patient) with 'has_classes'
  ``class_and_region_sizes``         ``_collect_class_and_region_sizes`` (:64-74)
  ``check_if_all_in_one_region``     ``_check_if_all_in_one_region`` (:50-62)
  ``DatasetAnalyzer``                the class: ``analyze_dataset`` returns the ``dataset_properties`` dict and writes nothing

A case is an array or tensor (C + 1, *spatial), float32, the label map last, as a cropped case is stored; or a pair (data float32
(C, *spatial), seg (S, *spatial) float32, int32 or a narrower integer type) as ``ImageCropper.crop`` returns them, of which the last seg
channel is the label map; or the path of an ``.npz`` with key 'data' (or an ``.npy``).  numpy or torch, host or device; nothing is written
to.  A float32 or int32 label map reaches the kernels in the dtype it is stored in.

Deviations from the reference, all stated in INTEGRATION.md 5g: mean and sd are Python floats accumulated in float64 (the reference's are
numpy's float32 pairwise sums); min, max, median and the percentiles are the reference's float32 values bit for bit, except that a zero
comes back as +0.0; the two region functions label with connectivity = rank, skimage's default.  Without a GPU the calls raise as every
operator of the package does: there is no host fall-back."""
from __future__ import annotations

import os
from collections import OrderedDict

import numpy as np
import torch

from . import postprocessing
from ._containers import load, to_working_device
from .ops import dataset_stats as K

__all__ = ["foreground_voxels", "order_statistics", "compute_stats", "collect_intensity_properties", "unique_labels", "analyse_segmentations",
           "class_and_region_sizes", "check_if_all_in_one_region", "DatasetAnalyzer", "launch_count"]

WHO = "dataset_analysis"
STEP = 10                      # DatasetAnalyzer.py:165: "no need to take every voxel"
_CAST_LABELS = (torch.uint8, torch.int8, torch.int16, torch.bool)     # label dtypes that int32 holds exactly


def launch_count() -> int:
    """Kernels this module's own family has launched in this process (the two region functions launch postprocessing's)."""
    return K.dstats_launch_count()


# ---- cases ------------------------------------------------------------------------------------------------------------------------------------------
def _case(entry):
    """(data float32 (C, *spatial), label map (*spatial) float32 or int32) on the working device, views of the caller's memory where it is
    already there."""
    if isinstance(entry, (str, os.PathLike)):
        path = os.fspath(entry)
        entry = np.load(path) if path.endswith(".npy") else np.load(path)['data']
    if isinstance(entry, (tuple, list)) and len(entry) == 2 and all(hasattr(e, "shape") and len(e.shape) >= 3 for e in entry):
        data, seg = (to_working_device(e, WHO, "cases", "iuf", plural=True) for e in entry)
        if seg.ndim != data.ndim or tuple(seg.shape[1:]) != tuple(data.shape[1:]) or seg.shape[0] < 1:
            raise RuntimeError(f"{WHO}: a case (data (C, *spatial), seg (S, *spatial)), got {tuple(data.shape)} and {tuple(seg.shape)}")
        seg = seg[-1]
    else:
        t = to_working_device(entry, WHO, "cases", "iuf", plural=True)
        if t.ndim not in (3, 4) or t.shape[0] < 2:
            raise RuntimeError(f"{WHO}: a case is (C + 1, *spatial) with 2 or 3 spatial axes, the label map last, got {tuple(t.shape)}")
        data, seg = t[:-1], t[-1]
    if data.ndim not in (3, 4):
        raise RuntimeError(f"{WHO}: a case has 2 or 3 spatial axes, got {tuple(data.shape[1:])}")
    if data.dtype != torch.float32:
        raise RuntimeError(f"{WHO}: modality volumes are float32, as cropped cases are stored, got {data.dtype}")
    if seg.dtype in _CAST_LABELS:                # (narrower integers: int32 holds them exactly; float32 and int32 are read as stored)
        seg = seg.to(torch.int32)
    if seg.dtype not in (torch.float32, torch.int32):
        raise RuntimeError(f"{WHO}: the label map is float32 or int32, got {seg.dtype}")
    return data, seg


def _check_step(step):
    if isinstance(step, bool) or not isinstance(step, (int, np.integer)) or step < 1:
        raise RuntimeError(f"{WHO}: step is a positive integer, got {step!r}")
    return int(step)


def foreground_voxels(data, modality_id, step=STEP):
    """DatasetAnalyzer.py:161-166 for one case: ``data[modality_id][data[-1] > 0][::step]`` as a float32 tensor on the device."""
    step = _check_step(step)
    vols, seg = _case(data)
    channels = vols.shape[0] + (0 if isinstance(data, (tuple, list)) else 1)
    ch = range(channels)[modality_id]
    vol = vols[ch:ch + 1] if ch < vols.shape[0] else seg[None]       # (the reference lets modality_id name the label map itself)
    if vol.dtype != torch.float32:
        raise RuntimeError(f"{WHO}: modality volumes are float32, got {vol.dtype}")
    count, state = K.dstats_fg_count(seg)
    count = int(count.item())
    out = torch.empty((1, -(-count // step)), dtype=torch.float32, device=seg.device)
    K.dstats_fg_sample(vol, state, count, step, out)
    return out[0]


# ---- order statistics ---------------------------------------------------------------------------------------------------------------------------------
def _values(values, what):
    t, back = load(values, WHO, what, "iuf")
    if t.dtype != torch.float32 or t.ndim != 1:
        raise RuntimeError(f"{WHO}: {what} is a one-dimensional float32 buffer, got {t.dtype} {tuple(t.shape)}")
    return t, back


def order_statistics(values, ranks):
    """The ``ranks[j]``-th smallest values (0-based) of the float32 buffer ``values``: ``np.partition(values, ranks)[ranks]`` without a sort,
    NaNs last as numpy sorts them.  A zero comes back as +0.0.  float32, in the container and on the device of ``values``."""
    t, back = _values(values, "values")
    ranks = [int(r) for r in np.asarray(ranks).reshape(-1)]
    got, _ = K.dstats_select(t, ranks)
    return back(got, torch.float32)


def _quantile_plan(n, percent):
    """numpy's ``percentile(list of float32, percent)`` (method 'linear'), its own expressions: the quantile becomes float32 because the data
    is, and so does the virtual index (n - 1) * q.  -> (previous rank, next rank, virtual index, previous index as numpy keeps it)."""
    q = np.asanyarray(np.true_divide(percent, np.float32(100)))
    virtual = np.asanyarray((n - 1) * q)
    previous = np.asanyarray(np.floor(virtual))
    following = np.asanyarray(previous + 1)
    if virtual >= n - 1:
        previous, following = np.asanyarray(-1.0), np.asanyarray(-1.0)
    if virtual < 0:
        previous, following = np.asanyarray(0.0), np.asanyarray(0.0)
    previous, following = previous.astype(np.intp), following.astype(np.intp)
    return int(previous) % n, int(following) % n, virtual, previous


def _lerp(a, b, virtual, previous):
    """numpy's ``_get_gamma`` and ``_lerp`` on float32 scalars: a + (b - a) g for g < 0.5, b - (b - a)(1 - g) otherwise."""
    t = np.asanyarray(np.asanyarray(virtual - previous), dtype=virtual.dtype)
    with np.errstate(all="ignore"):
        diff = np.subtract(b, a)
        r = np.asanyarray(np.add(a, diff * t))
        np.subtract(b, diff * (1 - t), out=r, where=t >= 0.5, casting="unsafe", dtype=type(r.dtype))
    return r[()]


def _stats_on_device(t):
    """``compute_stats`` of a float32 buffer on the device with at least one value: thirteen launches and one read."""
    n = t.numel()
    plans = [_quantile_plan(n, 99.5), _quantile_plan(n, 0.5)]
    wanted = [0, n - 1, (n - 1) // 2, n // 2] + [r for p in plans for r in p[:2]]
    ranks = sorted(set(wanted))
    moments = K.dstats_moments(t)
    values, _ = K.dstats_select(t, ranks)
    moments, values = moments.cpu().numpy(), values.cpu().numpy()
    if moments[3] > 0:                         # (numpy: a NaN in the sample makes every one of the seven a NaN)
        nan = np.float32(np.nan)
        return nan, float("nan"), float("nan"), nan, nan, nan, nan
    v = {r: values[i] for i, r in enumerate(ranks)}
    median = np.mean(np.array([v[(n - 1) // 2], v[n // 2]] if n % 2 == 0 else [v[n // 2]], dtype=np.float32))
    p99_5, p00_5 = (_lerp(v[lo], v[hi], virtual, previous) for lo, hi, virtual, previous in plans)
    return median, float(moments[1]), float(moments[2]), v[0], v[n - 1], p99_5, p00_5


def compute_stats(voxels):
    """DatasetAnalyzer.py:168-179: (median, mean, sd, mn, mx, percentile_99_5, percentile_00_5) of the float32 values ``voxels`` (a tensor, an
    array or the reference's list of float32 scalars).  No value gives seven NaNs, and so does a NaN among them.  median, mn, mx and the
    percentiles are numpy's float32 values; mean and sd are Python floats from a float64 accumulation."""
    if not isinstance(voxels, torch.Tensor):
        voxels = np.asarray(voxels)
    if len(voxels) == 0:
        return np.nan, np.nan, np.nan, np.nan, np.nan, np.nan, np.nan
    t, _ = _values(voxels, "voxels")
    return _stats_on_device(t)


_KEYS = ("median", "mean", "sd", "mn", "mx", "percentile_99_5", "percentile_00_5")


def _stats_or_nans(t):
    return _stats_on_device(t) if t.numel() else (np.nan,) * 7


def collect_intensity_properties(cases, num_modalities):
    """DatasetAnalyzer.py:181-223.  ``cases``: an ordered mapping identifier -> case (see the module's head).  The samples of every case are
    written by the sampling kernel itself into ONE buffer (num_modalities, total), case after case, each case's ``[::10]`` restarting at its
    own first foreground voxel; the dataset's statistics are those of a row of that buffer, a case's those of its slice."""
    num_modalities = int(num_modalities)
    ids = list(cases.keys())
    resident, counts, device = {}, [], None
    for k in ids:
        data, seg = _case(cases[k])
        if not 1 <= num_modalities <= data.shape[0]:
            raise RuntimeError(f"{WHO}: num_modalities = {num_modalities}, but case {k!r} has {data.shape[0]} modalities")
        count, state = K.dstats_fg_count(seg)
        counts.append(int(count.item()))
        device = seg.device
        if isinstance(cases[k], torch.Tensor) and cases[k].device == seg.device:
            resident[k] = (data, state)          # (already on the device: kept, at no cost; anything else is uploaded again for the sample)
    sizes = [-(-c // STEP) for c in counts]
    starts = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    buffer = torch.empty((max(num_modalities, 1), int(starts[-1])), dtype=torch.float32, device=device) if ids else None
    for i, k in enumerate(ids):
        if sizes[i] == 0:
            continue
        if k in resident:
            data, state = resident.pop(k)
        else:
            data, seg = _case(cases[k])
            _, state = K.dstats_fg_count(seg)
        K.dstats_fg_sample(data[:num_modalities], state, counts[i], STEP, buffer, int(starts[i]))
    results = OrderedDict()
    for mod_id in range(num_modalities):
        results[mod_id] = OrderedDict()
        whole = _stats_or_nans(buffer[mod_id]) if ids else (np.nan,) * 7
        props_per_case = OrderedDict()
        for i, k in enumerate(ids):
            local = _stats_or_nans(buffer[mod_id, int(starts[i]):int(starts[i + 1])])
            props_per_case[k] = OrderedDict(zip(_KEYS, local))
        results[mod_id]['local_props'] = props_per_case
        for key, value in zip(_KEYS, whole):
            results[mod_id][key] = value
    return results


# ---- labels -----------------------------------------------------------------------------------------------------------------------------------------
def _label_tensor(seg, what="label maps"):
    t, back = load(seg, WHO, what, "biuf", plural=True)
    if t.dtype in _CAST_LABELS:
        t = t.to(torch.int32)
    return t, back


def unique_labels(seg):
    """``np.unique(seg)`` (DatasetAnalyzer.py:78) of a label map of rank 2 or 3 whose labels lie in -1 .. 255: the sorted values, in seg's
    dtype and container.  Any other label raises."""
    t, back = _label_tensor(seg)
    words = K.dstats_unique_labels(t).cpu().numpy()
    values, outside = K.labels_of_bitmap(words)
    if outside:
        raise RuntimeError(f"{WHO}: unique_labels takes integer labels in -1 .. 255; the map holds another value")
    return back(torch.tensor(values, dtype=torch.int64, device=t.device))


def analyse_segmentations(cases, labels):
    """DatasetAnalyzer.py:113-132: (class_dct, props_per_patient); ``labels`` is dataset.json's 'labels', props_per_patient[id]['has_classes']
    the numpy array of the labels of the case's map."""
    props_per_patient = OrderedDict()
    for k in cases.keys():
        _, seg = _case(cases[k])
        has = unique_labels(seg)
        props_per_patient[k] = {'has_classes': has.cpu().numpy()}
    return labels, props_per_patient


def class_and_region_sizes(seg, all_classes, vol_per_voxel):
    """DatasetAnalyzer.py:64-74: (volume_per_class, region_volume_per_class); the regions of a class are its objects under FULL connectivity
    (skimage.measure.label's default, connectivity = rank), in the order of their first voxel."""
    t, _ = _label_tensor(seg)
    volume_per_class, region_volume_per_class = OrderedDict(), OrderedDict()
    for c in all_classes:
        mask = t == c
        volume_per_class[c] = np.int64(int(mask.sum().item())) * vol_per_voxel
        _, sizes = postprocessing.component_sizes(mask.to(torch.uint8), connectivity=t.ndim)
        region_volume_per_class[c] = [np.int64(s) * vol_per_voxel for s in sizes.cpu().tolist()]
    return volume_per_class, region_volume_per_class


def check_if_all_in_one_region(seg, regions):
    """DatasetAnalyzer.py:50-62: per region (a list of classes; its key is the tuple) whether its voxels form exactly ONE object under full
    connectivity."""
    t, _ = _label_tensor(seg)
    res = OrderedDict()
    for r in regions:
        mask = torch.zeros(t.shape, dtype=torch.bool, device=t.device)
        for c in r:
            mask |= t == c
        _, num = postprocessing.label(mask.to(torch.uint8), connectivity=t.ndim)
        res[tuple(r)] = num == 1
    return res


# ---- the class ----------------------------------------------------------------------------------------------------------------------------------------
_FILE_NAMES = ("folder_with_cropped_data", "props_per_case_file", "intensityproperties_file")


class DatasetAnalyzer(object):
    """``DatasetAnalyzer`` over cases in memory.  ``cases``: ordered mapping identifier -> case; ``properties``: identifier -> the case's
    properties dict (``ImageCropper``'s: 'size_after_cropping', 'original_spacing', 'original_size_of_raw_data', 'itk_spacing');
    ``dataset_json``: the dict of dataset.json ('labels', 'modality').  Nothing is read from or written to disk."""

    def __init__(self, cases, properties=None, dataset_json=None, overwrite=True, num_processes=None, **kwargs):
        for name in kwargs:
            if name in _FILE_NAMES:
                raise NotImplementedError(f"{WHO}: DatasetAnalyzer({name}=...) — folders of .npz / .pkl files are not part of this module; "
                                          "pass the cases, their properties and dataset.json's dict")
            raise TypeError(f"DatasetAnalyzer() got an unexpected keyword argument {name!r}")
        if isinstance(cases, (str, os.PathLike)):
            raise NotImplementedError(f"{WHO}: DatasetAnalyzer(folder_with_cropped_data={os.fspath(cases)!r}) — folders of .npz / .pkl files "
                                      "are not part of this module")
        if not overwrite:
            raise NotImplementedError(f"{WHO}: DatasetAnalyzer(overwrite=False) reads precomputed .pkl files, which this module does not keep")
        if properties is None or dataset_json is None:
            raise TypeError("DatasetAnalyzer(cases, properties, dataset_json): the properties and dataset.json's dict are required")
        self.cases, self.properties, self.dataset_json = cases, properties, dataset_json
        self.overwrite, self.num_processes = overwrite, num_processes
        self.sizes = self.spacings = None
        self.patient_identifiers = list(cases.keys())

    def __getattr__(self, name):
        if name in _FILE_NAMES:
            raise NotImplementedError(f"{WHO}: DatasetAnalyzer.{name} (.npz / .pkl files) is not part of this module")
        raise AttributeError(name)

    def load_properties_of_cropped(self, case_identifier):
        return self.properties[case_identifier]

    _check_if_all_in_one_region = staticmethod(check_if_all_in_one_region)
    _collect_class_and_region_sizes = staticmethod(class_and_region_sizes)
    _compute_stats = staticmethod(compute_stats)

    def _get_unique_labels(self, patient_identifier):
        return unique_labels(_case(self.cases[patient_identifier])[1]).cpu().numpy()

    def _load_seg_analyze_classes(self, patient_identifier, all_classes):
        """:81-107 -> (unique_classes, all_in_one_region, volume_per_class, region_sizes)."""
        _, seg = _case(self.cases[patient_identifier])
        vol_per_voxel = np.prod(self.properties[patient_identifier]['itk_spacing'])
        regions = [list(all_classes)] + [(c,) for c in all_classes]
        volume_per_class, region_sizes = class_and_region_sizes(seg, all_classes, vol_per_voxel)
        return unique_labels(seg).cpu().numpy(), check_if_all_in_one_region(seg, regions), volume_per_class, region_sizes

    def get_classes(self):
        return self.dataset_json['labels']

    def analyse_segmentations(self):
        return analyse_segmentations(self.cases, self.get_classes())

    def get_sizes_and_spacings_after_cropping(self):
        sizes = [self.properties[c]["size_after_cropping"] for c in self.patient_identifiers]
        spacings = [self.properties[c]["original_spacing"] for c in self.patient_identifiers]
        return sizes, spacings

    def get_modalities(self):
        modalities = self.dataset_json["modality"]
        return {int(k): modalities[k] for k in modalities.keys()}

    def get_size_reduction_by_cropping(self):
        size_reduction = OrderedDict()
        for p in self.patient_identifiers:
            props = self.properties[p]
            size_reduction[p] = np.prod(props['size_after_cropping']) / np.prod(props["original_size_of_raw_data"])
        return size_reduction

    def _get_voxels_in_foreground(self, patient_identifier, modality_id):
        return foreground_voxels(self.cases[patient_identifier], modality_id)

    def collect_intensity_properties(self, num_modalities):
        return collect_intensity_properties(self.cases, num_modalities)

    def analyze_dataset(self, collect_intensityproperties=True):
        """:225-256 without the pickle: the ``dataset_properties`` dict."""
        sizes, spacings = self.get_sizes_and_spacings_after_cropping()
        classes = self.get_classes()
        all_classes = [int(i) for i in classes.keys() if int(i) > 0]
        modalities = self.get_modalities()
        intensityproperties = self.collect_intensity_properties(len(modalities)) if collect_intensityproperties else None
        size_reductions = self.get_size_reduction_by_cropping()
        dataset_properties = dict()
        dataset_properties['all_sizes'] = sizes
        dataset_properties['all_spacings'] = spacings
        dataset_properties['all_classes'] = all_classes
        dataset_properties['modalities'] = modalities
        dataset_properties['intensityproperties'] = intensityproperties
        dataset_properties['size_reductions'] = size_reductions
        return dataset_properties
