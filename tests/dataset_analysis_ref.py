"""TEST INFRASTRUCTURE — the numpy restatement of the reference's DatasetAnalyzer (3D/d_lka_former/experiment_planning/DatasetAnalyzer.py)
on cases in memory: what one host core computes.  Held to tests/golden/reference_dataset_analysis.pt, which was recorded from the reference's
own functions; used by tests/dataset_analysis_cases.py and as the yardstick of scripts/time_dataset_analysis.py.  skimage.measure.label's
default (full connectivity) is scipy.ndimage.label with a full structure."""
from collections import OrderedDict

import numpy as np

KEYS = ("median", "mean", "sd", "mn", "mx", "percentile_99_5", "percentile_00_5")


def foreground_voxels(case, modality_id, step=10):
    """:161-166"""
    all_data = np.asarray(case)
    return all_data[modality_id][all_data[-1] > 0][::step]


def compute_stats(voxels):
    """:168-179, on the list of float32 scalars the reference builds"""
    voxels = list(voxels)
    if len(voxels) == 0:
        return np.nan, np.nan, np.nan, np.nan, np.nan, np.nan, np.nan
    with np.errstate(all="ignore"):
        return (np.median(voxels), np.mean(voxels), np.std(voxels), np.min(voxels), np.max(voxels), np.percentile(voxels, 99.5),
                np.percentile(voxels, 00.5))


def statistics64(voxels):
    """(count, mean, sd) of the sample in float64"""
    v = np.asarray(voxels, dtype=np.float64)
    with np.errstate(all="ignore"):
        return v.size, float(np.mean(v)), float(np.std(v))


def collect_intensity_properties(cases, num_modalities):
    """:181-223"""
    results = OrderedDict()
    for mod_id in range(num_modalities):
        results[mod_id] = OrderedDict()
        v = [list(foreground_voxels(case, mod_id)) for case in cases.values()]
        w = []
        for iv in v:
            w += iv
        whole = compute_stats(w)
        props_per_case = OrderedDict()
        for k, iv in zip(cases.keys(), v):
            props_per_case[k] = OrderedDict(zip(KEYS, compute_stats(iv)))
        results[mod_id]['local_props'] = props_per_case
        for key, value in zip(KEYS, whole):
            results[mod_id][key] = value
    return results


def _label_full(mask):
    from scipy import ndimage
    return ndimage.label(mask, ndimage.generate_binary_structure(mask.ndim, mask.ndim))


def check_if_all_in_one_region(seg, regions):
    """:50-62"""
    res = OrderedDict()
    for r in regions:
        new_seg = np.zeros(seg.shape)
        for c in r:
            new_seg[seg == c] = 1
        res[tuple(r)] = _label_full(new_seg)[1] == 1
    return res


def class_and_region_sizes(seg, all_classes, vol_per_voxel):
    """:64-74"""
    volume_per_class, region_volume_per_class = OrderedDict(), OrderedDict()
    for c in all_classes:
        region_volume_per_class[c] = []
        volume_per_class[c] = np.sum(seg == c) * vol_per_voxel
        labelmap, numregions = _label_full(seg == c)
        for l in range(1, numregions + 1):
            region_volume_per_class[c].append(np.sum(labelmap == l) * vol_per_voxel)
    return volume_per_class, region_volume_per_class
