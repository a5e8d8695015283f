"""Generates tests/golden/reference_preprocessing.pt from the REFERENCE'S OWN create_nonzero_mask, get_bbox_from_mask, crop_to_nonzero and
ImageCropper.crop (3D/d_lka_former/preprocessing/cropping.py:23-150) and GenericPreprocessor.resample_and_normalize
(3D/d_lka_former/preprocessing/preprocessing.py:228-306), loaded from their files.  The imports these never use are stubbed exactly as
tests/golden/make_golden_resampling.py stubs them (SimpleITK, batchgenerators' file helpers); d_lka_former.configuration is the reference's own
file.  skimage and batchgenerators are not installed: ``skimage.transform.resize`` and ``batchgenerators.augmentations.utils.resize_segmentation``
are bound to the scipy restatement of tests/resampling_ref.py.

What this fixture pins.  For cropping and normalisation: the reference's own code on scipy (binary_fill_holes) and numpy.  For the resampling
step of the pipeline calls: the same restatement that reference_resampling.pt pins (the reference's control flow on top of
scipy.ndimage.map_coordinates at (i + 0.5) * n_in / n_out - 0.5, mode 'nearest').  The pipeline rows are the reference's ImageCropper.crop, the
transposition of preprocess_test_case (:311-312) and resample_and_normalize, called one after the other as preprocess_test_case calls them once
the files are read.  The reference's get_bbox_from_mask and crop_to_bbox index three axes: the box and crop rows of the rank-2 case ("planar")
come from tests/preprocessing_ref.py, its mask from the reference.

The normalisation rows are resample_and_normalize with the module's resample_patient bound to the identity for the call: resample_data_or_seg
returns float32 after a resampling (:198) but float64 when the shapes agree (:133, :201), and the loop of :274-305 is recorded on float32 data, the
case every real call meets.

The inputs are rebuilt by tests/preprocessing_cases.py and only their SHA-256 is stored.  Results are tensors and plain Python values.  Per
normalisation call ``f64_gap`` is the largest distance, relative to max|out|, between the reference's output (numpy's float32 means) and the
float32 formula evaluated with numpy's float64 statistics; a gap beyond tests/preprocessing_cases.GAP_BOUND refuses to write the fixture.
Run: python tests/golden/make_golden_preprocessing.py"""
import contextlib
import copy
import importlib.util
import io
import os
import sys
import types
import warnings

import numpy as np
import scipy
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import preprocessing_cases as C   # noqa: E402
from tests import preprocessing_ref as PR    # noqa: E402
from tests import resampling_ref as R        # noqa: E402

REF = "/root/reference"
PKG = os.path.join(REF, "3D", "d_lka_former")


def load_reference():
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    def from_file(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod

    for name in ("d_lka_former", "d_lka_former.preprocessing", "batchgenerators", "batchgenerators.utilities", "batchgenerators.augmentations",
                 "skimage"):
        stub(name).__path__ = []
    stub("SimpleITK")
    stub("batchgenerators.utilities.file_and_folder_operations")
    stub("batchgenerators.augmentations.utils", resize_segmentation=R.resize_segmentation)
    stub("skimage.transform", resize=R.resize)
    from_file("d_lka_former.configuration", os.path.join(PKG, "configuration.py"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        crop = from_file("d_lka_former.preprocessing.cropping", os.path.join(PKG, "preprocessing", "cropping.py"))
        pre = from_file("d_lka_former.preprocessing.preprocessing", os.path.join(PKG, "preprocessing", "preprocessing.py"))
    return crop, pre


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **k)


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def record_crop(crop, name):
    data, seg = C.CROP_CASES[name]()
    assert data[0].size <= 25000
    rec = {"input": C.digest(data)}
    if seg is not None:
        rec["seg_input"] = C.digest(seg)
    if name == "all_zero":
        try:
            crop.crop_to_nonzero(data.copy())
        except ValueError:
            rec["raises"] = "ValueError"
        assert rec.get("raises") == "ValueError"
        return rec
    mask = crop.create_nonzero_mask(data)
    rec["mask"] = t(mask.astype(np.uint8))
    rank3 = data.ndim == 4
    own = crop if rank3 else PR
    rec["bbox"] = own.get_bbox_from_mask(mask, 0)
    for label, key in ((-1, "crop"), (-7, "crop_label_m7")):
        d, s, bbox = own.crop_to_nonzero(data.copy(), None if seg is None else seg.copy(), label)
        assert bbox == rec["bbox"]
        rec[key] = {"seg": t(s.astype(np.int8))}
        if key == "crop":
            rec[key]["data"] = t(d.copy())
    if rank3:
        d, s, props = quiet(crop.ImageCropper.crop, data.copy(), {"original_spacing": np.array([1.0, 1.0, 1.0])},
                            None if seg is None else seg.copy())
    else:
        d, s, props = PR.crop(data.copy(), {"original_spacing": np.array([1.0, 1.0, 1.0])}, None)
    assert props["crop_bbox"] == rec["bbox"]
    rec["cropper"] = {"seg": t(s.astype(np.int8)), "classes": [int(v) for v in props["classes"]],
                      "size_after_cropping": tuple(int(v) for v in props["size_after_cropping"])}
    # the restatement agrees with what was recorded
    assert np.array_equal(PR.create_nonzero_mask(data), mask) and PR.get_bbox_from_mask(mask) == rec["bbox"]
    nonzero = (data != 0).any(0)
    rec["filled"] = int(mask.sum()) - int(nonzero.sum())
    return rec


def record_normalize(pre, call):
    cid, schemes, use_mask = call
    data, seg = C.normalize_input()
    g = pre.GenericPreprocessor({c: schemes[c] for c in range(3)}, {c: use_mask[c] for c in range(3)}, [0, 1, 2], C.INTENSITY)
    props = {"original_spacing": np.array([1.0, 1.0, 1.0])}
    real = pre.resample_patient
    pre.resample_patient = lambda d, s, *a, **k: (d, s)     # (see the header: the loop runs on float32 data, as it does after a resampling)
    try:
        out, sout, _ = quiet(g.resample_and_normalize, data.copy(), np.array([1.0, 1.0, 1.0]), props, seg.copy())
    finally:
        pre.resample_patient = real
    assert out.dtype == np.float32 and out.shape == data.shape
    counts, gap = {}, 0.0
    for c, scheme in enumerate(schemes):
        p = C.INTENSITY[c]
        lower, upper = p['percentile_00_5'], p['percentile_99_5']
        if scheme == "CT":
            f = PR.formula32(data[c], seg[-1], scheme, use_mask[c], lower, upper, p['mean'], p['sd'])
            assert C.same_bits(f, out[c]), "the CT arithmetic is not plain float32 under this numpy"
            continue
        n, m64, s64 = PR.statistics64(data[c], seg[-1], scheme, use_mask[c], np.float32(lower), np.float32(upper))
        counts[c] = n
        f = PR.formula32(data[c], seg[-1], scheme, use_mask[c], lower, upper, m64, s64)
        gap = max(gap, float(np.abs(f.astype(np.float64) - out[c]).max() / np.abs(out[c]).max()))
    assert gap <= C.GAP_BOUND, f"{cid}: f64_gap {gap} beyond {C.GAP_BOUND}: the fixture is not written"
    assert C.same_bits(PR.normalize(data, seg, schemes, use_mask, C.INTENSITY), out)
    return {"input": C.digest(data), "seg_input": C.digest(seg), "out": t(out.copy()), "seg": t(sout.copy()), "counts": counts, "f64_gap": gap}


def record_pipeline(crop, pre, cid):
    shape, original, target, tf, schemes, use_mask, with_seg = C.PIPE_CALLS[cid]
    data, seg = C.pipeline_input(cid)
    n = len(schemes)
    g = pre.GenericPreprocessor({c: schemes[c] for c in range(n)}, {c: use_mask[c] for c in range(n)}, tf, {c: C.CT_PROPS for c in range(n)})
    props = {"original_spacing": np.array(original), "original_size_of_raw_data": np.array(shape[1:])}
    d, s, props = quiet(crop.ImageCropper.crop, data.copy(), props, None if seg is None else seg.copy())
    max_cropped = float(np.nanmax(np.abs(d)))
    d = d.transpose((0, *[i + 1 for i in tf]))             # preprocessing.py:311-312
    s = s.transpose((0, *[i + 1 for i in tf]))
    resampled, _ = quiet(pre.resample_patient, np.nan_to_num(d.copy(), nan=0.0), None, np.array(original)[tf], target, 3, 1,
                         force_separate_z=None, order_z_data=0, order_z_seg=0)
    d, s, props = quiet(g.resample_and_normalize, d.copy(), target, props, s.copy(), None)
    d = d.astype(np.float32)
    assert max(d[0].size, data[0].size) <= 25000
    rec = {"input": C.digest(data), "data": t(d.copy()), "seg": t(s.astype(np.int8)), "crop_bbox": props["crop_bbox"],
           "classes": [int(v) for v in props["classes"]], "size_after_cropping": tuple(int(v) for v in props["size_after_cropping"]),
           "size_after_resampling": tuple(int(v) for v in props["size_after_resampling"]), "max_cropped": max_cropped, "sd": {}}
    for c, scheme in enumerate(schemes):
        if scheme != "CT":
            sel = s[-1] >= 0 if use_mask[c] else np.ones(s.shape[1:], bool)
            rec["sd"][c] = float(resampled[c][sel].astype(np.float64).std())
    return rec


def main():
    crop, pre = load_reference()
    out = {"scipy": scipy.__version__, "numpy": np.__version__, "crop": {}, "normalize": {}, "pipeline": {}}
    for name in C.CROP_CASES:
        out["crop"][name] = record_crop(crop, name)
    c = out["crop"]
    assert c["pocket_leaks"]["filled"] == 0 and c["pocket_diagonal"]["filled"] == C.POCKET_CELLS == c["pocket_closed"]["filled"]
    assert c["depth_one"]["filled"] == 0 and c["touches_every_face"]["filled"] == 2 * 3 * 50 and c["planar"]["filled"] > 0
    assert c["single_cell"]["bbox"] == [[3, 4], [4, 5], [7, 8]] and c["touches_every_face"]["bbox"] == [[0, 4], [0, 9], [0, 70]]
    assert c["with_seg"]["cropper"]["classes"] == [-2, -1, 0, 1, 2, 3]
    for call in C.NORM_CALLS:
        out["normalize"][call[0]] = record_normalize(pre, call)
    for cid in C.PIPE_CALLS:
        out["pipeline"][cid] = record_pipeline(crop, pre, cid)
    path = os.path.join(HERE, "reference_preprocessing.pt")
    torch.save(out, path)
    print("wrote", path, os.path.getsize(path), "bytes")
    for name, rec in out["crop"].items():
        print("crop", name, rec.get("bbox"), "filled", rec.get("filled"))
    for cid, rec in out["normalize"].items():
        print("normalize", cid, "counts", rec["counts"], "f64_gap", rec["f64_gap"])
    for cid, rec in out["pipeline"].items():
        print("pipeline", cid, tuple(rec["data"].shape), rec["crop_bbox"], rec["classes"], rec["sd"])


if __name__ == "__main__":
    main()
