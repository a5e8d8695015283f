"""Generates tests/golden/reference_resampling.pt from the REFERENCE'S OWN resample_data_or_seg and resample_patient
(3D/d_lka_former/preprocessing/preprocessing.py:38-201) and lines 73-137 of save_segmentation_nifti_from_softmax
(3D/d_lka_former/inference/segmentation_export.py), loaded from their files.  The imports these never use are stubbed (SimpleITK,
batchgenerators' file helpers, the cropping module); d_lka_former.configuration is the reference's own file.  skimage and batchgenerators
are not installed: ``skimage.transform.resize`` and ``batchgenerators.augmentations.utils.resize_segmentation`` are bound to the scipy
restatement of tests/resampling_ref.py.  THAT is what this fixture pins: the reference's control flow (channel and slice loops, the separate-z
branch and its z step, the label rules, the argmax / region rule, the crop box and its clamp) on top of scipy.ndimage.map_coordinates at
(i + 0.5) * n_in / n_out - 0.5, mode 'nearest'.

The inputs are rebuilt by tests/resampling_cases.py and only their SHA-256 is stored.  Per call the fixture holds what the reference returned
(values in the dtype it returned them in, label maps as int8); for the argmax calls the uint8 argmax (or region map) of the reference's resampled probabilities and, packed
into bits, the cells whose two largest values (regions: whose distance from 0.5) are closer than 4e-6.  Tensors and plain Python values only.
Run: python tests/golden/make_golden_resampling.py"""
import copy
import importlib.util
import os
import sys
import textwrap
import types
import warnings

import numpy as np
import scipy
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import resampling_cases as C   # noqa: E402
from tests import resampling_ref as R     # noqa: E402

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
    stub("batchgenerators.utilities.file_and_folder_operations")
    stub("batchgenerators.augmentations.utils", resize_segmentation=R.resize_segmentation)
    stub("skimage.transform", resize=R.resize)
    stub("d_lka_former.preprocessing.cropping", get_case_identifier_from_npz=None, ImageCropper=None)
    from_file("d_lka_former.configuration", os.path.join(PKG, "configuration.py"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        pre = from_file("d_lka_former.preprocessing.preprocessing", os.path.join(PKG, "preprocessing", "preprocessing.py"))
    with open(os.path.join(PKG, "inference", "segmentation_export.py")) as f:
        export_lines = textwrap.dedent("".join(f.readlines()[72:137]))

    def export(segmentation_softmax, properties_dict, order=1, region_class_order=None, force_separate_z=None, interpolation_order_z=0):
        """Lines 73-137, run as they stand; also returns the resampled probabilities."""
        ns = dict(np=np, get_do_separate_z=pre.get_do_separate_z, get_lowres_axis=pre.get_lowres_axis,
                  resample_data_or_seg=pre.resample_data_or_seg, segmentation_softmax=segmentation_softmax,
                  properties_dict=copy.deepcopy(properties_dict), order=order, region_class_order=region_class_order,
                  force_separate_z=force_separate_z, interpolation_order_z=interpolation_order_z, verbose=False, resampled_npz_fname=None)
        keep = {}
        real = pre.resample_data_or_seg
        ns["resample_data_or_seg"] = lambda *a, **k: keep.setdefault("p", real(*a, **k))
        exec(compile(export_lines, "segmentation_export.py:73-137", "exec"), ns)
        return ns["seg_old_size"], keep.get("p", segmentation_softmax)

    return pre, export


def quiet(fn, *a, **k):
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def top_two_close(p):
    s = np.sort(p.astype(np.float64), 0)
    return (s[-1] - s[-2]) < C.GAP if p.shape[0] > 1 else np.zeros(p.shape[1:], bool)


def packed(mask):
    return torch.from_numpy(np.packbits(mask.reshape(-1)))


def main():
    pre, export = load_reference()
    assert pre.RESAMPLING_SEPARATE_Z_ANISO_THRESHOLD == 3
    out = {"scipy": scipy.__version__, "values": {}, "labels": {}, "argmax": {}, "regions": {}, "export": {}, "patient": {}}
    for cid, kind, case, ch, kw in C.VALUE_CALLS:
        x = C.make_input(kind, case, ch)
        y = quiet(pre.resample_data_or_seg, x, C.SHAPES[case][1], False, cval=0, **kw)
        assert y.dtype == x.dtype
        out["values"][cid] = {"input": C.digest(x), "out": torch.from_numpy(y.copy())}
    for cid in ("step_o3", "step_sep0_o3"):       # the clip bites: order 3 leaves the input's range at the steps
        x = C.make_input("step", "step")
        raw = R.resize(x[0], C.SHAPES["step"][1], 3, clip=False) if cid == "step_o3" else None
        if raw is not None:
            assert raw.max() > x.max() + 1.0 and raw.min() < x.min() - 1.0
        y = out["values"][cid]["out"].numpy()
        assert y.max() == x.max() and y.min() == x.min()
    for cid, kind, case, ch, kw in C.LABEL_CALLS:
        x = C.make_input(kind, case, ch)
        y = quiet(pre.resample_data_or_seg, x, C.SHAPES[case][1], True, cval=-1, **kw)
        assert y.dtype == x.dtype
        assert y.min() >= -128 and y.max() < 128
        out["labels"][cid] = {"input": C.digest(x), "out": torch.from_numpy(y.astype(np.int8))}
    for cid, kind, case, ch, kw in C.ARGMAX_CALLS:
        x = C.make_input(kind, case, ch)
        p = quiet(pre.resample_data_or_seg, x.astype(np.float64), C.SHAPES[case][1], False, cval=0, **kw)
        if kind == "tie":          # two identical planes: numpy takes the first; one value instead of a map
            assert (p.argmax(0) == 3).all() and (p[3] == p[7]).all()
            out["argmax"][cid] = {"input": C.digest(x), "argmax_everywhere": 3}
            continue
        out["argmax"][cid] = {"input": C.digest(x), "argmax": torch.from_numpy(p.argmax(0).astype(np.uint8)), "close": packed(top_two_close(p))}
    for cid, kind, case, ch, kw, regions in C.REGION_CALLS:
        x = C.make_input(kind, case, ch)
        p = quiet(pre.resample_data_or_seg, x.astype(np.float64), C.SHAPES[case][1], False, cval=0, **kw)
        seg = np.zeros(p.shape[1:])
        for i, c in enumerate(regions):          # segmentation_export.py:122-124
            seg[p[i] > 0.5] = c
        out["regions"][cid] = {"input": C.digest(x), "argmax": torch.from_numpy(seg.astype(np.uint8)),
                               "close": packed((np.abs(p - 0.5) < C.GAP).any(0))}
    for cid, kind, case, props, kw in C.EXPORT_CALLS:
        x = C.make_input(kind, case)
        seg, p = quiet(export, x.astype(np.float64), props, **kw)
        if kw.get("region_class_order") is None:
            close = top_two_close(p)
        else:
            close = (np.abs(p - 0.5) < C.GAP).any(0)
        full = np.zeros(seg.shape, bool)
        bbox = props["crop_bbox"]
        if bbox is None:
            full[...] = close
        else:
            lo = [b[0] for b in bbox]
            full[lo[0]:lo[0] + close.shape[0], lo[1]:lo[1] + close.shape[1], lo[2]:lo[2] + close.shape[2]] = close
        out["export"][cid] = {"input": C.digest(x), "argmax": torch.from_numpy(seg.astype(np.uint8)), "close": packed(full)}
    for cid, case, original, target, kw in C.PATIENT_CALLS:
        data, seg = C.make_input("image", case), C.make_input("labels_neg", case, (0, 1))
        d, s = quiet(pre.resample_patient, data, seg, original, target, **kw)
        out["patient"][cid] = {"input": C.digest(data), "data": torch.from_numpy(d.copy()), "seg": torch.from_numpy(s.copy())}
    e = out["export"]
    assert tuple(e["clamp"]["argmax"].shape) == (8, 20, 17) and not e["clamp"]["argmax"][:2].any() and e["clamp"]["argmax"][2:, 6:].any()
    path = os.path.join(HERE, "reference_resampling.pt")
    torch.save(out, path)
    print("wrote", path, os.path.getsize(path), "bytes")
    for sec in ("argmax", "regions", "export"):
        for cid, rec in out[sec].items():
            if "argmax" not in rec:
                continue
            n = rec["argmax"].numel()
            print(sec, cid, tuple(rec["argmax"].shape), "close cells:", int(np.unpackbits(rec["close"].numpy())[:n].sum()), "of", n)


if __name__ == "__main__":
    main()
