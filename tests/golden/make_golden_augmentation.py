"""Generates tests/golden/reference_augmentation.pt from the scipy restatement of the 3-D trainer's train-time transform chain
(tests/augmentation_ref.py: batchgenerators 0.21's rules on scipy.ndimage.map_coordinates, scipy.ndimage.gaussian_filter and
tests/resampling_ref.py).  batchgenerators is not installed: it is stubbed the way make_golden_resampling.py stubs it, so that the REFERENCE'S
OWN files can be loaded for what they define themselves: ``downsample_seg_for_ds_transform2`` (training/data_augmentation/downsampling.py:88),
``default_3D_augmentation_params`` (default_data_augmentation.py:35) and the values ``setup_DA_params`` writes over them
(d_lka_former_trainer_synapse.py:383-435, read from its lines).

The inputs are rebuilt by tests/augmentation_cases.py and only their SHA-256 is stored.  Per case the fixture holds what the restatement
returned, the exempt cells (source coordinate within 1e-9 of a border, 'constant') or the close cells (a label's weight within 4e-6 of 0.5) as
packed bits, and the parameter values read from the reference.  Tensors and plain Python values only.  It also MEASURES the float32
restatements behind BLUR_K and POINTWISE_K (augmentation_cases.py) and prints them.
Run: python tests/golden/make_golden_augmentation.py"""
import importlib.util
import os
import re
import sys
import types

import numpy as np
import scipy
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import augmentation_cases as C   # noqa: E402
from tests import augmentation_ref as A     # noqa: E402
from tests import resampling_ref as R       # noqa: E402

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

    class Anything:
        def __init__(self, *a, **k):
            pass

    for name in ("batchgenerators", "batchgenerators.augmentations", "batchgenerators.transforms", "batchgenerators.dataloading"):
        stub(name).__path__ = []
    stub("batchgenerators.augmentations.utils", resize_segmentation=R.resize_segmentation, convert_seg_image_to_one_hot_encoding_batched=None)
    sys.modules["batchgenerators.transforms"].AbstractTransform = Anything
    down = from_file("ref_downsampling", os.path.join(PKG, "training", "data_augmentation", "downsampling.py"))
    # default_data_augmentation.py imports the whole transform zoo; the dict is a literal: evaluate lines 35-90 alone
    with open(os.path.join(PKG, "training", "data_augmentation", "default_data_augmentation.py")) as f:
        src = f.read()
    body = src[src.index("default_3D_augmentation_params = {"):]
    body = body[:body.index("\n}") + 2]
    ns = {"np": np, "os": os}
    exec(compile(body, "default_data_augmentation.py:35-90", "exec"), ns)
    params = ns["default_3D_augmentation_params"]
    # setup_DA_params: the assignments of constants to self.data_aug_params in the 3-D branch
    with open(os.path.join(PKG, "training", "network_training", "d_lka_former_trainer_synapse.py")) as f:
        lines = f.readlines()[382:436]
    for line in lines:
        m = re.match(r"\s+self\.data_aug_params\[['\"](\w+)['\"]\] = (.+)$", line)
        if m and m.group(1) in ("rotation_x", "rotation_y", "rotation_z", "scale_range", "do_elastic", "selected_seg_channels") \
                and "default_2D" not in m.group(2):
            params[m.group(1)] = eval(m.group(2), {"np": np})
    return down.downsample_seg_for_ds_transform2, params


def packed(mask):
    return torch.from_numpy(np.packbits(np.ascontiguousarray(mask).reshape(-1)))


def to_numpy(t):
    return t.float().numpy() if t.dtype == torch.bfloat16 else t.numpy()


def plain(v):
    if isinstance(v, tuple):
        return [plain(i) for i in v]
    if isinstance(v, (np.floating, np.integer)):
        return v.item()
    return v


def main():
    downsample, ref_params = load_reference()
    out = {"scipy": scipy.__version__, "spatial": {}, "labels": {}, "blur": {}, "point": {}}
    # ---- spatial values
    for cid, dtype, order, mode, scale in C.SPATIAL_CALLS:
        t = C.spatial_input(dtype)
        x = to_numpy(t)
        rec = C.spatial_record(scale)
        y, _ = A.spatial(x, None, C.PATCH, rec, order, mode, 0)
        if dtype == "bfloat16":          # the restatement computes on the bf16 values held as float32; its astype is torch's conversion
            y64, _ = A.spatial(x.astype(np.float64), None, C.PATCH, rec, order, mode, 0)
            want = torch.from_numpy(y64).to(torch.bfloat16)
        else:
            want = torch.from_numpy(y.copy())
        exempt = A.border_cells(rec, C.SRC[2:], C.PATCH, C.EPS_BORDER)[1]
        assert exempt.mean() <= 0.001, (cid, exempt.mean())
        out["spatial"][cid] = {"input": C.digest(x), "out": want[1].clone(), "exempt": packed(exempt)}
        outside = (~np.isfinite(y[1].astype(float))).sum()
        print("spatial", cid, "exempt cells", int(exempt.sum()), "nan", int(outside), "zeros", float((y[1] == 0).mean()))
    # ---- spatial labels
    seg = C.label_input()
    for cid, order, mode, scale in C.LABEL_CALLS:
        rec = C.spatial_record(scale)
        _, y = A.spatial(np.zeros(C.SRC, np.float32), seg, C.PATCH, rec, 0, "constant", 0, order, mode, -1)
        close = A.label_weights_close(seg, C.PATCH, rec, C.GAP, mode, -1) if order == 1 else np.zeros(y.shape, bool)
        assert close.mean() <= 0.01
        assert 3 not in np.unique(seg) and len(np.unique(seg)) == 4
        out["labels"][cid] = {"input": C.digest(seg), "out": torch.from_numpy(y.astype(np.int8)), "close": packed(close), "absent_label": 3}
        print("labels", cid, "close cells", int(close.sum()), "of", close.size, "labels", np.unique(y).tolist(),
              "cells without a majority (0 from no label)", float((y == 0).mean()))
    s_h, rec_h, patch_h, want_h = C.halves_case()
    _, y = A.spatial(np.zeros(s_h.shape, np.float32), s_h, patch_h, rec_h, 0, "constant", 0, 1, "constant", -1)
    assert np.array_equal(y, want_h), "the hand-made halves case is not what the restatement returns"
    # ---- blur
    worst = 0.0
    for name, shape in C.BLUR_SHAPES.items():
        x = C.image(shape, 6)
        for i, rec in enumerate(C.blur_records()):
            y = A.gaussian_blur(x, rec)
            y32 = A.gaussian_blur_float32(x, rec)
            units = np.abs(y32.astype(np.float64) - y).max() / (2.0 ** -24 * np.abs(x).max())
            worst = max(worst, units)
            out["blur"][f"{name}_{i}"] = {"input": C.digest(x), "out": torch.from_numpy(y.copy())}
    print(f"blur: float32 restatement is off by at most {worst:.2f} units of 2^-24 max|x| (BLUR_K = {C.BLUR_K})")
    assert worst < C.BLUR_K
    # ---- point-wise stages
    x = C.point_input()
    noise = C.point_noise()
    r = C.point_records()
    out["point"]["input"] = C.digest(x)
    stage_out = {
        "noise": A.gaussian_noise(x, r["noise"], noise), "brightness": A.brightness_multiplicative(x, r["brightness"]),
        "additive": A.brightness_additive(x, r["additive"]), "contrast": A.contrast(x, r["contrast"]),
        "gamma": A.gamma(x, r["gamma"], False, False), "gamma_retain": A.gamma(x, r["gamma"], False, True),
        "gamma_inverted": A.gamma(x, r["gamma"], True, False), "gamma_inverted_retain": A.gamma(x, r["gamma"], True, True)}
    for k, y in stage_out.items():
        assert np.array_equal(y[1], x[1]) and np.isfinite(y).all()
        out["point"][k] = {"out": torch.from_numpy(y[0].copy())}
    c = r["chain"]

    def chain(v, f32):
        fn = (lambda a: a.astype(np.float32)) if f32 else (lambda a: a)
        if not f32:
            y = A.gaussian_noise(v, c["noise"], noise)
            y = A.brightness_multiplicative(y, c["brightness"])
            y = A.contrast(y, c["contrast"])
            y = A.gamma(y, c["gamma_inverted"], True, True)
            y = A.gamma(y, c["gamma"], False, True)
            return y
        # the float32 restatement: the same stages with float32 arithmetic and float32 statistics
        y = v + noise
        y = y * c["brightness"]["multiplier"].astype(np.float32)[:, :, None, None, None]
        for b in range(2):
            for ch in range(2):
                z = y[b, ch]
                m = z.mean(dtype=np.float32)
                y[b, ch] = np.clip((z - m) * np.float32(c["contrast"]["factor"][b, ch]) + m, z.min(), z.max())
        for key, inv in (("gamma_inverted", True), ("gamma", False)):
            for b in range(2):
                for ch in range(2):
                    z = -y[b, ch] if inv else y[b, ch]
                    m, sd = z.mean(dtype=np.float32), z.std(dtype=np.float32)
                    lo, rng = z.min(), z.max() - z.min()
                    z = np.power((z - lo) / np.float32(rng + np.float32(1e-7)), np.float32(c[key]["gamma"][b, ch])) * rng + lo
                    z = z - z.mean(dtype=np.float32)
                    z = z / (z.std(dtype=np.float32) + np.float32(1e-8)) * sd + m
                    y[b, ch] = -z if inv else z
        return fn(y)

    y = chain(x, False)
    y32 = chain(x.copy(), True)
    assert y32.dtype == np.float32
    units = np.abs(y32.astype(np.float64) - y).max() / (2.0 ** -24 * np.abs(x).max())
    print(f"point-wise chain: float32 restatement is off by at most {units:.2f} units of 2^-24 max|x| (POINTWISE_K = {C.POINTWISE_K})")
    y, _ = A.mirroring(y, None, c["mirror"])
    assert np.isfinite(y).all()
    out["point"]["chain"] = {"out": torch.from_numpy(y.copy())}
    z0 = stage_out["contrast"][0, 0]
    assert (z0 == x[0, 0].min()).sum() > 1 and (z0 == x[0, 0].max()).sum() > 1
    # ---- deep-supervision targets: the reference's own function
    seg = C.blocky_labels(C.DS_SHAPE, 12, labels=(0, 1, 2, 5), block=2).astype(np.float32)
    out["ds"] = {"input": C.digest(seg), "out": [torch.from_numpy(np.ascontiguousarray(t)) for t in downsample(seg, C.DS_SCALES, 0, 0)]}
    # ---- the pipeline with the trainer's parameters
    mine = C.pipeline_params()
    for k, v in mine.items():
        assert plain(ref_params[k]) == plain(v), f"{k}: the reference has {ref_params[k]!r}, the cases have {v!r}"
    data, seg, noise = C.pipeline_inputs()
    rec = C.pipeline_records()
    d, t = A.more_da(data, seg, C.PIPE_PATCH, mine, rec, noise, downsample, C.DS_SCALES)
    exempt = np.zeros(d.shape, bool)
    exempt[:, 0] = A.border_cells(rec["spatial"], C.PIPE_SRC[2:], C.PIPE_PATCH, C.EPS_BORDER)
    assert not exempt.any(), "choose another matrix: the pipeline case has cells on a border (blur and resampling would spread them)"
    close = A.label_weights_close(seg, C.PIPE_PATCH, rec["spatial"], C.GAP, "constant", -1)
    close, _ = A.mirroring(close, None, rec["mirror"])
    print("pipeline: close label cells", int(close.sum()), "labels", np.unique(t[0]).tolist())
    out["pipeline"] = {"params": {k: plain(v) for k, v in mine.items()}, "data": torch.from_numpy(d.copy()), "scale": float(np.abs(data).max()),
                       "target": [torch.from_numpy(np.ascontiguousarray(v)) for v in t], "exempt": packed(exempt), "close": packed(close),
                       "input": C.digest(data)}
    path = os.path.join(HERE, "reference_augmentation.pt")
    torch.save(out, path)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 2 ** 20


if __name__ == "__main__":
    main()
