"""Generates tests/golden/reference_augmentation2d.pt from the scipy restatement of the dummy-2D branch of the ACDC trainer's train-time
transform chain (tests/augmentation2d_ref.py: batchgenerators 0.21's augment_spatial with dim == 2 on scipy.ndimage.map_coordinates per plane
and per label, SimulateLowResolutionTransform with ignore_axes=(0,) on tests/resampling_ref.py, the colour stages of
tests/augmentation_ref.py).  batchgenerators is not needed.

The inputs are rebuilt by tests/augmentation2d_cases.py and only their SHA-256 is stored.  Per case the fixture holds what the restatement
returned, the exempt cells (source coordinate within 1e-9 of a border) and the close cells (a label's weight within 4e-6 of 0.5) as packed
bits with their counts, which this script asserts to be 0 on every case.  Tensors and plain Python values only.
Run: python tests/golden/make_golden_augmentation2d.py"""
import os
import sys

import numpy as np
import scipy
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import augmentation2d_cases as C   # noqa: E402
from tests import augmentation2d_ref as A     # noqa: E402


def packed(mask):
    return torch.from_numpy(np.packbits(np.ascontiguousarray(mask).reshape(-1)))


def to_numpy(t):
    return t.float().numpy() if t.dtype == torch.bfloat16 else t.numpy()


def main():
    out = {"scipy": scipy.__version__, "spatial": {}, "labels": {}, "tiny": {}}
    # ---- spatial values
    for cid, dtype, order, mode, variant in C.SPATIAL_CALLS:
        x = to_numpy(C.planes(C.spatial_input(dtype)))
        rec = C.spatial_record(variant)
        y, _ = A.spatial(x, None, C.PATCH, rec, order, mode, 0)
        if dtype == "bfloat16":          # the restatement computes on the bf16 values held as float64; its astype is torch's conversion
            y64, _ = A.spatial(x.astype(np.float64), None, C.PATCH, rec, order, mode, 0)
            want = torch.from_numpy(y64).to(torch.bfloat16)
        else:
            want = torch.from_numpy(y.copy())
        exempt = A.border_cells(rec, C.SRC[3:], C.PATCH, C.EPS_BORDER)[1]
        assert not exempt.any(), (cid, int(exempt.sum()))
        outside = A.outside_fraction(rec, 1, C.SRC[3:], C.PATCH)
        if variant in C.OUTSIDE:
            assert abs(outside - C.OUTSIDE[variant]) < 0.01, (cid, outside)
        out["spatial"][cid] = {"input": C.digest(x), "out": want[1].clone(), "exempt": packed(exempt), "exempt_cells": 0, "outside": outside}
        print("spatial", cid, "exempt cells", int(exempt.sum()), "outside", f"{outside:.3f}")
    # ---- spatial labels
    seg = C.planes(torch.from_numpy(C.label_input())).numpy()
    assert 3 not in np.unique(seg) and len(np.unique(seg)) == 4
    for cid, order, mode, variant in C.LABEL_CALLS:
        rec = C.spatial_record(variant)
        _, y = A.spatial(np.zeros(C.PLANES, np.float32), seg, C.PATCH, rec, 0, "constant", 0, order, mode, -1)
        close = A.label_weights_close(seg, C.PATCH, rec, C.GAP, mode, -1) if order == 1 else np.zeros(y.shape, bool)
        assert not close.any(), (cid, int(close.sum()))
        out["labels"][cid] = {"input": C.digest(seg), "out": torch.from_numpy(y.astype(np.int8)), "close": packed(close), "close_cells": 0}
        print("labels", cid, "close cells", int(close.sum()), "labels", np.unique(y).tolist(), "background", f"{float((y == 0).mean()):.3f}")
    s_h, rec_h, patch_h, want_h = C.halves_case()
    _, y = A.spatial(np.zeros(s_h.shape, np.float32), s_h, patch_h, rec_h, 0, "constant", 0, 1, "constant", -1)
    assert np.array_equal(y, want_h), "the hand-made halves case is not what the restatement returns"
    # ---- the tiny plane
    x, rec = C.tiny_case()
    x2 = x.reshape((1, 2) + C.TINY_SRC[3:])
    for mode in ("constant", "nearest"):
        y, _ = A.spatial(x2, None, C.TINY_PATCH, rec, 3, mode, 0)
        exempt = A.border_cells(rec, C.TINY_SRC[3:], C.TINY_PATCH, C.EPS_BORDER)
        assert not exempt.any() and A.outside_fraction(rec, 0, C.TINY_SRC[3:], C.TINY_PATCH) == 0
        out["tiny"][mode] = {"input": C.digest(x), "out": torch.from_numpy(y.copy()), "exempt_cells": 0}
    # ---- low resolution with ignore_axes=(0,)
    x = C.lowres_input()
    y, low_shapes = A.linear_downsampling(x, C.lowres_record(), 0, 3, ignore_axes=(0,))
    assert all(v is None or v[0] == C.LOW_SHAPE[2] for v in low_shapes.values())
    out["lowres"] = {"input": C.digest(x), "out": torch.from_numpy(y.copy()), "low_shapes": [list(v) for v in low_shapes.values() if v is not None]}
    print("lowres: low-resolution shapes", out["lowres"]["low_shapes"])
    # ---- the pipeline with the ACDC trainer's parameters
    params = C.pipeline_params()
    data, seg, noise = C.pipeline_inputs()
    rec = C.pipeline_records()
    d, t = A.more_da(data, seg, C.PIPE_PATCH, params, rec, noise, A.downsample_seg, C.DS_SCALES)
    exempt = A.border_cells(rec["spatial"], C.PIPE_SRC[3:], C.PIPE_PATCH, C.EPS_BORDER)
    assert not exempt.any(), "choose another matrix: the pipeline case has cells on a border (blur and resampling would spread them)"
    close = A.label_weights_close(C.planes(torch.from_numpy(seg)).numpy(), C.PIPE_PATCH, rec["spatial"], C.GAP, "constant", -1)
    assert not close.any(), int(close.sum())
    print("pipeline: labels", np.unique(t[0]).tolist(), "outside", A.outside_fraction(rec["spatial"], 1, C.PIPE_SRC[3:], C.PIPE_PATCH))
    out["pipeline"] = {"data": torch.from_numpy(d.copy()), "scale": float(np.abs(data).max()),
                       "target": [torch.from_numpy(np.ascontiguousarray(v)) for v in t], "exempt_cells": 0, "close_cells": 0,
                       "input": C.digest(data)}
    path = os.path.join(HERE, "reference_augmentation2d.pt")
    torch.save(out, path)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 2 ** 20


if __name__ == "__main__":
    main()
