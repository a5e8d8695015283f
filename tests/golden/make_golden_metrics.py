#!/usr/bin/env python
"""Records tests/golden/reference_metrics.pt: the cases of the metrics suites (tests/metrics_cases.py) and their float64 results from
MedPy 0.4.0's definitions restated with scipy (tests/metrics_ref.py).  Needs scipy; the GPU machine needs only the fixture.

    python tests/golden/make_golden_metrics.py

Masks are stored as uint8, label maps as uint8.  Per pair case and connectivity: dc, hd, hd95, asd, assd and the two directed distance
vectors, sorted — as exact integer squared distances (int32) with unit spacing, as float64 distances with a spacing."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import metrics_ref as R  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_metrics.pt")
SYNAPSE_CLASSES = [1, 2, 3, 4, 6, 7, 8, 11]   # inference_synapse.process_label


def ellipsoid(shape, centre, radii):
    g = np.indices(shape).astype(np.float64)
    return (sum(((g[i] - centre[i]) / radii[i]) ** 2 for i in range(len(shape))) <= 1.0).astype(np.uint8)


def pair_cases():
    """name -> (p, q, spacing, connectivities)"""
    cases = {}
    shp = (9, 70, 67)
    p = ellipsoid(shp, (4, 30, 30), (3.5, 22, 18))
    q = ellipsoid(shp, (4.5, 36, 34), (4.2, 20, 24))
    p[:3, :5, :4] = 1                                   # touches the array corner
    cases["ellipsoids_unit"] = (p, q, None, (1, 3))
    cases["ellipsoids_aniso"] = (p, q, (3.0, 0.75, 0.8), (1,))
    s = ellipsoid((40, 45), (18, 20), (12, 15))
    t = ellipsoid((40, 45), (22, 25), (15, 9))
    cases["slice_2d"] = (s, t, None, (1, 2))
    cases["slice_as_depth1_volume"] = (s[None], t[None], None, (1, 2, 3))
    cases["slice_2d_aniso"] = (s, t, (0.7, 1.9), (1,))
    cases["slice_2d_scalar_spacing"] = (s, t, 1.5, (1,))
    p = np.zeros((3, 5, 513), np.uint8)
    q = np.zeros_like(p)
    p[1, 2, 0] = 1
    q[1, 2, 512] = 1
    q[0, 0, 0] = 1
    cases["percentile_long_line"] = (p, q, None, (1,))
    z, y, x = np.indices((7, 12, 13))
    cases["diagonals"] = ((np.abs(z + y + x - 14) < 3).astype(np.uint8), (np.abs(-z - y + 2 * x - 18) < 3).astype(np.uint8), None, (1, 2, 3))
    rng = np.random.default_rng(7)
    for name, shp in (("extent1_d", (1, 23, 70)), ("extent1_h", (19, 1, 66)), ("extent1_w", (21, 67, 1)), ("below_one_wave", (3, 4, 5)),
                      ("tall_axes", (130, 9, 3))):
        dens = 0.1 if name == "tall_axes" else 0.3
        p = (rng.random(shp) < dens).astype(np.uint8)
        q = (rng.random(shp) < dens / 2).astype(np.uint8)
        cases[name] = (p, q, (1.25, 0.5, 2.0) if name == "tall_axes" else None, (1, 3))
    p = np.zeros((6, 7, 66), np.uint8)
    q = np.zeros_like(p)
    p[2, 3, 64] = 1
    q[1:5, 2:6, 3:40] = 1
    cases["single_cell"] = (p, q, None, (1,))
    full = np.ones((4, 6, 9), np.uint8)
    cases["full_against_block"] = (full, np.pad(np.ones((2, 2, 3), np.uint8), ((1, 1), (2, 2), (3, 3))), None, (1, 2))
    return cases


def label_case():
    """Prediction and label over the Synapse organs: class 4 is absent from the prediction, class 7 from both, class 6 fills the d = 0 face."""
    shp = (12, 40, 44)
    lab = np.zeros(shp, np.uint8)
    pred = np.zeros(shp, np.uint8)
    spec = {1: ((5, 10, 10), (3, 6, 7)), 2: ((6, 28, 12), (4, 5, 5)), 3: ((6, 12, 32), (3, 7, 6)), 4: ((8, 30, 34), (2, 4, 5)),
            8: ((6, 20, 22), (5, 3, 3)), 11: ((9, 33, 20), (2, 3, 8))}
    for c, (ctr, rad) in spec.items():
        lab[ellipsoid(shp, ctr, rad) > 0] = c
        if c != 4:
            pred[ellipsoid(shp, (ctr[0] + 0.6, ctr[1] - 1.3, ctr[2] + 1.1), (rad[0], rad[1] * 1.15, rad[2] * 0.9)) > 0] = c
    lab[0] = 6
    pred[0] = 6
    pred[1, 5:30] = 6
    return pred, lab


def record_pair(p, q, spacing, conns):
    out = {"p": torch.from_numpy(p), "q": torch.from_numpy(q), "spacing": spacing, "dc": float(R.dc(p, q)), "conn": {}}
    for cn in conns:
        ab, ba = np.sort(R.surface_distances(p, q, spacing, cn)), np.sort(R.surface_distances(q, p, spacing, cn))
        r = {"hd": float(R.hd(p, q, spacing, cn)), "hd95": float(R.hd95(p, q, spacing, cn)), "asd": float(R.asd(p, q, spacing, cn)),
             "assd": float(R.assd(p, q, spacing, cn))}
        if spacing is None:
            r["sq_ab"], r["sq_ba"] = torch.from_numpy(np.rint(ab ** 2).astype(np.int32)), torch.from_numpy(np.rint(ba ** 2).astype(np.int32))
            assert np.array_equal(np.sqrt(r["sq_ab"].numpy().astype(np.float64)), ab) and np.array_equal(np.sqrt(r["sq_ba"].numpy().astype(np.float64)), ba)
        else:
            r["sds_ab"], r["sds_ba"] = torch.from_numpy(ab), torch.from_numpy(ba)
        out["conn"][cn] = r
    return out


def record_labels(pred, lab, spacing):
    rows = {}
    for c in SYNAPSE_CLASSES:
        a, b = pred == c, lab == c
        both = a.any() and b.any()
        rows[c] = {"a": int(a.sum()), "b": int(b.sum()), "inter": int((a & b).sum()), "hd95": float(R.hd95(a, b, spacing, 1)) if both else None}
    return {"prediction": torch.from_numpy(pred), "label": torch.from_numpy(lab), "spacing": spacing, "classes": SYNAPSE_CLASSES, "rows": rows}


def main():
    fx = {"pairs": {name: record_pair(*c) for name, c in pair_cases().items()}, "labels": {}}
    pred, lab = label_case()
    fx["labels"]["synapse_unit"] = record_labels(pred, lab, None)
    fx["labels"]["synapse_aniso"] = record_labels(pred, lab, (3.0, 0.75, 0.8))
    torch.save(fx, OUT)
    print(OUT, os.path.getsize(OUT), "bytes")
    for name, c in fx["pairs"].items():
        print(name, tuple(c["p"].shape), {cn: (r["hd"], r["hd95"]) for cn, r in c["conn"].items()})
    for name, c in fx["labels"].items():
        print(name, {k: v["hd95"] for k, v in c["rows"].items()})


if __name__ == "__main__":
    main()
