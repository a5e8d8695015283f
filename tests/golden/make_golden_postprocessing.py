"""Generates tests/golden/reference_postprocessing.pt from the REFERENCE'S OWN remove_all_but_the_largest_connected_component
(3D/d_lka_former/postprocessing/connected_components.py:48-105, loaded from its file with the imports it never uses for this function stubbed:
SimpleITK, batchgenerators, d_lka_former.configuration / evaluation.evaluator / utilities.sitk_stuff) and from scipy.ndimage.label.

Per case: the label map; under "label", per connectivity the object map of (map != 0) (uint8 or int16 where the count allows), the object count and the
object sizes; under "remove", per call the arguments and the reference's filtered map (as uint8: every class id is below 256) and two dicts.  Tensors and plain Python values only.
The shapes are the smallest at which the kernels of csrc/cl_conn_comp.hip can go wrong: tiles are 4 x 8 x 64 (depth 1: 1 x 32 x 64; a single
line: 1 x 1 x 2048), flatten / rank blocks are 2048 cells.
Run: python tests/golden/make_golden_postprocessing.py"""
import importlib.util
import os
import sys
import types

import numpy as np
import scipy
import torch
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
VPV = 0.75 * 0.75 * 3.0


def load_reference():
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    for name in ("d_lka_former", "d_lka_former.evaluation", "d_lka_former.utilities", "batchgenerators", "batchgenerators.utilities"):
        stub(name).__path__ = []
    stub("d_lka_former.configuration", default_num_threads=1)
    stub("d_lka_former.evaluation.evaluator", aggregate_scores=None)
    stub("d_lka_former.utilities.sitk_stuff", copy_geometry=None)
    stub("batchgenerators.utilities.file_and_folder_operations")
    if "SimpleITK" not in sys.modules:
        stub("SimpleITK")
    spec = importlib.util.spec_from_file_location(
        "ref_connected_components", os.path.join(REF, "3D", "d_lka_former", "postprocessing", "connected_components.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.remove_all_but_the_largest_connected_component


def runs_line(n):
    """Runs of lengths 1, 2, 3, ... separated by single background cells."""
    line, pos, k = np.zeros(n, np.uint8), 0, 1
    while pos < n:
        line[pos:pos + k] = 1
        pos += k + 1
        k += 1
    return line


def build_cases():
    rng = np.random.default_rng(20240611)
    cases = {}

    # near the percolation threshold of the joint region: thousands of objects, extents no multiple of any tile
    u = rng.random((5, 37, 130))
    cases["random"] = np.select([u < 0.12, u < 0.24, u < 0.30], [1, 2, 3], 0).astype(np.int16)

    # a 1-cell-wide snake of class 1 in plane 0 that crosses the tile faces along w in every row and those along h every 8 rows, and a shorter
    # one of class 2 in plane 1 (columns instead of rows): one object each; the joint region (1, 2) is one object
    s = np.zeros((2, 33, 129), np.uint8)
    s[0, 0::2, :] = 1
    s[0, 1::4, 128] = 1
    s[0, 3::4, 0] = 1
    s[1, :, 0:97:4] = 2
    for k, w in enumerate(range(0, 96, 4)):   # columns w and w + 4 are linked at the bottom and at the top in turn
        s[1, 32 if k % 2 == 0 else 0, w + 1:w + 4] = 2
    cases["serpentine"] = s

    # a "U" whose arms meet only in row 35 (the second tile row), an "n" and a blob that start between the arms: numbering follows the first cell
    j = np.zeros((40, 70), np.uint8)
    j[0:36, 5] = 1
    j[0:36, 66] = 1
    j[35, 5:67] = 1
    j[3, 15:31] = 1
    j[3:21, 15] = 1
    j[3:21, 30] = 1
    j[10:13, 40:46] = 1
    cases["late_join"] = j

    # cubes A, B share only an edge, C, D only a corner: 4 / 3 / 2 objects at connectivity 1 / 2 / 3
    t = np.zeros((8, 8, 8), np.int32)
    t[0:2, 0:2, 0:2] = 1
    t[0:2, 2:4, 2:4] = 1
    t[4:6, 4:6, 4:6] = 1
    t[6:8, 6:8, 6:8] = 1
    cases["diagonal_touch"] = t

    # three objects of class 2, two of the largest size
    e = np.zeros((3, 9, 20), np.int64)
    e[0, 1:3, 1:4] = 2
    e[2, 5:8, 10:12] = 2
    e[1, 4, 15:18] = 2
    e[1, 0, 0] = 1
    cases["ties"] = e

    cases["all_background"] = np.zeros((3, 5, 70), np.uint8)
    full = np.full((3, 10, 70), 2, np.uint8)
    cases["class_fills_the_array"] = full
    cases["single_cell"] = np.ones((1,), np.uint8)
    cases["line_513"] = (rng.random(513) < 0.6).astype(np.uint8) * 3
    r2 = rng.random((67, 131))
    cases["image_67x131"] = np.select([r2 < 0.3, r2 < 0.58], [1, 2], 0).astype(np.uint8)
    cases["width_one"] = (rng.random((9, 70, 1)) < 0.6).astype(np.int16)
    # contiguous lines longer than one tile's span: 150 > 64 (depth 1), 4500 > 2048 (a single line)
    ll = np.zeros((1, 3, 150), np.uint8)
    ll[0, 0] = runs_line(150)
    ll[0, 2] = runs_line(150)[::-1]
    cases["long_line_150"] = ll
    cases["long_line_4500"] = runs_line(4500)
    return cases


REMOVE_CALLS = {
    "random": [([(1, 2), 3, 2], VPV, {(1, 2): 40.0, 3: 10.0, 2: 5.0}), ([(1, 2), 3, 2], VPV, None), (None, VPV, None)],
    "serpentine": [([1, 2], 1.0, None), ([(1, 2)], 1.0, None)],
    "late_join": [([1], 0.5, None)],
    "diagonal_touch": [([1], 1.0, None)],
    "ties": [([2], 2.0, None), ([2, 1, 7], 2.0, {2: 1.0, 1: 1.0, 7: 1.0})],
    "all_background": [(None, 1.0, None), ([1, (2, 3)], 1.0, None)],
    "class_fills_the_array": [([2], 1.5, None)],
    "single_cell": [([1], 1.0, None)],
    "line_513": [([3], 1.0, None), ([3], 1.0, {3: 3.0})],
    "image_67x131": [([1, 2], 1.0, None), ([(1, 2)], 0.1, {(1, 2): 0.3})],
    "width_one": [([1], 1.0, None)],
    "long_line_150": [([1], 1.0, {1: 9.0})],
    "long_line_4500": [([1], 1.0, {1: 50.0})],
}


def main():
    ref_remove = load_reference()
    out = {"scipy": scipy.__version__, "cases": {}}
    for name, image in build_cases().items():
        case = {"image": torch.from_numpy(image.copy()), "label": {}, "remove": []}
        for cn in range(1, image.ndim + 1):
            lmap, n = ndimage.label(image != 0, ndimage.generate_binary_structure(image.ndim, cn))
            sizes = np.bincount(lmap.ravel(), minlength=n + 1)[1:]
            case["label"][cn] = {"labels": torch.from_numpy(lmap.astype(np.uint8 if n < 2 ** 8 else np.int16 if n < 2 ** 15 else np.int32)), "num": int(n),
                                 "sizes": torch.from_numpy(sizes.astype(np.int64))}
        for classes, vpv, mins in REMOVE_CALLS[name]:
            img, removed, kept = ref_remove(image.copy(), classes, vpv, mins)
            plain = lambda d: {(k if isinstance(k, tuple) else int(k)): (None if v is None else float(v)) for k, v in d.items()}
            case["remove"].append({"classes": classes, "vpv": vpv, "min": mins, "image": torch.from_numpy(img.astype(np.uint8)),
                                   "largest_removed": plain(removed), "kept_size": plain(kept)})
        out["cases"][name] = case
    c = out["cases"]
    counts = [c["random"]["label"][cn]["num"] for cn in (1, 2, 3)]
    assert len(set(counts)) == 3, counts
    first = c["random"]["remove"][0]
    assert any(v is not None for v in first["largest_removed"].values())
    assert [c["diagonal_touch"]["label"][cn]["num"] for cn in (1, 2, 3)] == [4, 3, 2]
    assert c["serpentine"]["label"][1]["num"] == 1 and all(v is None for v in c["serpentine"]["remove"][0]["largest_removed"].values())
    assert c["late_join"]["label"][1]["num"] == 3
    path = os.path.join(HERE, "reference_postprocessing.pt")
    torch.save(out, path)
    print("wrote", path, os.path.getsize(path), "bytes; random-case object counts", counts)
    for name, case in c.items():
        print(name, tuple(case["image"].shape), {cn: v["num"] for cn, v in case["label"].items()},
              [(r["largest_removed"], r["kept_size"]) for r in case["remove"]])


if __name__ == "__main__":
    main()
