"""Generates tests/golden/reference_dataset_analysis.pt from the REFERENCE'S OWN DatasetAnalyzer
(3D/d_lka_former/experiment_planning/DatasetAnalyzer.py, loaded from its file with batchgenerators, skimage, d_lka_former.* and
multiprocessing.Pool stubbed): _compute_stats on every sample of tests/dataset_analysis_cases.py, _check_if_all_in_one_region and
_collect_class_and_region_sizes on its label maps, and collect_intensity_properties / analyze_dataset / analyse_segmentations on its
datasets, which are written as the .npz / .pkl / dataset.json files the reference reads into a temporary folder.

skimage is not installed: ``label`` is scipy.ndimage.label with a FULL structure (skimage.measure.label's default connectivity = rank), and
returns (labelmap, num) for return_num=True as skimage does.  The Pool stub runs map / starmap in this process, in order.

Per sample: the reference's seven values as a float32 tensor, n, the SHA-256 of the input, and the gap between the reference's float32 mean /
sd and numpy's float64 values of the same sample; a gap beyond GAP_BOUND (|m64| + s64) refuses to write the fixture (the f64_gap procedure
of make_golden_preprocessing.py).  Per foreground case: the count and the SHA-256 of modality[mask][::10] taken with numpy.  Tensors and plain
values only.  Run: python tests/golden/make_golden_dataset_analysis.py"""
import importlib.util
import json
import os
import pickle
import sys
import tempfile
import types

import numpy as np
import torch
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
REF = "/root/reference"

from tests import dataset_analysis_cases as C  # noqa: E402
from tests import dataset_analysis_ref as R  # noqa: E402


class _Pool(object):
    def __init__(self, *a):
        pass

    def map(self, f, xs):
        return [f(x) for x in xs]

    def starmap(self, f, xs):
        return [f(*x) for x in xs]

    def close(self):
        pass

    def join(self):
        pass


def _label(x, return_num=False):
    lmap, n = ndimage.label(x, ndimage.generate_binary_structure(np.ndim(x), np.ndim(x)))
    return (lmap, n) if return_num else lmap


def load_reference():
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    def load_pickle(path):
        with open(path, "rb") as f:
            return pickle.load(f)

    def save_pickle(obj, path):
        with open(path, "wb") as f:
            pickle.dump(obj, f)

    def load_json(path):
        with open(path) as f:
            return json.load(f)

    for name in ("d_lka_former", "d_lka_former.preprocessing", "batchgenerators", "batchgenerators.utilities", "skimage"):
        stub(name).__path__ = []
    stub("d_lka_former.configuration", default_num_threads=1)
    stub("d_lka_former.paths", nnFormer_raw_data=None, nnFormer_cropped_data=None)
    stub("d_lka_former.preprocessing.cropping",
         get_patient_identifiers_from_cropped_files=lambda folder: sorted(f[:-4] for f in os.listdir(folder) if f.endswith(".npz")))
    stub("batchgenerators.utilities.file_and_folder_operations", join=os.path.join, isfile=os.path.isfile, load_pickle=load_pickle,
         save_pickle=save_pickle, load_json=load_json)
    stub("skimage.morphology", label=_label)
    import multiprocessing
    real_pool = multiprocessing.Pool
    multiprocessing.Pool = _Pool
    try:
        spec = importlib.util.spec_from_file_location(
            "ref_dataset_analyzer", os.path.join(REF, "3D", "d_lka_former", "experiment_planning", "DatasetAnalyzer.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        multiprocessing.Pool = real_pool
    return mod.DatasetAnalyzer


def stats_record(ref_stats, sample):
    """ref_stats: the reference's seven values of ``sample``."""
    rec = {"stats32": torch.tensor([float(v) for v in ref_stats], dtype=torch.float64).to(torch.float32), "n": int(len(sample)),
           "input": C.digest(np.asarray(sample, np.float32)), "gap_mean": float("nan"), "gap_sd": float("nan")}
    if len(sample) == 0:
        return rec
    assert all(np.asarray(v).dtype == np.float32 for v in ref_stats), [np.asarray(v).dtype for v in ref_stats]
    n, m64, s64 = R.statistics64(sample)
    if np.isfinite(m64):
        rec["gap_mean"], rec["gap_sd"] = abs(float(ref_stats[1]) - m64), abs(float(ref_stats[2]) - s64)
        assert max(rec["gap_mean"], rec["gap_sd"]) <= C.GAP_BOUND * (abs(m64) + s64), f"gap {rec} beyond the bound: the fixture is not written"
    return rec


def record_dataset(DatasetAnalyzer, name):
    cases = C.dataset(name)
    props = C.dataset_properties(cases)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for k, v in cases.items():
            np.savez_compressed(os.path.join(tmp, k + ".npz"), data=v)
            with open(os.path.join(tmp, k + ".pkl"), "wb") as f:
                pickle.dump(props[k], f)
        with open(os.path.join(tmp, "dataset.json"), "w") as f:
            json.dump(C.DATASET_JSON, f)
        an = DatasetAnalyzer(tmp, overwrite=True, num_processes=1)
        assert an.patient_identifiers == list(cases)                     # (sorted file names: the cases' order)
        results = an.collect_intensity_properties(2)
        out["structure"] = C.describe(results)
        out["sizes"] = [len(s) for s in C.samples_of(cases, 0)]
        out["whole"], out["local"] = {}, {}
        for mod in (0, 1):
            per_case = C.samples_of(cases, mod)
            out["whole"][mod] = stats_record(tuple(results[mod][k] for k in C.KEYS), np.concatenate(per_case))
            out["local"][mod] = {k: stats_record(tuple(results[mod]['local_props'][k][q] for q in C.KEYS), s) for k, s in zip(cases, per_case)}
        if name == "three":
            dp = an.analyze_dataset()
            class_dct, per_patient = an.analyse_segmentations()
            assert class_dct == C.DATASET_JSON["labels"]
            out["analyze"] = {"keys": list(dp.keys()), "structure": C.describe(dp), "all_classes": [int(c) for c in dp["all_classes"]],
                              "modalities": dict(dp["modalities"]), "size_reductions": [float(v) for v in dp["size_reductions"].values()],
                              "segmentations_structure": C.describe(per_patient)}
    return out


def main():
    DatasetAnalyzer = load_reference()
    C.check_quantile_weights()
    out = {"numpy": np.__version__, "foreground": {}, "stats": {}, "datasets": {}, "regions": {}}
    for name, build in C.FG_CASES.items():
        case = build()
        out["foreground"][name] = {"count": int((case[-1] > 0).sum()), "samples": [C.digest(R.foreground_voxels(case, m)) for m in (0, 1)]}
    for name, build in C.STAT_CASES.items():
        sample = build()
        with np.errstate(all="ignore"):
            ref = DatasetAnalyzer._compute_stats(list(sample))
        out["stats"][name] = stats_record(ref, sample)
        mine = R.compute_stats(sample)
        assert all(C.same_value(a, b) for a, b in zip(ref, mine)), name
    out["empty"] = stats_record(DatasetAnalyzer._compute_stats([]), [])
    for name in C.DATASETS:
        out["datasets"][name] = record_dataset(DatasetAnalyzer, name)
    for name, seg in C.region_maps().items():
        vol, regions = DatasetAnalyzer._collect_class_and_region_sizes(seg, C.REGION_CLASSES, C.VPV)
        one = DatasetAnalyzer._check_if_all_in_one_region(seg, C.REGIONS)
        out["regions"][name] = {"input": C.digest(seg), "volume_per_class": {int(c): float(v) for c, v in vol.items()},
                                "region_volume_per_class": {int(c): [float(v) for v in vs] for c, vs in regions.items()},
                                "all_in_one_region": {k: bool(v) for k, v in one.items()},
                                "has_classes": [int(v) for v in np.unique(seg)]}
    assert len(out["regions"]["diagonal"]["region_volume_per_class"][1]) == 1
    assert out["regions"]["snake"]["all_in_one_region"][(1,)] and not out["regions"]["random"]["all_in_one_region"][(1,)]
    path = os.path.join(HERE, "reference_dataset_analysis.pt")
    torch.save(out, path)
    print("wrote", path, os.path.getsize(path), "bytes")
    for name, rec in out["stats"].items():
        print(name, rec["n"], rec["stats32"].tolist(), rec["gap_mean"], rec["gap_sd"])
    for name, rec in out["datasets"].items():
        print(name, rec["sizes"], {m: r["stats32"].tolist() for m, r in rec["whole"].items()})


if __name__ == "__main__":
    main()
