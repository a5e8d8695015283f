#!/usr/bin/env python
"""Times deformablelka_amd.dataset_analysis.collect_intensity_properties on a Synapse-sized synthetic dataset against the numpy restatement
of the reference's DatasetAnalyzer (tests/dataset_analysis_ref.py) on ONE host core of the same machine, and writes
profiles/dataset_analysis_notes.md.

  dataset   --cases cases of --shape built by formula (the ellipsoid organs of scripts/time_metrics.py under a CT-like image), one modality,
            the label map last: float32 (2, *shape), as a cropped case is stored.
  device    the cases resident on the device (the upload is timed apart): count + scan + sample per case into one buffer, then moments and
            the radix select per case and for the dataset.
  baseline  the same arrays on the host: modality[mask][::10] per case, lists of float32 scalars, np.median / mean / std / min / max /
            percentile, as the reference does it.  The reference for every ratio is THIS host restatement, never the device code.

    python scripts/time_dataset_analysis.py [--skip-baseline | --baseline-only] [--shape 150 400 400] [--cases 4] [--reps 5] [--notes FILE.md]

Every device timing is a host clock between synchronisations, after a warm-up call, the median of --reps runs.  A half that was not run is
written to the notes as "not measured"."""
import argparse
import json
import os
import sys
import time
from collections import OrderedDict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402

NOTES = os.path.join(ROOT, "profiles", "dataset_analysis_notes.md")


def make_case(shape, k):
    import time_metrics
    _, lab = time_metrics.make_case(tuple(shape), shift=(0, 0, 0))
    lab = np.roll(lab, 3 * k, axis=2)                      # the cases differ
    g = np.ogrid[:shape[0], :shape[1], :shape[2]]
    img = (100.0 * np.sin(0.05 * g[2] + k) * np.cos(0.07 * g[1]) + 3.0 * g[0] - 150.0).astype(np.float32)
    return np.stack([img, lab.astype(np.float32)])


def median_ms(fn, reps, sync=None):
    times = []
    for _ in range(reps):
        if sync:
            sync()
        t0 = time.perf_counter()
        fn()
        if sync:
            sync()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def write_notes(path, res):
    def ms(key):
        return f"{res[key]:.3f} ms" if key in res else "not measured"

    ratio = f"{res['numpy_collect_ms'] / res['hip_collect_ms']:.1f}x" if "numpy_collect_ms" in res and "hip_collect_ms" in res else "not measured"
    lines = [
        "# Dataset analysis: measured times", "",
        "Written by `scripts/time_dataset_analysis.py`; what a run did not measure says so.  The baseline is the numpy restatement of the",
        "reference's `DatasetAnalyzer` (`tests/dataset_analysis_ref.py`) on one host core of the same machine.", "",
        f"Dataset: {res['cases']} cases of {' x '.join(str(v) for v in res['shape'])} cells, one modality; foreground cells per case "
        f"{res['foreground']}; samples per case {res['samples']}.", "",
        "| what | time |", "|---|---|",
        f"| `collect_intensity_properties`, cases resident on the device | {ms('hip_collect_ms')} |",
        f"| of that: count + scan + sample of every case (one read-back per case) | {ms('hip_sample_ms')} |",
        f"| of that: `compute_stats` of the dataset's concatenation (13 launches, one read-back) | {ms('hip_stats_ms')} |",
        f"| upload of all cases (pageable host memory) | {ms('upload_ms')} |",
        f"| numpy restatement on one host core | {ms('numpy_collect_ms')} |",
        f"| ratio numpy / device (cases resident) | {ratio} |",
        f"| device values equal numpy's (median, mn, mx, percentiles bitwise) | {res.get('equal_numpy', 'not measured')} |", "",
        "Not measured: datasets that do not fit the device at once, several modalities per case, label maps stored as int32, the cost of",
        "reading the cases from disk, and any rate against the memory roofline.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[150, 400, 400])
    ap.add_argument("--cases", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-baseline", action="store_true")
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--notes", default=NOTES)
    args = ap.parse_args()
    try:
        os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})      # the baseline's one core (the device path's host work too)
    except (AttributeError, OSError):
        pass
    from tests import dataset_analysis_ref as R
    arrays = OrderedDict((f"case{k}", make_case(args.shape, k)) for k in range(args.cases))
    res = {"shape": args.shape, "cases": args.cases, "reps": args.reps, "foreground": [int((a[-1] > 0).sum()) for a in arrays.values()]}
    res["samples"] = [-(-c // 10) for c in res["foreground"]]
    want = None
    if not args.skip_baseline:
        want = R.collect_intensity_properties(arrays, 1)
        res["numpy_collect_ms"] = median_ms(lambda: R.collect_intensity_properties(arrays, 1), max(1, min(args.reps, 3)))
    if not args.baseline_only:
        import torch
        from deformablelka_amd import dataset_analysis as A
        assert torch.cuda.is_available(), "the GPU half needs the MI355X"
        sync = torch.cuda.synchronize
        t0 = time.perf_counter()
        resident = OrderedDict((k, torch.from_numpy(a).cuda()) for k, a in arrays.items())
        sync()
        res["upload_ms"] = (time.perf_counter() - t0) * 1e3
        got = A.collect_intensity_properties(resident, 1)
        res["hip_collect_ms"] = median_ms(lambda: A.collect_intensity_properties(resident, 1), args.reps, sync)
        res["hip_sample_ms"] = median_ms(lambda: [A.foreground_voxels(t, 0) for t in resident.values()], args.reps, sync)
        whole = torch.cat([A.foreground_voxels(t, 0) for t in resident.values()])
        res["hip_stats_ms"] = median_ms(lambda: A.compute_stats(whole), args.reps, sync)
        if want is not None:
            keys = ("median", "mn", "mx", "percentile_99_5", "percentile_00_5")
            res["equal_numpy"] = bool(all(np.float32(got[0][k]) == np.float32(want[0][k]) for k in keys)
                                      and abs(got[0]["mean"] - float(want[0]["mean"])) <= 1e-5 * (abs(got[0]["mean"]) + got[0]["sd"]))
    print(json.dumps(res))
    write_notes(args.notes, res)


if __name__ == "__main__":
    main()
