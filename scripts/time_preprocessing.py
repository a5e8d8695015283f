#!/usr/bin/env python
"""Times deformablelka_amd.preprocessing on a synthetic Synapse-sized case built by formula (1 x 148 x 512 x 512 float32: an elliptic "body" of
CT-like values with enclosed zero pockets, zeros around it) against the host baseline: the reference's algorithm (cropping.py:23-116 and the
CT branch of preprocessing.py:276-286) restated with scipy.ndimage.binary_fill_holes and numpy on one core.

    python scripts/time_preprocessing.py [--skip-baseline | --baseline-only] [--shape 148 512 512] [--reps 5] [--out FILE.json]

The two halves may run on different machines (the baseline needs scipy and no GPU).  The device half times the crop, the normalisation and the
whole preprocess_arrays (crop, order-3 resampling from spacing (3.0, 0.76, 0.76) to (2.0, 1.0, 1.0) with a separate z, CT normalisation) on a
device tensor, each after one warm-up call, between synchronisations."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

CT = {'mean': 77.5, 'sd': 142.1, 'percentile_00_5': -958.0, 'percentile_99_5': 326.7}
ORIGINAL, TARGET = (3.0, 0.76, 0.76), (2.0, 1.0, 1.0)


def make_case(shape):
    d, h, w = shape
    zz, yy, xx = np.meshgrid(np.arange(d, dtype=np.float32), np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij",
                             sparse=True)
    body = ((yy - h / 2) / (h * 0.40)) ** 2 + ((xx - w / 2) / (w * 0.45)) ** 2 <= 1.0
    body = body & (zz >= 4) & (zz < d - 4)
    values = (100.0 * np.sin(0.05 * xx) * np.cos(0.07 * yy) + 3.0 * zz - 150.0).astype(np.float32)
    values = np.where(values == 0, np.float32(1.0), values)
    pockets = ((zz % 16) >= 6) & ((zz % 16) < 10) & ((yy % 64) >= 24) & ((yy % 64) < 40) & ((xx % 64) >= 24) & ((xx % 64) < 40)
    return np.where(body & ~pockets, values, np.float32(0.0))[None].astype(np.float32)


def host_baseline(data):
    from scipy.ndimage import binary_fill_holes
    t0 = time.perf_counter()
    mask = np.zeros(data.shape[1:], dtype=bool)
    for c in range(data.shape[0]):
        mask = mask | (data[c] != 0)
    mask = binary_fill_holes(mask)
    coords = np.where(mask != 0)
    bbox = [[int(np.min(c)), int(np.max(c)) + 1] for c in coords]
    box = tuple(slice(lo, hi) for lo, hi in bbox)
    cropped = np.vstack([data[c][box][None] for c in range(data.shape[0])])
    seg = mask[box][None].astype(int)
    seg[seg == 0] = -1
    seg[seg > 0] = 0
    t1 = time.perf_counter()
    out = cropped.copy()
    for c in range(len(out)):
        out[c] = np.clip(out[c], CT['percentile_00_5'], CT['percentile_99_5'])
        out[c] = (out[c] - CT['mean']) / CT['sd']
    t2 = time.perf_counter()
    return bbox, int(mask.sum()), (t1 - t0) * 1e3, (t2 - t1) * 1e3


def timed(fn, reps):
    import torch
    fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[148, 512, 512])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-baseline", action="store_true")
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    data = make_case(args.shape)
    res = {"shape": args.shape}
    if not args.baseline_only:
        import torch
        from deformablelka_amd import preprocessing as P
        assert torch.cuda.is_available(), "the GPU half needs the MI355X"
        dev = torch.from_numpy(data).cuda()
        pre = P.GenericPreprocessor({0: "CT"}, {0: False}, [0, 1, 2], {0: CT})
        props = {"original_spacing": np.array(ORIGINAL)}
        cropped, seg, bbox = P.crop_to_nonzero(dev)
        res.update(hip_bbox=bbox, hip_mask_cells=int(P.create_nonzero_mask(dev).sum()))
        res["hip_crop_ms"] = timed(lambda: P.crop_to_nonzero(dev), args.reps)
        res["hip_normalize_ms"] = timed(lambda: pre.normalize(cropped, seg), args.reps)
        res["hip_preprocess_arrays_ms"] = timed(lambda: pre.preprocess_arrays(dev, TARGET, props), args.reps)
        t0 = time.perf_counter()
        out, _, _ = pre.preprocess_arrays(data, TARGET, props)
        res["hip_preprocess_arrays_ms_from_host_arrays"] = (time.perf_counter() - t0) * 1e3
        res["out_shape"] = list(out.shape)
        for k in ("hip_crop_ms", "hip_normalize_ms", "hip_preprocess_arrays_ms"):
            res[k + "_median"] = float(np.median(res[k]))
    if not args.skip_baseline:
        bbox, cells, crop_ms, norm_ms = host_baseline(data)
        res.update(scipy_bbox=bbox, scipy_mask_cells=cells, scipy_crop_ms=crop_ms, numpy_normalize_ms=norm_ms)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
