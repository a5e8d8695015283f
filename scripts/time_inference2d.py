#!/usr/bin/env python
"""Times deformablelka_amd.inference2d on a synthetic Synapse-sized volume built by formula (148 x 512 x 512 float32, patch 224, 9 classes)
against the host baseline: the two scipy.ndimage.zoom calls test_single_volume (2D/utils.py:63-110) makes per slice, on one core.

    python scripts/time_inference2d.py [--skip-baseline | --baseline-only] [--shape 148 512 512] [--patch 224] [--classes 9] [--reps 5] [--out FILE.json]

The two halves may run on different machines (the baseline needs scipy and no GPU).  The device half times, each after one warm-up call and
between synchronisations: the zoom of all slices to the patch size with the fused Normalize (cast, two prefilter passes, evaluation), the
argmax fused with the order-0 zoom back on logits of 24 slices and of the whole volume, and predict_volume with a stand-in net
(logits_k = -|x - c_k|, elementwise torch) at slice_batch 1 and 24.  The stand-in costs next to nothing, so the two predict_volume figures
show the evaluator's own overhead per forward, not a network's."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def make_volume(shape):
    s, h, w = shape
    zz, yy, xx = np.meshgrid(np.arange(s, dtype=np.float32), np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij",
                             sparse=True)
    return (0.5 + 0.45 * np.sin(0.05 * xx + 0.1 * zz) * np.cos(0.07 * yy)).astype(np.float32)


def host_baseline(volume, patch, classes):
    from scipy.ndimage import zoom
    s, h, w = volume.shape
    labels = ((np.arange(patch)[:, None] + np.arange(patch)[None, :]) % classes).astype(np.int64)
    t_in, t_back = [], []
    for i in range(s):
        t0 = time.perf_counter()
        zoom(volume[i], (patch / h, patch / w), order=3)
        t1 = time.perf_counter()
        zoom(labels, (h / patch, w / patch), order=0)
        t2 = time.perf_counter()
        t_in.append((t1 - t0) * 1e3)
        t_back.append((t2 - t1) * 1e3)
    return t_in, t_back


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
    ap.add_argument("--patch", type=int, default=224)
    ap.add_argument("--classes", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-baseline", action="store_true")
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    volume = make_volume(args.shape)
    patch, K = args.patch, args.classes
    res = {"shape": args.shape, "patch": patch, "classes": K, "reps": args.reps}
    if not args.baseline_only:
        import torch
        from deformablelka_amd import inference2d as I2, ops
        assert torch.cuda.is_available(), "the GPU half needs the MI355X"
        dev = torch.from_numpy(volume).cuda()
        centres = torch.linspace(-1.0, 1.0, K, device="cuda").view(1, K, 1, 1)

        def net(x):
            return -(x - centres).abs()
        xy = tuple(args.shape[1:])
        zoomed = I2.zoom_slices(dev, (patch, patch), mean=0.5, std=0.5)
        idx = I2._index_tables((patch, patch), xy, dev.device)
        logits24, logits_all = net(zoomed[:24, None]), net(zoomed[:, None])
        res["hip_zoom_in_ms"] = timed(lambda: I2.zoom_slices(dev, (patch, patch), mean=0.5, std=0.5), args.reps)
        res["hip_coefficients_ms"] = timed(lambda: ops.zoom2d_coefficients(dev), args.reps)
        res["hip_argmax_zoom_back_24_ms"] = timed(lambda: ops.zoom2d_argmax(logits24, xy, idx), args.reps)
        res["hip_argmax_zoom_back_all_ms"] = timed(lambda: ops.zoom2d_argmax(logits_all, xy, idx), args.reps)
        res["hip_predict_volume_sb1_ms"] = timed(lambda: I2.predict_volume(dev, net, (patch, patch), slice_batch=1), args.reps)
        res["hip_predict_volume_sb24_ms"] = timed(lambda: I2.predict_volume(dev, net, (patch, patch), slice_batch=24), args.reps)
        pred = I2.predict_volume(dev, net, (patch, patch))
        res["last_row_and_column_zero"] = bool(not zoomed[:, -1, :].ne(-1).any() and not zoomed[:, :, -1].ne(-1).any())
        res["prediction_classes"] = torch.unique(pred).tolist()
        for k in [k for k in res if k.endswith("_ms")]:
            res[k + "_median"] = float(np.median(res[k]))
    if not args.skip_baseline:
        t_in, t_back = host_baseline(volume, patch, K)
        res.update(scipy_zoom_in_ms_per_slice_median=float(np.median(t_in)), scipy_zoom_in_ms_per_slice_min_max=[min(t_in), max(t_in)],
                   scipy_zoom_back_ms_per_slice_median=float(np.median(t_back)), scipy_zoom_back_ms_per_slice_min_max=[min(t_back), max(t_back)],
                   scipy_zoom_in_ms_volume=float(np.sum(t_in)), scipy_zoom_back_ms_volume=float(np.sum(t_back)))
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
