#!/usr/bin/env python
"""Times deformablelka_amd.metrics.evaluate_label_maps on a synthetic Synapse-sized case (148 x 512 x 512, the eight organs of
inference_synapse.process_label as ellipsoids, the prediction a perturbed copy) against the host baseline: MedPy's definitions restated with
scipy (tests/metrics_ref.py), one organ after the other on the whole volume, as the reference's evaluators run them.

    python scripts/time_metrics.py [--skip-baseline | --baseline-only] [--shape 148 512 512] [--reps 5] [--out FILE.json]

The two halves may run on different machines (the baseline needs scipy and no GPU).  For the per-kernel split run the GPU half under
`rocprofv3 --kernel-trace --stats -- python scripts/time_metrics.py --skip-baseline --reps 1`."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

CLASSES = [1, 2, 3, 4, 6, 7, 8, 11]
# centre and radii as fractions of the extents: spleen, right kidney, left kidney, gallbladder, liver, stomach, aorta, pancreas
ORGANS = {1: ((.55, .55, .75), (.16, .09, .08)), 2: ((.40, .62, .33), (.13, .06, .05)), 3: ((.40, .62, .67), (.13, .06, .05)),
          4: ((.50, .40, .38), (.06, .04, .03)), 6: ((.58, .45, .30), (.24, .18, .17)), 7: ((.60, .38, .62), (.12, .10, .09)),
          8: ((.50, .55, .50), (.45, .025, .025)), 11: ((.47, .48, .52), (.05, .04, .10))}


def make_case(shape, shift=(1.5, -3.0, 2.0), scale=(1.0, 1.06, 0.95)):
    g = np.ogrid[:shape[0], :shape[1], :shape[2]]
    lab, pred = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    for c in sorted(ORGANS, key=lambda c: c != 6):   # the liver first: the small organs are painted over it
        ctr, rad = ORGANS[c]
        cc, rr = [ctr[i] * shape[i] for i in range(3)], [max(rad[i] * shape[i], 1.0) for i in range(3)]
        lab[sum(((g[i] - cc[i]) / rr[i]) ** 2 for i in range(3)) <= 1.0] = c
        pred[sum(((g[i] - cc[i] - shift[i]) / (rr[i] * scale[i])) ** 2 for i in range(3)) <= 1.0] = c
    return pred, lab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[148, 512, 512])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-baseline", action="store_true")
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pred, lab = make_case(tuple(args.shape))
    res = {"shape": args.shape, "classes": CLASSES}
    if not args.baseline_only:
        import torch
        from deformablelka_amd import metrics
        assert torch.cuda.is_available(), "the GPU half needs the MI355X"
        p, q = torch.from_numpy(pred).cuda(), torch.from_numpy(lab).cuda()
        out = metrics.evaluate_label_maps(p, q, CLASSES)   # warm-up
        times = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = metrics.evaluate_label_maps(p, q, CLASSES)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        metrics.evaluate_label_maps(pred, lab, CLASSES)
        res["hip_ms_from_host_arrays"] = (time.perf_counter() - t0) * 1e3
        res.update(hip_ms=times, hip_ms_median=float(np.median(times)), hip_dice=out["dice"].tolist(), hip_hd95=out["hd95"].tolist())
    if not args.skip_baseline:
        from tests import metrics_ref as R
        t0 = time.perf_counter()
        dice, h95 = [], []
        for c in CLASSES:
            dice.append(float(R.dc(pred == c, lab == c)))
            h95.append(float(R.hd95(pred == c, lab == c)))
        res.update(scipy_ms=(time.perf_counter() - t0) * 1e3, scipy_dice=dice, scipy_hd95=h95)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
