#!/usr/bin/env python
"""Times deformablelka_amd.dataloading at the Synapse trainer's sizes against the host path it replaces.

  batch            one DataLoader3D.generate_train_batch: B = 2, C = 1, the patch get_patch_size yields for (64, 128, 128) with the trainer's
                   rotation (+-30 degrees on every axis) and scale range ((0.85, 1.25) when it is called, d_lka_former_trainer_synapse.py:397-427),
                   oversample_foreground_percent 0.33, pad_mode 'constant', on --cases resident cases of --shape built by formula (the
                   ellipsoid organs of scripts/time_metrics.py under a CT-like image).  The host draw and the device apply are timed apart.
  class_locations  for one such case, the 13 Synapse organ labels asked for (the ellipsoids paint 8 of them), default parameters; the
                   permutation numpy draws on the host (RandomState.choice without replacement) is timed apart: it is part of both paths.
  baselines        on ONE host core of the same machine: tests/dataloading_ref.py's numpy batch (the reference's slices and np.pad) plus the
                   upload of the batch, and the reference's K-pass np.argwhere with the same draws.

    python scripts/time_dataloading.py [--skip-baseline | --baseline-only] [--shape 150 400 400] [--cases 4] [--reps 20] [--out FILE.json]

Every device timing is a host clock between synchronisations, after warm-up calls, medians of --reps runs; the draws are re-seeded so that
both paths cut the same boxes, and the batches are compared bit for bit."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402

FINAL = (64, 128, 128)
R30 = 30. / 360 * 2. * np.pi
ALL_CLASSES = list(range(1, 14))


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
    return float(np.median(times)), [round(t, 4) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[150, 400, 400])
    ap.add_argument("--cases", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-baseline", action="store_true")
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    try:
        os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})      # the baselines' one core (the device path's host work too)
    except (AttributeError, OSError):
        pass
    from deformablelka_amd import dataloading as D
    from tests import dataloading_ref as R
    patch = D.get_patch_size(FINAL, (-R30, R30), (-R30, R30), (-R30, R30), (0.85, 1.25))
    res = {"shape": args.shape, "cases": args.cases, "patch": patch.tolist(), "reps": args.reps}
    arrays = {f"case{k}": make_case(args.shape, k) for k in range(args.cases)}
    seg0 = arrays["case0"][-1]

    # class_locations on the host (the K-pass argwhere), kept as the loader's input for both paths
    t0 = time.perf_counter()
    locs0 = R.class_locations(seg0, ALL_CLASSES)
    host_cl_ms = (time.perf_counter() - t0) * 1e3
    props = {k: {"class_locations": R.class_locations(a[-1], ALL_CLASSES)} for k, a in arrays.items()}
    res["class_rows"] = {int(c): len(v) for c, v in locs0.items()}
    counts = [int((seg0 == c).sum()) for c in ALL_CLASSES]

    def permutations():
        rs = np.random.RandomState(1234)
        for n in counts:
            if n:
                rs.choice(n, max(min(10000, n), int(np.ceil(n * 0.01))), replace=False)
    res["host_permutation_ms"], _ = median_ms(permutations, 5)

    if not args.skip_baseline:
        res["numpy_class_locations_ms"], _ = median_ms(lambda: R.class_locations(seg0, ALL_CLASSES), 3)
        res["numpy_class_locations_first_ms"] = host_cl_ms
        cases = {k: (a.shape[1:], props[k]) for k, a in arrays.items()}
        rs, need = np.random.RandomState(11), np.zeros(3, int) + (patch - np.array(FINAL))
        host_batch = lambda: R.generate_train_batch(rs, arrays, cases, patch, need, 2, 0.33, "constant", {"constant_values": 0})  # noqa: E731
        host_batch()
        res["numpy_batch_ms"], res["numpy_batch_ms_all"] = median_ms(host_batch, args.reps)

    if not args.baseline_only:
        import torch
        assert torch.cuda.is_available(), "the GPU half needs the MI355X"
        sync = torch.cuda.synchronize
        data = {k: {"data": a, "properties": props[k]} for k, a in arrays.items()}
        t0 = time.perf_counter()
        loader = D.DataLoader3D(data, patch, FINAL, 2, False, 0.33, "r", "constant", {"constant_values": 0}, device="cuda", seed=11)
        sync()
        res["upload_all_cases_once_ms"] = (time.perf_counter() - t0) * 1e3
        for _ in range(3):
            loader.generate_train_batch()
        res["hip_batch_ms"], res["hip_batch_ms_all"] = median_ms(loader.generate_train_batch, args.reps, sync)
        rec = loader.last_draw
        resident = [loader._resident[k] for k in rec["keys"]]
        draw = lambda: D.draw_batch(loader.rs, loader._cases, patch, loader.need_to_pad, 2, 0.33)  # noqa: E731
        res["host_draw_ms"], _ = median_ms(draw, args.reps)
        apply = lambda: D.crop_batch(resident, rec["bbox_lb"], patch, "constant", {"constant_values": 0})  # noqa: E731
        res["hip_apply_ms"], res["hip_apply_ms_all"] = median_ms(apply, args.reps, sync)
        # the same boxes on the host: the same bits
        d, s = apply()
        rd, rseg = R.crop_batch([arrays[k] for k in rec["keys"]], rec["bbox_lb"], patch, "constant", {"constant_values": 0})
        res["batch_equals_numpy"] = bool(np.array_equal(d.cpu().numpy().view(np.int32), rd.view(np.int32)) and np.array_equal(s.cpu().numpy(), rseg))
        if not args.skip_baseline:
            pinned = torch.from_numpy(rd).pin_memory(), torch.from_numpy(rseg).pin_memory()
            upload = lambda: (pinned[0].cuda(non_blocking=True), pinned[1].cuda(non_blocking=True))  # noqa: E731
            upload()
            res["upload_batch_pinned_ms"], _ = median_ms(upload, args.reps, sync)
            pageable = lambda: (torch.from_numpy(rd).cuda(), torch.from_numpy(rseg).cuda())  # noqa: E731
            res["upload_batch_pageable_ms"], _ = median_ms(pageable, args.reps, sync)
        seg_dev = torch.from_numpy(seg0).cuda()
        for _ in range(2):
            got = D.class_locations(seg_dev, ALL_CLASSES)
        res["hip_class_locations_ms"], res["hip_class_locations_ms_all"] = median_ms(lambda: D.class_locations(seg_dev, ALL_CLASSES), 5, sync)
        res["class_locations_equal_numpy"] = all(np.array_equal(np.asarray(got[c]), np.asarray(locs0[c])) for c in ALL_CLASSES)
        from deformablelka_amd.ops import dataload
        counts_only = lambda: dataload.load_class_counts(seg_dev, ALL_CLASSES)[0].cpu()  # noqa: E731
        counts_only()
        res["hip_class_counts_ms"], _ = median_ms(counts_only, 10, sync)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
