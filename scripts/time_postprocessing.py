#!/usr/bin/env python
"""Times deformablelka_amd.postprocessing.remove_all_but_the_largest_connected_component on a synthetic Synapse-sized prediction
(148 x 512 x 512, the eight organs of scripts/time_metrics.py as ellipsoids plus salt noise: isolated cells of every organ's class) against
the host baseline: the reference's algorithm (connected_components.py:48-105), i.e. one scipy.ndimage.label per class and one full-volume
comparison per object to size it, another per removed object.

    python scripts/time_postprocessing.py [--skip-baseline | --baseline-only] [--shape 148 512 512] [--noise 200] [--reps 5] [--out FILE.json]

The two halves may run on different machines (the baseline needs scipy and no GPU).  The device half prints the time of each of the six launches
of the one pass (the library's launch trace) and the end-to-end time of one call on a device tensor and on a host array."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from scripts.time_metrics import CLASSES, make_case  # noqa: E402

VOLUME_PER_VOXEL = 0.75 * 0.75 * 3.0


def make_prediction(shape, noise, seed=0):
    """The organs plus `noise` isolated cells per class, on a lattice of pitch 2 so that no two of them touch."""
    _, lab = make_case(tuple(shape))
    rng = np.random.default_rng(seed)
    free = np.argwhere(lab[::2, ::2, ::2] == 0) * 2
    pick = free[rng.choice(len(free), size=min(noise * len(CLASSES), len(free)), replace=False)]
    lab[pick[:, 0], pick[:, 1], pick[:, 2]] = np.resize(np.asarray(CLASSES, np.uint8), len(pick))
    return lab


def host_baseline(image, classes, volume_per_voxel):
    """The per-class, per-object loop as the reference runs it (sizes by one comparison of the whole object map per object)."""
    from scipy.ndimage import label
    image = image.copy()
    largest_removed, kept_size, objects = {}, {}, 0
    for c in classes:
        mask = image == c
        lmap, n = label(mask.astype(int))
        objects += n
        sizes = {k: (lmap == k).sum() * volume_per_voxel for k in range(1, n + 1)}
        largest_removed[c] = kept_size[c] = None
        if n:
            kept_size[c] = max(sizes.values())
            for k in range(1, n + 1):
                if sizes[k] != kept_size[c]:
                    image[(lmap == k) & mask] = 0
                    largest_removed[c] = sizes[k] if largest_removed[c] is None else max(largest_removed[c], sizes[k])
    return image, largest_removed, kept_size, objects


def launch_times(fn, stream):
    """[(kernel name, ms)] of the launches `fn` makes, from the library's launch trace."""
    from ctypes import byref, c_float, create_string_buffer
    from deformablelka_amd import _lib as L
    lib = L.get_lib()
    L.check(lib.dlka_trace_start(256, stream), "trace_start")
    try:
        L.check(lib.dlka_trace_mark(stream), "trace_mark")
        fn()
    finally:
        rc = lib.dlka_trace_stop()
    L.check(rc, "trace_stop")
    buf, ms, rows = create_string_buffer(512), c_float(), []
    for i in range(lib.dlka_trace_count()):
        L.check(lib.dlka_trace_get(i, buf, 512, byref(ms)), "trace_get")
        if buf.value.decode() != "(mark)":
            rows.append((buf.value.decode(), float(ms.value)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[148, 512, 512])
    ap.add_argument("--noise", type=int, default=200, help="isolated cells per class")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-baseline", action="store_true")
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    image = make_prediction(args.shape, args.noise)
    res = {"shape": args.shape, "classes": CLASSES, "noise_per_class": args.noise}
    if not args.baseline_only:
        import torch
        from deformablelka_amd import _lib as L, postprocessing as P
        assert torch.cuda.is_available(), "the GPU half needs the MI355X"
        dev = torch.from_numpy(image).cuda()
        out, removed, kept = P.remove_all_but_the_largest_connected_component(dev, CLASSES, VOLUME_PER_VOXEL)   # warm-up
        times = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out, removed, kept = P.remove_all_but_the_largest_connected_component(dev, CLASSES, VOLUME_PER_VOXEL)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        P.remove_all_but_the_largest_connected_component(image, CLASSES, VOLUME_PER_VOXEL)
        res["hip_ms_from_host_arrays"] = (time.perf_counter() - t0) * 1e3
        rows = launch_times(lambda: P.remove_all_but_the_largest_connected_component(dev, CLASSES, VOLUME_PER_VOXEL), L.stream_ptr(dev))
        for name, ms in rows:
            print(f"{ms:10.3f} ms  {name}", file=sys.stderr)
        res.update(hip_ms=times, hip_ms_median=float(np.median(times)), hip_launch_ms=rows, hip_kept=[kept[c] for c in CLASSES],
                   hip_largest_removed=[removed[c] for c in CLASSES], hip_cells_left=int((out != 0).sum()))
    if not args.skip_baseline:
        t0 = time.perf_counter()
        out, removed, kept, objects = host_baseline(image, CLASSES, VOLUME_PER_VOXEL)
        res.update(scipy_ms=(time.perf_counter() - t0) * 1e3, scipy_objects=objects, scipy_kept=[float(kept[c]) for c in CLASSES],
                   scipy_largest_removed=[None if removed[c] is None else float(removed[c]) for c in CLASSES],
                   scipy_cells_left=int((out != 0).sum()))
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
