#!/usr/bin/env python
"""Cost of test-time mirroring in ``D_LKA_Former.predict_3D`` at Synapse size (GPU): a seeded synthetic 1 x 148 x 256 x 256 volume, 14 classes,
64 x 128 x 128 patch, step 0.5, Gaussian weighting (36 tiles), the real net in evaluation mode.  One process, warm-up first:

  none    predict_3D(do_mirroring=False)                     one forward per tile
  hip     predict_3D(do_mirroring=True)                      gather / blend / finalize kernels (csrc/cl_tiles.hip), 2 tiles x 8 mirrors per forward
  torch   the same through the torch restatement             one B = 1 forward per mirror, torch flips / softmax / blending (inference._MIRROR_IMPL)

and the data movement of one chunk alone (T = 2 tiles, M = 8 mirrors, K = 14): gather + blend against the torch operations they replace, with the
blend's algorithmic bandwidth (logits read once + score / weight maps read and written over the chunk's bounding box).
--profile re-runs the hip mode in a child process under ``rocprofv3 --kernel-trace --stats`` and reports the tile kernels' share of kernel time.

    python scripts/time_tta.py [--modes none hip torch] [--reps 2] [--bf16] [--profile DIR]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

PATCH, SHAPE, K = (64, 128, 128), (1, 148, 256, 256), 14


def _predict(net, vol, mirror, bf16):
    net.predict_3D(vol, mirror, use_sliding_window=True, step_size=0.5, patch_size=PATCH, use_gaussian=True, verbose=False, mixed_precision=bf16)
    torch.cuda.synchronize()


def time_modes(modes, reps, warmup, bf16):
    from deformablelka_amd import inference, training
    dev = torch.device("cuda", 0)
    net = training.initialize_network(1, K, PATCH, device=dev, wgrad_overlap=False).eval()
    vol = torch.randn(SHAPE, generator=torch.Generator().manual_seed(0)).to(dev)
    out = {}
    for mode in modes:
        inference._MIRROR_IMPL = "torch" if mode == "torch" else None
        for _ in range(warmup):
            _predict(net, vol, mode != "none", bf16)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            _predict(net, vol, mode != "none", bf16)
            ts.append(time.perf_counter() - t0)
        inference._MIRROR_IMPL = None
        ts.sort()
        out[mode] = {"s_per_volume": ts[len(ts) // 2], "volumes_per_s": 1.0 / ts[len(ts) // 2]}
        print(mode, json.dumps(out[mode]), flush=True)
    if "none" in out and "hip" in out:
        out["hip_over_none"] = out["hip"]["s_per_volume"] / out["none"]["s_per_volume"]
    if "torch" in out and "hip" in out:
        out["torch_over_hip"] = out["torch"]["s_per_volume"] / out["hip"]["s_per_volume"]
    return out


def _events(fn, reps=20):
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def time_chunk():
    """Data movement of one chunk: the HIP kernels against the torch operations of the reference's per-tile loop."""
    from deformablelka_amd import inference, ops
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(SHAPE, generator=g).to(dev)
    origins = [(0, 0, 0), (0, 0, 64)]                       # two neighbouring tiles (z step 64)
    masks = inference.mirror_masks((0, 1, 2))
    pd, ph, pw = PATCH
    logits = torch.randn((len(origins) * 8, K) + PATCH, generator=g).to(dev)
    gauss = inference.gaussian_importance_map(PATCH, device=dev)
    score = torch.zeros((K,) + SHAPE[1:], device=dev)
    weight = torch.zeros(SHAPE[1:], device=dev)

    def hip():
        ops.tiles_gather(x, origins, masks, PATCH, (0, 0, 0))
        ops.tiles_blend(logits, 1, 1 / 8, gauss, score, weight, origins, masks)

    def hip_blend():
        ops.tiles_blend(logits, 1, 1 / 8, gauss, score, weight, origins, masks)

    def torch_path():
        for t, (a, b, c) in enumerate(origins):
            tile = x[None, :, a:a + pd, b:b + ph, c:c + pw]
            ins = [torch.flip(tile, inference._flip_dims(m)) if m else tile for m in masks]   # the network inputs
            res = torch.zeros((1, K) + PATCH, device=dev)
            for j, m in enumerate(masks):
                p = torch.softmax(logits[t * 8 + j:t * 8 + j + 1], 1)
                res += 1 / 8 * (torch.flip(p, inference._flip_dims(m)) if m else p)
            res[:, :] *= gauss
            score[:, a:a + pd, b:b + ph, c:c + pw] += res[0]
            weight[a:a + pd, b:b + ph, c:c + pw] += gauss
        return ins

    ms_hip, ms_blend, ms_torch = _events(hip), _events(hip_blend), _events(torch_path)
    bbox = pd * ph * (pw + 64)
    nbytes = logits.numel() * 4 + 2 * (K + 1) * bbox * 4
    res = {"chunk_T": 2, "chunk_M": 8, "K": K, "hip_gather_blend_ms": ms_hip, "hip_blend_ms": ms_blend, "torch_ms": ms_torch,
           "blend_algorithmic_TBps": nbytes / ms_blend / 1e9, "blend_fraction_of_6.3TBps": nbytes / ms_blend / 1e9 / 6.3}
    print("chunk", json.dumps(res), flush=True)
    return res


def profile(outdir, bf16):
    """The hip mode once (after one warm-up) under rocprofv3 in a child process; share of the tile kernels in the kernel time."""
    cmd = ["timeout", "-k", "10", "600", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "-o", "t", "--",
           sys.executable, os.path.abspath(__file__), "--modes", "hip", "--reps", "1", "--warmup", "1", "--no-chunk"] + (["--bf16"] if bf16 else [])
    rc = subprocess.call(cmd)
    files = glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True)
    if rc != 0 or not files:
        return {"profile_rc": rc}
    total = tiles = 0.0
    rows = []
    with open(files[0]) as f:
        for r in csv.DictReader(f):
            ns = float(r["TotalDurationNs"])
            total += ns
            if "tiles_" in r["Name"]:
                tiles += ns
                rows.append((r["Name"][:80], int(r["Calls"]), ns / 1e6))
    res = {"kernel_ms_total": total / 1e6, "tile_kernels_ms": tiles / 1e6, "tile_kernels_share": tiles / total if total else None,
           "tile_kernels": rows}
    print("profile", json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--modes", nargs="*", default=["none", "hip", "torch"], choices=["none", "hip", "torch"])
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--bf16", action="store_true", help="mixed_precision=True (bf16 autocast)")
    ap.add_argument("--no-chunk", action="store_true", help="skip the one-chunk data-movement comparison")
    ap.add_argument("--profile", default=None, help="directory for a rocprofv3 --kernel-trace --stats run of the hip mode")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the MI355X")
    res = {"shape": SHAPE, "patch": PATCH, "classes": K, "bf16": args.bf16}
    if args.modes:
        res["predict"] = time_modes(args.modes, args.reps, args.warmup, args.bf16)
    if not args.no_chunk:
        res["chunk"] = time_chunk()
    if args.profile:
        res["profile"] = profile(args.profile, args.bf16)
    print(json.dumps(res))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
