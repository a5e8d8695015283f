"""Times a Synapse-sized export: 14 class probabilities from the network's grid to ~150 x 512 x 512, in-plane linear with nearest z (the
trainers' orders), as (1) deformablelka_amd.resampling.resample_and_argmax, one fused kernel; (2) the torch composition on the device:
F.interpolate per branch (bilinear in-plane per slice, nearest z) plus argmax, the same coordinate map; (3) with --host, the scipy
restatement (tests/resampling_ref.py through map_coordinates) on one host core, on a reduced number of channels and slices, scaled.
Prints one line per measurement and the algorithmic traffic of the fused path against the materialising one.

    python scripts/time_resampling.py [--classes 14] [--src 96 320 320] [--dst 150 512 512] [--reps 5] [--host]"""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deformablelka_amd import resampling as S   # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", type=int, default=14)
    ap.add_argument("--src", type=int, nargs=3, default=(96, 320, 320))
    ap.add_argument("--dst", type=int, nargs=3, default=(150, 512, 512))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host", action="store_true")
    a = ap.parse_args()
    c, src, dst = a.classes, tuple(a.src), tuple(a.dst)
    g = torch.Generator(device="cuda").manual_seed(0)
    p = torch.softmax(4.0 * torch.randn((c,) + src, device="cuda", generator=g), 0)

    fused = lambda: S.resample_and_argmax(p, dst, axis=[0], order=1, do_separate_z=True, order_z=0)   # noqa: E731

    def torch_composition():
        q = F.interpolate(p, size=dst[1:], mode="bilinear", align_corners=False)                       # (c, d, H, W): every slice in-plane
        q = F.interpolate(q[None], size=dst, mode="nearest-exact")[0] if src[0] != dst[0] else q     # nearest z
        return q.argmax(0).to(torch.uint8)

    unfused = lambda: S.resample_data_or_seg(p, dst, False, [0], 1, True, 0, 0).argmax(0)              # noqa: E731
    t_f, t_t, t_u = timed(fused, a.reps), timed(torch_composition, a.reps), timed(unfused, a.reps)
    agree = float((fused() == torch_composition()).float().mean())
    cells_in, cells_out = int(np.prod(src)), int(np.prod(dst))
    read, write, extra = c * cells_in * 4, cells_out, 2 * c * cells_out * 4
    print(f"shape {c} x {src} -> {dst}")
    print(f"fused resample_and_argmax           {1e3 * t_f:9.2f} ms   algorithmic {read / 1e6:.1f} MB read + {write / 1e6:.1f} MB written"
          f" = {(read + write) / t_f / 1e9:.1f} GB/s")
    print(f"product, materialised + argmax      {1e3 * t_u:9.2f} ms   + {extra / 1e6:.1f} MB written and read back")
    print(f"torch interpolate + argmax          {1e3 * t_t:9.2f} ms   label maps agree on {100 * agree:.4f} % of the cells")
    if a.host:
        from tests import resampling_ref as R
        x = p[:2, :8].cpu().numpy()
        t0 = time.perf_counter()
        for ch in x:
            for sl in ch:
                R.resize(sl, dst[1:], 1)
        per_slice = (time.perf_counter() - t0) / 16
        print(f"scipy restatement, one host core    {1e3 * per_slice * c * src[0]:9.0f} ms   in-plane step only, scaled from 16 slices"
              f" ({1e3 * per_slice:.1f} ms each); the z step and the argmax come on top")


if __name__ == "__main__":
    main()
