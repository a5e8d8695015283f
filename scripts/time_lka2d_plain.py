#!/usr/bin/env python
"""Times the plain 2-D LKA block's forward + backward at one decoder shape of bench.py's 2-D metric (B = 24; 96 x 56^2, 192 x 28^2, 384 x 14^2), on ONE card,
three variants alternating A B C A B C ...:

  fused        LKA_Attention as it routes itself: one C call per direction (csrc/capi_lka2d_plain_cl.hip)
  per_op       the same module forced onto the per-op path (LKA_Attention.per_op): nn_ops.conv2d / nn_ops.gelu, what the library's single operators give;
               for bf16 the module and x are bfloat16 throughout (the general operators take one dtype), the fused block runs under torch.autocast
  deformable   deformable_LKA_Attention at the same shape (bf16: under torch.autocast)

Device events around `iters` forward + backward passes per round after a warm-up; median, min and max of the rounds' per-pass times.  Also checks, once, that
fused and per_op agree on y.  One JSON line on stdout (and appended to --out).  Results: profiles/lka2d_plain_notes.md.

usage: python scripts/time_lka2d_plain.py --C 96 --hw 56 [--dtype bf16] [--B 24] [--iters 20] [--rounds 7] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--C", type=int, required=True)
    ap.add_argument("--hw", type=int, required=True)
    ap.add_argument("--B", type=int, default=24)
    ap.add_argument("--dtype", choices=["f32", "bf16"], default="f32")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_lka2d_plain.py measures on the GPU; there is none here")
    from deformablelka_amd.deformable_LKA import deformable_LKA_Attention
    from deformablelka_amd.LKA import LKA_Attention
    dev = torch.device("cuda", 0)
    bf = a.dtype == "bf16"
    torch.manual_seed(0)
    fused = LKA_Attention(a.C).to(dev)
    per_op = LKA_Attention(a.C).to(dev)
    per_op.load_state_dict(fused.state_dict())
    per_op.per_op = True
    if bf:
        per_op = per_op.bfloat16()
    deform = deformable_LKA_Attention(a.C).to(dev)
    x = torch.randn(a.B, a.C, a.hw, a.hw, device=dev)
    gy = torch.randn_like(x)
    assert fused.fused(x) and not per_op.fused(x)

    def step(m, autocast, xin):
        xin = xin.detach().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            y = m(xin)
        y.backward(gy.to(y.dtype))
        return y

    variants = {"fused": (fused, bf, x), "per_op": (per_op, False, x.bfloat16() if bf else x), "deformable": (deform, bf, x)}
    ys, refused = {}, {}
    for name, v in list(variants.items()):   # warm-up: code objects, allocator
        try:
            for _ in range(3):
                ys[name] = step(*v)
        except RuntimeError as e:            # a variant the library refuses at this shape / dtype is reported, not timed
            if name == "fused":
                raise
            refused[name] = str(e)[:200]
            del variants[name]
    torch.cuda.synchronize()
    agree = float((ys["fused"].detach().float() - ys["per_op"].detach().float()).abs().max()) if "per_op" in variants else None
    times = {name: [] for name in variants}
    for _ in range(a.rounds):
        for name, v in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                step(*v)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.iters)
    res = {"C": a.C, "hw": a.hw, "B": a.B, "dtype": a.dtype, "iters": a.iters, "rounds": a.rounds, "fused_vs_per_op_max_abs_y": agree}
    res.update({name + "_refused": why for name, why in refused.items()})
    for name, t in times.items():
        res[name + "_ms"] = {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
