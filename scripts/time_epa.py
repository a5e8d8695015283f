"""Times forward + backward of EPA (deformablelka_amd/transformerblock.py) at the four Synapse stages, B = 2: the fused path (csrc/cl_epa.hip) against the
operator-by-operator torch forward of the same module (``forward_per_op``: the reference's arithmetic) on the same GPU.  Per shape: warm-up, then
``--reps`` event-timed windows of ``--iters`` iterations per path, the two paths alternating window by window; median and spread per path; both paths see
the same inputs, eval mode (no dropout draws).
Prints one JSON line per stage.  Results are recorded in profiles/epa_notes.md."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STAGES = ((32 ** 3, 32, 64), (16 ** 3, 64, 64), (8 ** 3, 128, 64), (4 ** 3, 256, 32))   # (N, C, proj_size): D_LKA_Former_Encoder's defaults


def window(step, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)   # a window of some 0.3 - 0.6 s
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=2)
    args = ap.parse_args()
    from deformablelka_amd import transformerblock
    dev = "cuda"
    for N, C, P in STAGES:
        torch.manual_seed(0)
        m = transformerblock.EPA(N, C, P, 4).to(dev).eval()
        x = torch.randn(args.batch, N, C, device=dev, requires_grad=True)
        go = torch.randn(args.batch, N, C, device=dev)
        assert m.fused(x)

        def run(fwd):
            for p in m.parameters():
                p.grad = None
            x.grad = None
            fwd(x).backward(go)

        paths = (("fused", m.forward), ("per_op", m.forward_per_op))
        times = {name: [] for name, _ in paths}
        for name, fwd in paths:
            for _ in range(args.warmup):
                run(fwd)
        torch.cuda.synchronize()
        for _ in range(args.reps):   # the two paths alternate, window by window: drift of the machine lands on both
            for name, fwd in paths:
                times[name].append(window(lambda: run(fwd), args.iters))
        res = {}
        for name, t in times.items():
            res[name + "_ms_median"] = round(statistics.median(t), 4)
            res[name + "_ms_min_max"] = [round(min(t), 4), round(max(t), 4)]
        res["per_op_over_fused"] = round(res["per_op_ms_median"] / res["fused_ms_median"], 3)
        print(json.dumps({"N": N, "C": C, "P": P, "B": args.batch, **res}), flush=True)


if __name__ == "__main__":
    main()
