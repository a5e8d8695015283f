"""Times the fused Dice + cross-entropy loss (deformablelka_amd/losses.py, csrc/cl_seg_loss.hip) against the same loss composed from stock torch
ops (tests/seg_loss_ref.py: the reference's formulation, what a user would run without this package's loss), in ONE process on one MI355X,
alternating the two:

  (a) loss forward + backward at the three heads D_LKA_Former returns for a 64x128x128 patch (B = 2, K = 14), fp32 and bf16 logits;
  (b) the whole ``run_iteration`` of the full net with each of the two, and with the cross-entropy-only default for context.

Per run a window of ``--inner`` repetitions between two device events; ``--runs`` alternated runs (>= 7); medians and the min-max spread.  Bytes: the
algorithmic minimum (logits + labels forward; logits + labels + gradient backward) over the measured time gives the achieved rate of the fused
pair; measured HBM bytes come from rocprofv3 --pmc runs of ``--pmc-step`` on their own (no tracing in the same run).

    python scripts/time_seg_loss.py --out profiles/seg_loss_times.json            # (a) and (b)
    rocprofv3 --pmc FETCH_SIZE -d <dir> -- python scripts/time_seg_loss.py --pmc-step f32   # counters: a run of their own, ONE counter per run
    rocprofv3 --pmc WRITE_SIZE -d <dir> -- python scripts/time_seg_loss.py --pmc-step f32   # (both in one pass exceed what the hardware collects)
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deformablelka_amd import training  # noqa: E402
from tests import seg_loss_ref as R  # noqa: E402

DEV = "cuda:0"
DICE_KW = {"batch_dice": True, "smooth": 1e-5, "do_bg": False}


def head_shapes():
    nets = torch.load(os.path.join(ROOT, "tests", "golden", "reference_nets.pt"), weights_only=False)
    return [tuple(s[1:]) for s in nets["D_LKA_Former_plumbing"]["out_shapes"]]


def make_head(shape, B, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    K, spatial = shape[0], shape[1:]
    x = (torch.randn((B, K) + spatial, generator=gen) * 2.0).to(DEV, dtype).requires_grad_(True)
    y = torch.randint(0, K, (B, 1) + spatial, generator=gen).float().to(DEV)
    return x, y


def window(step, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        step()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def alternate(steps, runs, inner, warmup=3):
    for s in steps.values():
        for _ in range(warmup):
            s()
    torch.cuda.synchronize()
    times = {k: [] for k in steps}
    for _ in range(runs):
        for k, s in steps.items():
            times[k].append(window(s, inner))
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "spread_ms": max(v) - min(v), "runs": v} for k, v in times.items()}


def ref_composition_loss(weights):
    def fn(outputs, target):
        if isinstance(target, torch.Tensor):
            target = [target if target.shape[2:] == o.shape[2:] else torch.nn.functional.interpolate(target, size=o.shape[2:], mode="nearest") for o in outputs]
        return R.multiple_output([o.float() for o in outputs], target, weights, **DICE_KW)
    return fn


def heads_table(runs, inner, B=2):
    fused = training.initialize_loss(deep_supervision=False)
    rows = []
    for dtype in (torch.float32, torch.bfloat16):
        for h, shape in enumerate(head_shapes()):
            x, y = make_head(shape, B, dtype, h)

            def fused_fwd():
                return fused(x, y)

            def fused_step():
                x.grad = None
                fused(x, y).backward()

            def ref_fwd():
                return R.dc_and_ce(x, y, **DICE_KW)[0]

            def ref_step():
                x.grad = None
                R.dc_and_ce(x, y, **DICE_KW)[0].backward()

            with torch.no_grad():
                t_fwd = alternate({"fused": fused_fwd, "torch": ref_fwd}, runs, inner)
            t_all = alternate({"fused": fused_step, "torch": ref_step}, runs, inner)
            n = x.numel() // (B * shape[0])
            min_fwd = x.numel() * x.element_size() + B * n * 4
            min_bwd = 2 * x.numel() * x.element_size() + B * n * 4
            row = {"head": h, "shape": [B] + list(shape), "dtype": str(dtype).replace("torch.", ""), "forward": t_fwd, "forward_backward": t_all,
                   "min_bytes_forward": min_fwd, "min_bytes_backward": min_bwd,
                   "fused_forward_GBps_of_minimum": min_fwd / (t_fwd["fused"]["median_ms"] * 1e6),
                   "fused_backward_ms": t_all["fused"]["median_ms"] - t_fwd["fused"]["median_ms"]}
            bwd = row["fused_backward_ms"]
            row["fused_backward_GBps_of_minimum"] = min_bwd / (bwd * 1e6) if bwd > 0 else None
            d = t_all["torch"]["median_ms"] - t_all["fused"]["median_ms"]
            row["gain_ms"], row["gain_over_3x_torch_spread"] = d, d > 3 * t_all["torch"]["spread_ms"]
            rows.append(row)
            print(json.dumps({k: v for k, v in row.items() if k not in ("forward", "forward_backward")}), flush=True)
            print("   fwd      ", {k: (round(v["median_ms"], 4), round(v["min_ms"], 4), round(v["max_ms"], 4)) for k, v in t_fwd.items()}, flush=True)
            print("   fwd+bwd  ", {k: (round(v["median_ms"], 4), round(v["min_ms"], 4), round(v["max_ms"], 4)) for k, v in t_all.items()}, flush=True)
            del x, y
            torch.cuda.empty_cache()
    return rows


def iteration_table(runs, inner):
    torch.manual_seed(0)
    net = training.initialize_network(1, 14, (64, 128, 128), device=DEV).train()
    opt = training.initialize_optimizer(net, initial_lr=1e-4)
    x = torch.randn(2, 1, 64, 128, 128, device=DEV)
    tgt = torch.randint(0, 14, (2, 1, 64, 128, 128), device=DEV).float()
    fused = training.initialize_loss()
    comp = ref_composition_loss(fused.weight_factors)
    tgt_long = tgt[:, 0].long()
    steps = {"fused": lambda: training.run_iteration(net, opt, x, tgt, loss_fn=fused),
             "torch": lambda: training.run_iteration(net, opt, x, tgt, loss_fn=comp),
             "ce_only_default": lambda: training.run_iteration(net, opt, x, tgt_long)}
    t = alternate(steps, runs, inner, warmup=2)
    d = t["torch"]["median_ms"] - t["fused"]["median_ms"]
    out = {"times": t, "gain_ms": d, "gain_over_3x_torch_spread": d > 3 * t["torch"]["spread_ms"]}
    print("run_iteration", {k: (round(v["median_ms"], 3), round(v["min_ms"], 3), round(v["max_ms"], 3)) for k, v in t.items()}, "gain_ms", round(d, 3), flush=True)
    return out


def pmc_step(kind):
    """A few fused forward + backward calls at the largest head, for a counter run of their own."""
    dtype = torch.float32 if kind == "f32" else torch.bfloat16
    fused = training.initialize_loss(deep_supervision=False)
    x, y = make_head(head_shapes()[0], 2, dtype, 0)
    for _ in range(3):
        x.grad = None
        fused(x, y).backward()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--iter-inner", type=int, default=3)
    ap.add_argument("--skip-iteration", action="store_true")
    ap.add_argument("--pmc-step", choices=["f32", "bf16"])
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_seg_loss.py measures on the GPU; none found")
    if a.runs < 7:
        raise SystemExit("--runs must be at least 7")
    if a.pmc_step:
        pmc_step(a.pmc_step)
        return
    result = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "inner": a.inner, "heads": heads_table(a.runs, a.inner)}
    if not a.skip_iteration:
        result["run_iteration"] = iteration_table(a.runs, a.iter_inner)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
