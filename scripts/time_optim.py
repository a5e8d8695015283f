"""Times the optimizer step on the full net's own parameter list (training.initialize_network(1, 14, (64, 128, 128))): clip + step through
optim.SGD (csrc/cl_optim.hip) against clip_grad_norm_ + torch.optim.SGD(fused=True).  A report, not a gate.

    python scripts/time_optim.py [--out FILE] [--no-iteration] [--algorithm sgd|adamw|adam]

--algorithm adamw: optim.AdamW(weight_decay=1e-4) against torch.optim.AdamW(fused=True); adam: optim.Adam(3e-4, weight_decay=3e-5, amsgrad=True)
against torch.optim.Adam(amsgrad=True, fused=True); both with the clip, and torch's side also captured (capturable=True, which its fused step
needs inside a capture).

Protocol: gradients filled once; both sides warmed up; the two sides ALTERNATE, 9 samples each, one sample = one call between two events on an
idle stream (what the trainer's iteration sees at its end); median and min-max spread of both.  Also: the host time of one eager step() call
(no synchronisation inside the timed region), the captured step's replay (device time without the host's table walk), its update pass alone against the HBM rate a float4 streaming copy reaches on the MI355X (6.3 TB/s;
5 arrays of 4 bytes per element move with SGD, 7 with AdamW, 9 with amsgrad), and the whole run_iteration with either optimizer."""
import argparse
import statistics
import sys
import time

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from deformablelka_amd import optim, training   # noqa: E402

HBM_ACHIEVABLE = 6.3e12


def gpu_ms(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def host_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    dt = (time.perf_counter() - t) * 1e3
    torch.cuda.synchronize()
    return dt


def alternate(fa, fb, timer, n=9, warm=3):
    for _ in range(warm):
        fa(); fb()
    sa, sb = [], []
    for _ in range(n):
        sa.append(timer(fa))
        sb.append(timer(fb))
    return sa, sb


def line(name, s):
    return f"| {name} | {statistics.median(s):.3f} | {min(s):.3f} | {max(s):.3f} |"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-iteration", action="store_true")
    ap.add_argument("--algorithm", choices=["sgd", "adamw", "adam"], default="sgd")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = training.initialize_network(1, 14, (64, 128, 128), device=dev).train()
    params = list(net.parameters())
    n_el = sum(p.numel() for p in params)
    for p in params:
        p.grad = torch.randn_like(p) * 1e-3
    ref_graph = None
    if args.algorithm == "sgd":
        name, arrays = "SGD", 5
        hip = optim.SGD(params, 1e-6, momentum=0.99, nesterov=True, weight_decay=3e-5)
        ref = torch.optim.SGD(params, 1e-6, momentum=0.99, nesterov=True, weight_decay=3e-5, fused=True)
    elif args.algorithm == "adamw":
        name, arrays = "AdamW", 7   # p, g, m, v read; p, m, v written
        hip = optim.AdamW(params, 1e-6, weight_decay=1e-4)
        ref = torch.optim.AdamW(params, 1e-6, weight_decay=1e-4, fused=True)
        ref_graph = torch.optim.AdamW(params, 1e-6, weight_decay=1e-4, fused=True, capturable=True)
    else:
        name, arrays = "Adam", 9    # and max_exp_avg_sq read and written
        hip = optim.Adam(params, 1e-6, weight_decay=3e-5, amsgrad=True)
        ref = torch.optim.Adam(params, 1e-6, weight_decay=3e-5, amsgrad=True, fused=True)
        ref_graph = torch.optim.Adam(params, 1e-6, weight_decay=3e-5, amsgrad=True, fused=True, capturable=True)

    def hip_step():
        hip.step(max_grad_norm=12.0)

    def ref_step():
        torch.nn.utils.clip_grad_norm_(params, 12.0)
        ref.step()

    out = [f"{len(params)} tensors, {n_el} elements ({4 * n_el / 1e6:.0f} MB per array)", "",
           "| what (ms) | median of 9 | min | max |", "|---|---|---|---|"]
    a, b = alternate(hip_step, ref_step, gpu_ms)
    out += [line(f"clip + step, optim.{name}, events on an idle stream", a), line(f"clip + step, clip_grad_norm_ + torch fused {name}, same", b)]
    spread = max(max(a) - min(a), max(b) - min(b))
    gain = statistics.median(b) - statistics.median(a)
    out_verdict = f"difference of the medians {gain:.3f} ms, largest min-max spread {spread:.3f} ms: " + (
        "the HIP step is faster by more than three times the spread" if gain > 3 * spread else
        "NOT faster by more than three times the spread" if gain > 0 else "the HIP step is NOT faster")
    a, b = alternate(hip_step, ref_step, host_ms)
    out += [line(f"host time of one eager call, optim.{name}", a), line("host time of one eager call, torch", b)]
    # the device time without the host's table walk in front of the launches: the step captured once and replayed (how GraphedIteration runs it)
    graphs = {}
    for what, clip in (("clip + step", 12.0), ("update pass alone (no clip)", None)):
        torch.cuda.synchronize()
        graphs[what] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[what]):
            hip.step(max_grad_norm=clip)
        graphs[what].replay()
    torch_both = None
    if ref_graph is not None:   # torch's pair captured too (capturable=True), the two replays alternating
        def ref_graph_step():
            torch.nn.utils.clip_grad_norm_(params, 12.0)
            ref_graph.step()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                ref_graph_step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graphs["torch"] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs["torch"]):
            ref_graph_step()
        both, torch_both = alternate(graphs["clip + step"].replay, graphs["torch"].replay, gpu_ms)
    else:
        both = [gpu_ms(graphs["clip + step"].replay) for _ in range(9)]
    upd = [gpu_ms(graphs["update pass alone (no clip)"].replay) for _ in range(9)]
    out += [line(f"captured optim.{name} clip + step, one replay", both), line(f"captured optim.{name} update pass alone, one replay", upd)]
    if torch_both is not None:
        out += [line(f"captured clip_grad_norm_ + torch fused {name} (capturable), one replay", torch_both)]
        spread = max(max(both) - min(both), max(torch_both) - min(torch_both))
        gain = statistics.median(torch_both) - statistics.median(both)
        out_verdict += f"\ncaptured: difference of the medians {gain:.3f} ms, largest min-max spread {spread:.3f} ms: " + (
            "the HIP step is faster by more than three times the spread" if gain > 3 * spread else
            "NOT faster by more than three times the spread" if gain > 0 else "the HIP step is NOT faster")
    moved = arrays * 4 * n_el
    rate = moved / (statistics.median(upd) * 1e-3)
    out += ["", out_verdict, f"update pass: {moved / 1e6:.0f} MB moved, {rate / 1e12:.2f} TB/s = {100 * rate / HBM_ACHIEVABLE:.0f} % of the 6.3 TB/s a "
            "streaming copy reaches"]
    if not args.no_iteration:
        x = torch.randn(1, 1, 64, 128, 128, device=dev)
        tgt = torch.randint(0, 14, (1, 64, 128, 128), device=dev)
        a, b = alternate(lambda: training.run_iteration(net, hip, x, tgt), lambda: training.run_iteration(net, ref, x, tgt), gpu_ms)
        out += ["", "| run_iteration, full net, batch 1 (ms) | median of 9 | min | max |", "|---|---|---|---|",
                line(f"optim.{name}", a), line(f"torch fused {name} + clip_grad_norm_", b)]
    text = "\n".join(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
