#!/usr/bin/env python
"""bench.py — 3-D D-LKA fwd+bwd volumes/s on MI355X (BASELINE.json metric).

One *step* = forward + backward through the 21 D-LKA attention blocks that one 64x128x128 Synapse patch traverses in
D_LKA_Former (6x(C=32,32^3) + 6x(64,16^3) + 6x(128,8^3) + 3x(256,4^3)), batch 2 per GPU, plus the
gradient all-reduce (N>1) and a plain SGD update of all block parameters.  Inputs are synthetic and already resident
in HBM when the timed region starts.  `value` = volumes (patches) per second over all ranks.

    python bench.py --gpus 1 --steps 20 --warmup 5
    python bench.py --gpus 1 --steps 20 --warmup 5 --full
    python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs DIR
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

Prints ONE JSON line on rank 0 (see the driver contract).  A plain run sets up, warms up, times exactly `--steps` steps once and
prints the headline (`value`, `ms_per_step`, ...).  `--full` adds everything else:
  "repetitions":  the timed region run `--reps` (default 3) times back to back, the median reported
  "roofline":     dominant kernel, algorithmic flops|bytes per launch / HIP-event duration, vs the MI355X peak
  "cpu_baseline": the oracle block (ATen CPU convs + C deformable oracle) timed on the host cores, bounded sample
  "other_dtype", "tblock", "lka_modules", "lka2d", "fullnet": the companion metrics (`--extras` adds more and implies `--full`).
`--dump-outputs DIR` writes what the last timed step computed as DIR/<name>.npy (float32), see dump_outputs().
"""
import argparse
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

PEAK_HBM_GBS = 8000.0       # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
PEAK_F32_TFLOPS = 157.3     # fp32 vector == fp32-input MFMA peak
PEAK_BF16_TFLOPS = 2500.0   # dense bf16 MFMA (not the roof of the bf16 run: its contractions other than the offset conv stay on fp32 MFMA)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--full", action="store_true", help="also run everything besides the headline: repeated timed regions, roofline, CPU baseline, "
                    "the other dtype and the companion metrics (several minutes)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed step computed to DIR/<name>.npy (float32, < 64 MB in all)")
    ap.add_argument("--reps", type=int, default=None, help="repetitions of the timed K-step region; the median is reported "
                    "(default: 1, or 3 with --full)")
    ap.add_argument("--batch", type=int, default=2, help="volumes per GPU (BASELINE.json: b2)")
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16"])
    ap.add_argument("--no-graph", action="store_true", help="do not capture the step in a hipGraph")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--extras", action="store_true", help="also report the full-net training iteration, the 2-D block images/s and the sliding-window tiles/s "
                    "(SURVEY §8d secondary metrics; ~1 min)")
    ap.add_argument("--no-companion", action="store_true", help="skip the same step measured with the other activation dtype (N = 1 only)")
    ap.add_argument("--no-tblock", action="store_true", help="skip the second metric (wrapper-block stack through nn.Module/autograd)")
    ap.add_argument("--no-fullnet", action="store_true", help="skip the full-net trainer iteration (SURVEY section 8d metric iii; 5 timed iterations, ~10 s incl. building the net)")
    ap.add_argument("--no-lka2d", action="store_true", help="skip the 2-D block metric (BASELINE.json config 2: bf16, batch 24; ~0.15 s of GPU time)")
    ap.add_argument("--cpu-sample", default="stage", choices=["stage", "tiny"])
    args = ap.parse_args()
    if args.extras:   # the extras are reported beside everything --full reports
        args.full = True
    if args.reps is None:
        args.reps = 3 if args.full else 1
    return args


# ----------------------------------------------------------------------------------------------------------------
# roofline: per-kernel HIP-event durations of the step's OWN kernels (launch trace of the library, include/dlka.h)
# ----------------------------------------------------------------------------------------------------------------
def kernel_work(name, B, C, n, dbytes):
    """Algorithmic (flops, bytes) of ONE launch of kernel `name` inside a block of stage (C, n voxels per volume, batch B) — SURVEY.md §8d:
    flops per the block's formula terms, bytes = unique input bytes + output bytes of the operator the kernel implements (activations
    `dbytes` per element, offsets / grad_offset always fp32).  Kernels that only re-lay / fold / zero return (0, bytes or 0)."""
    E, Off, M = B * C * n, B * 81 * n, B * n
    s = dbytes
    contr, interp = 2 * 27 * C * C * M, 27 * M * (15 * C + 30)
    offc = 2 * 27 * C * 81 * M
    if "cl_deform_goff2_kernel" in name or "cl_deform_goff16_kernel" in name:      # Col (MFMA) + 8 corners x C dot products + 3 axes; writes grad_offset (+ the sample hand-over, see `extra`)
        return contr + 27 * M * (16 * C + 48), (2 * E) * s + 2 * Off * 4
    if "cl_deform_gx_fx2_kernel" in name or "cl_deform_gx_kernel" in name:
        return contr + 27 * M * (16 * C), 2 * E * s + Off * 4
    if "cl_deform_fwd" in name:
        return contr + interp, 2 * E * s + Off * 4
    if "cl_wgrad_samp_kernel" in name:        # dense stream over the stored samples S[tap][m][c] (round 6: IEEE halves on the fp32 path too)
        return contr, 27 * E * 2 + E * s
    if "cl_wgrad_deform_kernel" in name:
        return contr + interp, 2 * E * s + Off * 4
    if "cl_wgrad_dense_kernel" in name:
        return offc, E * s + Off * 4
    m = re.search(r"cl_(?:igemm|conv_wave|conv_kw)_kernel<(\d+), (\d+)", name)
    if m:                                     # <mode, planar output, ...>: mode 0 = forward conv, 2 = data gradient from a planar grad_out
        return offc, E * s + Off * 4
    m = re.search(r"cl_dwconv_(?:rowsN|rows|wgrad2|wgrad)_kernel<[^,]+, (\d+), (\d+)", name)
    if m:
        k = int(m.group(1))
        return 2 * k ** 3 * E, 2 * E * s
    if "cl_pointwise_pair_kernel" in name:
        return 2 * 2 * C * E, 4 * E * s
    if "cl_pointwise_kernel" in name:
        return 2 * C * E, 2 * E * s
    if "cl_wgrad_pw3_kernel" in name:
        return 3 * 2 * C * E, 6 * E * s
    return 0, 0


def trace_step(stack, reps=3):
    """Run the step's forward + backward `reps` times EAGERLY under the library's launch trace: a HIP timing event behind every kernel launch,
    on the launch's own stream (torch's current stream = the stream the C-ABI launches on).  Marks separate the blocks, so every record is
    attributed to its block's stage.  Returns {(stage, kernel name): [count per step, mean ms]} and the per-step sum of all records."""
    from ctypes import byref, c_float, create_string_buffer
    from deformablelka_amd import _lib as L
    lib = L.get_lib()
    dev = stack.device
    st = torch.cuda.current_stream(dev).cuda_stream
    stage_of = {}
    cs = sorted({b.C for b in stack.blocks})
    for i, b in enumerate(stack.blocks):
        stage_of[i] = cs.index(b.C)
    order = []      # (block index) per mark, in issue order

    def hook(i):
        order.append(i)
        L.check(lib.dlka_trace_mark(st), "trace_mark")

    # every kernel on ONE stream while tracing: the timed step lets the weight gradients of a block overlap the next block's data chain on a second
    # stream (DLKABlockStack._overlap); events of two streams interleave in the trace and concurrent kernels stretch each other, so the per-kernel
    # durations are taken from the same launches run back to back
    overlap_was = getattr(stack, "_overlap", False)
    stack._overlap = False
    stack.forward_backward()            # warm
    torch.cuda.synchronize()
    # keep the host AHEAD of the device: the records measure back-to-back execution only if every launch is queued before its turn
    try:
        torch.cuda._sleep(int(60e6))
    except Exception:
        pass
    L.check(lib.dlka_trace_start(8192, st), "trace_start")
    try:
        for _ in range(reps):
            order.append(-1)
            L.check(lib.dlka_trace_mark(st), "trace_mark")
            stack.forward_backward(on_block=hook)
    finally:
        rc = lib.dlka_trace_stop()
        stack._overlap = overlap_was
    L.check(rc, "trace_stop")
    n = lib.dlka_trace_count()
    buf = create_string_buffer(512)
    ms = c_float()
    acc, mark_i, cur, total, overhead = {}, -1, -1, 0.0, []
    for i in range(n):
        L.check(lib.dlka_trace_get(i, buf, 512, byref(ms)), "trace_get")
        name = buf.value.decode()
        if name == "(mark)":
            mark_i += 1
            cur = order[mark_i]
            overhead.append(ms.value)
            continue
        key = (stage_of.get(cur, -1), name)
        a = acc.setdefault(key, [0, 0.0])
        a[0] += 1
        a[1] += ms.value
        total += ms.value
    out = {k: (v[0] / reps, v[1] / v[0]) for k, v in acc.items()}
    nrec = sum(v[0] for v in acc.values()) / reps
    return out, total / reps, (sorted(overhead)[len(overhead) // 2] if overhead else 0.0), nrec


def short_kernel(name):
    return name.replace("void dlka::", "").replace("dlka::", "").split("(")[0]


def roofline_report(stack, B, dtype, ms_per_step):
    from deformablelka_amd.stack import SYNAPSE_STAGES
    dbytes = 4 if dtype == torch.float32 else 2
    per, traced_ms, mark_ms, nrec = trace_step(stack)
    # every record also holds its timing event's own cost: (sum of records - the hipGraph replay of the same kernels) / records
    ev_us = max(0.0, (traced_ms - ms_per_step) / max(nrec, 1.0) * 1e3)
    rows = []
    for (stage, name), (cnt, ms) in per.items():
        C, (H, W, D), _ = SYNAPSE_STAGES[stage] if 0 <= stage < len(SYNAPSE_STAGES) else (0, (0, 0, 0), 0)
        fl, by = kernel_work(name, B, C, H * W * D, dbytes) if C else (0, 0)
        rows.append({"kernel": short_kernel(name), "stage": stage, "launches_per_step": round(cnt, 2), "avg_us": round(ms * 1e3, 2),
                     "step_share": round(cnt * ms / traced_ms, 4), "algorithmic_flops": fl, "algorithmic_bytes": by})
    rows.sort(key=lambda r: -r["step_share"])
    log("launch trace of the step (eager, HIP events behind every launch): %.3f ms of kernel time per step, graph replay %.3f ms" % (traced_ms, ms_per_step))
    for r in rows[:24]:
        fl, us = r["algorithmic_flops"], r["avg_us"]
        log(f"  s{r['stage']} {r['kernel'][:70]:70s} x{r['launches_per_step']:<5} {us:9.2f} us  {100 * r['step_share']:5.1f} %  "
            f"{fl / us / 1e6 if us else 0:8.2f} TFLOP/s  {r['algorithmic_bytes'] / us / 1e3 if us else 0:8.1f} GB/s")
    dom = rows[0]
    fl, by, t = dom["algorithmic_flops"], dom["algorithmic_bytes"], dom["avg_us"] * 1e-6
    # fp32-input MFMA peak = fp32 vector peak: the yardstick of the fp32 path (its forward contraction IS on that pipe; the backward Col contractions run as
    # two-term bf16 splits since round 4, which the same yardstick prices conservatively) — and, for comparability, of the bf16 path too
    peak_tf = PEAK_F32_TFLOPS
    ridge = peak_tf * 1e12 / (PEAK_HBM_GBS * 1e9)
    if by and fl / by > ridge:
        ach, peak, unit, bound = fl / t / 1e12, peak_tf, "TFLOP/s", "mfma"
    else:
        ach, peak, unit, bound = by / t / 1e9, PEAK_HBM_GBS, "GB/s", "hbm"
    traffic = traffic_source = None
    pmc = os.path.join(ROOT, "profiles", "pmc_traffic_block.json")   # rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over the stage blocks (scripts/pmc_block.sh)
    if os.path.exists(pmc):
        try:
            blob = json.load(open(pmc))
            ent = blob.get("stage%d_%s" % (dom["stage"], "f32" if dbytes == 4 else "bf16"), {}).get(dom["kernel"])
            if ent:
                traffic = ent["hbm_bytes_per_launch"]
                traffic_source = "profiles/pmc_traffic_block.json (%s): committed rocprofv3 --pmc passes over the same block, NOT measured by this run" % blob.get("_meta", {}).get("round", "?")
            else:   # the kernel was renamed / re-templated since the counters were taken: say so instead of quoting another kernel's bytes
                traffic_source = ("STALE: profiles/pmc_traffic_block.json (%s) has no entry for this kernel name — re-run scripts/pmc_block.sh; "
                                  "tests/test_parity_gpu.py::test_pmc_traffic_file_names_the_step_kernels fails in this state" % blob.get("_meta", {}).get("round", "?"))
                log("WARNING: roofline.traffic is null:", traffic_source)
        except Exception:
            traffic = None
    C, (H, W, D), _ = SYNAPSE_STAGES[dom["stage"]]
    extra = {}
    if dbytes == 2 and bound == "mfma":   # the bf16 step's dominant kernel contracts on the bf16 matrix cores — its fraction of THAT pipe as well
        extra = {"frac_of_bf16_mfma_peak": round(ach / PEAK_BF16_TFLOPS, 5), "bf16_mfma_peak_TFLOPs": PEAK_BF16_TFLOPS}
    return {"bound": bound, "achieved": round(ach, 3), "peak": peak, "unit": unit, "frac": round(ach / peak, 5), **extra,
            "traffic": traffic, "traffic_source": traffic_source, "kernel": dom["kernel"], "kernel_us": dom["avg_us"],
            "kernel_us_less_event_cost": round(dom["avg_us"] - ev_us, 2),
            "launches_per_step": dom["launches_per_step"], "step_share": dom["step_share"],
            "algorithmic_flops": fl, "algorithmic_bytes": by, "shape": f"C={C},{H}x{W}x{D},B={B}",
            "method": "HIP events recorded on the launch stream behind EVERY kernel launch of the step's own forward+backward (library launch trace, "
                      "eager replay of the same call sequence the hipGraph holds, all on one stream — the timed step overlaps the weight gradients of a block "
                      "with the next block's data chain on a second stream; mean over 3 passes); dominant = largest launches x duration",
            "traced_kernel_ms_per_step": round(traced_ms, 4), "records_per_step": round(nrec, 1),
            "event_cost_us": {"per_record_vs_graph_replay": round(ev_us, 2), "two_events_back_to_back": round(mark_ms * 1e3, 2),
                              "note": "`achieved` uses the raw record (kernel + its event), i.e. it UNDERSTATES the kernel by this much"},
            "kernels": rows[:16]}


# ----------------------------------------------------------------------------------------------------------------
# CPU baseline: the oracle block on the host cores, bounded sample
# ----------------------------------------------------------------------------------------------------------------
def cpu_baseline(sample, batch, budget_s=40.0):
    """the oracle block (ATen CPU convs = the reference's own CPU path for nn.Conv3d/GELU, C oracle for the deformable conv,
    autograd backward) on the host cores — B = `batch`, fp32, offsets ~1 voxel, every one of the four stage shapes timed (no
    extrapolation between stages; the 21-block time is 6*t0 + 6*t1 + 6*t2 + 3*t3 of MEASURED per-stage medians).  Protocol per stage:
    warm-up + timed repetitions, median; BOUNDED: the plan's 3 warm + 10 timed shrink to what fits the time budget and the counts
    actually run are reported.  All host threads, then one thread (per-core figure) on the stages that still fit the budget."""
    import statistics
    import oracle
    from oracle import blocks
    import deformablelka_amd as dk
    from deformablelka_amd.stack import _offset_std_for
    oracle.build()
    cores = torch.get_num_threads()
    if sample == "tiny":
        stages = [(32, (8, 8, 8), 6), (64, (4, 4, 4), 6)]
    else:
        from deformablelka_amd.stack import SYNAPSE_STAGES
        stages = SYNAPSE_STAGES
    # untimed warm-up (thread pools, oneDNN primitive caches)
    _m = dk.LKA_Attention3d_deform(8)
    _P = {k: v.detach().clone().requires_grad_(True) for k, v in _m.state_dict().items()}
    blocks.lka3d_attention_volume(torch.randn(1, 8, 6, 6, 6, requires_grad=True), _P).sum().backward()

    def make(C, dims):
        torch.manual_seed(0)
        m = dk.LKA_Attention3d_deform(C)
        blocks.randomize_offsets_(m, std=_offset_std_for(C))
        P = {k: v.detach().clone().requires_grad_(True) for k, v in m.state_dict().items()}
        return P, torch.randn(batch, C, *dims, requires_grad=True), torch.randn(batch, C, *dims)

    def once(P, x, gy):
        t0 = time.perf_counter()
        blocks.lka3d_attention_volume(x, P).backward(gy)
        return time.perf_counter() - t0

    t_start = time.perf_counter()
    per_stage, reps = [], []
    share = budget_s * 0.7 / len(stages)
    for C, dims, nblk in reversed(list(stages)):        # small stages first: they always get their full repetitions
        P, x, gy = make(C, dims)
        t_stage = time.perf_counter()
        warm = 0
        while warm < 3 and (warm == 0 or time.perf_counter() - t_stage < share * 0.3):
            once(P, x, gy)
            warm += 1
        ts = []
        while len(ts) < 10 and (len(ts) < 1 or time.perf_counter() - t_stage < share):
            ts.append(once(P, x, gy))
        per_stage.insert(0, statistics.median(ts))
        reps.insert(0, (warm, len(ts)))
    total = sum(t * n for t, (_, _, n) in zip(per_stage, stages))
    # one thread
    one = {}
    torch.set_num_threads(1)
    os.environ["OMP_NUM_THREADS"] = "1"
    try:
        import ctypes
        try:
            ctypes.CDLL("libgomp.so.1").omp_set_num_threads(1)    # the C oracle's OpenMP team
        except OSError:
            pass
        for (C, dims, nblk), t_all in reversed(list(zip(stages, per_stage))):
            if time.perf_counter() - t_start + t_all * cores * 0.5 > budget_s:   # would not fit: say so instead of extrapolating
                one[f"C{C}"] = None
                continue
            P, x, gy = make(C, dims)
            once(P, x, gy)
            one[f"C{C}"] = round(once(P, x, gy), 4)
    finally:
        torch.set_num_threads(cores)
        try:
            ctypes.CDLL("libgomp.so.1").omp_set_num_threads(cores)
        except Exception:
            pass
    return {"value": round(batch / total, 5), "unit": "volumes/s", "cores": cores, "kind": "port",
            "sample": (f"oracle D-LKA block fwd+bwd at B={batch}, fp32, offsets ~1 voxel, one block of EACH of the 4 stage shapes timed "
                       f"(warm-up, timed repetitions per stage C=32/64/128/256: {reps}; median), 21-block time = 6*t0+6*t1+6*t2+3*t3; "
                       f"bounded to ~{budget_s:.0f} s (BASELINE.md §3 asks 3 warm + 10 timed)" if sample != "tiny" else "TINY shapes (debug only)"),
            "per_stage_block_s": [round(t, 4) for t in per_stage], "one_thread_block_s": one,
            "offline_protocol": ("profiles/r05z_cpu_baseline_protocol.json: the full BASELINE.md section 3 protocol (3 warm + 10 timed per stage, all four single-thread blocks: "
                                 "16.8 / 4.62 / 1.21 / 0.39 s) run offline on a GPU box's host by scripts/cpu_baseline_protocol.py; the in-run sample above is bounded and leaves "
                                 "a single-thread figure None where it would not fit"),
            "torch": torch.__version__,
            "wall_s": round(time.perf_counter() - t_start, 1)}


def step_work(batch, dbytes):
    """Algorithmic FLOPs and bytes of ONE step (fwd+bwd of the 21 blocks at B = batch), SURVEY.md §8d: bytes fwd+bwd = 43 E + 5 Off
    words per block (activations in the run's storage type, offsets always fp32), FLOPs = 3 x forward."""
    from deformablelka_amd.stack import SYNAPSE_STAGES
    fl = by = 0
    for C, (H, W, D), n in SYNAPSE_STAGES:
        N = H * W * D
        E, Off = batch * C * N, batch * 81 * N
        fwd = 6 * C * E + 936 * E + 2 * 27 * C * 81 * batch * N + 2 * 27 * C * C * batch * N + 27 * batch * N * (15 * C + 30)
        fl += n * 3 * fwd
        by += n * (43 * E * dbytes + 5 * Off * 4)
    return fl, by


DUMP_BUDGET_BYTES = 60_000_000   # --dump-outputs writes at most this much (float32)
DUMP_FLAT_SAMPLE = 1 << 20       # elements kept of the flat parameter / gradient buffers


def _seeded_sample(t, k, seed):
    """t flattened, or k of its elements at fixed positions (seeded, ascending) when it holds more."""
    flat = t.detach().reshape(-1)
    if flat.numel() <= k:
        return flat
    idx = torch.randperm(flat.numel(), generator=torch.Generator().manual_seed(seed))[:k].sort().values
    return flat[idx.to(flat.device)]


def dump_outputs(stack, out_dir):
    """What a caller of the timed step holds after the LAST step: per chain (stage instance, execution order) the output of its last block
    (`y`, [B, N, C]) and the gradient w.r.t. its input (`grad_x`), and the flat fp32 parameter and gradient buffers after the SGD update.  All as
    float32.  The flat buffers are always a fixed seeded sample of DUMP_FLAT_SAMPLE elements; the activations are written whole when they fit
    the budget, else each is a fixed seeded sample of the same fraction of its elements.  Returns {name: shape}."""
    import numpy as np
    acts = []
    for k, chain in enumerate(stack.chains):
        tag = "chain%d_C%d" % (k, chain[0].C)
        acts.append(("y_" + tag, chain[-1].y))
        acts.append(("grad_x_" + tag, chain[0].gx))
    flat = [("params_sample", stack.flat_params), ("grads_sample", stack.flat_grads)]
    room = DUMP_BUDGET_BYTES // 4 - sum(min(t.numel(), DUMP_FLAT_SAMPLE) for _, t in flat)
    total = sum(t.numel() for _, t in acts)
    arrays = []
    for i, (name, t) in enumerate(acts):
        if total <= room:
            arrays.append((name, t.detach()))
        else:
            arrays.append((name + "_sample", _seeded_sample(t, max(1, t.numel() * room // total), 1000 + i)))
    arrays += [(name, _seeded_sample(t, DUMP_FLAT_SAMPLE, 2000 + i)) for i, (name, t) in enumerate(flat)]
    os.makedirs(out_dir, exist_ok=True)
    shapes = {}
    for name, t in arrays:
        a = t.float().cpu().numpy()
        np.save(os.path.join(out_dir, name + ".npy"), a)
        shapes[name] = list(a.shape)
    return shapes


def tblock_metric(batch, steps, warmup, dev, overlap=False):
    """Second reported metric: the same 21 blocks INSIDE their wrapper (TransformerBlock_3D_single_deform_LKA: LayerNorm, gamma residual,
    UnetResBlock, conv8 — SURVEY.md §8 rows a1/f1), fwd+bwd through the nn.Module / autograd path, chained per stage instance."""
    import deformablelka_amd as dk
    from deformablelka_amd.stack import SYNAPSE_STAGES, CHAIN, _offset_std_for
    torch.manual_seed(0)
    chains = []
    for C, (H, W, D), n in SYNAPSE_STAGES:
        for c0 in range(0, n, CHAIN):
            mods = []
            for _ in range(min(CHAIN, n - c0)):
                m = dk.TransformerBlock_3D_single_deform_LKA(H * W * D, C, C, 4, dropout_rate=0.1, pos_embed=True)
                with torch.no_grad():
                    m.epa_block.spatial_gating_unit.deform_conv.conv_offset.weight.normal_(0, _offset_std_for(C))
                m.keep_channels_last = True
                m.wgrad_overlap = overlap   # the weight gradients on a side stream, joined at the end of backward() (transformerblock.WgradOverlap)
                mods.append(m.to(dev))
            x = torch.randn(batch, H, W, D, C, device=dev).permute(0, 4, 1, 2, 3).requires_grad_(True)
            gy = torch.randn(batch, H, W, D, C, device=dev).permute(0, 4, 1, 2, 3)
            chains.append((mods, x, gy))

    params = [p for mods, _, _ in chains for m in mods for p in m.parameters()] + [x for _, x, _ in chains]

    def step():
        # as the trainer's iteration does (optimizer.zero_grad(), set_to_none): without it autograd ACCUMULATES into the existing .grad tensors —
        # one extra elementwise add launch per parameter and block (26 x 21 x 4.7 us = 2.6 ms of a 21.4 ms step, rocprofv3 of scripts/prof_tblock.py)
        for p in params:
            p.grad = None
        for mods, x, gy in chains:
            y = x
            for m in mods:
                y = m(y)
            y.backward(gy)

    for _ in range(max(warmup, 2)):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    out = {"metric": "3D D-LKA transformer-block (wrapper + D-LKA) fwd+bwd volumes/sec (64x128x128)", "value": round(batch / dt, 3),
           "unit": "volumes/s", "ms_per_step": round(dt * 1e3, 3), "path": "nn.Module + autograd, eager (no hipGraph), training mode" + (", weight gradients on a side stream joined at the end of backward()" if overlap else ""),
           "blocks": sum(len(c[0]) for c in chains)}
    # the same nn.Module step captured in a hipGraph (autograd Functions launch on the capturing stream, outputs come from the graph's pool)
    try:
        for p in params:
            p.grad = None
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            step()
        for _ in range(2):
            g.replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            g.replay()
        torch.cuda.synchronize()
        dg = (time.perf_counter() - t0) / steps
        out["hipgraph"] = {"value": round(batch / dg, 3), "ms_per_step": round(dg * 1e3, 3), "path": "the same nn.Module step, captured once and replayed"}
    except Exception as e:   # capture is an extra: the eager figure above stands on its own
        out["hipgraph"] = {"error": repr(e)[:200]}
    return out


def lka_modules_metric(batch, steps, warmup, dev, overlap=True):
    """The headline's 21 D-LKA blocks as the TRAINERS call them (north_star: "exposed through PyTorch-ROCm as torch.autograd.Functions that keep the exact nn.Module
    signatures"): `LKA_Attention3d_deform.forward(x, B, C, H, W, D)` modules chained per stage instance through autograd — same shapes, same offset calibration, same
    block count as the engine step above; eager and replayed from a hipGraph.  overlap: `module.wgrad_overlap = True` — the engine's side-stream weight-gradient schedule
    for the module path (transformerblock.WgradOverlap: one join at the end of backward())."""
    import deformablelka_amd as dk
    from deformablelka_amd.stack import SYNAPSE_STAGES, chain_order, _offset_std_for
    torch.manual_seed(0)
    chains = []
    for C, (H, W, D), n in chain_order(SYNAPSE_STAGES):
        mods = []
        for _ in range(n):
            m = dk.LKA_Attention3d_deform(C)
            with torch.no_grad():
                m.spatial_gating_unit.deform_conv.conv_offset.weight.normal_(0, _offset_std_for(C))
            m.wgrad_overlap = overlap
            mods.append(m.to(dev))
        x = torch.randn(batch, H * W * D, C, device=dev, requires_grad=True)
        gy = torch.randn(batch, H * W * D, C, device=dev)
        chains.append((mods, x, gy, (batch, C, H, W, D)))
    params = [p for mods, _, _, _ in chains for m in mods for p in m.parameters()] + [x for _, x, _, _ in chains]

    def step():
        for p in params:
            p.grad = None
        for mods, x, gy, shp in chains:
            y = x
            for m in mods:
                y = m(y, *shp)
            y.backward(gy)

    for _ in range(max(warmup, 2)):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    out = {"metric": "3D D-LKA fwd+bwd volumes/sec (64x128x128), the 21 blocks through LKA_Attention3d_deform modules + autograd", "value": round(batch / dt, 3),
           "unit": "volumes/s", "ms_per_step": round(dt * 1e3, 3), "blocks": sum(len(c[0]) for c in chains),
           "path": "nn.Module + torch.autograd.Function, eager" + (", weight gradients on a side stream joined at the end of backward()" if overlap else "")}
    try:
        for p in params:
            p.grad = None
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            step()
        for _ in range(2):
            g.replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            g.replay()
        torch.cuda.synchronize()
        dg = (time.perf_counter() - t0) / steps
        out["hipgraph"] = {"value": round(batch / dg, 3), "ms_per_step": round(dg * 1e3, 3), "path": "the same nn.Module step, captured once and replayed"}
    except Exception as e:
        out["hipgraph"] = {"error": repr(e)[:200]}
    return out


def fullnet_metric(batch, steps, dev, bf16=False):
    """Third metric (SURVEY §8d iii / §8f-2): the WHOLE D_LKA_Former (42.35 M parameters; its 21 D-LKA transformer blocks on this repo's kernels,
    the conv / norm plumbing around them as GEMM re-expressions, HIP 3^3 convs and planar HIP norms), one trainer iteration per step — forward, deep-supervision loss, backward,
    clip_grad_norm_(12), SGD(momentum 0.99, nesterov) — on a synthetic 64x128x128 patch batch (d_lka_former_trainer_synapse.py:259-309)."""
    from deformablelka_amd import training
    from deformablelka_amd.stack import _offset_std_for
    torch.manual_seed(0)
    net = training.initialize_network(1, 14, (64, 128, 128), device=dev)
    with torch.no_grad():
        for blk in net.dlka_blocks():
            w = blk.epa_block.spatial_gating_unit.deform_conv.conv_offset.weight
            w.normal_(0, _offset_std_for(w.shape[1]))
    opt = training.initialize_optimizer(net, initial_lr=1e-6)
    x = torch.randn(batch, 1, 64, 128, 128, device=dev)
    tgt = torch.randint(0, 14, (batch, 64, 128, 128), device=dev)
    net.train()
    for _ in range(2):
        training.run_iteration(net, opt, x, tgt, bf16_autocast=bf16)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = training.run_iteration(net, opt, x, tgt, bf16_autocast=bf16)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    if not bool(torch.isfinite(loss)):
        raise RuntimeError("full-net loss is not finite")
    graphed = None
    if not bf16:
        try:   # the same iteration as one hipGraph launch (training.GraphedIteration)
            it = training.GraphedIteration(net, opt, x, tgt)
            for _ in range(2):
                it()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                gl = it()
            torch.cuda.synchronize()
            dg = (time.perf_counter() - t0) / steps
            if bool(torch.isfinite(gl)):
                graphed = {"value": round(batch / dg, 3), "ms_per_step": round(dg * 1e3, 2), "loss": round(float(gl), 4),
                           "path": "the same trainer iteration captured once in a hipGraph and replayed (training.GraphedIteration)"}
        except Exception as e:
            graphed = {"error": repr(e)[:200]}
    return {"metric": "3D D-LKA Former full-net training iteration volumes/sec (64x128x128)", "value": round(batch / dt, 3), "unit": "volumes/s",
            "hipgraph": graphed,
            "ms_per_step": round(dt * 1e3, 2), "params": sum(p.numel() for p in net.parameters()), "loss": round(float(loss), 4),
            "path": "nn.Module + autograd, eager; D-LKA blocks = HIP kernels; plumbing: stride == kernel convs = patchify / depth-to-space GEMMs (rocBLAS), 3^3 and 1x1x1 convs "
                    "and Instance / Batch / long-row GroupNorm = HIP kernels (the full-resolution 3^3 convs on the matrix cores in all three directions), loss and "
                    "optimizer (single-pass SGD) = torch" +
                    ("; torch.autocast(bf16) around forward + loss: torch layers only — the transformer blocks and the conv re-expressions stay on their fp32 paths" if bf16 else "")}


def lka2d_metric(steps, dev, dtype=torch.float32, with_cpu=False):
    """Secondary metric of SURVEY §8d / BASELINE.json config 2: the 2-D D-LKA attention block fwd+bwd at B=24 on the three decoder shapes of the
    224^2 net (2D/networks/MaxViT_deform_LKA.py:643-679), two blocks each — images/s through deformable_LKA_Attention, with the activation storage
    type `dtype` (bf16 = config 2 as written: "bf16 training"; fp32 parameters either way).  Also: the launch-trace roofline of its dominant kernel
    and (with_cpu) the BASELINE.md §3 "2D companion": the oracle block on the host cores, bounded."""
    import deformablelka_amd as dk
    from deformablelka_amd.init_utils import randomize_offset_nets
    shapes = [(384, 14), (192, 28), (96, 56)]
    torch.manual_seed(0)
    mods, xs, gys = [], [], []
    for C, n in shapes:
        for _ in range(2):
            m = dk.deformable_LKA_Attention(C).to(dev)
            randomize_offset_nets(m, 0.02)
            mods.append(m)
            xs.append(torch.randn(24, C, n, n, device=dev).to(dtype).requires_grad_(True))
            gys.append(torch.randn(24, C, n, n, device=dev).to(dtype))

    def step():
        for m, x, gy in zip(mods, xs, gys):
            m(x).backward(gy)
    for _ in range(2):
        step()
    torch.cuda.synchronize()
    per = []
    for m, x, gy in zip(mods[::2], xs[::2], gys[::2]):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            m(x).backward(gy)
        e1.record()
        torch.cuda.synchronize()
        per.append(round(e0.elapsed_time(e1) / steps, 3))
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    out = {"metric": "2D D-LKA attention blocks fwd+bwd images/sec (224x224 net, B=24: 2x(384,14^2)+2x(192,28^2)+2x(96,56^2))", "value": round(24 / dt, 2),
           "unit": "images/s", "dtype": "bf16" if dtype == torch.bfloat16 else "f32", "ms_per_step": round(dt * 1e3, 2),
           "ms_per_block_fwd_bwd": dict(zip(["384x14^2", "192x28^2", "96x56^2"], per))}
    # ---- launch trace of one step: per-kernel durations, dominant kernel, roofline ----
    try:
        from ctypes import byref, c_float, create_string_buffer
        from deformablelka_amd import _lib as L
        lib = L.get_lib()
        st = torch.cuda.current_stream(dev).cuda_stream
        try:
            torch.cuda._sleep(int(60e6))
        except Exception:
            pass
        # ONE stream for the traced pass (DLKA_LKA2D_FORK=0): with the library's internal fork streams on, the events behind a launch bracket whatever else runs beside it
        # and are not the kernel's duration; `value` above was timed with the forks on
        prev_fork = os.environ.get("DLKA_LKA2D_FORK")
        os.environ["DLKA_LKA2D_FORK"] = "0"
        lib.dlka_env_refresh()
        try:
            m0, x0, gy0 = mods[0], xs[0], gys[0]
            m0(x0).backward(gy0)   # (the one-stream path's first call outside the trace)
            torch.cuda.synchronize()
            L.check(lib.dlka_trace_start(8192, st), "trace_start")
            try:
                for i, (m, x, gy) in enumerate(zip(mods, xs, gys)):
                    L.check(lib.dlka_trace_mark(st), "trace_mark")
                    m(x).backward(gy)
            finally:
                rc = lib.dlka_trace_stop()
            L.check(rc, "trace_stop")
        finally:
            if prev_fork is None:
                os.environ.pop("DLKA_LKA2D_FORK", None)
            else:
                os.environ["DLKA_LKA2D_FORK"] = prev_fork
            lib.dlka_env_refresh()
        buf, ms, acc, blk, total = create_string_buffer(512), c_float(), {}, -1, 0.0
        for i in range(lib.dlka_trace_count()):
            L.check(lib.dlka_trace_get(i, buf, 512, byref(ms)), "trace_get")
            name = buf.value.decode()
            if name == "(mark)":
                blk += 1
                continue
            a = acc.setdefault((blk // 2, short_kernel(name)), [0, 0.0])
            a[0] += 1
            a[1] += ms.value
            total += ms.value
        rows = sorted(((v[1], k, v[0]) for k, v in acc.items()), reverse=True)
        dbytes = 2 if dtype == torch.bfloat16 else 4
        kern = []
        for tot, (si, name), cnt in rows[:int(os.environ.get("DLKA_BENCH_2D_ROWS", "10"))]:
            kern.append({"kernel": name, "shape": "C=%d,%dx%d" % (shapes[si][0], shapes[si][1], shapes[si][1]), "launches_per_step": cnt,
                         "avg_us": round(tot / cnt * 1e3, 2), "step_share": round(tot / total, 4)})
        tot, (si, name), cnt = rows[0]
        C, n = shapes[si]
        M, E = 24 * n * n, 24 * C * n * n
        t = tot / cnt * 1e-3
        # algorithmic work of the dominant kernel's operator: offset nets 2*K*C*2K flops per pixel, in E + offsets out;
        # depthwise deformable conv K taps x (7 flops blend + 2 MAC) per channel, x / offsets in, out
        if "igemm" in name or "conv_wave" in name or "wgrad_dense" in name:
            big = True   # the 7x7 net dominates where both exist under one name; report the mean over the launches it aggregates
            fl = 2 * C * M * (25 * 50 + 49 * 98) / 2
            by = E * dbytes + M * (50 + 98) / 2 * 4
        elif "ddw2d" in name:
            fl = M * C * (25 + 49) / 2 * 9
            by = 2 * E * dbytes + M * (50 + 98) / 2 * 4
        else:
            fl, by = 2 * C * E, 2 * E * dbytes
        ridge = PEAK_F32_TFLOPS * 1e12 / (PEAK_HBM_GBS * 1e9)
        if by and fl / by > ridge:
            ach, peak, unit, bound = fl / t / 1e12, PEAK_F32_TFLOPS, "TFLOP/s", "mfma"
        else:
            ach, peak, unit, bound = by / t / 1e9, PEAK_HBM_GBS, "GB/s", "hbm"
        traffic, traffic_source = None, "no profiles/pmc_traffic_lka2d.json entry for this kernel and shape (scripts/pmc_lka2d.sh)"
        try:   # HBM bytes per launch from the committed rocprofv3 --pmc passes over the same block (NOT measured by this run; launches of both convs / nets averaged)
            blob = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic_lka2d.json")))
            ent = blob.get("stage2d_C%d_bf16" % C, {}).get(name) if dtype == torch.bfloat16 else None
            if ent:
                traffic = ent["hbm_bytes_per_launch"]
                traffic_source = "profiles/pmc_traffic_lka2d.json (%s): committed rocprofv3 --pmc passes, NOT measured by this run" % blob.get("_meta", {}).get("round", "?")
        except Exception:
            pass
        out["roofline"] = {"bound": bound, "achieved": round(ach, 3), "peak": peak, "unit": unit, "frac": round(ach / peak, 5), "traffic": traffic, "traffic_source": traffic_source,
                           "kernel": name, "kernel_us": round(t * 1e6, 2), "shape": "C=%d,%dx%d,B=24" % (C, n, n), "algorithmic_flops": fl,
                           "algorithmic_bytes": by, "method": "library launch trace (HIP events behind every launch), one eager step on ONE stream (DLKA_LKA2D_FORK=0): the durations are the kernels' own",
                           "kernels": kern}
        if bound == "mfma" and dtype == torch.bfloat16:   # the offset nets' contractions run on bf16 MFMA (three-term operands) in this mode
            out["roofline"].update({"frac_of_bf16_mfma_peak": round(ach / PEAK_BF16_TFLOPS, 5), "bf16_mfma_peak_TFLOPs": PEAK_BF16_TFLOPS})
    except Exception as e:
        log("lka2d launch trace failed:", repr(e))
    if with_cpu:
        try:
            out["cpu_baseline"] = lka2d_cpu_baseline()
        except Exception as e:
            log("lka2d cpu baseline failed:", repr(e))
    return out


def lka2d_cpu_baseline(budget_s=25.0):
    """BASELINE.md §3 "2D companion": the oracle 2-D block (ATen CPU convs for the offset nets / projections = the reference's own CPU path for
    nn.Conv2d, the C restatement of torchvision's deform_conv2d for the deformable convs, autograd backward) fwd+bwd at B=24 on the three decoder
    shapes, all host threads; bounded — repetitions actually run are reported."""
    import statistics
    import oracle
    from oracle import blocks
    import deformablelka_amd as dk
    from deformablelka_amd.init_utils import randomize_offset_nets
    oracle.build()
    cores = torch.get_num_threads()
    per, reps = [], []
    t_start = time.perf_counter()
    for C, n in [(384, 14), (192, 28), (96, 56)]:
        torch.manual_seed(0)
        m = dk.deformable_LKA_Attention(C)
        randomize_offset_nets(m, 0.02)
        P = {k: v.detach().clone().requires_grad_(True) for k, v in m.state_dict().items()}
        x, gy = torch.randn(24, C, n, n, requires_grad=True), torch.randn(24, C, n, n)

        def once():
            t0 = time.perf_counter()
            blocks.lka2d_attention(x, P).backward(gy)
            return time.perf_counter() - t0
        once()
        ts = []
        while len(ts) < 5 and (len(ts) < 1 or time.perf_counter() - t_start < budget_s * (len(per) + 1) / 3):
            ts.append(once())
        per.append(statistics.median(ts))
        reps.append(len(ts))
    total = 2 * sum(per)
    return {"value": round(24 / total, 4), "unit": "images/s", "cores": cores, "kind": "port",
            "sample": f"oracle 2-D D-LKA block fwd+bwd at B=24, fp32, one block of each of the 3 decoder shapes timed (1 warm-up, {reps} timed, median), "
                      f"step = 2 blocks per shape; bounded to ~{budget_s:.0f} s (BASELINE.md §3 asks 3 + 10)",
            "per_block_s": [round(t, 4) for t in per], "wall_s": round(time.perf_counter() - t_start, 1)}


def inference_metric(dev):
    """BASELINE.json config 5: pancreas-style sliding-window inference, 96^3 tiles, stride 16, on a synthetic (240, 240, 160) volume =
    10 x 10 x 5 = 500 tiles (test_util.py:73-75), the volume, score map and counts resident in HBM; tiles/s, forward only."""
    from deformablelka_amd import inference, training
    torch.manual_seed(0)
    net = training.initialize_network(1, 2, (96, 96, 96), device=dev, patch_size=(2, 2, 2)).eval()
    net.do_ds = False
    vol = torch.randn(240, 240, 160, device=dev)
    small = vol[:112, :112, :96].contiguous()          # warm-up: 2 x 2 x 1 tiles
    inference.predict_single_case(net, small, 16, 16, (96, 96, 96), num_classes=2, tile_batch=4)
    torch.cuda.synchronize()
    n = inference.num_tiles(vol.shape, (96, 96, 96), 16, 16)
    t0 = time.perf_counter()
    lab, score = inference.predict_single_case(net, vol, 16, 16, (96, 96, 96), num_classes=2, tile_batch=4)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert lab.shape == vol.shape and bool(torch.isfinite(score).all())
    return {"metric": "3D D-LKA Former sliding-window inference tiles/sec (96^3 tiles, stride 16, 240x240x160 volume resident in HBM)",
            "value": round(n / dt, 2), "unit": "tiles/s", "tiles": n, "seconds_per_volume": round(dt, 2), "tile_batch": 4}


def inference_config5_metric(dev):
    """BASELINE.json config 5 AS WRITTEN: "40x224x224 tiles".  Such a tile only divides through the ACDC net's stem (1,4,4)
    (acdc/model_components.py:21) -> per-tile stage shapes 40x56x56 / 20x28x28 / 10x14x14 / 5x7x7 at C = 32 / 64 / 128 / 256, with the ACDC variant's
    anisotropic depthwise kernels (acdc/transformerblock.py:213-237) — deformablelka_amd.acdc on the fused kernels.  Synthetic stand-in volume
    (the dataset is not in the reference): 80 x 448 x 448 = 3 x 3 x 3 = 27 tiles at nnU-Net's step 0.5 with Gaussian blending
    (neural_network.py:292-428), the padded volume, score map and weights resident in HBM; tiles/s, forward only."""
    from deformablelka_amd import acdc, inference, training
    torch.manual_seed(0)
    tile = (40, 224, 224)
    net = training.initialize_network(1, 4, tile, device=dev, patch_size=(1, 4, 4), trans_block=acdc.TransformerBlock_3D_single_deform_LKA).eval()
    net.do_ds = False
    vol = torch.randn(1, 80, 448, 448, device=dev)
    # warm-up with the SAME volume: the score map / padded volume of the full size are allocated once, every kernel of the 27-tile pass has run (a two-tile
    # warm-up left 0.2 s of first-use cost in a 0.4 s measurement: 47 - 70 tiles/s from run to run)
    inference.predict_3d_tiled(net, vol, tile, 0.5, True, num_classes=4, tile_batch=2)
    torch.cuda.synchronize()
    steps_ = inference.compute_steps_for_sliding_window(tile, vol.shape[1:], 0.5)
    n = len(steps_[0]) * len(steps_[1]) * len(steps_[2])
    t0 = time.perf_counter()
    seg, probs = inference.predict_3d_tiled(net, vol, tile, 0.5, True, num_classes=4, tile_batch=2)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert seg.shape == vol.shape[1:] and bool(torch.isfinite(probs).all())
    return {"metric": "3D D-LKA Former (ACDC variant, stem (1,4,4)) sliding-window inference tiles/sec (40x224x224 tiles, step 0.5, Gaussian blending, "
                      "80x448x448 volume resident in HBM)", "value": round(n / dt, 2), "unit": "tiles/s", "tiles": n, "seconds_per_volume": round(dt, 2),
            "tile_batch": 2, "stage_shapes": "40x56x56 / 20x28x28 / 10x14x14 / 5x7x7"}


def companion_metric(batch, steps, warmup, dev, dtype, lr, roofline=True):
    """The same stack step (fwd + bwd of the 21 blocks + SGD update, hipGraph replay) with the OTHER activation storage type — reported next to
    the headline so that one default run shows both: fp32 (the reference's arithmetic, 1e-4 parity) and bf16 activations (north_star's target
    dtype; parity against the bf16-storage oracle)."""
    from deformablelka_amd.stack import DLKABlockStack
    from deformablelka_amd import dp
    st = DLKABlockStack(batch, device=dev, dtype=dtype, seed=1234, data_seed=4321)
    st.forward_backward()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st.forward_backward()

    def step():
        dp.step_single(st, lr, 1, None, g.replay)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    h = st.health()
    if not h["finite"]:
        raise RuntimeError(f"non-finite parameters or gradients: {h}")
    out = {"dtype": "bf16" if dtype == torch.bfloat16 else "f32", "value": round(batch * steps / el, 3), "unit": "volumes/s",
           "ms_per_step": round(el / steps * 1e3, 4), "steps": steps, "offset_std_voxels_by_stage": h["offset_std"]}
    if roofline:   # the same launch-trace roofline block as the headline's, for this dtype's step (round-4 verdict: none existed for the bf16 step)
        try:
            r = roofline_report(st, batch, dtype, el / steps * 1e3)
            r["kernels"] = r["kernels"][:8]
            out["roofline"] = r
        except Exception as e:
            log("companion roofline failed:", repr(e))
    return out


def spawn_ranks(args, harness=None):
    """`python bench.py --gpus N` with no WORLD_SIZE in the environment: start the N ranks ourselves (one process per GPU, torch.distributed.run
    = torchrun, rendezvous on 127.0.0.1) with the same arguments; rank 0 of the child job prints the JSON line on the inherited stdout."""
    import socket
    import subprocess
    if harness is None:
        have = torch.cuda.device_count()
        if have < args.gpus:
            raise SystemExit(f"bench.py --gpus {args.gpus}: only {have} GPU(s) visible on this node")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(sys.argv[0])] + sys.argv[1:]   # (sys.argv[0]: this file, or the test harness that calls main())
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    log("bench.py: spawning", args.gpus, "ranks:", " ".join(cmd))
    raise SystemExit(subprocess.call(cmd, env=env))


def main(harness=None):
    """harness: None for every measurement.  tests/bench_emu_harness.py passes a dict {"device", "process_group", "stages", "data", "setup"} to run the RANK LOGIC of this
    file — self-spawn, process group, shard seeds, barrier + max-over-ranks timing, the JSON line — on CPU tensors and `gloo` with the host emulator build of the kernels and
    a two-block toy stack (tests/test_bench_spawn.py); the line it prints says so in `data`, it is never a measurement, and nothing in this file imports test code."""
    EMU = harness is not None
    args = parse()
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        spawn_ranks(args, harness)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world} (launch N ranks, or let --gpus N spawn them)")
    if EMU:
        harness["setup"]()
        dev = harness["device"]
        args.no_graph = args.no_roofline = args.no_cpu_baseline = args.no_companion = args.no_tblock = args.no_fullnet = args.no_lka2d = True
    else:
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs an MI355X (torch.cuda.is_available() is False); there is no CPU fallback")
        if local_rank >= torch.cuda.device_count():
            raise SystemExit(f"bench.py: rank {rank} has no GPU of its own (LOCAL_RANK {local_rank}, {torch.cuda.device_count()} visible)")
        torch.cuda.set_device(local_rank)
        dev = torch.device("cuda", local_rank)
    sync = (lambda: None) if EMU else torch.cuda.synchronize
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if EMU:
            dist.init_process_group(harness["process_group"])
        else:
            dist.init_process_group("nccl", device_id=dev)  # nccl == RCCL on ROCm; ranks talk over xGMI
        if dist.get_world_size() != args.gpus:
            raise SystemExit(f"bench.py: the process group has {dist.get_world_size()} ranks, --gpus {args.gpus}")

    from deformablelka_amd.stack import DLKABlockStack
    dtype = torch.float32 if args.dtype == "f32" else torch.bfloat16
    # replicas start from the same parameters (seed); every rank gets its own shard of synthetic volumes (data_seed)
    stack = DLKABlockStack(args.batch, device=dev, dtype=dtype, seed=1234, data_seed=4321 + rank, **({"stages": harness["stages"]} if EMU else {}))
    # Synthetic grad_outputs (N(0,1), no loss behind them) make the block gradients huge; a training-sized step would blow
    # the parameters up within a few iterations (offsets -> inf/NaN, every sample dropped, kernels get FASTER: observed,
    # profiles/archive/r01i).  The SGD update is executed in full but with a step small enough that the data distribution the
    # kernels see (offset std ~ 1 voxel) is the same in the last timed step as in the first; checked after the run.
    lr = 1e-12

    def compute():
        stack.forward_backward()

    # N > 1: the step is cut where the backward pass has produced most of the gradient bytes (the C = 256 / 128 blocks come first in the
    # backward order and hold 84 % of them): their all-reduce runs on RCCL's stream while the second half of the backward pass computes.
    overlap = world > 1 or os.environ.get("DLKA_BENCH_FORCE_SPLIT") is not None
    if os.environ.get("DLKA_BENCH_NO_OVERLAP") is not None:
        overlap = False
    split = stack.split_index() if overlap else 0
    if split <= 0 or split >= len(stack.blocks):
        overlap = False
    cut = stack.grad_offset_of(split) if overlap else 0

    def compute_a():
        stack.forward()
        stack.backward(split, None)

    def compute_b():
        stack.backward(0, split)

    from deformablelka_amd import dp

    graph = None
    graph_a = graph_b = None
    # eager warm-up (also first-touch of every kernel), then capture
    compute()
    sync()
    if not args.no_graph:
        try:
            graph = torch.cuda.CUDAGraph()
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                compute()
            torch.cuda.current_stream().wait_stream(s)
            with torch.cuda.graph(graph):
                compute()
        except Exception as e:  # capture is an optimisation, not a requirement
            log("hipGraph capture failed, running eagerly:", repr(e))
            graph = None
            sync()
        if not dp.all_ranks_agree(graph is not None, dist, world, dev):   # every rank replays a graph, or none does
            graph = None

    def prepare_overlap():
        nonlocal graph_a, graph_b
        if args.no_graph or graph is None:
            return True            # eager halves need no preparation
        try:
            ga, gb = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            with torch.cuda.graph(ga):
                compute_a()
            with torch.cuda.graph(gb):
                compute_b()
            graph_a, graph_b = ga, gb
            return True
        except Exception as e:
            log("split capture failed:", repr(e))
            sync()
            return False

    def run_a():
        (graph_a.replay() if graph_a is not None else compute_a())

    def run_b():
        (graph_b.replay() if graph_b is not None else compute_b())

    def trial_overlap():   # the two compute halves WITHOUT collectives
        try:
            run_a()
            run_b()
            sync()
            return True
        except Exception as e:
            log("overlapped trial failed:", repr(e))
            sync()
            return False

    # the ADVICE-r1 finding: every local decision is reduced over the ranks before anyone acts on it (deformablelka_amd/dp.py,
    # tests/test_dist_gloo.py::test_all_ranks_take_the_same_allreduce_schedule)
    schedule = dp.choose_schedule(overlap, prepare_overlap, trial_overlap, dist, world, dev)
    if schedule != "overlap":
        graph_a = graph_b = None

    def step_simple():
        dp.step_single(stack, lr, world, dist, graph.replay if graph is not None else compute)   # one flat all-reduce + SGD update

    def step_overlapped():
        dp.step_overlap(stack, lr, world, dist, run_a, run_b, cut)

    step = step_overlapped if schedule == "overlap" else step_simple

    for _ in range(args.warmup):
        step()
    sync()
    if world > 1:
        dist.barrier()
    sync()
    # The timed region — EXACTLY `steps` steps between barrier + synchronize on both sides, MAX over ranks — is run `reps` times back to back (default 1;
    # 3 with --full: the region is 0.2 s on a pool that varies by +-2 % from box to box and by ~0.5 % from loop to loop); `value` is the MEDIAN repetition,
    # all of them are reported (`repetitions`).
    rep_elapsed = []
    for _ in range(max(1, args.reps)):
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        sync()
        if world > 1:
            dist.barrier()
        sync()
        el = time.perf_counter() - t0
        if world > 1:
            tt = torch.tensor([el], device=dev, dtype=torch.float64)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            el = float(tt.item())
        rep_elapsed.append(el)
    elapsed = sorted(rep_elapsed)[len(rep_elapsed) // 2]
    ms_per_step = elapsed / args.steps * 1e3
    value = args.batch * world * args.steps / elapsed
    health = stack.health()   # finite parameters / gradients and the offset statistics of the LAST executed step
    if not health["finite"]:
        raise SystemExit(f"bench invalid: non-finite parameters or gradients after the timed steps: {health}")
    if args.dump_outputs and rank == 0:   # before anything below runs the stack again
        log("bench.py: outputs of the last timed step ->", args.dump_outputs, dump_outputs(stack, args.dump_outputs))

    if rank == 0:
        out = {
            "metric": "3D D-LKA fwd+bwd volumes/sec (64x128x128, b2)", "value": round(value, 3), "unit": "volumes/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype,
            "repetitions": {"ms_per_step": [round(e / args.steps * 1e3, 4) for e in rep_elapsed], "min": round(min(rep_elapsed) / args.steps * 1e3, 4),
                            "max": round(max(rep_elapsed) / args.steps * 1e3, 4), "reported": "median"},
            "data": "synthetic" if not EMU else harness["data"],
            "config": {"workload": "3D D-LKA Former Synapse 64x128x128 patch: fwd+bwd of its 21 D-LKA attention blocks "
                                   "(6x(32,32^3)+6x(64,16^3)+6x(128,8^3)+3x(256,4^3)) + grad all-reduce + SGD update",
                       "batch_per_gpu": args.batch, "global_batch": args.batch * world, "parallelism": f"dp{world}",
                       "block_params": stack.num_params(), "hipgraph": graph is not None, "weight_gradients_on_side_stream": bool(getattr(stack, "_overlap", False)),
                       "allreduce_overlap": bool(step is step_overlapped), "allreduce_split_block": int(split),
                       "offset_std_voxels_stage0": health["offset_std"][0], "offset_std_voxels_by_stage": health["offset_std"]},
        }
        if args.full and not args.no_roofline:
            try:
                out["roofline"] = roofline_report(stack, args.batch, dtype, ms_per_step)
                fl, by = step_work(args.batch, 4 if dtype == torch.float32 else 2)
                t_step = ms_per_step * 1e-3
                out["roofline"]["step"] = {   # the WHOLE step against both roofs (north_star: achieved-HBM-bandwidth fraction)
                    "algorithmic_flops": fl, "algorithmic_bytes": by,
                    "hbm_frac": round(by / t_step / (PEAK_HBM_GBS * 1e9), 5), "achieved_GBps": round(by / t_step / 1e9, 1),
                    "fp32_frac": round(fl / t_step / (PEAK_F32_TFLOPS * 1e12), 5), "achieved_TFLOPs": round(fl / t_step / 1e12, 2),
                    "floor_ms_hbm": round(by / (PEAK_HBM_GBS * 1e9) * 1e3, 3), "floor_ms_fp32": round(fl / (PEAK_F32_TFLOPS * 1e12) * 1e3, 3)}
            except Exception as e:
                log("roofline timing failed:", repr(e))
                out["roofline"] = None
        if args.full and not args.no_cpu_baseline and world == 1:
            try:
                out["cpu_baseline"] = cpu_baseline(args.cpu_sample, args.batch)
            except Exception as e:
                log("cpu baseline failed:", repr(e))
                out["cpu_baseline"] = None
        if dtype == torch.float32:
            out["config"]["f32"] = ("fp32 storage and accumulation everywhere; contractions: forward deformable conv and pointwise convs on the fp32-input MFMA (exact products), "
                                    "forward offset conv as a three-term bf16 split (fp32-equivalent: it feeds floor()), BACKWARD contractions of the deformable conv and the "
                                    "offset conv's data / weight gradients as two-term bf16 splits (three products, fp32 accumulation, ~1e-5 relative, inside the 1e-3 gradient "
                                    "contract); DLKA_EXACT_FP32=1 puts all of them on the fp32-input MFMA (include/dlka.h)")
        if dtype == torch.bfloat16:
            out["config"]["bf16"] = ("bf16 STORAGE of every activation tensor (x, y, saved, intermediate gradients); fp32 parameters, offsets, "
                                     "grad_offset and accumulation; the offset-predict conv and the deformable conv's contractions (forward, Col of grad_offset / grad_input) on the "
                                     "bf16 matrix cores (v_mfma_f32_32x32x16_bf16 / 16x16x32, two-term weight records), the pointwise convs and the stored-sample weight gradient on fp32 MFMA")
        if args.full and world == 1 and not args.no_companion:
            try:
                out["other_dtype"] = companion_metric(args.batch, args.steps, args.warmup, dev, torch.bfloat16 if dtype == torch.float32 else torch.float32, lr,
                                                    roofline=not args.no_roofline)
            except Exception as e:
                log("companion dtype measurement failed:", repr(e))
                out["other_dtype"] = None
            torch.cuda.empty_cache()
        if args.full and not args.no_tblock and world == 1 and dtype == torch.float32:
            try:
                # (one stream: with `wgrad_overlap` — the schedule `training.initialize_network` turns on, which `lka_modules` / `fullnet` below run with — the eager wrapper stack
                #  measured 118.8 - 119.9 volumes/s in some processes and 108.8 - 109.3 in others on round 6's final tree (the replayed graph 119 - 120 either way): the eager
                #  loop sits at the edge of being bound by the host's launches, which the side stream's events add to; the stable figure is reported)
                out["tblock"] = tblock_metric(args.batch, max(3, args.steps // 2), 2, dev)
            except Exception as e:
                log("tblock metric failed:", repr(e))
                out["tblock"] = None
        if args.full and not args.no_tblock and world == 1 and dtype == torch.float32:
            try:
                out["lka_modules"] = lka_modules_metric(args.batch, max(3, args.steps // 2), 2, dev)
            except Exception as e:
                log("lka_modules metric failed:", repr(e))
                out["lka_modules"] = None
            torch.cuda.empty_cache()
        if args.full and not args.no_lka2d and world == 1 and dtype == torch.float32:   # BASELINE.json config 2 AS WRITTEN (bf16, B = 24) in every --full line
            try:                                                                         # (round-3 verdict); its host companion stays in --extras
                out["lka2d"] = lka2d_metric(5, dev, torch.bfloat16, with_cpu=False)
            except Exception as e:
                log("lka2d metric failed:", repr(e))
                out["lka2d"] = None
            torch.cuda.empty_cache()
        if args.full and not args.no_fullnet and world == 1 and dtype == torch.float32:   # SURVEY section 8d metric (iii) in every --full line, not only with
            try:                                                                           # --extras (round-4 verdict)
                out["fullnet"] = fullnet_metric(args.batch, 5, dev, bf16=False)
            except Exception as e:
                log("fullnet metric failed:", repr(e))
                out["fullnet"] = None
            torch.cuda.empty_cache()
        if args.extras and world == 1:
            for key, fn in (("fullnet_bf16", lambda: fullnet_metric(args.batch, 5, dev, bf16=True)),
                            ("lka2d", lambda: lka2d_metric(5, dev, torch.bfloat16, with_cpu=not args.no_cpu_baseline)),   # BASELINE.json config 2: bf16, B=24
                            ("lka2d_f32", lambda: lka2d_metric(5, dev, torch.float32)), ("inference", lambda: inference_metric(dev)),
                            ("inference_config5", lambda: inference_config5_metric(dev))):
                if dtype == torch.bfloat16:
                    continue
                try:
                    out[key] = fn()
                except Exception as e:
                    log(f"{key} metric failed:", repr(e))
                    out[key] = None
                torch.cuda.empty_cache()
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
