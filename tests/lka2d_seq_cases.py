"""Cases of tests/test_lka2d_seq_gpu.py: what "behaviour unchanged" means for the host code of the two channels-last 2-D attention blocks
(csrc/capi_lka2d_cl.hip, csrc/capi_lka2d_plain_cl.hip) and the frame they share (csrc/capi_lka2d_frame.h) — the kernels one forward and one backward call
launch, in host issue order, template arguments included.  RECORDED (tests/golden/lka2d_sequences.json) from the commit before the frame was written once,
and never taken from the code under test; the byte counts of the same blocks are pinned by tests/golden/block_layouts.json.

The launch trace (include/dlka.h dlka_trace_*) records every launch of the library on the launch's own stream, in the order the host issued them: the
deformable backward's kernels on the library's internal streams appear where the host launched them.  It does not record WHICH stream a launch went to.

    python -m tests.lka2d_seq_cases --recorded-from COMMIT      # on a machine with the GPU, with the library built from COMMIT"""
import argparse
import json
import os

import torch

from deformablelka_amd import _lib as L
from deformablelka_amd import ops
from deformablelka_amd.ops import lka2d_plain
from tests.planar_seq_cases import DTYPES, _block_params, _lka2d_shapes, _rand, kernel_sequence

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lka2d_sequences.json")
WIDTHS = (32, 96)     # one and three column tiles of the pointwise kernels
B, H, W = 1, 7, 6


def _plain_shapes(C):
    by_name = {"proj_1_w": (C, C, 1, 1), "conv0_w": (C, 1, 5, 5), "conv_spatial_w": (C, 1, 7, 7), "conv1_w": (C, C, 1, 1), "proj_2_w": (C, C, 1, 1)}
    return [by_name.get(f, (C,)) for f in L.LKA2D_PLAIN_FIELDS]


# block -> (fields, shapes(C), forward, backward).  lka2d_attention: the channels-last path (the general kernels are not forced; both widths have it).
BLOCKS = {
    "lka2d_attention": (L.LKA2D_FIELDS, _lka2d_shapes, ops.lka2d_attention_forward, ops.lka2d_attention_backward),
    "lka2d_plain_attention": (L.LKA2D_PLAIN_FIELDS, _plain_shapes, lka2d_plain.attention_forward, lka2d_plain.attention_backward),
}
IDS = [f"{blk}_{d}/C{C}/{dname}" for blk in BLOCKS for d in ("forward", "backward") for C in WIDTHS for dname in DTYPES]


def launches(dev, cid):
    """The kernels of the one call `cid` names, in host issue order."""
    call, width, dname = cid.split("/")
    blk, direction = call.rsplit("_", 1)
    C = int(width[1:])
    fields, shapes, forward, backward = BLOCKS[blk]
    params = _block_params(fields, dict(zip(fields, shapes(C))), dev, torch.float32)   # fp32 parameters on both paths: bf16 is an activation dtype
    gen = torch.Generator().manual_seed(2)
    x, gy = (_rand(gen, B, C, H, W).to(DTYPES[dname][1]).to(dev) for _ in range(2))
    if direction == "forward":
        return kernel_sequence(lambda: forward(x, params))
    _, saved = forward(x, params)
    return kernel_sequence(lambda: backward(x, params, gy, saved))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=FIXTURE)
    ap.add_argument("--recorded-from", required=True, help="the commit the library was built from")
    args = ap.parse_args()
    L.get_lib()
    rec = {"recorded_from": f"commit {args.recorded_from}: the parent of the commit that introduced csrc/capi_lka2d_frame.h",
           "launches": {cid: launches("cuda:0", cid) for cid in IDS}}
    assert all(rec["launches"].values())
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{args.out}: {len(rec['launches'])} launch sequences of {sorted(len(v) for v in rec['launches'].values())} kernels")


if __name__ == "__main__":
    main()
