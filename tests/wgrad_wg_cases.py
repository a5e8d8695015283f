"""Shared cases of tests/test_wgrad_wg_emu.py and tests/test_wgrad_wg_gpu.py: the weight-gradient kernels with multi-wave workgroups (cl_wgrad.hip:
the waves of a workgroup sum their accumulator tiles in LDS, one partial tile set per workgroup) against the ATen / oracle reference at the project's
contract (tests/parity.py: BWD_RTOL for every gradient), each case under the default and under DLKA_WGRAD_WAVES=1 (one-wave workgroups)."""
import contextlib
import os

import torch

from tests import parity

# B, C, dims — dense conv: Cout = 81, planar grad_out, 3^3 taps, with bias (the block's offset-predict conv); deformable conv: Cout = C
CONV_CASES = [
    (1, 32, (3, 3, 3)),    # 27 rows = one row tile: every wave of a workgroup but the first has no rows and must still reach the barriers
    (1, 64, (3, 3, 5)),    # 45 rows, two ci tiles: two row tiles, the second partial
    (1, 64, (5, 3, 5)),    # 75 rows: three row tiles — no multiple of the waves per workgroup, short last chunk
    (2, 32, (3, 3, 5)),    # 90 rows: row tiles straddle the batch boundary, N % 16 != 0
    (2, 32, (4, 4, 4)),    # N16 variants (N % 16 == 0), whole tiles
    (2, 64, (4, 4, 4)),
    (2, 32, (8, 8, 8)),    # 1024 rows: several workgroups along M; the padded kernel's general walk (W < 16)
    (2, 64, (8, 8, 8)),
]
WIDE_CASE = (2, 256, (4, 4, 4))   # eight ci tiles, the C = 256 stage's volume (fp32 only on the emulator, for time)
TOKEN_CASES = [(1, 32, (4, 4, 4)), (1, 32, (3, 3, 5))]   # pointwise K = 1 (cl_wgrad_pw3_kernel) and the deferred finalize table, through the token block

MODES = ["wg", "one_wave"]


@contextlib.contextmanager
def wgrad_waves(mode):
    """mode "one_wave": DLKA_WGRAD_WAVES=1 for the duration (the library reads it per call)."""
    old = os.environ.get("DLKA_WGRAD_WAVES")
    try:
        if mode == "one_wave":
            os.environ["DLKA_WGRAD_WAVES"] = "1"
        else:
            os.environ.pop("DLKA_WGRAD_WAVES", None)
        yield
    finally:
        if old is None:
            os.environ.pop("DLKA_WGRAD_WAVES", None)
        else:
            os.environ["DLKA_WGRAD_WAVES"] = old


def dense(dev, case, mode):
    B, C, dims = case
    with wgrad_waves(mode):
        parity.check_conv3d_cl(dev, B, C, 81, dims, 3, 1, 1, 1, planar=True, seed=13)


def deform(dev, case, mode):
    B, C, dims = case
    with wgrad_waves(mode):
        parity.check_deform3d_cl(dev, B, C, C, dims, off_mode="normal")


def tokens(dev, case, mode, bf16=False):
    B, C, dims = case
    with wgrad_waves(mode):
        if bf16:
            parity.check_lka3d_tokens_bf16(dev, B, C, dims)
        else:
            parity.check_lka3d_tokens(dev, B, C, dims)


def dense_twice_equal(dev, case, mode):
    """The same dense weight gradient twice: no atomics and a fixed summation order, so the results are the same bits."""
    from deformablelka_amd import ops
    B, C, dims = case
    gen = torch.Generator().manual_seed(21)
    x = parity.to_cl(torch.randn(B, C, *dims, generator=gen)).to(dev)
    w = (torch.randn(81, C, 3, 3, 3, generator=gen) * 0.05).to(dev)
    go = torch.randn(B, 81, *dims, generator=gen).to(dev)
    with wgrad_waves(mode):
        _, gw1, gb1 = ops.conv3d_backward_cl(x, w, go, 1, 1, 1, grad_out_planar=True)
        gw1, gb1 = gw1.clone(), gb1.clone()
        _, gw2, gb2 = ops.conv3d_backward_cl(x, w, go, 1, 1, 1, grad_out_planar=True)
    assert gw1.abs().max() > 0 and gb1.abs().max() > 0
    assert torch.equal(gw1, gw2), "dense weight gradient differs between two identical calls"
    assert torch.equal(gb1, gb2), "dense bias gradient differs between two identical calls"


# the four headline stage shapes (B = 2): C, (H, W, D)
STAGES = [(32, (32, 32, 32)), (64, (16, 16, 16)), (128, (8, 8, 8)), (256, (4, 4, 4))]


def partials_bytes(lib, C, dims, mode, dtype=0):
    H, W, D = dims
    with wgrad_waves(mode):
        return int(lib.dlka_lka3d_tokens_partials_bytes_v(2, C, H, W, D, dtype, 0))
