"""Shared cases of tests/test_dense_conv_emu.py and tests/test_dense_conv_gpu.py: the dense channels-last conv family launch_cl_igemm (csrc/cl_igemm.hip) chooses
between — cl_igemm_kernel, cl_conv_wave_kernel (csrc/cl_conv_wave.hip), cl_conv_kw_kernel (csrc/cl_conv_kw.hip) — member by member, at the smallest shapes at
which each member can still go wrong: waves with a short or empty unit range, the launcher's thresholds between eight and four waves and between one and several
column tiles, a partial last row tile, fewer rows than one workgroup, a tile across the batch boundary, column tiles beyond Cout, the planar channel tail, the tap
split's zero fill / bias / short last split, kernels whose three axes differ, the column-tile menu of launch_igemm_nt, the XCD swizzle's padding workgroups.  The
brick kernels and cl_pointwise have tests of their own; every shape here stays outside them (W no power of two, or D = 1, or too few rows).

Every case goes through ops.conv3d_forward_cl / ops.conv3d_backward_cl with groups = 1 on the seeded randn inputs of dwconv_cases._host (w ~ N(0, 1 / (Cin K)))
and is compared with F.conv3d in float64 on the CPU — forward, grad_input, grad_weight, grad_bias — at the contract's bounds, imported and not restated:
parity.FWD_ATOL on the forward, parity.BWD_RTOL of max |reference| on the three gradients.  Guard bands as in the depthwise tests (dwconv_cases.run_conv): x and
grad_out inside 1e30-filled allocations, every output inside a NaN-filled one — no element may stay NaN (a missed zero fill, an unwritten tail), no guard cell may
change.  All figures of a case are printed before its first failure is raised.

fp32 equivalence: use_split (csrc/cl_host_ops.hip) promises that the three-term forward does not move the offset conv's output at the 1e-5 level, which FWD_ATOL
cannot see.  For every forward with K > 1 the kernel's max error against float64 must be at most 4 x that of F.conv3d in float32 on the CPU on the same inputs:
both are fp32-accurate sums and differ in the summation order only.  (A two-term contraction drops products of relative size 2^-16: an order of magnitude above
that — an estimate from the sizes of the dropped terms, not a measurement.)

On the GPU the launch trace (parity.kernels_launched), taken for the forward and the backward call separately, must name of the dense family exactly the listed
forward member and exactly the listed data-gradient member.  The listed names are launch_cl_igemm / launch_cl_conv_kw / launch_cl_conv_wave / launch_igemm_nt read
under the default environment; the first traced run on the MI355X named every one of them as listed.  The weight-gradient kernels are printed, not asserted.

Measured on the MI355X (out and fp32: max abs error against float64 of the kernel and of F.conv3d in float32; gradients: max error over max |reference|):

  case                      forward member                            data-gradient member                    out      fp32     grad_input  grad_weight  grad_bias
  K1  32->81 (3,5,7)        cl_conv_kw_kernel<0, 1, 3, 8, 1, float>   cl_conv_kw_kernel<2, 0, 2, 8, 1, float>   6.6e-7   3.0e-6   4.0e-6      4.7e-6       9.5e-8
  K2  64->64 (3,3,5) B 2    cl_conv_kw_kernel<0, 0, 3, 8, 1, float>   cl_conv_kw_kernel<0, 0, 2, 8, 1, float>   9.1e-7   1.4e-6   3.9e-6      1.8e-7       6.4e-8
  K3  32->32 (2,5,9) 1x1x3  cl_conv_kw_kernel<0, 0, 3, 8, 1, float>   cl_conv_kw_kernel<0, 0, 2, 8, 1, float>   3.8e-7   9.6e-7   5.6e-6      2.1e-7       9.9e-8
  K4  32->64 (2,6,10) aniso cl_conv_kw_kernel<0, 0, 3, 8, 1, float>   cl_conv_kw_kernel<0, 0, 2, 8, 1, float>   5.0e-7   9.5e-7   4.3e-6      1.9e-7       1.3e-7
  K5  32->81 (11,13,19)     cl_conv_kw_kernel<0, 1, 3, 8, 1, float>   cl_conv_kw_kernel<2, 0, 2, 8, 1, float>   1.2e-6   1.7e-6   4.4e-6      4.4e-6       1.4e-7
  K5  32->81 (11,13,20)     cl_conv_kw_kernel<0, 1, 3, 4, 1, float>   cl_conv_kw_kernel<2, 0, 2, 8, 1, float>   1.7e-6   1.6e-6   4.1e-6      4.9e-6       1.2e-7
  K6  32->81 (25,26,26)     cl_conv_kw_kernel<0, 1, 3, 4, 3, float>   cl_conv_kw_kernel<2, 0, 2, 4, 1, float>   1.7e-6   3.5e-6   4.8e-6      4.3e-6       1.4e-7
  K7  64->128 (25,26,26)    cl_conv_kw_kernel<0, 0, 3, 4, 4, float>   cl_conv_kw_kernel<0, 0, 2, 4, 2, float>   1.5e-6   1.7e-6   4.8e-6      3.0e-7       1.9e-7
  W1  32->50 (1,7,9) B 2    cl_conv_wave_kernel<0, 1, 1, 3, 2, float> cl_conv_wave_kernel<2, 0, 1, 2, 2, float> 1.3e-6   1.6e-6   4.4e-6      5.1e-6       7.0e-8
  W2  64->98 (1,9,11) 7x7   cl_conv_wave_kernel<0, 1, 1, 3, 2, float> cl_igemm_kernel<2, 0, 1, 2, float>        4.7e-7   7.2e-7   4.9e-6      5.6e-6       7.8e-8
  W3  32->64 (1,6,10) cl    cl_conv_wave_kernel<0, 0, 1, 3, 2, float> cl_conv_wave_kernel<0, 0, 1, 2, 2, float> 8.1e-7   1.0e-6   4.9e-6      1.4e-7       9.8e-8
  W4  96->50 (1,7,9)        cl_conv_wave_kernel<0, 1, 1, 3, 2, float> cl_igemm_kernel<2, 0, 3, 2, float>        6.0e-7   1.3e-6   4.7e-6      5.2e-6       8.6e-8
  W4  192->50 (1,7,9)       cl_conv_wave_kernel<0, 1, 1, 3, 2, float> cl_igemm_kernel<2, 0, 2, 2, float>        7.7e-7   1.6e-6   5.6e-6      6.8e-6       7.2e-8
  W5  128->50 (1,7,9)       cl_conv_wave_kernel<0, 1, 1, 3, 2, float> cl_igemm_kernel<2, 0, 1 | 2 | 4, 2, float> 7.8e-7  1.5e-6   3.9e-6      4.9e-6       8.9e-8
  W5  256->50 (1,7,9)       cl_conv_wave_kernel<0, 1, 1, 3, 2, float> cl_igemm_kernel<2, 0, 2 | 4 | 8, 2, float> 1.1e-6  1.6e-6   4.2e-6      6.4e-6       1.0e-7
  I1  32->50 (1,129,128)    cl_igemm_kernel<0, 1, 2, 3, float>        cl_conv_wave_kernel<2, 0, 1, 2, 2, float> 1.7e-6   3.8e-6   4.5e-6      4.7e-6       1.7e-7
  E   32->14 (3,5,7) B 2    cl_igemm_kernel<0, 1, 1, 0, float>        cl_igemm_kernel<2, 0, 1, 0, float>        7.6e-7   -        1.0e-7      1.2e-7       6.7e-8
  E   64->81 (3,5,7)        cl_igemm_kernel<0, 1, 3, 0, float>        cl_igemm_kernel<2, 0, 1, 0, float>        1.0e-6   -        4.1e-7      1.5e-7       9.2e-8

The worst forward against the fp32 sum is 1.1 x (K5 at 270 tiles); every two-term data gradient sits at 4e-6 to 6e-6 of max |reference|, the exact MFMA at 1e-7.
Every K case runs twice with bitwise equal forward and grad_input.

Group E's backward: dlka_conv3d_backward_cl refuses K = 1 with a planar grad_out when grad_weight is asked for (dense_backward_weight; grad_input has been written
by then) and refuses the data gradient of a channels-last grad_out whose Cout is no multiple of 32 (dense_backward_data) — 14 and 81 are none.  Both refusals
are asserted as the RuntimeError the wrapper raises; the gradients are checked through the two calls that remain: planar without grad_weight (grad_input,
grad_bias), channels-last without grad_input (grad_weight, grad_bias).

That the cases bite was shown once with four edits of the kernels, never committed, on the emulator (groups K1 to K5, W, E; edits 3 and 4 may write outside a
tensor and never ran on the GPU):
  1. ups = units / KW in cl_conv_kw_kernel: all six cases of K1 to K5 failed (K3: zero units per wave), W and E passed;
  2. the bias added by every tap split (cl_igemm_kernel and cl_conv_wave_kernel, both epilogues): every case of W1 to W5 failed, K and E (no split) passed;
  3. the `n >= p.Cout` test removed from one epilogue: from cl_conv_wave_kernel's planar epilogue W1 failed by value (B = 2: columns 50 .. 63 of sample 0 land in sample 1's
     planes) and W2, W4, W5 passed (B = 1: the stray columns land behind the output, where an atomicAdd onto the NaN poison leaves the same NaN — the guard
     cannot see an atomic write, which is why W1 has two samples); from cl_conv_kw_kernel's, a plain store, K1 and both K5 failed (81 of 96 columns);
  4. the zero fill before a split launch skipped (launch_cl_igemm): every case of W1 to W5 failed with NaN left in the output."""
import functools
from typing import NamedTuple

import pytest
import torch
import torch.nn.functional as F

from deformablelka_amd import ops
from tests import dwconv_cases as dw
from tests import parity

FP32_EQUIV_MARGIN = 4.0      # the three-term forward against F.conv3d in float32, both measured against float64: only the summation order differs
XCD_MIN_DEFAULT = 16         # xcd_min_blocks(), csrc/dlka_common.h
FAMILY = ("cl_igemm_kernel", "cl_conv_wave_kernel", "cl_conv_kw_kernel", "cl_conv_brick", "cl_pointwise")

# kernel, padding, dilation triples
K333 = ((3, 3, 3), (1, 1, 1), (1, 1, 1))       # the 3-D offset-predict conv
K113 = ((1, 1, 3), (0, 0, 1), (1, 1, 1))
K133 = ((1, 3, 3), (0, 1, 1), (1, 1, 1))
K133_ANISO = ((1, 3, 3), (0, 2, 3), (1, 2, 3))   # kd != kh, dh != dw, ph != pw; the data gradient's flipped padding d (k - 1) - p = (0, 2, 3)
K155 = ((1, 5, 5), (0, 2, 2), (1, 1, 1))       # conv0's offset conv of the 2-D block
K177_D3 = ((1, 7, 7), (0, 9, 9), (1, 3, 3))    # conv_spatial's
K111 = ((1, 1, 1), (0, 0, 0), (1, 1, 1))


class Case(NamedTuple):
    group: str
    B: int
    Cin: int
    Cout: int
    dims: tuple      # (D, H, W)
    conv: tuple      # (k, p, d) triples
    planar: bool     # out and grad_out planar [B, Cout, D, H, W]; channels-last otherwise
    fwd: str         # the forward member, as the launch trace spells it
    dgrad: str       # the data-gradient member
    gpu_only: bool = False


def _kw(am, om, sp, waves, nt):
    return f"cl_conv_kw_kernel<{am}, {om}, {sp}, {waves}, {nt}, float>"


def _wave(am, om, sp):
    return f"cl_conv_wave_kernel<{am}, {om}, 1, {sp}, 2, float>"


def _igemm(am, om, nt, sp):
    return f"cl_igemm_kernel<{am}, {om}, {nt}, {sp}, float>"


# launch_cl_conv_kw (D > 1, K > 1, cl_igemm_pick_splits > 1): one 32-row x 32-column tile per workgroup; nt column tiles per workgroup where row_tiles * (NP / 32 / nt) * 4
# >= 2048; four waves where nt > 1 or tiles * 4 >= 1024, else eight.  Forward: three-term (SPLIT 3), AMODE 0; data gradient: two-term, AMODE 2 from a planar grad_out.
K_CASES = [
    # 105 rows: the last tile has 9.  Forward 27 units over 8 waves (ups 4): wave 7 empty; data gradient 81 units (ups 11): wave 7 has 4; channel tail 81 of 96 (AMODE 2)
    Case("K1", 1, 32, 81, (3, 5, 7), K333, True, _kw(0, 1, 3, 8, 1), _kw(2, 0, 2, 8, 1)),
    # channels-last both ways: the line-friendly A fetch; two column tiles in grid.z; 90 rows, 45 a sample: tile 1 straddles the batch boundary
    Case("K2", 2, 64, 64, (3, 3, 5), K333, False, _kw(0, 0, 3, 8, 1), _kw(0, 0, 2, 8, 1)),
    # 3 units over 8 waves: five empty waves
    Case("K3", 1, 32, 32, (2, 5, 9), K113, False, _kw(0, 0, 3, 8, 1), _kw(0, 0, 2, 8, 1)),
    # tap_decode with kd != kh != kw and per-axis dilation and padding
    Case("K4", 1, 32, 64, (2, 6, 10), K133_ANISO, False, _kw(0, 0, 3, 8, 1), _kw(0, 0, 2, 8, 1)),
    # 85 row tiles x 3 column tiles = 255 tiles: eight waves; 90 x 3 = 270: four waves of 7, 7, 7, 6 units
    Case("K5", 1, 32, 81, (11, 13, 19), K333, True, _kw(0, 1, 3, 8, 1), _kw(2, 0, 2, 8, 1)),
    Case("K5", 1, 32, 81, (11, 13, 20), K333, True, _kw(0, 1, 3, 4, 1), _kw(2, 0, 2, 8, 1)),
    # 529 row tiles: 529 * 4 >= 2048: all three column tiles in one workgroup
    Case("K6", 1, 32, 81, (25, 26, 26), K333, True, _kw(0, 1, 3, 4, 3), _kw(2, 0, 2, 4, 1), gpu_only=True),
    Case("K7", 1, 64, 128, (25, 26, 26), K133, False, _kw(0, 0, 3, 4, 4), _kw(0, 0, 2, 4, 2), gpu_only=True),
]

# D = 1: cl_conv_kw does not apply; the (tap, 32-channel chunk) units split over gridDim.y (cl_igemm_pick_splits: 512 workgroups wanted, at most 32 splits, at most one per
# unit), fp32 atomics on a zero-filled output, the bias from split 0.  cl_conv_wave takes the three-term forward up to 16 384 rows and the two-term data gradient of 32 columns.
W_CASES = [
    # 126 rows: less than one workgroup; forward 25 units in 25 splits, two column tiles; data gradient 50 units in 25 splits
    Case("W1", 2, 32, 50, (1, 7, 9), K155, True, _wave(0, 1, 3), _wave(2, 0, 2)),
    # forward 98 units: 25 splits of 4, the last with 2; four column tiles.  Data gradient 196 units, 64 columns: cl_igemm_kernel, one column tile per workgroup
    Case("W2", 1, 64, 98, (1, 9, 11), K177_D3, True, _wave(0, 1, 3), _igemm(2, 0, 1, 2)),
    Case("W3", 1, 32, 64, (1, 6, 10), K133, False, _wave(0, 0, 3), _wave(0, 0, 2)),
    # launch_igemm_nt at the 2-D nets' widths: 96 columns = three tiles in one workgroup; 192 = six, two at a time, grid.z = 3
    Case("W4", 1, 96, 50, (1, 7, 9), K155, True, _wave(0, 1, 3), _igemm(2, 0, 3, 2)),
    Case("W4", 1, 192, 50, (1, 7, 9), K155, True, _wave(0, 1, 3), _igemm(2, 0, 2, 2)),
]
# DLKA_IGEMM_NT (read per launch): (value or None, data-gradient member).  128 columns, 25 workgroups: one tile by default; 256 columns: two
W5_CASES = [
    (Case("W5", 1, 128, 50, (1, 7, 9), K155, True, _wave(0, 1, 3), None), ((None, 1), ("2", 2), ("4", 4))),
    (Case("W5", 1, 256, 50, (1, 7, 9), K155, True, _wave(0, 1, 3), None), ((None, 2), ("2", 2), ("4", 4), ("8", 8))),
]

# 16 512 rows: above cl_conv_wave's three-term limit; 129 row blocks: 4 tap splits (7, 7, 7, 4 units), the swizzled grid of 136 has 7 padding workgroups
I_CASES = [Case("I1", 1, 32, 50, (1, 129, 128), K155, True, _igemm(0, 1, 2, 3), _wave(2, 0, 2), gpu_only=True)]

# K = 1 with a planar output, which cl_pointwise does not take: the exact fp32-input MFMA (SPLIT 0).  Column tails 14 of 32 and 81 of 96.
E_CASES = [
    Case("E", 2, 32, 14, (3, 5, 7), K111, True, _igemm(0, 1, 1, 0), _igemm(2, 0, 1, 0)),
    Case("E", 1, 64, 81, (3, 5, 7), K111, True, _igemm(0, 1, 3, 0), _igemm(2, 0, 1, 0)),
]

SINGLE_CASES = K_CASES + W_CASES + I_CASES
EMU_SINGLE_CASES = [c for c in SINGLE_CASES if not c.gpu_only]


def case_id(c):
    k, p, d = c.conv
    return f"{c.group}-{c.B}x{c.Cin}to{c.Cout}x{'x'.join(map(str, c.dims))}-k{'x'.join(map(str, k))}d{'x'.join(map(str, d))}-{'planar' if c.planar else 'cl'}"


def taps(c):
    k = c.conv[0]
    return k[0] * k[1] * k[2]


# ---- reference ----------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _host(B, Cin, Cout, dims, conv, planar):
    """dwconv_cases._host with groups = 1 -> x (channels-last), w, b, grad_out and the float64 reference, out / grad_out in the case's layout; and the max error
    of F.conv3d in float32 on the CPU against float64 on the same inputs (what an fp32-accurate sum in another order differs by)."""
    x, w, b, go, ref = dw._host(B, Cin, dims, conv, True, Cout, 1)
    k, p, d = conv
    out32 = F.conv3d(parity.from_cl(x), w, b, 1, p, d, 1)
    ref = dict(ref)
    ref["fp32_err"] = float((parity.to_cl(out32).double() - ref["out"]).abs().max())
    if planar:
        go, ref["out"] = parity.from_cl(go), parity.from_cl(ref["out"])
    return x, w, b, go, ref


def host(c):
    return _host(c.B, c.Cin, c.Cout, c.dims, c.conv, c.planar)


# ---- the check ----------------------------------------------------------------------------------------------------------------------------------------
def _family(names):
    return sorted(n for n in names if n.startswith(FAMILY))


def assert_members(c, names, fwd=True, dgrad=True):
    """Of the dense family the forward ran the listed member and no other, and so did the backward; the weight-gradient kernels (tests/wgrad_wg_cases.py owns
    them) are printed."""
    what = case_id(c)
    f, bwd = names if fwd else (set(), names[0])
    print(f"[{what}] forward: {', '.join(_family(f))}   data gradient: {', '.join(_family(bwd))}   weight gradient: {', '.join(sorted(n for n in bwd if 'wgrad' in n))}")
    if fwd:
        assert _family(f) == [c.fwd], f"{what}: the forward ran {_family(f)}, expected {c.fwd}"
    if dgrad:
        assert _family(bwd) == [c.dgrad], f"{what}: the data gradient ran {_family(bwd)}, expected {c.dgrad}"


def _fp32_equivalent(c, got, ref):
    """use_split's promise for the three-term forward: its error against float64 within 4 x that of an fp32 sum."""
    def check():
        err = float((got["out"].double() - ref["out"]).abs().max())
        print(f"[{case_id(c)} out] fp32 equivalence: kernel {err:.3e}, F.conv3d in float32 {ref['fp32_err']:.3e} against float64 (margin {FP32_EQUIV_MARGIN:g})")
        assert err <= FP32_EQUIV_MARGIN * ref["fp32_err"], (f"{case_id(c)} out: max abs err {err:.3e} > {FP32_EQUIV_MARGIN:g} x {ref['fp32_err']:.3e}, "
                                                           "the error of F.conv3d in float32")
        return "out/fp32", err / ref["fp32_err"]
    return check


def single_op(dev, c, trace=False, dgrad=True):
    """Forward and backward through the wrappers with guard bands, the members named (GPU), the four outputs against float64 and the forward against the fp32 sum."""
    x, w, b, go, ref = host(c)
    got, names = dw.run_conv(dev, case_id(c), x, w, b, go, c.conv, 1, trace, out_planar=c.planar, grad_out_planar=c.planar)
    if trace:
        assert_members(c, names, dgrad=dgrad)
    dw.compare_with(case_id(c), got, ref, more=[_fp32_equivalent(c, got, ref)] if taps(c) > 1 else ())
    return got


def reproducible(dev, c, trace=False):
    """cl_conv_kw_kernel sums its waves' partial tiles in wave order: forward and data gradient are the same bits on every run (the file header of cl_conv_kw.hip)."""
    first, second = single_op(dev, c, trace), single_op(dev, c, trace)
    for name in ("out", "grad_input"):
        assert torch.equal(first[name], second[name]), f"{case_id(c)} {name}: {int((first[name] != second[name]).sum())} elements differ between two runs"


def forced_column_tiles(dev, c, runs, monkeypatch, trace=False):
    """launch_igemm_nt's column-tile menu: the default member, then DLKA_IGEMM_NT = n; every run meets the reference."""
    for value, nt in runs:
        if value is None:
            monkeypatch.delenv("DLKA_IGEMM_NT", raising=False)
        else:
            monkeypatch.setenv("DLKA_IGEMM_NT", value)
        single_op(dev, c._replace(dgrad=_igemm(2, 0, nt, 2)), trace)
    monkeypatch.delenv("DLKA_IGEMM_NT", raising=False)


def swizzle(dev, c, monkeypatch, trace=False):
    """cl_igemm_kernel's padding workgroups (bx < 0: they leave ahead of the barriers): swizzled by default, then DLKA_XCD_MIN above the row-block count: the
    same members, the reference met both times (not the same bits: the tap splits meet in atomics)."""
    nx = -(-c.B * c.dims[0] * c.dims[1] * c.dims[2] // 128)
    assert nx % 8 != 0 and nx >= XCD_MIN_DEFAULT, nx
    monkeypatch.delenv("DLKA_XCD_MIN", raising=False)
    single_op(dev, c, trace)
    monkeypatch.setenv("DLKA_XCD_MIN", str(nx + 1))
    single_op(dev, c, trace)


def exact_pointwise_planar(dev, c, trace=False):
    """K = 1 with planar out / grad_out.  The forward and the data gradient run cl_igemm_kernel on the fp32-input MFMA.  dlka_conv3d_backward_cl refuses the full
    planar backward (dense_backward_weight has no K = 1 kernel for a planar grad_out: DLKA_ERR_UNSUPPORTED -> RuntimeError), and a channels-last grad_out needs
    Cout % 32 == 0 for the data gradient (dense_backward_data), which 14 and 81 are not: grad_input and grad_bias come from the planar call without grad_weight,
    grad_weight and grad_bias from the channels-last call without grad_input."""
    what = case_id(c)
    x, w, b, go, ref = host(c)
    got, names = dw.run_conv(dev, what, x, w, b, go, c.conv, 1, trace, out_planar=True, grad_out_planar=True, need=(True, False, True))
    if trace:
        assert_members(c, names)
    dw.compare_with(what, got, ref, only=("out", "grad_input", "grad_bias"))
    go_cl = parity.to_cl(go)
    got, names = dw.run_conv(dev, what + " cl", x, w, b, go_cl, c.conv, 1, trace, grad_out_planar=False, forward=False, need=(False, True, True))
    if trace:
        assert_members(c, names, fwd=False, dgrad=False)
        assert _family(names[0]) == [], names
    dw.compare_with(what + " cl", got, ref, only=("grad_weight", "grad_bias"))
    xd, wd = x.to(dev), w.to(dev)
    with pytest.raises(RuntimeError):
        ops.conv3d_backward_cl(xd, wd, go.to(dev), c.conv[1], c.conv[2], 1, grad_out_planar=True)
    with pytest.raises(RuntimeError):
        ops.conv3d_backward_cl(xd, wd, go_cl.to(dev), c.conv[1], c.conv[2], 1, grad_out_planar=False, need=(True, False, False))
