"""TEST INFRASTRUCTURE — the cases and checks of the shared cubic B-spline preparation (csrc/cl_spline.hip: dlka_spline_pad,
dlka_spline_prefilter; ops.spline_coefficients / ops.spline_prefilter), shared by tests/test_spline_emu.py (wavefront emulator, CPU suite) and
tests/test_spline_gpu.py (MI355X).  Inputs and expected results are tensors in tests/golden/reference_spline.pt, recorded by
tests/golden/make_golden_spline.py.  No scipy here.

Every case holds two results.  "ref" is scipy.ndimage.spline_filter1d(order=3, mode='reflect' | 'mirror', output=float64), the reference.
"parent" is NOT a reference: it is a regression value, what the two prefilter kernels this one replaced (cl_resample.hip's 'reflect' one,
cl_augment.hip's 'mirror' one, of the commit before the consolidation) gave on the emulator for the same input.  The new kernel keeps their
operations in their order with contraction off, so it must equal them bit for bit, on the emulator and on the device.

Shapes: the smallest at which the recursion can go wrong.  Volumes (2, 3, 5) and (1, 4, 2), every axis, both boundaries: lines of 1 (returned
untouched), 2 (the 'mirror' start-value loop is empty and c[n - 2] is c[0]), 3, 4 and 5 cells.  float32 input goes through the pad kernel with
pad 0 (the cast) and with DLKA_RESAMPLE_SPLINE_PAD on one axis only (its clamp on both sides of that axis, and no shift on the others).

Bound against scipy: the largest |out - ref| / max|ref| of the PARENT's two kernels over these cases, measured on the emulator by the recorder, is
MEASURED = 5.688e-4 (case f64_1x4x2_ax2_reflect, lines of 2 cells).  The checks allow twice that, and not less than 4 float64 ulps of
max|ref|: the recursion is a handful of float64 operations per cell with |z| < 0.27, so rounding errors of earlier cells decay instead of
piling up.  The figure is not rounding.  It comes from the 'reflect' cases on lines of 2 to 5 cells alone (5.7e-4, 1.1e-4, 5.6e-6, 6.0e-7 for
n = 2, 3, 4, 5, about |z|^(2 n + 2)): there the kernels' result agrees with a dense float64 solve of the interpolation system under that
boundary to 3e-16 and scipy 1.15's does not.  Under 'mirror', and under 'reflect' on the padded line of 27 cells (the only way the pipeline
modules use 'reflect': behind DLKA_RESAMPLE_SPLINE_PAD edge samples), the parent's kernels are within 4.4e-16 of scipy."""
import os

import numpy as np
import torch

from deformablelka_amd import _lib as L
from deformablelka_amd import ops

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "reference_spline.pt")

MEASURED = 0.0005687971764252894   # printed by tests/golden/make_golden_spline.py

SHAPES = ((2, 3, 5), (1, 4, 2))
BOUNDARIES = {"reflect": L.DLKA_SPLINE_REFLECT, "mirror": L.DLKA_SPLINE_MIRROR}
# id: (input key, pad, boundary, axes)
CASES = {f"f64_{'x'.join(map(str, s))}_ax{ax}_{b}": (f"f64_{'x'.join(map(str, s))}", (0, 0, 0), b, (ax,))
         for s in SHAPES for ax in range(3) for b in BOUNDARIES}
CASES["f32_cast_mirror_ax12"] = ("f32_2x3x5", (0, 0, 0), "mirror", (1, 2))                              # the 2-D evaluator's use
CASES["f32_pad_ax1_reflect"] = ("f32_2x3x5", (0, L.DLKA_RESAMPLE_SPLINE_PAD, 0), "reflect", (1,))     # the resampling's, one filtered axis
PAD_ONLY = [c for c in CASES if c.startswith("f32_")]


def load_fixture():
    return torch.load(FIXTURE, weights_only=True)


def run(fx, cid, device):
    """(coefficients on ``device``, launches counted)."""
    key, pad, boundary, axes = CASES[cid]
    x = fx["inputs"][key].to(device)
    before = ops.resample_launch_count()
    coef = ops.spline_coefficients(x, pad, BOUNDARIES[boundary], axes)
    return coef, ops.resample_launch_count() - before


def check_against_scipy(fx, cid, device):
    coef, launches = run(fx, cid, device)
    key, pad, _, axes = CASES[cid]
    ref = fx["ref"][cid]
    assert launches == 1 + len(axes)
    assert coef.dtype == torch.float64 and coef.shape == ref.shape == tuple(n + 2 * p for n, p in zip(fx["inputs"][key].shape, pad))
    scale = float(ref.abs().max())
    err = float((coef.cpu() - ref).abs().max())
    bound = max(2.0 * MEASURED * scale, 4.0 * float(np.spacing(scale)))
    print(f"{cid}: max|out - scipy| = {err:.3e} ({err / scale:.3e} of max|scipy| = {scale:.6g}); bound {bound:.3e}")
    assert err <= bound
    return coef


def check_equals_parent(fx, cid, device):
    """Bit for bit what the two kernels of the commit before the consolidation gave (a regression value, not a reference)."""
    coef, _ = run(fx, cid, device)
    assert torch.equal(coef.cpu().view(torch.int64), fx["parent"][cid].view(torch.int64))


def check_lines_of_one_cell(fx, device):
    """n = 1: untouched, whatever the boundary."""
    x = fx["inputs"]["f64_1x4x2"]
    for b in BOUNDARIES:
        coef, launches = run(fx, f"f64_1x4x2_ax0_{b}", device)
        assert launches == 2 and torch.equal(coef.cpu().view(torch.int64), x.view(torch.int64))


def check_pad(fx, cid, device):
    """The pad launch alone is numpy's pad by edge samples and the exact cast."""
    key, pad, _, _ = CASES[cid]
    x = fx["inputs"][key]
    before = ops.resample_launch_count()
    out = ops.spline_coefficients(x.to(device), pad, L.DLKA_SPLINE_REFLECT, ())
    assert ops.resample_launch_count() - before == 1
    want = np.pad(x.numpy().astype(np.float64), [(p, p) for p in pad], mode="edge")
    assert out.dtype == torch.float64 and np.array_equal(out.cpu().numpy(), want)


def check_prefilter_alone(fx, device):
    """ops.spline_prefilter on a float64 volume is spline_coefficients without the pad launch: the same bits, one launch per axis, in place."""
    cid = "f64_2x3x5_ax1_mirror"
    coef = fx["inputs"]["f64_2x3x5"].clone().to(device)
    before = ops.resample_launch_count()
    out = ops.spline_prefilter(coef, L.DLKA_SPLINE_MIRROR, (1,))
    assert ops.resample_launch_count() - before == 1 and out is coef
    assert torch.equal(out.cpu().view(torch.int64), run(fx, cid, device)[0].cpu().view(torch.int64))


def check_unknown_boundary(fx, device):
    """An unknown boundary is refused by the library before anything is launched."""
    import ctypes
    import pytest
    x = fx["inputs"]["f64_2x3x5"].clone().to(device)
    keep = x.clone()
    counts = ops.resample_launch_count(), ops.augment_launch_count(), ops.zoom2d_launch_count()
    i3 = ctypes.c_int64 * 3
    for boundary in (2, -1):
        assert L.get_lib().dlka_spline_prefilter(L.ptr(x), i3(*x.shape), 1, boundary, L.stream_ptr(x)) == -8   # DLKA_ERR_UNSUPPORTED
        with pytest.raises(RuntimeError, match="spline_prefilter"):
            ops.spline_prefilter(x, boundary, (1,))
    assert (ops.resample_launch_count(), ops.augment_launch_count(), ops.zoom2d_launch_count()) == counts
    assert torch.equal(x, keep)
