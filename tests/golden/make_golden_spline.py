"""Generates tests/golden/reference_spline.pt: the inputs of tests/spline_cases.py, their cubic B-spline coefficients by
scipy.ndimage.spline_filter1d(order=3, mode='mirror' | 'reflect', output=float64) (scipy 1.15), and the regression values "parent".  Run from
the repository root:

    python tests/golden/make_golden_spline.py [--parent-lib LIB]

"parent" is what the two prefilter kernels that csrc/cl_spline.hip replaced gave for the same inputs: LIB is a wavefront-emulator build
(tests/emu) of the commit before the consolidation, which still exports dlka_resample_spline_pad, dlka_resample_spline_prefilter and
dlka_augment_spline_prefilter_mirror.  They are regression values of that commit, not a reference.  Without --parent-lib the ones already in
the fixture are kept, and the inputs must not have changed.  The recorder prints the largest |parent - scipy| / max|scipy| over the cases: the
figure MEASURED in tests/spline_cases.py.  The fixture holds tensors only."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import resampling_cases as RC   # noqa: E402
from tests import spline_cases as C        # noqa: E402


def inputs():
    out = {}
    for salt, shape in enumerate(C.SHAPES):
        out["f64_" + "x".join(map(str, shape))] = torch.from_numpy(RC.noise(shape, 71 + salt) * 4.0 - 1.0)
    out["f32_2x3x5"] = torch.from_numpy((RC.noise((2, 3, 5), 79) * 4.0 - 1.0).astype(np.float32))
    return out


def scipy_coefficients(x, pad, boundary, axes):
    from scipy.ndimage import spline_filter1d
    c = np.pad(x.numpy().astype(np.float64), [(p, p) for p in pad], mode="edge")
    for ax in axes:
        c = spline_filter1d(c, order=3, axis=ax, output=np.float64, mode=boundary)
    return torch.from_numpy(np.ascontiguousarray(c))


def parent_coefficients(lib, x, pad, boundary, axes):
    i3 = ctypes.c_int64 * 3
    x = x.contiguous()
    ext = [n + 2 * p for n, p in zip(x.shape, pad)]
    coef = torch.empty(ext, dtype=torch.float64)
    assert lib.dlka_resample_spline_pad(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(coef.data_ptr()), 0 if x.dtype == torch.float32 else 2,
                                        i3(*x.shape), i3(*pad), None) == 0
    fn = lib.dlka_resample_spline_prefilter if boundary == "reflect" else lib.dlka_augment_spline_prefilter_mirror
    for ax in axes:
        assert fn(ctypes.c_void_p(coef.data_ptr()), i3(*ext), ax, None) == 0
    return coef


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    args = ap.parse_args()
    fx = {"inputs": inputs(), "ref": {}, "parent": {}}
    if args.parent_lib:
        lib = ctypes.CDLL(os.path.abspath(args.parent_lib))
    else:
        old = C.load_fixture()
        assert all(torch.equal(old["inputs"][k], v) for k, v in fx["inputs"].items()), "the inputs changed: the regression values need --parent-lib"
    worst = 0.0
    for cid, (key, pad, boundary, axes) in C.CASES.items():
        x = fx["inputs"][key]
        ref = scipy_coefficients(x, pad, boundary, axes)
        parent = parent_coefficients(lib, x, pad, boundary, axes) if args.parent_lib else old["parent"][cid]
        err = float((parent - ref).abs().max() / ref.abs().max())
        print(f"{cid}: |parent - scipy| / max|scipy| = {err:.3e}")
        worst = max(worst, err)
        fx["ref"][cid], fx["parent"][cid] = ref, parent
    # scipy leaves a line of one cell as it is
    for b in C.BOUNDARIES:
        assert torch.equal(fx["ref"][f"f64_1x4x2_ax0_{b}"], fx["inputs"]["f64_1x4x2"])
    print(f"MEASURED = {worst!r}   (4 float64 ulps: {4 * 2.0 ** -52:.3e} of a power of two)")
    torch.save(fx, C.FIXTURE)
    print(f"{C.FIXTURE}: {os.path.getsize(C.FIXTURE)} bytes")
    assert os.path.getsize(C.FIXTURE) < 2 ** 20


if __name__ == "__main__":
    main()
