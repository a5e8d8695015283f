"""Shared cases of tests/test_mixed_dtype_emu.py and tests/test_mixed_dtype_gpu.py: the six general entry points of deformablelka_amd.ops that also take float64
(deform_conv3d_*, deform_conv2d_*, conv3d_*) hand every pointer to the library as the type of `input`.  A tensor of another dtype would be read at the wrong element
size — float32 parameters next to a float64 input: twice their bytes, past their end — so the wrappers refuse it before any launch, as the reference's op raises a
scalar-type mismatch.  For each entry point and each non-input tensor argument in turn: one float32 tensor among float64 ones, and the reverse; the call raises
RuntimeError naming the argument, and nothing was launched (GPU: the library's launch trace is empty; emulator, which has no trace: no library entry was called)."""
import pytest
import torch

from deformablelka_amd import _lib as L
from deformablelka_amd import ops


def _t(dtype, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(sum(shape))).to(dtype)


def _deform3d(dt):
    return dict(input=_t(dt, 1, 4, 3, 4, 5), weight=_t(dt, 6, 4, 3, 3, 3), bias=_t(dt, 6), offset=_t(dt, 1, 81, 3, 4, 5), grad_output=_t(dt, 1, 6, 3, 4, 5))


def _deform2d(dt):
    return dict(input=_t(dt, 1, 4, 5, 6), offset=_t(dt, 1, 18, 5, 6), weight=_t(dt, 6, 4, 3, 3), bias=_t(dt, 6), grad_output=_t(dt, 1, 6, 5, 6))


def _conv3d(dt):
    return dict(input=_t(dt, 1, 4, 3, 4, 5), weight=_t(dt, 6, 4, 3, 3, 3), bias=_t(dt, 6), grad_output=_t(dt, 1, 6, 3, 4, 5))


# name -> (tensors(dtype), the tensor arguments besides `input`, call(tensors))
ENTRIES = {
    "deform_conv3d_forward": (_deform3d, ("weight", "bias", "offset"),
                              lambda a: ops.deform_conv3d_forward(a["input"], a["weight"], a["bias"], a["offset"], 3, 1, 1, 1, 1, 1)),
    "deform_conv3d_backward": (_deform3d, ("weight", "bias", "offset", "grad_output"),
                               lambda a: ops.deform_conv3d_backward(a["input"], a["weight"], a["bias"], a["offset"], a["grad_output"], 3, 1, 1, 1, 1, 1)),
    "deform_conv2d_forward": (_deform2d, ("offset", "weight", "bias"),
                              lambda a: ops.deform_conv2d_forward(a["input"], a["offset"], a["weight"], a["bias"], 1, 1, 1)),
    "deform_conv2d_backward": (_deform2d, ("offset", "weight", "grad_output"),
                               lambda a: ops.deform_conv2d_backward(a["input"], a["offset"], a["weight"], a["grad_output"], 1, 1, 1)),
    "conv3d_forward": (_conv3d, ("weight", "bias"), lambda a: ops.conv3d_forward(a["input"], a["weight"], a["bias"], 1, 1, 1, 1)),
    "conv3d_backward": (_conv3d, ("weight", "grad_output"), lambda a: ops.conv3d_backward(a["input"], a["weight"], a["grad_output"], 1, 1, 1, 1)),
}
CASES = [(e, arg, odd) for e, (_, args, _) in ENTRIES.items() for arg in args for odd in ("f32", "f64")]


def case_id(c):
    return "-".join(c)


class _NoLibraryCall:
    """Stands in for the loaded library: any entry the wrapper reaches for fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the wrapper called the library ({name}) with mixed dtypes")


def refuses(dev, entry, arg, odd, monkeypatch):
    """`arg` is float32 among float64 tensors (odd = "f32") or float64 among float32 ones.  NEVER run against a tree without the check on the GPU: the unfixed
    call is an out-of-bounds device read."""
    make, _, call = ENTRIES[entry]
    rest, other = (torch.float64, torch.float32) if odd == "f32" else (torch.float32, torch.float64)
    a = {k: v.to(dev) for k, v in make(rest).items()}
    a[arg] = a[arg].to(other)
    if dev == "cpu":   # the emulator has no launch trace: no entry of the library may be reached at all
        monkeypatch.setattr(L, "get_lib", lambda: _NoLibraryCall())
        with pytest.raises(RuntimeError, match=f"`{arg}`"):
            call(a)
        return
    from tests import parity
    lib = L.get_lib()

    def attempt():
        with pytest.raises(RuntimeError, match=f"`{arg}`"):
            call(a)

    names = parity.kernels_launched(attempt)
    assert not names and lib.dlka_trace_count() == 0, sorted(names)


def same_dtype_still_runs(dev, entry):
    """The check does not get in the way: all-float64 and all-float32 calls go through."""
    make, _, call = ENTRIES[entry]
    for dt in (torch.float32, torch.float64):
        out = call({k: v.to(dev) for k, v in make(dt).items()})
        for t in (out if isinstance(out, tuple) else (out,)):
            assert t is None or (t.dtype == dt and torch.isfinite(t).all())
