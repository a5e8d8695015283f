"""Shared cases of tests/test_scale_emu.py and tests/test_scale_gpu.py: the backward shortcuts of the fp32 token path OFF unit scale.

The deformable conv's samples cross HBM as IEEE halves (DeformBwdArgs::samp_f16), grad_input accumulates in fixed point with a per-brick scale, the contractions
are two-term bf16 splits.  Every other test draws activations and gradients from N(0, 1); the reference (fp32 throughout) does not depend on scale, so neither may we.

Rescaling t exactly.  t is the deformable conv's input (= conv_spatial's output).  With s = 2^k, on a fresh block after blocks.randomize_offsets_:

    conv_spatial.weight, .bias   *= s          t          -> s t            (exactly: a power of two commutes with every fp32 rounding)
    conv_offset.weight           *= 1 / s      offsets    -> the same numbers
    deform_conv.weight           *= 1 / s      the output -> the same numbers

so the sampled cells, the block's output and every tensor outside that stretch are what they are at k = 0, the parameter gradients move by exact powers of two
(deform_conv.weight.grad by s), and the CPU oracle is fed the same rescaled parameters.  K_ALL = (-24, -12, 0, +12, +20): half normals end at 2^-14 and 65504 and |t|
reaches a few units, so +20 would saturate nearly every unscaled half, -24 puts a typical one at a single subnormal quantum, +-12 straddle the edges, 0 is the old coverage.

Checks at each k — no tolerance of their own:
  (a) parity.check_lka3d_tokens: the flips-counted + same-cells protocol against the oracle at parity.FWD_ATOL / BWD_RTOL, every gradient;
  (b) parity.check_lka3d_tokens_sample_handover: the stored-sample weight gradient against the gathering kernel at its 5e-4 / 1e-5 (fp32), 2e-2 (bf16);
  (c) metamorphic: deform_conv.weight.grad of (b)'s run at k, times 2^-k, against (b)'s run at k = 0, within the same 5e-4 of max (2e-2 for bf16).

That the bounds can be met at every k by the reference-exact route was checked on the emulator before the fix went in: with DLKA_SAMP_F16=0 (fp32 samples) all five
values of k pass (a) - (c) on the unmodified parent (every case of tests/test_scale_emu.py); with the parent's default (clamped, unscaled halves)
deform_conv.weight.grad missed (a)'s 1e-3 at k = -24 (5.4e-3), -12 (3.0e-3) and +20 (6.3e-3) at C = 32, (3, 4, 5) — DESIGN 4.4.

Not here: a non-finite sample at block level.  A non-finite element of t makes the predicted offsets of its neighbourhood NaN (conv_offset reads t), and neither the
oracle nor the reference's backward, which it restates line by line, guards a NaN coordinate (`q <= -1 || q >= size` is false for NaN: the floor is used as an index)."""
import functools
import os

import torch

from tests import parity

K_ALL = (-24, -12, 0, 12, 20)
DCW = "spatial_gating_unit.deform_conv.weight"
HANDOVER_RTOL = 5e-4     # parity.check_lka3d_tokens_sample_handover, fp32
HANDOVER_RTOL_BF16 = 2e-2


def _sgu(m):
    for name, mod in m.named_modules():
        if name.endswith("spatial_gating_unit"):
            return mod
    raise AssertionError("no spatial_gating_unit in the module")


def rescale_t(k):
    """prepare(module) for the parity helpers: t -> 2^k t, everything else unchanged (module docstring)."""
    def prepare(m):
        s = 2.0 ** k
        g = _sgu(m)
        with torch.no_grad():
            g.conv_spatial.weight.mul_(s)
            g.conv_spatial.bias.mul_(s)
            g.deform_conv.conv_offset.weight.mul_(1.0 / s)
            g.deform_conv.weight.mul_(1.0 / s)
    return prepare


class env:
    """DLKA_* switches that the library reads per call (not the read-once ones: those need a fresh process)."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def _handover_run(dev, B, C, dims, bf16, k, goff16):
    """(b) at k; returns the stored-sample run's deform_conv.weight.grad (CPU, fp32).  Cached: the k = 0 run is shared by every k's metamorphic check."""
    with env(**({"DLKA_GOFF16_MIN_ROWS": "1"} if goff16 else {})):
        g = parity.check_lka3d_tokens_sample_handover(dev, B, C, dims, dtype=torch.bfloat16 if bf16 else torch.float32, prepare=rescale_t(k))
    return g[DCW].clone()


def handover(dev, B, C, dims, k, bf16=False, goff16=False):
    """(b) and (c)."""
    gk = _handover_run(dev, B, C, tuple(dims), bf16, k, goff16)
    assert torch.isfinite(gk).all()
    if k == 0:
        return
    g0 = _handover_run(dev, B, C, tuple(dims), bf16, 0, goff16)
    err = parity.rel_err(gk * 2.0 ** -k, g0)
    print(f"[scale k={k:+d} C={C} dims={dims}{' bf16' if bf16 else ''}] deform_conv.weight.grad * 2^{-k} vs the k = 0 run: {err:.3e} of max")
    assert err <= (HANDOVER_RTOL_BF16 if bf16 else HANDOVER_RTOL), err


def oracle_protocol(dev, B, C, dims, k, bf16=False, goff16=False):
    """(a)."""
    with env(**({"DLKA_GOFF16_MIN_ROWS": "1"} if goff16 else {})):
        if bf16:
            parity.check_lka3d_tokens_bf16(dev, B, C, dims, prepare=rescale_t(k))
        else:
            parity.check_lka3d_tokens(dev, B, C, dims, offset_std=0.3, prepare=rescale_t(k))


def block(dev, B, C, dims, k, bf16=False, goff16=False):
    oracle_protocol(dev, B, C, dims, k, bf16, goff16)
    handover(dev, B, C, dims, k, bf16, goff16)


def wrapper_block(dev, B, C, dims, k):
    """The wrapper block (ops.tblock3d_*) with the D-LKA attention inside at 2^k: every gradient at the contract's tolerances (parity.check_tblock3d)."""
    parity.check_tblock3d(dev, B, C, dims, True, True, offset_std=0.3, prepare=rescale_t(k))


# ---- the single-operator channels-last entry ------------------------------------------------------------------------------------------------------------------
SCALES_CL = ((-20, 20), (20, -20), (20, 20))      # (x_log2, go_log2)
SHAPES_CL = ((32, (8, 8, 16)), (64, (4, 4, 32)), (32, (3, 4, 40)))   # Cout, dims: the two gx_fx2 windows, and the first-generation fixed-point window


def deform_cl(dev, Cout, dims, x_log2, go_log2):
    parity.check_deform3d_cl(dev, 1, 32, Cout, dims, off_mode="normal", seed=3, x_log2=x_log2, go_log2=go_log2)


def deform_cl_loud_rows(dev, Cout, dims):
    """grad_out ~ N(0, 1) except one row (voxel) per 4 x 4 x 4 brick, 2^12 times larger: the fixed-point scale of a brick comes from its own rows' norms, so the loud row sets it
    and the quiet rows keep 12 bits less — still inside the contract's tolerance relative to max |reference|."""
    def hook(go):
        go = go.clone()
        D, H, W = go.shape[2:]
        go[:, :, 1::4, 2::4, 3::4] *= 2.0 ** 12
        return go
    parity.check_deform3d_cl(dev, 1, 32, Cout, dims, off_mode="normal", seed=4, go_hook=hook)
