"""The backward shortcuts of the fp32 token path off unit scale, on the MI355X (tests/scale_cases.py has the construction, the checks and the bounds).  The shapes are
the smallest that reach each writer and reader of the half hand-over; the library's launch trace names the member that ran."""
import os
import subprocess
import sys
import textwrap

import pytest
import torch

from tests import parity
from tests import scale_cases as cases

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _members(names, prefix):
    return sorted(n for n in names if n.startswith(prefix))


@pytest.mark.parametrize("k", cases.K_ALL)
def test_token_block_at_scale(oracle, k):
    """C = 32, 8^3, B = 2: cl_deform_goff2_kernel<1, float, true, ...> writes, cl_wgrad_samp_kernel<3, float, true, true, ...> (bf16 matrix cores) reads."""
    names = parity.kernels_launched(lambda: cases.block(DEV, 2, 32, (8, 8, 8), k))
    assert _members(names, "cl_deform_goff2_kernel<1, float, true"), _members(names, "cl_deform_goff")
    assert _members(names, "cl_wgrad_samp_kernel<3, float, true, true"), _members(names, "cl_wgrad_samp")
    assert "cl_absmax_bits_kernel" in names


@pytest.mark.parametrize("k", cases.K_ALL)
def test_token_block_at_scale_16_row_writer(oracle, k):
    """The same shape through cl_deform_goff16_kernel<float, true, 4, 3> (DLKA_GOFF16_MIN_ROWS=1)."""
    names = parity.kernels_launched(lambda: cases.block(DEV, 2, 32, (8, 8, 8), k, goff16=True))
    assert _members(names, "cl_deform_goff16_kernel<float, true, 4, 3"), _members(names, "cl_deform_goff")


@pytest.mark.parametrize("k", cases.K_ALL)
@pytest.mark.parametrize("C,dims,nkc", [(64, (4, 4, 8), 2), (128, (4, 4, 4), 4)], ids=["two-chunks", "any-chunks"])
def test_token_block_at_scale_wider(oracle, C, dims, nkc, k):
    """Two 32-channel chunks, and the member for any chunk count (C = 128: the token path takes 32 | 64 | 128 | 256, not 96): NKC_REG = 0 (rows re-read per chunk),
    samples stored."""
    names = parity.kernels_launched(lambda: cases.block(DEV, 1, C, dims, k))
    assert _members(names, "cl_deform_goff2_kernel<0, float, true"), _members(names, "cl_deform_goff")
    assert _members(names, "cl_wgrad_samp_kernel<3, float, true, true"), _members(names, "cl_wgrad_samp")


@pytest.mark.parametrize("k", cases.K_ALL)
def test_token_block_at_scale_ragged_volume(oracle, k):
    cases.block(DEV, 2, 32, (5, 6, 7), k)


def test_token_block_at_scale_fp32_mfma_reader():
    """DLKA_SAMP_B16MFMA=0 (read once per process: a fresh child): cl_wgrad_samp_kernel<3, float, true, false, ...> widens the halves onto fp32-input MFMAs — hand-over
    (b) and metamorphic (c) checks at every k."""
    body = """
    import torch
    from tests import parity, scale_cases as cases
    def run():
        for k in cases.K_ALL:
            cases.handover("cuda", 2, 32, (8, 8, 8), k)
    names = parity.kernels_launched(run)
    assert [n for n in names if n.startswith("cl_wgrad_samp_kernel<3, float, true, false")], sorted(n for n in names if "wgrad_samp" in n)
    print("fp32 mfma reader ok")
    """
    env = dict(os.environ, PYTHONPATH=ROOT, DLKA_SAMP_B16MFMA="0")
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(body)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fp32 mfma reader ok" in r.stdout, r.stdout[-2000:] + "\n" + r.stderr[-4000:]


@pytest.mark.parametrize("k", (-20, 20))
def test_token_block_at_scale_bf16(oracle, k):
    """bf16 activations: the samples are bf16 (fp32's exponent range) — the path is scale-free as it stands; pinned here."""
    names = parity.kernels_launched(lambda: cases.block(DEV, 2, 32, (8, 8, 8), k, bf16=True))
    assert _members(names, "cl_wgrad_samp_kernel<3, bf16_t, false, false"), _members(names, "cl_wgrad_samp")


def test_wrapper_block_at_scale(oracle):
    """ops.tblock3d_* (the wrapper block calls the same deformable backward): k = +20, every gradient against the oracle composition."""
    names = parity.kernels_launched(lambda: cases.wrapper_block(DEV, 2, 32, (8, 8, 8), 20))
    assert _members(names, "cl_wgrad_samp_kernel<3, float, true, true"), _members(names, "cl_wgrad_samp")


@pytest.mark.parametrize("x_log2,go_log2", cases.SCALES_CL)
@pytest.mark.parametrize("Cout,dims", cases.SHAPES_CL)
def test_deform3d_cl_at_scale(oracle, Cout, dims, x_log2, go_log2):
    """Single-operator channels-last entry with x / grad_out at 2^(x_log2, go_log2): forward and all four gradients against the oracle on the two second-generation
    fixed-point windows and the first-generation one (the members test_deform3d_cl_gx_*_members name)."""
    names = parity.kernels_launched(lambda: cases.deform_cl(DEV, Cout, dims, x_log2, go_log2))
    want = "cl_deform_gx_kernel<true, float>" if dims == (3, 4, 40) else "cl_deform_gx_fx2_kernel<"
    assert _members(names, want), _members(names, "cl_deform_gx")


@pytest.mark.parametrize("Cout,dims", cases.SHAPES_CL)
def test_deform3d_cl_one_loud_row_per_brick(oracle, Cout, dims):
    cases.deform_cl_loud_rows(DEV, Cout, dims)
