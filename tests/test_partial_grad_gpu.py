"""Partial-gradient (null output pointers) and bf16 calls of the single-operator entry points on the MI355X: NaN-poisoned, guarded outputs against the
oracle (tests/partial_grad_cases.py has the cases, the tolerances and their derivation).  The same list as tests/test_partial_grad_emu.py — these are the
smallest shapes at which each branch is live — plus what the emulator file leaves out for time (the Og > 32 shape's subsets with grad_weight) and the
split-K shape of the channels-last conv."""
import pytest

from tests import partial_grad_cases as cases

pytestmark = pytest.mark.gpu

DEV = "cuda"


# ---- every non-empty subset of the outputs, fp32 and f64 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("need", cases.SUBSETS4, ids=cases.need_id)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("case", cases.DEFORM3D, ids=cases.case_id)
def test_deform3d_subsets(oracle, case, dtype, need):
    cases.deform3d_subset(DEV, case, dtype, need)


@pytest.mark.parametrize("need", cases.SUBSETS3 + cases.SUBSETS4, ids=cases.need_id2d)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("case", cases.DEFORM2D, ids=cases.case_id)
def test_deform2d_subsets_without_and_with_bias(oracle, case, dtype, need):
    cases.deform2d_subset(DEV, case, dtype, need)


@pytest.mark.parametrize("need", cases.SUBSETS3, ids=cases.need_id)
@pytest.mark.parametrize("case,dtype", [(c, "f32") for c in cases.CONV3D] + [(cases.CONV3D[0], "f64")], ids=lambda v: v if isinstance(v, str) else cases.case_id(v))
def test_conv3d_subsets(case, dtype, need):
    cases.conv3d_subset(DEV, case, dtype, need)


@pytest.mark.parametrize("need", cases.SUBSETS3, ids=cases.need_id)
@pytest.mark.parametrize("case", cases.CONV_CL + [cases.CONV_CL_SPLIT_K], ids=cases.case_id)
def test_conv3d_cl_subsets(case, need):
    cases.conv_cl_subset(DEV, case, need)


@pytest.mark.parametrize("need", cases.SUBSETS4, ids=cases.need_id)
@pytest.mark.parametrize("route", cases.ROUTES)
@pytest.mark.parametrize("case", cases.DEFORM_CL, ids=cases.case_id)
def test_deform3d_cl_subsets(oracle, case, route, need):
    cases.deform_cl_subset(DEV, case, "f32", need, route)


# ---- bf16 -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.DEFORM3D_BF16, ids=cases.case_id)
def test_deform3d_bf16_forward(oracle, case):
    cases.deform3d_forward(DEV, case, "bf16")


@pytest.mark.parametrize("need", [(True,) * 4] + cases.SINGLES4, ids=cases.need_id)
@pytest.mark.parametrize("case", cases.DEFORM3D_BF16, ids=cases.case_id)
def test_deform3d_bf16_backward(oracle, case, need):
    cases.deform3d_subset(DEV, case, "bf16", need)


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("case", cases.DEFORM2D_BF16, ids=cases.case_id)
def test_deform2d_bf16_forward(oracle, case, with_bias):
    cases.deform2d_forward(DEV, case, "bf16", with_bias)


@pytest.mark.parametrize("need", [(True,) * 4] + cases.SINGLES4, ids=cases.need_id2d)
@pytest.mark.parametrize("case", cases.DEFORM2D_BF16, ids=cases.case_id)
def test_deform2d_bf16_backward(oracle, case, need):
    cases.deform2d_subset(DEV, case, "bf16", need)


@pytest.mark.parametrize("case", cases.CONV3D_BF16, ids=cases.case_id)
def test_conv3d_bf16_forward(case):
    cases.conv3d_forward(DEV, case, "bf16")


@pytest.mark.parametrize("need", [(True,) * 3] + cases.SINGLES3, ids=cases.need_id)
@pytest.mark.parametrize("case", cases.CONV3D_BF16, ids=cases.case_id)
def test_conv3d_bf16_backward(case, need):
    cases.conv3d_subset(DEV, case, "bf16", need)


@pytest.mark.parametrize("case", cases.DEFORM_CL_BF16, ids=cases.case_id)
def test_deform3d_cl_bf16_forward(oracle, case):
    """`out` (bf16 storage) of the single-operator entry per element: it keeps the fp32-input MFMA — fp32 samples, exact products, one rounding at the store —
    as the general operator does; the bf16 matrix cores, which round every sample, are the fused block's choice (cl_host_ops.hip: deform_forward)."""
    cases.deform_cl_forward(DEV, case, "bf16")


@pytest.mark.parametrize("need", cases.SUBSETS4, ids=cases.need_id)
@pytest.mark.parametrize("route", cases.ROUTES)
@pytest.mark.parametrize("case", cases.DEFORM_CL_BF16, ids=cases.case_id)
def test_deform3d_cl_bf16_subsets_and_the_refused_ones(oracle, case, route, need):
    cases.deform_cl_subset(DEV, case, "bf16", need, route)


# ---- the wrappers and the product's autograd Functions ---------------------------------------------------------------------------------------------------
def test_cl_wrappers_take_need(oracle):
    cases.wrappers_return_none_for_what_is_not_needed(DEV)


def test_cl_wrappers_with_nothing_needed_return_none_without_a_library_call():
    cases.wrappers_with_nothing_needed_do_not_call_the_library(DEV)


def test_deform3d_cl_wrapper_bf16_allocates_fp32_gradients(oracle):
    cases.wrapper_bf16_deform_cl(DEV)


def test_conv3d_cl_refuses_bf16():
    cases.conv_cl_refuses_bf16(DEV)


@pytest.mark.parametrize("which", ["offset_only", "all_but_offset", "bias_frozen"])
def test_autograd_deform_conv2d_partial(oracle, which):
    cases.autograd_deform_conv2d(DEV, which)


@pytest.mark.parametrize("which", ["first_conv", "frozen_weight"])
def test_autograd_conv3d_partial(which):
    cases.autograd_conv3d(DEV, which)
