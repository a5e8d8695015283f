"""The channels-last depthwise kernels (csrc/cl_dwconv.hip) on the MI355X, member by member, against F.conv3d in float64 on the CPU (tests/dwconv_cases.py has
the cases, the check and the guard bands).  The launch trace names the member every case ran.  Everything tests/test_dwconv_emu.py runs, plus the member names,
the weight-gradient kernels above their row thresholds and the members only the token block reaches."""
import pytest
import torch

from tests import dwconv_cases as cases
from tests import parity

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def hip_backend(oracle):
    from deformablelka_amd import _lib
    _lib._set_backend_for_tests(None)
    assert torch.cuda.is_available()
    _lib.get_lib()   # fails loudly if libdlka_hip.so is missing — no fallback
    yield


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    """DLKA_DW_LDS and DLKA_XCD_MIN unset; the library's cached switches follow the environment into the test and out of it."""
    monkeypatch.delenv("DLKA_DW_LDS", raising=False)
    monkeypatch.delenv("DLKA_XCD_MIN", raising=False)
    parity._refresh_switches()
    yield
    monkeypatch.undo()
    parity._refresh_switches()


# ---- A to G: the five forward / data-gradient members; every case also runs the first-generation weight gradient ---------------------------------------------------
@pytest.mark.parametrize("case", cases.FORWARD_CASES, ids=cases.case_id)
def test_forward_and_data_gradient_members(case):
    cases.single_op(DEV, case, trace=True)


def test_without_bias():
    cases.single_op(DEV, cases.BIAS_NONE_CASE, with_bias=False, trace=True)


# ---- H: the XCD swizzle's padding workgroups -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.SWIZZLE_CASES, ids=cases.case_id)
def test_swizzled_grid_with_padding_workgroups_equals_the_plain_one(case, monkeypatch):
    cases.swizzle(DEV, case, monkeypatch, trace=True)


# ---- I: the weight-gradient members above the row thresholds: a short last row chunk ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.WGRAD_CASES, ids=cases.case_id)
def test_weight_gradient_members_with_a_short_last_chunk(case):
    cases.single_op(DEV, case, trace=True)


# ---- J: members only the token block reaches ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,C,dims", cases.TOKEN_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_token_block_runs_the_two_row_kernels_of_its_storage_type(B, C, dims, bf16, monkeypatch):
    cases.token_block(DEV, B, C, dims, bf16, monkeypatch)


def test_acdc_token_block_runs_the_one_row_kernel_of_5_taps_dilation_3(monkeypatch):
    cases.token_block_acdc(DEV, monkeypatch)
