"""The dense channels-last conv kernels (csrc/cl_igemm.hip, cl_conv_wave.hip, cl_conv_kw.hip) on the MI355X, member by member, against F.conv3d in float64 on the
CPU (tests/dense_conv_cases.py has the cases, the check and the guard bands).  The launch trace names the forward and the data-gradient member every case ran.
Everything tests/test_dense_conv_emu.py runs, plus the member names and the two large-row groups: K6 / K7 (several column tiles per workgroup) and I1
(cl_igemm_kernel with three-term operands on a swizzled grid with padding workgroups)."""
import pytest
import torch

from tests import dense_conv_cases as cases
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
    """DLKA_IGEMM_NT and DLKA_XCD_MIN unset; the library's cached switches follow the environment into the test and out of it."""
    monkeypatch.delenv("DLKA_IGEMM_NT", raising=False)
    monkeypatch.delenv("DLKA_XCD_MIN", raising=False)
    parity._refresh_switches()
    yield
    monkeypatch.undo()
    parity._refresh_switches()


# ---- K: cl_conv_kw_kernel, the contraction split over the waves of a workgroup ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.K_CASES, ids=cases.case_id)
def test_wave_split_members_are_right_and_reproducible(case):
    cases.reproducible(DEV, case, trace=True)


# ---- W: the tap split over gridDim.y with fp32 atomics (D = 1) ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.W_CASES, ids=cases.case_id)
def test_tap_split_members(case):
    cases.single_op(DEV, case, trace=True)


@pytest.mark.parametrize("case,runs", cases.W5_CASES, ids=lambda v: cases.case_id(v) if isinstance(v, cases.Case) else "")
def test_forced_column_tiles(case, runs, monkeypatch):
    cases.forced_column_tiles(DEV, case, runs, monkeypatch, trace=True)


# ---- I: cl_igemm_kernel with three-term operands; the XCD swizzle's padding workgroups ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.I_CASES, ids=cases.case_id)
def test_three_term_igemm_on_a_swizzled_grid_with_padding_workgroups(case, monkeypatch):
    cases.swizzle(DEV, case, monkeypatch, trace=True)


# ---- E: K = 1 with a planar output on the exact fp32-input MFMA ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.E_CASES, ids=cases.case_id)
def test_pointwise_with_planar_output_on_the_exact_mfma(case):
    cases.exact_pointwise_planar(DEV, case, trace=True)
