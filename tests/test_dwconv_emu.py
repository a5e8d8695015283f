"""The channels-last depthwise kernels (csrc/cl_dwconv.hip) on the wavefront emulator at the shapes of tests/dwconv_cases.py, against F.conv3d in float64: the
value checks and guard bands of groups A to H.  Left to the GPU file: the member names (the launch trace is GPU-only), the weight-gradient cases of 515 and
1025 rows, and the token-block runs.  The emulator answers a buffer load beyond its descriptor in software; what the hardware answers is the GPU file's to see."""
import pytest

from tests import dwconv_cases as cases
from tests import parity


@pytest.fixture(scope="module", autouse=True)
def emu_backend(oracle):
    from deformablelka_amd import _lib
    from tests import emu
    _lib._set_backend_for_tests(emu.load())
    yield
    _lib._set_backend_for_tests(None)


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    """DLKA_DW_LDS and DLKA_XCD_MIN unset; the library's cached switches follow the environment into the test and out of it."""
    monkeypatch.delenv("DLKA_DW_LDS", raising=False)
    monkeypatch.delenv("DLKA_XCD_MIN", raising=False)
    parity._refresh_switches()
    yield
    monkeypatch.undo()
    parity._refresh_switches()


DEV = "cpu"


@pytest.mark.parametrize("case", cases.FORWARD_CASES, ids=cases.case_id)
def test_forward_and_data_gradient_members(case):
    cases.single_op(DEV, case)


def test_without_bias():
    cases.single_op(DEV, cases.BIAS_NONE_CASE, with_bias=False)


@pytest.mark.parametrize("case", cases.SWIZZLE_CASES, ids=cases.case_id)
def test_swizzled_grid_with_padding_workgroups_equals_the_plain_one(case, monkeypatch):
    cases.swizzle(DEV, case, monkeypatch)
