"""The shared cubic B-spline preparation (csrc/cl_spline.hip) on the MI355X against the fixture recorded from scipy.ndimage.spline_filter1d, and
bit for bit against what the two prefilter kernels it replaced gave on the emulator (tests/golden/reference_spline.pt; scipy is not needed
here): the order of the float64 operations is theirs and contraction is off.  The same cases as the emulator suite (tests/spline_cases.py)."""
import pytest

from tests import spline_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
FX = C.load_fixture()


@pytest.mark.parametrize("cid", list(C.CASES))
def test_coefficients_are_scipys(cid):
    C.check_against_scipy(FX, cid, DEV)


@pytest.mark.parametrize("cid", list(C.CASES))
def test_coefficients_equal_the_replaced_kernels_bit_for_bit(cid):
    C.check_equals_parent(FX, cid, DEV)


def test_lines_of_one_cell_come_back_untouched():
    C.check_lines_of_one_cell(FX, DEV)


@pytest.mark.parametrize("cid", C.PAD_ONLY)
def test_pad_is_the_edge_pad_and_the_cast(cid):
    C.check_pad(FX, cid, DEV)


def test_prefilter_alone_is_the_routine_without_the_pad():
    C.check_prefilter_alone(FX, DEV)


def test_an_unknown_boundary_is_refused_and_launches_nothing():
    C.check_unknown_boundary(FX, DEV)
