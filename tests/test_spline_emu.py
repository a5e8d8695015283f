"""The shared cubic B-spline preparation (csrc/cl_spline.hip) on the wavefront emulator against the fixture recorded from
scipy.ndimage.spline_filter1d, and bit for bit against the two prefilter kernels it replaced (tests/golden/reference_spline.pt; scipy is not
needed here).  Cases, bound and checks: tests/spline_cases.py."""
import os

import pytest
import torch

from tests import spline_cases as C


@pytest.fixture(scope="module", autouse=True)
def emu_backend():
    from deformablelka_amd import _lib
    from tests import emu
    _lib._set_backend_for_tests(emu.load())
    yield
    _lib._set_backend_for_tests(None)


FX = C.load_fixture()


@pytest.mark.parametrize("cid", list(C.CASES))
def test_coefficients_are_scipys(cid):
    C.check_against_scipy(FX, cid, "cpu")


@pytest.mark.parametrize("cid", list(C.CASES))
def test_coefficients_equal_the_replaced_kernels_bit_for_bit(cid):
    C.check_equals_parent(FX, cid, "cpu")


def test_lines_of_one_cell_come_back_untouched():
    C.check_lines_of_one_cell(FX, "cpu")


@pytest.mark.parametrize("cid", C.PAD_ONLY)
def test_pad_is_the_edge_pad_and_the_cast(cid):
    C.check_pad(FX, cid, "cpu")


def test_prefilter_alone_is_the_routine_without_the_pad():
    C.check_prefilter_alone(FX, "cpu")


def test_an_unknown_boundary_is_refused_and_launches_nothing():
    C.check_unknown_boundary(FX, "cpu")


def test_the_fixture_is_small_and_holds_tensors_only():
    assert os.path.getsize(C.FIXTURE) < 2 ** 20
    assert set(FX) == {"inputs", "ref", "parent"} and set(FX["ref"]) == set(FX["parent"]) == set(C.CASES)
    assert all(isinstance(k, str) and isinstance(v, torch.Tensor) for part in FX.values() for k, v in part.items())
