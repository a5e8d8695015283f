"""The dummy-2D branch of deformablelka_amd.augmentation (the in-plane kernels of csrc/cl_augment.hip) on the MI355X against the fixture
recorded from the scipy restatement of the ACDC trainer's transform chain (tests/golden/reference_augmentation2d.pt; scipy is not needed
here).  The same cases as the emulator suite (tests/augmentation2d_cases.py), and two checks of its own: the integer and label paths equal
the emulator's bit for bit, and two device runs are bitwise equal."""
import pytest
import torch

from tests import augmentation2d_cases as C

from deformablelka_amd import augmentation as A  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda"
FX = C.load_fixture()
ids = lambda calls: [c[0] for c in calls]   # noqa: E731


@pytest.mark.parametrize("call", C.SPATIAL_CALLS, ids=ids(C.SPATIAL_CALLS))
def test_spatial_values_are_scipys_on_2d_planes(call):
    C.check_spatial(FX, call, DEV)


@pytest.mark.parametrize("call", C.LABEL_CALLS, ids=ids(C.LABEL_CALLS))
def test_spatial_labels_are_the_per_label_rule_on_4_neighbours(call):
    C.check_labels(FX, call, DEV)


@pytest.mark.parametrize("mode", ["constant", "nearest"])
def test_tiny_plane_narrower_than_a_lane(mode):
    C.check_tiny(FX, mode, DEV)


def test_exact_halves_later_label_wins():
    C.check_halves(DEV)


def test_planes_do_not_depend_on_their_neighbours_in_depth():
    C.check_depth_independence(DEV)


def test_launch_count_does_not_depend_on_batch_channels_or_depth():
    C.check_launch_count(DEV)


def test_low_resolution_keeps_the_ignored_axis():
    C.check_lowres(FX, DEV)


def test_pipeline_with_the_acdc_trainers_parameters():
    C.check_pipeline(FX, DEV)


def test_pipeline_seeded_runs_are_bitwise_equal():
    C.check_seeded_runs(DEV)


def test_refusals():
    C.check_refusals(DEV)


def test_c_entries_refuse_with_a_status():
    C.check_c_interface_refusals(DEV)


def _on_emulator(fn, *args):
    from deformablelka_amd import _lib
    from tests import emu
    lib = _lib._lib
    _lib._set_backend_for_tests(emu.load())
    try:
        return fn(*args, "cpu")
    finally:
        _lib._set_backend_for_tests(None)
        _lib._lib = lib


def test_integer_and_label_paths_equal_the_emulators_bit_for_bit():
    for call in C.SPATIAL_CALLS:
        if call[1] == "int16":
            assert torch.equal(C.run_spatial(call, DEV)[1].cpu(), _on_emulator(C.run_spatial, call)[1])
    for call in C.LABEL_CALLS:
        assert torch.equal(C.run_labels(call, DEV)[1].cpu(), _on_emulator(C.run_labels, call)[1])


def test_two_device_runs_are_bitwise_equal():
    for call in C.SPATIAL_CALLS:
        assert torch.equal(C.run_spatial(call, DEV)[1], C.run_spatial(call, DEV)[1])
    for call in C.LABEL_CALLS:
        assert torch.equal(C.run_labels(call, DEV)[1], C.run_labels(call, DEV)[1])
    assert torch.equal(C.run_lowres(DEV)[1], C.run_lowres(DEV)[1])
