"""deformablelka_amd.augmentation (csrc/cl_augment.hip) on the MI355X against the fixture recorded from the scipy restatement of the 3-D
trainer's transform chain (tests/golden/reference_augmentation.pt; scipy is not needed here).  The same cases as the emulator suite
(tests/augmentation_cases.py), and two checks of its own: the integer and label paths equal the emulator's bit for bit, and two device runs
are bitwise equal."""
import pytest
import torch

from tests import augmentation_cases as C

from deformablelka_amd import augmentation as A  # noqa: F401  (the feature: without it nothing here can run)

pytestmark = pytest.mark.gpu
DEV = "cuda"
FX = C.load_fixture()
ids = lambda calls: [c[0] for c in calls]   # noqa: E731


@pytest.mark.parametrize("call", C.SPATIAL_CALLS, ids=ids(C.SPATIAL_CALLS))
def test_spatial_values_are_scipys(call):
    C.check_spatial(FX, call, DEV)


@pytest.mark.parametrize("call", C.LABEL_CALLS, ids=ids(C.LABEL_CALLS))
def test_spatial_labels_are_the_per_label_rule(call):
    C.check_labels(FX, call, DEV)


def test_exact_halves_later_label_wins():
    C.check_halves(DEV)


@pytest.mark.parametrize("name", list(C.BLUR_SHAPES))
@pytest.mark.parametrize("i", [0, 1])
def test_gaussian_blur(name, i):
    C.check_blur(FX, name, i, DEV)


def test_channel_statistics():
    C.check_stats(DEV)


@pytest.mark.parametrize("stage", C.POINT_STAGES)
def test_pointwise_stage(stage):
    C.check_point(FX, stage, DEV)


@pytest.mark.parametrize("dt", C.STORAGE_DTYPES)
def test_gaussian_blur_storage_types(dt):
    C.check_blur_storage(dt, DEV)


@pytest.mark.parametrize("dt", C.STORAGE_DTYPES)
def test_channel_statistics_storage_types(dt):
    C.check_stats_storage(dt, DEV)


@pytest.mark.parametrize("dt", ["float64", "bfloat16"])
def test_pointwise_storage_types(dt):
    C.check_point_storage(dt, DEV)


def test_mirror_every_subset_of_axes():
    C.check_mirror(DEV)


def test_deep_supervision_targets_equal_the_references():
    C.check_ds(FX, DEV)


def test_pipeline_with_the_trainers_parameters():
    C.check_pipeline(FX, DEV)


def test_pipeline_seeded_runs_are_bitwise_equal():
    C.check_seeded_runs(DEV)


def test_unsupported_arguments_raise():
    C.check_unsupported(DEV)


def test_containers_and_dtypes():
    C.check_containers(DEV)


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
    assert all(torch.equal(a.cpu(), b) for a, b in zip(C.run_ds(DEV)[1], _on_emulator(C.run_ds)[1]))


def test_two_device_runs_are_bitwise_equal():
    for call in C.SPATIAL_CALLS:
        assert torch.equal(C.run_spatial(call, DEV)[1], C.run_spatial(call, DEV)[1])
    for call in C.LABEL_CALLS:
        assert torch.equal(C.run_labels(call, DEV)[1], C.run_labels(call, DEV)[1])
    for name in C.BLUR_SHAPES:
        assert torch.equal(C.run_blur(name, 0, DEV)[1], C.run_blur(name, 0, DEV)[1])
    for stage in C.POINT_STAGES:
        assert torch.equal(C.run_point(stage, DEV)[1], C.run_point(stage, DEV)[1])
    assert torch.equal(C.check_stats(DEV), C.check_stats(DEV))
