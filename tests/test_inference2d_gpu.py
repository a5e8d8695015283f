"""deformablelka_amd.inference2d (csrc/cl_zoom2d.hip) on the MI355X against the fixture recorded from scipy.ndimage.zoom and the restatement of
the reference's test_single_volume (tests/golden/reference_inference2d.pt; scipy is not needed here).  The same cases as the emulator suite
(tests/inference2d_cases.py), and two checks of its own: the label and argmax outputs equal the emulator's bit for bit, and two device runs of
every case are bitwise equal."""
import pytest
import torch

from tests import inference2d_cases as C

from deformablelka_amd import inference2d as I2  # noqa: F401  (the feature: without it nothing here can run; the MODULE, never a test_* name)

pytestmark = pytest.mark.gpu
DEV = "cuda"
FX = C.load_fixture()
ids = lambda calls: [c[0] for c in calls]   # noqa: E731


@pytest.mark.parametrize("call", C.ZOOM_CALLS, ids=ids(C.ZOOM_CALLS))
def test_zoom_values_are_scipys(call):
    C.check_zoom(FX, call, DEV)


@pytest.mark.parametrize("dt", C.LABEL_DTYPES)
@pytest.mark.parametrize("case", list(C.ZOOM_SHAPES))
def test_zoom_labels_are_equal(case, dt):
    C.check_zoom_labels(FX, case, dt, DEV)


@pytest.mark.parametrize("order", [1, 3])
@pytest.mark.parametrize("case", list(C.ZOOM_SHAPES))
def test_fused_normalize_and_bf16_store_are_bitwise(case, order):
    C.check_normalize_and_bf16(case, order, DEV)


def test_bf16_slices_through_two_taps_are_bitwise():
    C.check_bf16_slices_two_taps(DEV)


@pytest.mark.parametrize("call", C.ARGMAX_CALLS, ids=ids(C.ARGMAX_CALLS))
def test_argmax_fused_with_the_zoom_back(call):
    C.check_argmax(FX, call, DEV)


def test_end_to_end_patch_equal_to_the_slice_size():
    C.check_e2e_a(FX, DEV)


def test_end_to_end_patch_different_from_the_slice_size():
    C.check_e2e_b(FX, DEV)


def test_slice_batch_does_not_change_a_bit():
    C.check_slice_batch(DEV)


def test_the_2d_image_branch():
    C.check_image_2d(FX, DEV)


def test_inference_over_two_cases():
    C.check_inference(FX, DEV)


def test_resize_sample():
    C.check_resize_sample(FX, DEV)


def test_unsupported_arguments_raise():
    C.check_unsupported(DEV)


def test_containers_and_dtypes():
    C.check_containers(FX, DEV)


def test_launch_counts_do_not_depend_on_the_number_of_slices():
    C.check_launch_counts(DEV)


def test_the_nets_training_flag_is_restored():
    C.check_training_flag(DEV)


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


def test_label_and_argmax_outputs_equal_the_emulators_bit_for_bit():
    for call in C.ZOOM_CALLS:
        if call[2] == "int16" or call[3] == 0:
            assert torch.equal(C.run_zoom(call, DEV)[1].cpu(), _on_emulator(C.run_zoom, call)[1])
    for case in C.ZOOM_SHAPES:
        for dt in C.LABEL_DTYPES:
            assert torch.equal(C.check_zoom_labels(FX, case, dt, DEV).cpu(), _on_emulator(C.check_zoom_labels, FX, case, dt))
    for call in C.ARGMAX_CALLS:
        assert torch.equal(C.run_argmax(call, DEV).cpu(), _on_emulator(C.run_argmax, call))
    assert torch.equal(C.run_e2e("b", DEV)[3][1].cpu(), _on_emulator(C.run_e2e, "b")[3][1])


def test_two_device_runs_are_bitwise_equal():
    for call in C.ZOOM_CALLS:
        assert torch.equal(C.run_zoom(call, DEV)[1], C.run_zoom(call, DEV)[1])
    for call in C.ARGMAX_CALLS:
        assert torch.equal(C.run_argmax(call, DEV), C.run_argmax(call, DEV))
    a, b = C.run_e2e("b", DEV)[3], C.run_e2e("b", DEV)[3]
    assert torch.equal(a[1], b[1]) and a[0] == b[0]
