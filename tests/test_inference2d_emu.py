"""deformablelka_amd.inference2d (csrc/cl_zoom2d.hip) on the wavefront emulator against the fixture recorded from scipy.ndimage.zoom and the
restatement of the reference's test_single_volume (tests/golden/reference_inference2d.pt), and that restatement against the fixture.  Cases,
bounds and checks: tests/inference2d_cases.py."""
import os

import numpy as np
import pytest
import torch

from tests import inference2d_cases as C

from deformablelka_amd import inference2d as I2  # noqa: F401  (the feature: without it nothing here can run; the MODULE, never a test_* name)


@pytest.fixture(scope="module", autouse=True)
def emu_backend():
    from deformablelka_amd import _lib
    from tests import emu
    _lib._set_backend_for_tests(emu.load())
    yield
    _lib._set_backend_for_tests(None)


FX = C.load_fixture()
ids = lambda calls: [c[0] for c in calls]   # noqa: E731


@pytest.mark.parametrize("call", C.ZOOM_CALLS, ids=ids(C.ZOOM_CALLS))
def test_zoom_values_are_scipys(call):
    C.check_zoom(FX, call, "cpu")


@pytest.mark.parametrize("dt", C.LABEL_DTYPES)
@pytest.mark.parametrize("case", list(C.ZOOM_SHAPES))
def test_zoom_labels_are_equal(case, dt):
    C.check_zoom_labels(FX, case, dt, "cpu")


@pytest.mark.parametrize("order", [1, 3])
@pytest.mark.parametrize("case", list(C.ZOOM_SHAPES))
def test_fused_normalize_and_bf16_store_are_bitwise(case, order):
    C.check_normalize_and_bf16(case, order, "cpu")


def test_bf16_slices_through_two_taps_are_bitwise():
    C.check_bf16_slices_two_taps("cpu")


@pytest.mark.parametrize("call", C.ARGMAX_CALLS, ids=ids(C.ARGMAX_CALLS))
def test_argmax_fused_with_the_zoom_back(call):
    C.check_argmax(FX, call, "cpu")


def test_end_to_end_patch_equal_to_the_slice_size():
    C.check_e2e_a(FX, "cpu")


def test_end_to_end_patch_different_from_the_slice_size():
    C.check_e2e_b(FX, "cpu")


def test_slice_batch_does_not_change_a_bit():
    C.check_slice_batch("cpu")


def test_the_2d_image_branch():
    C.check_image_2d(FX, "cpu")


def test_inference_over_two_cases():
    C.check_inference(FX, "cpu")


def test_resize_sample():
    C.check_resize_sample(FX, "cpu")


def test_unsupported_arguments_raise():
    C.check_unsupported("cpu")


def test_containers_and_dtypes():
    C.check_containers(FX, "cpu")


def test_launch_counts_do_not_depend_on_the_number_of_slices():
    C.check_launch_counts("cpu")


def test_the_nets_training_flag_is_restored():
    C.check_training_flag("cpu")


def test_the_fixture_is_small_and_plain():
    assert os.path.getsize(C.FIXTURE) < 2 ** 20

    def plain(v):
        if isinstance(v, dict):
            return all(isinstance(k, (str, int)) and plain(x) for k, x in v.items())
        if isinstance(v, (list, tuple)):
            return all(plain(x) for x in v)
        return v is None or isinstance(v, (torch.Tensor, str, int, float, bool))
    assert plain(FX)


def test_the_c_abi_refuses_what_it_cannot_do():
    import ctypes
    from deformablelka_amd import _lib as L, ops
    lib = L.get_lib()
    x = torch.zeros(1, 4, 4)
    d = L.Zoom2dDesc()
    d.N, d.taps, d.in_dtype, d.out_dtype = 1, 3, L.DLKA_F32, L.DLKA_F32
    for ax in range(2):
        d.in_[ax], d.out[ax] = 4, 4
    y, idx, w = torch.zeros(1, 4, 4), torch.zeros(8, dtype=torch.int32), torch.zeros(32, dtype=torch.float64)
    before = ops.zoom2d_launch_count()
    assert lib.dlka_zoom2d_spline(L.ptr(x), L.ptr(y), ctypes.byref(d), L.ptr(idx), L.ptr(w), None) == -8          # taps
    d.taps, d.in_dtype = 4, L.DLKA_F32
    assert lib.dlka_zoom2d_spline(L.ptr(x), L.ptr(y), ctypes.byref(d), L.ptr(idx), L.ptr(w), None) == -6          # coefficients are float64
    d.taps, d.out_dtype, d.in_dtype, d.normalize = 2, L.DLKA_ZOOM2D_I16, L.DLKA_ZOOM2D_I16, 1
    assert lib.dlka_zoom2d_spline(L.ptr(x), L.ptr(y), ctypes.byref(d), L.ptr(idx), L.ptr(w), None) == -8          # Normalize of integers
    assert lib.dlka_zoom2d_nearest(L.ptr(x), L.ptr(y), ctypes.byref(d), 3, L.ptr(idx), None) == -6
    assert lib.dlka_zoom2d_nearest(L.ptr(x), L.ptr(x), ctypes.byref(d), 4, L.ptr(idx), None) == -8
    assert lib.dlka_zoom2d_argmax(L.ptr(x), L.ptr(y), ctypes.byref(d), 256, L.ptr(idx), None) == -8
    assert lib.dlka_zoom2d_argmax(None, L.ptr(y), ctypes.byref(d), 2, L.ptr(idx), None) == -1
    d.out[1] = 0
    assert lib.dlka_zoom2d_nearest(L.ptr(x), L.ptr(y), ctypes.byref(d), 4, L.ptr(idx), None) == -4
    assert ops.zoom2d_launch_count() == before
    with pytest.raises(RuntimeError, match="index table"):
        ops.zoom2d_index_tables([np.arange(5), np.arange(4)], (4, 4), "cpu")


def test_the_tables_hold_the_overshoot_pairs():
    """the pairs whose last coordinate exceeds n - 1, in the product's own tables."""
    for (n, m), over in (((512, 224), True), ((32, 16), True), ((28, 24), True), ((224, 512), False), ((19, 16), False), ((21, 24), False)):
        assert C.overshoots(n, m) == over
        for order in (0, 1, 3):
            first = I2._axis_table(n, m, order)[0]
            outside = first == (-1 if order == 0 else -2 ** 31)
            assert not outside[:-1].any() and bool(outside[-1]) == over


def test_restatement_reproduces_the_fixture():
    """tests/inference2d_ref.py (scipy) gives the recorded end-to-end results on this machine too."""
    pytest.importorskip("scipy")
    from tests import inference2d_ref as R
    shape, patch = C.E2E_B
    image, label = C.e2e_image(shape, C.E2E_B_SALT), C.e2e_label(shape, 37)
    ml, pred, _ = R.single_volume(image[None], label[None], C.StandInNet(), C.E2E_CLASSES, list(patch))
    assert np.array_equal(pred, FX["e2e_b"]["prediction"].numpy()) and [tuple(float(v) for v in m) for m in ml] == FX["e2e_b"]["metric_list"]
