"""deformablelka_amd.resampling (csrc/cl_resample.hip) on the wavefront emulator against the fixture recorded from the reference's own
resample_data_or_seg, resample_patient and export lines (tests/golden/reference_resampling.pt).  Cases, bounds and checks:
tests/resampling_cases.py."""
import numpy as np
import pytest
import torch

from tests import resampling_cases as C

from deformablelka_amd import resampling  # noqa: F401  (the feature: without it nothing here can run)


@pytest.fixture(scope="module", autouse=True)
def emu_backend():
    from deformablelka_amd import _lib
    from tests import emu
    _lib._set_backend_for_tests(emu.load())
    yield
    _lib._set_backend_for_tests(None)


FX = C.load_fixture()
ids = lambda calls: [c[0] for c in calls]   # noqa: E731


@pytest.mark.parametrize("call", C.VALUE_CALLS, ids=ids(C.VALUE_CALLS))
def test_values_are_the_references(call):
    C.check_values(FX, call, "cpu")


@pytest.mark.parametrize("call", C.LABEL_CALLS, ids=ids(C.LABEL_CALLS))
def test_label_maps_equal_the_references(call):
    C.check_labels(FX, call, "cpu")


def test_exact_halves_and_cells_without_a_majority():
    C.check_half_case_thresholds(FX)


@pytest.mark.parametrize("call", C.ARGMAX_CALLS, ids=ids(C.ARGMAX_CALLS))
def test_fused_argmax_is_the_references(call):
    C.check_argmax(FX, call, "cpu")


@pytest.mark.parametrize("call", C.ARGMAX_CALLS, ids=ids(C.ARGMAX_CALLS))
def test_fused_equals_unfused(call):
    C.check_fused_equals_unfused(call, "cpu")


@pytest.mark.parametrize("call", C.F64_ARGMAX_CALLS, ids=ids(C.F64_ARGMAX_CALLS))
def test_fused_equals_unfused_float64(call):
    C.check_fused_equals_unfused_f64(call, "cpu")


@pytest.mark.parametrize("call", C.REGION_CALLS, ids=ids(C.REGION_CALLS))
def test_regions_overwrite_in_order(call):
    C.check_regions(FX, call, "cpu")


@pytest.mark.parametrize("call", C.EXPORT_CALLS, ids=ids(C.EXPORT_CALLS))
def test_segmentation_from_softmax(call):
    C.check_export(FX, call, "cpu")


def test_segmentation_from_softmax_numpy():
    C.check_export(FX, C.EXPORT_CALLS[0], "cpu", as_numpy=True)


@pytest.mark.parametrize("call", C.PATIENT_CALLS, ids=ids(C.PATIENT_CALLS))
def test_resample_patient(call):
    C.check_patient(FX, call, "cpu")


def test_argument_errors():
    C.check_errors("cpu")


def test_containers_and_dtypes():
    C.check_containers(FX, "cpu")


def test_separate_z_decision():
    from deformablelka_amd import resampling as S
    assert S.RESAMPLING_SEPARATE_Z_ANISO_THRESHOLD == 3
    assert bool(S.get_do_separate_z((3.1, 1.0, 1.0))) and not bool(S.get_do_separate_z((3.0, 1.0, 1.0)))
    assert S.get_lowres_axis((1.0, 5.0, 1.0)).tolist() == [1] and S.get_lowres_axis((0.24, 1.25, 1.25)).tolist() == [1, 2]


def test_the_fixture_is_small_and_plain():
    import os
    assert os.path.getsize(C.FIXTURE) < 2 ** 20
    assert FX["export"]["clamp"]["argmax"].shape == (8, 20, 17)


def test_without_a_gpu_host_data_raises_as_the_metrics_do():
    from deformablelka_amd import _lib, resampling as S
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: host data is moved to it")
    lib = _lib._lib
    _lib._set_backend_for_tests(None)
    try:
        with pytest.raises(RuntimeError, match="libdlka_hip.so is missing|tensors must live on an AMD GPU"):
            S.resample_and_argmax(np.ones((2, 2, 2, 2), np.float32), (3, 3, 3))
    finally:
        _lib._set_backend_for_tests(lib)


# ---- the yardstick itself ---------------------------------------------------------------------------------------------------------------------
def test_restatement_is_what_zoom_returns():
    """tests/resampling_ref.py's resize without the clip is scipy.ndimage.zoom(grid_mode=True, mode='nearest'), bit for bit."""
    pytest.importorskip("scipy")
    from tests import resampling_ref as R
    x = C.make_input("image", "sep0")[0]
    for order in (0, 1, 3):
        assert np.array_equal(R.resize(x, (6, 14, 17), order, clip=False), R.zoom_check(x, (6, 14, 17), order))
