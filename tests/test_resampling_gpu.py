"""deformablelka_amd.resampling (csrc/cl_resample.hip) on the MI355X against the fixture recorded from the reference's own
resample_data_or_seg, resample_patient and export lines (tests/golden/reference_resampling.pt; scipy is not needed here).  The same cases as
the emulator suite (tests/resampling_cases.py), and the chain export -> post-processing -> metrics on the device."""
import pytest
import torch

from tests import resampling_cases as C

from deformablelka_amd import resampling  # noqa: F401  (the feature: without it nothing here can run)

pytestmark = pytest.mark.gpu
DEV = "cuda"
FX = C.load_fixture()
ids = lambda calls: [c[0] for c in calls]   # noqa: E731


@pytest.mark.parametrize("call", C.VALUE_CALLS, ids=ids(C.VALUE_CALLS))
def test_values_are_the_references(call):
    C.check_values(FX, call, DEV)


@pytest.mark.parametrize("call", C.LABEL_CALLS, ids=ids(C.LABEL_CALLS))
def test_label_maps_equal_the_references(call):
    C.check_labels(FX, call, DEV)


@pytest.mark.parametrize("call", C.ARGMAX_CALLS, ids=ids(C.ARGMAX_CALLS))
def test_fused_argmax_is_the_references(call):
    C.check_argmax(FX, call, DEV)


@pytest.mark.parametrize("call", C.ARGMAX_CALLS, ids=ids(C.ARGMAX_CALLS))
def test_fused_equals_unfused(call):
    C.check_fused_equals_unfused(call, DEV)


@pytest.mark.parametrize("call", C.F64_ARGMAX_CALLS, ids=ids(C.F64_ARGMAX_CALLS))
def test_fused_equals_unfused_float64(call):
    C.check_fused_equals_unfused_f64(call, DEV)


@pytest.mark.parametrize("call", C.REGION_CALLS, ids=ids(C.REGION_CALLS))
def test_regions_overwrite_in_order(call):
    C.check_regions(FX, call, DEV)


@pytest.mark.parametrize("call", C.EXPORT_CALLS, ids=ids(C.EXPORT_CALLS))
def test_segmentation_from_softmax(call):
    C.check_export(FX, call, DEV)


def test_segmentation_from_softmax_numpy():
    C.check_export(FX, C.EXPORT_CALLS[0], DEV, as_numpy=True)


@pytest.mark.parametrize("call", C.PATIENT_CALLS, ids=ids(C.PATIENT_CALLS))
def test_resample_patient(call):
    C.check_patient(FX, call, DEV)


def test_export_postprocess_score_on_the_device():
    C.check_chain(DEV)


def test_argument_errors():
    C.check_errors(DEV)


def test_containers_and_dtypes():
    C.check_containers(FX, DEV)


def test_host_tensor_comes_back_on_the_host():
    from deformablelka_amd import resampling as S
    x = torch.from_numpy(C.make_input("prob", "one_in"))
    out = S.resample_and_argmax(x, (4, 5, 7))
    assert out.device.type == "cpu" and torch.equal(out, S.resample_and_argmax(x.to(DEV), (4, 5, 7)).cpu())
