"""deformablelka_amd.postprocessing (csrc/cl_conn_comp.hip) on the wavefront emulator against the fixture recorded from the reference's own
remove_all_but_the_largest_connected_component and scipy.ndimage.label (tests/golden/reference_postprocessing.pt), and the scipy restatement
(tests/postprocessing_ref.py) against that fixture.  Every comparison is equality: tests/postprocessing_cases.py."""
import numpy as np
import pytest
import torch

from tests import postprocessing_cases as C

from deformablelka_amd import postprocessing  # noqa: F401  (the feature: without it nothing here can run)


@pytest.fixture(scope="module", autouse=True)
def emu_backend():
    from deformablelka_amd import _lib
    from tests import emu
    _lib._set_backend_for_tests(emu.load())
    yield
    _lib._set_backend_for_tests(None)


FX = C.load_fixture()
CASES = list(FX["cases"].keys())


@pytest.mark.parametrize("name", CASES)
def test_label_equals_scipy(name):
    C.check_label(name, FX["cases"][name], "cpu")


@pytest.mark.parametrize("name", CASES)
def test_remove_equals_the_reference(name):
    C.check_remove(name, FX["cases"][name], "cpu")


def test_connectivity_changes_the_objects():
    C.check_connectivity_counts(FX, "cpu")


def test_serpentine_is_one_object_per_class():
    C.check_serpentine(FX, "cpu")


def test_numbering_follows_the_first_cell():
    C.check_late_join(FX, "cpu")


def test_every_object_of_the_largest_size_is_kept():
    C.check_ties(FX, "cpu")


def test_the_fixture_covers_the_shapes_it_claims():
    shapes = {n: tuple(c["image"].shape) for n, c in FX["cases"].items()}
    assert shapes["random"] == (5, 37, 130) and shapes["serpentine"] == (2, 33, 129) and shapes["line_513"] == (513,)
    assert shapes["image_67x131"] == (67, 131) and shapes["width_one"][2] == 1 and shapes["single_cell"] == (1,)
    assert shapes["long_line_150"] == (1, 3, 150) and shapes["long_line_4500"] == (4500,)       # 150 > 64, 4500 > 2048: the tiles' spans along w
    assert not FX["cases"]["all_background"]["image"].any() and bool((FX["cases"]["class_fills_the_array"]["image"] == 2).all())
    first = FX["cases"]["random"]["remove"][0]
    assert first["classes"] == [(1, 2), 3, 2] and first["vpv"] == 0.75 * 0.75 * 3.0 and first["min"] == {(1, 2): 40.0, 3: 10.0, 2: 5.0}
    image, out = FX["cases"]["random"]["image"], first["image"]
    assert 0 < int((out != image).sum()) < int((image != 0).sum())                             # objects were removed ...
    small = FX["cases"]["random"]["remove"][1]["image"]
    assert int((small != 0).sum()) < int((out != 0).sum())                                      # ... and small ones kept that no minimum would keep
    absent = FX["cases"]["ties"]["remove"][1]
    assert absent["kept_size"][7] is None and absent["largest_removed"][7] is None              # a class that does not occur
    assert max(c["image"].numel() for c in FX["cases"].values()) <= 25000


def test_dtypes_and_containers():
    C.check_dtypes(FX, "cpu")


def test_more_entries_than_one_pass_takes():
    C.check_chunking(FX, "cpu")


def test_argument_errors():
    C.check_errors("cpu")


def test_library_refuses_bad_descriptions():
    C.check_c_abi_refuses("cpu")


def test_two_runs_are_bitwise_equal():
    C.check_reproducible(FX, "cpu")


def test_launches_of_one_call():
    C.check_launch_count(FX, "cpu")


def test_minimum_size_becomes_the_count_that_compares_alike():
    """count < T  <=>  float64(count) * vpv < minimum, for products that round."""
    from deformablelka_amd.postprocessing import _min_count
    rng = np.random.default_rng(5)
    for vpv in (0.75 * 0.75 * 3.0, 0.1, 1.0 / 3.0, 1e-3, 7.0, 0.6999999):
        for m in list(rng.random(40) * 50.0) + [vpv * k for k in range(0, 12)] + [np.float64(k) * vpv for k in (3, 7, 10, 33)]:
            t = _min_count(m, vpv)
            for count in range(max(0, t - 3), t + 4):
                assert (count < t) == bool(np.float64(count) * vpv < m), (vpv, m, count, t)
    assert _min_count(0.0, 1.0) == 0 and _min_count(-1.0, 1.0) == 0 and _min_count(float("inf"), 1.0) == 2 ** 31 - 1


def test_without_a_gpu_host_data_raises_as_the_metrics_do():
    from deformablelka_amd import _lib, postprocessing as P
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: host data is moved to it")
    lib = _lib._lib
    _lib._set_backend_for_tests(None)
    try:
        with pytest.raises(RuntimeError, match="libdlka_hip.so is missing|tensors must live on an AMD GPU"):
            P.label(np.ones((2, 2), np.uint8))
    finally:
        _lib._set_backend_for_tests(lib)


# ---- the yardstick itself ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_restatement_is_held_to_the_fixture(name):
    pytest.importorskip("scipy")
    from tests import postprocessing_ref as R
    case = FX["cases"][name]
    image = case["image"].numpy()
    for cn, want in case["label"].items():
        lmap, n = R.label(image, cn)
        assert n == want["num"] and np.array_equal(lmap, want["labels"].numpy())
    for call in case["remove"]:
        out, removed, kept = R.remove_all_but_the_largest_connected_component(image, call["classes"], call["vpv"], call["min"])
        assert np.array_equal(out, call["image"].numpy()) and removed == call["largest_removed"] and kept == call["kept_size"]
