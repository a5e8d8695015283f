"""deformablelka_amd.dataset_analysis (csrc/cl_dataset_stats.hip) on the wavefront emulator against the fixture recorded from the reference's
own DatasetAnalyzer (tests/golden/reference_dataset_analysis.pt) and against numpy on the same samples, and the numpy restatement
(tests/dataset_analysis_ref.py) against that fixture.  The cases and the bounds are in tests/dataset_analysis_cases.py."""
import os

import numpy as np
import pytest

from tests import dataset_analysis_cases as C

from deformablelka_amd import dataset_analysis  # noqa: F401  (the feature: without it nothing here can run)


@pytest.fixture(scope="module", autouse=True)
def emu_backend():
    from deformablelka_amd import _lib
    from tests import emu
    _lib._set_backend_for_tests(emu.load())
    yield
    _lib._set_backend_for_tests(None)


FX = C.load_fixture()


@pytest.mark.parametrize("name", list(C.FG_CASES))
def test_foreground_sample_equals_numpy(name):
    C.check_foreground(name, FX["foreground"][name], "cpu")


@pytest.mark.parametrize("name", list(C.STAT_CASES))
def test_stats_equal_numpy_and_the_reference(name):
    C.check_stats(name, FX["stats"][name], "cpu")


@pytest.mark.parametrize("name", list(C.STAT_CASES))
def test_order_statistics_equal_partition(name):
    C.check_order_statistics(name, "cpu")


@pytest.mark.parametrize("name", C.DATASETS)
def test_dataset_properties_equal_the_reference(name):
    C.check_dataset(name, FX["datasets"][name], "cpu")


def test_analyze_dataset_has_the_reference_s_structure():
    C.check_analyze_dataset(FX["datasets"]["three"]["analyze"], "cpu")


def test_intensityproperties_go_unchanged_into_the_preprocessor():
    C.check_chain(FX, "cpu")


@pytest.mark.parametrize("name", list(C.region_maps()))
def test_classes_and_regions_equal_the_reference(name):
    C.check_regions(name, FX["regions"][name], "cpu")


def test_nans_in_and_outside_the_foreground():
    C.check_nans("cpu")


def test_two_runs_are_bitwise_equal():
    C.check_reproducible("cpu")


def test_containers_and_files():
    C.check_containers("cpu")


def test_launches_do_not_depend_on_extents_or_foreground():
    C.check_launch_count("cpu")


def test_argument_errors():
    C.check_errors("cpu")


def test_library_refuses_bad_descriptions():
    C.check_c_abi_refuses("cpu")


def test_interpolation_restates_numpy():
    C.check_interpolation_restates_numpy()


def test_the_fixture_covers_what_it_claims():
    assert os.path.getsize(C.FIXTURE) < 2 ** 18
    C.check_quantile_weights()
    assert FX["datasets"]["three"]["sizes"] == [7, 130, 1001] and FX["datasets"]["empty_middle"]["sizes"] == [7, 0, 130]
    assert FX["empty"]["n"] == 0 and bool(np.isnan(FX["empty"]["stats32"].numpy()).all())
    assert [FX["foreground"][f"count{c}_3x5x70"]["count"] for c in C.COUNTS] == list(C.COUNTS)
    assert FX["datasets"]["three"]["analyze"]["keys"] == ["all_sizes", "all_spacings", "all_classes", "modalities", "intensityproperties",
                                                          "size_reductions"]


# ---- the yardstick itself ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.STAT_CASES))
def test_restatement_is_held_to_the_fixture(name):
    from tests import dataset_analysis_ref as R
    ref = FX["stats"][name]["stats32"].numpy()
    assert all(C.same_value(a, b) for a, b in zip(R.compute_stats(C.STAT_CASES[name]()), ref))


@pytest.mark.parametrize("name", C.DATASETS)
def test_dataset_restatement_is_held_to_the_fixture(name):
    from tests import dataset_analysis_ref as R
    got, rec = R.collect_intensity_properties(C.dataset(name), 2), FX["datasets"][name]
    assert C.describe(got) == rec["structure"]
    for mod in (0, 1):
        assert all(C.same_value(np.float32(got[mod][k]), r) for k, r in zip(C.KEYS, rec["whole"][mod]["stats32"].numpy()))
