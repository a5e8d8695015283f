"""deformablelka_amd.dataset_analysis (csrc/cl_dataset_stats.hip) on the MI355X against the fixture recorded from the reference's own
DatasetAnalyzer (tests/golden/reference_dataset_analysis.pt) and against numpy on the same samples: the same cases as the emulator suite
(tests/dataset_analysis_cases.py), and two volumes of 983 040 cells whose every statistic is known by formula."""
import numpy as np
import pytest
import torch

from tests import dataset_analysis_cases as C

from deformablelka_amd import dataset_analysis  # noqa: F401  (the feature: without it nothing here can run)

pytestmark = pytest.mark.gpu
DEV = "cuda"
FX = C.load_fixture()


@pytest.mark.parametrize("name", list(C.FG_CASES))
def test_foreground_sample_equals_numpy(name):
    C.check_foreground(name, FX["foreground"][name], DEV)


@pytest.mark.parametrize("name", list(C.STAT_CASES))
def test_stats_equal_numpy_and_the_reference(name):
    C.check_stats(name, FX["stats"][name], DEV)


@pytest.mark.parametrize("name", list(C.STAT_CASES))
def test_order_statistics_equal_partition(name):
    C.check_order_statistics(name, DEV)


@pytest.mark.parametrize("name", C.DATASETS)
def test_dataset_properties_equal_the_reference(name):
    C.check_dataset(name, FX["datasets"][name], DEV)
    C.check_dataset(name, FX["datasets"][name], DEV, as_numpy=True)


def test_analyze_dataset_has_the_reference_s_structure():
    C.check_analyze_dataset(FX["datasets"]["three"]["analyze"], DEV)


def test_intensityproperties_go_unchanged_into_the_preprocessor():
    C.check_chain(FX, DEV)


@pytest.mark.parametrize("name", list(C.region_maps()))
def test_classes_and_regions_equal_the_reference(name):
    C.check_regions(name, FX["regions"][name], DEV)


def test_nans_in_and_outside_the_foreground():
    C.check_nans(DEV)


def test_two_runs_are_bitwise_equal():
    C.check_reproducible(DEV)


def test_containers_and_files():
    C.check_containers(DEV)


def test_launches_do_not_depend_on_extents_or_foreground():
    C.check_launch_count(DEV)


def test_argument_errors():
    C.check_errors(DEV)


def test_library_refuses_bad_descriptions():
    C.check_c_abi_refuses(DEV)


@pytest.mark.parametrize("every", (1, 3))
def test_a_million_cells_by_formula(every):
    """x = raster index over 1 x 64 x 96 x 160 = 983 040 cells, exact in float32.  seg = 1 everywhere: the sample is 0, 10, 20, ...,
    n = 98 304.  seg = (i % 3 == 0): the foreground is 0, 3, 6, ... (327 680 cells) and the sample 0, 30, 60, ..., n = 32 768.  Every
    statistic comes from numpy on that arange; mean and sd within STAT_BOUND (|m64| + s64) of its float64 values."""
    from deformablelka_amd import dataset_analysis as A
    cells = 64 * 96 * 160
    i = torch.arange(cells, dtype=torch.int64)
    case = torch.stack([i.to(torch.float32), (i % every == 0).to(torch.float32)]).reshape(2, 64, 96, 160).to(DEV)
    want = np.arange(0, cells, 10 * every).astype(np.float32)
    assert len(want) == {1: 98304, 3: 32768}[every]
    got = A.foreground_voxels(case, 0)
    assert C.same_bits(C.to_np(got), want)
    ours = A.collect_intensity_properties({"formula": case}, 1)[0]
    stats = tuple(ours[k] for k in C.KEYS)
    assert stats == tuple(ours['local_props']["formula"][k] for k in C.KEYS)
    ref = (np.median(want), np.mean(want), np.std(want), np.min(want), np.max(want), np.percentile(want, 99.5), np.percentile(want, 0.5))
    for k in (0, 3, 4, 5, 6):
        assert C.same_value(stats[k], ref[k]), (C.KEYS[k], stats[k], ref[k])
    m64, s64 = float(np.mean(want.astype(np.float64))), float(np.std(want.astype(np.float64)))
    step = 10.0 * every
    assert m64 == step * (len(want) - 1) / 2 and abs(s64 - step * np.sqrt((len(want) ** 2 - 1) / 12.0)) <= 1e-9 * s64      # the closed forms
    tol = C.STAT_BOUND * (abs(m64) + s64)
    print(f"every {every}: |mean - m64| {abs(stats[1] - m64):.3e}, |sd - s64| {abs(stats[2] - s64):.3e}, bound {tol:.3e}")
    assert abs(stats[1] - m64) <= tol and abs(stats[2] - s64) <= tol
    ranks = [0, 1, 491, 492, len(want) // 2, len(want) - 2, len(want) - 1]
    assert C.same_bits(C.to_np(A.order_statistics(got, ranks)), want[ranks])
