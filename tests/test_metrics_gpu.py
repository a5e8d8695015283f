"""deformablelka_amd.metrics (csrc/cl_surface_dist.hip) on the MI355X against the fixture recorded from MedPy 0.4.0's definitions restated with
scipy (tests/golden/reference_metrics.pt; scipy is not needed here).  The same cases and tolerances as the emulator suite: tests/metrics_cases.py."""
import numpy as np
import pytest
import torch

from tests import metrics_cases as C

from deformablelka_amd import metrics  # noqa: F401  (the feature: without it nothing here can run)

pytestmark = pytest.mark.gpu
DEV = "cuda"
FX = C.load_fixture()
PAIRS = list(FX["pairs"].keys())


@pytest.mark.parametrize("name", PAIRS)
def test_pair_case(name):
    C.check_pair(name, FX["pairs"][name], DEV)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64], ids=["u8", "i64"])
@pytest.mark.parametrize("name", list(FX["labels"].keys()))
def test_label_maps(name, dtype):
    C.check_labels(name, FX["labels"][name], DEV, dtype)


def test_label_maps_narrow_integers():
    C.check_labels("synapse_unit", FX["labels"]["synapse_unit"], DEV, torch.int16)
    C.check_labels("synapse_unit", FX["labels"]["synapse_unit"], DEV, torch.int32)


def test_rank_is_honoured():
    C.check_rank_is_honoured(FX, DEV)


def test_percentile_interpolates_on_a_line_longer_than_512():
    from deformablelka_amd import metrics as M
    case = FX["pairs"]["percentile_long_line"]
    assert abs(M.hd95(case["p"].to(DEV), case["q"].to(DEV)) - C.PERCENTILE_HD95) <= 1e-12 * C.PERCENTILE_HD95
    assert M.hd(case["p"].to(DEV), case["q"].to(DEV)) == 512.0


def test_connectivity_changes_the_border():
    from deformablelka_amd import metrics as M
    case = FX["pairs"]["diagonals"]
    for cn, want in C.DIAGONALS_HD95.items():
        assert abs(M.hd95(case["p"].to(DEV), case["q"].to(DEV), connectivity=cn) - want) <= 1e-12 * want


def test_quirks():
    C.check_quirks(DEV)


def test_argument_errors():
    C.check_errors(DEV)


def test_library_refuses_bad_descriptions():
    C.check_c_abi_refuses(DEV)


def test_two_runs_are_bitwise_equal():
    C.check_reproducible(FX, DEV)


def test_host_inputs_are_moved_to_the_device():
    from deformablelka_amd import metrics as M, ops
    case = FX["pairs"]["below_one_wave"]
    before = ops.sd_launch_count()
    h = M.hd95(case["p"].numpy().astype(bool), case["q"])          # numpy and a host tensor
    assert ops.sd_launch_count() == before + 5
    assert h == M.hd95(case["p"].to(DEV), case["q"].to(DEV)) and abs(h - case["conn"][1]["hd95"]) <= 1e-12 * h
    lab = FX["labels"]["synapse_unit"]
    a = M.evaluate_label_maps(lab["prediction"].numpy(), lab["label"].long(), lab["classes"])
    b = M.evaluate_label_maps(lab["prediction"].to(DEV), lab["label"].to(DEV), lab["classes"])
    assert a["hd95"].tobytes() == b["hd95"].tobytes() and isinstance(a["dice"], np.ndarray)
