"""deformablelka_amd.metrics (csrc/cl_surface_dist.hip) on the wavefront emulator against the fixture recorded from MedPy 0.4.0's definitions
restated with scipy (tests/golden/reference_metrics.pt), and that restatement (tests/metrics_ref.py) against the fixture.  Tolerances:
tests/metrics_cases.py.  Reached on the emulator: distances, hd and hd95 equal with unit spacing, asd / assd <= 3e-16; with a spacing <= 3e-16."""
import numpy as np
import pytest
import torch

from tests import metrics_cases as C

from deformablelka_amd import metrics  # noqa: F401  (the feature: without it nothing here can run)


@pytest.fixture(scope="module", autouse=True)
def emu_backend():
    from deformablelka_amd import _lib
    from tests import emu
    _lib._set_backend_for_tests(emu.load())
    yield
    _lib._set_backend_for_tests(None)


FX = C.load_fixture()
PAIRS = list(FX["pairs"].keys())


@pytest.mark.parametrize("name", PAIRS)
def test_pair_case(name):
    C.check_pair(name, FX["pairs"][name], "cpu")


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16, torch.int32, torch.int64], ids=["u8", "i16", "i32", "i64"])
@pytest.mark.parametrize("name", list(FX["labels"].keys()))
def test_label_maps(name, dtype):
    C.check_labels(name, FX["labels"][name], "cpu", dtype)


def test_rank_is_honoured():
    C.check_rank_is_honoured(FX, "cpu")


def test_percentile_interpolates_on_a_line_longer_than_512():
    from deformablelka_amd import metrics as M
    case = FX["pairs"]["percentile_long_line"]
    assert tuple(case["p"].shape) == (3, 5, 513) and case["conn"][1]["hd95"] == C.PERCENTILE_HD95
    assert abs(M.hd95(case["p"], case["q"]) - C.PERCENTILE_HD95) <= 1e-12 * C.PERCENTILE_HD95
    assert M.hd(case["p"], case["q"]) == 512.0


def test_connectivity_changes_the_border():
    from deformablelka_amd import metrics as M
    case = FX["pairs"]["diagonals"]
    assert len(set(C.DIAGONALS_HD95.values())) == 3
    for cn, want in C.DIAGONALS_HD95.items():
        assert case["conn"][cn]["hd95"] == want
        assert abs(M.hd95(case["p"], case["q"], connectivity=cn) - want) <= 1e-12 * want


def test_quirks():
    C.check_quirks("cpu")


def test_argument_errors():
    C.check_errors("cpu")


def test_library_refuses_bad_descriptions():
    C.check_c_abi_refuses("cpu")


def test_two_runs_are_bitwise_equal(monkeypatch):
    C.check_reproducible(FX, "cpu")


def test_numpy_inputs_and_mixed_dtypes():
    from deformablelka_amd import metrics as M
    case = FX["pairs"]["below_one_wave"]
    p, q = case["p"].numpy().astype(bool), case["q"].numpy().astype(np.int32) * 5
    assert M.hd95(p, q) == M.hd95(case["p"], case["q"]) and M.dc(p, q) == case["dc"]
    lab = FX["labels"]["synapse_unit"]
    a = M.evaluate_label_maps(lab["prediction"].numpy(), lab["label"].long(), lab["classes"])
    b = M.evaluate_label_maps(lab["prediction"].float(), lab["label"].numpy().astype(np.uint16), lab["classes"])
    assert a["hd95"].tobytes() == b["hd95"].tobytes() and a["dice"].tobytes() == b["dice"].tobytes()


def test_more_classes_than_one_call_takes():
    from deformablelka_amd import metrics as M
    lab = FX["labels"]["synapse_unit"]
    classes = list(range(1, 41))
    many = M.evaluate_label_maps(lab["prediction"], lab["label"], classes)
    few = M.evaluate_label_maps(lab["prediction"], lab["label"], lab["classes"])
    for i, c in enumerate(lab["classes"]):
        assert many["hd95"][classes.index(c)] == few["hd95"][i] and many["dice"][classes.index(c)] == few["dice"][i]


def test_without_a_gpu_host_tensors_raise_as_the_losses_do():
    from deformablelka_amd import _lib, metrics as M
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: host data is moved to it")
    lib = _lib._lib
    _lib._set_backend_for_tests(None)
    try:
        with pytest.raises(RuntimeError, match="libdlka_hip.so is missing|tensors must live on an AMD GPU"):
            M.dc(np.ones((2, 2), np.uint8), np.ones((2, 2), np.uint8))
    finally:
        _lib._set_backend_for_tests(lib)


# ---- the yardstick itself ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PAIRS)
def test_restatement_is_held_to_the_fixture(name):
    pytest.importorskip("scipy")
    from tests import metrics_ref as R
    case = FX["pairs"][name]
    p, q, sp = case["p"].numpy(), case["q"].numpy(), case["spacing"]
    assert R.dc(p, q) == case["dc"]
    for cn, r in case["conn"].items():
        ab, ba = np.sort(R.surface_distances(p, q, sp, cn)), np.sort(R.surface_distances(q, p, sp, cn))
        if sp is None:
            assert np.array_equal(ab, np.sqrt(r["sq_ab"].numpy().astype(np.float64))) and np.array_equal(ba, np.sqrt(r["sq_ba"].numpy().astype(np.float64)))
        else:
            assert np.array_equal(ab, r["sds_ab"].numpy()) and np.array_equal(ba, r["sds_ba"].numpy())
        assert (R.hd(p, q, sp, cn), R.hd95(p, q, sp, cn), R.asd(p, q, sp, cn), R.assd(p, q, sp, cn)) == (r["hd"], r["hd95"], r["asd"], r["assd"])


def test_restatement_on_label_maps_and_cropping_is_exact():
    """The fixture's per-class rows, and the cropping argument of DESIGN.md on the host: the distances inside the joint bounding box equal those of
    the whole array."""
    pytest.importorskip("scipy")
    from tests import metrics_ref as R
    for case in FX["labels"].values():
        pred, lab = case["prediction"].numpy(), case["label"].numpy()
        for c, row in case["rows"].items():
            a, b = pred == c, lab == c
            assert (int(a.sum()), int(b.sum()), int((a & b).sum())) == (row["a"], row["b"], row["inter"])
            if row["hd95"] is None:
                continue
            assert R.hd95(a, b, case["spacing"], 1) == row["hd95"]
            idx = np.argwhere(a | b)
            box = tuple(slice(lo, hi + 1) for lo, hi in zip(idx.min(0), idx.max(0)))
            assert np.array_equal(R.surface_distances(a, b, case["spacing"], 1), R.surface_distances(a[box], b[box], case["spacing"], 1))
