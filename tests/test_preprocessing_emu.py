"""deformablelka_amd.preprocessing (csrc/cl_preprocess.hip) on the wavefront emulator against the fixture recorded from the reference's own
cropping.py and preprocessing.py (tests/golden/reference_preprocessing.pt), and the scipy / numpy restatement (tests/preprocessing_ref.py)
against that fixture.  The bounds are in tests/preprocessing_cases.py."""
import numpy as np
import pytest
import torch

from tests import preprocessing_cases as C

from deformablelka_amd import preprocessing  # noqa: F401  (the feature: without it nothing here can run)


@pytest.fixture(scope="module", autouse=True)
def emu_backend():
    from deformablelka_amd import _lib
    from tests import emu
    _lib._set_backend_for_tests(emu.load())
    yield
    _lib._set_backend_for_tests(None)


FX = C.load_fixture()


@pytest.mark.parametrize("name", list(C.CROP_CASES))
def test_crop_equals_the_reference(name):
    C.check_crop(name, FX["crop"][name], "cpu")


@pytest.mark.parametrize("call", C.NORM_CALLS, ids=[c[0] for c in C.NORM_CALLS])
def test_normalize_is_held_to_the_reference(call):
    C.check_normalize(call, FX["normalize"][call[0]], "cpu")


@pytest.mark.parametrize("cid", list(C.PIPE_CALLS))
def test_preprocess_arrays_is_held_to_the_reference(cid):
    C.check_pipeline(cid, FX["pipeline"][cid], "cpu")


def test_two_runs_are_bitwise_equal():
    C.check_reproducible(FX, "cpu")


def test_dtypes_and_containers():
    C.check_containers(FX, "cpu")


def test_argument_errors():
    C.check_errors("cpu")


def test_library_refuses_bad_descriptions():
    C.check_c_abi_refuses("cpu")


def test_launches_do_not_depend_on_the_extents():
    C.check_launch_count("cpu")


def test_the_fixture_covers_the_shapes_it_claims():
    crop = FX["crop"]
    shapes = {n: C.CROP_CASES[n]()[0].shape for n in C.CROP_CASES}
    assert shapes["random2"] == (2, 5, 37, 130) and shapes["depth_one"] == (1, 1, 33, 70) and shapes["planar"] == (2, 67, 131)
    assert all(int(np.prod(s[1:])) <= 25000 for s in shapes.values())
    assert not any(e % t == 0 for s in (shapes["random2"], shapes["pocket_closed"]) for e, t in zip(s[1:], (4, 8, 64)))
    data, _ = C.CROP_CASES["random2"]()
    mask, nonzero = crop["random2"]["mask"].numpy().astype(bool), (data != 0).any(0)
    (d0, d1), (h0, h1), (w0, w1) = crop["random2"]["bbox"]
    assert d0 > 0 and h0 > 0 and w0 > 0 and d1 < 5 and h1 < 37 and w1 < 130                          # the box lies strictly inside
    inside = np.zeros_like(mask)
    inside[d0 + 1:d1 - 1, h0 + 1:h1 - 1, w0 + 1:w1 - 1] = True
    assert int((mask & ~nonzero).sum()) == crop["random2"]["filled"] > 47                             # something was filled ...
    assert bool((~mask & inside).any()) and not mask[2, 23, 110]                                      # ... and something was not
    assert mask[2, 7, 60] and nonzero[2, 7, 60] and np.isnan(data[1, 2, 7, 60])                       # the NaN cell is not background
    assert np.isnan(crop["random2"]["crop"]["data"].numpy()).sum() == 1                               # and the public crop keeps it
    assert crop["pocket_leaks"]["filled"] == 0 and crop["depth_one"]["filled"] == 0
    assert crop["pocket_diagonal"]["filled"] == crop["pocket_closed"]["filled"] == C.POCKET_CELLS     # the cavity count, by formula
    assert crop["touches_every_face"]["bbox"] == [[0, 4], [0, 9], [0, 70]] and crop["single_cell"]["bbox"] == [[3, 4], [4, 5], [7, 8]]
    assert len(crop["planar"]["bbox"]) == 2 and crop["planar"]["filled"] > 0 and crop["all_zero"]["raises"] == "ValueError"
    assert crop["with_seg"]["cropper"]["classes"] == [-2, -1, 0, 1, 2, 3] and int(crop["with_seg"]["cropper"]["seg"].min()) == -1
    assert int((crop["with_seg"]["crop_label_m7"]["seg"] == -7).sum()) == int((crop["with_seg"]["crop"]["seg"] == -1).sum()) > 0
    assert all(rec["f64_gap"] <= C.GAP_BOUND for rec in FX["normalize"].values())
    x, seg = C.normalize_input()
    assert abs(float(x[2].mean()) - 1000.0) < 0.1 and 0.8 < float(x[2].std()) < 1.3 and bool((seg == -1).any())
    assert float(x[0].min()) < C.CT_PROPS['percentile_00_5'] and float(x[0].max()) > C.CT_PROPS['percentile_99_5']   # the clip bites
    assert C.PIPE_CALLS["synapse"][1] == (3.0, 0.76, 0.76) and C.PIPE_CALLS["transposed"][3] == [2, 0, 1]
    assert tuple(FX["pipeline"]["synapse"]["data"].shape) != C.PIPE_CALLS["synapse"][0]
    assert int(FX["pipeline"]["two_modalities"]["seg"].min()) == -1


def test_without_a_gpu_host_data_raises_as_the_metrics_do():
    from deformablelka_amd import _lib, preprocessing as P
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: host data is moved to it")
    lib = _lib._lib
    _lib._set_backend_for_tests(None)
    try:
        with pytest.raises(RuntimeError, match="libdlka_hip.so is missing|tensors must live on an AMD GPU"):
            P.create_nonzero_mask(np.ones((1, 2, 2, 2), np.float32))
    finally:
        _lib._set_backend_for_tests(lib)


# ---- the yardstick itself ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in C.CROP_CASES if n != "all_zero"])
def test_restatement_is_held_to_the_fixture(name):
    pytest.importorskip("scipy")
    from tests import preprocessing_ref as R
    rec = FX["crop"][name]
    data, seg = C.CROP_CASES[name]()
    assert np.array_equal(R.create_nonzero_mask(data), rec["mask"].numpy().astype(bool))
    for label, key in ((-1, "crop"), (-7, "crop_label_m7")):
        out, sout, bbox = R.crop_to_nonzero(data, seg, label)
        assert bbox == rec["bbox"] and C.same_bits(out, rec["crop"]["data"].numpy()) and np.array_equal(sout, rec[key]["seg"].numpy())
    out, sout, props = R.crop(data, {}, seg)
    assert np.array_equal(sout, rec["cropper"]["seg"].numpy()) and [int(v) for v in props["classes"]] == rec["cropper"]["classes"]


@pytest.mark.parametrize("call", C.NORM_CALLS, ids=[c[0] for c in C.NORM_CALLS])
def test_normalize_restatement_is_held_to_the_fixture(call):
    from tests import preprocessing_ref as R
    data, seg = C.normalize_input()
    assert C.same_bits(R.normalize(data, seg, call[1], call[2], C.INTENSITY), FX["normalize"][call[0]]["out"].numpy())
