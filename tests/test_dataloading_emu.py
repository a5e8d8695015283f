"""deformablelka_amd.dataloading (csrc/cl_dataload.hip) on the wavefront emulator against the fixture recorded from the reference's own
DataLoader3D.generate_train_batch and GenericPreprocessor._run_internal (tests/golden/reference_dataloading.pt), and the numpy restatement
(tests/dataloading_ref.py) against that fixture.  Every bound is equality; the cases are in tests/dataloading_cases.py."""
import os

import numpy as np
import pytest
import torch

from tests import dataloading_cases as C

from deformablelka_amd import dataloading  # noqa: F401  (the feature: without it nothing here can run)


@pytest.fixture(scope="module", autouse=True)
def emu_backend():
    from deformablelka_amd import _lib
    from tests import emu
    _lib._set_backend_for_tests(emu.load())
    yield
    _lib._set_backend_for_tests(None)


FX = C.load_fixture()


@pytest.mark.parametrize("cid", list(C.LOADER_CALLS))
def test_draws_are_the_reference_s(cid):
    C.check_draws(cid, FX["loader"][cid])


@pytest.mark.parametrize("cid", list(C.LOADER_CALLS))
def test_batches_equal_the_reference(cid):
    C.check_loader(cid, FX["loader"][cid], "cpu")


@pytest.mark.parametrize("name", list(C.CROP_CASES))
def test_crop_equals_the_restatement(name):
    C.check_crop(name, "cpu")


def test_seg_pads_with_minus_one_and_data_with_the_constant():
    C.check_seg_padding("cpu")


def test_a_batch_beyond_the_kernel_s_table_is_cut_into_chunks():
    C.check_chunking("cpu")


@pytest.mark.parametrize("name", list(C.CL_CASES))
def test_class_locations_equal_the_reference(name):
    C.check_class_locations(name, FX["class_locations"][name], "cpu")


def test_two_runs_are_bitwise_equal():
    C.check_reproducible("cpu")


def test_launches_do_not_depend_on_batch_channels_classes_or_extents():
    C.check_launch_count("cpu")


def test_dtypes_and_containers():
    C.check_containers(FX, "cpu")


def test_argument_errors():
    C.check_errors("cpu")


def test_library_refuses_bad_descriptions():
    C.check_c_abi_refuses("cpu")


def test_get_patch_size_is_the_reference_s():
    C.check_patch_size(FX)


def test_preprocess_arrays_records_class_locations():
    """all_classes= adds class_locations of the returned seg's last channel; without it the properties are as before."""
    from deformablelka_amd import preprocessing as P
    from tests import dataloading_ref as R
    from tests import preprocessing_cases as PC
    shape, original, target, tf, schemes, use_mask, _ = PC.PIPE_CALLS["two_modalities"]
    data, seg = PC.pipeline_input("two_modalities")
    pre = PC.preprocessor(P, tf, schemes, use_mask, {c: PC.CT_PROPS for c in range(len(schemes))})
    props = {"original_spacing": np.array(original)}
    out, sout, got = pre.preprocess_arrays(torch.from_numpy(data), target, props, torch.from_numpy(seg), all_classes=[1, 2, 7])
    out0, sout0, got0 = pre.preprocess_arrays(torch.from_numpy(data), target, props, torch.from_numpy(seg))
    assert "class_locations" not in got0 and "class_locations" not in props and set(got) == set(got0) | {"class_locations"}
    assert torch.equal(sout, sout0) and PC.same_bits(out.numpy(), out0.numpy())
    C._assert_locations(got["class_locations"], R.class_locations(sout.numpy()[-1], [1, 2, 7]), "preprocess_arrays")
    assert got["class_locations"][7] == [] and len(got["class_locations"][1]) > 0
    with pytest.raises(NotImplementedError, match="worker pool"):
        pre._run_internal


def test_the_fixture_covers_what_it_claims():
    assert os.path.getsize(C.FIXTURE) < 2 ** 20
    C.check_crop_properties()
    C.check_class_location_properties(FX)
    a, c = FX["loader"]["aliasing"]["batches"], FX["loader"]["constant2"]["batches"]
    assert len(a) == 3 and a[0]["keys"][0] == "small" and a[0]["need_to_pad"] == [1, 3, 0]      # enlarged by the first sample, for good
    assert all(b["force_fg"] == [False, False, True] for b in a + c)                              # round(3 * 0.67) = 2
    forced = [(b["keys"][2], b["selected_class"][2], b["bbox_lb"][2], b["selected_voxel"][2]) for b in c]
    assert any(k == "nofg" and cls == -1 and v == [-1, -1, -1] for k, cls, _, v in forced)        # no foreground: a random box
    past = [lb for k, cls, lb, _ in forced if k == "corner"]
    assert past and all(lb[d] + C.PATCH[d] > e for lb in past for d, e in enumerate((11, 13, 17)))   # not clamped from above: the patch pads


# ---- the yardstick itself ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(C.LOADER_CALLS))
def test_restatement_is_held_to_the_fixture(cid):
    from tests import dataloading_ref as R
    rec = FX["loader"][cid]
    data, (patch, final, B, p, mode, kwargs, seed, batches) = C.loader_inputs(cid)
    cases = {k: (v["data"].shape[1:], v["properties"]) for k, v in data.items()}
    rs, need = np.random.RandomState(seed), (np.array(patch) - np.array(final)).astype(int)
    for n in range(batches):
        keys, boxes = R.draw_boxes(rs, cases, patch, need, B, p)
        assert [str(k) for k in keys] == rec["batches"][n]["keys"] and boxes.tolist() == rec["batches"][n]["bbox_lb"]
        d, s = R.crop_batch([data[k]["data"] for k in keys], boxes, patch, mode, kwargs)
        assert C.digest(d) == rec["batches"][n]["data"] and C.digest(s) == rec["batches"][n]["seg"]


@pytest.mark.parametrize("name", list(C.CL_CASES))
def test_class_locations_restatement_is_held_to_the_fixture(name):
    from tests import dataloading_ref as R
    seg, classes = C.CL_CASES[name]()
    rec = FX["class_locations"][name]
    assert C.locations_digest(R.class_locations(seg, classes)) == {int(c): tuple(v) for c, v in rec["default"].items()}
    assert C.locations_digest(R.class_locations(seg, classes, **C.CL_SMALL)) == {int(c): tuple(v) for c, v in rec["small"].items()}
