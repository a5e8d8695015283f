"""deformablelka_amd.dataloading (csrc/cl_dataload.hip) on the MI355X against the fixture recorded from the reference's own
DataLoader3D.generate_train_batch and GenericPreprocessor._run_internal (tests/golden/reference_dataloading.pt).  The same cases as the
emulator suite (tests/dataloading_cases.py), the default parameters at a size the emulator is too slow for, and the hand-over from the
preprocessing through the loader and the augmentation to the trainer's (data, target).  Every bound is equality."""
import numpy as np
import pytest
import torch

from tests import dataloading_cases as C

from deformablelka_amd import dataloading  # noqa: F401  (the feature: without it nothing here can run)

pytestmark = pytest.mark.gpu
DEV = "cuda"
FX = C.load_fixture()


@pytest.mark.parametrize("cid", list(C.LOADER_CALLS))
def test_batches_equal_the_reference(cid):
    C.check_draws(cid, FX["loader"][cid])
    C.check_loader(cid, FX["loader"][cid], DEV)


@pytest.mark.parametrize("name", list(C.CROP_CASES))
def test_crop_equals_the_restatement(name):
    C.check_crop(name, DEV)


def test_seg_pads_with_minus_one_and_data_with_the_constant():
    C.check_seg_padding(DEV)


def test_a_batch_beyond_the_kernel_s_table_is_cut_into_chunks():
    C.check_chunking(DEV)


@pytest.mark.parametrize("name", list(C.CL_CASES))
def test_class_locations_equal_the_reference(name):
    C.check_class_locations(name, FX["class_locations"][name], DEV)


def test_two_runs_are_bitwise_equal():
    C.check_reproducible(DEV)


def test_launches_do_not_depend_on_batch_channels_classes_or_extents():
    C.check_launch_count(DEV)


def test_dtypes_and_containers():
    C.check_containers(FX, DEV)


def test_argument_errors():
    C.check_errors(DEV)


def test_library_refuses_bad_descriptions():
    C.check_c_abi_refuses(DEV)


def test_default_parameters_on_a_million_cells_by_formula():
    """104 x 100 x 100 = 1 040 000 cells, class 1 everywhere but on every 97th cell (class 2) and every 89th (-1): about 1 017 700 cells of
    class 1, so the target is ceil(0.01 n) > 10 000 rows, the 1 % branch at the default num_samples.  Against torch.nonzero of the same map
    and numpy's RandomState(1234), consumed in the order of all_classes."""
    from deformablelka_amd import dataloading as D
    i = torch.arange(104 * 100 * 100, dtype=torch.int64)
    seg = torch.ones(i.shape, dtype=torch.float32)
    seg[i % 97 == 0] = 2.0
    seg[i % 89 == 0] = -1.0
    seg = seg.reshape(104, 100, 100).to(DEV)
    got = D.class_locations(seg, [1, 2, 3])
    rndst = np.random.RandomState(1234)
    for c in (1, 2):
        locs = torch.nonzero(seg == c).cpu().numpy()
        target = max(min(10000, len(locs)), int(np.ceil(len(locs) * 0.01)))
        want = locs[rndst.choice(len(locs), target, replace=False)]
        assert got[c].dtype == np.int64 and np.array_equal(got[c], want), c
    n1 = int((seg == 1).sum())
    assert len(got[1]) == int(np.ceil(0.01 * n1)) > 10000 and len(got[2]) == 10000 < int((seg == 2).sum()) and got[3] == []


def test_from_preprocessing_to_the_trainer_s_batch_on_the_device(monkeypatch):
    """preprocess_arrays(..., all_classes=...) -> DataLoader3D(device=...) -> training.augmented_batches with MoreDAAugmentation ->
    (data, target) on the device with the trainer's shapes, two batches, and no tensor of a batch visits the host."""
    from deformablelka_amd import augmentation as A, dataloading as D, preprocessing as P, training
    from tests import augmentation_cases as AC
    from tests import preprocessing_cases as PC
    final = AC.PIPE_PATCH
    params = AC.pipeline_params()
    dataset = {}
    for n, cid in enumerate(("synapse", "transposed")):
        shape, original, target, tf, schemes, use_mask, _ = PC.PIPE_CALLS[cid]
        data, _ = PC.pipeline_input(cid)
        seg = np.floor(PC.noise((1,) + shape[1:], 95 + n) * 3.0).astype(np.float32)
        pre = PC.preprocessor(P, tf, schemes, use_mask, {c: PC.CT_PROPS for c in range(len(schemes))})
        out, sout, props = pre.preprocess_arrays(torch.from_numpy(data).to(DEV), target, {"original_spacing": np.array(original)},
                                                 torch.from_numpy(seg).to(DEV), all_classes=[1, 2])
        assert out.is_cuda and sout.is_cuda and set(props["class_locations"]) == {1, 2} and len(props["class_locations"][1]) > 0
        dataset[cid] = {"data": torch.cat((out, sout.to(torch.float32)), 0), "properties": props}
    patch = D.get_patch_size(final, params["rotation_x"], params["rotation_y"], params["rotation_z"], params["scale_range"])
    assert patch.tolist() == [18, 21, 18]
    loader = D.DataLoader3D(dataset, patch, final, 2, False, 0.33, "r", "constant", {"constant_values": 0}, device=DEV, seed=5)
    aug = A.MoreDAAugmentation(final, params, deep_supervision_scales=AC.DS_SCALES, seed=3)

    visits = []
    real_cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (visits.append(tuple(self.shape)), real_cpu(self, *a, **k))[1])
    batches = []
    for n, (d, t) in enumerate(training.augmented_batches(loader, aug)):
        batches.append((d, t))
        if n == 1:
            break
    monkeypatch.undo()
    assert not [s for s in visits if len(s) >= 3], visits                                     # nothing of a batch was read back
    assert loader.last_draw["force_fg"].tolist() == [False, True]
    for d, t in batches:
        assert d.is_cuda and d.dtype == torch.float32 and tuple(d.shape) == (2, 1) + final
        assert isinstance(t, list) and len(t) == 3 and all(v.is_cuda and v.dtype == torch.float32 for v in t)
        assert tuple(t[0].shape) == (2, 1) + final and float(t[0].min()) >= 0.0               # -1 removed by the chain
