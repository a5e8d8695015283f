"""deformablelka_amd.preprocessing (csrc/cl_preprocess.hip) on the MI355X against the fixture recorded from the reference's own cropping.py and
preprocessing.py (tests/golden/reference_preprocessing.pt; scipy is not needed here).  The same cases as the emulator suite
(tests/preprocessing_cases.py), and two built by formula at sizes the emulator is too slow for."""
import numpy as np
import pytest
import torch

from tests import preprocessing_cases as C

from deformablelka_amd import preprocessing  # noqa: F401  (the feature: without it nothing here can run)

pytestmark = pytest.mark.gpu
DEV = "cuda"
FX = C.load_fixture()


@pytest.mark.parametrize("name", list(C.CROP_CASES))
def test_crop_equals_the_reference(name):
    C.check_crop(name, FX["crop"][name], DEV)


@pytest.mark.parametrize("call", C.NORM_CALLS, ids=[c[0] for c in C.NORM_CALLS])
def test_normalize_is_held_to_the_reference(call):
    C.check_normalize(call, FX["normalize"][call[0]], DEV)


@pytest.mark.parametrize("cid", list(C.PIPE_CALLS))
def test_preprocess_arrays_is_held_to_the_reference(cid):
    C.check_pipeline(cid, FX["pipeline"][cid], DEV)


def test_two_runs_are_bitwise_equal():
    C.check_reproducible(FX, DEV)


def test_dtypes_and_containers():
    C.check_containers(FX, DEV)


def test_argument_errors():
    C.check_errors(DEV)


def test_library_refuses_bad_descriptions():
    C.check_c_abi_refuses(DEV)


def test_launches_do_not_depend_on_the_extents():
    C.check_launch_count(DEV)


def _shell(corridor):
    """A one-cell-thick hollow shell, inset 3 cells from every face of 64 x 96 x 160; optionally a zero-valued one-cell corridor from the cavity
    through the shell and the margin to the face w = 159."""
    D, H, W = 64, 96, 160
    x = torch.zeros((1, D, H, W), dtype=torch.float32)
    x[0, 3:D - 3, 3:H - 3, 3:W - 3] = 2.0
    x[0, 4:D - 4, 4:H - 4, 4:W - 4] = 0.0
    if corridor:
        x[0, D // 2, H // 2, W - 4:] = 0.0
    return x, (D, H, W)


def test_a_sealed_shell_is_filled_by_formula():
    from deformablelka_amd import preprocessing as P
    x, (D, H, W) = _shell(False)
    mask = P.create_nonzero_mask(x.to(DEV))
    assert int(mask.sum()) == (D - 6) * (H - 6) * (W - 6)
    assert P.get_bbox_from_mask(mask) == [[3, D - 3], [3, H - 3], [3, W - 3]]
    out, seg, bbox = P.crop_to_nonzero(x.to(DEV))
    assert bbox == [[3, D - 3], [3, H - 3], [3, W - 3]] and torch.equal(out.cpu(), x[:, 3:D - 3, 3:H - 3, 3:W - 3]) and not bool(seg.any())


def test_a_shell_with_a_corridor_is_not_filled_by_formula():
    from deformablelka_amd import preprocessing as P
    x, (D, H, W) = _shell(True)
    mask = P.create_nonzero_mask(x.to(DEV))
    shell = (D - 6) * (H - 6) * (W - 6) - (D - 8) * (H - 8) * (W - 8) - 1                           # the shell less the corridor's cell in it
    assert int(mask.sum()) == shell == int((x != 0).sum())
    assert torch.equal(mask.cpu(), x[0] != 0)
    assert P.get_bbox_from_mask(mask) == [[3, D - 3], [3, H - 3], [3, W - 3]]                       # the corridor is zero-valued: the box stays
    out, seg, bbox = P.crop_to_nonzero(x.to(DEV))
    assert int((seg == -1).sum()) == (D - 8) * (H - 8) * (W - 8) + 1


def test_statistics_of_a_ramp_by_formula():
    """x = 1 + (i mod 7) over 1 x 70 x 100 x 150 = 150 000 * 7 cells: every residue equally often, so the mean is 4 and the population variance
    (0 + 1 + 4 + 9) * 2 / 7 = 4 exactly; under the mask (seg = (i mod 7) - 1 >= 0 drops residue 0) the mean is 4.5 and the variance 35 / 12."""
    from deformablelka_amd import preprocessing as P
    shape = (1, 70, 100, 150)
    i = torch.arange(70 * 100 * 150, dtype=torch.int64)
    x = (1 + i % 7).to(torch.float32).reshape(shape)
    seg = ((i % 7) - 1).clamp(max=0).to(torch.float32).reshape(shape)
    for use_mask, mean, var in ((False, 4.0, 4.0), (True, 4.5, 35.0 / 12.0)):
        pre = P.GenericPreprocessor({0: "nonCT"}, {0: use_mask}, [0, 1, 2])
        out, stats = pre.normalize(x.to(DEV), seg.to(DEV))
        n, m, s = stats.cpu().tolist()[0]
        assert n == (6 if use_mask else 7) * 150000 and abs(m - mean) <= 1e-12 * mean and abs(s - var ** 0.5) <= 1e-12 * var ** 0.5
        want = (x - torch.tensor(m).to(torch.float32)) / (torch.tensor(s).to(torch.float32) + torch.tensor(1e-8, dtype=torch.float32))
        if use_mask:
            want = torch.where(seg >= 0, want, torch.zeros_like(want))
        assert out.is_cuda and torch.equal(out.cpu().view(torch.int32), want.view(torch.int32))
    props = {0: {'mean': 3.7, 'sd': 1.9, 'percentile_00_5': 1.5, 'percentile_99_5': 6.25}}
    out, _ = P.GenericPreprocessor({0: "CT"}, {0: True}, [0, 1, 2], props).normalize(x.to(DEV), seg.to(DEV))
    f = lambda v: torch.tensor(v, dtype=torch.float64).to(torch.float32)   # noqa: E731
    want = (torch.minimum(torch.maximum(x, f(1.5)), f(6.25)) - f(3.7)) / f(1.9)
    want = torch.where(seg >= 0, want, torch.zeros_like(want))
    assert torch.equal(out.cpu().view(torch.int32), want.view(torch.int32))                        # the CT arithmetic, bit for bit


def test_a_device_tensor_stays_on_the_device():
    from deformablelka_amd import preprocessing as P, resampling
    data, seg, out, sout, props = C.run_pipeline(P, "two_modalities", DEV)
    assert out.is_cuda and sout.is_cuda and out.dtype == torch.float32
    again, _ = resampling.resample_patient(out, None, (1.25, 1.25, 1.25), (1.0, 1.0, 1.0), 1, 0)  # straight into the next stage
    assert again.is_cuda and again.shape[0] == 2
    batch = out[None].contiguous()                                                                 # the network's (b, c, x, y, z)
    assert batch.is_cuda and batch.data_ptr() == out.data_ptr()
    x = torch.from_numpy(data).to(DEV)
    cropped, cseg, bbox = P.crop_to_nonzero(x)
    mask = P.create_nonzero_mask(x)
    normed, stats = C.preprocessor(P, [0, 1, 2], ("nonCT", "nonCT"), (True, True)).normalize(cropped, cseg)
    assert all(t.is_cuda for t in (cropped, cseg, mask, normed, stats))
