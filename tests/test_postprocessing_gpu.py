"""deformablelka_amd.postprocessing (csrc/cl_conn_comp.hip) on the MI355X against the fixture recorded from the reference's own
remove_all_but_the_largest_connected_component and scipy.ndimage.label (tests/golden/reference_postprocessing.pt; scipy is not needed here).
The same cases as the emulator suite (tests/postprocessing_cases.py), and two built by formula at sizes the emulator is too slow for."""
import numpy as np
import pytest
import torch

from tests import postprocessing_cases as C

from deformablelka_amd import postprocessing  # noqa: F401  (the feature: without it nothing here can run)

pytestmark = pytest.mark.gpu
DEV = "cuda"
FX = C.load_fixture()
CASES = list(FX["cases"].keys())


@pytest.mark.parametrize("name", CASES)
def test_label_equals_scipy(name):
    C.check_label(name, FX["cases"][name], DEV)


@pytest.mark.parametrize("name", CASES)
def test_remove_equals_the_reference(name):
    C.check_remove(name, FX["cases"][name], DEV)


def test_connectivity_changes_the_objects():
    C.check_connectivity_counts(FX, DEV)


def test_serpentine_is_one_object_per_class():
    C.check_serpentine(FX, DEV)


def test_numbering_follows_the_first_cell():
    C.check_late_join(FX, DEV)


def test_every_object_of_the_largest_size_is_kept():
    C.check_ties(FX, DEV)


def test_dtypes_and_containers():
    C.check_dtypes(FX, DEV)


def test_more_entries_than_one_pass_takes():
    C.check_chunking(FX, DEV)


def test_argument_errors():
    C.check_errors(DEV)


def test_library_refuses_bad_descriptions():
    C.check_c_abi_refuses(DEV)


def test_two_runs_are_bitwise_equal():
    C.check_reproducible(FX, DEV)


def test_launches_of_one_call():
    C.check_launch_count(FX, DEV)


def test_host_tensor_comes_back_on_the_host():
    from deformablelka_amd import postprocessing as P
    case = FX["cases"]["late_join"]
    labels, n = P.label(case["image"])
    assert labels.device.type == "cpu" and n == 3 and torch.equal(labels, case["label"][1]["labels"].to(torch.int32))


def test_a_million_cells_by_formula():
    """A 1-cell-wide path of class 1 through every tile of a 64 x 96 x 160 map (a comb in every even plane, the planes linked through single
    cells of the odd planes), isolated cells of class 1 and of class 2 in the odd planes.  No scipy, no fixture: one object of known size, 79872
    of one cell each, numbered in raster order; class 2 has only objects of one cell, which are all of the largest size and stay."""
    from deformablelka_amd import postprocessing as P
    D, H, W = 64, 96, 160
    img = torch.zeros((D, H, W), dtype=torch.uint8)
    img[0::2, 0::2, :] = 1
    img[0::2, 1::4, W - 1] = 1
    img[0::2, 3:H - 1:4, 0] = 1
    img[1::4, H - 2, 0] = 1          # planes d, d + 2 linked at the end of the comb for d % 4 == 0 ...
    img[3:D - 1:4, 0, 0] = 1         # ... and at its start for d % 4 == 2
    snake = int((img == 1).sum())
    assert snake == (D // 2) * ((H // 2) * W + (H // 2 - 1)) + (D // 2 - 1)
    noise = torch.zeros_like(img, dtype=torch.bool)
    noise[1::2, 1::2, 4:158:3] = True
    other = torch.zeros_like(noise)
    other[1::2, 1::2, 5:158:3] = True
    n_noise = (D // 2) * (H // 2) * 52
    assert int(noise.sum()) == n_noise == 79872 and int(other.sum()) == (D // 2) * (H // 2) * 51
    img[noise] = 1
    img[other] = 2
    dev = img.to(DEV)
    labels, sizes = P.component_sizes(dev == 1)
    assert sizes.numel() == 1 + n_noise and int(sizes[0]) == snake and bool((sizes[1:] == 1).all())
    lab = labels.cpu()
    assert bool((lab[(img == 1) & ~noise] == 1).all()) and bool((lab[img != 1] == 0).all())
    assert torch.equal(lab[noise], torch.arange(2, 2 + n_noise, dtype=torch.int32))          # raster order of the first (only) cell
    out, removed, kept = P.remove_all_but_the_largest_connected_component(dev, [1, 2], 2.0)
    want = img.clone()
    want[noise] = 0
    assert torch.equal(out.cpu(), want) and removed == {1: 2.0, 2: None} and kept == {1: 2.0 * snake, 2: 2.0}
    out, removed, kept = P.remove_all_but_the_largest_connected_component(dev, [1, 2], 2.0, {1: 2.0, 2: 1.0})
    assert torch.equal(out, dev) and removed == {1: None, 2: None} and kept == {1: 2.0 * snake, 2: 2.0}
    joint, _, kept = P.remove_all_but_the_largest_connected_component(dev, [(1, 2)], 1.0)
    assert torch.equal(joint.cpu(), torch.where(noise | other, torch.zeros_like(img), img)) and kept == {(1, 2): float(snake)}


def test_long_lines_by_formula():
    """Runs of lengths 1, 2, 3, ... along lines much longer than a tile's span (64 cells; 2048 for a single line)."""
    from deformablelka_amd import postprocessing as P

    def runs(n):
        line, lengths, pos, k = torch.zeros(n, dtype=torch.int16), [], 0, 1
        while pos < n:
            line[pos:pos + k] = 5
            lengths.append(min(k, n - pos))
            pos += k + 1
            k += 1
        return line, lengths

    line, lengths = runs(200001)
    labels, sizes = P.component_sizes(line.to(DEV))
    assert sizes.tolist() == lengths and int(labels[-1]) in (0, len(lengths))
    row, lengths = runs(70001)
    img = torch.zeros((1, 3, 70001), dtype=torch.int16)
    img[0, 0], img[0, 2] = row, row.flip(0)
    labels, sizes = P.component_sizes(img.to(DEV), 3)
    assert sizes.tolist() == lengths + lengths[::-1]
    out, removed, kept = P.remove_all_but_the_largest_connected_component(img.to(DEV), [5], 0.5, {5: 100.0})
    biggest = max(lengths)
    assert kept == {5: 0.5 * biggest} and removed == {5: 99.5}                               # 199 cells < 100.0 / 0.5 <= 200 cells
    small = torch.tensor([n < 200 and n != biggest for n in lengths + lengths[::-1]])
    assert int((out != 0).sum()) == int(sizes.cpu()[~small].sum())
