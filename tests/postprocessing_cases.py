"""TEST INFRASTRUCTURE: the checks the emulator and the GPU suites of deformablelka_amd.postprocessing share, against
tests/golden/reference_postprocessing.pt (recorded by tests/golden/make_golden_postprocessing.py from the reference's own
remove_all_but_the_largest_connected_component and from scipy.ndimage.label).

Everything compared is an integer, or the float64 product of an integer count and the given volume per voxel: every comparison is EQUALITY."""
import os

import numpy as np
import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_postprocessing.pt")
RANDOM_COUNTS = {1: 1709, 2: 53, 3: 12}      # objects of the "random" case's (map != 0) under connectivity 1, 2, 3 (scipy): pairwise different
DIAGONAL_COUNTS = {1: 4, 2: 3, 3: 2}
LAUNCHES_PER_PASS = 6                        # local, merge, flatten, scan, rank, output (csrc/cl_conn_comp.hip); component_sizes adds the table


def load_fixture():
    return torch.load(FIXTURE, weights_only=False)


def same_dict(got, want):
    """Equal keys and values, and every value None or a Python float."""
    return got == want and all(v is None or type(v) is float for v in got.values())


def check_label(name, case, device):
    from deformablelka_amd import postprocessing as P
    image = case["image"].to(device)
    for cn, want in case["label"].items():
        labels, n = P.label(image, cn)
        assert type(n) is int and n == want["num"], (name, cn, n, want["num"])
        assert labels.dtype == torch.int32 and labels.device == image.device and labels.shape == image.shape
        assert torch.equal(labels.cpu(), want["labels"].to(torch.int32)), (name, cn)
        labels2, sizes = P.component_sizes(image, cn)
        assert torch.equal(labels2, labels) and sizes.dtype == torch.int64 and sizes.device == image.device
        assert torch.equal(sizes.cpu(), want["sizes"]), (name, cn)


def run_remove(case, call, device):
    from deformablelka_amd import postprocessing as P
    image = case["image"].to(device)
    keep = image.clone()
    out, removed, kept = P.remove_all_but_the_largest_connected_component(image, call["classes"], call["vpv"], call["min"])
    assert torch.equal(image, keep)                                   # the argument is not written to
    assert out.dtype == image.dtype and out.device == image.device and out.data_ptr() != image.data_ptr()
    return out, removed, kept


def check_remove(name, case, device):
    for i, call in enumerate(case["remove"]):
        out, removed, kept = run_remove(case, call, device)
        assert torch.equal(out.cpu().to(torch.int64), call["image"].to(torch.int64)), (name, i)
        assert same_dict(removed, call["largest_removed"]), (name, i, removed, call["largest_removed"])
        assert same_dict(kept, call["kept_size"]), (name, i, kept, call["kept_size"])
        assert list(removed.keys()) == list(call["largest_removed"].keys())


def check_connectivity_counts(fx, device):
    from deformablelka_amd import postprocessing as P
    for name, counts in (("random", RANDOM_COUNTS), ("diagonal_touch", DIAGONAL_COUNTS)):
        case = fx["cases"][name]
        assert len(set(counts.values())) == 3
        for cn, want in counts.items():
            assert case["label"][cn]["num"] == want
            assert P.label(case["image"].to(device), cn)[1] == want, (name, cn)


def check_serpentine(fx, device):
    """One object per class, as large as the class: a merge that stops before it has converged leaves several."""
    from deformablelka_amd import postprocessing as P
    case = fx["cases"]["serpentine"]
    image = case["image"].to(device)
    for c in (1, 2):
        labels, sizes = P.component_sizes(image == c)
        assert sizes.tolist() == [int((case["image"] == c).sum())]
    out, removed, kept = P.remove_all_but_the_largest_connected_component(image, [1, 2], 1.0)
    assert torch.equal(out, image) and removed == {1: None, 2: None}
    assert kept == {1: float((case["image"] == 1).sum()), 2: float((case["image"] == 2).sum())}


def check_late_join(fx, device):
    from deformablelka_amd import postprocessing as P
    case = fx["cases"]["late_join"]
    labels, n = P.label(case["image"].to(device))
    got = [int(labels[p]) for p in ((0, 5), (0, 66), (35, 30), (3, 15), (20, 30), (10, 40))]
    assert n == 3 and got == [1, 1, 1, 2, 2, 3], got


def check_ties(fx, device):
    case = fx["cases"]["ties"]
    out, removed, kept = run_remove(case, case["remove"][0], device)
    assert int((out == 2).sum()) == 12 and removed == {2: 6.0} and kept == {2: 12.0}    # both objects of 6 cells stay, the one of 3 goes
    assert torch.equal(out.cpu(), case["remove"][0]["image"].to(out.dtype))


def check_dtypes(fx, device):
    from deformablelka_amd import postprocessing as P
    case = fx["cases"]["image_67x131"]
    want, call = case["label"][1], case["remove"][0]
    for dtype in (torch.uint8, torch.int16, torch.int32, torch.int64, torch.bool):
        image = case["image"].to(device=device, dtype=dtype)
        keep = image.clone()
        labels, n = P.label(image)
        assert n == want["num"] and torch.equal(labels.cpu(), want["labels"].to(torch.int32)) and torch.equal(image, keep), dtype
        if dtype != torch.bool:
            out, removed, kept = P.remove_all_but_the_largest_connected_component(image, call["classes"], call["vpv"])
            assert out.dtype == dtype and torch.equal(out.cpu().to(torch.uint8), call["image"]) and torch.equal(image, keep)
            assert removed == call["largest_removed"] and kept == call["kept_size"]
    for npdtype in (np.uint8, np.int8, np.uint16, np.int64, np.float32, bool):    # numpy in, numpy out, same dtype
        arr = case["image"].numpy().astype(npdtype)
        before = arr.copy()
        labels, n = P.label(arr)
        assert isinstance(labels, np.ndarray) and labels.dtype == np.int32 and n == want["num"]
        assert np.array_equal(labels, want["labels"].numpy()) and np.array_equal(arr, before)
        labels, sizes = P.component_sizes(arr)
        assert isinstance(sizes, np.ndarray) and sizes.dtype == np.int64 and np.array_equal(sizes, want["sizes"].numpy())
        if npdtype is not bool:
            out, removed, kept = P.remove_all_but_the_largest_connected_component(arr, call["classes"], call["vpv"])
            assert isinstance(out, np.ndarray) and out.dtype == arr.dtype and out is not arr and np.array_equal(arr, before)
            assert np.array_equal(out.astype(np.uint8), call["image"].numpy()) and removed == call["largest_removed"]
    host = case["image"].clone()                                                   # a host tensor in: a host tensor out
    out, _, _ = P.remove_all_but_the_largest_connected_component(host, call["classes"], call["vpv"])
    assert out.device == host.device and torch.equal(out, call["image"]) and torch.equal(host, case["image"])


def check_chunking(fx, device):
    """More entries than one pass takes: the same answers as the fixture's per-class rows (the call with for_which_classes=None)."""
    from deformablelka_amd import _lib as L, postprocessing as P
    case = fx["cases"]["random"]
    call = case["remove"][2]
    assert call["classes"] is None and call["min"] is None
    classes = list(range(1, 41))
    assert len(classes) > L.DLKA_CC_K_MAX
    out, removed, kept = P.remove_all_but_the_largest_connected_component(case["image"].to(device), classes, call["vpv"])
    assert torch.equal(out.cpu().to(torch.uint8), call["image"])
    for c in classes:
        assert removed[c] == call["largest_removed"].get(c) and kept[c] == call["kept_size"].get(c), c
    assert list(removed.keys()) == classes


def check_errors(device):
    import pytest
    from deformablelka_amd import postprocessing as P
    a = torch.zeros((4, 5, 6), dtype=torch.uint8, device=device)
    a[1, 2, 3] = 1
    with pytest.raises(AssertionError, match="cannot remove background"):
        P.remove_all_but_the_largest_connected_component(a, [1, 0], 1.0)
    with pytest.raises(RuntimeError, match="rank 1, 2 or 3"):
        P.label(a[None])
    with pytest.raises(RuntimeError, match="rank 1, 2 or 3"):
        P.remove_all_but_the_largest_connected_component(a[None], [1], 1.0)
    for cn in (0, 4):
        with pytest.raises(RuntimeError, match="connectivity must be between 1 and the rank"):
            P.label(a, cn)
    with pytest.raises(RuntimeError, match="connectivity must be between 1 and the rank"):
        P.label(a[0], 3)
    with pytest.raises(RuntimeError, match="connectivity must be between 1 and the rank"):
        P.component_sizes(a[0, 0], 2)
    with pytest.raises(RuntimeError, match="uint8, int16, int32, int64"):
        P.label(a.to(torch.complex64))
    with pytest.raises(ValueError, match="volume_per_voxel must be positive"):
        P.remove_all_but_the_largest_connected_component(a, [1], 0.0)


def check_c_abi_refuses(device):
    """The library's own checks, past the Python ones: nothing is launched on a bad description."""
    import ctypes
    from deformablelka_amd import _lib as L, ops
    a = torch.ones((4, 5, 6), dtype=torch.uint8, device=device)
    labels, filtered, summary, (d, ws) = ops.cc_components(a, [(1, 2), (3,)], 1, [2, 2])
    lib, before = L.get_lib(), ops.cc_launch_count()

    def call(desc, ws_bytes=None, filt=filtered):
        return lib.dlka_cc_components(L.ptr(a), ctypes.byref(desc), L.ptr(ws), ws.numel() if ws_bytes is None else ws_bytes, L.ptr(labels),
                                      L.ptr(filt), L.ptr(summary), L.stream_ptr(a))

    def bad(**fields):
        b = L.ConnCompDesc.from_buffer_copy(d)
        for k, v in fields.items():
            if isinstance(v, tuple):
                getattr(b, k)[v[0]] = v[1]
            else:
                setattr(b, k, v)
        return b

    for fields, code in (({"K": 0}, -8), ({"K": L.DLKA_CC_K_MAX + 1}, -8), ({"rank": 4}, -4), ({"rank": 0}, -4), ({"connectivity": 0}, -8),
                         ({"connectivity": 4}, -8), ({"label_dtype": 7}, -6), ({"n_ids": 0}, -8), ({"n_ids": L.DLKA_CC_IDS_MAX + 1}, -8),
                         ({"class_id": (2, 1)}, -8),                      # id 1 in both entries: overlapping id sets
                         ({"entry_of": (0, 2)}, -4), ({"ext": (1, -5)}, -4), ({"ext": (1, 0)}, -4), ({"min_count": (1, -1)}, -4),
                         ({"ext": (0, 1 << 31)}, -8),                     # 2^31 * 5 * 6 cells
                         ({"ext": (0, 71582789)}, -8)):                   # 71582789 * 30 = 2^31 + 22 cells
        b = bad(**fields)
        assert call(b) == code, fields
        assert lib.dlka_cc_workspace_bytes(ctypes.byref(b)) == 0
        assert lib.dlka_cc_component_table(ctypes.byref(b), L.ptr(ws), ws.numel(), 1, L.ptr(labels), L.ptr(labels), L.stream_ptr(a)) == code
    flat = bad(rank=2)                                                    # rank 2 with a depth of 4
    assert call(flat) == -4
    assert call(d, ws_bytes=100) == -7 and call(d, filt=a) == -8          # (the filtered map must not be the image)
    assert ops.cc_launch_count() == before
    assert call(d) == 0 and ops.cc_launch_count() == before + LAUNCHES_PER_PASS


def check_reproducible(fx, device):
    """Two runs of every fixture case: the component map, the sizes, the owners, the summary and the filtered map are bitwise equal."""
    from deformablelka_amd import ops
    for name, case in fx["cases"].items():
        image = case["image"].to(device)
        for call in case["remove"]:
            classes = call["classes"] if call["classes"] is not None else [int(v) for v in torch.unique(case["image"]).tolist() if v > 0]
            entries, seen = [], set()
            for c in classes:                                             # one pass: the entries that share no id with an earlier one
                ids = tuple(c) if isinstance(c, (list, tuple)) else (c,)
                if not seen & set(ids):
                    entries.append(ids)
                    seen |= set(ids)
            if not entries:
                continue
            runs = []
            for _ in range(2):
                labels, filtered, summary, state = ops.cc_components(image, entries, min(2, image.ndim), [3] * len(entries))
                n = int(summary[0])
                sizes, owner = ops.cc_component_table(state, n)
                runs.append([t.cpu() for t in (labels, filtered, summary, sizes, owner)])
            assert all(torch.equal(x, y) for x, y in zip(*runs)), name
            labels, filtered, summary, sizes, owner = runs[0]
            assert int(sizes.sum()) == int((labels != 0).sum()) and int(labels.max()) == int(summary[0]) == sizes.numel()
            assert owner.numel() == 0 or (0 <= int(owner.min()) and int(owner.max()) < len(entries))


def check_launch_count(fx, device):
    from deformablelka_amd import ops, postprocessing as P
    case = fx["cases"]["image_67x131"]
    call = case["remove"][0]
    before = ops.cc_launch_count()
    out, removed, kept = P.remove_all_but_the_largest_connected_component(case["image"].numpy(), call["classes"], call["vpv"])   # numpy: moved over
    assert ops.cc_launch_count() == before + LAUNCHES_PER_PASS                                     # all classes in ONE pass
    assert isinstance(out, np.ndarray) and np.array_equal(out, call["image"].numpy()) and removed == call["largest_removed"]
    P.component_sizes(case["image"].to(device))
    assert ops.cc_launch_count() == before + 2 * LAUNCHES_PER_PASS + 1
    two = fx["cases"]["random"]
    P.remove_all_but_the_largest_connected_component(two["image"].to(device), two["remove"][0]["classes"], 1.0)
    assert ops.cc_launch_count() == before + 4 * LAUNCHES_PER_PASS + 1                             # [(1, 2), 3, 2]: class 2 twice, two passes
