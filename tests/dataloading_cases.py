"""TEST INFRASTRUCTURE — the cases and checks of deformablelka_amd.dataloading, shared by tests/test_dataloading_emu.py (wavefront emulator,
CPU suite) and tests/test_dataloading_gpu.py (MI355X).  The expected results are in tests/golden/reference_dataloading.pt, recorded by
tests/golden/make_golden_dataloading.py from the reference's own DataLoader3D.generate_train_batch and GenericPreprocessor._run_internal.

The INPUTS are not stored: they are rebuilt here by formula (the integer hash of tests/resampling_cases.py), so they are the same bits on every
machine; the fixture holds their SHA-256 and every check compares it first.

Bounds (the issue's): EQUALITY everywhere.  Nothing here is arithmetic: a batch is a bit copy of cells and constants, a box is integers, a
class location is integers.  Batches are compared by SHA-256 with the fixture and cell by cell with the numpy restatement
(tests/dataloading_ref.py), which is itself held to the fixture."""
import copy
import os

import numpy as np
import torch

from tests.resampling_cases import digest, noise

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "reference_dataloading.pt")
LAUNCHES = {"crop_batch": 1, "class_counts": 2, "class_select": 2}       # csrc/cl_dataload.hip
TILE = 2048                                                              # cells one wave owns in the class kernels
PATCH = (8, 12, 10)


def load_fixture():
    return torch.load(FIXTURE, weights_only=False)


def to_np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))


# ---- cases of the loader: (C + 1, X, Y, Z) float32, the label map last ---------------------------------------------------------------------------
def case_array(shape, salt, labels="mixed"):
    c = shape[0] - 1
    x = np.empty(shape, np.float32)
    x[:c] = ((noise((c,) + tuple(shape[1:]), salt) - 0.5) * 200.0).astype(np.float32)
    n = noise(shape[1:], salt + 50)
    if labels == "mixed":                          # -1 (outside the nonzero mask), 0 and the classes 1..3
        seg = np.floor(n * 5.0) - 1.0
    elif labels == "none":                         # no foreground at all
        seg = np.where(n < 0.2, -1.0, 0.0)
    else:                                          # "corner": class 2 in the last 2 x 2 x 2 cells only
        seg = np.where(n < 0.2, -1.0, 0.0)
        seg[-2:, -2:, -2:] = 2.0
    x[c] = seg.astype(np.float32)
    return x


def all_locations(seg, classes=(1, 2, 3)):
    """class_locations that list EVERY cell of a class: the loader's input, independent of the sampling under test."""
    out = {}
    for c in classes:
        locs = np.argwhere(seg == c)
        out[c] = locs if len(locs) else []
    return out


# id -> (cases: key -> (shape, salt, labels), patch_size, final_patch_size, batch_size, oversample, pad_mode, pad_kwargs_data, seed, batches)
LOADER_CALLS = {
    # the first sample of the first batch is "small": need_to_pad grows from (0, 2, 0) to (1, 3, 0) and stays so
    "aliasing": ({"small": ((2, 7, 9, 13), 61, "mixed"), "mid": ((2, 12, 15, 16), 62, "mixed"), "big": ((2, 20, 17, 21), 63, "mixed")},
                 PATCH, (8, 10, 10), 3, 0.33, "edge", None, 7, 3),
    # two modalities, a nonzero constant; "nofg" falls back to random boxes, a forced box on "corner" runs past the upper end
    "constant2": ({"nofg": ((3, 9, 14, 12), 64, "none"), "corner": ((3, 11, 13, 17), 65, "corner"), "plain": ((3, 10, 16, 13), 66, "mixed")},
                  PATCH, (6, 10, 8), 3, 0.33, "constant", {"constant_values": 2.5}, 4, 4),
}


def loader_inputs(cid):
    """(data dict as DataLoader3D takes it, the call's other arguments)."""
    specs, patch, final, B, p, mode, kwargs, seed, batches = LOADER_CALLS[cid]
    data = {}
    for key, (shape, salt, labels) in specs.items():
        arr = case_array(shape, salt, labels)
        data[key] = {"data": arr, "properties": {"class_locations": all_locations(arr[-1]), "name": key}}
    return data, (patch, final, B, p, mode, kwargs, seed, batches)


def inputs_digest(data):
    return {k: digest(v["data"]) for k, v in data.items()}


# ---- crop cases: id -> (list of (shape, salt), boxes, pad_mode, pad_kwargs_data) -------------------------------------------------------------------
CROP_CASES = {
    "smaller_edge": ([((2, 7, 9, 13), 71)], [(0, -1, 2)], "edge", None),
    "smaller_constant": ([((2, 7, 9, 13), 71)], [(-1, -2, 3)], "constant", {"constant_values": -3.25}),
    "negative_and_past": ([((2, 12, 15, 16), 72)], [(-3, 9, 4)], "edge", None),                 # x below 0, y past the end
    "inside": ([((2, 12, 15, 16), 72)], [(2, 1, 3)], "constant", None),                           # no padding; rows of 16 read from column 3
    "mixed_batch_c1": ([((2, 7, 9, 13), 71), ((2, 12, 15, 16), 72), ((2, 20, 17, 21), 73)], [(-1, -2, 4), (5, -4, 7), (13, 6, -2)],
                       "constant", {"constant_values": 1.5}),
    "mixed_batch_c2": ([((3, 9, 14, 12), 74), ((3, 11, 13, 17), 75), ((3, 10, 16, 13), 76)], [(2, 3, 3), (-5, 2, 9), (3, -1, -7)], "edge", None),
    "default_zero": ([((3, 9, 14, 12), 74)], [(4, 5, 6)], "constant", None),                    # the data reads 0 outside, the seg -1
    "odd_patch": ([((2, 7, 9, 13), 71), ((2, 12, 15, 16), 72)], [(-2, 1, 5), (9, 11, 13)], "edge", None),   # patch (5, 7, 9): 315 cells, quads straddle samples
}
CROP_PATCH = {"odd_patch": (5, 7, 9)}


def crop_inputs(name):
    specs, boxes, mode, kwargs = CROP_CASES[name]
    return [case_array(shape, salt) for shape, salt in specs], np.array(boxes, np.int64), CROP_PATCH.get(name, PATCH), mode, kwargs


# ---- class_locations cases: id -> (label map float32 (X, Y, Z), all_classes) ---------------------------------------------------------------------
def _branches():
    """20 000 cells: class 1 on 7000 of them (1 %: 70 rows at num_samples=50), class 2 on 31 (fewer than num_samples), class 3 absent."""
    shape = (20, 25, 40)
    i = np.arange(20000)
    seg = np.where(i % 20 < 7, 1.0, 0.0)
    seg[(i % 20 == 9) & (i % 660 == 9)] = 2.0
    seg[i % 20 == 11] = -1.0
    seg[i % 20 == 13] = 9.0                        # not in all_classes
    return seg.reshape(shape).astype(np.float32), [1, 2, 3]


def _edges():
    """6549 cells = 3 tiles and 405 cells: class 1 across the wave boundary 63 | 64 and the tile boundary 2047 | 2048, class 2 in the last,
    partial tile only (its last cell included), class 5 absent; -1 and 7 are ignored."""
    shape = (3, 37, 59)
    seg = np.zeros(3 * 37 * 59)
    seg[60:70] = 1.0
    seg[2040:2060] = 1.0
    seg[4095], seg[4096] = 1.0, 1.0
    seg[6200:6230] = 2.0
    seg[-1] = 2.0
    seg[100:140], seg[6300:6320] = -1.0, 7.0
    return seg.reshape(shape).astype(np.float32), [1, 2, 5]


def _many():
    """10 373 cells with the labels -1 .. 38, of which 1 .. 32 are asked for: K = 32."""
    shape = (11, 23, 41)
    return (np.floor(noise(shape, 81) * 40.0) - 1.0).astype(np.float32), list(range(1, 33))


def _with_background():
    """Class 0 asked for as well, and the classes out of order: the RandomState is consumed in the order of all_classes."""
    seg, _ = _edges()
    return seg, [2, 0, 1]


CL_CASES = {"branches": _branches, "edges": _edges, "one_class": lambda: (_edges()[0], [2]), "many": _many, "with_background": _with_background}
CL_SMALL = dict(num_samples=50, min_percent_coverage=0.01, seed=1234)


def locations_digest(locs):
    """class -> (rows, SHA-256 of the int64 rows)."""
    return {int(c): (len(v), digest(np.asarray(v, dtype=np.int64).reshape(-1, 3))) for c, v in locs.items()}


# ---- checks -------------------------------------------------------------------------------------------------------------------------------------
def check_draws(cid, rec):
    """draw_batch with RandomState(seed) gives the keys, flags and boxes the reference gave after np.random.seed(seed), batch after batch."""
    from deformablelka_amd import dataloading as D
    data, (patch, final, B, p, mode, kwargs, seed, batches) = loader_inputs(cid)
    assert inputs_digest(data) == rec["inputs"]
    cases = {k: {"shape": v["data"].shape[1:], "properties": v["properties"]} for k, v in data.items()}
    need_to_pad = (np.array(patch) - np.array(final)).astype(int)
    rs = np.random.RandomState(seed)
    for n in range(batches):
        got, want = D.draw_batch(rs, cases, patch, need_to_pad, B, p), rec["batches"][n]
        assert [str(k) for k in got["keys"]] == want["keys"], (cid, n)
        assert got["bbox_lb"].tolist() == want["bbox_lb"], (cid, n, got["bbox_lb"].tolist(), want["bbox_lb"])
        assert got["force_fg"].tolist() == want["force_fg"] and need_to_pad.tolist() == want["need_to_pad"], (cid, n)
        assert got["selected_class"].tolist() == want["selected_class"] and got["selected_voxel"].tolist() == want["selected_voxel"], (cid, n)
        assert got["bbox_lb"].dtype == np.int64 and got["force_fg"].dtype == bool


def check_loader(cid, rec, device):
    """DataLoader3D's batches are the reference's, bit for bit."""
    from deformablelka_amd import dataloading as D
    from tests import dataloading_ref as R
    data, (patch, final, B, p, mode, kwargs, seed, batches) = loader_inputs(cid)
    assert inputs_digest(data) == rec["inputs"]
    before = copy.deepcopy(data)
    loader = D.DataLoader3D(data, patch, final, B, False, p, "r", mode, kwargs, device=device, seed=seed)
    c = next(iter(data.values()))["data"].shape[0] - 1
    assert loader.data_shape == (B, c) + tuple(patch) and loader.seg_shape == (B, 1) + tuple(patch)
    for n in range(batches):
        batch, want = next(loader), rec["batches"][n]
        assert set(batch) == {"data", "seg", "properties", "keys"}
        d, s = batch["data"], batch["seg"]
        assert d.dtype == s.dtype == torch.float32 and d.device.type == s.device.type == torch.device(device).type
        assert tuple(d.shape) == loader.data_shape and tuple(s.shape) == loader.seg_shape
        assert [str(k) for k in batch["keys"]] == want["keys"] and loader.last_draw["bbox_lb"].tolist() == want["bbox_lb"], (cid, n)
        assert [pr["name"] for pr in batch["properties"]] == want["keys"]
        rd, rseg = R.crop_batch([data[k]["data"] for k in want["keys"]], want["bbox_lb"], patch, mode, kwargs)
        print(f"{cid} batch {n}: cells that differ from the restatement: data {int((to_np(d).view(np.int32) != rd.view(np.int32)).sum())}, "
              f"seg {int((to_np(s) != rseg).sum())}")
        assert same_bits(to_np(d), rd) and same_bits(to_np(s), rseg), (cid, n)
        assert digest(to_np(d)) == want["data"] and digest(to_np(s)) == want["seg"], (cid, n)
    assert loader.need_to_pad.tolist() == rec["batches"][-1]["need_to_pad"]
    for k in data:                                                                           # the caller's arrays are untouched
        assert same_bits(data[k]["data"], before[k]["data"])


def check_crop(name, device):
    from deformablelka_amd import dataloading as D
    from tests import dataloading_ref as R
    arrays, boxes, patch, mode, kwargs = crop_inputs(name)
    cases = [torch.from_numpy(a.copy()).to(device) for a in arrays]
    d, s = D.crop_batch(cases, boxes, patch, mode, kwargs)
    rd, rseg = R.crop_batch(arrays, boxes, patch, mode, kwargs)
    assert d.dtype == s.dtype == torch.float32 and d.device == cases[0].device and tuple(d.shape) == rd.shape and tuple(s.shape) == rseg.shape
    print(f"{name}: cells that differ: data {int((to_np(d).view(np.int32) != rd.view(np.int32)).sum())}, seg {int((to_np(s) != rseg).sum())}")
    assert same_bits(to_np(d), rd) and same_bits(to_np(s), rseg), name
    assert all(same_bits(to_np(t), a) for t, a in zip(cases, arrays))
    return to_np(d), to_np(s), arrays, boxes, patch


def check_crop_properties():
    """What the crop cases claim to cover."""
    _, boxes, patch, _, _ = crop_inputs("smaller_edge")
    assert all(e < p for e, p in zip((7, 9), patch[:2])) and 13 % 4 != 0 and patch[2] % 4 != 0 and (12 - 9) % 2 == 1
    arrays, boxes, patch, _, _ = crop_inputs("negative_and_past")
    assert boxes[0][0] < 0 and boxes[0][1] + patch[1] > arrays[0].shape[2]
    assert len({a.shape for a in crop_inputs("mixed_batch_c1")[0]}) == 3 and crop_inputs("mixed_batch_c2")[0][0].shape[0] == 3
    assert int(np.prod(CROP_PATCH["odd_patch"])) % 4 != 0
    assert max(int(np.prod(a.shape[1:])) for n in CROP_CASES for a in crop_inputs(n)[0]) <= 20000


def check_seg_padding(device):
    """Outside the case the label map reads -1 while the data reads the constant (0 by default, or the one given)."""
    for name, constant in (("default_zero", 0.0), ("smaller_constant", -3.25)):
        d, s, arrays, boxes, patch = check_crop(name, device)
        lb, shape = boxes[0], arrays[0].shape[1:]
        grid = np.meshgrid(*[np.arange(patch[ax]) + lb[ax] for ax in range(3)], indexing="ij")
        outside = ~np.logical_and.reduce([(g >= 0) & (g < shape[ax]) for ax, g in enumerate(grid)])
        assert outside.any() and not outside.all()
        assert bool((s[0, 0][outside] == -1.0).all()) and bool((d[0][:, outside] == np.float32(constant)).all())
        assert bool((s[0, 0][~outside] >= -1.0).all())


def check_chunking(device):
    """B = DLKA_LOAD_B_MAX + 1 takes two launches and equals the rows of unchunked calls."""
    from deformablelka_amd import _lib as L, dataloading as D
    from tests import dataloading_ref as R
    arrays, _, patch, _, _ = crop_inputs("mixed_batch_c2")
    B = L.DLKA_LOAD_B_MAX + 1
    resident = [torch.from_numpy(a.copy()).to(device) for a in arrays]
    cases = [resident[b % 3] for b in range(B)]
    boxes = np.array([[(b * 3) % 11 - 4, (b * 5) % 13 - 5, (b * 7) % 9 - 3] for b in range(B)], np.int64)
    before = D.launch_count()
    d, s = D.crop_batch(cases, boxes, patch, "edge")
    assert D.launch_count() == before + 2
    head = D.crop_batch(cases[:L.DLKA_LOAD_B_MAX], boxes[:L.DLKA_LOAD_B_MAX], patch, "edge")
    tail = D.crop_batch(cases[-1:], boxes[-1:], patch, "edge")
    assert D.launch_count() == before + 4
    assert torch.equal(d[:-1], head[0]) and torch.equal(s[:-1], head[1]) and torch.equal(d[-1:], tail[0]) and torch.equal(s[-1:], tail[1])
    rd, rseg = R.crop_batch([arrays[b % 3] for b in range(B)], boxes, patch, "edge")
    assert same_bits(to_np(d), rd) and same_bits(to_np(s), rseg)


def _assert_locations(got, want, what):
    assert list(got.keys()) == list(want.keys()), what
    for c in want:
        if len(want[c]) == 0:
            assert isinstance(got[c], list) and got[c] == [], (what, c)
            continue
        assert isinstance(got[c], np.ndarray) and got[c].dtype == np.int64 and got[c].shape == np.asarray(want[c]).shape, (what, c)
        bad = np.flatnonzero((got[c] != want[c]).any(1))
        assert bad.size == 0, (what, c, "first differing row", int(bad[0]), got[c][bad[0]].tolist(), np.asarray(want[c])[bad[0]].tolist())


def check_class_locations(name, rec, device):
    from deformablelka_amd import dataloading as D
    from tests import dataloading_ref as R
    seg, classes = CL_CASES[name]()
    assert digest(seg) == rec["input"] and seg.size <= 20000, name
    t = torch.from_numpy(seg.copy()).to(device)
    for key, kw in (("default", {}), ("small", CL_SMALL)):
        got = D.class_locations(t, classes, **kw)
        _assert_locations(got, R.class_locations(seg, classes, **kw), (name, key))
        assert locations_digest(got) == {int(c): tuple(v) for c, v in rec[key].items()}, (name, key)
        as_int = D.class_locations(t.to(torch.int32), classes, **kw)                         # an int32 map: the same rows
        _assert_locations(as_int, got, (name, key, "int32"))
    assert same_bits(to_np(t), seg)


def check_class_location_properties(fx):
    """What the class_locations cases claim to cover."""
    seg, classes = CL_CASES["branches"]()
    assert int((seg == 1).sum()) == 7000 and int((seg == 2).sum()) == 31 and int((seg == 3).sum()) == 0 and bool((seg == -1).any())
    assert bool((seg == 9).any()) and 9 not in classes
    rec = fx["class_locations"]["branches"]
    assert rec["small"][1][0] == 70 and rec["small"][2][0] == 31 and rec["small"][3][0] == 0
    assert rec["default"][1][0] == 7000 and rec["default"][3][0] == 0
    seg, classes = CL_CASES["edges"]()
    flat = seg.reshape(-1)
    assert flat.size % TILE != 0 and flat.size // TILE == 3
    assert flat[63] == flat[64] == 1.0 and flat[TILE - 1] == flat[TILE] == 1.0 and flat[2 * TILE - 1] == flat[2 * TILE] == 1.0
    assert np.flatnonzero(flat == 2).min() >= 3 * TILE and flat[-1] == 2.0 and bool((flat == -1).any()) and bool((flat == 7).any())
    assert len(CL_CASES["one_class"]()[1]) == 1 and len(CL_CASES["many"]()[1]) == 32
    seg, classes = CL_CASES["many"]()
    assert all(bool((seg == c).any()) for c in classes) and float(seg.min()) == -1.0 and float(seg.max()) > 32


def check_reproducible(device):
    """Two runs: the same bits."""
    from deformablelka_amd import dataloading as D
    for name in ("mixed_batch_c2", "odd_patch"):
        arrays, boxes, patch, mode, kwargs = crop_inputs(name)
        cases = [torch.from_numpy(a.copy()).to(device) for a in arrays]
        a, b = D.crop_batch(cases, boxes, patch, mode, kwargs), D.crop_batch(cases, boxes, patch, mode, kwargs)
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]), name
    for name in ("edges", "many"):
        seg, classes = CL_CASES[name]()
        t = torch.from_numpy(seg).to(device)
        a, b = D.class_locations(t, classes, **CL_SMALL), D.class_locations(t, classes, **CL_SMALL)
        _assert_locations(a, b, name)


def check_launch_count(device):
    """Launches per call, whatever B, C, K and the extents are."""
    from deformablelka_amd import dataloading as D
    from deformablelka_amd.ops import dataload
    for name in ("smaller_edge", "mixed_batch_c1", "mixed_batch_c2", "odd_patch"):
        arrays, boxes, patch, mode, kwargs = crop_inputs(name)
        cases = [torch.from_numpy(a.copy()).to(device) for a in arrays]
        before = dataload.load_launch_count()
        D.crop_batch(cases, boxes, patch, mode, kwargs)
        assert dataload.load_launch_count() == before + LAUNCHES["crop_batch"], name
    for name in CL_CASES:
        seg, classes = CL_CASES[name]()
        before = dataload.load_launch_count()
        D.class_locations(torch.from_numpy(seg).to(device), classes)
        assert dataload.load_launch_count() == before + LAUNCHES["class_counts"] + LAUNCHES["class_select"], name
    seg, _ = CL_CASES["edges"]()
    before = dataload.load_launch_count()
    assert D.class_locations(torch.from_numpy(seg).to(device), [5, 6]) == {5: [], 6: []}     # nothing to select: the counts alone
    assert dataload.load_launch_count() == before + LAUNCHES["class_counts"]
    assert D.launch_count() == dataload.load_launch_count()


def check_containers(fx, device):
    """numpy in, tensors in (host or device, float or integer): the same rows; entries read from .npy / .npz files; nothing written to."""
    import pickle
    import tempfile
    from deformablelka_amd import dataloading as D
    seg, classes = CL_CASES["edges"]()
    want = D.class_locations(torch.from_numpy(seg.copy()).to(device), classes, **CL_SMALL)
    for form in (seg.copy(), seg.astype(np.int16), seg.astype(np.int64), seg.astype(np.float64), torch.from_numpy(seg.copy()),
                 torch.from_numpy(seg.astype(np.int64))):
        before = form.clone() if isinstance(form, torch.Tensor) else form.copy()
        _assert_locations(D.class_locations(form, classes, **CL_SMALL), want, type(form))
        assert np.array_equal(to_np(form), to_np(before))
    np_classes = D.class_locations(seg, np.array(classes), **CL_SMALL)
    assert [int(c) for c in np_classes] == classes
    cid = "aliasing"
    data, (patch, final, B, p, mode, kwargs, seed, batches) = loader_inputs(cid)
    with tempfile.TemporaryDirectory() as tmp:
        files = {}
        for n, (k, v) in enumerate(data.items()):
            if n == 0:                                                               # an unpacked case: X.npy beside the X.npz it is named by
                np.save(os.path.join(tmp, k + ".npy"), v["data"])
            else:
                np.savez_compressed(os.path.join(tmp, k + ".npz"), data=v["data"])
            files[k] = {"data_file": os.path.join(tmp, k + ".npz")}
            if n == 1:
                with open(os.path.join(tmp, k + ".pkl"), "wb") as f:
                    pickle.dump(v["properties"], f)
                files[k]["properties_file"] = os.path.join(tmp, k + ".pkl")
            else:
                files[k]["properties"] = v["properties"]
        from_files = D.DataLoader3D(files, patch, final, B, False, p, "r", mode, kwargs, device=device, seed=seed)
    tensors = {k: {"data": torch.from_numpy(v["data"].copy()).to(device), "properties": v["properties"]} for k, v in data.items()}
    from_tensors = D.DataLoader3D(tensors, patch, final, B, False, p, "r", mode, kwargs, device=device, seed=seed)
    for n in range(batches):
        want_b = fx["loader"][cid]["batches"][n]
        for loader in (from_files, from_tensors):
            b = loader.generate_train_batch()
            assert digest(to_np(b["data"])) == want_b["data"] and digest(to_np(b["seg"])) == want_b["seg"]


def check_errors(device):
    import pytest
    from deformablelka_amd import dataloading as D
    arrays, boxes, patch, mode, kwargs = crop_inputs("smaller_edge")
    cases = [torch.from_numpy(a.copy()).to(device) for a in arrays]
    data, (lpatch, final, B, p, lmode, lkwargs, seed, _) = loader_inputs("aliasing")
    for call in (lambda: D.crop_batch(cases, boxes, patch, "reflect"), lambda: D.crop_batch(cases, boxes, patch, "constant", {"constant_values": (1, 2)}),
                 lambda: D.crop_batch(cases, boxes, patch, "edge", {"constant_values": 1}), lambda: D.DataLoader2D,
                 lambda: D.DataLoader3D(data, lpatch, final, B, True), lambda: D.DataLoader3D(data, lpatch, final, B, pad_mode="wrap"),
                 lambda: D.unpack_dataset, lambda: D.class_locations(arrays[0], [1])):
        with pytest.raises(NotImplementedError):
            call()
    for call in (lambda: D.crop_batch(cases, boxes[:, :2], patch), lambda: D.crop_batch(cases + cases, boxes, patch),
                 lambda: D.crop_batch([cases[0].to(torch.float64)], boxes, patch), lambda: D.crop_batch([cases[0][0]], boxes, patch),
                 lambda: D.crop_batch([], boxes[:0], patch), lambda: D.crop_batch(cases, boxes, (8, 0, 10)),
                 lambda: D.class_locations(arrays[0][-1], list(range(33)))):
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(ValueError, match="empty axis"):                                # np.pad's refusal: the box misses the case
        D.crop_batch(cases, np.array([[7, 0, 0]]), patch, "edge")
    with pytest.raises(ValueError, match="need_to_pad"):
        D.draw_batch(np.random.RandomState(0), {}, patch, [0, 0, 0], 2, 0.0)
    with pytest.raises(AttributeError):
        D.no_such_name
    no_locations = {"a": {"shape": (9, 9, 9), "properties": {}}}
    with pytest.raises(RuntimeError, match="rerun the preprocessing"):
        D.draw_batch(np.random.RandomState(0), no_locations, patch, np.zeros(3, int), 2, 1.0)
    assert D.class_locations(arrays[0][-1], []) == {}
    loader = D.DataLoader3D(data, lpatch, final, 5, oversample_foreground_percent=0.33, device=device)
    assert [loader.get_do_oversample(j) for j in range(5)] == [False, False, False, True, True] and iter(loader) is loader


def check_c_abi_refuses(device):
    """The library's own checks, past the Python ones: nothing is launched on a bad description."""
    import ctypes
    from deformablelka_amd import _lib as L
    from deformablelka_amd.ops import dataload
    case = torch.zeros((2, 4, 5, 6), dtype=torch.float32, device=device)
    out, seg_out = torch.empty((1, 1, 3, 3, 3), device=device), torch.empty((1, 1, 3, 3, 3), device=device)
    lib, st, null = L.get_lib(), L.stream_ptr(case), ctypes.c_void_p(0)

    def crop_desc(**fields):
        d = L.LoadCropDesc()
        d.B, d.C, d.mode, d.constant = 1, 1, L.DLKA_LOAD_EDGE, 0.0
        for ax in range(3):
            d.patch[ax], d.sample[0].ext[ax], d.sample[0].lb[ax] = 3, case.shape[1 + ax], -1
        d.sample[0].data = case.data_ptr()
        for k, v in fields.items():
            if k in ("ext", "lb"):
                getattr(d.sample[0], k)[v[0]] = v[1]
            elif k == "data":
                d.sample[0].data = v
            elif isinstance(v, tuple):
                getattr(d, k)[v[0]] = v[1]
            else:
                setattr(d, k, v)
        return d

    before = dataload.load_launch_count()
    for fields, code in (({"B": 0}, -4), ({"C": 0}, -4), ({"B": L.DLKA_LOAD_B_MAX + 1}, -8), ({"mode": 2}, -8), ({"patch": (1, 0)}, -4),
                         ({"patch": (2, (1 << 30) + 1)}, -8), ({"ext": (0, 0)}, -4), ({"ext": (2, -6)}, -4), ({"ext": (0, 1 << 31)}, -8),
                         ({"ext": (1, 1 << 29)}, -8), ({"lb": (1, (1 << 30) + 1)}, -8), ({"lb": (1, -(1 << 30) - 1)}, -8), ({"data": None}, -1)):
        assert lib.dlka_load_crop_batch(ctypes.byref(crop_desc(**fields)), L.ptr(out), L.ptr(seg_out), st) == code, fields
    assert lib.dlka_load_crop_batch(None, L.ptr(out), L.ptr(seg_out), st) == -1
    assert lib.dlka_load_crop_batch(ctypes.byref(crop_desc()), null, L.ptr(seg_out), st) == -1
    assert lib.dlka_load_crop_batch(ctypes.byref(crop_desc()), L.ptr(out), null, st) == -1

    labels = torch.zeros((4, 5, 6), dtype=torch.float32, device=device)
    ws = torch.zeros(1 << 12, dtype=torch.uint8, device=device)
    totals_dev = torch.zeros(L.DLKA_LOAD_K_MAX, dtype=torch.int32, device=device)
    sel = torch.zeros(4, dtype=torch.int32, device=device)
    rows = torch.zeros((4, 3), dtype=torch.int32, device=device)
    host = (ctypes.c_int64 * L.DLKA_LOAD_K_MAX)(*([0] * L.DLKA_LOAD_K_MAX))
    host[0] = 120

    def classes_desc(**fields):
        d = L.LoadClassesDesc()
        d.K, d.dtype = 2, L.DLKA_LOAD_F32
        for ax in range(3):
            d.ext[ax] = labels.shape[ax]
        d.class_id[0], d.class_id[1] = 0, 1
        for k, v in fields.items():
            if isinstance(v, tuple):
                getattr(d, k)[v[0]] = v[1]
            else:
                setattr(d, k, v)
        return d

    def entries(d, lab=L.ptr(labels), w=ws.numel(), tot=host):
        r = ctypes.byref(d)
        return [lib.dlka_load_class_counts(lab, r, L.ptr(ws), w, L.ptr(totals_dev), st),
                lib.dlka_load_class_select(lab, r, L.ptr(ws), w, tot, L.ptr(ws), w, L.ptr(sel), L.ptr(sel), 4, L.ptr(rows), st)]

    for fields, code in (({"K": 0}, -4), ({"K": L.DLKA_LOAD_K_MAX + 1}, -8), ({"dtype": 2}, -6), ({"ext": (1, 0)}, -4), ({"ext": (0, 1 << 31)}, -8),
                         ({"class_id": (1, 0)}, -4), ({"class_id": (1, 1 << 25)}, -8)):
        d = classes_desc(**fields)
        assert entries(d) == [code] * 2, fields
        assert lib.dlka_load_counts_workspace_bytes(ctypes.byref(d)) == 0 and lib.dlka_load_select_workspace_bytes(ctypes.byref(d), host) == 0
    d = classes_desc()
    assert entries(d, lab=null) == [-1] * 2 and entries(d, w=4) == [-7] * 2
    bad = (ctypes.c_int64 * L.DLKA_LOAD_K_MAX)(*([0] * L.DLKA_LOAD_K_MAX))
    bad[0], bad[1] = 100, 21                                                          # more cells than the map has
    assert lib.dlka_load_class_select(L.ptr(labels), ctypes.byref(d), L.ptr(ws), ws.numel(), bad, L.ptr(ws), ws.numel(), L.ptr(sel), L.ptr(sel), 4,
                                      L.ptr(rows), st) == -4 and lib.dlka_load_select_workspace_bytes(ctypes.byref(d), bad) == 0
    assert lib.dlka_load_class_select(L.ptr(labels), ctypes.byref(d), L.ptr(ws), ws.numel(), host, L.ptr(ws), ws.numel(), L.ptr(sel), L.ptr(sel), 0,
                                      L.ptr(rows), st) == -4
    assert dataload.load_launch_count() == before
    assert lib.dlka_load_crop_batch(ctypes.byref(crop_desc()), L.ptr(out), L.ptr(seg_out), st) == 0
    ws2 = torch.zeros(1 << 12, dtype=torch.uint8, device=device)
    r = ctypes.byref(d)
    assert lib.dlka_load_class_counts(L.ptr(labels), r, L.ptr(ws), ws.numel(), L.ptr(totals_dev), st) == 0
    assert totals_dev.cpu().tolist()[:2] == [120, 0]
    assert lib.dlka_load_class_select(L.ptr(labels), r, L.ptr(ws), ws.numel(), host, L.ptr(ws2), ws2.numel(), L.ptr(sel), L.ptr(sel), 4, L.ptr(rows),
                                      st) == 0
    assert rows.cpu().tolist() == [[0, 0, 0]] * 4                                     # slot 0, rank 0, four times
    assert dataload.load_launch_count() == before + sum(LAUNCHES.values())
    # a rank or slot that does not exist reads nothing: (-1, -1, -1)
    sel_slot = torch.tensor([0, 1, 5, 0], dtype=torch.int32, device=device)
    sel_rank = torch.tensor([119, 0, 0, 120], dtype=torch.int32, device=device)
    assert lib.dlka_load_class_select(L.ptr(labels), r, L.ptr(ws), ws.numel(), host, L.ptr(ws2), ws2.numel(), L.ptr(sel_slot), L.ptr(sel_rank), 4,
                                      L.ptr(rows), st) == 0
    assert rows.cpu().tolist() == [[3, 4, 5], [-1, -1, -1], [-1, -1, -1], [-1, -1, -1]]


def check_patch_size(fx):
    """get_patch_size against the values recorded from the reference's function."""
    from deformablelka_amd import dataloading as D
    for args, want in fx["patch_size"]:
        got = D.get_patch_size(*args)
        assert isinstance(got, np.ndarray) and got.dtype.kind == "i" and got.tolist() == want, (args, got, want)
