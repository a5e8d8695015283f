"""TEST INFRASTRUCTURE: the checks the emulator and the GPU suites of deformablelka_amd.metrics share, against tests/golden/reference_metrics.pt
(recorded by tests/golden/make_golden_metrics.py from MedPy 0.4.0's definitions restated with scipy).

Tolerances.  Unit spacing: every squared distance is an integer below 2^53, so the sorted distance vectors and hd are EQUAL to the square roots
of the fixture's integers; hd95, asd, assd within 1e-12 relative (interpolation and summation order).  With a spacing: distances and all four
metrics within 1e-9 relative (float64 on both sides, the order of the three additions differs)."""
import os

import numpy as np
import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_metrics.pt")
UNIT_RTOL, SPACED_RTOL = 1e-12, 1e-9
# hd95 of the "diagonals" pair under connectivity 1, 2, 3 (scipy restatement): pairwise different
DIAGONALS_HD95 = {1: 11.874342087037917, 2: 11.575836902790225, 3: 11.482584970453587}
PERCENTILE_HD95 = 461.02360679774995   # between sqrt(5) and 512 at 0.95 * (3 - 1) = 1.9


def load_fixture():
    return torch.load(FIXTURE, weights_only=False)


def rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return float("inf")
    if got.size == 0:
        return 0.0
    den = np.where(want == 0, 1.0, np.abs(want))
    return float(np.max(np.abs(got - want) / den))


def check_pair(name, case, device):
    """Returns the largest relative errors seen {"dist", "hd", "hd95", "asd", "assd"}."""
    from deformablelka_amd import metrics as M
    p, q, sp = case["p"].to(device), case["q"].to(device), case["spacing"]
    assert M.dc(p, q) == case["dc"], name
    worst = dict(dist=0.0, hd=0.0, hd95=0.0, asd=0.0, assd=0.0)
    for cn, r in case["conn"].items():
        ab, ba = np.sort(M.surface_distances(p, q, sp, cn)), np.sort(M.surface_distances(q, p, sp, cn))
        got = M.surface_metrics(p, q, sp, cn)      # (what hd, hd95, asd and assd return: check_quirks)
        assert all(isinstance(v, float) for v in got.values())
        if sp is None:
            want_ab, want_ba = np.sqrt(r["sq_ab"].numpy().astype(np.float64)), np.sqrt(r["sq_ba"].numpy().astype(np.float64))
            tol = UNIT_RTOL
        else:
            want_ab, want_ba = r["sds_ab"].numpy(), r["sds_ba"].numpy()
            tol = SPACED_RTOL
        errs = {"dist": max(rel(ab, want_ab), rel(ba, want_ba))}
        errs.update({k: rel(got[k], r[k]) for k in got})
        print(f"{name} connectivity {cn}: " + ", ".join(f"{k} {v:.3g}" for k, v in errs.items()))
        if sp is None:
            assert np.array_equal(ab, want_ab) and np.array_equal(ba, want_ba), (name, cn)
            assert got["hd"] == r["hd"], (name, cn, got["hd"], r["hd"])
        for k, v in errs.items():
            assert v <= tol, (name, cn, k, v)
            worst[k] = max(worst[k], v)
    return worst


def check_labels(name, case, device, dtype):
    """evaluate_label_maps under both empty-organ conventions against per-class calls and against the fixture."""
    from deformablelka_amd import metrics as M
    pred, lab = case["prediction"].to(device=device, dtype=dtype), case["label"].to(device=device, dtype=dtype)
    sp, classes = case["spacing"], case["classes"]
    tol = UNIT_RTOL if sp is None else SPACED_RTOL
    plain = M.evaluate_label_maps(pred, lab, classes, voxelspacing=sp)
    nnunet = M.evaluate_label_maps(pred, lab, classes, voxelspacing=sp, nan_for_nonexisting=True)
    for res in (plain, nnunet):
        assert res["dice"].shape == (len(classes),) and res["dice"].dtype == np.float64 and res["hd95"].dtype == np.float64
    kinds = set()
    for i, c in enumerate(classes):
        row = case["rows"][c]
        a, b = pred == c, lab == c
        if row["a"] and row["b"]:
            kinds.add("both")
            dice = 2.0 * row["inter"] / (row["a"] + row["b"])
            assert plain["dice"][i] == dice == nnunet["dice"][i] == M.dc(a, b)
            single = M.hd95(a, b, sp, 1)
            assert plain["hd95"][i] == single == nnunet["hd95"][i]           # the batched pass and the single pair: the same bits
            assert rel(single, row["hd95"]) <= tol, (name, c, single, row["hd95"])
        elif row["a"] + row["b"] == 0:
            kinds.add("neither")
            assert plain["dice"][i] == 1.0 and plain["hd95"][i] == 0.0
            assert np.isnan(nnunet["dice"][i]) and np.isnan(nnunet["hd95"][i])
        else:
            kinds.add("one")
            assert plain["dice"][i] == 0.0 == nnunet["dice"][i] and plain["hd95"][i] == 0.0 and np.isnan(nnunet["hd95"][i])
    assert kinds == {"both", "neither", "one"}


def check_rank_is_honoured(fx, device):
    """The same slice as an image and as a volume of depth 1: in the volume every mask cell is border."""
    from deformablelka_amd import metrics as M
    flat, vol = fx["pairs"]["slice_2d"], fx["pairs"]["slice_as_depth1_volume"]
    assert torch.equal(flat["p"][None], vol["p"]) and flat["conn"][1]["hd95"] != vol["conn"][1]["hd95"]
    h2 = M.hd95(flat["p"].to(device), flat["q"].to(device))
    h3 = M.hd95(vol["p"].to(device), vol["q"].to(device))
    assert rel(h2, flat["conn"][1]["hd95"]) <= UNIT_RTOL and rel(h3, vol["conn"][1]["hd95"]) <= UNIT_RTOL and h2 != h3


def check_quirks(device):
    from deformablelka_amd import metrics as M
    z = torch.zeros((4, 5, 6), dtype=torch.uint8, device=device)
    a = z.clone()
    a[1:3, 1:4, 2:5] = 1
    b = z.clone()
    b[2:4, 2:5, 1:4] = 3
    assert M.dc(z, z) == 0.0                                       # MedPy 0.4.0: ZeroDivisionError -> 0.0
    assert M.dc(a, z) == 0.0 and M.dc(a, a) == 1.0
    assert M.dc(a, b) == 2.0 * int(((a > 0) & (b > 0)).sum()) / (int((a > 0).sum()) + int((b > 0).sum()))
    assert M.dc(a.bool(), b.cpu().numpy().astype(np.float32)) == M.dc(a, b)       # bool, float, numpy and host inputs
    keep_a, keep_b = a.clone(), b.clone()
    dice, h95 = M.calculate_metric_percase(a, b)
    assert torch.equal(a, keep_a) and torch.equal(b, keep_b)      # not written to (b holds 3s)
    assert dice == M.dc(a, b) and h95 == M.hd95(a, b) and isinstance(h95, float)
    assert M.calculate_metric_percase(a, z) == (1, 0)
    assert M.calculate_metric_percase(z, a) == (0, 0) and M.calculate_metric_percase(z, z) == (0, 0)
    neg = a.to(torch.int16) * -1                                   # utils.py binarises by > 0: a negative value is background there, foreground for medpy
    assert M.calculate_metric_percase(neg, a) == (0, 0) and M.dc(neg, a) == 1.0
    assert M.hd(a, a) == 0.0 and M.assd(a, a) == 0.0
    both = M.surface_metrics(a, b, (1.0, 2.0, 0.5), 2)
    assert both == {"hd": M.hd(a, b, (1.0, 2.0, 0.5), 2), "hd95": M.hd95(a, b, (1.0, 2.0, 0.5), 2), "asd": M.asd(a, b, (1.0, 2.0, 0.5), 2),
                    "assd": M.assd(a, b, (1.0, 2.0, 0.5), 2)}
    c = b.clone()
    c[0, 0, 5] = 3                                                 # (a and b are congruent blocks: their two directed means agree; a and c are not: the scipy restatement gives 0.9335 and 0.9755)
    assert abs(M.asd(a, c) - M.asd(c, a)) > 1e-3 and abs(M.assd(a, c) - (M.asd(a, c) + M.asd(c, a)) / 2) < 1e-15
    assert M.hd95(a, b, voxelspacing=2.0) == 2.0 * M.hd95(a, b) or abs(M.hd95(a, b, voxelspacing=2.0) - 2.0 * M.hd95(a, b)) < 1e-12


def check_errors(device):
    import pytest
    from deformablelka_amd import metrics as M
    z = torch.zeros((4, 5, 6), dtype=torch.uint8, device=device)
    a = z.clone()
    a[1, 2, 3] = 1
    for fn in (M.hd, M.hd95, M.asd, M.assd):
        with pytest.raises(RuntimeError, match="first supplied array does not contain any binary object"):
            fn(z, a)
        with pytest.raises(RuntimeError, match="second supplied array does not contain any binary object"):
            fn(a, z)
    with pytest.raises(RuntimeError, match="rank 2 or 3"):
        M.hd95(a[0, 0], a[0, 0])
    with pytest.raises(RuntimeError, match="rank 2 or 3"):
        M.dc(a[None], a[None])
    with pytest.raises(RuntimeError, match="differ in extents"):
        M.hd95(a, a[:, :, :5])
    with pytest.raises(RuntimeError, match="voxelspacing has 2 entries for rank 3"):
        M.hd95(a, a, voxelspacing=(1.0, 2.0))
    with pytest.raises(RuntimeError, match="voxelspacing must be positive"):
        M.hd95(a, a, voxelspacing=(1.0, 0.0, 1.0))
    for cn in (0, 4):
        with pytest.raises(RuntimeError, match="connectivity must be between 1 and the rank"):
            M.hd95(a, a, connectivity=cn)
    with pytest.raises(RuntimeError, match="connectivity must be between 1 and the rank"):
        M.hd95(a[0], a[0], connectivity=3)
    with pytest.raises(RuntimeError, match="uint8, int16, int32, int64 or bool"):
        M.evaluate_label_maps(a.to(torch.complex64), a.to(torch.complex64), [1])


def check_c_abi_refuses(device):
    """The library's own checks, past the Python ones: nothing is launched on a bad description or a box outside the maps."""
    import ctypes
    from deformablelka_amd import _lib as L, ops
    a = torch.ones((4, 5, 6), dtype=torch.uint8, device=device)
    stats, d, p, q = ops.sd_label_stats(a, a, [1])
    lib, before = L.get_lib(), ops.sd_launch_count()
    out = torch.empty(1024, dtype=torch.float64, device=device)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=device)

    def call(desc, box, cells=1024, ws_bytes=1 << 16):
        arr = (ctypes.c_int64 * 6)(*box)
        return lib.dlka_sd_distances(L.ptr(p), L.ptr(q), ctypes.byref(desc), arr, L.ptr(ws), ws_bytes, L.ptr(out), cells, L.stream_ptr(p))

    for field, value, code in (("rank", 4, -4), ("connectivity", 4, -8), ("connectivity", 0, -8), ("label_dtype", 7, -6), ("K", 0, -8), ("K", 33, -8)):
        bad = L.SurfaceDistDesc.from_buffer_copy(d)
        setattr(bad, field, value)
        assert call(bad, [0, 0, 0, 4, 5, 6]) == code, field
        assert lib.dlka_sd_stats_workspace_bytes(ctypes.byref(bad)) == 0
    assert call(d, [0, 0, 0, 4, 5, 7]) == -4 and call(d, [0, 0, 1, 4, 5, 6]) == -4 and call(d, [-1, 0, 0, 4, 5, 6]) == -4
    assert call(d, [0, 0, 0, 4, 5, 6], cells=239) == -4 and call(d, [0, 0, 0, 4, 5, 6], ws_bytes=100) == -7
    assert ops.sd_launch_count() == before
    assert call(d, [0, 0, 0, 4, 5, 6]) == 0 and ops.sd_launch_count() == before + 3


def check_reproducible(fx, device):
    from deformablelka_amd import metrics as M, ops
    case = fx["labels"]["synapse_aniso"]
    pred, lab = case["prediction"].to(device), case["label"].to(device)
    before = ops.sd_launch_count()
    runs = []
    for _ in range(2):
        stats, d, p, q = ops.sd_label_stats(pred, lab, case["classes"], list(case["spacing"]), 1)
        st = stats.cpu()
        boxes = [list(r[3:6]) + list(r[6:9] - r[3:6] + 1) if r[1] > 0 and r[2] > 0 else [0] * 6 for r in st.numpy()]
        sq, _ = ops.sd_distances(p, q, d, boxes)
        runs.append((st, sq.cpu()))
    assert ops.sd_launch_count() == before + 10        # the HIP path ran: 2 + 3 launches per run
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    a, b = M.evaluate_label_maps(pred, lab, case["classes"], case["spacing"]), M.evaluate_label_maps(pred, lab, case["classes"], case["spacing"])
    assert a["hd95"].tobytes() == b["hd95"].tobytes() and a["dice"].tobytes() == b["dice"].tobytes()
