"""TEST INFRASTRUCTURE — the cases and checks of deformablelka_amd.preprocessing, shared by tests/test_preprocessing_emu.py (wavefront emulator,
CPU suite) and tests/test_preprocessing_gpu.py (MI355X).  The expected results are in tests/golden/reference_preprocessing.pt, recorded by
tests/golden/make_golden_preprocessing.py from the reference's own cropping.py and preprocessing.py.

The INPUTS are not stored: they are rebuilt here by formula (the integer hash of tests/resampling_cases.py, IEEE additions, multiplications and
divisions only), so they are the same bits on every machine; the fixture holds their SHA-256 and every check compares it first.

Bounds (the issue's).  Mask, box, cropped data, cropped seg, classes, size_after_*: equality; seg after the pipeline: equality.  CT on
unresampled data: bitwise.  CT2 / nonCT: the count equals the reference's; |mean - m64| and |sd - s64| <= 1e-12 (|m64| + s64) against numpy's
float64 values (float64 summation error at 25 000 terms is about 25000 * 1.1e-16 = 3e-12 relative in the worst case and about sqrt of that in
fixed-order folds: a wide margin); the output is bitwise the float32 formula evaluated in numpy with the returned mean and sd, and within
1e-5 max|out| of the reference's output (numpy's float32 pairwise sums err by about log2(n) 6e-8 relative; the recorder measured the gap per
call, stored it as f64_gap and refused a fixture beyond the bound).  Pipeline data, with delta = 1e-6 max|cropped data| (the order-3 bound of
tests/resampling_cases.py): CT delta / sd + 2 float32 ulps of the value; nonCT (2 + max|out|) delta / sd + 2 ulps."""
import copy
import os

import numpy as np
import torch

from tests.resampling_cases import digest, noise, smooth

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "reference_preprocessing.pt")
STAT_BOUND = 1e-12
GAP_BOUND = 1e-5
POCKET_CELLS = 2 * 4 * 17
LAUNCHES = {"background": 1, "fill_bbox": 3, "mask_bbox": 2, "crop": 1, "channel_stats": 4, "normalize": 1}   # csrc/cl_preprocess.hip
CC_LAUNCHES = 6


def load_fixture():
    return torch.load(FIXTURE, weights_only=False)


# ---- cropping cases: name -> (data float32 (c, *spatial), seg float32 (1, *spatial) or None) ----------------------------------------------------
def _random2():
    shape = (5, 37, 130)
    n0, n1 = noise((1,) + shape, 11)[0], noise((1,) + shape, 12)[0]
    x = np.zeros((2,) + shape, np.float32)
    x[0] = np.where(n0 > 0.25, 1.0 + 100.0 * n0, 0.0)
    x[1] = np.where(n1 > 0.6, -50.0 * n1, 0.0)
    x[:, 1:4, 5:11, 57:71] = 5.0
    x[:, 2, 6:10, 58:70] = 0.0                 # an enclosed pocket of 48 cells across the tile faces h = 8 and w = 64 ...
    x[1, 2, 7, 60] = np.nan                    # ... one of them a NaN: != 0, not background
    x[:, 1:4, 20:27, 100:121] = 7.0
    x[:, 2, 21:26, 101:120] = 0.0              # a pocket of the same kind ...
    x[:, 2, 23, 101:130] = 0.0                 # ... open to the margin through a corridor
    x[:, 0], x[:, -1] = 0.0, 0.0               # the margin: the box lies strictly inside
    x[:, :, :2], x[:, :, -3:] = 0.0, 0.0
    x[..., :3], x[..., -2:] = 0.0, 0.0
    return x, None


def _pocket(kind):
    x = np.zeros((1, 6, 19, 75), np.float32)
    x[0, 1:5, 1:18, 1:74] = 3.0
    x[0, 2:4, 2:6, 2:19] = 0.0                 # the cavity: POCKET_CELLS cells
    if kind == "leaks":                        # a one-cell corridor along h (across h = 8), then along w (across w = 64) to the margin
        x[0, 2, 6:16, 18] = 0.0
        x[0, 2, 15, 18:75] = 0.0
    if kind == "diagonal":                     # (2, 1, 1) is open to the margin and meets the cavity cell (2, 2, 2) across an edge only
        x[0, 2, 1, 1] = 0.0
    return x, None


def _touches_every_face():
    x = np.full((1, 4, 9, 70), 2.0, np.float32)
    x[0, 1:3, 3:6, 10:60] = 0.0
    return x, None


def _depth_one():
    x = np.zeros((1, 1, 33, 70), np.float32)
    x[0, 0, 5:28, 6:64] = 1.0
    x[0, 0, 8:25, 9:61] = 0.0                  # a hole of the plane; in three dimensions every cell lies on a face
    return x, None


def _planar():
    x = np.zeros((2, 67, 131), np.float32)
    x[0, 5:30, 7:120] = 1.0
    x[0, 8:27, 10:117] = 0.0                   # a closed ring: filled
    x[0, 35:62, 7:120] = 4.0
    x[0, 38:59, 10:117] = 0.0
    x[0, 45, 7:10] = 0.0                       # an open ring: not filled
    n = noise((1, 67, 131), 13)[0]
    x[1, 10:25, 20:100] = np.where(n > 0.6, n, 0.0)[10:25, 20:100]
    return x, None


def _single_cell():
    x = np.zeros((1, 5, 9, 11), np.float32)
    x[0, 3, 4, 7] = -2.5
    return x, None


def _all_zero():
    return np.zeros((1, 3, 5, 7), np.float32), None


def _with_seg():
    shape = (6, 10, 22)                        # 1320 cells, a multiple of 4: two channels on the 16-byte path
    n = noise((2,) + shape, 14)
    x = np.zeros((2,) + shape, np.float32)
    x[:, 1:5, 1:9, 2:20] = (1.0 + n)[:, 1:5, 1:9, 2:20]
    x[:, 2:4, 3:6, 5:12] = 0.0                 # enclosed: inside the mask
    x[:, 3, 4, 20] = 1.0                       # one cell widens the box: the column w = 20 is outside the mask elsewhere
    seg = np.floor(noise((1,) + shape, 15) * 4.0).astype(np.float32)
    seg[0, 2, 2, 3] = -2.0
    return x, seg


CROP_CASES = {
    "random2": _random2, "pocket_leaks": lambda: _pocket("leaks"), "pocket_diagonal": lambda: _pocket("diagonal"),
    "pocket_closed": lambda: _pocket("closed"), "touches_every_face": _touches_every_face, "depth_one": _depth_one, "planar": _planar,
    "single_cell": _single_cell, "all_zero": _all_zero, "with_seg": _with_seg,
}

# ---- normalisation calls on (3, 9, 21, 40) ------------------------------------------------------------------------------------------------------
CT_PROPS = {'mean': 77.5, 'sd': 142.1, 'percentile_00_5': -958.0, 'percentile_99_5': 326.7}
BIG_PROPS = {'mean': 1000.2, 'sd': 1.1, 'percentile_00_5': 998.5, 'percentile_99_5': 1001.6}
INTENSITY = {0: CT_PROPS, 1: CT_PROPS, 2: BIG_PROPS}
NORM_SHAPE = (3, 9, 21, 40)


def normalize_input():
    n = noise(NORM_SHAPE, 21)
    x = np.zeros(NORM_SHAPE, np.float32)
    x[:2] = ((smooth(n[:2]) - 0.5) * 4000.0).astype(np.float32)          # beyond both percentiles in places
    # mean about 1000, sd about 1: the cancellation case.  In steps of 0.5, so that numpy's float32 sums of the reference are exact and its
    # float32 mean is the rounded exact mean: one float32 ulp of a mean near 1000 is 6.1e-5, which alone is 3.4e-5 max|out| here, so against a
    # reference whose mean is an ulp off NO implementation could hold GAP_BOUND (the recorder met exactly that gap on unquantised values).
    x[2] = (1000.0 + np.floor((n[2] - 0.5) * 7.0 + 0.5) / 2.0).astype(np.float32)
    seg = np.floor(noise((1,) + NORM_SHAPE[1:], 22) * 3.0).astype(np.float32)
    seg[0, :, :4, :] = -1.0
    seg[0, :2] = -1.0
    return x, seg


# (id, schemes, use_nonzero_mask)
NORM_CALLS = [
    ("plain", ("CT", "CT2", "nonCT"), (False, False, False)),
    ("masked", ("CT", "CT2", "nonCT"), (True, True, True)),
    ("rotated", ("nonCT", "CT", "CT2"), (True, False, True)),
]

# ---- pipeline calls: id -> (shape, original spacing, target spacing (transposed), transpose_forward, schemes, use mask, with seg) ---------------
PIPE_CALLS = {
    "synapse": ((1, 12, 40, 44), (3.0, 0.76, 0.76), (2.0, 1.0, 1.0), [0, 1, 2], ("CT",), (False,), False),
    "two_modalities": ((2, 14, 20, 22), (1.0, 1.0, 1.0), (1.25, 1.25, 1.25), [0, 1, 2], ("nonCT", "nonCT"), (True, True), True),
    "transposed": ((1, 10, 18, 24), (1.0, 0.8, 0.9), (1.0, 1.0, 1.2), [2, 0, 1], ("CT",), (True,), False),
}


def pipeline_input(cid):
    shape, _, _, _, _, _, with_seg = PIPE_CALLS[cid]
    salt = 31 + list(PIPE_CALLS).index(cid)
    v = ((smooth(noise(shape, salt)) - 0.5) * 2000.0).astype(np.float32)
    d, h, w = shape[1:]
    zz, yy, xx = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    body = ((yy - (h - 1) / 2.0) / (h / 2.0 - 2.0)) ** 2 + ((xx - (w - 1) / 2.0) / (w / 2.0 - 3.0)) ** 2 <= 1.0
    body &= (zz >= 1) & (zz < d - 1)
    x = np.where(body[None] & (v != 0), v, np.float32(0.0)).astype(np.float32)
    x[:, d // 2, h // 2 - 2:h // 2 + 2, w // 2 - 3:w // 2 + 3] = 0.0      # an enclosed pocket
    if cid == "two_modalities":
        x[1, d // 2, h // 2, w // 2] = np.nan                             # removed after the crop (preprocessing.py:250)
    seg = np.floor(noise((1,) + shape[1:], salt + 50) * 3.0).astype(np.float32) if with_seg else None
    return x, seg


def preprocessor(P, transpose_forward, schemes, use_mask, intensity=None):
    n = len(schemes)
    return P.GenericPreprocessor({c: schemes[c] for c in range(n)}, {c: use_mask[c] for c in range(n)}, transpose_forward,
                                 {c: (intensity or INTENSITY)[c] for c in range(n)})


# ---- helpers ------------------------------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    """Equality of float32 arrays bit for bit (NaN cells included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))


def to_np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def on(device, x):
    return None if x is None else torch.from_numpy(x.copy()).to(device)


# ---- checks -------------------------------------------------------------------------------------------------------------------------------------
def check_crop(name, rec, device):
    import pytest
    from deformablelka_amd import preprocessing as P
    data, seg = CROP_CASES[name]()
    assert digest(data) == rec["input"] and (seg is None or digest(seg) == rec["seg_input"]), name
    t, s = on(device, data), on(device, seg)
    if name == "all_zero":
        assert rec["raises"] == "ValueError"
        for call in (lambda: P.crop_to_nonzero(t), lambda: P.ImageCropper.crop(t, {"original_spacing": (1, 1, 1)}),
                     lambda: P.get_bbox_from_mask(torch.zeros((3, 5, 7), dtype=torch.bool, device=device))):
            with pytest.raises(ValueError):
                call()
        assert not bool(P.create_nonzero_mask(t).any())
        return
    mask = P.create_nonzero_mask(t)
    assert mask.dtype == torch.bool and mask.device == t.device and mask.shape == t.shape[1:]
    assert torch.equal(mask.cpu(), rec["mask"].to(torch.bool)), name
    bbox = P.get_bbox_from_mask(mask, 0)
    assert bbox == rec["bbox"] and all(type(v) is int for b in bbox for v in b), (name, bbox, rec["bbox"])
    want = rec["mask"].numpy()[tuple(slice(lo, hi) for lo, hi in bbox)]
    assert np.array_equal(to_np(P.crop_to_bbox(mask, bbox)), want.astype(bool))
    for label, key in ((-1, "crop"), (-7, "crop_label_m7")):
        out, sout, box = P.crop_to_nonzero(t, s, label)
        assert box == rec["bbox"] and out.device == t.device and sout.device == t.device
        assert same_bits(to_np(out), rec["crop"]["data"].numpy()), (name, label)
        assert np.array_equal(to_np(sout).astype(np.int64), rec[key]["seg"].numpy().astype(np.int64)), (name, label)
        assert sout.dtype == (torch.int64 if s is None else s.dtype)
    props = {"original_spacing": np.array([1.0, 1.0, 1.0]), "keep": [1, 2]}
    props_before = copy.deepcopy(props)
    out, sout, got = P.ImageCropper.crop(t, props, s)
    assert same_bits(to_np(out), rec["crop"]["data"].numpy())
    assert np.array_equal(to_np(sout).astype(np.int64), rec["cropper"]["seg"].numpy().astype(np.int64)), name
    assert got["crop_bbox"] == rec["bbox"] and isinstance(got["classes"], np.ndarray)
    assert got["classes"].astype(np.int64).tolist() == rec["cropper"]["classes"], (name, got["classes"])
    assert tuple(got["size_after_cropping"]) == tuple(rec["cropper"]["size_after_cropping"]) and got["keep"] is props["keep"]
    assert set(props.keys()) == set(props_before.keys()) and np.array_equal(props["original_spacing"], props_before["original_spacing"])
    assert same_bits(to_np(t), data) and (s is None or np.array_equal(to_np(s), seg))            # the arguments are untouched (NaN included)


def run_normalize(P, call, device):
    cid, schemes, use_mask = call
    data, seg = normalize_input()
    t, s = on(device, data), on(device, seg)
    pre = preprocessor(P, [0, 1, 2], schemes, use_mask)
    out, stats = pre.normalize(t, s)
    assert same_bits(to_np(t), data) and np.array_equal(to_np(s), seg)
    return data, seg, out, stats, pre, t, s


def check_normalize(call, rec, device):
    from deformablelka_amd import preprocessing as P
    from tests import preprocessing_ref as R
    cid, schemes, use_mask = call
    data, seg, out, stats, pre, t, s = run_normalize(P, call, device)
    assert digest(data) == rec["input"] and digest(seg) == rec["seg_input"]
    assert out.dtype == torch.float32 and out.device == t.device and stats.dtype == torch.float64 and tuple(stats.shape) == (3, 3)
    got, st, ref = to_np(out), to_np(stats), rec["out"].numpy()
    assert rec["f64_gap"] <= GAP_BOUND
    for c, scheme in enumerate(schemes):
        p = INTENSITY[c]
        lower, upper = p['percentile_00_5'], p['percentile_99_5']
        if scheme == "CT":
            print(f"{cid} ch{c} CT: cells that differ from the reference: {int((got[c].view(np.int32) != ref[c].view(np.int32)).sum())}")
            assert same_bits(got[c], ref[c]), (cid, c)
            assert same_bits(got[c], R.formula32(data[c], seg[-1], scheme, use_mask[c], lower, upper, p['mean'], p['sd']))
            continue
        count, m64, s64 = R.statistics64(data[c], seg[-1], scheme, use_mask[c], np.float32(lower), np.float32(upper))
        n, mean, sd = int(st[c, 0]), float(st[c, 1]), float(st[c, 2])
        tol = STAT_BOUND * (abs(m64) + s64)
        print(f"{cid} ch{c} {scheme}: count {n} / {count}, |mean - m64| {abs(mean - m64):.3e}, |sd - s64| {abs(sd - s64):.3e}, bound {tol:.3e}")
        assert n == count == rec["counts"][c] and count > 100, (cid, c, n, count, rec["counts"][c])
        assert abs(mean - m64) <= tol and abs(sd - s64) <= tol, (cid, c, mean - m64, sd - s64, tol)
        assert same_bits(got[c], R.formula32(data[c], seg[-1], scheme, use_mask[c], lower, upper, mean, sd)), (cid, c)
        gap = float(np.abs(got[c].astype(np.float64) - ref[c]).max())
        print(f"{cid} ch{c} {scheme}: max |out - reference| {gap:.3e}, bound {GAP_BOUND * float(np.abs(got[c]).max()):.3e}")
        assert gap <= GAP_BOUND * float(np.abs(got[c]).max()), (cid, c, gap)
    # the public entry with nothing to resample: the same bits, seg below -1 mapped, properties copied
    props = {"original_spacing": np.array([1.0, 1.0, 1.0])}
    out2, seg2, got_props = pre.resample_and_normalize(t, (1.0, 1.0, 1.0), props, s)
    assert same_bits(to_np(out2), got) and np.array_equal(to_np(seg2), rec["seg"].numpy()) and seg2.dtype == s.dtype
    assert tuple(got_props["size_after_resampling"]) == NORM_SHAPE[1:] and got_props["spacing_after_resampling"] == (1.0, 1.0, 1.0)
    assert "size_after_resampling" not in props


def run_pipeline(P, cid, device, as_numpy=False):
    shape, original, target, tf, schemes, use_mask, with_seg = PIPE_CALLS[cid]
    data, seg = pipeline_input(cid)
    pre = preprocessor(P, tf, schemes, use_mask, {c: CT_PROPS for c in range(len(schemes))})
    props = {"original_spacing": np.array(original), "original_size_of_raw_data": np.array(shape[1:])}
    args = (data.copy(), seg if seg is None else seg.copy()) if as_numpy else (on(device, data), on(device, seg))
    out, sout, got = pre.preprocess_arrays(args[0], target, props, args[1])
    assert same_bits(to_np(args[0]), data) and (seg is None or np.array_equal(to_np(args[1]), seg))
    assert set(props.keys()) == {"original_spacing", "original_size_of_raw_data"}
    return data, seg, out, sout, got


def check_pipeline(cid, rec, device):
    from deformablelka_amd import preprocessing as P
    shape, original, target, tf, schemes, use_mask, with_seg = PIPE_CALLS[cid]
    data, seg, out, sout, got = run_pipeline(P, cid, device)
    assert digest(data) == rec["input"]
    assert out.dtype == torch.float32 and out.device.type == torch.device(device).type and sout.device == out.device
    ref, o = rec["data"].numpy(), to_np(out)
    assert o.shape == ref.shape and np.array_equal(to_np(sout).astype(np.int64), rec["seg"].numpy().astype(np.int64)), cid
    assert got["crop_bbox"] == rec["crop_bbox"] and got["classes"].astype(np.int64).tolist() == rec["classes"]
    assert tuple(got["size_after_cropping"]) == tuple(rec["size_after_cropping"])
    assert tuple(got["size_after_resampling"]) == tuple(rec["size_after_resampling"]) == ref.shape[1:]
    assert tuple(got["spacing_after_resampling"]) == tuple(target)
    delta = 1e-6 * rec["max_cropped"]
    for c, scheme in enumerate(schemes):
        sd = CT_PROPS['sd'] if scheme == "CT" else rec["sd"][c]
        factor = 1.0 if scheme == "CT" else 2.0 + float(np.abs(o[c]).max())
        bound = factor * delta / sd + 2.0 * np.spacing(np.abs(ref[c]))
        err = np.abs(o[c].astype(np.float64) - ref[c])
        print(f"{cid} ch{c} {scheme}: max error {float(err.max()):.3e}, smallest bound {float(bound.min()):.3e}, worst ratio "
              f"{float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), (cid, c, float((err / bound).max()))


def check_reproducible(fx, device):
    """Two runs: masks, boxes, crops, statistics and normalised data are the same bits."""
    from deformablelka_amd import ops, preprocessing as P
    for name in ("random2", "planar", "with_seg"):
        data, seg = CROP_CASES[name]()
        t = on(device, data)
        s = None if seg is None else on(device, seg).to(torch.int32)
        runs = []
        for _ in range(2):
            mask, box = ops.prep_nonzero_mask(t)
            bbox = P._box_list(box, t.ndim - 1)
            out, sout = ops.prep_crop(t, s, mask, bbox, -1, True)
            runs.append([mask.cpu(), box.cpu()[:7], out.cpu().view(torch.int32), sout.cpu()])
        assert all(torch.equal(a, b) for a, b in zip(*runs)), name
    for call in NORM_CALLS:
        a = run_normalize(P, call, device)
        b = run_normalize(P, call, device)
        assert same_bits(to_np(a[2]), to_np(b[2])) and np.array_equal(to_np(a[3]).view(np.int64), to_np(b[3]).view(np.int64)), call[0]


def check_containers(fx, device):
    """numpy in, numpy out; a host tensor in, a host tensor out; other dtypes are converted in the wrapper."""
    from deformablelka_amd import preprocessing as P
    rec = fx["crop"]["with_seg"]
    data, seg = CROP_CASES["with_seg"]()
    for dtype in (np.float32, np.float64, np.int16):
        arr = (data * 8.0).astype(dtype) if dtype == np.int16 else data.astype(dtype)
        sarr = seg.astype(np.int16)
        before, sbefore = arr.copy(), sarr.copy()
        mask = P.create_nonzero_mask(arr)
        assert isinstance(mask, np.ndarray) and mask.dtype == bool and np.array_equal(mask, rec["mask"].numpy().astype(bool))
        assert P.get_bbox_from_mask(mask) == rec["bbox"]
        out, sout, bbox = P.crop_to_nonzero(arr, sarr)
        assert isinstance(out, np.ndarray) and out.dtype == dtype and sout.dtype == np.int16 and bbox == rec["bbox"]
        assert np.array_equal(sout, rec["crop"]["seg"].numpy().astype(np.int16))
        want = rec["crop"]["data"].numpy()
        assert np.array_equal(out, (want * 8.0).astype(dtype) if dtype == np.int16 else want.astype(dtype))
        assert np.array_equal(arr, before) and np.array_equal(sarr, sbefore)
    host = torch.from_numpy(data.copy())
    out, sout, _ = P.crop_to_nonzero(host)
    assert out.device.type == "cpu" and sout.dtype == torch.int64 and same_bits(out.numpy(), rec["crop"]["data"].numpy())
    cid = "two_modalities"
    d0, s0, out, sout, props = run_pipeline(P, cid, device, as_numpy=True)
    assert isinstance(out, np.ndarray) and out.dtype == np.float32 and isinstance(sout, np.ndarray) and sout.dtype == s0.dtype
    _, _, out_t, sout_t, _ = run_pipeline(P, cid, device)
    assert same_bits(out, to_np(out_t)) and np.array_equal(sout, to_np(sout_t))


def check_errors(device):
    import pytest
    from deformablelka_amd import preprocessing as P
    x = torch.ones((1, 2, 3, 4, 5), device=device)
    for call in (lambda: P.create_nonzero_mask(x), lambda: P.crop_to_nonzero(x), lambda: P.create_nonzero_mask(x[0, 0, 0]),
                 lambda: P.get_bbox_from_mask(x[0] != 0), lambda: P.PreprocessorFor2D, lambda: P.ImageCropper(1, "/tmp/x"),
                 lambda: P.ImageCropper(1).load_crop_save, lambda: preprocessor(P, [0, 1, 2], ("CT",), (False,)).run,
                 lambda: preprocessor(P, [0, 1, 2], ("CT",), (False,)).preprocess_arrays(x[0, 0], (1, 1), {"original_spacing": (1, 1)})):
        with pytest.raises(NotImplementedError):
            call()
    pre = preprocessor(P, [0, 1, 2], ("CT", "CT2"), (False, False))
    with pytest.raises(AssertionError, match="as many entries as data"):
        pre.resample_and_normalize(x[0, :1], (1, 1, 1), {"original_spacing": (1, 1, 1)}, torch.zeros((1, 3, 4, 5), device=device))
    with pytest.raises(AssertionError, match="intensity properties"):
        P.GenericPreprocessor({0: "CT"}, {0: False}, [0, 1, 2]).normalize(x[0, :1])
    try:
        import SimpleITK  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="SimpleITK"):
            pre.preprocess_test_case(["a.nii.gz"], (1, 1, 1))


def check_c_abi_refuses(device):
    """The library's own checks, past the Python ones: nothing is launched on a bad description."""
    import ctypes
    from deformablelka_amd import _lib as L, ops
    x = torch.ones((2, 4, 5, 6), dtype=torch.float32, device=device)
    seg = torch.zeros((4, 5, 6), dtype=torch.int32, device=device)
    mask, box = ops.prep_nonzero_mask(x)
    labels = torch.zeros((4, 5, 6), dtype=torch.int32, device=device)
    bgmap = torch.zeros_like(mask)
    out = torch.empty_like(x)
    d, _ = ops._prep_desc(x)
    for ax in range(3):
        d.lo[ax], d.hi[ax] = 0, d.ext[ax]
    table = torch.zeros((2, L.DLKA_PREP_REC), dtype=torch.float64, device=device)
    table[:, 0] = L.DLKA_PREP_NONCT
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=device)
    lib, st, before = L.get_lib(), L.stream_ptr(x), ops.prep_launch_count()
    null = ctypes.c_void_p(0)

    def entries(desc, data=L.ptr(x), o=L.ptr(out), w=ws.numel()):
        r = ctypes.byref(desc)
        bgp = L.ptr(bgmap) if data.value else null
        return [lib.dlka_prep_background(data, r, L.ptr(mask), st),
                lib.dlka_prep_fill_bbox(bgp, L.ptr(labels), r, L.ptr(ws), w, L.ptr(mask), L.ptr(box), st),
                lib.dlka_prep_mask_bbox(bgp, r, L.ptr(box), st),
                lib.dlka_prep_crop(data, null, L.ptr(mask), r, o, null, st),
                lib.dlka_prep_channel_stats(data, L.ptr(seg), r, L.ptr(table), L.ptr(ws), w, st),
                lib.dlka_prep_normalize(data, L.ptr(seg), r, L.ptr(table), o, st)]

    def bad(**fields):
        b = L.PrepDesc.from_buffer_copy(d)
        for k, v in fields.items():
            if isinstance(v, tuple):
                getattr(b, k)[v[0]] = v[1]
            else:
                setattr(b, k, v)
        return b

    for fields, code in (({"rank": 4}, -4), ({"rank": 1}, -4), ({"ext": (1, 0)}, -4), ({"ext": (2, -3)}, -4), ({"C": 0}, -4),
                         ({"C": L.DLKA_PREP_C_MAX + 1}, -8), ({"ext": (0, 1 << 31)}, -8)):
        b = bad(**fields)
        assert entries(b) == [code] * 6, fields
        assert lib.dlka_prep_fill_workspace_bytes(ctypes.byref(b)) == 0 and lib.dlka_prep_stats_workspace_bytes(ctypes.byref(b)) == 0
    assert entries(bad(rank=2))[0] == -4                                           # rank 2 with a depth of 4
    assert entries(d, data=null) == [-1] * 6                                       # null pointers
    assert lib.dlka_prep_crop(L.ptr(x), null, L.ptr(mask), ctypes.byref(bad(hi=(1, 6))), L.ptr(out), null, st) == -4   # a box outside the array
    assert lib.dlka_prep_crop(L.ptr(x), null, L.ptr(mask), ctypes.byref(bad(lo=(2, 6))), L.ptr(out), null, st) == -4   # an empty box
    assert lib.dlka_prep_crop(L.ptr(x), null, L.ptr(mask), ctypes.byref(d), L.ptr(x), null, st) == -8
    assert lib.dlka_prep_crop(L.ptr(x), null, null, ctypes.byref(d), L.ptr(out), L.ptr(labels), st) == -1               # a label map without a mask
    r = ctypes.byref(d)
    assert lib.dlka_prep_fill_bbox(L.ptr(bgmap), L.ptr(labels), r, L.ptr(ws), 8, L.ptr(mask), L.ptr(box), st) == -7     # workspaces too small
    assert lib.dlka_prep_channel_stats(L.ptr(x), L.ptr(seg), r, L.ptr(table), L.ptr(ws), 8, st) == -7
    assert ops.prep_launch_count() == before
    assert entries(d) == [0] * 6 and ops.prep_launch_count() == before + sum(LAUNCHES.values())


def check_launch_count(device):
    """Launches per entry point, whatever the extents."""
    from deformablelka_amd import ops, preprocessing as P
    per_mask = LAUNCHES["background"] + LAUNCHES["fill_bbox"]
    for name in ("single_cell", "random2", "planar"):
        data, _ = CROP_CASES[name]()
        t = on(device, data)
        before, cc = ops.prep_launch_count(), ops.cc_launch_count()
        mask = P.create_nonzero_mask(t)
        assert ops.prep_launch_count() == before + per_mask and ops.cc_launch_count() == cc + CC_LAUNCHES, name
        P.get_bbox_from_mask(mask)
        assert ops.prep_launch_count() == before + per_mask + LAUNCHES["mask_bbox"]
        P.crop_to_nonzero(t)
        assert ops.prep_launch_count() == before + 2 * per_mask + LAUNCHES["mask_bbox"] + LAUNCHES["crop"], name
    for call in NORM_CALLS:
        before = ops.prep_launch_count()
        run_normalize(P, call, device)
        assert ops.prep_launch_count() == before + LAUNCHES["channel_stats"] + LAUNCHES["normalize"]
    before = ops.prep_launch_count()
    run_pipeline(P, "synapse", device)                                             # CT alone: no statistics
    assert ops.prep_launch_count() == before + per_mask + LAUNCHES["crop"] + LAUNCHES["normalize"]
