"""TEST INFRASTRUCTURE — the cases and checks of deformablelka_amd.dataset_analysis, shared by tests/test_dataset_analysis_emu.py (wavefront
emulator, CPU suite) and tests/test_dataset_analysis_gpu.py (MI355X).  The expected results are in tests/golden/reference_dataset_analysis.pt,
recorded by tests/golden/make_golden_dataset_analysis.py from the reference's own DatasetAnalyzer._compute_stats,
_check_if_all_in_one_region, _collect_class_and_region_sizes, collect_intensity_properties and analyze_dataset.

The INPUTS are not stored: they are rebuilt here by formula (the integer hash of tests/resampling_cases.py), the same bits on every machine.

Bounds (the issue's).  EQUALITY, dtype included, for the foreground sample, the order statistics, mn, mx, the median and both percentiles,
against numpy on the same list and against the reference's recorded values; a zero compares by value (the selection returns +0.0 for either
zero).  Count exact.  |mean - m64| and |sd - s64| <= STAT_BOUND (|m64| + s64) against numpy's float64 values of the same sample
(tests/preprocessing_cases.py: 1e-12), and within the gap the recorder measured between the reference's float32 mean / sd and those float64
values plus one float32 ulp; the recorder refused a fixture whose gap exceeds GAP_BOUND (|m64| + s64) (1e-5).  The chain: GAP_BOUND max|out|.

Quantile neighbours: the issue names n = 200, 201 and 1001 and asks that the interpolation weight g be nonzero in at least two.  numpy's
virtual index is FLOAT32 for a float32 sample ((n - 1) * float32(q / 100)): it is 199.0 and 1.0 for n = 201, 995.0 and 5.0 for n = 1001,
so g = 0 in both; only n = 200 interpolates (g = 0.005005 and 0.995).  The three stay and n = 130 (g = 0.355, 0.645) and n = 1445 (g = 0.780,
0.220) join them; check_quantile_weights asserts all of this."""
import ctypes
import os
from collections import OrderedDict

import numpy as np
import torch

from tests.preprocessing_cases import GAP_BOUND, STAT_BOUND
from tests.resampling_cases import digest, noise

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "reference_dataset_analysis.pt")
LAUNCHES = {"fg_count": 2, "fg_sample": 1, "moments": 4, "select": 9, "unique_labels": 1}      # csrc/cl_dataset_stats.hip
STATS_LAUNCHES = LAUNCHES["moments"] + LAUNCHES["select"]
VPV = 0.75 * 0.75 * 3.0
KEYS = ("median", "mean", "sd", "mn", "mx", "percentile_99_5", "percentile_00_5")


def load_fixture():
    return torch.load(FIXTURE, weights_only=False)


def to_np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def on(device, a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(device)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))


def same_value(a, b):
    """float32 scalars: the same bits; two NaNs; or two zeros (the selection canonicalises -0.0)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != np.float32 or b.dtype != np.float32:
        return False
    if np.isnan(a) and np.isnan(b):
        return True
    if a == 0 and b == 0:
        return True
    return a.view(np.int32) == b.view(np.int32)


def same_values(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and all(same_value(x, y) for x, y in zip(a.ravel(), b.ravel()))


# ---- foreground cases: (2 modalities + label map, *spatial) float32 ----------------------------------------------------------------------------------
def _volumes(shape, salt, channels=2):
    x = np.empty((channels,) + tuple(shape), np.float32)
    x[0] = (noise(shape, salt) * 1400.0 - 1000.0).astype(np.float32)          # CT-like
    for c in range(1, channels):
        x[c] = ((noise(shape, salt + 10 * c) - 0.5) * 7.0).astype(np.float32)
    return x


def exact_count_case(shape, count, salt):
    """Exactly ``count`` foreground cells (labels 1..3) scattered by hash; the other cells are -1 or 0."""
    n = int(np.prod(shape))
    order = np.argsort(noise((n,), salt + 1), kind="stable")[:count]
    seg = np.where(noise((n,), salt + 2) < 0.5, -1.0, 0.0)
    seg[order] = 1.0 + (order % 3)
    return np.concatenate([_volumes(shape, salt), seg.reshape((1,) + tuple(shape)).astype(np.float32)])


def scattered_case(shape, salt, p=0.3):
    u = noise(shape, salt + 3)
    seg = np.select([u < p / 2, u < p, u < 0.6], [1.0, 2.0, -1.0], 0.0)
    return np.concatenate([_volumes(shape, salt), seg[None].astype(np.float32)])


def box_case():
    """One solid box over tile borders (a wave owns 2048 consecutive cells; a row of this shape has 130)."""
    shape = (5, 37, 130)
    seg = np.where(noise(shape, 77) < 0.3, -1.0, 0.0)
    seg[1:4, 5:30, 20:120] = 2.0
    return np.concatenate([_volumes(shape, 7), seg[None].astype(np.float32)])


COUNTS = (0, 1, 9, 10, 11, 63, 64, 65, 641)
FG_CASES = OrderedDict()
for _s, _shape in enumerate(((3, 5, 70), (5, 37, 130))):
    for _c in COUNTS:
        FG_CASES[f"count{_c}_{'x'.join(map(str, _shape))}"] = (lambda sh=_shape, c=_c, s=_s: exact_count_case(sh, c, 100 * s + c))
    FG_CASES[f"scattered_{'x'.join(map(str, _shape))}"] = (lambda sh=_shape, s=_s: scattered_case(sh, 31 + s))
FG_CASES["box_5x37x130"] = box_case
FG_CASES["rank2_33x129"] = lambda: scattered_case((33, 129), 41)


def check_foreground(name, rec, device):
    from deformablelka_amd import dataset_analysis as A
    from tests import dataset_analysis_ref as R
    case = FG_CASES[name]()
    seg = case[-1]
    count = int((seg > 0).sum())
    assert count == rec["count"] and (seg == -1).any() and (seg == 0).any() and (count == 0 or (seg > 0).any())
    pair = (on(device, case[:-1]), on(device, seg[None].astype(np.int32)))               # as ImageCropper.crop returns a case
    for mod in (0, 1):
        want = R.foreground_voxels(case, mod)
        assert digest(want) == rec["samples"][mod] and len(want) == -(-count // 10)
        t = on(device, case)
        for got in (A.foreground_voxels(t, mod), A.foreground_voxels(pair, mod)):
            assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and got.device.type == torch.device(device).type
            assert same_bits(to_np(got), want), (name, mod)
        assert same_bits(to_np(t), case)
    for step in (1, 3):
        assert same_bits(to_np(A.foreground_voxels(on(device, case), 0, step)), R.foreground_voxels(case, 0, step)), (name, step)


# ---- samples for the statistics ------------------------------------------------------------------------------------------------------------------------
def _shuffle(v, salt):
    return np.ascontiguousarray(np.asarray(v, np.float32)[np.argsort(noise((len(v),), salt), kind="stable")])


def _f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def special200():
    """n = 200: ranks 198, 199 (the 99.5 % neighbours) are 1.5 and 300000.0, whose keys differ in the top byte; ranks 0, 1 (the 0.5 %
    neighbours) are 0xC47A0010 and 0xC47A0003 (about -1000.001), whose keys differ in the lowest byte only."""
    body = ((noise((196,), 61) - 0.5) * 1000.0).astype(np.float32) * np.float32(0.002)   # inside (-1, 1)
    return _shuffle(np.concatenate([body, np.array([1.5, 300000.0], np.float32), _f32([0xC47A0010, 0xC47A0003])]), 62)


STAT_CASES = OrderedDict([
    ("all_equal", lambda: np.full(777, 3.25, np.float32)),
    ("clipped_ct", lambda: np.clip((noise((1001,), 51) * 2300.0 - 1500.0).astype(np.float32), np.float32(-958.0), np.float32(326.7))),
    ("negative", lambda: (-1.0 - noise((333,), 52) * 1000.0).astype(np.float32)),
    ("both_zeros", lambda: _shuffle(np.concatenate([np.full(120, -0.0, np.float32), np.zeros(120, np.float32),
                                                     ((noise((60,), 53) - 0.5) * 1e-3).astype(np.float32)]), 54)),
    ("subnormals_and_infinities", lambda: _shuffle(np.concatenate([_f32([1, 2, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000]),
                                                                    np.array([np.inf, -np.inf, np.inf], np.float32),
                                                                    ((noise((191,), 55) - 0.5) * 10.0).astype(np.float32)]), 56)),
    ("size_1", lambda: np.array([2.5], np.float32)),
    ("size_2", lambda: np.array([3.0, -1.0], np.float32)),
    ("n200", lambda: (noise((200,), 57) * 1400.0 - 1000.0).astype(np.float32)),
    ("n201", lambda: (noise((201,), 58) * 1400.0 - 1000.0).astype(np.float32)),
    ("n1001", lambda: (noise((1001,), 59) * 1400.0 - 1000.0).astype(np.float32)),
    ("n130", lambda: (noise((130,), 60) * 1400.0 - 1000.0).astype(np.float32)),
    ("n1445", lambda: (noise((1445,), 63) * 1400.0 - 1000.0).astype(np.float32)),
    ("special200", special200),
])


def virtual_index(n, percent):
    """numpy's, for a float32 sample: float32"""
    return np.asanyarray((n - 1) * np.asanyarray(np.true_divide(percent, np.float32(100))))


def check_quantile_weights():
    g = {n: [float(v - np.floor(v)) for v in (virtual_index(n, 99.5), virtual_index(n, 0.5))] for n in (200, 201, 1001, 130, 1445)}
    assert virtual_index(200, 99.5).dtype == np.float32
    assert g[201] == [0.0, 0.0] and g[1001] == [0.0, 0.0]                      # what the module's head says of the issue's three sizes
    assert sum(all(0.0 < w < 1.0 for w in g[n]) for n in (200, 130, 1445)) == 3
    assert min(g[130] + g[1445]) > 0.2 and g[200][0] < 0.5 <= g[200][1]          # both branches of numpy's _lerp
    s = np.sort(special200())
    key = lambda v: (lambda u: (~u & 0xFFFFFFFF) if u >> 31 else u | 0x80000000)(int(np.asarray(v, np.float32).view(np.uint32)))
    assert key(s[198]) >> 24 != key(s[199]) >> 24 and key(s[0]) >> 8 == key(s[1]) >> 8 and key(s[0]) != key(s[1])
    ct = STAT_CASES["clipped_ct"]()
    tied = float(((ct == np.float32(-958.0)) | (ct == np.float32(326.7))).mean())
    assert 0.35 < tied < 0.5, tied


def check_interpolation_restates_numpy():
    """The host half of compute_stats against np.percentile itself, on sorted samples of many sizes (no device involved)."""
    from deformablelka_amd import dataset_analysis as A
    for n in list(range(1, 70)) + [199, 200, 201, 1000, 1001, 4097, 98304, 20000003]:
        v = np.sort((noise((min(n, 5000),), n) * 1400.0 - 1000.0).astype(np.float32))
        for percent in (99.5, 0.5):
            lo, hi, virtual, previous = A._quantile_plan(n, percent)
            assert 0 <= lo <= hi < n and (hi - lo <= 1 or n > 2 ** 24)       # (beyond 2^24 numpy's float32 index + 1 may skip a rank: restated as is)
            if n <= 5000:
                assert same_value(A._lerp(v[lo], v[hi], virtual, previous), np.percentile(list(v), percent)), (n, percent)


def compare_stats(got, sample, rec, what):
    """got: the seven of compute_stats; sample: the float32 values; rec: the reference's record of the same sample."""
    from tests import dataset_analysis_ref as R
    want = R.compute_stats(sample)
    ref = rec["stats32"].numpy()
    assert len(got) == 7 and rec["n"] == len(sample)
    if len(sample) == 0:
        assert all(np.isnan(v) for v in got) and all(np.isnan(v) for v in want) and bool(np.isnan(ref).all())
        return
    for i in (0, 3, 4, 5, 6):
        assert same_value(got[i], want[i]), (what, KEYS[i], got[i], want[i])
        assert same_value(got[i], ref[i]), (what, KEYS[i], got[i], ref[i])
    n, m64, s64 = R.statistics64(sample)
    assert isinstance(got[1], float) and isinstance(got[2], float)
    if not np.isfinite(m64):
        assert np.isnan(got[1]) == np.isnan(m64) and np.isnan(got[2]) and np.isnan(want[1]) == np.isnan(m64)
        return
    tol = STAT_BOUND * (abs(m64) + s64)
    print(f"{what}: n {n}, |mean - m64| {abs(got[1] - m64):.3e}, |sd - s64| {abs(got[2] - s64):.3e}, bound {tol:.3e}; reference's float32 gap "
          f"{rec['gap_mean']:.3e} / {rec['gap_sd']:.3e}")
    assert abs(got[1] - m64) <= tol and abs(got[2] - s64) <= tol, (what, got[1] - m64, got[2] - s64, tol)
    assert max(rec["gap_mean"], rec["gap_sd"]) <= GAP_BOUND * (abs(m64) + s64)
    assert abs(got[1] - float(ref[1])) <= rec["gap_mean"] + float(np.spacing(np.abs(ref[1]))), (what, got[1], ref[1])
    assert abs(got[2] - float(ref[2])) <= rec["gap_sd"] + float(np.spacing(np.abs(ref[2]))), (what, got[2], ref[2])


def check_stats(name, rec, device):
    from deformablelka_amd import dataset_analysis as A
    sample = STAT_CASES[name]()
    assert digest(sample) == rec["input"]
    t = on(device, sample)
    compare_stats(A.compute_stats(t), sample, rec, name)
    assert same_bits(to_np(t), sample)


def check_order_statistics(name, device):
    from deformablelka_amd import dataset_analysis as A
    sample = STAT_CASES[name]()
    n = len(sample)
    ranks = sorted({0, n - 1, n // 2, (n - 1) // 2, n // 3, (2 * n) // 3, n // 200, (199 * n) // 200})
    with np.errstate(all="ignore"):
        want = np.partition(sample, ranks)[ranks]
    got = A.order_statistics(on(device, sample), ranks)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and same_values(to_np(got), want), (name, to_np(got), want)
    back = A.order_statistics(sample, list(reversed(ranks)))                                    # numpy in, numpy out; any order of ranks
    assert isinstance(back, np.ndarray) and back.dtype == np.float32 and same_values(back, want[::-1])
    if name == "subnormals_and_infinities":                                                      # NaNs sort last, as numpy sorts them
        with_nan = np.concatenate([sample[:50], _f32([0x7FC00000, 0xFFC00001]), sample[50:]])
        got = to_np(A.order_statistics(on(device, with_nan), [0, n - 1, n, n + 1]))
        assert same_values(got[:2], want[[0, -1]]) and np.isnan(got[2]) and np.isnan(got[3])


# ---- datasets --------------------------------------------------------------------------------------------------------------------------------------------
def dataset(name):
    """identifier -> case.  "three": 65, 1295 and 10005 foreground cells, so samples of 7, 130 and 1001 values: the offsets in the
    concatenation (7, 137) are no multiples of 64.  "empty_middle": a case without foreground between two others.  The identifiers sort in this
    order: the reference lists a folder's cases sorted."""
    if name == "three":
        spec = (("case_a", (3, 5, 70), 65), ("case_b", (5, 37, 130), 1295), ("case_c", (5, 37, 130), 10005))
    else:
        spec = (("e1_first", (3, 5, 70), 65), ("e2_nothing", (4, 6, 9), 0), ("e3_last", (5, 37, 130), 1295))
    return OrderedDict((k, exact_count_case(shape, count, 200 + 7 * i)) for i, (k, shape, count) in enumerate(spec))


DATASETS = ("three", "empty_middle")


def dataset_properties(cases):
    props = OrderedDict()
    for i, (k, v) in enumerate(cases.items()):
        shape = np.array(v.shape[1:])
        props[k] = {"size_after_cropping": shape, "original_size_of_raw_data": shape + np.array([i, 2, 3]),
                    "original_spacing": np.array([3.0, 0.75 + 0.01 * i, 0.75]), "itk_spacing": np.array([0.75, 0.75 + 0.01 * i, 3.0])}
    return props


DATASET_JSON = {"labels": {"0": "background", "1": "spleen", "2": "kidney", "3": "liver"}, "modality": {"0": "CT", "1": "noise"}}


def describe(obj):
    """The shape of a result: container types, key order and the kind of every leaf (a real number, whatever its float type)."""
    if isinstance(obj, dict):
        return [type(obj).__name__, [[repr(k), describe(v)] for k, v in obj.items()]]
    if isinstance(obj, (list, tuple)):
        return [type(obj).__name__, [describe(v) for v in obj]]
    if isinstance(obj, np.ndarray):
        return ["ndarray", list(obj.shape), obj.dtype.kind]
    if isinstance(obj, (float, np.floating)):
        return "real"
    if isinstance(obj, (int, np.integer)):
        return "integer"
    return type(obj).__name__


def samples_of(cases, mod):
    from tests import dataset_analysis_ref as R
    return [R.foreground_voxels(v, mod) for v in cases.values()]


def check_dataset(name, rec, device, as_numpy=False):
    from deformablelka_amd import dataset_analysis as A
    cases = dataset(name)
    given = cases if as_numpy else OrderedDict((k, on(device, v)) for k, v in cases.items())
    got = A.collect_intensity_properties(given, 2)
    assert describe(got) == rec["structure"], (describe(got), rec["structure"])
    for mod in (0, 1):
        per_case = samples_of(cases, mod)
        assert [len(s) for s in per_case] == rec["sizes"]
        compare_stats(tuple(got[mod][k] for k in KEYS), np.concatenate(per_case), rec["whole"][mod], f"{name} mod {mod}")
        for k, s in zip(cases, per_case):
            compare_stats(tuple(got[mod]['local_props'][k][q] for q in KEYS), s, rec["local"][mod][k], f"{name} mod {mod} {k}")
    for k, v in given.items():
        assert same_bits(to_np(v), cases[k])
    return got


def check_analyze_dataset(rec, device):
    import pytest
    from deformablelka_amd import dataset_analysis as A
    cases = dataset("three")
    props = dataset_properties(cases)
    an = A.DatasetAnalyzer(OrderedDict((k, on(device, v)) for k, v in cases.items()), props, DATASET_JSON)
    got = an.analyze_dataset()
    assert list(got.keys()) == rec["keys"] and type(got) is dict and describe(got) == rec["structure"]
    assert got["all_classes"] == rec["all_classes"] == [1, 2, 3] and got["modalities"] == rec["modalities"]
    assert list(got["size_reductions"].keys()) == list(cases) and [float(v) for v in got["size_reductions"].values()] == rec["size_reductions"]
    assert all(np.array_equal(a, props[k]["size_after_cropping"]) for a, k in zip(got["all_sizes"], cases))
    assert all(np.array_equal(a, props[k]["original_spacing"]) for a, k in zip(got["all_spacings"], cases))
    assert an.analyze_dataset(collect_intensityproperties=False)["intensityproperties"] is None
    class_dct, per_patient = an.analyse_segmentations()
    assert class_dct is DATASET_JSON["labels"] and describe(per_patient) == rec["segmentations_structure"]
    for k, v in cases.items():
        assert np.array_equal(per_patient[k]['has_classes'], np.unique(v[-1])) and per_patient[k]['has_classes'].dtype == np.float32
    uniq, one, vol, regions = an._load_seg_analyze_classes("case_b", got["all_classes"])
    assert np.array_equal(uniq, np.unique(cases["case_b"][-1])) and list(one.keys()) == [(1, 2, 3), (1,), (2,), (3,)]
    assert float(vol[1]) == float(np.sum(cases["case_b"][-1] == 1) * np.prod(props["case_b"]["itk_spacing"]))
    for call in (lambda: A.DatasetAnalyzer(cases, props, DATASET_JSON, folder_with_cropped_data="/data"), lambda: A.DatasetAnalyzer("/data"),
                 lambda: A.DatasetAnalyzer(cases, props, DATASET_JSON, overwrite=False), lambda: an.props_per_case_file,
                 lambda: an.intensityproperties_file):
        with pytest.raises(NotImplementedError, match="folder_with_cropped_data|overwrite|props_per_case_file|intensityproperties_file"):
            call()
    return got


def check_chain(fx, device):
    """The hand-over: this module's intensityproperties, unchanged, into GenericPreprocessor; against the reference's recorded properties."""
    from deformablelka_amd import dataset_analysis as A, preprocessing as P
    cases = dataset("three")
    ours = A.collect_intensity_properties(OrderedDict((k, on(device, v)) for k, v in cases.items()), 2)
    ref = fx["datasets"]["three"]["whole"][0]["stats32"].numpy()
    theirs = {0: {k: ref[i] for i, k in enumerate(KEYS)}}
    data = on(device, dataset("empty_middle")["e3_last"][:1])
    seg = on(device, np.where(noise((1, 5, 37, 130), 91) < 0.2, -1, 0).astype(np.int32))
    a, _ = P.GenericPreprocessor({0: 'CT'}, {0: True}, (0, 1, 2), intensityproperties=ours).normalize(data, seg)
    b, _ = P.GenericPreprocessor({0: 'CT'}, {0: True}, (0, 1, 2), intensityproperties=theirs).normalize(data, seg)
    a, b = to_np(a).astype(np.float64), to_np(b).astype(np.float64)
    gap, bound = float(np.abs(a - b).max()), GAP_BOUND * float(np.abs(a).max())
    print(f"chain: max |A - B| {gap:.3e}, bound {bound:.3e}, max |out| {float(np.abs(a).max()):.3f}")
    assert float(np.abs(a).max()) > 1.0 and gap <= bound


# ---- NaNs, reproducibility, containers -----------------------------------------------------------------------------------------------------------------
def check_nans(device):
    from deformablelka_amd import dataset_analysis as A
    case = scattered_case((5, 37, 130), 32)
    clean = A.collect_intensity_properties({"c": on(device, case)}, 2)
    outside = case.copy()
    flat = outside[0].reshape(-1)
    flat[np.flatnonzero(case[-1].reshape(-1) <= 0)[::7]] = np.nan                 # NaNs outside the foreground: nothing changes
    got = A.collect_intensity_properties({"c": on(device, outside)}, 2)
    for mod in (0, 1):
        for k in KEYS:
            a, b = clean[mod][k], got[mod][k]
            assert (a == b and type(a) is type(b)) if isinstance(a, float) else same_value(a, b), (mod, k)
    inside = case.copy()
    fg = np.flatnonzero(case[-1].reshape(-1) > 0)
    inside[0].reshape(-1)[fg[30]] = np.nan                                          # rank 30 of the foreground: sampled (30 % 10 == 0)
    t = on(device, inside)
    got = A.collect_intensity_properties({"c": t}, 2)
    assert all(np.isnan(got[0][k]) for k in KEYS) and all(np.isnan(got[0]['local_props']["c"][k]) for k in KEYS)
    assert not any(np.isnan(got[1][k]) for k in KEYS)
    assert np.array_equal(to_np(t).view(np.int32), inside.view(np.int32))           # inputs untouched, NaNs included
    seven = A.compute_stats(on(device, np.array([1.0, np.nan, 3.0], np.float32)))
    assert len(seven) == 7 and all(np.isnan(v) for v in seven)
    assert all(np.isnan(v) for v in A.compute_stats([])) and len(A.compute_stats(np.zeros(0, np.float32))) == 7


def _flat(results):
    return [results[m][k] for m in results for k in KEYS] + [v for m in results for c in results[m]['local_props'].values() for v in c.values()]


def check_reproducible(device):
    from deformablelka_amd import dataset_analysis as A
    cases = OrderedDict((k, on(device, v)) for k, v in dataset("three").items())
    a, b = _flat(A.collect_intensity_properties(cases, 2)), _flat(A.collect_intensity_properties(cases, 2))
    assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() and type(x) is type(y) for x, y in zip(a, b))
    case = scattered_case((5, 37, 130), 33)
    assert same_bits(to_np(A.foreground_voxels(on(device, case), 0)), to_np(A.foreground_voxels(on(device, case), 0)))


def check_containers(device):
    """numpy in, tensors in (host or device), files in: the same values; nothing written to."""
    import tempfile
    from deformablelka_amd import dataset_analysis as A
    cases = dataset("empty_middle")
    want = _flat(A.collect_intensity_properties(OrderedDict((k, on(device, v)) for k, v in cases.items()), 2))
    with tempfile.TemporaryDirectory() as tmp:
        files = OrderedDict()
        for k, v in cases.items():
            files[k] = os.path.join(tmp, k + ".npz")
            np.savez_compressed(files[k], data=v)
        forms = (OrderedDict((k, v.copy()) for k, v in cases.items()), OrderedDict((k, torch.from_numpy(v.copy())) for k, v in cases.items()), files,
                 OrderedDict((k, (v[:-1].copy(), v[-1:].astype(np.int32))) for k, v in cases.items()))
        for form in forms:
            got = _flat(A.collect_intensity_properties(form, 2))
            assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(got, want))
    sample = STAT_CASES["n130"]()
    a, b, c = A.compute_stats(sample), A.compute_stats(list(sample)), A.compute_stats(torch.from_numpy(sample.copy()))
    assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() == np.asarray(z).tobytes() for x, y, z in zip(a, b, c))
    seg = cases["e3_last"][-1]
    for form, dtype in ((seg.copy(), np.float32), (seg.astype(np.int32), np.int32), (seg.astype(np.int16), np.int16)):
        got = A.unique_labels(form)
        assert isinstance(got, np.ndarray) and got.dtype == dtype and np.array_equal(got, np.unique(form))
    got = A.unique_labels(on(device, seg.astype(np.int32)))
    assert isinstance(got, torch.Tensor) and got.dtype == torch.int32 and got.cpu().tolist() == [-1, 0, 1, 2, 3]
    edge = np.zeros((3, 4, 70), np.int32)
    edge[2, 3, 69], edge[0, 0, 0], edge[1, 1, 1] = 255, -1, 31
    assert A.unique_labels(edge).tolist() == [-1, 0, 31, 255]


# ---- labels and regions ------------------------------------------------------------------------------------------------------------------------------------
def region_maps():
    rng = np.random.default_rng(20240611)
    u = rng.random((5, 37, 130))
    maps = OrderedDict(random=np.select([u < 0.12, u < 0.24, u < 0.30], [1, 2, 3], 0).astype(np.int16))
    s = np.zeros((2, 33, 129), np.uint8)            # a one-cell-wide snake of class 1 in plane 0 and one of class 2 in plane 1
    s[0, 0::2, :] = 1
    s[0, 1::4, 128] = 1
    s[0, 3::4, 0] = 1
    s[1, :, 0:97:4] = 2
    for k, w in enumerate(range(0, 96, 4)):
        s[1, 32 if k % 2 == 0 else 0, w + 1:w + 4] = 2
    maps["snake"] = s
    t = np.zeros((6, 6, 6), np.int32)               # two cubes of class 1 that touch in one corner: one object under full connectivity
    t[0:2, 0:2, 0:2] = 1
    t[2:4, 2:4, 2:4] = 1
    t[5, 5, 0] = 2
    maps["diagonal"] = t
    return maps


REGION_CLASSES = [1, 2, 3]
REGIONS = [[1, 2, 3], (1,), (2,), (3,), [1, 2]]


def check_regions(name, rec, device):
    from deformablelka_amd import dataset_analysis as A
    from tests import dataset_analysis_ref as R
    seg = region_maps()[name]
    assert digest(seg) == rec["input"]
    for form in (on(device, seg), seg.copy()):
        vol, regions = A.class_and_region_sizes(form, REGION_CLASSES, VPV)
        one = A.check_if_all_in_one_region(form, REGIONS)
        assert type(vol) is OrderedDict and type(regions) is OrderedDict and type(one) is OrderedDict
        assert list(vol.keys()) == REGION_CLASSES == list(regions.keys()) and list(one.keys()) == [tuple(r) for r in REGIONS]
        assert {c: float(v) for c, v in vol.items()} == rec["volume_per_class"]
        assert {c: [float(v) for v in vs] for c, vs in regions.items()} == rec["region_volume_per_class"]
        assert {k: bool(v) for k, v in one.items()} == rec["all_in_one_region"]
        assert to_np(A.unique_labels(form)).astype(np.int64).tolist() == rec["has_classes"]
    rvol, rregions = R.class_and_region_sizes(seg, REGION_CLASSES, VPV)                       # the restatement, held to the same record
    assert {c: float(v) for c, v in rvol.items()} == rec["volume_per_class"]
    assert {c: [float(v) for v in vs] for c, vs in rregions.items()} == rec["region_volume_per_class"]
    assert {k: bool(v) for k, v in R.check_if_all_in_one_region(seg, REGIONS).items()} == rec["all_in_one_region"]
    if name == "diagonal":
        assert len(rec["region_volume_per_class"][1]) == 1 and rec["all_in_one_region"][(1,)] is True
        from deformablelka_amd import postprocessing
        assert postprocessing.label(seg == 1, connectivity=1)[1] == 2                          # two objects had connectivity 1 been read


# ---- launches and refusals -------------------------------------------------------------------------------------------------------------------------------
def check_launch_count(device):
    from deformablelka_amd import dataset_analysis as A
    from deformablelka_amd.ops import dataset_stats as K
    per_case = LAUNCHES["fg_count"] + LAUNCHES["fg_sample"]
    for name in ("count1_3x5x70", "count641_3x5x70", "count65_5x37x130", "scattered_5x37x130", "rank2_33x129"):   # extents and foreground cells
        t = on(device, FG_CASES[name]())
        before = K.dstats_launch_count()
        A.foreground_voxels(t, 0)
        assert K.dstats_launch_count() == before + per_case, name
    before = K.dstats_launch_count()
    assert A.foreground_voxels(on(device, FG_CASES["count0_3x5x70"]()), 0).numel() == 0       # nothing to sample: the count alone
    assert K.dstats_launch_count() == before + LAUNCHES["fg_count"]
    for name in ("size_1", "n130", "n1001", "all_equal"):
        t = on(device, STAT_CASES[name]())
        before = K.dstats_launch_count()
        A.compute_stats(t)
        assert K.dstats_launch_count() == before + STATS_LAUNCHES, name
    for name, nonempty in (("three", 3), ("empty_middle", 2)):
        cases = OrderedDict((k, on(device, v)) for k, v in dataset(name).items())
        before = K.dstats_launch_count()
        A.collect_intensity_properties(cases, 2)                                                # two modalities share a case's three launches
        assert K.dstats_launch_count() == before + 3 * LAUNCHES["fg_count"] + nonempty * LAUNCHES["fg_sample"] + 2 * (1 + nonempty) * STATS_LAUNCHES
    before = K.dstats_launch_count()
    A.unique_labels(on(device, region_maps()["random"].astype(np.int32)))
    assert K.dstats_launch_count() == before + LAUNCHES["unique_labels"] and A.launch_count() == K.dstats_launch_count()


def check_errors(device):
    """Every refusal comes before any launch, but the labels outside -1 .. 255, which only the kernel's flag can report."""
    import pytest
    from deformablelka_amd import dataset_analysis as A
    from deformablelka_amd.ops import dataset_stats as K
    case = FG_CASES["count65_3x5x70"]()
    sample = on(device, STAT_CASES["n130"]())
    before = K.dstats_launch_count()
    for call in (lambda: A.foreground_voxels(on(device, case.astype(np.float64)), 0),            # wrong dtypes
                 lambda: A.foreground_voxels((on(device, case[:-1]), on(device, case[-1:].astype(np.int64))), 0),
                 lambda: A.foreground_voxels((on(device, case[:-1].astype(np.float64)), on(device, case[-1:].astype(np.int32))), 0),
                 lambda: A.compute_stats(on(device, STAT_CASES["n130"]().astype(np.float64))),
                 lambda: A.order_statistics(on(device, STAT_CASES["n130"]().astype(np.float64)), [0]),
                 lambda: A.unique_labels(on(device, case[-1].astype(np.int64))),
                 lambda: A.unique_labels(on(device, case[-1].astype(np.float64))),
                 lambda: A.foreground_voxels(on(device, case[:, 0, 0]), 0),                       # rank outside 2..3
                 lambda: A.foreground_voxels(on(device, case[:, None, None]), 0),
                 lambda: A.unique_labels(on(device, case[-1, 0, 0].astype(np.int32))),
                 lambda: A.foreground_voxels(on(device, case[-1:]), 0),                           # no modality
                 lambda: A.order_statistics(sample, list(range(9))),                               # more than 8 ranks
                 lambda: A.order_statistics(sample, []),
                 lambda: A.order_statistics(sample, [130]),                                        # a rank >= n
                 lambda: A.order_statistics(sample, [-1]),
                 lambda: A.order_statistics(sample[:0], [0]),
                 lambda: A.order_statistics(on(device, np.zeros((2, 5), np.float32)), [0]),
                 lambda: A.foreground_voxels(on(device, case), 0, step=0),
                 lambda: A.foreground_voxels(on(device, case), 0, step=2.5),
                 lambda: A.collect_intensity_properties({"a": on(device, case)}, 3)):
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(IndexError):
        A.foreground_voxels(on(device, case), 3)
    with pytest.raises(NotImplementedError, match="folder_with_cropped_data"):
        A.DatasetAnalyzer({"a": case}, {}, DATASET_JSON, folder_with_cropped_data="/somewhere")
    assert K.dstats_launch_count() == before
    for bad in (256, -2):
        seg = case[-1].astype(np.int32)
        seg[1, 2, 3] = bad
        with pytest.raises(RuntimeError, match="-1 .. 255"):
            A.unique_labels(on(device, seg))
    half = case[-1].copy()
    half[0, 0, 0] = 1.5
    with pytest.raises(RuntimeError, match="-1 .. 255"):
        A.unique_labels(on(device, half))


def check_c_abi_refuses(device):
    """The library's own checks, past the Python ones: nothing is launched on a bad description."""
    from deformablelka_amd import _lib as L
    from deformablelka_amd.ops import dataset_stats as K
    seg = torch.zeros((4, 5, 6), dtype=torch.int32, device=device)
    data = torch.zeros((2, 4, 5, 6), dtype=torch.float32, device=device)
    ws = torch.zeros(1 << 15, dtype=torch.uint8, device=device)
    count = torch.zeros(1, dtype=torch.int64, device=device)
    out = torch.zeros((2, 16), dtype=torch.float32, device=device)
    x = torch.zeros(100, dtype=torch.float32, device=device)
    res = torch.zeros(4, dtype=torch.float64, device=device)
    vals = torch.zeros(8, dtype=torch.float32, device=device)
    bitmap = torch.zeros(L.DLKA_DSTATS_LABEL_WORDS, dtype=torch.int32, device=device)
    lib, st, null = L.get_lib(), L.stream_ptr(seg), ctypes.c_void_p(0)

    def desc(**fields):
        d = L.DatasetStatsDesc()
        d.rank, d.C, d.label_dtype, d.step = 3, 2, L.DLKA_DSTATS_I32, 10
        for ax in range(3):
            d.ext[ax] = seg.shape[ax]
        for k, v in fields.items():
            if isinstance(v, tuple):
                getattr(d, k)[v[0]] = v[1]
            else:
                setattr(d, k, v)
        return d

    def sample(d, s=L.ptr(seg), w=ws.numel(), m=12, stride=16, offset=0):
        return lib.dlka_dstats_fg_sample(L.ptr(data), s, ctypes.byref(d) if d is not None else None, L.ptr(ws), w, m, L.ptr(out), stride, offset, st)

    def entries(d, s=L.ptr(seg), w=ws.numel()):
        ref = ctypes.byref(d) if d is not None else None
        return (lib.dlka_dstats_fg_count(s, ref, L.ptr(ws), w, L.ptr(count), st), sample(d, s, w), lib.dlka_dstats_unique_labels(s, ref, L.ptr(bitmap), st))

    before = K.dstats_launch_count()
    for fields, code in (({"rank": 1}, -4), ({"rank": 4}, -4), ({"C": 0}, -4), ({"C": L.DLKA_PREP_C_MAX + 1}, -8), ({"label_dtype": 2}, -6),
                         ({"step": 0}, -4), ({"step": 1 << 31}, -8), ({"ext": (1, 0)}, -4), ({"ext": (2, -6)}, -4), ({"ext": (0, 1 << 31)}, -8),
                         ({"ext": (1, 1 << 29)}, -8), ({"rank": 2}, -4)):
        assert entries(desc(**fields)) == (code, code, code), fields
        assert lib.dlka_dstats_fg_workspace_bytes(ctypes.byref(desc(**fields))) == 0
    assert entries(None) == (-1, -1, -1) and entries(desc(), s=null) == (-1, -1, -1)
    assert lib.dlka_dstats_fg_count(L.ptr(seg), ctypes.byref(desc()), L.ptr(ws), 3, L.ptr(count), st) == -7 and sample(desc(), w=3) == -7
    assert sample(desc(), m=0) == -4 and sample(desc(), m=13) == -4                  # ceil(120 / 10) = 12 samples at the most
    assert sample(desc(), offset=-1) == -4 and sample(desc(), offset=5) == -4 and sample(desc(), stride=11) == -4
    assert lib.dlka_dstats_fg_count(L.ptr(seg), ctypes.byref(desc()), L.ptr(ws), ws.numel(), null, st) == -1
    assert lib.dlka_dstats_fg_sample(null, L.ptr(seg), ctypes.byref(desc()), L.ptr(ws), ws.numel(), 12, L.ptr(out), 16, 0, st) == -1
    assert lib.dlka_dstats_unique_labels(L.ptr(seg), ctypes.byref(desc()), null, st) == -1

    def moments(n, p=L.ptr(x), w=ws.numel(), r=L.ptr(res)):
        return lib.dlka_dstats_moments(p, n, L.ptr(ws), w, r, st)

    def select(n, ranks, p=L.ptr(x), w=ws.numel(), v=L.ptr(vals), k=None):
        host = (ctypes.c_int64 * max(len(ranks), 1))(*ranks)
        return lib.dlka_dstats_select(p, n, host, len(ranks) if k is None else k, L.ptr(ws), w, v, L.ptr(count), st)

    assert moments(0) == -4 and moments(-5) == -4 and moments(1 << 32) == -8 and moments(100, p=null) == -1 and moments(100, r=null) == -1
    assert moments(100, w=8) == -7 and lib.dlka_dstats_moments_workspace_bytes(0) == 0 and lib.dlka_dstats_moments_workspace_bytes(1 << 32) == 0
    assert select(0, [0]) == -4 and select(1 << 32, [0]) == -8 and select(100, [0], p=null) == -1 and select(100, [0], v=null) == -1
    assert select(100, [], k=0) == -4 and select(100, list(range(9))) == -8 and select(100, [100]) == -4 and select(100, [5, -1]) == -4
    assert select(100, [0], w=64) == -7
    assert lib.dlka_dstats_select(L.ptr(x), 100, None, 1, L.ptr(ws), ws.numel(), L.ptr(vals), L.ptr(count), st) == -1
    assert lib.dlka_dstats_select_workspace_bytes() <= ws.numel()
    assert K.dstats_launch_count() == before
