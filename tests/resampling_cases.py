"""TEST INFRASTRUCTURE — the cases and checks of deformablelka_amd.resampling, shared by tests/test_resampling_emu.py (wavefront emulator, CPU
suite) and tests/test_resampling_gpu.py (MI355X).  The expected results are in tests/golden/reference_resampling.pt, recorded by
tests/golden/make_golden_resampling.py from the reference's own resample_data_or_seg / resample_patient / export lines.

The INPUTS are not stored: they are rebuilt here from an integer hash with IEEE additions, multiplications and divisions only (no libm, no
numpy reduction), so they are the same bits on every machine; the fixture holds their SHA-256 and every check compares it first.

Bounds (the issue's): orders 0 / 1 values |out - ref| <= 2e-6 max|x| (order 0: equal); order 3 <= 1e-6 max|x|; label maps equal; the fused
argmax equal wherever the reference's top-two gap is >= 4e-6, with at most 1 % of the cells below that gap."""
import hashlib
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "reference_resampling.pt")
GAP = 4e-6

# name: ((c, x, y, z), (x', y', z'))
SHAPES = {
    "up": ((14, 6, 17, 19), (13, 40, 45)),          # 1: up on every axis, nothing a multiple of a tile or a wave
    "half": ((3, 9, 40, 131), (9, 20, 67)),         # 2: down by exactly 2 in-plane, z unchanged
    "one_in": ((2, 1, 5, 7), (4, 5, 7)),            # 3: an axis of extent 1 on either side
    "one_out": ((2, 4, 5, 7), (1, 9, 7)),
    "mixed": ((1, 20, 9, 33), (7, 30, 33)),         # 5, 6: down, up and unchanged; C = 1
    "sep0": ((2, 6, 9, 11), (6, 14, 17)),           # 4: separate axis 0 unchanged (mixed: changed)
    "sep1": ((2, 7, 4, 9), (11, 7, 13)),            #    separate axis 1 changed
    "sep2": ((2, 7, 9, 4), (11, 14, 4)),            #    separate axis 2 unchanged
    "step": ((1, 5, 9, 11), (9, 20, 23)),           # order 3 overshoots at the steps: the clip bites
}


def noise(shape, salt):
    """float64 in [0, 1) from a 64-bit integer hash of the cell index."""
    n = int(np.prod(shape))
    with np.errstate(over="ignore"):
        h = (np.arange(n, dtype=np.uint64) + np.uint64(salt * 1000003 + 12345)) * np.uint64(0x9E3779B97F4A7C15)
        h ^= h >> np.uint64(29)
        h = h * np.uint64(0xBF58476D1CE4E5B9)
        h ^= h >> np.uint64(32)
    return ((h >> np.uint64(11)).astype(np.float64) / float(2 ** 53)).reshape(shape)


def smooth(x):
    """3-cell box along the three spatial axes, edge cells repeated; explicit additions."""
    for ax in (1, 2, 3):
        n = x.shape[ax]
        idx = np.arange(n)
        x = (np.take(x, np.maximum(idx - 1, 0), ax) + x + np.take(x, np.minimum(idx + 1, n - 1), ax)) / 3.0
    return x


def probabilities(name, salt=1):
    """Spatially smooth class probabilities that sum to 1 (float32)."""
    v = smooth(smooth(noise(SHAPES[name][0], salt)))
    v = v * v
    v = v * v
    v = v * v
    total = v[0].copy()
    for c in range(1, v.shape[0]):
        total = total + v[c]
    return (v / total).astype(np.float32)


def image(name, salt=2):
    return ((smooth(noise(SHAPES[name][0], salt)) - 0.5) * 2000.0).astype(np.float32)


def step_image():
    x = np.zeros(SHAPES["step"][0], np.float32)
    x[:, 1:3, 2:6, 3:8] = 1000.0
    x[:, 3:, 6:, :4] = -500.0
    return x


def labels(name, salt=3, lo=0, hi=4):
    """iid labels lo..hi (int16)."""
    return (np.floor(noise(SHAPES[name][0], salt) * float(hi - lo + 1)) + float(lo)).astype(np.int16)


def tie_probabilities():
    """Classes 3 and 7 are the same plane and dominate the others: the argmax is 3 everywhere."""
    p = probabilities("up", salt=7) * np.float32(0.125)
    p[3] = np.float32(0.5) + p[3]
    p[7] = p[3]
    return p


INPUTS = {
    "prob": probabilities, "image": image, "labels": labels,
    "labels_neg": lambda name: labels(name, salt=4, lo=-1, hi=2),
    "image_i16": lambda name: np.trunc(image(name, salt=5)).astype(np.int16),
    "step": lambda name: step_image(), "tie": lambda name: tie_probabilities(),
    "regions": lambda name: smooth(noise(SHAPES[name][0], 9)).astype(np.float32),
}


def make_input(kind, name, channels=None):
    x = INPUTS[kind](name)
    return np.ascontiguousarray(x if channels is None else x[channels[0]:channels[1]])


def digest(x):
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()


def _sep(axis, order, order_z):
    return dict(axis=[axis], order=order, do_separate_z=True, order_z=order_z)


# resample_data_or_seg, is_seg=False: (id, input kind, case, channel range, keyword arguments)
VALUE_CALLS = [(f"{case}_o{order}", "image", case, ch, dict(order=order))
               for case, ch in (("up", (0, 1)), ("half", (0, 1)), ("one_in", None), ("one_out", None), ("mixed", None)) for order in (0, 1, 3)
               if (case, order) != ("mixed", 0)]
VALUE_CALLS += [
    ("mixed_sep0_o1_z0", "image", "mixed", None, _sep(0, 1, 0)), ("mixed_sep0_o1_z1", "image", "mixed", None, _sep(0, 1, 1)),
    ("mixed_sep0_o3_z1", "image", "mixed", None, _sep(0, 3, 1)), ("sep1_o0_z1", "image", "sep1", None, _sep(1, 0, 1)),
    ("sep0_o1_z1", "image", "sep0", None, _sep(0, 1, 1)), ("sep0_o3_z0", "image", "sep0", None, _sep(0, 3, 0)),
    ("sep1_o1_z0", "image", "sep1", None, _sep(1, 1, 0)), ("sep1_o1_z1", "image", "sep1", None, _sep(1, 1, 1)),
    ("sep1_o3_z1", "image", "sep1", None, _sep(1, 3, 1)),
    ("sep2_o1_z0", "image", "sep2", None, _sep(2, 1, 0)), ("sep2_o3_z1", "image", "sep2", None, _sep(2, 3, 1)),
    ("step_o3", "step", "step", None, dict(order=3)), ("step_sep0_o3", "step", "step", None, _sep(0, 3, 0)),
    ("int16_o0", "image_i16", "sep0", None, dict(order=0)), ("int16_o1", "image_i16", "sep0", None, dict(order=1)),
    ("int16_o3", "image_i16", "sep0", None, dict(order=3)),
]
# resample_data_or_seg, is_seg=True
LABEL_CALLS = [
    ("half_o0", "labels", "half", (0, 1), dict(order=0)), ("half_o1", "labels", "half", (0, 1), dict(order=1)),
    ("up_neg_o1", "labels_neg", "up", (0, 1), dict(order=1)), ("sep0_neg_o0", "labels_neg", "sep0", None, dict(order=0)),
    ("one_in_o1", "labels", "one_in", None, dict(order=1)), ("one_out_o1", "labels", "one_out", None, dict(order=1)),
    ("mixed_o1", "labels", "mixed", None, dict(order=1)),
    ("mixed_sep0_o1_z1", "labels_neg", "mixed", None, _sep(0, 1, 1)), ("mixed_sep0_o1_z0", "labels", "mixed", None, _sep(0, 1, 0)),
    ("mixed_sep0_o0_z1", "labels", "mixed", None, _sep(0, 0, 1)),
    ("sep0_o1_z1", "labels", "sep0", None, _sep(0, 1, 1)), ("sep1_o1_z1", "labels_neg", "sep1", None, _sep(1, 1, 1)),
    ("sep2_o1_z1", "labels", "sep2", None, _sep(2, 1, 1)),
]
# resample_and_argmax: the argmax of the reference's resampled probabilities
ARGMAX_CALLS = [(f"{case}_o1", "prob", case, None, dict(order=1)) for case in ("up", "half", "one_in", "one_out", "mixed", "sep0", "sep1", "sep2")]
ARGMAX_CALLS += [
    ("up_sep0_z0", "prob", "up", None, _sep(0, 1, 0)), ("up_sep0_z1", "prob", "up", None, _sep(0, 1, 1)),
    ("half_sep0_z0", "prob", "half", None, _sep(0, 1, 0)), ("one_in_sep0_z0", "prob", "one_in", None, _sep(0, 1, 0)),
    ("one_out_sep0_z1", "prob", "one_out", None, _sep(0, 1, 1)), ("mixed_sep0_z0", "prob", "mixed", None, _sep(0, 1, 0)),
    ("sep0_sep0_z1", "prob", "sep0", None, _sep(0, 1, 1)), ("sep1_sep1_z0", "prob", "sep1", None, _sep(1, 1, 0)),
    ("sep1_sep1_z1", "prob", "sep1", None, _sep(1, 1, 1)), ("sep2_sep2_z1", "prob", "sep2", None, _sep(2, 1, 1)),
    ("tie_o1", "tie", "up", None, dict(order=1)),
]
REGION_CALLS = [("half_regions", "regions", "half", None, dict(order=1), (1, 2, 3)), ("half_regions_sep", "regions", "half", None, _sep(0, 1, 0), (2, 1, 3))]


def _props(after, full, bbox, original=(1.0, 1.0, 1.0), resampled=(1.0, 1.0, 1.0)):
    return {"size_after_cropping": after, "original_size_of_raw_data": full, "crop_bbox": bbox, "original_spacing": original,
            "spacing_after_resampling": resampled}


# segmentation_from_softmax: (id, input kind, case, properties, keyword arguments)
EXPORT_CALLS = [
    ("clamp", "prob", "sep0", _props((6, 14, 17), (8, 20, 17), [[2, 9], [6, 99], [0, 3]]), {}),          # the box ends where the volume ends
    ("no_box", "prob", "sep0", _props((6, 14, 17), (6, 14, 17), None), {}),
    ("sep_original", "prob", "sep0", _props((6, 14, 17), (7, 15, 18), [[1, 7], [0, 14], [1, 18]], original=(5.0, 1.0, 1.25)), {}),
    ("sep_resampled", "prob", "sep1", _props((11, 7, 13), (11, 7, 13), [[0, 11], [0, 7], [0, 13]], resampled=(1.0, 4.0, 1.0)),
     dict(interpolation_order_z=1)),
    ("two_lowres_axes", "prob", "sep0", _props((6, 14, 17), (6, 14, 17), None, original=(3.5, 3.5, 1.0)), {}),
    ("equal_shapes", "prob", "sep0", _props((6, 9, 11), (8, 9, 12), [[1, 7], [0, 9], [1, 12]], original=(5.0, 1.0, 1.0)), {}),
    ("forced", "prob", "sep2", _props((11, 14, 4), (11, 14, 4), None, original=(1.0, 1.0, 2.0)), dict(force_separate_z=True, interpolation_order_z=1)),
    ("regions", "regions", "half", _props((9, 20, 67), (9, 22, 70), [[0, 9], [2, 22], [3, 70]]), dict(region_class_order=(1, 2, 3))),
]
# resample_patient: (id, case, original spacing, target spacing, keyword arguments)
PATIENT_CALLS = [
    ("aniso", "sep0", (3.0, 0.8, 0.8), (1.5, 1.0, 1.0), dict(order_seg=1, force_separate_z=None)),
    ("iso", "sep0", (1.0, 0.8, 0.8), (1.5, 1.0, 0.5), dict()),
]


def load_fixture():
    return torch.load(FIXTURE, weights_only=False)


def _inp(fx, section, cid, kind, case, ch, dev, as_numpy=False):
    x = make_input(kind, case, ch)
    assert digest(x) == fx[section][cid]["input"], f"{section}/{cid}: the rebuilt input differs from the recorded one"
    return x if as_numpy else torch.from_numpy(x).to(dev)


def check_values(fx, call, dev):
    from deformablelka_amd import resampling as S
    cid, kind, case, ch, kw = call
    x = _inp(fx, "values", cid, kind, case, ch, dev)
    want = fx["values"][cid]["out"]
    out = S.resample_data_or_seg(x, SHAPES[case][1], False, **kw)
    assert isinstance(out, torch.Tensor) and out.device == x.device and out.dtype == x.dtype and tuple(out.shape) == tuple(want.shape)
    scale = float(x.abs().max())
    if not x.is_floating_point():
        # float64 inside; the reference truncates a float64 value that the bound below allows on either side of an integer
        err = int((out.cpu().to(torch.int64) - want.to(torch.int64)).abs().max())
        print(f"values/{cid}: integer, max |out - ref| = {err}")
        assert err <= (0 if kw["order"] == 0 else 1)
        return
    err = float((out.cpu().double() - want.double()).abs().max())
    orders = {kw["order"], kw.get("order_z", 0) if kw.get("do_separate_z") else kw["order"]}
    bound = 0.0 if orders == {0} else (1e-6 if 3 in orders else 2e-6) * scale
    print(f"values/{cid}: max |out - ref| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def check_labels(fx, call, dev):
    from deformablelka_amd import resampling as S
    cid, kind, case, ch, kw = call
    x = _inp(fx, "labels", cid, kind, case, ch, dev)
    out = S.resample_data_or_seg(x, SHAPES[case][1], True, cval=-1, **kw)
    assert out.dtype == x.dtype and out.device == x.device
    assert torch.equal(out.cpu(), fx["labels"][cid]["out"].to(out.dtype))        # (stored as int8: the labels are -1..4)


def _close(rec):
    shape = tuple(rec["argmax"].shape)
    return torch.from_numpy(np.unpackbits(rec["close"].numpy())[:int(np.prod(shape))].reshape(shape).astype(bool))


def check_argmax(fx, call, dev):
    """Equal wherever the reference's two largest resampled probabilities are GAP apart; at most 1 % of the cells are closer."""
    from deformablelka_amd import resampling as S
    cid, kind, case, ch, kw = call
    x = _inp(fx, "argmax", cid, kind, case, ch, dev)
    rec = fx["argmax"][cid]
    out = S.resample_and_argmax(x, SHAPES[case][1], **kw)
    assert out.dtype == torch.uint8 and out.device == x.device
    if kind == "tie":      # two identical planes: the first one, everywhere
        assert rec["argmax_everywhere"] == 3 and bool((out == 3).all()) and tuple(out.shape) == SHAPES[case][1]
        return
    close = _close(rec)
    frac = float(close.float().mean())
    print(f"argmax/{cid}: {100 * frac:.4f} % of the cells below a gap of {GAP}")
    assert frac <= 0.01
    assert torch.equal(out.cpu()[~close], rec["argmax"][~close])
    assert torch.equal(out, S.resample_and_argmax(x, SHAPES[case][1], **kw))          # bitwise reproducible


def check_fused_equals_unfused(call, dev):
    from deformablelka_amd import resampling as S
    _, kind, case, ch, kw = call
    x = torch.from_numpy(make_input(kind, case, ch)).to(dev)
    full = S.resample_data_or_seg(x, SHAPES[case][1], False, **kw)
    assert torch.equal(S.resample_and_argmax(x, SHAPES[case][1], **kw).long(), full.argmax(0))


# float64 probabilities through the fused kernel: output rows of 6 (the last lane holds 2 voxels) and 8 (whole quads); linear on every axis, an
# unchanged axis (one tap), and in-plane linear with nearest z
F64_ARGMAX_CALLS = [("f64_o1_w6", (2, 3, 4, 5), (4, 5, 6), dict(order=1)), ("f64_o1_w8_x_unchanged", (2, 3, 4, 7), (3, 5, 8), dict(order=1)),
                    ("f64_sep_w8", (2, 3, 4, 5), (4, 5, 8), _sep(0, 1, 0))]


def check_fused_equals_unfused_f64(call, dev):
    """As check_fused_equals_unfused: bit for bit the argmax of the float64 channels that the unfused kernel writes."""
    from deformablelka_amd import resampling as S
    _, shape, out, kw = call
    x = torch.from_numpy(np.asarray(noise(shape, 23), dtype=np.float64)).to(dev)
    full = S.resample_data_or_seg(x, out, False, **kw)
    assert full.dtype == torch.float64
    assert torch.equal(S.resample_and_argmax(x, out, **kw).long(), full.argmax(0))


def check_regions(fx, call, dev):
    from deformablelka_amd import resampling as S
    cid, kind, case, ch, kw, regions = call
    x = _inp(fx, "regions", cid, kind, case, ch, dev)
    rec = fx["regions"][cid]
    out = S.resample_and_argmax(x, SHAPES[case][1], regions_class_order=regions, **kw)
    close = _close(rec)
    assert float(close.float().mean()) <= 0.01
    assert torch.equal(out.cpu()[~close], rec["argmax"][~close])
    full = S.resample_data_or_seg(x, SHAPES[case][1], False, **kw)
    want = torch.zeros_like(out)
    for i, c in enumerate(regions):
        want[full[i] > 0.5] = c
    assert torch.equal(out, want)
    overlap = ((full > 0.5).sum(0) > 1).float().mean()
    assert float(overlap) > 0.01                                                       # the regions do overlap


def check_export(fx, call, dev, as_numpy=False):
    import copy
    from deformablelka_amd import resampling as S
    cid, kind, case, props, kw = call
    x = _inp(fx, "export", cid, kind, case, None, dev, as_numpy)
    rec = fx["export"][cid]
    mine = copy.deepcopy(props)
    out = S.segmentation_from_softmax(x, mine, **kw)
    assert mine == props                                                               # the reference edits crop_bbox in place
    if as_numpy:
        assert isinstance(out, np.ndarray) and out.dtype == np.uint8
        out = torch.from_numpy(out)
    else:
        assert out.dtype == torch.uint8 and out.device == x.device
    close = _close(rec)
    assert tuple(out.shape) == tuple(rec["argmax"].shape) and float(close.float().mean()) <= 0.01
    assert torch.equal(out.cpu()[~close], rec["argmax"][~close])


def check_patient(fx, call, dev):
    from deformablelka_amd import resampling as S
    cid, case, original, target, kw = call
    data = torch.from_numpy(make_input("image", case)).to(dev)
    seg = torch.from_numpy(make_input("labels_neg", case, (0, 1))).to(dev)
    rec = fx["patient"][cid]
    assert digest(data.cpu().numpy()) == rec["input"]
    d, s = S.resample_patient(data, seg, original, target, **kw)
    assert tuple(d.shape[1:]) == tuple(s.shape[1:]) == tuple(rec["data"].shape[1:])
    assert float((d.cpu().double() - rec["data"].double()).abs().max()) <= 1e-6 * float(data.abs().max())
    assert torch.equal(s.cpu(), rec["seg"])
    d2, none = S.resample_patient(data, None, original, target, **kw)
    assert none is None and torch.equal(d2, d)


def check_half_case_thresholds(fx):
    """Case 2, order 1: along y every output cell weighs two source rows 0.5 each (40 -> 20); along z (131 -> 67) the weights vary, and the
    middle column reads source column 65 alone.  There the fixture has cells where two labels hold exactly 0.5 each (the larger wins); where
    the four source cells hold four labels and both columns count, no label reaches 0.5 (0)."""
    seg = make_input("labels", "half", (0, 1)).astype(np.int64)[0]
    want = fx["labels"]["half_o1"]["out"].numpy().astype(np.int64)[0]
    c = (np.arange(67) + 0.5) * (131.0 / 67.0) - 0.5
    lo = np.floor(c).astype(int)
    assert c[33] == 65.0
    top, bottom = seg[:, 0:40:2, 65], seg[:, 1:40:2, 65]
    halves = top != bottom
    assert halves.sum() > 50 and np.array_equal(want[:, :, 33][halves], np.maximum(top, bottom)[halves])
    cols = np.array([x for x in range(67) if c[x] != lo[x] and 0 <= lo[x] < 130])
    quad = np.stack([seg[:, 0:40:2][:, :, lo[cols]], seg[:, 0:40:2][:, :, lo[cols] + 1], seg[:, 1:40:2][:, :, lo[cols]],
                     seg[:, 1:40:2][:, :, lo[cols] + 1]], -1)
    quad.sort(-1)
    distinct = (quad[..., 0] != quad[..., 1]) & (quad[..., 1] != quad[..., 2]) & (quad[..., 2] != quad[..., 3])
    assert distinct.sum() > 50 and not want[:, :, cols][distinct].any()


def check_chain(dev):
    """predict -> export -> post-process -> score without leaving the device: tensors in, tensors out."""
    from deformablelka_amd import metrics, postprocessing, resampling as S
    call = EXPORT_CALLS[0]
    x = torch.from_numpy(make_input(call[1], call[2])).to(dev)
    seg = S.segmentation_from_softmax(x, call[3])
    kept, _, _ = postprocessing.remove_all_but_the_largest_connected_component(seg, [1, 2, 3], 1.0)
    assert isinstance(kept, torch.Tensor) and kept.device == seg.device and kept.dtype == torch.uint8 and kept.shape == seg.shape
    assert int((kept != 0).sum()) <= int((seg != 0).sum())
    scores = metrics.evaluate_label_maps(kept, seg, [1, 2, 3])
    assert scores is not None


def check_errors(dev):
    import pytest
    from deformablelka_amd import resampling as S
    x = torch.from_numpy(make_input("image", "one_in")).to(dev)
    with pytest.raises(NotImplementedError, match="order"):
        S.resample_data_or_seg(x, (4, 5, 7), False, order=2)
    with pytest.raises(NotImplementedError, match="order_z"):
        S.resample_data_or_seg(x, (4, 5, 7), False, axis=[0], order=1, do_separate_z=True, order_z=3)
    with pytest.raises(NotImplementedError, match="order"):
        S.resample_data_or_seg(x.to(torch.int16), (4, 5, 7), True, order=3)
    with pytest.raises(NotImplementedError, match="order"):
        S.resample_and_argmax(x, (4, 5, 7), order=3)
    with pytest.raises(AssertionError):
        S.resample_data_or_seg(x[0], (4, 5, 7), False, order=1)
    with pytest.raises(AssertionError):
        S.resample_patient(x[0], None, (1, 1, 1), (2, 2, 2))
    with pytest.raises(AssertionError):
        S.resample_data_or_seg(x, (4, 5, 7), False, axis=[0, 1], order=1, do_separate_z=True)
    same = S.resample_data_or_seg(x, (1, 5, 7), False, order=3)                         # equal shapes: nothing is resampled
    assert torch.equal(same, x)


def check_containers(fx, dev):
    """numpy in gives numpy out; a host tensor comes back on the host; the arguments are not written to."""
    from deformablelka_amd import resampling as S
    x = make_input("image", "one_in")
    keep = x.copy()
    out = S.resample_data_or_seg(x, (4, 5, 7), False, order=1)
    assert isinstance(out, np.ndarray) and out.dtype == x.dtype and np.array_equal(x, keep)
    assert np.array_equal(out, fx["values"]["one_in_o1"]["out"].numpy()) or np.abs(out - fx["values"]["one_in_o1"]["out"].numpy()).max() <= 2e-6 * np.abs(x).max()
    lab = S.resample_and_argmax(make_input("prob", "one_in"), (4, 5, 7))
    assert isinstance(lab, np.ndarray) and lab.dtype == np.uint8
    half = torch.from_numpy(x).to(dev).to(torch.float64)
    assert S.resample_data_or_seg(half, (4, 5, 7), False, order=1).dtype == torch.float64
