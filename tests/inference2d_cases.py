"""TEST INFRASTRUCTURE — the cases and checks of deformablelka_amd.inference2d, shared by tests/test_inference2d_emu.py (wavefront emulator, CPU
suite) and tests/test_inference2d_gpu.py (MI355X).  The expected results are in tests/golden/reference_inference2d.pt, recorded by
tests/golden/make_golden_inference2d.py from scipy.ndimage.zoom and the restatement of the reference's test_single_volume
(tests/inference2d_ref.py).  No scipy here.

The INPUTS are not stored: they are rebuilt from tests/resampling_cases.py's integer hash with IEEE operations only, so they are the same bits
on every machine; the fixture holds their SHA-256 and every check compares it first.

Bounds (the issue's, taken from tests/resampling_cases.py and tests/metrics_cases.py): zoom values equal at order 0, |out - ref| <= 2e-6 max|x|
at order 1 and <= 1e-6 max|x| at order 3, integers within 1.  Exempt are the cells whose coordinate lies below n - 1 by at most 1e-9 (a
coordinate EQUAL to n - 1 is inside by scipy's rule and is not exempt), at most 0.1 % of the cells; the recorder asserts the cases have none.
The rows and columns whose coordinate overshoots n - 1 must be exactly 0.  The normalised output is bitwise the float32 (z - mean) / std of
the product's own un-normalised output, the bfloat16 output bitwise that float32 output rounded.  Order-0, label and argmax outputs are equal
everywhere, with no exemption (the recorder asserts that no order-0 coordinate lies within 1e-9 of a half, but for output column 10 of the
issue's 24 -> 21, which sits on 11.5 and is held to equality like every other cell).  End to end: the prediction is equal except where the
reference's top-two logit gap at the selected source pixel is below resampling_cases.GAP, at most 1 % of the cells; metric lists within
metrics_cases.UNIT_RTOL."""
import os

import numpy as np
import torch

from tests import metrics_cases as MC
from tests import resampling_cases as RC

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "reference_inference2d.pt")
MEAN, STD = 0.5, 0.5

# name: ((N, H, W), (oh, ow), rows overshoot, columns overshoot)
ZOOM_SHAPES = {
    "rows": ((3, 32, 21), (16, 24), True, False),     # 32 -> 16: the last output row is 0; columns upsample
    "cols": ((2, 19, 28), (16, 24), False, True),     # 28 -> 24: the last output column is 0
    "ragged": ((2, 19, 21), (16, 23), False, False),  # neither; the width is no multiple of 4
    "same": ((2, 16, 24), (16, 24), False, False),    # untouched, bitwise
}
ZOOM_CALLS = [(f"{case}_{dt}_o{order}", case, dt, order) for case in ZOOM_SHAPES for dt in ("float32", "int16") for order in (0, 1, 3)]
LABEL_DTYPES = ("uint8", "int32", "int64")

# name: ((N, h, w), (x, y), kind)
ARGMAX_SHAPES = {
    "up": ((3, 16, 24), (32, 21), "plain"),
    "down": ((2, 32, 28), (16, 24), "no_zero"),       # class 0 never wins in the logits: the zero last row and column come from the rule alone
    "tie": ((2, 32, 28), (16, 24), "tie"),
    "same": ((2, 16, 24), (16, 24), "plain"),
}
ARGMAX_CALLS = [(f"{case}_{dt}_K{K}", case, dt, K) for case in ARGMAX_SHAPES for dt in ("float32", "bfloat16") for K in (9, 2)
                if not (case == "tie" and K == 2)]

E2E_CLASSES = 6
E2E_CENTRES = (0.0, 1.0, 2.0, 50.0, 4.0, 60.0)       # classes 3 and 5 are never predicted
E2E_A = ((4, 16, 24), (16, 24))                      # patch = slice size
E2E_B = ((5, 32, 21), (16, 24))
E2E_2D = (16, 24)
E2E_B_SALT = 31                                      # (picked by the recorder: the reference stays within the 1 % exemption)


def overshoots(n, m):
    """True when scipy's last coordinate (m - 1) * ((n - 1) / (m - 1)) exceeds n - 1."""
    return float(m - 1) * (float(n - 1) / float(m - 1)) > float(n - 1)


def coordinates(n, m):
    return np.arange(m, dtype=np.float64) * (float(n - 1) / float(m - 1))


def exempt_axis(n, m):
    cc = coordinates(n, m)
    return (cc < float(n - 1)) & (cc >= float(n - 1) - 1e-9)


def half_axis(n, m):
    """Order-0 coordinates within 1e-9 of a half."""
    cc = coordinates(n, m)
    return np.abs(cc - np.floor(cc) - 0.5) <= 1e-9


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------
def zoom_input(case, dt):
    shape = ZOOM_SHAPES[case][0]
    x = (RC.smooth(RC.noise((1,) + shape, 11 + len(case)))[0] - 0.5) * 4000.0
    return np.ascontiguousarray(np.trunc(x).astype(np.int16) if dt == "int16" else x.astype(np.float32))


def label_input(case, dt):
    shape = ZOOM_SHAPES[case][0]
    return np.ascontiguousarray(np.floor(RC.noise(shape, 17) * 9.0).astype(dt))


def logits_input(case, K):
    """(N, K, h, w) float32, every value a multiple of 1/32 below 8 (exact in bfloat16 too); the K values of a pixel are pairwise different."""
    (n, h, w), _, kind = ARGMAX_SHAPES[case]
    base = np.floor(RC.noise((n, K, h, w), 23 + K) * 16.0) / 2.0
    x = base + (np.arange(K, dtype=np.float64) / 32.0)[None, :, None, None]
    if kind == "no_zero":
        x[:, 0] = -100.0
    if kind == "tie":
        x = x * 0.125
        x[:, 3] = 9.0
        x[:, 7] = 9.0
    return np.ascontiguousarray(x.astype(np.float32))


def e2e_image(shape, salt):
    """float32 (S, x, y) in about [0.3, 2.7]: normalised with mean = std = 0.5 it spans the centres 0, 1, 2 and 4."""
    v = RC.smooth(RC.noise((1,) + tuple(shape), salt))[0]
    return np.ascontiguousarray(((v - 0.5) * 6.0 + 1.5).astype(np.float32))


def e2e_label(shape, salt):
    """int64 labels 0..3 in blobs (class 3: in the label only; 4: in the prediction only; 5: in neither)."""
    v = RC.smooth(RC.noise((1,) + tuple(shape), salt))[0]
    return np.ascontiguousarray(np.clip(np.floor((v - 0.5) * 12.0 + 1.5), 0, 3).astype(np.int64))


class StandInNet(torch.nn.Module):
    """logits_k = -|x - c_k|: one IEEE subtraction, abs and negation per value, the same bits on the host and the device."""

    def __init__(self, centres=E2E_CENTRES):
        super().__init__()
        self.register_buffer("centres", torch.tensor(centres, dtype=torch.float32).view(1, -1, 1, 1))
        self.batches = []

    def forward(self, x):
        assert x.ndim == 4 and x.shape[1] == 1 and x.dtype == torch.float32
        assert not self.training and not torch.is_grad_enabled()
        self.batches.append(int(x.shape[0]))
        return -(x - self.centres).abs()


def load_fixture():
    return torch.load(FIXTURE, weights_only=False)


def _inp(rec, x):
    assert RC.digest(x) == rec["input"], "the rebuilt input differs from the recorded one"
    return x


def unpack(bits, shape):
    return torch.from_numpy(np.unpackbits(bits.numpy())[:int(np.prod(shape))].reshape(shape).astype(bool))


# ---- zoom ----------------------------------------------------------------------------------------------------------------------------------------
def run_zoom(call, dev):
    from deformablelka_amd import inference2d as I2
    _, case, dt, order = call
    x = torch.from_numpy(zoom_input(case, dt)).to(dev)
    return x, I2.zoom_slices(x, ZOOM_SHAPES[case][1], order=order)


def check_zoom(fx, call, dev):
    from deformablelka_amd import inference2d as I2
    cid, case, dt, order = call
    (n, h, w), (oh, ow), rows_over, cols_over = ZOOM_SHAPES[case]
    rec = fx["zoom"][cid]
    _inp(rec, zoom_input(case, dt))
    x, out = run_zoom(call, dev)
    want = rec["out"]
    assert isinstance(out, torch.Tensor) and out.device == x.device and out.dtype == x.dtype and tuple(out.shape) == tuple(want.shape) == (n, oh, ow)
    got = out.cpu()
    assert overshoots(h, oh) == rows_over and overshoots(w, ow) == cols_over
    if rows_over:
        assert not got[:, -1, :].any() and not want[:, -1, :].any()
    if cols_over:
        assert not got[:, :, -1].any() and not want[:, :, -1].any()
    if case == "same":
        assert torch.equal(got, x.cpu()) and torch.equal(want, x.cpu())
        return
    exempt = torch.from_numpy(exempt_axis(h, oh)[:, None] | exempt_axis(w, ow)[None, :])
    assert float(exempt.float().mean()) <= 0.001
    keep = ~exempt[None].expand_as(got)
    if order == 0:
        assert torch.equal(got[keep], want[keep])
    elif dt == "int16":
        err = int((got.to(torch.int64) - want.to(torch.int64))[keep].abs().max())
        print(f"zoom/{cid}: integer, max |out - ref| = {err}")
        assert err <= 1
    else:
        scale = float(x.abs().max())
        err = float((got.double() - want.double())[keep].abs().max())
        bound = (1e-6 if order == 3 else 2e-6) * scale
        print(f"zoom/{cid}: max |out - ref| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound
    # one slice through zoom() is that slice of the stack, and the factors give the same output size
    one = I2.zoom(x[0], (oh / h, ow / w), order=order)
    assert torch.equal(one, out[0])


def check_zoom_labels(fx, case, dt, dev):
    from deformablelka_amd import inference2d as I2
    rec = fx["labels"][f"{case}_{dt}"]
    x = torch.from_numpy(_inp(rec, label_input(case, dt))).to(dev)
    out = I2.zoom_slices(x, ZOOM_SHAPES[case][1], order=0)
    assert out.dtype == x.dtype and torch.equal(out.cpu(), rec["out"].to(out.dtype))       # (stored as uint8: the labels are 0..8)
    return out


def check_normalize_and_bf16(case, order, dev):
    """Bitwise: the fused Normalize is float32 (z - mean) / std of the product's own output, the bfloat16 store that value rounded."""
    from deformablelka_amd import inference2d as I2
    x = torch.from_numpy(zoom_input(case, "float32")).to(dev)
    size = ZOOM_SHAPES[case][1]
    z = I2.zoom_slices(x, size, order=order).cpu()
    mean, std = 0.25, 0.75
    want = (z - torch.tensor(mean, dtype=torch.float32)) / torch.tensor(std, dtype=torch.float32)      # IEEE on the host
    zn = I2.zoom_slices(x, size, order=order, mean=mean, std=std)
    assert zn.dtype == torch.float32 and torch.equal(zn.cpu(), want)
    zb = I2.zoom_slices(x, size, order=order, mean=mean, std=std, dtype=torch.bfloat16)
    assert zb.dtype == torch.bfloat16 and torch.equal(zb.cpu(), want.to(torch.bfloat16))
    plain = I2.zoom_slices(x, size, order=order, dtype=torch.bfloat16)
    assert torch.equal(plain.cpu(), z.to(torch.bfloat16))
    if ZOOM_SHAPES[case][2]:                                   # the zero row is normalised like every other value
        assert bool((zn.cpu()[:, -1, :] == want[0, -1, 0]).all()) and float(want[0, -1, 0]) == float(np.float32(-mean) / np.float32(std))


BF16_ZOOMS = (((2, 5, 7), (4, 6)), ((2, 5, 6), (5, 8)))      # output rows of 6 (the last lane holds 2 pixels) and 8 (whole quads)


def check_bf16_slices_two_taps(dev):
    """Bitwise, as check_normalize_and_bf16: order 1 of bfloat16 slices is order 1 of the same values held in float32 (checked against scipy
    above) with the bfloat16 store; the sum is float64 of identical inputs either way."""
    from deformablelka_amd import inference2d as I2
    for salt, (shape, size) in enumerate(BF16_ZOOMS):
        x = torch.from_numpy(e2e_image(shape, 53 + salt)).to(torch.bfloat16).to(dev)
        out = I2.zoom_slices(x, size, order=1)
        assert out.dtype == torch.bfloat16 and tuple(out.shape) == (shape[0],) + size
        assert torch.equal(out.cpu(), I2.zoom_slices(x.float(), size, order=1, dtype=torch.bfloat16).cpu())


# ---- argmax fused with the zoom back ---------------------------------------------------------------------------------------------------------
def run_argmax(call, dev):
    from deformablelka_amd import inference2d as I2, ops
    _, case, dt, K = call
    (n, h, w), xy, _ = ARGMAX_SHAPES[case]
    logits = torch.from_numpy(logits_input(case, K)).to(dev).to(getattr(torch, dt))
    idx = I2._index_tables((h, w), xy, logits.device) if (h, w) != xy else ops.zoom2d_index_tables([np.arange(h), np.arange(w)], (h, w),
                                                                                                    logits.device)
    return ops.zoom2d_argmax(logits, xy, idx)


def check_argmax(fx, call, dev):
    cid, case, dt, K = call
    (n, h, w), xy, kind = ARGMAX_SHAPES[case]
    rec = fx["argmax"][cid]
    _inp(rec, logits_input(case, K))
    out = run_argmax(call, dev)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (n,) + xy
    got = out.cpu()
    assert torch.equal(got, rec["out"])
    if kind in ("no_zero", "tie"):                             # 32 -> 16 and 28 -> 24 overshoot
        assert not got[:, -1, :].any() and not got[:, :, -1].any()
        inner = got[:, :-1, :-1]
        assert bool((inner == 3).all()) if kind == "tie" else bool((inner != 0).all())


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------------
def _metrics_close(got, want):
    assert len(got) == len(want)
    for (d, h), (wd, wh) in zip(got, want):
        assert MC.rel(d, wd) <= MC.UNIT_RTOL and MC.rel(h, wh) <= MC.UNIT_RTOL, (got, want)


def run_e2e(which, dev, slice_batch=24):
    from deformablelka_amd import inference2d as I2
    shape, patch = E2E_A if which == "a" else E2E_B
    image = e2e_image(shape, 29 if which == "a" else E2E_B_SALT)
    label = e2e_label(shape, 37)
    net = StandInNet().to(dev)
    res = I2.test_single_volume(torch.from_numpy(image)[None].to(dev), torch.from_numpy(label)[None].to(dev), net, E2E_CLASSES,
                                patch_size=list(patch), slice_batch=slice_batch, return_prediction=True)
    return image, label, net, res


def check_e2e_a(fx, dev):
    rec = fx["e2e_a"]
    image, label, net, (metric_list, pred) = run_e2e("a", dev)
    _inp(rec, image)
    assert pred.dtype == torch.int64 and torch.equal(pred.cpu(), rec["prediction"].to(torch.int64))
    _metrics_close(metric_list, rec["metric_list"])
    assert len(metric_list) == E2E_CLASSES - 1
    # class 3: missing in the prediction only -> (0, 0); class 4: in the label only -> (1, 0); class 5: in neither -> (0, 0)
    assert tuple(metric_list[2]) == (0, 0) and tuple(metric_list[3]) == (1, 0) and tuple(metric_list[4]) == (0, 0)
    assert metric_list[0][1] > 0 and metric_list[1][1] > 0
    assert net.batches == [4]


def check_e2e_b(fx, dev):
    from deformablelka_amd import metrics as M
    rec = fx["e2e_b"]
    image, label, net, (metric_list, pred) = run_e2e("b", dev)
    _inp(rec, image)
    want = rec["prediction"].to(torch.int64)
    close = unpack(rec["close"], tuple(want.shape))
    frac = float(close.float().mean())
    print(f"e2e_b: {100 * frac:.4f} % of the cells below a logit gap of {RC.GAP}")
    assert frac <= 0.01
    got = pred.cpu()
    assert torch.equal(got[~close], want[~close])
    per_class = [M.calculate_metric_percase(pred == i, torch.from_numpy(label).to(pred.device) == i) for i in range(1, E2E_CLASSES)]
    _metrics_close(metric_list, per_class)
    assert net.batches == [5]


def check_slice_batch(dev):
    runs = {sb: run_e2e("b", dev, sb) for sb in (1, 2, 5)}
    assert runs[1][2].batches == [1] * 5 and runs[2][2].batches == [2, 2, 1] and runs[5][2].batches == [5]
    assert torch.equal(runs[1][3][1], runs[2][3][1]) and torch.equal(runs[1][3][1], runs[5][3][1])
    assert runs[1][3][0] == runs[2][3][0] == runs[5][3][0]


def check_image_2d(fx, dev):
    """The reference's 2-D branch: no zoom and no Normalize."""
    from deformablelka_amd import inference2d as I2
    rec = fx["e2e_2d"]
    image = _inp(rec, e2e_image((1,) + E2E_2D, 41)[0] * np.float32(2.0) - np.float32(1.0))
    label = e2e_label((1,) + E2E_2D, 43)[0]
    net = StandInNet().to(dev)
    metric_list, pred = I2.test_single_volume(torch.from_numpy(image)[None].to(dev), torch.from_numpy(label)[None].to(dev), net, E2E_CLASSES,
                                              patch_size=[8, 8], return_prediction=True)
    assert tuple(pred.shape) == E2E_2D and torch.equal(pred.cpu(), rec["prediction"].to(torch.int64))
    _metrics_close(metric_list, rec["metric_list"])
    assert torch.equal(I2.predict_volume(torch.from_numpy(image).to(dev), net, (8, 8)).cpu().to(torch.int64), pred.cpu())


INFERENCE_CASES = (((4, 16, 16), 29, 37), ((3, 16, 16), 47, 38))     # (shape, image salt, label salt); img_size 16: nothing is zoomed


class _Loader(list):
    pass


def inference_loader(dev):
    cases = [{"image": torch.from_numpy(e2e_image(shape, si))[None].to(dev), "label": torch.from_numpy(e2e_label(shape, sl))[None].to(dev),
              "case_name": [f"case{i:04d}"]} for i, (shape, si, sl) in enumerate(INFERENCE_CASES)]
    loader = _Loader(cases)
    loader.dataset = cases
    return loader


def check_inference(fx, dev):
    import types
    from deformablelka_amd import inference2d as I2
    args = types.SimpleNamespace(num_classes=E2E_CLASSES, img_size=16, z_spacing=1)
    net = StandInNet().to(dev)
    net.train()
    performance, mean_hd95 = I2.inference(net, inference_loader(dev), args)
    rec = fx["inference"]
    assert MC.rel(performance, rec["performance"]) <= MC.UNIT_RTOL and MC.rel(mean_hd95, rec["mean_hd95"]) <= MC.UNIT_RTOL
    assert net.training and net.batches == [4, 3]


def resize_inputs():
    image = np.ascontiguousarray(zoom_input("rows", "float32")[:, :, :16] / np.float32(2000.0))     # (3, 32, 16)
    label = np.ascontiguousarray(label_input("rows", "int64")[:, :, :16])
    return image, label


def check_resize_sample(fx, dev):
    from deformablelka_amd import inference2d as I2
    rec = fx["resize"]
    image, label = resize_inputs()
    _inp(rec, image)
    out = I2.resize_sample(torch.from_numpy(image).to(dev), torch.from_numpy(label).to(dev), 16)
    assert set(out) == {"image", "label"}
    img, lab = out["image"], out["label"]
    assert img.dtype == torch.float32 and tuple(img.shape) == (3, 1, 16, 16) and lab.dtype == torch.int64 and tuple(lab.shape) == (3, 1, 16, 16)
    assert torch.equal(lab.cpu(), rec["label"].to(torch.int64))
    err = float((img.cpu().double() - rec["image"].double()).abs().max())
    bound = 1e-6 * float(np.abs(image).max()) / STD
    print(f"resize_sample: max |out - ref| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert not lab[:, 0, -1, :].any() and bool((img[:, 0, -1, :] == -1).all())                      # 32 -> 16 overshoots: (0 - 0.5) / 0.5
    small_i, small_l = np.ascontiguousarray(image[:, :16]), np.ascontiguousarray(label[:, :16])   # already 16 x 16: Normalize only
    same = I2.resize_sample(torch.from_numpy(small_i).to(dev), torch.from_numpy(small_l).to(dev), 16)
    want = (torch.from_numpy(small_i) - torch.tensor(MEAN)) / torch.tensor(STD)
    assert torch.equal(same["image"].cpu()[:, 0], want) and torch.equal(same["label"].cpu()[:, 0], torch.from_numpy(small_l))


# ---- further checks ------------------------------------------------------------------------------------------------------------------------------
def check_unsupported(dev):
    import pytest
    from deformablelka_amd import inference2d as I2
    x = torch.from_numpy(zoom_input("ragged", "float32")).to(dev)
    for name, kw in (("output", dict(output=np.float32)), ("mode", dict(mode="nearest")), ("cval", dict(cval=1.0)),
                     ("prefilter", dict(prefilter=False)), ("grid_mode", dict(grid_mode=True)), ("order", dict(order=2)),
                     ("order", dict(order=5))):
        with pytest.raises(NotImplementedError, match=name):
            I2.zoom(x[0], 1.5, **kw)
    with pytest.raises(NotImplementedError, match="rank"):
        I2.zoom(x, 1.5)
    with pytest.raises(NotImplementedError, match="length 1"):
        I2.zoom(x[0], (1 / 19, 1.0))
    with pytest.raises(NotImplementedError, match="order"):
        I2.zoom_slices(x, (8, 8), order=2)
    with pytest.raises(NotImplementedError, match="test_save_path"):
        I2.test_single_volume(x[None], x[None].long(), StandInNet().to(dev), E2E_CLASSES, test_save_path="/nowhere")
    with pytest.raises(NotImplementedError):
        I2.zoom_slices(x.to(torch.int16), (8, 8), order=3, mean=0.5, std=0.5)


def check_containers(fx, dev):
    """numpy in gives numpy out; a host tensor comes back on the host; inputs are not written."""
    from deformablelka_amd import inference2d as I2
    call = ZOOM_CALLS[[c[0] for c in ZOOM_CALLS].index("ragged_float32_o3")]
    x = zoom_input("ragged", "float32")
    keep = x.copy()
    size = ZOOM_SHAPES["ragged"][1]
    out = I2.zoom_slices(x, size)
    assert isinstance(out, np.ndarray) and out.dtype == np.float32 and np.array_equal(x, keep)
    assert torch.equal(torch.from_numpy(out), run_zoom(call, dev)[1].cpu())
    host = I2.zoom_slices(torch.from_numpy(x), size)
    assert isinstance(host, torch.Tensor) and host.device.type == "cpu" and torch.equal(host, torch.from_numpy(out))
    z = I2.zoom(x[0].astype(np.int16), 1.5, order=1)
    assert isinstance(z, np.ndarray) and z.dtype == np.int16 and z.shape == (28, 32)
    lab8 = I2.zoom(label_input("ragged", "uint8")[0], 2, order=0)
    assert isinstance(lab8, np.ndarray) and lab8.dtype == np.uint8
    # the evaluator: numpy and host tensors, float labels, nothing written
    image, label = e2e_image(E2E_A[0], 29), e2e_label(E2E_A[0], 37)
    ki, kl = image.copy(), label.copy()
    net = StandInNet().to(dev)
    ml, pred = I2.test_single_volume(image[None], label[None].astype(np.float32), net, E2E_CLASSES, patch_size=list(E2E_A[1]), return_prediction=True)
    assert isinstance(pred, np.ndarray) and pred.dtype == np.float32 and np.array_equal(image, ki) and np.array_equal(label, kl)
    assert np.array_equal(pred.astype(np.int64), fx["e2e_a"]["prediction"].numpy().astype(np.int64))
    _metrics_close(ml, fx["e2e_a"]["metric_list"])
    ml2 = I2.test_single_volume(torch.from_numpy(image)[None], torch.from_numpy(label)[None].to(torch.int16), net, E2E_CLASSES,
                                patch_size=list(E2E_A[1]))
    assert isinstance(ml2, list) and ml2 == ml


def launches():
    from deformablelka_amd import ops
    return ops.zoom2d_launch_count() + ops.resample_launch_count() + ops.augment_launch_count()


def check_launch_counts(dev):
    from deformablelka_amd import inference2d as I2, ops
    x = torch.from_numpy(zoom_input("rows", "float32")).to(dev)
    x5 = torch.cat([x, x[:2]])
    counts = {}
    for order in (0, 1, 3):
        for n, t in ((1, x[:1]), (5, x5)):
            before = launches()
            I2.zoom_slices(t, (16, 24), order=order)
            counts[order, n] = launches() - before
        assert counts[order, 1] == counts[order, 5] > 0
    assert counts[0, 1] == 1 and counts[1, 1] == 1 and counts[3, 1] == 4      # cast, two prefilter passes, evaluation
    for n in (1, 5):
        logits = torch.from_numpy(logits_input("up", 9)).to(dev)
        logits = torch.cat([logits, logits[:2]])[:n]
        idx = I2._index_tables((16, 24), (32, 21), logits.device)
        before = ops.zoom2d_launch_count()
        ops.zoom2d_argmax(logits, (32, 21), idx)
        assert ops.zoom2d_launch_count() - before == 1


def check_training_flag(dev):
    from deformablelka_amd import inference2d as I2
    image = torch.from_numpy(e2e_image(E2E_A[0], 29)).to(dev)
    for flag in (True, False):
        net = StandInNet().to(dev)
        net.train(flag)
        I2.predict_volume(image, net, E2E_A[1])
        assert net.training is flag

        def boom(x):
            raise ValueError("net")
        net.forward = boom
        try:
            I2.predict_volume(image, net, E2E_A[1])
        except ValueError:
            pass
        assert net.training is flag
