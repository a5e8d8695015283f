"""TEST INFRASTRUCTURE — the cases, builders and checks of deformablelka_amd.augmentation, shared by tests/test_augmentation_emu.py (wavefront
emulator, CPU suite) and tests/test_augmentation_gpu.py (MI355X).  The expected results are in tests/golden/reference_augmentation.pt,
recorded by tests/golden/make_golden_augmentation.py from the scipy restatement tests/augmentation_ref.py.  Nothing here imports scipy.

The INPUTS are rebuilt from tests/resampling_cases.py's integer hash (IEEE operations only: the same bits on every machine); the fixture holds
their SHA-256 and every check compares it first.

Bounds.  Spatial values: resampling_cases.check_values' (float64 inside): equal at order 0, 2e-6 max|x| at order 1, 1e-6 max|x| at order 3,
integers within 1; cells within 1e-9 of a border are exempt under 'constant' (recorded, at most 0.1 %).  Labels: equal, except where a label's
weight is within GAP of 0.5 (recorded, at most 1 %).  Blur and the point-wise stages: K * 2^-24 * max|x|, K from a float32 restatement with
another summation order, see BLUR_K and POINTWISE_K."""
import os

import numpy as np
import torch

from tests import resampling_cases as RC

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "reference_augmentation.pt")
GAP = RC.GAP
EPS_BORDER = 1e-9

# Largest error of the float32 restatement of the blur (augmentation_ref.gaussian_blur_float32: float32 products and sums, plain left-to-right
# correlation, against scipy's float64 symmetric form) on the cases below, in units of 2^-24 max|x|: 2.24 (make_golden_augmentation.py
# prints it).  The product sums in float64 and rounds once per axis, so it owes at most 3 * 0.5 units itself.  K = 4: the measured 2.24 with
# a margin of 1.76 units.
BLUR_K = 4.0
# The same for the point-wise stages.  The product evaluates every stage in float64 from float64 statistics and rounds once to the storage
# type: 0.5 unit per stage relative to the value, on values of up to 1.25 max|x| after the brightness stage, so five stages owe less than
# 3.2 units.  The float32 restatement of the chain (noise, brightness, contrast, two gammas with retain_stats; float32 arithmetic and
# statistics throughout, make_golden_augmentation.py) is off by 8.61 units.  K = 12: the measured 8.61 with a margin of 3.39 units.
POINTWISE_K = 12.0

SRC, PATCH = (2, 2, 11, 19, 14), (8, 12, 10)
BLUR_SHAPES = {"blur": (1, 3, 9, 13, 11), "blur_short": (1, 3, 3, 13, 2)}     # blur_short: axes shorter than the radius 4, reflect wraps twice
POINT_SHAPE = (2, 2, 7, 9, 130)
DS_SHAPE, DS_SCALES = (2, 1, 8, 12, 10), [[1, 1, 1], [1, .5, .5], [.5, .25, .25]]
PIPE_SRC, PIPE_PATCH = (2, 1, 12, 20, 16), (8, 12, 10)


def image(shape, salt, dtype=np.float32):
    x = (RC.smooth(RC.noise((shape[0] * shape[1],) + tuple(shape[2:]), salt)).reshape(shape) - 0.5) * 2000.0
    return np.trunc(x).astype(dtype) if np.dtype(dtype).kind == "i" else x.astype(dtype)


def blocky_labels(shape, salt, labels=(0, 1, 2, 4), block=3, dtype=np.int16):
    """Blocks of `block` cells with one label each: most cells have a clear majority among their 8 neighbours."""
    coarse = tuple(-(-n // block) for n in shape[2:])
    pick = np.floor(RC.noise((shape[0] * shape[1],) + coarse, salt) * float(len(labels))).astype(np.int64).reshape(shape[:2] + coarse)
    lab = np.asarray(labels)[pick]
    for ax in (2, 3, 4):
        lab = np.repeat(lab, block, ax)
    return np.ascontiguousarray(lab[:, :, :shape[2], :shape[3], :shape[4]]).astype(dtype)


def rotation(ax, ay, az):
    def c(a):
        return np.cos(a)

    def s(a):
        return np.sin(a)

    rx = np.array([[1, 0, 0], [0, c(ax), -s(ax)], [0, s(ax), c(ax)]])
    ry = np.array([[c(ay), 0, s(ay)], [0, 1, 0], [-s(ay), 0, c(ay)]])
    rz = np.array([[c(az), -s(az), 0], [s(az), c(az), 0], [0, 0, 1]])
    return np.dot(np.dot(np.dot(np.identity(3), rx), ry), rz)


def spatial_record(scale, src=SRC, lb=(1, 3, 2), angle=30.0):
    """Sample 0: a plain crop at lb.  Sample 1: `angle` degrees about all three axes, one scale factor, the centre of the source."""
    a = angle / 360.0 * 2.0 * np.pi
    return {"modified": np.array([False, True]), "angles": np.array([[0., 0., 0.], [a, a, a]]),
            "rotation": np.stack([np.identity(3), rotation(a, a, a)]), "scale": np.array([[1., 1., 1.], [scale, scale, scale]]),
            "center": np.array([[0., 0., 0.], [src[2] / 2. - 0.5, src[3] / 2. - 0.5, src[4] / 2. - 0.5]]),
            "crop_lb": np.array([list(lb), [0, 0, 0]])}


# (id, input dtype, order, mode, scale)
SPATIAL_CALLS = [(f"s{str(scale).replace('.', '')}_o{order}_{mode}", "float32", order, mode, scale)
                 for scale in (0.7, 1.4) for order in (0, 1, 3) for mode in ("constant", "nearest")]
SPATIAL_CALLS += [("bf16_o1_constant", "bfloat16", 1, "constant", 1.4), ("int16_o3_nearest", "int16", 3, "nearest", 0.7),
                  ("int16_o0_constant", "int16", 0, "constant", 1.4)]
# (id, order, mode, scale); cval -1
LABEL_CALLS = [("l14_o0", 0, "constant", 1.4), ("l14_o1", 1, "constant", 1.4), ("l07_o1", 1, "constant", 0.7), ("l14_o1_nearest", 1, "nearest", 1.4)]


def spatial_input(dtype):
    if dtype == "bfloat16":
        return torch.from_numpy(image(SRC, 2)).to(torch.bfloat16)
    return torch.from_numpy(image(SRC, 2 if dtype == "float32" else 5, np.dtype(dtype)))


def label_input():
    return blocky_labels(SRC, 3)


def halves_case():
    """Labels in slabs along W and a map that shifts by exactly half a voxel along W: every interior cell weighs two neighbours 0.5 each.
    Source column pairs (w, w + 1): (1, 3) -> 3 (both reach 0.5, the later label wins), (3, 3) -> 3, (3, 0) -> 3 (0.5 >= 0.5), (0, 2) -> 2."""
    seg = np.zeros((1, 1, 4, 5, 6), np.int16)
    seg[..., 0], seg[..., 1], seg[..., 2], seg[..., 3], seg[..., 4], seg[..., 5] = 1, 3, 3, 0, 2, 2
    rec = {"modified": np.array([True]), "rotation": np.identity(3)[None], "scale": np.ones((1, 3)),
           "center": np.array([[1.5, 2.0, 2.5]]), "crop_lb": np.zeros((1, 3), np.int64)}
    # patch (4, 5, 5): coords along W = arange(5) - 2 + 2.5 = 0.5 .. 4.5
    want = np.broadcast_to(np.array([3, 3, 3, 2, 2], np.int16), (1, 1, 4, 5, 5))
    return seg, rec, (4, 5, 5), want


BLUR_SIGMA = np.array([[0.5, 0.0, 0.77]]), np.array([[1.0, 0.77, 0.0]])          # two calls per shape: every sigma, a skipped channel in each


def blur_records():
    return [{"apply": np.array([True]), "sigma": s} for s in BLUR_SIGMA]


def point_input():
    x = image(POINT_SHAPE, 7)
    x[1, 1] = 3.25                      # a constant channel: range 0
    return x


def point_records():
    """Stage records for POINT_SHAPE.  The `_one` records flag sample 0 only: sample 1 has to come back bit for bit."""
    one, both = np.array([True, False]), np.array([True, True])
    return {
        "noise": {"apply": one, "variance": np.array([0.07, 0.0])},
        "brightness": {"apply": one, "multiplier": np.array([[0.8, 1.2], [1.0, 1.0]])},
        "additive": {"apply": one, "add": np.array([[12.5, -3.0], [0.0, 0.0]])},
        "contrast": {"apply": one, "factor": np.array([[1.25, 0.75], [1.0, 1.0]])},          # 1.25 clips on both sides
        "gamma": {"apply": one, "gamma": np.array([[0.7, 1.5], [1.0, 1.0]])},
        "chain": {"noise": {"apply": both, "variance": np.array([0.07, 0.1])},
                  "brightness": {"apply": both, "multiplier": np.array([[0.8, 1.2], [1.25, 0.75]])},
                  "contrast": {"apply": both, "factor": np.array([[1.25, 0.75], [1.1, 0.9]])},
                  "gamma_inverted": {"apply": both, "gamma": np.array([[0.7, 1.5], [1.3, 0.8]])},
                  "gamma": {"apply": both, "gamma": np.array([[1.4, 0.9], [0.75, 1.2]])},
                  "mirror": {"flip": np.array([[True, False, True], [False, True, True]])}},
    }


def point_noise():
    """A fixed 'normal' field for the noise stage (scaled; what normal(0, variance) would be)."""
    return ((RC.noise(POINT_SHAPE, 11) - 0.5) * 40.0).astype(np.float32)


def pipeline_params():
    """The trainer's data_aug_params (default_3D_augmentation_params after setup_DA_params); the fixture stores the values read from the
    reference's files and the test compares them with these."""
    r = 30. / 360 * 2. * np.pi
    return {"selected_data_channels": None, "selected_seg_channels": [0], "do_elastic": False, "elastic_deform_alpha": (0., 900.),
            "elastic_deform_sigma": (9., 13.), "p_eldef": 0.2, "do_scaling": True, "scale_range": (0.7, 1.4),
            "independent_scale_factor_for_each_axis": False, "p_independent_scale_per_axis": 1, "p_scale": 0.2, "do_rotation": True,
            "rotation_x": (-r, r), "rotation_y": (-r, r), "rotation_z": (-r, r), "rotation_p_per_axis": 1, "p_rot": 0.2, "random_crop": False,
            "random_crop_dist_to_border": None, "do_gamma": True, "gamma_retain_stats": True, "gamma_range": (0.7, 1.5), "p_gamma": 0.3,
            "do_mirror": True, "mirror_axes": (0, 1, 2), "dummy_2D": False, "mask_was_used_for_normalization": None,
            "border_mode_data": "constant", "all_segmentation_labels": None, "move_last_seg_chanel_to_data": False,
            "cascade_do_cascade_augmentations": False, "do_additive_brightness": False, "additive_brightness_p_per_sample": 0.15,
            "additive_brightness_p_per_channel": 0.5, "additive_brightness_mu": 0.0, "additive_brightness_sigma": 0.1}


def pipeline_records():
    """Every stage on, for both samples; sample 0 keeps a plain crop in the spatial stage."""
    both = np.array([True, True])
    rec = {"spatial": spatial_record(0.9, PIPE_SRC, (2, 4, 3), 20.0), "noise": {"apply": both, "variance": np.array([0.05, 0.09])},
           "blur": {"apply": both, "sigma": np.array([[0.6], [0.9]])}, "brightness": {"apply": both, "multiplier": np.array([[0.8], [1.2]])},
           "contrast": {"apply": both, "factor": np.array([[1.2], [0.8]])}, "lowres": {"apply": both, "zoom": np.array([[0.6], [0.85]])},
           "gamma_inverted": {"apply": both, "gamma": np.array([[0.8], [1.3]])}, "gamma": {"apply": both, "gamma": np.array([[1.4], [0.75]])},
           "mirror": {"flip": np.array([[True, False, True], [False, True, False]])}}
    return rec


def pipeline_inputs():
    data = image(PIPE_SRC, 13)
    seg = blocky_labels(PIPE_SRC, 14, labels=(-1, 0, 1, 2)).astype(np.float32)
    noise = ((RC.noise((2, 1) + PIPE_PATCH, 15) - 0.5) * 30.0).astype(np.float32)
    return data, seg, noise


digest = RC.digest


def load_fixture():
    return torch.load(FIXTURE, weights_only=False)


def unpack(bits, shape):
    return torch.from_numpy(np.unpackbits(bits.numpy())[:int(np.prod(shape))].reshape(shape).astype(bool))


def _as_numpy(t):
    return t.float().numpy() if t.dtype == torch.bfloat16 else t.numpy()


# ---- checks ------------------------------------------------------------------------------------------------------------------------------------
def run_spatial(call, dev):
    from deformablelka_amd import augmentation as A
    cid, dtype, order, mode, scale = call
    x = spatial_input(dtype).to(dev)
    keep = x.clone()
    out, none = A.augment_spatial(x, None, PATCH, order_data=order, border_mode_data=mode, border_cval_data=0, params=spatial_record(scale))
    assert none is None and torch.equal(x, keep)                                              # the input is not written to
    assert out.dtype == x.dtype and out.device == x.device and tuple(out.shape) == SRC[:2] + PATCH
    return x, out


def check_spatial(fx, call, dev):
    cid, dtype, order, mode, scale = call
    rec = fx["spatial"][cid]
    x, out = run_spatial(call, dev)
    assert digest(_as_numpy(x.cpu())) == rec["input"], f"spatial/{cid}: the rebuilt input differs from the recorded one"
    lb = spatial_record(scale)["crop_lb"][0]
    box = x[0, :, lb[0]:lb[0] + PATCH[0], lb[1]:lb[1] + PATCH[1], lb[2]:lb[2] + PATCH[2]]
    assert torch.equal(out[0], box)                                                           # the plain crop: bit for bit
    want, got = rec["out"], out[1].cpu()
    exempt = unpack(rec["exempt"], tuple(want.shape[1:]))[None].expand_as(want) if mode == "constant" else torch.zeros(want.shape, dtype=torch.bool)
    frac = float(exempt.float().mean())
    assert frac <= 0.001, f"spatial/{cid}: {100 * frac:.3f} % of the cells are exempt"
    scale_x = float(x.abs().max())
    if not x.is_floating_point():
        err = int((got.to(torch.int64) - want.to(torch.int64)).abs()[~exempt].max())
        print(f"spatial/{cid}: integer, max |out - ref| = {err}")
        assert err <= (0 if order == 0 else 1)
        return
    err = float((got.double() - want.double()).abs()[~exempt].max())
    bound = 0.0 if order == 0 else (1e-6 if order == 3 else 2e-6) * scale_x
    print(f"spatial/{cid}: max |out - ref| = {err:.3e}, bound {bound:.3e}, exempt {int(exempt.sum())}")
    assert err <= bound


def run_labels(call, dev):
    from deformablelka_amd import augmentation as A
    cid, order, mode, scale = call
    seg = torch.from_numpy(label_input()).to(dev)
    data = torch.zeros(SRC, dtype=torch.float32, device=dev)
    _, out = A.augment_spatial(data, seg, PATCH, order_data=0, order_seg=order, border_mode_seg=mode, border_cval_seg=-1,
                               params=spatial_record(scale))
    assert out.dtype == seg.dtype and out.device == seg.device and tuple(out.shape) == SRC[:2] + PATCH
    return seg, out


def check_labels(fx, call, dev):
    cid, order, mode, scale = call
    rec = fx["labels"][cid]
    seg, out = run_labels(call, dev)
    assert digest(seg.cpu().numpy()) == rec["input"]
    want = rec["out"].to(out.dtype)
    close = unpack(rec["close"], tuple(want.shape))
    frac = float(close.float().mean())
    print(f"labels/{cid}: {100 * frac:.3f} % of the cells within {GAP} of the threshold")
    assert frac <= 0.01
    assert torch.equal(out.cpu()[~close], want[~close])
    assert rec["absent_label"] == 3 and not bool((out == 3).any()) and len(torch.unique(out)) >= 3


def check_halves(dev):
    from deformablelka_amd import augmentation as A
    seg, rec, patch, want = halves_case()
    data = np.zeros(seg.shape, np.float32)
    _, out = A.augment_spatial(data, seg, patch, order_data=0, order_seg=1, border_mode_seg="constant", border_cval_seg=-1, params=rec)
    assert np.array_equal(out.cpu().numpy(), want)


def run_blur(name, i, dev):
    from deformablelka_amd import augmentation as A
    x = torch.from_numpy(image(BLUR_SHAPES[name], 6)).to(dev)
    return x, A.augment_gaussian_blur(x, (0.5, 1.), params=blur_records()[i])


def check_blur(fx, name, i, dev):
    rec = fx["blur"][f"{name}_{i}"]
    x, out = run_blur(name, i, dev)
    assert digest(x.cpu().numpy()) == rec["input"] and out.dtype == x.dtype and out.shape == x.shape
    sigma = BLUR_SIGMA[i][0]
    for c in range(3):
        if sigma[c] == 0:
            assert torch.equal(out[0, c], x[0, c])                                            # a skipped channel: bit for bit
    err = float((out.cpu().double() - rec["out"].double()).abs().max())
    bound = BLUR_K * 2.0 ** -24 * float(x.abs().max())
    print(f"blur/{name}_{i}: max |out - ref| = {err:.3e}, bound {bound:.3e} ({err / (2.0 ** -24 * float(x.abs().max())):.2f} units)")
    assert err <= bound


def run_point(stage, dev):
    """The stage alone (sample 0 flagged) or the chain on POINT_SHAPE."""
    from deformablelka_amd import augmentation as A
    x = torch.from_numpy(point_input()).to(dev)
    noise = torch.from_numpy(point_noise()).to(dev)
    r = point_records()
    if stage == "noise":
        return x, A.augment_gaussian_noise(x, params=r["noise"], noise=noise)
    if stage == "brightness":
        return x, A.augment_brightness_multiplicative(x, (0.75, 1.25), params=r["brightness"])
    if stage == "additive":
        return x, A.augment_brightness_additive(x, params=r["additive"])
    if stage == "contrast":
        return x, A.augment_contrast(x, params=r["contrast"])
    if stage in ("gamma", "gamma_retain", "gamma_inverted", "gamma_inverted_retain"):
        return x, A.augment_gamma(x, (0.7, 1.5), invert_image="inverted" in stage, retain_stats="retain" in stage, params=r["gamma"])
    assert stage == "chain"
    c = r["chain"]
    y = A.augment_gaussian_noise(x, params=c["noise"], noise=noise)
    y = A.augment_brightness_multiplicative(y, params=c["brightness"])
    y = A.augment_contrast(y, params=c["contrast"])
    y = A.augment_gamma(y, invert_image=True, retain_stats=True, params=c["gamma_inverted"])
    y = A.augment_gamma(y, invert_image=False, retain_stats=True, params=c["gamma"])
    y, _ = A.augment_mirroring(y, None, params=c["mirror"])
    return x, y


POINT_STAGES = ["noise", "brightness", "additive", "contrast", "gamma", "gamma_retain", "gamma_inverted", "gamma_inverted_retain", "chain"]


def check_point(fx, stage, dev):
    rec = fx["point"][stage]
    x, out = run_point(stage, dev)
    assert digest(x.cpu().numpy()) == fx["point"]["input"] and out.dtype == x.dtype and out.shape == x.shape and out.device == x.device
    assert bool(torch.isfinite(out).all())                                                    # the constant channel (range 0) included
    if stage == "chain":
        got = out.cpu()
    else:
        assert torch.equal(out[1], x[1])                                                      # the sample that is not flagged: bit for bit
        got = out[0].cpu()
    scale = float(x.abs().max())
    err = float((got.double() - rec["out"].double()).abs().max())
    bound = POINTWISE_K * 2.0 ** -24 * scale
    print(f"point/{stage}: max |out - ref| = {err:.3e}, bound {bound:.3e} ({err / (2.0 ** -24 * scale):.2f} units)")
    assert err <= bound
    if stage == "contrast":
        lo, hi = float(x[0, 0].min()), float(x[0, 0].max())
        assert int((out[0, 0] == lo).sum()) > 1 and int((out[0, 0] == hi).sum()) > 1          # the clip bites on both sides


def check_stats(dev):
    """The statistics kernel against float64 torch sums: a row of 130 cells crosses a wave, a workgroup chunk and a tail."""
    from deformablelka_amd import ops
    x = torch.from_numpy(point_input()).to(dev)
    s = ops.augment_channel_stats(x).cpu()
    v = x.cpu().double().reshape(4, -1)
    mean = v.mean(1)
    assert torch.equal(s[:, 2], v.min(1).values) and torch.equal(s[:, 3], v.max(1).values)
    assert float((s[:, 0] - v.sum(1)).abs().max()) <= 1e-12 * float(v.abs().sum(1).max())
    assert float((s[:, 1] - ((v - mean[:, None]) ** 2).sum(1)).abs().max()) <= 1e-12 * float((v ** 2).sum(1).max())
    assert float(s[3, 1]) == 0.0                                                               # the constant channel
    big = torch.from_numpy(image((1, 2, 40, 40, 41), 8)).to(dev)                              # several workgroups per channel
    sb = ops.augment_channel_stats(big).cpu()
    vb = big.cpu().double().reshape(2, -1)
    assert float((sb[:, 0] - vb.sum(1)).abs().max()) <= 1e-12 * float(vb.abs().sum(1).max())
    assert torch.equal(sb, ops.augment_channel_stats(big).cpu())
    return s


# ---- every storage type through the gaussian, statistics and point-wise entries ----------------------------------------------------------------
# float32 (and int16 point-wise) run in the cases above.  Last axes of 6 (the last lane of a row holds fewer than 4 cells) and 8 (whole quads).
STORAGE_DTYPES = ("float64", "int16", "bfloat16")
STORAGE_SHAPES = ((1, 2, 3, 5, 6), (1, 2, 4, 3, 8))
STORAGE_SIGMA = np.array([[0.5, 0.77]])
# bfloat16 keeps 8 significant bits: two neighbouring values below max|x| are at most 2^-7 max|x| apart.  The references here round float64 to
# bfloat16 in one step, the kernels through float32 as torch's conversions do, so a stored value may land on the neighbour: one step per store.
BF16_STEP = 2.0 ** -7


def storage_input(shape, salt, dt, dev):
    t = torch.from_numpy(image(shape, salt, np.int16 if dt == "int16" else np.float64))
    return (t.to(torch.bfloat16) if dt == "bfloat16" else t).to(dev)


def check_blur_storage(dt, dev):
    """scipy's gaussian_filter in the storage type itself (augmentation_ref.gaussian_blur, what recorded the float32 fixture) at the float32
    cases' bound.  numpy has no bfloat16: there the float64 filter axis by axis, every axis' result rounded to bfloat16 as the kernel stores
    it between the axes; three stores, three steps."""
    import pytest
    ndimage = pytest.importorskip("scipy.ndimage")
    from deformablelka_amd import augmentation as A
    from tests import augmentation_ref as R
    rec = {"apply": np.array([True]), "sigma": STORAGE_SIGMA}
    for k, shape in enumerate(STORAGE_SHAPES):
        x = storage_input(shape, 12 + k, dt, dev)
        out = A.augment_gaussian_blur(x, params=rec)
        assert out.dtype == x.dtype and out.shape == x.shape and out.device == x.device
        scale = float(x.double().abs().max())
        if dt == "bfloat16":
            ref = x.cpu().clone()
            for c in range(shape[1]):
                for ax in range(3):
                    ref[0, c] = torch.from_numpy(ndimage.gaussian_filter1d(ref[0, c].double().numpy(), float(STORAGE_SIGMA[0, c]), axis=ax)).to(torch.bfloat16)
            bound = 3 * BF16_STEP * scale
        else:
            ref = torch.from_numpy(R.gaussian_blur(x.cpu().numpy(), rec))
            bound = BLUR_K * 2.0 ** -24 * scale
        err = float((out.cpu().double() - ref.double()).abs().max())
        print(f"blur/{dt}_{shape[-1]}: max |out - ref| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound


def check_stats_storage(dt, dev):
    """check_stats' float64 torch sums and bounds, the input in every storage type."""
    from deformablelka_amd import ops
    for k, shape in enumerate(STORAGE_SHAPES):
        x = storage_input(shape, 14 + k, dt, dev)
        s = ops.augment_channel_stats(x).cpu()
        v = x.cpu().double().reshape(shape[0] * shape[1], -1)
        mean = v.mean(1)
        assert torch.equal(s[:, 2], v.min(1).values) and torch.equal(s[:, 3], v.max(1).values)
        assert float((s[:, 0] - v.sum(1)).abs().max()) <= 1e-12 * float(v.abs().sum(1).max())
        assert float((s[:, 1] - ((v - mean[:, None]) ** 2).sum(1)).abs().max()) <= 1e-12 * float((v ** 2).sum(1).max())


def check_point_storage(dt, dev):
    """The additive stage against its float64 restatement (augmentation_ref.scale_add: x * 1 + add) at the float32 stages' bound; bfloat16:
    that result rounded to bfloat16, one store, one step."""
    from deformablelka_amd import augmentation as A
    rec = {"apply": np.array([True]), "add": np.array([[12.5, -3.0]])}
    for k, shape in enumerate(STORAGE_SHAPES):
        x = storage_input(shape, 16 + k, dt, dev)
        out = A.augment_brightness_additive(x, params=rec)
        assert out.dtype == x.dtype and out.shape == x.shape and out.device == x.device
        ref = x.cpu().double() * 1.0 + torch.from_numpy(rec["add"]).reshape(1, 2, 1, 1, 1)
        scale = float(ref.abs().max())
        bound = BF16_STEP * scale if dt == "bfloat16" else POINTWISE_K * 2.0 ** -24 * scale
        err = float((out.cpu().double() - ref.to(out.dtype).double()).abs().max())
        print(f"point/{dt}_{shape[-1]}: max |out - ref| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound


def check_mirror(dev):
    from deformablelka_amd import augmentation as A
    x = torch.from_numpy(image((2, 2, 5, 6, 7), 9)).to(dev)
    seg = torch.from_numpy(blocky_labels((2, 1, 5, 6, 7), 10, block=2)).to(dev)
    for mask in range(8):
        flip = np.array([[bool(mask & 1), bool(mask & 2), bool(mask & 4)], [False, False, False]])
        out, out_seg = A.augment_mirroring(x, seg, params={"flip": flip})
        dims = [1 + a for a in range(3) if flip[0, a]]
        assert torch.equal(out[0], torch.flip(x[0], dims) if dims else x[0]) and torch.equal(out[1], x[1])
        assert torch.equal(out_seg[0], torch.flip(seg[0], dims) if dims else seg[0]) and torch.equal(out_seg[1], seg[1])
        assert out_seg.dtype == seg.dtype


def run_ds(dev):
    from deformablelka_amd import augmentation as A
    seg = torch.from_numpy(blocky_labels(DS_SHAPE, 12, labels=(0, 1, 2, 5), block=2).astype(np.float32)).to(dev)
    return seg, A.downsample_seg_for_ds_transform2(seg, DS_SCALES, 0, 0)


def check_ds(fx, dev):
    seg, out = run_ds(dev)
    rec = fx["ds"]
    assert digest(seg.cpu().numpy()) == rec["input"] and len(out) == 3 and out[0] is not None
    for got, want in zip(out, rec["out"]):
        assert got.dtype == seg.dtype and torch.equal(got.cpu(), want.to(got.dtype))
    assert [tuple(o.shape) for o in out] == [(2, 1, 8, 12, 10), (2, 1, 8, 6, 5), (2, 1, 4, 3, 2)]


def run_pipeline(dev, seed=5):
    from deformablelka_amd import augmentation as A
    data, seg, noise = pipeline_inputs()
    aug = A.MoreDAAugmentation(PIPE_PATCH, pipeline_params(), deep_supervision_scales=DS_SCALES, seed=seed)
    d, s, n = torch.from_numpy(data).to(dev), torch.from_numpy(seg).to(dev), torch.from_numpy(noise).to(dev)
    keep = d.clone(), s.clone()
    before = A.launch_count()
    out = aug(d, s, records=pipeline_records(), noise=n)
    launches = A.launch_count() - before
    assert torch.equal(d, keep[0]) and torch.equal(s, keep[1])                                # the inputs are not written to
    return out, launches


# 2 channels x (pad + 3 prefilters) + spatial values + spatial labels; noise 1; blur 3; brightness 1; contrast 4 + 1; low resolution 2 channels x
# (1 down + 5 up); two gammas with retain_stats 2 x (4 + 1 + 4 + 1); target 1; two deep-supervision maps 2
PIPELINE_LAUNCHES = 8 + 2 + 1 + 3 + 1 + 5 + 12 + 20 + 1 + 2


def check_pipeline(fx, dev):
    rec = fx["pipeline"]
    assert rec["params"] == {k: (list(v) if isinstance(v, tuple) else v) for k, v in pipeline_params().items()}
    out, launches = run_pipeline(dev)
    data, target = out["data"], out["target"]
    assert data.dtype == torch.float32 and tuple(data.shape) == (2, 1) + PIPE_PATCH
    assert isinstance(target, list) and [tuple(t.shape) for t in target] == [(2, 1, 8, 12, 10), (2, 1, 8, 6, 5), (2, 1, 4, 3, 2)]
    assert all(t.dtype == torch.float32 and t.device == data.device for t in target)
    assert all(not bool((t == -1).any()) for t in target)
    print(f"pipeline: {launches} launches")
    assert launches == PIPELINE_LAUNCHES
    scale = float(rec["scale"])
    # the summed bounds: order 3 spatial 1e-6, then blur BLUR_K and six point-wise stages POINTWISE_K each in units of 2^-24, each on values of at
    # most 1.25 x the input's range (brightness), and the low-resolution pair at resampling's 1e-6 for order 3
    bound = (1e-6 + 1e-6 + (BLUR_K + 6 * POINTWISE_K) * 2.0 ** -24) * 1.25 * scale
    exempt = unpack(rec["exempt"], tuple(data.shape))
    err = float((data.cpu().double() - rec["data"].double()).abs()[~exempt].max())
    print(f"pipeline: max |data - ref| = {err:.3e}, bound {bound:.3e}, exempt {int(exempt.sum())}")
    assert float(exempt.float().mean()) <= 0.001 and err <= bound
    close = unpack(rec["close"], tuple(target[0].shape))
    assert float(close.float().mean()) <= 0.01
    assert torch.equal(target[0].cpu()[~close], rec["target"][0][~close])
    if not bool(close.any()):
        for got, want in zip(target[1:], rec["target"][1:]):
            assert torch.equal(got.cpu(), want)
    again, _ = run_pipeline(dev)
    assert torch.equal(again["data"], data) and all(torch.equal(a, b) for a, b in zip(again["target"], target))
    return out


def check_seeded_runs(dev):
    """With a seed, two instances draw the same records and the same noise: bitwise equal batches, nothing handed in."""
    from deformablelka_amd import augmentation as A
    data, seg, _ = pipeline_inputs()
    d, s = torch.from_numpy(data).to(dev), torch.from_numpy(seg).to(dev)
    params = dict(pipeline_params(), p_rot=1.0, p_scale=1.0, p_gamma=1.0)
    outs = []
    for _ in range(2):
        aug = A.MoreDAAugmentation(PIPE_PATCH, params, deep_supervision_scales=DS_SCALES, seed=1234)
        rec = aug.draw(2, PIPE_SRC[2:], 1)
        rec["noise"]["apply"][:] = True
        rec["noise"]["variance"][:] = 0.05
        outs.append(aug(d, s, records=rec))
    assert torch.equal(outs[0]["data"], outs[1]["data"]) and all(torch.equal(a, b) for a, b in zip(outs[0]["target"], outs[1]["target"]))
    assert bool(torch.isfinite(outs[0]["data"]).all())


def check_unsupported(dev):
    import pytest
    from deformablelka_amd import augmentation as A
    base = pipeline_params()
    for key, value in (("do_elastic", True), ("dummy_2D", True), ("selected_data_channels", [0]), ("move_last_seg_chanel_to_data", True),
                       ("cascade_do_cascade_augmentations", True), ("mask_was_used_for_normalization", {0: True})):
        with pytest.raises(NotImplementedError, match=key):
            A.MoreDAAugmentation(PIPE_PATCH, dict(base, **{key: value}))
    with pytest.raises(NotImplementedError, match="regions"):
        A.MoreDAAugmentation(PIPE_PATCH, base, regions=[[1, 2]])
    with pytest.raises(NotImplementedError, match="soft_ds"):
        A.MoreDAAugmentation(PIPE_PATCH, base, soft_ds=True)
    x = torch.zeros((1, 1, 6, 6, 6), device=dev)
    with pytest.raises(NotImplementedError, match="do_elastic_deform"):
        A.augment_spatial(x, None, (4, 4, 4), do_elastic_deform=True)
    with pytest.raises(NotImplementedError, match="order_data"):
        A.augment_spatial(x, None, (4, 4, 4), order_data=2)
    with pytest.raises(NotImplementedError, match="order_seg"):
        A.augment_spatial(x, x, (4, 4, 4), order_seg=3)
    with pytest.raises(NotImplementedError, match="border_mode_data"):
        A.augment_spatial(x, None, (4, 4, 4), border_mode_data="reflect")
    with pytest.raises(NotImplementedError, match="border_cval_seg"):
        A.augment_spatial(x, x, (4, 4, 4), order_seg=1, border_cval_seg=1)
    with pytest.raises(NotImplementedError, match="per_channel"):
        A.augment_gamma(x, per_channel=False)
    with pytest.raises(NotImplementedError, match="preserve_range"):
        A.augment_contrast(x, preserve_range=False)
    with pytest.raises(NotImplementedError, match="selected_seg_channels"):
        A.MoreDAAugmentation((4, 4, 4), dict(base, selected_seg_channels=[1]))(x, torch.cat([x, x], 1))


def check_containers(dev):
    """numpy in, a device tensor out in the input's dtype; float16 and int32 go through the kernels' types and come back."""
    from deformablelka_amd import augmentation as A
    x = image((1, 1, 6, 7, 9), 16)
    keep = x.copy()
    rec = {"modified": np.array([False]), "rotation": np.identity(3)[None], "scale": np.ones((1, 3)), "center": np.zeros((1, 3)),
           "crop_lb": np.array([[1, 2, 3]])}
    out, _ = A.augment_spatial(x, None, (4, 4, 4), params=rec)
    assert isinstance(out, torch.Tensor) and out.dtype == torch.float32 and np.array_equal(x, keep)
    assert np.array_equal(out.cpu().numpy(), x[:, :, 1:5, 2:6, 3:7])
    for dtype in (torch.float16, torch.int32, torch.float64):
        t = torch.from_numpy(np.trunc(x / 8)).to(dtype).to(dev)
        o, _ = A.augment_spatial(t, None, (4, 4, 4), params=rec)
        assert o.dtype == dtype and torch.equal(o, t[:, :, 1:5, 2:6, 3:7])
