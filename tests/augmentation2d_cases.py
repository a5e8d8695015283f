"""TEST INFRASTRUCTURE — the cases, builders and checks of the dummy-2D branch of deformablelka_amd.augmentation (the ACDC trainer's
anisotropic patch: the spatial step on (B, C D, H, W) planes, the low-resolution stage with ignore_axes=(0,)), shared by
tests/test_augmentation2d_emu.py (wavefront emulator, CPU suite) and tests/test_augmentation2d_gpu.py (MI355X).  The expected results are in
tests/golden/reference_augmentation2d.pt, recorded by tests/golden/make_golden_augmentation2d.py from the scipy restatement
tests/augmentation2d_ref.py.  Nothing here imports scipy.

The INPUTS are rebuilt from tests/resampling_cases.py's integer hash; the fixture holds their SHA-256 and every check compares it first.

Bounds: those of tests/augmentation_cases.py.  Spatial values equal at order 0, 2e-6 max|x| at order 1, 1e-6 max|x| at order 3, integers within
1; cells within 1e-9 of a border are exempt under 'constant' (at most 0.1 %).  Labels equal, except where a label's weight is within GAP of 0.5
(at most 1 %).  Both sets are recorded in the fixture and are EMPTY on every case here (the generator asserts it).  The low-resolution stage:
resampling's 1e-6 max|x| (order 3 on the way up).  The pipeline: the summed bound of augmentation_cases.check_pipeline."""
import os

import numpy as np
import torch

from tests import augmentation_cases as C3
from tests import resampling_cases as RC

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "reference_augmentation2d.pt")
GAP = RC.GAP
EPS_BORDER = 1e-9

# W = 10: two full lanes of 4 cells and one of 2; P = C D = 10 planes per sample; more than one workgroup (2 x 10 x 12 x 3 = 720 lanes)
SRC, PATCH = (2, 2, 5, 19, 14), (12, 10)
PLANES = (SRC[0], SRC[1] * SRC[2]) + SRC[3:]
CROP_LB, CENTER = (3, 2), (9.0, 6.5)
# (angle in degrees, scale_y, scale_x); the first and the last sample 18 % and 10 % of the cells outside the source
VARIANTS = {"a30_s14": (30.0, 1.4, 1.4), "a30_s07": (30.0, 0.7, 0.7), "a170_s14_09": (170.0, 1.4, 0.9), "am95_s07_12": (-95.0, 0.7, 1.2)}
OUTSIDE = {"a30_s14": 0.18, "am95_s07_12": 0.10}
TINY_SRC, TINY_PATCH = (1, 1, 2, 4, 3), (5, 3)                 # W below the 4 cells of a lane; the extension wraps on axes of 4 and 3 cells
LOW_SHAPE = (2, 2, 6, 12, 10)
LOW_ZOOM = np.array([[0.5, 0.77], [0.0, 0.77]])
PIPE_SRC, PIPE_PATCH = (2, 1, 8, 20, 16), (12, 10)
DS_SCALES = [[1, 1, 1], [1, .5, .5], [.5, .25, .25]]

# The 2-D spatial step (values at order 3 plus labels), whatever B, C and D are: the batch's stack of planes is one volume, so 1 pad (the
# cast to float64 under 'constant') + 2 in-plane prefilters, then the values and the labels
SPATIAL2D_LAUNCHES = 3 + 1 + 1
# The chain: the spatial step; noise 1; blur 3; brightness 1; contrast 4 + 1; low resolution 2 channels x (1 down + 5 up: pad, 3 prefilters (the
# depth axis is not resized but resize filters it), evaluation); two gammas with retain_stats 2 x (4 + 1 + 4 + 1); target 1; two
# deep-supervision maps 2
PIPELINE2D_LAUNCHES = SPATIAL2D_LAUNCHES + 1 + 3 + 1 + 5 + 12 + 20 + 1 + 2

image = C3.image
digest = RC.digest
unpack = C3.unpack


def rotation_2d(a):
    return np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])


def blocky_labels_inplane(shape, salt, labels=(0, 1, 2, 4), block=3, dtype=np.int16):
    """(B, C, D, H, W): blocks of `block` x `block` cells in every plane with one label each, every plane on its own."""
    coarse = (shape[2],) + tuple(-(-n // block) for n in shape[3:])
    pick = np.floor(RC.noise((shape[0] * shape[1],) + coarse, salt) * float(len(labels))).astype(np.int64).reshape(shape[:2] + coarse)
    lab = np.asarray(labels)[pick]
    for ax in (3, 4):
        lab = np.repeat(lab, block, ax)
    return np.ascontiguousarray(lab[:, :, :, :shape[3], :shape[4]]).astype(dtype)


def spatial_record(variant):
    """Sample 0: a plain crop at CROP_LB.  Sample 1: one in-plane rotation and two scale factors about CENTER."""
    angle, sy, sx = VARIANTS[variant]
    a = angle / 360.0 * 2.0 * np.pi
    return {"modified": np.array([False, True]), "angles": np.array([[0.], [a]]), "rotation": np.stack([np.identity(2), rotation_2d(a)]),
            "scale": np.array([[1., 1.], [sy, sx]]), "center": np.array([[0., 0.], list(CENTER)]), "crop_lb": np.array([list(CROP_LB), [0, 0]])}


# (id, input dtype, order, mode, variant)
SPATIAL_CALLS = [(f"{v}_o{order}_{mode}", "float32", order, mode, v) for v in VARIANTS for order in (0, 1, 3) for mode in ("constant", "nearest")]
SPATIAL_CALLS += [("bf16_o1_constant", "bfloat16", 1, "constant", "a30_s14"), ("int16_o3_nearest", "int16", 3, "nearest", "a30_s07"),
                  ("int16_o0_constant", "int16", 0, "constant", "a30_s14")]
# (id, order, mode, variant); cval -1
LABEL_CALLS = [(f"{v}_l{order}_{mode}", order, mode, v) for v in VARIANTS for order, mode in ((0, "constant"), (1, "constant"), (1, "nearest"))]


def spatial_input(dtype):
    """(B, C, D, H, W)."""
    if dtype == "bfloat16":
        return torch.from_numpy(image(SRC, 22)).to(torch.bfloat16)
    return torch.from_numpy(image(SRC, 22 if dtype == "float32" else 25, np.dtype(dtype)))


def label_input():
    return blocky_labels_inplane(SRC, 23)


def tiny_case():
    """No rotation, scale 0.5 about (1.5, 1.0): coordinates 0.5 .. 2.5 along H and 0.5, 1.0, 1.5 along W, all exact."""
    x = image(TINY_SRC, 24)
    rec = {"modified": np.array([True]), "angles": np.zeros((1, 1)), "rotation": np.identity(2)[None], "scale": np.array([[0.5, 0.5]]),
           "center": np.array([[1.5, 1.0]]), "crop_lb": np.zeros((1, 2), np.int64)}
    return x, rec


def halves_case():
    """Labels in slabs along W and a map that shifts by exactly half a cell along W (whole cells along H): every cell weighs two of its four
    neighbours 0.5 each and the other two 0.  Source column pairs (w, w + 1): (1, 3) -> 3 (both reach 0.5, the later label wins), (3, 3) -> 3,
    (3, 0) -> 3 (0.5 >= 0.5 beats background), (0, 2) -> 2, (2, 2) -> 2."""
    seg = np.zeros((1, 2, 5, 6), np.int16)
    seg[..., 0], seg[..., 1], seg[..., 2], seg[..., 3], seg[..., 4], seg[..., 5] = 1, 3, 3, 0, 2, 2
    rec = {"modified": np.array([True]), "rotation": np.identity(2)[None], "scale": np.ones((1, 2)), "center": np.array([[2.0, 2.5]]),
           "crop_lb": np.zeros((1, 2), np.int64)}
    # patch (5, 5): coordinates along W = arange(5) - 2 + 2.5 = 0.5 .. 4.5, along H = 0 .. 4
    want = np.broadcast_to(np.array([3, 3, 3, 2, 2], np.int16), (1, 2, 5, 5))
    return seg, rec, (5, 5), want


def lowres_input():
    return image(LOW_SHAPE, 26)


def lowres_record():
    return {"apply": np.array([True, True]), "zoom": LOW_ZOOM}


def pipeline_params():
    """The ACDC trainer's data_aug_params: setup_DA_params with do_dummy_2D_data_aug sets dummy_2D and takes rotation_x from
    default_2D_augmentation_params (-180 .. 180 degrees)."""
    return dict(C3.pipeline_params(), dummy_2D=True, rotation_x=(-np.pi, np.pi))


def pipeline_records():
    """Every stage on, for both samples; sample 0 keeps a plain crop in the spatial stage, sample 1 turns by 140 degrees in-plane."""
    both = np.array([True, True])
    a = 140.0 / 360.0 * 2.0 * np.pi
    spatial = {"modified": np.array([False, True]), "angles": np.array([[0.], [a]]), "rotation": np.stack([np.identity(2), rotation_2d(a)]),
               "scale": np.array([[1., 1.], [0.9, 0.9]]), "center": np.array([[0., 0.], [9.5, 7.5]]), "crop_lb": np.array([[4, 3], [0, 0]])}
    return {"spatial": spatial, "noise": {"apply": both, "variance": np.array([0.05, 0.09])},
            "blur": {"apply": both, "sigma": np.array([[0.6], [0.9]])}, "brightness": {"apply": both, "multiplier": np.array([[0.8], [1.2]])},
            "contrast": {"apply": both, "factor": np.array([[1.2], [0.8]])}, "lowres": {"apply": both, "zoom": np.array([[0.6], [0.85]])},
            "gamma_inverted": {"apply": both, "gamma": np.array([[0.8], [1.3]])}, "gamma": {"apply": both, "gamma": np.array([[1.4], [0.75]])},
            "mirror": {"flip": np.array([[True, False, True], [False, True, False]])}}


def pipeline_inputs():
    data = image(PIPE_SRC, 27)
    seg = blocky_labels_inplane(PIPE_SRC, 28, labels=(-1, 0, 1, 2)).astype(np.float32)
    noise = ((RC.noise((2, 1, PIPE_SRC[2]) + PIPE_PATCH, 29) - 0.5) * 30.0).astype(np.float32)
    return data, seg, noise


def load_fixture():
    return torch.load(FIXTURE, weights_only=False)


def _as_numpy(t):
    return t.float().numpy() if t.dtype == torch.bfloat16 else t.numpy()


def planes(t):
    """Convert3DTo2DTransform's view: (B, C, D, H, W) -> (B, C D, H, W)."""
    return t.reshape((t.shape[0], t.shape[1] * t.shape[2]) + tuple(t.shape[3:]))


# ---- checks ------------------------------------------------------------------------------------------------------------------------------------
def run_spatial(call, dev):
    from deformablelka_amd import augmentation as A
    cid, dtype, order, mode, variant = call
    x = planes(spatial_input(dtype)).to(dev)
    keep = x.clone()
    out, none = A.augment_spatial(x, None, PATCH, order_data=order, border_mode_data=mode, border_cval_data=0, params=spatial_record(variant))
    assert none is None and torch.equal(x, keep)                                              # the input is not written to
    assert out.dtype == x.dtype and out.device == x.device and tuple(out.shape) == PLANES[:2] + PATCH
    return x, out


def check_values(cid, x, got, want, exempt, order, mode):
    frac = float(exempt.float().mean())
    assert frac <= 0.001, f"spatial/{cid}: {100 * frac:.3f} % of the cells are exempt"
    if mode != "constant":
        exempt = torch.zeros_like(exempt)
    if not x.is_floating_point():
        err = int((got.to(torch.int64) - want.to(torch.int64)).abs()[~exempt].max())
        print(f"spatial/{cid}: integer, max |out - ref| = {err}")
        assert err <= (0 if order == 0 else 1)
        return
    err = float((got.double() - want.double()).abs()[~exempt].max())
    bound = 0.0 if order == 0 else (1e-6 if order == 3 else 2e-6) * float(x.abs().max())
    print(f"spatial/{cid}: max |out - ref| = {err:.3e}, bound {bound:.3e}, exempt {int(exempt.sum())}")
    assert err <= bound


def check_spatial(fx, call, dev):
    cid, dtype, order, mode, variant = call
    rec = fx["spatial"][cid]
    x, out = run_spatial(call, dev)
    assert digest(_as_numpy(x.cpu())) == rec["input"], f"spatial/{cid}: the rebuilt input differs from the recorded one"
    box = x[0, :, CROP_LB[0]:CROP_LB[0] + PATCH[0], CROP_LB[1]:CROP_LB[1] + PATCH[1]]
    assert torch.equal(out[0], box)                                                           # the plain crop: bit for bit
    want, got = rec["out"], out[1].cpu()
    assert rec["exempt_cells"] == 0
    exempt = unpack(rec["exempt"], tuple(want.shape[1:]))[None].expand_as(want)
    check_values(cid, x, got, want, exempt, order, mode)
    if variant in OUTSIDE and mode == "constant" and order == 0 and dtype == "float32":
        assert abs(rec["outside"] - OUTSIDE[variant]) < 0.01                                  # the case does leave the source


def run_labels(call, dev):
    from deformablelka_amd import augmentation as A
    cid, order, mode, variant = call
    seg = planes(torch.from_numpy(label_input())).to(dev)
    data = torch.zeros(PLANES, dtype=torch.float32, device=dev)
    _, out = A.augment_spatial(data, seg, PATCH, order_data=0, order_seg=order, border_mode_seg=mode, border_cval_seg=-1,
                               params=spatial_record(variant))
    assert out.dtype == seg.dtype and out.device == seg.device and tuple(out.shape) == PLANES[:2] + PATCH
    return seg, out


def check_labels(fx, call, dev):
    cid, order, mode, variant = call
    rec = fx["labels"][cid]
    seg, out = run_labels(call, dev)
    assert digest(seg.cpu().numpy()) == rec["input"]
    want = rec["out"].to(out.dtype)
    close = unpack(rec["close"], tuple(want.shape))
    frac = float(close.float().mean())
    print(f"labels/{cid}: {100 * frac:.3f} % of the cells within {GAP} of the threshold")
    assert frac <= 0.01 and rec["close_cells"] == int(close.sum()) == 0
    assert torch.equal(out.cpu()[~close], want[~close])
    assert not bool((out == 3).any()) and len(torch.unique(out)) >= 3                          # label 3 is absent: no value is ever blended
    box = seg[0, :, CROP_LB[0]:CROP_LB[0] + PATCH[0], CROP_LB[1]:CROP_LB[1] + PATCH[1]]
    assert torch.equal(out[0], box)


def check_tiny(fx, mode, dev):
    from deformablelka_amd import augmentation as A
    x, rec = tiny_case()
    t = planes(torch.from_numpy(x)).to(dev)
    out, _ = A.augment_spatial(t, None, TINY_PATCH, order_data=3, border_mode_data=mode, border_cval_data=0, params=rec)
    r = fx["tiny"][mode]
    assert digest(x) == r["input"] and tuple(out.shape) == (1, 2) + TINY_PATCH and r["exempt_cells"] == 0
    want = r["out"]
    check_values(f"tiny_{mode}", t, out.cpu(), want, torch.zeros(want.shape, dtype=torch.bool), 3, mode)


def check_halves(dev):
    from deformablelka_amd import augmentation as A
    seg, rec, patch, want = halves_case()
    _, out = A.augment_spatial(np.zeros(seg.shape, np.float32), seg, patch, order_data=0, order_seg=1, border_mode_seg="constant",
                               border_cval_seg=-1, params=rec)
    assert np.array_equal(out.cpu().numpy(), want)


def _spatial_step(x, seg, rec):
    from deformablelka_amd import augmentation as A
    return A.augment_spatial(x, seg, PATCH, order_data=3, border_mode_data="nearest", order_seg=1, border_mode_seg="constant",
                             border_cval_seg=-1, params=rec)


def check_depth_independence(dev):
    """Depth is no interpolation axis: a plane's result does not depend on the planes around it."""
    x5, s5 = spatial_input("float32").to(dev), torch.from_numpy(label_input()).to(dev)
    rec = spatial_record("a30_s14")
    out, out_seg = _spatial_step(planes(x5), planes(s5), rec)
    P = PLANES[1]
    for p in range(P):
        one, one_seg = _spatial_step(planes(x5)[:, p:p + 1], planes(s5)[:, p:p + 1], rec)
        assert torch.equal(one[:, 0], out[:, p]) and torch.equal(one_seg[:, 0], out_seg[:, p])
    perm = [3, 0, 4, 1, 2]
    got, got_seg = _spatial_step(planes(x5[:, :, perm]), planes(s5[:, :, perm]), rec)
    B, C, D = SRC[:3]
    assert torch.equal(got.reshape((B, C, D) + PATCH), out.reshape((B, C, D) + PATCH)[:, :, perm])
    assert torch.equal(got_seg.reshape((B, C, D) + PATCH), out_seg.reshape((B, C, D) + PATCH)[:, :, perm])


def run_launches(shape, dev):
    """Launches of the 2-D spatial step (order-3 values plus order-1 labels) on a batch of `shape` = (B, C, D, H, W), every sample modified."""
    from deformablelka_amd import augmentation as A
    B = shape[0]
    one = spatial_record("a30_s07")
    rec = {k: np.stack([v[1]] * B) for k, v in one.items()}
    x = planes(torch.from_numpy(image(shape, 30))).to(dev)
    seg = planes(torch.from_numpy(blocky_labels_inplane(shape, 31))).to(dev)
    before = A.launch_count()
    for mode in ("constant", "nearest"):
        A.augment_spatial(x, seg, PATCH, order_data=3, border_mode_data=mode, order_seg=1, border_mode_seg="constant", border_cval_seg=-1,
                          params=rec)
    return (A.launch_count() - before) // 2


def check_launch_count(dev):
    small, large = run_launches((1, 1, 2) + SRC[3:], dev), run_launches(SRC, dev)
    print(f"2-D spatial step: {small} launches at (B, C, D) = (1, 1, 2), {large} at {SRC[:3]}")
    assert small == large == SPATIAL2D_LAUNCHES


def run_lowres(dev):
    from deformablelka_amd import augmentation as A
    x = torch.from_numpy(lowres_input()).to(dev)
    targets = []
    inner = A.resampling.resample_data_or_seg

    def recording(data, new_shape, *args, **kw):
        targets.append(tuple(int(v) for v in new_shape))
        return inner(data, new_shape, *args, **kw)

    A.resampling.resample_data_or_seg = recording
    try:
        out = A.augment_linear_downsampling_scipy(x, order_downsample=0, order_upsample=3, ignore_axes=(0,), params=lowres_record())
    finally:
        A.resampling.resample_data_or_seg = inner
    return x, out, targets


def check_lowres(fx, dev):
    rec = fx["lowres"]
    x, out, targets = run_lowres(dev)
    assert digest(x.cpu().numpy()) == rec["input"] and out.dtype == x.dtype and out.shape == x.shape and out.device == x.device
    assert torch.equal(out[1, 0], x[1, 0])                                                     # the skipped channel: bit for bit
    # down and up per channel with a zoom: the low-resolution array keeps the depth extent
    assert targets == [(6, 6, 5), LOW_SHAPE[2:], (6, 9, 8), LOW_SHAPE[2:], (6, 9, 8), LOW_SHAPE[2:]]
    assert [tuple(v) for v in rec["low_shapes"]] == [(6, 6, 5), (6, 9, 8), (6, 9, 8)]
    err = float((out.cpu().double() - rec["out"].double()).abs().max())
    bound = 1e-6 * float(x.abs().max())
    print(f"lowres: max |out - ref| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound


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


def check_pipeline(fx, dev):
    rec = fx["pipeline"]
    out, launches = run_pipeline(dev)
    data, target = out["data"], out["target"]
    assert data.dtype == torch.float32 and tuple(data.shape) == (2, 1, 8) + PIPE_PATCH
    assert isinstance(target, list) and [tuple(t.shape) for t in target] == [(2, 1, 8, 12, 10), (2, 1, 8, 6, 5), (2, 1, 4, 3, 2)]
    assert all(t.dtype == torch.float32 and t.device == data.device for t in target)
    assert all(not bool((t == -1).any()) for t in target)
    print(f"pipeline: {launches} launches")
    assert launches == PIPELINE2D_LAUNCHES
    assert digest(pipeline_inputs()[0]) == rec["input"]
    scale = float(rec["scale"])
    # the summed bounds of augmentation_cases.check_pipeline: order 3 spatial 1e-6, blur BLUR_K and six point-wise stages POINTWISE_K each in
    # units of 2^-24, each on values of at most 1.25 x the input's range (brightness), and the low-resolution pair at resampling's 1e-6
    bound = (1e-6 + 1e-6 + (C3.BLUR_K + 6 * C3.POINTWISE_K) * 2.0 ** -24) * 1.25 * scale
    assert rec["exempt_cells"] == 0 and rec["close_cells"] == 0
    err = float((data.cpu().double() - rec["data"].double()).abs().max())
    print(f"pipeline: max |data - ref| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    for got, want in zip(target, rec["target"]):
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
        assert rec["spatial"]["rotation"].shape == (2, 2, 2) and rec["spatial"]["modified"].all()
        rec["noise"]["apply"][:] = True
        rec["noise"]["variance"][:] = 0.05
        outs.append(aug(d, s, records=rec))
    assert torch.equal(outs[0]["data"], outs[1]["data"]) and all(torch.equal(a, b) for a, b in zip(outs[0]["target"], outs[1]["target"]))
    assert bool(torch.isfinite(outs[0]["data"]).all()) and tuple(outs[0]["data"].shape) == (2, 1, 8) + PIPE_PATCH


def check_refusals(dev):
    import pytest
    from deformablelka_amd import augmentation as A
    base = pipeline_params()
    with pytest.raises(NotImplementedError, match=r"dummy_2D.*patch_size\[1:\]"):
        A.MoreDAAugmentation((8, 12, 10), base)                                                # the 3-entry patch with dummy_2D
    with pytest.raises(NotImplementedError, match="without dummy_2D"):
        A.MoreDAAugmentation((12, 10), dict(base, dummy_2D=False))                             # the pure 2-D chain stays out
    for key, value in (("do_elastic", True), ("move_last_seg_chanel_to_data", True), ("mask_was_used_for_normalization", {0: True})):
        with pytest.raises(NotImplementedError, match=key):
            A.MoreDAAugmentation((12, 10), dict(base, **{key: value}))
    with pytest.raises(NotImplementedError, match="regions"):
        A.MoreDAAugmentation((12, 10), base, regions=[[1, 2]])
    with pytest.raises(NotImplementedError, match="soft_ds"):
        A.MoreDAAugmentation((12, 10), base, soft_ds=True)
    x4, x5 = torch.zeros((1, 2, 6, 6), device=dev), torch.zeros((1, 1, 2, 6, 6), device=dev)
    with pytest.raises(ValueError, match="patch_size"):
        A.augment_spatial(x5, None, (4, 4))                                                    # mixed ranks
    with pytest.raises(ValueError, match="patch_size"):
        A.augment_spatial(x4, None, (2, 4, 4))
    with pytest.raises(ValueError, match="rank"):
        A.augment_spatial(x4, x5, (4, 4))
    with pytest.raises(ValueError, match="rank"):
        A.draw_spatial(np.random.RandomState(0), (2, 6, 6), (4, 4), 1)
    with pytest.raises(ValueError, match="rank"):
        A.draw_spatial(np.random.RandomState(0), (6, 6), (2, 4, 4), 1)
    with pytest.raises(NotImplementedError, match="order_data"):
        A.augment_spatial(x4, None, (4, 4), order_data=2)
    with pytest.raises(NotImplementedError, match="do_elastic_deform"):
        A.augment_spatial(x4, None, (4, 4), do_elastic_deform=True)
    with pytest.raises(NotImplementedError, match="border_cval_seg"):
        A.augment_spatial(x4, x4, (4, 4), order_seg=1, border_cval_seg=1)
    with pytest.raises(ValueError, match="ignore_axes"):
        A.augment_linear_downsampling_scipy(x5, ignore_axes=(3,))
    with pytest.raises(ValueError, match="src_shape"):
        A.MoreDAAugmentation((12, 10), base).draw(1, (20, 16), 1)


def check_c_interface_refusals(dev):
    """The 2-D entries refuse a 3-D description, bad extents and dtypes with a status and launch nothing."""
    import ctypes
    from deformablelka_amd import _lib as L
    from deformablelka_amd import ops
    lib = L.get_lib()
    x = torch.zeros((1, 2, 6, 6), dtype=torch.float32, device=dev)
    y = torch.zeros((1, 2, 4, 4), dtype=torch.float32, device=dev)
    maps, plain = torch.zeros((1, 6), dtype=torch.float64, device=dev), torch.zeros((1, 3), dtype=torch.int32, device=dev)
    seg, out = x.to(torch.int32), y.to(torch.int32)

    def desc(src=(6, 6, 0), out_=(4, 4, 0), dtype=L.DLKA_F32, order=1, mode=L.DLKA_AUG_CONSTANT, pad=0, cval=0.0):
        d = L.AugmentDesc()
        d.B, d.C, d.dtype, d.order, d.mode, d.pad, d.cval = 1, 2, dtype, order, mode, pad, cval
        for ax in range(3):
            d.src[ax], d.out[ax] = src[ax], out_[ax]
        return d

    before = ops.augment_launch_count()
    bad = [desc(src=(2, 6, 6), out_=(2, 4, 4)), desc(src=(6, 6, 1)), desc(out_=(4, 0, 0)), desc(src=(0, 6, 0)), desc(dtype=7), desc(order=2),
           desc(mode=5), desc(pad=12)]
    for d in bad:
        rc = lib.dlka_augment_spatial2d(L.ptr(x), None, L.ptr(y), ctypes.byref(d), L.ptr(maps), L.ptr(plain), L.stream_ptr(x))
        assert rc != 0
    for d in (desc(src=(2, 6, 6), out_=(2, 4, 4)), desc(order=3), desc(order=1, cval=0.5), desc(pad=1)):
        rc = lib.dlka_augment_spatial2d_labels(L.ptr(seg), L.ptr(out), ctypes.byref(d), L.ptr(maps), L.ptr(plain), L.stream_ptr(seg))
        assert rc != 0
    assert ops.augment_launch_count() == before
    with __import__("pytest").raises(RuntimeError, match="leaves the source"):
        ops.augment_spatial2d(x, (4, 4), np.zeros((1, 2, 3)), np.array([[1, 3, 0]]), 0, L.DLKA_AUG_CONSTANT, 0.0)
