"""The 3-D trainers' train-time augmentation on the HIP kernels of ``csrc/cl_augment.hip`` (include/dlka.h: ``dlka_augment_*``): what
``get_moreDA_augmentation`` (3D/d_lka_former/training/data_augmentation/data_augmentation_moreDA.py:60-147) composes from batchgenerators'
transforms and the reference runs on scipy in four worker processes (d_lka_former_trainer_synapse.py:114).

Every transform is split in two.  ``draw_*`` runs on the host, takes a ``numpy.random.RandomState`` and returns a plain dict of numpy arrays
(flags, matrices, factors, sigmas) for the batch; ``augment_*`` runs on the device and is a pure function of its input and that record
(``params=``; without one it draws with ``rs``).  The rules are batchgenerators 0.21's, restated in DESIGN.md 4.18.

  ``draw_spatial`` / ``augment_spatial``      SpatialTransform: rotation, scaling, centre or random crop; orders 0 / 1 / 3 for the image,
                                              0 / 1 for the label map, border modes 'constant' and 'nearest'; no elastic deformation.
                                              Rank-4 arrays (B, P, H, W) with a 2-entry patch_size are batchgenerators' dim == 2 form: one
                                              in-plane rotation, scale and crop per sample for all of its planes
  ``augment_gaussian_noise``, ``augment_gaussian_blur``, ``augment_brightness_multiplicative``, ``augment_brightness_additive``,
  ``augment_contrast``, ``augment_linear_downsampling_scipy``, ``augment_gamma``, ``augment_mirroring``   the colour and mirror transforms
  ``downsample_seg_for_ds_transform2``        training/data_augmentation/downsampling.py:88, on ``resampling``'s label path
  ``MoreDAAugmentation``                      the chain of data_augmentation_moreDA.py:60-147, and with ``dummy_2D`` its :54-75 / :91-94 form
                                              (the ACDC trainer's anisotropic patch): the spatial step on the planes, the rest in 3-D

Unlike the package's per-sample functions these take the batch: ``data`` (B, C, D, H, W), ``seg`` (B, Cs, D, H, W), numpy arrays or tensors on
either side (host data is moved to the device).  The inputs are not written to; results are device tensors in the input's dtype.  Without a
GPU the calls raise as every operator of the package does: there is no host fall-back."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from . import ops
from . import resampling
from ._containers import to_working_device

__all__ = ["draw_spatial", "augment_spatial", "draw_gaussian_noise", "augment_gaussian_noise", "draw_gaussian_blur", "augment_gaussian_blur",
           "draw_brightness_multiplicative", "augment_brightness_multiplicative", "draw_brightness_additive", "augment_brightness_additive",
           "draw_contrast", "augment_contrast", "draw_linear_downsampling_scipy", "augment_linear_downsampling_scipy", "draw_gamma",
           "augment_gamma", "draw_mirroring", "augment_mirroring", "downsample_seg_for_ds_transform2", "MoreDAAugmentation", "launch_count"]

_MODES = {"constant": L.DLKA_AUG_CONSTANT, "nearest": L.DLKA_AUG_NEAREST}
_NATIVE = (torch.float32, torch.bfloat16, torch.float64, torch.int16)


def launch_count() -> int:
    """Kernel launches of this module so far (this process): the augmentation kernels and the resampling kernels it composes."""
    return ops.augment_launch_count() + ops.resample_launch_count()


# ---- containers ------------------------------------------------------------------------------------------------------------------------------
def _device(x, what, ndim=(5,)):
    """A detached tensor on the working device; never the caller's own storage when it is going to be returned."""
    t = to_working_device(x, "augmentation", what)
    if t.ndim not in ndim:
        raise RuntimeError(f"augmentation: {what} is (b, c, x, y, z)" + (" or (b, planes, y, z)" if 4 in ndim else "") + f", got {tuple(t.shape)}")
    return t


def _native(t):
    """(tensor in a dtype the kernels store, the dtype to give back)."""
    if t.dtype in _NATIVE:
        return t, t.dtype
    if t.dtype == torch.float16:
        return t.to(torch.float32), t.dtype
    return t.to(torch.float64), t.dtype          # other integers and bool: float64 holds them; the way back truncates as astype does


def _rs(rs):
    return rs if rs is not None else np.random.RandomState()


def _range_factor(rs, lo, hi):
    """batchgenerators' draw of a scale, contrast or gamma factor."""
    if rs.random_sample() < 0.5 and lo < 1:
        return rs.uniform(lo, 1)
    return rs.uniform(max(lo, 1), hi)


def _per_channel(v, B, C, what):
    v = np.asarray(v, dtype=np.float64)
    if v.shape != (B, C):
        raise ValueError(f"augmentation: params['{what}'] is (batch, channels) = ({B}, {C}), got {v.shape}")
    return v


def _steps(B, C):
    return np.zeros((B * C, 1, 6))


# ---- SpatialTransform ------------------------------------------------------------------------------------------------------------------------
def _rotation_2d(a):
    return np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])


def _rotation(ax, ay, az):
    def rx(a):
        return np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])

    def ry(a):
        return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])

    def rz(a):
        return np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])

    return np.dot(np.dot(np.dot(np.identity(3), rx(ax)), ry(ay)), rz(az))


def draw_spatial(rs, src_shape, patch_size, batch, patch_center_dist_from_border=30, do_elastic_deform=False, do_rotation=True,
                 angle_x=(0, 2 * np.pi), angle_y=(0, 2 * np.pi), angle_z=(0, 2 * np.pi), do_scale=True, scale=(0.75, 1.25), random_crop=True,
                 p_scale_per_sample=1, p_rot_per_sample=1, independent_scale_for_each_axis=False, p_rot_per_axis=1,
                 p_independent_scale_per_axis=1, **_apply_only):
    """Per sample: ``modified`` (bool), ``angles`` (3), ``rotation`` (3, 3; coords <- (coords^T . rotation)^T), ``scale`` (3), ``center`` (3; where
    the patch centre lands in the source when the sample is modified) and ``crop_lb`` (3; the box when it is not).  With two spatial axes
    (batchgenerators' dim == 2): one angle (``angle_x``) and trailing extents of 2, ``angles`` (1), ``rotation`` (2, 2)."""
    if do_elastic_deform:
        raise NotImplementedError("augmentation: do_elastic_deform=True (the 3-D trainer sets do_elastic = False)")
    src_shape, patch_size = tuple(int(v) for v in src_shape), tuple(int(v) for v in patch_size)
    if len(src_shape) != len(patch_size):
        raise ValueError(f"augmentation: patch_size {patch_size} and the source {src_shape} differ in rank")
    dim = len(patch_size)
    if dim not in (2, 3):
        raise NotImplementedError(f"augmentation: patch_size and the source have two or three spatial axes, got {dim}")
    if any(p > s for p, s in zip(patch_size, src_shape)):
        raise ValueError(f"augmentation: patch_size {patch_size} is larger than the source {src_shape}")
    dist = patch_center_dist_from_border
    dist = [dist] * dim if not isinstance(dist, (list, tuple, np.ndarray)) else list(dist)
    rec = {"modified": np.zeros(batch, bool), "angles": np.zeros((batch, 3 if dim == 3 else 1)),
           "rotation": np.tile(np.identity(dim), (batch, 1, 1)), "scale": np.ones((batch, dim)), "center": np.zeros((batch, dim)),
           "crop_lb": np.zeros((batch, dim), np.int64)}
    for b in range(batch):
        if do_rotation and rs.uniform() < p_rot_per_sample:
            a = [rs.uniform(r[0], r[1]) if rs.uniform() <= p_rot_per_axis else 0.0 for r in (angle_x, angle_y, angle_z)[:len(rec["angles"][b])]]
            rec["angles"][b], rec["rotation"][b], rec["modified"][b] = a, _rotation(*a) if dim == 3 else _rotation_2d(*a), True
        if do_scale and rs.uniform() < p_scale_per_sample:
            if independent_scale_for_each_axis and rs.uniform() < p_independent_scale_per_axis:
                rec["scale"][b] = [_range_factor(rs, scale[0], scale[1]) for _ in range(dim)]
            else:
                rec["scale"][b] = _range_factor(rs, scale[0], scale[1])
            rec["modified"][b] = True
        if rec["modified"][b]:
            for d in range(dim):
                rec["center"][b, d] = rs.uniform(dist[d], src_shape[d] - dist[d]) if random_crop else src_shape[d] / 2. - 0.5
        else:
            for d in range(dim):
                margin = int(dist[d]) - patch_size[d] // 2 if random_crop else 0
                lo, hi = margin, src_shape[d] - patch_size[d] - margin
                rec["crop_lb"][b, d] = rs.randint(lo, hi + 1) if random_crop and hi > lo >= 0 else (src_shape[d] - patch_size[d]) // 2
    return rec


def _spatial_tables(params, B, dim=3):
    mod = np.asarray(params["modified"]).astype(bool).reshape(-1)
    if np.asarray(params["rotation"]).size != len(mod) * dim * dim:
        raise ValueError(f"augmentation: the spatial record is not one of {dim} spatial axes (rotation {np.asarray(params['rotation']).shape})")
    rot = np.asarray(params["rotation"], dtype=np.float64).reshape(-1, dim, dim)
    sc = np.asarray(params["scale"], dtype=np.float64).reshape(-1, dim)
    ctr = np.asarray(params["center"], dtype=np.float64).reshape(-1, dim)
    lb = np.asarray(params["crop_lb"]).astype(np.int64).reshape(-1, dim)
    if not (len(mod) == len(rot) == len(sc) == len(ctr) == len(lb) == B):
        raise ValueError(f"augmentation: the spatial record is for {len(mod)} samples, the batch has {B}")
    maps, plain = np.zeros((B, dim, dim + 1)), np.zeros((B, dim + 1), np.int32)
    for b in range(B):
        if mod[b]:
            maps[b, :, :dim] = rot[b].T * sc[b][:, None]       # source axis d = sum_e g[e] rotation[e][d], times scale[d]
            maps[b, :, dim] = ctr[b]
        else:
            plain[b, 0], plain[b, 1:] = 1, lb[b]
    return maps, plain


def augment_spatial(data, seg, patch_size, patch_center_dist_from_border=30, do_elastic_deform=False, alpha=(0., 1000.), sigma=(10., 13.),
                    do_rotation=True, angle_x=(0, 2 * np.pi), angle_y=(0, 2 * np.pi), angle_z=(0, 2 * np.pi), do_scale=True,
                    scale=(0.75, 1.25), border_mode_data='nearest', border_cval_data=0, order_data=3, border_mode_seg='constant',
                    border_cval_seg=0, order_seg=0, random_crop=True, p_el_per_sample=1, p_scale_per_sample=1, p_rot_per_sample=1,
                    independent_scale_for_each_axis=False, p_rot_per_axis=1, p_independent_scale_per_axis=1, params=None, rs=None):
    """batchgenerators' ``augment_spatial`` without the elastic deformation (``do_elastic_deform`` defaults to False here and True raises).
    ``seg`` may be None.  Returns (data, seg) of extents ``patch_size``.  Rank-4 ``data`` / ``seg`` (B, P, H, W) with a 2-entry ``patch_size``
    is its dim == 2 form: every plane of a sample goes through the same in-plane transform (``ops.augment_spatial2d``)."""
    if do_elastic_deform:
        raise NotImplementedError("augmentation: do_elastic_deform=True (the 3-D trainer sets do_elastic = False)")
    if order_data not in (0, 1, 3):
        raise NotImplementedError(f"augmentation: order_data={order_data!r} (supported: 0, 1, 3)")
    if seg is not None and order_seg not in (0, 1):
        raise NotImplementedError(f"augmentation: order_seg={order_seg!r} (supported: 0, 1)")
    for name, mode in (("border_mode_data", border_mode_data), ("border_mode_seg", border_mode_seg)):
        if mode not in _MODES:
            raise NotImplementedError(f"augmentation: {name}={mode!r} (supported: 'constant', 'nearest')")
    x = _device(data, "data", (4, 5))
    B, patch_size = x.shape[0], tuple(int(v) for v in patch_size)
    dim = x.ndim - 2
    if len(patch_size) != dim:
        raise ValueError(f"augmentation: patch_size {patch_size} does not go with data {tuple(x.shape)} of {dim} spatial axes")
    spatial, spatial_labels = (ops.augment_spatial, ops.augment_spatial_labels) if dim == 3 else (ops.augment_spatial2d,
                                                                                                  ops.augment_spatial2d_labels)
    if params is None:
        params = draw_spatial(_rs(rs), x.shape[2:], patch_size, B, patch_center_dist_from_border, False, do_rotation, angle_x, angle_y, angle_z,
                              do_scale, scale, random_crop, p_scale_per_sample, p_rot_per_sample, independent_scale_for_each_axis,
                              p_rot_per_axis, p_independent_scale_per_axis)
    maps, plain = _spatial_tables(params, B, dim)
    xn, back = _native(x)
    out = spatial(xn, patch_size, maps, plain, order_data, _MODES[border_mode_data], float(border_cval_data)).to(back)
    out_seg = None
    if seg is not None:
        s = _device(seg, "seg", (4, 5))
        if s.ndim != x.ndim:
            raise ValueError(f"augmentation: seg {tuple(s.shape)} and data {tuple(x.shape)} differ in rank")
        if s.shape[0] != B or tuple(s.shape[2:]) != tuple(x.shape[2:]):
            raise ValueError(f"augmentation: seg {tuple(s.shape)} does not go with data {tuple(x.shape)}")
        if order_seg == 1 and border_mode_seg == "constant" and not float(border_cval_seg) < 0.5:
            raise NotImplementedError(f"augmentation: border_cval_seg={border_cval_seg!r} with order_seg=1 (every label would pass the 0.5 "
                                      "threshold outside the volume; supported: values below 0.5)")
        labels = resampling._as_labels(s)
        out_seg = spatial_labels(labels, patch_size, maps, plain, order_seg, _MODES[border_mode_seg], float(border_cval_seg))
        out_seg = out_seg.to(s.dtype)
    return out, out_seg


# ---- noise -------------------------------------------------------------------------------------------------------------------------------------
def draw_gaussian_noise(rs, batch, noise_variance=(0, 0.1), p_per_sample=1):
    rec = {"apply": np.zeros(batch, bool), "variance": np.zeros(batch)}
    for b in range(batch):
        if rs.uniform() < p_per_sample:
            rec["apply"][b] = True
            rec["variance"][b] = noise_variance[0] if noise_variance[0] == noise_variance[1] else rs.uniform(noise_variance[0], noise_variance[1])
    return rec


def _noise_field(x, params, noise, generator):
    if noise is not None:
        n = _device(noise, "noise")
        if n.shape != x.shape:
            raise ValueError(f"augmentation: noise {tuple(n.shape)} does not go with data {tuple(x.shape)}")
        return n.to(x.dtype)
    # the package hands the variance to numpy.random.normal as the standard deviation; so does this
    std = torch.as_tensor(np.asarray(params["variance"], dtype=np.float64), dtype=torch.float32).reshape(-1, 1, 1, 1, 1)
    field = torch.randn(x.shape, generator=generator, dtype=torch.float32, device=generator.device if generator is not None else x.device)
    return (field.to(x.device) * std.to(x.device)).to(x.dtype)


def _apply_noise(x, params, noise=None, generator=None, flip=None):
    apply = np.asarray(params["apply"]).astype(bool).reshape(-1)
    if not apply.any() and flip is None:
        return x
    steps = _steps(x.shape[0], x.shape[1])
    steps[np.repeat(apply, x.shape[1]), 0, 0] = L.DLKA_AUG_OP_NOISE
    return ops.augment_pointwise(x, steps, noise=_noise_field(x, params, noise, generator) if apply.any() else None, flip=flip)


def augment_gaussian_noise(data, noise_variance=(0, 0.1), p_per_sample=1, params=None, rs=None, noise=None, generator=None):
    """Samples flagged in the record get ``+ normal(0, variance)``: ``noise`` is that field when given ((B, C, D, H, W), already scaled), else it
    is drawn on the device from ``generator`` (a ``torch.Generator``; the stream is torch's, not numpy's)."""
    x, back = _native(_device(data, "data"))
    if params is None:
        params = draw_gaussian_noise(_rs(rs), x.shape[0], noise_variance, p_per_sample)
    y = _apply_noise(x, params, noise, generator)
    return (y.clone() if y is x else y).to(back)


# ---- blur --------------------------------------------------------------------------------------------------------------------------------------
def draw_gaussian_blur(rs, batch, channels, sigma_range=(1, 5), per_channel=True, p_per_channel=1, p_per_sample=1):
    """``sigma`` (batch, channels); 0: the channel is left alone."""
    rec = {"apply": np.zeros(batch, bool), "sigma": np.zeros((batch, channels))}
    for b in range(batch):
        if rs.uniform() < p_per_sample:
            rec["apply"][b] = True
            sigma = None if per_channel else rs.uniform(sigma_range[0], sigma_range[1])
            for c in range(channels):
                if rs.uniform() <= p_per_channel:
                    rec["sigma"][b, c] = rs.uniform(sigma_range[0], sigma_range[1]) if per_channel else sigma
    return rec


def _gaussian_weights(sigma):
    """scipy.ndimage.gaussian_filter1d's kernel (truncate 4, order 0): radius and the weights from the centre outwards."""
    radius = int(4.0 * float(sigma) + 0.5)
    if radius > L.DLKA_AUG_RADIUS_MAX:
        raise NotImplementedError(f"augmentation: sigma={sigma!r} needs a radius of {radius} cells (supported: up to {L.DLKA_AUG_RADIUS_MAX})")
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2)
    phi = phi / phi.sum()
    return radius, phi[radius:]


def _apply_blur(x, params):
    sigma = _per_channel(params["sigma"], x.shape[0], x.shape[1], "sigma").reshape(-1)
    if not (sigma > 0).any():
        return x
    radius, weights = np.full(len(sigma), -1, np.int32), np.zeros((len(sigma), L.DLKA_AUG_RADIUS_MAX + 1))
    for i, s in enumerate(sigma):
        if s > 0:
            radius[i], w = _gaussian_weights(s)
            weights[i, :len(w)] = w
    return ops.augment_gaussian(x, radius, weights)


def augment_gaussian_blur(data, sigma_range=(1, 5), per_channel=True, p_per_channel=1, p_per_sample=1, params=None, rs=None):
    """``scipy.ndimage.gaussian_filter(channel, sigma, order=0)`` for every channel whose sigma in the record is > 0; the others come back
    bit for bit."""
    x, back = _native(_device(data, "data"))
    if params is None:
        params = draw_gaussian_blur(_rs(rs), x.shape[0], x.shape[1], sigma_range, per_channel, p_per_channel, p_per_sample)
    y = _apply_blur(x, params)
    return (y.clone() if y is x else y).to(back)


# ---- brightness ----------------------------------------------------------------------------------------------------------------------------------
def draw_brightness_multiplicative(rs, batch, channels, multiplier_range=(0.5, 2), per_channel=True, p_per_sample=1):
    rec = {"apply": np.zeros(batch, bool), "multiplier": np.ones((batch, channels))}
    for b in range(batch):
        if rs.uniform() < p_per_sample:
            rec["apply"][b] = True
            rec["multiplier"][b] = [rs.uniform(*multiplier_range) for _ in range(channels)] if per_channel else rs.uniform(*multiplier_range)
    return rec


def draw_brightness_additive(rs, batch, channels, mu=0.0, sigma=0.1, per_channel=True, p_per_sample=1, p_per_channel=1):
    rec = {"apply": np.zeros(batch, bool), "add": np.zeros((batch, channels))}
    for b in range(batch):
        if rs.uniform() < p_per_sample:
            rec["apply"][b] = True
            if per_channel:
                for c in range(channels):
                    if rs.uniform() <= p_per_channel:
                        rec["add"][b, c] = rs.normal(mu, sigma)
            else:
                value = rs.normal(mu, sigma)
                for c in range(channels):
                    if rs.uniform() <= p_per_channel:
                        rec["add"][b, c] = value
    return rec


def _apply_scale_add(x, apply, mul, add, flip=None):
    apply = np.repeat(np.asarray(apply).astype(bool).reshape(-1), x.shape[1])
    if not apply.any() and flip is None:
        return x
    steps = _steps(x.shape[0], x.shape[1])
    steps[apply, 0, 0] = L.DLKA_AUG_OP_SCALE_ADD
    steps[:, 0, 1], steps[:, 0, 2] = mul.reshape(-1), add.reshape(-1)
    return ops.augment_pointwise(x, steps, flip=flip)


def augment_brightness_multiplicative(data, multiplier_range=(0.5, 2), per_channel=True, p_per_sample=1, params=None, rs=None):
    x, back = _native(_device(data, "data"))
    B, C = x.shape[:2]
    if params is None:
        params = draw_brightness_multiplicative(_rs(rs), B, C, multiplier_range, per_channel, p_per_sample)
    y = _apply_scale_add(x, params["apply"], _per_channel(params["multiplier"], B, C, "multiplier"), np.zeros((B, C)))
    return (y.clone() if y is x else y).to(back)


def augment_brightness_additive(data, mu=0.0, sigma=0.1, per_channel=True, p_per_sample=1, p_per_channel=1, params=None, rs=None):
    x, back = _native(_device(data, "data"))
    B, C = x.shape[:2]
    if params is None:
        params = draw_brightness_additive(_rs(rs), B, C, mu, sigma, per_channel, p_per_sample, p_per_channel)
    y = _apply_scale_add(x, params["apply"], np.ones((B, C)), _per_channel(params["add"], B, C, "add"))
    return (y.clone() if y is x else y).to(back)


# ---- contrast ------------------------------------------------------------------------------------------------------------------------------------
def draw_contrast(rs, batch, channels, contrast_range=(0.75, 1.25), per_channel=True, p_per_sample=1):
    rec = {"apply": np.zeros(batch, bool), "factor": np.ones((batch, channels))}
    for b in range(batch):
        if rs.uniform() < p_per_sample:
            rec["apply"][b] = True
            if per_channel:
                rec["factor"][b] = [_range_factor(rs, contrast_range[0], contrast_range[1]) for _ in range(channels)]
            else:
                rec["factor"][b] = _range_factor(rs, contrast_range[0], contrast_range[1])
    return rec


def _apply_contrast(x, params, flip=None):
    apply = np.repeat(np.asarray(params["apply"]).astype(bool).reshape(-1), x.shape[1])
    if not apply.any() and flip is None:
        return x
    steps = _steps(x.shape[0], x.shape[1])
    steps[apply, 0, 0] = L.DLKA_AUG_OP_CONTRAST
    steps[:, 0, 1] = _per_channel(params["factor"], x.shape[0], x.shape[1], "factor").reshape(-1)
    return ops.augment_pointwise(x, steps, stats0=ops.augment_channel_stats(x) if apply.any() else None, flip=flip)


def augment_contrast(data, contrast_range=(0.75, 1.25), preserve_range=True, per_channel=True, p_per_sample=1, params=None, rs=None):
    """``(x - mean) * factor + mean`` per channel, clipped to the channel's previous [min, max]."""
    if not preserve_range:
        raise NotImplementedError("augmentation: preserve_range=False (the trainer's ContrastAugmentationTransform keeps the default True)")
    x, back = _native(_device(data, "data"))
    if params is None:
        params = draw_contrast(_rs(rs), x.shape[0], x.shape[1], contrast_range, per_channel, p_per_sample)
    y = _apply_contrast(x, params)
    return (y.clone() if y is x else y).to(back)


# ---- SimulateLowResolution -------------------------------------------------------------------------------------------------------------------------
def draw_linear_downsampling_scipy(rs, batch, channels, zoom_range=(0.5, 1), per_channel=True, p_per_channel=1, p_per_sample=1):
    """``zoom`` (batch, channels); 0: the channel is left alone."""
    rec = {"apply": np.zeros(batch, bool), "zoom": np.zeros((batch, channels))}
    for b in range(batch):
        if rs.uniform() < p_per_sample:
            rec["apply"][b] = True
            zoom = None if per_channel else rs.uniform(zoom_range[0], zoom_range[1])
            for c in range(channels):
                if rs.uniform() < p_per_channel:
                    rec["zoom"][b, c] = rs.uniform(zoom_range[0], zoom_range[1]) if per_channel else zoom
    return rec


def _apply_lowres(x, params, order_downsample, order_upsample, ignore_axes=None):
    zoom = _per_channel(params["zoom"], x.shape[0], x.shape[1], "zoom")
    if not (zoom > 0).any():
        return x
    shape = np.array(x.shape[2:])
    y = x.clone()
    for b in range(x.shape[0]):
        for c in range(x.shape[1]):
            if zoom[b, c] > 0:
                target = np.round(shape * zoom[b, c]).astype(int)
                for i in ignore_axes or ():
                    target[i] = shape[i]
                low = resampling.resample_data_or_seg(x[b, c:c + 1], target, False, order=order_downsample)
                y[b, c:c + 1] = resampling.resample_data_or_seg(low, shape, False, order=order_upsample)
    return y


def augment_linear_downsampling_scipy(data, zoom_range=(0.5, 1), per_channel=True, p_per_channel=1, channels=None, order_downsample=1,
                                      order_upsample=0, ignore_axes=None, p_per_sample=1, params=None, rs=None):
    """Every channel with a zoom in the record goes down to ``round(shape * zoom)`` and back up (``resize(..., mode='edge',
    anti_aliasing=False)``: ``resampling.resample_data_or_seg``).  ``ignore_axes``: spatial axes whose extent the low-resolution array keeps
    (the dummy-2D branch passes ``(0,)``)."""
    if channels is not None:
        raise NotImplementedError("augmentation: channels= (the trainer's SimulateLowResolutionTransform processes every channel)")
    if ignore_axes is not None:
        ignore_axes = tuple(int(i) for i in ignore_axes)
        if any(i not in (0, 1, 2) for i in ignore_axes):
            raise ValueError(f"augmentation: ignore_axes={ignore_axes!r} (spatial axes 0, 1, 2)")
    x, back = _native(_device(data, "data"))
    if params is None:
        params = draw_linear_downsampling_scipy(_rs(rs), x.shape[0], x.shape[1], zoom_range, per_channel, p_per_channel, p_per_sample)
    y = _apply_lowres(x, params, order_downsample, order_upsample, ignore_axes)
    return (y.clone() if y is x else y).to(back)


# ---- gamma ---------------------------------------------------------------------------------------------------------------------------------------
def draw_gamma(rs, batch, channels, gamma_range=(0.5, 2), per_channel=True, p_per_sample=1):
    rec = {"apply": np.zeros(batch, bool), "gamma": np.ones((batch, channels))}
    for b in range(batch):
        if rs.uniform() < p_per_sample:
            rec["apply"][b] = True
            rec["gamma"][b] = [_range_factor(rs, gamma_range[0], gamma_range[1]) for _ in range(channels)]
    return rec


def _apply_gamma(x, params, invert_image, retain_stats, flip=None):
    apply = np.repeat(np.asarray(params["apply"]).astype(bool).reshape(-1), x.shape[1])
    if not apply.any() and flip is None:
        return x
    steps = _steps(x.shape[0], x.shape[1])
    steps[apply, 0, 0] = L.DLKA_AUG_OP_GAMMA
    steps[:, 0, 1] = _per_channel(params["gamma"], x.shape[0], x.shape[1], "gamma").reshape(-1)
    steps[:, 0, 2] = -1.0 if invert_image else 1.0
    if not apply.any():
        return ops.augment_pointwise(x, steps, flip=flip)
    before = ops.augment_channel_stats(x)
    if not retain_stats:
        return ops.augment_pointwise(x, steps, stats0=before, flip=flip)
    y = ops.augment_pointwise(x, steps, stats0=before)
    steps[apply, 0, 0] = L.DLKA_AUG_OP_RETAIN
    return ops.augment_pointwise(y, steps, stats0=before, stats1=ops.augment_channel_stats(y), flip=flip)


def augment_gamma(data, gamma_range=(0.5, 2), invert_image=False, epsilon=1e-7, per_channel=True, retain_stats=False, p_per_sample=1,
                  params=None, rs=None):
    """Per channel ``((x - min) / (max - min + 1e-7)) ** gamma * (max - min) + min``, on the negated image when ``invert_image``; with
    ``retain_stats`` the channel's mean and (population) standard deviation are restored afterwards."""
    if not per_channel:
        raise NotImplementedError("augmentation: per_channel=False (the trainer's GammaTransforms are per channel)")
    if float(epsilon) != 1e-7:
        raise NotImplementedError(f"augmentation: epsilon={epsilon!r} (supported: 1e-7)")
    x, back = _native(_device(data, "data"))
    if params is None:
        params = draw_gamma(_rs(rs), x.shape[0], x.shape[1], gamma_range, per_channel, p_per_sample)
    y = _apply_gamma(x, params, invert_image, retain_stats)
    return (y.clone() if y is x else y).to(back)


# ---- mirror --------------------------------------------------------------------------------------------------------------------------------------
def draw_mirroring(rs, batch, axes=(0, 1, 2)):
    rec = {"flip": np.zeros((batch, 3), bool)}
    for b in range(batch):
        for a in (0, 1, 2):
            if a in axes and rs.uniform() < 0.5:
                rec["flip"][b, a] = True
    return rec


def _flip_masks(params, B):
    flip = np.asarray(params["flip"]).astype(bool)
    if flip.shape != (B, 3):
        raise ValueError(f"augmentation: params['flip'] is (batch, 3) = ({B}, 3), got {flip.shape}")
    return (flip * np.array([1, 2, 4])).sum(1).astype(np.int32)


def augment_mirroring(data, seg=None, axes=(0, 1, 2), params=None, rs=None):
    """Spatial axis a of sample b is reversed where ``params['flip'][b, a]``; data and seg together."""
    x, back = _native(_device(data, "data"))
    if params is None:
        params = draw_mirroring(_rs(rs), x.shape[0], axes)
    flip = _flip_masks(params, x.shape[0])
    out = ops.augment_pointwise(x, _steps(x.shape[0], x.shape[1]), flip=flip).to(back)
    if seg is None:
        return out, None
    s, sback = _native(_device(seg, "seg"))
    return out, ops.augment_pointwise(s, _steps(s.shape[0], s.shape[1]), flip=flip).to(sback)


# ---- deep-supervision targets ------------------------------------------------------------------------------------------------------------------------
def downsample_seg_for_ds_transform2(seg, ds_scales=((1, 1, 1), (0.5, 0.5, 0.5), (0.25, 0.25, 0.25)), order=0, cval=0, axes=None):
    """training/data_augmentation/downsampling.py:88-105: one label map per entry of ``ds_scales``; an entry of ones is ``seg`` itself."""
    s = _device(seg, "seg")
    if axes is not None and list(axes) != [2, 3, 4]:
        raise NotImplementedError(f"augmentation: axes={axes!r} (supported: None, the three spatial axes)")
    output = []
    for sc in ds_scales:
        if all(i == 1 for i in sc):
            output.append(s)
            continue
        new_shape = np.array(s.shape).astype(float)
        for i, a in enumerate((2, 3, 4)):
            new_shape[a] *= sc[i]
        new_shape = np.round(new_shape).astype(int)
        flat = s.reshape((s.shape[0] * s.shape[1],) + tuple(s.shape[2:]))
        out = resampling.resample_data_or_seg(flat, new_shape[2:], True, order=order, cval=cval)
        output.append(out.reshape(tuple(s.shape[:2]) + tuple(int(v) for v in new_shape[2:])))
    return output


# ---- the chain -----------------------------------------------------------------------------------------------------------------------------------
_CASCADE_KEYS = ("move_last_seg_chanel_to_data", "cascade_do_cascade_augmentations")


class MoreDAAugmentation:
    """``get_moreDA_augmentation``'s train transforms (data_augmentation_moreDA.py:60-147) for one batch:
    ``__call__(data, seg) -> {'data': float32 tensor, 'target': float32 tensor, or the list of them when deep_supervision_scales is given}``.

    ``params`` has the keys of ``default_3D_augmentation_params``.  ``seed`` seeds the numpy stream of the draws and the torch stream of the noise
    field; two instances with the same seed give bitwise equal batches.  ``draw(batch, src_shape, channels)`` returns the records of one call and
    ``__call__(..., records=...)`` applies given ones.

    ``params['dummy_2D']`` (the ACDC trainer's anisotropic 16 x 160 x 160 patch, data_augmentation_moreDA.py:54-75) takes the 2-entry
    ``patch_size`` the trainer passes (``patch_size[1:]``): data and seg (B, C, D, H, W) go through the spatial step as (B, C D, H, W) planes,
    one in-plane transform per sample, and come back as (B, C, D, h, w); the low-resolution stage keeps the depth extent
    (``ignore_axes=(0,)``, :91-94); everything else runs in 3-D as without it."""

    def __init__(self, patch_size, params, deep_supervision_scales=None, order_data=3, order_seg=1, border_val_seg=-1, seed=None, soft_ds=False,
                 regions=None):
        assert params.get('mirror') is None, "old version of params, use new keyword do_mirror"
        if params.get("selected_data_channels") is not None:
            raise NotImplementedError("augmentation: selected_data_channels")
        self.patch_size = tuple(int(v) for v in patch_size)
        self.dummy_2D = bool(params.get("dummy_2D"))
        if self.dummy_2D and len(self.patch_size) != 2:
            raise NotImplementedError(f"augmentation: dummy_2D with patch_size {self.patch_size} (the trainer passes patch_size[1:], the two "
                                      "in-plane extents)")
        if not self.dummy_2D and len(self.patch_size) != 3:
            raise NotImplementedError(f"augmentation: patch_size {self.patch_size} without dummy_2D (three spatial extents; the 2-D loader's "
                                      "chain is not part of this module)")
        if params.get("do_elastic"):
            raise NotImplementedError("augmentation: do_elastic (the 3-D trainer sets do_elastic = False)")
        for key in _CASCADE_KEYS:
            if params.get(key):
                raise NotImplementedError(f"augmentation: {key} (the cascade)")
        if regions is not None:
            raise NotImplementedError("augmentation: regions")
        if soft_ds:
            raise NotImplementedError("augmentation: soft_ds")
        mask = params.get("mask_was_used_for_normalization")
        if mask is not None and any(bool(v) for v in (mask.values() if hasattr(mask, "values") else mask)):
            raise NotImplementedError("augmentation: mask_was_used_for_normalization with a channel set (MaskTransform)")
        self.params = dict(params)
        self.deep_supervision_scales = deep_supervision_scales
        self.order_data, self.order_seg, self.border_val_seg = order_data, order_seg, border_val_seg
        self.rs = np.random.RandomState(seed)
        self.seed = seed
        self.generator = None

    def _spatial_keywords(self):
        p = self.params
        return dict(patch_center_dist_from_border=p.get("random_crop_dist_to_border") if p.get("random_crop_dist_to_border") is not None else 30,
                    do_rotation=p.get("do_rotation"), angle_x=p.get("rotation_x"), angle_y=p.get("rotation_y"), angle_z=p.get("rotation_z"),
                    p_rot_per_axis=p.get("rotation_p_per_axis"), do_scale=p.get("do_scaling"), scale=p.get("scale_range"),
                    random_crop=p.get("random_crop"), p_scale_per_sample=p.get("p_scale"), p_rot_per_sample=p.get("p_rot"),
                    independent_scale_for_each_axis=p.get("independent_scale_factor_for_each_axis"))

    def draw(self, batch, src_shape, channels):
        """The records of one call, drawn in the chain's order.  ``src_shape``: the three spatial extents of the batch (with ``dummy_2D`` the
        spatial record is drawn for its last two)."""
        p, rs = self.params, self.rs
        src_shape = tuple(int(v) for v in src_shape)
        if len(src_shape) != 3:
            raise ValueError(f"augmentation: src_shape {src_shape} (the three spatial extents of the batch)")
        rec = {"spatial": draw_spatial(rs, src_shape[1:] if self.dummy_2D else src_shape, self.patch_size, batch, **self._spatial_keywords()),
               "noise": draw_gaussian_noise(rs, batch, (0, 0.1), 0.1),
               "blur": draw_gaussian_blur(rs, batch, channels, (0.5, 1.), True, 0.5, 0.2),
               "brightness": draw_brightness_multiplicative(rs, batch, channels, (0.75, 1.25), True, 0.15)}
        if p.get("do_additive_brightness"):
            rec["additive"] = draw_brightness_additive(rs, batch, channels, p.get("additive_brightness_mu"), p.get("additive_brightness_sigma"), True,
                                                       p.get("additive_brightness_p_per_sample"), p.get("additive_brightness_p_per_channel"))
        rec["contrast"] = draw_contrast(rs, batch, channels, (0.75, 1.25), True, 0.15)
        rec["lowres"] = draw_linear_downsampling_scipy(rs, batch, channels, (0.5, 1), True, 0.5, 0.25)
        rec["gamma_inverted"] = draw_gamma(rs, batch, channels, p.get("gamma_range"), True, 0.1)
        if p.get("do_gamma"):
            rec["gamma"] = draw_gamma(rs, batch, channels, p.get("gamma_range"), True, p["p_gamma"])
        if p.get("do_mirror") or p.get("mirror"):
            rec["mirror"] = draw_mirroring(rs, batch, p.get("mirror_axes"))
        return rec

    def __call__(self, data, seg, records=None, noise=None):
        p = self.params
        x, s = _device(data, "data"), _device(seg, "seg")
        selected = p.get("selected_seg_channels")
        if selected is not None and list(selected) != list(range(s.shape[1])):
            raise NotImplementedError(f"augmentation: selected_seg_channels={selected!r} on {s.shape[1]} seg channels (supported: all of them)")
        B, C = x.shape[:2]
        rec = records if records is not None else self.draw(B, x.shape[2:], C)
        if noise is None and self.generator is None and bool(np.asarray(rec["noise"]["apply"]).any()):
            self.generator = torch.Generator(device=x.device)
            self.generator.manual_seed(int(self.seed) if self.seed is not None else int(self.rs.randint(0, 2 ** 31 - 1)))
        if self.dummy_2D:                                                   # Convert3DTo2DTransform: (channel, depth slice) -> plane
            if tuple(s.shape[2:]) != tuple(x.shape[2:]):
                raise ValueError(f"augmentation: seg {tuple(s.shape)} does not go with data {tuple(x.shape)}")
            depth, x, s = x.shape[2], x.reshape(B, -1, *x.shape[3:]), s.reshape(B, -1, *s.shape[3:])
        x, s = augment_spatial(x, s, self.patch_size, do_elastic_deform=False, border_mode_data=p.get("border_mode_data"), border_cval_data=0,
                               order_data=self.order_data, border_mode_seg="constant", border_cval_seg=self.border_val_seg,
                               order_seg=self.order_seg, params=rec["spatial"])
        if self.dummy_2D:                                                   # Convert2DTo3DTransform
            x, s = x.reshape(B, C, depth, *x.shape[2:]), s.reshape(B, -1, depth, *s.shape[2:])
        x = x if x.dtype == torch.float32 else x.to(torch.float32)          # the loader's batches are float32; so is NumpyToTensor('float')
        flip = _flip_masks(rec["mirror"], B) if "mirror" in rec else np.zeros(B, np.int32)
        last = "gamma" if "gamma" in rec else "gamma_inverted"              # the mirror rides on the last streaming pass of the image
        x = _apply_noise(x, rec["noise"], noise, self.generator)
        x = _apply_blur(x, rec["blur"])
        x = _apply_scale_add(x, rec["brightness"]["apply"], _per_channel(rec["brightness"]["multiplier"], B, C, "multiplier"), np.zeros((B, C)))
        if "additive" in rec:
            x = _apply_scale_add(x, rec["additive"]["apply"], np.ones((B, C)), _per_channel(rec["additive"]["add"], B, C, "add"))
        x = _apply_contrast(x, rec["contrast"])
        x = _apply_lowres(x, rec["lowres"], 0, 3, (0,) if self.dummy_2D else None)
        retain = bool(p.get("gamma_retain_stats"))
        x = _apply_gamma(x, rec["gamma_inverted"], True, retain, flip if last == "gamma_inverted" else None)
        if "gamma" in rec:
            x = _apply_gamma(x, rec["gamma"], False, retain, flip)
        # RemoveLabelTransform(-1, 0) and the mirror of the target in one pass
        sn, _ = _native(s)
        steps = _steps(B, s.shape[1])
        steps[:, 0, 0], steps[:, 0, 1], steps[:, 0, 2] = L.DLKA_AUG_OP_REPLACE, -1.0, 0.0
        target = ops.augment_pointwise(sn, steps, flip=flip)
        if self.deep_supervision_scales is not None:
            target = [t.to(torch.float32) for t in downsample_seg_for_ds_transform2(target, self.deep_supervision_scales, 0, 0)]
        else:
            target = target.to(torch.float32)
        return {"data": x, "target": target}
