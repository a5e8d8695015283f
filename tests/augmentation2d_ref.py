"""TEST INFRASTRUCTURE — the dummy-2D branch of the ACDC trainer's augmentation (data_augmentation_moreDA.py:54-75 and :91-94; batchgenerators
0.21's augment_spatial with dim == 2 between Convert3DTo2DTransform and Convert2DTo3DTransform) restated through numpy and
scipy.ndimage.map_coordinates on 2-D planes, per plane and per label, never imported by the product.  The colour stages and ``resize`` come
from tests/augmentation_ref.py and tests/resampling_ref.py.  Every function takes the record that the product's ``draw_*`` returns.
tests/golden/make_golden_augmentation2d.py records the fixture from these."""
import numpy as np
from scipy import ndimage

from tests import augmentation_ref as A3
from tests import resampling_ref as R


def coordinates(rec, b, patch_size):
    """The (2, h, w) source coordinates of sample b, as augment_spatial builds them for dim == 2."""
    coords = np.array(np.meshgrid(*[np.arange(p, dtype=np.float64) - (p - 1) / 2. for p in patch_size], indexing='ij'))
    coords = np.dot(coords.reshape(2, -1).transpose(), np.asarray(rec["rotation"][b], dtype=np.float64)).transpose().reshape(coords.shape)
    for d in range(2):
        coords[d] *= float(rec["scale"][b][d])
        coords[d] += float(rec["center"][b][d])
    return coords


def spatial(data, seg, patch_size, rec, order_data=3, border_mode_data='nearest', border_cval_data=0, order_seg=0, border_mode_seg='constant',
            border_cval_seg=0):
    """data (B, P, H, W), seg (B, Ps, H, W) or None: every plane is one 2-D map_coordinates call (interpolate_img)."""
    out = np.zeros(data.shape[:2] + tuple(patch_size), data.dtype)
    out_seg = None if seg is None else np.zeros(seg.shape[:2] + tuple(patch_size), seg.dtype)
    for b in range(data.shape[0]):
        if rec["modified"][b]:
            coords = coordinates(rec, b, patch_size)
            for c in range(data.shape[1]):
                out[b, c] = A3.interpolate_img(data[b, c], coords, order_data, border_mode_data, border_cval_data)
            for c in range(0 if seg is None else seg.shape[1]):
                out_seg[b, c] = A3.interpolate_img(seg[b, c], coords, order_seg, border_mode_seg, border_cval_seg, is_seg=True)
        else:
            box = tuple(slice(int(lb), int(lb) + p) for lb, p in zip(rec["crop_lb"][b], patch_size))
            out[b] = data[(b, slice(None)) + box]
            if seg is not None:
                out_seg[b] = seg[(b, slice(None)) + box]
    return out, out_seg


def spatial_5d(data, seg, patch_size, rec, **kw):
    """Convert3DTo2DTransform, the 2-D SpatialTransform, Convert2DTo3DTransform."""
    B, C, D = data.shape[:3]
    s2 = None if seg is None else seg.reshape((B, -1) + seg.shape[3:])
    x, s = spatial(data.reshape((B, C * D) + data.shape[3:]), s2, patch_size, rec, **kw)
    return x.reshape((B, C, D) + tuple(patch_size)), None if s is None else s.reshape((B, -1, D) + tuple(patch_size))


def border_cells(rec, src_shape, patch_size, eps=1e-9):
    """(B, h, w) bool: cells of modified samples with a source coordinate within eps of 0 or n - 1 (the 'constant' decision may differ)."""
    out = np.zeros((len(rec["modified"]),) + tuple(patch_size), bool)
    for b in range(out.shape[0]):
        if rec["modified"][b]:
            coords = coordinates(rec, b, patch_size)
            for d in range(2):
                out[b] |= (np.abs(coords[d]) < eps) | (np.abs(coords[d] - (src_shape[d] - 1)) < eps)
    return out


def outside_fraction(rec, b, src_shape, patch_size):
    coords = coordinates(rec, b, patch_size)
    out = np.zeros(tuple(patch_size), bool)
    for d in range(2):
        out |= (coords[d] < 0) | (coords[d] > src_shape[d] - 1)
    return float(out.mean())


def label_weights_close(seg, patch_size, rec, gap, mode='constant', cval=0):
    """(B, Ps, h, w) bool: cells where some label's order-1 interpolant is within gap of 0.5."""
    out = np.zeros(seg.shape[:2] + tuple(patch_size), bool)
    for b in range(seg.shape[0]):
        if rec["modified"][b]:
            coords = coordinates(rec, b, patch_size)
            for c in range(seg.shape[1]):
                for lab in np.unique(seg[b, c]):
                    out[b, c] |= np.abs(ndimage.map_coordinates((seg[b, c] == lab).astype(float), coords, order=1, mode=mode, cval=cval) - 0.5) < gap
    return out


def linear_downsampling(data, rec, order_downsample=0, order_upsample=3, ignore_axes=None):
    """augment_linear_downsampling_scipy with ignore_axes: the target keeps the extent of those spatial axes.  Returns (result, the shapes of
    the low-resolution arrays per (b, c); None where the channel is skipped)."""
    out = data.copy()
    shape = np.array(data.shape[2:])
    low_shapes = {}
    for b in range(data.shape[0]):
        for c in range(data.shape[1]):
            z = float(rec["zoom"][b][c])
            low_shapes[(b, c)] = None
            if z > 0:
                target = np.round(shape * z).astype(int)
                if ignore_axes is not None:
                    for i in ignore_axes:
                        target[i] = shape[i]
                low = R.resize(data[b, c].astype(float), target, order=order_downsample, mode='edge', anti_aliasing=False)
                low_shapes[(b, c)] = tuple(int(v) for v in low.shape)
                out[b, c] = R.resize(low, shape, order=order_upsample, mode='edge', anti_aliasing=False).astype(data.dtype)
    return out, low_shapes


def more_da(data, seg, patch_size, params, rec, noise, downsample, deep_supervision_scales=None, order_data=3, order_seg=1, border_val_seg=-1):
    """get_moreDA_augmentation's train chain with params['dummy_2D'] on the records of MoreDAAugmentation.draw.  ``downsample`` is
    downsample_seg_for_ds_transform2 (training/data_augmentation/downsampling.py:88) restated by the caller."""
    x, s = spatial_5d(data, seg, patch_size, rec["spatial"], order_data=order_data, border_mode_data=params["border_mode_data"],
                      border_cval_data=0, order_seg=order_seg, border_mode_seg="constant", border_cval_seg=border_val_seg)
    x = A3.gaussian_noise(x, rec["noise"], noise)
    x = A3.gaussian_blur(x, rec["blur"])
    x = A3.brightness_multiplicative(x, rec["brightness"])
    if "additive" in rec:
        x = A3.brightness_additive(x, rec["additive"])
    x = A3.contrast(x, rec["contrast"])
    x, _ = linear_downsampling(x, rec["lowres"], 0, 3, ignore_axes=(0,))
    x = A3.gamma(x, rec["gamma_inverted"], True, params["gamma_retain_stats"])
    if "gamma" in rec:
        x = A3.gamma(x, rec["gamma"], False, params["gamma_retain_stats"])
    if "mirror" in rec:
        x, s = A3.mirroring(x, s, rec["mirror"])
    s = s.copy()
    s[s == -1] = 0
    target = downsample(s, deep_supervision_scales) if deep_supervision_scales is not None else s
    return x.astype(np.float32), [t.astype(np.float32) for t in target] if isinstance(target, list) else target.astype(np.float32)


def downsample_seg(seg, ds_scales, order=0):
    """downsample_seg_for_ds_transform2 (order 0, all axes): resize_segmentation of every (b, c) to round(shape * scale)."""
    output = []
    for sc in ds_scales:
        if all(i == 1 for i in sc):
            output.append(seg)
            continue
        new_shape = np.array(seg.shape).astype(float)
        for i, a in enumerate((2, 3, 4)):
            new_shape[a] *= sc[i]
        new_shape = np.round(new_shape).astype(int)
        out = np.zeros(new_shape, dtype=seg.dtype)
        for b in range(seg.shape[0]):
            for c in range(seg.shape[1]):
                out[b, c] = R.resize_segmentation(seg[b, c], new_shape[2:], order)
        output.append(out)
    return output
