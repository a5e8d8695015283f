"""TEST INFRASTRUCTURE — the rules of deformablelka_amd.augmentation (batchgenerators 0.21's transforms as the 3-D trainer chains them, DESIGN.md
4.18) restated through numpy and scipy, never imported by the product.  Built on scipy.ndimage.map_coordinates, scipy.ndimage.gaussian_filter
and tests/resampling_ref.py (resize, resize_segmentation) and nothing else.  Every function takes the record that the product's ``draw_*``
returns, so parity tests hand the same record to both sides.  tests/golden/make_golden_augmentation.py records the fixture from these."""
import numpy as np
from scipy import ndimage

from tests import resampling_ref as R


def coordinates(rec, b, src_shape, patch_size):
    """The (3, D, H, W) source coordinates of sample b, as augment_spatial builds them."""
    coords = np.array(np.meshgrid(*[np.arange(p, dtype=np.float64) - (p - 1) / 2. for p in patch_size], indexing='ij'))
    coords = np.dot(coords.reshape(3, -1).transpose(), np.asarray(rec["rotation"][b], dtype=np.float64)).transpose().reshape(coords.shape)
    for d in range(3):
        coords[d] *= float(rec["scale"][b][d])
        coords[d] += float(rec["center"][b][d])
    return coords


def interpolate_img(img, coords, order, mode, cval, is_seg=False):
    if is_seg and order != 0:
        result = np.zeros(coords.shape[1:], img.dtype)
        for c in np.unique(img):
            result[ndimage.map_coordinates((img == c).astype(float), coords, order=order, mode=mode, cval=cval) >= 0.5] = c
        return result
    return ndimage.map_coordinates(img.astype(float), coords, order=order, mode=mode, cval=cval).astype(img.dtype)


def spatial(data, seg, patch_size, rec, order_data=3, border_mode_data='nearest', border_cval_data=0, order_seg=0, border_mode_seg='constant',
            border_cval_seg=0):
    out = np.zeros(data.shape[:2] + tuple(patch_size), data.dtype)
    out_seg = None if seg is None else np.zeros(seg.shape[:2] + tuple(patch_size), seg.dtype)
    for b in range(data.shape[0]):
        if rec["modified"][b]:
            coords = coordinates(rec, b, data.shape[2:], patch_size)
            for c in range(data.shape[1]):
                out[b, c] = interpolate_img(data[b, c], coords, order_data, border_mode_data, border_cval_data)
            for c in range(0 if seg is None else seg.shape[1]):
                out_seg[b, c] = interpolate_img(seg[b, c], coords, order_seg, border_mode_seg, border_cval_seg, is_seg=True)
        else:
            box = tuple(slice(int(lb), int(lb) + p) for lb, p in zip(rec["crop_lb"][b], patch_size))
            out[b] = data[(b, slice(None)) + box]
            if seg is not None:
                out_seg[b] = seg[(b, slice(None)) + box]
    return out, out_seg


def border_cells(rec, src_shape, patch_size, eps=1e-9):
    """(B, D, H, W) bool: cells of modified samples with a source coordinate within eps of 0 or n - 1 (the 'constant' decision may differ)."""
    out = np.zeros((len(rec["modified"]),) + tuple(patch_size), bool)
    for b in range(out.shape[0]):
        if rec["modified"][b]:
            coords = coordinates(rec, b, src_shape, patch_size)
            for d in range(3):
                out[b] |= (np.abs(coords[d]) < eps) | (np.abs(coords[d] - (src_shape[d] - 1)) < eps)
    return out


def label_weights_close(seg, patch_size, rec, gap, mode='constant', cval=0):
    """(B, Cs, D, H, W) bool: cells where some label's order-1 interpolant is within gap of 0.5."""
    out = np.zeros(seg.shape[:2] + tuple(patch_size), bool)
    for b in range(seg.shape[0]):
        if rec["modified"][b]:
            coords = coordinates(rec, b, seg.shape[2:], patch_size)
            for c in range(seg.shape[1]):
                for lab in np.unique(seg[b, c]):
                    out[b, c] |= np.abs(ndimage.map_coordinates((seg[b, c] == lab).astype(float), coords, order=1, mode=mode, cval=cval) - 0.5) < gap
    return out


def _store(v, dtype):
    return v.astype(dtype)


def gaussian_noise(data, rec, noise):
    out = data.copy()
    for b in range(data.shape[0]):
        if rec["apply"][b]:
            out[b] = _store(data[b].astype(np.float64) + noise[b].astype(np.float64), data.dtype)
    return out


def gaussian_blur(data, rec):
    out = data.copy()
    for b in range(data.shape[0]):
        for c in range(data.shape[1]):
            if rec["sigma"][b][c] > 0:
                out[b, c] = ndimage.gaussian_filter(data[b, c], float(rec["sigma"][b][c]), order=0)
    return out


def gaussian_blur_float32(data, rec):
    """The same filter with float32 sums in another order (plain correlation, left to right): what measures the bound of the blur tests."""
    out = data.copy()
    for b in range(data.shape[0]):
        for c in range(data.shape[1]):
            s = float(rec["sigma"][b][c])
            if s <= 0:
                continue
            r = int(4.0 * s + 0.5)
            k = np.arange(-r, r + 1)
            w = np.exp(-0.5 / (s * s) * k ** 2)
            w = (w / w.sum()).astype(np.float32)
            v = data[b, c].astype(np.float32)
            for ax in range(3):
                n = v.shape[ax]
                acc = np.zeros_like(v)
                for j, wj in zip(k, w):
                    idx = np.arange(n) + j
                    idx = np.mod(idx, 2 * n)
                    idx = np.where(idx >= n, 2 * n - 1 - idx, idx)
                    acc = (acc + np.take(v, idx, ax) * wj).astype(np.float32)
                v = acc
            out[b, c] = v
    return out


def scale_add(data, apply, mul, add):
    out = data.copy()
    for b in range(data.shape[0]):
        if apply[b]:
            for c in range(data.shape[1]):
                out[b, c] = _store(data[b, c].astype(np.float64) * float(mul[b][c]) + float(add[b][c]), data.dtype)
    return out


def brightness_multiplicative(data, rec):
    return scale_add(data, rec["apply"], rec["multiplier"], np.zeros(data.shape[:2]))


def brightness_additive(data, rec):
    return scale_add(data, rec["apply"], np.ones(data.shape[:2]), rec["add"])


def contrast(data, rec):
    out = data.copy()
    for b in range(data.shape[0]):
        if rec["apply"][b]:
            for c in range(data.shape[1]):
                x = data[b, c].astype(np.float64)
                mn, minm, maxm = x.mean(), x.min(), x.max()
                out[b, c] = _store(np.clip((x - mn) * float(rec["factor"][b][c]) + mn, minm, maxm), data.dtype)
    return out


def gamma(data, rec, invert_image=False, retain_stats=False, epsilon=1e-7):
    out = data.copy()
    for b in range(data.shape[0]):
        if rec["apply"][b]:
            for c in range(data.shape[1]):
                x = data[b, c].astype(np.float64)
                if invert_image:
                    x = -x
                mn, sd = x.mean(), x.std()
                minm, rnge = x.min(), x.max() - x.min()
                x = np.power((x - minm) / float(rnge + epsilon), float(rec["gamma"][b][c])) * rnge + minm
                x = _store(x, data.dtype).astype(np.float64)         # the array the package holds between the two steps is the data's dtype
                if retain_stats:
                    x = x - x.mean()
                    x = x / (x.std() + 1e-8) * sd
                    x = x + mn
                if invert_image:
                    x = -x
                out[b, c] = _store(x, data.dtype)
    return out


def linear_downsampling(data, rec, order_downsample=0, order_upsample=3):
    out = data.copy()
    shape = np.array(data.shape[2:])
    for b in range(data.shape[0]):
        for c in range(data.shape[1]):
            z = float(rec["zoom"][b][c])
            if z > 0:
                target = np.round(shape * z).astype(int)
                low = R.resize(data[b, c].astype(float), target, order=order_downsample, mode='edge', anti_aliasing=False)
                out[b, c] = R.resize(low, shape, order=order_upsample, mode='edge', anti_aliasing=False).astype(data.dtype)
    return out


def mirroring(data, seg, rec):
    out, out_seg = data.copy(), None if seg is None else seg.copy()
    for b in range(data.shape[0]):
        for a in range(3):
            if rec["flip"][b][a]:
                out[b] = np.flip(out[b], 1 + a)
                if seg is not None:
                    out_seg[b] = np.flip(out_seg[b], 1 + a)
    return out, out_seg


def more_da(data, seg, patch_size, params, rec, noise, downsample, deep_supervision_scales=None, order_data=3, order_seg=1, border_val_seg=-1):
    """get_moreDA_augmentation's train chain (data_augmentation_moreDA.py:60-147) on the records of MoreDAAugmentation.draw.  ``downsample``
    is the reference's own downsample_seg_for_ds_transform2."""
    x, s = spatial(data, seg, patch_size, rec["spatial"], order_data, params["border_mode_data"], 0, order_seg, "constant", border_val_seg)
    x = gaussian_noise(x, rec["noise"], noise)
    x = gaussian_blur(x, rec["blur"])
    x = brightness_multiplicative(x, rec["brightness"])
    if "additive" in rec:
        x = brightness_additive(x, rec["additive"])
    x = contrast(x, rec["contrast"])
    x = linear_downsampling(x, rec["lowres"], 0, 3)
    x = gamma(x, rec["gamma_inverted"], True, params["gamma_retain_stats"])
    if "gamma" in rec:
        x = gamma(x, rec["gamma"], False, params["gamma_retain_stats"])
    if "mirror" in rec:
        x, s = mirroring(x, s, rec["mirror"])
    s = s.copy()
    s[s == -1] = 0
    target = downsample(s, deep_supervision_scales, 0, 0) if deep_supervision_scales is not None else s
    return x.astype(np.float32), [t.astype(np.float32) for t in target] if isinstance(target, list) else target.astype(np.float32)
