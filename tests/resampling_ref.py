"""TEST INFRASTRUCTURE — the semantics of deformablelka_amd.resampling restated through scipy, never imported by the product.

skimage and batchgenerators are not needed: ``resize`` is skimage.transform.resize(x, new, order, mode='edge', anti_aliasing=False, cval=...)
and ``resize_segmentation`` is batchgenerators.augmentations.utils.resize_segmentation, both stated through
scipy.ndimage.map_coordinates(mode='nearest') at the source coordinates (i + 0.5) * n_in / n_out - 0.5 (bitwise what
scipy.ndimage.zoom(grid_mode=True, mode='nearest') returns for orders 0, 1 and 3).  tests/golden/make_golden_resampling.py binds these two
into the reference's own resample_data_or_seg / resample_patient / export when it records the fixture."""
import numpy as np
from scipy import ndimage


def resize(image, output_shape, order=1, mode='edge', cval=0, clip=True, preserve_range=False, anti_aliasing=False, **kwargs):
    assert mode == 'edge' and not anti_aliasing
    x = np.asarray(image).astype(float)
    output_shape = tuple(int(v) for v in output_shape)
    assert len(output_shape) == x.ndim
    grids = np.meshgrid(*[(np.arange(o, dtype=np.float64) + 0.5) * (float(n) / o) - 0.5 for n, o in zip(x.shape, output_shape)], indexing='ij')
    out = ndimage.map_coordinates(x, np.array(grids), order=order, mode='nearest')
    if order >= 1 and clip:
        out = np.clip(out, x.min(), x.max())
    return out


def resize_segmentation(segmentation, new_shape, order=3, cval=0):
    tpe = segmentation.dtype
    assert len(segmentation.shape) == len(new_shape), "new shape must have same dimensionality as segmentation"
    if order == 0:
        return resize(segmentation.astype(float), new_shape, order, mode="edge", clip=True, anti_aliasing=False).astype(tpe)
    reshaped = np.zeros(new_shape, dtype=segmentation.dtype)
    for c in np.unique(segmentation):
        reshaped_multihot = resize((segmentation == c).astype(float), new_shape, order, mode="edge", clip=True, anti_aliasing=False)
        reshaped[reshaped_multihot >= 0.5] = c
    return reshaped


def zoom_check(x, new_shape, order):
    """The statement above, checked: zoom(grid_mode=True, mode='nearest') without the clip."""
    return ndimage.zoom(np.asarray(x).astype(float), [o / n for n, o in zip(x.shape, new_shape)], order=order, mode='nearest', grid_mode=True)
