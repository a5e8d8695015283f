"""TEST INFRASTRUCTURE: nnU-Net's connected-component post-processing (3D/d_lka_former/postprocessing/connected_components.py:48-105 of the
reference) restated with scipy, for the host halves of the tests and of scripts/time_postprocessing.py.  tests/test_postprocessing_emu.py holds
it to the fixture recorded from the reference's own function (tests/golden/reference_postprocessing.pt)."""
import numpy as np
from scipy import ndimage


def label(mask, connectivity=1):
    mask = np.asarray(mask) != 0
    return ndimage.label(mask, ndimage.generate_binary_structure(mask.ndim, connectivity))


def remove_all_but_the_largest_connected_component(image, for_which_classes, volume_per_voxel, minimum_valid_object_size=None):
    """Returns (a filtered COPY of image, largest_removed, kept_size); entries are applied in order, each on the map the previous one left."""
    image = np.array(image, copy=True)
    if for_which_classes is None:
        for_which_classes = [int(c) for c in np.unique(image) if c > 0]
    if 0 in for_which_classes:
        raise AssertionError("cannot remove background")
    largest_removed, kept_size = {}, {}
    for c in for_which_classes:
        key = tuple(c) if isinstance(c, (list, tuple)) else c
        mask = np.isin(image, list(key) if isinstance(key, tuple) else [key])
        lmap, n = ndimage.label(mask)
        sizes = np.bincount(lmap.ravel(), minlength=n + 1)[1:].astype(np.float64) * volume_per_voxel
        largest_removed[key] = kept_size[key] = None
        if n == 0:
            continue
        top = sizes.max()
        kept_size[key] = float(top)
        drop = sizes != top
        if minimum_valid_object_size is not None:
            drop &= sizes < minimum_valid_object_size[key]
        if drop.any():
            largest_removed[key] = float(sizes[drop].max())
            image[np.isin(lmap, np.flatnonzero(drop) + 1)] = 0
    return image, largest_removed, kept_size
