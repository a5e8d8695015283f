"""TEST INFRASTRUCTURE: MedPy 0.4.0's medpy.metric.binary (dc, hd, hd95, asd, assd and their __surface_distances) restated with scipy, the
yardstick of deformablelka_amd.metrics.  Needs scipy; the GPU tests read only the fixture recorded from it (tests/golden/reference_metrics.pt)."""
import numpy as np


def surface_distances(result, reference, voxelspacing=None, connectivity=1):
    from scipy.ndimage import binary_erosion, distance_transform_edt, generate_binary_structure
    result, reference = np.atleast_1d(np.asarray(result).astype(bool)), np.atleast_1d(np.asarray(reference).astype(bool))
    if voxelspacing is not None:
        voxelspacing = np.asarray([voxelspacing] * result.ndim if np.isscalar(voxelspacing) else voxelspacing, dtype=np.float64)
    footprint = generate_binary_structure(result.ndim, connectivity)
    if 0 == np.count_nonzero(result):
        raise RuntimeError("The first supplied array does not contain any binary object.")
    if 0 == np.count_nonzero(reference):
        raise RuntimeError("The second supplied array does not contain any binary object.")
    result_border = result ^ binary_erosion(result, structure=footprint, iterations=1)
    reference_border = reference ^ binary_erosion(reference, structure=footprint, iterations=1)
    dt = distance_transform_edt(~reference_border, sampling=voxelspacing)
    return dt[result_border]


def dc(result, reference):
    result, reference = np.asarray(result).astype(bool), np.asarray(reference).astype(bool)
    inter, total = np.count_nonzero(result & reference), np.count_nonzero(result) + np.count_nonzero(reference)
    return 2.0 * inter / float(total) if total else 0.0


def hd(result, reference, voxelspacing=None, connectivity=1):
    return max(surface_distances(result, reference, voxelspacing, connectivity).max(), surface_distances(reference, result, voxelspacing, connectivity).max())


def hd95(result, reference, voxelspacing=None, connectivity=1):
    return np.percentile(np.hstack((surface_distances(result, reference, voxelspacing, connectivity),
                                    surface_distances(reference, result, voxelspacing, connectivity))), 95)


def asd(result, reference, voxelspacing=None, connectivity=1):
    return surface_distances(result, reference, voxelspacing, connectivity).mean()


def assd(result, reference, voxelspacing=None, connectivity=1):
    return np.mean((asd(result, reference, voxelspacing, connectivity), asd(reference, result, voxelspacing, connectivity)))
