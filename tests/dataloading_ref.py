"""TEST INFRASTRUCTURE — numpy restatement of what deformablelka_amd.dataloading computes: the class_locations lines of
GenericPreprocessor._run_internal (3D/d_lka_former/preprocessing/preprocessing.py:333-348), the cut-and-pad of
DataLoader3D.generate_train_batch (training/dataloading/dataset_loading.py:331-368) and the loader's draws (:224, :275-329).  Held to
tests/golden/reference_dataloading.pt, which was recorded from the reference's own code; it tells WHICH cell differs where the fixture holds a
digest, and it is the host baseline of scripts/time_dataloading.py.  Never used by the product."""
import numpy as np


def class_locations(seg, all_classes, num_samples=10000, min_percent_coverage=0.01, seed=1234):
    """preprocessing.py:333-348, line by line, on one label map."""
    rndst = np.random.RandomState(seed)
    class_locs = {}
    for c in all_classes:
        all_locs = np.argwhere(seg == c)
        if len(all_locs) == 0:
            class_locs[c] = []
            continue
        target_num_samples = min(num_samples, len(all_locs))
        target_num_samples = max(target_num_samples, int(np.ceil(len(all_locs) * min_percent_coverage)))
        selected = all_locs[rndst.choice(len(all_locs), target_num_samples, replace=False)]
        class_locs[c] = selected
    return class_locs


def crop(case_all_data, bbox_lb, patch_size, pad_mode="constant", pad_kwargs_data=None):
    """dataset_loading.py:331-368 for one sample: (data (C, *patch), seg (1, *patch)) float32."""
    shape = case_all_data.shape[1:]
    lb = [int(v) for v in bbox_lb]
    ub = [lb[d] + int(patch_size[d]) for d in range(3)]
    valid = tuple(slice(max(0, lb[d]), min(shape[d], ub[d])) for d in range(3))
    pad = ((0, 0),) + tuple((-min(0, lb[d]), max(ub[d] - shape[d], 0)) for d in range(3))
    cut = np.copy(case_all_data[(slice(None),) + valid])
    data = np.pad(cut[:-1], pad, pad_mode, **(pad_kwargs_data or {}))
    seg = np.pad(cut[-1:], pad, 'constant', **{'constant_values': -1})
    return data.astype(np.float32), seg.astype(np.float32)


def crop_batch(cases, bbox_lb, patch_size, pad_mode="constant", pad_kwargs_data=None):
    """The batch of ``crop``: (data (B, C, *patch), seg (B, 1, *patch))."""
    rows = [crop(c, lb, patch_size, pad_mode, pad_kwargs_data) for c, lb in zip(cases, bbox_lb)]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


def do_oversample(batch_idx, batch_size, oversample_foreground_percent):
    return not batch_idx < round(batch_size * (1 - oversample_foreground_percent))


def draw_boxes(rs, cases, patch_size, need_to_pad, batch_size, oversample_foreground_percent):
    """:224, :275-329: (keys, bbox_lb (B, 3)).  ``cases``: key -> (shape, properties); ``need_to_pad`` is updated in place as the reference's
    aliased array is."""
    keys = rs.choice(list(cases.keys()), batch_size, True, None)
    boxes = np.zeros((batch_size, 3), np.int64)
    for j, i in enumerate(keys):
        shape, properties = cases[i]
        for d in range(3):
            if need_to_pad[d] + shape[d] < patch_size[d]:
                need_to_pad[d] = patch_size[d] - shape[d]
        lb = [- need_to_pad[d] // 2 for d in range(3)]
        ub = [shape[d] + need_to_pad[d] // 2 + need_to_pad[d] % 2 - patch_size[d] for d in range(3)]
        voxels = None
        if do_oversample(j, batch_size, oversample_foreground_percent):
            locs = properties['class_locations']
            fg = np.array([c for c in locs.keys() if len(locs[c]) != 0])
            fg = fg[fg > 0]
            if len(fg) != 0:
                voxels = locs[rs.choice(fg)]
        if voxels is not None:
            voxel = voxels[rs.choice(len(voxels))]
            boxes[j] = [max(lb[d], voxel[d] - patch_size[d] // 2) for d in range(3)]
        else:
            boxes[j] = [rs.randint(lb[d], ub[d] + 1) for d in range(3)]
    return keys, boxes


def generate_train_batch(rs, arrays, cases, patch_size, need_to_pad, batch_size, oversample_foreground_percent, pad_mode, pad_kwargs_data):
    """One batch on the host, as the reference forms it: the baseline the timing script uploads."""
    keys, boxes = draw_boxes(rs, cases, patch_size, need_to_pad, batch_size, oversample_foreground_percent)
    data, seg = crop_batch([arrays[k] for k in keys], boxes, patch_size, pad_mode, pad_kwargs_data)
    return {'data': data, 'seg': seg, 'keys': keys}
