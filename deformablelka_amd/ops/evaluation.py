"""What the trainers and evaluators compute on label maps: the segmentation losses, overlap counts and surface distances, connected components."""
import ctypes
from ctypes import byref

import torch

from .. import _lib as L
from ._call import WS, _SD_DTYPES, _rank_padded_ext, call, call_ws, table_dtype


# ---- the trainers' segmentation losses (include/dlka.h: dlka_seg_loss_*, dlka_seg_eval_counts) ---------------------------------------------
def _seg_desc(logits, labels, mode=L.DLKA_SEG_LOSS_NNUNET, batch_dice=False, do_bg=True, smooth=1.0, weight_ce=1.0, weight_dice=1.0, class_weight=None):
    """Checks of the planar pair (logits (B, K, *), labels (B, 1, *) or (B, *) float32 / int64, read as they are) and the description of the call."""
    L.require_device(logits, labels)
    if logits.ndim < 3:
        raise RuntimeError(f"seg_loss: logits must be (B, K, *spatial), got {tuple(logits.shape)}")
    B, K = int(logits.shape[0]), int(logits.shape[1])
    N = logits[0, 0].numel()
    if K > L.DLKA_SEG_LOSS_K_MAX:
        raise NotImplementedError(f"seg_loss: K = {K} classes (the kernels keep at most {L.DLKA_SEG_LOSS_K_MAX} in registers)")
    spatial = tuple(logits.shape[2:])
    if tuple(labels.shape) not in ((B, 1) + spatial, (B,) + spatial):
        raise RuntimeError(f"seg_loss: labels {tuple(labels.shape)} are not a label map of logits {tuple(logits.shape)}")
    if labels.device != logits.device:
        raise RuntimeError("seg_loss: logits and labels live on different devices")
    if labels.dtype not in (torch.float32, torch.int64):
        labels = labels.float() if labels.is_floating_point() else labels.long()
    d = L.SegLossDesc()
    d.B, d.K, d.N = B, K, N
    d.dtype, d.label_dtype = L.dtype_code(logits), (L.DLKA_LABEL_F32 if labels.dtype == torch.float32 else L.DLKA_LABEL_I64)
    d.mode, d.batch_dice, d.do_bg = int(mode), int(bool(batch_dice)), int(bool(do_bg))
    d.smooth, d.weight_ce, d.weight_dice = float(smooth), float(weight_ce), float(weight_dice)
    for k in range(K):
        d.class_weight[k] = 1.0 if class_weight is None else float(class_weight[k])
    return d, logits.contiguous(), labels.contiguous()


def seg_loss_forward(logits, labels, **kw):
    """Returns (loss (), dc (B, K), stats (B, 4K + 2), coef (3BK + 1,), desc, logits, labels): the last three are what ``seg_loss_backward`` takes."""
    d, logits, labels = _seg_desc(logits, labels, **kw)
    B, K = d.B, d.K
    out = torch.empty(1 + B * K + B * (4 * K + 2) + 3 * B * K + 1, dtype=torch.float32, device=logits.device)
    loss, dc, stats, coef = out[0:1], out[1:1 + B * K], out[1 + B * K:1 + B * K + B * (4 * K + 2)], out[1 + B * K + B * (4 * K + 2):]
    call_ws("seg_loss_forward", ("seg_loss_workspace_bytes", byref(d)), logits, L.ptr(logits), L.ptr(labels), byref(d), WS, L.ptr(loss), L.ptr(dc),
            L.ptr(stats), L.ptr(coef), L.stream_ptr(logits))
    return loss.reshape(()), dc.view(B, K), stats.view(B, 4 * K + 2), coef, d, logits, labels


def seg_loss_backward(logits, labels, d, coef, grad_output):
    """The logits' gradient, in their dtype; ``grad_output`` is read on the device (one float32 value)."""
    grad_output = grad_output.to(torch.float32).contiguous()
    L.require_device(logits, labels, coef, grad_output)
    gx = torch.empty_like(logits)
    call("seg_loss_backward", L.ptr(logits), L.ptr(labels), byref(d), L.ptr(coef), L.ptr(grad_output), L.ptr(gx), L.stream_ptr(logits))
    return gx


def seg_eval_counts(logits, labels):
    """(tp, fp, fn), each (K - 1,) int64: hard counts of the foreground classes over the batch (argmax: first maximum)."""
    d, logits, labels = _seg_desc(logits, labels)
    counts = torch.empty((3, d.K - 1), dtype=torch.int64, device=logits.device)
    call_ws("seg_eval_counts", ("seg_loss_workspace_bytes", byref(d)), logits, L.ptr(logits), L.ptr(labels), byref(d), WS, L.ptr(counts),
            L.stream_ptr(logits))
    return counts[0], counts[1], counts[2]


# ---- overlap counts and surface distances of label maps (include/dlka.h: dlka_sd_*) ----------------------------------------------------------
_LABEL_MAPS = "label maps are uint8, int16, int32, int64 or bool"   # what the refusals of the two label-map families say of _SD_DTYPES


def _sd_desc(prediction, label, class_ids=None, voxelspacing=None, connectivity=1):
    """Checks of the pair of maps and the description of the call; ``class_ids=None``: the maps are masks (value != 0)."""
    L.require_device(prediction, label)
    rank = prediction.ndim
    if rank not in (2, 3):
        raise RuntimeError(f"surface distances: the maps must have rank 2 or 3, got {tuple(prediction.shape)}")
    if tuple(prediction.shape) != tuple(label.shape):
        raise RuntimeError(f"surface distances: the two maps differ in extents, {tuple(prediction.shape)} against {tuple(label.shape)}")
    if prediction.numel() == 0:
        raise RuntimeError(f"surface distances: empty extents {tuple(prediction.shape)}")
    if prediction.device != label.device:
        raise RuntimeError("surface distances: the two maps live on different devices")
    for t in (prediction, label):
        table_dtype(t, _SD_DTYPES, "surface distances", _LABEL_MAPS)
    if prediction.dtype != label.dtype:
        common = torch.promote_types(prediction.dtype, label.dtype)
        common = common if common in _SD_DTYPES else torch.int64
        prediction, label = prediction.to(common), label.to(common)
    if voxelspacing is None:
        spacing = [1.0] * rank
    else:
        spacing = [float(s) for s in voxelspacing]
        if len(spacing) != rank:
            raise RuntimeError(f"surface distances: voxelspacing has {len(spacing)} entries for rank {rank}")
        if not all(0.0 < s < 1e100 for s in spacing):
            raise RuntimeError(f"surface distances: voxelspacing must be positive, got {spacing}")
    connectivity = int(connectivity)
    if not 1 <= connectivity <= rank:
        raise RuntimeError(f"surface distances: connectivity must be between 1 and the rank ({rank}), got {connectivity}")
    ids = [0] if class_ids is None else [int(c) for c in class_ids]
    if not 1 <= len(ids) <= L.DLKA_SD_K_MAX:
        raise RuntimeError(f"surface distances: between 1 and {L.DLKA_SD_K_MAX} classes per call, got {len(ids)}")
    d = L.SurfaceDistDesc()
    d.connectivity, d.label_dtype, d.K, d.mask_mode = connectivity, _SD_DTYPES[prediction.dtype], len(ids), int(class_ids is None)
    _rank_padded_ext(d, prediction.shape)
    for ax in range(3):
        d.spacing[ax] = 1.0 if ax < 3 - rank else spacing[ax - (3 - rank)]
    for k, c in enumerate(ids):
        d.class_id[k] = c
    return d, prediction.contiguous(), label.contiguous()


def sd_label_stats(prediction, label, class_ids=None, voxelspacing=None, connectivity=1):
    """Returns (stats (K, 9) int64 on the device = |a & b|, |a|, |b|, box lo d h w, box hi d h w per class; desc, prediction, label): the last
    three are what ``sd_distances`` takes."""
    d, prediction, label = _sd_desc(prediction, label, class_ids, voxelspacing, connectivity)
    stats = torch.empty((d.K, 9), dtype=torch.int64, device=prediction.device)
    call_ws("sd_label_stats", ("sd_stats_workspace_bytes", byref(d)), prediction, L.ptr(prediction), L.ptr(label), byref(d), WS, L.ptr(stats),
            L.stream_ptr(prediction))
    return stats, d, prediction, label


def sd_distances(prediction, label, d, boxes):
    """boxes: K rows (lo d, h, w, extent d, h, w) on the host, an extent of 0 skips the class.  Returns (sqdist float64 on the device, offsets):
    class c with n_c box cells has the squared distances prediction -> label at sqdist[offsets[c] : offsets[c] + n_c] and label -> prediction in
    the n_c cells behind them, -1 off the border."""
    L.require_device(prediction, label)
    flat = [int(v) for row in boxes for v in row]
    if len(flat) != 6 * d.K:
        raise RuntimeError(f"sd_distances: {d.K} boxes of 6 integers expected")
    arr = (ctypes.c_int64 * len(flat))(*flat)
    lib = L.get_lib()
    total = int(lib.dlka_sd_distance_cells(byref(d), arr))
    if total < 0:
        raise RuntimeError("sd_distances: a box lies outside the maps")
    offsets, off = [], 0
    for k in range(d.K):
        offsets.append(off)
        n = flat[6 * k + 3] * flat[6 * k + 4] * flat[6 * k + 5]
        off += 2 * n
    sq = torch.empty(total, dtype=torch.float64, device=prediction.device)
    ws = L.scratch(12 * total, prediction)
    if total:
        call("sd_distances", L.ptr(prediction), L.ptr(label), byref(d), arr, L.ptr(ws), ws.numel(), L.ptr(sq), total, L.stream_ptr(prediction))
    return sq, offsets


# ---- connected components of label maps and the largest-component filter (include/dlka.h: dlka_cc_*) -----------------------------------------
def _cc_desc(image, entries=None, connectivity=1, min_counts=None):
    """Checks of the map and the description of one pass; ``entries``: sequences of class ids, pairwise disjoint; None: the mask (value != 0)."""
    L.require_device(image)
    rank = image.ndim
    if rank not in (1, 2, 3):
        raise RuntimeError(f"connected components: the map must have rank 1, 2 or 3, got {tuple(image.shape)}")
    if image.numel() == 0:
        raise RuntimeError(f"connected components: empty extents {tuple(image.shape)}")
    if image.numel() >= 2 ** 31:
        raise RuntimeError(f"connected components: fewer than 2^31 cells per map, got {image.numel()}")
    table_dtype(image, _SD_DTYPES, "connected components", _LABEL_MAPS)
    connectivity = int(connectivity)
    if not 1 <= connectivity <= rank:
        raise RuntimeError(f"connected components: connectivity must be between 1 and the rank ({rank}), got {connectivity}")
    d = L.ConnCompDesc()
    d.connectivity, d.label_dtype, d.mask_mode = connectivity, _SD_DTYPES[image.dtype], int(entries is None)
    _rank_padded_ext(d, image.shape)
    if entries is None:
        d.K, d.n_ids = 1, 0
    else:
        pairs = [(int(c), k) for k, ids in enumerate(entries) for c in ids]
        if not 1 <= len(entries) <= L.DLKA_CC_K_MAX or not 1 <= len(pairs) <= L.DLKA_CC_IDS_MAX:
            raise RuntimeError(f"connected components: between 1 and {L.DLKA_CC_K_MAX} entries and at most {L.DLKA_CC_IDS_MAX} class ids per pass, "
                               f"got {len(entries)} and {len(pairs)}")
        if len({c for c, _ in pairs}) != len(pairs):
            raise RuntimeError("connected components: the entries of one pass must not share a class id")
        d.K, d.n_ids = len(entries), len(pairs)
        for j, (c, k) in enumerate(pairs):
            d.class_id[j], d.entry_of[j] = c, k
    if min_counts is not None:
        if len(min_counts) != d.K:
            raise RuntimeError(f"connected components: {d.K} minimum counts expected, got {len(min_counts)}")
        d.has_min = 1
        for k, t in enumerate(min_counts):
            d.min_count[k] = int(t)
    return d, image.contiguous()


def cc_components(image, entries=None, connectivity=1, min_counts=None, want_filtered=True):
    """One pass.  Returns (labels int32 like the map, filtered (dtype of the map) or None, summary int32 (DLKA_CC_SUMMARY,) on the device =
    [components, largest size per entry ..., largest removed size per entry ...], state): ``state`` is what ``cc_component_table`` takes."""
    d, image = _cc_desc(image, entries, connectivity, min_counts)
    labels = torch.empty(image.shape, dtype=torch.int32, device=image.device)
    filtered = torch.empty_like(image) if want_filtered else None
    summary = torch.empty(L.DLKA_CC_SUMMARY, dtype=torch.int32, device=image.device)
    ws = call_ws("cc_components", ("cc_workspace_bytes", byref(d)), image, L.ptr(image), byref(d), WS, L.ptr(labels), L.ptr(filtered), L.ptr(summary),
                 L.stream_ptr(image))
    return labels, filtered, summary, (d, ws)


def cc_component_table(state, n):
    """(sizes int64 (n,), owner int32 (n,)) of the components 1..n of the pass that returned ``state``."""
    d, ws = state
    sizes = torch.empty(n, dtype=torch.int64, device=ws.device)
    owner = torch.empty(n, dtype=torch.int32, device=ws.device)
    call("cc_component_table", byref(d), L.ptr(ws), ws.numel(), n, L.ptr(sizes), L.ptr(owner), L.stream_ptr(ws))
    return sizes, owner
