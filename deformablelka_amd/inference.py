"""Sliding-window (tiled) inference with everything resident on the device (BASELINE.json config 5).

Two reference procedures, restated for the GPU:
  * ``predict_3d_tiled`` — nnU-Net's ``_internal_predict_3D_3Dconv_tiled`` (3D/d_lka_former/network_architecture/neural_network.py:
    292-428) with ``_compute_steps_for_sliding_window`` (:266-290) and the Gaussian importance map ``_get_gaussian`` (:250-263);
  * ``predict_single_case`` — the pancreas evaluation ``test_single_case`` (3D/pancreas_code/test_util.py:45-111): fixed strides,
    softmax per tile, plain averaging.
The reference moves every tile host -> device and its prediction device -> host (test_util.py:88,92; neural_network.py:383-386 unless
``all_in_gpu``); here the padded volume, the score map and the weight map live in HBM for the whole volume (a 288 GB device holds any
clinical volume many times over), tiles are gathered and blended on the device, several tiles go through the network per call, and
only the final label / probability maps leave.  Accumulation is fp32 (the reference's ``all_in_gpu`` branch uses fp16).

Test-time mirroring (``predict_3d_tiled(..., do_mirroring=True)``, nnU-Net's ``_internal_maybe_mirror_and_pred_3D``, :502-560): on the device a
chunk of tiles and all its mirrors are gathered from the unpadded volume by one kernel, go through ONE forward, and are blended into the score map
by a second (csrc/cl_tiles.hip, include/dlka.h: dlka_tiles_*); a third writes probabilities and labels at the end.  On the CPU the same
prediction runs as a literal restatement of the reference's loops in torch — the executable specification the HIP path is tested against."""
from __future__ import annotations

import math
import warnings
from typing import Callable, List, Sequence, Tuple

import torch
import torch.nn.functional as F


def compute_steps_for_sliding_window(patch_size: Sequence[int], image_size: Sequence[int], step_size: float) -> List[List[int]]:
    """neural_network.py:266-290: at most ``patch * step_size`` apart, evenly spread so that the last tile ends at the border."""
    assert all(i >= j for i, j in zip(image_size, patch_size)), "image size must be as large or larger than patch_size"
    assert 0 < step_size <= 1, "step_size must be larger than 0 and smaller or equal to 1"
    target = [i * step_size for i in patch_size]
    num_steps = [int(math.ceil((i - k) / j)) + 1 for i, j, k in zip(image_size, target, patch_size)]
    steps = []
    for dim in range(len(patch_size)):
        max_step = image_size[dim] - patch_size[dim]
        actual = max_step / (num_steps[dim] - 1) if num_steps[dim] > 1 else 99999999999
        steps.append([int(round(actual * i)) for i in range(num_steps[dim])])
    return steps


def gaussian_importance_map(patch_size: Sequence[int], sigma_scale: float = 1. / 8, device=None) -> torch.Tensor:
    """neural_network.py:250-263: a unit impulse at the patch centre filtered with ``scipy.ndimage.gaussian_filter(sigma = size *
    sigma_scale, mode='constant')``, normalised to max 1, zeros replaced by the smallest non-zero value.  The filter is separable and the
    input an impulse, so the map is the outer product of three sampled 1-D kernels (scipy truncates them at 4 sigma)."""
    axes = []
    for n in patch_size:
        sigma = n * sigma_scale
        radius = int(4.0 * sigma + 0.5)
        xs = torch.arange(-radius, radius + 1, dtype=torch.float64)
        k = torch.exp(-0.5 * (xs / sigma) ** 2)
        k = k / k.sum()
        line = torch.zeros(n, dtype=torch.float64)
        c = n // 2
        lo, hi = max(0, c - radius), min(n, c + radius + 1)
        line[lo:hi] = k[lo - (c - radius):hi - (c - radius)]
        axes.append(line)
    g = axes[0]
    for a in axes[1:]:
        g = g.unsqueeze(-1) * a
    g = (g / g.max()).to(torch.float32)
    g[g == 0] = g[g != 0].min()
    return g.to(device) if device is not None else g


def softmax_helper(x: torch.Tensor) -> torch.Tensor:
    """Softmax over the class axis: the trainer's ``inference_apply_nonlin`` (d_lka_former_trainer_synapse.py:185).  The HIP blending kernel
    recognises this function by identity and computes it in registers; any other nonlinearity runs in torch before the blend."""
    return torch.softmax(x, 1)


def _pad_amounts(shape: Sequence[int], patch_size: Sequence[int]) -> List[Tuple[int, int]]:
    """pad_nd_image(..., 'constant') up to the patch size: below = d // 2, above = the rest."""
    return [(max(p - n, 0) // 2, max(p - n, 0) - max(p - n, 0) // 2) for n, p in zip(shape, patch_size)]


def _pad_to_patch(x: torch.Tensor, patch_size: Sequence[int], value: float = 0.0) -> Tuple[torch.Tensor, Tuple[slice, ...]]:
    """Symmetric constant padding up to the patch size (batchgenerators' ``pad_nd_image(..., 'constant')`` as called at :308, and
    test_util.py:49-71); returns the padded volume and the slicer that undoes it."""
    pads, slicer = [], []
    for n, p in zip(x.shape[-3:], patch_size):
        d = max(p - n, 0)
        lo = d // 2
        pads.append((lo, d - lo))
        slicer.append(slice(lo, lo + n))
    if any(a or b for a, b in pads):
        x = F.pad(x, [v for a, b in reversed(pads) for v in (a, b)], mode="constant", value=value)
    return x, tuple(slicer)


def _run_tiles(net: Callable, data: torch.Tensor, origins: List[Tuple[int, int, int]], patch_size, tile_batch: int, post: Callable,
               score: torch.Tensor, weight: torch.Tensor, tile_weight: torch.Tensor):
    pd, ph, pw = patch_size
    for i in range(0, len(origins), tile_batch):
        chunk = origins[i:i + tile_batch]
        tiles = torch.stack([data[:, x:x + pd, y:y + ph, z:z + pw] for x, y, z in chunk])       # gathered on the device
        pred = net(tiles)
        if isinstance(pred, (list, tuple)):   # deep supervision: the full-resolution head
            pred = pred[0]
        pred = post(pred).float()
        for t, (x, y, z) in enumerate(chunk):   # overlapping tiles of one chunk must be blended one after the other
            score[:, x:x + pd, y:y + ph, z:z + pw] += pred[t] * tile_weight
            weight[x:x + pd, y:y + ph, z:z + pw] += tile_weight


@torch.no_grad()
def predict_3d_tiled(net: Callable, x: torch.Tensor, patch_size: Sequence[int], step_size: float = 0.5, use_gaussian: bool = True,
                     num_classes: int = None, tile_batch: int = 4, nonlin: Callable = None, *, do_mirroring: bool = False,
                     mirror_axes: Sequence[int] = (0, 1, 2), pad_value: float = 0.0):
    """x: (C, X, Y, Z) on the device.  Returns (predicted_segmentation (X, Y, Z) int64, class_probabilities (K, X, Y, Z) fp32), both on
    the device.  ``nonlin`` = the network's ``inference_apply_nonlin`` (softmax over classes in the reference trainer,
    d_lka_former_trainer_synapse.py:185).
    ``do_mirroring``: test-time mirroring along ``mirror_axes`` (0 = x, 1 = y, 2 = z; :502-560): on a GPU tensor the HIP path (gather, one
    forward over ``tile_batch`` tiles x their mirrors, blend; finalize once), on a CPU tensor the torch restatement of the reference.
    ``pad_value``: the constant of the padding up to the patch size (pad_kwargs['constant_values'])."""
    assert x.ndim == 4, "x must be (c, x, y, z)"
    if do_mirroring:
        return _predict_mirrored(net, x, patch_size, step_size, use_gaussian, tile_batch, nonlin, mirror_axes, pad_value,
                                 impl=_MIRROR_IMPL or ("hip" if x.is_cuda else "torch"))
    nonlin = nonlin if nonlin is not None else (lambda t: torch.softmax(t, 1))
    data, slicer = _pad_to_patch(x, patch_size, pad_value)
    steps = compute_steps_for_sliding_window(patch_size, data.shape[1:], step_size)
    origins = [(a, b, c) for a in steps[0] for b in steps[1] for c in steps[2]]
    if use_gaussian and len(origins) > 1:
        tw = gaussian_importance_map(patch_size, 1. / 8, device=x.device)
    else:
        tw = torch.ones(tuple(patch_size), device=x.device)
    if num_classes is None:
        probe = net(data[None, :, :patch_size[0], :patch_size[1], :patch_size[2]])
        num_classes = (probe[0] if isinstance(probe, (list, tuple)) else probe).shape[1]
    score = torch.zeros((num_classes,) + tuple(data.shape[1:]), device=x.device, dtype=torch.float32)
    weight = torch.zeros(tuple(data.shape[1:]), device=x.device, dtype=torch.float32)
    _run_tiles(net, data, origins, patch_size, tile_batch, nonlin, score, weight, tw)
    probs = (score / weight)[(slice(None),) + slicer]
    return probs.argmax(0), probs


# ---- test-time mirroring ---------------------------------------------------------------------------------------------------------------
# The reference's visiting order (neural_network.py:526-557): m = 0 .. 7 flips the axes {}, {z}, {y}, {z, y}, {x}, {z, x}, {y, x}, {z, y, x},
# each taken only when all its axes are in mirror_axes.  Mask bits: 1 = x, 2 = y, 4 = z (include/dlka.h: dlka_tiles_gather).
_REF_MIRROR_MASKS = (0, 4, 2, 6, 1, 5, 3, 7)
# Measurement / test switch: "torch" sends mirrored prediction of a GPU tensor through the torch restatement instead of the HIP kernels
# (scripts/time_tta.py, tests/test_tta_gpu.py).  None: by device.
_MIRROR_IMPL = None


def mirror_masks(mirror_axes: Sequence[int]) -> List[int]:
    """The mirrors the reference runs for ``mirror_axes``, in its order."""
    return [mk for mk in _REF_MIRROR_MASKS if all(a in mirror_axes for a in range(3) if mk >> a & 1)]


def _flip_dims(mask: int) -> Tuple[int, ...]:
    """torch.flip dims of a mask on a (b, c, x, y, z) tensor, in the reference's listing order (z first: (4, 3, 2))."""
    return tuple(d + 2 for d in (2, 1, 0) if mask >> d & 1)


def _first_head(pred):
    return pred[0] if isinstance(pred, (list, tuple)) else pred   # deep supervision: the full-resolution head


def _predict_mirrored(net: Callable, x: torch.Tensor, patch_size: Sequence[int], step_size: float, use_gaussian: bool, tile_batch: int,
                      nonlin: Callable, mirror_axes: Sequence[int], pad_value: float, impl: str):
    nonlin = nonlin if nonlin is not None else softmax_helper
    patch_size = tuple(int(p) for p in patch_size)
    masks = mirror_masks(mirror_axes)
    scale = 1.0 / 2 ** len(mirror_axes)   # num_results (:517-518)
    training = bool(getattr(net, "training", False))
    if training:
        warnings.warn("Network is in train mode during inference. This may be intended, or not...")   # neural_network.py:134-135
    pads = _pad_amounts(x.shape[1:], patch_size)
    padded = tuple(n + a + b for n, (a, b) in zip(x.shape[1:], pads))
    steps = compute_steps_for_sliding_window(patch_size, padded, step_size)
    origins = [(a, b, c) for a in steps[0] for b in steps[1] for c in steps[2]]
    gauss = gaussian_importance_map(patch_size, 1. / 8, device=x.device) if use_gaussian and len(origins) > 1 else None
    if impl == "hip":
        return _mirrored_hip(net, x, patch_size, pads, padded, origins, masks, scale, gauss, tile_batch, nonlin, pad_value, training)
    return _mirrored_torch(net, x, patch_size, pads, origins, masks, scale, gauss, nonlin, pad_value)


def _mirrored_torch(net, x, patch_size, pads, origins, masks, scale, gauss, nonlin, pad_value):
    """Literal restatement of :403-428 with :502-560 (the non-``all_in_gpu`` branch, fp32 accumulation): per tile, one B = 1 forward per
    mirror; the nonlinearity's output flipped back, scaled by 1 / num_results and summed in visiting order; times the importance map;
    added into the score map, the map itself into the weight map."""
    data, slicer = _pad_to_patch(x, patch_size, pad_value)
    pd, ph, pw = patch_size
    score = weight = None
    add = gauss if gauss is not None else torch.ones(patch_size, device=x.device)
    for (ox, oy, oz) in origins:
        tile = data[None, :, ox:ox + pd, oy:oy + ph, oz:oz + pw]
        result = None
        for mk in masks:
            dims = _flip_dims(mk)
            pred = nonlin(_first_head(net(torch.flip(tile, dims) if dims else tile)))
            pred = torch.flip(pred, dims) if dims else pred
            if result is None:
                result = torch.zeros((1, pred.shape[1]) + patch_size, dtype=torch.float, device=x.device)
            result += scale * pred
        if gauss is not None:
            result[:, :] *= gauss
        if score is None:
            score = torch.zeros((result.shape[1],) + tuple(data.shape[1:]), dtype=torch.float32, device=x.device)
            weight = torch.zeros(tuple(data.shape[1:]), dtype=torch.float32, device=x.device)
        score[:, ox:ox + pd, oy:oy + ph, oz:oz + pw] += result[0]
        weight[ox:ox + pd, oy:oy + ph, oz:oz + pw] += add
    probs = (score / weight)[(slice(None),) + slicer]
    return probs.argmax(0), probs


def _mirrored_hip(net, x, patch_size, pads, padded, origins, masks, scale, gauss, tile_batch, nonlin, pad_value, training):
    """gather -> one forward over T tiles x M mirrors -> blend, per chunk of ``tile_batch`` tiles; finalize once.  In train mode every
    input goes through the net on its own (B = 1), so that batch statistics keep the reference's grouping."""
    from . import _lib, ops
    x = x.float()
    lo = [a for a, _ in pads]
    code = _lib.DLKA_TILES_SOFTMAX if nonlin is softmax_helper else _lib.DLKA_TILES_IDENTITY
    T = max(1, min(int(tile_batch), _lib.DLKA_TILES_MAX_T))
    score = weight = None
    for i in range(0, len(origins), T):
        chunk = origins[i:i + T]
        inp = ops.tiles_gather(x, chunk, masks, patch_size, lo, pad_value)
        if training:
            pred = torch.cat([_first_head(net(inp[b:b + 1])) for b in range(inp.shape[0])])
        else:
            pred = _first_head(net(inp))
        if code == _lib.DLKA_TILES_IDENTITY:
            pred = nonlin(pred)
        if pred.dtype not in (torch.float32, torch.bfloat16):
            pred = pred.float()
        if score is None:
            K = pred.shape[1]
            if K > _lib.DLKA_TILES_K_MAX:
                raise RuntimeError(f"predict_3d_tiled: {K} classes, the mirrored HIP path blends at most {_lib.DLKA_TILES_K_MAX}")
            score = torch.zeros((K,) + padded, dtype=torch.float32, device=x.device)
            weight = torch.zeros(padded, dtype=torch.float32, device=x.device)
        ops.tiles_blend(pred, code, scale, gauss, score, weight, chunk, masks)
    return ops.tiles_finalize(score, weight, lo, tuple(x.shape[1:]))


@torch.no_grad()
def predict_single_case(net: Callable, image: torch.Tensor, stride_xy: int, stride_z: int, patch_size: Sequence[int], num_classes: int = 1,
                        tile_batch: int = 4):
    """test_util.py:45-111.  image: (W, H, D) on the device.  Returns (label_map (W, H, D) int64, score_map (K, W, H, D) fp32)."""
    data, slicer = _pad_to_patch(image[None], patch_size)
    ww, hh, dd = data.shape[1:]
    sx = math.ceil((ww - patch_size[0]) / stride_xy) + 1
    sy = math.ceil((hh - patch_size[1]) / stride_xy) + 1
    sz = math.ceil((dd - patch_size[2]) / stride_z) + 1
    origins = [(min(stride_xy * a, ww - patch_size[0]), min(stride_xy * b, hh - patch_size[1]), min(stride_z * c, dd - patch_size[2]))
               for a in range(sx) for b in range(sy) for c in range(sz)]
    score = torch.zeros((num_classes, ww, hh, dd), device=image.device, dtype=torch.float32)
    cnt = torch.zeros((ww, hh, dd), device=image.device, dtype=torch.float32)
    ones = torch.ones(tuple(patch_size), device=image.device)
    _run_tiles(net, data, origins, patch_size, tile_batch, lambda t: torch.softmax(t, 1), score, cnt, ones)
    score = (score / cnt.unsqueeze(0))[(slice(None),) + slicer]
    return score.argmax(0), score


def num_tiles(image_size: Sequence[int], patch_size: Sequence[int], stride_xy: int, stride_z: int) -> int:
    """Tiles ``predict_single_case`` runs (test_util.py:73-75)."""
    sizes = [max(i, p) for i, p in zip(image_size, patch_size)]
    return (math.ceil((sizes[0] - patch_size[0]) / stride_xy) + 1) * (math.ceil((sizes[1] - patch_size[1]) / stride_xy) + 1) * \
           (math.ceil((sizes[2] - patch_size[2]) / stride_z) + 1)
