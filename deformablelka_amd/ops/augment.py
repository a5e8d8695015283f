"""Train-time augmentation."""
import math
from ctypes import byref

import numpy as np
import torch

from .. import _lib as L
from .. import ops as _ops   # another family's wrapper is called through the package, as the product modules call it
from ._call import WS, _AUG_DTYPES, _I3, _RS_DTYPES, call, call_ws, table_dtype


# ---- train-time augmentation (include/dlka.h: dlka_augment_*) -----------------------------------------------------------------------------
# rank 3: volumes (b, c, x, y, z).  rank 2, the dummy-2D branch: (b, p, y, z), p the planes of a sample (channels x depth slices); the
# description's third extents are 0.  The words the messages of a rank use:
_AUG_WORDS = {3: ("(b, c, x, y, z)", "channel", "three", "volumes"), 2: ("(b, p, y, z)", "plane", "two", "planes")}


def _aug_volume(x, what, rank=3):
    L.require_device(x)
    if x.ndim != 2 + rank or x.numel() == 0:
        raise RuntimeError(f"augment: {what} is {_AUG_WORDS[rank][0]} with no empty axis, got {tuple(x.shape)}")
    if x[0, 0].numel() >= 2 ** 31:
        raise RuntimeError(f"augment: fewer than 2^31 cells per {_AUG_WORDS[rank][1]}")
    return x.contiguous()


def _aug_data(x, rank=3):
    x = _aug_volume(x, "data", rank)
    table_dtype(x, _AUG_DTYPES, "augment", f"float32, bfloat16, float64 or int16 {_AUG_WORDS[rank][3]}")
    return x


def _aug_desc(x, out, order, mode, cval, pad=0, dtype=L.DLKA_F32):
    rank = x.ndim - 2
    out = tuple(int(v) for v in out)
    if len(out) != rank or min(out) < 1 or math.prod(out) >= 2 ** 31:
        raise RuntimeError(f"augment: {_AUG_WORDS[rank][2]} positive patch extents below 2^31 cells, got {out}")
    d = L.AugmentDesc()
    d.B, d.C, d.dtype, d.order, d.mode, d.pad, d.cval = int(x.shape[0]), int(x.shape[1]), dtype, int(order), int(mode), int(pad), float(cval)
    for ax in range(3):
        d.src[ax], d.out[ax] = (int(x.shape[2 + ax]), out[ax]) if ax < rank else (0, 0)
    return d, out


def _aug_sample_tables(x, out, maps, plain):
    """maps (B, rank, rank + 1) float64 and plain (B, 1 + rank) int (flag, lower bound per axis) on the device.  The kernels trust the boxes:
    checked here."""
    rank = x.ndim - 2
    maps = np.ascontiguousarray(np.asarray(maps, dtype=np.float64).reshape(-1, rank * (rank + 1)))
    plain = np.ascontiguousarray(np.asarray(plain, dtype=np.int32).reshape(-1, 1 + rank))
    if maps.shape[0] != x.shape[0] or plain.shape[0] != x.shape[0]:
        raise RuntimeError(f"augment: one map and one crop record per sample ({x.shape[0]})")
    for b in range(plain.shape[0]):
        if plain[b, 0] and any(plain[b, 1 + ax] < 0 or plain[b, 1 + ax] + out[ax] > x.shape[2 + ax] for ax in range(rank)):
            raise RuntimeError(f"augment: the crop of sample {b} at {plain[b, 1:].tolist()} leaves the source {tuple(x.shape[2:])}")
    return torch.from_numpy(maps).to(x.device), torch.from_numpy(plain).to(x.device)


def _aug_spline_source(x, mode):
    """What the prefilter reads (float32 / float64), and scipy's padding and start values for ``mode``."""
    src = x if x.dtype in _RS_DTYPES else x.to(torch.float64 if x.dtype == torch.int16 else torch.float32)
    return (src, L.DLKA_RESAMPLE_SPLINE_PAD, L.DLKA_SPLINE_REFLECT) if mode == L.DLKA_AUG_NEAREST else (src, 0, L.DLKA_SPLINE_MIRROR)


def _aug_spatial(x, out, maps, plain, order, mode, cval, rank):
    x = _aug_data(x, rank)
    coefficients, entry = ((augment_spline_coefficients, "augment_spatial") if rank == 3
                           else (augment_spline_coefficients2d, "augment_spatial2d"))
    coef, pad = (coefficients(x, mode) if order == 3 and not all(int(p[0]) for p in np.asarray(plain).reshape(-1, 1 + rank)) else (None, 0))
    if order == 3 and coef is None:
        order = 0                                            # every sample is a plain crop: nothing is interpolated
    d, out = _aug_desc(x, out, order, mode, cval, pad, _AUG_DTYPES[x.dtype])
    m, p = _aug_sample_tables(x, out, maps, plain)
    y = torch.empty(tuple(x.shape[:2]) + out, dtype=x.dtype, device=x.device)
    call(entry, L.ptr(x), L.ptr(coef), L.ptr(y), byref(d), L.ptr(m), L.ptr(p), L.stream_ptr(x))
    return y


def _aug_spatial_labels(seg, out, maps, plain, order, mode, cval, rank):
    seg = _aug_volume(seg, "seg", rank)
    if seg.dtype != torch.int32:
        raise RuntimeError(f"augment: int32 label maps, got {seg.dtype}")
    d, out = _aug_desc(seg, out, order, mode, cval)
    m, p = _aug_sample_tables(seg, out, maps, plain)
    y = torch.empty(tuple(seg.shape[:2]) + out, dtype=torch.int32, device=seg.device)
    entry = "augment_spatial_labels" if rank == 3 else "augment_spatial2d_labels"
    call(entry, L.ptr(seg), L.ptr(y), byref(d), L.ptr(m), L.ptr(p), L.stream_ptr(seg))
    return y


def augment_spline_coefficients(x, mode):
    """float64 cubic B-spline coefficients of every channel of ``x`` (b, c, x, y, z), as scipy.ndimage.map_coordinates prepares them: mode
    'nearest' pads DLKA_RESAMPLE_SPLINE_PAD edge samples and filters with the 'reflect' start values, 'constant' filters the array itself
    with the 'mirror' ones.  Returns (coefficients (b, c, x + 2 pad, ...), pad)."""
    x = _aug_volume(x, "data")
    src, pad, boundary = _aug_spline_source(x, mode)
    ext = [int(n) + 2 * pad for n in x.shape[2:]]
    if ext[0] * ext[1] * ext[2] >= 2 ** 31:
        raise RuntimeError("augment: fewer than 2^31 cells per padded channel")
    coef = torch.empty([x.shape[0], x.shape[1]] + ext, dtype=torch.float64, device=x.device)
    for b in range(x.shape[0]):
        for c in range(x.shape[1]):
            _ops.spline_coefficients(src[b, c], (pad, pad, pad), boundary, range(3), out=coef[b, c])
    return coef, pad


def augment_spatial(x, out, maps, plain, order, mode, cval):
    """``x`` (b, c, x, y, z; float32, bfloat16, float64, int16) sampled at the per-sample affine ``maps`` with scipy's map_coordinates rules
    (orders 0, 1, 3; mode DLKA_AUG_CONSTANT / DLKA_AUG_NEAREST); samples whose ``plain`` flag is set are copied boxes."""
    return _aug_spatial(x, out, maps, plain, order, mode, cval, 3)


def augment_spatial_labels(seg, out, maps, plain, order, mode, cval):
    """int32 label maps (b, c, x, y, z) at the same coordinates: order 0 the nearest cell, order 1 the largest label whose trilinear weight is
    >= 0.5, else 0."""
    return _aug_spatial_labels(seg, out, maps, plain, order, mode, cval, 3)


def augment_spline_coefficients2d(x, mode):
    """float64 cubic B-spline coefficients of every plane of ``x`` (b, p, y, z), as scipy.ndimage.map_coordinates prepares them for a 2-D
    array: the in-plane axes alone are padded (mode 'nearest': DLKA_RESAMPLE_SPLINE_PAD edge samples, 'reflect' start values; 'constant': no
    padding, 'mirror') and filtered.  The batch's stack of planes is ONE volume (b p, y, z) filtered along its axes 1 and 2: three launches
    whatever b and p are; a stack of 2^31 padded cells or more goes sample by sample.  Returns (coefficients (b, p, y + 2 pad, z + 2 pad), pad)."""
    x = _aug_volume(x, "data", 2)
    src, pad, boundary = _aug_spline_source(x, mode)
    B, P = int(x.shape[0]), int(x.shape[1])
    ext = [int(n) + 2 * pad for n in x.shape[2:]]
    if P * ext[0] * ext[1] >= 2 ** 31:
        raise RuntimeError("augment: fewer than 2^31 cells per padded sample")
    coef = torch.empty([B, P] + ext, dtype=torch.float64, device=x.device)
    if B * P * ext[0] * ext[1] < 2 ** 31:
        _ops.spline_coefficients(src.reshape(B * P, *x.shape[2:]), (0, pad, pad), boundary, (1, 2), out=coef.reshape(B * P, *ext))
    else:
        for b in range(B):
            _ops.spline_coefficients(src[b], (0, pad, pad), boundary, (1, 2), out=coef[b])
    return coef, pad


def augment_spatial2d(x, out, maps, plain, order, mode, cval):
    """``x`` (b, p, y, z; float32, bfloat16, float64, int16): every plane of sample b sampled at the in-plane affine ``maps[b]`` (2, 3) with
    scipy's 2-D map_coordinates rules (orders 0, 1, 3: 1 / 4 / 16 taps; mode DLKA_AUG_CONSTANT / DLKA_AUG_NEAREST); samples whose ``plain``
    flag is set are copied in-plane boxes.  batchgenerators' augment_spatial with dim == 2 on the planes the dummy-2D branch makes."""
    return _aug_spatial(x, out, maps, plain, order, mode, cval, 2)


def augment_spatial2d_labels(seg, out, maps, plain, order, mode, cval):
    """int32 label planes (b, p, y, z) at the same coordinates: order 0 the nearest cell, order 1 the largest label whose bilinear weight over
    the 4 in-plane neighbours is >= 0.5, else 0."""
    return _aug_spatial_labels(seg, out, maps, plain, order, mode, cval, 2)


def augment_gaussian(x, radius, weights):
    """scipy.ndimage.gaussian_filter of every channel of ``x`` (b, c, x, y, z), one launch per axis: ``radius`` (b * c,) int, < 0 = the channel
    is copied; ``weights`` (b * c, DLKA_AUG_RADIUS_MAX + 1) float64, centre first."""
    x = _aug_data(x)
    n = x.shape[0] * x.shape[1]
    radius = np.ascontiguousarray(np.asarray(radius, dtype=np.int32).reshape(-1))
    weights = np.ascontiguousarray(np.asarray(weights, dtype=np.float64))
    if radius.shape != (n,) or weights.shape != (n, L.DLKA_AUG_RADIUS_MAX + 1) or radius.max() > L.DLKA_AUG_RADIUS_MAX:
        raise RuntimeError(f"augment: {n} radii of at most {L.DLKA_AUG_RADIUS_MAX} and their weight rows expected")
    r, w = torch.from_numpy(radius).to(x.device), torch.from_numpy(weights).to(x.device)
    for ax in range(3):
        y = torch.empty_like(x)
        call("augment_gaussian", L.ptr(x), L.ptr(y), _AUG_DTYPES[x.dtype], n, _I3(*x.shape[2:]), ax, L.ptr(r), L.ptr(w), L.stream_ptr(x))
        x = y
    return x


def augment_channel_stats(x):
    """(b * c, 4) float64 on the device: sum, sum of squares about the mean, min, max of every channel of ``x`` (b, c, x, y, z)."""
    x = _aug_data(x)
    n, cells = x.shape[0] * x.shape[1], x[0, 0].numel()
    if n > 65535:
        raise RuntimeError("augment: at most 65535 channels in a batch")
    stats = torch.empty((n, 4), dtype=torch.float64, device=x.device)
    call_ws("augment_channel_stats", ("augment_stats_workspace_bytes", n, cells), x, L.ptr(x), L.ptr(stats), WS, _AUG_DTYPES[x.dtype], n, cells,
            L.stream_ptr(x))
    return stats


def augment_pointwise(x, steps, noise=None, stats0=None, stats1=None, flip=None):
    """One streaming pass over ``x`` (b, c, x, y, z): ``steps`` (b * c, k <= DLKA_AUG_OPS_MAX, 6) float64 rows (code, p0 .. p4) applied in turn
    per channel; ``flip`` (b,) int, bit a reverses spatial axis a of the stored result."""
    x = _aug_data(x)
    n = x.shape[0] * x.shape[1]
    steps = np.asarray(steps, dtype=np.float64)
    if steps.ndim != 3 or steps.shape[0] != n or steps.shape[1] > L.DLKA_AUG_OPS_MAX or steps.shape[2] != 6:
        raise RuntimeError(f"augment: steps are ({n}, <= {L.DLKA_AUG_OPS_MAX}, 6), got {steps.shape}")
    table = np.zeros((n, L.DLKA_AUG_OPS_MAX, 6))
    table[:, :steps.shape[1]] = steps
    codes = set(table[:, :, 0].reshape(-1).tolist())
    if not codes <= set(float(c) for c in range(7)):
        raise RuntimeError(f"augment: unknown step codes {sorted(codes)}")
    if float(L.DLKA_AUG_OP_NOISE) in codes:
        if noise is None or noise.shape != x.shape or noise.dtype != x.dtype or noise.device != x.device:
            raise RuntimeError("augment: the noise step takes a field of the data's shape, dtype and device")
        noise = noise.contiguous()
    need0 = codes & {float(L.DLKA_AUG_OP_CONTRAST), float(L.DLKA_AUG_OP_GAMMA), float(L.DLKA_AUG_OP_RETAIN)}
    for s, need in ((stats0, bool(need0)), (stats1, float(L.DLKA_AUG_OP_RETAIN) in codes)):
        if need and (s is None or tuple(s.shape) != (n, 4) or s.dtype != torch.float64 or s.device != x.device or not s.is_contiguous()):
            raise RuntimeError(f"augment: ({n}, 4) float64 channel statistics on the data's device expected")
    f = None
    if flip is not None:
        flip = np.ascontiguousarray(np.asarray(flip, dtype=np.int32).reshape(-1))
        if flip.shape != (x.shape[0],) or flip.min() < 0 or flip.max() > 7:
            raise RuntimeError(f"augment: one flip mask 0..7 per sample ({x.shape[0]})")
        f = torch.from_numpy(flip).to(x.device)
    t = torch.from_numpy(table).to(x.device)
    y = torch.empty_like(x)
    call("augment_pointwise", L.ptr(x), L.ptr(noise), L.ptr(y), _AUG_DTYPES[x.dtype], x.shape[0], x.shape[1], _I3(*x.shape[2:]), L.ptr(t), L.ptr(stats0),
         L.ptr(stats1), L.ptr(f), L.stream_ptr(x))
    return y
