"""Shared cases of tests/test_tiles_emu.py and tests/test_tiles_gpu.py: the three sliding-window tile kernels of csrc/cl_tiles.hip (dlka_tiles_gather, dlka_tiles_blend,
dlka_tiles_finalize) called directly through ops.tiles_gather / tiles_blend / tiles_finalize, at wave and class-bucket edges; plus predict_3d_tiled through the HIP path
with a batch-invariant elementwise net (GPU only).

Every check takes a device string, draws its inputs on the CPU from a seeded torch.Generator and moves them to the device.  The references are plain torch on the CPU,
never the product: F.pad + torch.flip (gather), a per-tile loop in float64 in the order of nnU-Net's _internal_maybe_mirror_and_pred_3D (blend; the same loop in float32
is the second yardstick, as _torch_blend of tests/test_tta.py), score / weight + torch.argmax (finalize).  A case is built once (functools.lru_cache) and never written to.

Which kernel member a case reaches.  All three kernels run one wave of 64 lanes per z-row, TILES_ROWS = 4 rows per workgroup; "passes" is how often the loop
`for (k = threadIdx.x; k < width; k += 64)` runs for a lane of the row, "last" is the number of rows of the last workgroup where it is not 4.

  gather    wide           864 rows, 70 wide: 2 passes (64 + 6); origins inside the volume and in the padding at either end; the z-flip crosses lane 63
            passes         48 rows, 129 wide: 3 passes (64 + 64 + 1)
            small_1.5/inf  320 rows, 6 wide: the volume (1, 2, 3) is smaller than the patch (4, 5, 6) in every axis
            one_row        1 row: last = 1
            rows_27        27 rows: 7 workgroups, last = 3
            table          64 tiles x 8 masks, patch (1, 1, 2): every entry of the by-value origin table, tile 63 included
  blend     k17            KB = 32 (K = 17, one past the KB = 16 bucket); box 5 x 4 x 131: 20 rows, 3 passes (64 + 64 + 3); up to three tiles deep
            k32            KB = 32 at the cap; box 3 x 5 x 70: 15 rows, last = 3; 2 passes
            k5             KB = 8; box 9 x 8 x 11: 72 rows, 1 pass; voxels inside the box that no tile covers (the `loaded` flag)
            k9             KB = 16; box 2 x 2 x 200: 4 rows (two of them uncovered), 4 passes (3 x 64 + 8); tiles shifted by 1 and by 64 along z
            sweep_k1 / k4  KB = 4 at K = 1 and at its upper edge; sweep_k8: KB = 8 at its edge; sweep_k16: KB = 16 at its edge (the k5 geometry)
            offset         KB = 4; bx0, by0, bz0 = 3, 2, 66; box 3 x 5 x 9: 15 rows, last = 3
            twice          KB = 4; the same origin listed twice; box 3 x 3 x 4: 9 rows, last = 1
            table          KB = 4; 64 tiles of patch (1, 1, 2) in a 4 x 4 x 9 map
  finalize  3x5x70         15 rows, last = 3; 2 passes (64 + 6); low pads (1, 2, 3) inside (5, 8, 75)
            1x1x130        1 row, last = 1; 3 passes (64 + 64 + 2); inside (2, 1, 131) at low pads (1, 0, 1)

Tolerances.  gather and finalize are bitwise.  blend with the identity member is bitwise equal to the float32 loop (score and weight): the kernel has FP contraction off
and adds in the loop's order.  The weight map is bitwise equal to the float32 loop for every member (a plain sum of the importance map).  For every member, per element

    |got - ref64| <= 1e-6 (1 + |ref64|)                                                                                                        (BLEND_RTOL)

NaN positions must be the reference's; equal infinities count as equal.  Where the bound comes from: on the cases below the float32 torch loop itself stays within
3.3e-7 of float64 in this measure (a ratio of 0.33, reached by sums over three tiles of logits near 80), and so does the emulator's host build; 1e-6 leaves about
3x for a device expf and division that round differently from the host's.  A wrong flip, tile, class or order is off by 1e-2 or more.  Every check prints its worst ratio (|err| / bound) before it asserts.

Worst ratios measured on the MI355X (largest |err| / bound over all cases of a group; every bitwise assertion held there as well):

  blend identity 0.330 (k32 fp32; the float32 torch loop's own distance from float64)    blend softmax 0.166 (k17 fp32)    blend sigmoid 0.105 (k32 fp32)
  predict_3d_tiled 0.000: all seven variants equal ref_predict_tiled on the device bit for bit; near-tie share of the reference at most 0.0014 (bf16 sigmoid)"""
import functools
import math
import warnings

import pytest
import torch
import torch.nn.functional as F

from deformablelka_amd import _lib, inference, ops

BLEND_RTOL = 1e-6

NONLIN = {"identity": _lib.DLKA_TILES_IDENTITY, "softmax": _lib.DLKA_TILES_SOFTMAX, "sigmoid": _lib.DLKA_TILES_SIGMOID}
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def _sync(dev):
    if dev != "cpu":
        torch.cuda.synchronize()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def bit_equal(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _flip_dims(mask, first):
    """torch.flip dims of a mirror mask (bit 0 = x, 1 = y, 2 = z) on a tensor whose x axis is dim `first`."""
    return tuple(d + first for d in (0, 1, 2) if mask >> d & 1)


def _flip(t, mask, first):
    dims = _flip_dims(mask, first)
    return torch.flip(t, dims) if dims else t


def _distinct_origins(n, hi, seed):
    """n distinct origins (x, y, z) with 0 <= v < hi[d], in a seeded random order."""
    allv = [(a, b, c) for a in range(hi[0]) for b in range(hi[1]) for c in range(hi[2])]
    perm = torch.randperm(len(allv), generator=torch.Generator().manual_seed(seed))[:n]
    return tuple(allv[int(i)] for i in perm)


# ---- 1. gather ------------------------------------------------------------------------------------------------------------------------------------------------------
ALL_MASKS = tuple(range(8))
# id: (C, volume, patch, low pads, high pads, pad value, origins in padded coordinates, masks)
GATHER_CASES = {
    "wide": (3, (5, 6, 70), (2, 3, 70), (1, 2, 3), (2, 1, 4), -2.5,
             ((1, 2, 3), (3, 3, 3), (0, 0, 0), (6, 6, 7), (0, 6, 5), (6, 0, 1)), ALL_MASKS),    # the first two lie inside the volume
    "passes": (1, (2, 2, 150), (1, 2, 129), (0, 0, 0), (0, 0, 0), 0.0, ((0, 0, 0), (1, 0, 21), (0, 0, 10)), ALL_MASKS),
    "small_1.5": (2, (1, 2, 3), (4, 5, 6), None, None, 1.5, ((0, 0, 0),), ALL_MASKS),           # pads: inference._pad_amounts
    "small_inf": (2, (1, 2, 3), (4, 5, 6), None, None, float("inf"), ((0, 0, 0),), ALL_MASKS),
    "one_row": (1, (3, 4, 9), (1, 1, 5), (0, 0, 0), (0, 0, 0), 0.0, ((1, 2, 3),), (4,)),
    "rows_27": (1, (3, 4, 9), (3, 1, 5), (0, 0, 0), (0, 0, 0), 0.0, ((0, 0, 0), (0, 3, 4), (0, 1, 2)), (0, 4, 3)),
    "table": (1, (4, 4, 9), (1, 1, 2), (1, 0, 1), (0, 1, 0), 0.25, _distinct_origins(64, (5, 5, 9), 101), ALL_MASKS),
}


@functools.lru_cache(maxsize=None)
def _gather_case(cid):
    C, vol, patch, lo, hi, pad_value, origins, masks = GATHER_CASES[cid]
    if lo is None:
        pads = inference._pad_amounts(vol, patch)
        lo, hi = tuple(a for a, _ in pads), tuple(b for _, b in pads)
    x = torch.randn((C,) + vol, generator=torch.Generator().manual_seed(1100 + sum(vol) + len(origins)))
    padded = F.pad(x, [lo[2], hi[2], lo[1], hi[1], lo[0], hi[0]], value=pad_value)
    assert all(0 <= o[d] and o[d] + patch[d] <= padded.shape[d + 1] for o in origins for d in range(3)) and len(set(origins)) == len(origins)
    ref = torch.stack([_flip(padded[:, a:a + patch[0], b:b + patch[1], c:c + patch[2]], m, 1) for a, b, c in origins for m in masks])
    return x, lo, ref


def gather(dev, cid):
    """ops.tiles_gather is bitwise torch.flip of the constant-padded slice, b = t * M + m; one launch."""
    C, vol, patch, _, _, pad_value, origins, masks = GATHER_CASES[cid]
    x, lo, ref = _gather_case(cid)
    n0 = ops.tiles_launch_count()
    out = ops.tiles_gather(x.to(dev), list(origins), list(masks), patch, lo, pad_value)
    _sync(dev)
    assert ops.tiles_launch_count() == n0 + 1
    assert out.shape == ref.shape == (len(origins) * len(masks), C) + patch and out.dtype == torch.float32
    out = out.cpu()
    bad = [(b // len(masks), masks[b % len(masks)]) for b in range(out.shape[0]) if not bit_equal(out[b], ref[b])]
    assert not bad, f"gather {cid}: (tile, mask) {bad[:8]} of {len(bad)} differ from torch.flip of the padded slice"


# ---- 2. blend -------------------------------------------------------------------------------------------------------------------------------------------------------
# id: (K, patch, score extent, origins)
BLEND_SHAPES = {
    "k17": (17, (3, 2, 70), (5, 4, 131), ((0, 0, 0), (1, 1, 30), (2, 2, 61), (0, 2, 61), (2, 0, 5))),
    "k32": (32, (2, 3, 65), (3, 5, 70), ((0, 0, 0), (1, 2, 5), (1, 0, 3))),
    "k5": (5, (4, 5, 6), (9, 8, 11), ((0, 0, 0), (2, 1, 3), (5, 3, 5), (2, 0, 0))),
    "k9": (9, (1, 1, 129), (2, 2, 200), ((0, 0, 0), (1, 1, 71), (0, 0, 64), (0, 0, 1))),
    "offset": (3, (2, 3, 5), (7, 8, 80), ((3, 2, 70), (4, 4, 66), (3, 3, 68))),
    "twice": (3, (2, 2, 3), (4, 4, 6), ((1, 1, 1), (1, 1, 1), (0, 0, 0))),
    "table": (2, (1, 1, 2), (4, 4, 9), _distinct_origins(64, (4, 4, 8), 202)),
}
BLEND_SHAPES.update({f"sweep_k{K}": (K,) + BLEND_SHAPES["k5"][1:] for K in (1, 4, 8, 16)})
BLEND_MAIN = ("k17", "k32", "k5", "k9")                      # every nonlin x dtype x mask list x importance map
BLEND_FURTHER = ("offset", "twice", "table")                 # every nonlin x dtype, all eight mirrors, with the importance map
BLEND_SWEEP = tuple(f"sweep_k{K}" for K in (1, 4, 8, 16))    # softmax, fp32, all eight mirrors, with the importance map
MASK_LISTS = {"xyz": tuple(inference.mirror_masks((0, 1, 2))), "none": (0,), "y": tuple(inference.mirror_masks((1,)))}
ALL_VARIANTS = tuple((mk, gs) for mk in MASK_LISTS for gs in (True, False))
assert len(BLEND_SHAPES["table"][3]) == _lib.DLKA_TILES_MAX_T and MASK_LISTS["xyz"] == (0, 4, 2, 6, 1, 5, 3, 7) and MASK_LISTS["y"] == (0, 2)


def _blend_loop(logits, nonlin, scale, gauss, score, weight, origins, masks, patch, dtype):
    """The reference's order in `dtype`: per tile, sum over the mirrors of scale * flip-back(nonlin(logits)); times the importance map; added into score, the map
    into weight (neural_network.py:526-559, :414-415)."""
    M = len(masks)
    f = {"identity": lambda v: v, "softmax": lambda v: torch.softmax(v, 0), "sigmoid": torch.sigmoid}[nonlin]
    g = None if gauss is None else gauss.to(dtype)
    for t, (a, b, c) in enumerate(origins):
        r = torch.zeros((logits.shape[1],) + patch, dtype=dtype)
        for j, m in enumerate(masks):
            r += scale * _flip(f(logits[t * M + j].to(dtype)), m, 1)
        if g is not None:
            r *= g
        sl = (slice(a, a + patch[0]), slice(b, b + patch[1]), slice(c, c + patch[2]))
        score[(slice(None),) + sl] += r
        weight[sl] += g if g is not None else 1.0


@functools.lru_cache(maxsize=None)
def _blend_case(sid, nonlin, dtype, mask_id, use_gauss):
    K, patch, ext, origins = BLEND_SHAPES[sid]
    masks = MASK_LISTS[mask_id]
    T, M, P = len(origins), len(masks), math.prod(patch)
    assert T >= 3
    g = torch.Generator().manual_seed(2000 + 97 * K + 7 * T + M + sum(ext))
    logits = 2 * torch.randn((T * M, K) + patch, generator=g)
    logits[(T - 1) * M:T * M, K - 1] += 80.0                # one (tile, class) block far up: softmax's max subtraction, sigmoid saturated at 1
    logits[0:M, 0] -= 90.0                                  # and one far down: expf(90) overflows to inf in the sigmoid, 1 / (1 + inf) = 0
    flat = logits.view(T * M, K, P)
    flat[M, :, P // 3] = 0.75                               # tile 1, first mirror: all classes equal
    flat[2 * M - 1, K // 2, P // 2] = float("-inf")         # tile 1, last mirror
    flat[2 * M, K - 1, P - 1] = float("nan")                # tile 2, first mirror, the last voxel of the patch
    logits = logits.to(DTYPES[dtype])
    s0, w0 = torch.rand((K,) + ext, generator=g), torch.rand(ext, generator=g)     # not zeros: a lost read shows
    gauss = inference.gaussian_importance_map(patch) if use_gauss else None
    covered = torch.zeros(ext, dtype=torch.bool)
    for a, b, c in origins:
        covered[a:a + patch[0], b:b + patch[1], c:c + patch[2]] = True
    refs = []
    for dt in (torch.float64, torch.float32):
        s, w = s0.clone().to(dt), w0.clone().to(dt)
        _blend_loop(logits, nonlin, 1.0 / M, gauss, s, w, origins, masks, patch, dt)
        refs.append((s, w))
    return logits, gauss, s0, w0, covered, refs[0], refs[1]


def blend_ratio(what, got, ref64):
    """max over the elements of |got - ref64| / (BLEND_RTOL (1 + |ref64|)); NaN exactly where the reference has NaN; equal infinities count as equal.  Printed."""
    got, ref64 = got.detach().double().cpu(), ref64.double().cpu()
    assert got.shape == ref64.shape, (what, tuple(got.shape), tuple(ref64.shape))
    assert torch.equal(torch.isnan(got), torch.isnan(ref64)), \
        f"{what}: NaN at {int(torch.isnan(got).sum())} elements, the reference has {int(torch.isnan(ref64).sum())} (or elsewhere)"
    ok = ~torch.isnan(ref64)
    g, r = got[ok], ref64[ok]
    same = g == r
    ratio = torch.where(same, torch.zeros_like(g), (g - r).abs() / (BLEND_RTOL * (1 + r.abs()))).nan_to_num(nan=float("inf"))
    if ratio.numel() == 0:
        return 0.0
    at = int(ratio.argmax())
    worst = float(ratio[at])
    print(f"[{what}] max |err| / (1e-6 (1 + |ref|)) = {worst:.3f} (got {float(g[at]):.9g}, ref {float(r[at]):.9g})")
    return worst


def _bit_equal_but_nan(a, b):
    """Bitwise equal wherever b is not NaN, NaN exactly where b is."""
    a, b = a.detach().cpu(), b.detach().cpu()
    nan = torch.isnan(b)
    return a.shape == b.shape and torch.equal(torch.isnan(a), nan) and torch.equal(_bits(a)[~nan], _bits(b)[~nan])


def _blend_variant(dev, sid, nonlin, dtype, mask_id, use_gauss):
    K, patch, ext, origins = BLEND_SHAPES[sid]
    masks = MASK_LISTS[mask_id]
    logits, gauss, s0, w0, covered, (s64, w64), (s32, w32) = _blend_case(sid, nonlin, dtype, mask_id, use_gauss)
    what = f"blend {sid} {nonlin} {dtype} masks={mask_id} gauss={use_gauss}"
    runs = []
    for _ in range(2):
        s, w = s0.clone().to(dev), w0.clone().to(dev)
        n0 = ops.tiles_launch_count()
        ops.tiles_blend(logits.to(dev), NONLIN[nonlin], 1.0 / len(masks), None if gauss is None else gauss.to(dev), s, w, list(origins), list(masks))
        _sync(dev)
        assert ops.tiles_launch_count() == n0 + 1, what
        runs.append((s.cpu(), w.cpu()))
    (s, w), (s2, w2) = runs
    fails = []
    blend_ratio(what + " score of the float32 torch loop", s32, s64)
    worst = blend_ratio(what + " score", s, s64)
    if not worst <= 1.0:
        fails.append(f"score exceeds 1e-6 (1 + |ref64|) by a factor {worst:.3f}")
    if not blend_ratio(what + " weight", w, w64) <= 1.0:
        fails.append("weight exceeds the bound")
    if not bit_equal(w, w32):
        fails.append("weight is not bitwise the float32 sum of the importance map")
    if nonlin == "identity" and not _bit_equal_but_nan(s, s32):
        fails.append(f"identity: score differs from the float32 loop at {int((_bits(s) != _bits(s32)).sum())} elements")
    if not (bit_equal(s[:, ~covered], s0[:, ~covered]) and bit_equal(w[~covered], w0[~covered])):
        inside = torch.zeros_like(covered)
        lo = [min(o[d] for o in origins) for d in range(3)]
        hi = [max(o[d] for o in origins) + patch[d] for d in range(3)]
        inside[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = True
        ch = ((_bits(s) != _bits(s0)).any(0) | (_bits(w) != _bits(w0))) & ~covered
        fails.append(f"{int(ch.sum())} voxels that no tile covers were written ({int((ch & inside).sum())} of them inside the bounding box)")
    if not (bit_equal(s, s2) and bit_equal(w, w2)):
        fails.append("a second call on fresh copies gives another result")
    assert not fails, what + ": " + "; ".join(fails)
    return worst


def blend(dev, sid, nonlin, dtype, variants=ALL_VARIANTS):
    """ops.tiles_blend on shape `sid` over the (mask list, importance map) variants; every variant is run even when one fails.  Returns the worst ratio."""
    assert int((~_blend_case(sid, nonlin, dtype, *variants[0])[4]).sum()) > 0, "the case has no voxel outside its tiles"
    fails, worst = [], 0.0
    for mask_id, use_gauss in variants:
        try:
            worst = max(worst, _blend_variant(dev, sid, nonlin, dtype, mask_id, use_gauss))
        except AssertionError as e:
            fails.append(str(e))
    assert not fails, "\n".join(fails)
    print(f"[blend {sid} {nonlin} {dtype}] worst ratio over {len(variants)} variants: {worst:.3f}")
    return worst


def blend_box_has_uncovered_voxels():
    """The premise of the `loaded` cases: k5 and k9 have voxels inside the bounding box that no tile covers; `offset` has a box away from the origin."""
    for sid in ("k5", "k9"):
        K, patch, ext, origins = BLEND_SHAPES[sid]
        covered = _blend_case(sid, "identity", "fp32", "none", False)[4]
        hi = [max(o[d] for o in origins) + patch[d] for d in range(3)]
        assert all(min(o[d] for o in origins) == 0 for d in range(3)) and int((~covered[:hi[0], :hi[1], :hi[2]]).sum()) > 0, sid
    assert [min(o[d] for o in BLEND_SHAPES["offset"][3]) for d in range(3)] == [3, 2, 66]


# ---- 3. finalize ----------------------------------------------------------------------------------------------------------------------------------------------------
# id: (score extent, low pads, kept region, kept voxels that get: NaN in class 0, NaN in the last class, +inf, -inf, all classes equal)
FINALIZE_SHAPES = {
    "3x5x70": ((5, 8, 75), (1, 2, 3), (3, 5, 70), ((0, 0, 5), (1, 2, 64), (2, 4, 69), (1, 1, 10), (2, 0, 65))),
    "1x1x130": ((2, 1, 131), (1, 0, 1), (1, 1, 130), ((0, 0, 3), (0, 0, 64), (0, 0, 129), (0, 0, 70), (0, 0, 128))),
}
FINALIZE_K = (1, 4, 32)


@functools.lru_cache(maxsize=None)
def _finalize_case(sid, K):
    ext, lo, shape, vox = FINALIZE_SHAPES[sid]
    g = torch.Generator().manual_seed(3000 + K + sum(ext))
    score = torch.randint(0, 3, (K,) + ext, generator=g).float()          # few distinct values: many ties, the first maximum must win
    at = [tuple(v[d] + lo[d] for d in range(3)) for v in vox]
    score[(0,) + at[0]] = float("nan")
    score[(K - 1,) + at[1]] = float("nan")
    score[(K // 2,) + at[2]] = float("inf")
    score[(K // 2,) + at[3]] = float("-inf")
    score[(slice(None),) + at[4]] = 1.0
    weight = torch.rand(ext, generator=g) + 0.5
    keep = tuple(slice(a, a + n) for a, n in zip(lo, shape))
    ref = (score / weight)[(slice(None),) + keep]
    return score, weight, ref, ref.argmax(0)


def finalize(dev, sid, K):
    """ops.tiles_finalize: probs bitwise score / weight of the kept region (NaN where the reference has NaN), seg = torch.argmax (first maximum, NaN wins); one launch."""
    ext, lo, shape, _ = FINALIZE_SHAPES[sid]
    score, weight, ref, rseg = _finalize_case(sid, K)
    n0 = ops.tiles_launch_count()
    seg, probs = ops.tiles_finalize(score.to(dev), weight.to(dev), lo, shape)
    _sync(dev)
    assert ops.tiles_launch_count() == n0 + 1
    seg, probs = seg.cpu(), probs.cpu()
    assert probs.shape == (K,) + shape and probs.dtype == torch.float32 and seg.shape == shape and seg.dtype == torch.int64
    assert int(torch.isnan(ref).sum()) == 2 and int(torch.isinf(ref).sum()) == 2
    assert torch.equal(torch.isnan(probs), torch.isnan(ref))
    assert bit_equal(probs.nan_to_num(-1.0), ref.nan_to_num(-1.0)), \
        f"finalize {sid} K={K}: {int((_bits(probs.nan_to_num(-1.0)) != _bits(ref.nan_to_num(-1.0))).sum())} elements are not score / weight"
    assert torch.equal(seg, rseg), f"finalize {sid} K={K}: {int((seg != rseg).sum())} labels differ from torch.argmax"
    if K == 1:
        assert int(seg.abs().max()) == 0


# ---- 4. refusals leave memory alone ------------------------------------------------------------------------------------------------------------------------------------
REFUSALS = ("K_33", "tile_outside", "tiles_65")


def blend_refusal(dev, which):
    """A refused ops.tiles_blend raises, counts no launch and leaves score and weight bitwise as they were."""
    g = torch.Generator().manual_seed(4000)
    K, patch, ext, origins, msg = {
        "K_33": (_lib.DLKA_TILES_K_MAX + 1, (2, 2, 2), (2, 2, 2), [(0, 0, 0)], "unsupported"),
        "tile_outside": (3, (2, 2, 2), (3, 2, 2), [(0, 0, 0), (2, 0, 0)], "invalid shape"),          # the second tile ends at x = 4 > 3
        "tiles_65": (2, (1, 1, 2), (4, 4, 9), list(_distinct_origins(_lib.DLKA_TILES_MAX_T + 1, (4, 4, 8), 404)), "unsupported"),
    }[which]
    logits = torch.randn((len(origins), K) + patch, generator=g)
    s0, w0 = torch.rand((K,) + ext, generator=g), torch.rand(ext, generator=g)
    s, w = s0.clone().to(dev), w0.clone().to(dev)
    n0 = ops.tiles_launch_count()
    with pytest.raises(RuntimeError, match=msg):
        ops.tiles_blend(logits.to(dev), _lib.DLKA_TILES_SOFTMAX, 1.0, None, s, w, origins, [0])
    _sync(dev)
    assert ops.tiles_launch_count() == n0, "a refused call counted a launch"
    assert bit_equal(s, s0) and bit_equal(w, w0), "a refused call wrote score or weight"


def launch_counts(dev):
    """A successful gather, blend and finalize each add exactly 1 to tiles_launch_count()."""
    g = torch.Generator().manual_seed(4100)
    patch, ext, origins, masks = (2, 2, 3), (2, 2, 4), [(0, 0, 0), (0, 0, 1)], [0, 7]
    x = torch.randn((2,) + ext, generator=g).to(dev)
    n = ops.tiles_launch_count()
    inp = ops.tiles_gather(x, origins, masks, patch, (0, 0, 0))
    assert ops.tiles_launch_count() == n + 1
    score, weight = torch.zeros((2,) + ext).to(dev), torch.zeros(ext).to(dev)
    ops.tiles_blend(inp, _lib.DLKA_TILES_SIGMOID, 0.5, None, score, weight, origins, masks)
    assert ops.tiles_launch_count() == n + 2
    seg, probs = ops.tiles_finalize(score, weight, (0, 0, 0), ext)
    _sync(dev)
    assert ops.tiles_launch_count() == n + 3
    assert bool(torch.isfinite(probs).all()) and seg.shape == ext       # the two tiles cover every voxel of the map


# ---- 5. GPU only: predict_3d_tiled through the HIP path ---------------------------------------------------------------------------------------------------------------
PREDICT_K, PREDICT_VOLUME, PREDICT_PATCH, PREDICT_PAD_VALUE = 14, (2, 5, 19, 100), (8, 8, 72), 1.5
PREDICT_TILES = 8                                    # steps x: [0], y: [0, 4, 7, 11], z: [0, 28] on the padded (8, 19, 100)
PREDICT_AXES = ((0, 1, 2), (0, 2))
PREDICT_VARIANTS = ("softmax", "softmax_batch3", "sigmoid_callable", "tuple", "bf16_softmax", "bf16_sigmoid", "train_mode")
SEG_GAP, SEG_GAP_SHARE = 4e-6, 0.01


class RampNet(torch.nn.Module):
    """logits[:, k] = a[k] x[:, 0] + b[k] x[:, 1] + ramp[k]: elementwise torch ops only, so an input's prediction does not depend on what else is in the batch;
    ramp[k] is a fixed plane over the patch with its own slope along each axis, so it is symmetric under no flip.  Counts its forwards."""

    def __init__(self, dev, tuple_out=False, out_dtype=None):
        super().__init__()
        g = torch.Generator().manual_seed(5000)
        K, (pd, ph, pw) = PREDICT_K, PREDICT_PATCH
        self.a = torch.randn(K, generator=g).view(1, K, 1, 1, 1).to(dev)
        self.b = torch.randn(K, generator=g).view(1, K, 1, 1, 1).to(dev)
        c = 2 * torch.randn(3, K, generator=g)
        i, j, k = torch.arange(pd).view(pd, 1, 1) / pd, torch.arange(ph).view(1, ph, 1) / ph, torch.arange(pw).view(1, 1, pw) / pw
        self.ramp = (c[0].view(K, 1, 1, 1) * i + c[1].view(K, 1, 1, 1) * j + c[2].view(K, 1, 1, 1) * k)[None].to(dev)
        self.tuple_out, self.out_dtype, self.batches = tuple_out, out_dtype, []
        self.eval()

    def forward(self, x):
        self.batches.append(int(x.shape[0]))
        y = self.a * x[:, 0:1] + self.b * x[:, 1:2] + self.ramp
        if self.out_dtype is not None:
            y = y.to(self.out_dtype)
        return (y, y[:, :, ::2, ::2, ::2]) if self.tuple_out else y


def _sigmoid_nonlin(t):
    return torch.sigmoid(t)


def predict_tiled(dev, variant, mirror_axes):
    """inference.predict_3d_tiled(do_mirroring=True) on a GPU tensor (gather, one forward per chunk, blend; finalize once) against ref_predict_tiled of
    tests/test_tta.py (one B = 1 forward per tile and mirror, torch flips and blending) on the same device.  Returns the worst ratio of the probabilities."""
    from tests.test_tta import ref_predict_tiled
    x = torch.randn(PREDICT_VOLUME, generator=torch.Generator().manual_seed(5100)).to(dev)
    bf16 = variant.startswith("bf16")
    net = RampNet(dev, tuple_out=variant == "tuple", out_dtype=torch.bfloat16 if bf16 else None)
    nonlin = _sigmoid_nonlin if "sigmoid" in variant else inference.softmax_helper
    ref_net = (lambda t: net(t)[0]) if variant == "tuple" else net
    M = len(inference.mirror_masks(mirror_axes))
    # bf16 logits with softmax_helper: as D_LKA_Former.predict_3D(mixed_precision=True) runs them, inside autocast, where torch.softmax of a bf16 tensor is
    # computed and returned in float32 (the in-kernel softmax does the same); outside autocast the torch reference would round its probabilities to bf16.
    auto = torch.autocast("cuda", dtype=torch.bfloat16, enabled=variant == "bf16_softmax")
    kw = dict(tile_batch=3 if variant == "softmax_batch3" else 4, nonlin=nonlin, do_mirroring=True, mirror_axes=mirror_axes, pad_value=PREDICT_PAD_VALUE)
    chunks = [3, 3, 2] if variant == "softmax_batch3" else [4, 4]          # tiles per gather / blend pair
    n0 = ops.tiles_launch_count()
    with torch.no_grad(), auto:
        if variant == "train_mode":
            net.train()
            with pytest.warns(UserWarning, match="Network is in train mode during inference"):
                seg, probs = inference.predict_3d_tiled(net, x, PREDICT_PATCH, 0.5, True, **kw)
            assert net.batches == [1] * (PREDICT_TILES * M), "train mode: one forward per input"
        else:
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                seg, probs = inference.predict_3d_tiled(net, x, PREDICT_PATCH, 0.5, True, **kw)
            assert not [w for w in caught if "train mode" in str(w.message)]
            assert net.batches == [t * M for t in chunks], "one forward per chunk of tiles x mirrors"
        torch.cuda.synchronize()
        assert ops.tiles_launch_count() == n0 + 2 * len(chunks) + 1      # gather + blend per chunk, one finalize
        rseg, rprobs = ref_predict_tiled(ref_net, nonlin, x, PREDICT_PATCH, 0.5, mirror_axes, True, PREDICT_K, PREDICT_PAD_VALUE)
    what = f"predict_3d_tiled {variant} axes={mirror_axes}"
    assert probs.shape == (PREDICT_K,) + PREDICT_VOLUME[1:] and probs.dtype == torch.float32 and seg.dtype == torch.int64
    top2 = torch.topk(rprobs, 2, dim=0).values
    clear = (top2[0] - top2[1]) > SEG_GAP
    share = 1.0 - float(clear.float().mean())
    print(f"[{what}] share of voxels whose two largest reference probabilities are within {SEG_GAP:g}: {share:.5f}")
    assert share <= SEG_GAP_SHARE, f"{what}: {share:.4f} of the reference's voxels are near-ties"
    worst = blend_ratio(what + " probs", probs, rprobs)
    assert worst <= 1.0, f"{what}: probs exceed 1e-6 (1 + |ref|) by a factor {worst:.3f}"
    assert torch.equal(seg, probs.argmax(0)), f"{what}: seg is not the argmax of the product's own probabilities"
    assert torch.equal(seg[clear], rseg[clear]), f"{what}: {int((seg[clear] != rseg[clear]).sum())} clear voxels carry another label than the reference"
    return worst
