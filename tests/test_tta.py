"""Sliding-window prediction with test-time mirroring on the CPU: the torch path of ``inference.predict_3d_tiled(do_mirroring=True)`` against a
restatement of nnU-Net's loops (3D/d_lka_former/network_architecture/neural_network.py:292-428 with :502-560), the three tile kernels
(csrc/cl_tiles.hip) on the wavefront emulator against torch, and the contract of ``D_LKA_Former.predict_3D`` (:73-166)."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))


# ---- the reference, restated --------------------------------------------------------------------------------------------------------------
def _ref_maybe_mirror_and_pred_3d(net, nonlin, x, mirror_axes, do_mirroring, mult, num_classes):
    """_internal_maybe_mirror_and_pred_3D (:502-560), written out."""
    result = torch.zeros([1, num_classes] + list(x.shape[2:]), dtype=torch.float, device=x.device)
    mirror_idx, num_results = (8, 2 ** len(mirror_axes)) if do_mirroring else (1, 1)
    for m in range(mirror_idx):
        if m == 0:
            result += 1 / num_results * nonlin(net(x))
        if m == 1 and (2 in mirror_axes):
            result += 1 / num_results * torch.flip(nonlin(net(torch.flip(x, (4,)))), (4,))
        if m == 2 and (1 in mirror_axes):
            result += 1 / num_results * torch.flip(nonlin(net(torch.flip(x, (3,)))), (3,))
        if m == 3 and (2 in mirror_axes) and (1 in mirror_axes):
            result += 1 / num_results * torch.flip(nonlin(net(torch.flip(x, (4, 3)))), (4, 3))
        if m == 4 and (0 in mirror_axes):
            result += 1 / num_results * torch.flip(nonlin(net(torch.flip(x, (2,)))), (2,))
        if m == 5 and (0 in mirror_axes) and (2 in mirror_axes):
            result += 1 / num_results * torch.flip(nonlin(net(torch.flip(x, (4, 2)))), (4, 2))
        if m == 6 and (0 in mirror_axes) and (1 in mirror_axes):
            result += 1 / num_results * torch.flip(nonlin(net(torch.flip(x, (3, 2)))), (3, 2))
        if m == 7 and (0 in mirror_axes) and (1 in mirror_axes) and (2 in mirror_axes):
            result += 1 / num_results * torch.flip(nonlin(net(torch.flip(x, (4, 3, 2)))), (4, 3, 2))
    if mult is not None:
        result[:, :] *= mult
    return result


def ref_predict_tiled(net, nonlin, x, patch_size, step_size, mirror_axes, use_gaussian, num_classes, pad_value=0.0):
    """_internal_predict_3D_3Dconv_tiled (:292-428), the non-all_in_gpu branch with fp32 accumulation; pad_nd_image(..., 'constant') as
    F.pad (below = d // 2).  x: (c, x, y, z) on any device; returns (seg, probs) on that device."""
    from deformablelka_amd.inference import compute_steps_for_sliding_window, gaussian_importance_map
    pads = [(max(p - n, 0) // 2, max(p - n, 0) - max(p - n, 0) // 2) for n, p in zip(x.shape[1:], patch_size)]
    data = F.pad(x, [v for a, b in reversed(pads) for v in (a, b)], value=pad_value)
    slicer = tuple(slice(a, a + n) for (a, _), n in zip(pads, x.shape[1:]))
    steps = compute_steps_for_sliding_window(patch_size, data.shape[1:], step_size)
    num_tiles = len(steps[0]) * len(steps[1]) * len(steps[2])
    if use_gaussian and num_tiles > 1:
        g = gaussian_importance_map(patch_size, device=x.device)
        add = g
    else:
        g, add = None, torch.ones(patch_size, device=x.device)
    agg = torch.zeros([num_classes] + list(data.shape[1:]), device=x.device)
    nb = torch.zeros([num_classes] + list(data.shape[1:]), device=x.device)
    for lx in steps[0]:
        for ly in steps[1]:
            for lz in steps[2]:
                sl = (slice(lx, lx + patch_size[0]), slice(ly, ly + patch_size[1]), slice(lz, lz + patch_size[2]))
                patch = data[(None, slice(None)) + sl]
                agg[(slice(None),) + sl] += _ref_maybe_mirror_and_pred_3d(net, nonlin, patch, mirror_axes, True, g, num_classes)[0]
                nb[(slice(None),) + sl] += add
    probs = agg[(slice(None),) + slicer] / nb[(slice(None),) + slicer]
    return probs.argmax(0), probs


def _conv_net(seed=0):
    torch.manual_seed(seed)
    net = torch.nn.Conv3d(1, 3, 3, padding=1)   # not flip-equivariant: a wrong flip shows
    with torch.no_grad():
        net.weight.normal_(0, 0.5)
    return net.eval()


AXES_SUBSETS = [s for r in range(4) for s in itertools.combinations((0, 1, 2), r)]


@pytest.mark.parametrize("mirror_axes", AXES_SUBSETS, ids=lambda a: "axes" + "".join(map(str, a)))
@pytest.mark.parametrize("use_gaussian", [True, False])
def test_torch_mirrored_path_matches_the_reference(mirror_axes, use_gaussian):
    from deformablelka_amd import inference as inf
    net = _conv_net()
    x = torch.randn(1, 13, 11, 9, generator=torch.Generator().manual_seed(1))
    sm = inf.softmax_helper
    with torch.no_grad():
        for vol, patch, pad_value in ((x, (6, 8, 6), 0.0), (x[:, :4], (6, 8, 6), 0.0), (x[:, :4], (6, 8, 6), 1.5)):   # smaller than the patch along x
            rseg, rprobs = ref_predict_tiled(net, sm, vol, patch, 0.5, mirror_axes, use_gaussian, 3, pad_value)
            seg, probs = inf.predict_3d_tiled(net, vol, patch, 0.5, use_gaussian, tile_batch=3, nonlin=sm, do_mirroring=True,
                                              mirror_axes=mirror_axes, pad_value=pad_value)
            assert probs.shape == rprobs.shape and seg.dtype == torch.int64
            assert (probs - rprobs).abs().max().item() <= 1e-5
            assert torch.equal(seg, rseg)


def test_mirror_masks_follow_the_reference_order():
    from deformablelka_amd.inference import mirror_masks
    assert mirror_masks((0, 1, 2)) == [0, 4, 2, 6, 1, 5, 3, 7]   # m = 0..7: {}, z, y, zy, x, zx, yx, zyx (bit 1 = x, 2 = y, 4 = z)
    assert mirror_masks((0, 2)) == [0, 4, 1, 5]
    assert mirror_masks(()) == [0]


def test_default_predict_3d_tiled_is_unchanged():
    """do_mirroring=False (the default) keeps the existing path."""
    from deformablelka_amd import inference as inf
    net = _conv_net()
    x = torch.randn(1, 13, 11, 9, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        seg, probs = inf.predict_3d_tiled(net, x, (6, 8, 6), 0.5, True, tile_batch=3)
        rseg, rprobs = ref_predict_tiled(net, inf.softmax_helper, x, (6, 8, 6), 0.5, (), True, 3)
    assert (probs - rprobs).abs().max().item() <= 1e-5 and torch.equal(seg, rseg)


# ---- the kernels on the emulator ------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def emu_backend():
    from deformablelka_amd import _lib
    from tests import emu
    _lib._set_backend_for_tests(emu.load())
    yield
    _lib._set_backend_for_tests(None)


def _flip_dims(mask):
    return tuple(d + 1 for d in (0, 1, 2) if mask >> d & 1)   # on a (c, x, y, z) tile


def test_gather_is_flip_of_the_padded_slice(emu_backend):
    from deformablelka_amd import ops
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 5, 6, 7, generator=g)
    patch, lo, hi = (4, 5, 4), (2, 1, 3), (3, 4, 2)
    padded = F.pad(x, [lo[2], hi[2], lo[1], hi[1], lo[0], hi[0]], value=-2.5)
    origins = [(0, 0, 0), (6, 6, 8), (2, 3, 1), (6, 1, 5)]   # the first two reach into the padding at both ends
    masks = list(range(8))
    out = ops.tiles_gather(x, origins, masks, patch, lo, -2.5)
    assert out.shape == (len(origins) * 8, 2) + patch
    for t, (a, b, c) in enumerate(origins):
        tile = padded[:, a:a + patch[0], b:b + patch[1], c:c + patch[2]]
        for m in masks:
            dims = _flip_dims(m)
            assert torch.equal(out[t * 8 + m], torch.flip(tile, dims) if dims else tile), (t, m)


def _torch_blend(logits, nonlin, scale, gauss, score, weight, origins, masks, patch):
    M = len(masks)
    f = {0: lambda v: v, 1: lambda v: torch.softmax(v, 0), 2: torch.sigmoid}[nonlin]
    for t, (a, b, c) in enumerate(origins):
        r = torch.zeros((logits.shape[1],) + patch)
        for j, m in enumerate(masks):
            dims = _flip_dims(m)
            p = f(logits[t * M + j].float())
            r += scale * (torch.flip(p, dims) if dims else p)
        if gauss is not None:
            r *= gauss
        sl = (slice(a, a + patch[0]), slice(b, b + patch[1]), slice(c, c + patch[2]))
        score[(slice(None),) + sl] += r
        weight[sl] += gauss if gauss is not None else 1.0


@pytest.mark.parametrize("K", [1, 3, 14])
@pytest.mark.parametrize("nonlin", [0, 1, 2], ids=["identity", "softmax", "sigmoid"])
def test_blend_matches_torch(K, nonlin, emu_backend):
    from deformablelka_amd import inference, ops
    g = torch.Generator().manual_seed(10 + K + nonlin)
    patch, ext = (4, 5, 6), (9, 8, 11)
    origins = [(0, 0, 0), (2, 1, 3), (5, 3, 5), (2, 0, 0)]   # overlapping tiles of one chunk
    masks = inference.mirror_masks((0, 1, 2))
    gauss = inference.gaussian_importance_map(patch)
    for dtype, gw in ((torch.float32, gauss), (torch.bfloat16, gauss), (torch.float32, None)):
        logits = (2 * torch.randn((len(origins) * 8, K) + patch, generator=g)).to(dtype)
        s0 = torch.rand((K,) + ext, generator=g)
        w0 = torch.rand(ext, generator=g)
        rs, rw = s0.clone(), w0.clone()
        _torch_blend(logits, nonlin, 1 / 8, gw, rs, rw, origins, masks, patch)
        runs = []
        for _ in range(2):
            s, w = s0.clone(), w0.clone()
            ops.tiles_blend(logits, nonlin, 1 / 8, gw, s, w, origins, masks)
            runs.append((s, w))
        assert (runs[0][0] - rs).abs().max().item() <= 1e-6 and (runs[0][1] - rw).abs().max().item() <= 1e-6, dtype
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_finalize_matches_torch_argmax_on_ties(emu_backend):
    from deformablelka_amd import ops
    K, ext, lo, shape = 4, (5, 6, 7), (1, 2, 0), (3, 4, 7)
    score = torch.randint(0, 3, (K,) + ext, generator=torch.Generator().manual_seed(4)).float()   # few distinct values: many ties
    score[2, 1, 2, 3] = float("nan")
    score[:, 2, 3, 4] = 1.0                                                                      # all equal
    weight = torch.rand(ext) + 0.5
    seg, probs = ops.tiles_finalize(score, weight, lo, shape)
    ref = (score / weight)[:, lo[0]:lo[0] + shape[0], lo[1]:lo[1] + shape[1], lo[2]:lo[2] + shape[2]]
    assert torch.equal(probs.nan_to_num(-1), ref.nan_to_num(-1))
    assert torch.equal(seg, ref.argmax(0))


def test_blend_rejects_too_many_classes_without_launching(emu_backend):
    from deformablelka_amd import _lib, ops
    K = _lib.DLKA_TILES_K_MAX + 1
    patch = (2, 2, 2)
    logits = torch.zeros((1, K) + patch)
    score, weight = torch.zeros((K,) + patch), torch.zeros(patch)
    n0 = ops.tiles_launch_count()
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.tiles_blend(logits, 1, 1.0, None, score, weight, [(0, 0, 0)], [0])
    assert ops.tiles_launch_count() == n0


# ---- D_LKA_Former.predict_3D ------------------------------------------------------------------------------------------------------------------
def _lite_net(k=3):
    import deformablelka_amd as dk
    from make_golden_nets import LiteBlock
    torch.manual_seed(5)
    net = dk.D_LKA_Former(in_channels=1, out_channels=k, img_size=[16, 32, 32], feature_size=4, hidden_size=64, num_heads=4, depths=[1, 1, 1, 1],
                          dims=[8, 16, 32, 64], do_ds=True, trans_block=LiteBlock)
    net.inference_apply_nonlin = dk.inference.softmax_helper
    return net.eval()


def test_predict_3d_contract_numpy_in_numpy_out():
    net = _lite_net()
    x = np.random.RandomState(0).randn(1, 20, 30, 40).astype(np.float32)
    seg, probs = net.predict_3D(x, True, mirror_axes=(0, 2), use_sliding_window=True, patch_size=(16, 32, 32), use_gaussian=True, verbose=False,
                                mixed_precision=False)
    assert isinstance(seg, np.ndarray) and isinstance(probs, np.ndarray)
    assert seg.shape == (20, 30, 40) and seg.dtype == np.int64 and probs.shape == (3, 20, 30, 40) and probs.dtype == np.float32
    assert np.abs(probs.sum(0) - 1).max() < 1e-5 and np.array_equal(seg, probs.argmax(0))
    with torch.no_grad():   # the restated reference, first deep-supervision head
        rseg, rprobs = ref_predict_tiled(lambda t: net(t)[0], net.inference_apply_nonlin, torch.from_numpy(x), (16, 32, 32), 0.5, (0, 2), True, 3)
    assert np.abs(probs - rprobs.numpy()).max() <= 1e-5 and np.array_equal(seg, rseg.numpy())


def test_predict_3d_reference_errors():
    import deformablelka_amd as dk
    net = _lite_net()
    x = np.zeros((1, 16, 32, 32), np.float32)
    with pytest.raises(ValueError, match="mirror axes. duh"):
        net.predict_3D(x, True, mirror_axes=(0, 3), verbose=False)
    with pytest.raises(AssertionError):
        net.predict_3D(x, True, step_size=1.5, use_sliding_window=True, patch_size=(16, 32, 32), verbose=False)
    with pytest.raises(AssertionError):
        net.predict_3D(x[0], True, verbose=False)
    with pytest.raises(NotImplementedError):
        net.predict_3D(x, True, pad_border_mode="reflect", verbose=False)
    with pytest.raises(ValueError):   # 20 > img_size 16 along x: not one patch after padding
        net.predict_3D(np.zeros((1, 20, 32, 32), np.float32), True, use_sliding_window=False, verbose=False)
    t = torch.randn(2, 3)
    assert torch.equal(dk.D_LKA_Former.inference_apply_nonlin(t), t)   # SegmentationNetwork's default: identity


def test_predict_3d_regions_class_order():
    net = _lite_net()
    x = np.random.RandomState(1).randn(1, 16, 32, 36).astype(np.float32)
    kw = dict(use_sliding_window=True, patch_size=(16, 32, 32), use_gaussian=True, verbose=False, mixed_precision=False)
    seg, probs = net.predict_3D(x, True, mirror_axes=(1,), regions_class_order=(1, 2, 5), **kw)
    ref = np.zeros(probs.shape[1:], dtype=np.float32)
    for i, c in enumerate((1, 2, 5)):
        ref[probs[i] > 0.5] = c
    assert seg.dtype == np.float32 and np.array_equal(seg, ref) and (seg > 0).any()


def test_predict_3d_without_sliding_window_equals_one_tile():
    net = _lite_net()
    x = np.random.RandomState(2).randn(1, 16, 30, 32).astype(np.float32)   # padded to img_size along y
    kw = dict(verbose=False, mixed_precision=False)
    seg0, probs0 = net.predict_3D(x, True, use_sliding_window=False, **kw)
    seg1, probs1 = net.predict_3D(x, True, use_sliding_window=True, patch_size=(16, 32, 32), use_gaussian=True, **kw)
    assert probs0.shape == (3, 16, 30, 32)
    assert np.array_equal(probs0, probs1) and np.array_equal(seg0, seg1)
