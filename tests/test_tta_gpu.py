"""Sliding-window prediction with test-time mirroring on the MI355X: the HIP tile kernels (csrc/cl_tiles.hip) against the torch restatement of
nnU-Net's loops on the same device, and ``D_LKA_Former.predict_3D`` with the real network."""
import numpy as np
import pytest
import torch

from tests.test_tta import ref_predict_tiled

DEV = "cuda:0"


@pytest.mark.gpu
def test_hip_mirrored_path_matches_the_torch_path_on_the_device():
    from deformablelka_amd import inference, ops
    torch.manual_seed(0)
    net = torch.nn.Conv3d(1, 3, 3, padding=1).to(DEV).eval()
    with torch.no_grad():
        net.weight.normal_(0, 0.5)
    x = torch.randn(1, 37, 30, 45, device=DEV)
    for axes, gauss in (((0, 1, 2), True), ((1,), False), ((0, 2), True)):
        n0 = ops.tiles_launch_count()
        seg, probs = inference.predict_3d_tiled(net, x, (16, 24, 32), 0.5, gauss, tile_batch=3, nonlin=inference.softmax_helper,
                                                do_mirroring=True, mirror_axes=axes)
        torch.cuda.synchronize()
        assert ops.tiles_launch_count() > n0
        inference._MIRROR_IMPL = "torch"
        try:
            rseg, rprobs = inference.predict_3d_tiled(net, x, (16, 24, 32), 0.5, gauss, tile_batch=3, nonlin=inference.softmax_helper,
                                                      do_mirroring=True, mirror_axes=axes)
        finally:
            inference._MIRROR_IMPL = None
        assert (probs - rprobs).abs().max().item() <= 1e-6, axes
        assert torch.equal(seg, rseg)
        seg2, probs2 = inference.predict_3d_tiled(net, x, (16, 24, 32), 0.5, gauss, tile_batch=3, nonlin=inference.softmax_helper,
                                                  do_mirroring=True, mirror_axes=axes)
        assert torch.equal(probs, probs2) and torch.equal(seg, seg2)   # no atomics: bitwise reproducible


def _pancreas_net():
    from deformablelka_amd import training
    torch.manual_seed(0)
    return training.initialize_network(1, 2, (96, 96, 96), device=DEV, patch_size=(2, 2, 2)).eval()


@pytest.mark.gpu
def test_predict_3d_with_the_real_network_matches_the_reference_restatement():
    """Pancreas configuration of test_sliding_window_with_the_real_network (96^3 tiles, stem (2,2,2), 2 classes, 112x100x96): the HIP path
    (two tiles x eight mirrors per forward) against the reference's own grouping (one B = 1 forward per mirror, torch flips and blending)."""
    from deformablelka_amd import inference
    net = _pancreas_net()
    vol = torch.randn(1, 112, 100, 96, generator=torch.Generator().manual_seed(1)).numpy()
    kw = dict(use_sliding_window=True, patch_size=(96, 96, 96), use_gaussian=True, mixed_precision=False, verbose=False)
    seg, probs = net.predict_3D(vol, True, **kw)
    seg2, probs2 = net.predict_3D(vol, True, **kw)
    # Not bitwise: the stem's GroupNorm (network.GroupNorm, one group over 32 x 48^3 values per sample) takes its long-row path, whose moments
    # (dlka_batchnorm_planar_forward, csrc/planar_ops.hip) are summed with float atomics; the tile kernels themselves are bitwise reproducible
    # (test_hip_mirrored_path_matches_the_torch_path_on_the_device).
    assert np.abs(probs - probs2).max() <= 1e-6
    with torch.no_grad():
        rseg, rprobs = ref_predict_tiled(lambda t: net(t)[0], inference.softmax_helper, torch.from_numpy(vol).to(DEV), (96, 96, 96), 0.5,
                                         (0, 1, 2), True, 2)
    rprobs, rseg = rprobs.cpu().numpy(), rseg.cpu().numpy()
    assert probs.shape == (2, 112, 100, 96) and seg.shape == (112, 100, 96)
    assert np.abs(probs - rprobs).max() <= 1e-4
    top2 = np.sort(rprobs, 0)
    clear = (top2[-1] - top2[-2]) > 1e-3
    assert np.array_equal(seg[clear], rseg[clear])


@pytest.mark.gpu
def test_predict_3d_mixed_precision():
    net = _pancreas_net()
    vol = torch.randn(1, 112, 100, 96, generator=torch.Generator().manual_seed(2)).numpy()
    kw = dict(use_sliding_window=True, patch_size=(96, 96, 96), use_gaussian=True, verbose=False)
    _, p32 = net.predict_3D(vol, True, mixed_precision=False, **kw)
    seg, p16 = net.predict_3D(vol, True, mixed_precision=True, **kw)
    assert np.isfinite(p16).all() and np.abs(p16.sum(0) - 1).max() <= 1e-4
    assert np.abs(p16 - p32).max() <= 2e-2
    assert seg.shape == vol.shape[1:]
