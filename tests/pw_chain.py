"""Shared body of tests/test_pw_chain_emu.py and tests/test_pw_chain_gpu.py: the workgroup-tiled pointwise chain (cl_pointwise_chain_kernel, C = 64 / 128 / 256:
conv1 + gate -> proj_2 + shortcut and their data gradients in one launch each) against the separate launches (DLKA_PW_UNFUSED=1)."""
import os

import torch

from tests.parity import rel_err


def _align256(n):
    return (n + 255) & ~255


def saved_f_g1_m(saved, B, C, dims, dtype):
    """f (deformable conv output), g1 (conv1 output) and m (gate output) inside the opaque `saved` buffer of a token-layout forward call: f and g1 follow
    the predicted offsets (dlka_lka3d_tokens_saved_offsets_v), m is the last tensor of the buffer (capi_lka3d_tokens.hip, tokens_forward_impl)."""
    import ctypes
    from deformablelka_amd import _lib
    D, H, W = dims
    lib = _lib.get_lib()
    dt = _lib.DLKA_F32 if dtype == torch.float32 else _lib.DLKA_BF16
    o = ctypes.c_size_t(0)
    assert lib.dlka_lka3d_tokens_saved_offsets_v(B, C, D, H, W, dt, 0, ctypes.byref(o)) == 0
    N = D * H * W
    eb = B * N * C * (4 if dtype == torch.float32 else 2)
    f0 = int(o.value) + _align256(B * 81 * N * 4)
    g0 = f0 + _align256(eb)
    m0 = lib.dlka_lka3d_tokens_saved_bytes_v(B, C, D, H, W, dt, 0) - _align256(eb)
    return tuple(saved[s:s + eb].view(dtype).view(B, N, C).float().cpu().clone() for s in (f0, g0, m0))


def check_chain(dev, B, C, dims, dtype, bitwise, blocks_run=1, seed=0):
    """One D-LKA block forward + backward, fused and with DLKA_PW_UNFUSED=1.  bitwise: torch.equal on y, x.grad (not with bitwise = "forward") and the saved g1 / m / f; else the bounds of
    tests/parity.py::check_lka3d_tokens_pointwise_pair.  The launch counter must move by 2 per block (forward + backward) in the fused run only, and the
    depthwise pair counter must move alike in both."""
    import deformablelka_amd as dk
    from deformablelka_amd import _lib, ops
    from oracle import blocks
    torch.manual_seed(seed)
    H, W, D = dims
    m = dk.LKA_Attention3d_deform(C)
    blocks.randomize_offsets_(m, std=0.2)
    m = m.to(dev)
    x = torch.randn(B, H * W * D, C).to(dev).to(dtype)
    gy = torch.randn(B, H * W * D, C).to(dev).to(dtype)
    lib = _lib.get_lib()

    def run():
        for q in m.parameters():
            q.grad = None
        c0, d0 = lib.dlka_pw_chain_launch_count(), lib.dlka_dwpair_launch_count()
        xd = x.clone().requires_grad_(True)
        y = m(xd, B, C, H, W, D)
        y.backward(gy)
        grads = {"x": xd.grad.float().cpu(), **{k: q.grad.detach().float().cpu().clone() for k, q in m.named_parameters()}}
        counts = (lib.dlka_pw_chain_launch_count() - c0, lib.dlka_dwpair_launch_count() - d0)
        _, saved = ops.lka3d_attention_tokens_forward(x, [p.detach() for p in m.block_params()], (H, W, D))
        return y.detach().float().cpu(), grads, saved_f_g1_m(saved, B, C, (H, W, D), dtype), counts

    old = os.environ.get("DLKA_PW_UNFUSED")
    old256 = os.environ.get("DLKA_PW_CHAIN_256")
    try:
        os.environ["DLKA_PW_CHAIN_256"] = "1"   # C = 256 is off by default (it measured slower than its two launches): the kernel is checked all the same
        os.environ.pop("DLKA_PW_UNFUSED", None)
        y_f, g_f, s_f, n_f = run()
        os.environ["DLKA_PW_UNFUSED"] = "1"
        y_u, g_u, s_u, n_u = run()
    finally:
        if old256 is None:
            os.environ.pop("DLKA_PW_CHAIN_256", None)
        else:
            os.environ["DLKA_PW_CHAIN_256"] = old256
        if old is None:
            os.environ.pop("DLKA_PW_UNFUSED", None)
        else:
            os.environ["DLKA_PW_UNFUSED"] = old
    assert n_f[0] == 2 * blocks_run, n_f          # one chain launch forward, one backward
    assert n_u[0] == 0, n_u
    assert n_f[1] == n_u[1], (n_f, n_u)           # the depthwise pair is not touched by the switch
    bf = dtype != torch.float32
    if bitwise:
        assert torch.equal(y_f, y_u), f"y differs in {int((y_f != y_u).sum())} elements (max {float((y_f - y_u).abs().max()):.3e})"
        for name, a, b in zip(("f", "g1", "m"), s_f, s_u):
            assert torch.equal(a, b), f"saved {name} differs in {int((a != b).sum())} elements"
        if bitwise != "forward":   # ("forward": a GPU run, where grad_input of the deformable conv collects its halo in fp32 atomics)
            assert torch.equal(g_f["x"], g_u["x"]), f"x.grad differs in {int((g_f['x'] != g_u['x']).sum())} elements"
    else:
        assert rel_err(y_f, y_u) < (1e-2 if bf else 1e-6), rel_err(y_f, y_u)
        for name, a, b in zip(("f", "g1", "m"), s_f, s_u):
            assert rel_err(a, b) < (1e-2 if bf else 1e-6), (name, rel_err(a, b))
    for name in g_f:
        assert rel_err(g_f[name], g_u[name]) < (2e-2 if bf else 1e-5), (name, rel_err(g_f[name], g_u[name]))
