"""Shared parity checks: the HIP path (through the C-ABI, via deformablelka_amd.ops) against the CPU oracle.
Used by tests/test_parity_emu.py (host-compiled kernels on the wavefront emulator, tiny shapes, CPU-only
container) and by tests/test_parity_gpu.py (-m gpu, real MI355X, reference-sized shapes)."""
import os

import torch
import torch.nn.functional as F

import oracle
from deformablelka_amd import ops

# tolerances (BASELINE.json north_star / SURVEY §8c): fwd fp32 <= 1e-4 abs vs oracle; bwd <= 1e-3 rel
FWD_ATOL = 1e-4
BWD_RTOL = 1e-3


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-6)).item()


def _refresh_switches():
    """The library reads its A/B switches once (dlka_env_refresh re-reads): call after every change of DLKA_WGRAD_PAD / DLKA_DWPAIR / DLKA_PREP_TILED / the fork switches."""
    from deformablelka_amd import _lib
    _lib.get_lib().dlka_env_refresh()


def kernels_launched(fn):
    """fn() under the launch trace (include/dlka.h dlka_trace_*; GPU only) -> the demangled names of the kernels the library launched, without the dlka:: prefix"""
    from ctypes import create_string_buffer
    from deformablelka_amd import _lib as L
    lib = L.get_lib()
    L.check(lib.dlka_trace_start(4096, torch.cuda.current_stream().cuda_stream), "trace_start")
    try:
        fn()
    finally:
        rc = lib.dlka_trace_stop()
    L.check(rc, "trace_stop")
    buf, names = create_string_buffer(512), set()
    for i in range(lib.dlka_trace_count()):
        L.check(lib.dlka_trace_get(i, buf, 512, None), "trace_get")
        names.add(buf.value.decode().replace("void dlka::", "").replace("dlka::", "").split("(")[0])
    return names


def assert_close(name, got, ref, atol=None, rtol=None):
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    if atol is not None:
        err = (got - ref).abs().max().item()
        assert err <= atol, f"{name}: max abs err {err:.3e} > {atol}"
    if rtol is not None:
        err = rel_err(got, ref)
        assert err <= rtol, f"{name}: max rel err {err:.3e} > {rtol}"


def make_deform3d(B, C, Cout, dims, k, s, p, d, g, dg, off_mode="normal", seed=0, scale=1.0, x_log2=0, go_log2=0):
    """x_log2 / go_log2: x and grad_out times 2^x_log2 / 2^go_log2 (exact: the same random numbers at another scale)."""
    gen = torch.Generator().manual_seed(seed)
    k3 = (k,) * 3 if isinstance(k, int) else tuple(k)
    s3 = (s,) * 3 if isinstance(s, int) else tuple(s)
    p3 = (p,) * 3 if isinstance(p, int) else tuple(p)
    d3 = (d,) * 3 if isinstance(d, int) else tuple(d)
    D, H, W = dims
    o = lambda i, kk, ss, pp, dd: (i + 2 * pp - (dd * (kk - 1) + 1)) // ss + 1
    Do, Ho, Wo = (o(D, k3[0], s3[0], p3[0], d3[0]), o(H, k3[1], s3[1], p3[1], d3[1]), o(W, k3[2], s3[2], p3[2], d3[2]))
    K = k3[0] * k3[1] * k3[2]
    x = torch.randn(B, C, D, H, W, generator=gen)
    w = torch.randn(Cout, C // g, *k3, generator=gen) * (1.0 / (C // g * K) ** 0.5)
    b = torch.randn(Cout, generator=gen)
    shp = (B, dg * 3 * K, Do, Ho, Wo)
    if off_mode == "zero":
        off = torch.zeros(shp)
    elif off_mode == "uniform3":       # U(-3,3)
        off = (torch.rand(shp, generator=gen) * 6 - 3)
    elif off_mode == "wild":           # N(0,4^2): many out-of-bounds samples
        off = torch.randn(shp, generator=gen) * 4
    elif off_mode == "integer":        # exact integers incl. -1 and size
        off = torch.randint(-2, 3, shp, generator=gen).float()
    else:
        off = torch.randn(shp, generator=gen) * scale
    go = torch.randn(B, Cout, Do, Ho, Wo, generator=torch.Generator().manual_seed(seed + 1))
    x, go = x * 2.0 ** x_log2, go * 2.0 ** go_log2
    return x, off, w, b, go, (k3, s3, p3, d3)


def check_deform3d(dev, B, C, Cout, dims, k, s, p, d, g, dg, off_mode="normal", seed=0, check_bwd=True, check_index=True):
    x, off, w, b, go, (k3, s3, p3, d3) = make_deform3d(B, C, Cout, dims, k, s, p, d, g, dg, off_mode, seed)
    ref = oracle.deform_conv3d_forward(x, w, b, off, s3, p3, d3, g, dg)
    xd, od, wd, bd, god = (t.to(dev) for t in (x, off, w, b, go))
    out = ops.deform_conv3d_forward(xd, wd, bd, od, k3, s3, p3, d3, g, dg, 64)
    assert_close("deform3d fwd", out, ref, atol=FWD_ATOL)
    if check_index:
        ridx, rmask = oracle.deform_conv3d_sample_index(off, dims, k3, s3, p3, d3, dg)
        # sample_cell3 on its own (= what the fixed-point grad_input kernel calls); setup_tap (general kernels); gather_describe3 (channels-last
        # gathers); lane_tap (grad_input window kernels) — every site of the rule in the library.  A cell is reported only inside the guard.
        want = ridx * rmask[..., None].to(ridx.dtype)
        for path in (0, 1, 2, 3):
            idx, mask = ops.deform_conv3d_sample_index(od, dims, k3, s3, p3, d3, dg, path=path)
            assert torch.equal(mask.cpu(), rmask), f"guard mask not bit-exact (path {path})"
            assert torch.equal(idx.cpu(), want), f"floor indices not bit-exact (path {path})"
    if check_bwd:
        rgi, rgo, rgw, rgb = oracle.deform_conv3d_backward(x, w, b, off, go, s3, p3, d3, g, dg, q1_literal=False)
        gi, goff, gw, gb = ops.deform_conv3d_backward(xd, wd, bd, od, god, k3, s3, p3, d3, g, dg, 64)
        # integer-valued coordinates sit on the kink of the interpolant: the one-sided derivative is what both
        # the reference and we compute, so it still has to match.
        assert_close("deform3d grad_input", gi, rgi, rtol=BWD_RTOL)
        assert_close("deform3d grad_offset", goff, rgo, rtol=BWD_RTOL)
        assert_close("deform3d grad_weight", gw, rgw, rtol=BWD_RTOL)
        assert_close("deform3d grad_bias", gb, rgb, rtol=BWD_RTOL)


def make_deform2d(B, C, Cout, H, W, k, s, p, d, g, og, off_mode="normal", seed=0):
    gen = torch.Generator().manual_seed(seed)
    kh, kw = k
    o = lambda i, kk: (i + 2 * p - (d * (kk - 1) + 1)) // s + 1
    Ho, Wo = o(H, kh), o(W, kw)
    x = torch.randn(B, C, H, W, generator=gen)
    w = torch.randn(Cout, C // g, kh, kw, generator=gen) * (1.0 / (C // g * kh * kw) ** 0.5)
    shp = (B, og * 2 * kh * kw, Ho, Wo)
    if off_mode == "zero":
        off = torch.zeros(shp)
    elif off_mode == "integer":
        off = torch.randint(-2, 3, shp, generator=gen).float()
    elif off_mode == "wild":
        off = torch.randn(shp, generator=gen) * 4
    else:
        off = torch.randn(shp, generator=gen) * 1.5
    go = torch.randn(B, Cout, Ho, Wo, generator=torch.Generator().manual_seed(seed + 1))
    return x, off, w, go


def embed_offsets_2d_in_3d(off, K, og):
    """torchvision offsets [B, og*2K, Ho, Wo] ((dy, dx) per tap) -> D3D offsets [B, og*3K, 1, Ho, Wo] ((dd = 0, dh = dy, dw = dx) per tap)."""
    B, _, Ho, Wo = off.shape
    o2 = off.reshape(B, og, K, 2, Ho, Wo)
    o3 = torch.zeros(B, og, K, 3, 1, Ho, Wo, dtype=off.dtype)
    o3[:, :, :, 1, 0] = o2[:, :, :, 0]
    o3[:, :, :, 2, 0] = o2[:, :, :, 1]
    return o3.reshape(B, og * 3 * K, 1, Ho, Wo)


def expected_index_2d(off, H, W, k, s, p, d, og):
    """(idx [B,og,K,Ho,Wo,2], mask [B,og,K,Ho,Wo]) the 2-D index entry must produce BIT FOR BIT: floor cell and guard from the oracle's D3D
    index routine on the D = 1 embedding (deform_im2col_cuda.cuh:244-259 with qd = 0 exactly), `reach` (q >= -1 && q < size: the domain of
    torchvision's unguarded coordinate weight) formed here in fp32 exactly as the rule forms q: float(int base) + offset."""
    kh, kw = k
    K = kh * kw
    B, _, Ho, Wo = off.shape
    ridx, rmask = oracle.deform_conv3d_sample_index(embed_offsets_2d_in_3d(off, K, og), (1, H, W), (1, kh, kw), (1, s, s), (0, p, p), (1, d, d), og)
    ridx, rmask = ridx[:, :, :, 0], rmask[:, :, :, 0]          # [B,og,K,Ho,Wo,(3)]
    o2 = off.reshape(B, og, K, 2, Ho, Wo).float()
    tj = (torch.arange(K) // kw).view(1, 1, K, 1, 1)
    tk = (torch.arange(K) % kw).view(1, 1, K, 1, 1)
    by = (torch.arange(Ho).view(1, 1, 1, Ho, 1) * s - p + tj * d).to(torch.float32)
    bx = (torch.arange(Wo).view(1, 1, 1, 1, Wo) * s - p + tk * d).to(torch.float32)
    qy, qx = by + o2[:, :, :, 0], bx + o2[:, :, :, 1]
    reach = (qy >= -1) & (qx >= -1) & (qy < H) & (qx < W)
    assert bool((rmask.bool() & ~reach).sum() == 0)
    cell = torch.stack([torch.floor(qy), torch.floor(qx)], -1).to(torch.int32) * reach[..., None].to(torch.int32)
    inside = rmask.bool()
    assert torch.equal(cell[inside], ridx[..., 1:3][inside])    # the fp32 floor formed here == the oracle's, wherever the oracle forms one
    return cell, rmask | (reach.to(torch.uint8) << 1)


def check_index2d(dev, off, H, W, k, s, p, d, og, paths=(0, 1, 2)):
    want_idx, want_mask = expected_index_2d(off, H, W, k, s, p, d, og)
    for path in paths:   # sample_cell2 on its own (= the window scatter of cl_ddw2d.hip); setup_tap<2> (general kernels); describe2 (cl_ddw2d.hip)
        idx, mask = ops.deform_conv2d_sample_index(off.to(dev), (H, W), k, s, p, d, og, path=path)
        assert torch.equal(mask.cpu(), want_mask), f"2-D guard / reach mask not bit-exact (path {path})"
        assert torch.equal(idx.cpu(), want_idx), f"2-D floor cell not bit-exact (path {path})"


def check_deform2d(dev, B, C, Cout, H, W, k, s, p, d, g, og, off_mode="normal", seed=0, with_bias=False):
    x, off, w, go = make_deform2d(B, C, Cout, H, W, k, s, p, d, g, og, off_mode, seed)
    check_index2d(dev, off, H, W, k, s, p, d, og)
    bias = torch.randn(Cout, generator=torch.Generator().manual_seed(5)) if with_bias else None
    ref = oracle.deform_conv2d_forward(x, off, w, bias, s, p, d)
    xd, od, wd, god = (t.to(dev) for t in (x, off, w, go))
    bd = None if bias is None else bias.to(dev)
    out = ops.deform_conv2d_forward(xd, od, wd, bd, s, p, d)
    assert_close("deform2d fwd", out, ref, atol=FWD_ATOL)
    rgi, rgo, rgw, rgb = oracle.deform_conv2d_backward(x, off, w, go, s, p, d, with_bias=with_bias)
    gi, goff, gw, gb = ops.deform_conv2d_backward(xd, od, wd, god, s, p, d, with_bias=with_bias)
    assert_close("deform2d grad_input", gi, rgi, rtol=BWD_RTOL)
    assert_close("deform2d grad_offset", goff, rgo, rtol=BWD_RTOL)
    assert_close("deform2d grad_weight", gw, rgw, rtol=BWD_RTOL)
    if with_bias:
        assert_close("deform2d grad_bias", gb, rgb, rtol=BWD_RTOL)


def check_conv3d(dev, B, C, Cout, dims, k, s, p, d, g, seed=0, use_aten_ref=True):
    gen = torch.Generator().manual_seed(seed)
    k3 = (k,) * 3 if isinstance(k, int) else tuple(k)
    x = torch.randn(B, C, *dims, generator=gen)
    w = torch.randn(Cout, C // g, *k3, generator=gen) * (1.0 / (C // g * k3[0] * k3[1] * k3[2]) ** 0.5)
    b = torch.randn(Cout, generator=gen)
    if use_aten_ref:   # the reference's own CPU path for these ops is ATen's conv (nn.Conv3d)
        xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
        ref = F.conv3d(xr, wr, br, s, p, d, g)
        go = torch.randn(ref.shape, generator=gen)
        ref.backward(go.double())
        rgi, rgw, rgb = xr.grad, wr.grad, br.grad
        ref = ref.detach()
    else:
        ref = oracle.conv3d_forward(x, w, b, s, p, d, g)
        go = torch.randn(ref.shape, generator=gen)
        rgi, rgw, rgb = oracle.conv3d_backward(x, w, go, s, p, d, g)
    out = ops.conv3d_forward(x.to(dev), w.to(dev), b.to(dev), s, p, d, g)
    assert_close("conv3d fwd", out, ref, atol=FWD_ATOL)
    gi, gw, gb = ops.conv3d_backward(x.to(dev), w.to(dev), go.to(dev), s, p, d, g)
    assert_close("conv3d grad_input", gi, rgi, rtol=BWD_RTOL)
    assert_close("conv3d grad_weight", gw, rgw, rtol=BWD_RTOL)
    assert_close("conv3d grad_bias", gb, rgb, rtol=BWD_RTOL)


# ------------------------------------------------------------------------------------------------------------
# channels-last fast path
# ------------------------------------------------------------------------------------------------------------
def to_cl(t):   # [B,C,D,H,W] -> [B,D,H,W,C]
    return t.permute(0, 2, 3, 4, 1).contiguous()


def from_cl(t):
    return t.permute(0, 4, 1, 2, 3).contiguous()


def check_conv3d_cl(dev, B, C, Cout, dims, k, p, d, g, planar=False, seed=0):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, *dims, generator=gen)
    w = torch.randn(Cout, C // g, k, k, k, generator=gen) * (1.0 / (C // g * k ** 3) ** 0.5)
    b = torch.randn(Cout, generator=gen)
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    ref = F.conv3d(xr, wr, br, 1, p, d, g)
    go = torch.randn(ref.shape, generator=gen)
    ref.backward(go.double())
    out = ops.conv3d_forward_cl(to_cl(x).to(dev), w.to(dev), b.to(dev), p, d, g, out_planar=planar)
    assert_close("conv3d_cl fwd", out if planar else from_cl(out), ref.detach(), atol=FWD_ATOL)
    gi, gw, gb = ops.conv3d_backward_cl(to_cl(x).to(dev), w.to(dev), (go if planar else to_cl(go)).to(dev), p, d, g, grad_out_planar=planar)
    assert_close("conv3d_cl grad_input", from_cl(gi), xr.grad, rtol=BWD_RTOL)
    assert_close("conv3d_cl grad_weight", gw, wr.grad, rtol=BWD_RTOL)
    assert_close("conv3d_cl grad_bias", gb, br.grad, rtol=BWD_RTOL)


def check_deform3d_cl(dev, B, C, Cout, dims, off_mode="normal", seed=0, dtype=torch.float32, x_log2=0, go_log2=0, go_hook=None):
    """dtype = torch.bfloat16: bf16 storage of x / out / grad_out (everything else fp32) against the oracle on the bf16-rounded activations, at the bf16
    contract (BF16_RTOL of max |reference|, as tests/partial_grad_cases.py holds the same entry points to).
    x_log2 / go_log2: the activations / grad_out at another power-of-two scale (tests/scale_cases.py).  FWD_ATOL is an absolute bound on an output of magnitude ~1;
    with x (and so the output) 2^x_log2 times larger, x_log2 > 0, one fp32 ulp of the output already exceeds it, so the bound scales with the output: FWD_ATOL * 2^x_log2.
    At x_log2 <= 0 it stays FWD_ATOL.  The gradients' bound is relative and unchanged.  go_hook(go) -> go: edits grad_out before both sides see it."""
    x, off, w, b, go, (k3, s3, p3, d3) = make_deform3d(B, C, Cout, dims, 3, 1, 1, 1, 1, 1, off_mode, seed, x_log2=x_log2, go_log2=go_log2)
    if go_hook is not None:
        go = go_hook(go)
    bf = dtype == torch.bfloat16
    if bf:
        x, go = x.bfloat16().float(), go.bfloat16().float()
    fwd_tol, bwd_tol = (dict(rtol=BF16_RTOL), dict(rtol=BF16_RTOL)) if bf else (dict(atol=FWD_ATOL), dict(rtol=BWD_RTOL))
    ref = oracle.deform_conv3d_forward(x, w, b, off, 1, 1, 1, 1, 1)
    out = ops.deform_conv3d_forward_cl(to_cl(x).to(dev).to(dtype), off.to(dev), w.to(dev), b.to(dev), 1, 1)
    if x_log2 > 0 and not bf:
        fwd_tol = dict(atol=FWD_ATOL * 2.0 ** x_log2)
    assert_close("deform3d_cl fwd", from_cl(out), ref, **fwd_tol)
    rgi, rgo, rgw, rgb = oracle.deform_conv3d_backward(x, w, b, off, go, 1, 1, 1, 1, 1, q1_literal=False)
    gi, goff, gw, gb = ops.deform_conv3d_backward_cl(to_cl(x).to(dev).to(dtype), off.to(dev), w.to(dev), to_cl(go).to(dev).to(dtype), 1, 1)
    assert_close("deform3d_cl grad_input", from_cl(gi), rgi, **bwd_tol)
    assert_close("deform3d_cl grad_offset", goff, rgo, **bwd_tol)
    assert_close("deform3d_cl grad_weight", gw, rgw, **bwd_tol)
    assert_close("deform3d_cl grad_bias", gb, rgb, **bwd_tol)


def check_deform3d_cl_gx_worst_case(dev, C, dims, B=1):
    """Adversarial input for the fixed-point grad_input window (cl_deform_gx_kernel<true>): grad_out = +1 everywhere, W = +1 everywhere and
    EVERY (voxel, tap) sample aimed exactly at ONE input voxel (integer position -> corner weight 1), so that the cell of that voxel
    receives, from each brick whose window covers it, R*K contributions of the same sign at the Cauchy-Schwarz maximum |Col| = Cout —
    precisely the case the overflow bound is built for.  (Bricks farther away reach the voxel through the global-atomic path.)"""
    D, H, W = dims
    K = 27
    tgt = (D // 2, H // 2, W // 2)
    x = torch.randn(B, C, D, H, W, generator=torch.Generator().manual_seed(0))
    w = torch.ones(C, C, 3, 3, 3)
    b = torch.zeros(C)
    go = torch.ones(B, C, D, H, W)
    zd, zh, zw = torch.meshgrid(torch.arange(D), torch.arange(H), torch.arange(W), indexing="ij")
    off = torch.zeros(B, K, 3, D, H, W)
    for t in range(K):
        ti, tj, tk = t // 9, (t // 3) % 3, t % 3
        off[:, t, 0] = (tgt[0] - (zd + ti - 1)).float()
        off[:, t, 1] = (tgt[1] - (zh + tj - 1)).float()
        off[:, t, 2] = (tgt[2] - (zw + tk - 1)).float()
    off = off.reshape(B, 3 * K, D, H, W)
    rgi, _, _, _ = oracle.deform_conv3d_backward(x, w, b, off, go, 1, 1, 1, 1, 1, q1_literal=False)
    assert abs(rgi[0, 0, tgt[0], tgt[1], tgt[2]].item() - C * K * D * H * W) < 1e-3 * C * K * D * H * W   # everything lands on the target
    gi, _, _, _ = ops.deform_conv3d_backward_cl(to_cl(x).to(dev), off.to(dev), w.to(dev), to_cl(go).to(dev), 1, 1)
    assert_close("gx worst case", from_cl(gi), rgi, rtol=1e-5)


def check_deform3d_cl_gx_fixed_vs_fp64(dev, B, C, dims, max_rel=4e-4):
    """The fixed-point window against the fp64 window (DLKA_GX_FIXED=0) on the same inputs: its quantisation error, relative to
    max|grad_input|.  The provable headroom (R*K contributions per cell) leaves ~17 bits for the largest possible contribution; measured on
    the MI355X 1.9e-4 (C=32, 32^3) / 2.4e-4 (C=64, 16^3) with a power-of-two scale — bounded here at 4e-4, against the 1e-3 contract."""
    x, off, w, b, go, _ = make_deform3d(B, C, C, dims, 3, 1, 1, 1, 1, 1, "normal", 0)
    args = (to_cl(x).to(dev), off.to(dev), w.to(dev), to_cl(go).to(dev), 1, 1)
    old = os.environ.get("DLKA_GX_FIXED")
    try:
        os.environ["DLKA_GX_FIXED"] = "1"
        g_fx = ops.deform_conv3d_backward_cl(*args)[0].cpu()
        os.environ["DLKA_GX_FIXED"] = "0"
        g_64 = ops.deform_conv3d_backward_cl(*args)[0].cpu()
    finally:
        if old is None:
            os.environ.pop("DLKA_GX_FIXED", None)
        else:
            os.environ["DLKA_GX_FIXED"] = old
    err = rel_err(g_fx, g_64)
    print(f"[gx fixed-point vs fp64 window, C={C} dims={dims}] max rel err {err:.3e}")
    assert 0 < err <= max_rel, err      # > 0: the two variants really are different kernels
    return err


def check_deform3d_cl_gx_fx2_vs_fx1(dev, B, C, dims, off_mode="normal", scale=1.0):
    """Second-generation fixed-point grad_input kernel (compile-time window strides, guard cells, one test per sample) against the first one
    (DLKA_GX_FIXED=2): same scale, integer window sums, roundings that differ by at most one quantum per contribution -> 2e-5 wherever every
    sample stays inside window + guard; a sample beyond the halo is quantised partly (fx1) or not at all (fx2: all its corners take fp32 global atomics) -> 2e-4 there."""
    x, off, w, b, go, _ = make_deform3d(B, C, C, dims, 3, 1, 1, 1, 1, 1, off_mode, 0, scale=scale)
    args = (to_cl(x).to(dev), off.to(dev), w.to(dev), to_cl(go).to(dev), 1, 1)
    old = os.environ.get("DLKA_GX_FIXED")
    try:
        os.environ["DLKA_GX_FIXED"] = "1"
        g2 = ops.deform_conv3d_backward_cl(*args)[0].cpu()
        os.environ["DLKA_GX_FIXED"] = "2"
        g1 = ops.deform_conv3d_backward_cl(*args)[0].cpu()
        os.environ["DLKA_GX_FIXED"] = "0"
        g64 = ops.deform_conv3d_backward_cl(*args)[0].cpu()
    finally:
        if old is None:
            os.environ.pop("DLKA_GX_FIXED", None)
        else:
            os.environ["DLKA_GX_FIXED"] = old
    far = off.abs().max().item() > 2.9
    err = rel_err(g2, g1)
    print(f"[gx fx2 vs fx1 C={C} dims={dims} {off_mode} x{scale}] rel err {err:.3e}; fx2 vs fp64 window {rel_err(g2, g64):.3e}")
    if far:   # a sample beyond the halo: fx1 quantises its in-window corners, fx2 sends all of them through exact fp32 atomics
        assert err < 2e-4, err
    else:   # same scale; fx2 rounds the exact product once, fx1 the fp32 product: a few quanta (1 / 155 343 of the largest contribution) at most
        assert err < 2e-5, err
    assert rel_err(g2, g64) < 4e-4


def check_lka3d_tokens(dev, B, C, dims, seed=0, offset_std=0.02, atol=FWD_ATOL, rtol=BWD_RTOL, report_offsets=False, acdc=False, volume=False, prepare=None,
                       grads_out=None):
    """Token-layout fused block vs the oracle block (oracle/blocks.py) at the CONTRACT's tolerances: forward 1e-4 abs (north_star), every
    gradient 1e-3 rel.

    grad_offset is discontinuous where a sampling coordinate crosses an integer, and the two implementations sum the offset-predict conv in a
    different order: a sample whose coordinate lands within fp32 rounding of a cell boundary can take the neighbouring cell in one of them.  So
    the comparison is made twice:
      (1) the oracle on ITS OWN offsets: every tensor at the contract's tolerance except the gradients that collect grad_offset (conv_offset.*
          directly; conv_spatial / conv0 / proj_1 and grad_x through grad_t), which get `flip_rtol` — and the flipped samples are COUNTED;
      (2) the oracle fed the kernels' offset VALUES (straight-through, `offsets_override`): both sides sample the same cells and EVERY gradient
          must be inside 1e-3.  (2) passing is the demonstration that (1)'s residual is the flips and nothing else.
    volume=True: the same comparison through ``forward_volume`` — the NCDHW entry point ``dlka_lka3d_attention_forward/backward`` (general
    per-op kernels) instead of the token-layout fused call."""
    import deformablelka_amd as dk
    from deformablelka_amd import ops
    from oracle import blocks
    torch.manual_seed(seed)
    H, W, D = dims
    N = H * W * D
    if acdc:   # the ACDC variant's depthwise pair (acdc/transformerblock.py:213-237)
        from deformablelka_amd import acdc as _acdc
        m = _acdc.LKA_Attention3d_deform(C)
    else:
        m = dk.LKA_Attention3d_deform(C)
    variant = m.variant
    blocks.randomize_offsets_(m, std=offset_std)
    if prepare is not None:   # (tests/scale_cases.py: rescales parameters; the oracle sees the module's state_dict AFTER it)
        prepare(m)
    x = torch.randn(B, C, H, W, D) if volume else torch.randn(B, N, C)
    gy = torch.randn_like(x)
    m0 = {k: v.detach().clone() for k, v in m.state_dict().items()}

    def oracle_fn(xr, P, override, used):
        if volume:
            return blocks.lka3d_attention_volume(xr, P, offsets_override=override, offsets_out=used)
        return blocks.lka3d_attention_tokens(xr, P, B, C, H, W, D, offsets_override=override, offsets_out=used)

    m = m.to(dev)
    xd = x.to(dev).requires_grad_(True)
    # the kernels' predicted offsets come from the `saved` buffer of THE forward call whose gradients are checked (a second, identical call can
    # differ in the last bit where the offset conv is tap-split over fp32 atomics — enough to move a boundary sample into the other cell and to make
    # the flip count and the same-cells comparison describe a different run: seen on the ACDC 20x28x28 stage, round 3)
    captured = {}
    fwd_name = "lka3d_attention_forward" if volume else "lka3d_attention_tokens_forward"
    orig_fwd = getattr(ops, fwd_name)

    def spy(*a, **k):
        out = orig_fwd(*a, **k)
        captured["saved"] = out[1]
        return out

    setattr(ops, fwd_name, spy)
    try:
        y = m.forward_volume(xd) if volume else m(xd, B, C, H, W, D)
    finally:
        setattr(ops, fwd_name, orig_fwd)
    y.backward(gy.to(dev))
    if volume:
        assert "saved" in captured, "forward_volume did not go through the fused NCDHW entry point"
    if "saved" not in captured:   # (a path that does not go through the fused token call: general per-op composition)
        _, captured["saved"] = ops.lka3d_attention_tokens_forward(x.detach().to(dev), [p_.detach() for p_ in m.block_params()], dims, variant)
    off_hip = ops.lka3d_tokens_saved_offsets(captured["saved"], B, C, dims).cpu().clone()
    grads = {k: p.grad for k, p in m.named_parameters()}
    if grads_out is not None:
        grads_out.update({k: g.detach().float().cpu().clone() for k, g in grads.items()})
    return compare_lka3d_with_oracle(f"tokens C={C} dims={dims}", oracle_fn, x, gy, m0, dims, y, xd.grad, grads, off_hip, atol=atol, rtol=rtol,
                                     report=report_offsets)


def compare_lka3d_with_oracle(tag, oracle_fn, x, gy, params, dims, y, gx, grads, off_hip, atol=FWD_ATOL, rtol=BWD_RTOL, report=False):
    """The flips-counted + same-cells protocol (docstring of check_lka3d_tokens) for ANY run of the 3-D block: oracle_fn(x, P, offsets_override, offsets_out) -> y is the
    oracle block on CPU tensors, params its state_dict-keyed parameters; y / gx / grads (dict by the same keys) / off_hip are what the run under test produced (any device)."""
    def run_oracle(override=None):
        P = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
        xr = x.detach().cpu().clone().requires_grad_(True)   # (detach: on the CPU backend `x.to(dev)` IS x, and requires_grad_ marks it)
        used = []
        yr = oracle_fn(xr, P, override, used)
        yr.backward(gy.detach().cpu())
        run_oracle.offsets = used[0]
        return yr.detach(), xr.grad, {k: v.grad for k, v in P.items()}

    yr, gxr, gr = run_oracle()
    off_ref = run_oracle.offsets   # the offsets THIS oracle run sampled with
    off_hip = off_hip.detach().cpu()
    k3 = ((3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1))
    i_h, m_h = oracle.deform_conv3d_sample_index(off_hip, dims, *k3)
    i_r, m_r = oracle.deform_conv3d_sample_index(off_ref, dims, *k3)
    flipped = int(((i_h != i_r).any(-1) | (m_h != m_r)).sum())
    y2, gx2, g2 = run_oracle(off_hip)
    if report or os.environ.get("DLKA_PARITY_VERBOSE"):
        print(f"[{tag}] y abs {(y.detach().cpu() - yr).abs().max().item():.3e} gx rel {rel_err(gx, gxr):.3e}; "
              f"offsets max |hip - oracle| {(off_hip - off_ref).abs().max().item():.2e}, cell-flipped samples {flipped} of {m_r.numel()}")
        for k, g in grads.items():
            if gr[k] is not None and gr[k].abs().max() > 0:
                print(f"    {k:55s} own offsets {rel_err(g, gr[k]):.3e}   same cells {rel_err(g, g2[k]):.3e}")
    # Both caps BEFORE the flip-dependent bound is derived from the count: the predicted offsets themselves agree to fp32 rounding of a 27 C-term sum, and
    # only a handful of samples may sit close enough to a cell boundary for that to move them (the same cap the mixed-bf16 check uses).
    off_err = (off_hip - off_ref).abs().max().item()
    assert off_err <= 1e-4, f"{tag}: predicted offsets max |hip - oracle| {off_err:.3e} > 1e-4"
    assert flipped <= max(3, int(2e-5 * m_r.numel())), f"{tag}: {flipped} of {m_r.numel()} sampling cells differ from the oracle's (cap max(3, 2e-5 n))"
    # own offsets with flips: a flipped sample's grad_offset is O(1) off, and the gradients that collect grad_offset sum ~sqrt(samples) such terms: 8e-3 covers the real
    # volumes; a SMALL volume needs the 1 / sqrt(samples) term (fuzz, B = 1, 8^3: ONE flipped sample of 13 824 put conv_offset.weight.grad at 1.16e-2,
    # profiles/r08_notes.md).  The comparison on identical cells below stays at the contract's 1e-3 regardless.
    # (per flipped sample: the engine's decoder block with N(0, 1) grad_y and TWO flips measured 8.9e-3 on conv_offset.weight.grad; the count is capped above.)
    flip_rtol = rtol if flipped == 0 else min(5e-2, max(8 * rtol * flipped, 3.0 * (flipped / m_r.numel()) ** 0.5))
    exposed = ("conv_offset", "conv_spatial.", "conv0.", "proj_1.")
    assert_close(tag + " y", y, yr, atol=atol)
    assert_close(tag + " gx", gx, gxr, rtol=flip_rtol)
    assert_close(tag + " y (same cells)", y, y2, atol=atol)
    assert_close(tag + " gx (same cells)", gx, gx2, rtol=rtol)
    for k, g_hip in grads.items():
        g = gr[k]
        if g is not None and g.abs().max() > 0:
            assert_close(f"{tag} grad " + k, g_hip, g, rtol=flip_rtol if any(e in k for e in exposed) else rtol)
            assert_close(f"{tag} grad (same cells) " + k, g_hip, g2[k], rtol=rtol)
    return flipped


STACK_PARAM_NAMES = ("proj_1.weight", "proj_1.bias", "spatial_gating_unit.conv0.weight", "spatial_gating_unit.conv0.bias", "spatial_gating_unit.conv_spatial.weight",
                     "spatial_gating_unit.conv_spatial.bias", "spatial_gating_unit.deform_conv.conv_offset.weight", "spatial_gating_unit.deform_conv.conv_offset.bias",
                     "spatial_gating_unit.deform_conv.weight", "spatial_gating_unit.deform_conv.bias", "spatial_gating_unit.conv1.weight", "spatial_gating_unit.conv1.bias",
                     "proj_2.weight", "proj_2.bias")   # dlka_lka3d_params order (include/dlka.h) = LKA_Attention3d_deform.block_params()


def check_stack_step(st, entry_blocks, oracle_blocks, sync=None):
    """The state a `DLKABlockStack` step left behind (every block's x / y / grad_y / grad_x / saved / gradients are resident) against
      (1) the per-block entry points (`dlka_lka3d_attention_tokens_forward/backward`: one stream, private scratch, in-call weight preparation and folds) run now on the
          same x / grad_y, for `entry_blocks`: y, the predicted offsets, grad_x and all 14 parameter gradients — the backward entry both on the ENGINE's saved
          activations (identical cells: only the order of the few fp32 atomics may differ, 2e-3) and on its own forward pass (cells that differ counted);
      (2) the CPU oracle block with the flips-counted + same-cells protocol (compare_lka3d_with_oracle), for `oracle_blocks`.
    The stack must not have been stepped (parameter update) since the pass."""
    from deformablelka_amd import ops
    from oracle import blocks
    sync = sync or (torch.cuda.synchronize if st.device.type == "cuda" else (lambda: None))
    B = st.B
    k3 = ((3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1))
    exposed = ("conv_offset", "conv_spatial.", "conv0.", "proj_1.")

    def scaled(a, b):
        return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-6))

    report = []
    for bi in entry_blocks:
        blk = st.blocks[bi]
        C, dims = blk.C, blk.dims
        tag = f"block {bi} (C={C}, {dims})"
        x, gy = blk.x.clone(), blk.gy.clone()
        params = [p.clone() for p in blk.params]
        y1, saved1 = ops.lka3d_attention_tokens_forward(x, params, dims, 0)
        e_y = scaled(blk.y, y1)
        off_e = ops.lka3d_tokens_saved_offsets(blk.saved, B, C, dims, st.dtype).cpu()
        off_1 = ops.lka3d_tokens_saved_offsets(saved1, B, C, dims, st.dtype).cpu()
        e_off = float((off_e - off_1).abs().max())
        i_e, m_e = oracle.deform_conv3d_sample_index(off_e, dims, *k3)
        i_1, m_1 = oracle.deform_conv3d_sample_index(off_1, dims, *k3)
        flipped = int(((i_e != i_1).any(-1) | (m_e != m_1)).sum())
        gx_a, g_a = ops.lka3d_attention_tokens_backward(x, params, gy, blk.saved, dims, 0)
        gx_b, g_b = ops.lka3d_attention_tokens_backward(x, params, gy, saved1, dims, 0)
        sync()
        errs_a = {"gx": scaled(blk.gx, gx_a), **{n: scaled(g, ga) for n, g, ga in zip(STACK_PARAM_NAMES, blk.grads, g_a) if float(ga.abs().max()) > 0}}
        errs_b = {"gx": scaled(blk.gx, gx_b), **{n: scaled(g, gb) for n, g, gb in zip(STACK_PARAM_NAMES, blk.grads, g_b) if float(gb.abs().max()) > 0}}
        report.append((tag, e_y, e_off, flipped, max(errs_a.values()), max(errs_b.values())))
        ytol = 2e-5 if st.dtype == torch.float32 else 1.6e-2   # (bf16 storage: one ulp of the largest element where an fp32 sum lands on the other side of a rounding boundary)
        assert e_y <= ytol, f"{tag}: y differs from the per-block entry by {e_y:.3e} of max|y|"
        assert e_off <= 1e-5, f"{tag}: predicted offsets differ from the per-block entry by {e_off:.3e}"
        assert flipped <= 3, f"{tag}: {flipped} sampling cells differ between the engine's and the per-block forward pass"
        gtol = 2e-3 if st.dtype == torch.float32 else 1.6e-2
        for n, e in errs_a.items():
            assert e <= gtol, f"{tag}: {n} differs from the per-block backward entry (engine's saved activations) by {e:.3e}"
        flip_tol = gtol if flipped == 0 else max(8e-3, gtol, 3.0 * (flipped / m_e.numel()) ** 0.5)
        for n, e in errs_b.items():
            lim = flip_tol if (n == "gx" or any(t in n for t in exposed)) else gtol
            assert e <= lim, f"{tag}: {n} differs from the per-block entry (own forward pass, {flipped} cells differ) by {e:.3e} > {lim:.1e}"
    for r in report:
        print("[engine vs per-block entry] %s: y %.1e offsets %.1e cells %d  grads (engine's saved) %.1e (own forward) %.1e" % r)
    for bi in oracle_blocks:
        assert st.dtype == torch.float32
        blk = st.blocks[bi]
        C, dims = blk.C, blk.dims
        H, W, D = dims
        P = {n: p.detach().cpu().clone() for n, p in zip(STACK_PARAM_NAMES, blk.params)}
        grads = {n: g.detach().cpu().clone() for n, g in zip(STACK_PARAM_NAMES, blk.grads)}
        off_e = ops.lka3d_tokens_saved_offsets(blk.saved, B, C, dims).cpu().clone()

        def oracle_fn(xr, Pr, override, used, _s=(B, C, H, W, D)):
            return blocks.lka3d_attention_tokens(xr, Pr, *_s, offsets_override=override, offsets_out=used)

        compare_lka3d_with_oracle(f"engine block {bi} C={C} dims={dims}", oracle_fn, blk.x.float().cpu(), blk.gy.float().cpu(), P, dims,
                                  blk.y.float().cpu(), blk.gx.float().cpu(), grads, off_e, report=True)


def check_forward_reproducible(dev, B, C, dims, dtype=torch.float32, runs=5, offset_std=0.3, expect_kw=None):
    """Round 6 (VERDICT r5 missing #3): the forward pass of the token-layout block is BITWISE reproducible — output y and the predicted sampling offsets equal across
    `runs` identical calls.  The reference's forward is im2col + addmm (deform_conv_cuda.cu:95-123): no atomics.  At the 16^3 / 8^3 / 4^3 stages rounds 1 - 5 split the taps of
    the offset conv and of the deformable conv over the grid and let the partial sums meet in fp32 atomics (the last bit — and with it the cell of a boundary sample — varied from
    run to run); now the offset conv splits its contraction over the waves of a workgroup (cl_conv_kw.hip, summed in wave order) and the deformable conv's tap ranges meet in
    slabs summed in slab order.  expect_kw: True = assert that cl_conv_kw_kernel ran (the shape is below the row-tiling threshold)."""
    import deformablelka_amd as dk
    from deformablelka_amd import _lib, ops
    from oracle import blocks
    torch.manual_seed(11)
    H, W, D = dims
    m = dk.LKA_Attention3d_deform(C)
    blocks.randomize_offsets_(m, std=offset_std)
    m = m.to(dev)
    x = torch.randn(B, H * W * D, C).to(dev).to(dtype)
    params = [p_.detach() for p_ in m.block_params()]
    lib = _lib.get_lib()
    n0 = lib.dlka_conv_kw_launch_count()
    first = None
    for r in range(runs):
        y, saved = ops.lka3d_attention_tokens_forward(x, params, dims, m.variant)
        off = ops.lka3d_tokens_saved_offsets(saved, B, C, dims, dtype).clone()
        if first is None:
            first = (y.clone(), off)
            continue
        assert torch.equal(off, first[1]), f"run {r}: predicted offsets differ in {int((off != first[1]).sum())} elements (max {float((off - first[1]).abs().max()):.3e})"
        assert torch.equal(y, first[0]), f"run {r}: y differs in {int((y != first[0]).sum())} elements"
    if expect_kw is not None:
        assert (lib.dlka_conv_kw_launch_count() - n0 > 0) == expect_kw, (n0, lib.dlka_conv_kw_launch_count())


def check_lka3d_tokens_phased_backward(dev, B, C, dims, dtype=torch.float32, seed=0):
    """ops.lka3d_attention_tokens_backward(side_stream=...): the data chain (phase 1), the weight gradients into block-private partial sums (phase 2) and their fold by
    dlka_wgrad_finalize_run_slot give what the one-call pass gives — the same kernels on the same operands (only the order of a few fp32 atomics may differ)."""
    import deformablelka_amd as dk
    from deformablelka_amd import ops
    from oracle import blocks
    torch.manual_seed(seed)
    H, W, D = dims
    m = dk.LKA_Attention3d_deform(C)
    blocks.randomize_offsets_(m, std=0.3)
    m = m.to(dev)
    x = torch.randn(B, H * W * D, C).to(dev).to(dtype)
    gy = torch.randn(B, H * W * D, C).to(dev).to(dtype)
    params = [p_.detach() for p_ in m.block_params()]
    y, saved = ops.lka3d_attention_tokens_forward(x, params, dims, m.variant)
    gx0, g0 = ops.lka3d_attention_tokens_backward(x, params, gy, saved, dims, m.variant)
    gx1, g1, keep = ops.lka3d_attention_tokens_backward(x, params, gy, saved, dims, m.variant, side_stream="inline")
    tol = 2e-3 if dtype == torch.float32 else 2e-2
    for k, (a_, b_) in enumerate(zip([gx0, *g0], [gx1, *g1])):
        assert torch.isfinite(b_.float()).all(), k
        scale = max(float(a_.float().abs().max()), 1e-6)
        assert float((a_.float() - b_.float()).abs().max()) <= tol * scale, (k, float((a_.float() - b_.float()).abs().max()) / scale)


def check_tblock3d_forward_reproducible(dev, B, C, dims, training=True, runs=4, lka_bf16=False):
    """Round 6: the wrapper block's forward is bitwise reproducible too — also in TRAINING mode, whose BatchNorm batch statistics were fp32 atomic sums until the per-workgroup partial sums
    were folded in fixed order (cl_bn_stats_det_q_kernel): output, both sets of batch statistics and the activation patterns equal across `runs` identical calls."""
    import deformablelka_amd as dk
    from deformablelka_amd import ops
    from oracle import blocks
    torch.manual_seed(13)
    H, W, D = dims
    m = dk.TransformerBlock_3D_single_deform_LKA(H * W * D, C, C, 4, dropout_rate=0.1, pos_embed=True)
    blocks.randomize_offsets_(m, std=0.3)
    with torch.no_grad():
        m.gamma.normal_(0.5, 0.2)
    m = m.to(dev).train(training)
    x = torch.randn(B, H * W * D, C).to(dev)
    tparams = [None if p is None else p.detach() for p in m.wrapper_params()]
    lparams = [p.detach() for p in m.epa_block.block_params()]
    mask = torch.ones(B, C).to(dev)
    first = None
    for r in range(runs):
        stats = torch.zeros(6 * C, dtype=torch.float32).to(dev)
        if not training:
            stats[C:2 * C] = 1.0
            stats[4 * C:5 * C] = 1.0
        y, saved = ops.tblock3d_forward(x, False, tparams, lparams, mask, training, stats, dims, 1e-5, 1e-5, 0, lka_bf16)
        # (`saved` itself has alignment gaps of uninitialised memory: compare what it holds — the predicted offsets and the two LeakyReLU activation patterns)
        cur = (y.clone(), stats.clone(), torch.cat([ops.tblock3d_saved_offsets(saved, B, C, dims, 0, lka_bf16).reshape(-1).clone()] +
                                                   [t.reshape(-1).float() for t in ops.tblock3d_saved_activation_signs(saved, B, C, dims, 0, lka_bf16)]))
        if first is None:
            first = cur
            continue
        assert torch.equal(cur[1], first[1]), f"run {r}: batch statistics differ (max {float((cur[1] - first[1]).abs().max()):.3e})"
        assert torch.equal(cur[0], first[0]), f"run {r}: y differs in {int((cur[0] != first[0]).sum())} elements"
        assert torch.equal(cur[2], first[2]), f"run {r}: predicted offsets / activation patterns differ in {int((cur[2] != first[2]).sum())} elements"


def check_lka3d_tokens_sample_handover(dev, B, C, dims, dtype=torch.float32, seed=0, offset_std=0.3, prepare=None):
    """The deformable conv's weight gradient from the samples the grad_offset kernel stores (default) against the weight-gradient kernel that
    gathers for itself (dlka_lka3d_force_wgrad_gather(1) / DLKA_WGRAD_GATHER=1): same fma chain for every sample, same MFMA order over the rows -> the two agree to summation
    order, and no other gradient notices the switch."""
    import deformablelka_amd as dk
    from oracle import blocks
    torch.manual_seed(seed)
    H, W, D = dims
    m = dk.LKA_Attention3d_deform(C)
    blocks.randomize_offsets_(m, std=offset_std)
    if prepare is not None:
        prepare(m)
    m = m.to(dev)
    x = torch.randn(B, H * W * D, C).to(dev).to(dtype)
    gy = torch.randn(B, H * W * D, C).to(dev).to(dtype)

    def run():
        for q in m.parameters():
            q.grad = None
        xd = x.clone().requires_grad_(True)
        m(xd, B, C, H, W, D).backward(gy)
        return {"x": xd.grad.float().cpu(), **{k: q.grad.detach().float().cpu().clone() for k, q in m.named_parameters()}}

    from deformablelka_amd import _lib
    lib = _lib.get_lib()
    old = lib.dlka_lka3d_force_wgrad_gather(0)
    try:
        g_s = run()
        lib.dlka_lka3d_force_wgrad_gather(1)
        g_g = run()
    finally:
        lib.dlka_lka3d_force_wgrad_gather(old)
    k = "spatial_gating_unit.deform_conv.weight"
    assert g_s[k].abs().max() > 0
    for name in g_s:   # (not bit-equal at block level: upstream tap-split partial sums meet in atomics, so grad_out itself moves by ~1e-7 per run)
        # round 6: the fp32 path hands its samples over as IEEE halves (11 significant bits; grad_out, products and accumulation fp32): the deformable conv's weight gradient
        # agrees with the gathering kernel's to the rounding of the samples — a random-sign sum over M rows keeps its relative error at ~2^-12, 5e-4 of max at the outside
        tol = 2e-2 if dtype != torch.float32 else (5e-4 if name == k else 1e-5)
        assert rel_err(g_s[name], g_g[name]) < tol, (name, rel_err(g_s[name], g_g[name]))
    return g_s


def check_lka3d_tokens_pointwise_pair(dev, B, dims, dtype=torch.float32, seed=0):
    """conv1 + gate -> proj_2 + shortcut (and their data gradients) as one launch (cl_pointwise_pair_kernel, C = 32) against the two separate
    launches (DLKA_PW_UNFUSED=1): same MFMA order, same epilogue arithmetic, same rounding of the stored intermediate -> output and gradients
    agree to the summation order of the atomics elsewhere in the block."""
    import deformablelka_amd as dk
    from oracle import blocks
    torch.manual_seed(seed)
    C = 32
    H, W, D = dims
    m = dk.LKA_Attention3d_deform(C)
    blocks.randomize_offsets_(m, std=0.2)
    m = m.to(dev)
    x = torch.randn(B, H * W * D, C).to(dev).to(dtype)
    gy = torch.randn(B, H * W * D, C).to(dev).to(dtype)

    def run():
        for q in m.parameters():
            q.grad = None
        xd = x.clone().requires_grad_(True)
        y = m(xd, B, C, H, W, D)
        y.backward(gy)
        return y.detach().float().cpu(), {"x": xd.grad.float().cpu(), **{k: q.grad.detach().float().cpu().clone() for k, q in m.named_parameters()}}

    old = os.environ.get("DLKA_PW_UNFUSED")
    try:
        os.environ.pop("DLKA_PW_UNFUSED", None)
        y_f, g_f = run()
        os.environ["DLKA_PW_UNFUSED"] = "1"
        y_u, g_u = run()
    finally:
        if old is None:
            os.environ.pop("DLKA_PW_UNFUSED", None)
        else:
            os.environ["DLKA_PW_UNFUSED"] = old
    # (not torch.equal: at small volumes the deformable conv upstream is tap-split and its partial sums meet in atomics — f itself moves by ~1e-7)
    assert rel_err(y_f, y_u) < (1e-6 if dtype == torch.float32 else 1e-2), rel_err(y_f, y_u)
    for name in g_f:
        assert rel_err(g_f[name], g_u[name]) < (1e-5 if dtype == torch.float32 else 2e-2), (name, rel_err(g_f[name], g_u[name]))


def check_lka2d_attention(dev, B, C, H, W, seed=0, offset_std=0.03, atol=FWD_ATOL, rtol=BWD_RTOL, report=False):
    """deformable_LKA_Attention (2D/deformable_LKA/deformable_LKA.py:124-140) vs the oracle block at the CONTRACT's tolerances (forward 1e-4 abs,
    every gradient 1e-3 rel); widths with C % 32 == 0 take the channels-last fast path (MFMA offset nets + cl_ddw2d.hip), the rest the general
    NCHW kernels.  Same treatment as the 3-D block (check_lka3d_tokens): the comparison is made twice —
      (1) the oracle on ITS OWN offsets, the cell-flipped samples of BOTH deformable convs counted (product side: the kernels' own predicted
          offsets read back from `saved` and run through the product's index entry, dlka_deform_conv2d_sample_index_path; oracle side: the pinned
          rule on the oracle run's offsets); only when flips were counted do the gradients that collect grad_offset get `8 * rtol`;
      (2) the oracle fed the kernels' offset VALUES (straight through): identical cells, EVERY gradient inside `rtol`."""
    import deformablelka_amd as dk
    from deformablelka_amd import ops as _ops
    from oracle import blocks
    torch.manual_seed(seed)
    m = dk.deformable_LKA_Attention(C)
    blocks.randomize_offsets_(m, std=offset_std)
    x = torch.randn(B, C, H, W)
    gy = torch.randn(B, C, H, W)
    m0 = {k: v.detach().clone() for k, v in m.state_dict().items()}

    def run_oracle(override=None):
        P = {k: v.detach().clone().requires_grad_(True) for k, v in m0.items()}
        xr = x.detach().clone().requires_grad_(True)
        used = []
        yr = blocks.lka2d_attention(xr, P, offsets_override=override, offsets_out=used)
        yr.backward(gy)
        run_oracle.offsets = used
        return yr.detach(), xr.grad, {k: v.grad for k, v in P.items()}

    yr, gxr, gr = run_oracle()
    off_ref = run_oracle.offsets
    m = m.to(dev)
    xd = x.to(dev).requires_grad_(True)
    captured = {}
    orig_fwd = _ops.lka2d_attention_forward

    def spy(*a, **k):
        out = orig_fwd(*a, **k)
        captured["saved"] = out[1]
        return out

    _ops.lka2d_attention_forward = spy
    try:
        y = m(xd)
    finally:
        _ops.lka2d_attention_forward = orig_fwd
    y.backward(gy.to(dev))
    assert "saved" in captured, "the 2-D block did not go through dlka_lka2d_attention_forward"
    off_hip = [o.float().cpu().clone() for o in _ops.lka2d_saved_offsets(captured["saved"], xd)]
    flipped, total = 0, 0
    for oh, orf, (k, p, d) in zip(off_hip, off_ref, ((5, 2, 1), (7, 9, 3))):
        i_h, m_h = _ops.deform_conv2d_sample_index(oh.to(dev), (H, W), (k, k), 1, p, d, 1, path=0)
        i_r, m_r = expected_index_2d(orf, H, W, (k, k), 1, p, d, 1)
        flipped += int(((i_h.cpu() != i_r).any(-1) | (m_h.cpu() != m_r)).sum())
        total += m_r.numel()
    y2, gx2, g2 = run_oracle(tuple(off_hip))
    errs = {"y_abs": (y.detach().cpu() - yr).abs().max().item(), "gx": rel_err(xd.grad, gxr)}
    errs2 = {"y_abs": (y.detach().cpu() - y2).abs().max().item(), "gx": rel_err(xd.grad, gx2)}
    for k, p in m.named_parameters():
        if gr[k] is not None and gr[k].abs().max() > 0:
            errs[k] = rel_err(p.grad, gr[k])
            errs2[k] = rel_err(p.grad, g2[k])
    if report or os.environ.get("DLKA_PARITY_VERBOSE"):
        short = lambda k: ".".join(k.split(".")[-2:])
        print(f"[lka2d C={C} {H}x{W} B={B}] cell-flipped samples {flipped} of {total}; offsets max |hip - oracle| "
              f"{max((a - b).abs().max().item() for a, b in zip(off_hip, off_ref)):.2e}")
        print("    own offsets: " + " ".join(f"{short(k)}={v:.1e}" for k, v in errs.items()))
        print("    same cells:  " + " ".join(f"{short(k)}={v:.1e}" for k, v in errs2.items()))
    # One flipped sample changes ITS grad_offset entry by O(|Col|); relative to a gradient's max norm that is 1e-3 .. 1e-2 per flip depending on how
    # many samples the tensor sums (measured on the MI355X at B = 24, (96, 56^2): 9 flips of 5.6 M -> conv_spatial.offset_net.weight 1.3e-2 on the oracle's
    # own offsets, 6e-6 on identical cells).  With flips counted, comparison (1) therefore only keeps a sanity bound for the exposed gradients; the
    # statement of record is comparison (2): identical cells, every gradient inside the contract's 1e-3.
    flip_rtol = rtol if flipped == 0 else max(8 * rtol, 5e-2)
    # what collects grad_offset: the offset nets directly, and everything upstream of either deformable conv's input
    exposed = ("offset_net", "conv0.deform_conv", "proj_1.")
    assert errs["y_abs"] <= atol and errs2["y_abs"] <= atol, (errs["y_abs"], errs2["y_abs"])
    for k, v in errs.items():
        if k == "y_abs":
            continue
        lim = flip_rtol if (k == "gx" or any(e in k for e in exposed)) else rtol
        assert v <= lim, f"lka2d {k}: rel err {v:.3e} > {lim} (flipped samples: {flipped})"
        assert errs2[k] <= rtol, f"lka2d {k} (same cells): rel err {errs2[k]:.3e} > {rtol}"
    errs["flipped"] = flipped
    return errs


def check_lka2d_attention_bf16(dev, B, C, H, W, seed=0, offset_std=0.03, rtol=None, report=False):
    """The 2-D block with bf16 activations (DLKA_BF16: BASELINE.json config 2) against the fp32 oracle block fed the same bf16-rounded input, and
    against the bf16-storage model — every output and gradient within 2e-2.  Holds because the offset-determining chain stays fp32."""
    import deformablelka_amd as dk
    from oracle import blocks
    rtol = BF16_RTOL if rtol is None else rtol
    torch.manual_seed(seed)
    m = dk.deformable_LKA_Attention(C)
    blocks.randomize_offsets_(m, std=offset_std)
    x = torch.randn(B, C, H, W).bfloat16()
    gy = torch.randn(B, C, H, W).bfloat16()
    m0 = {k: v.detach().clone() for k, v in m.state_dict().items()}

    def run_oracle(store):
        P = {k: v.detach().clone().requires_grad_(True) for k, v in m0.items()}
        xr = x.float().requires_grad_(True)
        yr = blocks.lka2d_attention(xr, P, store=store)
        yr.backward(gy.float())
        return yr.detach(), xr.grad, {k: v.grad for k, v in P.items()}

    y32, gx32, g32 = run_oracle(None)
    y16, gx16, g16 = run_oracle(blocks.bf16_storage)
    m = m.to(dev)
    xd = x.to(dev).requires_grad_(True)
    y = m(xd)
    assert y.dtype == torch.bfloat16
    y.backward(gy.to(dev))
    errs = {"y": rel_err(y, y32), "gx": rel_err(xd.grad, gx32)}
    errs16 = {"y": rel_err(y, y16), "gx": rel_err(xd.grad, gx16)}
    for k, p in m.named_parameters():
        assert p.grad.dtype == torch.float32
        if g32[k] is not None and g32[k].abs().max() > 0:
            errs[k] = rel_err(p.grad, g32[k])
            errs16[k] = rel_err(p.grad, g16[k])
    if report or os.environ.get("DLKA_PARITY_VERBOSE"):
        short = lambda k: ".".join(k.split(".")[-3:])
        print(f"[bf16 lka2d C={C} {H}x{W} B={B}] vs fp32 oracle: " + " ".join(f"{short(k)}={v:.1e}" for k, v in errs.items()))
        print(f"[bf16 lka2d C={C} {H}x{W} B={B}] vs bf16-storage oracle: " + " ".join(f"{short(k)}={v:.1e}" for k, v in errs16.items()))
    for k in errs:
        assert errs[k] <= rtol, f"bf16 lka2d {k}: rel err vs fp32 oracle {errs[k]:.3e} > {rtol}"
        assert errs16[k] <= rtol, f"bf16 lka2d {k}: rel err vs bf16-storage oracle {errs16[k]:.3e} > {rtol}"
    return errs


BF16_RTOL = 2e-2   # bf16 path vs the fp32 oracle <= 2e-2 rel (of max |reference|)


def check_lka3d_tokens_bf16(dev, B, C, dims, seed=0, offset_std=0.38, rtol=BF16_RTOL, via_autocast=False, report=False, prepare=None):
    """DLKA_BF16 token path: bf16 activations (x, y, every saved tensor, the intermediate gradients), fp32 parameters / offsets /
    accumulation — against the fp32 oracle block fed the SAME bf16-rounded input.  via_autocast: fp32 tensors inside torch.autocast(bf16)
    (the block's autocast policy) instead of explicit bf16 tensors."""
    import deformablelka_amd as dk
    from oracle import blocks
    torch.manual_seed(seed)
    H, W, D = dims
    N = H * W * D
    m = dk.LKA_Attention3d_deform(C)
    blocks.randomize_offsets_(m, std=offset_std)
    if prepare is not None:
        prepare(m)
    x = torch.randn(B, N, C).bfloat16()
    gy = torch.randn(B, N, C).bfloat16()
    def run_oracle(store):
        P = {k: v.detach().clone().requires_grad_(True) for k, v in m0.items()}
        xr = x.float().requires_grad_(True)
        yr = blocks.lka3d_attention_tokens(xr, P, B, C, H, W, D, store=store)
        yr.backward(gy.float())
        return yr.detach(), xr.grad, {k: v.grad for k, v in P.items()}

    m0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    y32, gx32, g32 = run_oracle(None)                      # the reference's fp32 block
    y16, gx16, g16 = run_oracle(blocks.bf16_storage)       # the same arithmetic with bf16-STORED activations: the model of the DLKA_BF16 path
    m = m.to(dev)
    if via_autocast:
        xd = x.float().to(dev).requires_grad_(True)
        with torch.autocast(torch.device(dev).type, dtype=torch.bfloat16):
            y = m(xd, B, C, H, W, D)
    else:
        xd = x.to(dev).requires_grad_(True)
        y = m(xd, B, C, H, W, D)
    assert y.dtype == torch.bfloat16, y.dtype
    y.backward(gy.to(dev))
    errs = {"y": rel_err(y, y32), "gx": rel_err(xd.grad, gx32)}
    errs16 = {"y": rel_err(y, y16), "gx": rel_err(xd.grad, gx16)}
    for k, p in m.named_parameters():
        assert p.grad.dtype == torch.float32
        if g32[k] is not None and g32[k].abs().max() > 0:
            errs[k] = rel_err(p.grad, g32[k])
            errs16[k] = rel_err(p.grad, g16[k])
    if report or os.environ.get("DLKA_PARITY_VERBOSE"):
        short = lambda k: ".".join(k.split(".")[-2:])
        print(f"[bf16 tokens C={C} dims={dims}] vs fp32 oracle: " + " ".join(f"{short(k)}={v:.1e}" for k, v in errs.items()))
        print(f"[bf16 tokens C={C} dims={dims}] vs bf16-storage oracle: " + " ".join(f"{short(k)}={v:.1e}" for k, v in errs16.items()))
    # the bf16 path within 2e-2 (of max |reference|) of the fp32 oracle — EVERY quantity, no exceptions.  That holds because the
    # DLKA_BF16 block keeps the chain that decides the sampling cells (a -> conv0 -> conv_spatial -> conv_offset) on fp32 tensors: with those
    # stored as bf16 the predicted offsets move by ~0.4 %, samples near an integer coordinate change cell, and conv_offset / conv_spatial / conv0 /
    # proj_1 gradients land 5e-2 .. 1.8e-1 from the fp32 block (round 2 measured exactly that; tests/test_oracle_bf16_model.py reproduces it on the
    # CPU with per-tensor storage flags).  The bf16-storage model (oracle.blocks.bf16_storage) must be matched at least as closely.
    for k in errs:
        assert errs[k] <= rtol, f"bf16 tokens {k}: rel err vs fp32 oracle {errs[k]:.3e} > {rtol}"
        assert errs16[k] <= rtol, f"bf16 tokens {k}: rel err vs bf16-storage oracle {errs16[k]:.3e} > {rtol}"
    return errs


def check_lka3d_volume_bf16(dev, B, C, dims, seed=0, offset_std=0.3, rtol=BF16_RTOL, report=False):
    """The general NCDHW block (dlka_lka3d_attention_forward / _backward) with bf16 TENSORS THROUGHOUT — activations, offsets and parameters — the one
    mode in which its backward pass accumulates grad_input / grad_weight in the fp32 areas of its workspace and casts them back.  y, grad_x and all 14
    parameter gradients against the bf16-storage oracle (oracle.blocks.bf16_storage on every activation, the offset-determining chain included:
    chain_store) on the same bf16-rounded x, grad_y and parameters, fed the kernels' own offset VALUES (read from `saved`): bf16 offsets differ from the
    oracle's by an ulp here and there, which moves samples into other cells — the same-cells protocol of check_lka3d_tokens takes that out.
    Bar: BF16_RTOL of max |reference| for every quantity.  The oracle models the forward pass's roundings; what it leaves out is the backward pass's own
    (at most ten bf16 stores between grad_y and any output, half an ulp = 2^-9 relative each: below 10 * 2^-9 = 2e-2 even if they all pointed one way)."""
    import deformablelka_amd as dk
    from deformablelka_amd import ops
    from oracle import blocks
    torch.manual_seed(seed)
    m = dk.LKA_Attention3d_deform(C)
    blocks.randomize_offsets_(m, std=offset_std)
    P0 = {k: v.detach().bfloat16() for k, v in m.state_dict().items()}
    x, gy = torch.randn(B, C, *dims).bfloat16(), torch.randn(B, C, *dims).bfloat16()
    params = [P0[k].to(dev) for k in STACK_PARAM_NAMES]
    y, saved = ops.lka3d_attention_forward(x.to(dev), params)
    gx, grads = ops.lka3d_attention_backward(x.to(dev), params, gy.to(dev), saved)
    assert y.dtype == gx.dtype == torch.bfloat16 and all(g.dtype == torch.bfloat16 for g in grads)
    # `saved` (csrc/dlka_capi.hip carve_lka3d_saved): h, a, t1, t, off, ... — each area a multiple of 256 bytes
    E, n_off = x.numel(), B * 81 * x[0, 0].numel()
    at = 4 * ((E * 2 + 255) // 256 * 256)
    off_hip = saved[at:at + n_off * 2].view(torch.bfloat16).view(B, 81, *dims).float().cpu()
    P = {k: v.float().requires_grad_(True) for k, v in P0.items()}
    xr = x.float().requires_grad_(True)
    yr = blocks.lka3d_attention_volume(xr, P, store=blocks.bf16_storage, chain_store=blocks.bf16_storage, offsets_override=off_hip)
    yr.backward(gy.float())
    errs = {"y": rel_err(y, yr.detach()), "gx": rel_err(gx, xr.grad)}
    errs.update({k: rel_err(g, P[k].grad) for k, g in zip(STACK_PARAM_NAMES, grads)})
    if report or os.environ.get("DLKA_PARITY_VERBOSE"):
        print(f"[bf16 volume C={C} dims={dims}] vs bf16-storage oracle, same cells: " + " ".join(f"{'.'.join(k.split('.')[-2:])}={v:.1e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= rtol, f"bf16 volume {k}: rel err vs bf16-storage oracle {v:.3e} > {rtol}"
    return errs


# ---- the wrapper block (TransformerBlock_3D_single_deform_LKA) and its pieces ------------------------------------------------
def offset_view(t, elems=1):
    """A contiguous copy of ``t`` that starts ``elems`` elements into a fresh allocation: same values, a data pointer that is NOT 16-byte aligned.  ops.py only calls
    .contiguous(), so such a view reaches the C API with its own pointer and the launchers must fall back from their 16-byte (quad) kernels."""
    buf = torch.empty(t.numel() + elems, dtype=t.dtype, device=t.device)
    v = buf[elems:].view(t.shape)
    v.copy_(t.detach())
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


def _put(t, dev, name, unaligned):
    """``t`` on ``dev``; as an offset_view when ``unaligned`` is "all" or names this operand."""
    if t is None:
        return None
    t = t.to(dev)
    return offset_view(t) if unaligned == "all" or name in unaligned else t


LN_SCALE = 2.0   # std of the LayerNorm test rows
LN_MEAN_ULPS = {20.0: 4.14, 100.0: 4.34, 500.0: 3.96}   # bound of the row mean in fp32 ulps of |mean|: twice torch's own fp32 error (check_layernorm_tokens)


def layernorm_inputs(B, C, N, planar, pos, seed=0, mean_over_std=None):
    """(x, w, b, pos_embed or None, g_xn, g_res) of check_layernorm_tokens."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, N, generator=g) * LN_SCALE if planar else torch.randn(B, N, C, generator=g) * LN_SCALE
    w, b = torch.randn(C, generator=g), torch.randn(C, generator=g)
    pe = torch.randn(1, N, C, generator=g) if pos else None
    gxn, gres = torch.randn(B, N, C, generator=g), torch.randn(B, N, C, generator=g)
    if mean_over_std is None:
        x = x + 0.5
    else:
        sign = (torch.rand(B, N, 1, generator=g) < 0.5).float() * 2 - 1
        off = LN_SCALE * mean_over_std * sign * (0.8 + 0.4 * torch.rand(B, N, 1, generator=g))
        x = x + (off.permute(0, 2, 1) if planar else off)
    return x, w, b, pe, gxn, gres


def check_layernorm_tokens(dev, B, C, N, planar, pos, seed=0, mean_over_std=None, unaligned=()):
    """LayerNorm over tokens (+ pos_embed), forward and backward.  Returns the forward results (xt, xn, stats) on the CPU.

    unaligned: "all" or a collection of operand names ("x", "pos", "w", "b", "gxn", "gres", "xt", "stats") passed as offset_view()s — same reference, same tolerances.

    mean_over_std=None: the rows of x are N(0.5, 2) and the reference is torch's fp32 F.layer_norm (the cases this check has always had).

    mean_over_std=r: every token row is N(m, 2) with m = +-2 r (1 +- 0.2), sign and jitter drawn per row.  The reference is FLOAT64 F.layer_norm and its autograd gradients
    evaluated on the fp32 xt the kernel returned (xt = x + pos is one correctly rounded fp32 add and is first held to the fp32 sum), so the comparison sees the kernels'
    arithmetic and not the representation error of x.  Bounds:
      stats mean   LN_MEAN_ULPS fp32 ulps of the row's |mean| (see below: one ulp is tighter than fp32 summation of C values delivers)
      stats rstd   rtol 1e-4
      xn           atol max(2e-5, 4e-7 * r * 2): ulp(|mean|) carried into (x - mean) * rstd (check_batchnorm_cl's form for the same fp32 floor)
      gradients    rtol 1e-4, unscaled: an error d of the mean moves xhat by d * rstd ~ 1.5e-7 r per ulp, i.e. 7e-5 at r = 500, and the gradients by less
    torch's OWN fp32 CPU kernels (torch.native_layer_norm and its autograd) against the same float64 reference on these inputs, worst over the five emulator and the
    five GPU shapes of test_layernorm_tokens_large_mean:
      r      xn abs    (bound)   mean, ulps   rstd rel   gxt rel    gw rel     gb rel     gpos rel
      20     1.14e-5   (2e-5)    2.07         6.76e-7    5.16e-7    2.27e-6    5.04e-7    3.79e-7
      100    5.11e-5   (8e-5)    2.17         2.43e-6    3.37e-6    6.51e-6    5.04e-7    2.71e-6
      500    3.43e-4   (4e-4)    1.98         3.46e-5    2.03e-5    3.57e-5    5.04e-7    1.62e-5
    torch is inside every bound but "one ulp of |mean|": summing C fp32 values of one sign rounds at every level of the tree, and its own row mean is about 2 ulps off
    at each ratio.  The mean's bound is therefore TWICE torch's measured error at that ratio (LN_MEAN_ULPS = 4.14 / 4.34 / 3.96 ulps); every other bound stands as the
    fp32 floor gives it.  None of them was set from the HIP kernels' output.
    The one-pass variance E[x^2] - mean^2 these kernels computed before missed the bounds at every ratio and shape; worst over the five emulator shapes:
      r      xn abs     rstd rel   gxt rel    gw rel
      20     3.35e-4    4.49e-5    2.55e-5    2.35e-5      (xn alone outside its bound)
      100    6.18e-3    1.34e-3    6.24e-4    6.25e-4
      500    1.42e-1    3.48e-2    1.76e-2    2.17e-2"""
    from deformablelka_amd import ops
    x, w, b, pe, gxn, gres = layernorm_inputs(B, C, N, planar, pos, seed, mean_over_std)
    t32 = x.permute(0, 2, 1) if planar else x
    if pos:
        t32 = t32 + pe
    u = unaligned
    wd_, bd_ = _put(w, dev, "w", u), _put(b, dev, "b", u)
    xt, xn, stats = ops.layernorm_tokens_forward(_put(x, dev, "x", u), planar, _put(pe, dev, "pos", u), wd_, bd_)
    fwd = (xt.cpu().clone(), xn.cpu().clone(), stats.cpu().clone())
    gxt, gw, gb, gpos = ops.layernorm_tokens_backward(_put(gxn, dev, "gxn", u), _put(gres, dev, "gres", u), _put(xt, dev, "xt", u), _put(stats, dev, "stats", u), wd_,
                                                      with_pos=pos)
    assert_close("ln xt", xt, t32, atol=1e-6)
    if mean_over_std is None:
        xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        per = pe.clone().requires_grad_(True) if pos else None
        t = xr.permute(0, 2, 1) if planar else xr
        if pos:
            t = t + per
        n = F.layer_norm(t, (C,), wr, br, 1e-5)
        (n * gxn).sum().backward(retain_graph=True)
        (t * gres).sum().backward()
        assert_close("ln xn", xn, n.detach(), atol=2e-5)
        ref_gx = xr.grad.permute(0, 2, 1) if planar else xr.grad
        ref_gpos = per.grad if pos else None
    else:
        r = float(mean_over_std)
        td, wr, br = xt.cpu().double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
        n = F.layer_norm(td, (C,), wr, br, 1e-5)
        ((n * gxn.double()).sum() + (td * gres.double()).sum()).backward()
        mean64 = td.detach().mean(-1).reshape(-1)
        rstd64 = torch.rsqrt(td.detach().var(-1, unbiased=False) + 1e-5).reshape(-1)
        e_mean = ((stats[:, 0].cpu().double() - mean64).abs() / 2.0 ** (torch.floor(torch.log2(mean64.abs())) - 23)).max().item()   # in fp32 ulps of the row's |mean|
        e_rstd, e_xn = rel_err(stats[:, 1], rstd64), (xn.cpu().double() - n.detach()).abs().max().item()
        print(f"[ln r={r:g} B={B} C={C} N={N} planar={planar} pos={pos}] mean err {e_mean:.2f} ulp; rstd rel {e_rstd:.3e}; xn abs {e_xn:.3e}; "
              f"gxt rel {rel_err(gxt, td.grad):.3e}; gw rel {rel_err(gw, wr.grad):.3e}; gb rel {rel_err(gb, br.grad):.3e}")
        assert e_mean <= LN_MEAN_ULPS[r], f"ln mean: {e_mean:.2f} fp32 ulps of |mean| off, more than {LN_MEAN_ULPS[r]}"
        assert_close("ln rstd", stats[:, 1], rstd64, rtol=1e-4)
        assert_close("ln xn", xn, n.detach(), atol=max(2e-5, 4e-7 * r * LN_SCALE))
        ref_gx, ref_gpos = td.grad, td.grad.sum(0, keepdim=True)
    assert_close("ln gx", gxt, ref_gx, rtol=1e-4)
    assert_close("ln gw", gw, wr.grad, rtol=1e-4)
    assert_close("ln gb", gb, br.grad, rtol=1e-4)
    if pos:
        assert_close("ln gpos", gpos, ref_gpos, rtol=1e-4)
    return fwd


def check_layernorm_unsupported_width(dev, C=257):
    """LayerNorm keeps at most 4 channels per lane (C <= 256): a wider row is refused with DLKA_ERR_UNSUPPORTED by both directions, and nothing is written."""
    from deformablelka_amd import _lib as L, ops
    B, N = 1, 5
    x, w, b = torch.randn(B, N, C).to(dev), torch.randn(C).to(dev), torch.randn(C).to(dev)
    with raises_status(-8):
        ops.layernorm_tokens_forward(x, False, None, w, b)
    mark = 1234.5
    outs = [torch.full((B, N, C), mark).to(dev), torch.full((B, N, C), mark).to(dev), torch.full((B * N, 2), mark).to(dev)]
    lib = L.get_lib()
    rc = lib.dlka_layernorm_tokens_forward(L.ptr(x), 0, L.ptr(None), L.ptr(w), L.ptr(b), *(L.ptr(o) for o in outs), B, N, C, 1e-5, L.dtype_code(x), L.stream_ptr(x))
    assert rc == -8, rc
    gouts = [torch.full((B, N, C), mark).to(dev), torch.full((C,), mark).to(dev), torch.full((C,), mark).to(dev), torch.full((1, N, C), mark).to(dev)]
    rc = lib.dlka_layernorm_tokens_backward(L.ptr(x), L.ptr(x), L.ptr(x), L.ptr(outs[2]), L.ptr(w), *(L.ptr(o) for o in gouts), B, N, C, L.dtype_code(x), L.stream_ptr(x))
    assert rc == -8, rc
    for o in outs + gouts:
        assert bool((o.cpu() == mark).all())


class raises_status:
    """The library's error for a dlka_status code, as ops.py raises it (RuntimeError "...(dlka status <code>)")."""

    def __init__(self, code):
        self.code = code

    def __enter__(self):
        return self

    def __exit__(self, et, ev, tb):
        assert et is not None, f"expected dlka status {self.code}, the call succeeded"
        assert issubclass(et, RuntimeError) and f"(dlka status {self.code})" in str(ev), (et, ev)
        return True


def check_batchnorm_cl(dev, M, C, training, with_res, seed=0, mean_over_std=0.2, unaligned=()):
    """BatchNorm (+ residual) + LeakyReLU over channels-last rows, forward and backward.  Returns y on the CPU.
    unaligned: "all" or a collection of operand names ("x", "res", "w", "b", "stats" (eval mode: caller-supplied), "gy", "y") passed as offset_view()s."""
    from deformablelka_amd import ops
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, C, generator=g) * 1.5 + 1.5 * mean_over_std
    res = torch.randn(M, C, generator=g) if with_res else None
    w, b = torch.randn(C, generator=g), torch.randn(C, generator=g)
    rm, rv = torch.randn(C, generator=g) * 0.2, torch.rand(C, generator=g) + 0.5
    gy = torch.randn(M, C, generator=g)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    rr = res.clone().requires_grad_(True) if with_res else None
    v = F.batch_norm(xr, None if training else rm, None if training else rv, wr, br, training, 0.1, 1e-5)
    if with_res:
        v = v + rr
    y_ref = F.leaky_relu(v, 0.01)
    u = unaligned
    if training:
        stats = torch.empty(3 * C).to(dev)
    else:
        stats = _put(torch.cat([rm, torch.rsqrt(rv + 1e-5), rv]), dev, "stats", u)
    xd_, wd_ = _put(x, dev, "x", u), _put(w, dev, "w", u)
    y = ops.batchnorm_cl_forward(xd_, _put(res, dev, "res", u), wd_, _put(b, dev, "b", u), stats, training)
    if os.environ.get("DLKA_PARITY_VERBOSE"):
        print(f"[bn M={M} C={C} training={training}] y abs {(y.cpu().double() - y_ref.detach().double()).abs().max().item():.3e}")
    # fp32 floor: x carries ulp(|mean|) of representation error into (x - mean) * rstd, e.g. 6e-5 at mean 750
    assert_close("bn y", y, y_ref.detach(), atol=max(2e-5, 4e-7 * 1.5 * mean_over_std))
    if training:
        assert_close("bn mean", stats[:C], x.double().mean(0), atol=max(1e-5, 2e-7 * 1.5 * mean_over_std))   # one fp32 ulp of |mean|
        assert_close("bn var", stats[2 * C:], x.double().var(0, unbiased=True), rtol=1e-4)
    # LeakyReLU has a kink at 0: where the pre-activation is within rounding of 0 the two forwards may sit on different sides of it (slope 1 vs
    # 0.01), and a single such element moves gw / gb by ~1e-3.  The reference backward therefore takes the activation pattern of the
    # forward under test (sign of ITS y), which is what a backward pass consistent with that forward has to use.
    gpre = gy * torch.where(y.detach().cpu() > 0, torch.ones(()), torch.full((), 0.01))
    v.backward(gpre)
    gx, gres, gw, gb = ops.batchnorm_cl_backward(_put(gy, dev, "gy", u), xd_, _put(y, dev, "y", u), wd_, stats, training, with_res=with_res)
    assert_close("bn gx", gx, xr.grad, rtol=max(2e-4, 2e-6 * mean_over_std))
    assert_close("bn gw", gw, wr.grad, rtol=max(2e-4, 2e-6 * mean_over_std))
    assert_close("bn gb", gb, br.grad, rtol=2e-4)
    if with_res:
        assert_close("bn gres", gres, rr.grad, rtol=1e-5)
    return y.detach().cpu().clone()


def check_scale_residual(dev, M, C, seed=0, unaligned=()):
    """out = xt + gamma * e and its backward, then the Dropout3d channel scale.  Returns out on the CPU.  The backward takes C % 32 == 0 only: at any other width it must
    refuse with DLKA_ERR_SHAPE.  unaligned: "all" or a collection of operand names ("xt", "e", "gamma", "gy") passed as offset_view()s."""
    from deformablelka_amd import ops
    g = torch.Generator().manual_seed(seed)
    xt, e, gm, gy = torch.randn(M, C, generator=g), torch.randn(M, C, generator=g), torch.randn(C, generator=g), torch.randn(M, C, generator=g)
    u = unaligned
    ed_, gmd_ = _put(e, dev, "e", u), _put(gm, dev, "gamma", u)
    out = ops.scale_residual_forward(_put(xt, dev, "xt", u), ed_, gmd_)
    assert_close("sr out", out, xt + gm * e, atol=1e-6)
    if C % 32:
        with raises_status(-4):
            ops.scale_residual_backward(_put(gy, dev, "gy", u), ed_, gmd_)
    else:
        ge, gg = ops.scale_residual_backward(_put(gy, dev, "gy", u), ed_, gmd_)
        assert_close("sr ge", ge, gy * gm, atol=1e-6)
        assert_close("sr ggamma", gg, (gy * e).sum(0), rtol=1e-4)
    B = 3
    x3, mask = torch.randn(B, 7, C, generator=g), torch.rand(B, C, generator=g)
    assert_close("channel scale", ops.channel_scale(_put(x3, dev, "x3", u), _put(mask, dev, "mask", u)), x3 * mask[:, None, :], atol=1e-6)
    return out.cpu().clone()


def check_norm_ops_unaligned(dev, op, M, C):
    """A quad width (C in {32, 64, 128, 256}) takes the 16-byte kernels only while EVERY pointer they load or store 16 bytes through is aligned (the quad_aligned
    terms of the launchers in csrc/cl_norm.hip).  Three ways through the same check, same reference, same tolerances: (c) aligned — the quad kernels; (a) every
    caller-supplied operand an offset_view — the general kernels; (b) one operand at a time offset — the launcher must notice that operand alone (an incomplete guard
    list shows as a misaligned 16-byte load: a crash on the emulator, a wrong result or fault on the GPU).  The forward results (no atomics in those kernels; the
    training-mode BatchNorm statistics, which have, sit inside their own tolerance) of every variant agree with (c) within the check's tolerances.
    op: "ln" (LayerNorm with pos_embed, M = N tokens of one sample), "bn_eval" / "bn_train" (BatchNorm + residual + LeakyReLU), "sr" (scale-residual)."""
    if op == "ln":
        run = lambda u: check_layernorm_tokens(dev, 1, C, M, False, True, unaligned=u)
        names, tols = ("x", "pos", "w", "b", "gxn", "gres", "xt", "stats"), (dict(atol=1e-6), dict(atol=2e-5), dict(rtol=1e-4))
    elif op in ("bn_eval", "bn_train"):
        run = lambda u: (check_batchnorm_cl(dev, M, C, op == "bn_train", True, unaligned=u),)
        names, tols = ("x", "res", "w", "b", "gy", "y") + (("stats",) if op == "bn_eval" else ()), (dict(atol=2e-5),)
    else:
        run = lambda u: (check_scale_residual(dev, M, C, unaligned=u),)
        names, tols = ("xt", "e", "gamma", "gy"), (dict(atol=1e-6),)
    aligned = run(())
    for u in ["all"] + [(n,) for n in names]:
        got = run(u)
        for i, (a, r, t) in enumerate(zip(got, aligned, tols)):
            assert_close(f"{op} forward result {i}, unaligned={u}, against the aligned run", a, r, **t)


# The LeakyReLU-kink protocol (wrapper block, assembled net).  LeakyReLU's slope jumps from 0.01 to 1 at 0: a pre-activation within fp32 rounding of 0 can sit on
# different sides in two correct implementations, and ONE such element moves a gradient summed over N voxels by ~1 / sqrt(N) of its scale.  As for floor() in the
# deformable conv (cells counted, oracle re-run on the kernels' cells) the elements are IDENTIFIED, COUNTED and CAPPED, and the oracle is re-run on the kernels' own
# activation pattern (read back from `saved`: dlka_tblock3d_saved_activations_v) — after which EVERY element of EVERY gradient is held to the contract's 1e-3.
KINK_NEAR = 1e-4          # a disagreeing pre-activation must be this close to 0, relative to max |z| of its tensor (fp32 rounding of a 27 C-term sum: ~1e-6)
KINK_MAX_FRACTION = 2e-5  # ... and at most max(3, this fraction) of a tensor's elements may disagree (expected for z ~ N(0, 1) +- 1e-6: ~1e-6 of them)


def tokens_to_volume(t, B, C, dims):
    """[B, N, C] tokens -> [B, C, *dims] (the reference's permuted view, transformerblock.py:626)."""
    return t.permute(0, 2, 1).reshape(B, C, *dims)


def kink_report(pre_out):
    """pre_out: [(z, pattern used)] per LeakyReLU (oracle.blocks.leaky_relu_signed).  Returns (number of elements whose pattern differs from the oracle's own z > 0,
    the largest |z| / max|z| among them, total elements) and asserts the caps above."""
    n_dis, worst, total = 0, 0.0, 0
    for z, pat in pre_out:
        dis = pat != (z > 0)
        k = int(dis.sum())
        total += z.numel()
        if k:
            rel = float(z[dis].abs().max() / z.abs().max().clamp_min(1e-30))
            worst = max(worst, rel)
            assert rel <= KINK_NEAR, f"activation pattern differs at a pre-activation {rel:.2e} of max|z| away from LeakyReLU's kink (> {KINK_NEAR}): not a rounding flip"
            assert k <= max(3, int(KINK_MAX_FRACTION * z.numel())), f"{k} of {z.numel()} LeakyReLU pre-activations on the other side of the kink"
        n_dis += k
    return n_dis, worst, total


def check_tblock3d(dev, B, C, dims, training, pos, seed=0, offset_std=0.02, atol=FWD_ATOL, rtol=BWD_RTOL, chain=False, report=False, acdc=False,
                   token_mean_over_std=0.0, prepare=None):
    """The fused wrapper block vs the oracle composition (oracle/blocks.py transformer_block_3d): forward 1e-4 abs (north_star), EVERY gradient 1e-3 rel
    (SURVEY §8c), every element of it — on identical sampling cells (the oracle fed the kernels' predicted offsets, as check_lka3d_tokens does) and on the
    kernels' activation pattern at UnetResBlock's two LeakyReLUs (kink protocol above: disagreements counted and capped).  chain=True: two applications of the
    block, each with its own offsets / patterns.  The plain comparison (oracle on its own cells and pattern) is reported and sanity-bounded.
    token_mean_over_std=r: every token (voxel) of the N(0, 1) input is shifted by +-r (1 +- 0.2), sign and jitter drawn per token — the rows the block's LayerNorm
    sees then have |mean| >> std (check_layernorm_tokens, mean_over_std)."""
    import deformablelka_amd as dk
    from deformablelka_amd import ops as _ops
    from oracle import blocks
    torch.manual_seed(seed)
    H, W, D = dims
    N = H * W * D
    if acdc:
        from deformablelka_amd import acdc as _acdc
        m = _acdc.TransformerBlock_3D_single_deform_LKA(N, C, C, 4, dropout_rate=0.1, pos_embed=pos)
    else:
        m = dk.TransformerBlock_3D_single_deform_LKA(N, C, C, 4, dropout_rate=0.1, pos_embed=pos)
    blocks.randomize_offsets_(m, std=offset_std)
    if prepare is not None:
        prepare(m)
    with torch.no_grad():
        m.gamma.normal_(0.5, 0.2)
        if pos:
            m.pos_embed.normal_(0, 0.5)
        for bn in (m.conv51.norm1, m.conv51.norm2):
            bn.weight.normal_(1.0, 0.2)
            bn.bias.normal_(0, 0.2)
            bn.running_mean.normal_(0, 0.3)
            bn.running_var.uniform_(0.5, 1.5)
    m.train(training)
    x = torch.randn(B, C, H, W, D)
    gy = torch.randn(B, C, H, W, D)
    mask = torch.nn.functional.dropout3d(torch.ones(B, C, 1, 1, 1), 0.1, True).view(B, C) if training else None
    if token_mean_over_std:
        sign = (torch.rand(B, 1, H, W, D) < 0.5).float() * 2 - 1
        x = x + token_mean_over_std * sign * (0.8 + 0.4 * torch.rand(B, 1, H, W, D))
    napp = 2 if chain else 1

    def run_oracle(overrides=None):
        """overrides: per application (offsets, (s1, s2, s2_known)) from the kernels' forward pass, or None = the oracle's own cells and pattern."""
        Pr = {k: (v.detach().clone().requires_grad_(True) if v.is_floating_point() and "running" not in k else v.detach().clone())
              for k, v in m0.items()}
        xr_ = x.detach().clone().requires_grad_(True)
        pre, offs = [], []
        yr_ = xr_
        for a_ in range(napp):
            o_, s_ = overrides[a_] if overrides is not None else (None, None)
            yr_ = blocks.transformer_block_3d(yr_, Pr, training, mask, offsets_override=o_, offsets_out=offs, act_signs=s_, pre_out=pre)
        yr_.backward(gy)
        return yr_.detach(), xr_.grad, {k: v.grad for k, v in Pr.items() if torch.is_tensor(v) and v.requires_grad}, pre, offs
    m0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    y0, gx0, g0, _, off0 = run_oracle()
    m = m.to(dev)
    m._draw_drop_mask = lambda B_, C_, dtype, device: mask.to(device)
    xd = x.to(dev).requires_grad_(True)
    m.keep_channels_last = chain
    saved_log = []
    orig = _ops.tblock3d_forward

    def spy(*a, **k):
        out = orig(*a, **k)
        saved_log.append(out[1])
        return out

    _ops.tblock3d_forward = spy
    try:
        y = m(xd)
        if chain:
            assert y.permute(0, 2, 3, 4, 1).is_contiguous()   # opt-in: the channels_last_3d view of the token memory
            y = m(y)                                          # second application reads the tokens in place (x_planar = 0)
        else:
            assert y.is_contiguous()                          # default: contiguous NCDHW like the reference (transformerblock.py:626-630)
    finally:
        _ops.tblock3d_forward = orig
    assert len(saved_log) == napp
    y.backward(gy.to(dev))
    variant = m.epa_block.variant
    overrides, flipped, nsamp = [], 0, 0
    k3 = ((3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1))
    for a_, sv in enumerate(saved_log):
        off_hip = _ops.tblock3d_saved_offsets(sv, B, C, dims, variant).cpu().clone()
        s1, s2, k2 = (tokens_to_volume(t.cpu(), B, C, dims) for t in _ops.tblock3d_saved_activation_signs(sv, B, C, dims, variant))
        overrides.append((off_hip, (s1, s2, k2)))
        i_h, m_h = oracle.deform_conv3d_sample_index(off_hip, dims, *k3)
        i_r, m_r = oracle.deform_conv3d_sample_index(off0[a_], dims, *k3)
        flipped += int(((i_h != i_r).any(-1) | (m_h != m_r)).sum())
        nsamp += m_r.numel()
    yr, gxr, gr, pre, _ = run_oracle(overrides)
    n_dis, worst_z, n_act = kink_report(pre)
    if report or os.environ.get("DLKA_PARITY_VERBOSE"):
        print(f"[tblock C={C} dims={dims}] y abs {(y.detach().cpu() - yr).abs().max().item():.3e} of max |y| {yr.abs().max().item():.3e}; gx rel {rel_err(xd.grad, gxr):.3e} "
              f"(own cells / pattern: {rel_err(xd.grad, gx0):.3e}); cells that differ {flipped} of {nsamp}; LeakyReLU patterns that differ {n_dis} of {n_act} "
              f"(|z| <= {worst_z:.1e} of max)")
        for k, p in m.named_parameters():
            if gr.get(k) is not None:
                print(f"  {k:60s} {rel_err(p.grad, gr[k]):.3e}   (own cells / pattern {rel_err(p.grad, g0[k]):.3e})")
    assert flipped <= max(3, int(2e-5 * nsamp)), f"tblock: {flipped} of {nsamp} sampling cells differ from the oracle's"
    bad = []
    e = (y.detach().cpu().double() - yr.double()).abs().max().item()
    if e > atol:
        bad.append(f"y abs {e:.3e} > {atol}")
    e = (y.detach().cpu().double() - y0.double()).abs().max().item()
    if e > atol:
        bad.append(f"y abs (oracle on its own cells) {e:.3e} > {atol}")
    e = rel_err(xd.grad, gxr)
    if e > rtol:
        bad.append(f"gx rel {e:.3e} > {rtol}")
    # the plain comparison: each differing cell / pattern element moves a gradient by at most ~1 / sqrt(voxels) of its scale
    loose = max(8 * rtol, 4.0 * (flipped + n_dis) / (B * N) ** 0.5) if flipped + n_dis else rtol
    for k, p in m.named_parameters():
        g = gr.get(k)
        if g is not None and g.abs().max() > 0:
            e = rel_err(p.grad, g)
            if e > rtol:
                bad.append(f"{k} rel {e:.3e} > {rtol}")
            e = rel_err(p.grad, g0[k])
            if e > loose:
                bad.append(f"{k} rel (oracle on its own cells / pattern) {e:.3e} > {loose:.3e}")
    assert not bad, "tblock: " + "; ".join(bad)


def check_tblock3d_mixed_bf16(dev, B, C, dims, training=True, seed=0, offset_std=0.3, rtol=BF16_RTOL, via_autocast=True, report=False, bn_bias=6.0):
    """The wrapper block in its MIXED mode (dlka_tblock3d_*, dtype = DLKA_BF16: fp32 wrapper, the D-LKA attention inside on bf16 activations) — selected by
    torch.autocast(bfloat16) or by a bf16 input — against the fp32 oracle block and against the bf16-storage model of that mode
    (oracle.blocks.transformer_block_3d(lka_store=bf16_storage)): output and every gradient within 2e-2 of max |reference|."""
    import deformablelka_amd as dk
    from deformablelka_amd import ops as _ops
    from oracle import blocks
    torch.manual_seed(seed)
    H, W, D = dims
    m = dk.TransformerBlock_3D_single_deform_LKA(H * W * D, C, C, 4, dropout_rate=0.1, pos_embed=True)
    blocks.randomize_offsets_(m, std=offset_std)
    with torch.no_grad():
        m.gamma.normal_(0.5, 0.2)
        m.pos_embed.normal_(0, 0.5)
        for bn in (m.conv51.norm1, m.conv51.norm2):
            bn.weight.normal_(1.0, 0.2)
            # LeakyReLU has a kink at 0 and bf16 rounding moves ~1e-3 of the pre-activations across it: each such element changes ITS gradient term by a
            # factor 100, i.e. a relative error of ~sqrt(flipped fraction) ~ 3 - 6 % in every gradient upstream of the activation — a property of bf16
            # activations in front of a kink (any framework), not of these kernels, and unrelated to what this test is for (the bf16 hand-over tensors
            # xn / e / g_e / g_xn of the mixed mode).  The biases keep both activations on their linear side here; the kink itself is covered in fp32
            # by check_tblock3d.
            bn.bias.fill_(bn_bias)
    m.train(training)
    x = torch.randn(B, C, H, W, D)
    if not via_autocast:
        x = x.bfloat16().float()   # (the block is handed a bf16 tensor: both sides see the rounded input)
    gy = torch.randn(B, C, H, W, D)
    mask = torch.nn.functional.dropout3d(torch.ones(B, C, 1, 1, 1), 0.1, True).view(B, C) if training else None
    m0 = {k: v.detach().clone() for k, v in m.state_dict().items()}

    def run_oracle(store, override=None, offsets_out=None):
        Pr = {k: (v.detach().clone().requires_grad_(True) if v.is_floating_point() and "running" not in k else v.detach().clone()) for k, v in m0.items()}
        xr = x.detach().clone().requires_grad_(True)
        yr = blocks.transformer_block_3d(xr, Pr, training, mask, lka_store=store, offsets_override=override, offsets_out=offsets_out)
        yr.backward(gy)
        return yr.detach(), xr.grad, {k: v.grad for k, v in Pr.items() if torch.is_tensor(v) and v.requires_grad}

    offs32 = []
    y32, gx32, g32 = run_oracle(None, offsets_out=offs32)
    m = m.to(dev)
    m._draw_drop_mask = lambda B_, C_, dtype, device: mask.to(device)
    flags, saved_log = [], []
    orig = _ops.tblock3d_forward

    def spy(*a, **k):
        flags.append(bool(a[11]) if len(a) > 11 else bool(k.get("lka_bf16", False)))
        out = orig(*a, **k)
        saved_log.append(out[1])
        return out

    _ops.tblock3d_forward = spy
    try:
        if via_autocast:
            xd = x.to(dev).requires_grad_(True)
            with torch.autocast(torch.device(dev).type, dtype=torch.bfloat16):
                y = m(xd)
        else:
            xd = x.to(dev).bfloat16().requires_grad_(True)
            y = m(xd)
    finally:
        _ops.tblock3d_forward = orig
    assert flags == [True], f"the wrapper block did not select its mixed bf16 mode: {flags}"
    assert y.dtype == torch.float32
    y.backward(gy.to(dev))
    # (1) The sampling cells.  Round 5: the chain that decides them starts from LayerNorm's UNROUNDED fp32 output (dlka_tblock3d_forward_v hands the attention an fp32
    # twin of its bf16 input), so the predicted offsets agree with the fp32 block's to fp32 rounding: the cells that differ are counted and must be (almost) none.  Round 4
    # started the chain from the bf16 tensor: 2^-9 in front of floor() flipped ~1e-3 of the cells and moved conv_offset.weight.grad by 5 - 10 %.
    off_hip = _ops.tblock3d_saved_offsets(saved_log[0], B, C, dims, 0, lka_bf16=True).cpu().clone()
    flips = int((torch.floor(off_hip) != torch.floor(offs32[0].reshape(off_hip.shape))).sum()) if via_autocast else 0
    nsamp = off_hip.numel()
    # (2) three CPU runs on the kernels' OWN cells (their predicted offsets, read back from `saved`): the fp32 oracle, and the bf16-storage MODEL of the mode (same
    # arithmetic, every hand-over tensor rounded where the kernels round it, the chain from the unrounded LayerNorm output)
    y32c, gx32c, g32c = run_oracle(None, off_hip)
    y16, gx16, g16 = run_oracle(blocks.bf16_storage, off_hip)
    errs = {"y": rel_err(y, y32c), "gx": rel_err(xd.grad, gx32c)}           # kernels vs fp32 oracle
    errs16 = {"y": rel_err(y, y16), "gx": rel_err(xd.grad, gx16)}           # kernels vs the model
    model = {"y": rel_err(y16, y32c), "gx": rel_err(gx16, gx32c)}           # the model vs fp32 oracle: what bf16 storage itself costs
    for k, p_ in m.named_parameters():
        assert p_.grad is not None and p_.grad.dtype == torch.float32, k
        if g32c.get(k) is not None and g32c[k].abs().max() > 0:
            errs[k] = rel_err(p_.grad, g32c[k])
            errs16[k] = rel_err(p_.grad, g16[k])
            model[k] = rel_err(g16[k], g32c[k])
    if report or os.environ.get("DLKA_PARITY_VERBOSE"):
        worst = sorted(errs.items(), key=lambda kv: -kv[1])[:5]
        worst16 = sorted(errs16.items(), key=lambda kv: -kv[1])[:5]
        worstm = sorted(model.items(), key=lambda kv: -kv[1])[:3]
        tag = f"[tblock mixed bf16 C={C} dims={dims} bn bias {bn_bias}]"
        print(f"{tag} cells that differ from the fp32 block's: {flips} of {nsamp}; y vs fp32 oracle (own cells) {rel_err(y, y32):.1e}")
        print(f"{tag} worst vs fp32 oracle (same cells): " + " ".join(f"{k.split('.')[-2:]}={v:.1e}" for k, v in worst))
        print(f"{tag} worst vs bf16-storage model (same cells): " + " ".join(f"{k.split('.')[-2:]}={v:.1e}" for k, v in worst16))
        print(f"{tag} the MODEL vs fp32 oracle (same cells): " + " ".join(f"{k.split('.')[-2:]}={v:.1e}" for k, v in worstm))
    assert rel_err(y, y32) <= rtol, f"tblock mixed bf16 y: rel err vs fp32 oracle {rel_err(y, y32):.3e} > {rtol}"
    assert flips <= max(3, int(2e-5 * nsamp)), f"tblock mixed bf16: {flips} of {nsamp} sampling cells differ from the fp32 block's"
    # (3) The kernels implement the MODEL: every output / gradient within 2e-2 of it (max norm), with BatchNorm bias 6 (both LeakyReLUs on their linear side) AND 0 (the
    # regime a freshly initialised net trains in).  Shapes below ~1000 voxels are exempt at bias 0: two correct implementations of the same bf16 arithmetic put the few
    # pre-activations within rounding of 0 on different sides of LeakyReLU's kink, and ONE such element moves a gradient by ~1 / sqrt(voxels).
    # PER-ELEMENT tensors (grad_x, pos_embed.grad) at bias 0 are held in a norm that one element cannot move: relative L2 error <= 2e-2 AND at most 1e-4 of the
    # elements off by more than 2e-2 of the maximum — an element whose pre-activation sits within rounding of LeakyReLU's kink has ITS gradient term changed by a
    # factor 100 between any two implementations (measured on the MI355X at (32, 32^3): 21 % of max|grad_x| on a handful of elements, everything else 4e-3).
    def robust(a_, b_):
        a_, b_ = a_.detach().cpu().double(), b_.detach().cpu().double()
        d = (a_ - b_).abs()
        return float(d.norm() / b_.norm().clamp_min(1e-30)), float((d > rtol * b_.abs().max()).double().mean())
    per_element = {"gx": (xd.grad, gx16)}
    if m.pos_embed is not None and g16.get("pos_embed") is not None:
        per_element["pos_embed"] = (m.pos_embed.grad, g16["pos_embed"])
    if bn_bias >= 3.0 or B * H * W * D >= 1000:
        for k in errs16:
            if bn_bias < 3.0 and k in per_element:
                l2, frac = robust(*per_element[k])
                assert l2 <= rtol and frac <= 1e-4, f"tblock mixed bf16 {k} (bn bias {bn_bias}): vs the bf16-storage model L2 {l2:.3e}, {frac:.2e} of the elements beyond {rtol}"
                continue
            # bias 0: the SUMS collect the kink's noise too (~1e-3 of conv51's pre-activations sit within bf16 rounding of 0; measured kernels-vs-model 3.9e-2 on
            # conv51.conv1.weight at (64, 16^3) where the model itself is 4.9e-2 from the fp32 oracle): two implementations of the mode cannot be closer to each other
            # than the mode is to fp32, so the bound there is max(2e-2, model-vs-oracle); with both activations linear (bias 6) it is 2e-2 flat.
            lim16 = rtol if bn_bias >= 3.0 else max(rtol, model[k])
            assert errs16[k] <= lim16, f"tblock mixed bf16 {k} (bn bias {bn_bias}): rel err vs the bf16-storage model {errs16[k]:.3e} > {lim16:.3e}"
    # (4) ... and against the fp32 oracle ("bf16 path vs fp32 oracle <= 2e-2"): 2e-2 wherever bf16 STORAGE ITSELF allows it, i.e. every tensor is within
    # max(2e-2, twice the distance of the model from the fp32 oracle).  What the model cannot reach no implementation of bf16 hand-over tensors can: a bf16 tensor
    # (the attention's output e) in front of a LeakyReLU flips the side of the pre-activations within 2^-9 of 0, each flipped element changes ITS gradient term by
    # a factor 100 (slope 1 | 0.01) — isolated elements of grad_x / pos_embed.grad even at bias 6 (the second LeakyReLU adds the residual stream, which reaches -6),
    # and 2 - 5 % of conv51's parameter gradients at bias 0 (measured on the CPU model: conv51.conv2.weight 4.9e-2 at (64, 16^3)).
    for k in errs:
        lim = max(rtol, 2.0 * model[k])
        assert errs[k] <= lim, f"tblock mixed bf16 {k} (bn bias {bn_bias}): rel err vs the fp32 oracle {errs[k]:.3e} > {lim:.3e} (model vs oracle {model[k]:.3e})"
    return errs


def check_tblock3d_phased_backward(dev, B, C, dims, lka_bf16=False, seed=0):
    """dlka_tblock3d_backward_phase_v: the data chain (phase 1) followed by the weight gradients (phase 2) gives what the one-call pass (phase 0) gives — the same
    kernels on the same operands; only the order of a few fp32 atomics (tap-split / chunk-split outputs, LayerNorm / BatchNorm channel sums) may differ."""
    import deformablelka_amd as dk
    from deformablelka_amd import ops
    from oracle import blocks
    torch.manual_seed(seed)
    H, W, D = dims
    m = dk.TransformerBlock_3D_single_deform_LKA(H * W * D, C, C, 4, dropout_rate=0.1, pos_embed=True)
    blocks.randomize_offsets_(m, std=0.3)
    m = m.to(dev).train()
    x = torch.randn(B, H * W * D, C, device=dev)
    gy = torch.randn(B, H * W * D, C, device=dev)
    tparams = [None if p is None else p.detach() for p in m.wrapper_params()]
    lparams = [p.detach() for p in m.epa_block.block_params()]
    stats = torch.empty(6 * C, dtype=torch.float32, device=dev)
    mask = torch.ones(B, C, device=dev)
    y, saved = ops.tblock3d_forward(x, False, tparams, lparams, mask, True, stats, dims, 1e-5, 1e-5, 0, lka_bf16)
    whole = ops.tblock3d_backward(tparams, lparams, mask, True, stats, gy, saved, dims, 0, lka_bf16)
    split = ops.tblock3d_backward(tparams, lparams, mask, True, stats, gy, saved, dims, 0, lka_bf16, side_stream="inline")

    def flat(r):
        return [r[0]] + [t for t in r[1] if t is not None] + list(r[2])
    for k, (a_, b_) in enumerate(zip(flat(whole), flat(split))):
        assert torch.isfinite(b_).all(), k
        scale = max(float(a_.abs().max()), 1e-6)
        assert float((a_.float() - b_.float()).abs().max()) <= 2e-3 * scale, (k, float((a_.float() - b_.float()).abs().max()), scale)


def check_dwpair_equals_unfused(dev, B, C, dims, lka_bf16=False, seed=0):
    """cl_dwpair.hip (round 5): the small-volume stages run dw 5^3 -> dw 7^3 dil 3 (and, backward, their data gradients + GELU') as ONE launch with the intermediate in
    LDS.  Against the same block with DLKA_DWPAIR=0 (one launch per conv): the same fp32 FMAs in another order, so every output agrees to rounding (fp32) / to a bf16 ulp
    of the stored gradients (DLKA_BF16 storage) — and the saved activations t1, t the weight gradients read are the fused kernel's own stores."""
    import deformablelka_amd as dk
    from deformablelka_amd import ops
    from oracle import blocks
    torch.manual_seed(seed)
    H, W, D = dims
    m = dk.TransformerBlock_3D_single_deform_LKA(H * W * D, C, C, 4, dropout_rate=0.1, pos_embed=True)
    blocks.randomize_offsets_(m, std=0.05)
    m = m.to(dev).train()
    x = torch.randn(B, H * W * D, C, device=dev)
    gy = torch.randn(B, H * W * D, C, device=dev)
    tparams = [None if p is None else p.detach() for p in m.wrapper_params()]
    lparams = [p.detach() for p in m.epa_block.block_params()]
    mask = torch.ones(B, C, device=dev)
    old = os.environ.get("DLKA_DWPAIR")
    res = []
    try:
        from deformablelka_amd import _lib
        lib = _lib.get_lib()
        for mode in ("1", "0"):
            os.environ["DLKA_DWPAIR"] = mode
            _refresh_switches()
            n0 = lib.dlka_dwpair_launch_count()
            stats = torch.empty(6 * C, dtype=torch.float32, device=dev)
            y, saved = ops.tblock3d_forward(x, False, tparams, lparams, mask, True, stats, dims, 1e-5, 1e-5, 0, lka_bf16)
            r = ops.tblock3d_backward(tparams, lparams, mask, True, stats, gy, saved, dims, 0, lka_bf16)
            res.append([y, r[0]] + [t for t in r[1] if t is not None] + list(r[2]))
            assert lib.dlka_dwpair_launch_count() - n0 == (2 if mode == "1" else 0), (mode, n0, lib.dlka_dwpair_launch_count())   # which kernel produced it
    finally:
        if old is None:
            os.environ.pop("DLKA_DWPAIR", None)
        else:
            os.environ["DLKA_DWPAIR"] = old
        _refresh_switches()
    tol = 2e-2 if lka_bf16 else 2e-3
    worst = 0.0
    for k, (a_, b_) in enumerate(zip(*res)):
        assert torch.isfinite(a_).all(), k
        scale = max(float(b_.abs().max()), 1e-6)
        err = float((a_.float() - b_.float()).abs().max()) / scale
        worst = max(worst, err)
        assert err <= tol, (k, err)
    return worst


def check_prep_tiled_equals_elementwise(dev, stages, dtype=torch.float32):
    """Weight preparation tile by tile through LDS (cl_igemm.hip prep_job_tile, round 5) writes BITWISE what the element-per-lane re-layout writes (DLKA_PREP_TILED=0,
    decided when the job table is built): every prepared form of every block of a stack — plain fp32, two- and three-term bf16 records, forward / flipped / column
    orders, zero padding of Cout = 81 to 96 — compared over the blocks' whole `saved` buffers (zeroed first: both forms must also leave the same bytes untouched)."""
    from deformablelka_amd.stack import DLKABlockStack
    old = os.environ.get("DLKA_PREP_TILED")
    bufs = []
    try:
        for mode in ("1", "0"):
            os.environ["DLKA_PREP_TILED"] = mode
            _refresh_switches()
            st = DLKABlockStack(1, stages=stages, device=dev, dtype=dtype, seed=7)
            for b in st.blocks:
                b.saved.zero_()
            st.prepare()
            if torch.device(dev).type == "cuda":
                torch.cuda.synchronize()
            bufs.append([b.saved.clone().cpu() for b in st.blocks])
    finally:
        if old is None:
            os.environ.pop("DLKA_PREP_TILED", None)
        else:
            os.environ["DLKA_PREP_TILED"] = old
        _refresh_switches()
    for k, (a_, b_) in enumerate(zip(*bufs)):
        assert bool(a_.view(torch.uint8).ne(0).any()), k
        assert torch.equal(a_.view(torch.uint8), b_.view(torch.uint8)), (k, int(a_.view(torch.uint8).ne(b_.view(torch.uint8)).sum()))


def check_wgrad_pad_equals_unpadded(dev, B, Cin, Cout, dims, k, pad, dil, seed=0):
    """The dense weight gradient from the zero-padded copy of its input (cl_wgrad_dense_pad_kernel, round 5) against the kernels that test every (tap, row)'s coordinates
    (DLKA_WGRAD_PAD=0): where both contract with the same arithmetic (N % 16 == 0) the same products in the same order — a padding row contributes exact zeros — so the two
    agree BITWISE; elsewhere to the split's 1e-5.  Both are also held to the fp64 conv.
    dims = (D, H, W) of a channels-last volume, planar grad_out (the layout the offset tensors keep)."""
    from deformablelka_amd import ops
    g = torch.Generator().manual_seed(seed)
    D, H, W = dims
    k3, p3, d3 = ops._triple(k), ops._triple(pad), ops._triple(dil)
    x = torch.randn(B, D, H, W, Cin, generator=g)
    w = torch.randn(Cout, Cin, *k3, generator=g) * 0.05
    go = torch.randn(B, Cout, D, H, W, generator=g)
    old = os.environ.get("DLKA_WGRAD_PAD")
    res = []
    try:
        for mode in ("1", "0"):
            os.environ["DLKA_WGRAD_PAD"] = mode
            _refresh_switches()
            _, gw, gb = ops.conv3d_backward_cl(x.to(dev), w.to(dev), go.to(dev), p3, d3, 1, grad_out_planar=True)
            res.append((gw.cpu(), gb.cpu()))
    finally:
        if old is None:
            os.environ.pop("DLKA_WGRAD_PAD", None)
        else:
            os.environ["DLKA_WGRAD_PAD"] = old
        _refresh_switches()
    if (D * H * W) % 16 == 0:
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), float((res[0][0] - res[1][0]).abs().max())
    else:   # N % 16 != 0 with fp32 activations: the unpadded route is the exact fp32-input MFMA there, the padded kernels always contract as two-term bf16 splits (~1e-5)
        assert rel_err(res[0][0], res[1][0]) <= 1e-4 and rel_err(res[0][1], res[1][1]) <= 1e-4
    xr = x.permute(0, 4, 1, 2, 3).double().requires_grad_(True)
    wr = w.double().requires_grad_(True)
    F.conv3d(xr, wr, None, 1, p3, d3).backward(go.double())
    assert rel_err(res[0][0], wr.grad) <= 1e-3
