"""Shared cases of tests/test_planar_emu.py and tests/test_planar_gpu.py: the planar (NCDHW) plumbing kernels of csrc/planar_ops.hip — BatchNorm statistics, apply and
backward, the 1x1x1 convolution with its MFMA weight gradient — and the modules of network.py over them, at ragged and edge shapes; plus the stand-alone GELU.

Every check takes a device string, draws its inputs from a seeded torch.Generator on the CPU and compares with plain float64 torch on the CPU (F.batch_norm in training
mode, matmul / einsum, erfc), never with the product.  A reference is computed once per case (functools.lru_cache) and never written to.  Nothing is compared bitwise
between runs: the statistics and the weight gradient meet in float atomics.

Tolerances — per element |got - ref| <= atol + rtol |ref| — are the ones the suite already holds for these entries (test_batchnorm_planar_training_mode of
test_parity_emu.py, test_pointwise_planar_conv_real_shapes_vs_torch of test_parity_gpu.py):

  BatchNorm   y 1e-4 / 1e-4;  mean 1e-5 / 1e-5;  unbiased variance 1e-3 / 1e-7;  gx 1e-3 / 1e-4 max|gx_ref|;  gw 1e-3 / 1e-3;  gb 1e-4 / 1e-4
  pointwise   y, gx 1e-5 / 1e-5;  gw, gb 1e-4 / 1e-4 max|ref|
  GELU fp32   torch.allclose(atol=1e-6) forward, (atol=1e-5) backward, as test_gelu of test_parity_emu.py (allclose's default rtol = 1e-5 included)
  GELU bf16   one bf16 ulp of the float64 reference value: 2^(floor(log2 |ref|) - 7), at the bottom of the range bf16's smallest subnormal 2^-133

No case below needed another bound."""
import functools
import math
from unittest import mock

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from deformablelka_amd import ops

BN_TOL = {"y": (1e-4, 1e-4), "mean": (1e-5, 1e-5), "var": (1e-3, 1e-7), "gx": (1e-3, None), "gw": (1e-3, 1e-3), "gb": (1e-4, 1e-4)}   # gx: atol = 1e-4 max|gx_ref|
PW_TOL = {"y": (1e-5, 1e-5), "gx": (1e-5, 1e-5), "gw": (1e-4, None), "gb": (1e-4, None)}                                                 # gw, gb: atol = 1e-4 max|ref|
EPS = 1e-5


def shape_id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def assert_close(what, got, ref, rtol, atol):
    """Per element |got - ref| <= atol + rtol |ref|; prints the worst ratio and where it is before it asserts."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} of {got.numel()} elements are not finite"
    err = (got - ref).abs()
    ratio = (err / (atol + rtol * ref.abs())).flatten()
    at = int(ratio.argmax())
    worst = float(ratio[at])
    print(f"[{what}] max |err| / ({atol:.1e} + {rtol:.0e} |ref|) = {worst:.3f} at element {at} (got {float(got.flatten()[at]):.7g}, ref {float(ref.flatten()[at]):.7g}); "
          f"max abs err {float(err.max()):.3e}")
    assert worst <= 1.0, f"{what}: |got - ref| exceeds {atol:.1e} + {rtol:.0e} |ref| by a factor {worst:.3f} at element {at}"


def _scaled(tol, ref):
    rtol, atol = tol
    return rtol, (1e-4 * max(float(ref.abs().max()), 1e-30) if atol is None else atol)


# ---- 1. BatchNorm kernels -----------------------------------------------------------------------------------------------------------------------------------------
# PL_CHUNK = 4096 elements of a plane per workgroup of the apply kernels, PL_RCHUNK = 32768 of the reducing kernels, 256 threads; N & 3 picks the scalar branch.
BN_SHAPES = [
    (3, 4, 1, 1, 1),       # N = 1: only thread 0 of each workgroup has data
    (2, 5, 1, 2, 2),       # N = 4: one vector load per plane
    (3, 5, 2, 3, 7),       # N = 42: scalar branch, one workgroup (the emulator suite's case)
    (1, 2, 8, 16, 32),     # N = 4096: exactly one apply workgroup
    (1, 2, 32, 32, 32),    # N = 32768: exactly one reduce workgroup
    (2, 3, 1, 5, 6557),    # N = 32785 = 32768 + 17: scalar; two reduce workgroups, the second with 17 elements; nine apply workgroups, the last with 17
    (2, 3, 5, 2, 3278),    # N = 32780 = 32768 + 12: vector; the second reduce workgroup has three active threads
    (2, 3, 1, 3, 4099),    # N = 12297: scalar, three full apply chunks plus 9
]
BN_SHAPES_SMALL = [s for s in BN_SHAPES if math.prod(s[2:]) <= 4096]
BN_SHAPES_327XX = [s for s in BN_SHAPES if 32768 < math.prod(s[2:]) < 32800]


def bn_reference(x, w, b, gy):
    """F.batch_norm in training mode in double: y, the batch mean, the unbiased variance (what momentum = 1 leaves in the running estimates) and all gradients."""
    C = x.shape[1]
    xr = x.double().requires_grad_(True)
    wr = None if w is None else w.double().requires_grad_(True)
    br = None if b is None else b.double().requires_grad_(True)
    rm, rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    yr = F.batch_norm(xr, rm, rv, wr, br, True, 1.0, EPS)
    yr.backward(gy.double())
    return {"y": yr.detach(), "mean": rm, "var": rv, "gx": xr.grad, "gw": None if w is None else wr.grad, "gb": None if b is None else br.grad}


def _bn_params(C, affine, shape, g):
    w = torch.randn(C, generator=g) if affine else None
    b = torch.randn(C, generator=g) if affine else None
    return w, b, torch.randn(shape, generator=g)


@functools.lru_cache(maxsize=None)
def _bn_case(shape, affine):
    g = torch.Generator().manual_seed(1000 + sum(shape))
    x = torch.randn(shape, generator=g)
    c = shape[1] - 1
    x[:, c] = x[:, c] * 0.01 + 300.0            # |mean| >> std: the pivoted sums must keep this channel's variance
    w, b, gy = _bn_params(shape[1], affine, shape, g)
    return x, w, b, gy, bn_reference(x, w, b, gy)


def check_batchnorm(dev, what, x, w, b, gy, ref, per_channel_y=False):
    """ops.batchnorm_planar_forward / _backward on (x, w, b, gy) — which may be non-contiguous views — against `ref`."""
    affine = w is not None
    to = lambda t: None if t is None else t.to(dev)
    y, stats = ops.batchnorm_planar_forward(to(x), to(w), to(b), EPS)
    gx, gw, gb = ops.batchnorm_planar_backward(to(gy), to(x), to(w), stats, affine)
    assert y.shape == x.shape and gx.shape == x.shape and stats.shape[1] == x.shape[1]
    assert (gw is None) == (not affine) and (gb is None) == (not affine)
    failures = []

    def chk(name, got, r, tol):
        try:
            assert_close(f"{what} {name}", got, r, *tol)
        except AssertionError as e:
            failures.append(str(e))

    if per_channel_y:
        for c in range(x.shape[1]):
            chk(f"y[:, {c}]", y[:, c], ref["y"][:, c], BN_TOL["y"])
    else:
        chk("y", y, ref["y"], BN_TOL["y"])
    chk("mean", stats[0], ref["mean"], BN_TOL["mean"])
    chk("var", stats[2], ref["var"], BN_TOL["var"])
    chk("gx", gx, ref["gx"], _scaled(BN_TOL["gx"], ref["gx"]))
    if affine:
        chk("gw", gw, ref["gw"], BN_TOL["gw"])
        chk("gb", gb, ref["gb"], BN_TOL["gb"])
    assert not failures, "\n".join(failures)


def batchnorm(dev, shape, affine):
    x, w, b, gy, ref = _bn_case(shape, affine)
    check_batchnorm(dev, f"bn {shape_id(shape)} affine={affine}", x, w, b, gy, ref)


# ---- 2. pivot robustness -------------------------------------------------------------------------------------------------------------------------------------------
# The kernels form var = m2 - m1^2 about a per-channel pivot; with d = (pivot - mean) / std the relative variance error is about eps_fp32 (1 + d^2).  The voxel
# x[0, c, 0, 0, 0] — what zero padding or a cropped background makes atypical — must not be able to spoil it.  The float64 reference includes the outlier in its
# statistics: this is about arithmetic, not about outlier rejection.
PIVOT_SHAPES = [(2, 4, 1, 1, 4099), (2, 4, 1, 200, 200)]     # N = 4099; N = 40000: two reduce workgroups
PIVOT_KINDS = ["outliers", "zero_corner"]


@functools.lru_cache(maxsize=None)
def _pivot_case(shape, kind):
    g = torch.Generator().manual_seed(2000 + sum(shape))
    x = torch.randn(shape, generator=g)
    if kind == "outliers":
        x[0, 1, 0, 0, 0], x[0, 2, 0, 0, 0], x[0, 3, 0, 0, 0] = 100.0, 1000.0, -1000.0
        x[-1, 0, -1, -1, -1] = 1000.0       # the control: the same outlier where it is not the first voxel
    else:
        x = x * 0.01 + 300.0
        x[0, :, 0, 0, 0] = 0.0
    w, b, gy = _bn_params(shape[1], True, shape, g)
    return x, w, b, gy, bn_reference(x, w, b, gy)


def pivot(dev, shape, kind):
    x, w, b, gy, ref = _pivot_case(shape, kind)
    check_batchnorm(dev, f"bn pivot {kind} {shape_id(shape)}", x, w, b, gy, ref, per_channel_y=True)


# ---- 3. modules over these kernels ---------------------------------------------------------------------------------------------------------------------------------
def batchnorm3d_module(dev, momentum):
    """network.BatchNorm3d against nn.BatchNorm3d in double over two training iterations: y, running_mean, running_var, num_batches_tracked after each."""
    from deformablelka_amd.network import BatchNorm3d
    shape = (2, 3, 1, 5, 6557)
    g = torch.Generator().manual_seed(3000)
    a, r = BatchNorm3d(3, momentum=momentum), nn.BatchNorm3d(3, momentum=momentum).double()
    with torch.no_grad():
        a.weight.copy_(torch.randn(3, generator=g) * 0.3 + 1.0)
        a.bias.copy_(torch.randn(3, generator=g) * 0.2)
    r.load_state_dict(a.state_dict())
    a = a.to(dev)
    for it in range(2):
        x = torch.randn(shape, generator=g) * (1.0 + it) + 0.5 * it
        x[:, 2] = x[:, 2] * 0.01 + 300.0
        y, yr = a(x.to(dev)), r(x.double())
        what = f"BatchNorm3d momentum={momentum} iteration {it}"
        assert_close(f"{what} y", y, yr, *BN_TOL["y"])
        assert_close(f"{what} running_mean", a.running_mean, r.running_mean, *BN_TOL["mean"])
        assert_close(f"{what} running_var", a.running_var, r.running_var, *BN_TOL["var"])
        assert int(a.num_batches_tracked) == int(r.num_batches_tracked) == it + 1


def _instance_norm_f64(x):
    xd = x.double().flatten(2)
    xh = (xd - xd.mean(-1, keepdim=True)) / torch.sqrt(xd.var(-1, unbiased=False, keepdim=True) + EPS)
    return xh.view(x.shape)


def instancenorm_grid_limit(dev):
    """network.InstanceNorm3d at B * C = 65535 planes — grid.y at its limit — against a float64 restatement: output and input gradient."""
    from deformablelka_amd import nn_ops
    from deformablelka_amd.network import InstanceNorm3d
    g = torch.Generator().manual_seed(3100)
    x = torch.randn(1, 65535, 2, 2, 2, generator=g) * 1.7 + 0.4
    gy = torch.randn(x.shape, generator=g)
    xr = x.double().requires_grad_(True)
    yr = _instance_norm_f64(xr)
    yr.backward(gy.double())
    xa = x.to(dev).requires_grad_(True)
    with mock.patch.object(nn_ops, "batch_norm_train", wraps=nn_ops.batch_norm_train) as spy:
        y = InstanceNorm3d(65535).to(dev)(xa)
    assert spy.call_count == 1, "65535 planes belong to the planar kernels"
    y.backward(gy.to(dev))
    assert_close("InstanceNorm3d 65535 planes y", y, yr, *BN_TOL["y"])
    assert_close("InstanceNorm3d 65535 planes gx", xa.grad, xr.grad, *_scaled(BN_TOL["gx"], xr.grad))


def instancenorm_past_grid_limit(dev):
    """65536 planes: the module takes the stock path and equals nn.InstanceNorm3d."""
    from deformablelka_amd import nn_ops
    from deformablelka_amd.network import InstanceNorm3d
    x = torch.randn(1, 65536, 2, 2, 2, generator=torch.Generator().manual_seed(3200)).to(dev)
    with mock.patch.object(nn_ops, "batch_norm_train", side_effect=AssertionError("65536 planes do not fit the grid")):
        y = InstanceNorm3d(65536).to(dev)(x)
    assert torch.equal(y, nn.InstanceNorm3d(65536).to(dev)(x))
    assert_close("InstanceNorm3d 65536 planes y", y, _instance_norm_f64(x.cpu()), *BN_TOL["y"])


def batchnorm_entry_past_grid_limit(dev):
    """ops.batchnorm_planar_forward on 65536 planes raises the shape error and launches nothing: the NaN-filled output stays as it was."""
    x = torch.randn(1, 65536, 8, generator=torch.Generator().manual_seed(3300)).to(dev)
    out = torch.full_like(x, float("nan"))
    with pytest.raises(RuntimeError, match="invalid shape"):
        ops.batchnorm_planar_forward(x, None, None, EPS, out=out)
    if dev != "cpu":
        torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), "the refused call wrote its output"
    with pytest.raises(RuntimeError, match="invalid shape"):
        ops.batchnorm_planar_backward(x, x, None, torch.zeros(ops.PLANAR_BN_STATS_ROWS, 65536).to(dev), False)


def one_value_per_channel(dev):
    """nn.BatchNorm3d in training mode refuses one value per channel, nn.InstanceNorm3d one spatial element (ValueError): the modules behave as the stock layers."""
    from deformablelka_amd.network import BatchNorm3d, InstanceNorm3d
    x = torch.randn(1, 4, 1, 1, 1, generator=torch.Generator().manual_seed(3400)).to(dev)
    for layer in (nn.BatchNorm3d(4), BatchNorm3d(4)):
        with pytest.raises(ValueError, match="more than 1 value per channel"):
            layer.to(dev).train()(x)
    bn = BatchNorm3d(4).to(dev).eval()
    assert torch.equal(bn(x), nn.BatchNorm3d(4).to(dev).eval()(x))
    x2 = torch.randn(2, 3, 1, 1, 1, generator=torch.Generator().manual_seed(3401)).to(dev)
    for layer in (nn.InstanceNorm3d(3), InstanceNorm3d(3)):
        with pytest.raises(ValueError, match="more than 1 spatial element"):
            layer.to(dev)(x2)


def groupnorm_odd_row(dev):
    """network.GroupNorm.planar_forward on (1, 6, 7, 11, 13) with 2 groups — rows of 3 * 1001 = 3003 elements, the scalar branch — against a float64 restatement:
    output and all gradients."""
    from deformablelka_amd.network import GroupNorm
    shape, G = (1, 6, 7, 11, 13), 2
    C = shape[1]
    g = torch.Generator().manual_seed(3500)
    a = GroupNorm(G, C)
    with torch.no_grad():
        a.weight.copy_(torch.randn(C, generator=g) * 0.3 + 1.0)
        a.bias.copy_(torch.randn(C, generator=g) * 0.2)
    x = torch.randn(shape, generator=g) * 1.7 + 0.4
    x[:, 0] += 30.0                       # a channel far from its group's mean
    gy = torch.randn(shape, generator=g)
    xr, wr, br = (t.detach().double().requires_grad_(True) for t in (x, a.weight, a.bias))
    xd = xr.view(shape[0], G, -1)
    xh = ((xd - xd.mean(-1, keepdim=True)) / torch.sqrt(xd.var(-1, unbiased=False, keepdim=True) + a.eps)).view(shape)
    yr = xh * wr.view(1, C, 1, 1, 1) + br.view(1, C, 1, 1, 1)
    yr.backward(gy.double())
    a = a.to(dev)
    xa = x.to(dev).requires_grad_(True)
    y = a.planar_forward(xa)
    y.backward(gy.to(dev))
    assert_close("GroupNorm 3003-element rows y", y, yr, *BN_TOL["y"])
    assert_close("GroupNorm 3003-element rows gx", xa.grad, xr.grad, *_scaled(BN_TOL["gx"], xr.grad))
    assert_close("GroupNorm 3003-element rows gw", a.weight.grad, wr.grad, *BN_TOL["gw"])
    assert_close("GroupNorm 3003-element rows gb", a.bias.grad, br.grad, *BN_TOL["gb"])


def batchnorm_transposed_and_wrong_dtype(dev):
    """The entries take a non-contiguous x / grad_out (they make them contiguous, as ops.gelu_forward does) and refuse what is not float32."""
    shape = (2, 3, 7, 4, 5)
    g = torch.Generator().manual_seed(3600)
    x = torch.randn(shape, generator=g).transpose(2, 4)
    x[:, 1] = x[:, 1] * 0.01 + 300.0
    w, b, _ = _bn_params(3, True, (1,), g)
    gy = torch.randn(shape, generator=g).transpose(2, 4)
    assert not x.is_contiguous() and not gy.is_contiguous()
    ref = bn_reference(x, w, b, gy)
    check_batchnorm(dev, "bn transposed", x, w, b, gy, ref)
    xc = x.contiguous().to(dev)
    for bad in (torch.float64, torch.bfloat16):
        with pytest.raises(RuntimeError, match="float32"):
            ops.batchnorm_planar_forward(xc.to(bad), None, None, EPS)
    _, stats = ops.batchnorm_planar_forward(xc, None, None, EPS)
    with pytest.raises(RuntimeError, match="float32"):
        ops.batchnorm_planar_backward(xc.double(), xc, None, stats, False)
    with pytest.raises(RuntimeError, match="float32"):
        ops.batchnorm_planar_backward(xc, xc.double(), None, stats, False)


# ---- 4. pointwise planar kernels -----------------------------------------------------------------------------------------------------------------------------------
PW_COUT_TRAINED = (1, 2, 14, 16)
PW_PAIRS = [(ci, co) for ci in ops.PLANAR_PW_CIN for co in PW_COUT_TRAINED]
PW_FORWARD_ONLY = [(ci, co) for co in (3, 33, 64) for ci in (1, 14, 32)]
PW_SPATIAL = (1, 4, 257)                              # N = 1028, N % 16 == 4: the weight gradient runs chunk = 1024 in two workgroups, the second holds four voxels
PW_TAILS = [4, 8, 12, 1032, 1036]                     # with (16, 14): every ragged MFMA tail, alone in its workgroup and behind 1024 voxels
PW_NCT4 = [(ci, co) for ci in (33, 48, 64) for co in (5, 16)]
# B, (Cin, Cout), spatial — and the voxels per workgroup launch_pl_pw_backward picks (wgrad_chunk)
PW_CHUNKS = [(16, (4, 8), (1, 4, 16385), 4096),      # N = 65540: cdiv(N, 16384) * 16 = 80 < 256 -> 4096: 17 workgroups per item (272 >= 256), the last with four voxels
             (64, (2, 4), (1, 4, 16385), 16384)]     # cdiv(N, 16384) * 64 = 320 >= 256: the chunk stays 16384, five workgroups per item, the last with four voxels


def wgrad_chunk(B, N):
    """The rule of launch_pl_pw_backward restated: a workgroup of pl_pw_bwd_weight_kernel contracts `chunk` voxels of one batch item — four waves, chunk / 4 each,
    a multiple of 16 per wave as the 16x16x4 MFMA wants — and ends with one atomic per output.  Long runs mean few atomics; but B * cdiv(N, chunk) workgroups must
    cover the chip's 256 CUs, so the chunk starts at 16384 and is quartered while that product stays under 256, down to 1024 (256 voxels per wave)."""
    chunk = 16384
    while chunk > 1024 and -(-N // chunk) * B < 256:
        chunk //= 4
    return chunk


@functools.lru_cache(maxsize=8)
def _pw_case(B, cin, cout, spatial):
    g = torch.Generator().manual_seed(4000 + 131 * cin + 7 * cout + math.prod(spatial) + B)
    x = torch.randn((B, cin) + spatial, generator=g)
    w = torch.randn(cout, cin, 1, 1, 1, generator=g) / math.sqrt(cin)
    b = torch.randn(cout, generator=g)
    gy = torch.randn((B, cout) + spatial, generator=g)
    xd, wd, gd = x.double().flatten(2), w.double().view(cout, cin), gy.double().flatten(2)
    y0 = torch.matmul(wd, xd)
    ref = {"y_nobias": y0.view(gy.shape), "y": (y0 + b.double().view(1, -1, 1)).view(gy.shape), "gx": torch.matmul(wd.t(), gd).view(x.shape),
           "gw": torch.einsum("bon,bin->oi", gd, xd).view(w.shape), "gb": gd.sum((0, 2))}
    return x, w, b, gy, ref


def _pw_check_backward(dev, what, case, need):
    x, w, b, gy, ref = case
    got = ops.pointwise_planar_backward(x.to(dev), w.to(dev), gy.to(dev), need)
    for name, t, n in zip(("gx", "gw", "gb"), got, need):
        assert (t is not None) == bool(n), f"{what}: {name} {'missing' if n else 'returned without being asked for'}"
        if n:
            assert_close(f"{what} {name}", t, ref[name], *_scaled(PW_TOL[name], ref[name]))


def pointwise(dev, B, cin, cout, spatial):
    """Forward and all three gradients, with and without bias."""
    case = _pw_case(B, cin, cout, spatial)
    x, w, b, gy, ref = case
    what = f"pw {cin}->{cout} B={B} N={math.prod(spatial)}"
    assert ops.pointwise_planar_supported(x, w)
    xd, wd = x.to(dev), w.to(dev)
    assert_close(f"{what} y", ops.pointwise_planar_forward(xd, wd, b.to(dev)), ref["y"], *PW_TOL["y"])
    assert_close(f"{what} y (no bias)", ops.pointwise_planar_forward(xd, wd, None), ref["y_nobias"], *PW_TOL["y"])
    _pw_check_backward(dev, what, case, (True, True, True))
    _pw_check_backward(dev, what + " (no bias)", case, (True, True, False))


def pointwise_forward_only(dev, cin, cout):
    """Cout outside the gradient kernels' menu: inference only."""
    x, w, b, gy, ref = _pw_case(2, cin, cout, PW_SPATIAL)
    with torch.no_grad():
        assert ops.pointwise_planar_supported(x.clone().requires_grad_(True), w, need_weight_grad=False)
        y = ops.pointwise_planar_forward(x.to(dev), w.to(dev), b.to(dev))
    assert not ops.pointwise_planar_supported(x, w, need_weight_grad=True)
    assert_close(f"pw {cin}->{cout} forward only y", y, ref["y"], *PW_TOL["y"])


def pointwise_chunk(dev, B, pair, spatial, chunk):
    assert wgrad_chunk(B, math.prod(spatial)) == chunk and wgrad_chunk(2, math.prod(PW_SPATIAL)) == 1024
    pointwise(dev, B, pair[0], pair[1], spatial)


def pointwise_nct4(dev, cin, cout):
    """Cin 33..64: the NCT = 4 instantiation of the weight-gradient kernel, asked for the weight and bias gradient only."""
    case = _pw_case(2, cin, cout, PW_SPATIAL)
    x, w, b, gy, _ = case
    _pw_check_backward(dev, f"pw wgrad {cin}->{cout}", case, (False, True, True))
    if cout not in ops.PLANAR_PW_CIN:   # no data-gradient kernel holds that many grad_out channels
        with pytest.raises(RuntimeError, match="unsupported"):
            ops.pointwise_planar_backward(x.to(dev), w.to(dev), gy.to(dev), (True, True, True))


def pointwise_wgrad_refuses_cout_17(dev):
    x, w, b, gy, _ = _pw_case(2, 33, 17, PW_SPATIAL)
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.pointwise_planar_backward(x.to(dev), w.to(dev), gy.to(dev), (False, True, True))


def pointwise_unaligned_falls_back(dev):
    """N % 4 != 0: pointwise_planar_supported is False, the entry refuses, network.Convolution falls back and equals the float64 matmul: output and all gradients."""
    from deformablelka_amd.network import Convolution
    cin, cout, spatial = 16, 14, (3, 5, 7)
    x, w, b, gy, ref = _pw_case(2, cin, cout, spatial)
    assert not ops.pointwise_planar_supported(x, w)
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.pointwise_planar_forward(x.to(dev), w.to(dev), b.to(dev))
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.pointwise_planar_backward(x.to(dev), w.to(dev), gy.to(dev))
    conv = Convolution(cin, cout, 1, 1, bias=True)
    with torch.no_grad():
        conv.conv.weight.copy_(w)
        conv.conv.bias.copy_(b)
    conv = conv.to(dev)
    xa = x.clone().to(dev).requires_grad_(True)   # (a clone: on the emulator .to() is the cached host tensor itself)
    y = conv(xa)
    y.backward(gy.to(dev))
    assert_close("Convolution 16->14 N=105 y", y, ref["y"], *PW_TOL["y"])
    for name, t in (("gx", xa.grad), ("gw", conv.conv.weight.grad), ("gb", conv.conv.bias.grad)):
        assert_close(f"Convolution 16->14 N=105 {name}", t, ref[name], *_scaled(PW_TOL[name], ref[name]))


# ---- 5. GELU -------------------------------------------------------------------------------------------------------------------------------------------------------
GELU_SIZES = [1, 255, 257, 2048 * 256 + 3]    # the last wraps the grid-stride loop
GELU_SIZES_SMALL = GELU_SIZES[:3]


@functools.lru_cache(maxsize=None)
def _gelu_case(n, bf16):
    g = torch.Generator().manual_seed(5000 + n)
    x, gy = torch.randn(n, generator=g) * 3, torch.randn(n, generator=g)
    if bf16:
        x, gy = x.bfloat16(), gy.bfloat16()
    xr = x.double().requires_grad_(True)
    yr = 0.5 * xr * torch.erfc(-xr / math.sqrt(2.0))    # x Phi(x) with Phi as erfc: 1 + erf cancels in double too (no bit of it is left below x = -8.3)
    yr.backward(gy.double())
    return x, gy, yr.detach(), xr.grad


def gelu_f32(dev, n):
    x, gy, yr, gxr = _gelu_case(n, False)
    assert_close(f"gelu n={n} y", ops.gelu_forward(x.to(dev)), yr, 1e-5, 1e-6)
    assert_close(f"gelu n={n} gx", ops.gelu_backward(x.to(dev), gy.to(dev)), gxr, 1e-5, 1e-5)


def _assert_within_one_bf16_ulp(what, got, ref):
    assert got.dtype == torch.bfloat16 and got.shape == ref.shape
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all())
    ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126))) - 7)    # (2^-126: below it the spacing stays 2^-133, bf16's smallest subnormal)
    ratio = ((got - ref).abs() / ulp).flatten()
    at = int(ratio.argmax())
    print(f"[{what}] max |err| / ulp_bf16(ref) = {float(ratio[at]):.3f} at element {at} (got {float(got.flatten()[at]):.6g}, ref {float(ref.flatten()[at]):.6g}); "
          f"{int((ratio > 1).sum())} of {ratio.numel()} elements beyond one ulp")
    assert float(ratio[at]) <= 1.0, f"{what}: {int((ratio > 1).sum())} of {ratio.numel()} elements are more than one bf16 ulp from the reference, the worst {float(ratio[at]):.3f} ulp"


def gelu_bf16(dev, n):
    """bf16 in, bf16 out, against the float64 GELU of the bf16 values, within one bf16 ulp of the reference value — which scales with the value: with x = 3 randn
    about 5 % of the elements lie below -4.5, where Phi(x) formed as 0.5 (1 + erff(x / sqrt 2)) keeps no bit of it (the stand-alone kernels used to return -0
    for references of -1e-8 .. -1e-38, up to 253 ulp; csrc/eltwise.hip now takes erfcf there)."""
    x, gy, yr, gxr = _gelu_case(n, True)
    failures = []
    for what, got, ref in ((f"gelu bf16 n={n} y", ops.gelu_forward(x.to(dev)), yr), (f"gelu bf16 n={n} gx", ops.gelu_backward(x.to(dev), gy.to(dev)), gxr)):
        try:
            _assert_within_one_bf16_ulp(what, got, ref)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)
