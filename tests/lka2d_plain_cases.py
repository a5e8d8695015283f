"""Shared cases of tests/test_lka2d_plain_emu.py and tests/test_lka2d_plain_gpu.py: the plain (non-deformable) 2-D LKA block — csrc/cl_dw2d.hip,
csrc/capi_lka2d_plain_cl.hip, deformablelka_amd/ops/lka2d_plain.py, LKA.py, decoder2d_lka.py.

The oracle is written here from torch.nn.functional (conv2d, gelu, layer_norm) in float64 on the CPU, computed once per case (functools.lru_cache) and never
written to.  The bounds are the contract's, imported from tests/parity.py and not restated: FWD_ATOL on outputs, BWD_RTOL of max |reference| on every
gradient, BF16_RTOL of max |reference| where the activations are bf16 storage.  Inputs are seeded randn, depthwise weights ~ N(0, 1 / k^2): one missing or
misplaced tap moves a border output by a few 1e-2.

Operator level: the two depthwise members through ops.lka2d_plain.dwconv2d_{forward,backward}_cl with guard bands — x and grad_out are views inside 1e30-filled
allocations (a read the range check should have answered with 0 shows as a huge error; two images, so a read that bleeds across the batch meets real data of the
wrong image and misses the reference), the outputs the wrappers allocate are views inside NaN-filled ones (partial_grad_cases.Guarded): no element may stay NaN, no
guard cell may change.

The state_dict key lists below were written once from the reference's constructors (2D/deformable_LKA/LKA.py:4-28, 2D/networks/MaxViT_LKA_Decoder.py:27-111,
449-529) and are plain names."""
import functools
from unittest import mock

import torch
import torch.nn.functional as F

from deformablelka_amd.ops import lka2d_plain
from tests import parity
from tests.partial_grad_cases import GUARD_MIN, Guarded, assert_matches

POISON = 1e30
K5 = (5, 2, 1)    # kernel, padding, dilation: conv0
K7 = (7, 9, 3)    # conv_spatial

# (B, C, H, W), dtype
OP_SHAPES = [
    ((2, 32, 5, 7), "f32"),      # every 7x7-dil-3 tap row partly outside; two images: bleed across the batch
    ((1, 32, 19, 13), "f32"),    # H = 2 * 9 + 1 exactly; ragged W
    ((2, 96, 6, 33), "f32"),     # C / 32 = 3; W past one tile (five 8-wide runs, the last with one pixel)
    ((1, 64, 1, 40), "f32"),     # a single row
    ((1, 32, 23, 23), "bf16"),   # bf16 activations
]
OP_CASES = [(shape, dt, conv) for shape, dt in OP_SHAPES for conv in (K5, K7)]
MEMBER = {("f32", 5): "cl_dw2d_kernel<float, 5, 1, 8>", ("f32", 7): "cl_dw2d_kernel<float, 7, 3, 8>",
          ("bf16", 5): "cl_dw2d_kernel<bf16_t, 5, 1, 8>", ("bf16", 7): "cl_dw2d_kernel<bf16_t, 7, 3, 8>"}

# (B, C, H, W), mode: "f32" fused | "bf16" fused under torch.autocast | "per_op" (C / 32 outside the fused set)
BLOCK_CASES = [((2, 32, 7, 9), "f32"), ((2, 96, 14, 14), "f32"), ((2, 64, 14, 14), "bf16"), ((2, 48, 7, 9), "per_op"),
               ((1, 192, 6, 5), "f32"), ((1, 384, 5, 4), "bf16")]    # the two widest decoder widths: 6 and 12 column tiles in the pointwise kernels

ATTENTION_KEYS = ["proj_1.weight", "proj_1.bias", "spatial_gating_unit.conv0.weight", "spatial_gating_unit.conv0.bias",
                  "spatial_gating_unit.conv_spatial.weight", "spatial_gating_unit.conv_spatial.bias", "spatial_gating_unit.conv1.weight",
                  "spatial_gating_unit.conv1.bias", "proj_2.weight", "proj_2.bias"]
BLOCK_KEYS = (["layer_scale_1", "layer_scale_2", "norm1.weight", "norm1.bias"] + ["attn." + k for k in ATTENTION_KEYS] + ["norm2.weight", "norm2.bias"]
              + ["mlp.fc1.weight", "mlp.fc1.bias", "mlp.dwconv.dwconv.weight", "mlp.dwconv.dwconv.bias", "mlp.fc2.weight", "mlp.fc2.bias"])
DECODER_KEYS = (["x1_linear.weight", "x1_linear.bias", "concat_linear.weight", "concat_linear.bias", "layer_up.expand.weight", "layer_up.norm.weight",
                 "layer_up.norm.bias"] + ["layer_lka_1." + k for k in BLOCK_KEYS] + ["layer_lka_2." + k for k in BLOCK_KEYS])
DECODER_LAST_KEYS = DECODER_KEYS[:7] + ["last_layer.weight", "last_layer.bias"] + DECODER_KEYS[7:]


def case_id(c):
    return "-".join("x".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in c)


def to_cl(t):    # [B,C,H,W] -> [B,H,W,C]
    return t.permute(0, 2, 3, 1).contiguous()


# ---- operator level -----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _op_host(shape, dtype, conv):
    """Seeded channels-last x and grad_out (bf16: rounded to bf16, what the kernel sees) and F.conv2d in float64: out and the three gradients."""
    B, C, H, W = shape
    k, p, d = conv
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(B, C, H, W, generator=gen)
    w = torch.randn(C, 1, k, k, generator=gen) * (1.0 / k)
    b = torch.randn(C, generator=gen)
    go = torch.randn(B, C, H, W, generator=gen)
    if dtype == "bf16":
        x, go = x.bfloat16().float(), go.bfloat16().float()
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    out = F.conv2d(xr, wr, br, 1, p, d, C)
    out.backward(go.double())
    ref = {"out": to_cl(out.detach()), "grad_input": to_cl(xr.grad), "grad_weight": wr.grad, "grad_bias": br.grad}
    return to_cl(x), w, b, to_cl(go), ref


class GuardedInput:
    """`t` as a view inside an allocation that extends max(256, numel) elements — at least one row of W * C — on each side, filled with 1e30."""

    def __init__(self, t, dev):
        n = t.numel()
        self.n, self.g = n, max(GUARD_MIN, n)
        assert self.g >= t.shape[-1] * t.shape[-2]
        self.buf = torch.full((n + 2 * self.g,), POISON, dtype=t.dtype, device=dev)
        self.view = self.buf[self.g:self.g + n].view(t.shape)
        self.view.copy_(t)
        self.saved = self.buf.clone()

    def assert_unchanged(self, name):
        assert torch.equal(self.buf, self.saved), f"{name}: an input or its guard band was written"


class _GuardedAllocator:
    """Stands in for the name `torch` in deformablelka_amd/ops/lka2d_plain.py during one call: the outputs the wrappers allocate become views inside NaN-filled
    allocations with guard cells on each side; everything else is torch's."""

    def __init__(self):
        self.made = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, shape, dtype=None, device=None):
        g = Guarded(tuple(shape), dtype, device)
        self.made.append(g)
        return g.view


def run_op(dev, shape, dtype, conv, trace=False):
    """The two wrappers on guard-banded inputs with guarded outputs -> ({name: output on the CPU}, kernel names launched (None without the trace))."""
    x, w, b, go, _ = _op_host(shape, dtype, conv)
    k, p, d = conv
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    gx, ggo = GuardedInput(x.to(tdt), dev), GuardedInput(go.to(tdt), dev)
    wd, bd = w.to(dev), b.to(dev)
    alloc = _GuardedAllocator()
    got = {}

    def call():
        with mock.patch.object(lka2d_plain, "torch", alloc):
            got["out"] = lka2d_plain.dwconv2d_forward_cl(gx.view, wd, bd, p, d)
            got["grad_input"], got["grad_weight"], got["grad_bias"] = lka2d_plain.dwconv2d_backward_cl(gx.view, wd, ggo.view, p, d)

    names = parity.kernels_launched(call) if trace else call()
    what = case_id((shape, dtype, conv))
    assert len(alloc.made) == 4, f"{what}: {len(alloc.made)} outputs were allocated through the wrappers, expected 4"
    for g, name in zip(alloc.made, ("out", "grad_input", "grad_weight", "grad_bias")):
        g.assert_guards_untouched(f"{what} {name}")
    gx.assert_unchanged(f"{what} x")
    ggo.assert_unchanged(f"{what} grad_out")
    assert got["out"].dtype == got["grad_input"].dtype == tdt and got["grad_weight"].dtype == got["grad_bias"].dtype == torch.float32
    return {n: t.detach().float().cpu().clone() for n, t in got.items()}, names


def compare_op(shape, dtype, conv, got):
    """fp32: the contract.  bf16 activations: out and grad_input are bf16 STORAGE of an fp32 sum — per element 2^-8 |ref| + the fp32 bound
    (partial_grad_cases' "bf16" mode); grad_weight / grad_bias are fp32 sums over the bf16-rounded inputs the reference also saw: the fp32 contract."""
    ref = _op_host(shape, dtype, conv)[4]
    what = case_id((shape, dtype, conv))
    failures = []
    for name in ("out", "grad_input", "grad_weight", "grad_bias"):
        mode = "bf16" if dtype == "bf16" and name in ("out", "grad_input") else "f32"
        try:
            assert_matches(f"{what} {name}", got[name], ref[name], mode, forward=(name == "out"))
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)


def single_op(dev, shape, dtype, conv, trace=False):
    got, names = run_op(dev, shape, dtype, conv, trace)
    if trace:
        dw = sorted(n for n in names if n.startswith("cl_dw2d") or n.startswith("cl_ddw2d") or n.startswith("cl_dwconv"))
        t = "bf16_t" if dtype == "bf16" else "float"
        k, _, d = conv
        print(f"[{case_id((shape, dtype, conv))}] launched: {', '.join(dw)}")
        assert dw == sorted([MEMBER[(dtype, k)], f"cl_dw2d_wgrad_kernel<{t}, {k}, {d}, 8>"]), dw
    compare_op(shape, dtype, conv, got)
    return got


# ---- block level ----------------------------------------------------------------------------------------------------------------------------------------
def attention_f64(x, P, prefix=""):
    """LKA_Attention restated in float64: y = proj_2(u * conv1(conv_spatial(conv0(u)))) + x, u = GELU(proj_1 x).  P: name -> tensor (state_dict keys)."""
    g = lambda k: P[prefix + k]
    C = x.shape[1]
    u = F.gelu(F.conv2d(x, g("proj_1.weight"), g("proj_1.bias")))
    a = F.conv2d(u, g("spatial_gating_unit.conv0.weight"), g("spatial_gating_unit.conv0.bias"), 1, 2, 1, C)
    a = F.conv2d(a, g("spatial_gating_unit.conv_spatial.weight"), g("spatial_gating_unit.conv_spatial.bias"), 1, 9, 3, C)
    a = F.conv2d(a, g("spatial_gating_unit.conv1.weight"), g("spatial_gating_unit.conv1.bias"))
    return F.conv2d(u * a, g("proj_2.weight"), g("proj_2.bias")) + x


def block_f64(x, H, W, P, prefix=""):
    """LKABlock restated in float64 (tokens [B, N, C])."""
    g = lambda k: P[prefix + k]
    B, N, C = x.shape
    x = x.permute(0, 2, 1).reshape(B, C, H, W)
    y = F.layer_norm(x.permute(0, 2, 3, 1), (C,), g("norm1.weight"), g("norm1.bias")).permute(0, 3, 1, 2)
    x = x + g("layer_scale_1")[None, :, None, None] * attention_f64(y, P, prefix + "attn.")
    y = F.layer_norm(x.permute(0, 2, 3, 1), (C,), g("norm2.weight"), g("norm2.bias")).permute(0, 3, 1, 2)
    hid = g("mlp.fc1.weight").shape[0]
    y = F.conv2d(y, g("mlp.fc1.weight"), g("mlp.fc1.bias"))
    y = F.gelu(F.conv2d(y, g("mlp.dwconv.dwconv.weight"), g("mlp.dwconv.dwconv.bias"), 1, 1, 1, hid))
    y = F.conv2d(y, g("mlp.fc2.weight"), g("mlp.fc2.bias"))
    x = x + g("layer_scale_2")[None, :, None, None] * y
    return x.reshape(B, C, N).permute(0, 2, 1)


def _attention_state(C, seed):
    """Seeded parameters under the state_dict keys: 1x1 weights ~ N(0, 1/C), depthwise ~ N(0, 1/k^2), biases ~ N(0, 0.1^2)."""
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen)
    P = {}
    for name in ("proj_1", "spatial_gating_unit.conv1", "proj_2"):
        P[name + ".weight"], P[name + ".bias"] = r(C, C, 1, 1) / C ** 0.5, 0.1 * r(C)
    P["spatial_gating_unit.conv0.weight"], P["spatial_gating_unit.conv0.bias"] = r(C, 1, 5, 5) / 5, 0.1 * r(C)
    P["spatial_gating_unit.conv_spatial.weight"], P["spatial_gating_unit.conv_spatial.bias"] = r(C, 1, 7, 7) / 7, 0.1 * r(C)
    return {k: P[k] for k in ATTENTION_KEYS}


@functools.lru_cache(maxsize=None)
def _attention_host(shape, seed=0):
    B, C, H, W = shape
    P = _attention_state(C, 20 + seed)
    gen = torch.Generator().manual_seed(30 + seed)
    x, gy = torch.randn(B, C, H, W, generator=gen), torch.randn(B, C, H, W, generator=gen)
    Pr = {k: v.double().requires_grad_(True) for k, v in P.items()}
    xr = x.double().requires_grad_(True)
    y = attention_f64(xr, Pr)
    y.backward(gy.double())
    ref = {"y": y.detach(), "grad_x": xr.grad}
    ref.update({k: v.grad for k, v in Pr.items()})
    return x, gy, P, ref


def run_attention(dev, shape, mode):
    """LKA_Attention fwd + bwd on `dev` -> {"y", "grad_x", the ten state_dict keys: gradients} on the CPU."""
    from deformablelka_amd.LKA import LKA_Attention
    x, gy, P, _ = _attention_host(shape)
    m = LKA_Attention(shape[1])
    m.load_state_dict(P, strict=True)
    m = m.to(dev)
    xd = x.clone().to(dev).requires_grad_(True)
    assert m.fused(xd) == (mode != "per_op")
    if mode == "bf16":
        with torch.autocast(torch.device(dev).type, dtype=torch.bfloat16):
            y = m(xd)
        assert y.dtype == torch.bfloat16
    else:
        y = m(xd)
        assert y.dtype == torch.float32
    y.backward(gy.to(dev).to(y.dtype))
    got = {"y": y.detach().float().cpu(), "grad_x": xd.grad.float().cpu()}
    for k, p in m.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32, k
        got[k] = p.grad.cpu().clone()
    return got


def compare_attention(shape, mode, got):
    """fp32 (fused or per-op): FWD_ATOL on y, BWD_RTOL of max |ref| on grad_x and all ten parameter gradients.  bf16 activations: parity.BF16_RTOL of
    max |ref| on everything, as parity.check_lka2d_attention_bf16 holds the deformable block."""
    ref = _attention_host(shape)[3]
    what = case_id((shape, mode))
    assert set(got) == set(ref) and len(got) == 12
    failures = []
    for name in ref:
        try:
            assert_matches(f"{what} {name}", got[name], ref[name], "cl_bf16" if mode == "bf16" else "f32", forward=(name == "y"))
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)


def lkablock_state(dim, seed):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen)
    hid = 4 * dim
    P = {"layer_scale_1": 0.5 + 0.1 * r(dim), "layer_scale_2": 0.5 + 0.1 * r(dim), "norm1.weight": 1 + 0.1 * r(dim), "norm1.bias": 0.1 * r(dim)}
    P.update({"attn." + k: v for k, v in _attention_state(dim, seed + 1).items()})
    P.update({"norm2.weight": 1 + 0.1 * r(dim), "norm2.bias": 0.1 * r(dim), "mlp.fc1.weight": r(hid, dim, 1, 1) / dim ** 0.5, "mlp.fc1.bias": 0.1 * r(hid),
              "mlp.dwconv.dwconv.weight": r(hid, 1, 3, 3) / 3, "mlp.dwconv.dwconv.bias": 0.1 * r(hid), "mlp.fc2.weight": r(dim, hid, 1, 1) / hid ** 0.5,
              "mlp.fc2.bias": 0.1 * r(dim)})
    return {k: P[k] for k in BLOCK_KEYS}


@functools.lru_cache(maxsize=None)
def _lkablock_host(B, H, W, dim):
    P = lkablock_state(dim, 40)
    gen = torch.Generator().manual_seed(41)
    x, gy = torch.randn(B, H * W, dim, generator=gen), torch.randn(B, H * W, dim, generator=gen)
    Pr = {k: v.double().requires_grad_(True) for k, v in P.items()}
    xr = x.double().requires_grad_(True)
    y = block_f64(xr, H, W, Pr)
    y.backward(gy.double())
    ref = {"y": y.detach(), "grad_x": xr.grad}
    ref.update({k: v.grad for k, v in Pr.items()})
    return x, gy, P, ref


def lkablock(dev, B=2, H=7, W=9, dim=32):
    """LKABlock on tokens (B, H W, dim) against the float64 restatement at the bounds the deformableLKABlock goldens are replayed at
    (golden_checks.replay: forward FWD_ATOL, every gradient BWD_RTOL of max |reference|)."""
    from deformablelka_amd.decoder2d_lka import LKABlock
    x, gy, P, ref = _lkablock_host(B, H, W, dim)
    m = LKABlock(dim)
    m.load_state_dict(P, strict=True)
    m = m.to(dev)
    xd = x.clone().to(dev).requires_grad_(True)
    y = m(xd, H, W)
    y.backward(gy.to(dev))
    assert_matches("LKABlock y", y.detach().cpu(), ref["y"], "f32", forward=True)
    assert_matches("LKABlock grad_x", xd.grad.cpu(), ref["grad_x"], "f32")
    for k, p in m.named_parameters():
        assert_matches(f"LKABlock grad {k}", p.grad.cpu(), ref[k], "f32")
