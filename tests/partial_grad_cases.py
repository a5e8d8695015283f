"""Shared cases of tests/test_partial_grad_emu.py and tests/test_partial_grad_gpu.py: the single-operator backward entry points of the C-ABI asked for a
SUBSET of their gradients (a null pointer for every gradient the caller does not want), and the bf16 instantiations of the general operators and of the
channels-last deformable conv — neither is reached by the fused blocks the rest of the suite drives.

Every call goes to the library entry directly, the way deformablelka_amd/ops.py does, with outputs this module owns: each requested gradient lives inside
a larger tensor with max(256, numel) guard elements on each side, the whole tensor and the workspace are filled with NaN before the call (a caching
allocator would otherwise hand back the block a previous full call filled with the right answer).  After the call the guards are compared bitwise with a
saved copy, the outputs hold no NaN, and they match the oracle (ATen in double for the plain convs) at

  fp32   parity.FWD_ATOL (forward, max abs) / parity.BWD_RTOL (every gradient, max abs error over max |reference|) — the contract, unchanged
  f64    1e-12 of max |reference| (tests/f64_checks.py), the oracle run in double
  bf16   general operators (fp32 arithmetic, ONE rounding at the store or cast): per element |got - ref| <= 2^-8 |ref| + t, t = FWD_ATOL for the forward,
         BWD_RTOL max|ref| for a gradient; 2^-8 is one bf16 ulp (half an ulp of rounding + an fp32 difference that moves the value across a rounding boundary)
  bf16   channels-last deformable conv (bf16 x / out / grad_out, everything else fp32): the four fp32 gradients 2e-2 of max |reference| (parity.BF16_RTOL,
         the bar of check_lka3d_tokens_bf16 for this mode); `out`, bf16 storage, per element as above

the reference being computed once per case (functools.lru_cache) on the same — for bf16: the bf16-rounded — inputs and never written to."""
import functools
import itertools
from ctypes import byref

import torch
import torch.nn.functional as F

import oracle
from deformablelka_amd import _lib as L
from deformablelka_amd import ops
from tests import parity

GUARD_MIN = 256
F64_RTOL = 1e-12          # tests/f64_checks.py
BF16_ULP = 2.0 ** -8
DTYPES = {"f32": torch.float32, "f64": torch.float64, "bf16": torch.bfloat16}
_BITS = {torch.float32: torch.int32, torch.float64: torch.int64, torch.bfloat16: torch.int16}

NAMES4 = ("grad_input", "grad_offset", "grad_weight", "grad_bias")
NAMES3 = ("grad_input", "grad_weight", "grad_bias")
NAMES2D = ("grad_input", "grad_offset", "grad_weight")


def subsets(n):
    """Every non-empty subset of n outputs as a `need` tuple; the full set first."""
    return sorted((s for s in itertools.product((True, False), repeat=n) if any(s)), key=lambda s: -sum(s))


SUBSETS3, SUBSETS4 = subsets(3), subsets(4)
SINGLES3, SINGLES4 = [s for s in SUBSETS3 if sum(s) == 1], [s for s in SUBSETS4 if sum(s) == 1]


def need_id(need):
    return "".join(c if n else "-" for c, n in zip("iowb" if len(need) == 4 else "iwb", need))


def need_id2d(need):
    return "".join(c if n else "-" for c, n in zip("iowb", need))


def case_id(c):
    return "-".join("x".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in c)


# ---- poisoned, guarded outputs ------------------------------------------------------------------------------------------------------------------------
class Guarded:
    """An output of `shape` inside a NaN-filled tensor with max(256, numel) guard elements on each side (a writer of elements twice as wide as `dtype` still
    ends inside the tensor: the guard check fails, the heap survives)."""

    def __init__(self, shape, dtype, dev):
        n = 1
        for v in shape:
            n *= int(v)
        self.n, self.g = n, max(GUARD_MIN, n)
        self.buf = torch.full((n + 2 * self.g,), float("nan"), dtype=dtype, device=dev)
        self.view = self.buf[self.g:self.g + n].view(*shape)
        self.saved = self.buf.view(_BITS[dtype]).clone()

    def assert_guards_untouched(self, name):
        bits = self.buf.view(_BITS[self.buf.dtype])
        assert torch.equal(bits[:self.g], self.saved[:self.g]), f"{name}: the guard in front of the output was written"
        assert torch.equal(bits[self.g + self.n:], self.saved[self.g + self.n:]), f"{name}: the guard behind the output was written"

    def assert_untouched(self, name):
        assert torch.equal(self.buf.view(_BITS[self.buf.dtype]), self.saved), f"{name}: written by a call the library refused"


def poisoned_workspace(nbytes, like):
    """All-ones bytes: a NaN in every float format the library carves accumulators in."""
    return L.scratch(nbytes, like).fill_(0xFF)


def call_guarded(what, dev, spec, need, launch, expect_rc=0):
    """spec: (name, shape, dtype) per output of the entry, need: which of them to ask for; launch(ptrs) -> status.  Returns {name: tensor on the CPU} of the
    requested outputs after the guard check (expect_rc != 0: the library must refuse with that status and leave every output as it was)."""
    outs, ptrs = {}, []
    for (name, shape, dtype), n in zip(spec, need):
        if n:
            outs[name] = Guarded(shape, dtype, dev)
        ptrs.append(L.ptr(outs[name].view if n else None))
    rc = launch(ptrs)
    if expect_rc:
        assert rc == expect_rc, f"{what}: status {rc}, expected {expect_rc}"
        for name, o in outs.items():
            o.assert_untouched(f"{what} {name}")
        return None
    L.check(rc, what)
    res = {}
    for name, o in outs.items():
        o.assert_guards_untouched(f"{what} {name}")
        res[name] = o.view.detach().cpu().clone()
    return res


# ---- comparison ---------------------------------------------------------------------------------------------------------------------------------------
def assert_matches(what, got, ref, mode, forward=False):
    """mode: "f32" | "f64" | "bf16" (per element) | "cl_bf16" (2e-2 of max |ref|).  Prints the measured figure before it asserts."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert not torch.isnan(got).any(), f"{what}: {int(torch.isnan(got).sum())} of {got.numel()} elements were never written (NaN poison)"
    got, ref = got.double(), ref.double()
    err, scale = (got - ref).abs(), max(float(ref.abs().max()), 1e-6)
    if mode == "bf16":
        t = parity.FWD_ATOL if forward else parity.BWD_RTOL * scale
        bound = BF16_ULP * ref.abs() + t
        ratio = (err / bound).flatten()
        at = int(ratio.argmax())
        worst = float(ratio[at])
        print(f"[{what}] bf16: max |err| / (2^-8 |ref| + {t:.1e}) = {worst:.3f} (there: err {float(err.flatten()[at]):.3e}, ref {float(ref.flatten()[at]):.3e}); "
              f"max abs err {float(err.max()):.3e}, max |ref| {scale:.3e}")
        assert worst <= 1.0, f"{what}: |got - ref| exceeds 2^-8 |ref| + {t:.1e} by a factor {worst:.3f}"
        return worst
    if forward and mode == "f32":
        print(f"[{what}] max abs err {float(err.max()):.3e}")
        assert float(err.max()) <= parity.FWD_ATOL, f"{what}: max abs err {float(err.max()):.3e} > {parity.FWD_ATOL}"
        return float(err.max())
    rtol = {"f32": parity.BWD_RTOL, "f64": F64_RTOL, "cl_bf16": parity.BF16_RTOL}[mode]
    rel = float(err.max()) / scale
    print(f"[{what}] {mode}: max rel err {rel:.3e} (bar {rtol:.0e})")
    assert rel <= rtol, f"{what}: max rel err {rel:.3e} > {rtol}"
    return rel


def _check_all(what, got, ref, mode):
    return {name: assert_matches(f"{what} {name}", t, ref[name], mode) for name, t in got.items()}


def _dev_inputs(dev, tensors, dtype):
    return [None if t is None else t.to(DTYPES[dtype]).to(dev).contiguous() for t in tensors]


def _rounded(tensors, dtype):
    """What the kernels see: for bf16 the bf16-rounded values widened again, for f64 the fp32 values widened."""
    rt = torch.float64 if dtype == "f64" else torch.float32
    return [None if t is None else t.to(DTYPES[dtype]).to(rt) for t in tensors]


# ---- general NCDHW 3-D deformable conv ----------------------------------------------------------------------------------------------------------------
# B, C, Cout, dims, k, s, p, d, g, dg, off_mode
DEFORM3D = [
    (2, 4, 6, (7, 6, 5), (3, 2, 3), (2, 1, 1), (1, 0, 1), (1, 2, 1), 2, 2, "wild"),   # ragged, grouped: the generic OGR == 0 kernel
    (1, 40, 36, (3, 4, 5), 3, 1, 1, 1, 1, 1, "normal"),                                # Og > 32
    (1, 8, 8, (5, 5, 5), 3, 1, 1, 1, 1, 1, "integer"),                                 # the register path, OGR = 8
]
DEFORM3D_BF16 = [DEFORM3D[2], DEFORM3D[1]]


@functools.lru_cache(maxsize=None)
def _deform3d_host(case, dtype):
    *cfg, mode = case
    x, off, w, b, go, geo = parity.make_deform3d(*cfg, off_mode=mode, seed=3)
    xr, offr, wr, br, gor = _rounded((x, off, w, b, go), dtype)
    k3, s3, p3, d3 = geo
    ref = dict(zip(NAMES4, oracle.deform_conv3d_backward(xr, wr, br, offr, gor, s3, p3, d3, cfg[8], cfg[9], q1_literal=False)))
    ref["out"] = oracle.deform_conv3d_forward(xr, wr, br, offr, s3, p3, d3, cfg[8], cfg[9])
    return (x, off, w, b, go), geo, ref


@functools.lru_cache(maxsize=None)
def _deform3d_dev(dev, case, dtype):
    host, geo, _ = _deform3d_host(case, dtype)
    return _dev_inputs(dev, host, dtype), geo


def deform3d_backward(dev, case, dtype, need):
    (x, off, w, b, go), (k3, s3, p3, d3) = _deform3d_dev(dev, case, dtype)
    lib = L.get_lib()
    g = ops._geom(x.shape, w.shape[0], k3, s3, p3, d3, case[8], case[9], 64)
    dt = L.dtype_code(x, allow_f64=True)
    wsb = lib.dlka_deform_conv3d_backward_workspace(byref(g), dt)
    ws = poisoned_workspace(wsb, x)
    spec = [(n, t.shape, x.dtype) for n, t in zip(NAMES4, (x, off, w, b))]
    return call_guarded("deform3d backward", dev, spec, need, lambda p: lib.dlka_deform_conv3d_backward(
        L.ptr(x), L.ptr(off), L.ptr(w), L.ptr(go), *p, L.ptr(ws), wsb, byref(g), dt, L.stream_ptr(x)))


@functools.lru_cache(maxsize=None)
def _deform3d_full(dev, case, dtype):
    return deform3d_backward(dev, case, dtype, (True,) * 4)


def deform3d_subset(dev, case, dtype, need):
    ref = _deform3d_host(case, dtype)[2]
    got = deform3d_backward(dev, case, dtype, need)
    assert set(got) == {n for n, k in zip(NAMES4, need) if k}
    _check_all(f"deform3d {dtype} {need_id(need)}", got, ref, dtype)
    if need[1]:   # one plain store per element from the same instantiation, with or without grad_input: the same bits as the full call
        assert torch.equal(got["grad_offset"], _deform3d_full(dev, case, dtype)["grad_offset"]), "grad_offset differs from the full call's"


def deform3d_forward(dev, case, dtype):
    (x, off, w, b, go), (k3, s3, p3, d3) = _deform3d_dev(dev, case, dtype)
    lib = L.get_lib()
    g = ops._geom(x.shape, w.shape[0], k3, s3, p3, d3, case[8], case[9], 64)
    dt = L.dtype_code(x, allow_f64=True)
    wsb = lib.dlka_deform_conv3d_forward_workspace(byref(g), dt)
    ws = poisoned_workspace(wsb, x)
    got = call_guarded("deform3d forward", dev, [("out", go.shape, x.dtype)], (True,), lambda p: lib.dlka_deform_conv3d_forward(
        L.ptr(x), L.ptr(off), L.ptr(w), L.ptr(b), *p, L.ptr(ws), wsb, byref(g), dt, L.stream_ptr(x)))
    assert_matches(f"deform3d {dtype} out", got["out"], _deform3d_host(case, dtype)[2]["out"], dtype, forward=True)


# ---- general NCDHW 2-D deformable conv (torchvision semantics) ----------------------------------------------------------------------------------------
# B, C, Cout, H, W, k, s, p, d, g, og, off_mode
DEFORM2D = [
    (2, 4, 6, 7, 9, (3, 3), 2, 1, 1, 2, 2, "normal"),
    (1, 4, 4, 12, 11, (7, 7), 1, 9, 3, 4, 1, "wild"),     # depthwise, as the 2-D D-LKA block's conv_spatial
]
DEFORM2D_BF16 = [DEFORM2D[1]]


@functools.lru_cache(maxsize=None)
def _deform2d_host(case, dtype):
    *cfg, mode = case
    x, off, w, go = parity.make_deform2d(*cfg, off_mode=mode, seed=4)
    bias = torch.randn(cfg[2], generator=torch.Generator().manual_seed(5))
    xr, offr, wr, gor, br = _rounded((x, off, w, go, bias), dtype)
    s, p, d = cfg[6], cfg[7], cfg[8]
    ref = dict(zip(NAMES4, oracle.deform_conv2d_backward(xr, offr, wr, gor, s, p, d, with_bias=True)))
    ref["out"] = oracle.deform_conv2d_forward(xr, offr, wr, br, s, p, d)
    ref["out_nobias"] = oracle.deform_conv2d_forward(xr, offr, wr, None, s, p, d)
    return (x, off, w, go, bias), ref


@functools.lru_cache(maxsize=None)
def _deform2d_dev(dev, case, dtype):
    return _dev_inputs(dev, _deform2d_host(case, dtype)[0], dtype)


def deform2d_backward(dev, case, dtype, need):
    """need: (grad_input, grad_offset, grad_weight) without bias, (..., grad_bias) with."""
    x, off, w, go, bias = _deform2d_dev(dev, case, dtype)
    s, p, d = (ops._pair(v) for v in case[6:9])
    lib = L.get_lib()
    g = ops._geom2d(x.shape, w.shape, s, p, d, off.shape[1])
    dt = L.dtype_code(x, allow_f64=True)
    wsb = lib.dlka_deform_conv2d_backward_workspace(byref(g), dt)
    ws = poisoned_workspace(wsb, x)
    spec = [(n, t.shape, x.dtype) for n, t in zip(NAMES4, (x, off, w, bias))]
    need4 = tuple(need) + (False,) * (4 - len(need))
    return call_guarded("deform2d backward", dev, spec, need4, lambda q: lib.dlka_deform_conv2d_backward(
        L.ptr(x), L.ptr(off), L.ptr(w), L.ptr(go), *q, L.ptr(ws), wsb, byref(g), dt, L.stream_ptr(x)))


@functools.lru_cache(maxsize=None)
def _deform2d_full(dev, case, dtype):
    return deform2d_backward(dev, case, dtype, (True,) * 4)


def deform2d_subset(dev, case, dtype, need):
    ref = _deform2d_host(case, dtype)[1]
    got = deform2d_backward(dev, case, dtype, need)
    assert set(got) == {n for n, k in zip(NAMES4, need) if k}
    _check_all(f"deform2d {dtype} {need_id2d(need)}", got, ref, dtype)
    if need[1]:
        assert torch.equal(got["grad_offset"], _deform2d_full(dev, case, dtype)["grad_offset"]), "grad_offset differs from the full call's"


def deform2d_forward(dev, case, dtype, with_bias):
    x, off, w, go, bias = _deform2d_dev(dev, case, dtype)
    s, p, d = (ops._pair(v) for v in case[6:9])
    lib = L.get_lib()
    g = ops._geom2d(x.shape, w.shape, s, p, d, off.shape[1])
    dt = L.dtype_code(x, allow_f64=True)
    wsb = lib.dlka_deform_conv2d_forward_workspace(byref(g), dt)
    ws = poisoned_workspace(wsb, x)
    got = call_guarded("deform2d forward", dev, [("out", go.shape, x.dtype)], (True,), lambda q: lib.dlka_deform_conv2d_forward(
        L.ptr(x), L.ptr(off), L.ptr(w), L.ptr(bias if with_bias else None), *q, L.ptr(ws), wsb, byref(g), dt, L.stream_ptr(x)))
    assert_matches(f"deform2d {dtype} out", got["out"], _deform2d_host(case, dtype)[1]["out" if with_bias else "out_nobias"], dtype, forward=True)


# ---- general NCDHW plain conv -------------------------------------------------------------------------------------------------------------------------
# B, C, Cout, dims, k, s, p, d, g
CONV3D = [
    (1, 8, 12, (7, 6, 5), 3, 2, 1, 1, 2),                              # strided, grouped
    (1, 16, 16, (7, 8, 6), (3, 5, 5), 1, (1, 6, 6), (1, 3, 3), 16),    # depthwise, dilated
    (1, 12, 16, (5, 4, 40), 3, 1, 1, 1, 1),                            # the row kernels (W % 8 == 0)
]
CONV3D_BF16 = [CONV3D[0]]


def _aten_conv3d(x, w, b, go, s, p, d, g):
    """ATen in double: out and the three gradients."""
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    out = F.conv3d(xr, wr, br, s, p, d, g)
    out.backward(go.double())
    return {"out": out.detach(), "grad_input": xr.grad, "grad_weight": wr.grad, "grad_bias": br.grad}


@functools.lru_cache(maxsize=None)
def _conv3d_host(case, dtype):
    B, C, Cout, dims, k, s, p, d, g = case
    gen = torch.Generator().manual_seed(6)
    k3 = ops._triple(k)
    x = torch.randn(B, C, *dims, generator=gen)
    w = torch.randn(Cout, C // g, *k3, generator=gen) * (1.0 / (C // g * k3[0] * k3[1] * k3[2]) ** 0.5)
    b = torch.randn(Cout, generator=gen)
    oshape = F.conv3d(x, w, b, s, p, d, g).shape
    go = torch.randn(oshape, generator=gen)
    ref = _aten_conv3d(*_rounded((x, w, b, go), dtype), s, p, d, g)
    return (x, w, b, go), ref


@functools.lru_cache(maxsize=None)
def _conv3d_dev(dev, case, dtype):
    return _dev_inputs(dev, _conv3d_host(case, dtype)[0], dtype)


def _conv3d_geom(case, x, w):
    k, s, p, d, g = case[4:9]
    return ops._geom(x.shape, w.shape[0], tuple(w.shape[2:5]), ops._triple(s), ops._triple(p), ops._triple(d), g)


def conv3d_backward(dev, case, dtype, need):
    x, w, b, go = _conv3d_dev(dev, case, dtype)
    lib = L.get_lib()
    g = _conv3d_geom(case, x, w)
    dt = L.dtype_code(x, allow_f64=True)
    wsb = lib.dlka_conv3d_backward_workspace(byref(g), dt)
    ws = poisoned_workspace(wsb, x)
    spec = [(n, t.shape, x.dtype) for n, t in zip(NAMES3, (x, w, b))]
    return call_guarded("conv3d backward", dev, spec, need, lambda q: lib.dlka_conv3d_backward(
        L.ptr(x), L.ptr(w), L.ptr(go), *q, L.ptr(ws), wsb, byref(g), dt, L.stream_ptr(x)))


def conv3d_subset(dev, case, dtype, need):
    got = conv3d_backward(dev, case, dtype, need)
    assert set(got) == {n for n, k in zip(NAMES3, need) if k}
    _check_all(f"conv3d {dtype} {need_id(need)}", got, _conv3d_host(case, dtype)[1], dtype)


def conv3d_forward(dev, case, dtype):
    x, w, b, go = _conv3d_dev(dev, case, dtype)
    lib = L.get_lib()
    g = _conv3d_geom(case, x, w)
    dt = L.dtype_code(x, allow_f64=True)
    wsb = lib.dlka_conv3d_forward_workspace(byref(g), dt)
    ws = poisoned_workspace(wsb, x)
    got = call_guarded("conv3d forward", dev, [("out", go.shape, x.dtype)], (True,), lambda q: lib.dlka_conv3d_forward(
        L.ptr(x), L.ptr(w), L.ptr(b), *q, L.ptr(ws), wsb, byref(g), dt, L.stream_ptr(x)))
    assert_matches(f"conv3d {dtype} out", got["out"], _conv3d_host(case, dtype)[1]["out"], dtype, forward=True)


# ---- channels-last plain conv (fp32 only) -------------------------------------------------------------------------------------------------------------
# B, C, Cout, dims, k, p, d, g, planar grad_out
CONV_CL = [
    (1, 32, 81, (6, 6, 6), 3, 1, 1, 1, True),       # dense 3^3, the offset-predict conv: planar grad_out
    (1, 32, 32, (5, 6, 7), 1, 0, 1, 1, False),      # pointwise
    (1, 32, 32, (6, 6, 6), 5, 2, 1, 32, False),     # depthwise 5^3
    (1, 32, 32, (6, 6, 6), 7, 9, 3, 32, False),     # depthwise 7^3, dilation 3
]
CONV_CL_SPLIT_K = (2, 256, 81, (4, 4, 4), 3, 1, 1, 1, True)   # eight ci tiles on 64 rows a sample: the data gradient splits K (GPU file only)


@functools.lru_cache(maxsize=None)
def _conv_cl_host(case):
    B, C, Cout, dims, k, p, d, g, planar = case
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(B, C, *dims, generator=gen)
    w = torch.randn(Cout, C // g, k, k, k, generator=gen) * (1.0 / (C // g * k ** 3) ** 0.5)
    b = torch.randn(Cout, generator=gen)
    go = torch.randn(B, Cout, *dims, generator=gen)
    ref = _aten_conv3d(x, w, b, go, 1, p, d, g)
    ref["grad_input"] = parity.to_cl(ref["grad_input"])
    return (parity.to_cl(x), w, go if planar else parity.to_cl(go)), ref


@functools.lru_cache(maxsize=None)
def _conv_cl_dev(dev, case):
    return _dev_inputs(dev, _conv_cl_host(case)[0], "f32")


def conv_cl_backward(dev, case, need, dtype="f32", expect_rc=0):
    x, w, go = _conv_cl_dev(dev, case)
    if dtype != "f32":
        x, go = x.to(DTYPES[dtype]), go.to(DTYPES[dtype])
    B, C, Cout, dims, k, p, d, g, planar = case
    lib = L.get_lib()
    geom = ops._geom_cl(x.shape, Cout, (k, k, k), ops._triple(p), ops._triple(d), g)
    dt = L.dtype_code(x)
    wsb = lib.dlka_conv3d_cl_workspace(byref(geom), dt, 1)
    ws = poisoned_workspace(wsb, x)
    spec = [("grad_input", x.shape, x.dtype), ("grad_weight", w.shape, torch.float32), ("grad_bias", (Cout,), torch.float32)]
    return call_guarded("conv3d_cl backward", dev, spec, need, lambda q: lib.dlka_conv3d_backward_cl(
        L.ptr(x), L.ptr(w), L.ptr(go), int(planar), *q, L.ptr(ws), wsb, byref(geom), dt, L.stream_ptr(x)), expect_rc=expect_rc)


def conv_cl_subset(dev, case, need):
    got = conv_cl_backward(dev, case, need)
    assert set(got) == {n for n, k in zip(NAMES3, need) if k}
    _check_all(f"conv3d_cl {need_id(need)}", got, _conv_cl_host(case)[1], "f32")


# ---- channels-last deformable conv (fp32; DLKA_BF16: x / out / grad_out bf16, everything else fp32) ------------------------------------------------------
# B, C (= Cout), dims, off_mode
DEFORM_CL = [
    (1, 32, (5, 6, 7), "normal"),
    (1, 32, (9, 9, 9), "integer"),
    (1, 64, (4, 4, 4), "wild"),       # small enough that the forward's tap split is live
]
DEFORM_CL_BF16 = [DEFORM_CL[0], DEFORM_CL[2]]
ROUTES = [0, 1]   # dlka_lka3d_force_wgrad_gather: 0 = the weight gradient may stream stored samples, 1 = it gathers for itself
DLKA_ERR_UNSUPPORTED = -8   # include/dlka.h


def cl_bf16_refused(need):
    """dlka_deform_conv3d_backward_cl with DLKA_BF16 refuses grad_bias without grad_weight (the bias sums ride in the weight-gradient kernel; the column-sum
    kernel that serves fp32 reads fp32 rows)."""
    return bool(need[3] and not need[2])


@functools.lru_cache(maxsize=None)
def _deform_cl_host(case, dtype):
    B, C, dims, mode = case
    x, off, w, b, go, _ = parity.make_deform3d(B, C, C, dims, 3, 1, 1, 1, 1, 1, mode, 8)
    if dtype == "bf16":   # activations only
        x, go = x.bfloat16().float(), go.bfloat16().float()
    ref = dict(zip(NAMES4, oracle.deform_conv3d_backward(x, w, b, off, go, 1, 1, 1, 1, 1, q1_literal=False)))
    ref["grad_input"] = parity.to_cl(ref["grad_input"])
    ref["out"] = parity.to_cl(oracle.deform_conv3d_forward(x, w, b, off, 1, 1, 1, 1, 1))
    return (parity.to_cl(x), off, w, b, parity.to_cl(go)), ref


@functools.lru_cache(maxsize=None)
def _deform_cl_dev(dev, case, dtype):
    x, off, w, b, go = _dev_inputs(dev, _deform_cl_host(case, dtype)[0], "f32")
    if dtype == "bf16":
        x, go = x.bfloat16(), go.bfloat16()   # exact: the host values are bf16-rounded already
    return x, off, w, b, go


class wgrad_route:
    """dlka_lka3d_force_wgrad_gather(route) for the duration, the old value restored on the way out."""

    def __init__(self, route):
        self.route = route

    def __enter__(self):
        self.old = L.get_lib().dlka_lka3d_force_wgrad_gather(int(self.route))

    def __exit__(self, *exc):
        L.get_lib().dlka_lka3d_force_wgrad_gather(self.old)


def deform_cl_backward(dev, case, dtype, need, route, expect_rc=0):
    x, off, w, b, go = _deform_cl_dev(dev, case, dtype)
    lib = L.get_lib()
    geom = ops._geom_cl(x.shape, w.shape[0], (3, 3, 3), (1, 1, 1), (1, 1, 1), 1)
    dt = L.dtype_code(x)
    wsb = lib.dlka_deform_conv3d_cl_workspace(byref(geom), dt, 1)
    ws = poisoned_workspace(wsb, x)
    gdt = ops.deform_cl_grad_dtype(x)   # what the wrapper allocates: a wrong answer here lands in the guards
    spec = [(n, t.shape, gdt) for n, t in zip(NAMES4, (x, off, w, b))]
    with wgrad_route(route):
        return call_guarded("deform3d_cl backward", dev, spec, need, lambda q: lib.dlka_deform_conv3d_backward_cl(
            L.ptr(x), L.ptr(off), L.ptr(w), L.ptr(go), *q, L.ptr(ws), wsb, byref(geom), dt, L.stream_ptr(x)), expect_rc=expect_rc)


def deform_cl_subset(dev, case, dtype, need, route):
    """fp32: the contract; bf16: 2e-2 of max |reference| — or, for a subset the library refuses, the refusal with every output left as it was."""
    if dtype == "bf16" and cl_bf16_refused(need):
        deform_cl_backward(dev, case, dtype, need, route, expect_rc=DLKA_ERR_UNSUPPORTED)
        return None
    got = deform_cl_backward(dev, case, dtype, need, route)
    assert set(got) == {n for n, k in zip(NAMES4, need) if k}
    for t in got.values():
        assert t.dtype == torch.float32
    return _check_all(f"deform3d_cl {dtype} route {route} {need_id(need)}", got, _deform_cl_host(case, dtype)[1], "f32" if dtype == "f32" else "cl_bf16")


def deform_cl_forward(dev, case, dtype):
    x, off, w, b, go = _deform_cl_dev(dev, case, dtype)
    lib = L.get_lib()
    geom = ops._geom_cl(x.shape, w.shape[0], (3, 3, 3), (1, 1, 1), (1, 1, 1), 1)
    dt = L.dtype_code(x)
    wsb = lib.dlka_deform_conv3d_cl_workspace(byref(geom), dt, 0)
    ws = poisoned_workspace(wsb, x)
    got = call_guarded("deform3d_cl forward", dev, [("out", go.shape, x.dtype)], (True,), lambda q: lib.dlka_deform_conv3d_forward_cl(
        L.ptr(x), L.ptr(off), L.ptr(w), L.ptr(b), *q, L.ptr(ws), wsb, byref(geom), dt, L.stream_ptr(x)))
    return assert_matches(f"deform3d_cl {dtype} out", got["out"], _deform_cl_host(case, dtype)[1]["out"], dtype, forward=True)


# ---- the wrappers of deformablelka_amd/ops.py ---------------------------------------------------------------------------------------------------------
def wrappers_return_none_for_what_is_not_needed(dev):
    case = CONV_CL[1]
    x, w, go = _conv_cl_dev(dev, case)
    ref = _conv_cl_host(case)[1]
    gi, gw, gb = ops.conv3d_backward_cl(x, w, go, case[5], case[6], case[7], grad_out_planar=case[8], need=(False, True, False))
    assert gi is None and gb is None
    assert_matches("ops.conv3d_backward_cl grad_weight", gw.cpu(), ref["grad_weight"], "f32")
    gi, gw, gb = ops.conv3d_backward_cl(x, w, go, case[5], case[6], case[7], grad_out_planar=case[8], need=(True, False, True))
    assert gw is None
    assert_matches("ops.conv3d_backward_cl grad_input", gi.cpu(), ref["grad_input"], "f32")
    assert_matches("ops.conv3d_backward_cl grad_bias", gb.cpu(), ref["grad_bias"], "f32")
    dcase = DEFORM_CL[0]
    x, off, w, b, go = _deform_cl_dev(dev, dcase, "f32")
    ref = _deform_cl_host(dcase, "f32")[1]
    gi, goff, gw, gb = ops.deform_conv3d_backward_cl(x, off, w, go, 1, 1, need=(False, True, False, True))
    assert gi is None and gw is None
    assert_matches("ops.deform_conv3d_backward_cl grad_offset", goff.cpu(), ref["grad_offset"], "f32")
    assert_matches("ops.deform_conv3d_backward_cl grad_bias", gb.cpu(), ref["grad_bias"], "f32")
    gi, goff, gw, gb = ops.deform_conv3d_backward_cl(x, off, w, go, 1, 1, need=(True, False, True, False))
    assert goff is None and gb is None
    assert_matches("ops.deform_conv3d_backward_cl grad_input", gi.cpu(), ref["grad_input"], "f32")
    assert_matches("ops.deform_conv3d_backward_cl grad_weight", gw.cpu(), ref["grad_weight"], "f32")


def wrappers_with_nothing_needed_do_not_call_the_library(dev):
    """C = 5 is a width the channels-last entries refuse (DLKA_ERR_UNSUPPORTED -> RuntimeError): with nothing asked for the wrappers return before the call."""
    import pytest
    x = torch.randn(1, 2, 2, 2, 5).to(dev)
    w = torch.randn(5, 5, 3, 3, 3).to(dev)
    off = torch.zeros(1, 81, 2, 2, 2).to(dev)
    assert ops.conv3d_backward_cl(x, w, x, 1, 1, 1, need=(False, False, False)) == (None, None, None)
    assert ops.deform_conv3d_backward_cl(x, off, w, x, 1, 1, need=(False,) * 4) == (None,) * 4
    with pytest.raises(RuntimeError):
        ops.conv3d_backward_cl(x, w, x, 1, 1, 1, need=(True, False, False))
    with pytest.raises(RuntimeError):
        ops.deform_conv3d_backward_cl(x, off, w, x, 1, 1, need=(True, False, False, False))


def wrapper_bf16_deform_cl(dev):
    """ops.deform_conv3d_{forward,backward}_cl with bf16 x / grad_out: `out` bf16, the four gradients fp32 and right; the subset the library refuses raises."""
    import pytest
    case = DEFORM_CL_BF16[0]
    x, off, w, b, go = _deform_cl_dev(dev, case, "bf16")
    ref = _deform_cl_host(case, "bf16")[1]
    out = ops.deform_conv3d_forward_cl(x, off, w, b, 1, 1)
    assert out.dtype == torch.bfloat16 and out.shape == go.shape
    grads = ops.deform_conv3d_backward_cl(x, off, w, go, 1, 1)
    for name, t, like in zip(NAMES4, grads, (x, off, w, b)):
        assert t.dtype == torch.float32 and t.shape == like.shape, (name, t.dtype, t.shape)
        assert_matches(f"ops.deform_conv3d_backward_cl bf16 {name}", t.cpu(), ref[name], "cl_bf16")
    gi, goff, gw, gb = ops.deform_conv3d_backward_cl(x, off, w, go, 1, 1, need=(True, False, True, True))
    assert goff is None and gi.dtype == gw.dtype == gb.dtype == torch.float32
    with pytest.raises(RuntimeError):
        ops.deform_conv3d_backward_cl(x, off, w, go, 1, 1, need=(True, True, False, True))
    with pytest.raises(RuntimeError):   # bf16 is the storage of the activations only
        ops.deform_conv3d_backward_cl(x, off, w.bfloat16(), go, 1, 1)


def conv_cl_refuses_bf16(dev):
    """dlka_conv3d_{forward,backward}_cl are fp32 only: bf16 is refused before anything is launched, at the entry (outputs untouched) and through the wrappers."""
    import pytest
    case = CONV_CL[1]
    conv_cl_backward(dev, case, (True, True, True), dtype="bf16", expect_rc=DLKA_ERR_UNSUPPORTED)
    x, w, go = _conv_cl_dev(dev, case)
    with pytest.raises(RuntimeError):
        ops.conv3d_backward_cl(x.bfloat16(), w, go.bfloat16(), case[5], case[6], case[7])
    with pytest.raises(RuntimeError):
        ops.conv3d_forward_cl(x.bfloat16(), w, None, case[5], case[6], case[7])


# ---- through autograd: the `need` the product's own Functions form from needs_input_grad -----------------------------------------------------------------
def autograd_deform_conv2d(dev, which):
    """tv_ops.DeformConv2d.  which: "offset_only" (weight and bias frozen, input without grad), "all_but_offset" (its complement), "bias_frozen"."""
    from deformablelka_amd import tv_ops
    case = DEFORM2D[0]
    (x, off, w, go, bias), ref = _deform2d_host(case, "f32")
    B, C, Cout, H, W, k, s, p, d, g, og, _ = case
    m = tv_ops.DeformConv2d(C, Cout, k, stride=s, padding=p, dilation=d, groups=g, bias=True)
    with torch.no_grad():
        m.weight.copy_(w)
        m.bias.copy_(bias)
    m = m.to(dev)
    want = {"offset_only": (False, True, False, False), "all_but_offset": (True, False, True, True), "bias_frozen": (True, True, True, False)}[which]
    xd = x.clone().to(dev).requires_grad_(want[0])    # (clones: on the emulator .to() is the shared host tensor itself)
    od = off.clone().to(dev).requires_grad_(want[1])
    m.weight.requires_grad_(want[2])
    m.bias.requires_grad_(want[3])
    y = m(xd, od)
    assert_matches(f"DeformConv2d {which} out", y.detach().cpu(), ref["out"], "f32", forward=True)
    y.backward(go.to(dev))
    for name, t, k_ in zip(NAMES4, (xd, od, m.weight, m.bias), want):
        if k_:
            assert_matches(f"DeformConv2d {which} {name}", t.grad.cpu(), ref[name], "f32")
        else:
            assert t.grad is None, f"{name} has a gradient it did not ask for"


def autograd_conv3d(dev, which):
    """nn_ops.conv3d against ATen in double.  which: "first_conv" (x without grad, as the net's first conv), "frozen_weight" (trainable bias only besides x)."""
    from deformablelka_amd import nn_ops
    case = CONV3D[0]
    (x, w, b, go), ref = _conv3d_host(case, "f32")
    s, p, d, g = case[5:9]
    want = {"first_conv": (False, True, True), "frozen_weight": (True, False, True)}[which]
    xd, wd, bd = (t.clone().to(dev).requires_grad_(k_) for t, k_ in zip((x, w, b), want))   # (clones: on the emulator .to() is the shared host tensor itself)
    y = nn_ops.conv3d(xd, wd, bd, s, p, d, g)
    assert_matches(f"nn_ops.conv3d {which} out", y.detach().cpu(), ref["out"], "f32", forward=True)
    y.backward(go.to(dev))
    for name, t, k_ in zip(NAMES3, (xd, wd, bd), want):
        if k_:
            assert_matches(f"nn_ops.conv3d {which} {name}", t.grad.cpu(), ref[name], "f32")
        else:
            assert t.grad is None, f"{name} has a gradient it did not ask for"
