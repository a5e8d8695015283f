"""Shared cases of tests/test_planar_seq_emu.py and tests/test_planar_seq_gpu.py: what "behaviour unchanged" means for the HOST code of the general NCDHW
("planar") path, csrc/dlka_capi.hip — the numbers its size queries return and the kernels its backward entry points launch, in order, template arguments
included.  Both are RECORDED (tests/golden/planar_sequences.json, tests/golden/make_golden_planar_sequences.py) from the commit before the path's backward
launch sequences were written once, and never taken from the code under test.  The numerical suites (parity, partial_grad_cases) then show that the
arguments of those launches are still the right ones.

  sizes      host only, any build of the library: the six operator workspace queries and the four block queries, fp32 and bf16
  launches   GPU only (the launch trace, include/dlka.h dlka_trace_*, has no emulator side): one backward call per entry, fp32 and — where the entry
             accepts it — bf16; the 2-D block with the general kernels forced (dlka_lka2d_force_general), the switch restored afterwards"""
import json
import os
from ctypes import byref, create_string_buffer

import torch

from deformablelka_amd import _lib as L
from deformablelka_amd import ops

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "planar_sequences.json")
DTYPES = {"f32": (L.DLKA_F32, torch.float32), "bf16": (L.DLKA_BF16, torch.bfloat16)}


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


# ---- sizes --------------------------------------------------------------------------------------------------------------------------------------------
# name: B, C, Cout, (D, H, W), k, pad, group, deformable_group (stride 1, dilation 1).  The deformable kernels pad Og = Cout / group to a multiple of
# their output block (csrc/deform_conv.hip: deform_pick_cob): Og = 5 and Og = 81 are no multiple of any block.
OP_SHAPES = {
    "tiny": (1, 2, 2, (2, 3, 3), 3, 1, 1, 1),
    "grouped": (1, 4, 6, (3, 4, 5), 3, 1, 2, 2),
    "og5": (2, 4, 5, (3, 4, 5), 3, 1, 1, 2),
    "og81": (1, 8, 81, (3, 4, 5), 3, 1, 1, 1),
}
BLOCK3D = [(1, 8, (3, 4, 5)), (1, 40, (3, 4, 5))]
BLOCK2D = [(1, 40, (7, 6)), (1, 96, (7, 6))]          # C = 96 also has the channels-last fast path: its sizes are a maximum over two paths


def op_geom(shape, two_d=False):
    B, C, Cout, (D, H, W), k, p, g, dg = shape
    if two_d:
        return L.ConvGeom(B, C, 1, H, W, Cout, 1, k, k, 1, 1, 1, 0, p, p, 1, 1, 1, g, dg, 64)
    return L.ConvGeom(B, C, D, H, W, Cout, k, k, k, 1, 1, 1, p, p, p, 1, 1, 1, g, dg, 64)


def sizes(lib):
    """{id: bytes} of every size query of the planar path over the shapes above."""
    out = {}
    for dname, (dt, _) in DTYPES.items():
        for sname, shape in OP_SHAPES.items():
            for fam, two_d in (("deform_conv3d", False), ("deform_conv2d", True), ("conv3d", False)):
                g = op_geom(shape, two_d)
                for direction in ("forward", "backward"):
                    out[f"{fam}_{direction}_workspace/{sname}/{dname}"] = int(getattr(lib, f"dlka_{fam}_{direction}_workspace")(byref(g), dt))
        for B, C, (D, H, W) in BLOCK3D:
            for q in ("saved", "workspace"):
                out[f"lka3d_{q}_bytes/C{C}/{dname}"] = int(getattr(lib, f"dlka_lka3d_{q}_bytes")(B, C, D, H, W, dt))
        for B, C, (H, W) in BLOCK2D:
            for q in ("saved", "workspace"):
                out[f"lka2d_{q}_bytes/C{C}/{dname}"] = int(getattr(lib, f"dlka_lka2d_{q}_bytes")(B, C, H, W, dt))
    return out


# ---- launches -----------------------------------------------------------------------------------------------------------------------------------------
def kernel_sequence(fn):
    """fn() under the launch trace -> the demangled kernel names in launch order, template arguments kept, without the dlka:: prefix and the argument list."""
    lib = L.get_lib()
    L.check(lib.dlka_trace_start(4096, torch.cuda.current_stream().cuda_stream), "trace_start")
    try:
        fn()
    finally:
        rc = lib.dlka_trace_stop()
    L.check(rc, "trace_stop")
    buf, names = create_string_buffer(1024), []
    for i in range(lib.dlka_trace_count()):
        L.check(lib.dlka_trace_get(i, buf, 1024, None), "trace_get")
        names.append(buf.value.decode().replace("void dlka::", "").replace("dlka::", "").split("(")[0])
    return names


def _rand(gen, *shape, scale=1.0):
    return torch.randn(*shape, generator=gen) * scale


def _op_tensors(dev, dtype, two_d):
    B, C, Cout, (D, H, W), k, p, g, dg = OP_SHAPES["grouped"]
    gen = torch.Generator().manual_seed(0)
    sp, kk, noff = ((H, W), (k, k), 2) if two_d else ((D, H, W), (k, k, k), 3)
    K = k ** len(kk)
    t = dict(x=_rand(gen, B, C, *sp), off=_rand(gen, B, dg * noff * K, *sp, scale=0.5), w=_rand(gen, Cout, C // g, *kk, scale=0.2), b=_rand(gen, Cout),
             go=_rand(gen, B, Cout, *sp))
    return {n: v.to(dtype).to(dev).contiguous() for n, v in t.items()}


def _deform_backward(dev, dname, two_d, need):
    dt, dtype = DTYPES[dname]
    t = _op_tensors(dev, dtype, two_d)
    g = op_geom(OP_SHAPES["grouped"], two_d)
    lib = L.get_lib()
    fam = "deform_conv2d" if two_d else "deform_conv3d"
    wsb = getattr(lib, f"dlka_{fam}_backward_workspace")(byref(g), dt)
    ws = L.scratch(wsb, t["x"])
    outs = [torch.empty_like(t[n]) if want else None for n, want in zip(("x", "off", "w", "b"), need)]

    def call():
        L.check(getattr(lib, f"dlka_{fam}_backward")(L.ptr(t["x"]), L.ptr(t["off"]), L.ptr(t["w"]), L.ptr(t["go"]), *(L.ptr(o) for o in outs), L.ptr(ws), wsb,
                                                     byref(g), dt, L.stream_ptr(t["x"])), f"{fam} backward")
    return kernel_sequence(call)


def _conv_backward(dev, dname):
    dt, dtype = DTYPES[dname]
    t = _op_tensors(dev, dtype, False)
    g = op_geom(OP_SHAPES["grouped"])
    lib = L.get_lib()
    wsb = lib.dlka_conv3d_backward_workspace(byref(g), dt)
    ws = L.scratch(wsb, t["x"])
    outs = [torch.empty_like(t[n]) for n in ("x", "w", "b")]

    def call():
        L.check(lib.dlka_conv3d_backward(L.ptr(t["x"]), L.ptr(t["w"]), L.ptr(t["go"]), *(L.ptr(o) for o in outs), L.ptr(ws), wsb, byref(g), dt,
                                         L.stream_ptr(t["x"])), "conv3d backward")
    return kernel_sequence(call)


def _block_params(fields, shapes, dev, dtype):
    gen = torch.Generator().manual_seed(1)
    return [_rand(gen, *shapes[f], scale=0.1).to(dtype).to(dev) for f in fields]


def _lka3d_backward(dev, dname):
    _, dtype = DTYPES[dname]
    B, C, dims = BLOCK3D[0]
    pw, b = (C, C, 1, 1, 1), (C,)
    shapes = dict(zip(L.LKA3D_FIELDS, (pw, b, (C, 1, 5, 5, 5), b, (C, 1, 7, 7, 7), b, (81, C, 3, 3, 3), (81,), (C, C, 3, 3, 3), b, pw, b, pw, b)))
    params = _block_params(L.LKA3D_FIELDS, shapes, dev, dtype)
    gen = torch.Generator().manual_seed(2)
    x, gy = (_rand(gen, B, C, *dims).to(dtype).to(dev) for _ in range(2))
    _, saved = ops.lka3d_attention_forward(x, params)
    return kernel_sequence(lambda: ops.lka3d_attention_backward(x, params, gy, saved))


def _lka2d_backward_general(dev, dname):
    _, dtype = DTYPES[dname]
    B, C, (H, W) = BLOCK2D[0]
    shapes = dict(zip(L.LKA2D_FIELDS, _lka2d_shapes(C)))
    params = _block_params(L.LKA2D_FIELDS, shapes, dev, dtype)
    gen = torch.Generator().manual_seed(2)
    x, gy = (_rand(gen, B, C, H, W).to(dtype).to(dev) for _ in range(2))
    lib = L.get_lib()
    old = lib.dlka_lka2d_force_general(1)
    try:
        _, saved = ops.lka2d_attention_forward(x, params)
        return kernel_sequence(lambda: ops.lka2d_attention_backward(x, params, gy, saved))
    finally:
        lib.dlka_lka2d_force_general(old)


def _lka2d_shapes(C):
    by_name = {"proj_1_w": (C, C, 1, 1), "conv0_offset_w": (50, C, 5, 5), "conv0_offset_b": (50,), "conv0_w": (C, 1, 5, 5),
               "conv_spatial_offset_w": (98, C, 7, 7), "conv_spatial_offset_b": (98,), "conv_spatial_w": (C, 1, 7, 7), "conv1_w": (C, C, 1, 1),
               "proj_2_w": (C, C, 1, 1)}
    return [by_name.get(f, (C,)) for f in L.LKA2D_FIELDS]


# id: (runner, dtypes the entry accepts on this path).  The general 2-D block is fp32 only: DLKA_BF16 there means the channels-last path.
LAUNCHES = {
    "deform_conv3d_backward/all": (lambda dev, d: _deform_backward(dev, d, False, (True,) * 4), ("f32", "bf16")),
    "deform_conv3d_backward/grad_weight_only": (lambda dev, d: _deform_backward(dev, d, False, (False, False, True, False)), ("f32", "bf16")),
    "deform_conv2d_backward/all": (lambda dev, d: _deform_backward(dev, d, True, (True,) * 4), ("f32", "bf16")),
    "conv3d_backward/all": (_conv_backward, ("f32", "bf16")),
    "lka3d_attention_backward": (_lka3d_backward, ("f32", "bf16")),
    "lka2d_attention_backward/general": (_lka2d_backward_general, ("f32",)),
}
LAUNCH_IDS = [f"{k}/{d}" for k, (_, ds) in LAUNCHES.items() for d in ds]


def launches(dev, cid):
    name, dname = cid.rsplit("/", 1)
    return LAUNCHES[name][0](dev, dname)
