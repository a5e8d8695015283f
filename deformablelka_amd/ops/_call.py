"""What every operator family shares: argument normalisation, geometry, pointer structs, the call-and-check helpers, the block forward / backward
pair, the side-stream hand-over and the launch counters."""
from __future__ import annotations

import ctypes
import math
from ctypes import byref
from typing import Callable, NamedTuple, Tuple

import torch

from .. import _lib as L


def _triple(v) -> Tuple[int, int, int]:
    if isinstance(v, int):
        return (v, v, v)
    v = tuple(int(x) for x in v)
    if len(v) != 3:
        raise ValueError(f"expected an int or a 3-tuple, got {v}")
    return v


def _pair(v) -> Tuple[int, int]:
    if isinstance(v, int):
        return (v, v)
    v = tuple(int(x) for x in v)
    if len(v) != 2:
        raise ValueError(f"expected an int or a 2-tuple, got {v}")
    return v


def _require_input_dtype(input, **named):
    """The general operators hand EVERY pointer to the library as the type of `input` (float32, bfloat16 or float64): a tensor of another dtype would be read at
    the wrong element size — past its end when it is the narrower one.  The reference's op raises a scalar-type mismatch there; so does this, before any launch."""
    for name, t in named.items():
        if t is not None and t.dtype != input.dtype:
            raise RuntimeError(f"expected `{name}` to have the dtype of `input` ({input.dtype}), got {t.dtype}")


def require_fp32_params(what, x, **named):
    """bfloat16 is an ACTIVATION dtype of the channels-last and token-layout blocks: the library reads every parameter as float32 whatever x is.  A parameter
    of another dtype is refused before any launch."""
    for name, t in named.items():
        if t is not None and t.dtype != torch.float32:
            raise RuntimeError(f"{what}: `{name}` must be float32 (bfloat16 is the storage of the activations only), got {t.dtype} next to {x.dtype} activations")


def lka2d_width_ok(C: int) -> bool:
    """Widths the channels-last 2-D attention blocks cover, plain and deformable, in float32 and with bfloat16 activations alike: C / 32 in
    {1, 2, 3, 4, 6, 8, 12} (csrc/capi_lka2d_frame.h: frame_width_ok)."""
    return C % 32 == 0 and C // 32 in (1, 2, 3, 4, 6, 8, 12)


# ---- dtype tables of the pipeline families: torch dtype -> the library's code -------------------------------------------------------------
_SD_DTYPES = {torch.uint8: L.DLKA_SD_U8, torch.bool: L.DLKA_SD_U8, torch.int16: L.DLKA_SD_I16, torch.int32: L.DLKA_SD_I32, torch.int64: L.DLKA_SD_I64}
_RS_DTYPES = {torch.float32: L.DLKA_F32, torch.float64: L.DLKA_F64}
_AUG_DTYPES = {torch.float32: L.DLKA_F32, torch.bfloat16: L.DLKA_BF16, torch.float64: L.DLKA_F64, torch.int16: L.DLKA_AUG_I16}
_ZM_DTYPES = {torch.float32: L.DLKA_F32, torch.bfloat16: L.DLKA_BF16, torch.float64: L.DLKA_F64, torch.int16: L.DLKA_ZOOM2D_I16}
_I3 = ctypes.c_int64 * 3   # three extents, as the resampling and augmentation entries take them


def table_dtype(t, table, family, accepted):
    """The code of t's dtype in ``table``, or the family's refusal ``accepted`` spells out ("label maps are uint8, ... or bool")."""
    if t.dtype not in table:
        raise RuntimeError(f"{family}: {accepted}, got {t.dtype}")
    return table[t.dtype]


# ---- geometry -----------------------------------------------------------------------------------------------------------------------------
def _geom(x_shape, cout, k, s, p, d, group, dg=1, im2col_step=64) -> L.ConvGeom:
    B, C, D, H, W = (int(v) for v in x_shape)
    return L.ConvGeom(B, C, D, H, W, int(cout), *k, *s, *p, *d, int(group), int(dg), int(im2col_step))


def _out_dims(g: L.ConvGeom):
    f = L.get_lib().dlka_conv_out_size
    return (f(g.D, g.pd, g.dd, g.kd, g.sd), f(g.H, g.ph, g.dh, g.kh, g.sh), f(g.W, g.pw, g.dw, g.kw, g.sw))


def _geom2d(x_shape, weight_shape, s, p, d, offset_channels):
    B, C, H, W = (int(v) for v in x_shape)
    Cout, Cg, kh, kw = (int(v) for v in weight_shape)
    if C % Cg != 0:
        raise RuntimeError("input channels must be divisible by weight.shape[1]")
    og = offset_channels // (2 * kh * kw)
    if og == 0 or offset_channels != og * 2 * kh * kw:
        raise RuntimeError(f"offset.shape[1] = {offset_channels} is not a multiple of 2*kh*kw = {2 * kh * kw}")
    return L.ConvGeom(B, C, 1, H, W, Cout, 1, kh, kw, 1, s[0], s[1], 0, p[0], p[1], 1, d[0], d[1], C // Cg, og, 64)


def _geom_cl(x_shape, cout, k, p, d, group, dg=1):
    B, D, H, W, C = (int(v) for v in x_shape)
    return L.ConvGeom(B, C, D, H, W, int(cout), *k, 1, 1, 1, *p, *d, int(group), int(dg), 64)


def _rank_padded_ext(d, shape):
    """d.rank and d.ext of a description whose kernels always see three axes: the leading extents of a lower rank are 1."""
    d.rank = len(shape)
    for ax in range(3):
        d.ext[ax] = 1 if ax < 3 - d.rank else int(shape[ax - (3 - d.rank)])


# ---- tensors in and out -------------------------------------------------------------------------------------------------------------------
def ptr_struct(cls, fields, tensors):
    """A struct of device pointers, one per field; a None entry is a null pointer."""
    st = cls()
    for n, t in zip(fields, tensors):
        setattr(st, n, None if t is None else t.data_ptr())
    return st


def grads_like(tensors, need):
    """A fresh gradient per tensor ``need`` asks for, None for the others (the library takes those as null)."""
    return [torch.empty_like(t) if n else None for t, n in zip(tensors, need)]


def saved_view(saved, byte_offset, shape, dtype=torch.float32):
    """The tensor of ``shape`` that starts ``byte_offset`` bytes into an opaque ``saved`` buffer."""
    o = int(byte_offset)
    return saved[o:o + math.prod(shape) * dtype.itemsize].view(dtype).view(*shape)


# ---- calls --------------------------------------------------------------------------------------------------------------------------------
def call(entry, *args, label=None):
    """``dlka_<entry>(*args)``; a status other than 0 raises under ``label`` (the entry's name unless given)."""
    L.check(getattr(L.get_lib(), "dlka_" + entry)(*args), label or entry)


WS = object()   # where an entry takes its (workspace pointer, byte count) pair


def call_ws(entry, query, anchor, *args, label=None):
    """``call`` for an entry with a workspace: ``query`` = (size-query name, *its arguments) gives the byte count, the buffer comes from the caching
    allocator on ``anchor``'s device, and pointer and count replace ``WS`` in ``args``.  Returns the workspace."""
    nbytes = getattr(L.get_lib(), "dlka_" + query[0])(*query[1:])
    ws = L.scratch(nbytes, anchor)
    i = args.index(WS)
    call(entry, *args[:i], L.ptr(ws), nbytes, *args[i + 1:], label=label)
    return ws


# ---- the launch counters: <family>_launch_count() = kernels the family has launched in this process ---------------------------------------
COUNTED_FAMILIES = ("tiles", "seg_loss", "sd", "cc", "resample", "augment", "prep", "zoom2d")


def _launch_counter(family):
    def count() -> int:
        return int(getattr(L.get_lib(), f"dlka_{family}_launch_count")())
    count.__name__ = count.__qualname__ = f"{family}_launch_count"
    return count


globals().update({f"{f}_launch_count": _launch_counter(f) for f in COUNTED_FAMILIES})


# ---- whole blocks: one forward / backward pair ----------------------------------------------------------------------------------------------
class Block(NamedTuple):
    """What tells the fused blocks' entry points apart."""
    entry: str              # dlka_<entry>_forward<v> / _backward<v>; the labels are "<entry>_forward" / "<entry>_backward"
    sizes: str              # dlka_<sizes>_saved_bytes<v> / _workspace_bytes<v>
    v: str                  # "_v": the entries end in a variant argument
    ptrs: type              # the parameters' pointer struct ...
    fields: tuple           # ... and its fields, in the order the parameters come
    params: Callable        # (x, params) -> the tensors handed to the library (contiguous; refuses what the block does not take)
    extents: Callable       # (x, dims) -> the extents the entries take
    refusal: int            # status raised when the size query refuses the shape
    cast_grad: bool         # grad_y is brought to x's dtype


def block_forward(b: Block, x, params, dims=None, variant=()):
    L.require_device(x, *params)
    x = x.contiguous()
    params = b.params(x, params)
    lib = L.get_lib()
    tail = (*b.extents(x, dims), L.dtype_code(x), *variant)
    sb = getattr(lib, f"dlka_{b.sizes}_saved_bytes{b.v}")(*tail)
    wb = getattr(lib, f"dlka_{b.sizes}_workspace_bytes{b.v}")(*tail)
    if sb == 0:
        L.check(b.refusal, b.entry + "_forward")
    saved, ws = L.scratch(sb, x), L.scratch(wb, x)
    y = torch.empty_like(x)
    ps = ptr_struct(b.ptrs, b.fields, params)
    call(b.entry + "_forward" + b.v, L.ptr(x), byref(ps), L.ptr(y), L.ptr(saved), sb, L.ptr(ws), wb, *tail, L.stream_ptr(x), label=b.entry + "_forward")
    return y, saved


def block_backward_args(b: Block, x, params, grad_y, saved, dims=None, variant=()):
    """-> (args, tail, gx, grads, keep): an entry is called as (*args, [phase arguments,] *tail, stream); ``keep`` = [ws, grad_y, saved, x] as the call reads them."""
    L.require_device(x, grad_y, saved, *params)
    x, grad_y = x.contiguous(), (grad_y.to(x.dtype) if b.cast_grad else grad_y).contiguous()
    params = b.params(x, params)
    tail = (*b.extents(x, dims), L.dtype_code(x), *variant)
    wb = getattr(L.get_lib(), f"dlka_{b.sizes}_workspace_bytes{b.v}")(*tail)
    ws = L.scratch(wb, x)
    gx = torch.empty_like(x)
    grads = [torch.empty_like(t) for t in params]
    ps, gs = ptr_struct(b.ptrs, b.fields, params), ptr_struct(b.ptrs, b.fields, grads)
    args = (L.ptr(x), byref(ps), L.ptr(grad_y), L.ptr(saved), saved.numel(), L.ptr(gx), byref(gs), L.ptr(ws), wb)
    return args, tail, gx, grads, [ws, grad_y, saved, x]


def block_backward(b: Block, x, params, grad_y, saved, dims=None, variant=()):
    args, tail, gx, grads, _ = block_backward_args(b, x, params, grad_y, saved, dims, variant)
    call(b.entry + "_backward" + b.v, *args, *tail, L.stream_ptr(x), label=b.entry + "_backward")
    return gx, grads


# ---- a backward pass in two parts, the second on a side stream ----------------------------------------------------------------------------
def side_stream_phases(run_phase, anchor, side_stream):
    """``run_phase(1, stream)``, the data-gradient chain, on ``anchor``'s current stream; ``run_phase(2, stream)``, the weight gradients, on ``side_stream``
    behind an event recorded after part 1 — and NOT joined: that is the caller's job.  ``side_stream`` "inline": both parts back to back on the
    current stream (tests: the split pass equals the whole one).

    What part 2 READS the caller keeps referenced until its join: memory released after the join is reused by work that is ordered behind it, so no
    record_stream() is needed.  What it WRITES — the parameter gradients — must NOT be referenced: autograd's AccumulateGrad takes ownership of a returned
    gradient only while nobody else holds it, and would otherwise COPY it on the current stream, i.e. before the side stream has written it (seen as garbage
    gradients, profiles/r08_notes.md); as `.grad` they outlive the join by themselves."""
    cur = L.stream_ptr(anchor)
    run_phase(1, cur)
    if isinstance(side_stream, str):
        side = cur
    else:
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(anchor.device))
        side_stream.wait_event(ev)
        side = ctypes.c_void_p(side_stream.cuda_stream)
    run_phase(2, side)
