"""Shared cases of tests/test_dwconv_emu.py and tests/test_dwconv_gpu.py: the channels-last depthwise family of csrc/cl_dwconv.hip, member by member — the five
forward / data-gradient kernels launch_cl_dwconv_t chooses between and the two weight-gradient kernels of launch_cl_dwconv_wgrad_t — at the smallest shapes at
which each member can still go wrong: tail groups and the partly empty last block of the two-row kernel, the 4-wide variant, a wave whose runs would straddle
rows, the one-row kernel on the fp32-only shapes, the padding workgroups of the XCD swizzle, the short last row chunk of both weight-gradient kernels.

Every single-operator case goes through ops.conv3d_forward_cl / ops.conv3d_backward_cl on seeded randn inputs (as parity.check_conv3d_cl draws them) and is
compared with F.conv3d in float64 on the CPU — forward, grad_input, grad_weight, grad_bias — at the contract's bounds, imported and not restated:
parity.FWD_ATOL on the forward, parity.BWD_RTOL of max |reference| on the three gradients.  With w ~ N(0, 1 / k^3) one missing or misplaced tap moves a
boundary output by about 5e-2, one dropped row chunk a weight-gradient element by percent.  A reference is computed once per case (functools.lru_cache) and
never written to.

Guard bands: x and grad_out are views inside allocations that extend max(256, numel) elements — at least one full row of W * C — on each side, filled with
1e30: a read the hardware range check should have answered with 0 shows as a huge error.  The outputs the wrappers allocate are views inside NaN-filled
allocations of the same proportions (partial_grad_cases.Guarded): no element may stay NaN, no guard cell may change.

On the GPU the launch trace (parity.kernels_launched) names the member that ran: the listed forward member and no other cl_dwconv* forward member, the listed
weight-gradient member and no other.

Measured on the MI355X, worst case of each group (out: max abs error, bound 1e-4; gradients: max error over max |reference|, bound 1e-3):

  group  forward / data-gradient member                       weight gradient        out      grad_input  grad_weight  grad_bias
  A      cl_dwconv_rowsN_kernel<float, 7, 3, 8, 2, true>      wgrad_kernel 7, 3      8.6e-7   1.4e-7      2.3e-7       2.8e-7
  B      cl_dwconv_rowsN_kernel<float, 7, 3, 8, 2, false>     wgrad_kernel 7, 3      5.2e-7   8.4e-8      1.9e-7       1.2e-7
  C      cl_dwconv_rowsN_kernel<float, 7, 3, 4, 2, false>     wgrad_kernel 7, 3      7.1e-7   1.1e-7      1.4e-7       1.2e-7
  D      cl_dwconv_rowsN_kernel<float, 5, 1, 4, 2, false>     wgrad_kernel 5, 1      2.5e-6   4.0e-7      1.8e-7       1.1e-7
  E      cl_dwconv_rowsN_kernel<float, 5, 1, 8, 2, false>     wgrad_kernel 5, 1      2.3e-6   5.7e-7      2.1e-7       2.3e-7
  F      cl_dwconv_rows_kernel<float, 7 3 | 5 3 | 3 1 | 7 1>  wgrad_kernel, the same 1.8e-6   2.8e-7      1.3e-7       9.2e-8
  G      cl_dwconv_kernel<float, 7 3 | 5 1, 8>                wgrad_kernel, the same 1.4e-6   3.1e-7      1.2e-7       1.3e-7
  H      one each of A, C, F, plain and swizzled: bitwise equal out and grad_input    7.5e-7   1.4e-7      2.2e-7       2.4e-7
  I      wgrad2_kernel 7, 3 (515 rows, C = 32 and 64), wgrad2_kernel 5, 1 (1025 rows),
         wgrad_kernel 7, 3 (515 rows, W = 7)                                         3.6e-6   3.8e-7      3.2e-7       2.6e-7

That the cases bite was shown once with three edits of cl_dwconv.hip, never committed: dw_row_groups without tail groups and without the partly empty block left
NaN in every rowsN case whose H is no multiple of 2 dil (A at H = 6 and 12, E at H = 6 and the groups F, G passed); rowbytes = (W + 1) C SB in the two row kernels
failed every case of A to F, H and the rowsN cases of I with errors of 1e29 (G and the W = 7 case of I run cl_dwconv_kernel, which has no descriptor);
xb = rows / rows_per_block in the weight-gradient launcher failed all four cases of I (6e-2 at 515 rows) and the 81-row case of H.  No edit reaches group G's kernel — its
bounds are explicit comparisons — so there the member's name and the reference carry the case."""
import functools
from typing import NamedTuple
from unittest import mock

import torch
import torch.nn.functional as F

from deformablelka_amd import ops
from deformablelka_amd.ops import channels_last
from tests import parity
from tests.partial_grad_cases import GUARD_MIN, Guarded, assert_matches

POISON = 1e30

# kernel, padding, dilation triples
K7D3 = ((7, 7, 7), (9, 9, 9), (3, 3, 3))     # conv_spatial of the D-LKA block
K5D1 = ((5, 5, 5), (2, 2, 2), (1, 1, 1))     # conv0
K3D1 = ((3, 3, 3), (1, 1, 1), (1, 1, 1))
K7D1 = ((7, 7, 7), (3, 3, 3), (1, 1, 1))
ACDC = ((3, 5, 5), (1, 6, 6), (1, 3, 3))     # the ACDC variant's conv_spatial at 128 channels


class Case(NamedTuple):
    group: str
    B: int
    C: int
    dims: tuple      # (D, H, W)
    conv: tuple      # (k, p, d) triples
    member: str      # the forward / data-gradient kernel, as the launch trace spells it
    wgrad: str       # the weight-gradient kernel


def _rows(t, kw, dil, tw=8):
    return f"cl_dwconv_rows_kernel<{t}, {kw}, {dil}, {tw}>"


def _rows_n(t, kw, dil, tw, wl=False):
    return f"cl_dwconv_rowsN_kernel<{t}, {kw}, {dil}, {tw}, 2, {'true' if wl else 'false'}>"


def _first(t, kw, dil):
    return f"cl_dwconv_kernel<{t}, {kw}, {dil}, 8>"


def _wg(kw, dil, gen=1):
    return f"cl_dwconv_wgrad{'2' if gen == 2 else ''}_kernel<float, {kw}, {dil}, 8>"


# launch_cl_dwconv_t: cpb = min(C, 256) channels and 256 / cpb runs per workgroup; a wave holds wpr = 2 runs at C = 32, one otherwise; the two-row kernels take the cubic
# 7^3 dil 3 from H >= 6 and 5^3 from H >= 2 when cdiv(W, 8) % wpr == 0; 4 outputs per work-item below 384 (7^3) / 1024 (5^3) waves when W % 4 == 0.
A = [Case("A", 1, 32, (3, H, 9), K7D3, _rows_n("float", 7, 3, 8, True), _wg(7, 3)) for H in range(6, 14)]   # H = 6, 12: exact blocks; 7, 8, 9, 13: tail groups with
A.append(Case("A", 2, 32, (3, 9, 9), K7D3, _rows_n("float", 7, 3, 8, True), _wg(7, 3)))                      # rem 1, 2, 3, 1; 10, 11: the partly empty regular block
B_ = [Case("B", 1, 64, (3, 7, 9), K7D3, _rows_n("float", 7, 3, 8), _wg(7, 3)),
      Case("B", 1, 512, (2, 7, 5), K7D3, _rows_n("float", 7, 3, 8), _wg(7, 3))]        # two channel groups in grid.z
C_ = [Case("C", 1, 32, (3, 8, 16), K7D3, _rows_n("float", 7, 3, 4), _wg(7, 3)),
      Case("C", 1, 64, (3, 9, 12), K7D3, _rows_n("float", 7, 3, 4), _wg(7, 3))]        # W ragged for 8-wide runs (the weight gradient's), exact for 4-wide ones
D_ = [Case("D", 2, 32, (5, 7, 16), K5D1, _rows_n("float", 5, 1, 4), _wg(5, 1)),        # odd H: a tail group of one row
      Case("D", 1, 128, (3, 5, 4), K5D1, _rows_n("float", 5, 1, 4), _wg(5, 1))]
E_ = [Case("E", 2, 32, (5, 6, 9), K5D1, _rows_n("float", 5, 1, 8), _wg(5, 1)),
      Case("E", 2, 64, (4, 7, 13), K5D1, _rows_n("float", 5, 1, 8), _wg(5, 1))]
F_ = [Case("F", 1, 32, (4, 5, 9), K7D3, _rows("float", 7, 3), _wg(7, 3)),              # H < 2 dil
      Case("F", 1, 32, (3, 7, 9), ACDC, _rows("float", 5, 3), _wg(5, 3)),
      Case("F", 1, 64, (3, 4, 10), K3D1, _rows("float", 3, 1), _wg(3, 1)),
      Case("F", 1, 64, (3, 4, 10), K7D1, _rows("float", 7, 1), _wg(7, 1))]
G_ = [Case("G", 1, 32, (3, 7, 7), K7D3, _first("float", 7, 3), _wg(7, 3)),             # C = 32 and cdiv(W, 8) odd: a wave's two runs would straddle rows
      Case("G", 2, 32, (3, 4, 20), K5D1, _first("float", 5, 1), _wg(5, 1))]
FORWARD_CASES = A + B_ + C_ + D_ + E_ + F_ + G_     # all of them below the weight gradient's row thresholds: the first-generation kernel

# launch_cl_dwconv_wgrad_t: rows = B D H; 64 row chunks (128 from 1024 rows on) of cdiv(rows, chunks) rows each; the second generation from 512 rows (7^3) / 1024 (5^3)
# where a wave's runs do not straddle rows.
I_ = [Case("I", 1, 32, (5, 103, 9), K7D3, _rows_n("float", 7, 3, 8, True), _wg(7, 3, 2)),   # 515 rows: 58 chunks of 9, the last with 2; 58 >= 16: swizzled by default
      Case("I", 1, 64, (5, 103, 5), K7D3, _rows_n("float", 7, 3, 8), _wg(7, 3, 2)),
      Case("I", 1, 32, (5, 205, 9), K5D1, _rows_n("float", 5, 1, 8), _wg(5, 1, 2)),         # 1025 rows: 114 chunks of 9, the last with 8
      Case("I", 1, 32, (5, 103, 7), K7D3, _first("float", 7, 3), _wg(7, 3))]                # above the threshold, but rows would straddle: the first generation
WGRAD_CASES = I_

BIAS_NONE_CASE = A[3]                                 # H = 9: regular groups and two tail groups, the second with one row
# one each of groups A, C and F, with a B that leaves the swizzled grid padding workgroups: grid.x = 12, 12 and 10 (checked by swizzle())
SWIZZLE_CASES = [A[3]._replace(group="H", B=3), C_[0]._replace(group="H", B=2), F_[0]._replace(group="H", B=2)]


def case_id(c):
    k, p, d = c.conv
    return f"{c.group}-{c.B}x{c.C}x{'x'.join(map(str, c.dims))}-k{'x'.join(map(str, k))}d{d[2]}"


# ---- reference ----------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _host(B, C, dims, conv, with_bias, Cout=None, groups=None):
    """Seeded inputs (channels-last x and grad_out) and F.conv3d in float64: out and the three gradients.  Depthwise (Cout = groups = C) unless told otherwise
    (tests/dense_conv_cases.py: groups = 1); w ~ N(0, 1 / (taps * C / groups))."""
    k, p, d = conv
    Cout, groups = Cout or C, groups or C
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(B, C, *dims, generator=gen)
    w = torch.randn(Cout, C // groups, *k, generator=gen) * (1.0 / (C // groups * k[0] * k[1] * k[2]) ** 0.5)
    b = torch.randn(Cout, generator=gen)
    go = torch.randn(B, Cout, *dims, generator=gen)
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    out = F.conv3d(xr, wr, br if with_bias else None, 1, p, d, groups)
    out.backward(go.double())
    ref = {"out": parity.to_cl(out.detach()), "grad_input": parity.to_cl(xr.grad), "grad_weight": wr.grad, "grad_bias": go.double().sum((0, 2, 3, 4))}
    return parity.to_cl(x), w, (b if with_bias else None), parity.to_cl(go), ref


# ---- guard bands --------------------------------------------------------------------------------------------------------------------------------------
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
    """Stands in for the name `torch` in deformablelka_amd/ops/channels_last.py during one call: the outputs the wrappers allocate become views inside NaN-filled
    allocations with guard cells on each side (partial_grad_cases.Guarded); everything else is torch's."""

    def __init__(self):
        self.made = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, shape, dtype=None, device=None):
        g = Guarded(tuple(shape), dtype, device)
        self.made.append(g)
        return g.view

    def grads_like(self, tensors, need):
        return [self.empty(t.shape, t.dtype, t.device) if n else None for t, n in zip(tensors, need)]


def _guarded_outputs(alloc):
    return mock.patch.multiple(channels_last, torch=alloc, grads_like=alloc.grads_like)


# ---- the check ----------------------------------------------------------------------------------------------------------------------------------------
def run_conv(dev, what, x, w, b, go, conv, groups, trace=False, out_planar=False, grad_out_planar=False, forward=True, need=(True, True, True)):
    """The two wrappers on guard-banded inputs (x channels-last; go in the layout grad_out_planar names) with guarded outputs -> ({name: output on the CPU},
    (kernel names the forward launched, kernel names the backward launched) — None without the trace).  forward / need: which of the four outputs to ask for.
    The guard cells are checked here; the values are not."""
    k, p, d = conv
    gx, ggo = GuardedInput(x, dev), GuardedInput(go, dev)
    assert gx.view.is_contiguous() and ggo.view.is_contiguous()
    wd, bd = w.to(dev), (None if b is None else b.to(dev))
    alloc = _GuardedAllocator()
    got = {}

    def call_forward():
        with _guarded_outputs(alloc):
            got["out"] = ops.conv3d_forward_cl(gx.view, wd, bd, p, d, groups, out_planar=out_planar)

    def call_backward():
        with _guarded_outputs(alloc):
            grads = ops.conv3d_backward_cl(gx.view, wd, ggo.view, p, d, groups, grad_out_planar=grad_out_planar, need=need)
            got.update({n: t for n, t, k_ in zip(("grad_input", "grad_weight", "grad_bias"), grads, need) if k_})

    names = []
    for fn in ([call_forward] if forward else []) + ([call_backward] if any(need) else []):
        names.append(parity.kernels_launched(fn) if trace else fn())
    asked = [n for n, k_ in zip(("out", "grad_input", "grad_weight", "grad_bias"), (forward,) + tuple(need)) if k_]
    assert len(alloc.made) == len(asked), f"{what}: {len(alloc.made)} outputs were allocated through the wrappers, expected {len(asked)}"
    assert all(any(t.data_ptr() == g.view.data_ptr() for g in alloc.made) for t in got.values())
    for g, name in zip(alloc.made, asked):
        g.assert_guards_untouched(f"{what} {name}")
    gx.assert_unchanged(f"{what} x")
    ggo.assert_unchanged(f"{what} grad_out")
    return {n: t.detach().cpu().clone() for n, t in got.items()}, (tuple(names) if trace else None)


def run(dev, case, with_bias=True, trace=False):
    """run_conv on a depthwise case -> ({name: output on the CPU}, kernel names launched (None without the trace))."""
    x, w, b, go, _ = _host(case.B, case.C, case.dims, case.conv, with_bias)
    got, names = run_conv(dev, case_id(case), x, w, b, go, case.conv, case.C, trace)
    return got, (names[0] | names[1] if trace else None)


def assert_members(case, names):
    """The listed forward / data-gradient member and no other cl_dwconv* forward member; the listed weight-gradient member and no other."""
    dw = sorted(n for n in names if n.startswith("cl_dwconv"))
    fwd = [n for n in dw if "wgrad" not in n]
    wg = [n for n in dw if "wgrad" in n]
    print(f"[{case_id(case)}] launched: {', '.join(dw)}")
    assert fwd == [case.member], f"{case_id(case)}: forward / data gradient ran {fwd}, expected {case.member}"
    assert wg == [case.wgrad], f"{case_id(case)}: weight gradient ran {wg}, expected {case.wgrad}"


def compare_with(what, got, ref, only=None, more=()):
    """Every output against the float64 reference at the contract's bounds; all of them are measured and printed before the first failure is raised.
    more: further checks, each a callable that asserts and returns (name, figure); they are measured and printed with the rest.  -> {name: figure}"""
    failures, figures = [], {}
    for name in only or ("out", "grad_input", "grad_weight", "grad_bias"):
        try:
            figures[name] = assert_matches(f"{what} {name}", got[name], ref[name], "f32", forward=(name == "out"))
        except AssertionError as e:
            failures.append(str(e))
    for check in more:
        try:
            name, figures[name] = check()
        except AssertionError as e:
            failures.append(str(e))
    print(f"[{what}] worst error: " + "  ".join(f"{n} {v:.2e}" for n, v in figures.items()) +
          f"   (bounds: out {parity.FWD_ATOL:.0e} abs, gradients {parity.BWD_RTOL:.0e} of max |ref|)")
    assert not failures, "\n".join(failures)
    return figures


def compare(case, got, with_bias=True, only=None):
    compare_with(case_id(case), got, _host(case.B, case.C, case.dims, case.conv, with_bias)[4], only)


def single_op(dev, case, with_bias=True, trace=False, only=None):
    got, names = run(dev, case, with_bias, trace)
    if trace:
        assert_members(case, names)
    compare(case, got, with_bias, only)
    return got


# ---- XCD swizzle --------------------------------------------------------------------------------------------------------------------------------------
def _row_groups(H, dil):
    """dw_row_groups(H, 2, dil).groups restated: regular groups over the full blocks of 2 dil rows and, where 1 .. dil rows remain, tail groups of two rows."""
    blk = 2 * dil
    full, rem = divmod(H, blk)
    return full * dil + (rem + 1) // 2 if full >= 1 and 1 <= rem <= dil else dil * -(-H // blk)


def forward_grid_x(case):
    """grid.x of the forward launch before the swizzle rounds it up to a multiple of 8 (launch_cl_dwconv_t restated for the members of SWIZZLE_CASES)."""
    D, H, W = case.dims
    tw = 4 if ", 4, 2," in case.member else 8
    rows = case.B * D * (_row_groups(H, case.conv[2][2]) if "rowsN" in case.member else H)
    return -(-rows * -(-W // tw) // (256 // min(case.C, 256)))


def swizzle(dev, case, monkeypatch, trace=False):
    """DLKA_XCD_MIN=1 against unset: the same member, the reference met both times, forward and grad_input bitwise equal (no atomics meet in them).  The grid has
    padding workgroups — in the LDS-weights kernel they pass the barrier before they leave — and stays below the default threshold of 16 workgroups."""
    nx = forward_grid_x(case)
    assert nx % 8 != 0 and nx < 16, nx
    monkeypatch.delenv("DLKA_XCD_MIN", raising=False)
    parity._refresh_switches()
    plain = single_op(dev, case, trace=trace)
    monkeypatch.setenv("DLKA_XCD_MIN", "1")
    parity._refresh_switches()
    swz = single_op(dev, case, trace=trace)
    for name in ("out", "grad_input"):
        assert torch.equal(plain[name], swz[name]), f"{case_id(case)} {name}: {int((plain[name] != swz[name]).sum())} elements differ between the plain and the swizzled grid"


# ---- members only the token block reaches: bf16_t storage, the fused GELU' epilogue of the data gradient, the bf16 copy out_lo -----------------------------------
# B, C, dims (the block's H, W, D: the convs' D, H, W)
TOKEN_CASES = [(1, 32, (7, 7, 9)), (1, 64, (5, 9, 12))]
# The ACDC pair is (3, 5, 5) dilation (1, 3, 3) at 128 channels only (acdc.py; 32 and 64 channels take (5, 7, 7) dilation 3): the listed member needs C = 128.
TOKEN_ACDC_CASE = (1, 128, (3, 7, 9))


def _dw_names(names):
    dw = sorted(n for n in names if n.startswith("cl_dwconv") or n.startswith("cl_dwpair"))
    print("launched: " + ", ".join(dw))
    return dw


def token_block(dev, B, C, dims, bf16, monkeypatch):
    """The token block with DLKA_DWPAIR=0 at its existing bounds; both depthwise convs ran a two-row kernel of the run's storage type.  fp32: forward and data
    gradient (with the GELU' epilogue) are `float`.  bf16: the forward convs are the `float` kernels that also write the bf16 copy (out_lo), the data gradients and
    the weight gradients the `bf16_t` instantiations."""
    monkeypatch.setenv("DLKA_DWPAIR", "0")
    parity._refresh_switches()
    check = parity.check_lka3d_tokens_bf16 if bf16 else parity.check_lka3d_tokens
    dw = _dw_names(parity.kernels_launched(lambda: check(dev, B, C, dims)))
    assert not any(n.startswith("cl_dwpair") for n in dw), dw
    for t in ("float", "bf16_t") if bf16 else ("float",):
        for kw, dil in ((5, 1), (7, 3)):
            assert any(n.startswith(f"cl_dwconv_rowsN_kernel<{t}, {kw}, {dil}, ") for n in dw), (t, kw, dil, dw)
    t = "bf16_t" if bf16 else "float"
    for kw, dil in ((5, 1), (7, 3)):
        assert f"cl_dwconv_wgrad_kernel<{t}, {kw}, {dil}, 8>" in dw, dw


def token_block_acdc(dev, monkeypatch):
    monkeypatch.setenv("DLKA_DWPAIR", "0")
    parity._refresh_switches()
    B, C, dims = TOKEN_ACDC_CASE
    dw = _dw_names(parity.kernels_launched(lambda: parity.check_lka3d_tokens(dev, B, C, dims, acdc=True)))
    assert _rows("float", 5, 3) in dw, dw
