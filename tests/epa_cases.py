"""TEST INFRASTRUCTURE — cases and checks of the UNETR++ efficient paired attention (csrc/cl_epa.hip, deformablelka_amd/ops/epa.py, the EPA and
TransformerBlock classes of transformerblock.py and acdc.py), shared by tests/test_epa_emu.py (wavefront emulator) and tests/test_epa_gpu.py (MI355X).

Oracle: the reference's own output (tests/golden/reference_epa*.pt, tests/golden/make_golden_epa.py) and, for everything those records do not reach, the
float64 restatement tests/epa_ref.py, itself checked against the records.  Tolerances: the project's contract — forward 1e-4 absolute, every gradient
1e-3 of max |reference| (parity.assert_close)."""
import contextlib
import os
from unittest import mock

import torch

from tests import epa_ref, parity
from tests.partial_grad_cases import Guarded

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HEADS = 4

_EPA_KEYS = ["temperature", "temperature2", "qkvv.weight", "E.weight", "E.bias", "F.weight", "F.bias", "out_proj.weight", "out_proj.bias",
             "out_proj2.weight", "out_proj2.bias"]


def _res_keys(name):
    keys = [f"{name}.conv1.conv.weight", f"{name}.conv2.conv.weight"]
    for n in ("norm1", "norm2"):
        keys += [f"{name}.{n}.{k}" for k in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
    return keys


def _block_keys(acdc, pos_embed=True):
    return (["gamma"] + (["pos_embed"] if pos_embed else []) + ["norm.weight", "norm.bias"] + ["epa_block." + k for k in _EPA_KEYS] + _res_keys("conv51")
            + (_res_keys("conv52") if acdc else []) + ["conv8.1.weight", "conv8.1.bias"])


# state_dict key lists of the four classes, in the reference's registration order
STATE_KEYS = {"synapse_epa": _EPA_KEYS, "acdc_epa": _EPA_KEYS, "synapse_block": _block_keys(False), "acdc_block": _block_keys(True)}

# (D, P, N): the smallest shapes at which each part can go wrong.  N = 60: less than one wave; 120: a ragged last wave; 600: three 256-token chunks of the
# statistics pass and three token tiles, so the ordered folds run.  B = 2 throughout.
OPERATOR_CASES = [(8, 32, 60), (8, 64, 120), (16, 32, 120), (16, 64, 60), (32, 32, 60), (32, 64, 120), (64, 32, 120), (64, 64, 60), (8, 64, 600), (64, 64, 600)]
EMU_OPERATOR_CASES = [c for c in OPERATOR_CASES if c != (64, 64, 600)]   # (the emulator runs lanes as fibers: the largest case is the GPU's)


def case_id(c):
    return "D%d_P%d_N%d" % c


def classes(tag):
    from deformablelka_amd import acdc, transformerblock
    mod = acdc if tag.startswith("acdc") else transformerblock
    return mod.EPA if tag.endswith("epa") else mod.TransformerBlock


_RECORDS = {}


def record(tag):
    """The reference's own run of class ``tag`` (loaded once, never changed)."""
    if tag not in _RECORDS:
        name = "reference_epa.pt" if tag.endswith("epa") else "reference_epa_block_%s.pt" % tag.split("_")[0]
        _RECORDS.update({k: v for k, v in torch.load(os.path.join(GOLDEN, name)).items() if k != "config"})
        if tag == "acdc_block":   # the gradients of its four 3^3 conv weights are kept in a file of their own (the committed-file limit)
            extra = torch.load(os.path.join(GOLDEN, "reference_epa_block_acdc_conv_grads.pt"))["acdc_block_conv_grads"]
            assert len(extra) == 4
            _RECORDS[tag]["grad_params"].update(extra)
    return _RECORDS[tag]


def make_operator(D, P, N, B=2, seed=0, scale=1.0, temp=None, zero_cols=False, masks=False):
    g = torch.Generator().manual_seed(seed)
    C = HEADS * D
    t = dict(qkvv=torch.randn(B, N, 4 * C, generator=g) * scale, kp=torch.randn(B, C, P, generator=g) * scale, vp=torch.randn(B, C, P, generator=g),
             temperature=(0.5 + 2 * torch.rand(HEADS, 1, 1, generator=g)) if temp is None else torch.full((HEADS, 1, 1), float(temp)),
             temperature2=(0.5 + 2 * torch.rand(HEADS, 1, 1, generator=g)) if temp is None else torch.full((HEADS, 1, 1), float(temp)))
    if zero_cols:   # one all-zero Q column and one all-zero K column: the 1e-12 clamp, forward and backward
        t["qkvv"][:, :, D + 1] = 0
        t["qkvv"][:, :, C + 2] = 0
    m1 = m2 = None
    if masks:
        m1 = torch.empty(B, HEADS, D, D).bernoulli_(0.7, generator=g) / 0.7
        m2 = torch.empty(B, HEADS, N, P).bernoulli_(0.6, generator=g).to(torch.uint8)
    go = (torch.randn(B, N, C, generator=g), torch.randn(B, N, C, generator=g))
    return t, m1, m2, 1 / 0.6, go


_REF_CACHE = {}


def operator_reference(key, t, m1, m2, scale, go):
    """float64 restatement of one operator case: outputs and gradients (computed once per case)."""
    if key not in _REF_CACHE:
        leaves = {k: v.double().clone().requires_grad_(True) for k, v in t.items()}
        x_sa, x_ca = epa_ref.attention(leaves["qkvv"], leaves["kp"], leaves["vp"], leaves["temperature"], leaves["temperature2"], HEADS,
                                       None if m1 is None else m1.double(), None if m2 is None else m2.double() * scale)
        torch.autograd.backward([x_sa, x_ca], [go[0].double(), go[1].double()])
        _REF_CACHE[key] = (x_sa.detach(), x_ca.detach(), {k: v.grad for k, v in leaves.items()})
    return _REF_CACHE[key]


class _GuardedAllocator:
    """Stands in for the name `torch` in deformablelka_amd/ops/epa.py during one call: every output the wrappers allocate is a view inside a NaN-filled
    allocation with guard cells on each side."""

    def __init__(self):
        self.made = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, shape, dtype=None, device=None):
        g = Guarded(tuple(shape), dtype, device)
        self.made.append(g)
        return g.view

    def empty_like(self, t):
        return self.empty(t.shape, t.dtype, t.device)


GUARD_BYTES = 4096   # (a multiple of the 256-byte alignment the library carves its workspace with)


@contextlib.contextmanager
def guards(alloc):
    """The wrappers' outputs through ``alloc``, and their scratch buffers (saved statistics, workspace: ``_lib.scratch``) between 4096-byte bands of 0xA5
    that must read back unchanged."""
    from deformablelka_amd import _lib as L
    from deformablelka_amd.ops import epa
    made = []

    def scratch(nbytes, like):
        n = max(int(nbytes), 1)
        buf = torch.full((n + 2 * GUARD_BYTES,), 0xA5, dtype=torch.uint8, device=like.device)
        made.append((buf, n))
        return buf[GUARD_BYTES:GUARD_BYTES + n]

    with mock.patch.object(epa, "torch", alloc), mock.patch.object(L, "scratch", scratch):
        yield
    assert len(made) == 3, len(made)   # saved statistics, forward workspace, backward workspace
    for i, (buf, n) in enumerate(made):
        assert bool((buf[:GUARD_BYTES] == 0xA5).all()) and bool((buf[GUARD_BYTES + n:] == 0xA5).all()), f"scratch buffer {i}: a guard band was written"


def run_operator(dev, t, m1, m2, scale, go, guard=False):
    """ops.epa forward + backward -> {name: tensor on the CPU}; guard: the outputs sit between guard bands that must stay untouched."""
    from deformablelka_amd.ops import epa
    d = {k: v.to(dev) for k, v in t.items()}
    m1d, m2d = (None if m is None else m.to(dev) for m in (m1, m2))
    alloc = _GuardedAllocator()
    with guards(alloc) if guard else contextlib.nullcontext():
        x_sa, x_ca, saved = epa.attention_forward(d["qkvv"], d["kp"], d["vp"], d["temperature"], d["temperature2"], m1d, m2d, scale)
        grads = epa.attention_backward(d["qkvv"], d["kp"], d["vp"], d["temperature"], d["temperature2"], go[0].to(dev), go[1].to(dev), saved, m1d, m2d, scale)
    if guard:
        assert len(alloc.made) == 7, len(alloc.made)   # x_sa, x_ca; g_qkvv, g_kp, g_vp and the two per-sample temperature gradients
        for i, g in enumerate(alloc.made):
            g.assert_guards_untouched(f"output {i}")
    out = {"x_sa": x_sa, "x_ca": x_ca}
    out.update(zip(("qkvv", "kp", "vp", "temperature", "temperature2"), grads))
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def check_operator(dev, D, P, N, guard=False, **kw):
    t, m1, m2, scale, go = make_operator(D, P, N, **kw)
    ref_sa, ref_ca, ref_g = operator_reference((D, P, N, tuple(sorted(kw.items()))), t, m1, m2, scale, go)
    got = run_operator(dev, t, m1, m2, scale, go, guard)
    tag = f"epa D={D} P={P} N={N} {kw}"
    for name, ref in (("x_sa", ref_sa), ("x_ca", ref_ca)):
        print(f"[{tag}] {name} max abs err {(got[name].double() - ref).abs().max().item():.3e}")
        parity.assert_close(f"{tag} {name}", got[name], ref, atol=parity.FWD_ATOL)
    for name, ref in ref_g.items():
        g = got[name].double()
        if name == "qkvv":   # slot 3 (Vs) and the spatial branch's part of K are reached through vp / kp only: the operator leaves them to the caller's GEMMs
            C = HEADS * D
            assert bool((g[:, :, 3 * C:] == 0).all()), f"{tag}: slot 3 of g_qkvv is not zero"
        print(f"[{tag}] grad {name} rel err {parity.rel_err(g, ref):.3e}")
        parity.assert_close(f"{tag} grad {name}", g, ref, rtol=parity.BWD_RTOL)
    return got


def check_offset_views(dev):
    """Contiguous views that start 4 bytes into their storage (not 16-byte aligned) give the bits of the aligned call."""
    t, m1, m2, scale, go = make_operator(8, 32, 60)

    def shifted(v):
        buf = torch.empty(v.numel() + 1, dtype=v.dtype)
        buf[1:].copy_(v.reshape(-1))
        return buf[1:].view(v.shape)

    t2 = {k: shifted(v) for k, v in t.items()}
    go2 = tuple(shifted(g) for g in go)
    if dev != "cpu":   # (a device copy of a view is a fresh, aligned allocation: shift on the device)
        t2 = {k: shifted(v).to(dev) for k, v in t.items()}
        t2 = {k: torch.cat([v.reshape(-1)[:1], v.reshape(-1)])[1:].view(v.shape) for k, v in t2.items()}
        assert all(v.data_ptr() % 16 for v in t2.values())
    same_bits(run_operator(dev, t, m1, m2, scale, go), run_operator(dev, t2, m1, m2, scale, go2))


def same_bits(a, b):
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"{k}: two identical calls differ"


# ---- modules ---------------------------------------------------------------------------------------------------------------------------------
def load_module(tag, dev):
    rec = record(tag)
    cfg = dict(input_size=120, hidden_size=32, proj_size=32, num_heads=HEADS)
    m = classes(tag)(**cfg) if tag.endswith("epa") else classes(tag)(**cfg, dropout_rate=0.1, pos_embed=True)
    assert list(m.state_dict().keys()) == STATE_KEYS[tag]
    m.load_state_dict(rec["state_dict"], strict=True)
    return m.to(dev).eval(), rec


def check_module_against_reference(tag, dev, per_op=False):
    """The module on the reference's input against the reference's own output and gradients; per_op: through ``forward_per_op`` (torch only)."""
    m, rec = load_module(tag, dev)
    if per_op:
        m.forward = m.forward_per_op
    if tag.endswith("epa") and not per_op:
        assert m.fused(rec["inputs"][0].to(dev)), "the fixture's width must take the fused kernels"
    x = rec["inputs"][0].detach().clone().to(dev).requires_grad_(True)   # (a copy: on the CPU `.to(dev)` is the record's own tensor)
    y = m(x)
    y.backward(rec["grad_output"].to(dev))
    print(f"[{tag}] y max abs err {(y.detach().cpu() - rec['output']).abs().max().item():.3e}")
    parity.assert_close(f"{tag} y", y.detach(), rec["output"], atol=parity.FWD_ATOL)
    parity.assert_close(f"{tag} grad x", x.grad, rec["grad_inputs"][0], rtol=parity.BWD_RTOL)
    named = dict(m.named_parameters())
    for k, g in rec["grad_params"].items():
        assert named[k].grad is not None, k
        print(f"[{tag}] grad {k} rel err {parity.rel_err(named[k].grad, g):.3e}")
        parity.assert_close(f"{tag} grad {k}", named[k].grad, g, rtol=parity.BWD_RTOL)


def check_restatement_against_reference(tag):
    """tests/epa_ref.py in float64 on the reference's EPA record: output and every gradient."""
    rec = record(tag)
    P = {k: v.double().clone().requires_grad_(True) for k, v in rec["state_dict"].items()}
    x = rec["inputs"][0].double().requires_grad_(True)
    y = epa_ref.epa(x, P, HEADS)
    y.backward(rec["grad_output"].double())
    parity.assert_close(f"{tag} restatement y", y.detach(), rec["output"], atol=parity.FWD_ATOL)
    parity.assert_close(f"{tag} restatement grad x", x.grad, rec["grad_inputs"][0], rtol=parity.BWD_RTOL)
    for k, g in rec["grad_params"].items():
        got = P[k].grad
        if tag.startswith("synapse") and k.startswith("E."):   # E is F: the shared layer's gradient is the sum of both uses
            got = got + P["F." + k[2:]].grad
        parity.assert_close(f"{tag} restatement grad {k}", got, g, rtol=parity.BWD_RTOL)


def check_module_against_restatement(dev, tag="synapse_epa", C=32, N=60, P=32, train_masks=False, seed=3):
    """An EPA of any width against the float64 restatement on the same parameters; train_masks: training mode with injected multipliers."""
    torch.manual_seed(seed)
    D = C // HEADS
    m = classes(tag)(input_size=N, hidden_size=C, proj_size=P, num_heads=HEADS)
    with torch.no_grad():
        m.temperature.uniform_(0.5, 2.5)
        m.temperature2.uniform_(0.5, 2.5)
    x = torch.randn(2, N, C)
    go = torch.randn(2, N, C)
    m1 = m2 = None
    scale = 1.0
    if train_masks:
        m1 = torch.empty(2, HEADS, D, D).bernoulli_(0.8) / 0.8
        m2 = torch.empty(2, HEADS, N, P).bernoulli_(0.7).to(torch.uint8)
        scale = 1 / 0.7
    Pd = {k: v.detach().double().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    xr = x.double().requires_grad_(True)
    yr = epa_ref.epa(xr, Pd, HEADS, None if m1 is None else m1.double(), None if m2 is None else m2.double() * scale)
    yr.backward(go.double())
    m = m.to(dev).train(train_masks)
    if train_masks:
        m._draw_masks = lambda B, N_, device: (m1.to(device), m2.to(device), scale)
    xd = x.to(dev).requires_grad_(True)
    y = m(xd)
    y.backward(go.to(dev))
    tagc = f"{tag} C={C} N={N} P={P} masks={train_masks}"
    parity.assert_close(f"{tagc} y", y.detach(), yr.detach(), atol=parity.FWD_ATOL)
    parity.assert_close(f"{tagc} grad x", xd.grad, xr.grad, rtol=parity.BWD_RTOL)
    for k, p in m.named_parameters():
        ref = Pd[k].grad
        if m.E is m.F and k.startswith("E."):
            ref = ref + Pd["F." + k[2:]].grad
        parity.assert_close(f"{tagc} grad {k}", p.grad, ref, rtol=parity.BWD_RTOL)
    return m


def check_net(dev):
    """D_LKA_Former(trans_block=TransformerBlock) at the small constructor of tests/test_nets.py: one forward + backward, finite and non-zero
    gradients on every parameter."""
    import deformablelka_amd as dk
    from deformablelka_amd import transformerblock
    torch.manual_seed(0)
    net = dk.D_LKA_Former(in_channels=1, out_channels=3, img_size=[32, 32, 32], depths=[1, 1, 1, 1], dims=[32, 64, 128, 256], do_ds=False,
                          trans_block=transformerblock.TransformerBlock).to(dev).train()
    assert any(isinstance(m, transformerblock.EPA) for m in net.modules())
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, transformerblock.TransformerBlock):
                m.gamma.fill_(0.5)
    y = net(torch.randn(1, 1, 32, 32, 32).to(dev))
    y.square().mean().backward()
    for k, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, k
