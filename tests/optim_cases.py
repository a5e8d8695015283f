"""Shared cases of the optimizer tests (tests/test_optim_emu.py on the wavefront emulator, tests/test_optim_gpu.py on the MI355X): tensor lists at
the sizes where csrc/cl_optim.hip can go wrong, the trainers' hyperparameter rows, and one checked step — the kernels' result against the float64
restatement (tests/optim_ref.py) applied to the kernels' own previous float32 state, under bounds derived from fp32 rounding; torch's CPU float32
clip_grad_norm_ + torch.optim.SGD is held to the same bounds from the same state (the bounds are not below the reference's own rounding)."""
import ctypes

import torch

from deformablelka_amd import _lib as L
from tests import optim_ref as R

T, C = L.DLKA_OPTIM_TENSORS_PER_LAUNCH, L.DLKA_OPTIM_CHUNK
LR = 0.1   # lr |u| comparable to |p|: a wrong update cannot hide under the rounding of p

# the three trainers' rows: (momentum, nesterov, weight_decay, clip)
HYPER = {
    "synapse3d": dict(momentum=0.99, nesterov=True, weight_decay=3e-5, clip=12.0),    # d_lka_former_trainer_synapse.py:197-205, :291-309
    "maxvit2d": dict(momentum=0.9, nesterov=False, weight_decay=1e-4, clip=None),     # trainer_MaxViT_deform_LKA.py:114
    "no_momentum": dict(momentum=0.0, nesterov=False, weight_decay=1e-4, clip=12.0),
}


def spec(n, off="", grad=True, transposed=False):
    """One tensor: n elements (or a 2-D shape); off: which of 'p', 'g', 'b' are views one element off 16-byte alignment."""
    return dict(shape=n if isinstance(n, tuple) else (n,), off=off, grad=grad, transposed=transposed)


def _cycle(n):
    sizes = [1, 3, 4, 5, 7, 16, 33, 255, 257]
    return [spec(sizes[i % len(sizes)]) for i in range(n)]


OFF_SIZES = [257, C + 1, 5, 4, 2 * C]
LISTS = {
    "sizes": [spec(n) for n in (1, 3, 4, 5, 255, 256, 257, C - 1, C, C + 1, 2 * C + 3, 0)] + [spec(9, grad=False), spec(6)],
    "cut_minus_1": _cycle(T - 1),
    "cut_exact": _cycle(T),
    "cut_plus_1": _cycle(T + 1),
    "cut_twice_plus_1": _cycle(2 * T + 1),
    "off_param": [spec(n, off="p") for n in OFF_SIZES],
    "off_grad": [spec(n, off="g") for n in OFF_SIZES],
    "off_buf": [spec(n, off="b") for n in OFF_SIZES],
    "off_all": [spec(n, off="pgb") for n in OFF_SIZES],
    "aligned_twin": [spec(n) for n in OFF_SIZES],   # off_all's values at aligned addresses
    "layout": [spec((6, 10), transposed=True), spec((3, 5, 7)), spec((64, 65), transposed=True)],
}


def place(values, off, device):
    """`values` on `device`, contiguous, at a 16-byte aligned address or (off) one element past one."""
    n = values.numel()
    if off:
        base = torch.zeros(n + 8, dtype=torch.float32, device=device)
        t = base[1:n + 1].view(values.shape)
    else:
        t = torch.zeros(values.shape, dtype=torch.float32, device=device)
    t.copy_(values)
    if n:
        assert t.data_ptr() % 16 == (4 if off else 0)
    return t


def make_params(specs, device, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return [place(torch.randn(s["shape"], generator=gen), "p" in s["off"], device).requires_grad_(True) for s in specs]


def make_grads(specs, device, seed, scale=1.0):
    """One gradient per tensor (None without one); `transposed`: the values in the transposed layout, so that the strides differ from the parameter's."""
    gen = torch.Generator().manual_seed(1000 + seed)
    out = []
    for s in specs:
        v = torch.randn(s["shape"], generator=gen) * scale
        if not s["grad"]:
            out.append(None)
        elif s["transposed"]:
            g = place(v.t().contiguous(), False, device).t()
            assert g.stride() != v.stride()
            out.append(g)
        else:
            out.append(place(v, "g" in s["off"], device))
    return out


def make_optimizer(params, specs, hyper, lrs=(LR,), max_grad_norm=None):
    """optim.SGD over len(lrs) groups (the list cut into equal runs); misaligned momentum buffers ('b') are put into the state as zero views."""
    from deformablelka_amd import optim
    k = len(lrs)
    per = (len(params) + k - 1) // k
    groups = [dict(params=params[i * per:(i + 1) * per], lr=lrs[i]) for i in range(k)]
    opt = optim.SGD(groups, lrs[0], momentum=hyper["momentum"], weight_decay=hyper["weight_decay"], nesterov=hyper["nesterov"],
                    max_grad_norm=max_grad_norm)
    if hyper["momentum"] != 0:
        for p, s in zip(params, specs):
            if "b" in s["off"] and s["grad"]:
                opt.state[p]["momentum_buffer"] = place(torch.zeros(s["shape"]), True, p.device)
    return opt


def group_lr(opt, params):
    lr = {}
    for g in opt.param_groups:
        for p in g["params"]:
            lr[id(p)] = float(g["lr"])
    return [lr[id(p)] for p in params]


REACHED = {"norm": 0.0, "buf": 0.0, "param": 0.0, "torch_buf": 0.0, "torch_param": 0.0}   # largest error / bound seen by this process


def _ratio(err, bound):
    if err.numel() == 0:
        return 0.0
    r = err / bound.clamp_min(1e-300)
    r = torch.where((err == 0) & (bound == 0), torch.zeros_like(r), r)
    return float(r.max())


def _torch_cpu_step(p_old, grads, buf_old, lrs, hyper):
    """torch's own float32 step on the CPU from the same state: the reference implementation."""
    ps, opts = [], []
    for p, g, b, lr in zip(p_old, grads, buf_old, lrs):
        q = p.clone().requires_grad_(True)
        ps.append(q)
        if g is None:
            continue
        q.grad = g.clone()
        o = torch.optim.SGD([q], lr, momentum=hyper["momentum"], weight_decay=hyper["weight_decay"], nesterov=hyper["nesterov"])
        if b is not None and hyper["momentum"] != 0:
            o.state[q]["momentum_buffer"] = b.clone()
        opts.append((o, q))
    if hyper["clip"] is not None:
        torch.nn.utils.clip_grad_norm_(ps, hyper["clip"])
    for o, _ in opts:
        o.step()
    bufs = {id(q): o.state[q].get("momentum_buffer") for o, q in opts}
    return [q.detach() for q in ps], [bufs.get(id(q)) for q in ps]


def checked_step(opt, params, grads, hyper, label=""):
    """Sets the gradients, steps, and holds parameters, buffers and norm to the bounds; returns the new (params, bufs) on the CPU."""
    p_old = [p.detach().cpu().clone() for p in params]
    buf_old = [opt.state[p]["momentum_buffer"].detach().cpu().clone() if opt.state.get(p, {}).get("momentum_buffer") is not None else None
               for p in params]
    g_cpu = [None if g is None else g.detach().cpu().contiguous().clone() for g in grads]
    for p, g in zip(params, grads):
        p.grad = g
    lrs = group_lr(opt, params)
    opt.step(max_grad_norm=hyper["clip"])
    p_new = [p.detach().cpu().clone() for p in params]
    buf_new = [opt.state[p]["momentum_buffer"].detach().cpu().clone() if opt.state.get(p, {}).get("momentum_buffer") is not None else None
               for p in params]
    for g, g0 in zip(grads, g_cpu):   # the step does not write the gradients
        assert g is None or torch.equal(g.detach().cpu(), g0)
    norm64 = R.grad_norm([g for g in g_cpu if g is not None])
    coef = R.clip_coef(norm64, hyper["clip"])
    if hyper["clip"] is not None:
        got = float(opt.last_grad_norm)
        err = abs(got - float(norm64))
        REACHED["norm"] = max(REACHED["norm"], err / (2.0 ** -23 * float(norm64)) if float(norm64) > 0 else 0.0)
        print(f"{label} norm {got:.9g} ref {float(norm64):.17g} rel err {err / max(float(norm64), 1e-300):.3e}")
        assert err <= 2.0 ** -23 * float(norm64)
    else:
        assert opt.last_grad_norm is None
    tp, tb = _torch_cpu_step(p_old, g_cpu, buf_old, lrs, hyper)
    worst = dict(buf=0.0, param=0.0, torch_buf=0.0, torch_param=0.0)
    for i, (po, g, bo, lr) in enumerate(zip(p_old, g_cpu, buf_old, lrs)):
        if g is None:
            assert torch.equal(p_new[i], po) and buf_new[i] is None
            continue
        p64, b64, gc = R.sgd_step(po, g.view(po.shape), bo, coef, lr, hyper["momentum"], hyper["weight_decay"], hyper["nesterov"])
        bb, pb = R.bounds(po, gc, bo, lr, hyper["momentum"], hyper["weight_decay"])
        worst["param"] = max(worst["param"], _ratio((p_new[i].double() - p64).abs(), pb))
        worst["torch_param"] = max(worst["torch_param"], _ratio((tp[i].double() - p64).abs(), pb))
        if hyper["momentum"] != 0:
            worst["buf"] = max(worst["buf"], _ratio((buf_new[i].double() - b64).abs(), bb))
            worst["torch_buf"] = max(worst["torch_buf"], _ratio((tb[i].double() - b64).abs(), bb))
            assert buf_new[i].stride() == po.stride()
        else:
            assert buf_new[i] is None
    for k, v in worst.items():
        REACHED[k] = max(REACHED[k], v)
    print(f"{label} error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert worst["torch_param"] <= 1.0 and worst["torch_buf"] <= 1.0, "the bounds are below torch's own CPU float32 rounding"
    assert worst["param"] <= 1.0 and worst["buf"] <= 1.0
    return p_new, buf_new


def run_list(name, hyper_name, device, steps=2, lrs=(LR,), grad_scale=1.0, schedule=None):
    """`steps` checked steps of list `name` from seed 0; schedule(step) -> the learning rate of group 0 for that step."""
    specs, hyper = LISTS[name], HYPER[hyper_name]
    params = make_params(specs, device)
    opt = make_optimizer(params, specs, hyper, lrs)
    out = None
    for k in range(steps):
        if schedule is not None:
            opt.param_groups[0]["lr"] = schedule(k)
        out = checked_step(opt, params, make_grads(specs, device, k, grad_scale), hyper, f"{name}/{hyper_name} step {k}:")
    norm = None if opt.last_grad_norm is None else opt.last_grad_norm.detach().cpu().clone()
    return out[0], out[1], norm


def same_bits(a, b):
    assert len(a[0]) == len(b[0])
    for x, y in zip(a[0] + a[1], b[0] + b[1]):
        assert (x is None and y is None) or torch.equal(x, y)
    assert (a[2] is None and b[2] is None) or torch.equal(a[2], b[2])


# ---- non-finite gradients ------------------------------------------------------------------------------------------------------------------------------
def check_nonfinite(bad, device):
    """One inf / nan gradient element: the parameters torch's CPU step gives — the same NaN positions, finite values within twice the parameter
    bound of each other (each is within the bound of the exact step)."""
    specs, hyper = [spec(257), spec(C + 1), spec(5)], HYPER["synapse3d"]
    params = make_params(specs, device)
    grads = make_grads(specs, device, 0)
    grads[1][C] = bad
    opt = make_optimizer(params, specs, hyper)
    p_old = [p.detach().cpu().clone() for p in params]
    g_cpu = [g.detach().cpu().clone() for g in grads]
    for p, g in zip(params, grads):
        p.grad = g
    opt.step(max_grad_norm=hyper["clip"])
    tp, _ = _torch_cpu_step(p_old, g_cpu, [None] * 3, [LR] * 3, hyper)
    for p, q, po, g in zip(params, tp, p_old, g_cpu):
        got = p.detach().cpu()
        assert torch.equal(torch.isnan(got), torch.isnan(q))
        _, pb = R.bounds(po, torch.zeros_like(po, dtype=torch.float64), None, LR, hyper["momentum"], hyper["weight_decay"])   # (g_c = g * 0)
        ok = ~torch.isnan(q)
        assert ((got.double() - q.double()).abs()[ok] <= 2 * pb[ok]).all()
    norm = float(opt.last_grad_norm)
    assert norm != norm if bad != bad else norm == float("inf")
    n_nan = sum(int(torch.isnan(p.detach()).sum()) for p in params)
    assert n_nan == (1 if bad == float("inf") else sum(p.numel() for p in params))   # inf * 0 in that element; a NaN norm everywhere


# ---- state dicts ----------------------------------------------------------------------------------------------------------------------------------------
STATE_SPECS = [spec(257), spec(C + 1), spec((6, 10)), spec(5)]


def check_state_dict_torch_to_hip(device):
    hyper = HYPER["synapse3d"]
    cpu = make_params(STATE_SPECS, "cpu")
    ref = torch.optim.SGD(cpu, LR, momentum=hyper["momentum"], weight_decay=hyper["weight_decay"], nesterov=hyper["nesterov"])
    for k in range(2):
        for p, g in zip(cpu, make_grads(STATE_SPECS, "cpu", k)):
            p.grad = g
        torch.nn.utils.clip_grad_norm_(cpu, hyper["clip"])
        ref.step()
    params = [place(p.detach(), False, device).requires_grad_(True) for p in cpu]
    opt = make_optimizer(params, STATE_SPECS, hyper)
    opt.load_state_dict(ref.state_dict())
    for p, q in zip(params, cpu):
        assert torch.equal(opt.state[p]["momentum_buffer"].cpu(), ref.state[q]["momentum_buffer"])
    checked_step(opt, params, make_grads(STATE_SPECS, device, 2), hyper, "state_dict torch -> hip:")


def check_state_dict_hip_to_torch(device):
    hyper = HYPER["synapse3d"]
    params = make_params(STATE_SPECS, device)
    opt = make_optimizer(params, STATE_SPECS, hyper)
    for k in range(2):
        p_cpu, b_cpu = checked_step(opt, params, make_grads(STATE_SPECS, device, k), hyper, "state_dict hip -> torch:")
    cpu = [p.clone().requires_grad_(True) for p in p_cpu]
    ref = torch.optim.SGD(cpu, LR, momentum=hyper["momentum"], weight_decay=hyper["weight_decay"], nesterov=hyper["nesterov"])
    ref.load_state_dict(opt.state_dict())
    g = make_grads(STATE_SPECS, "cpu", 2)
    g0 = [x.clone() for x in g]
    for p, x in zip(cpu, g):
        p.grad = x
    torch.nn.utils.clip_grad_norm_(cpu, hyper["clip"])
    ref.step()
    coef = R.clip_coef(R.grad_norm(g0), hyper["clip"])
    for q, po, bo, x in zip(cpu, p_cpu, b_cpu, g0):
        p64, b64, gc = R.sgd_step(po, x, bo, coef, LR, hyper["momentum"], hyper["weight_decay"], hyper["nesterov"])
        bb, pb = R.bounds(po, gc, bo, LR, hyper["momentum"], hyper["weight_decay"])
        assert ((q.detach().double() - p64).abs() <= pb).all()
        assert ((ref.state[q]["momentum_buffer"].double() - b64).abs() <= bb).all()


# ---- clip_grad_norm_ -------------------------------------------------------------------------------------------------------------------------------------
def check_clip_grad_norm(name, device, scale):
    from deformablelka_amd import optim
    specs = [s for s in LISTS[name] if not s["transposed"]]
    params = make_params(specs, device)
    grads = make_grads(specs, device, 3, scale)
    g0 = [None if g is None else g.detach().cpu().clone() for g in grads]
    for p, g in zip(params, grads):
        p.grad = g
    norm = optim.clip_grad_norm_(params, 12.0)
    norm64 = R.grad_norm([g for g in g0 if g is not None])
    coef = R.clip_coef(norm64, 12.0)
    assert norm.shape == () and abs(float(norm) - float(norm64)) <= 2.0 ** -23 * float(norm64)
    assert (float(coef) < 1.0) == (scale >= 1.0)
    for p, g in zip(params, g0):
        if g is not None:
            assert ((p.grad.detach().cpu().double() - g.double() * coef).abs() <= 4 * R.EPS * g.double().abs()).all()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------------
def check_refusals(device):
    """Every refusal of include/dlka.h's dlka_optim_* block returns its status and launches nothing."""
    lib = L.get_lib()
    OK, NULL, SHAPE, DTYPE, WS, UNSUP = 0, -1, -4, -6, -7, -8
    t = [torch.zeros(8, dtype=torch.float32, device=device) for _ in range(6)]
    scal = torch.ones(4, dtype=torch.float32, device=device)
    ws = torch.zeros(64, dtype=torch.uint8, device=device)
    n = 2

    def table(ts):
        a = (ctypes.c_void_p * len(ts))()
        for i, x in enumerate(ts):
            a[i] = x.data_ptr()
        return a

    def cnt(*v):
        return (ctypes.c_int64 * len(v))(*v)

    P, G, B, N8 = table(t[0:2]), table(t[2:4]), table(t[4:6]), cnt(8, 8)
    wsp, sp = ctypes.c_void_p(ws.data_ptr()), ctypes.c_void_p(scal.data_ptr())

    def desc(**kw):
        base = dict(n_tensors=n, dtype=L.DLKA_F32, nesterov=1, has_momentum=1, clip=1, momentum=0.9, weight_decay=0.0, max_norm=12.0, lr_index=0)
        base.update(kw)
        return ctypes.byref(L.OptimDesc(**base))

    big = 4097   # 4097 tensors of 2^31 - 1 elements: more than 2^31 - 1 chunks
    BIGP, BIGN = (ctypes.c_void_p * big)(*([t[0].data_ptr()] * big)), cnt(*([2 ** 31 - 1] * big))
    rows = [
        ("norm: NULL table", lambda: lib.dlka_optim_grad_norm(None, N8, n, 0, wsp, 64, sp, None), NULL),
        ("norm: NULL counts", lambda: lib.dlka_optim_grad_norm(G, None, n, 0, wsp, 64, sp, None), NULL),
        ("norm: NULL norm_out", lambda: lib.dlka_optim_grad_norm(G, N8, n, 0, wsp, 64, None, None), NULL),
        ("norm: n < 0", lambda: lib.dlka_optim_grad_norm(G, N8, -1, 0, wsp, 64, sp, None), SHAPE),
        ("norm: negative count", lambda: lib.dlka_optim_grad_norm(G, cnt(8, -1), n, 0, wsp, 64, sp, None), SHAPE),
        ("norm: dtype", lambda: lib.dlka_optim_grad_norm(G, N8, n, L.DLKA_BF16, wsp, 64, sp, None), DTYPE),
        ("norm: count over 2^31 - 1", lambda: lib.dlka_optim_grad_norm(G, cnt(8, 2 ** 31), n, 0, wsp, 64, sp, None), UNSUP),
        ("norm: chunk total over 2^31 - 1", lambda: lib.dlka_optim_grad_norm(BIGP, BIGN, big, 0, wsp, 64, sp, None), UNSUP),
        ("norm: NULL tensor address", lambda: lib.dlka_optim_grad_norm((ctypes.c_void_p * 2)(), N8, n, 0, wsp, 64, sp, None), NULL),
        ("norm: NULL workspace", lambda: lib.dlka_optim_grad_norm(G, N8, n, 0, None, 64, sp, None), WS),
        ("norm: small workspace", lambda: lib.dlka_optim_grad_norm(G, N8, n, 0, wsp, 8, sp, None), WS),
        ("norm: misaligned workspace", lambda: lib.dlka_optim_grad_norm(G, N8, n, 0, ctypes.c_void_p(ws.data_ptr() + 4), 60, sp, None), WS),
        ("norm: empty list", lambda: lib.dlka_optim_grad_norm(None, None, 0, 0, None, 0, None, None), OK),
        ("scale: NULL table", lambda: lib.dlka_optim_scale(None, N8, n, 0, sp, 12.0, None), NULL),
        ("scale: NULL norm", lambda: lib.dlka_optim_scale(G, N8, n, 0, None, 12.0, None), NULL),
        ("scale: n < 0", lambda: lib.dlka_optim_scale(G, N8, -2, 0, sp, 12.0, None), SHAPE),
        ("scale: negative count", lambda: lib.dlka_optim_scale(G, cnt(-8, 8), n, 0, sp, 12.0, None), SHAPE),
        ("scale: dtype", lambda: lib.dlka_optim_scale(G, N8, n, L.DLKA_F64, sp, 12.0, None), DTYPE),
        ("scale: count over 2^31 - 1", lambda: lib.dlka_optim_scale(G, cnt(2 ** 31, 8), n, 0, sp, 12.0, None), UNSUP),
        ("scale: empty list", lambda: lib.dlka_optim_scale(G, N8, 0, 0, sp, 12.0, None), OK),
        ("step: NULL descriptor", lambda: lib.dlka_optim_sgd_step(P, G, B, N8, None, sp, sp, None), NULL),
        ("step: NULL params", lambda: lib.dlka_optim_sgd_step(None, G, B, N8, desc(), sp, sp, None), NULL),
        ("step: NULL grads", lambda: lib.dlka_optim_sgd_step(P, None, B, N8, desc(), sp, sp, None), NULL),
        ("step: NULL counts", lambda: lib.dlka_optim_sgd_step(P, G, B, None, desc(), sp, sp, None), NULL),
        ("step: NULL bufs with has_momentum", lambda: lib.dlka_optim_sgd_step(P, G, None, N8, desc(), sp, sp, None), NULL),
        ("step: NULL norm_dev with clip", lambda: lib.dlka_optim_sgd_step(P, G, B, N8, desc(), sp, None, None), NULL),
        ("step: NULL lr_dev", lambda: lib.dlka_optim_sgd_step(P, G, B, N8, desc(), None, sp, None), NULL),
        ("step: n_tensors < 0", lambda: lib.dlka_optim_sgd_step(P, G, B, N8, desc(n_tensors=-1), sp, sp, None), SHAPE),
        ("step: negative count", lambda: lib.dlka_optim_sgd_step(P, G, B, cnt(8, -8), desc(), sp, sp, None), SHAPE),
        ("step: dtype", lambda: lib.dlka_optim_sgd_step(P, G, B, N8, desc(dtype=L.DLKA_BF16), sp, sp, None), DTYPE),
        ("step: count over 2^31 - 1", lambda: lib.dlka_optim_sgd_step(P, G, B, cnt(8, 2 ** 31), desc(), sp, sp, None), UNSUP),
        ("step: chunk total over 2^31 - 1", lambda: lib.dlka_optim_sgd_step(BIGP, BIGP, BIGP, BIGN, desc(n_tensors=big), sp, sp, None), UNSUP),
        ("step: empty list", lambda: lib.dlka_optim_sgd_step(None, None, None, None, desc(n_tensors=0), None, None, None), OK),
    ]
    for what, call, want in rows:
        before = lib.dlka_optim_launch_count()
        got = call()
        assert got == want, (what, got, want)
        assert lib.dlka_optim_launch_count() == before, what
    assert lib.dlka_optim_workspace_bytes(N8, n) == 16 and lib.dlka_optim_workspace_bytes(cnt(C + 1, 0, 1), 3) == 24
    assert lib.dlka_optim_workspace_bytes(cnt(8, -1), 2) == 0 and lib.dlka_optim_workspace_bytes(None, 2) == 0
    assert all(float(x.abs().sum()) == 0 for x in t)   # nothing was written


def check_not_implemented(device):
    import pytest
    from deformablelka_amd import optim
    p = [torch.zeros(4, device=device, requires_grad=True)]
    for kw, word in ((dict(dampening=0.1), "dampening"), (dict(maximize=True), "maximize"), (dict(differentiable=True), "differentiable")):
        with pytest.raises(NotImplementedError, match=word):
            optim.SGD(p, 0.1, momentum=0.9, **kw)
    with pytest.raises(NotImplementedError, match="params"):
        optim.SGD([torch.zeros(4, dtype=torch.float64, device=device, requires_grad=True)], 0.1)
    with pytest.raises(NotImplementedError, match="params"):
        optim.SGD([torch.zeros(4, 4, device=device)[:, ::2].requires_grad_(True)], 0.1)
    if device == "cpu":   # (sparse tensors: host logic only)
        opt = optim.SGD(p, 0.1)
        p[0].grad = torch.zeros(4).to_sparse()
        with pytest.raises(NotImplementedError, match="sparse"):
            opt.step()
        with pytest.raises(NotImplementedError, match="sparse"):
            optim.clip_grad_norm_(p, 1.0)
    p[0].grad = torch.zeros(4, device=device)
    with pytest.raises(NotImplementedError, match="norm_type"):
        optim.clip_grad_norm_(p, 1.0, norm_type=1.0)
    with pytest.raises(NotImplementedError, match="norm_type"):
        optim.clip_grad_norm_(p, 1.0, norm_type=float("inf"))
    with pytest.raises(NotImplementedError, match="error_if_nonfinite"):
        optim.clip_grad_norm_(p, 1.0, error_if_nonfinite=True)
    ref = torch.optim.SGD([torch.zeros(4, requires_grad=True)], 0.1, momentum=0.9, dampening=0.5)
    with pytest.raises(NotImplementedError, match="dampening"):
        optim.SGD(p, 0.1, momentum=0.9).load_state_dict(ref.state_dict())


def check_interface(device):
    """torch's argument names and order, poly_lr, the class attributes training.py tests for, lr uploads."""
    import inspect
    from deformablelka_amd import optim
    names = list(inspect.signature(optim.SGD.__init__).parameters)
    assert names[:7] == ["self", "params", "lr", "momentum", "dampening", "weight_decay", "nesterov"] and "max_grad_norm" in names
    assert list(inspect.signature(optim.clip_grad_norm_).parameters) == ["parameters", "max_norm", "norm_type", "error_if_nonfinite", "foreach"]
    assert optim.SGD.lr_on_device is True and optim.SGD.clips_in_step is True
    assert optim.poly_lr(3, 10, 0.01) == 0.01 * (1 - 3 / 10) ** 0.9 and optim.poly_lr(0, 5, 0.1, 2.0) == 0.1
    p = [torch.ones(4, device=device, requires_grad=True), torch.ones(3, device=device, requires_grad=True)]
    opt = optim.SGD([dict(params=p[:1]), dict(params=p[1:], lr=0.5)], 0.25, max_grad_norm=None)
    assert set(opt.param_groups[0]) == set(torch.optim.SGD([torch.zeros(1, requires_grad=True)], 0.1).param_groups[0])
    opt.sync_lr()
    assert opt.lr_tensor.dtype == torch.float32 and opt.lr_tensor.cpu().tolist() == [0.25, 0.5]
    held = opt.lr_tensor
    opt.sync_lr()
    assert opt.lr_tensor is held
    opt.param_groups[1]["lr"] = 0.125
    for q in p:
        q.grad = torch.ones_like(q)
    opt.step()   # momentum 0, no clip: p -= lr
    assert opt.lr_tensor.cpu().tolist() == [0.25, 0.125] and opt.last_grad_norm is None
    assert p[0].detach().cpu().tolist() == [0.75] * 4 and p[1].detach().cpu().tolist() == [0.875] * 3
    assert opt.state_dict()["state"] == {}
    p[0].grad, p[1].grad = None, None
    opt.step(max_grad_norm=1.0)   # no gradients at all: nothing moves, the norm is 0
    assert float(opt.last_grad_norm) == 0.0 and p[0].detach().cpu().tolist() == [0.75] * 4


# ---- the small net of the trainer tests (tests/test_tta.py::_lite_net, restated) --------------------------------------------------------------------------
class LiteBlock(torch.nn.Module):
    """Cheap transformer-block stand-in with the reference's constructor signature: tokens, a per-token linear map, back to the volume, a 1x1x1 conv."""

    def __init__(self, input_size, hidden_size, proj_size, num_heads, dropout_rate=0.0, pos_embed=False):
        super().__init__()
        self.lin = torch.nn.Linear(hidden_size, hidden_size)
        self.conv = torch.nn.Conv3d(hidden_size, hidden_size, 1)

    def forward(self, x):
        B, Ch, H, W, D = x.shape
        t = x.reshape(B, Ch, H * W * D).permute(0, 2, 1)
        t = t + torch.tanh(self.lin(t))
        v = t.reshape(B, H, W, D, Ch).permute(0, 4, 1, 2, 3)
        return v + self.conv(v)


def lite_net(k=3):
    import deformablelka_amd as dk
    torch.manual_seed(5)
    return dk.D_LKA_Former(in_channels=1, out_channels=k, img_size=[16, 32, 32], feature_size=4, hidden_size=64, num_heads=4, depths=[1, 1, 1, 1],
                           dims=[8, 16, 32, 64], do_ds=True, trans_block=LiteBlock)
