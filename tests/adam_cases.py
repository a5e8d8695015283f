"""Shared cases of the Adam / AdamW tests (tests/test_adam_emu.py on the wavefront emulator, tests/test_adam_gpu.py on the MI355X): tensor lists at
the sizes where csrc/cl_optim.hip's Adam launches can go wrong, the trainers' hyperparameter rows, and one checked step — the kernels' result
against the float64 restatement (tests/adam_ref.py) applied to the kernels' own previous float32 state, under that file's rounding bounds; torch's
CPU float32 clip_grad_norm_ + Adam / AdamW step from the same state is held to the same bounds in every case."""
import ctypes

import torch

from deformablelka_amd import _lib as L
from tests import adam_ref as R
from tests import optim_ref
from tests.optim_cases import make_grads, make_params, place, spec

T, C = L.DLKA_OPTIM_ADAM_TENSORS_PER_LAUNCH, L.DLKA_OPTIM_CHUNK
LR = 0.1   # an update comparable to |p|: a wrong one cannot hide under the rounding of p

HYPER = {
    "lka2d_adamw": dict(decoupled=True, weight_decay=1e-4, amsgrad=False, clip=None),          # 2D/trainer_MaxViT_LKA.py:114
    "trainer3d_adam": dict(decoupled=False, weight_decay=3e-5, amsgrad=True, clip=12.0),       # Trainer_synapse.py:270-273 (+ the nnFormer trainers' clip)
    "adamw_amsgrad_clip": dict(decoupled=True, weight_decay=1e-2, amsgrad=True, clip=12.0),
    "adam_plain": dict(decoupled=False, weight_decay=0.0, amsgrad=False, clip=None),
}
for _h in HYPER.values():
    _h.update(beta1=0.9, beta2=0.999, eps=1e-8)


def _cycle(n):
    sizes = [1, 3, 4, 5, 7, 16, 33, 255, 257]
    return [spec(sizes[i % len(sizes)]) for i in range(n)]


def _absent_at(s, k):
    s = dict(s)
    s["absent_at"] = k   # no gradient at step k only
    return s


OFF_SIZES = [257, C + 1, 5, 4, 2 * C]
LISTS = {
    "sizes": [spec(n) for n in (1, 3, 4, 5, 255, 256, 257, C - 1, C, C + 1, 2 * C + 3, 0)] + [spec(9, grad=False), _absent_at(spec(6), 1),
                                                                                             _absent_at(spec(0), 1)],
    "cut_minus_1": _cycle(T - 1),
    "cut_exact": _cycle(T),
    "cut_plus_1": _cycle(T + 1),
    "cut_twice_plus_1": _cycle(2 * T + 1),
    "off_param": [spec(n, off="p") for n in OFF_SIZES],
    "off_grad": [spec(n, off="g") for n in OFF_SIZES],
    "off_exp_avg": [spec(n, off="m") for n in OFF_SIZES],
    "off_exp_avg_sq": [spec(n, off="v") for n in OFF_SIZES],
    "off_max_exp_avg_sq": [spec(n, off="x") for n in OFF_SIZES],
    "off_all": [spec(n, off="pgmvx") for n in OFF_SIZES],
    "aligned_twin": [spec(n) for n in OFF_SIZES],   # off_all's values at aligned addresses
    "layout": [spec((6, 10), transposed=True), spec((3, 5, 7)), spec((64, 65), transposed=True)],
}
STATE_KEYS = (("m", "exp_avg"), ("v", "exp_avg_sq"), ("x", "max_exp_avg_sq"))


def make_optimizer(params, specs, hyper, lrs=(LR,), max_grad_norm=None):
    """optim.Adam / AdamW over len(lrs) groups (the list cut into equal runs); misaligned state ('m', 'v', 'x') is put in as zero views."""
    from deformablelka_amd import optim
    k = len(lrs)
    per = (len(params) + k - 1) // k
    groups = [dict(params=params[i * per:(i + 1) * per], lr=lrs[i]) for i in range(k)]
    cls = optim.AdamW if hyper["decoupled"] else optim.Adam
    opt = cls(groups, lrs[0], betas=(hyper["beta1"], hyper["beta2"]), eps=hyper["eps"], weight_decay=hyper["weight_decay"],
              amsgrad=hyper["amsgrad"], max_grad_norm=max_grad_norm)
    for p, s in zip(params, specs):
        for letter, key in STATE_KEYS:
            if letter in s["off"] and s["grad"] and (key != "max_exp_avg_sq" or hyper["amsgrad"]):
                opt.state[p][key] = place(torch.zeros(s["shape"]), True, p.device)
    return opt


def group_lr(opt, params):
    lr = {}
    for g in opt.param_groups:
        for p in g["params"]:
            lr[id(p)] = float(g["lr"])
    return [lr[id(p)] for p in params]


REACHED = {k: 0.0 for k in ("norm", "exp_avg", "exp_avg_sq", "max_exp_avg_sq", "param", "torch_exp_avg", "torch_exp_avg_sq",
                            "torch_max_exp_avg_sq", "torch_param")}   # largest error / bound seen by this process


def _ratio(err, bound):
    if err.numel() == 0:
        return 0.0
    r = err / bound.clamp_min(1e-300)
    r = torch.where((err == 0) & (bound == 0), torch.zeros_like(r), r)
    return float(r.max())


def _state(opt, p):
    """(exp_avg, exp_avg_sq, max_exp_avg_sq, count) of a parameter on the CPU; Nones and 0 before its first step."""
    st = opt.state.get(p, {})
    get = lambda k: st[k].detach().cpu().clone() if st.get(k) is not None else None   # noqa: E731
    return get("exp_avg"), get("exp_avg_sq"), get("max_exp_avg_sq"), float(st["step"]) if "step" in st else 0.0


def torch_class(hyper):
    return torch.optim.AdamW if hyper["decoupled"] else torch.optim.Adam


def _torch_cpu_step(p_old, grads, old, lrs, hyper):
    """torch's own float32 step on the CPU from the same state: the reference implementation."""
    ps, opts = [], []
    for p, g, (m, v, x, t), lr in zip(p_old, grads, old, lrs):
        q = p.clone().requires_grad_(True)
        ps.append(q)
        if g is None:
            continue
        q.grad = g.clone().view(q.shape)
        o = torch_class(hyper)([q], lr, betas=(hyper["beta1"], hyper["beta2"]), eps=hyper["eps"], weight_decay=hyper["weight_decay"],
                               amsgrad=hyper["amsgrad"])
        if m is not None and v is not None:
            st = dict(step=torch.tensor(t), exp_avg=m.clone(), exp_avg_sq=v.clone())
            if hyper["amsgrad"]:
                st["max_exp_avg_sq"] = x.clone() if x is not None else torch.zeros_like(m)
            o.state[q] = st
        opts.append((o, q))
    if hyper["clip"] is not None:
        torch.nn.utils.clip_grad_norm_(ps, hyper["clip"])
    for o, _ in opts:
        o.step()
    state = {id(q): o.state[q] for o, q in opts}
    return [q.detach() for q in ps], [state.get(id(q)) for q in ps]


def checked_step(opt, params, grads, hyper, want_counts, label=""):
    """Sets the gradients, steps, and holds parameters, state, counts and norm to the bounds; want_counts: the counts after this step."""
    p_old = [p.detach().cpu().clone() for p in params]
    old = [_state(opt, p) for p in params]
    g_cpu = [None if g is None else g.detach().cpu().contiguous().clone() for g in grads]
    for p, g in zip(params, grads):
        p.grad = g
    lrs = group_lr(opt, params)
    opt.step(max_grad_norm=hyper["clip"])
    p_new = [p.detach().cpu().clone() for p in params]
    new = [_state(opt, p) for p in params]
    for g, g0 in zip(grads, g_cpu):   # the step does not write the gradients
        assert g is None or torch.equal(g.detach().cpu(), g0)
    assert [n[3] for n in new] == [float(c) for c in want_counts], (label, [n[3] for n in new], want_counts)
    for p in params:
        if "step" in opt.state.get(p, {}):
            s = opt.state[p]["step"]
            assert s.dim() == 0 and s.dtype == torch.float32 and s.device == p.device
    norm64 = optim_ref.grad_norm([g for g in g_cpu if g is not None])
    coef = optim_ref.clip_coef(norm64, hyper["clip"])
    if hyper["clip"] is not None:
        got = float(opt.last_grad_norm)
        err = abs(got - float(norm64))
        REACHED["norm"] = max(REACHED["norm"], err / (2.0 ** -23 * float(norm64)) if float(norm64) > 0 else 0.0)
        assert err <= 2.0 ** -23 * float(norm64)
    else:
        assert opt.last_grad_norm is None
    tp, ts = _torch_cpu_step(p_old, g_cpu, old, lrs, hyper)
    worst = {k: 0.0 for k in REACHED if k != "norm"}
    for i, (po, g, (m, v, x, t), lr) in enumerate(zip(p_old, g_cpu, old, lrs)):
        if g is None:
            assert torch.equal(p_new[i], po) and new[i][3] == t
            for a, b in zip(new[i][:3], (m, v, x)):
                assert (a is None and b is None) or torch.equal(a, b)
            continue
        assert new[i][3] == t + 1
        ref = R.adam_step(po, g.view(po.shape), m, v, x, t + 1, coef, lr, hyper)
        got = dict(param=p_new[i], exp_avg=new[i][0], exp_avg_sq=new[i][1], max_exp_avg_sq=new[i][2])
        tor = dict(param=tp[i], exp_avg=ts[i]["exp_avg"], exp_avg_sq=ts[i]["exp_avg_sq"], max_exp_avg_sq=ts[i].get("max_exp_avg_sq"))
        assert float(ts[i]["step"]) == t + 1
        for key, rk, bk in (("param", "p", "bound_p"), ("exp_avg", "m", "bound_m"), ("exp_avg_sq", "v", "bound_v"),
                            ("max_exp_avg_sq", "vmax", "bound_v")):
            if ref[rk] is None:
                assert got[key] is None
                continue
            assert got[key].stride() == po.stride() and got[key].shape == po.shape
            worst[key] = max(worst[key], _ratio((got[key].double() - ref[rk]).abs(), ref[bk]))
            worst["torch_" + key] = max(worst["torch_" + key], _ratio((tor[key].double() - ref[rk]).abs(), ref[bk]))
    for k, val in worst.items():
        REACHED[k] = max(REACHED[k], val)
    print(f"{label} error / bound: " + ", ".join(f"{k} {val:.3f}" for k, val in worst.items()))
    assert all(val <= 1.0 for k, val in worst.items() if k.startswith("torch_")), "the bounds are below torch's own CPU float32 rounding"
    assert all(val <= 1.0 for val in worst.values())
    return p_new, new


def run_list(name, hyper_name, device, steps=3, lrs=(LR,), grad_scale=1.0, schedule=None):
    """`steps` checked steps of list `name` from seed 0 (three by default: the bias corrections make step 1 special, and the 'absent_at' tensors
    miss step 2); schedule(step) -> the learning rate of group 0 for that step."""
    specs, hyper = LISTS[name], HYPER[hyper_name]
    params = make_params(specs, device)
    opt = make_optimizer(params, specs, hyper, lrs)
    counts = [0] * len(specs)
    out = None
    for k in range(steps):
        if schedule is not None:
            opt.param_groups[0]["lr"] = schedule(k)
        grads = make_grads(specs, device, k, grad_scale)
        for i, s in enumerate(specs):
            if s.get("absent_at") == k:
                grads[i] = None
            counts[i] += grads[i] is not None
        out = checked_step(opt, params, grads, hyper, counts, f"{name}/{hyper_name} step {k}:")
    norm = None if opt.last_grad_norm is None else opt.last_grad_norm.detach().cpu().clone()
    return out[0], out[1], norm


def same_bits(a, b):
    assert len(a[0]) == len(b[0])
    for x, y in zip(a[0], b[0]):
        assert torch.equal(x, y)
    for sa, sb in zip(a[1], b[1]):
        assert sa[3] == sb[3]
        for x, y in zip(sa[:3], sb[:3]):
            assert (x is None and y is None) or torch.equal(x, y)
    assert (a[2] is None and b[2] is None) or torch.equal(a[2], b[2])


# ---- non-finite gradients ------------------------------------------------------------------------------------------------------------------------------
def check_nonfinite(bad, hyper_name, device):
    """One inf / nan gradient element, two steps (the second runs on the state the first left): the NaN positions of torch's CPU step in the
    parameters and in every state tensor."""
    specs, hyper = [spec(257), spec(C + 1), spec(5)], HYPER[hyper_name]
    params = make_params(specs, device)
    opt = make_optimizer(params, specs, hyper)
    for k in range(2):
        grads = make_grads(specs, device, k)
        if k == 0:
            grads[1][C] = bad
        p_old = [p.detach().cpu().clone() for p in params]
        old = [_state(opt, p) for p in params]
        g_cpu = [g.detach().cpu().clone() for g in grads]
        for p, g in zip(params, grads):
            p.grad = g
        opt.step(max_grad_norm=hyper["clip"])
        tp, ts = _torch_cpu_step(p_old, g_cpu, old, [LR] * 3, hyper)
        n_nan = 0
        for p, q, st in zip(params, tp, ts):
            got = [p.detach().cpu()] + list(_state(opt, p)[:3])
            want = [q, st["exp_avg"], st["exp_avg_sq"], st.get("max_exp_avg_sq")]
            for a, b in zip(got, want):
                assert (a is None) == (b is None)
                if a is not None:
                    assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.isinf(a), torch.isinf(b))
            n_nan += int(torch.isnan(got[0]).sum())
        if k == 0:   # with a clip the norm is inf or NaN: coef 0 (inf * 0 in that element alone) or NaN (everywhere); without, that element alone
            everywhere = hyper["clip"] is not None and bad != bad
            assert n_nan == (sum(p.numel() for p in params) if everywhere else 1)


# ---- state dicts ----------------------------------------------------------------------------------------------------------------------------------------
STATE_SPECS = [spec(257), spec(C + 1), spec((6, 10)), spec(5)]


def _torch_optimizer(params, hyper):
    return torch_class(hyper)(params, LR, betas=(hyper["beta1"], hyper["beta2"]), eps=hyper["eps"], weight_decay=hyper["weight_decay"],
                              amsgrad=hyper["amsgrad"])


def check_state_dict_torch_to_hip(hyper_name, device):
    hyper = HYPER[hyper_name]
    cpu = make_params(STATE_SPECS, "cpu")
    ref = _torch_optimizer(cpu, hyper)
    for k in range(2):
        for p, g in zip(cpu, make_grads(STATE_SPECS, "cpu", k)):
            p.grad = g
        if hyper["clip"] is not None:
            torch.nn.utils.clip_grad_norm_(cpu, hyper["clip"])
        ref.step()
    params = [place(p.detach(), False, device).requires_grad_(True) for p in cpu]
    opt = make_optimizer(params, STATE_SPECS, hyper)
    opt.load_state_dict(ref.state_dict())
    lo, hi = opt._steps.data_ptr(), opt._steps.data_ptr() + 4 * opt._steps.numel()
    for p, q in zip(params, cpu):
        for key in ref.state[q]:
            assert torch.equal(opt.state[p][key].cpu(), ref.state[q][key]), key
        s = opt.state[p]["step"]
        assert float(s) == 2.0 and s.dim() == 0 and s.dtype == torch.float32 and s.device == p.device and lo <= s.data_ptr() < hi
    assert all(g["capturable"] for g in opt.param_groups)
    checked_step(opt, params, make_grads(STATE_SPECS, device, 2), hyper, [3] * 4, f"state_dict torch -> hip, {hyper_name}:")


def check_state_dict_hip_to_torch(hyper_name, device):
    """The hand-over to torch's class on the CPU (the reference implementation of every check here).  torch runs capturable=True on a GPU only,
    so a hand-over to CPU parameters clears the flag in the dict."""
    hyper = HYPER[hyper_name]
    params = make_params(STATE_SPECS, device)
    opt = make_optimizer(params, STATE_SPECS, hyper)
    for k in range(2):
        p_cpu, st_cpu = checked_step(opt, params, make_grads(STATE_SPECS, device, k), hyper, [k + 1] * 4, f"state_dict hip -> torch, {hyper_name}:")
    theirs = [p.clone().requires_grad_(True) for p in p_cpu]
    ref = _torch_optimizer(theirs, hyper)
    sd = opt.state_dict()
    for g in sd["param_groups"]:
        g["capturable"] = False
    ref.load_state_dict(sd)
    g = make_grads(STATE_SPECS, "cpu", 2)
    g0 = [x.detach().cpu().clone() for x in g]
    for p, x in zip(theirs, g):
        p.grad = x
    if hyper["clip"] is not None:
        torch.nn.utils.clip_grad_norm_(theirs, hyper["clip"])
    ref.step()
    coef = optim_ref.clip_coef(optim_ref.grad_norm(g0), hyper["clip"])
    for q, po, (m, v, x, t), gr in zip(theirs, p_cpu, st_cpu, g0):
        r = R.adam_step(po, gr, m, v, x, t + 1, coef, LR, hyper)
        st = ref.state[q]
        assert float(st["step"]) == 3.0
        assert ((q.detach().cpu().double() - r["p"]).abs() <= r["bound_p"]).all()
        assert ((st["exp_avg"].cpu().double() - r["m"]).abs() <= r["bound_m"]).all()
        assert ((st["exp_avg_sq"].cpu().double() - r["v"]).abs() <= r["bound_v"]).all()
        if hyper["amsgrad"]:
            assert ((st["max_exp_avg_sq"].cpu().double() - r["vmax"]).abs() <= r["bound_v"]).all()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------------
def check_refusals(device):
    """Every refusal of include/dlka.h's dlka_optim_adam_step returns its status, launches nothing and writes nothing."""
    lib = L.get_lib()
    OK, NULL, SHAPE, DTYPE, WS, UNSUP = 0, -1, -4, -6, -7, -8
    t = [torch.zeros(8, dtype=torch.float32, device=device) for _ in range(12)]
    scal = torch.ones(4, dtype=torch.float32, device=device)
    ws = torch.zeros(16, dtype=torch.float32, device=device)
    n = 2

    def table(ts):
        a = (ctypes.c_void_p * len(ts))()
        for i, x in enumerate(ts):
            a[i] = x.data_ptr()
        return a

    def cnt(*v):
        return (ctypes.c_int64 * len(v))(*v)

    P, G, M, V, X, S, N8 = table(t[0:2]), table(t[2:4]), table(t[4:6]), table(t[6:8]), table(t[8:10]), table(t[10:12]), cnt(8, 8)
    wsp, sp = ctypes.c_void_p(ws.data_ptr()), ctypes.c_void_p(scal.data_ptr())
    HOLE = (ctypes.c_void_p * 2)()
    HOLE[0] = t[0].data_ptr()

    def desc(**kw):
        base = dict(n_tensors=n, dtype=L.DLKA_F32, decoupled=1, amsgrad=1, clip=1, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, max_norm=12.0,
                    lr_index=0)
        base.update(kw)
        return ctypes.byref(L.OptimAdamDesc(**base))

    def call(p=P, g=G, m=M, v=V, x=X, s=S, c=N8, d=None, lr=sp, norm=sp, w=wsp, wb=64):
        return lib.dlka_optim_adam_step(p, g, m, v, x, s, c, d if d is not None else desc(), lr, norm, w, wb, None)

    big = 4097   # 4097 tensors of 2^31 - 1 elements: more than 2^31 - 1 chunks
    BIGP, BIGN = (ctypes.c_void_p * big)(*([t[0].data_ptr()] * big)), cnt(*([2 ** 31 - 1] * big))
    rows = [
        ("NULL descriptor", lambda: lib.dlka_optim_adam_step(P, G, M, V, X, S, N8, None, sp, sp, wsp, 64, None), NULL),
        ("NULL params", lambda: call(p=None), NULL),
        ("NULL grads", lambda: call(g=None), NULL),
        ("NULL exp_avg", lambda: call(m=None), NULL),
        ("NULL exp_avg_sq", lambda: call(v=None), NULL),
        ("NULL max_exp_avg_sq with amsgrad", lambda: call(x=None), NULL),
        ("NULL steps", lambda: call(s=None), NULL),
        ("NULL counts", lambda: call(c=None), NULL),
        ("NULL lr_dev", lambda: call(lr=None), NULL),
        ("NULL norm_dev with clip", lambda: call(norm=None), NULL),
        ("n_tensors < 0", lambda: call(d=desc(n_tensors=-1)), SHAPE),
        ("negative count", lambda: call(c=cnt(8, -8)), SHAPE),
        ("negative lr_index", lambda: call(d=desc(lr_index=-1)), SHAPE),
        ("beta1 = 1", lambda: call(d=desc(beta1=1.0)), SHAPE),
        ("beta2 < 0", lambda: call(d=desc(beta2=-0.5)), SHAPE),
        ("eps < 0", lambda: call(d=desc(eps=-1e-8)), SHAPE),
        ("weight_decay NaN", lambda: call(d=desc(weight_decay=float("nan"))), SHAPE),
        ("dtype", lambda: call(d=desc(dtype=L.DLKA_BF16)), DTYPE),
        ("count over 2^31 - 1", lambda: call(c=cnt(8, 2 ** 31)), UNSUP),
        ("chunk total over 2^31 - 1", lambda: call(p=BIGP, g=BIGP, m=BIGP, v=BIGP, x=BIGP, s=BIGP, c=BIGN, d=desc(n_tensors=big), wb=8 * big), UNSUP),
        ("NULL tensor address", lambda: call(m=HOLE), NULL),
        ("NULL count address", lambda: call(s=HOLE), NULL),
        ("NULL workspace", lambda: call(w=None), WS),
        ("small workspace", lambda: call(wb=8), WS),
        ("misaligned workspace", lambda: call(w=ctypes.c_void_p(ws.data_ptr() + 2), wb=62), WS),
        ("empty list", lambda: lib.dlka_optim_adam_step(None, None, None, None, None, None, None, desc(n_tensors=0), None, None, None, 0, None), OK),
    ]
    for what, fn, want in rows:
        before = lib.dlka_optim_launch_count()
        got = fn()
        assert got == want, (what, got, want)
        assert lib.dlka_optim_launch_count() == before, what
    assert lib.dlka_optim_adam_workspace_bytes(2) == 16 and lib.dlka_optim_adam_workspace_bytes(0) == 0 and lib.dlka_optim_adam_workspace_bytes(-3) == 0
    assert all(float(x.abs().sum()) == 0 for x in t) and float(ws.abs().sum()) == 0   # nothing was written
    # the accepted call: one tick launch and one update launch; without amsgrad or clip the optional pointers may be NULL
    before = lib.dlka_optim_launch_count()
    assert call(x=None, norm=None, d=desc(amsgrad=0, clip=0)) == OK
    assert lib.dlka_optim_launch_count() == before + 2
    assert t[10].cpu().tolist() == [1.0] + [0.0] * 7 and t[11].cpu().tolist() == [1.0] + [0.0] * 7
    bc = ws.cpu()[:4].double()
    assert torch.allclose(bc, torch.tensor([0.1, 0.001 ** 0.5] * 2, dtype=torch.float64), rtol=2.0 ** -23, atol=0)


def check_not_implemented(device):
    import pytest
    from deformablelka_amd import optim
    p = [torch.zeros(4, device=device, requires_grad=True)]
    for cls in (optim.Adam, optim.AdamW):
        for kw, word in ((dict(maximize=True), "maximize"), (dict(differentiable=True), "differentiable"), (dict(capturable=False), "capturable"),
                         (dict(lr=torch.tensor(0.1)), "lr"), (dict(betas=(torch.tensor(0.9), 0.999)), "betas")):
            with pytest.raises(NotImplementedError, match=word):
                cls(p, **kw)
        with pytest.raises(NotImplementedError, match="params"):
            cls([torch.zeros(4, dtype=torch.float64, device=device, requires_grad=True)])
        with pytest.raises(NotImplementedError, match="params"):
            cls([torch.zeros(4, 4, device=device)[:, ::2].requires_grad_(True)])
        for kw in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)), dict(betas=(0.9, -0.1)), dict(weight_decay=-1.0)):
            with pytest.raises(ValueError):
                cls(p, **kw)
        cls(p, foreach=True, fused=True)   # accepted, ignored
    opt = optim.Adam(p, amsgrad=True)
    p[0].grad = torch.zeros(4, device=device)
    opt.step()
    opt.state[p[0]]["exp_avg_sq"] = opt.state[p[0]]["exp_avg_sq"].double()
    opt.invalidate_tables()
    with pytest.raises(NotImplementedError, match="exp_avg_sq"):
        opt.step()
    if device == "cpu":   # (sparse tensors: host logic only)
        opt = optim.Adam(p)
        p[0].grad = torch.zeros(4).to_sparse()
        with pytest.raises(NotImplementedError, match="sparse"):
            opt.step()
    ref = torch.optim.Adam([torch.zeros(4, requires_grad=True)], maximize=True)
    with pytest.raises(NotImplementedError, match="maximize"):
        optim.Adam(p).load_state_dict(ref.state_dict())


def check_interface(device):
    """torch's argument names, order and defaults, its param_groups keys, the class attributes training.py tests for, lr uploads."""
    import inspect
    from deformablelka_amd import optim
    lead = ["self", "params", "lr", "betas", "eps", "weight_decay", "amsgrad"]
    for ours, theirs in ((optim.Adam, torch.optim.Adam), (optim.AdamW, torch.optim.AdamW)):
        a, b = inspect.signature(ours.__init__).parameters, inspect.signature(theirs.__init__).parameters
        assert list(a)[:7] == lead == list(b)[:7]
        assert [a[k].default for k in lead[2:]] == [b[k].default for k in lead[2:]]
        assert all(a[k].kind == inspect.Parameter.KEYWORD_ONLY for k in list(a)[7:]) and "max_grad_norm" in a
        assert {"foreach", "maximize", "capturable", "differentiable", "fused"} <= set(a)
        assert ours.lr_on_device is True and ours.clips_in_step is True and issubclass(ours, torch.optim.Optimizer)
        q = [torch.zeros(1, requires_grad=True)]
        assert set(ours(q).param_groups[0]) == set(theirs(q).param_groups[0])
        assert ours(q).param_groups[0]["decoupled_weight_decay"] == theirs(q).param_groups[0]["decoupled_weight_decay"]
    p = [torch.ones(4, device=device, requires_grad=True), torch.ones(3, device=device, requires_grad=True)]
    opt = optim.Adam([dict(params=p[:1]), dict(params=p[1:], lr=0.5)], 0.25)
    opt.sync_lr()
    assert opt.lr_tensor.dtype == torch.float32 and opt.lr_tensor.cpu().tolist() == [0.25, 0.5]
    held = opt.lr_tensor
    opt.sync_lr()
    assert opt.lr_tensor is held
    opt.param_groups[1]["lr"] = 0.125
    for q in p:
        q.grad = torch.ones_like(q)
    opt.step()   # the first Adam step moves every element by lr (eps apart), whatever the gradient's size
    assert opt.lr_tensor.cpu().tolist() == [0.25, 0.125] and opt.last_grad_norm is None
    assert torch.allclose(p[0].detach().cpu(), torch.full((4,), 0.75), rtol=1e-6) and torch.allclose(p[1].detach().cpu(), torch.full((3,), 0.875), rtol=1e-6)
    assert set(opt.state[p[0]]) == {"step", "exp_avg", "exp_avg_sq"} and set(optim.Adam(p, amsgrad=True).state) == set()
    p[0].grad, p[1].grad = None, None
    opt.step(max_grad_norm=1.0)   # no gradients at all: nothing moves, no count advances, the norm is 0
    assert float(opt.last_grad_norm) == 0.0 and float(opt.state[p[0]]["step"]) == 1.0
    opt.add_param_group(dict(params=[torch.ones(2, device=device, requires_grad=True)]))   # the count tensor grows, the counts move with it
    assert float(opt.state[p[0]]["step"]) == 1.0 and opt._count_tensor().numel() == 3 and float(opt.state[p[1]]["step"]) == 1.0


def check_reduce_lr_on_plateau(device):
    """The 3-D base trainers' scheduler writes param_groups; the next step uploads what it wrote."""
    from deformablelka_amd import optim
    p = [torch.ones(5, device=device, requires_grad=True)]
    opt = optim.Adam(p, 3e-4, weight_decay=3e-5, amsgrad=True)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, factor=0.2, patience=0)
    p[0].grad = torch.ones_like(p[0])
    opt.step()
    sched.step(1.0)
    sched.step(2.0)   # no improvement: lr *= 0.2
    assert opt.param_groups[0]["lr"] == 3e-4 * 0.2
    before = p[0].detach().cpu().clone()
    opt.step()
    assert opt.lr_tensor.cpu().tolist() == [float(torch.tensor(3e-4 * 0.2, dtype=torch.float32))]
    moved = (before - p[0].detach().cpu()).abs().max()
    assert 0.5 * 6e-5 < float(moved) < 2 * 6e-5   # a step of about lr
    sd = sched.state_dict()
    torch.optim.lr_scheduler.ReduceLROnPlateau(opt, factor=0.2, patience=0).load_state_dict(sd)


# ---- the small net of the trainer tests ---------------------------------------------------------------------------------------------------------------
from tests.optim_cases import lite_net   # noqa: E402,F401
