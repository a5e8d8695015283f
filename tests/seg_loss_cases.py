"""Shared by tests/test_seg_loss_emu.py and tests/test_seg_loss_gpu.py: the fixture cases of tests/golden/reference_losses.pt run through
``deformablelka_amd.losses`` on a device, under the tolerances of DESIGN.md §"Tolerances": loss and Dice coefficients 1e-4 absolute, gradients
1e-3 of max|grad| per head, bf16 logits 2e-2.  Every element of every gradient is compared; every measured figure is printed before it is asserted."""
import os

import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_losses.pt")
TOL = {torch.float32: (1e-4, 1e-3), torch.bfloat16: (2e-2, 2e-2)}   # (loss / dc absolute, gradient relative to max|grad| of the head)


def load_fixture():
    return torch.load(FIXTURE, weights_only=False)


def case_names():
    return list(load_fixture()["cases"].keys())


def build_loss(case):
    from deformablelka_amd import losses
    if case["kind"] == "dice2d":
        fn = losses.DiceLoss(case["logits"][0].shape[1])
        return lambda xs, ys: fn(xs[0], ys[0], weight=case["weight"], softmax=True), None
    base = losses.DC_and_CE_loss(dict(case["dice_kw"]), {}, weight_ce=case["weight_ce"], weight_dice=case["weight_dice"])
    if case["weights"] is None:
        return lambda xs, ys: base(xs[0], ys[0]), base
    multi = losses.MultipleOutputLoss2(base, case["weights"])
    return lambda xs, ys: multi(list(xs), list(ys)), base


def run_fused(case, device, dtype=torch.float32, label_dtype=torch.float32):
    """(loss, grads, dcs of every head)"""
    from deformablelka_amd import losses
    xs = [x.detach().to(device=device, dtype=dtype).clone().requires_grad_(True) for x in case["logits"]]
    ys = [y.to(device=device, dtype=label_dtype) for y in case["labels"]]
    fn, _ = build_loss(case)
    loss = fn(xs, ys)
    loss.backward()
    grads = [x.grad if x.grad is not None else torch.zeros_like(x) for x in xs]
    dcs = []
    for x, y in zip(xs, ys):   # the coefficients of every head on its own
        if case["kind"] == "dice2d":
            from deformablelka_amd import _lib as L, ops
            dcs.append(ops.seg_loss_forward(x.detach(), y, mode=L.DLKA_SEG_LOSS_DICE2D)[1][0])
        else:
            kw = case["dice_kw"]
            dc = losses.dc_and_ce(x.detach(), y, kw["batch_dice"], kw["do_bg"], kw["smooth"])[1]
            dcs.append(dc[0] if kw["batch_dice"] else dc)
    return loss.detach(), grads, dcs


def check_case(name, case, device, dtype=torch.float32, label_dtype=torch.float32):
    tol_abs, tol_grad = TOL[dtype]
    loss, grads, dcs = run_fused(case, device, dtype, label_dtype)
    e_loss = abs(float(loss) - float(case["loss"]))
    print(f"{name} [{dtype}, labels {label_dtype}]: loss {float(loss):.8f} ref {float(case['loss']):.8f} err {e_loss:.3e}")
    errs = []
    for h, (g, gr) in enumerate(zip(grads, case["grads"])):
        assert g.dtype == dtype and g.shape == gr.shape
        scale = float(gr.abs().max())
        e = float((g.detach().cpu().double() - gr.double()).abs().max())
        errs.append((e, scale))
        print(f"  head {h}: grad max abs err {e:.3e}, max|grad| {scale:.3e}, relative {e / scale if scale else 0.0:.3e}")
    dc_errs = []
    for h, (dc, dcr) in enumerate(zip(dcs, case["dc"])):
        k0 = 0 if case["kind"] == "dice2d" or case["dice_kw"]["do_bg"] else 1
        d = dc.detach().cpu().double()
        assert d.shape == dcr.shape
        e = float((d[..., k0:] - dcr[..., k0:]).abs().max())
        dc_errs.append(e)
        print(f"  head {h}: dc max abs err {e:.3e}")
        assert float(d[..., :k0].abs().sum()) == 0.0   # a dropped background reports 0
    assert e_loss <= tol_abs
    for e, scale in errs:
        assert e <= tol_grad * scale if scale else e == 0.0
    for e in dc_errs:
        assert e <= tol_abs
    return e_loss, max((e / s if s else 0.0) for e, s in errs), max(dc_errs)


def check_counts(case, device, label_dtype=torch.float32):
    from deformablelka_amd import losses
    for x, y, ref in zip(case["logits"], case["labels"], case["counts"]):
        tp, fp, fn = losses.online_eval_counts(x.to(device), y.to(device=device, dtype=label_dtype))
        got = torch.stack([tp, fp, fn]).cpu()
        assert got.dtype == torch.int64
        assert torch.equal(got, ref), (got, ref)


def check_unaligned_vector_shape(device, label_dtype=torch.float32):
    """K = 4, N = 3 * 4 * 4 = 48 (a multiple of 4): aligned, the launchers' seg_vec takes the 16-byte kernels; with logits and labels that start one element into
    their allocation (tests/parity.py offset_view: contiguous, data pointer not 16-byte aligned) the same shape has to take the scalar ones.  Both runs against
    tests/seg_loss_ref.py in float64 under the tolerances above, forward, Dice coefficients, online-evaluation counts and every element of the gradient."""
    from deformablelka_amd import losses
    from tests import seg_loss_ref as R
    from tests.parity import offset_view
    tol_abs, tol_grad = TOL[torch.float32]
    gen = torch.Generator().manual_seed(4)
    B, K, spatial = 2, 4, (3, 4, 4)
    x = torch.randn((B, K) + spatial, generator=gen) * 2.0
    y = torch.randint(0, K, (B, 1) + spatial, generator=gen)
    kw = {"batch_dice": True, "smooth": 1e-5, "do_bg": False}
    xr = x.double().requires_grad_(True)
    ref, dcr = R.dc_and_ce(xr, y, **kw)
    ref.backward()
    for aligned in (True, False):
        xd, yd = x.clone().to(device), y.to(device=device, dtype=label_dtype)
        if not aligned:
            xd, yd = offset_view(xd), offset_view(yd)
        xd.requires_grad_(True)
        loss = losses.DC_and_CE_loss(dict(kw), {})(xd, yd)
        loss.backward()
        dc = losses.dc_and_ce(xd.detach(), yd, **kw)[1][0]
        e_loss = abs(float(loss) - float(ref))
        e_grad = float((xd.grad.cpu().double() - xr.grad).abs().max() / xr.grad.abs().max())
        e_dc = float((dc.cpu().double()[1:] - dcr.detach()[1:]).abs().max())
        print(f"K=4 N=48 {'aligned' if aligned else 'offset by one element'}: loss err {e_loss:.3e}, grad rel {e_grad:.3e}, dc err {e_dc:.3e}")
        assert e_loss <= tol_abs and e_grad <= tol_grad and e_dc <= tol_abs
        tp, fp, fn = losses.online_eval_counts(xd.detach(), yd)
        assert torch.equal(torch.stack([tp, fp, fn]).cpu(), R.eval_counts(x, y))
