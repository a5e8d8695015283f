"""The fused Dice + cross-entropy losses (csrc/cl_seg_loss.hip, deformablelka_amd/losses.py) on the wavefront emulator against the fixture recorded
from the reference's own classes (tests/golden/reference_losses.pt, float64), under DESIGN.md §"Tolerances": loss and Dice coefficients 1e-4
absolute, gradients 1e-3 of max|grad| per head, bf16 logits 2e-2.  Reached on the emulator (fp32 logits): loss <= 4e-7, dc <= 5e-8, gradients
<= 5e-7 relative; bf16 logits: loss <= 3e-4, gradients <= 7e-3 relative (the rounding of the inputs and of the stored gradient)."""
import inspect

import pytest
import torch

from tests import seg_loss_cases as C
from tests import seg_loss_ref as R


@pytest.fixture(scope="module", autouse=True)
def emu_backend():
    from deformablelka_amd import _lib
    from tests import emu
    _lib._set_backend_for_tests(emu.load())
    yield
    _lib._set_backend_for_tests(None)


FX = C.load_fixture()
NAMES = list(FX["cases"].keys())


@pytest.mark.parametrize("label_dtype", [torch.float32, torch.int64], ids=["labels_f32", "labels_i64"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", NAMES)
def test_fixture_case(name, dtype, label_dtype):
    C.check_case(name, FX["cases"][name], "cpu", dtype, label_dtype)


@pytest.mark.parametrize("label_dtype", [torch.float32, torch.int64], ids=["labels_f32", "labels_i64"])
def test_vector_shape_at_unaligned_pointers(label_dtype):
    """A shape whose aligned twin takes the 16-byte kernels (K = 4, N % 4 == 0), logits and labels one element off 16-byte alignment: the scalar kernels."""
    C.check_unaligned_vector_shape("cpu", label_dtype)


@pytest.mark.parametrize("name", NAMES)
def test_online_eval_counts(name):
    C.check_counts(FX["cases"][name], "cpu")
    C.check_counts(FX["cases"][name], "cpu", torch.int64)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_is_held_to_the_fixture(name):
    """tests/seg_loss_ref.py in float64 against the reference's own classes: rounding only."""
    case = FX["cases"][name]
    xs = [x.double().requires_grad_(True) for x in case["logits"]]
    ys = case["labels"]
    if case["kind"] == "dice2d":
        loss, dc = R.dice2d(xs[0], ys[0], case["weight"])
        dcs = [dc]
    else:
        kw = dict(case["dice_kw"], weight_ce=case["weight_ce"], weight_dice=case["weight_dice"])
        loss = R.multiple_output(xs, ys, case["weights"], **kw) if case["weights"] is not None else R.dc_and_ce(xs[0], ys[0], **kw)[0]
        dcs = [R.soft_dice_coefficients(x.detach(), y, case["dice_kw"]["batch_dice"], case["dice_kw"]["smooth"]) for x, y in zip(xs, ys)]
    loss.backward()
    assert abs(float(loss.detach()) - float(case["loss"])) < 1e-12
    for x, y, g, dc, dcr, cnt in zip(xs, ys, case["grads"], dcs, case["dc"], case["counts"]):
        got = x.grad if x.grad is not None else torch.zeros_like(x)
        assert (got - g.double()).abs().max() <= 1e-7 * max(float(g.abs().max()), 1e-30)   # (the fixture stores float32 gradients)
        assert (dc - dcr).abs().max() < 1e-12
        assert torch.equal(R.eval_counts(x.detach().float(), y), cnt)


def test_two_runs_are_bitwise_equal(monkeypatch):
    monkeypatch.setenv("HIPEMU_THREADS", "1")
    case = FX["cases"]["trainer_three_heads"]
    a, b = C.run_fused(case, "cpu"), C.run_fused(case, "cpu")
    assert torch.equal(a[0], b[0])
    for ga, gb, da, db in zip(a[1], b[1], a[2], b[2]):
        assert torch.equal(ga, gb) and torch.equal(da, db)


BAD_LABELS = [(torch.float32, -1.0), (torch.float32, 14.0), (torch.float32, 2.5), (torch.float32, float("nan")), (torch.float32, 1e30),
              (torch.int64, -1), (torch.int64, 14), (torch.int64, 2 ** 40)]


@pytest.mark.parametrize("label_dtype,bad", BAD_LABELS, ids=[f"{'f32' if d == torch.float32 else 'i64'}_{b}" for d, b in BAD_LABELS])
def test_invalid_labels_never_index_and_give_nan(label_dtype, bad):
    """Emulator only: nothing feeds bad labels to a GPU.  nnU-Net's loss (the reference's scatter_ would raise) comes out NaN; the statistics count
    the voxel as belonging to no class."""
    from deformablelka_amd import losses, ops
    torch.manual_seed(0)
    x = torch.randn(2, 14, 2, 4, 4, requires_grad=True)
    y = torch.randint(0, 14, (2, 1, 2, 4, 4)).to(label_dtype)
    y[1, 0, 1, 2, 3] = bad
    loss = losses.DC_and_CE_loss({"batch_dice": True, "smooth": 1e-5, "do_bg": False}, {})(x, y)
    assert torch.isnan(loss)
    loss.backward()
    assert torch.isnan(x.grad).all()
    stats = ops.seg_loss_forward(x.detach(), y)[2]
    assert float(stats[:, -1].sum()) == 1.0 and float(stats[:, 3 * 14:4 * 14].sum()) == 2 * 32 - 1


def test_invalid_labels_in_the_2d_dice_belong_to_no_class():
    """2D/utils.py builds the one-hot by equality: a label outside the classes matches none — same value as the restatement."""
    from deformablelka_amd import losses
    torch.manual_seed(1)
    x = torch.randn(2, 9, 6, 10)
    y = torch.randint(0, 9, (2, 6, 10)).float()
    y[0, 0, 0], y[1, 2, 3], y[1, 5, 9] = -3.0, 9.0, 4.5
    xf = x.clone().requires_grad_(True)
    loss = losses.DiceLoss(9)(xf, y, softmax=True)
    loss.backward()
    xr = x.double().requires_grad_(True)
    ref = R.dice2d(xr, y)[0]
    ref.backward()
    assert abs(float(loss) - float(ref)) <= 1e-4
    assert (xf.grad.double() - xr.grad).abs().max() <= 1e-3 * xr.grad.abs().max()


def test_not_implemented_arguments_are_named():
    from deformablelka_amd import inference, losses
    dice_kw = {"batch_dice": True, "smooth": 1e-5, "do_bg": False}
    for kw, word in ((dict(ignore_label=0), "ignore_label"), (dict(square_dice=True), "square_dice"), (dict(log_dice=True), "log_dice")):
        with pytest.raises(NotImplementedError, match=word):
            losses.DC_and_CE_loss(dice_kw, {}, **kw)
    with pytest.raises(NotImplementedError, match="ce_kwargs"):
        losses.DC_and_CE_loss(dice_kw, {"reduction": "none"})
    with pytest.raises(NotImplementedError, match="apply_nonlin"):
        losses.SoftDiceLoss()
    with pytest.raises(NotImplementedError, match="apply_nonlin"):
        losses.SoftDiceLoss(apply_nonlin=torch.sigmoid)
    x, y = torch.randn(1, 4, 2, 4, 4), torch.zeros(1, 1, 2, 4, 4)
    with pytest.raises(NotImplementedError, match="loss_mask"):
        losses.SoftDiceLoss(apply_nonlin=inference.softmax_helper)(x, y, loss_mask=torch.ones_like(y))
    with pytest.raises(NotImplementedError, match="one-hot"):
        losses.DC_and_CE_loss(dice_kw, {})(x, torch.zeros_like(x))
    with pytest.raises(NotImplementedError, match="softmax=False"):
        losses.DiceLoss(4)(x[:, :, 0], y[:, 0, 0])
    with pytest.raises(NotImplementedError, match="K = 33"):
        losses.DC_and_CE_loss(dice_kw, {})(torch.randn(1, 33, 2, 2, 2), torch.zeros(1, 1, 2, 2, 2))


def test_soft_dice_alone_and_k32():
    """SoftDiceLoss on its own (no CE term), and the widest class bucket (K = 32, scalar loads)."""
    from deformablelka_amd import inference, losses
    torch.manual_seed(2)
    for K, kw in ((14, dict(batch_dice=False, do_bg=True, smooth=1.0)), (32, dict(batch_dice=True, do_bg=False, smooth=1e-5)), (7, dict(batch_dice=True, do_bg=True, smooth=0.5))):
        x = torch.randn(2, K, 3, 4, 4)
        y = torch.randint(0, K, (2, 1, 3, 4, 4)).float()
        xf, xr = x.clone().requires_grad_(True), x.double().requires_grad_(True)
        loss = losses.SoftDiceLoss(apply_nonlin=inference.softmax_helper, **kw)(xf, y)
        ref = R.dc_and_ce(xr, y, weight_ce=0, **kw)[0]
        loss.backward(); ref.backward()
        assert abs(float(loss) - float(ref)) <= 1e-4
        assert (xf.grad.double() - xr.grad).abs().max() <= 1e-3 * xr.grad.abs().max()


def test_backward_agrees_with_a_finite_difference_of_the_forward():
    """No fp64 kernel is built: central differences of the fp32 forward, element by element, at B = 1, K = 4, N = 8.  Bound per element: the gradient
    contract (1e-3 max|grad|) plus the rounding of the two forwards, 4 eps |loss| / (2 h) with eps = 2^-24 (each forward is a handful of fp32
    roundings of a value of size |loss|), plus the truncation h^2 / 6 * |f'''| <= h^2 (the third derivatives of softmax terms scaled by 1 / N are below 1)."""
    from deformablelka_amd import losses
    torch.manual_seed(3)
    fn = losses.DC_and_CE_loss({"batch_dice": True, "smooth": 1e-5, "do_bg": False}, {})
    x = torch.randn(1, 4, 2, 2, 2)
    y = torch.randint(0, 4, (1, 1, 2, 2, 2)).float()
    xg = x.clone().requires_grad_(True)
    loss = fn(xg, y)
    loss.backward()
    g = xg.grad.flatten()
    h = 1e-2
    fd = torch.zeros_like(g, dtype=torch.float64)
    for i in range(g.numel()):
        xp, xm = x.clone().flatten(), x.clone().flatten()
        xp[i] += h; xm[i] -= h
        fd[i] = (float(fn(xp.view_as(x), y)) - float(fn(xm.view_as(x), y))) / (float(xp[i]) - float(xm[i]))
    bound = 1e-3 * float(g.abs().max()) + 4 * 2.0 ** -24 * abs(float(loss)) / (2 * h) + h * h
    err = float((fd - g.double()).abs().max())
    print(f"finite difference: max err {err:.3e}, bound {bound:.3e}, max|grad| {float(g.abs().max()):.3e}")
    assert err <= bound


def test_signatures_and_state_dict_match_the_reference():
    from deformablelka_amd import inference, losses
    for name, sig in FX["signatures"].items():
        cls = getattr(losses, name)
        assert str(inspect.signature(cls.__init__)) == sig["__init__"], name
        assert str(inspect.signature(cls.forward)) == sig["forward"], name
    # no parameters or buffers on either side
    base = losses.DC_and_CE_loss({"batch_dice": True, "smooth": 1e-5, "do_bg": False}, {})
    for m in (base, losses.MultipleOutputLoss2(base, [1, 0.5]), losses.DiceLoss(9), losses.SoftDiceLoss(apply_nonlin=inference.softmax_helper)):
        assert list(m.state_dict().keys()) == []


def test_initialize_loss_is_the_trainers_configuration():
    from deformablelka_amd import losses, training
    fn = training.initialize_loss()
    assert isinstance(fn, losses.MultipleOutputLoss2) and isinstance(fn.loss, losses.DC_and_CE_loss)
    assert fn.weight_factors == [1 / 1.75, 0.5 / 1.75, 0.25 / 1.75]
    assert (fn.loss.dc.batch_dice, fn.loss.dc.do_bg, fn.loss.dc.smooth, fn.loss.weight_ce, fn.loss.weight_dice) == (True, False, 1e-5, 1, 1)
    assert isinstance(training.initialize_loss(deep_supervision=False), losses.DC_and_CE_loss)
    case = FX["cases"]["trainer_three_heads"]
    got = fn([x.clone() for x in case["logits"]], list(case["labels"]))
    assert abs(float(got) - float(case["loss"])) <= 1e-4
    # one full-resolution label volume is down-sampled to the heads (nearest neighbour), as deep_supervision_loss does
    full = case["labels"][0]
    ys = [full] + [torch.nn.functional.interpolate(full, size=x.shape[2:], mode="nearest") for x in case["logits"][1:]]
    assert torch.equal(fn(list(case["logits"]), full[:, 0].long()), fn(list(case["logits"]), ys))
