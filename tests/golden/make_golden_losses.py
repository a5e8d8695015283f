"""Generates tests/golden/reference_losses.pt from the REFERENCE'S OWN loss classes on the CPU, evaluated in float64 on float32-representable
inputs:

  3D/d_lka_former/training/loss_functions/dice_loss.py        SoftDiceLoss, DC_and_CE_loss, get_tp_fp_fn_tn
  3D/d_lka_former/training/loss_functions/deep_supervision.py MultipleOutputLoss2
  2D/utils.py                                                 DiceLoss

Per case: the inputs (float32 logits, float32 label maps (B, 1, *) as both loaders deliver them; the 2-D labels (B, H, W)), the loss, every head's
gradient (rounded to float32), the per-class Dice coefficients from the reference's get_tp_fp_fn_tn, and the online-evaluation counts by the
expressions of Trainer_synapse.py:697-718 (all K - 1 foreground classes, summed over the batch).  Also the ``inspect.signature`` strings of the
four classes.  Packages the 2-D utils module imports but never uses for the loss (medpy, SimpleITK, scipy, torchvision) are stubbed when absent.
Run: python tests/golden/make_golden_losses.py"""
import importlib
import inspect
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"


def _stub(name, **attrs):
    try:
        importlib.import_module(name)
        return
    except Exception:
        pass
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    if "." in name:
        parent, leaf = name.rsplit(".", 1)
        setattr(sys.modules[parent], leaf, m)


def load_reference():
    sys.path.insert(0, os.path.join(REF, "3D"))
    from d_lka_former.training.loss_functions import deep_supervision, dice_loss
    _stub("medpy", metric=None)
    _stub("SimpleITK")
    _stub("scipy")
    _stub("scipy.ndimage", zoom=None)
    _stub("torchvision", transforms=None)
    spec = importlib.util.spec_from_file_location("ref2d_utils", os.path.join(REF, "2D", "utils.py"))
    utils2d = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(utils2d)
    return dice_loss, deep_supervision, utils2d


def make_inputs(gen, B, K, spatial, absent=(), label_rank_full=True):
    x = torch.randn((B, K) + tuple(spatial), generator=gen, dtype=torch.float32) * 2.0
    present = [k for k in range(K) if k not in absent]
    y = torch.tensor(present)[torch.randint(0, len(present), (B, 1) + tuple(spatial), generator=gen)].float()
    # every present class really occurs (the first voxels of sample 0 run through them)
    flat = y[0, 0].reshape(-1)
    flat[:len(present)] = torch.tensor(present, dtype=torch.float32)[:flat.numel()]
    for k in absent:
        x[:, k] = -30.0 + 0.25 * x[:, k]   # p_k ~ 1e-13: the smooth and the 1e-8 terms decide dc_k
    return x, (y if label_rank_full else y[:, 0])


def eval_counts(x, y):
    # Trainer_synapse.py:697-718 for every foreground class
    K = x.shape[1]
    seg = torch.softmax(x, 1).argmax(1)
    t = y[:, 0] if y.ndim == x.ndim else y
    axes = tuple(range(1, t.ndim))
    tp = torch.stack([((seg == c).float() * (t == c).float()).sum(axes) for c in range(1, K)], 1).sum(0)
    fp = torch.stack([((seg == c).float() * (t != c).float()).sum(axes) for c in range(1, K)], 1).sum(0)
    fn = torch.stack([((seg != c).float() * (t == c).float()).sum(axes) for c in range(1, K)], 1).sum(0)
    return torch.stack([tp, fp, fn]).long()


def main():
    dice_loss, deep_supervision, utils2d = load_reference()
    gen = torch.Generator().manual_seed(20240607)
    softmax_helper = lambda t: torch.softmax(t, 1)   # noqa: E731  (what dice_loss.softmax_helper is)
    cases = {}

    def nnunet_case(name, B, K, shapes, dice_kw, weights=None, absent=(), weight_ce=1, weight_dice=1):
        xs, ys = zip(*[make_inputs(gen, B, K, s, absent) for s in shapes])
        xd = [x.double().requires_grad_(True) for x in xs]
        base = dice_loss.DC_and_CE_loss(dict(dice_kw), {}, weight_ce=weight_ce, weight_dice=weight_dice)
        loss = deep_supervision.MultipleOutputLoss2(base, weights)(xd, list(ys)) if weights is not None else base(xd[0], ys[0])
        loss.backward()
        dcs = []
        for x, y in zip(xd, ys):
            axes = ([0] if dice_kw["batch_dice"] else []) + list(range(2, x.ndim))
            tp, fp, fn, _ = dice_loss.get_tp_fp_fn_tn(softmax_helper(x.detach()), y, axes, None, False)
            dcs.append((2 * tp + dice_kw["smooth"]) / (2 * tp + fp + fn + dice_kw["smooth"] + 1e-8))
        cases[name] = dict(kind="nnunet", logits=list(xs), labels=list(ys), dice_kw=dict(dice_kw), weights=weights, weight_ce=weight_ce,
                           weight_dice=weight_dice, loss=loss.detach(), head_losses=[base(x.detach(), y) for x, y in zip(xd, ys)],
                           grads=[(x.grad if x.grad is not None else torch.zeros_like(x)).float() for x in xd], dc=dcs, counts=[eval_counts(x, y) for x, y in zip(xs, ys)])

    trainer = {"batch_dice": True, "smooth": 1e-5, "do_bg": False}
    w = [1.0, 0.5, 0.25]
    nnunet_case("trainer_three_heads", 2, 14, [(8, 16, 16), (4, 8, 8), (2, 4, 4)], trainer, [v / sum(w) for v in w])
    nnunet_case("sample_dice", 2, 14, [(2, 8, 8)], {"batch_dice": False, "smooth": 1e-5, "do_bg": False})
    nnunet_case("with_background", 2, 14, [(2, 8, 8)], {"batch_dice": True, "smooth": 1.0, "do_bg": True})
    nnunet_case("acdc_k4", 2, 4, [(2, 8, 8)], trainer)
    nnunet_case("odd_n", 3, 5, [(3, 5, 7)], {"batch_dice": False, "smooth": 1e-5, "do_bg": True})
    nnunet_case("absent_classes", 2, 14, [(2, 8, 8)], trainer, absent=(3, 7, 11))
    nnunet_case("absent_classes_sample_dice", 2, 14, [(2, 8, 8)], {"batch_dice": False, "smooth": 1e-5, "do_bg": False}, absent=(3, 7, 11))
    nnunet_case("weights_skip_head", 2, 4, [(2, 8, 8), (1, 4, 4), (1, 2, 2)], trainer, [0.75, 0.0, 0.25], weight_ce=0.5, weight_dice=2)

    for name, weight in (("dice2d", None), ("dice2d_weight", [0.5, 1.0, 2.0, 0.25, 1.5, 1.0, 0.0, 3.0, 0.75])):
        x, y = make_inputs(gen, 3, 9, (12, 20), label_rank_full=False)
        xd = x.double().requires_grad_(True)
        loss = utils2d.DiceLoss(9)(xd, y, weight=weight, softmax=True)
        loss.backward()
        p, oh = torch.softmax(xd.detach(), 1), torch.stack([(y == k) for k in range(9)], 1).double()
        dc = (2 * (p * oh).sum((0, 2, 3)) + 1e-5) / ((p * p).sum((0, 2, 3)) + oh.sum((0, 2, 3)) + 1e-5)
        cases[name] = dict(kind="dice2d", logits=[x], labels=[y], weight=weight, loss=loss.detach(), grads=[xd.grad.float()], dc=[dc],
                           counts=[eval_counts(x, y)])

    signatures = {}
    for cls in (dice_loss.SoftDiceLoss, dice_loss.DC_and_CE_loss, deep_supervision.MultipleOutputLoss2, utils2d.DiceLoss):
        signatures[cls.__name__] = {"__init__": str(inspect.signature(cls.__init__)), "forward": str(inspect.signature(cls.forward))}
    out = os.path.join(HERE, "reference_losses.pt")
    torch.save({"cases": cases, "signatures": signatures}, out)
    print(out, os.path.getsize(out), "bytes")
    for k, v in cases.items():
        print(k, float(v["loss"]))
    print(signatures)


if __name__ == "__main__":
    main()
