"""The losses the reference's trainers step, on the fused HIP kernels of ``csrc/cl_seg_loss.hip`` (include/dlka.h: ``dlka_seg_loss_*``).

Names, constructor signatures and call conventions are the reference's, so that both trainers can take the classes unchanged:

  ``SoftDiceLoss``, ``DC_and_CE_loss``   3D/d_lka_former/training/loss_functions/dice_loss.py:158-194, :304-361 (nnU-Net)
  ``MultipleOutputLoss2``                3D/d_lka_former/training/loss_functions/deep_supervision.py:19-43
  ``DiceLoss``                           2D/utils.py:11-47
  ``online_eval_counts``                 the hard tp / fp / fn of Trainer_synapse.py:697-718 (run_online_evaluation)

One head costs one streaming read of the logits forward (plus a finishing launch over the per-workgroup partial sums) and one read plus one
write backward; nothing of the logits' size is kept between the two.  The fused path covers softmax as the nonlinearity, label-map targets
(float32 or int64, ``(B, 1, *)`` or ``(B, *)``), both ``batch_dice`` and ``do_bg`` values, any ``smooth`` and weights, K <= 32.  What it does
not cover raises ``NotImplementedError`` naming the argument — at construction where the argument is a constructor's.  There is no fall-back
to a torch composition."""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib as L
from . import ops


class _SegLossFunction(torch.autograd.Function):
    """loss, dc = f(logits); the backward recomputes the softmax from the saved logits and reads ``grad_output`` on the device."""

    @staticmethod
    def forward(ctx, logits, labels, kw):
        loss, dc, _stats, coef, d, x, y = ops.seg_loss_forward(logits.detach(), labels, **kw)
        ctx.save_for_backward(x, y, coef)
        ctx.desc = d
        ctx.mark_non_differentiable(dc)
        return loss, dc

    @staticmethod
    def backward(ctx, grad_loss, _grad_dc):
        x, y, coef = ctx.saved_tensors
        return ops.seg_loss_backward(x, y, ctx.desc, coef, grad_loss).view_as(x), None, None


def _check_target(logits, target):
    if target.ndim == logits.ndim and target.shape[1] != 1:
        raise NotImplementedError("target: one-hot targets are not covered by the fused loss; pass a label map (B, 1, *) or (B, *)")


def dc_and_ce(logits, target, batch_dice=False, do_bg=True, smooth=1.0, weight_ce=1.0, weight_dice=1.0):
    """(loss, dc): ``weight_ce * CE(logits, target) + weight_dice * (-mean(dc))`` with nnU-Net's soft Dice of softmax(logits, 1); dc is (B, K)
    (rows equal under ``batch_dice``; 0 for a dropped background), detached."""
    _check_target(logits, target)
    return _SegLossFunction.apply(logits, target, dict(mode=L.DLKA_SEG_LOSS_NNUNET, batch_dice=batch_dice, do_bg=do_bg, smooth=smooth,
                                                       weight_ce=weight_ce, weight_dice=weight_dice))


def _is_softmax(fn) -> bool:
    from . import inference
    return fn is inference.softmax_helper or getattr(fn, "__name__", None) == "softmax_helper"   # (the reference's own helper of that name too)


class SoftDiceLoss(nn.Module):
    """dc_k = (2 tp + smooth) / (2 tp + fp + fn + smooth + 1e-8) over the voxels of a sample (of the batch with ``batch_dice``), class 0 dropped
    unless ``do_bg``; returns -mean(dc).  ``apply_nonlin`` must be the softmax helper: the kernel fuses it."""

    def __init__(self, apply_nonlin=None, batch_dice=False, do_bg=True, smooth=1.):
        super().__init__()
        if not _is_softmax(apply_nonlin):
            raise NotImplementedError(f"apply_nonlin: the fused soft Dice applies softmax over the classes itself (pass softmax_helper), got {apply_nonlin!r}")
        self.do_bg = do_bg
        self.batch_dice = batch_dice
        self.apply_nonlin = apply_nonlin
        self.smooth = smooth

    def forward(self, x, y, loss_mask=None):
        if loss_mask is not None:
            raise NotImplementedError("loss_mask: masked Dice is not covered by the fused loss")
        return dc_and_ce(x, y, self.batch_dice, self.do_bg, self.smooth, weight_ce=0.0, weight_dice=1.0)[0]


class DC_and_CE_loss(nn.Module):
    """``weight_ce * CE + weight_dice * SoftDiceLoss(softmax, **soft_dice_kwargs)``; the CE term is the mean over all voxels.  One fused launch pair
    per call computes both terms."""

    def __init__(self, soft_dice_kwargs, ce_kwargs, aggregate="sum", square_dice=False, weight_ce=1, weight_dice=1, log_dice=False, ignore_label=None):
        super().__init__()
        if ignore_label is not None:
            raise NotImplementedError("ignore_label: not covered by the fused loss")
        if square_dice:
            raise NotImplementedError("square_dice: SoftDiceLossSquared is not covered by the fused loss")
        if log_dice:
            raise NotImplementedError("log_dice: not covered by the fused loss")
        if ce_kwargs:
            raise NotImplementedError(f"ce_kwargs: the fused cross-entropy is the plain mean over all voxels, got {ce_kwargs!r}")
        if aggregate != "sum":
            raise NotImplementedError("aggregate: only 'sum' (as in the reference)")
        from . import inference
        self.log_dice = log_dice
        self.weight_dice = weight_dice
        self.weight_ce = weight_ce
        self.aggregate = aggregate
        self.ignore_label = ignore_label
        self.dc = SoftDiceLoss(apply_nonlin=inference.softmax_helper, **soft_dice_kwargs)
        self.last_dc = None   # (B, K) Dice coefficients of the latest call, detached: for logging

    def forward(self, net_output, target):
        loss, self.last_dc = dc_and_ce(net_output, target, self.dc.batch_dice, self.dc.do_bg, self.dc.smooth, self.weight_ce, self.weight_dice)
        return loss


class MultipleOutputLoss2(nn.Module):
    """sum_i weight_factors[i] * loss(x[i], y[i]) over lists of outputs and targets; heads with a zero weight (except the first) are skipped."""

    def __init__(self, loss, weight_factors=None):
        super().__init__()
        self.weight_factors = weight_factors
        self.loss = loss

    def forward(self, x, y):
        assert isinstance(x, (tuple, list)), "x must be either tuple or list"
        assert isinstance(y, (tuple, list)), "y must be either tuple or list"
        weights = [1] * len(x) if self.weight_factors is None else self.weight_factors
        total = weights[0] * self.loss(x[0], y[0])
        for i in range(1, len(x)):
            if weights[i] != 0:
                total = total + weights[i] * self.loss(x[i], y[i])
        return total


class DiceLoss(nn.Module):
    """The 2-D trainer's Dice: per class over the whole batch 1 - (2 sum p t + 1e-5) / (sum p^2 + sum t + 1e-5), t the one-hot by equality,
    weighted by ``weight`` and divided by ``n_classes``.  No host synchronisation."""

    def __init__(self, n_classes):
        super().__init__()
        if n_classes > L.DLKA_SEG_LOSS_K_MAX:
            raise NotImplementedError(f"n_classes: at most {L.DLKA_SEG_LOSS_K_MAX}")
        self.n_classes = n_classes

    def forward(self, inputs, target, weight=None, softmax=False):
        if not softmax:
            raise NotImplementedError("softmax=False: the fused Dice takes logits and applies the softmax itself")
        _check_target(inputs, target)
        if inputs.shape[1] != self.n_classes:
            raise AssertionError(f"predict {tuple(inputs.shape)} & target {tuple(target.shape)} shape do not match (n_classes = {self.n_classes})")
        if weight is not None and len(weight) != self.n_classes:
            raise AssertionError(f"weight has {len(weight)} entries for {self.n_classes} classes")
        return _SegLossFunction.apply(inputs, target, dict(mode=L.DLKA_SEG_LOSS_DICE2D, class_weight=None if weight is None else list(weight)))[0]


def online_eval_counts(output, target):
    """(tp, fp, fn), each (K - 1,) int64 on the device: the hard counts of the foreground classes 1 .. K-1 summed over the batch, with
    argmax(softmax(output)) = the first maximum of the logits.  Which classes a trainer skips afterwards is its business."""
    _check_target(output, target)
    with torch.no_grad():
        return ops.seg_eval_counts(output.detach(), target)
