"""Plain-torch restatement of the trainers' losses, used only by tests and by scripts/time_seg_loss.py as "what a user would run today": the
reference's formulation as a composition of stock ops (softmax, scattered one-hot, tp / fp / fn, reductions, a second log-softmax + NLL for
the cross-entropy), differentiated by autograd.  tests/test_seg_loss_emu.py holds it to the fixture recorded from the reference's own classes
(tests/golden/reference_losses.pt)."""
import torch
import torch.nn.functional as F


def _label_map(logits, target):
    return (target[:, 0] if target.ndim == logits.ndim else target).long()


def soft_dice_coefficients(logits, target, batch_dice, smooth):
    """dc (K,) with batch_dice, else (B, K)."""
    p = torch.softmax(logits, 1)
    onehot = torch.zeros_like(p)
    onehot.scatter_(1, _label_map(logits, target)[:, None], 1)
    axes = ([0] if batch_dice else []) + list(range(2, logits.ndim))
    tp = (p * onehot).sum(axes)
    fp = (p * (1 - onehot)).sum(axes)
    fn = ((1 - p) * onehot).sum(axes)
    return (2 * tp + smooth) / (2 * tp + fp + fn + smooth + 1e-8)


def dc_and_ce(logits, target, batch_dice=False, do_bg=True, smooth=1.0, weight_ce=1, weight_dice=1):
    """(loss, dc)"""
    dc = soft_dice_coefficients(logits, target, batch_dice, smooth)
    kept = dc if do_bg else (dc[1:] if batch_dice else dc[:, 1:])
    ce = F.cross_entropy(logits, _label_map(logits, target))
    return weight_ce * ce + weight_dice * (-kept.mean()), dc


def multiple_output(outputs, targets, weights, **kw):
    total = weights[0] * dc_and_ce(outputs[0], targets[0], **kw)[0]
    for i in range(1, len(outputs)):
        if weights[i] != 0:
            total = total + weights[i] * dc_and_ce(outputs[i], targets[i], **kw)[0]
    return total


def dice2d(logits, target, weight=None):
    """(loss, per-class (2 I + s) / (Z + Y + s))"""
    K = logits.shape[1]
    p = torch.softmax(logits, 1)
    onehot = torch.stack([target == k for k in range(K)], 1).to(p.dtype)
    weight = [1] * K if weight is None else weight
    loss, coeffs = 0.0, []
    for k in range(K):
        inter, y_sum, z_sum = (p[:, k] * onehot[:, k]).sum(), (onehot[:, k] * onehot[:, k]).sum(), (p[:, k] * p[:, k]).sum()
        c = (2 * inter + 1e-5) / (z_sum + y_sum + 1e-5)
        coeffs.append(c)
        loss = loss + (1 - c) * weight[k]
    return loss / K, torch.stack(coeffs)


def eval_counts(logits, target):
    """(3, K - 1) int64: hard tp / fp / fn of the foreground classes over the batch."""
    K = logits.shape[1]
    seg = torch.softmax(logits.float(), 1).argmax(1)
    t = _label_map(logits, target)
    rows = [[((seg == c) & (t == c)).sum() for c in range(1, K)], [((seg == c) & (t != c)).sum() for c in range(1, K)],
            [((seg != c) & (t == c)).sum() for c in range(1, K)]]
    return torch.stack([torch.stack(r) for r in rows]).long()
