"""The plain (non-deformable) 2-D large-kernel attention — ``LKA`` and ``LKA_Attention`` with the constructor / forward signatures and ``state_dict``
keys of 2D/deformable_LKA/LKA.py:4-37: the ablation partner of ``deformable_LKA_Attention``.

``LKA_Attention.forward`` runs the whole block as ONE C-ABI call per direction (``dlka_lka2d_plain_attention_forward/backward``, channels-last HIP
kernels) where the fused block covers the width (C / 32 in {1, 2, 3, 4, 6, 8, 12}) and the activation dtype (float32, or bfloat16 activations next to
float32 parameters).  Any other width, and ``LKA`` used on its own, runs operator by operator through the general HIP kernels (``nn_ops.conv2d``,
``nn_ops.gelu``), so every C works.  Which path each decoder shape takes, and why, is measured in profiles/lka2d_plain_notes.md."""
import torch
import torch.nn as nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import nn_ops, ops
from .ops import lka2d_plain


def _conv(x, c):
    return nn_ops.conv2d(x, c.weight, c.bias, c.stride, c.padding, c.dilation, c.groups)


class LKA(nn.Module):
    """LKA.py:4-18: depthwise 5x5, depthwise 7x7 dilation 3, 1x1, gate."""

    def __init__(self, dim):
        super().__init__()
        self.conv0 = nn.Conv2d(dim, dim, 5, padding=2, groups=dim)
        self.conv_spatial = nn.Conv2d(dim, dim, 7, stride=1, padding=9, groups=dim, dilation=3)
        self.conv1 = nn.Conv2d(dim, dim, 1)

    def forward(self, x):
        attn = _conv(x, self.conv0)
        attn = _conv(attn, self.conv_spatial)
        attn = _conv(attn, self.conv1)
        return x * attn


class _LKA2dPlainFn(Function):
    @staticmethod
    def forward(ctx, x, *params):
        y, saved = lka2d_plain.attention_forward(x, params)
        ctx.save_for_backward(x, saved, *params)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, saved, *params = ctx.saved_tensors
        gx, grads = lka2d_plain.attention_backward(x, params, gy, saved)
        return (gx, *grads)


class LKA_Attention(nn.Module):
    """LKA.py:21-37."""

    per_op = False   # True: every width takes the per-op path (A/B measurements; scripts/time_lka2d_plain.py)

    def __init__(self, d_model):
        super().__init__()
        self.proj_1 = nn.Conv2d(d_model, d_model, 1)
        self.activation = nn.GELU()
        self.spatial_gating_unit = LKA(d_model)
        self.proj_2 = nn.Conv2d(d_model, d_model, 1)

    def block_params(self):
        """The 10 tensors in ``dlka_lka2d_plain_params`` order (include/dlka.h)."""
        s = self.spatial_gating_unit
        return (self.proj_1.weight, self.proj_1.bias, s.conv0.weight, s.conv0.bias, s.conv_spatial.weight, s.conv_spatial.bias,
                s.conv1.weight, s.conv1.bias, self.proj_2.weight, self.proj_2.bias)

    def fused(self, x):
        """Whether ``forward(x)`` is the one-call block: a covered width (measured faster than the per-op path at every decoder shape,
        profiles/lka2d_plain_notes.md), float32 parameters, float32 or bfloat16 activations."""
        return (not self.per_op and x.ndim == 4 and lka2d_plain.supported(int(x.shape[1])) and x.dtype in lka2d_plain.ACTIVATION_DTYPES
                and self.proj_1.weight.dtype == torch.float32)

    def forward(self, x):
        # Autocast policy (the reference registers none), as deformable_LKA_Attention's: inside torch.autocast(dtype=torch.bfloat16) the block takes bf16
        # activations with fp32 parameters / accumulation where the fused block covers the width; elsewhere x keeps its dtype.
        act = ops.autocast_activation_dtype(x)
        if act != x.dtype and act == torch.bfloat16 and self.fused(x):
            x = x.to(act)
        if self.fused(x):
            return _LKA2dPlainFn.apply(x, *self.block_params())
        # per-op path: one dtype for activations and parameters (the general operators refuse a mixture; bf16 activations are the fused block's mode)
        if x.dtype != self.proj_1.weight.dtype:
            raise RuntimeError(f"LKA_Attention: {x.dtype} activations next to {self.proj_1.weight.dtype} parameters at C = {int(x.shape[1])}: the fused block "
                               "takes float32 or bfloat16 activations with float32 parameters at C / 32 in {1, 2, 3, 4, 6, 8, 12}; every other width "
                               "wants one dtype for both")
        y = nn_ops.gelu(_conv(x, self.proj_1))
        y = self.spatial_gating_unit(y)
        return _conv(y, self.proj_2) + x
