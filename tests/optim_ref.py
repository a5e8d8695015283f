"""Float64 restatement of clip_grad_norm_ + torch.optim.SGD (dampening 0) from the formulas of include/dlka.h (dlka_optim_*), and the fp32
rounding bounds the optimizer tests hold the kernels — and torch's own CPU float32 step — to."""
import torch

EPS = 2.0 ** -24


def grad_norm(grads):
    return torch.sqrt(sum((g.double() ** 2).sum() for g in grads)) if grads else torch.zeros((), dtype=torch.float64)


def clip_coef(norm64, max_norm):
    """min(1, max_norm / (norm + 1e-6)); 1 without clipping"""
    if max_norm is None:
        return torch.ones((), dtype=torch.float64)
    return torch.clamp(max_norm / (norm64 + 1e-6), max=1.0)


def sgd_step(p, g, buf, coef, lr, momentum, weight_decay, nesterov):
    """(p_new, buf_new, g_c) in float64 from float32 or float64 state; buf None: zeros."""
    p, g = p.double(), g.double()
    buf = torch.zeros_like(p) if buf is None else buf.double()
    gc = g * coef
    d = gc + weight_decay * p
    if momentum != 0:
        buf_new = momentum * buf + d
        u = d + momentum * buf_new if nesterov else buf_new
    else:
        buf_new, u = buf, d
    return p - lr * u, buf_new, gc


def bounds(p_old, gc, buf_old, lr, momentum, weight_decay):
    """(buffer bound, parameter bound) per element: a handful of fp32 roundings, each relative to one term of the sums."""
    p_old, gc = p_old.double().abs(), gc.abs()
    buf_old = torch.zeros_like(p_old) if buf_old is None else buf_old.double().abs()
    b = 8 * EPS * (momentum * buf_old + gc + weight_decay * p_old)
    p = 16 * EPS * (p_old + lr * (1 + momentum) * (gc + weight_decay * p_old + momentum * buf_old))
    return b, p
