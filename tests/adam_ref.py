"""Float64 restatement of torch.optim.Adam / AdamW (amsgrad, clip folded in) from the formulas of include/dlka.h (dlka_optim_adam_step), and the
fp32 rounding bounds the Adam tests hold the kernels — and torch's own CPU float32 step — to.

The bounds count roundings of 2^-24 (EPS), each relative to one term, along the operation sequence:

  g_c         5 relative to G = |g coef| + wd |p| (the last only where the decay goes into the gradient): the float32 norm 1, + 1e-6 1, the quotient
              max_norm / . 1, g * coef 1, + wd p 1.  (The restatement's coef comes from the float64 norm.)
  exp_avg     m + (g_c - m)(1 - beta1):  (1 - beta1) (5 G + 1 (|g_c| + |m|) [the difference] + 2 |g_c - m| [the constant, the product]) + 1 |m_new|
              <= 10 (|m| + G) for every beta1.
  exp_avg_sq  beta2 v + (1 - beta2) g_c^2:  3 on beta2 v (the constant, the product, the sum), 14 on (1 - beta2) G^2 (twice g_c's 5, the square,
              the constant, the product, the sum).  max_exp_avg_sq = max(old, v): the same bound (max moves by no more than its argument).
  parameter   p (1 - lr wd) - (lr / bc1) m / (sqrt(w) / bc2 + eps):  4 on P = |p| (1 + lr wd) (1 - lr wd, its product with p, the final
              difference, one spare for lr wd itself), 10 on S = step_size |m_new| / denom (lr as float32, bc1 as float32, their quotient, the
              product with m, the quotient by denom, the root, bc2 as float32, the quotient by it, + eps, the final difference) — plus what the
              new exp_avg and exp_avg_sq carry in: step_size bound_m / denom, and S (bound_v / 2 w) (sqrt(w) / bc2) / denom (the root halves a
              relative error).  m_new can be small beside |m| + |g_c| (a cancellation), so its error is carried in absolutely, not as a
              count on S."""
import torch

EPS = 2.0 ** -24
N_M, N_V_OLD, N_V_G, N_P, N_S = 10, 3, 14, 4, 10


def adam_step(p, g, m, v, vmax, t, coef, lr, h):
    """One step in float64 from float32 or float64 state (m, v, vmax None: zeros); t: the count AFTER this step.  h: beta1, beta2, eps,
    weight_decay, decoupled, amsgrad.  Returns a dict: p, m, v, vmax (None without amsgrad) and the magnitudes the bounds need."""
    p, g = p.double(), g.double()
    m = torch.zeros_like(p) if m is None else m.double()
    v = torch.zeros_like(p) if v is None else v.double()
    vmax = torch.zeros_like(p) if vmax is None else vmax.double()
    b1, b2, wd = h["beta1"], h["beta2"], h["weight_decay"]
    gc = g * coef
    G = gc.abs()
    P = p.abs() * (1 + lr * wd)
    if h["decoupled"]:
        p = p * (1 - lr * wd)
    elif wd != 0:
        G = G + wd * p.abs()
        gc = gc + wd * p
    m_new = m + (gc - m) * (1 - b1)
    v_new = b2 * v + (1 - b2) * gc * gc
    w = v_new
    if h["amsgrad"]:
        vmax = torch.maximum(vmax, v_new)
        w = vmax
    bc1, bc2 = 1 - b1 ** t, (1 - b2 ** t) ** 0.5
    root = w.sqrt() / bc2
    denom = root + h["eps"]
    step_size = lr / bc1
    p_new = p - step_size * m_new / denom
    bound_m = N_M * EPS * (m.abs() + G)
    bound_v = EPS * (N_V_OLD * b2 * v + N_V_G * (1 - b2) * G * G)
    S = step_size * m_new.abs() / denom
    carried_v = torch.where(w > 0, S * (bound_v / (2 * w).clamp_min(1e-300)) * root / denom, torch.zeros_like(S))
    bound_p = EPS * (N_P * P + N_S * S) + step_size * bound_m / denom + carried_v
    return dict(p=p_new, m=m_new, v=v_new, vmax=vmax if h["amsgrad"] else None, bound_p=bound_p, bound_m=bound_m, bound_v=bound_v)
