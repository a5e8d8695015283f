"""TEST INFRASTRUCTURE — the UNETR++ efficient paired attention restated in plain float64 torch, the dropout multipliers M1 / M2 as arguments.
Checked against the reference's own output (tests/golden/reference_epa.pt) in tests/test_epa_emu.py, and the oracle for everything the fixture
does not reach.  Never used by the product."""
import torch


def attention(qkvv, kp, vp, temperature, temperature2, heads, m1=None, m2=None):
    """qkvv [B, N, 4 C], kp / vp [B, C, P], temperatures [heads, 1, 1]; m1 [B, heads, D, D] and m2 [B, heads, N, P] multipliers.
    -> (x_sa, x_ca), both [B, N, C]; x_sa in the reference's permute(0, 3, 1, 2).reshape(B, N, C) order."""
    B, N, C4 = qkvv.shape
    C = C4 // 4
    D = C // heads
    s = qkvv.reshape(B, N, 4, heads, D)
    q, k, vc = (s[:, :, i].permute(0, 2, 1, 3) for i in range(3))            # [B, heads, N, D]
    nq = torch.linalg.vector_norm(q, dim=2, keepdim=True).clamp_min(1e-12)      # column norms over the tokens (a zero column: no gradient through the norm)
    nk = torch.linalg.vector_norm(k, dim=2, keepdim=True).clamp_min(1e-12)
    qh, kh = q / nq, k / nk
    a = ((qh.transpose(-2, -1) @ kh) * temperature).softmax(-1)                # [B, heads, D, D]
    if m1 is not None:
        a = a * m1.reshape(a.shape).to(a.dtype)
    x_ca = (vc @ a.transpose(-2, -1)).permute(0, 2, 1, 3).reshape(B, N, C)    # x_ca[n, h D + i] = sum_j a[i, j] vc[n, j]
    kph, vph = kp.reshape(B, heads, D, -1), vp.reshape(B, heads, D, -1)
    sm = ((qh @ kph) * temperature2).softmax(-1)                               # [B, heads, N, P]
    if m2 is not None:
        sm = sm * m2.reshape(sm.shape).to(sm.dtype)
    y = sm @ vph.transpose(-2, -1)                                              # [B, heads, N, D]
    x_sa = y.permute(0, 3, 1, 2).reshape(B, N, C)
    return x_sa, x_ca


def epa(x, P, heads, m1=None, m2=None):
    """EPA.forward on x [B, N, C] with the module's state_dict-keyed parameters P (E and F by their own keys)."""
    C = x.shape[2]
    qkvv = x @ P["qkvv.weight"].t()
    if "qkvv.bias" in P:
        qkvv = qkvv + P["qkvv.bias"]
    kp = qkvv[:, :, C:2 * C].transpose(1, 2) @ P["E.weight"].t() + P["E.bias"]
    vp = qkvv[:, :, 3 * C:].transpose(1, 2) @ P["F.weight"].t() + P["F.bias"]
    x_sa, x_ca = attention(qkvv, kp, vp, P["temperature"], P["temperature2"], heads, m1, m2)
    return torch.cat((x_sa @ P["out_proj.weight"].t() + P["out_proj.bias"], x_ca @ P["out_proj2.weight"].t() + P["out_proj2.bias"]), -1)

