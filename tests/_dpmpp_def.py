"""TEST INFRASTRUCTURE ONLY -- the definition the DPM-Solver++(2M) tests measure against, in plain torch on the CPU: the logSNR
time-step rule, the float64 coefficient table, the fp32 per-step update with one rounding per written operation, and the analytic
model of the convergence test.  Written from the definition alone; it shares no code with the package.

    ab = cumprod(1 - betas);  lam[t] = 0.5 * log(ab[t + shift] / (1 - ab[t + shift])),  t = 0 .. hi = T - 1 - shift
    g_k = lam[0] + (lam[hi] - lam[0]) * k / (S - 1);  idx_k = the lowest t nearest to g_k;  forward pass, cap, backward pass

    a = ab[tau_k + shift];  a' = ab[tau_(k-1) + shift] (k > 0), a' = final_alpha_bar (k = 0);  h = lam(a') - lam(a)
    row k = (s1m = sqrt(1 - a), sa = sqrt(a), A = sqrt(1 - a') / sqrt(1 - a), B, C),  g = -sqrt(a') * expm1(-h)
    k = S-1 or k = 0:  B = g, C = 0;   a' = 1:  A = 0, B = 1, C = 0;   else r = h_(k+1) / h,  B = g * (1 + 1 / (2r)),  C = -g / (2r)

    eps = w1 * eps_c - wf * eps_u                         w1 = (float)(1 + w), wf = (float)w
    x0  = (x - eps * s1m) / sa ;  if clip_x0: x0 = clamp(x0, -1, 1)
    v   = A * x + B * x0 ;  if C != 0: v = v + C * x0_prev ;  x0_prev = x0 ;  x = v
"""
import math

import numpy as np
import torch

S1M, SA, A_, B_, C_ = range(5)


def alphas_bar(betas):
    return torch.cumprod(1.0 - torch.as_tensor(betas).detach().cpu().double(), dim=0)


def lam_of(v):
    return 0.5 * torch.log(v / (1.0 - v))


def logsnr_steps(betas, S, shift=0):
    ab = alphas_bar(betas)
    hi = ab.numel() - 1 - shift
    if S == 1:
        return [hi]
    lam = [float(lam_of(ab[t + shift])) for t in range(hi + 1)]
    idx = []
    for k in range(S):
        g = lam[0] + (lam[hi] - lam[0]) * k / (S - 1)
        best = 0
        for t in range(1, hi + 1):
            if abs(lam[t] - g) < abs(lam[best] - g):          # strict: the lowest t on a tie
                best = t
        idx.append(best)
    for k in range(1, S):
        idx[k] = max(idx[k], idx[k - 1] + 1)
    idx[-1] = min(idx[-1], hi)
    for k in range(S - 2, -1, -1):
        idx[k] = min(idx[k], idx[k + 1] - 1)
    return idx


def table(betas, tau, shift=0, final_alpha_bar=1.0):
    """float64 [S, 5]."""
    ab = alphas_bar(betas)
    S = len(tau)
    rows = [None] * S
    h_prev = None
    f64 = dict(dtype=torch.float64)
    for k in range(S - 1, -1, -1):
        a = ab[tau[k] + shift]
        ap = ab[tau[k - 1] + shift] if k > 0 else torch.tensor(float(final_alpha_bar), **f64)
        if float(ap) == 1.0:
            A, B, Cc, h = torch.tensor(0.0, **f64), torch.tensor(1.0, **f64), torch.tensor(0.0, **f64), None
        else:
            h = lam_of(ap) - lam_of(a)
            A = torch.sqrt(1.0 - ap) / torch.sqrt(1.0 - a)
            g = -torch.sqrt(ap) * torch.expm1(-h)
            if k == S - 1 or k == 0:
                B, Cc = g, torch.tensor(0.0, **f64)
            else:
                r = h_prev / h
                B, Cc = g * (1.0 + 1.0 / (2.0 * r)), -g / (2.0 * r)
        rows[k] = torch.stack([torch.sqrt(1.0 - a), torch.sqrt(a), A, B, Cc])
        h_prev = h
    return torch.stack(rows)


def guided_eps(eps_c, eps_u, w):
    """eps = w1 * eps_c - wf * eps_u with w1 = (float)(1 + w), wf = (float)w."""
    return torch.tensor(np.float32(1.0 + w)) * eps_c - torch.tensor(np.float32(w)) * eps_u


def update(x, eps, x0_prev, row, clip_x0):
    """One update on CPU tensors of one dtype (fp32 for the kernels, float64 for the arithmetic tests) -> (x', x0).  ``x0_prev`` is
    not touched when C == 0 (it may hold NaN, or be None).  torch.clamp keeps a NaN a NaN."""
    assert x.dtype == eps.dtype == row.dtype
    s1m, sa, A, B, Cc = (row[i] for i in range(5))
    x0 = (x - eps * s1m) / sa
    if clip_x0:
        x0 = torch.clamp(x0, -1.0, 1.0)
    v = A * x + B * x0
    if float(Cc) != 0.0:
        v = v + Cc * x0_prev
    return v, x0


# ----------------------------------------------------------------------------------------------------------------------
# the analytic model: data N(MU, SD^2), whose noise prediction and probability-flow solution are closed-form
# ----------------------------------------------------------------------------------------------------------------------
MU, SD = 0.3, 0.5
START = (1.7, -0.4, 0.2, -2.1)


def gauss_eps(x, a):
    """E[eps | x_t = x] at alphas_bar a: sqrt(1 - a) * (x - sqrt(a) * MU) / (SD^2 * a + 1 - a)."""
    return math.sqrt(1.0 - a) * (x - math.sqrt(a) * MU) / (SD * SD * a + 1.0 - a)


def gauss_flow(x, a_from, a_to):
    """The probability-flow ODE's exact solution: it keeps the standardised value under the marginal N(sqrt(a) MU, SD^2 a + 1 - a)."""
    var = lambda a: SD * SD * a + 1.0 - a                                                     # noqa: E731
    return math.sqrt(a_to) * MU + math.sqrt(var(a_to) / var(a_from)) * (x - math.sqrt(a_from) * MU)
