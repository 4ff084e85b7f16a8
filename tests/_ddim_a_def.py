"""The definition the strided DDIM tests of the label-conditioned sampler measure against, in plain torch on the CPU: the time-step
rule, the float64 coefficient table, and the fp32 per-step update with one rounding per written operation.  Written from the
definition alone; it shares no code with the package.

    tau_k = ((k + 1) * T) // S - 1,  k = 0 .. S-1
    ab = cumprod(1 - betas);  a = ab[tau_k];  a' = ab[tau_(k-1)] (k > 0), a' = 1 (k = 0)
    sigma = eta * sqrt((1 - a') / (1 - a)) * sqrt(1 - a / a')
    row k = (s1m = sqrt(1 - a), sa = sqrt(a), san = sqrt(a'), c2 = sqrt(max(1 - a' - sigma^2, 0)), sigma)      float64, then fp32 once

    eps = w1 * eps_c - wf * eps_u                         w1 = (float)(1 + w), wf = (float)w
    x0  = (x - eps * s1m) / sa
    if clip_x0:  x0 = min(max(x0, -1), 1);  eps = (x - sa * x0) / s1m
    v   = san * x0 + c2 * eps
    if k > 0 and sigma > 0:  v = v + sigma * z
"""
import numpy as np
import torch

S1M, SA, SAN, C2, SIGMA = range(5)


def timesteps(T, S):
    return [((k + 1) * T) // S - 1 for k in range(S)]


def table(betas, tau, eta):
    """float64 [S, 5] from a float64 betas vector and the time-step list."""
    betas = torch.as_tensor(betas).detach().cpu().double()
    ab = torch.cumprod(1.0 - betas, dim=0)
    rows = []
    for k, t in enumerate(tau):
        a = ab[t]
        ap = ab[tau[k - 1]] if k > 0 else torch.tensor(1.0, dtype=torch.float64)
        sigma = eta * torch.sqrt((1.0 - ap) / (1.0 - a)) * torch.sqrt(1.0 - a / ap)
        arg = 1.0 - ap - sigma * sigma
        rows.append(torch.stack([torch.sqrt(1.0 - a), torch.sqrt(a), torch.sqrt(ap),
                                 torch.sqrt(torch.clamp(arg, min=0.0)), sigma]))
    return torch.stack(rows)


def c2_sqrt_argument(betas, tau, eta):
    """The argument of c2's square root before the max(., 0), float64 [S]."""
    betas = torch.as_tensor(betas).detach().cpu().double()
    ab = torch.cumprod(1.0 - betas, dim=0)
    a = ab[torch.tensor(list(tau))]
    ap = torch.cat([torch.ones(1, dtype=torch.float64), a[:-1]])
    sigma = eta * torch.sqrt((1.0 - ap) / (1.0 - a)) * torch.sqrt(1.0 - a / ap)
    return 1.0 - ap - sigma * sigma


def guided_eps(eps_c, eps_u, w):
    """eps = w1 * eps_c - wf * eps_u with w1 = (float)(1 + w), wf = (float)w."""
    return torch.tensor(np.float32(1.0 + w)) * eps_c - torch.tensor(np.float32(w)) * eps_u


def update(x, eps, z, row, k, clip_x0):
    """One update in fp32 on CPU tensors from the guided eps; `row` is the fp32 cast of table()[k]; z may be None when no noise is
    added (k = 0 or sigma = 0).  torch.clamp keeps a NaN a NaN."""
    assert x.dtype == torch.float32 and eps.dtype == torch.float32 and row.dtype == torch.float32
    s1m, sa, san, c2, sigma = (row[i] for i in range(5))
    x0 = (x - eps * s1m) / sa
    if clip_x0:
        x0 = torch.clamp(x0, -1.0, 1.0)
        eps = (x - sa * x0) / s1m
    v = san * x0 + c2 * eps
    if k > 0 and float(sigma) > 0:
        v = v + sigma * z
    return v


def step(x, eps_c, eps_u, z, row, k, w, clip_x0):
    return update(x, guided_eps(eps_c, eps_u, w), z, row, k, clip_x0)
