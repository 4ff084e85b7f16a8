"""TEST INFRASTRUCTURE ONLY -- the definition the multi-sample posterior tests measure against, in plain Python / torch on the CPU.
Written from the definition alone; it shares no code with the package.

    mix(z):  z += 0x9E3779B97F4A7C15 ; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9 ; z = (z ^ z >> 27) * 0x94D049BB133111EB ; z ^ z >> 31
    seed(s, image, replica) = mix(mix(mix(s) ^ image) ^ replica)                                   (all mod 2^64)

    row k of the eta table, a = ab[tau_k + 1], a' = ab[tau_(k-1) + 1] (k = 0: ab[0]):
        c1 = eta * sqrt((1 - a / a') * (1 - a') / (1 - a)) ;  c2 = sqrt((1 - a') - c1^2)
        (sqrt(1 - a), sqrt(a), sqrt(a'), c1, c2)

    y0 = (y - eps * s1m) / sa ;  y' = ((san * y0) + (c1 * z)) + (c2 * eps)          five fp32 operations, one rounding each

    m = (x_0 + x_1 + ...) / K ;  std = sqrt(((x_0 - m)^2 + (x_1 - m)^2 + ...) / (K - 1)), 0 for K = 1
        in float64, summed in replica order, each rounded once to fp32
"""
import torch

M64 = (1 << 64) - 1
Y_T_OFFSET = (1 << 32) - 1


def mix(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def seed_of(seed, image, replica):
    return mix(mix(mix(seed & M64) ^ (image & M64)) ^ (replica & M64))


def as_int64(s):
    """A uint64 as the int64 of the same bits (what a torch tensor holds)."""
    return s - (1 << 64) if s >= (1 << 63) else s


def eta_table(betas, tau, eta):
    """float64 [S, 5], row k = (s1m, sa, san, c1, c2) of the image-conditioned sampler's step from tau_k to tau_(k-1)."""
    ab = torch.cumprod(1.0 - torch.as_tensor(betas).detach().cpu().double(), dim=0)
    rows = []
    for k, t in enumerate(tau):
        a = ab[t + 1]
        an = ab[tau[k - 1] + 1] if k > 0 else ab[0]
        c1 = eta * torch.sqrt((1 - a / an) * (1 - an) / (1 - a))
        rows.append(torch.stack([torch.sqrt(1 - a), torch.sqrt(a), torch.sqrt(an), c1, torch.sqrt((1 - an) - c1 * c1)]))
    return torch.stack(rows)


def eta_step(y, eps, z, row):
    """One update on fp32 CPU tensors: the five written operations, one rounding each."""
    assert y.dtype == eps.dtype == z.dtype == row.dtype == torch.float32
    s1m, sa, san, c1, c2 = (row[i] for i in range(5))
    y0 = (y - eps * s1m) / sa
    return ((san * y0) + (c1 * z)) + (c2 * eps)


def stats(x):
    """x fp32 [B, K, n] -> (mean, std) fp32 [B, n]."""
    K = x.shape[1]
    xd = x.double()
    s = xd[:, 0].clone()
    for k in range(1, K):
        s = s + xd[:, k]
    m = s / K
    if K == 1:
        return m.float(), torch.zeros_like(m).float()
    d = xd[:, 0] - m
    q = d * d
    for k in range(1, K):
        d = xd[:, k] - m
        q = q + d * d
    return m.float(), torch.sqrt(q / (K - 1)).float()


def eta_loop(model_eps, img01, y_T, alphas_bar, tau, eta, noise_by_step):
    """The reference's DDIM loop (diffusion/Diffusion.py:243-267) in fp32 on the CPU with ``eta`` in place of its literal 0 and the
    draws handed in: ``model_eps(x6, t)`` is the reference-shaped model, ``alphas_bar`` the float64 schedule, ``tau`` the increasing
    time steps, ``noise_by_step[j]`` the ``randn_like`` of the j-th step in call order.  -> the pre-clip state after every step."""
    y, traj = y_T, []
    tau_next = [-1] + list(tau[:-1])
    for j, (i, i_next) in enumerate(zip(reversed(tau), reversed(tau_next))):
        t = torch.full((y.shape[0],), i, dtype=torch.long)
        at, at_next = alphas_bar[i + 1].float(), alphas_bar[i_next + 1].float()
        eps = model_eps(torch.cat([img01, y], dim=1).float(), t)
        y0 = (y - eps * (1 - at).sqrt()) / at.sqrt()
        c1 = eta * ((1 - at / at_next) * (1 - at_next) / (1 - at)).sqrt()
        c2 = ((1 - at_next) - c1 ** 2).sqrt()
        y = at_next.sqrt() * y0 + c1 * noise_by_step[j] + c2 * eps
        traj.append(y)
    return traj


# res.txt of evaluate(samples=K): today's lines, `samples:`, per score `<name>_sample_avg:` / `<name>_sample_std:`, `uncertainty_avg:`
def res_keys(today):
    names = [k[:-len("_orgin_avg:")] for k in today]
    return list(today) + ["samples:"] + [f"{n}_sample_{w}:" for n in names for w in ("avg", "std")] + ["uncertainty_avg:"]
