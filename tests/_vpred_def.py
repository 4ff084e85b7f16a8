"""TEST INFRASTRUCTURE ONLY -- the definition the v-prediction / min-SNR tests measure against, in plain torch on the CPU, operations
written out.  Written from the definition alone; it shares no code with the package.

For sample b with k = t[b], a = sqrt(ab)[k] and s = sqrt(1 - ab)[k] AS THE FP32 CASTS ``extract`` PRODUCES, ``out`` the network's
output and ``div`` the y0 divisor (the reference's literal 255):

    prediction "eps":  target = noise               y0 = ((1 / a) * (y_t - s * out)) / div    eps_hat = out
                       chain = d y0 / d out = -(1 / a) * s / div
    prediction "v":    target = a * noise - s * gt  y0 = (a * y_t - s * out) / div            eps_hat = a * out + s * y_t
                       chain = -s / div                                                       (Salimans & Ho 2022)

    snr[k] = ab[k] / (1 - ab[k])                                   float64
    min-SNR-gamma (Hang et al. 2023):  w[k] = min(snr, gamma) / snr  for eps,  min(snr, gamma) / (snr + 1)  for v;  fp32 cast once
    mse = w[k] * (out - target)^2   (no weight: no multiply);  the terms taken on y0 are not weighted
    d_out = d_mse * w * 2 * (out - target) + (d_y0 + d_col * dcol/dy0) * chain

The sampler's conversion is ``eps_hat`` in fp32: two products and one sum, one rounding each, with a, s at the time step the model
was CALLED with (the trainer's ``ab[t]``, not the DDIM loop's ``ab[t + 1]``)."""
import torch
import torch.nn.functional as F

B1, BT, T = 1e-4, 0.02, 1000


def schedule(beta_1=B1, beta_T=BT, n=T):
    """-> (betas, alphas_bar) in float64, as the modules form them."""
    betas = torch.linspace(beta_1, beta_T, n).double()
    return betas, torch.cumprod(1.0 - betas, dim=0)


def tables32(ab):
    """-> (sqrt(ab), sqrt(1 - ab)) as the fp32 tables: the square root in float64, then one cast."""
    return torch.sqrt(ab).float(), torch.sqrt(1.0 - ab).float()


def snr(ab):
    return ab / (1.0 - ab)


def weights(ab, gamma, prediction):
    """float64 [T]."""
    r = snr(ab)
    capped = torch.minimum(r, torch.full_like(r, float(gamma)))
    return capped / r if prediction == "eps" else capped / (r + 1.0)


def _col(a, t):
    return a[t].double().view(-1, 1, 1, 1)


def tail(prediction, out, noise, y_t, gt, t, sa32, s1m32, w32=None, div=255.0):
    """The definition in float64 on fp32 (or float64) inputs -> dict(target, y0, eps_hat, mse, chain); ``w32``: the fp32 weight table or
    None.  ``chain`` is [B, 1, 1, 1]."""
    a, s = _col(sa32, t), _col(s1m32, t)
    o, n, y, g = out.double(), noise.double(), y_t.double(), gt.double()
    if prediction == "eps":
        target = n
        y0 = ((1.0 / a) * (y - s * o)) / div
        eps_hat = o
        chain = -(1.0 / a) * s / div
    else:
        assert prediction == "v"
        target = a * n - s * g
        y0 = (a * y - s * o) / div
        eps_hat = a * o + s * y
        chain = -s / div
    mse = (o - target) ** 2
    if w32 is not None:
        mse = _col(w32, t) * mse
    return dict(target=target, y0=y0, eps_hat=eps_hat, mse=mse, chain=chain)


def colour(y0, gt):
    """-> (col, d col / d y0) in float64 from the given y0 (the eps branches of F.normalize / cosine_similarity depend on the exact
    fp32 value of y0, so the tests start this from the kernel's own y0, as the existing tail test does)."""
    u = y0.detach().cpu().double().requires_grad_(True)
    cos = F.cosine_similarity(F.normalize(u, p=2, dim=1), F.normalize(gt.double(), p=2, dim=1), dim=1)
    col = 1 - cos.mean()
    (gu,) = torch.autograd.grad(col, u)
    return col.detach(), gu


def d_out(prediction, out, noise, y_t, gt, t, sa32, s1m32, w32, div, y0, d_mse, d_y0, d_col):
    """The backward of the definition in float64; an absent incoming gradient is None."""
    d = tail(prediction, out, noise, y_t, gt, t, sa32, s1m32, w32, div)
    g = torch.zeros_like(d["mse"])
    if d_mse is not None:
        w = 1.0 if w32 is None else _col(w32, t)
        g = g + d_mse.double() * w * 2 * (out.double() - d["target"])
    inner = torch.zeros_like(g)
    if d_y0 is not None:
        inner = inner + d_y0.double()
    if d_col is not None:
        inner = inner + d_col.double() * colour(y0, gt)[1]
    return g + inner * d["chain"]


def v_y0_fp32(out, y_t, t, sa32, s1m32):
    """y0 of prediction "v" at div = 1 in fp32: two products, one difference."""
    a, s = sa32[t].view(-1, 1, 1, 1), s1m32[t].view(-1, 1, 1, 1)
    assert out.dtype == y_t.dtype == a.dtype == torch.float32
    return a * y_t - s * out


def v_to_eps_fp32(out, y, t, sa32, s1m32):
    """The sampler's conversion on fp32 CPU tensors [B, ...]: a * out + s * y, one rounding per written operation."""
    shape = [out.shape[0]] + [1] * (out.dim() - 1)
    a, s = sa32[t].view(shape), s1m32[t].view(shape)
    assert out.dtype == y.dtype == a.dtype == torch.float32
    return a * out + s * y


def as_eps_model(model_v, sa32, s1m32):
    """``model_v(x6, t)`` read as a v network -> the reference-shaped ``model_eps(x6, t)``: the state the model sees is channels 3: of
    its input."""
    def model_eps(x6, t):
        return v_to_eps_fp32(model_v(x6, t), x6[:, 3:].float(), t, sa32, s1m32)
    return model_eps


def ddim_loop(model_eps, img01, y_T, ab, tau, eta=0.0, noise_by_step=None):
    """The reference's DDIM loop (diffusion/Diffusion.py:243-267) in fp32 on the CPU on the increasing time steps ``tau``; with
    ``noise_by_step`` (the draw of the j-th step in call order) the stochastic term is kept with ``eta`` in place of the literal 0.
    -> the pre-clip state after every step."""
    y, traj = y_T, []
    tau = list(tau)
    tau_next = [-1] + tau[:-1]
    for j, (i, i_next) in enumerate(zip(reversed(tau), reversed(tau_next))):
        t = torch.full((y.shape[0],), i, dtype=torch.long)
        at, at_next = ab[i + 1].float(), ab[i_next + 1].float()
        eps = model_eps(torch.cat([img01, y], dim=1).float(), t)
        y0 = (y - eps * (1 - at).sqrt()) / at.sqrt()
        if noise_by_step is None:
            c2 = (1 - at_next).sqrt()
            y = at_next.sqrt() * y0 + c2 * eps
        else:
            c1 = eta * ((1 - at / at_next) * (1 - at_next) / (1 - at)).sqrt()
            c2 = ((1 - at_next) - c1 ** 2).sqrt()
            y = ((at_next.sqrt() * y0) + (c1 * noise_by_step[j])) + (c2 * eps)
        traj.append(y)
    return traj


def dpmpp_loop(model_eps, img01, y_T, tau, tab32, update):
    """DPM-Solver++(2M) on ``tau`` with the fp32 table ``tab32`` (row k of tests/_dpmpp_def.table at shift 1) and that module's
    ``update(x, eps, x0_prev, row, clip_x0)``."""
    y, prev, traj = y_T, None, []
    for k in range(len(tau) - 1, -1, -1):
        t = torch.full((y.shape[0],), tau[k], dtype=torch.long)
        eps = model_eps(torch.cat([img01, y], dim=1).float(), t)
        y, prev = update(y, eps, prev, tab32[k], False)
        traj.append(y)
    return traj


def tiled_ddim_loop(model_eps, img01, y_T, ab, tau, lay, windows, blend):
    """The DDIM loop over overlapping windows (tests/_tiled_def.py: ``lay`` a Layout, ``windows`` and ``blend`` its functions): every
    window goes through ``model_eps`` -- so the conversion of a v network sees the WINDOW's own y -- the estimates are blended and
    one update is applied to the full image."""
    B = y_T.shape[0]
    cond_w = windows(img01, lay)
    y, traj = y_T, []
    tau = list(tau)
    tau_next = [-1] + tau[:-1]
    for i, i_next in zip(reversed(tau), reversed(tau_next)):
        t = torch.full((cond_w.shape[0],), i, dtype=torch.long)
        at, at_next = ab[i + 1].float(), ab[i_next + 1].float()
        eps = blend(model_eps(torch.cat([cond_w, windows(y, lay)], dim=1).float(), t), B, lay)
        y0 = (y - eps * (1 - at).sqrt()) / at.sqrt()
        y = at_next.sqrt() * y0 + (1 - at_next).sqrt() * eps
        traj.append(y)
    return traj


def ancestral_loop(model_eps, img01, y_T, betas, noise_by_step):
    """The reference's ancestral loop (diffusion/Diffusion.py:224-236) in fp32 on the CPU with the draws handed in ->
    the pre-clip state after every step.  ``noise_by_step[k]`` is the draw of the k-th step in call order (the last step adds none)."""
    n = betas.numel()
    alphas = 1.0 - betas
    ab = torch.cumprod(alphas, dim=0)
    ab_prev = F.pad(ab, [1, 0], value=1)[:n]
    coeff1 = torch.sqrt(1.0 / alphas)
    coeff2 = coeff1 * (1.0 - alphas) / torch.sqrt(1.0 - ab)
    posterior_var = betas * (1.0 - ab_prev) / (1.0 - ab)
    var = torch.cat([posterior_var[1:2], betas[1:]])
    y, traj = y_T, []
    for k, step in enumerate(reversed(range(n))):
        t = torch.full((y.shape[0],), step, dtype=torch.long)
        eps = model_eps(torch.cat([img01, y], dim=1).float(), t)
        mean = coeff1[step].float() * y - coeff2[step].float() * eps
        y = mean + torch.sqrt(var[step].float()) * noise_by_step[k] if step > 0 else mean
        traj.append(y)
    return traj
