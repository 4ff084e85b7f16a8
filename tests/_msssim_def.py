"""The MS-SSIM + L1 loss the package implements (hdiff_amd.Loss.loss.MSSSIMLoss), written out in torch in two independent forms,
and the inputs of its tests.  Helper module, not a test file.

Definition (x prediction, y target, [B, 3, H, W]; sigmas (0.5, 1, 2, 4, 8), data_range 1, K (0.01, 0.03), alpha 0.025,
compensation 200): g_s = the 1-D Gaussian exp(-k^2 / (2 s^2)) over k = -(n // 2) .. n // 2, n = int(4 sigma_max + 1), normalised
to sum 1; G_s * a = zero-padded correlation of a plane with g_s g_s^T.  For a pair (channel c, scale s): mu_x = G*x_c, mu_y = G*y_c,
s_x = G*(x_c^2) - mu_x^2, s_y likewise, s_xy = G*(x_c y_c) - mu_x mu_y, l = (2 mu_x mu_y + C1) / (mu_x^2 + mu_y^2 + C1),
cs = (2 s_xy + C2) / (s_x + s_y + C2).  A layout lists 15 pairs and three indices: PIcs = product of cs over the 15, lM = product of
l over the three, ms = 1 - lM PIcs, l1 = channel mean of G_{sigma_max} * |x_c - y_c|,
loss = compensation (alpha ms + (1 - alpha) l1 / data_range), reduced by mean or sum over [B, H, W].

  dense_loss      the kornia layout as ONE grouped 33x33 convolution per product (15 output maps, groups = 3): map o reads channel
                  o // 5 with sigmas[o // 3], lM over maps 12, 13, 14
  separable_loss  any layout, pair by pair, as a row filter followed by a column filter, driven by layout_table()
"""
import torch
import torch.nn.functional as F

SIGMAS = (0.5, 1.0, 2.0, 4.0, 8.0)


def gauss_1d(sigma, half, dtype):
    k = torch.arange(-half, half + 1, dtype=torch.float64)
    g = torch.exp(-(k * k) / (2.0 * sigma * sigma))
    return (g / g.sum()).to(dtype)


def layout_table(layout, n=5):
    """-> (list of 15 (channel, scale index) pairs, the three indices whose l enters lM)."""
    if layout == "kornia":
        return [(o // n, o // 3) for o in range(3 * n)], [3 * n - 3, 3 * n - 2, 3 * n - 1]
    if layout == "per_channel":
        pairs = [(c, s) for c in range(3) for s in range(n)]
        return pairs, [i for i, (_, s) in enumerate(pairs) if s == n - 1]
    raise ValueError(layout)


def _finish(l_maps, cs_maps, l_idx, l1, alpha, compensation, data_range, reduction):
    pics = cs_maps[0]
    for m in cs_maps[1:]:
        pics = pics * m
    lm = l_maps[l_idx[0]] * l_maps[l_idx[1]] * l_maps[l_idx[2]]
    pix = compensation * (alpha * (1.0 - lm * pics) + (1.0 - alpha) * l1 / data_range)
    return pix.mean() if reduction == "mean" else pix.sum()


def dense_loss(x, y, sigmas=SIGMAS, data_range=1.0, K=(0.01, 0.03), alpha=0.025, compensation=200.0, reduction="mean"):
    n = len(sigmas)
    half = int(4 * sigmas[-1] + 1) // 2
    c1, c2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    g = [gauss_1d(s, half, torch.float64) for s in sigmas]
    win = torch.stack([torch.outer(g[o // 3], g[o // 3]) for o in range(3 * n)]).unsqueeze(1).to(x.dtype).to(x.device)   # [15, 1, 33, 33]

    def filt(a, w):
        return F.conv2d(a, w, padding=half, groups=3)
    mux, muy = filt(x, win), filt(y, win)
    sx = filt(x * x, win) - mux * mux
    sy = filt(y * y, win) - muy * muy
    sxy = filt(x * y, win) - mux * muy
    l = (2 * mux * muy + c1) / (mux * mux + muy * muy + c1)
    cs = (2 * sxy + c2) / (sx + sy + c2)
    l1 = filt((x - y).abs(), win[-3:]).mean(dim=1)
    last = 3 * n
    return _finish([l[:, o] for o in range(last)], [cs[:, o] for o in range(last)], [last - 3, last - 2, last - 1], l1, alpha,
                   compensation, data_range, reduction)


def _sep(a, g):
    """Zero-padded separable filter of [B, H, W] planes with the 1-D window g."""
    half = g.numel() // 2
    a = a.unsqueeze(1)
    a = F.conv2d(a, g.view(1, 1, 1, -1), padding=(0, half))
    a = F.conv2d(a, g.view(1, 1, -1, 1), padding=(half, 0))
    return a.squeeze(1)


def separable_loss(x, y, layout="kornia", sigmas=SIGMAS, data_range=1.0, K=(0.01, 0.03), alpha=0.025, compensation=200.0,
                   reduction="mean"):
    n = len(sigmas)
    half = int(4 * sigmas[-1] + 1) // 2
    c1, c2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    g = [gauss_1d(s, half, x.dtype).to(x.device) for s in sigmas]
    pairs, l_idx = layout_table(layout, n)
    cache = {}
    for c, s in pairs:
        if (c, s) in cache:
            continue
        xc, yc = x[:, c], y[:, c]
        mux, muy = _sep(xc, g[s]), _sep(yc, g[s])
        sx = _sep(xc * xc, g[s]) - mux * mux
        sy = _sep(yc * yc, g[s]) - muy * muy
        sxy = _sep(xc * yc, g[s]) - mux * muy
        cache[(c, s)] = ((2 * mux * muy + c1) / (mux * mux + muy * muy + c1), (2 * sxy + c2) / (sx + sy + c2))
    l1 = sum(_sep((x[:, c] - y[:, c]).abs(), g[-1]) for c in range(3)) / 3.0
    return _finish([cache[p][0] for p in pairs], [cache[p][1] for p in pairs], l_idx, l1, alpha, compensation, data_range, reduction)


def loss_and_grad(fn, x, y, dtype, upstream=1.0, **kw):
    """-> (loss, d(upstream * loss)/dx) of ``fn`` evaluated on the CPU in ``dtype``."""
    xd = x.detach().cpu().to(dtype).requires_grad_(True)
    yd = y.detach().cpu().to(dtype)
    loss = fn(xd, yd, **kw)
    (loss * upstream).backward()
    return loss.detach(), xd.grad.detach()


# ----------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------
def smooth_field(B, H, W, gen):
    """A smooth random field in [0, 1]: coarse noise enlarged bilinearly."""
    ch, cw = max(2, H // 8 + 1), max(2, W // 8 + 1)
    coarse = torch.rand(B, 3, ch, cw, generator=gen, dtype=torch.float64)
    return F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)


def image_like_pair(B, H, W, seed, noise=0.05):
    """(prediction, target) fp32 in [0, 1]: one smooth field, a distorted and noisy copy as the prediction."""
    gen = torch.Generator().manual_seed(seed)
    y = smooth_field(B, H, W, gen)
    x = 0.85 * y + 0.1 * smooth_field(B, H, W, gen) + noise * torch.randn(B, 3, H, W, generator=gen, dtype=torch.float64)
    y = y + 0.02 * torch.randn(B, 3, H, W, generator=gen, dtype=torch.float64)
    return x.clamp(0, 1).float(), y.clamp(0, 1).float()


def uniform_pair(B, H, W, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(B, 3, H, W, generator=gen), torch.rand(B, 3, H, W, generator=gen)


def trainer_like_pair(B, H, W, seed):
    """The reference trainer's own operands: a target in [-1, 1] and a prediction carrying the stray / 255."""
    gen = torch.Generator().manual_seed(seed)
    y = (smooth_field(B, H, W, gen) * 2 - 1).float()
    x = ((y.double() + 0.3 * torch.randn(B, 3, H, W, generator=gen, dtype=torch.float64)) / 255.0).float()
    return x, y
