"""Definitions the perceptual kernels and classes are held to (no package import).

  * the VGG trunk, the summed L1 loss on its taps, the Charbonnier map and the LPIPS distance: torch on the CPU, in the dtype of the
    tensors handed in (float64 is the reference; the same code in float32 is the yardstick an fp32 implementation is measured by);
  * ReLU, 2x2 max-pooling forward / backward and the L1-mean backward: fp32 numpy with the tie and sign rules of include/hdiff.h
    (the first maximal element of a window in row-major order takes the gradient; sign(0) = 0).

Fixture recipe (the margins of test_perceptual_cpu.py were checked with exactly this):
  weights  torch.Generator().manual_seed(seed); per conv in order randn(c, cin, 3, 3) * sqrt(2 / (9 cin)), then randn(c) * 0.05, float64
  images   torch.Generator().manual_seed(1000 + seed); x = rand(1, 3, H, W) * 2 - 1, y = clamp(x + 0.3 randn(1, 3, H, W), -1, 1), float64
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

VGG_CFGS = {
    "vgg11": [64, "M", 128, "M", 256, 256, "M", 512, 512, "M", 512, 512, "M"],
    "vgg13": [64, 64, "M", 128, 128, "M", 256, 256, "M", 512, 512, "M", 512, 512, "M"],
    "vgg16": [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"],
    "vgg19": [64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512, 512, 512, 512, "M"],
}
LOSS_TAPS = (3, 8, 15, 22)
LPIPS_TAPS = (3, 8, 15, 22, 29)
LPIPS_SHIFT = (-0.030, -0.088, -0.188)
LPIPS_SCALE = (0.458, 0.448, 0.450)
DELTA = 2e-5
GRAD_FIXTURES = ((8, 8, 2), (8, 8, 4), (9, 11, 2))          # (H, W, seed)


def layers_of(cfg):
    """The Sequential as a list of ("conv", cin, cout) / ("relu",) / ("pool",)."""
    layers, cin = [], 3
    for v in cfg:
        if v == "M":
            layers.append(("pool",))
        else:
            layers += [("conv", cin, v), ("relu",)]
            cin = v
    return layers


def make_weights(cfg, seed):
    """-> [(weight, bias)] per conv in order, float64."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for layer in layers_of(cfg):
        if layer[0] == "conv":
            _, cin, c = layer
            w = torch.randn(c, cin, 3, 3, generator=g, dtype=torch.float64) * math.sqrt(2.0 / (9 * cin))
            b = torch.randn(c, generator=g, dtype=torch.float64) * 0.05
            out.append((w, b))
    return out


def make_images(seed, H, W, B=1):
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.rand(B, 3, H, W, generator=g, dtype=torch.float64) * 2 - 1
    y = (x + 0.3 * torch.randn(B, 3, H, W, generator=g, dtype=torch.float64)).clamp(-1, 1)
    return x, y


def rounded(weights):
    """The weights as an fp32 implementation holds them, promoted back: what the float64 reference of a GPU run is evaluated on."""
    return [(w.float().double(), b.float().double()) for w, b in weights]


def state_dict_of(cfg, weights):
    """The weights under torchvision's ``features`` keys, fp32."""
    sd, k = {}, 0
    for i, layer in enumerate(layers_of(cfg)):
        if layer[0] == "conv":
            sd[f"{i}.weight"], sd[f"{i}.bias"] = weights[k][0].float(), weights[k][1].float()
            k += 1
    return sd


def trunk(x, weights, cfg, taps, record=None):
    """Activations at the Sequential indices ``taps`` in the dtype of ``x``.  ``record``: a dict that receives "pre" (every conv
    output) and "pool_in" (every pooling input) up to the last tap."""
    taps = sorted(t for t in set(taps) if t < len(layers_of(cfg)))
    out, k = [], 0
    for i, layer in enumerate(layers_of(cfg)[:taps[-1] + 1]):
        if layer[0] == "conv":
            w, b = weights[k]
            k += 1
            x = F.conv2d(x, w.to(x.dtype), b.to(x.dtype), padding=1)
            if record is not None:
                record.setdefault("pre", []).append(x)
        elif layer[0] == "relu":
            x = torch.relu(x)
        else:
            if record is not None:
                record.setdefault("pool_in", []).append(x)
            x = F.max_pool2d(x, 2, 2)
        if i in taps:
            out.append(x)
    return out


def tap_terms(x, y, weights, cfg, taps=LOSS_TAPS):
    return [(fx - fy).abs().mean() for fx, fy in zip(trunk(x, weights, cfg, taps), trunk(y, weights, cfg, taps))]


def loss_def(x, y, weights, cfg, taps=LOSS_TAPS):
    """Sum over the taps of mean |feat(x) - feat(y)|."""
    return sum(tap_terms(x, y, weights, cfg, taps))


def loss_and_grad(x, y, weights, cfg, taps=LOSS_TAPS, dtype=torch.float64):
    """-> (value, d value / d x) as float64 numbers / tensor, evaluated in ``dtype``; ``y`` is a constant."""
    xx = x.to(dtype).clone().requires_grad_(True)
    value = loss_def(xx, y.to(dtype), weights, cfg, taps)
    (grad,) = torch.autograd.grad(value, xx)
    return float(value.detach()), grad.double()


def margins(x, y, weights, cfg, taps=LOSS_TAPS):
    """-> (min |pre-activation| of the x pass, min gap between the two largest entries of a pooling window whose largest is not 0,
    min non-zero |feat(x) - feat(y)| over the taps), in float64."""
    rec = {}
    fx = trunk(x.double(), weights, cfg, taps, rec)
    fy = trunk(y.double(), weights, cfg, taps)
    pre = min(float(p.abs().min()) for p in rec["pre"])
    gap = math.inf
    for p in rec["pool_in"]:
        H, W = p.shape[2] // 2 * 2, p.shape[3] // 2 * 2
        win = F.unfold(p[:, :, :H, :W].reshape(-1, 1, H, W), 2, stride=2)          # [planes, 4, windows]
        top = win.sort(dim=1, descending=True).values
        live = top[:, 0] != 0
        if live.any():
            gap = min(gap, float((top[:, 0] - top[:, 1])[live].min()))
    tap = math.inf
    for a, b in zip(fx, fy):
        d = (a - b).abs()
        if (d != 0).any():
            tap = min(tap, float(d[d != 0].min()))
    return pre, gap, tap


def charbonnier_def(a, b):
    d = a - b
    return torch.sqrt(d * d + 1) - 1


def charbonnier_grad_def(a, b, dy):
    d = a - b
    return dy * d / torch.sqrt(d * d + 1)


def lpips_def(a01, b01, weights, lin):
    """LPIPS v0.1 (VGG16) of images in [0, 1], in their dtype: -> [N]."""
    dt = a01.dtype
    shift = torch.tensor(LPIPS_SHIFT, dtype=dt).view(1, 3, 1, 1)
    scale = torch.tensor(LPIPS_SCALE, dtype=dt).view(1, 3, 1, 1)
    cfg = VGG_CFGS["vgg16"]
    f0 = trunk(((a01 * 2 - 1) - shift) / scale, weights, cfg, LPIPS_TAPS)
    f1 = trunk(((b01 * 2 - 1) - shift) / scale, weights, cfg, LPIPS_TAPS)
    total = torch.zeros(a01.shape[0], dtype=dt)
    for u, v, w in zip(f0, f1, lin):
        nu = u / (u.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10)
        nv = v / (v.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10)
        total = total + (w.to(dt).view(1, -1, 1, 1) * (nu - nv) ** 2).sum(dim=1).mean(dim=(1, 2))
    return total


def make_lin(seed):
    """Five non-negative weight vectors ``rand * 2 / C`` shaped [1, C, 1, 1], float64."""
    g = torch.Generator().manual_seed(2000 + seed)
    return [torch.rand(1, c, 1, 1, generator=g, dtype=torch.float64) * 2 / c for c in (64, 128, 256, 512, 512)]


# ---------------------------------------------------------------------------------------------------- fp32 numpy, bit for bit
def relu_fwd(x):
    x = np.asarray(x, dtype=np.float32)
    return np.where(x > 0, x, np.where(np.isnan(x), x, np.float32(0))).astype(np.float32)          # a NaN stays a NaN


def relu_bwd(y, dy):
    return np.where(np.asarray(y, dtype=np.float32) > 0, np.asarray(dy, dtype=np.float32), np.float32(0)).astype(np.float32)


def _windows(x):
    """[planes, H, W] -> the four window entries in row-major order, each [planes, H // 2, W // 2]."""
    H, W = x.shape[1] // 2 * 2, x.shape[2] // 2 * 2
    x = x[:, :H, :W]
    return x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2]


def _choice(x):
    w = _windows(x)
    top, k = w[0].copy(), np.zeros(w[0].shape, dtype=np.int64)
    for j in (1, 2, 3):
        later = ~np.isnan(top) & ((w[j] > top) | np.isnan(w[j]))      # strictly greater only; a NaN counts as maximal, the first wins
        top = np.where(later, w[j], top)
        k = np.where(later, j, k)
    return top, k


def pool_fwd(x):
    return _choice(np.asarray(x, dtype=np.float32))[0].astype(np.float32)


def pool_bwd(x, dy):
    x, dy = np.asarray(x, dtype=np.float32), np.asarray(dy, dtype=np.float32)
    _, k = _choice(x)
    dx = np.zeros_like(x)
    OH, OW = k.shape[1], k.shape[2]
    for j, (r, c) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        dx[:, r:2 * OH:2, c:2 * OW:2] = np.where(k == j, dy, np.float32(0))
    return dx


def l1_bwd(a, b, g):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    c = np.float32(g) / np.float32(a.size)
    return np.where(a > b, c, np.where(a < b, -c, np.float32(0))).astype(np.float32)
