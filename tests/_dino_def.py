"""The definition the DINOv2 perceptual loss (hdiff_amd/dino.py, csrc/dino.hip) is held to: a ViT trunk written out operation by
operation in torch, token-major as dinov2 writes it, in whatever dtype it is handed (float64 is the reference, float32 on the CPU is
the yardstick an fp32 implementation is measured against).  Nothing of the package is imported here.

crop 2 pixels per side -> 14 x 14 patches -> patch matmul -> class token + resized position embedding -> blocks (LayerNorm, qkv,
softmax attention written out, proj, LayerScale, LayerNorm, fc1, exact GELU, fc2, LayerScale) -> LayerNorm.  The taps carry the
multiplicities of the modules that return the same tensor; the loss is sum over taps of multiplicity * mean smooth_l1(a - b).
"""
import math

import torch
import torch.nn.functional as F

PATCH, CROP, EPS = 14, 2, 1e-6


def crop(x):
    return x[:, :, CROP:x.shape[2] - CROP, CROP:x.shape[3] - CROP]


def unfold(x):
    """(B, 3, H, W) cropped -> (B, h*w, 588), columns in (c, ky, kx) order"""
    B, _, H, W = x.shape
    h, w = H // PATCH, W // PATCH
    return x.reshape(B, 3, h, PATCH, w, PATCH).permute(0, 2, 4, 1, 3, 5).reshape(B, h * w, 3 * PATCH * PATCH)


def layer_norm(x, w, b, eps=EPS):
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    var = (d * d).mean(-1, keepdim=True)
    return d / torch.sqrt(var + eps) * w + b


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def attention(qkv, heads):
    """(B, N, 3C) -> (B, N, C): dinov2's reshape(B, N, 3, heads, D), softmax(q k^T / sqrt(D)) v"""
    B, N, C3 = qkv.shape
    D = C3 // 3 // heads
    q, k, v = qkv.reshape(B, N, 3, heads, D).permute(2, 0, 3, 1, 4)
    s = (q * D ** -0.5) @ k.transpose(-2, -1)
    s = s - s.max(-1, keepdim=True).values
    p = torch.exp(s)
    p = p / p.sum(-1, keepdim=True)
    return (p @ v).transpose(1, 2).reshape(B, N, C3 // 3)


def smooth_l1(d):
    a = d.abs()
    return torch.where(a < 1.0, 0.5 * d * d, a - 0.5)


def resize_pos(pos, h, w):
    """(1, 1 + M*M, C) -> (1, 1 + h*w, C): bicubic, align_corners=False, no antialias, scale factors (h + 0.1) / M, (w + 0.1) / M"""
    n = pos.shape[1] - 1
    M = int(round(math.sqrt(n)))
    if (h, w) == (M, M):
        return pos
    g = pos[:, 1:].reshape(1, M, M, -1).permute(0, 3, 1, 2)
    g = F.interpolate(g, scale_factor=((h + 0.1) / M, (w + 0.1) / M), mode="bicubic", align_corners=False, antialias=False)
    assert tuple(g.shape[-2:]) == (h, w)
    return torch.cat([pos[:, :1], g.permute(0, 2, 3, 1).reshape(1, h * w, -1)], dim=1)


BLOCK_TAPS = (("norm1", 1), ("qkv", 1), ("proj", 3), ("ls1", 1), ("norm2", 1), ("fc1", 1), ("act", 2), ("fc2", 3), ("ls2", 1), ("out", 1))


def tap_list(depth):
    """[(key, multiplicity)] in forward order; "patch" appears twice (patch_embed.proj; patch_embed.norm + patch_embed)"""
    taps = [("patch", 1), ("patch", 2)]
    for i in range(depth):
        taps += [(f"{i}.{k}", m) for k, m in BLOCK_TAPS]
    return taps + [("norm", 1), ("cls", 2)]


def features(sd, x, heads, depth, dtype=torch.float64):
    """-> {key: tensor}, token-major"""
    p = {k: v.to(dtype) for k, v in sd.items()}
    x = crop(x.to(dtype))
    B, _, H, W = x.shape
    h, w = H // PATCH, W // PATCH
    Cc = p["cls_token"].shape[-1]
    f = {}
    t = unfold(x) @ p["patch_embed.proj.weight"].reshape(Cc, -1).t() + p["patch_embed.proj.bias"]
    f["patch"] = t
    t = torch.cat([p["cls_token"].expand(B, -1, -1), t], dim=1) + resize_pos(p["pos_embed"], h, w)
    for i in range(depth):
        q = f"blocks.{i}."
        n1 = layer_norm(t, p[q + "norm1.weight"], p[q + "norm1.bias"])
        qkv = n1 @ p[q + "attn.qkv.weight"].t() + p[q + "attn.qkv.bias"]
        pr = attention(qkv, heads) @ p[q + "attn.proj.weight"].t() + p[q + "attn.proj.bias"]
        s1 = p[q + "ls1.gamma"] * pr
        t1 = t + s1
        n2 = layer_norm(t1, p[q + "norm2.weight"], p[q + "norm2.bias"])
        fc1 = n2 @ p[q + "mlp.fc1.weight"].t() + p[q + "mlp.fc1.bias"]
        act = gelu(fc1)
        fc2 = act @ p[q + "mlp.fc2.weight"].t() + p[q + "mlp.fc2.bias"]
        s2 = p[q + "ls2.gamma"] * fc2
        t = t1 + s2
        for k, v in (("norm1", n1), ("qkv", qkv), ("proj", pr), ("ls1", s1), ("norm2", n2), ("fc1", fc1), ("act", act), ("fc2", fc2),
                     ("ls2", s2), ("out", t)):
            f[f"{i}.{k}"] = v
    f["norm"] = layer_norm(t, p["norm.weight"], p["norm.bias"])
    f["cls"] = f["norm"][:, 0]
    return f


def loss(sd, xa, xb, heads, depth, dtype=torch.float64, per_image=False):
    fa, fb = features(sd, xa, heads, depth, dtype), features(sd, xb, heads, depth, dtype)
    B = xa.shape[0]
    total = torch.zeros(B, dtype=dtype)
    for key, m in tap_list(depth):
        d = fa[key] - fb[key]
        total = total + m * smooth_l1(d).reshape(B, -1).sum(1) / d.numel()
    return total if per_image else total.sum()


def loss_and_grad(sd, xa, xb, heads, depth, dtype=torch.float64):
    xa = xa.to(dtype).clone().requires_grad_(True)
    v = loss(sd, xa, xb, heads, depth, dtype)
    v.backward()
    return v.detach(), xa.grad.detach()


def tap_abs_differences(sd, xa, xb, heads, depth):
    """every |a - b| of every tap tensor (each tensor once), float64, one flat vector"""
    fa, fb = features(sd, xa, heads, depth), features(sd, xb, heads, depth)
    keys = []
    for key, _ in tap_list(depth):
        if key not in keys:
            keys.append(key)
    return torch.cat([(fa[k] - fb[k]).abs().reshape(-1) for k in keys])


def state_names(depth):
    names = ["cls_token", "pos_embed", "mask_token", "patch_embed.proj.weight", "patch_embed.proj.bias"]
    for i in range(depth):
        names += [f"blocks.{i}.{n}" for n in ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight",
                                              "attn.proj.bias", "ls1.gamma", "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias",
                                              "mlp.fc2.weight", "mlp.fc2.bias", "ls2.gamma")]
    return names + ["norm.weight", "norm.bias"]


def make_state(embed, depth, pos_grid, seed):
    """fp32 weights of a small trunk, scaled so that the features are O(1): dense weights 1 / sqrt(fan in), affine weights near 1"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    Cc = embed
    sd = {"cls_token": 0.5 * r(1, 1, Cc), "pos_embed": 0.5 * r(1, 1 + pos_grid ** 2, Cc), "mask_token": torch.zeros(1, Cc),
          "patch_embed.proj.weight": r(Cc, 3, PATCH, PATCH) / math.sqrt(588.0), "patch_embed.proj.bias": 0.1 * r(Cc)}
    for i in range(depth):
        q = f"blocks.{i}."
        for n, (o, k) in (("attn.qkv", (3 * Cc, Cc)), ("attn.proj", (Cc, Cc)), ("mlp.fc1", (4 * Cc, Cc)), ("mlp.fc2", (Cc, 4 * Cc))):
            sd[q + n + ".weight"] = r(o, k) / math.sqrt(k)
            sd[q + n + ".bias"] = 0.1 * r(o)
        for n in ("norm1", "norm2"):
            sd[q + n + ".weight"] = 1.0 + 0.1 * r(Cc)
            sd[q + n + ".bias"] = 0.1 * r(Cc)
        sd[q + "ls1.gamma"] = 0.5 + torch.rand(Cc, generator=g)
        sd[q + "ls2.gamma"] = 0.5 + torch.rand(Cc, generator=g)
    sd["norm.weight"], sd["norm.bias"] = 1.0 + 0.1 * r(Cc), 0.1 * r(Cc)
    return {k: sd[k].float() for k in state_names(depth)}


# (embed, heads, depth, H, W, pos grid, batch, seed): the seeds were searched on the CPU for the two conditions check_fixture states
FIXTURES = {
    "e32": dict(embed=32, heads=2, depth=2, H=32, W=46, pos_grid=5, B=2, seed=2),
    "e128": dict(embed=128, heads=2, depth=1, H=60, W=60, pos_grid=5, B=2, seed=15),
}
MARGIN = 2e-5


def fixture(name):
    c = FIXTURES[name]
    sd = make_state(c["embed"], c["depth"], c["pos_grid"], c["seed"])
    g = torch.Generator().manual_seed(1000 + c["seed"])
    xa = torch.randn(c["B"], 3, c["H"], c["W"], generator=g)
    xb = torch.randn(c["B"], 3, c["H"], c["W"], generator=g)
    return sd, xa, xb, c


def check_fixture(sd, xa, xb, c):
    """-> (share of tap elements in the quadratic branch, in the linear branch, the smallest | |a - b| - 1 |)"""
    d = tap_abs_differences(sd, xa, xb, c["heads"], c["depth"])
    quad = float((d < 1.0).double().mean())
    return quad, 1.0 - quad, float((d - 1.0).abs().min())
