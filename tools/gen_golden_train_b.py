"""TEST INFRASTRUCTURE ONLY -- golden vectors for the second tree's trainer (tests/golden/dyn_trainer_small.npz).

Run where the reference checkout is available (``oracle.reference_loader.REFERENCE_ROOT``):

    python tools/gen_golden_train_b.py

The model is the REAL reference ``DynamicUNet`` (``oracle.reference_loader.load_model_b``), built with the seed recipe of
tests/golden/dyn_unet_small.npz (small config, seed 4242, the two tail edits, the stored sinusoidal table), B = 2, dropout 0.
The colour term is the reference's own ``angular_color_loss`` class, compiled at run time from the text of Loss/loss.py where it
lies (the file's imports need torchvision / kornia, so it cannot be imported whole); nothing of it is copied here.  The trainer
arithmetic around the two (reference diffusion/Diffusion.py:45-180: input scaling, q_sample, the model call, mse, y_0_pred with
its trailing / 255, the weighted terms) is written out below.  The DINO and MS-SSIM terms are pinned with the plain-torch
stand-ins ``dino_standin`` / ``msssim_standin``, which the tests pass to the package's trainer as well.

Stored (per case): the five returned terms, and for every parameter its gradient at fixed sample positions (SAMPLE_RULE) with the
gradient's absolute maximum, or the fact that it is None.  Trajectory: three clip(1.0) + torch.optim.AdamW(weight_decay=1e-4)
steps alternating the two pairs, so that middle blocks freeze and thaw; parameters (sampled) and the total norm after each step.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import reference_loader as RL  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
N_SAMPLES = 64
BETA = (1e-4, 0.02)
B, S = 2, 16
CASES = [("uw", True), ("uw", False), ("atm", True), ("atm", False)]
TRAJ = [("uw", False), ("atm", True), ("uw", False)]
LR, WD = 1e-4, 1e-4


def sample_idx(numel: int) -> np.ndarray:
    """SAMPLE_RULE: up to N_SAMPLES evenly spaced flat positions (the tests use the same rule)."""
    return np.unique(np.linspace(0, numel - 1, min(numel, N_SAMPLES)).round().astype(np.int64))


def dino_standin(y0, gt):
    """Differentiable stand-in for the DINOv2 perceptual term (the same callable is passed to the package's trainer)."""
    return (y0 * gt).mean() * 40.0


def msssim_standin(y0, gt):
    return ((y0 * 255.0 - gt) ** 2).mean() * 0.1


def load_angular_color_loss():
    path = os.path.join(RL.REFERENCE_ROOT, "Loss", "loss.py")
    with open(path) as fh:
        lines = fh.readlines()
    a = next(i for i, l in enumerate(lines) if l.startswith("class angular_color_loss"))
    b = next(i for i in range(a + 1, len(lines)) if lines[i].startswith("class "))
    kept = ["\n"] * len(lines)
    kept[a:b] = lines[a:b]
    ns = {"torch": torch, "nn": nn, "F": F}
    exec(compile("".join(kept), path, "exec"), ns)
    return ns["angular_color_loss"]()


def pair(kind: str, g: torch.Generator):
    """(gt, input) uint8-valued float images: 'uw' has a blue cast (blue mean > red), 'atm' a red / haze cast."""
    gt = torch.randint(0, 256, (B, 3, S, S), generator=g).float()
    inp = torch.randint(0, 200, (B, 3, S, S), generator=g).float()
    if kind == "uw":
        inp[:, 0] *= 0.3
        inp[:, 2] = inp[:, 2] * 0.5 + 100
    else:
        inp[:, 2] *= 0.3
        inp[:, 0] = inp[:, 0] * 0.5 + 100
    return gt, inp


def small_model(RMB):
    d = np.load(os.path.join(GOLDEN, "dyn_unet_small.npz"))
    cfg = json.loads(bytes(d["cfg_json"]).decode())
    torch.manual_seed(int(d["seed"][0]))
    m = RMB.DynamicUNet(**cfg)
    with torch.no_grad():
        m.tail[2].weight.mul_(float(d["tail_gain"][0]))
        m.tail[2].bias.add_(float(d["tail_bias_add"][0]))
        m.time_embedding.timembedding[0].weight.copy_(torch.from_numpy(d["temb_table"]))
    return m.train(), cfg


def extract(v, t, x_shape):
    out = torch.gather(v, index=t, dim=0).float()
    return out.view([t.shape[0]] + [1] * (len(x_shape) - 1))


def trainer_forward(model, sab, s1mab, color, gt_images, input_image, t, noise, context_zero):
    input_image = (input_image.float() / 255.0) * 2 - 1
    gt_images = (gt_images.float() / 255.0) * 2 - 1
    y_t = extract(sab, t, gt_images.shape) * gt_images + extract(s1mab, t, gt_images.shape) * noise
    x = torch.cat([input_image, y_t], dim=1).float()
    noise_pred = model(x, t, gt_images, context_zero=context_zero)
    loss = 0
    mse_loss = F.mse_loss(noise_pred, noise, reduction="none")
    loss += mse_loss
    y_0_pred = 1 / extract(sab, t, gt_images.shape) * (y_t - extract(s1mab, t, gt_images.shape) * noise_pred).float() / 255.0
    perceptual_dino = dino_standin(y_0_pred, gt_images) * 0.5
    loss += perceptual_dino
    msssim = msssim_standin(y_0_pred, gt_images) * 0.0045
    loss += msssim
    col_loss = color(y_0_pred, gt_images) * 1.0
    loss += col_loss
    return [loss, mse_loss, perceptual_dino, msssim, col_loss]


def _f32(t):
    return t.detach().float().contiguous().numpy()


def param_names(model):
    return [name for name, _ in model.named_parameters()]


def grads_of(model, prefix, out):
    """{prefix}/grad_samples: the sampled gradients of all parameters, concatenated in named_parameters() order (a None
    gradient contributes NaNs); {prefix}/gradmax: max |grad| per parameter (NaN = None)."""
    samples, gmax = [], []
    for _, p in model.named_parameters():
        n = len(sample_idx(p.numel()))
        if p.grad is None:
            samples.append(np.full(n, np.nan, dtype=np.float32))
            gmax.append(np.nan)
            continue
        g = p.grad.detach().reshape(-1)
        samples.append(_f32(g[torch.from_numpy(sample_idx(g.numel()))]))
        gmax.append(g.abs().max().item())
    out[f"{prefix}/grad_samples"] = np.concatenate(samples)
    out[f"{prefix}/gradmax"] = np.array(gmax, dtype=np.float32)


def main():
    torch.set_num_threads(8)
    RMB = RL.load_model_b()
    color = load_angular_color_loss()
    betas = torch.linspace(BETA[0], BETA[1], 1000).double()
    ab = torch.cumprod(1. - betas, dim=0)
    sab, s1mab = torch.sqrt(ab), torch.sqrt(1. - ab)
    g = torch.Generator().manual_seed(2024)
    data = {}
    for kind in ("uw", "atm"):
        gt, inp = pair(kind, g)
        data[kind] = (gt, inp, torch.randint(0, 1000, (B,), generator=g), torch.randn(B, 3, S, S, generator=g))
    out = {"beta": np.array(BETA), "n_samples": np.array([N_SAMPLES]), "lr_wd": np.array([LR, WD])}
    for kind, (gt, inp, t, noise) in data.items():
        out[f"{kind}/gt"], out[f"{kind}/input"], out[f"{kind}/t"], out[f"{kind}/noise"] = _f32(gt), _f32(inp), t.numpy(), _f32(noise)
    for kind, cz in CASES:
        m, _ = small_model(RMB)
        gt, inp, t, noise = data[kind]
        terms = trainer_forward(m, sab, s1mab, color, gt, inp, t, noise, cz)
        terms[0].mean().backward()
        tag = f"case/{kind}_cz{int(cz)}"
        for nm, v in zip(("loss", "mse_loss", "perceptual_dino", "msssim", "col_loss"), terms):
            out[f"{tag}/{nm}"] = _f32(v)
        grads_of(m, tag, out)
        print(tag, "loss mean", terms[0].mean().item(), "col", terms[4].item(), "frozen", int(np.isnan(out[f"{tag}/gradmax"]).sum()))
    m, _ = small_model(RMB)
    out["param_names"] = np.array(param_names(m))
    opt = torch.optim.AdamW(m.parameters(), lr=LR, weight_decay=WD)
    for k, (kind, cz) in enumerate(TRAJ):
        gt, inp, t, noise = data[kind]
        opt.zero_grad()
        loss = trainer_forward(m, sab, s1mab, color, gt, inp, t, noise, cz)[0]
        loss.mean().backward()
        total = torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
        opt.step()
        out[f"traj/{k}/loss_mean"] = np.array([loss.mean().item()])
        out[f"traj/{k}/total_norm"] = np.array([total.item()])
        out[f"traj/{k}/param_samples"] = np.concatenate([_f32(p.detach().reshape(-1)[torch.from_numpy(sample_idx(p.numel()))])
                                                         for p in m.parameters()])
        print("traj step", k, kind, "loss", loss.mean().item(), "norm", total.item())
    path = os.path.join(GOLDEN, "dyn_trainer_small.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
