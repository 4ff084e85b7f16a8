"""Bench tool: the VGG perceptual loss (forward + backward through ``Loss.loss.PerceptualLoss_vgg``) and one ``quality.LPIPS`` call on
the HIP path, each against the same trunk written in plain torch ops (``F.conv2d`` / ``relu`` / ``max_pool2d`` / ``l1_loss``, fp32, same
GPU, same random weights).  The two arms alternate in one process: ``--alternate K`` rounds, in each round ``--reps`` timed calls of the
one arm and then of the other, every block under its own clock / power sampler.  A figure is the median over all timed calls of its
arm, with the engine clock and board power sampled while that arm ran.

  python tools/bench_perceptual.py --alternate 3 [--size 256] [--loss-batch 2 16] [--lpips-batch 8] [--reps 5]

The torch arm is the yardstick, not the code under test.  No time here is a gate: there is no earlier number to hold.  One JSON line
per measurement."""
import argparse, json, os, sys, warnings
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

ap = argparse.ArgumentParser()
ap.add_argument("--alternate", type=int, default=3); ap.add_argument("--size", type=int, default=256)
ap.add_argument("--loss-batch", type=int, nargs="+", default=[2, 16]); ap.add_argument("--lpips-batch", type=int, nargs="+", default=[8])
ap.add_argument("--reps", type=int, default=5); ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--mode", default=None, help="contraction mode (default: the library's)")
a = ap.parse_args()
if a.alternate < 1 or a.reps < 1:
    sys.exit("bench_perceptual.py: --alternate and --reps must be at least 1")
if not torch.cuda.is_available():
    sys.exit("bench_perceptual.py needs an MI355X (there is no CPU path to time)")

import hdiff_amd  # noqa: E402
from bench import ClockSampler  # noqa: E402
from hdiff_amd import perceptual, quality  # noqa: E402
from hdiff_amd.Loss.loss import PerceptualLoss_vgg  # noqa: E402

if a.mode:
    hdiff_amd.set_contraction_mode(a.mode)
dev = torch.device("cuda", 0)
torch.manual_seed(0)
with warnings.catch_warnings():
    warnings.simplefilter("ignore")                        # random weights on purpose: the timing does not depend on them
    native_loss = PerceptualLoss_vgg(model="vgg16").to(dev)
trunk = native_loss.perceptual
layers = trunk.layers
params = {i: (getattr(trunk, str(i)).weight, getattr(trunk, str(i)).bias) for i in trunk.conv_indices()}
lin = [torch.rand(1, c, 1, 1) * 2 / c for c in quality.LPIPS.CHANNELS]
native_lpips = quality.LPIPS(trunk, lin).to(dev)
lin_dev = [w.to(dev) for w in lin]
SHIFT = torch.tensor(quality.LPIPS.SHIFT, device=dev).view(1, 3, 1, 1)
SCALE = torch.tensor(quality.LPIPS.SCALE, device=dev).view(1, 3, 1, 1)


def torch_trunk(x, taps):
    out = []
    for i, layer in enumerate(layers[:max(taps) + 1]):
        if layer[0] == "conv":
            x = F.conv2d(x, params[i][0], params[i][1], padding=1)
        elif layer[0] == "relu":
            x = F.relu(x)
        else:
            x = F.max_pool2d(x, 2, 2)
        if i in taps:
            out.append(x)
    return out


def torch_loss(x, y):
    taps = native_loss.layer_indices["vgg16"]
    fx = torch_trunk(x, taps)
    with torch.no_grad():
        fy = torch_trunk(y, taps)
    return sum(F.l1_loss(u, v) for u, v in zip(fx, fy))


def torch_lpips(a01, b01):
    with torch.no_grad():
        f0 = torch_trunk(((a01 * 2 - 1) - SHIFT) / SCALE, quality.LPIPS.TAPS)
        f1 = torch_trunk(((b01 * 2 - 1) - SHIFT) / SCALE, quality.LPIPS.TAPS)
        total = 0
        for u, v, w in zip(f0, f1, lin_dev):
            nu = u / (u.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10)
            nv = v / (v.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10)
            total = total + (w * (nu - nv) ** 2).sum(dim=1).mean(dim=(1, 2))
    return total


def loss_once(fn, x, y):
    x = x.detach().requires_grad_(True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    loss = fn(x, y)
    loss.backward()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1), loss.detach(), x.grad


def lpips_once(fn, x, y):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn(x, y)
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1), out, None


def measure(what, once, arms, x, y, B):
    last = {}
    for _ in range(a.warmup):
        for name, fn in arms:
            last[name] = once(fn, x, y)
    times = {name: [] for name, _ in arms}
    clocks = {name: [] for name, _ in arms}
    for _ in range(a.alternate):
        for name, fn in arms:
            clock = ClockSampler(0)
            with clock:
                for _ in range(a.reps):
                    times[name].append(once(fn, x, y)[0])
            clocks[name].append(clock.summary())
    line = {"what": what, "size": a.size, "batch": B, "alternate": a.alternate, "reps": a.reps,
            "mode": hdiff_amd.get_contraction_mode(), "gpu": torch.cuda.get_device_name(dev)}
    for name, _ in arms:
        t = sorted(times[name])
        mhz = [c["sclk_mhz_mean"] for c in clocks[name] if c.get("sclk_mhz_mean") is not None]
        watts = [c["board_power_w_mean"] for c in clocks[name] if c.get("board_power_w_mean") is not None]
        line[f"{name}_ms_median"], line[f"{name}_ms_min"] = round(t[len(t) // 2], 4), round(t[0], 4)
        line[f"{name}_sclk_mhz_mean"] = round(sum(mhz) / len(mhz), 1) if mhz else None
        line[f"{name}_board_power_w_mean"] = round(sum(watts) / len(watts), 1) if watts else None
    line["torch_over_native_median"] = round(line["torch_ms_median"] / line["native_ms_median"], 2)
    vn, vt = last["native"][1].double(), last["torch"][1].double()
    line["value_rel_diff"] = float(((vn - vt).abs() / vt.abs()).max())
    if last["native"][2] is not None:
        gn, gt = last["native"][2], last["torch"][2]
        line["grad_rel_l2_diff"] = float((gn - gt).norm() / gt.norm())
    print(json.dumps(line), flush=True)


g = torch.Generator().manual_seed(7)
for B in a.loss_batch:
    x = (torch.rand(B, 3, a.size, a.size, generator=g) * 2 - 1).to(dev)
    y = (x + 0.3 * torch.randn(B, 3, a.size, a.size, generator=g).to(dev)).clamp(-1, 1)
    measure("PerceptualLoss_vgg vgg16 fwd+bwd", loss_once, (("native", native_loss), ("torch", torch_loss)), x, y, B)
    del x, y
    torch.cuda.empty_cache()
for B in a.lpips_batch:
    x = torch.rand(B, 3, a.size, a.size, generator=g).to(dev)
    y = (x + 0.2 * torch.randn(B, 3, a.size, a.size, generator=g).to(dev)).clamp(0, 1)
    measure("LPIPS vgg16", lpips_once, (("native", native_lpips.metric), ("torch", torch_lpips)), x, y, B)
