"""Bench tool: the DINOv2 perceptual loss (forward + backward through ``Loss.loss.PerceptualLoss_dino``, ``dinov2_vits14``, random
weights) on the HIP path against the same trunk and the same taps written in plain torch ops (``F.conv2d`` / ``layer_norm`` / ``linear`` /
``scaled_dot_product_attention`` / ``gelu`` / ``smooth_l1_loss``, fp32, same GPU, same weights).  The two arms alternate in one process:
``--alternate K`` rounds, in each round ``--reps`` timed calls of the one arm and then of the other, every block under its own clock /
power sampler.  A figure is the median over all timed calls of its arm, with the engine clock and board power sampled while that
arm ran.

  python tools/bench_dino.py --alternate 3 [--size 256] [--batch 2 16] [--reps 5] [--model dinov2_vits14] [--dense conv tokens]

``--dense`` names the dense-layer routes of the trunk (``dino.dense_route``) to time as arms of their own beside the torch arm, on one set
of weights: the arms are then called ``conv`` / ``tokens`` instead of ``native``, every arm reports its fastest, median and slowest call
and the median of each round, and ``a_over_b_median`` compares each pair.

The torch arm is the yardstick, not the code under test.  No time here is a gate: there is no earlier number to hold.  One JSON line
per measurement."""
import argparse, json, os, sys, warnings
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

ap = argparse.ArgumentParser()
ap.add_argument("--alternate", type=int, default=3); ap.add_argument("--size", type=int, default=256)
ap.add_argument("--batch", type=int, nargs="+", default=[2, 16]); ap.add_argument("--model", default="dinov2_vits14")
ap.add_argument("--reps", type=int, default=5); ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--mode", default=None, help="contraction mode (default: the library's)")
ap.add_argument("--dense", nargs="+", default=None, choices=["conv", "tokens"], help="dense-layer routes to time as separate arms")
a = ap.parse_args()
if a.alternate < 1 or a.reps < 1:
    sys.exit("bench_dino.py: --alternate and --reps must be at least 1")
if not torch.cuda.is_available():
    sys.exit("bench_dino.py needs an MI355X (there is no CPU path to time)")

import hdiff_amd  # noqa: E402
from bench import ClockSampler  # noqa: E402
from hdiff_amd import dino  # noqa: E402
from hdiff_amd.Loss.loss import PerceptualLoss_dino  # noqa: E402

if a.mode:
    hdiff_amd.set_contraction_mode(a.mode)
dev = torch.device("cuda", 0)
torch.manual_seed(0)
with warnings.catch_warnings():
    warnings.simplefilter("ignore")                        # random weights on purpose: the timing does not depend on them
    native_loss = PerceptualLoss_dino(a.model).to(dev)
    trunk = native_loss.perceptual
    trunk._warned_random = True
P = dict(trunk.named_parameters())
HEADS, DEPTH, C = trunk.heads, trunk.depth, trunk.embed_dim
TAPS = [(key, m) for _, key, m in native_loss.taps]
NATIVE = [("native", native_loss)]
if a.dense:
    NATIVE = []
    state = {k: v.detach().cpu() for k, v in trunk.state_dict().items()}
    for choice in dict.fromkeys(a.dense):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            arm = PerceptualLoss_dino(a.model, dense=choice)
            arm.perceptual.load_dinov2(state)
        NATIVE.append((choice, arm.to(dev)))


def torch_features(x):
    x = x[:, :, 2:x.shape[2] - 2, 2:x.shape[3] - 2]
    h, w = x.shape[2] // 14, x.shape[3] // 14
    f = {}
    t = F.conv2d(x, P["patch_embed.proj.weight"], P["patch_embed.proj.bias"], stride=14).flatten(2).transpose(1, 2)
    f["patch"] = t
    pos = trunk._pos(h, w, dev).t().unsqueeze(0)           # the same resized embedding, token-major
    t = torch.cat([P["cls_token"].expand(t.shape[0], -1, -1), t], dim=1) + pos
    for i in range(DEPTH):
        q = f"blocks.{i}."
        n1 = F.layer_norm(t, (C,), P[q + "norm1.weight"], P[q + "norm1.bias"], 1e-6)
        qkv = F.linear(n1, P[q + "attn.qkv.weight"], P[q + "attn.qkv.bias"])
        B, N, _ = qkv.shape
        qq, kk, vv = qkv.reshape(B, N, 3, HEADS, C // HEADS).permute(2, 0, 3, 1, 4)
        o = F.scaled_dot_product_attention(qq, kk, vv).transpose(1, 2).reshape(B, N, C)
        pr = F.linear(o, P[q + "attn.proj.weight"], P[q + "attn.proj.bias"])
        s1 = P[q + "ls1.gamma"] * pr
        t1 = t + s1
        n2 = F.layer_norm(t1, (C,), P[q + "norm2.weight"], P[q + "norm2.bias"], 1e-6)
        fc1 = F.linear(n2, P[q + "mlp.fc1.weight"], P[q + "mlp.fc1.bias"])
        act = F.gelu(fc1)
        fc2 = F.linear(act, P[q + "mlp.fc2.weight"], P[q + "mlp.fc2.bias"])
        s2 = P[q + "ls2.gamma"] * fc2
        t = t1 + s2
        for k, v in (("norm1", n1), ("qkv", qkv), ("proj", pr), ("ls1", s1), ("norm2", n2), ("fc1", fc1), ("act", act), ("fc2", fc2),
                     ("ls2", s2), ("out", t)):
            f[f"{i}.{k}"] = v
    f["norm"] = F.layer_norm(t, (C,), P["norm.weight"], P["norm.bias"], 1e-6)
    f["cls"] = f["norm"][:, 0]
    return f


def torch_loss(x, y):
    fx = torch_features(x)
    with torch.no_grad():
        fy = torch_features(y)
    return sum(m * F.smooth_l1_loss(fx[k], fy[k]) for k, m in TAPS)


def once(fn, x, y):
    x = x.detach().requires_grad_(True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    loss = fn(x, y)
    loss.backward()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1), loss.detach(), x.grad


def measure(what, arms, x, y, B):
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
    line = {"what": what, "size": a.size, "batch": B, "alternate": a.alternate, "reps": a.reps, "taps": len(TAPS),
            "mode": hdiff_amd.get_contraction_mode(), "gpu": torch.cuda.get_device_name(dev)}
    for name, _ in arms:
        t = sorted(times[name])
        mhz = [c["sclk_mhz_mean"] for c in clocks[name] if c.get("sclk_mhz_mean") is not None]
        watts = [c["board_power_w_mean"] for c in clocks[name] if c.get("board_power_w_mean") is not None]
        line[f"{name}_ms_median"], line[f"{name}_ms_min"] = round(t[len(t) // 2], 4), round(t[0], 4)
        if a.dense:
            line[f"{name}_ms_max"] = round(t[-1], 4)
            rounds = [sorted(times[name][i * a.reps:(i + 1) * a.reps]) for i in range(a.alternate)]
            line[f"{name}_ms_round_medians"] = [round(r[len(r) // 2], 4) for r in rounds]
        line[f"{name}_sclk_mhz_mean"] = round(sum(mhz) / len(mhz), 1) if mhz else None
        line[f"{name}_board_power_w_mean"] = round(sum(watts) / len(watts), 1) if watts else None
    names = [name for name, _ in arms]
    for i, over in enumerate(names):
        for under in names[:i]:
            line[f"{over}_over_{under}_median"] = round(line[f"{over}_ms_median"] / line[f"{under}_ms_median"], 2)
    vt, gt = last["torch"][1].double(), last["torch"][2]
    for name in names[:-1]:
        tag = "" if name == "native" else f"{name}_"
        line[f"{tag}value_rel_diff"] = float(((last[name][1].double() - vt).abs() / vt.abs()).max())
        line[f"{tag}grad_rel_l2_diff"] = float((last[name][2] - gt).norm() / gt.norm())
    print(json.dumps(line), flush=True)


g = torch.Generator().manual_seed(7)
for B in a.batch:
    # the trainer's ranges: the prediction as y_0_pred / 255, the target in [-1, 1]
    x = (torch.rand(B, 3, a.size, a.size, generator=g) / 255.0).to(dev)
    y = (torch.rand(B, 3, a.size, a.size, generator=g) * 2 - 1).to(dev)
    measure(f"PerceptualLoss_dino {a.model} fwd+bwd", tuple(NATIVE) + (("torch", torch_loss),), x, y, B)
    del x, y
    torch.cuda.empty_cache()
