"""Bench tool: forward + backward of the native MS-SSIM + L1 loss (csrc/msssim.hip) against a torch composite of the same definition
(tests/_msssim_def.py dense_loss: grouped 33x33 convolutions, fp32, on the same GPU).  The two alternate in one process; each
figure is the median of --reps timed calls after --warmup calls of both, with the engine clock sampled over the timed loop.

  python tools/bench_msssim.py --size 256 --batch 2 8 [--reps 20]

The composite is the yardstick, not the code under test; the native path must be the faster of the two.  One JSON line per batch."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=256); ap.add_argument("--batch", type=int, nargs="+", default=[2, 8])
ap.add_argument("--reps", type=int, default=20); ap.add_argument("--warmup", type=int, default=3)
a = ap.parse_args()
if a.reps < 10:
    sys.exit("bench_msssim.py: --reps must be at least 10 (the figure is a median)")
if not torch.cuda.is_available():
    sys.exit("bench_msssim.py needs an MI355X (there is no CPU path to time)")

import _msssim_def as D  # noqa: E402
from bench import ClockSampler  # noqa: E402
from hdiff_amd.Loss.loss import MSSSIMLoss  # noqa: E402

dev = torch.device("cuda", 0)
native, composite = MSSSIMLoss(), D.dense_loss          # both the kornia layout, the trainer's


def once(fn, x, y):
    """-> (ms of loss + backward by device events, loss, gradient)"""
    x = x.detach().requires_grad_(True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    loss = fn(x, y)
    loss.backward()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1), loss.detach(), x.grad


for B in a.batch:
    x, y = (t.to(dev) for t in D.image_like_pair(B, a.size, a.size, 7))
    for _ in range(a.warmup):
        _, ln, gn = once(native, x, y)
        _, lc, gc = once(composite, x, y)
    tn, tc = [], []
    clock = ClockSampler(0)
    with clock:
        for _ in range(a.reps):              # alternating: both see the same clock and the same neighbours
            tn.append(once(native, x, y)[0])
            tc.append(once(composite, x, y)[0])
    tn.sort(); tc.sort()
    c = clock.summary()
    print(json.dumps({"what": "msssim_l1 fwd+bwd", "layout": "kornia", "size": a.size, "batch": B, "reps": a.reps,
                      "native_ms_median": round(tn[len(tn) // 2], 4), "native_ms_min": round(tn[0], 4),
                      "composite_ms_median": round(tc[len(tc) // 2], 4), "composite_ms_min": round(tc[0], 4),
                      "speedup_median": round(tc[len(tc) // 2] / tn[len(tn) // 2], 2),
                      "loss_rel_diff": abs(float(ln) - float(lc)) / abs(float(lc)),
                      "grad_rel_diff": float((gn - gc).abs().max() / gc.abs().max()),
                      "sclk_mhz_mean": c.get("sclk_mhz_mean"), "sclk_mhz_min": c.get("sclk_mhz_min"),
                      "gpu": torch.cuda.get_device_name(dev)}), flush=True)
