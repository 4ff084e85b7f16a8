"""The tree-A sampler step (bench.py's headline workload: 256x256, batch 8, hipGraph replay) in the contraction modes, ALTERNATELY
inside one process, engine clock and board power sampled beside each timing (bench.ClockSampler).

    python tools/bench_modes.py [--contract f32,bf16x3,f16] [--alternate 3] [--steps 3] [--warmup 1] [--size 256] [--batch 8]

One captured step per mode (a graph bakes the mode it was captured in); the arms are timed in turn --alternate times.  Prints one
line per timing and one JSON summary line.  bench.py's headline stays the default mode; this tool is the comparison."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import hdiff_amd  # noqa: E402
import bench  # noqa: E402
from hdiff_amd.DiffusionFreeGuidence.DiffusionCondition import GaussianDiffusionSampler, _SamplerPlan  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--contract", default="f32,bf16x3,f16")
ap.add_argument("--alternate", type=int, default=3)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--batch", type=int, default=8)
a = ap.parse_args()
modes = a.contract.split(",")
assert all(m in ("f32", "bf16x3", "f16") for m in modes), modes
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
before = hdiff_amd.get_contraction_mode()
model = bench._model(bench.MODEL, dev)
g = torch.Generator().manual_seed(1234)
x_T = torch.randn(a.batch, 3, a.size, a.size, generator=g).to(dev)
labels = (torch.arange(a.batch) % 2 + 1).to(dev)
arms = {}
with torch.no_grad():
    for m in modes:          # one sampler, one captured step per mode: the UNet plan (buffers, packed weights) is shared
        hdiff_amd.set_contraction_mode(m)
        sampler = GaussianDiffusionSampler(model, bench.BETA[0], bench.BETA[1], bench.MODEL["T"], w=bench.GUIDANCE_W).to(dev)
        sp = _SamplerPlan(sampler, a.batch, a.size, a.size, dev)
        plan = sp.variant(False, 1234)
        sp.unet.plan.pack_weights()
        plan.capture()
        arms[m] = (sampler, sp, plan)
    times = {m: [] for m in modes}
    for rep in range(a.alternate):
        for m in modes:
            hdiff_amd.set_contraction_mode(m)
            _, sp, plan = arms[m]
            sp.reset(x_T, labels)
            for _ in range(a.warmup):
                plan.replay()
            torch.cuda.synchronize(dev)
            clock = bench.ClockSampler(0)
            with clock:
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    plan.replay()
                torch.cuda.synchronize(dev)
                dt = (time.perf_counter() - t0) / a.steps
            assert int(sp.nan_flag.item()) == 0, "nan in tensor."
            c = clock.summary()
            times[m].append(dt * 1e3)
            print(f"step {m:6s} {a.size}x{a.size} batch {a.batch} rep {rep}: {dt * 1e3:.2f} ms  {1.0 / dt:.3f} steps/s  "
                  f"sclk {c.get('sclk_mhz_mean')} MHz  board {c.get('board_power_w_mean')} W", flush=True)
hdiff_amd.set_contraction_mode(before)
summary = {m: {"ms_per_step_mean": sum(t) / len(t), "ms_per_step_min": min(t), "ms_per_step_max": max(t), "repetitions": len(t)}
           for m, t in times.items()}
print(json.dumps({"metric": f"denoising step in the contraction modes, alternating ({a.size}x{a.size}, batch {a.batch}, hipGraph replay)",
                  "unit": "ms/step", "modes": summary}))
