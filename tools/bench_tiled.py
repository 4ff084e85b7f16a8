"""Whole DDIM steps of the image-conditioned sampler on an image larger than the model's training size: overlapping-window
sampling (``tile=``) against the untiled step, ALTERNATELY inside one process, engine clock and board power sampled beside each
timing (bench.ClockSampler).

    python tools/bench_tiled.py [--size 512] [--tile 256] [--overlap 32] [--tile-batch N] [--alternate 3] [--steps 3] [--warmup 1]
                                 [--solver ddim|dpmpp2m] [--spacing uniform|logsnr]

Default model (DynamicUNet ch=128, ch_mult=[1,2,2,2], num_res_blocks=2), batch 1, random-init weights, hipGraph replay.  With the
defaults the tiled step is 3x3 windows of 256x256 in one model evaluation at batch 9; the untiled step puts the middle attention
blocks at L = 4096 instead of 1024.  A third arm times the untiled 256x256 batch-1 step, the unit the tiled step is expected to
cost 9 of.  --solver dpmpp2m times the DPM-Solver++(2M) step in all three arms (--spacing: its time steps, logsnr by default; a
step's cost does not depend on them).  Prints one line per timing and one JSON summary line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import hdiff_amd  # noqa: E402,F401
import bench  # noqa: E402
from hdiff_amd.diffusion.Diffusion import GaussianDiffusionSampler, _StepPlan, _TiledStepPlan, logsnr_timesteps  # noqa: E402
from hdiff_amd.diffusion.Model import DynamicUNet  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--tile", type=int, default=256)
ap.add_argument("--overlap", type=int, default=32)
ap.add_argument("--tile-batch", type=int, default=None)
ap.add_argument("--ddim-step", type=int, default=100)
ap.add_argument("--alternate", type=int, default=3)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--solver", choices=["ddim", "dpmpp2m"], default="ddim")
ap.add_argument("--spacing", choices=["uniform", "logsnr"], default=None)
a = ap.parse_args()
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
torch.manual_seed(0)
model = DynamicUNet(T=1000, ch=128, ch_mult=[1, 2, 2, 2], num_res_blocks=2, dropout=0.0).eval().to(dev)
samp = GaussianDiffusionSampler(model, 1e-4, 0.02, 1000).to(dev)
g = torch.Generator().manual_seed(1)
spacing = a.spacing or ("logsnr" if a.solver == "dpmpp2m" else "uniform")
seq = tuple(logsnr_timesteps(samp.betas, a.ddim_step, shift=1)) if spacing == "logsnr" else None     # None: the reference's steps
arms = {}
with torch.no_grad():
    # the step plans keep their window / image plans alive; each is captured once
    tiled = _TiledStepPlan(samp, 1, a.size, a.size, dev, a.ddim_step, a.tile, a.overlap, a.tile_batch, a.solver, seq)
    arms[f"tiled {a.size} (tile {a.tile}, overlap {a.overlap}, {tiled.n_windows} windows, {len(tiled.chunks)} chunk(s))"] = \
        (tiled, tiled.y, tiled.cond, a.size)
    whole = _StepPlan(samp, 1, a.size, a.size, dev, a.ddim_step, solver=a.solver, seq=seq)
    arms[f"untiled {a.size}"] = (whole, whole.unet.y, whole.unet.cond, a.size)
    t = min(a.tile, a.size)
    unit = _StepPlan(samp, 1, t, t, dev, a.ddim_step, solver=a.solver, seq=seq)
    arms[f"untiled {t}"] = (unit, unit.unet.y, unit.unet.cond, t)
    for sp, _, _, _ in arms.values():
        sp.unet.plan.pack_weights()
        sp.plan.capture()
    times = {k: [] for k in arms}
    for rep in range(a.alternate):
        for name, (sp, y, cond, size) in arms.items():
            cond.copy_(torch.rand(1, 3, size, size, generator=g))
            y.copy_(torch.randn(1, 3, size, size, generator=g))
            sp.step.fill_(sp.n_steps - 1)
            sp.nan_flag.zero_()
            for _ in range(a.warmup):
                sp.plan.replay()
            torch.cuda.synchronize(dev)
            clock = bench.ClockSampler(0)
            with clock:
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    sp.plan.replay()
                torch.cuda.synchronize(dev)
                dt = (time.perf_counter() - t0) / a.steps
            assert int(sp.nan_flag.item()) == 0, "nan in tensor."
            c = clock.summary()
            times[name].append(dt * 1e3)
            print(f"step {name} rep {rep}: {dt * 1e3:.2f} ms  sclk {c.get('sclk_mhz_mean')} MHz  board {c.get('board_power_w_mean')} W",
                  flush=True)
summary = {k: {"ms_per_step_mean": sum(v) / len(v), "ms_per_step_min": min(v), "ms_per_step_max": max(v), "repetitions": len(v)}
           for k, v in times.items()}
plan_bytes = {k: v[0].unet.plan.bytes_allocated() for k, v in arms.items()}          # the buffers of the model plan of each arm
print(json.dumps({"metric": f"whole {a.solver} step of the image-conditioned sampler, batch 1, tiled against untiled, alternating "
                            "(hipGraph replay)", "unit": "ms/step", "arms": summary, "model_plan_bytes": plan_bytes}))
