"""Time of ONE WHOLE `GaussianDiffusionSampler.forward` of the label-conditioned tree (bench.py's model and guidance weight): the
T-step ancestral loop against the strided DDIM sampler, ALTERNATELY inside one process, engine clock and board power sampled beside
each timing (bench.ClockSampler).

    python tools/bench_sample_a.py [--ddim-steps 50] [--eta 0] [--T 1000] [--size 256] [--batch 8] [--contract bf16x3|f32|f16]
                                   [--alternate 2] [--no-ancestral] [--solver ddim|dpmpp2m|both] [--spacing uniform|logsnr]

One call = everything a user waits for: weight pack, loop state reset, S (or T) graph replays, the NaN check and the final clip;
--solver chooses the update of the strided arm (dpmpp2m: DPM-Solver++(2M); both: one arm each, alternating), --spacing its time steps
(default: the solver's own).  The first call of each arm (plan build + graph capture) is printed as a warm-up and not counted.  --T is the length of the sampler's
schedule, i.e. the number of steps of the ancestral arm (the model keeps bench.py's T = 1000 embedding table; a shorter schedule
makes the ancestral arm affordable, its time per step is the same).  Prints one line per timing and one JSON summary line."""
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
from hdiff_amd.DiffusionFreeGuidence.DiffusionCondition import GaussianDiffusionSampler, ddim_timesteps  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ddim-steps", type=int, default=50)
ap.add_argument("--eta", type=float, default=0.0)
ap.add_argument("--T", type=int, default=bench.MODEL["T"])
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--contract", choices=["f32", "bf16x3", "f16"], default="bf16x3")
ap.add_argument("--alternate", type=int, default=2)
ap.add_argument("--no-ancestral", action="store_true", help="time the strided arm(s) alone")
ap.add_argument("--solver", choices=["ddim", "dpmpp2m", "both"], default="ddim")
ap.add_argument("--spacing", choices=["uniform", "logsnr"], default=None)
a = ap.parse_args()
assert 1 <= a.T <= bench.MODEL["T"], "--T cannot exceed the model's time-embedding table"
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
before = hdiff_amd.get_contraction_mode()
hdiff_amd.set_contraction_mode(a.contract)
model = bench._model(bench.MODEL, dev)
g = torch.Generator().manual_seed(1234)
x_T = torch.randn(a.batch, 3, a.size, a.size, generator=g).to(dev)
labels = (torch.arange(a.batch) % 2 + 1).to(dev)
# one sampler per arm: each keeps its own captured step alive (a sampler holds ONE live variant), the UNet plan is the model's
arms = {}
if not a.no_ancestral:
    arms["ancestral"] = (GaussianDiffusionSampler(model, *bench.BETA, a.T, w=bench.GUIDANCE_W).to(dev), {}, a.T)
for solver in (("ddim", "dpmpp2m") if a.solver == "both" else (a.solver,)):
    kw = dict(ddim_steps=a.ddim_steps, eta=a.eta if solver == "ddim" else 0.0)            # dpmpp2m is deterministic
    if solver != "ddim" or a.spacing is not None:                                         # the plain DDIM arm is called as before
        kw.update(solver=solver, spacing=a.spacing)
    arms[f"{solver}{a.ddim_steps}"] = (GaussianDiffusionSampler(model, *bench.BETA, a.T, w=bench.GUIDANCE_W).to(dev), kw,
                                       len(ddim_timesteps(a.T, a.ddim_steps)))
times = {name: [] for name in arms}
clocks = {name: [] for name in arms}
try:
    with torch.no_grad():
        torch.manual_seed(0)
        for rep in range(a.alternate + 1):                        # repetition 0 is the warm-up: plan build and graph capture, not counted
            for name, (sampler, kw, steps) in arms.items():
                torch.cuda.synchronize(dev)
                clock = bench.ClockSampler(0)
                with clock:
                    t0 = time.perf_counter()
                    out = sampler(x_T, labels, **kw)
                    torch.cuda.synchronize(dev)
                    dt = time.perf_counter() - t0
                assert torch.isfinite(out).all()
                c = clock.summary()
                tag = "warm-up (includes the graph capture)" if rep == 0 else f"rep {rep}"
                print(f"{name:10s} {a.size}x{a.size} batch {a.batch} {a.contract} {tag}: {dt:.3f} s/batch  {steps} steps  "
                      f"{dt / steps * 1e3:.2f} ms/step  {a.batch / dt:.3f} images/s  sclk {c.get('sclk_mhz_mean')} MHz  "
                      f"board {c.get('board_power_w_mean')} W", flush=True)
                if rep > 0:
                    times[name].append(dt)
                    clocks[name].append((c.get("sclk_mhz_mean"), c.get("board_power_w_mean")))
finally:
    hdiff_amd.set_contraction_mode(before)
summary = {}
for name, (sampler, kw, steps) in arms.items():
    t = times[name]
    if t:
        mean = sum(t) / len(t)
        summary[name] = {"steps": steps, "s_per_batch_mean": mean, "s_per_batch_min": min(t), "s_per_batch_max": max(t),
                         "ms_per_step_mean": mean / steps * 1e3, "images_per_s": a.batch / mean, "repetitions": len(t),
                         "sclk_mhz_board_w": clocks[name]}
print(json.dumps({"metric": f"whole sampler forward, {'' if a.no_ancestral else 'ancestral against '}strided {' and '.join(n for n in arms if n != 'ancestral')}, alternating ({a.size}x{a.size}, batch {a.batch}, "
                            f"schedule T = {a.T}, {a.contract}, hipGraph replay)", "unit": "s/batch", "eta": a.eta, "spacing": a.spacing, "arms": summary}))
