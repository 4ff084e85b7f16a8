"""Does train -> sample -> score learn anything?  One small run from clean images alone, with nothing read from disk.

Procedural scenes at 64 x 64 (``synth.procedural_scenes``) are the clean targets; their degraded inputs are drawn on the device by
``Synth.underwater()`` behind ``DeviceLoader`` (``hdiff_amd/synth.py``).  A small ``DynamicUNet`` is trained with
``GaussianDiffusionTrainer`` (squared error, native MS-SSIM and colour terms), ``optim.AdamW`` and ``optim.EMA``.  At a few points of
the run the averaged weights sample a HELD-OUT set of scenes -- degraded once, under a fixed key -- with 20 DDIM steps through
``Evaluate.evaluate(..., color=True)``, and the scores of the output against the clean target stand beside those of the degraded
input against the same target: PSNR, SSIM and CIEDE2000.

The trainer is called by keyword, ``trainer(gt_images=clean, input_image=degraded, stage)``: the clean image is diffused and the
degraded one conditions the network, which is what the sampler assumes.  (``Train.train`` keeps the reference loop's positional call.)

    python tools/train_synth_demo.py [--steps 2000] [--batch 16] [--scenes 256] [--held 32] [--evals 4] [--max-seconds 240]
                                     [--prediction eps|v] [--solver ddim|dpmpp2m] [--out profiles/synth_demo.txt]

No outcome is asserted: the figures are the result, and they describe procedural scenes under a recalled coefficient table only."""
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
from hdiff_amd import device_data as DD  # noqa: E402
from hdiff_amd import optim as hdiff_optim  # noqa: E402
from hdiff_amd import quality  # noqa: E402
from hdiff_amd import synth as SY  # noqa: E402
from hdiff_amd.Loss.loss import MSSSIMLoss  # noqa: E402
from hdiff_amd.diffusion import Evaluate as EV  # noqa: E402
from hdiff_amd.diffusion.Diffusion import GaussianDiffusionSampler, GaussianDiffusionTrainer  # noqa: E402
from hdiff_amd.diffusion.Model import DynamicUNet  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--scenes", type=int, default=256, help="training scenes")
ap.add_argument("--held", type=int, default=32, help="held-out scenes that are sampled and scored")
ap.add_argument("--side", type=int, default=64)
ap.add_argument("--evals", type=int, default=4, help="evenly spaced evaluations, the last one after the last step")
ap.add_argument("--max-seconds", type=float, default=240.0, help="training stops at the next evaluation point after this much wall time")
ap.add_argument("--lr", type=float, default=2e-4)
ap.add_argument("--ema", type=float, default=0.995)
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--prediction", default="eps", choices=("eps", "v"))
ap.add_argument("--solver", default="ddim", choices=("ddim", "dpmpp2m"))
ap.add_argument("--out", default=None, help="append the report to this file")
a = ap.parse_args()

dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
MODEL = dict(T=1000, ch=32, ch_mult=[1, 2, 2], num_res_blocks=1)
BETAS = (1e-4, 0.02)
lines = []


def say(text: str) -> None:
    print(text, flush=True)
    lines.append(text)


scenes = torch.from_numpy(SY.procedural_scenes(a.scenes + a.held, a.side, a.side, seed=a.seed))
train_clean, held_clean = scenes[:a.scenes].contiguous(), scenes[a.scenes:].contiguous()
water = SY.Synth.underwater()
train_cache = DD.PairCache(train_clean, train_clean, None, "procedural-train").to(dev)
held_cache = DD.PairCache(held_clean, held_clean, None, "procedural-held").to(dev)
loader = DD.DeviceLoader(train_cache, a.batch, shuffle=True, drop_last=True, augment=DD.Augment(hflip=0.5, vflip=0.5), seed=a.seed,
                         synth=water)
held = [tuple(batch) for batch in DD.DeviceLoader(held_cache, a.batch, drop_last=False, seed=a.seed + 1, synth=water, synth_epoch=0)]

meter = quality.QualityMeter(color=True)
for inp, label in held:
    meter.update(inp.float() / 255, label.float() / 255)
before = meter.compute()

torch.manual_seed(a.seed)
model = DynamicUNet(dropout=0.1, **MODEL).to(dev).train()
extra = {} if a.prediction == "eps" else {"prediction": a.prediction}
trainer = GaussianDiffusionTrainer(model, BETAS[0], BETAS[1], MODEL["T"], msssim_loss=MSSSIMLoss(), **extra).to(dev)
opt = hdiff_optim.AdamW(model.parameters(), lr=a.lr, weight_decay=1e-4)
ema = hdiff_optim.EMA(model.parameters(), decay=a.ema)
judge = DynamicUNet(dropout=0.0, **MODEL).to(dev).eval()                   # the averaged weights are sampled from a copy
sampler = GaussianDiffusionSampler(judge, BETAS[0], BETAS[1], MODEL["T"], **extra).to(dev)

say(f"# synthetic-degradation demonstration: {a.scenes} procedural scenes of {a.side}x{a.side} for training, {a.held} held out; "
    f"Synth.underwater() (water-type table unpinned); DynamicUNet {MODEL}; batch {a.batch}, AdamW lr {a.lr}, EMA {a.ema}, "
    f"prediction {a.prediction}; scored with 20 {a.solver} steps on the averaged weights, seed {a.seed}; {torch.cuda.get_device_name(0)}")
say(f"degraded input vs clean target (held out): psnr {before['psnr']:.3f} dB  ssim {before['ssim']:.4f}  ciede2000 {before['ciede2000']:.3f}")


def score(step: int, wall: float, recent: float) -> dict:
    judge.load_state_dict(ema.shadow_state_dict(model))
    torch.manual_seed(a.seed + 1)                                           # the same y_T at every evaluation
    r = EV.evaluate(sampler, held, ddim_step=20, color=True, **({} if a.solver == "ddim" else {"solver": a.solver}))
    say(f"step {step:6d}  wall {wall:7.1f} s  loss (mean since the last line) {recent:10.5f}  output vs clean target: "
        f"psnr {r['psnr']:.3f} dB  ssim {r['ssim']:.4f}  ciede2000 {r['ciede2000']:.3f}")
    return {"step": step, "wall_s": wall, "loss": recent, "psnr": r["psnr"], "ssim": r["ssim"], "ciede2000": r["ciede2000"]}


points = sorted({max(1, round(a.steps * (k + 1) / a.evals)) for k in range(a.evals)})
records, step, epoch, since, count = [], 0, 0, torch.zeros((), dtype=torch.float64, device=dev), 0
clock = bench.ClockSampler(0)
t0 = time.perf_counter()
with clock:
    while step < a.steps:
        loader.set_epoch(epoch)
        epoch += 1
        for inp, label in loader:
            opt.zero_grad()
            terms = trainer(gt_images=label, input_image=inp, stage=1)
            terms[0].mean().backward()
            opt.step(max_grad_norm=1.0)
            ema.update()
            since += terms[0].detach().double().mean()
            count += 1
            step += 1
            if step in points:
                torch.cuda.synchronize(dev)
                wall = time.perf_counter() - t0
                records.append(score(step, wall, float(since) / count))
                since.zero_()
                count = 0
                if wall > a.max_seconds and step < a.steps:
                    say(f"stopped after step {step}: {wall:.0f} s of wall time is past --max-seconds {a.max_seconds:.0f}")
                    step = a.steps
            if step >= a.steps:
                break
c = clock.summary()
last = records[-1]
say(f"{last['step']} steps in {last['wall_s']:.1f} s by the wall clock, evaluations included; sclk {c.get('sclk_mhz_mean')} MHz, "
    f"board {c.get('board_power_w_mean')} W")
verdict = {k: last[k] - before[k] for k in ("psnr", "ssim", "ciede2000")}
say(f"output minus input at the last evaluation: psnr {verdict['psnr']:+.3f} dB  ssim {verdict['ssim']:+.4f}  "
    f"ciede2000 {verdict['ciede2000']:+.3f} (lower is better)")
print(json.dumps({"metric": "held-out procedural scenes, output of 20 sampling steps against the degraded input, both scored against the "
                            "clean target", "input": {k: before[k] for k in ("psnr", "ssim", "ciede2000")}, "evaluations": records,
                  "output_minus_input": verdict, "prediction": a.prediction, "solver": a.solver}))
if a.out is not None:
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n\n")
