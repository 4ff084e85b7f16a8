"""Throughput of the second tree's DDIM sampler (DynamicUNet, image-conditioned) on one MI355X.

    python tools/bench_ddim.py [--size 256] [--batch 8] [--ddim-step 100] [--reps 2] [--contract bf16x3|f32|f16]
                                [--solver ddim|dpmpp2m] [--spacing uniform|logsnr] [--prediction eps|v [eps|v]] [--alternate 3]

One "step" = one DDIM iteration of diffusion/Diffusion.py:248-263 for the whole batch = one DynamicUNet forward + the fused
update (--solver dpmpp2m: the DPM-Solver++(2M) update, by default on logSNR time steps).  Prints one JSON line (same field names as bench.py where they apply).

--prediction v times a sampler built with prediction="v": every step then runs one hdiff_v_to_eps behind the model (the weights are
random either way; what is timed is the launch list).  With TWO values (--prediction eps v) the two samplers share the model and are
timed ALTERNATELY inside one process, --alternate times each, engine clock and board power sampled beside each timing
(bench.ClockSampler, as tools/bench_tiled.py does); one line per timing, then one JSON summary line."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch
import hdiff_amd
from hdiff_amd.diffusion.Model import DynamicUNet
from hdiff_amd.diffusion.Diffusion import GaussianDiffusionSampler

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--ddim-step", type=int, default=100)
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--contract", choices=["f32", "bf16x3", "f16"], default="bf16x3",
                help="the library's default mode is bf16x3; f16: the opt-in sampling mode (single-piece fp16 attention forward)")
ap.add_argument("--solver", choices=["ddim", "dpmpp2m"], default="ddim")
ap.add_argument("--spacing", choices=["uniform", "logsnr"], default=None)
ap.add_argument("--prediction", choices=["eps", "v"], nargs="+", default=["eps"],
                help="one value: that sampler alone; two: both, alternating in one process")
ap.add_argument("--alternate", type=int, default=3, help="with two --prediction values: timings per arm")
a = ap.parse_args()
solver_kw = {} if a.solver == "ddim" and a.spacing is None else dict(solver=a.solver, spacing=a.spacing)
hdiff_amd.set_contraction_mode(a.contract)
dev = torch.device("cuda", 0)
torch.manual_seed(0)
model = DynamicUNet(T=1000, ch=128, ch_mult=[1, 2, 2, 2], num_res_blocks=2, dropout=0.0).eval().to(dev)
img = torch.randint(0, 256, (a.batch, 3, a.size, a.size), generator=torch.Generator().manual_seed(1)).float().to(dev)
workload = (f"image-conditioned DDIM sampling, {a.size}x{a.size}, batch {a.batch}, DynamicUNet ch=128 ch_mult=[1,2,2,2] "
            "num_res_blocks=2 (43.2 M params), random-init weights, hipGraph replay")


def sampler(prediction):
    kw = {} if prediction == "eps" else dict(prediction=prediction)
    return GaussianDiffusionSampler(model, 1e-4, 0.02, 1000, **kw).to(dev)


def timed(samp, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = samp(img, ddim=True, ddim_step=a.ddim_step, **solver_kw)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    return (time.perf_counter() - t0) / reps


if len(a.prediction) == 1:
    samp = sampler(a.prediction[0])
    with torch.no_grad():
        samp(img, ddim=True, ddim_step=a.ddim_step, **solver_kw)            # warm-up: builds the plan, packs weights, captures the graph
        dt = timed(samp, a.reps)
    n_steps = next(iter(samp._plans.values())).n_steps
    step_tflop = model.plan_for(a.batch, a.size, a.size, dev, True).plan.flops / 1e12
    print(json.dumps({"metric": f"{a.solver} denoising-steps/sec ({a.size}x{a.size}, {n_steps} steps)", "value": n_steps / dt,
                      "unit": "denoising-steps/s", "ms_per_step": dt / n_steps * 1e3, "images_per_s": a.batch / dt,
                      "algorithmic_tflop_per_step": step_tflop, "whole_step_tflops": step_tflop / (dt / n_steps),
                      "config": {"workload": workload, "attention_contract": a.contract, "solver": a.solver, "spacing": a.spacing,
                                 "prediction": a.prediction[0]}}))
else:
    import bench
    if len(set(a.prediction)) != len(a.prediction):
        ap.error("--prediction: name each arm once")
    arms = {p: sampler(p) for p in a.prediction}
    times = {p: [] for p in arms}
    with torch.no_grad():
        for samp in arms.values():                                            # each arm's plan is built and captured once
            samp(img, ddim=True, ddim_step=a.ddim_step, **solver_kw)
        n_steps = next(iter(next(iter(arms.values()))._plans.values())).n_steps
        for rep in range(a.alternate):
            for p, samp in arms.items():
                clock = bench.ClockSampler(0)
                with clock:
                    dt = timed(samp, a.reps)
                c = clock.summary()
                times[p].append(dt / n_steps * 1e3)
                print(f"prediction {p} rep {rep}: {dt / n_steps * 1e3:.3f} ms/step  sclk {c.get('sclk_mhz_mean')} MHz  "
                      f"board {c.get('board_power_w_mean')} W", flush=True)
    launches = {p: [op[0] for op in next(iter(s._plans.values())).plan.ops].count("hdiff_v_to_eps") for p, s in arms.items()}
    summary = {p: {"ms_per_step_mean": sum(v) / len(v), "ms_per_step_min": min(v), "ms_per_step_max": max(v), "repetitions": len(v),
                   "v_to_eps_launches_per_step": launches[p]} for p, v in times.items()}
    print(json.dumps({"metric": f"whole {a.solver} step of the image-conditioned sampler ({a.size}x{a.size}, batch {a.batch}, {n_steps} "
                                "steps per call), by what the model predicts, alternating", "unit": "ms/step", "arms": summary,
                      "config": {"workload": workload, "attention_contract": a.contract, "solver": a.solver, "spacing": a.spacing}}))
