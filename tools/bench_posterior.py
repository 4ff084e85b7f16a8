"""K posterior samples of one image from ONE step plan at batch K (``GaussianDiffusionSampler.posterior``) against K single-image
``forward`` calls on the path as it was, ALTERNATELY inside one process, engine clock and board power sampled beside each timing
(bench.ClockSampler); a third arm times ``hdiff_sample_stats`` alone by device events.

    python tools/bench_posterior.py [--size 256] [--samples 8] [--ddim-step 20] [--eta 0.5] [--sample-batch N] [--alternate 3]
                                     [--warmup 1] [--stats-reps 20]

Default model (DynamicUNet ch=128, ch_mult=[1,2,2,2], num_res_blocks=2), one image, random-init weights, hipGraph replay in both
sampling arms (each arm has its own sampler, so each keeps its captured plan across the alternation; they share the model).  A
timing is the whole call: uploads, the K x steps model evaluations, the clip and -- for ``posterior`` -- the statistics.  Prints one
line per timing and one JSON summary line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import hdiff_amd  # noqa: E402,F401
import bench  # noqa: E402
from hdiff_amd import _capi  # noqa: E402
from hdiff_amd.diffusion.Diffusion import GaussianDiffusionSampler  # noqa: E402
from hdiff_amd.diffusion.Model import DynamicUNet  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--samples", type=int, default=8)
ap.add_argument("--ddim-step", type=int, default=20)
ap.add_argument("--eta", type=float, default=0.5)
ap.add_argument("--sample-batch", type=int, default=None)
ap.add_argument("--alternate", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--stats-reps", type=int, default=20)
a = ap.parse_args()
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
torch.manual_seed(0)
model = DynamicUNet(T=1000, ch=128, ch_mult=[1, 2, 2, 2], num_res_blocks=2, dropout=0.0).eval().to(dev)
one_plan = GaussianDiffusionSampler(model, 1e-4, 0.02, 1000).to(dev)
k_calls = GaussianDiffusionSampler(model, 1e-4, 0.02, 1000).to(dev)
K, n = a.samples, 3 * a.size * a.size
img = torch.randint(0, 256, (1, 3, a.size, a.size), generator=torch.Generator().manual_seed(1)).float().to(dev)
stack = torch.randn(1, K, n, device=dev).clamp(-1, 1)
mean, std = torch.empty(1, n, device=dev), torch.empty(1, n, device=dev)


def posterior_call():
    one_plan.posterior(img, K, ddim_step=a.ddim_step, eta=a.eta, seed=0, sample_batch=a.sample_batch)


def single_calls():
    for _ in range(K):
        k_calls(img, ddim=True, ddim_step=a.ddim_step)


def stats_alone():
    """-> ms per launch, from device events around --stats-reps launches."""
    lib, s = _capi.lib(), torch.cuda.current_stream(dev).cuda_stream
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.stats_reps):
        _capi.check(lib.hdiff_sample_stats(stack.data_ptr(), 1, K, C.c_int64(n), mean.data_ptr(), std.data_ptr(), s), "sample_stats")
    t1.record()
    torch.cuda.synchronize(dev)
    return t0.elapsed_time(t1) / a.stats_reps


def timed(fn):
    torch.cuda.synchronize(dev)
    clock = bench.ClockSampler(0)
    with clock:
        t0 = time.perf_counter()
        ms = fn()
        torch.cuda.synchronize(dev)
        dt = (time.perf_counter() - t0) * 1e3
    return (dt if ms is None else ms), clock.summary()


arms = {f"posterior: one plan at batch {K if a.sample_batch is None else min(K, a.sample_batch)}, {K} samples": posterior_call,
        f"{K} forward calls at batch 1": single_calls,
        f"hdiff_sample_stats alone, K = {K}, n = {n} (device events)": stats_alone}
times = {k: [] for k in arms}
with torch.no_grad():
    for fn in arms.values():
        for _ in range(a.warmup):                       # builds and captures the plans
            fn()
    for rep in range(a.alternate):
        for name, fn in arms.items():
            ms, c = timed(fn)
            times[name].append(ms)
            print(f"{name} rep {rep}: {ms:.3f} ms  sclk {c.get('sclk_mhz_mean')} MHz  board {c.get('board_power_w_mean')} W", flush=True)
summary = {k: {"ms_mean": sum(v) / len(v), "ms_min": min(v), "ms_max": max(v), "repetitions": len(v)} for k, v in times.items()}
names = list(arms)
per = a.ddim_step * K
print(json.dumps({"metric": f"{K} samples of one {a.size}x{a.size} image, {a.ddim_step} DDIM steps, eta {a.eta}: one posterior call against "
                            f"{K} forward calls, alternating (hipGraph replay)", "unit": "ms/call", "arms": summary,
                  "ms_per_sample_and_step": {names[0]: summary[names[0]]["ms_mean"] / per, names[1]: summary[names[1]]["ms_mean"] / per},
                  "speedup_one_plan_over_k_calls": summary[names[1]]["ms_mean"] / summary[names[0]]["ms_mean"]}))
