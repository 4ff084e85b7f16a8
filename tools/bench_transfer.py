"""Guided full-resolution transfer (hdiff_amd/transfer.py, csrc/transfer.hip), three measurements, arms ALTERNATING inside one process,
engine clock and board power sampled beside each timing (bench.ClockSampler):

  (a) ``guided_fit`` at ``--size`` x ``--size`` plus ``guided_apply`` on a synthetic ``--width`` x ``--height`` uint8 image, against the
      same fit followed by the apply in plain torch ops: ``F.interpolate(coef, size=(H, W), mode="bilinear", align_corners=False)`` and
      an ``einsum`` (which materialise the twelve upsampled planes: 580 MB at 4032 x 3024), clamp, round, cast;
  (b) the apply alone by device events around ``--reps`` consecutive launches, as GB/s of its ``6 H W`` bytes, beside the ~6.3 TB/s
      streaming ceiling of the device;
  (c) one whole ``GuidedEnhancer`` call on a ``--photo-width`` x ``--photo-height`` image with the default ``DynamicUNet`` and
      ``--ddim-step`` steps, against ``sampler(img, ddim=True, ddim_step=..., tile=256)`` on the same image and against one plain
      ``--size`` x ``--size`` sampling call.

    python tools/bench_transfer.py [--alternate 3] [--reps 20] [--skip-model]

Prints one line per timing and one JSON summary line.  No time is fixed in advance and no condition is checked: the expectations to
confirm or refute are that (a)'s native arm is no slower than the torch arm beyond the arms' own spread, and that (c)'s enhancer call
costs about what the model-sized sampling call costs."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import hdiff_amd  # noqa: E402,F401
import bench  # noqa: E402
from hdiff_amd import transfer as T  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--width", type=int, default=4032)
ap.add_argument("--height", type=int, default=3024)
ap.add_argument("--photo-width", type=int, default=1024)
ap.add_argument("--photo-height", type=int, default=768)
ap.add_argument("--ddim-step", type=int, default=20)
ap.add_argument("--radius", type=int, default=8)
ap.add_argument("--eps", type=float, default=1e-3)
ap.add_argument("--alternate", type=int, default=3)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--skip-model", action="store_true", help="leave (c) out: no model is built")
a = ap.parse_args()
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
STREAM_CEILING_GBS = 6300.0


def synthetic(H, W, seed):
    """A smooth colour field plus noise, quantised: uint8 [H, W, 3] on the device."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32) / H, torch.arange(W, dtype=torch.float32) / W, indexing="ij")
    field = torch.stack([0.5 + 0.3 * torch.sin(6 * xx + c) * torch.cos(4 * yy - c) for c in range(3)], dim=-1)
    return ((0.8 * field + 0.2 * torch.rand(H, W, 3, generator=g)).clamp(0, 1) * 255).round().to(torch.uint8).to(dev)


H, W = a.height, a.width
img = synthetic(H, W, 0)
low = T.resample(img, a.size)[None] / 255
target = (low.flip(1) ** 0.8 * 0.9 + 0.05).clamp(0, 1).contiguous()          # channels swapped, a power, a gain: something to fit


def native_arm():
    coef = T.guided_fit(low, target, radius=a.radius, eps=a.eps)
    return T.guided_apply(coef[0], img)


def torch_arm():
    coef = T.guided_fit(low, target, radius=a.radius, eps=a.eps)
    up = F.interpolate(coef, size=(H, W), mode="bilinear", align_corners=False)[0]
    full = img.permute(2, 0, 1).float() / 255
    q = torch.einsum("cjyx,jyx->cyx", up[:9].view(3, 3, H, W), full) + up[9:]
    return (q.clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous()


def wall(fn, reps):
    for _ in range(a.warmup):
        out = fn()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3 / reps, out


def apply_events():
    coef = T.guided_fit(low, target, radius=a.radius, eps=a.eps)[0]
    out = torch.empty_like(img)
    for _ in range(a.warmup):
        T._apply_u8_into(coef, img, out)
    torch.cuda.synchronize(dev)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(a.reps):
        T._apply_u8_into(coef, img, out)
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / a.reps, out


def timed(arm, label, fmt):
    clock = bench.ClockSampler(0)
    with clock:
        ms, res = arm()
    c = clock.summary()
    print(f"{label} {fmt(ms)}  sclk {c.get('sclk_mhz_mean')} MHz  board {c.get('board_power_w_mean')} W", flush=True)
    return ms, res


times = {"a_native_fit_apply_ms": [], "a_torch_fit_interpolate_einsum_ms": [], "b_apply_alone_ms": []}
for rep in range(a.alternate):
    ms0, out0 = timed(lambda: wall(native_arm, a.reps), f"(a) native fit + apply       rep {rep}:", lambda ms: f"{ms:.3f} ms per image of {W}x{H}")
    ms1, out1 = timed(lambda: wall(torch_arm, max(a.reps // 4, 1)), f"(a) torch interpolate+einsum rep {rep}:",
                      lambda ms: f"{ms:.3f} ms per image of {W}x{H}")
    ms2, _ = timed(apply_events, f"(b) apply alone              rep {rep}:",
                   lambda ms: f"{ms:.4f} ms = {6.0 * H * W / ms / 1e6:.0f} GB/s of its 6 H W bytes ({a.reps} launches between two events; "
                              f"ceiling ~{STREAM_CEILING_GBS:.0f})")
    for k, ms in zip(times, (ms0, ms1, ms2)):
        times[k].append(ms)
    gap = (out0.int() - out1.int()).abs()
    print(f"    native against torch: {int((gap > 0).sum())} of {gap.numel()} bytes differ, largest difference {int(gap.max())}", flush=True)
    del out0, out1, gap
torch.cuda.empty_cache()

model_times = {}
if not a.skip_model:
    from hdiff_amd.diffusion.Diffusion import GaussianDiffusionSampler
    from hdiff_amd.diffusion.Model import DynamicUNet
    torch.manual_seed(0)
    model = DynamicUNet(T=1000, ch=128, ch_mult=[1, 2, 2, 2], num_res_blocks=2, dropout=0.0).eval().to(dev)      # random weights: time only
    sampler = GaussianDiffusionSampler(model, 1e-4, 0.02, 1000).to(dev)
    photo = synthetic(a.photo_height, a.photo_width, 1)
    photo_f = photo.permute(2, 0, 1)[None].float().contiguous()
    small_f = T.resample(photo, a.size)[None]
    enhance = T.GuidedEnhancer(sampler, size=a.size, radius=a.radius, eps=a.eps, ddim_step=a.ddim_step)
    arms = (("c_enhancer_call_ms", f"(c) GuidedEnhancer {a.photo_width}x{a.photo_height}     ", lambda: enhance(photo)),
            ("c_tiled_sampling_ms", f"(c) sampler tile=256 {a.photo_width}x{a.photo_height}   ",
             lambda: sampler(photo_f, ddim=True, ddim_step=a.ddim_step, tile=256)),
            ("c_model_sized_sampling_ms", f"(c) sampler {a.size}x{a.size} alone        ", lambda: sampler(small_f, ddim=True, ddim_step=a.ddim_step)))
    model_times = {k: [] for k, _, _ in arms}
    with torch.no_grad():
        for k, _, fn in arms:                        # plans are built and captured on the first call
            fn()
        torch.cuda.synchronize(dev)
        for rep in range(a.alternate):
            for k, label, fn in arms:
                ms, _ = timed(lambda: wall(fn, 1), f"{label} rep {rep}:", lambda ms: f"{ms:.1f} ms per call ({a.ddim_step} steps)")
                model_times[k].append(ms)

summary = {k: {"mean": sum(v) / len(v), "min": min(v), "max": max(v), "repetitions": len(v)} for k, v in {**times, **model_times}.items() if v}
line = {"metric": f"guided transfer: fit at {a.size}x{a.size} + apply on uint8 {W}x{H}, native against torch ops; the apply alone; "
                  f"GuidedEnhancer on {a.photo_width}x{a.photo_height} against tiled sampling; alternating", "unit": "ms", "arms": summary,
        "b_apply_gb_per_s_mean": 6.0 * H * W / summary["b_apply_alone_ms"]["mean"] / 1e6, "stream_ceiling_gb_per_s": STREAM_CEILING_GBS,
        "a_torch_over_native": summary["a_torch_fit_interpolate_einsum_ms"]["mean"] / summary["a_native_fit_apply_ms"]["mean"]}
if model_times:
    line["c_tiled_over_enhancer"] = summary["c_tiled_sampling_ms"]["mean"] / summary["c_enhancer_call_ms"]["mean"]
    line["c_enhancer_over_model_sized_sampling"] = summary["c_enhancer_call_ms"]["mean"] / summary["c_model_sized_sampling_ms"]["mean"]
print(json.dumps(line))
