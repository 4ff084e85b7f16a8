"""The classical baselines for one batch of 8 images at 256x256, two ways, ALTERNATELY inside one process, engine clock and board power
sampled beside each timing (bench.ClockSampler):

  (a) hip: ``classical.dehaze`` (each prior, with and without the guided refinement) and ``classical.white_balance``, timed by device
      events around ``--reps`` consecutive calls (nothing synchronises in between);
  (b) torch: the same steps in plain torch ops on the device -- ``-max_pool2d(-x)`` for the windowed minimum, ``torch.topk`` for the
      cut, a gather for the airlight, elementwise ops for transmission and recovery (fp32 throughout, so NOT the definition's
      rounding: it is the comparison arm, not a reference).  The refinement is ``transfer.guided_fit`` / ``guided_apply`` in both arms.

It also times ``Evaluate.evaluate`` over ``--eval-batches`` batches with a stand-in sampler (one elementwise op, so the loop and the
scores are what is timed) without and with ``baselines=("input", "gray_world", "dcp")``, wall clock with one synchronisation.

    python tools/bench_classical.py [--batch 8] [--size 256] [--alternate 3] [--reps 20] [--warmup 3]
    python tools/bench_classical.py --contrast [--alternate 3]      # CLAHE and equalisation against the host path (contrast_arms)

Prints one line per timing and one JSON summary line.  No condition is checked: the figures are reported as they come."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import hdiff_amd  # noqa: E402,F401
import bench  # noqa: E402
from hdiff_amd import classical, transfer  # noqa: E402
from hdiff_amd.diffusion import Evaluate  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--alternate", type=int, default=3)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--eval-batches", type=int, default=4)
ap.add_argument("--contrast", action="store_true", help="time CLAHE and equalisation (and nothing else): see contrast_arms()")
ap.add_argument("--host-reps", type=int, default=2)
ap.add_argument("--photo-reps", type=int, default=5)
a = ap.parse_args()
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
g = torch.Generator().manual_seed(0)
# image-like content: smooth colour fields plus noise under a grey veil
yy, xx = torch.meshgrid(torch.arange(a.size, dtype=torch.float32), torch.arange(a.size, dtype=torch.float32), indexing="ij")
base = torch.stack([0.5 + 0.4 * torch.sin(xx / 25 + c) * torch.cos(yy / 35 - c) for c in range(3)])
clean = (base[None] + 0.05 * torch.randn(a.batch, 3, a.size, a.size, generator=g)).clamp(0, 1)
depth = (0.3 + 0.6 * yy / a.size)[None, None]
img = (clean * depth + 0.85 * (1 - depth)).clamp(0, 1).to(dev)
clean = clean.to(dev)
PATCH, OMEGA, T0, TOP, REFINE = 15, 0.95, 0.1, 1e-3, (16, 1e-3)


def window_min_torch(x):
    return -F.max_pool2d(-x, PATCH, stride=1, padding=PATCH // 2)      # max_pool2d pads with -inf: the window is clipped at the border


def dehaze_torch(x, prior, refine):
    x = x.clamp(0, 1)
    if prior == "inverted_dcp":
        x = 1 - x
    ch = x[:, 1:] if prior == "udcp" else x
    N, _, H, W = x.shape
    dark = window_min_torch(ch.amin(1, keepdim=True)).reshape(N, -1)
    n_top = max(1, int(math.floor(TOP * H * W)))
    cut = torch.topk(dark, n_top, dim=1).values[:, -1:]
    total = x.double().sum(1).reshape(N, -1).masked_fill(dark < cut, -1.0)
    at = total.argmax(1)
    A = x.reshape(N, 3, -1).gather(2, at[:, None, None].expand(N, 3, 1)).clamp_min(1 / 255)[..., None]
    ratio = x / A
    t = 1 - OMEGA * window_min_torch((ratio[:, 1:] if prior == "udcp" else ratio).amin(1, keepdim=True))
    if refine is not None:
        coef = transfer.guided_fit(x, t.expand(N, 3, H, W).contiguous(), radius=refine[0], eps=refine[1])
        t = transfer.guided_apply(coef, x, clamp=False)[:, :1]
    J = ((x - A) / t.clamp_min(T0) + A).clamp(0, 1)
    return 1 - J if prior == "inverted_dcp" else J


def white_balance_torch(x):
    x = x.clamp(0, 1)
    m = x.double().mean((2, 3))
    gains = m.mean(1, keepdim=True) / m.clamp_min(1e-6)
    return (x.double() * gains[:, :, None, None]).clamp(0, 1).float()


def device_arm(fn, reps=None):
    reps = a.reps if reps is None else reps
    for _ in range(a.warmup):
        out = fn()
    torch.cuda.synchronize(dev)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        out = fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps, out


def stand_in_sampler(inp, **kwargs):
    return inp / 127.5 - 1


def evaluate_arm(baselines):
    batches = [((img * 255), (clean * 255)) for _ in range(a.eval_batches)]
    Evaluate.evaluate(stand_in_sampler, batches[:1], ddim_step=1, baselines=baselines)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    res = Evaluate.evaluate(stand_in_sampler, batches, ddim_step=1, baselines=baselines)
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3 / a.eval_batches, res


def timed(arm, label, fmt):
    clock = bench.ClockSampler(0)
    with clock:
        ms, res = arm()
    c = clock.summary()
    print(f"{label} {fmt(ms)}  sclk {c.get('sclk_mhz_mean')} MHz  board {c.get('board_power_w_mean')} W", flush=True)
    return ms, res


def contrast_arms():
    """``--contrast``: ``clahe_rgb``, ``clahe_lab`` and ``equalize`` (``classical.CONTRAST_BASELINES``) on the batch, the device arm as
    above; the comparison arm is the only host path there is -- a copy to the host, then the vectorised numpy definition
    (tests/_contrast_def.py) image by image, wall clock -- and for ``equalize`` also ``PIL.ImageOps.equalize`` per image on the copied
    bytes; every host arm makes one untimed call first.  Then one ``clahe_lab`` call on a single 4032x3024 image beside the bytes its
    kernels must move."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import _contrast_def as D
    from PIL import Image, ImageOps

    def host_arm(fn):
        fn(img[0].cpu().numpy())                                      # first-call costs (Pillow's, numpy's) stay out of the timing
        t0 = time.perf_counter()
        for _ in range(a.host_reps):
            host = img.cpu().numpy()                                  # the copy is part of the host path
            out = np.stack([fn(im) for im in host])
        return (time.perf_counter() - t0) * 1e3 / a.host_reps, out

    def pillow(im):
        rgb = np.floor(im.astype(np.float64).clip(0, 1) * 255.0 + 0.5).astype(np.uint8).transpose(1, 2, 0)
        return np.asarray(ImageOps.equalize(Image.fromarray(np.ascontiguousarray(rgb), "RGB"))).transpose(2, 0, 1) / np.float32(255.0)

    arms = [("clahe_rgb", classical.CONTRAST_BASELINES["clahe_rgb"], lambda im: D.clahe_def(im, space="rgb")["out"], None),
            ("clahe_lab", classical.CONTRAST_BASELINES["clahe_lab"], lambda im: D.clahe_def(im, space="lab")["out"], None),
            ("equalize", classical.CONTRAST_BASELINES["equalize"], lambda im: D.equalize_def(im, space="rgb")["out"], pillow)]
    per_host = lambda ms: f"{ms:.2f} ms per batch of {a.batch} x {a.size}x{a.size} (copy + numpy, wall clock, {a.host_reps} runs)"      # noqa: E731
    per_pil = lambda ms: f"{ms:.2f} ms per batch of {a.batch} x {a.size}x{a.size} (copy + bytes + Pillow, wall clock, {a.host_reps} runs)"      # noqa: E731
    results = {}
    for rep in range(a.alternate):
        for name, hip, ref, pil in arms:
            ms0, out0 = timed(lambda: device_arm(lambda: hip(img)), f"{name:34s} hip   rep {rep}:", per_call)
            ms1, out1 = timed(lambda: host_arm(ref), f"{name:34s} numpy rep {rep}:", per_host)
            results.setdefault(name, {"hip_ms": [], "numpy_ms": []})
            results[name]["hip_ms"].append(ms0)
            results[name]["numpy_ms"].append(ms1)
            if pil is not None:
                ms2, out2 = timed(lambda: host_arm(pil), f"{name:34s} PIL   rep {rep}:", per_pil)
                results[name].setdefault("pillow_ms", []).append(ms2)
            if rep == 0:
                print(f"{'':34s} max |hip - numpy| on this batch: {np.abs(out0.cpu().numpy() - out1).max():.2e}"
                      + ("" if pil is None else f"; max |hip - PIL|: {np.abs(out0.cpu().numpy() - out2).max():.2e}"), flush=True)
    # one photograph-sized image
    H, W = 3024, 4032
    gen = torch.Generator().manual_seed(1)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    photo = torch.stack([0.5 + 0.4 * torch.sin(xs / 250 + c) * torch.cos(ys / 350 - c) for c in range(3)])[None]
    photo = (photo + 0.05 * torch.randn(1, 3, H, W, generator=gen)).clamp(0, 1).to(dev)
    px = H * W
    moved = {"quantise": 13 * px, "luts": px + 64 * 256, "apply": 25 * px + 64 * 256}      # bytes: 3 fp32 in, 1 byte out; 1 byte in;
    total = sum(moved.values())                                                              # 3 fp32 + 1 byte in, 3 fp32 out
    for rep in range(a.alternate):
        ms, _ = timed(lambda: device_arm(lambda: classical.clahe(photo), a.photo_reps), f"{'clahe_lab 1 x 4032x3024':34s} hip   rep {rep}:",
                      lambda ms: f"{ms:.4f} ms per call ({a.photo_reps} calls between two events)")
        results.setdefault("clahe_lab_4032x3024", {"hip_ms": []})["hip_ms"].append(ms)
    best = min(results["clahe_lab_4032x3024"]["hip_ms"])
    print(f"   bytes the kernels must move at 4032x3024: quantise {moved['quantise'] / 1e6:.1f} MB, luts {moved['luts'] / 1e6:.1f} MB, "
          f"apply {moved['apply'] / 1e6:.1f} MB (its four table reads per pixel come from 16 KiB of tables and are not counted); "
          f"{total / 1e6:.1f} MB in all = {total / 6.3e12 * 1e3:.4f} ms at 6.3 TB/s, against {best:.4f} ms measured "
          f"({total / (best * 1e-3) / 1e12:.3f} TB/s)", flush=True)
    summary = {name: {k: {"mean": sum(v) / len(v), "min": min(v), "max": max(v), "repetitions": len(v)} for k, v in arm.items()}
               for name, arm in results.items()}
    print(json.dumps({"metric": f"contrast baselines on one batch of {a.batch} at {a.size}x{a.size}: hdiff_amd.classical against a copy "
                                "to the host and the numpy definition (and PIL.ImageOps.equalize), alternating; clahe_lab on one "
                                "4032x3024 image", "unit": "ms", "bytes_4032x3024": moved, "arms": summary}))


per_call = lambda ms: f"{ms:.4f} ms per call on {a.batch} x {a.size}x{a.size} ({a.reps} calls between two events)"      # noqa: E731
if a.contrast:
    contrast_arms()
    sys.exit(0)

cases = [(f"dehaze {prior}{'' if refine is None else ' refined'}",
          (lambda p=prior, r=refine: classical.dehaze(img, prior=p, patch=PATCH, omega=OMEGA, t0=T0, top=TOP, refine=r)),
          (lambda p=prior, r=refine: dehaze_torch(img, p, r)))
         for prior in ("dcp", "udcp", "inverted_dcp") for refine in (None, REFINE)]
cases.append(("white_balance p=1", lambda: classical.white_balance(img, p=1.0), lambda: white_balance_torch(img)))
times = {}
for rep in range(a.alternate):
    for name, hip, ref in cases:
        ms0, out0 = timed(lambda: device_arm(hip), f"{name:34s} hip   rep {rep}:", per_call)
        ms1, out1 = timed(lambda: device_arm(ref), f"{name:34s} torch rep {rep}:", per_call)
        times.setdefault(name, {"hip_ms": [], "torch_ms": []})
        times[name]["hip_ms"].append(ms0)
        times[name]["torch_ms"].append(ms1)
        if rep == 0:
            print(f"{'':34s} max |hip - torch| on this batch: {(out0 - out1).abs().max().item():.2e}", flush=True)
    per_batch = lambda ms: f"{ms:.3f} ms per batch of {a.batch} ({a.eval_batches} batches, wall clock)"      # noqa: E731
    ms0, _ = timed(lambda: evaluate_arm(None), f"{'evaluate':34s} plain rep {rep}:", per_batch)
    ms1, res = timed(lambda: evaluate_arm(("input", "gray_world", "dcp")), f"{'evaluate with three baselines':34s}       rep {rep}:", per_batch)
    times.setdefault("evaluate", {"plain_ms": [], "with_baselines_ms": []})
    times["evaluate"]["plain_ms"].append(ms0)
    times["evaluate"]["with_baselines_ms"].append(ms1)
    if rep == 0:
        print("   PSNR of the batch: " + ", ".join(f"{n} {res['baselines'][n]['psnr']:.2f} dB" for n in res["baselines"]), flush=True)
summary = {name: {k: {"mean": sum(v) / len(v), "min": min(v), "max": max(v), "repetitions": len(v)} for k, v in arms.items()}
           for name, arms in times.items()}
print(json.dumps({"metric": f"classical baselines on one batch of {a.batch} at {a.size}x{a.size}: hdiff_amd.classical against the same "
                            "steps in torch ops on the device, alternating; Evaluate.evaluate per batch without / with three baselines",
                  "unit": "ms", "arms": summary}))
