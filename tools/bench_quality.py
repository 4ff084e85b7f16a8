"""Scoring one batch of 8 images at 256x256 two ways, ALTERNATELY inside one process, engine clock and board power sampled beside
each timing (bench.ClockSampler):

  (a) device: ``quality.QualityMeter.update(pred, target)`` -- PSNR, SSIM and UIQM with its parts for the whole batch, timed by device
      events around ``--reps`` consecutive updates (nothing synchronises in between);
  (b) host: what it replaces -- copy the batch to the host, then ``metrics.psnr`` / ``metrics.ssim`` and ``uw_metrics.getUIQM`` per
      image in one Python thread.

    python tools/bench_quality.py [--batch 8] [--size 256] [--alternate 3] [--reps 50] [--warmup 5]

Prints one line per timing and one JSON summary line.  The one condition checked (exit status 1 otherwise): the device arm for the
WHOLE batch takes less than the host arm for ONE image in the same run -- any sound kernel clears that by an order of magnitude; it
is there to catch a hidden per-image synchronisation or host fallback.

With ``--uciqe`` three arms alternate instead: ``QualityMeter.update`` without UCIQE, ``QualityMeter(uciqe=True).update``, and the host
path the latter replaces (copy the batch, then ``uw_metrics.nmetrics`` per image in one Python thread).  The JSON line holds what
UCIQE adds per update (the difference of the two device arms), its ratio to the host path and to one 29.4 ms DDIM step; the
condition checked is that the added device time for the whole batch stays below the host time for one image.

With ``--distribution`` four arms alternate: the device part of ``DistributionMeter.compute`` (``quality.moments`` of two banks of
``--rows`` x ``--width`` features and ``quality.kid_sums``), the host path it stands in for (copy the features, ``np.cov`` and three
float64 Gram products), ``frechet_from_moments`` on the host, and one ``DistributionMeter.update`` of the batch (predictions and
targets) through ``dinov2_vits14`` with random weights.  No condition is checked: the figures are reported as they come.

With ``--niqe`` four arms alternate: ``QualityMeter.update`` without NIQE, ``QualityMeter(niqe=model).update`` at ``--niqe-patch``
(default 32; the model is fitted on the targets of the batch), ``quality.niqe`` of ONE ``--niqe-full`` image (default 3024 x 4032) at
patch 96 -- wall clock, its one synchronisation, copy and host finish included -- and the only host path that exists for it: copy the
image, then the vectorised numpy definition ``tests/_niqe_def.py``.  The JSON line holds what NIQE adds per update and its ratio to one
29.4 ms DDIM step, and the two full-size times.  No condition is checked.

With ``--color`` five arms alternate: ``QualityMeter.update`` plain, with UCIQE (the comparable multi-launch score, for scale) and with
the colour differences (``color=True``: CIEDE2000, its 95th percentile, CIE76, the angular error); ``quality.color_difference`` of a
batch of 8 x 8 images, which is the cost of its fifteen launches with next to no arithmetic behind them; and the host path the kernel
replaces: copy both batches, then the vectorised numpy CIEDE2000 of ``tests/_color_def.py`` per image.  The JSON line holds what the
colour columns and what UCIQE add per update, and the launch floor.  No condition is checked."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import hdiff_amd  # noqa: E402,F401
import bench  # noqa: E402
from hdiff_amd import metrics, quality, uw_metrics  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--alternate", type=int, default=3)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--uciqe", action="store_true", help="time QualityMeter.update without / with UCIQE against uw_metrics.nmetrics on the host")
ap.add_argument("--distribution", action="store_true", help="time the set-level scores: moments + KID sums against numpy on the host, "
                "frechet_from_moments, and one DistributionMeter.update through dinov2_vits14")
ap.add_argument("--niqe", action="store_true", help="time QualityMeter.update without / with NIQE, and quality.niqe of one full-size "
                "image against the numpy definition on the host")
ap.add_argument("--color", action="store_true", help="time QualityMeter.update without / with the colour differences (and with UCIQE, "
                "for scale) against a vectorised numpy CIEDE2000 on the host")
ap.add_argument("--niqe-patch", type=int, default=32, help="--niqe: block side of the meter arm")
ap.add_argument("--niqe-full", type=int, nargs=2, default=(3024, 4032), metavar=("H", "W"), help="--niqe: the full-size image")
ap.add_argument("--rows", type=int, default=1024, help="--distribution: rows per feature bank")
ap.add_argument("--width", type=int, default=384, help="--distribution: feature width")
a = ap.parse_args()
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
g = torch.Generator().manual_seed(0)
# image-like content: smooth colour fields plus noise, the prediction a perturbed target
yy, xx = torch.meshgrid(torch.arange(a.size, dtype=torch.float32), torch.arange(a.size, dtype=torch.float32), indexing="ij")
base = torch.stack([0.5 + 0.4 * torch.sin(xx / 25 + c) * torch.cos(yy / 35 - c) for c in range(3)])
target = (base[None] + 0.05 * torch.randn(a.batch, 3, a.size, a.size, generator=g)).clamp(0, 1)
pred = (target + 0.03 * torch.randn(a.batch, 3, a.size, a.size, generator=g)).clamp(0, 1)
pred_d, target_d = pred.to(dev), target.to(dev)


def device_arm(uciqe=False, niqe=None, color=False):
    meter = quality.QualityMeter(capacity=a.batch * (a.reps + a.warmup), uciqe=uciqe, niqe=niqe, color=color)
    for _ in range(a.warmup):
        meter.update(pred_d, target_d)
    torch.cuda.synchronize(dev)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(a.reps):
        meter.update(pred_d, target_d)
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / a.reps, meter.compute()


def host_arm():
    t0 = time.perf_counter()
    p = pred_d.cpu().numpy().transpose(0, 2, 3, 1)
    t = target_d.cpu().numpy().transpose(0, 2, 3, 1)
    rows = []
    for i in range(a.batch):
        pi, ti = np.clip(p[i], 0, 1) * 255, np.clip(t[i], 0, 1) * 255
        rows.append((metrics.psnr(ti, pi, 255.0), metrics.ssim(ti, pi, 255.0, channel_axis=2), uw_metrics.getUIQM(pi)))
    return (time.perf_counter() - t0) * 1e3, rows


def timed(arm, label, fmt):
    """One arm under the clock sampler: prints its line, returns (ms, what the arm returned)."""
    clock = bench.ClockSampler(0)
    with clock:
        ms, res = arm()
    c = clock.summary()
    print(f"{label} {fmt(ms)}  sclk {c.get('sclk_mhz_mean')} MHz  board {c.get('board_power_w_mean')} W", flush=True)
    return ms, res


def uciqe_host_arm():
    t0 = time.perf_counter()
    p = pred_d.cpu().numpy().transpose(0, 2, 3, 1)
    rows = [uw_metrics.nmetrics(np.clip(p[i], 0, 1).astype(np.float64))[1] for i in range(a.batch)]
    return (time.perf_counter() - t0) * 1e3, rows


if a.uciqe:
    times = {"meter_ms": [], "meter_with_uciqe_ms": [], "host_nmetrics_batch_ms": []}
    for rep in range(a.alternate):
        per_update = lambda ms: f"{ms:.4f} ms per update of {a.batch} ({a.reps} updates between two events)"      # noqa: E731
        ms0, _ = timed(device_arm, f"meter            rep {rep}:", per_update)
        ms1, res = timed(lambda: device_arm(uciqe=True), f"meter with UCIQE rep {rep}:", per_update)
        ms2, rows = timed(uciqe_host_arm, f"host nmetrics    rep {rep}:",
                          lambda ms: f"{ms:.2f} ms per batch of {a.batch} = {ms / a.batch:.2f} ms per image")
        for k, ms in zip(times, (ms0, ms1, ms2)):
            times[k].append(ms)
        gap = max(abs(res["per_image"][i, 6] - rows[i]) / abs(rows[i]) for i in range(a.batch))
        print(f"                 device against host on this batch: UCIQE rel {gap:.1e}", flush=True)
    summary = {k: {"mean": sum(v) / len(v), "min": min(v), "max": max(v), "repetitions": len(v)} for k, v in times.items()}
    added = [w - p for w, p in zip(times["meter_with_uciqe_ms"], times["meter_ms"])]
    added_worst, host_image_best = max(added), min(times["host_nmetrics_batch_ms"]) / a.batch
    ok = added_worst < host_image_best
    print(json.dumps({"metric": f"QualityMeter.update of one batch of {a.batch} at {a.size}x{a.size} without / with UCIQE, against "
                                f"uw_metrics.nmetrics per image on the host, alternating",
                      "unit": "ms/batch", "arms": summary, "uciqe_added_ms_per_update": {"mean": sum(added) / len(added), "max": added_worst},
                      "host_over_added_device": summary["host_nmetrics_batch_ms"]["mean"] / (sum(added) / len(added)),
                      "added_ms_over_29.4_ms_ddim_step": (sum(added) / len(added)) / 29.4,
                      "host_ms_per_image_min": host_image_best, "added_device_batch_below_one_host_image": ok}))
    sys.exit(0 if ok else 1)

if a.color:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _color_def as color_def  # noqa: E402
    tiny_p, tiny_t = pred_d[:, :, :8, :8].contiguous(), target_d[:, :, :8, :8].contiguous()

    def floor_arm():
        """``color_difference`` where the fifteen launches are all there is: a batch of 8 x 8 images."""
        for _ in range(a.warmup):
            quality.color_difference(tiny_p, tiny_t)
        torch.cuda.synchronize(dev)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(a.reps):
            out = quality.color_difference(tiny_p, tiny_t)
        end.record()
        end.synchronize()
        return start.elapsed_time(end) / a.reps, out

    def color_host_arm():
        t0 = time.perf_counter()
        p, t = pred_d.cpu().numpy(), target_d.cpu().numpy()
        rows = [float(np.mean(color_def.pixels_def(p[i], t[i])[0])) for i in range(a.batch)]
        return (time.perf_counter() - t0) * 1e3, rows

    times = {"meter_ms": [], "meter_with_uciqe_ms": [], "meter_with_color_ms": [], "color_launch_floor_ms": [], "host_ciede2000_batch_ms": []}
    for rep in range(a.alternate):
        per_update = lambda ms: f"{ms:.4f} ms per update of {a.batch} ({a.reps} updates between two events)"      # noqa: E731
        ms0, _ = timed(device_arm, f"meter             rep {rep}:", per_update)
        ms1, _ = timed(lambda: device_arm(uciqe=True), f"meter with UCIQE  rep {rep}:", per_update)
        ms2, res = timed(lambda: device_arm(color=True), f"meter with colour rep {rep}:", per_update)
        ms3, _ = timed(floor_arm, f"colour at 8x8     rep {rep}:",
                       lambda ms: f"{ms:.4f} ms per call of {a.batch} ({a.reps} calls between two events)")
        ms4, rows = timed(color_host_arm, f"host CIEDE2000    rep {rep}:",
                          lambda ms: f"{ms:.2f} ms per batch of {a.batch} = {ms / a.batch:.2f} ms per image (copy included)")
        for k, ms in zip(times, (ms0, ms1, ms2, ms3, ms4)):
            times[k].append(ms)
        gap = max(abs(res["per_image"][i, 6] - rows[i]) / abs(rows[i]) for i in range(a.batch))
        print(f"                  device against host on this batch: mean CIEDE2000 rel {gap:.1e}; set mean {res['ciede2000']:.6g}, "
              f"p95 {res['ciede2000_p95']:.6g}, CIE76 {res['deltae76']:.6g}, angular {res['angular']:.6g} deg", flush=True)
    summary = {k: {"mean": sum(v) / len(v), "min": min(v), "max": max(v), "repetitions": len(v)} for k, v in times.items()}
    added = [w - p for w, p in zip(times["meter_with_color_ms"], times["meter_ms"])]
    added_uciqe = [w - p for w, p in zip(times["meter_with_uciqe_ms"], times["meter_ms"])]
    print(json.dumps({"metric": f"QualityMeter.update of one batch of {a.batch} at {a.size}x{a.size} plain / with UCIQE / with the colour "
                                f"differences; color_difference of {a.batch} images of 8x8 (its launches alone); a vectorised numpy "
                                f"CIEDE2000 per image on the host; alternating",
                      "unit": "ms", "arms": summary, "color_added_ms_per_update": {"mean": sum(added) / len(added), "max": max(added)},
                      "uciqe_added_ms_per_update": {"mean": sum(added_uciqe) / len(added_uciqe), "max": max(added_uciqe)},
                      "launch_floor_over_color_added": summary["color_launch_floor_ms"]["mean"] / (sum(added) / len(added)),
                      "added_ms_over_29.4_ms_ddim_step": (sum(added) / len(added)) / 29.4,
                      "host_over_added_device": summary["host_ciede2000_batch_ms"]["mean"] / (sum(added) / len(added))}))
    sys.exit(0)

if a.niqe:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _niqe_def as niqe_def  # noqa: E402
    model = quality.NIQEModel.fit([target_d], patch=a.niqe_patch)
    H, W = a.niqe_full
    fy, fx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    full = torch.stack([0.5 + 0.3 * torch.sin(fx / 40 + c) * torch.cos(fy / 55 - c) for c in range(3)])
    # the model: the same field with a quarter of the noise (this times the score and compares two implementations; it judges nothing)
    model_full = quality.NIQEModel.fit([(full + 0.01 * torch.randn(3, H, W, generator=g)).clamp(0, 1)[None].to(dev)], patch=96)
    full = (full + 0.04 * torch.randn(3, H, W, generator=g)).clamp(0, 1)[None].to(dev)
    del fy, fx

    def full_arm():
        quality.niqe(full, model_full)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(5):
            score = quality.niqe(full, model_full)          # synchronises once per call
        return (time.perf_counter() - t0) * 1e3 / 5, float(score[0])

    def full_host_arm():
        t0 = time.perf_counter()
        img = full[0].cpu().numpy()
        score = niqe_def.niqe(img, model_full.mean, model_full.cov, 96)
        return (time.perf_counter() - t0) * 1e3, score

    times = {"meter_ms": [], "meter_with_niqe_ms": [], "full_device_ms": [], "full_host_definition_ms": []}
    for rep in range(a.alternate):
        per_update = lambda ms: f"{ms:.4f} ms per update of {a.batch} ({a.reps} updates between two events)"      # noqa: E731
        ms0, _ = timed(device_arm, f"meter                 rep {rep}:", per_update)
        ms1, res = timed(lambda: device_arm(niqe=model), f"meter with NIQE       rep {rep}:", per_update)
        ms2, got = timed(full_arm, f"niqe of {H}x{W}    rep {rep}:", lambda ms: f"{ms:.3f} ms per image, wall clock (5 calls)")
        ms3, want = timed(full_host_arm, f"host definition       rep {rep}:", lambda ms: f"{ms:.1f} ms per image (copy included)")
        for k, ms in zip(times, (ms0, ms1, ms2, ms3)):
            times[k].append(ms)
        print(f"                      full-size score: device {got!r} host {want!r} rel {abs(got - want) / abs(want):.1e}; "
              f"meter NIQE mean {res['niqe']:.6g}, undefined {res['niqe_undefined']}", flush=True)
    summary = {k: {"mean": sum(v) / len(v), "min": min(v), "max": max(v), "repetitions": len(v)} for k, v in times.items()}
    added = [w - p for w, p in zip(times["meter_with_niqe_ms"], times["meter_ms"])]
    print(json.dumps({"metric": f"QualityMeter.update of one batch of {a.batch} at {a.size}x{a.size} without / with NIQE at patch "
                                f"{a.niqe_patch}; quality.niqe of one {H}x{W} image at patch 96 against the numpy definition on the "
                                f"host; alternating",
                      "unit": "ms", "arms": summary, "niqe_added_ms_per_update": {"mean": sum(added) / len(added), "max": max(added)},
                      "added_ms_over_29.4_ms_ddim_step": (sum(added) / len(added)) / 29.4,
                      "full_host_over_device": summary["full_host_definition_ms"]["mean"] / summary["full_device_ms"]["mean"]}))
    sys.exit(0)

if a.distribution:
    import warnings
    from hdiff_amd.dino import DinoV2Features
    rows, width = a.rows, a.width
    passes = 25 * a.reps                     # a pass is well under a millisecond: enough of them for a window of a few tenths of a second
    fa = (torch.randn(rows, width, generator=g) * 0.05 + torch.randn(width, generator=g)).to(dev)
    fb = (torch.randn(rows, width, generator=g) * 0.06 + torch.randn(width, generator=g) + 0.01).to(dev)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                  # random weights: this times the trunk, it scores nothing
        features = quality.DinoFeatures(DinoV2Features("dinov2_vits14").to(dev))
        features(pred_d)

    def sums_arm():
        """The device part of ``DistributionMeter.compute``: the moments of both banks and the three kernel sums."""
        for _ in range(a.warmup):
            quality.moments(fa), quality.moments(fb), quality.kid_sums(fa, fb)
        torch.cuda.synchronize(dev)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(passes):
            ma, mb, sums = quality.moments(fa), quality.moments(fb), quality.kid_sums(fa, fb)
        end.record()
        end.synchronize()
        return start.elapsed_time(end) / passes, (ma, mb, sums)

    def sums_host_arm():
        """Copy the features, then ``np.cov`` of each set and the three float64 Gram products of KID."""
        t0 = time.perf_counter()
        xa, xb = fa.cpu().numpy().astype(np.float64), fb.cpu().numpy().astype(np.float64)
        ma, mb = (xa.mean(axis=0), np.cov(xa, rowvar=False)), (xb.mean(axis=0), np.cov(xb, rowvar=False))
        kaa, kbb, kab = (xa @ xa.T / width + 1) ** 3, (xb @ xb.T / width + 1) ** 3, (xa @ xb.T / width + 1) ** 3
        sums = (kaa.sum() - np.trace(kaa), kbb.sum() - np.trace(kbb), kab.sum())
        return (time.perf_counter() - t0) * 1e3, (ma, mb, sums)

    def frechet_arm():
        """The host part of ``compute``: two copies and ``frechet_from_moments`` (two symmetric eigensolves)."""
        (_, mean_a, cov_a), (_, mean_b, cov_b) = quality.moments(fa), quality.moments(fb)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fd = quality.frechet_from_moments(mean_a, cov_a, mean_b, cov_b)
        return (time.perf_counter() - t0) * 1e3, fd

    def update_arm():
        meter = quality.DistributionMeter(features, capacity=a.batch * (a.reps + a.warmup))
        for _ in range(a.warmup):
            meter.update(pred_d, target_d)
        torch.cuda.synchronize(dev)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(a.reps):
            meter.update(pred_d, target_d)
        end.record()
        end.synchronize()
        return start.elapsed_time(end) / a.reps, len(meter._bank[0])

    times = {"device_moments_and_kid_sums_ms": [], "host_cov_and_gram_ms": [], "host_frechet_ms": [], "update_ms": []}
    for rep in range(a.alternate):
        ms0, dev_res = timed(sums_arm, f"device moments + KID sums rep {rep}:",
                             lambda ms: f"{ms:.4f} ms per pass over {rows} + {rows} rows of {width} ({passes} passes between two events)")
        ms1, host_res = timed(sums_host_arm, f"host np.cov + Gram        rep {rep}:", lambda ms: f"{ms:.2f} ms (copy included)")
        ms2, fd = timed(frechet_arm, f"host frechet_from_moments rep {rep}:", lambda ms: f"{ms:.2f} ms (copy included)")
        ms3, _ = timed(update_arm, f"update through vits14     rep {rep}:",
                       lambda ms: f"{ms:.4f} ms per update of {a.batch} + {a.batch} images at {a.size}x{a.size} ({a.reps} updates between "
                                  "two events)")
        for k, ms in zip(times, (ms0, ms1, ms2, ms3)):
            times[k].append(ms)
        cov_gap = max(float(np.abs(d[2].cpu().numpy() - h[1]).max() / np.abs(h[1]).max()) for d, h in zip(dev_res[:2], host_res[:2]))
        sum_gap = max(abs(float(x) - float(y)) / abs(float(y)) for x, y in zip(dev_res[2].cpu().numpy(), host_res[2]))
        print(f"                          device against host: cov {cov_gap:.1e} of the largest entry, KID sums rel {sum_gap:.1e}; "
              f"fd {fd:.6g}", flush=True)
    summary = {k: {"mean": sum(v) / len(v), "min": min(v), "max": max(v), "repetitions": len(v)} for k, v in times.items()}
    print(json.dumps({"metric": f"set-level scores: moments + KID sums of {rows} + {rows} rows of {width} on the device against np.cov + "
                                f"float64 Gram products on the host; frechet_from_moments on the host; one DistributionMeter.update of "
                                f"{a.batch} + {a.batch} images at {a.size}x{a.size} through dinov2_vits14 (random weights); alternating",
                      "unit": "ms", "arms": summary,
                      "host_over_device": summary["host_cov_and_gram_ms"]["mean"] / summary["device_moments_and_kid_sums_ms"]["mean"]}))
    sys.exit(0)

times = {"device_batch_ms": [], "host_batch_ms": []}
for rep in range(a.alternate):
    clock = bench.ClockSampler(0)
    with clock:
        ms, res = device_arm()
    c = clock.summary()
    times["device_batch_ms"].append(ms)
    print(f"device  rep {rep}: {ms:.4f} ms per batch of {a.batch} ({a.reps} updates between two events)  sclk {c.get('sclk_mhz_mean')} MHz  "
          f"board {c.get('board_power_w_mean')} W", flush=True)
    clock = bench.ClockSampler(0)
    with clock:
        ms, rows = host_arm()
    c = clock.summary()
    times["host_batch_ms"].append(ms)
    print(f"host    rep {rep}: {ms:.2f} ms per batch of {a.batch} = {ms / a.batch:.2f} ms per image  sclk {c.get('sclk_mhz_mean')} MHz  "
          f"board {c.get('board_power_w_mean')} W", flush=True)
    gaps = [abs(res["per_image"][i, 0] - rows[i][0]) for i in range(a.batch)], [abs(res["per_image"][i, 1] - rows[i][1]) for i in range(a.batch)], \
        [abs(res["per_image"][i, 2] - rows[i][2]) / abs(rows[i][2]) for i in range(a.batch)]
    print(f"        device against host on this batch: |dPSNR| {max(gaps[0]):.1e} dB  |dSSIM| {max(gaps[1]):.1e}  UIQM rel {max(gaps[2]):.1e}",
          flush=True)
dev_worst, host_image_best = max(times["device_batch_ms"]), min(times["host_batch_ms"]) / a.batch
summary = {k: {"mean": sum(v) / len(v), "min": min(v), "max": max(v), "repetitions": len(v)} for k, v in times.items()}
ok = dev_worst < host_image_best
print(json.dumps({"metric": f"PSNR + SSIM + UIQM of one batch of {a.batch} at {a.size}x{a.size}, device against host, alternating",
                  "unit": "ms/batch", "arms": summary, "host_ms_per_image_min": host_image_best,
                  "device_batch_below_one_host_image": ok}))
sys.exit(0 if ok else 1)
