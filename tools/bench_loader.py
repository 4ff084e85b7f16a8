"""What feeds ``diffusion.Train.train``, two ways, ALTERNATELY inside one process, engine clock and board power sampled beside each
timing (bench.ClockSampler), on a synthetic paired set written to a temporary directory (LoLI layout; ``--files`` JPEGs in all, half
degraded and half reference, made with PIL from a fixed generator) at ``--size`` (default 4032x3024, the HDR+ gallery's 12 megapixels)
and the same again at 256x256:

  (a) host: the ``DataLoader`` as ``train`` builds it (the sets' default transform = decode + resize to 256x256, ``--workers`` workers,
      ``pin_memory``, ``drop_last``) with ``.to(device)`` per batch, one whole epoch by the wall clock after a synchronise, images/s;
  (b) device: ``device_data.DeviceLoader`` over the cache of the same set, without and with augmentation (both flips, quarter turns,
      crops from half the height, shuffled), ``--reps`` epochs between two device events (the default makes the window about half a
      second), images/s.  The launches are issued from Python one batch at a time, as the driver issues them: the figure is the rate
      at which batches can be had, not the kernel's own time.

The one-off ``build_cache`` of each set is timed too.  An image is one 3 x 256 x 256 array: a pair counts two, so the figures set
against the 78 images/s that the measured 51.18 ms step of the default DynamicUNet at 256x256, batch 2 consumes
(profiles/train_b_ema.txt).

    python tools/bench_loader.py [--files 64] [--size 4032x3024] [--alternate 3] [--batch 2] [--workers 4] [--reps 2000]

``--synth`` measures the synthetic degradation (hdiff_amd/synth.py) instead: a clean-only cache of ``--files`` procedural scenes at
256x256 (no files), and ``DeviceLoader`` without the generator, with ``Synth.underwater()`` plus sensor noise (every stage on, every
sample selected) and with that behind the augmentation, alternating in the same way.  ``synth.degrade`` alone on a resident batch is
timed too, which is the two kernels without the Python around the loader.

    python tools/bench_loader.py --synth [--files 64] [--alternate 3] [--batch 2] [--reps 2000]

Prints one line per timing and one JSON summary line.  No condition is checked: the figures are the result."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import hdiff_amd  # noqa: E402,F401
import bench  # noqa: E402
from hdiff_amd import device_data as DD  # noqa: E402
from hdiff_amd.datasets import Atmospheric_Dataset  # noqa: E402

STEP_MS, STEP_IMAGES = 51.18, 4            # profiles/train_b_ema.txt: one optimizer step at 256x256, batch 2 = 2 pairs

ap = argparse.ArgumentParser()
ap.add_argument("--files", type=int, default=64, help="JPEGs per set: half degraded, half reference")
ap.add_argument("--size", default="4032x3024", help="WxH of the large set")
ap.add_argument("--alternate", type=int, default=3)
ap.add_argument("--batch", type=int, default=2, help="pairs per batch")
ap.add_argument("--workers", type=int, default=4)
ap.add_argument("--reps", type=int, default=2000, help="epochs between the two device events of a device arm")
ap.add_argument("--synth", action="store_true", help="the synthetic-degradation arms on procedural scenes, no host arms")
a = ap.parse_args()
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
big_w, big_h = (int(v) for v in a.size.lower().split("x"))
pairs = a.files // 2


def write_set(root: str, width: int, height: int) -> float:
    """``pairs`` image-like pairs (smooth colour fields, coarse noise, the degraded side darker) as JPEGs; returns the mean file size."""
    from PIL import Image
    rng = np.random.default_rng(0)
    yy, xx = np.meshgrid(np.linspace(0, 1, height, dtype=np.float32), np.linspace(0, 1, width, dtype=np.float32), indexing="ij")
    total = 0
    for sub in ("Train/low", "Train/high"):
        os.makedirs(os.path.join(root, sub))
    for i in range(pairs):
        base = np.stack([0.5 + 0.4 * np.sin(7 * xx + c + i) * np.cos(5 * yy - c) for c in range(3)], axis=-1)
        noise = Image.fromarray(rng.integers(0, 256, (min(height, 378), min(width, 504), 3), dtype=np.uint8))
        noise = noise.resize((width, height), Image.BILINEAR)
        high = np.clip(base * 255 * 0.8 + np.asarray(noise, dtype=np.float32) * 0.2, 0, 255).astype(np.uint8)
        low = (high.astype(np.float32) * 0.35).astype(np.uint8)
        for sub, img in (("Train/low", low), ("Train/high", high)):
            path = os.path.join(root, sub, f"img{i:03d}.jpg")
            Image.fromarray(img).save(path, quality=90)
            total += os.path.getsize(path)
    return total / (2 * pairs)


def timed(arm, label):
    clock = bench.ClockSampler(0)
    with clock:
        rate, note = arm()
    c = clock.summary()
    print(f"{label} {rate:10.1f} images/s  ({note})  sclk {c.get('sclk_mhz_mean')} MHz  board {c.get('board_power_w_mean')} W", flush=True)
    return rate


def host_arm(data):
    from torch.utils.data import DataLoader
    loader = DataLoader(data, batch_size=a.batch, num_workers=a.workers, drop_last=True, pin_memory=True)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    n, first = 0, None
    for inp, label in loader:                       # the workers start inside the timing: they do at every epoch of the driver
        inp, label = inp.to(dev), label.to(dev)
        n += inp.shape[0] + label.shape[0]
        if first is None:
            first = time.perf_counter() - t0
    torch.cuda.synchronize(dev)
    s = time.perf_counter() - t0
    return n / s, f"one epoch of {n} images in {s:.2f} s by the wall clock, the first batch after {first:.2f} s"


def device_arm(loader):
    for _ in loader:                                # warm-up epoch
        pass
    torch.cuda.synchronize(dev)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 0
    start.record()
    for e in range(a.reps):
        loader.set_epoch(e)
        for inp, label in loader:
            n += inp.shape[0] + label.shape[0]
    end.record()
    end.synchronize()
    ms = start.elapsed_time(end)
    return n / (ms * 1e-3), f"{a.reps} epochs = {n} images in {ms:.1f} ms between two device events, {ms / (a.reps * len(loader)) * 1e3:.0f} us per batch"


def synth_arms():
    from hdiff_amd import synth as SY
    clean = torch.from_numpy(SY.procedural_scenes(a.files, 256, 256, seed=0))
    cache = DD.PairCache(clean, clean, None, "procedural").to(dev)
    s = SY.Synth.underwater(gamma=(0.7, 1.6), gain=(0.6, 1.1), shot=(0.0, 0.01), read=(0.0, 0.02))
    augment = DD.Augment(hflip=0.5, vflip=0.5, rot90=True, crop=0.5, crop_min=0.5)
    loaders = {"device_plain": DD.DeviceLoader(cache, a.batch),
               "device_synth": DD.DeviceLoader(cache, a.batch, synth=s),
               "device_augmented_synth": DD.DeviceLoader(cache, a.batch, shuffle=True, augment=augment, seed=1, synth=s)}
    idx = torch.arange(a.files, dtype=torch.int64, device=dev)
    label, out = cache.a.clone(), torch.empty_like(cache.a)

    def kernels_arm():
        SY.degrade(label, idx, synth=s, seed=1, epoch=0, out=out)
        torch.cuda.synchronize(dev)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = max(a.reps // 20, 1)
        start.record()
        for e in range(reps):
            SY.degrade(label, idx, synth=s, seed=1, epoch=e, out=out)
        end.record()
        end.synchronize()
        ms = start.elapsed_time(end)
        return reps * a.files / (ms * 1e-3), f"{reps} batches of {a.files} images in {ms:.1f} ms, {ms / reps * 1e3:.0f} us per batch of two launches"

    rates = {k: [] for k in loaders}
    rates["degrade_alone"] = []
    for rep_ in range(a.alternate):
        for k, loader in loaders.items():
            rates[k].append(timed(lambda: device_arm(loader), f"{k:>22} rep {rep_}:"))
        rates["degrade_alone"].append(timed(kernels_arm, f"{'degrade_alone':>22} rep {rep_}:"))
    consumed = STEP_IMAGES / (STEP_MS * 1e-3)
    summary = {k: {"mean": sum(v) / len(v), "min": min(v), "max": max(v), "repetitions": len(v)} for k, v in rates.items()}
    print(json.dumps({"metric": f"images/s of device_data.DeviceLoader at 256x256, batch {a.batch} pairs, over {a.files} procedural scenes: "
                                "without the synthetic degradation, with it, and with it behind the augmentation, alternating; "
                                "degrade_alone counts degraded images of one resident batch",
                      "unit": "images/s", "arms": summary, "step_consumes_images_per_s": consumed,
                      "over_the_step": {k: v["mean"] / consumed for k, v in summary.items()}}))


if a.synth:
    synth_arms()
    sys.exit(0)

with tempfile.TemporaryDirectory() as tmp:
    sets, caches, build_s = {}, {}, {}
    for name, (w, h) in (("large", (big_w, big_h)), ("small", (256, 256))):
        t0 = time.perf_counter()
        mean_bytes = write_set(os.path.join(tmp, name), w, h)
        print(f"wrote {2 * pairs} JPEGs of {w}x{h} ({mean_bytes / 1e6:.2f} MB each) in {time.perf_counter() - t0:.1f} s", flush=True)
        sets[name] = Atmospheric_Dataset("LoLI", task="train", root=os.path.join(tmp, name))
    for name, data in sets.items():
        t0 = time.perf_counter()
        cache = DD.build_cache(data, num_workers=a.workers)
        build_s[name] = time.perf_counter() - t0
        caches[name] = cache.to(dev)
        print(f"build_cache {name}: {build_s[name]:.2f} s once for {2 * len(cache)} images = {2 * len(cache) / build_s[name]:.1f} images/s "
              f"({a.workers} workers; {tuple(cache.a.shape)} uint8 per side, {2 * cache.a.numel() / 1e6:.1f} MB on the device)", flush=True)
    augment = DD.Augment(hflip=0.5, vflip=0.5, rot90=True, crop=0.5, crop_min=0.5)
    plain = DD.DeviceLoader(caches["large"], a.batch)
    augmented = DD.DeviceLoader(caches["large"], a.batch, shuffle=True, augment=augment, seed=1)
    rates = {"host_large": [], "host_small": [], "device_plain": [], "device_augmented": []}
    for rep in range(a.alternate):
        rates["host_large"].append(timed(lambda: host_arm(sets["large"]), f"host   {a.size:>9} rep {rep}:"))
        rates["host_small"].append(timed(lambda: host_arm(sets["small"]), f"host     256x256 rep {rep}:"))
        rates["device_plain"].append(timed(lambda: device_arm(plain), f"device     plain rep {rep}:"))
        rates["device_augmented"].append(timed(lambda: device_arm(augmented), f"device augmented rep {rep}:"))

consumed = STEP_IMAGES / (STEP_MS * 1e-3)
summary = {k: {"mean": sum(v) / len(v), "min": min(v), "max": max(v), "repetitions": len(v)} for k, v in rates.items()}
print(json.dumps({"metric": f"images/s of what feeds diffusion.Train.train at 256x256, batch {a.batch} pairs: host DataLoader ({a.workers} "
                            f"workers) on {a.size} and 256x256 JPEGs against device_data.DeviceLoader, alternating",
                  "unit": "images/s", "arms": summary, "build_cache_s": build_s, "files_per_set": 2 * pairs,
                  "step_consumes_images_per_s": consumed,
                  "over_the_step": {k: v["mean"] / consumed for k, v in summary.items()}}))
