"""The fixtures tests/test_synth_cpu.py and tests/test_gpu_synth.py share: the settings, shapes, batches and epochs the kernels are
compared at, and the bridge from a ``Synth`` to the plain dict tests/_synth_def.py takes.  Every fixture without sensor noise has its
rounding margin checked on the host (test_synth_cpu.py); the noisy ones need the device's noise and are checked where it is drawn."""
import numpy as np

from hdiff_amd import synth as SY

SEED = 20240917
N_CACHE = 9
IDX7 = (5, 2, 8, 2, 0, 7, 3)          # non-monotone, one entry twice
IDX1 = (4,)
SHAPES = ((1, 1), (3, 5), (8, 13), (32, 32))
EPOCHS = (0, 1, 2 ** 31 - 1)
MARGIN = 1e-9

VARIANTS = {
    "underwater": SY.Synth.underwater(),                                   # the medium alone, a water type per sample
    "haze": SY.Synth.haze(),                                               # the medium alone, one beta
    "exposure": SY.Synth(gamma=(1.5, 3.0), gain=(0.3, 0.9)),               # the exposure curve alone
    "noise": SY.Synth(shot=(0.001, 0.01), read=(0.002, 0.02)),             # the sensor noise alone
    "all": SY.Synth.underwater(gamma=(0.7, 1.6), gain=(0.6, 1.1), shot=(0.0, 0.01), read=(0.0, 0.02)),
    "mixed": SY.Synth.underwater(gamma=(0.7, 1.6), gain=(0.6, 1.1), shot=(0.0, 0.01), read=(0.0, 0.02), p_medium=0.6, p_exposure=0.5,
                                 p_noise=0.5),
}
NOISY = ("noise", "all", "mixed")


def settings_of(s: SY.Synth) -> dict:
    return {"type_beta": [b for _, b in s.type_betas()], "beta": s.beta, "airlight": s.airlight, "veil": s.veil, "depth": s.range_m,
            "field_mean": s.field_mean, "field_grad": s.field_grad, "field_amp": s.field_amp, "gamma": s.gamma, "gain": s.gain,
            "shot": s.shot, "read": s.read}


def cache_images(H: int, W: int) -> np.ndarray:
    """The clean cache of a fixture: uint8 [N_CACHE, 3, H, W], the extremes 0 and 255 included."""
    a = np.random.default_rng([SEED, H, W]).integers(0, 256, (N_CACHE, 3, H, W), dtype=np.uint8)
    a[0, :, 0, 0] = (0, 255, 128)
    return a


def fixtures():
    """``(name, variant, H, W, idx, epoch)``: every variant at every shape with the batch of 7, the epochs in rotation; the batch of 1
    at every shape and epoch with all stages on."""
    out, k = [], 0
    for H, W in SHAPES:
        for v in VARIANTS:
            e = EPOCHS[k % len(EPOCHS)]
            k += 1
            out.append((f"{v}-{H}x{W}-B7-e{e}", v, H, W, IDX7, e))
        for e in EPOCHS:
            out.append((f"all-{H}x{W}-B1-e{e}", "all", H, W, IDX1, e))
    return out
