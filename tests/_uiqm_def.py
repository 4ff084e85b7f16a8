"""The definition the device UIQM kernels (csrc/quality.hip) are held to, in numpy, and the test images both quality test files use.

``uiqm_def`` restates ``hdiff_amd.uw_metrics.getUIQM`` (pinned to the reference's functions by tests/golden/uw_metrics.npz) with fp32
roundings at the same places and ONE difference: the trimmed means of UICM add the kept samples in float64, where the reference adds
them one by one in fp32.  The Sobel filter is written out (one fp32 subtraction with the border pixel repeated, then [1, 2, 1]
formed exactly and rounded once); tests/test_quality_cpu.py checks that this is scipy's ``ndimage.sobel`` on an fp32 plane."""
import math

import numpy as np

SIZES = ((16, 24), (19, 27), (40, 71))
KINDS = ("smooth", "noise", "sat", "ties")


def image(kind: str, H: int, W: int) -> np.ndarray:
    """[H, W, 3] fp32 in [0, 1]."""
    k = KINDS.index(kind)
    rng = np.random.default_rng(100 * H + k)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    base = np.stack([0.5 + 0.4 * np.sin(x / 5 + c) * np.cos(y / 7 - c) for c in range(3)], axis=-1)
    g = 0.05 * rng.standard_normal((H, W, 3))
    if kind == "smooth":
        img = base + g
    elif kind == "noise":
        img = rng.random((H, W, 3))
    elif kind == "sat":
        img = 1.8 * base - 0.4 + g
    else:
        img = np.round(np.clip(base + g, 0, 1) * 15) / 15
    return np.clip(img, 0, 1).astype(np.float32)


def images(H: int, W: int):
    """The four kinds at one size, in KINDS order."""
    return [image(k, H, W) for k in KINDS]


def scaled(img01: np.ndarray) -> np.ndarray:
    """What the reference's metric calls receive (rotinas.py:918): np.clip(img, 0, 1) * 255 as an fp32 image."""
    return (np.clip(np.asarray(img01, dtype=np.float32), 0, 1) * np.float32(255)).astype(np.float32)


def _seq_sum(v) -> float:
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    return float(np.cumsum(v)[-1]) if v.size else 0.0


def trimmed_mean(v: np.ndarray) -> np.float32:
    v = np.sort(v.reshape(-1), kind="stable")
    K = v.size
    t_l, t_r = math.ceil(0.1 * K), math.floor(0.1 * K)
    kept = v[t_l + 1:K - t_r]
    return np.float32(np.float64(np.float32(1 / (K - t_l - t_r))) * _seq_sum(kept))


def uicm_def(x: np.ndarray) -> float:
    R, G, B = (x[:, :, c].reshape(-1) for c in range(3))
    rg = R - G
    yb = ((R + G) / np.float32(2)) - B
    assert rg.dtype == np.float32 and yb.dtype == np.float32
    mu_rg, mu_yb = trimmed_mean(rg), trimmed_mean(yb)
    var_rg = _seq_sum((rg - mu_rg).astype(np.float64) ** 2) / rg.size
    var_yb = _seq_sum((yb - mu_yb).astype(np.float64) ** 2) / yb.size
    return (-0.0268 * math.sqrt(float(mu_rg) ** 2 + float(mu_yb) ** 2)) + (0.1586 * math.sqrt(var_rg + var_yb))


def sobel_def(p: np.ndarray, axis: int) -> np.ndarray:
    """ndimage.sobel(p, axis) on an fp32 plane."""
    assert p.dtype == np.float32
    e = np.pad(p, 1, mode="edge")
    if axis == 0:
        d = e[2:, :] - e[:-2, :]                                   # [H, W + 2], fp32
        d = d.astype(np.float64)
        return (2.0 * d[:, 1:-1] + (d[:, :-2] + d[:, 2:])).astype(np.float32)
    d = (e[:, 2:] - e[:, :-2]).astype(np.float64)                  # [H + 2, W]
    return (2.0 * d[1:-1, :] + (d[:-2, :] + d[2:, :])).astype(np.float32)


def eme_def(t: np.ndarray) -> float:
    H, W = t.shape
    lo = np.array([[t[i:i + 8, j:j + 8].min() for j in range(0, W, 8)] for i in range(0, H, 8)], dtype=np.float64)
    hi = np.array([[t[i:i + 8, j:j + 8].max() for j in range(0, W, 8)] for i in range(0, H, 8)], dtype=np.float64)
    lo = np.where(lo == 0, lo + 1, lo)
    hi = np.where(hi == 0, hi + 1, hi)
    with np.errstate(all="ignore"):
        return float((2.0 / lo.size) * np.log(hi / lo).sum())


def uism_def(x: np.ndarray) -> float:
    vals = []
    for c in range(3):
        p = x[:, :, c]
        with np.errstate(all="ignore"):
            mag = np.hypot(sobel_def(p, 0), sobel_def(p, 1))
            s = np.float32(255.0) / np.max(mag)
            t = (mag * s) * p
        assert t.dtype == np.float32
        vals.append(eme_def(t))
    return (0.299 * vals[0]) + (0.587 * vals[1]) + (0.144 * vals[2])


def uiconm_def(x: np.ndarray) -> float:
    H, W = x.shape[:2]
    total, n = 0.0, 0
    for j in range(W // 8):                        # column by column, as the reference loops
        for i in range(H // 8):
            blk = x[8 * i:8 * i + 8, 8 * j:8 * j + 8, :]
            hi, lo = blk.max(), blk.min()
            top, bot = hi - lo, hi + lo
            n += 1
            if top == 0 or bot == 0:
                continue
            r = np.float64(top / bot)
            total += r * np.log(r)
    return float((-1.0 / n) * total)


def uiqm_def(x255: np.ndarray):
    """(uicm, uism, uiconm, uiqm) of an fp32 [H, W, 3] image with values in [0, 255]."""
    x = np.asarray(x255)
    assert x.dtype == np.float32
    a, b, c = uicm_def(x), uism_def(x), uiconm_def(x)
    return a, b, c, (0.0282 * a) + (0.2953 * b) + (3.5753 * c)
