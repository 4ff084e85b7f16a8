"""The definition the device UCIQE kernels (csrc/uciqe.hip) are held to: the UCIQE part of the reference's ``nmetrics``
(metrics/metrics.py:301-337; ``hdiff_amd.uw_metrics.nmetrics`` is the host restatement) in float64, every operation and its order written
out, every sum a left-to-right loop, no BLAS.  The colour conversion is the one ``uw_metrics._srgb_to_lab`` restates (sRGB, D65, the
matrix and white point scikit-image uses).

``uciqe_def(x, scale)`` takes an fp32 ``[3, H, W]`` image: ``rgb = min(max(x, 0), 1) * scale`` with the clip in fp32 and everything
after it in double.  ``scale = 1`` is the measure on the image's colour range; ``scale = 255`` is what the reference's call evaluates
(rotinas.py:916, 923 hand ``nmetrics`` a float image in [0, 255], which the conversion takes as being in [0, 1] already)."""
import math

import numpy as np

MATRIX = ((0.412453, 0.357580, 0.180423), (0.212671, 0.715160, 0.072169), (0.019334, 0.119193, 0.950227))
WHITE = (0.95047, 1.0, 1.08883)
C_SC, C_CONL, C_US = 0.4680, 0.2745, 0.2576


def lab_def(rgb: np.ndarray):
    """(L, a, b) planes of float64 sRGB planes ``rgb[0..2]`` (nominally in [0, 1])."""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.float64 and rgb.shape[0] == 3
    with np.errstate(invalid="ignore"):
        lin = [np.where(v > 0.04045, ((v + 0.055) / 1.055) ** 2.4, v / 12.92) for v in rgb]
    f = []
    for row, white in zip(MATRIX, WHITE):
        t = (((row[0] * lin[0]) + (row[1] * lin[1])) + (row[2] * lin[2])) / white      # the three products, added left to right
        f.append(np.where(t > 0.008856, np.cbrt(t), (7.787 * t) + (16.0 / 116.0)))
    fx, fy, fz = f
    return (116.0 * fy) - 16.0, 500.0 * (fx - fy), 200.0 * (fy - fz)


def seq_sum(v) -> float:
    """Left-to-right sum in double."""
    total = 0.0
    for e in np.asarray(v, dtype=np.float64).reshape(-1).tolist():
        total += e
    return total


def top_count(H: int, W: int) -> int:
    """int(np.round(0.01 * H * W)): half to even, as Python's round() of a float also rounds."""
    return int(round(0.01 * H * W))


def uciqe_def(x: np.ndarray, scale: float = 1.0):
    """(sc, conl, us, uciqe) of an fp32 [3, H, W] image; conl and uciqe are NaN when the image has fewer than 50 pixels."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 3 and x.shape[0] == 3
    _, H, W = x.shape
    n = H * W
    clipped = np.minimum(np.maximum(x, np.float32(0)), np.float32(1))
    assert clipped.dtype == np.float32
    L, a, b = lab_def(clipped.astype(np.float64) * float(scale))
    L = L.reshape(-1)
    chroma = np.sqrt((a * a) + (b * b)).reshape(-1)
    uc = seq_sum(chroma) / n
    d = chroma - uc
    sc = math.sqrt(seq_sum(d * d) / n)                                # two passes, not sum(c^2) - n uc^2
    top = top_count(H, W)
    if top == 0:
        conl = float("nan")
    else:
        sl = np.sort(L, kind="stable")
        conl = (seq_sum(sl[::-1][:top]) / top) - (seq_sum(sl[:top]) / top)
    sat = []
    for c, l in zip(chroma.tolist(), L.tolist()):
        sat.append(0.0 if (c == 0.0 or l == 0.0) else c / l)
    us = seq_sum(sat) / n
    return sc, conl, us, ((C_SC * sc) + (C_CONL * conl)) + (C_US * us)
