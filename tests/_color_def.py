"""The definition the device colour-difference kernels (csrc/color_diff.hip) are held to: CIEDE2000, CIE76 and the angular error
between a prediction and its target, in float64, every operation and its order written out, every sum a left-to-right loop.

``color_def(p, t)`` takes two fp32 ``[3, H, W]`` images: ``rgb = min(max(x, 0), 1)`` with the clip in fp32 and everything after it in
double.  L*a*b* is ``_uciqe_def.lab_def`` (sRGB, D65), imported and not restated.

CIEDE2000 follows Sharma, Wu and Dalal, "The CIEDE2000 color-difference formula: implementation notes, supplementary test data, and
mathematical observations" (Color Research and Application 30, 2005) with kL = kC = kH = 1; ``tests/golden/ciede2000_sharma.json``
holds the 34 pairs of their supplementary table.  Seventh powers are taken by multiplications, hue is ``atan2(b, a') * (180 / pi)``
plus 360 where negative and 0 where ``a' == 0 and b == 0``, trigonometric arguments are ``degrees * (pi / 180)``.

The angular error is ``atan2(|u x v|, u . v) * (180 / pi)`` on the clipped RGB vectors -- not ``acos``, whose rounding noise at
parallel vectors is about 1e-6 degrees -- and a pixel counts when both vectors have a non-zero component.

The hue rules branch at a hue difference of exactly 180 degrees, and two pairs of the published table (rows 10 and 14: exactly
opposite chroma vectors) sit on that branch, where the last bit of the two angles decides the value.  numpy's ``arctan2`` returns the
correctly rounded angles at both, which is what puts them on the side the table prints; the device does not rely on such luck and
rounds its hue ``atan2`` correctly by construction (csrc/color_diff.hip: ``atan2_cr``)."""
import math

import numpy as np

from _uciqe_def import lab_def, seq_sum

R2D = 180.0 / math.pi
D2R = math.pi / 180.0
POW25_7 = 6103515625.0


def pow7(x):
    x2 = x * x
    x4 = x2 * x2
    return (x4 * x2) * x


def hue_def(b, ap):
    """h' in degrees, in [0, 360); 0 where both components are 0."""
    h = np.arctan2(b, ap) * R2D
    h = np.where(h < 0.0, h + 360.0, h)
    return np.where((ap == 0.0) & (b == 0.0), 0.0, h)


def ciede2000_terms(L1, a1, b1, L2, a2, b2):
    """Every intermediate of the formula, as a dict of float64 arrays shaped like the inputs; "de00" is the result."""
    L1, a1, b1, L2, a2, b2 = (np.asarray(v, dtype=np.float64) for v in (L1, a1, b1, L2, a2, b2))
    c1 = np.sqrt((a1 * a1) + (b1 * b1))
    c2 = np.sqrt((a2 * a2) + (b2 * b2))
    cb7 = pow7((c1 + c2) / 2.0)
    g = 0.5 * (1.0 - np.sqrt(cb7 / (cb7 + POW25_7)))
    ap1 = (1.0 + g) * a1
    ap2 = (1.0 + g) * a2
    cp1 = np.sqrt((ap1 * ap1) + (b1 * b1))
    cp2 = np.sqrt((ap2 * ap2) + (b2 * b2))
    h1 = hue_def(b1, ap1)
    h2 = hue_def(b2, ap2)
    dl = L2 - L1
    dc = cp2 - cp1
    cc = cp1 * cp2
    d = h2 - h1
    dh = np.where(cc == 0.0, 0.0, np.where(np.abs(d) <= 180.0, d, np.where(d > 180.0, d - 360.0, d + 360.0)))
    dH = (2.0 * np.sqrt(cc)) * np.sin((dh / 2.0) * D2R)
    lb = (L1 + L2) / 2.0
    cb = (cp1 + cp2) / 2.0
    hs = h1 + h2
    hb = np.where(cc == 0.0, hs, np.where(np.abs(h1 - h2) <= 180.0, hs / 2.0, np.where(hs < 360.0, (hs + 360.0) / 2.0,
                                                                                        (hs - 360.0) / 2.0)))
    t = (((1.0 - (0.17 * np.cos((hb - 30.0) * D2R))) + (0.24 * np.cos((2.0 * hb) * D2R)))
         + (0.32 * np.cos(((3.0 * hb) + 6.0) * D2R))) - (0.20 * np.cos(((4.0 * hb) - 63.0) * D2R))
    q = (hb - 275.0) / 25.0
    dtheta = 30.0 * np.exp(-(q * q))
    cbp7 = pow7(cb)
    rc = 2.0 * np.sqrt(cbp7 / (cbp7 + POW25_7))
    l50 = (lb - 50.0) * (lb - 50.0)
    sl = 1.0 + ((0.015 * l50) / np.sqrt(20.0 + l50))
    sc = 1.0 + (0.045 * cb)
    sh = 1.0 + ((0.015 * cb) * t)
    rt = -np.sin((2.0 * dtheta) * D2R) * rc
    tl = dl / sl
    tc = dc / sc
    th = dH / sh
    de = np.sqrt((((tl * tl) + (tc * tc)) + (th * th)) + ((rt * tc) * th))
    return {"de00": de, "h1": h1, "h2": h2, "cc": cc, "dh": dh, "hb": hb}


def ciede2000_lab_def(lab1, lab2) -> np.ndarray:
    """Delta E00 of ``[n, 3]`` float64 Lab rows -> ``[n]``."""
    lab1, lab2 = np.asarray(lab1, dtype=np.float64), np.asarray(lab2, dtype=np.float64)
    assert lab1.ndim == 2 and lab1.shape[1] == 3 and lab1.shape == lab2.shape
    return ciede2000_terms(lab1[:, 0], lab1[:, 1], lab1[:, 2], lab2[:, 0], lab2[:, 1], lab2[:, 2])["de00"]


def clipped(x: np.ndarray) -> np.ndarray:
    """min(max(x, 0), 1) in fp32, then double."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 3 and x.shape[0] == 3
    c = np.minimum(np.maximum(x, np.float32(0)), np.float32(1))
    assert c.dtype == np.float32
    return c.astype(np.float64)


def angle_def(u: np.ndarray, v: np.ndarray):
    """(angle in degrees, valid) per pixel of float64 ``[3, ...]`` vectors."""
    cx = (u[1] * v[2]) - (u[2] * v[1])
    cy = (u[2] * v[0]) - (u[0] * v[2])
    cz = (u[0] * v[1]) - (u[1] * v[0])
    cross = np.sqrt(((cx * cx) + (cy * cy)) + (cz * cz))
    dot = ((u[0] * v[0]) + (u[1] * v[1])) + (u[2] * v[2])
    valid = ((u[0] != 0.0) | (u[1] != 0.0) | (u[2] != 0.0)) & ((v[0] != 0.0) | (v[1] != 0.0) | (v[2] != 0.0))
    return np.arctan2(cross, dot) * R2D, valid


def pixels_def(p: np.ndarray, t: np.ndarray):
    """(de00, de76, angle, valid, terms) per pixel, ``[H, W]`` each, of two finite fp32 ``[3, H, W]`` images."""
    u, v = clipped(p), clipped(t)
    assert u.shape == v.shape
    L1, a1, b1 = lab_def(u)
    L2, a2, b2 = lab_def(v)
    dl, da, db = L2 - L1, a2 - a1, b2 - b1
    de76 = np.sqrt(((dl * dl) + (da * da)) + (db * db))
    terms = ciede2000_terms(L1, a1, b1, L2, a2, b2)
    angle, valid = angle_def(u, v)
    return terms["de00"], de76, angle, valid, terms


def p95_index(n: int) -> int:
    """Nearest rank: the index of the 95th percentile in the ascending sort of n samples."""
    return (95 * n + 99) // 100 - 1


def color_def(p: np.ndarray, t: np.ndarray):
    """(de00, de00_p95, de76, angular) of two fp32 ``[3, H, W]`` images; a non-finite value in either makes all four NaN."""
    p, t = np.asarray(p), np.asarray(t)
    if not (np.isfinite(p).all() and np.isfinite(t).all()):
        return (float("nan"),) * 4
    de00, de76, angle, valid, _ = pixels_def(p, t)
    n = de00.size
    flat = de00.reshape(-1)
    p95 = float(np.sort(flat, kind="stable")[p95_index(n)])
    count = int(valid.sum())
    angular = seq_sum(angle.reshape(-1)[valid.reshape(-1)]) / count if count else float("nan")
    return seq_sum(flat) / n, p95, seq_sum(de76) / n, angular


# The image pairs the GPU tests compare, (H, W, seed, near): prediction and target drawn independently, or, for `near`, the target a
# noisy copy of the prediction.  tests/test_color_cpu.py holds every one of them to its hue-branch margins.
FIXTURES = ((8, 13, 2000, False), (33, 47, 2003, False), (72, 120, 2001, False), (72, 120, 2002, True),
            (8, 13, 2004, True), (33, 47, 2005, True))      # the last two fill the batches of three at the small sizes


def fixture(H: int, W: int, seed: int, near: bool = False):
    """(prediction, target), fp32 ``[3, H, W]``."""
    rng = np.random.default_rng(seed)
    p = rng.random((3, H, W), dtype=np.float32)
    if near:
        t = p + np.float32(0.05) * rng.standard_normal((3, H, W)).astype(np.float32)
        assert t.dtype == np.float32
        return p, t
    return p, rng.random((3, H, W), dtype=np.float32)
