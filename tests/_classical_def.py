"""The definition ``csrc/classical.hip`` is held to: the dark-channel prior (He, Sun, Tang 2009), its underwater variant over G and
B (Drews et al. 2013), the inverted-image form for low light (Dong et al. 2011) and gray-world / shades-of-gray white balance, in
numpy with every operation and its order written out.  Images are fp32 ``[3, H, W]``; ``f32(.)`` is ONE rounding of a float64 value.

    X        = min(max(I, 0), 1) in fp32                      ("inverted_dcp": X = f32(1 - that), and the result is f32(1 - J))
    D[y, x]  = min over the channel set and the (2 r + 1)^2 window clipped at the border of X,  r = patch // 2
    n_top    = max(1, floor(top * H * W));  cut = element H W - n_top of the ascending sort of D
    airlight = the pixel with D >= cut of the largest (f64(X_R) + f64(X_G)) + f64(X_B), the lowest linear index at equal sums;
               A_c = max(X_c there, f32(1 / 255)); an airlight given by the caller is held to the same floor
    M        = min over the channel set of f32(f64(X_c) / f64(A_c))
    t_raw    = f32(1 - omega * f64(windowmin(M)))
    J_c      = f32(clamp((f64(X_c) - f64(A_c)) / max(f64(t), t0) + f64(A_c), 0, 1))
    white balance: m_c = (mean of f64(X_c)^p)^(1 / p) (the mean itself at p = 1, the maximum at p = inf),
               g_c = ((m_0 + m_1) + m_2) / 3 / max(m_c, 1e-6),  out_c = f32(clamp(f64(X_c) * g_c, 0, 1))
A minimum is exact and every other value above is one correctly rounded IEEE operation after another, so the kernels are held bit for
bit on D, cut, A and t_raw and to the fp32 value or its neighbour on M and J; the white-balance sums are float64 sums in numpy's
order, which the kernels' fixed-order sums meet to 1e-11 relative."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
CHANNELS = {"rgb": (0, 1, 2), "gb": (1, 2)}
PRIORS = {"dcp": ("rgb", False), "udcp": ("gb", False), "inverted_dcp": ("rgb", True)}


def clipped(img) -> np.ndarray:
    """min(max(I, 0), 1) in fp32."""
    img = np.asarray(img)
    assert img.dtype == np.float32 and img.ndim == 3 and img.shape[0] == 3
    return np.minimum(np.maximum(img, f32(0.0)), f32(1.0))


def window_min(plane: np.ndarray, patch: int) -> np.ndarray:
    """The minimum over the (2 r + 1)^2 window clipped at the border, pixel by pixel."""
    assert patch % 2 == 1 and 1 <= patch <= 63
    r = patch // 2
    H, W = plane.shape
    rows = np.empty_like(plane)
    for x in range(W):
        rows[:, x] = plane[:, max(0, x - r):min(W, x + r + 1)].min(axis=1)
    out = np.empty_like(plane)
    for y in range(H):
        out[y] = rows[max(0, y - r):min(H, y + r + 1)].min(axis=0)
    return out


def dark_channel_def(x: np.ndarray, patch: int, channels: str = "rgb") -> np.ndarray:
    """``x``: clipped fp32 ``[3, H, W]`` -> fp32 ``[H, W]``."""
    return window_min(x[list(CHANNELS[channels])].min(axis=0), patch)


def n_top_of(top: float, H: int, W: int) -> int:
    return max(1, int(math.floor(top * H * W)))


def airlight_def(x: np.ndarray, dark: np.ndarray, n_top: int):
    """-> (A fp32 ``[3]``, cut fp32, the airlight pixel's linear index)."""
    HW = dark.size
    assert 1 <= n_top <= HW
    cut = np.sort(dark.reshape(-1), kind="stable")[HW - n_top]
    flat = x.reshape(3, -1).astype(f64)
    total = (flat[0] + flat[1]) + flat[2]
    cand = np.flatnonzero(dark.reshape(-1) >= cut)
    best = cand[np.argmax(total[cand])]          # argmax returns the first of equal maxima: the lowest index
    A = np.maximum(x.reshape(3, -1)[:, best], f32(1.0 / 255.0))
    return A.astype(f32), f32(cut), int(best)


def transmission_def(x: np.ndarray, A: np.ndarray, patch: int, omega: float, channels: str = "rgb"):
    """-> (M, t_raw), fp32 ``[H, W]`` each."""
    ch = list(CHANNELS[channels])
    ratio = (x[ch].astype(f64) / np.asarray(A, dtype=f32)[ch].astype(f64)[:, None, None]).astype(f32)
    M = ratio.min(axis=0)
    t_raw = (f64(1.0) - f64(omega) * window_min(M, patch).astype(f64)).astype(f32)
    return M, t_raw


def recover_def(x: np.ndarray, A: np.ndarray, t: np.ndarray, t0: float) -> np.ndarray:
    a = np.asarray(A, dtype=f32).astype(f64)[:, None, None]
    j = ((x.astype(f64) - a) / np.maximum(t.astype(f64), f64(t0))[None]) + a
    return np.minimum(np.maximum(j, 0.0), 1.0).astype(f32)


def dehaze_def(img, *, prior: str = "dcp", patch: int = 15, omega: float = 0.95, t0: float = 0.1, top: float = 1e-3, airlight=None,
               refine=None) -> dict:
    """One fp32 ``[3, H, W]`` image -> dict of ``J``, ``dark``, ``A``, ``cut``, ``index``, ``M``, ``t_raw``, ``t``.  ``refine``: None, or a
    callable ``(X, t_raw) -> t`` (the guided filter is ``hdiff_amd.transfer``'s own and has its own definition)."""
    channels, invert = PRIORS[prior]
    x = clipped(img)
    if invert:
        x = f32(1.0) - x
    H, W = x.shape[1:]
    dark = dark_channel_def(x, patch, channels)
    cut = index = None
    if airlight is None:
        A, cut, index = airlight_def(x, dark, n_top_of(top, H, W))
    else:
        A = np.maximum(np.asarray(airlight, dtype=f32), f32(1.0 / 255.0))      # an override is held to the same floor
    M, t_raw = transmission_def(x, A, patch, omega, channels)
    t = t_raw if refine is None else refine(x, t_raw)
    J = recover_def(x, A, t, t0)
    if invert:
        J = f32(1.0) - J
    return {"J": J, "dark": dark, "A": A, "cut": cut, "index": index, "M": M, "t_raw": t_raw, "t": t}


def white_balance_def(img, p: float = 1.0):
    """-> (out fp32 ``[3, H, W]``, gains float64 ``[3]``)."""
    assert p >= 1.0
    x = clipped(img).astype(f64)
    flat = x.reshape(3, -1)
    if math.isinf(p):
        m = flat.max(axis=1)
    elif p == 1.0:
        m = flat.sum(axis=1) / f64(flat.shape[1])
    else:
        m = np.power(np.power(flat, f64(p)).sum(axis=1) / f64(flat.shape[1]), f64(1.0) / f64(p))
    gray = ((m[0] + m[1]) + m[2]) / f64(3.0)
    g = gray / np.maximum(m, f64(1e-6))
    out = np.minimum(np.maximum(x * g[:, None, None], 0.0), 1.0).astype(f32)
    return out, g


def neighbours_ok(got: np.ndarray, want: np.ndarray):
    """(all within one fp32 step of ``want``, the count that differs at all) for finite fp32 arrays."""
    got, want = np.asarray(got, dtype=f32), np.asarray(want, dtype=f32)
    lo, hi = np.nextafter(want, f32(-np.inf)), np.nextafter(want, f32(np.inf))
    return bool(((got >= lo) & (got <= hi)).all()), int((got != want).sum())


# ---------------------------------------------------------------------------------------------------------------- scores and fixtures
def psnr(a01: np.ndarray, b01: np.ndarray) -> float:
    mse = float(np.mean((np.asarray(a01, f64) - np.asarray(b01, f64)) ** 2))
    return 10.0 * math.log10(1.0 / mse) if mse > 0 else float("inf")


def angular_error(a01: np.ndarray, b01: np.ndarray) -> float:
    """Mean angle in degrees between the RGB vectors of two ``[3, H, W]`` images, over the pixels where neither is black."""
    u, v = np.asarray(a01, f64).reshape(3, -1), np.asarray(b01, f64).reshape(3, -1)
    ok = (np.abs(u).sum(0) > 0) & (np.abs(v).sum(0) > 0)
    u, v = u[:, ok], v[:, ok]
    cross = np.linalg.norm(np.cross(u.T, v.T), axis=1)
    return float(np.degrees(np.arctan2(cross, (u * v).sum(0))).mean())


def scene_sets(n: int = 8, side: int = 64, seed: int = 11, table_seed: int = 5):
    """The procedural fixtures of the effect tests: ``{name: (clean01, degraded01)}``, fp32 ``[n, 3, side, side]`` each, for the haze,
    the noise-free low-light and the underwater settings, degraded by the synthetic degradation's own definition."""
    import _synth_def as SD
    from _synth_fixtures import settings_of
    from hdiff_amd import synth as SY
    clean = SY.procedural_scenes(n, side, side, seed)
    kinds = {"haze": SY.Synth.haze(), "lowlight": SY.Synth(gamma=(1.5, 3.0), gain=(0.3, 0.9)), "underwater": SY.Synth.underwater()}
    out = {}
    for name, s in kinds.items():
        table = SD.param_table(table_seed, 0, range(n), settings_of(s))
        deg = np.stack([SD.apply(clean[i], table[i])[0] for i in range(n)])
        out[name] = ((clean / f32(255.0)).astype(f32), (deg / f32(255.0)).astype(f32))
    return out
