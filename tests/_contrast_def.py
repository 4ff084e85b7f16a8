"""The definition ``csrc/contrast.hip`` is held to: contrast-limited adaptive histogram equalisation (CLAHE, Zuiderveld 1994, in the
form OpenCV made common -- written from memory, see "not pinned" in ``hdiff_amd/classical.py``) and global histogram equalisation by
Pillow's rule (``PIL.ImageOps.equalize``), on 8-bit planes, in numpy with every operation and its order written out.  Images are fp32
``[3, H, W]``; ``f32(.)`` is ONE rounding of a float64 value.

    X        = min(max(I, 0), 1) in fp32, a NaN counting as 0 (what ``fminf(fmaxf(v, 0), 1)`` of csrc/classical.hip gives)
    "rgb":     q_c = uint8(floor(f64(X_c) * 255 + 0.5)) on each channel;  out_c = f32(f64(q'_c) / 255)
    "lab":     (L, a, b) = srgb_to_lab(f64(X));  q = uint8(clamp(floor(L * 2.55 + 0.5), 0, 255));  L' = f64(q') / 2.55;
               out = f32(clamp(lab_to_srgb(L', a, b), 0, 1))
    CLAHE on one plane q [H, W], grid (tiles_y, tiles_x), clip_limit:
      pad      right and bottom by (t - n % t) % t pixels with reflect-101 (row H + k is row H - 2 - k); th x tw = Hp / tiles_y x
               Wp / tiles_x, area = th * tw.  (OpenCV pads a FULL extra tile on an axis that divides when the other does not; this does
               not.)
      clip     = max(1, floor(clip_limit * area / 256)) in double for clip_limit > 0; no clipping at 0.  (A clip above `area` clips
               nothing, so min(clip, area) -- which is what the device is handed -- gives the same tables.)
      per tile h = the 256-bin histogram of the padded tile;  excess = sum(max(h - clip, 0));  h = min(h, clip);  h += excess // 256;
               r = excess % 256;  if r > 0: step = max(256 // r, 1), and h[0], h[step], h[2 step], ... gain 1 each until r additions are
               made (r * step <= 256: the index never passes 255 first).  One pass.
      table    lut[i] = uint8(min(rint(f32(cumsum(h)[i]) * scale), 255)), scale = f32(255) / f32(area), the product in fp32, halves to
               even
      blend    at (y, x) with value v:  fx = f32(x) * inv_tw - 0.5f;  x1 = floor(fx);  xa = fx - x1;  xa1 = 1 - xa;  tiles max(x1, 0) and
               min(x1 + 1, tiles_x - 1);  the same in y;  inv_tw = f32(1) / f32(tw)
               res = (lut[y1, x1][v] * xa1 + lut[y1, x2][v] * xa) * ya1 + (lut[y2, x1][v] * xa1 + lut[y2, x2][v] * xa) * ya,
               every operation one fp32 rounding;  q' = uint8(clamp(rint(res), 0, 255))
    equalisation of one plane (Pillow's rule):  h = the histogram;  with fewer than two non-empty bins the plane is unchanged;
               step = (sum(h) - the last non-zero h) // 255;  at step == 0 the plane is unchanged;  otherwise
               lut[i] = min((step // 2 + sum(h[:i])) // step, 255).  The min is what Pillow's ``point`` does with an entry above 255 (it
               clips a table entry to [0, 255]; tests/test_contrast_cpu.py holds a fixture that reaches 300).
Everything but the colour conversion is integer arithmetic or single fp32 operations, so the kernels are held bit for bit on q, on every
table and on the "rgb" output; the "lab" output passes through pow and cbrt in double: CLAHE's is held to the fp32 value or its
neighbour, the equalisation's bit for bit (both met the value in every element on the MI355X).  The fixtures the kernels are run on are
in tests/_contrast_fixtures.py."""
import math

import numpy as np

from _uciqe_def import MATRIX, WHITE, lab_def

f32, f64 = np.float32, np.float64
BINS = 256
MAX_TILES = 16


# ---------------------------------------------------------------------------------------------------------------- colour
def clipped(img) -> np.ndarray:
    """min(max(I, 0), 1) in fp32; a NaN gives 0."""
    img = np.asarray(img)
    assert img.dtype == np.float32 and img.ndim == 3 and img.shape[0] == 3
    return np.minimum(np.maximum(np.where(np.isnan(img), f32(0.0), img), f32(0.0)), f32(1.0)).astype(f32)


def matrix_inverse():
    """The inverse of the RGB -> XYZ matrix by cofactors, every product and difference written out (csrc/lab.h computes the same
    expressions from the same nine literals)."""
    (a, b, c), (d, e, f), (g, h, i) = MATRIX
    A, B, C = (e * i) - (f * h), (f * g) - (d * i), (d * h) - (e * g)
    det = ((a * A) + (b * B)) + (c * C)
    return (((A / det), ((c * h) - (b * i)) / det, ((b * f) - (c * e)) / det),
            ((B / det), ((a * i) - (c * g)) / det, ((c * d) - (a * f)) / det),
            ((C / det), ((b * g) - (a * h)) / det, ((a * e) - (b * d)) / det))


def lab_to_srgb_def(L, a, b) -> np.ndarray:
    """float64 (L, a, b) planes -> float64 sRGB planes ``[3, ...]``, NOT clipped: the inverse of ``_uciqe_def.lab_def``, branch for
    branch.  (sRGB values in (0.04045, 0.0404517] come back through the other branch of the transfer curve, 2e-7 off: the curve's two
    pieces do not meet exactly at the published constants.)"""
    L, a, b = (np.asarray(v, dtype=f64) for v in (L, a, b))
    fy = (L + 16.0) / 116.0
    fx = fy + (a / 500.0)
    fz = fy - (b / 200.0)
    xyz = []
    for fv, white in zip((fx, fy, fz), WHITE):
        cube = (fv * fv) * fv
        xyz.append(np.where(cube > 0.008856, cube, (fv - (16.0 / 116.0)) / 7.787) * white)
    out = []
    for row in matrix_inverse():
        lin = ((row[0] * xyz[0]) + (row[1] * xyz[1])) + (row[2] * xyz[2])
        with np.errstate(invalid="ignore"):
            out.append(np.where(lin > 0.0031308, (1.055 * np.power(lin, 1.0 / 2.4)) - 0.055, 12.92 * lin))
    return np.stack(out)


def quantise_def(x: np.ndarray, space: str):
    """clipped fp32 ``[3, H, W]`` -> (q uint8 ``[P, H, W]``, the Lab planes or None)."""
    if space == "rgb":
        return np.floor((x.astype(f64) * 255.0) + 0.5).astype(np.uint8), None
    assert space == "lab"
    L, a, b = lab_def(x.astype(f64))
    return np.minimum(np.maximum(np.floor((L * 2.55) + 0.5), 0.0), 255.0).astype(np.uint8)[None], (L, a, b)


def dequantise_def(q2: np.ndarray, space: str, lab) -> np.ndarray:
    if space == "rgb":
        return (q2.astype(f64) / 255.0).astype(f32)
    rgb = lab_to_srgb_def(q2[0].astype(f64) / 2.55, lab[1], lab[2])
    return np.minimum(np.maximum(rgb, 0.0), 1.0).astype(f32)


# ---------------------------------------------------------------------------------------------------------------- CLAHE
def tile_geometry(H: int, W: int, grid):
    """-> (th, tw, area, Hp, Wp)."""
    ty, tx = grid
    assert 1 <= ty <= MAX_TILES and 1 <= tx <= MAX_TILES and H >= ty and W >= tx
    Hp, Wp = H + (ty - H % ty) % ty, W + (tx - W % tx) % tx
    return Hp // ty, Wp // tx, (Hp // ty) * (Wp // tx), Hp, Wp


def clip_level(clip_limit: float, area: int) -> int:
    """The count a bin is cut at; `area` (nothing is cut) at clip_limit 0."""
    assert clip_limit >= 0.0
    if clip_limit == 0.0:
        return area
    c = (f64(clip_limit) * f64(area)) / f64(256.0)
    return area if c >= area else max(1, int(math.floor(c)))


def host_constants(H: int, W: int, grid):
    """-> (inv_th, inv_tw, scale) in fp32, one division each."""
    th, tw, area, _, _ = tile_geometry(H, W, grid)
    return f32(1.0) / f32(th), f32(1.0) / f32(tw), f32(255.0) / f32(area)


def tile_histograms(plane: np.ndarray, grid) -> np.ndarray:
    """uint8 ``[H, W]`` -> int64 ``[tiles_y, tiles_x, 256]`` over the padded tiles."""
    H, W = plane.shape
    ty, tx = grid
    th, tw, _, Hp, Wp = tile_geometry(H, W, grid)
    padded = np.pad(plane, ((0, Hp - H), (0, Wp - W)), mode="reflect")
    tiles = padded.reshape(ty, th, tx, tw).transpose(0, 2, 1, 3).reshape(ty * tx, th * tw).astype(np.int64)
    flat = tiles + (np.arange(ty * tx, dtype=np.int64) * BINS)[:, None]
    return np.bincount(flat.reshape(-1), minlength=ty * tx * BINS).reshape(ty, tx, BINS)


def redistribute(h: np.ndarray, clip: int) -> np.ndarray:
    """int64 ``[..., 256]`` histograms -> the clipped and redistributed ones."""
    excess = np.maximum(h - clip, 0).sum(axis=-1, keepdims=True)
    h = np.minimum(h, clip) + excess // BINS
    r = excess % BINS
    step = np.maximum(BINS // np.maximum(r, 1), 1)
    i = np.arange(BINS, dtype=np.int64)
    return h + ((r > 0) & (i % step == 0) & (i // step < r))


def clahe_luts_def(plane: np.ndarray, grid, clip_limit: float, return_hist: bool = False):
    """uint8 ``[H, W]`` -> uint8 ``[tiles_y, tiles_x, 256]``."""
    H, W = plane.shape
    area = tile_geometry(H, W, grid)[2]
    h = redistribute(tile_histograms(plane, grid), clip_level(clip_limit, area))
    scale = host_constants(H, W, grid)[2]
    lut = np.minimum(np.rint(np.cumsum(h, axis=-1).astype(f32) * scale), f32(255.0)).astype(np.uint8)
    return (lut, h) if return_hist else lut


def blend_at(lut: np.ndarray, shape, grid, ys, xs, vs, dtype=f32) -> np.ndarray:
    """``res`` of the values ``vs`` put at the pixels ``(ys, xs)`` of an ``H x W`` plane with the tables ``lut``.  The weights are
    fp32 whatever ``dtype`` is; ``dtype=f64`` carries the same products and sums out in double (exact but for sums of more than 53
    bits), which tells whether the fp32 ``res`` was rounded at all."""
    H, W = shape
    ty, tx = grid
    inv_th, inv_tw, _ = host_constants(H, W, grid)

    def axis(at, inv, tiles):
        fv = (np.asarray(at).astype(f32) * inv) - f32(0.5)
        v1 = np.floor(fv)
        va = fv - v1
        i1 = v1.astype(np.int64)
        return np.maximum(i1, 0), np.minimum(i1 + 1, tiles - 1), va.astype(dtype), (f32(1.0) - va).astype(dtype)

    y1, y2, ya, ya1 = axis(ys, inv_th, ty)
    x1, x2, xa, xa1 = axis(xs, inv_tw, tx)
    v = np.asarray(vs).astype(np.int64)
    l11, l12, l21, l22 = (lut[yy, xx, v].astype(dtype) for yy, xx in ((y1, x1), (y1, x2), (y2, x1), (y2, x2)))
    res = (((l11 * xa1) + (l12 * xa)) * ya1) + (((l21 * xa1) + (l22 * xa)) * ya)
    assert res.dtype == dtype
    return res


def blend_def(plane: np.ndarray, lut: np.ndarray, grid, return_res: bool = False):
    """uint8 ``[H, W]`` and its tables -> uint8 ``[H, W]`` (and the fp32 ``res`` before its rounding)."""
    H, W = plane.shape
    res = blend_at(lut, (H, W), grid, np.arange(H)[:, None], np.arange(W)[None, :], plane)
    out = np.minimum(np.maximum(np.rint(res), f32(0.0)), f32(255.0)).astype(np.uint8)
    return (out, res) if return_res else out


def clahe_def(img, *, clip_limit: float = 2.0, grid=(8, 8), space: str = "lab") -> dict:
    """One fp32 ``[3, H, W]`` image -> dict of ``out`` (fp32 ``[3, H, W]``), ``q``, ``q2`` (uint8 ``[P, H, W]``, before and after) and
    ``lut`` (uint8 ``[P, tiles_y, tiles_x, 256]``)."""
    x = clipped(img)
    q, lab = quantise_def(x, space)
    lut = np.stack([clahe_luts_def(p, grid, clip_limit) for p in q])
    q2 = np.stack([blend_def(p, t, grid) for p, t in zip(q, lut)])
    return {"out": dequantise_def(q2, space, lab), "q": q, "q2": q2, "lut": lut, "lab": lab}


# ---------------------------------------------------------------------------------------------------------------- equalisation
def equalize_lut_def(plane: np.ndarray) -> np.ndarray:
    """uint8 ``[H, W]`` -> uint8 ``[256]``; the identity table where Pillow leaves the plane unchanged."""
    h = np.bincount(plane.reshape(-1).astype(np.int64), minlength=BINS)
    identity = np.arange(BINS).astype(np.uint8)
    filled = np.flatnonzero(h)
    if filled.size < 2:
        return identity
    step = (int(h.sum()) - int(h[filled[-1]])) // 255
    if step == 0:
        return identity
    before = np.cumsum(h) - h                                  # sum(h[:i])
    return np.minimum((step // 2 + before) // step, 255).astype(np.uint8)


def equalize_def(img, *, space: str = "rgb") -> dict:
    x = clipped(img)
    q, lab = quantise_def(x, space)
    lut = np.stack([equalize_lut_def(p) for p in q])
    q2 = np.stack([t[p] for p, t in zip(q, lut)])
    return {"out": dequantise_def(q2, space, lab), "q": q, "q2": q2, "lut": lut, "lab": lab}


# ---------------------------------------------------------------------------------------------------------------- checks
def neighbours_ok(got: np.ndarray, want: np.ndarray):
    """(all within one fp32 step of ``want``, the count that differs at all) for finite fp32 arrays."""
    got, want = np.asarray(got, dtype=f32), np.asarray(want, dtype=f32)
    lo, hi = np.nextafter(want, f32(-np.inf)), np.nextafter(want, f32(np.inf))
    return bool(((got >= lo) & (got <= hi)).all()), int((got != want).sum())
