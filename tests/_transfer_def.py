"""The float64 definitions the kernels of csrc/transfer.hip are held to, operations and their order written out: the triangle-filter
resample, the guided-filter fit with a colour guide, and the application of the upsampled map.  Also the seeded fixtures the uint8 tests
share, and the interpolated magnitude sum S against which an fp32 result is judged."""
import numpy as np

# ---------------------------------------------------------------------------------------------------------------- resample


def _taps(o: int, n_in: int, n_out: int):
    """(first tap, weights normalised to sum 1) of output index ``o``: centre (o + 0.5) in / out, support max(in / out, 1)."""
    scale = n_in / n_out
    support = max(scale, 1.0)
    c = (o + 0.5) * scale
    lo = max(int(c - support + 0.5), 0)
    hi = min(int(c + support + 0.5), n_in)
    raw = [max(0.0, 1.0 - abs((k + 0.5 - c) / support)) for k in range(lo, hi)]
    total = 0.0
    for v in raw:                    # in tap order
        total += v
    return lo, [v / total for v in raw]


def resample_rows64(img_u8: np.ndarray, w: int) -> np.ndarray:
    """The horizontal pass: uint8 [H, W, 3] -> float64 [H, w, 3], products added in tap order."""
    H, W, _ = img_u8.shape
    src = img_u8.astype(np.float64)
    tmp = np.zeros((H, w, 3), dtype=np.float64)
    for o in range(w):
        lo, weights = _taps(o, W, w)
        acc = np.zeros((H, 3), dtype=np.float64)
        for j, wk in enumerate(weights):
            acc = acc + wk * src[:, lo + j, :]
        tmp[:, o, :] = acc
    return tmp


def resample64(img_u8: np.ndarray, size) -> np.ndarray:
    """uint8 [H, W, 3] -> float64 [3, h, w] in [0, 255]; the kernel's value is this rounded once to fp32."""
    h, w = (size, size) if isinstance(size, int) else size
    H = img_u8.shape[0]
    tmp = resample_rows64(img_u8, w)
    out = np.zeros((h, w, 3), dtype=np.float64)
    for o in range(h):
        lo, weights = _taps(o, H, h)
        acc = np.zeros((w, 3), dtype=np.float64)
        for j, wk in enumerate(weights):
            acc = acc + wk * tmp[lo + j, :, :]
        out[o] = acc
    return np.ascontiguousarray(out.transpose(2, 0, 1))


# ---------------------------------------------------------------------------------------------------------------- fit
def _bounds(n: int, r: int):
    idx = np.arange(n)
    return np.maximum(idx - r, 0), np.minimum(idx + r, n - 1)


def window_sum(planes: np.ndarray, r: int) -> np.ndarray:
    """[..., h, w] -> the sum over the clipped window [y-r, y+r] x [x-r, x+r]: along x, then along y, each a direct sum in index order."""
    h, w = planes.shape[-2:]
    xlo, xhi = _bounds(w, r)
    ylo, yhi = _bounds(h, r)
    sx = np.zeros_like(planes)
    for x in range(w):
        acc = np.zeros(planes.shape[:-1], dtype=np.float64)
        for k in range(xlo[x], xhi[x] + 1):
            acc = acc + planes[..., k]
        sx[..., x] = acc
    sy = np.zeros_like(planes)
    for y in range(h):
        acc = np.zeros(planes.shape[:-2] + (w,), dtype=np.float64)
        for k in range(ylo[y], yhi[y] + 1):
            acc = acc + sx[..., k, :]
        sy[..., y, :] = acc
    return sy


def window_count(h: int, w: int, r: int) -> np.ndarray:
    xlo, xhi = _bounds(w, r)
    ylo, yhi = _bounds(h, r)
    return ((yhi - ylo + 1)[:, None] * (xhi - xlo + 1)[None, :]).astype(np.float64)


def window_mean(planes: np.ndarray, r: int) -> np.ndarray:
    return window_sum(planes, r) / window_count(planes.shape[-2], planes.shape[-1], r)


def fit_ab64(I: np.ndarray, p: np.ndarray, r: int, eps: float) -> np.ndarray:
    """I, p: [3, h, w] (any float dtype) -> float64 [12, h, w]: a[c][0..2] and b[c] per pixel BEFORE the second window mean."""
    I, p = I.astype(np.float64), p.astype(np.float64)
    planes = [I[0], I[1], I[2], p[0], p[1], p[2],
              I[0] * I[0], I[0] * I[1], I[0] * I[2], I[1] * I[1], I[1] * I[2], I[2] * I[2]]
    planes += [I[j] * p[c] for j in range(3) for c in range(3)]
    m = window_mean(np.stack(planes), r)
    s00, s01, s02 = m[6] - m[0] * m[0] + eps, m[7] - m[0] * m[1], m[8] - m[0] * m[2]
    s11, s12, s22 = m[9] - m[1] * m[1] + eps, m[10] - m[1] * m[2], m[11] - m[2] * m[2] + eps
    with np.errstate(all="ignore"):              # a non-finite image stays non-finite, quietly
        l00 = np.sqrt(s00)
        l10, l20 = s01 / l00, s02 / l00
        l11 = np.sqrt(s11 - l10 * l10)
        l21 = (s12 - l20 * l10) / l11
        l22 = np.sqrt(s22 - l20 * l20 - l21 * l21)
        ab = np.zeros((12,) + I.shape[1:], dtype=np.float64)
        for c in range(3):
            c0, c1, c2 = m[12 + c] - m[0] * m[3 + c], m[15 + c] - m[1] * m[3 + c], m[18 + c] - m[2] * m[3 + c]
            z0 = c0 / l00
            z1 = (c1 - l10 * z0) / l11
            z2 = (c2 - l20 * z0 - l21 * z1) / l22
            a2 = z2 / l22
            a1 = (z1 - l21 * a2) / l11
            a0 = (z0 - l10 * a1 - l20 * a2) / l00
            ab[3 * c], ab[3 * c + 1], ab[3 * c + 2] = a0, a1, a2
            ab[9 + c] = m[3 + c] - (a0 * m[0] + a1 * m[1] + a2 * m[2])
    return ab


def fit64(I: np.ndarray, p: np.ndarray, r: int, eps: float) -> np.ndarray:
    """[3, h, w] pair -> float64 coefficients [12, h, w]; the kernel's value is this rounded once to fp32."""
    with np.errstate(all="ignore"):
        return window_mean(fit_ab64(I, p, r, eps), r)


def fit(I: np.ndarray, p: np.ndarray, r: int, eps: float) -> np.ndarray:
    """[N, 3, h, w] or [3, h, w] -> fp32 coefficients."""
    if I.ndim == 4:
        return np.stack([fit64(a, b, r, eps).astype(np.float32) for a, b in zip(I, p)])
    return fit64(I, p, r, eps).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- apply
def _source(n_out: int, n_in: int):
    s = np.clip((np.arange(n_out, dtype=np.float64) + 0.5) * n_in / n_out - 0.5, 0.0, n_in - 1.0)
    i0 = np.floor(s).astype(np.int64)
    return i0, np.minimum(i0 + 1, n_in - 1), s - i0


def upsample64(planes: np.ndarray, H: int, W: int) -> np.ndarray:
    """[..., h, w] -> float64 [..., H, W]: half-pixel centres, clamped; along x at both rows, then along y."""
    planes = planes.astype(np.float64)
    y0, y1, fy = _source(H, planes.shape[-2])
    x0, x1, fx = _source(W, planes.shape[-1])
    top = planes[..., y0, :][..., x0] * (1.0 - fx) + planes[..., y0, :][..., x1] * fx
    bot = planes[..., y1, :][..., x0] * (1.0 - fx) + planes[..., y1, :][..., x1] * fx
    return top * (1.0 - fy)[:, None] + bot * fy[:, None]


def apply64(coef: np.ndarray, F: np.ndarray):
    """coef [12, h, w] (fp32 values), F float64 [3, H, W] -> (q [3, H, W], S [3, H, W]) in float64, unclamped: q_c = A_c0 F_0 + A_c1 F_1
    + A_c2 F_2 + b_c, and the magnitude sum S_c = up(|A_c0|) |F_0| + up(|A_c1|) |F_1| + up(|A_c2|) |F_2| + up(|b_c|)."""
    H, W = F.shape[-2:]
    A, S = upsample64(coef, H, W), upsample64(np.abs(coef.astype(np.float64)), H, W)
    Fa = np.abs(F)
    q = np.stack([A[3 * c] * F[0] + A[3 * c + 1] * F[1] + A[3 * c + 2] * F[2] + A[9 + c] for c in range(3)])
    s = np.stack([S[3 * c] * Fa[0] + S[3 * c + 1] * Fa[1] + S[3 * c + 2] * Fa[2] + S[9 + c] for c in range(3)])
    return q, s


def apply_u8_64(coef: np.ndarray, img_u8: np.ndarray):
    """coef [12, h, w], img uint8 [H, W, 3] -> (v, S) as [H, W, 3] float64: v = 255 clamp(q, 0, 1) before the rounding to a byte, with
    F = fp32(byte) / fp32(255) rounded to fp32 as the kernel takes it."""
    F = (img_u8.astype(np.float32) / np.float32(255.0)).astype(np.float64).transpose(2, 0, 1)
    q, s = apply64(coef, F)
    return 255.0 * np.clip(q, 0.0, 1.0).transpose(1, 2, 0), s.transpose(1, 2, 0)


APPLY_FACTOR = 16 * 2.0 ** -24      # at most sixteen fp32 roundings between the loads and the store, each relative to S


def tie_excused(v: np.ndarray, S: np.ndarray) -> np.ndarray:
    """Where the definition's 255 clamp(q, 0, 1) lies within 255 * 16 * 2^-24 * S of a half-integer: an fp32 result may round to the
    other neighbour there."""
    return np.abs(v - np.floor(v) - 0.5) <= 255.0 * APPLY_FACTOR * S


# ---------------------------------------------------------------------------------------------------------------- fixtures
APPLY_SIZES = (((5, 7), (5, 7)), ((5, 7), (13, 29)), ((16, 19), (45, 61)), ((33, 40), (97, 131)), ((8, 8), (3, 5)), ((1, 1), (4, 9)),
               ((6, 6), (9, 1)))
# beyond those: a row of more than one 1024-pixel strip whose length is a multiple of four, and such a row at equal size
EXTRA_APPLY_SIZES = (((3, 40), (2, 1100)), ((5, 8), (5, 8)))
FIXTURE_RADIUS, FIXTURE_EPS = 2, 1e-3           # the fit of the uint8 fixtures
COLOUR_MATRIX =np.array([[0.80, 0.15, -0.05], [0.05, 0.90, 0.10], [-0.10, 0.20, 0.70]])


def u8_fixture(small, large, seed: int = 0):
    """A seeded pair for the uint8 tests: (img uint8 [H, W, 3], low [3, h, w] fp32 in [0, 1], target [3, h, w] fp32 in [0, 1]).  The image is
    a smooth colour field plus 0.3 of uniform noise, quantised; the low image a subsample of it; the target a fixed 3 x 3 colour matrix,
    a 0.8 power and 2 % noise, clipped."""
    (h, w), (H, W) = small, large
    rng = np.random.default_rng(1000 * seed + 7 * H + W)
    yy, xx = np.meshgrid(np.arange(H) / max(H, 1), np.arange(W) / max(W, 1), indexing="ij")
    field = np.stack([0.5 + 0.3 * np.sin(2.0 * xx + c) * np.cos(1.5 * yy - c) for c in range(3)], axis=-1)
    img = np.clip(0.7 * field + 0.3 * rng.random((H, W, 3)), 0, 1)
    img_u8 = np.rint(img * 255).astype(np.uint8)
    ys = np.minimum((np.arange(h) * H) // h, H - 1)
    xs = np.minimum((np.arange(w) * W) // w, W - 1)
    low = (img_u8[ys][:, xs].astype(np.float32) / np.float32(255)).transpose(2, 0, 1)
    mixed = np.einsum("cj,jyx->cyx", COLOUR_MATRIX, low.astype(np.float64))
    target = np.clip(np.clip(mixed, 0, 1) ** 0.8 + 0.02 * (rng.random((3, h, w)) - 0.5), 0, 1).astype(np.float32)
    return img_u8, np.ascontiguousarray(low), target


def adjacent_or_equal(got: np.ndarray, want64: np.ndarray) -> np.ndarray:
    """Elementwise: ``got`` (fp32) is the fp32 rounding of ``want64`` or a float next to it."""
    want = want64.astype(np.float32)
    return (got == want) | (got == np.nextafter(want, np.float32(np.inf))) | (got == np.nextafter(want, np.float32(-np.inf)))
