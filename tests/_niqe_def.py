"""The float64 definition of NIQE that csrc/niqe.hip is held to (Mittal, Soundararajan, Bovik 2013, "Making a completely blind image
quality analyzer"), in numpy, operations and their order written out.  It follows the authors' MATLAB release as recalled; NOTHING here
is pinned to that release or to its shipped pristine parameters.  Deliberate deviations, stated where they occur:

  * rows with a non-finite feature leave the mean AND the covariance (the release drops them per column for the mean, ``nanmean``);
  * the pseudo-inverse is ``numpy.linalg.pinv(hermitian=True)`` at its default cutoff (MATLAB's ``pinv`` uses another tolerance);
  * a NaN ``rn`` has ``alpha = NaN`` (a table search has no answer for it), and an image with a NaN pixel inside the cropped area has
    NaN in every feature, so that its score is NaN: the project's rule that a non-finite pixel spoils its own image;
  * the reduction by two is MATLAB's ``imresize(im, 0.5)`` as recalled: bicubic (Keys, a = -0.5) with the kernel stretched by two.

An image is ``[3, H, W]`` in [0, 1] (any float dtype).  Sums over a block are numpy's (pairwise) reductions; the device adds in another
order, which is what the 1e-11 gates of tests/test_gpu_niqe.py allow for.

A constant non-zero block is outside every comparison: its sigma is ``sqrt(|E[x^2] - mu^2|)`` of two equal numbers, a rounding residue,
so its features are finite and rounding-dependent in any implementation, the release included.  The fixtures below carry noise
everywhere.
"""
import math

import numpy as np

ROW = 36
GAM = 0.2 + 0.001 * np.arange(9801, dtype=np.float64)
_lgamma = np.vectorize(math.lgamma, otypes=[np.float64])
_TABLE = None


def table() -> np.ndarray:
    """R(g) = Gamma(2/g)^2 / (Gamma(1/g) Gamma(3/g)) over GAM, through lgamma; it rises with g."""
    global _TABLE
    if _TABLE is None:
        _TABLE = np.exp((2.0 * _lgamma(2.0 / GAM) - _lgamma(1.0 / GAM)) - _lgamma(3.0 / GAM))
    return _TABLE


def g7() -> np.ndarray:
    x = np.arange(-3, 4, dtype=np.float64)
    w = np.exp(-(x * x) / (2.0 * (7.0 / 6.0) ** 2))
    return w / w.sum()


def cubic(x: float) -> float:
    x = abs(x)
    if x <= 1.0:
        return 1.5 * x ** 3 - 2.5 * x ** 2 + 1.0
    if x <= 2.0:
        return -0.5 * x ** 3 + 2.5 * x ** 2 - 4.0 * x + 2.0
    return 0.0


def half_weights() -> np.ndarray:
    """The eight taps at distances -3.5 .. 3.5 from the output centre, ``cubic(d / 2)``, normalised (exact binary fractions)."""
    w = np.array([cubic(d / 2.0) for d in (-3.5, -2.5, -1.5, -0.5, 0.5, 1.5, 2.5, 3.5)], dtype=np.float64)
    return w / w.sum()


def _taps_rows(pad: np.ndarray, w: np.ndarray, out_w: int, step: int) -> np.ndarray:
    """sum_k w[k] * pad[:, step * j + k], taps added in ascending k, starting from 0."""
    acc = np.zeros((pad.shape[0], out_w), dtype=np.float64)
    for k in range(len(w)):
        acc = acc + w[k] * pad[:, k:k + step * (out_w - 1) + 1:step]
    return acc


def filt(im: np.ndarray) -> np.ndarray:
    """The 7 x 7 Gaussian window, separably: along the rows, then along the columns, replicated edges."""
    w = g7()
    pad = np.pad(im, 3, mode="edge")
    rows = _taps_rows(pad, w, im.shape[1], 1)                       # [H + 6, W]
    return _taps_rows(rows.T, w, im.shape[0], 1).T


def half(im: np.ndarray) -> np.ndarray:
    """[H, W] -> [H / 2, W / 2]: output j sits at 2 j + 0.5 and reads inputs 2 j - 3 .. 2 j + 4, indices clamped; rows, then columns."""
    w = half_weights()
    pad = np.pad(im, ((3, 4), (3, 4)), mode="edge")
    rows = _taps_rows(pad, w, im.shape[1] // 2, 2)                  # [H + 7, W / 2]
    return _taps_rows(rows.T, w, im.shape[0] // 2, 2).T


def gray(img: np.ndarray, quantize: bool = True) -> np.ndarray:
    v = img.astype(np.float64)
    c = 255.0 * np.where(np.isnan(v), np.nan, np.minimum(np.maximum(v, 0.0), 1.0))
    if quantize:
        c = np.floor(c + 0.5)
    g = (0.298936021293775 * c[0] + 0.587043074451121 * c[1]) + 0.114020904255103 * c[2]
    if quantize:
        g = np.floor(g + 0.5)
    return g


def mscn(im: np.ndarray):
    """-> (m, sigma)"""
    mu = filt(im)
    sigma = np.sqrt(np.abs(filt(im * im) - mu * mu))
    return (im - mu) / (sigma + 1.0), sigma


def blocks(plane: np.ndarray, p: int) -> np.ndarray:
    """[bh p, bw p] -> [bh bw, p, p], blocks in row-major order."""
    bh, bw = plane.shape[0] // p, plane.shape[1] // p
    return plane.reshape(bh, p, bw, p).transpose(0, 2, 1, 3).reshape(bh * bw, p, p)


def table_margin(rn: np.ndarray) -> np.ndarray:
    """Relative distance of each rn from the nearest midpoint between two table entries (inf for a NaN rn): how far an estimate is from
    the point where its ``alpha`` would change."""
    R = table()
    mids = (R[:-1] + R[1:]) / 2.0
    flat = np.asarray(rn, dtype=np.float64).ravel()
    out = np.full(flat.shape, np.inf)
    good = np.isfinite(flat)
    j = np.clip(np.searchsorted(mids, flat[good]), 1, len(mids) - 1)
    near = np.minimum(np.abs(flat[good] - mids[j - 1]), np.abs(flat[good] - mids[j]))
    out[good] = near / np.abs(flat[good])
    return out.reshape(np.shape(rn))


def aggd(v: np.ndarray):
    """The asymmetric generalised Gaussian estimate of every vector ``v[i]`` (``[B, n]``) -> (alpha, bl, br, rn), each ``[B]``."""
    with np.errstate(all="ignore"):
        sq = v * v
        neg, pos = v < 0, v > 0
        ls = np.sqrt(np.where(neg, sq, 0.0).sum(axis=1) / neg.sum(axis=1))
        rs = np.sqrt(np.where(pos, sq, 0.0).sum(axis=1) / pos.sum(axis=1))
        n = float(v.shape[1])
        mabs, msq = np.abs(v).sum(axis=1) / n, sq.sum(axis=1) / n
        gh = ls / rs
        rh = (mabs * mabs) / msq
        rn = ((rh * (gh * gh * gh + 1.0)) * (gh + 1.0)) / ((gh * gh + 1.0) * (gh * gh + 1.0))
        R = table()
        alpha = np.array([GAM[int(np.argmin((R - r) ** 2))] if r == r else np.nan for r in rn], dtype=np.float64)
        safe = np.where(np.isnan(alpha), 1.0, alpha)
        c = np.sqrt(np.exp(_lgamma(1.0 / safe) - _lgamma(3.0 / safe)))
        c = np.where(np.isnan(alpha), np.nan, c)
        return alpha, ls * c, rs * c, rn


SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))


def block_features(b: np.ndarray):
    """[B, p, p] blocks of m -> (feats [B, 18], rn [B, 5]).  The shifts are circular inside the block (``blkproc`` hands the release's
    feature function one block at a time)."""
    B = b.shape[0]
    feats = np.empty((B, 18), dtype=np.float64)
    rns = np.empty((B, 5), dtype=np.float64)
    alpha, bl, br, rns[:, 0] = aggd(b.reshape(B, -1))
    feats[:, 0], feats[:, 1] = alpha, (bl + br) / 2.0
    for q, d in enumerate(SHIFTS):
        pair = b * np.roll(b, d, axis=(1, 2))
        alpha, bl, br, rns[:, q + 1] = aggd(pair.reshape(B, -1))
        safe = np.where(np.isnan(alpha), 1.0, alpha)
        with np.errstate(all="ignore"):
            ratio = np.where(np.isnan(alpha), np.nan, np.exp(_lgamma(2.0 / safe) - _lgamma(1.0 / safe)))
            feats[:, 2 + 4 * q:6 + 4 * q] = np.stack([alpha, (br - bl) * ratio, bl, br], axis=1)
    return feats, rns


def features(img: np.ndarray, patch: int = 96, quantize: bool = True):
    """-> (feats [P, 36], sharp [P], margin [P, 10]): the rows of one image, the mean of sigma over each block at scale 1, and the
    table margin of each of the ten estimates of a row."""
    if patch % 2 or patch < 8:
        raise ValueError(f"patch = {patch}; it must be even and at least 8")
    H, W = img.shape[1], img.shape[2]
    bh, bw = H // patch, W // patch
    if bh < 1 or bw < 1:
        raise ValueError(f"an image of {H} x {W} holds no block of patch = {patch}")
    im = gray(img, quantize)[:bh * patch, :bw * patch]
    spoiled = bool(np.isnan(im).any())
    feats = np.empty((bh * bw, ROW), dtype=np.float64)
    margin = np.empty((bh * bw, 10), dtype=np.float64)
    sharp = None
    for s in (1, 2):
        p = patch // s
        with np.errstate(all="ignore"):
            m, sigma = mscn(im)
        if s == 1:
            sharp = blocks(sigma, p).reshape(bh * bw, -1).sum(axis=1) / float(p * p)
        f, rn = block_features(blocks(m, p))
        feats[:, 18 * (s - 1):18 * s] = f
        margin[:, 5 * (s - 1):5 * s] = table_margin(rn)
        if s == 1:
            im = half(im)
    if spoiled:
        feats[:] = np.nan
    return feats, sharp, margin


def valid_rows(feats: np.ndarray, sharp=None, sharp_threshold: float = 0.0) -> np.ndarray:
    """[P] bool: all 36 finite and, with a threshold, ``sharp > threshold * max(sharp of the image)``."""
    ok = np.isfinite(feats).all(axis=1)
    if sharp_threshold > 0.0:
        with np.errstate(all="ignore"):
            ok &= sharp > sharp_threshold * np.fmax.reduce(sharp)
    return ok


def moments(rows: np.ndarray):
    """-> (mean [36], unbiased cov [36, 36], count) of the rows ``[n, 36]``; NaN where undefined."""
    n = rows.shape[0]
    with np.errstate(all="ignore"):
        mean = rows.sum(axis=0) / float(n) if n else np.full(ROW, np.nan)
        d = rows - mean
        cov = (d.T @ d) / float(n - 1) if n >= 2 else np.full((ROW, ROW), np.nan)
    return mean, cov, n


def score(mu_pris, cov_pris, mean, cov, count) -> float:
    if count < 2 or not (np.isfinite(mean).all() and np.isfinite(cov).all()):
        return float("nan")
    d = np.asarray(mu_pris, dtype=np.float64) - mean
    inv = np.linalg.pinv((np.asarray(cov_pris, dtype=np.float64) + cov) / 2.0, hermitian=True)
    return float(np.sqrt(d @ inv @ d))


def niqe(img: np.ndarray, mu_pris, cov_pris, patch: int = 96, quantize: bool = True) -> float:
    feats, _, _ = features(img, patch, quantize)
    mean, cov, n = moments(feats[valid_rows(feats)])
    return score(mu_pris, cov_pris, mean, cov, n)


def fit(images, patch: int = 96, sharp_threshold: float = 0.75, quantize: bool = True):
    """-> (mu_pris, cov_pris, kept): from each image the finite rows sharper than ``sharp_threshold * max``; moments of all of them.
    ``kept`` lists the boolean selection per image."""
    rows, kept = [], []
    for img in images:
        feats, sharp, _ = features(img, patch, quantize)
        ok = valid_rows(feats, sharp, sharp_threshold)
        kept.append(ok)
        rows.append(feats[ok])
    mean, cov, _ = moments(np.concatenate(rows))
    return mean, cov, kept


# ---------------------------------------------------------------------------------------------------------------- fixtures
def image(seed: int, H: int, W: int, noise: float = 0.04) -> np.ndarray:
    """A seeded ``[3, H, W]`` fp32 image in [0, 1]: three waves whose amplitude varies over the image (blocks differ in sharpness) and
    Gaussian noise on every pixel of every channel."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((3, H, W), dtype=np.float64)
    envelope = 0.35 + 0.65 * (0.5 + 0.5 * np.sin(2 * np.pi * (x / max(W, 1) * rng.uniform(0.7, 1.6) + rng.uniform())) *
                              np.cos(2 * np.pi * (y / max(H, 1) * rng.uniform(0.7, 1.6) + rng.uniform())))
    for c in range(3):
        fx, fy, ph = rng.uniform(0.05, 0.9), rng.uniform(0.05, 0.9), rng.uniform(0, 2 * np.pi)
        wave = np.sin(fx * x + fy * y + ph) + 0.5 * np.sin(1.7 * fy * x - 1.3 * fx * y + 2 * ph)
        out[c] = 0.5 + 0.17 * envelope * wave + noise * rng.standard_normal((H, W))
    return np.clip(out, 0.0, 1.0).astype(np.float32)


# What the tests compare on the device.  tests/test_niqe_cpu.py asserts that every estimate of every fixture listed by
# ``compared_fixtures`` keeps a table margin of at least 1e-9, so that the device's ``alpha`` must equal the definition's exactly.
FEATURE_CASES = [(8, 43, 61),        # cropping on both axes, 5 x 7 blocks, scale-2 blocks of 4 x 4
                 (16, 48, 64),
                 (96, 192, 288),     # the real block side, six blocks
                 (96, 97, 200)]      # 1 x 2 blocks
FEATURE_SEEDS = (1, 2, 3)
ZERO_SEED = 4
FIT_SEEDS = (100, 101, 102, 103, 104, 105)
SCORE_SEED = 7
CLEAN_NOISE, NOISY_NOISE = 0.01, 0.15


def compared_fixtures():
    """(seed, H, W, noise, patch, quantize) of every image whose device features are compared with this definition."""
    out = [(s, H, W, 0.04, p, q) for p, H, W in FEATURE_CASES for s in FEATURE_SEEDS for q in (True, False)]
    out += [(s, 64, 160, 0.04, 16, True) for s in FEATURE_SEEDS]
    out += [(s, 96, 128, CLEAN_NOISE, 16, True) for s in FIT_SEEDS]
    out += [(FIT_SEEDS[0], 43, 61, CLEAN_NOISE, 16, True)]
    out += [(SCORE_SEED, 96, 128, CLEAN_NOISE, 16, True), (SCORE_SEED, 96, 128, NOISY_NOISE, 16, True)]
    return out
