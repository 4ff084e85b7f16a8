"""The definitions ``csrc/distribution.hip`` is held to, in numpy float64 with the loops written out in the kernels' order: the moments
of a set of feature rows (two passes, the rows added in order), the three kernel sums of KID under ``k(x, y) = (x.y / d + 1)^3`` (the
dot product added over the channels in order, the cube as ``(t * t) * t``), the unbiased KID estimate, and the Frechet distance by the
``scipy.linalg.sqrtm`` route the reference's FID takes (``utils/rotinas.py``), against which ``quality.frechet_from_moments`` is
compared.  numpy's elementwise operations round once each and never contract a product into a sum."""
import math

import numpy as np

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def offset_features(n: int, d: int, seed: int) -> np.ndarray:
    """fp32 ``[n, d]`` rows whose per-channel mean is about 1e3 times their spread: the case in which a one-pass covariance cancels."""
    rng = np.random.default_rng(seed)
    centre = 1e3 * (1.0 + rng.random(d))
    return (centre + rng.standard_normal((n, d))).astype(np.float32)


def positive_features(n: int, d: int, seed: int) -> np.ndarray:
    """fp32 ``[n, d]`` rows with positive entries: every kernel value is then above 1 and a relative error of a sum is well-posed."""
    rng = np.random.default_rng(seed)
    return (np.abs(rng.standard_normal((n, d))) + 0.1).astype(np.float32)


def moments_def(x: np.ndarray):
    """-> (mean[d], cov[d, d]) of fp32 rows ``[n, d]``; ``n = 1`` gives a NaN covariance."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 2
    n, d = x.shape
    x64 = x.astype(np.float64)
    total = np.zeros(d)
    for r in range(n):
        total = total + x64[r]
    mean = total / float(n)
    scatter = np.zeros((d, d))
    for r in range(n):
        c = x64[r] - mean
        scatter = scatter + c[:, None] * c[None, :]
    with np.errstate(all="ignore"):
        return mean, scatter / (float(n) - 1.0)


def kernel_matrix(x: np.ndarray, y: np.ndarray) -> np.ndarray:
    """``k(x_i, y_j)`` for all pairs, ``[n, m]``."""
    x, y = np.asarray(x), np.asarray(y)
    assert x.dtype == np.float32 and y.dtype == np.float32 and x.shape[1] == y.shape[1]
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    d = x.shape[1]
    dot = np.zeros((x.shape[0], y.shape[0]))
    for c in range(d):
        dot = dot + x64[:, c][:, None] * y64[:, c][None, :]
    t = dot / float(d) + 1.0
    return (t * t) * t


def kid_sums_def(a: np.ndarray, b: np.ndarray):
    """-> (sum over i != j of k(a_i, a_j), the same over b, sum over all pairs of k(a_i, b_j)); each sum exactly rounded."""
    kaa, kbb, kab = kernel_matrix(a, a), kernel_matrix(b, b), kernel_matrix(a, b)
    off = lambda k: math.fsum(k[i, j] for i in range(k.shape[0]) for j in range(k.shape[1]) if i != j)      # noqa: E731
    return off(kaa), off(kbb), math.fsum(kab.ravel())


def kid_from_sums(sums, n: int, m: int) -> float:
    if n < 2 or m < 2:
        return float("nan")
    return sums[0] / (n * (n - 1)) + sums[1] / (m * (m - 1)) - 2 * sums[2] / (n * m)


def kid_def(a: np.ndarray, b: np.ndarray) -> float:
    return kid_from_sums(kid_sums_def(a, b), a.shape[0], b.shape[0])


def frechet_sqrtm(mean_a, cov_a, mean_b, cov_b) -> float:
    """The reference's route: ``|dmu|^2 + tr (S_a + S_b - 2 sqrtm(S_a S_b))``, the real part where ``sqrtm`` comes out complex."""
    from scipy import linalg
    covmean = linalg.sqrtm(np.asarray(cov_a, dtype=np.float64) @ np.asarray(cov_b, dtype=np.float64))
    if isinstance(covmean, tuple):
        covmean = covmean[0]
    if np.iscomplexobj(covmean):
        covmean = covmean.real
    diff = np.asarray(mean_a, dtype=np.float64) - np.asarray(mean_b, dtype=np.float64)
    return float(diff @ diff + np.trace(cov_a) + np.trace(cov_b) - 2.0 * np.trace(covmean))


def commuting_fixture(d: int, seed: int, rank=None):
    """-> (mean_a, cov_a, mean_b, cov_b, exact): ``S_a = Q diag(a) Q^T``, ``S_b = Q diag(b) Q^T`` with ``a, b`` in [0.1, 2] (the trailing
    ``a_k`` zero from ``rank`` on), for which the distance is ``|dmu|^2 + sum a + sum b - 2 sum sqrt(a b)``."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    a, b = rng.uniform(0.1, 2.0, d), rng.uniform(0.1, 2.0, d)
    if rank is not None:
        a[rank:] = 0.0
    mean_a, mean_b = rng.standard_normal(d), rng.standard_normal(d)
    cov_a, cov_b = (q * a) @ q.T, (q * b) @ q.T
    cov_a, cov_b = (cov_a + cov_a.T) / 2, (cov_b + cov_b.T) / 2
    diff = mean_a - mean_b
    exact = math.fsum(diff * diff) + math.fsum(a) + math.fsum(b) - 2.0 * math.fsum(np.sqrt(a * b))
    return mean_a, cov_a, mean_b, cov_b, exact


def generic_fixture(d: int, seed: int):
    """Moments of two sets of ``2 d`` random rows with different scales per channel: full rank, not commuting."""
    rng = np.random.default_rng(seed)
    mix = rng.standard_normal((d, d)) / np.sqrt(d)
    xa = rng.standard_normal((2 * d, d)) @ mix + rng.standard_normal(d)
    xb = (rng.standard_normal((2 * d, d)) * rng.uniform(0.5, 1.5, d)) + rng.standard_normal(d)
    return xa.mean(axis=0), np.cov(xa, rowvar=False).reshape(d, d), xb.mean(axis=0), np.cov(xb, rowvar=False).reshape(d, d)
