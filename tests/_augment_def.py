"""The definition the batch-assembly kernel (csrc/batch_assemble.hip) is held to, bit for bit: numpy and Python integers only, no
floating point anywhere.

Random words: ``philox4x32_10(seed, ctr_lo, ctr_hi)`` as csrc/philox.h defines it (key = the two halves of the 64-bit seed, counter =
the two 64-bit words, ten rounds, four 32-bit words out).  Sample ``i`` (its index in the cache) at epoch ``e`` draws
``A = philox(seed, i, 2 e)`` and ``B = philox(seed, i, 2 e + 1)``.

Parameters: a probability is a threshold ``th`` in [0, 2^32]; an event happens iff its word is ``< th``:
  hflip = A[0] < th_h, vflip = A[1] < th_v, k = A[2] >> 30 if quarter turns are on else 0, cropped = A[3] < th_c;
  cropped: ch = lo_h + ((B[0] (H - lo_h + 1)) >> 32), cw = clamp((2 ch W + H) // (2 H), 1, W), y0 = (B[1] (H - ch + 1)) >> 32,
  x0 = (B[2] (W - cw + 1)) >> 32; otherwise the box is the image.

Crop and resize back to H x W: bilinear with half-pixel centres, always a magnification.  Along an axis of ``n`` outputs over a box of
``c`` source positions from ``c0``: D = 2 n, num = (2 o + 1) c - n, i = floor(num / D) (a true floor: num is negative for the first
outputs of a small box), f = num - i D, taps c0 + clamp(i, 0, c - 1) and c0 + clamp(i + 1, 0, c - 1) (clamped to the box, not the
image), weights D - f and f.  A pixel is (acc + Dy Dx / 2) // (Dy Dx) with
acc = (Dy - fy) ((Dx - fx) p00 + fx p01) + fy ((Dx - fx) p10 + fx p11) in 64-bit integers.

Order: crop-resize, then ``C[:, ::-1]`` if hflip, ``C[::-1, :]`` if vflip, ``np.rot90(C, k)`` over (H, W); the same parameters for all
three channels and both images of a pair."""
from collections import namedtuple

import numpy as np

M32 = 0xFFFFFFFF
ONE = 1 << 32

Params = namedtuple("Params", "hflip vflip k cropped y0 x0 ch cw")


def philox4x32_10(seed: int, ctr_lo: int, ctr_hi: int):
    """Four 32-bit words, as ``hdiff::philox4x32_10`` (csrc/philox.h)."""
    return philox_raw((seed & M32, (seed >> 32) & M32), (ctr_lo & M32, (ctr_lo >> 32) & M32, ctr_hi & M32, (ctr_hi >> 32) & M32))


def philox_raw(key, counter):
    """Philox4x32-10 on (two key words, four counter words)."""
    c = [int(v) & M32 for v in counter]
    k0, k1 = int(key[0]) & M32, int(key[1]) & M32
    for _ in range(10):
        p0 = 0xD2511F53 * c[0]
        p1 = 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c[3] ^ k1) & M32, p0 & M32]
        k0 = (k0 + 0x9E3779B9) & M32
        k1 = (k1 + 0xBB67AE85) & M32
    return tuple(c)


def draw(seed: int, epoch: int, i: int, H: int, W: int, th_h: int, th_v: int, rot90: bool, th_c: int, lo_h: int) -> Params:
    """The parameters of sample ``i`` at ``epoch``."""
    assert 0 <= th_h <= ONE and 0 <= th_v <= ONE and 0 <= th_c <= ONE and 1 <= lo_h <= H and 0 <= epoch < 2 ** 31
    A = philox4x32_10(seed, i, 2 * epoch)
    B = philox4x32_10(seed, i, 2 * epoch + 1)
    hflip, vflip, cropped = A[0] < th_h, A[1] < th_v, A[3] < th_c
    k = (A[2] >> 30) if rot90 else 0
    if not cropped:
        return Params(hflip, vflip, k, False, 0, 0, H, W)
    ch = lo_h + ((B[0] * (H - lo_h + 1)) >> 32)
    cw = min(max((2 * ch * W + H) // (2 * H), 1), W)
    y0 = (B[1] * (H - ch + 1)) >> 32
    x0 = (B[2] * (W - cw + 1)) >> 32
    return Params(hflip, vflip, k, True, y0, x0, ch, cw)


def axis(n: int, c: int, c0: int):
    """(first tap, second tap, weight of the second tap of D = 2 n) for the ``n`` outputs over the box [c0, c0 + c), int64 arrays."""
    o = np.arange(n, dtype=np.int64)
    D = 2 * n
    num = (2 * o + 1) * c - n
    i = np.floor_divide(num, D)                   # numpy's integer floor_divide is a true floor
    f = num - i * D
    return c0 + np.clip(i, 0, c - 1), c0 + np.clip(i + 1, 0, c - 1), f


def crop_resize(img: np.ndarray, y0: int, x0: int, ch: int, cw: int) -> np.ndarray:
    """The box [y0, y0 + ch) x [x0, x0 + cw) of a uint8 [..., H, W] array magnified back to H x W."""
    img = np.asarray(img)
    assert img.dtype == np.uint8
    H, W = img.shape[-2:]
    assert 1 <= ch <= H and 1 <= cw <= W and 0 <= y0 <= H - ch and 0 <= x0 <= W - cw
    ya, yb, fy = axis(H, ch, y0)
    xa, xb, fx = axis(W, cw, x0)
    Dy, Dx = 2 * H, 2 * W
    src = img.astype(np.int64)
    fy, fx = fy[:, None], fx[None, :]
    p00, p01 = src[..., ya[:, None], xa[None, :]], src[..., ya[:, None], xb[None, :]]
    p10, p11 = src[..., yb[:, None], xa[None, :]], src[..., yb[:, None], xb[None, :]]
    acc = (Dy - fy) * ((Dx - fx) * p00 + fx * p01) + fy * ((Dx - fx) * p10 + fx * p11)
    out = (acc + (Dy * Dx) // 2) // (Dy * Dx)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def apply(img: np.ndarray, p: Params) -> np.ndarray:
    """One uint8 [3, H, W] (or [H, W]) image under the parameters ``p``."""
    C = crop_resize(img, p.y0, p.x0, p.ch, p.cw)
    if p.hflip:
        C = C[..., :, ::-1]
    if p.vflip:
        C = C[..., ::-1, :]
    return np.ascontiguousarray(np.rot90(C, p.k, axes=(-2, -1)))


def assemble_def(a: np.ndarray, b: np.ndarray, idx, *, seed: int, epoch: int, th_h: int = 0, th_v: int = 0, rot90: bool = False,
                 th_c: int = 0, lo_h=None):
    """(out_a, out_b) of a batch: uint8 [B, 3, H, W] each."""
    H, W = a.shape[-2:]
    lo_h = H if lo_h is None else lo_h
    ps = [draw(seed, epoch, int(i), H, W, th_h, th_v, rot90, th_c, lo_h) for i in idx]
    return (np.stack([apply(a[int(i)], p) for i, p in zip(idx, ps)]), np.stack([apply(b[int(i)], p) for i, p in zip(idx, ps)]))
