"""The fixtures of the contrast tests (tests/test_contrast_cpu.py, tests/test_gpu_contrast.py), apart from the definition they are
checked against (tests/_contrast_def.py): the image kinds, the cases (geometries x clip limits x kinds), the byte planes of the
equalisation, and the machinery that keeps every "rgb" blend of a case clear of a tie.

``settle`` changes what some fixtures are.  It first trades pixel values inside a tile's histogram, which keeps every level and every
table; where no partner exists it gives the pixel a neighbouring byte, which adds a level.  ``constant`` is never changed.  Under the
(1, 1) grid (one table on every side of a pixel: a blend of four equal integers) nothing is changed at all, so ``remainder`` has its
three remainders exactly where its steps are asserted and ``two_level`` two levels; the same holds with one pixel per tile (8 x 8
under (8, 8), where every weight is a multiple of 1/4); tests/test_contrast_cpu.py asserts all three.  Under the other grids a ``two_level`` plane ends with up to 35 levels and a ``remainder`` plane
with up to 224 altered pixels: there they are "mostly two-level" and "long constant runs", no more."""
import numpy as np

from _contrast_def import blend_at, clahe_luts_def, clipped, f32, f64, quantise_def, tile_geometry

TIE_MARGIN = 1e-4


def near_tie(lut: np.ndarray, shape, grid, ys, xs, vs) -> np.ndarray:
    """True where the fp32 ``res`` is BOTH rounded (it differs from the same expression carried out in double) AND within
    ``TIE_MARGIN`` of a ``.5``: where the byte could hang on the last bit of an fp32 operation."""
    r32 = blend_at(lut, shape, grid, ys, xs, vs).astype(f64)
    r64 = blend_at(lut, shape, grid, ys, xs, vs, dtype=f64)
    return (r32 != r64) & (np.abs((r32 - np.floor(r32)) - 0.5) < TIE_MARGIN)


def swap_groups(shape, grid) -> np.ndarray:
    """int64 ``[H, W]``: two pixels carry the same number iff every tile counts them equally often (the pixel itself and its mirror
    images in the padding), so that exchanging their values leaves every tile's histogram -- every table -- as it was."""
    H, W = shape
    th, tw, _, Hp, Wp = tile_geometry(H, W, grid)
    source = np.pad(np.arange(H * W).reshape(H, W), ((0, Hp - H), (0, Wp - W)), mode="reflect")
    tile = (np.arange(Hp)[:, None] // th) * grid[1] + (np.arange(Wp)[None, :] // tw)
    # a pixel's multiset of tiles as the sum of one fixed 62-bit number per tile and appearance
    mark = np.random.default_rng(257).integers(1, 2 ** 62, grid[0] * grid[1], dtype=np.int64)
    key = np.zeros(H * W, dtype=np.int64)
    np.add.at(key, source.reshape(-1), mark[np.broadcast_to(tile, source.shape).reshape(-1)])
    return np.unique(key, return_inverse=True)[1].reshape(H, W)


def settle(x: np.ndarray, grid, clip_limit: float) -> np.ndarray:
    """fp32 ``[n, 3, H, W]`` -> the same images with a few pairs of pixel values exchanged inside a channel, so that no ``"rgb"``
    blend of the result is ``near_tie``: a pixel whose blend is, trades its value with a pixel of its swap group where both blends
    are clear of one.  The tables do not move under such an exchange.  A pixel without such a partner (a small group, or one value
    throughout it) takes a neighbouring byte instead; that moves the tables, so the plane is gone through again."""
    x = np.array(x)
    H, W = x.shape[2:]
    groups = swap_groups((H, W), grid)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for img in x:
        for c in range(3):
            for attempt in range(1, 33):
                q = quantise_def(clipped(img), "rgb")[0][c]
                lut = clahe_luts_def(q, grid, clip_limit)
                bad = near_tie(lut, (H, W), grid, yy, xx, q)
                if not bad.any():
                    break
                free = ~bad
                for y, xcol in zip(*np.nonzero(bad)):
                    ys, xs = np.nonzero(free & (groups == groups[y, xcol]))
                    ok = ~near_tie(lut, (H, W), grid, np.full(ys.shape, y), np.full(xs.shape, xcol), q[ys, xs]) \
                        & ~near_tie(lut, (H, W), grid, ys, xs, np.full(ys.shape, q[y, xcol]))
                    if ok.any():
                        k = int(np.flatnonzero(ok)[0])
                        y2, x2 = ys[k], xs[k]
                        img[c, y, xcol], img[c, y2, x2] = img[c, y2, x2], img[c, y, xcol]
                        free[y2, x2] = False
                    else:
                        img[c, y, xcol] = f32(f64((int(q[y, xcol]) + attempt) % 256) / 255.0)
            else:
                raise AssertionError(f"channel {c} does not settle: grid {grid}, clip_limit {clip_limit}")
    return x


def bytes_image(planes) -> np.ndarray:
    """uint8 ``[3, H, W]`` -> the fp32 image whose "rgb" quantisation is exactly those bytes."""
    return (np.asarray(planes, dtype=np.uint8).astype(f64) / 255.0).astype(f32)


def fixture(kind: str, shape, n: int = 3, seed: int = 0) -> np.ndarray:
    """fp32 ``[n, 3, H, W]``.  ``noise``: a smooth colour field under noise, in [-0.1, 1.1] (the clip has work to do); ``constant``: one
    level per image and channel (all of a tile's excess comes from one bin); ``two_level``: two levels split along a diagonal;
    ``ramp``: a horizontal ramp with a vertical one in another channel; ``remainder``: byte planes of three constant-run patterns
    whose single-tile histogram at clip 1 leaves excess % 256 = 1, 100 and 200 -- the steps 256, 2 and 1 of the redistribution
    (checked in tests/test_contrast_cpu.py); it needs at least 216 pixels."""
    H, W = shape
    rng = np.random.default_rng([seed, H, W, n, sum(map(ord, kind))])
    yy, xx = np.meshgrid(np.arange(H, dtype=f64), np.arange(W, dtype=f64), indexing="ij")
    if kind == "noise":
        field = np.stack([[0.5 + 0.45 * np.sin(yy / 9 + c + i) * np.cos(xx / 7 - c) for c in range(3)] for i in range(n)])
        x = (field + 0.3 * (rng.random((n, 3, H, W)) - 0.5)).astype(f32)
    elif kind == "constant":
        x = np.broadcast_to(rng.integers(0, 256, (n, 3, 1, 1)).astype(f64) / 255.0, (n, 3, H, W)).astype(f32)
    elif kind == "two_level":
        lo, hi = rng.integers(0, 100, (n, 3, 1, 1)), rng.integers(150, 256, (n, 3, 1, 1))
        x = (np.where((yy * W + xx * H) < (H * W), lo, hi).astype(f64) / 255.0).astype(f32)
    elif kind == "ramp":
        rx, ry = xx / max(W - 1, 1), yy / max(H - 1, 1)
        x = np.stack([np.stack([rx, ry, 0.5 * (rx + ry)]) * (1.0 - 0.2 * i) for i in range(n)]).astype(f32)
    elif kind == "remainder":
        assert H * W >= 216
        planes = np.empty((n, 3, H * W), dtype=np.uint8)
        for c, distinct in enumerate(remainder_levels(H * W)):
            planes[:, c] = np.minimum(np.arange(H * W), distinct - 1)       # `distinct` levels: excess at clip 1 is H W - distinct
        x = np.stack([bytes_image(np.roll(p, 7 * i, axis=1).reshape(3, H, W)) for i, p in enumerate(planes)])
    else:
        raise ValueError(kind)
    return x + f32(0.0)                          # no -0


# the cases of tests/test_gpu_contrast.py, whose margins tests/test_contrast_cpu.py asserts: 8 x 8 under (8, 8) has one pixel per tile;
# 19 x 24 is padded to 24 x 24 by (8, 8) and to 20 x 24 by (2, 3); 75 x 101 is padded on both axes by every grid but (1, 1), by more
# than a tile's width (11 columns, tiles of 7) under (16, 16)
GEOMETRIES = (((8, 8), (1, 1)), ((8, 8), (2, 3)), ((8, 8), (8, 8)), ((19, 24), (1, 1)), ((19, 24), (2, 3)), ((19, 24), (8, 8)),
              ((75, 101), (1, 1)), ((75, 101), (2, 3)), ((75, 101), (8, 8)), ((75, 101), (16, 16)))
CLIP_LIMITS = (0.0, 2.0, 40.0, 1e-6)            # 1e-6: floor(clip_limit area / 256) = 0 at every tile here, so clip == 1
KINDS = ("noise", "constant", "two_level", "ramp", "remainder")


BATCH = {"noise": 3, "constant": 1, "two_level": 1, "ramp": 1, "remainder": 1}


def kinds_for(shape):
    return tuple(k for k in KINDS if k != "remainder" or shape[0] * shape[1] >= 216)


_settled = {}


def case_images(kind: str, shape, grid, clip_limit: float) -> np.ndarray:
    """The fixture of one case (``BATCH[kind]`` images), settled for that case's tables; built once."""
    key = (kind, tuple(shape), tuple(grid), float(clip_limit))
    if key not in _settled:
        x = settle(fixture(kind, shape, BATCH[kind]), grid, clip_limit)
        x.setflags(write=False)
        _settled[key] = x
    return _settled[key]


def over_255_plane() -> np.ndarray:
    """16 x 20 bytes: the levels 0..254 once and 0..44 a second time, then twenty pixels of 255.  step = (320 - 20) // 255 = 1, so
    lut[i] = sum(h[:i]), which reaches 300 at i = 255 and passes 255 from i = 211 on."""
    return np.concatenate([np.arange(300) % 255, np.full(20, 255)]).astype(np.uint8).reshape(16, 20)


def byte_fixtures() -> dict:
    """uint8 ``[3, H, W]`` planes for the equalisation: what Pillow is asked about, and (through ``bytes_image``) the device."""
    rng = np.random.default_rng(8)
    ramp = (np.arange(16 * 20) % 256).astype(np.uint8).reshape(16, 20)
    two = np.where(np.arange(320).reshape(16, 20) < 100, 30, 200).astype(np.uint8)
    few = np.where(np.arange(320).reshape(16, 20) < 100, 3, 9).astype(np.uint8)      # 320 - 220 = 100 < 255: step == 0
    noise = rng.integers(0, 256, (3, 48, 64)).astype(np.uint8)
    dark = (rng.integers(0, 256, (48, 64)) // 4).astype(np.uint8)
    return {
        "constant": np.stack([np.full((16, 20), v, dtype=np.uint8) for v in (0, 77, 255)]),
        "two_level": np.stack([two, 255 - two, np.where(two == 30, 0, 255).astype(np.uint8)]),
        "step_0": np.stack([few, ramp[:, ::-1].copy(), rng.integers(0, 256, (16, 20)).astype(np.uint8)]),
        "over_255": np.stack([over_255_plane(), over_255_plane()[::-1].copy(), ramp]),
        "noise": noise,
        "dark": np.stack([dark, noise[0], 255 - dark]),
    }


def equalize_fixtures() -> dict:
    """fp32 ``[n, 3, H, W]`` batches for the equalisation in both spaces: the byte fixtures; greys of the identity and over-255 planes
    (in "lab" a grey byte b has q = its lightness level, increasing in b, so the L plane of ``grey_over_255`` has the same
    histogram shape: step 1, entries up to 300) and a constant colour; noise on 75 x 101 (more than one workgroup's share of pixels
    per plane) in a batch of 3."""
    out = {name: bytes_image(planes)[None] for name, planes in byte_fixtures().items()}
    out["grey_over_255"] = bytes_image(np.stack([over_255_plane()] * 3))[None]
    out["grey_step_0"] = bytes_image(np.stack([byte_fixtures()["step_0"][0]] * 3))[None]
    out["colour"] = np.broadcast_to(np.array([0.3, 0.55, 0.8], dtype=f32)[None, :, None, None], (1, 3, 9, 13)).copy()
    out["noise_75x101"] = fixture("noise", (75, 101), 3, seed=4)
    return out


def remainder_levels(pixels: int):
    """The numbers of distinct byte levels (at most 256) of the ``remainder`` planes: a plane of `pixels` pixels with d distinct
    levels, each taken once but the last, has excess pixels - d at clip 1; d is chosen so that excess % 256 is 1, 100 and 200."""
    out = []
    for want in (1, 100, 200):
        d = next(d for d in range(min(pixels - 1, 256), 0, -1) if (pixels - d) % 256 == want)
        out.append(d)
    return out
