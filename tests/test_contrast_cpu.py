"""The contrast baselines without a GPU: the definition (tests/_contrast_def.py) against Pillow's ``ImageOps.equalize``, against closed
forms and a hand-worked plane, the margins of the fixtures tests/test_gpu_contrast.py holds the kernels to, and the host-side argument
checks of ``hdiff_amd.classical.clahe`` / ``equalize`` and of the baseline names."""
import numpy as np
import pytest
import torch

import _classical_def as CD
import _contrast_def as D
import _contrast_fixtures as F
from _uciqe_def import lab_def
from hdiff_amd import classical
from hdiff_amd.diffusion import Evaluate

f32, f64 = np.float32, np.float64


# ---------------------------------------------------------------------------------------------------------------- Pillow anchor
over_255_plane = F.over_255_plane


def test_equalize_is_pillows_byte_for_byte():
    from PIL import Image, ImageOps
    fx = F.byte_fixtures()
    # the fixtures are what their names say
    assert D.equalize_lut_def(fx["constant"][1]).tolist() == list(range(256))
    h = np.bincount(fx["step_0"][0].reshape(-1), minlength=256)
    assert np.count_nonzero(h) >= 2 and (320 - h[np.flatnonzero(h)[-1]]) // 255 == 0
    h = np.bincount(over_255_plane().reshape(-1), minlength=256)
    raw = (np.cumsum(h) - h)                                  # step = 1, step // 2 = 0
    assert (320 - h[255]) // 255 == 1 and raw[255] == 300 and raw[211] > 255 >= raw[210]
    assert (D.equalize_lut_def(over_255_plane())[211:] == 255).all()          # what Pillow's point() makes of them, checked next
    for name, planes in fx.items():
        pil = np.asarray(ImageOps.equalize(Image.fromarray(np.ascontiguousarray(planes.transpose(1, 2, 0)), "RGB"))).transpose(2, 0, 1)
        luts = np.stack([D.equalize_lut_def(p) for p in planes])
        assert np.array_equal(np.stack([t[p] for p, t in zip(planes, luts)]), pil), name
        got = D.equalize_def(F.bytes_image(planes), space="rgb")            # and through the float interface
        assert np.array_equal(got["q"], planes) and np.array_equal(got["q2"], pil), name
        assert np.array_equal(got["out"], (pil.astype(f64) / 255.0).astype(f32)), name
    for name in ("constant", "step_0"):                        # the identity cases leave the plane alone
        assert np.array_equal(D.equalize_def(F.bytes_image(fx[name]))["q2"][0], fx[name][0]), name


def test_equalize_lab_changes_lightness_alone():
    rng = np.random.default_rng(9)
    x = (0.2 + 0.3 * rng.random((3, 24, 24))).astype(f32)
    got = D.equalize_def(x, space="lab")
    assert got["q"].shape == (1, 24, 24) and got["lut"].shape == (1, 256)
    L, a, b = lab_def(got["out"].astype(f64))
    # where the new colour is inside the sRGB cube (elsewhere the clip to [0, 1] moves a and b too)
    raw = D.lab_to_srgb_def(got["q2"][0].astype(f64) / 2.55, got["lab"][1], got["lab"][2])
    inside = ((raw >= 0.0) & (raw <= 1.0)).all(axis=0)
    assert inside.mean() > 0.5
    assert np.abs(a - got["lab"][1])[inside].max() < 1e-4 and np.abs(b - got["lab"][2])[inside].max() < 1e-4      # fp32 output
    assert np.abs(L - got["q2"][0] / 2.55)[inside].max() < 1e-4
    assert L.std() > 2.0 * got["lab"][0].std()


# ---------------------------------------------------------------------------------------------------------------- CLAHE
@pytest.mark.parametrize("shape,grid", F.GEOMETRIES)
def test_redistribution_keeps_the_area_and_tables_rise(shape, grid):
    area = D.tile_geometry(shape[0], shape[1], grid)[2]
    for clip_limit in F.CLIP_LIMITS:
        for kind in F.kinds_for(shape):
            for img in F.fixture(kind, shape, 1):
                for plane in D.quantise_def(D.clipped(img), "rgb")[0]:
                    lut, h = D.clahe_luts_def(plane, grid, clip_limit, return_hist=True)
                    assert (h.sum(axis=-1) == area).all() and (h >= 0).all(), (kind, clip_limit)
                    assert (np.diff(lut.astype(np.int64), axis=-1) >= 0).all() and (lut[..., -1] == 255).all(), (kind, clip_limit)
                    if clip_limit > 0:
                        clip = D.clip_level(clip_limit, area)
                        assert h.max() <= clip + area // 256 + 1


def test_clip_levels():
    assert D.clip_level(0.0, 1024) == 1024 and D.clip_level(2.0, 1024) == 8 and D.clip_level(40.0, 1024) == 160
    assert D.clip_level(1e-6, 1024) == 1 and D.clip_level(2.0, 1) == 1 and D.clip_level(1e9, 35) == 35
    assert D.clip_level(float("inf"), 35) == 35
    for shape, grid in F.GEOMETRIES:
        assert D.clip_level(1e-6, D.tile_geometry(shape[0], shape[1], grid)[2]) == 1
        assert classical._tile_constants(*shape, *grid, 40.0)[0] == D.clip_level(40.0, D.tile_geometry(*shape, grid)[2])


def test_remainder_fixture_takes_every_step():
    """One tile at clip 1: the three channels leave excess % 256 = 1, 100 and 200 -- the steps 256, 2 and 1."""
    for shape in ((19, 24), (75, 101)):
        q = D.quantise_def(D.clipped(F.fixture("remainder", shape, 1)[0]), "rgb")[0]
        rs = [int(np.maximum(D.tile_histograms(p, (1, 1)) - 1, 0).sum() % 256) for p in q]
        assert rs == [1, 100, 200] and [max(256 // r, 1) for r in rs] == [256, 2, 1]
        for p, r in zip(q, rs):
            raw = D.tile_histograms(p, (1, 1))[0, 0]
            h = D.clahe_luts_def(p, (1, 1), 1e-6, return_hist=True)[1][0, 0]
            excess = int(np.maximum(raw - 1, 0).sum())
            bumped = np.flatnonzero(h - (np.minimum(raw, 1) + excess // 256))
            assert bumped.tolist() == [k * (256 // r) for k in range(r)]


def test_one_tile_without_clipping_is_plain_equalisation():
    rng = np.random.default_rng(12)
    for shape in ((8, 8), (19, 24), (75, 101)):
        plane = rng.integers(0, 256, shape).astype(np.uint8)
        cdf = np.cumsum(np.bincount(plane.reshape(-1), minlength=256))
        want = np.minimum(np.rint(cdf.astype(f32) * (f32(255.0) / f32(plane.size))), 255).astype(np.uint8)
        lut = D.clahe_luts_def(plane, (1, 1), 0.0)
        assert lut.shape == (1, 1, 256) and np.array_equal(lut[0, 0], want)
        # one table on every side of every pixel: the blend of four equal integers rounds back to the integer
        assert np.array_equal(D.blend_def(plane, lut, (1, 1)), want[plane])
        out = D.clahe_def(F.bytes_image(np.stack([plane] * 3)), clip_limit=0.0, grid=(1, 1), space="rgb")
        assert np.array_equal(out["q2"][1], want[plane]) and np.array_equal(out["out"][1], (want[plane].astype(f64) / 255.0).astype(f32))


def test_hand_worked_plane():
    """4 x 4 on a (2, 2) grid, no clipping.  Tiles are 2 x 2, area 4, scale 63.75, so a table is 0, 64, 128 (127.5 to even), 191 or
    255 after 0, 1, 2, 3 or 4 of the tile's pixels.  inv_tw = 0.5: columns 0 and 1 read the left tiles alone (fx = -0.5 -> both
    indices 0; fx = 0 -> weight 1 on tile 0), column 2 reads both at 1/2 (fx = 0.5), column 3 the right tiles alone (fx = 1); rows
    likewise."""
    plane = np.array([[0, 0, 10, 20],
                      [0, 5, 30, 40],
                      [7, 7, 200, 200],
                      [7, 7, 200, 255]], dtype=np.uint8)
    lut = D.clahe_luts_def(plane, (2, 2), 0.0)

    def table(steps):                                 # {first level: value from there on}
        t = np.zeros(256, dtype=np.uint8)
        for at, value in steps.items():
            t[at:] = value
        return t

    assert np.array_equal(lut[0, 0], table({0: 191, 5: 255}))                      # 0, 0, 0, 5
    assert np.array_equal(lut[0, 1], table({10: 64, 20: 128, 30: 191, 40: 255}))   # 10, 20, 30, 40
    assert np.array_equal(lut[1, 0], table({7: 255}))                              # 7, 7, 7, 7
    assert np.array_equal(lut[1, 1], table({200: 191, 255: 255}))                  # 200, 200, 200, 255
    want = np.array([[191, 191, 160, 128],        # (0, 2): (255 + 64) / 2 = 159.5 -> 160;   (0, 3): table 01 at 20
                     [191, 255, 223, 255],        # (1, 2): (255 + 191) / 2 = 223
                     [255, 255, 239, 223],        # (2, 2): ((255 + 255) / 2 + (255 + 191) / 2) / 2 = 239;   (2, 3): (255 + 191) / 2
                     [255, 255, 223, 255]], dtype=np.uint8)
    got, res = D.blend_def(plane, lut, (2, 2), return_res=True)
    assert np.array_equal(got, want) and res[0, 2] == 159.5
    # with a clip of 1 (clip_limit 64 -> 64 * 4 / 256) tile 10 keeps 1 of its 4 pixels in bin 7 and hands 3 out: excess // 256 = 0, r = 3,
    # step = 85 -> bins 0, 85, 170.  cumsum: 1 from 0, 2 from 7, 3 from 85, 4 from 170.
    clipped = D.clahe_luts_def(plane, (2, 2), 64.0)
    assert np.array_equal(clipped[1, 0], table({0: 64, 7: 128, 85: 191, 170: 255}))


def test_reflect_101_padding():
    plane = np.arange(5 * 7, dtype=np.uint8).reshape(5, 7)
    h = D.tile_histograms(plane, (2, 3))                  # padded to 6 x 9: row 5 is row 3, columns 7 and 8 are columns 5 and 4
    assert h.shape == (2, 3, 256) and (h.sum(axis=-1) == 9).all()
    padded = np.concatenate([plane, plane[3:4]], axis=0)
    padded = np.concatenate([padded, padded[:, 5:6], padded[:, 4:5]], axis=1)
    for ty in range(2):
        for tx in range(3):
            assert np.array_equal(h[ty, tx], np.bincount(padded[3 * ty:3 * ty + 3, 3 * tx:3 * tx + 3].reshape(-1), minlength=256))


# ---------------------------------------------------------------------------------------------------------------- colour
def test_lab_round_trip():
    g = np.linspace(0.0, 1.0, 18)
    rgb = np.stack(np.meshgrid(g, g, g, indexing="ij")).reshape(3, -1)
    back = D.lab_to_srgb_def(*lab_def(rgb))
    print("lab round trip: max |x' - x| =", np.abs(back - rgb).max())
    assert np.abs(back - rgb).max() <= 1e-12
    inv = np.array(D.matrix_inverse())
    assert np.abs(inv @ np.array(D.MATRIX) - np.eye(3)).max() < 1e-15


# ---------------------------------------------------------------------------------------------------------------- fixture margins
@pytest.mark.parametrize("shape,grid", F.GEOMETRIES)
def test_fixture_margins(shape, grid):
    """No fixture of the GPU tests hangs on a tie: L 2.55 + 0.5 stays 1e-9 off an integer, and every "rgb" blend is either carried out
    without a rounding or stays 1e-4 off a .5."""
    H, W = shape
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for clip_limit in F.CLIP_LIMITS:
        for kind in F.kinds_for(shape):
            x, raw = F.case_images(kind, shape, grid, clip_limit), F.fixture(kind, shape, F.BATCH[kind])
            # what settling may not touch: one table around every pixel, one pixel per tile (dyadic weights), a constant plane
            if grid == (1, 1) or (shape, grid) == ((8, 8), (8, 8)) or kind == "constant":
                assert np.array_equal(x, raw), (kind, clip_limit)
            for img in x:
                x = D.clipped(img)
                v = lab_def(x.astype(f64))[0] * 2.55 + 0.5
                assert np.abs(v - np.rint(v)).min() >= 1e-9, (kind, clip_limit)
                for plane in D.quantise_def(x, "rgb")[0]:
                    lut = D.clahe_luts_def(plane, grid, clip_limit)
                    r32 = D.blend_at(lut, shape, grid, yy, xx, plane).astype(f64)
                    rounded = r32 != D.blend_at(lut, shape, grid, yy, xx, plane, dtype=f64)
                    assert (np.abs((r32[rounded] - np.floor(r32[rounded])) - 0.5) >= F.TIE_MARGIN).all(), (kind, clip_limit)
                    assert F.TIE_MARGIN == 1e-4 and not F.near_tie(lut, shape, grid, yy, xx, plane).any()


def test_equalize_fixture_margins_and_cases():
    fx = F.equalize_fixtures()
    for name, batch in fx.items():
        for img in batch:
            v = lab_def(D.clipped(img).astype(f64))[0] * 2.55 + 0.5
            assert np.abs(v - np.rint(v)).min() >= 1e-9, name
    # the "lab" planes of the grey fixtures are the cases their names say
    q = D.quantise_def(D.clipped(fx["grey_over_255"][0]), "lab")[0][0]
    h = np.bincount(q.reshape(-1), minlength=256)
    assert h[255] == 20 and (320 - h[255]) // 255 == 1 and (np.cumsum(h) - h)[255] == 300
    assert D.equalize_lut_def(q)[255] == 255 and (D.equalize_lut_def(q).astype(np.int64) < (np.cumsum(h) - h)).any()
    q = D.quantise_def(D.clipped(fx["grey_step_0"][0]), "lab")[0][0]
    h = np.bincount(q.reshape(-1), minlength=256)
    assert np.count_nonzero(h) == 2 and (320 - h[np.flatnonzero(h)[-1]]) // 255 == 0
    for name in ("grey_step_0", "colour", "constant"):
        got = D.equalize_def(fx[name][0], space="lab")
        assert np.array_equal(got["lut"][0], np.arange(256)) and np.array_equal(got["q2"], got["q"]), name


# ---------------------------------------------------------------------------------------------------------------- names and arguments
def test_baseline_names():
    assert set(classical.BASELINES) == {"input", "gray_world", "dcp", "udcp", "inverted_dcp"}
    assert set(classical.CONTRAST_BASELINES) == {"clahe_lab", "clahe_rgb", "equalize"}
    with pytest.raises(ValueError, match="clahe_lab"):                     # the message lists both tables
        classical.resolve_baselines(("input", "clahe"))
    got = classical.resolve_baselines(("input", "clahe_lab", "equalize", ("mine", lambda x: x)))
    assert [n for n, _ in got] == ["input", "clahe_lab", "equalize", "mine"]
    assert got[1][1] is classical.CONTRAST_BASELINES["clahe_lab"] and got[0][1] is classical.BASELINES["input"]
    with pytest.raises(ValueError):
        classical.resolve_baselines(("clahe_rgb", "clahe_rgb"))

    def sampler(*a, **k):
        raise AssertionError("the sampler must not run")

    with pytest.raises(ValueError):
        Evaluate.evaluate(sampler, iter(()), ddim_step=2, baselines=("input", "clahe"))


def test_argument_checks_come_before_any_device_work():
    cpu = torch.zeros(1, 3, 8, 8)
    for bad in (dict(grid=(0, 8)), dict(grid=(8, 17)), dict(grid=(8,)), dict(grid=8), dict(grid=(2.0, 2)), dict(grid=(9, 8)),
                dict(grid=(1, 9)), dict(clip_limit=-1.0), dict(clip_limit=float("nan")), dict(space="hsv"), dict(space="LAB")):
        with pytest.raises(ValueError):
            classical.clahe(cpu, **bad)
    with pytest.raises(TypeError):
        classical.clahe(cpu, clip_limit="2")
    with pytest.raises(ValueError):
        classical.equalize(cpu, space="luv")
    with pytest.raises(ValueError):
        classical.clahe(torch.zeros(1, 1, 8, 8))
    # good settings reach the tensor check: CPU tensors are refused, there is no fallback
    for call in (lambda: classical.clahe(cpu), lambda: classical.clahe(cpu, clip_limit=0, grid=(1, 1), space="rgb"),
                 lambda: classical.equalize(cpu), lambda: classical.equalize(cpu, space="lab"),
                 lambda: classical.CONTRAST_BASELINES["clahe_rgb"](cpu)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_host_constants_are_the_fp32_quotients():
    for shape, grid in F.GEOMETRIES + (((3024, 4032), (8, 8)), ((32768, 32768), (1, 1)), ((1000, 777), (16, 13))):
        clip, scale, inv_th, inv_tw = classical._tile_constants(*shape, *grid, 2.0)
        want = D.host_constants(shape[0], shape[1], grid)
        assert (f32(inv_th), f32(inv_tw), f32(scale)) == want and (inv_th, inv_tw, scale) == tuple(float(v) for v in want)
        assert clip == D.clip_level(2.0, D.tile_geometry(shape[0], shape[1], grid)[2])


# ---------------------------------------------------------------------------------------------------------------- effect
def test_clahe_widens_the_lightness_of_the_haze_set():
    """Measured with this definition on the eight 64 x 64 procedural scenes under the haze preset, means over the scenes: the
    standard deviation of L* 4.364 -> 6.907 (+2.543; the clean scenes have 12.337), PSNR against the clean scene 11.31 -> 9.67 dB.
    CLAHE stretches local contrast and does not invert the veil: PSNR falls, and nothing is asserted about it."""
    clean, deg = CD.scene_sets()["haze"]

    def spread(im):
        return float(lab_def(D.clipped(im).astype(f64))[0].std())

    outs = [D.clahe_def(deg[i], space="lab")["out"] for i in range(8)]
    before, after = np.mean([spread(deg[i]) for i in range(8)]), np.mean([spread(o) for o in outs])
    p0 = np.mean([CD.psnr(deg[i], clean[i]) for i in range(8)])
    p1 = np.mean([CD.psnr(outs[i], clean[i]) for i in range(8)])
    print(f"haze: std of L* {before:.3f} -> {after:.3f}; PSNR {p0:.2f} -> {p1:.2f} dB")
    assert after - before >= 0.5 * 2.543
