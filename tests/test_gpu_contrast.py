"""GPU checks of the contrast baselines (csrc/contrast.hip, hdiff_amd/classical.clahe / equalize) and of their names in the evaluation
loop, against the definition of tests/_contrast_def.py.

Gates.  The quantisation is an exact double product and a floor; a histogram, its clipping, the redistribution and the prefix sum are
integers; a table entry is one fp32 product rounded to nearest even; the blend is seven fp32 operations in a written order; q' / 255 is
one double division rounded once.  So in "rgb" q, every table and the output are held BIT FOR BIT, no element excluded.  In "lab" q
passes through pow and cbrt in double, whose last bits need not agree between two libraries: the fixtures keep L 2.55 + 0.5 at
least 1e-9 from an integer (asserted in tests/test_contrast_cpu.py), so q and the tables are bit for bit too, and the output -- the
inverse conversion in double, rounded once -- is held to the definition's fp32 value or its neighbour for CLAHE; every such test prints
how many elements met the value itself (all of them, on the MI355X).  The equalisation is held BIT FOR BIT in both spaces, output
included: its "lab" output goes through the same conversion and met the value in every element, and that is asserted.

Cases (tests/_contrast_fixtures.GEOMETRIES x CLIP_LIMITS x KINDS): 8 x 8 to 75 x 101; grids (1, 1), (2, 3), (8, 8) -- one pixel per tile on
8 x 8 -- and (16, 16) on 75 x 101, where both axes are padded, the columns by more than a tile; clip_limit 0, 2, 40 and 1e-6 (clip ==
1); noise in batches of 3, a constant, a two-level image, a ramp, and the planes whose excess % 256 takes the steps 256, 2 and 1.  The
fixtures are settled so that no blend hangs on a tie (tests/_contrast_fixtures.py): under the (1, 1) grid and with one pixel per tile
nothing is changed, so the remainder planes take their steps and the two-level planes have two levels exactly there, and the constant
is never changed; under the other grids pixels trade values or move by a byte, so "two-level", "ramp" and "remainder" describe those
planes only approximately (a two-level plane ends with up to 35 levels)."""
import functools
import gc
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hdiff_amd  # noqa: E402,F401
from hdiff_amd import classical as CL  # noqa: E402
from hdiff_amd import quality as Q  # noqa: E402
from hdiff_amd.diffusion import Evaluate as EV  # noqa: E402

import _contrast_def as D  # noqa: E402
import _contrast_fixtures as F  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_POOL = {}


@pytest.fixture(scope="module", autouse=True)
def private_memory_pool():
    """Every allocation of this module comes from a pool of its own: the caching allocator's default pool, whose leftover blocks
    later tests' memory accounting depends on (tests/test_gpu_fused_dropout.py), is left as this module found it.  The pool is kept
    until the process ends (a few hundred KB): releasing it empties cached blocks, which is a change of the allocator's state too."""
    with torch.cuda.use_mem_pool(_POOL.setdefault("pool", torch.cuda.MemPool())):
        yield
    big.cache_clear()
    gc.collect()
    torch.cuda.synchronize()


def bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return a.view(np.int32) if a.dtype == np.float32 else a


def arr(v):
    return v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)


def same(got, want):
    got, want = bits(got), bits(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want)


@functools.lru_cache(maxsize=None)
def big():
    """The batch of the whole-call tests: 3 noise images at 75 x 101, on the device."""
    return torch.from_numpy(F.fixture("noise", (75, 101), 3, seed=1)).to(DEV)


# ---------------------------------------------------------------------------------------------------------------- CLAHE
@pytest.mark.parametrize("shape,grid", F.GEOMETRIES)
def test_clahe_rgb_is_the_definition_bit_for_bit(shape, grid):
    for clip_limit in F.CLIP_LIMITS:
        for kind in F.kinds_for(shape):
            x = F.case_images(kind, shape, grid, clip_limit)
            out, parts = CL.clahe(torch.tensor(x, device=DEV), clip_limit=clip_limit, grid=grid, space="rgb", return_parts=True)
            assert out.dtype == torch.float32 and tuple(out.shape) == x.shape
            assert parts["q"].dtype == torch.uint8 and tuple(parts["q"].shape) == x.shape
            assert parts["lut"].dtype == torch.uint8 and tuple(parts["lut"].shape) == (x.shape[0], 3) + tuple(grid) + (256,)
            for i, im in enumerate(x):
                want = D.clahe_def(im, clip_limit=clip_limit, grid=grid, space="rgb")
                where = (kind, clip_limit, i)
                assert same(parts["q"][i], want["q"]), ("q",) + where
                assert same(parts["lut"][i], want["lut"]), ("lut",) + where
                assert same(out[i], want["out"]), ("out",) + where


@pytest.mark.parametrize("shape,grid", F.GEOMETRIES)
def test_clahe_lab_against_the_definition(shape, grid):
    met = total = 0
    for clip_limit in F.CLIP_LIMITS:
        for kind in F.kinds_for(shape):
            x = F.case_images(kind, shape, grid, clip_limit)
            out, parts = CL.clahe(torch.tensor(x, device=DEV), clip_limit=clip_limit, grid=grid, space="lab", return_parts=True)
            assert tuple(parts["q"].shape) == (x.shape[0], 1) + shape
            assert tuple(parts["lut"].shape) == (x.shape[0], 1) + tuple(grid) + (256,)
            for i, im in enumerate(x):
                want = D.clahe_def(im, clip_limit=clip_limit, grid=grid, space="lab")
                where = (kind, clip_limit, i)
                assert same(parts["q"][i], want["q"]), ("q",) + where
                assert same(parts["lut"][i], want["lut"]), ("lut",) + where
                ok, off = D.neighbours_ok(out[i].cpu().numpy(), want["out"])
                total += want["out"].size
                met += want["out"].size - off
                assert ok, ("out",) + where
    print(f"clahe lab {shape} {grid}: {met} of {total} output elements met the definition's fp32 value itself")


def test_defaults_and_the_named_baselines():
    x = big()
    want = [D.clahe_def(im) for im in x.cpu().numpy()]                       # clip_limit 2.0, grid (8, 8), "lab"
    out, parts = CL.clahe(x, return_parts=True)
    for i, w in enumerate(want):
        assert same(parts["q"][i], w["q"]) and same(parts["lut"][i], w["lut"]) and D.neighbours_ok(out[i].cpu().numpy(), w["out"])[0]
    assert same(CL.CONTRAST_BASELINES["clahe_lab"](x), out)
    assert same(CL.CONTRAST_BASELINES["clahe_rgb"](x), CL.clahe(x, clip_limit=2.0, grid=(8, 8), space="rgb"))
    assert same(CL.CONTRAST_BASELINES["equalize"](x), CL.equalize(x, space="rgb"))
    assert same(CL.clahe(x.double()), out) and same(CL.clahe(x.half()), CL.clahe(x.half().float()))
    # a clip above the tile's area clips nothing: clip_limit 1e9 and inf are clip_limit 0
    for big_limit in (1e9, float("inf")):
        assert same(CL.clahe(x, clip_limit=big_limit, space="rgb"), CL.clahe(x, clip_limit=0, space="rgb"))


# ---------------------------------------------------------------------------------------------------------------- equalisation
@pytest.mark.parametrize("space", ("rgb", "lab"))
def test_equalize_against_the_definition(space):
    seen = set()
    for name, x in F.equalize_fixtures().items():
        out, parts = CL.equalize(torch.from_numpy(x).to(DEV), space=space, return_parts=True)
        planes = {"rgb": 3, "lab": 1}[space]
        assert tuple(parts["q"].shape) == (x.shape[0], planes) + x.shape[2:] and tuple(parts["lut"].shape) == (x.shape[0], planes, 256)
        for i, im in enumerate(x):
            want = D.equalize_def(im, space=space)
            assert same(parts["q"][i], want["q"]), ("q", name, i)
            assert same(parts["lut"][i], want["lut"]), ("lut", name, i)
            for plane, lut in zip(want["q"], want["lut"]):
                h = np.bincount(plane.reshape(-1), minlength=256)
                step = (plane.size - int(h[np.flatnonzero(h)[-1]])) // 255
                if np.count_nonzero(h) < 2:
                    seen.add("identity: one bin")
                elif step == 0:
                    seen.add("identity: step 0")
                elif ((step // 2 + np.cumsum(h) - h) // step > 255).any():
                    seen.add("over 255")
            assert same(out[i], want["out"]), ("out", name, i)
    assert seen == {"identity: one bin", "identity: step 0", "over 255"}, seen


def test_equalize_is_pillows_on_the_device():
    """The anchor itself, end to end: bytes in, the device's output times 255, against ``PIL.ImageOps.equalize``."""
    from PIL import Image, ImageOps
    for name, planes in F.byte_fixtures().items():
        pil = np.asarray(ImageOps.equalize(Image.fromarray(np.ascontiguousarray(planes.transpose(1, 2, 0)), "RGB"))).transpose(2, 0, 1)
        out = CL.equalize(torch.from_numpy(F.bytes_image(planes)[None]).to(DEV), space="rgb")[0]
        assert np.array_equal(np.rint(out.cpu().numpy().astype(np.float64) * 255.0).astype(np.uint8), pil), name


# ---------------------------------------------------------------------------------------------------------------- whole calls
CALLS = (("clahe rgb", lambda x: CL.clahe(x, space="rgb", return_parts=True)),
         ("clahe lab", lambda x: CL.clahe(x, grid=(2, 3), clip_limit=40.0, return_parts=True)),
         ("equalize rgb", lambda x: CL.equalize(x, return_parts=True)),
         ("equalize lab", lambda x: CL.equalize(x, space="lab", return_parts=True)))


def test_results_repeat_and_do_not_depend_on_the_batch():
    x = big()
    for name, call in CALLS:
        first, again, alone = call(x), call(x), call(x[2:3])
        assert same(first[0], again[0]) and same(first[0][2], alone[0][0]), name
        for k in ("q", "lut"):
            assert same(first[1][k], again[1][k]) and same(first[1][k][2], alone[1][k][0]), (name, k)


def test_a_nan_pixel_stays_in_its_own_image():
    x = big()
    dirty = x.clone()
    dirty[1, 1, 40, 50] = float("nan")
    zero = x.clone()
    zero[1, 1, 40, 50] = 0.0
    for name, call in CALLS:
        a, b, c = call(x), call(dirty), call(zero)
        assert same(a[0][[0, 2]], b[0][[0, 2]]) and same(a[1]["lut"][[0, 2]], b[1]["lut"][[0, 2]]), name
        assert same(b[0], c[0]) and same(b[1]["q"], c[1]["q"]) and same(b[1]["lut"], c[1]["lut"]), name      # a NaN reads as 0
        assert bool(torch.isfinite(b[0]).all()), name


def test_clahe_and_equalize_replay_from_a_captured_graph():
    x = big()
    eager_c = CL.clahe(x)
    eager_r = CL.clahe(x, space="rgb", grid=(16, 16))
    eager_e = CL.equalize(x)
    static = torch.zeros_like(x)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        out_c = CL.clahe(static)
        out_r = CL.clahe(static, space="rgb", grid=(16, 16))
        out_e = CL.equalize(static)
    static.copy_(x)
    for _ in range(2):                                               # the second replay starts from used workspaces
        for o in (out_c, out_r, out_e):
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert same(out_c, eager_c) and same(out_r, eager_r) and same(out_e, eager_e)


def test_bad_arguments_are_refused_before_any_launch():
    x = big()
    for bad in (dict(grid=(17, 8)), dict(grid=(0, 1)), dict(clip_limit=-0.5), dict(clip_limit=float("nan")), dict(space="hsv")):
        with pytest.raises(ValueError):
            CL.clahe(x, **bad)
    with pytest.raises(ValueError):
        CL.clahe(x[:, :, :7], grid=(8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CL.clahe(torch.zeros(1, 3, 8, 8))
    lib = hdiff_amd.lib()
    assert lib.hdiff_clahe_luts(None, 1, 3, 8, 8, 17, 8, 1, 1.0, None, None) == -1 and b"grid" in lib.hdiff_last_error()
    assert lib.hdiff_clahe_luts(None, 1, 3, 7, 8, 8, 8, 1, 1.0, None, None) == -1 and b"per tile" in lib.hdiff_last_error()
    assert lib.hdiff_clahe_luts(None, 1, 3, 8, 8, 2, 2, 17, 1.0, None, None) == -1 and b"clip" in lib.hdiff_last_error()
    assert lib.hdiff_clahe_luts(None, 1, 2, 8, 8, 2, 2, 16, 1.0, None, None) == -1 and b"planes" in lib.hdiff_last_error()
    assert lib.hdiff_contrast_apply(None, None, None, 1, 8, 8, 0, 9, 1, 1.0, 1.0, None, None) == -1 and b"per tile" in lib.hdiff_last_error()
    assert lib.hdiff_contrast_apply(None, None, None, 1, 8, 8, 0, 2, 2, 2.0, 1.0, None, None) == -1 and b"inv_th" in lib.hdiff_last_error()
    assert lib.hdiff_equalize_luts(None, 1, 3, 8, 8, None, None, None) == -1 and b"null" in lib.hdiff_last_error()


# ---------------------------------------------------------------------------------------------------------------- evaluation loop
def stand_in_sampler(inp, **kwargs):
    return inp / 127.5 - 1


def test_evaluate_scores_the_contrast_baselines_and_changes_nothing_else(tmp_path):
    g = torch.Generator().manual_seed(5)
    batches = [(torch.randint(0, 256, (2, 3, 32, 32), generator=g, dtype=torch.uint8).to(DEV),
                torch.randint(0, 256, (2, 3, 32, 32), generator=g, dtype=torch.uint8).to(DEV),
                [f"img_{2 * i}.png", f"img_{2 * i + 1}.png"]) for i in range(2)]
    plain_dir, with_dir = str(tmp_path / "plain"), str(tmp_path / "with")
    names = ("input", "clahe_lab", "equalize")
    plain = EV.evaluate(stand_in_sampler, batches, ddim_step=2, save_dir=plain_dir)
    res = EV.evaluate(stand_in_sampler, batches, ddim_step=2, save_dir=with_dir, baselines=names)
    # without the names: today's keys and today's six lines, nothing else
    assert set(plain) == {"n", "psnr", "ssim", "uiqm", "uicm", "uism", "uiconm", "per_image"}
    plain_txt = open(os.path.join(plain_dir, "res.txt"), "rb").read()
    assert [ln.split(":")[0] + ":" for ln in plain_txt.decode().split("\n")[1:]] == [k for k, _ in EV.RES_KEYS]
    # with them: the same result beside one new key, the same bytes in front of the new lines, the same images
    assert set(res) == set(plain) | {"baselines"} and list(res["baselines"]) == list(names)
    assert np.array_equal(arr(res["per_image"]), arr(plain["per_image"]))
    assert all(res[k] == plain[k] for k in plain if k != "per_image")
    with_txt = open(os.path.join(with_dir, "res.txt"), "rb").read()
    assert with_txt.startswith(plain_txt)
    tail = with_txt[len(plain_txt):].decode().split("\n")[1:]
    scores = [k for _, k in EV.RES_KEYS]
    assert [ln.split(":")[0] for ln in tail] == [f"{s}_{n}_avg" for n in names for s in scores]
    assert "psnr_clahe_lab_avg:" in with_txt.decode() and "uiconm_equalize_avg:" in with_txt.decode()
    for ln in tail:
        key, value = ln.split(":")
        s, n = next((s, n) for n in names for s in scores if key == f"{s}_{n}_avg")
        assert value == str(res["baselines"][n][s])
    for name in os.listdir(plain_dir):
        if name != "res.txt":
            assert open(os.path.join(plain_dir, name), "rb").read() == open(os.path.join(with_dir, name), "rb").read(), name
    # every baseline's meter is the main meter's configuration fed fn(input / 255) against target / 255
    table = dict(CL.BASELINES, **CL.CONTRAST_BASELINES)
    for n in names:
        meter = Q.QualityMeter()
        for b in batches:
            meter.update(table[n](b[0].float() / 255), b[1].float() / 255)
        want = meter.compute()
        assert np.array_equal(arr(res["baselines"][n]["per_image"]), arr(want["per_image"])), n
        assert all(res["baselines"][n][k] == want[k] for k in want if k != "per_image")
    per = {n: arr(res["baselines"][n]["per_image"]) for n in names}
    assert not np.array_equal(per["clahe_lab"], per["input"]) and not np.array_equal(per["equalize"], per["clahe_lab"])
    with pytest.raises(ValueError):
        EV.evaluate(stand_in_sampler, batches, ddim_step=2, baselines=("input", "clahe"))
