"""GPU checks of the classical baselines (csrc/classical.hip, hdiff_amd/classical.py) and of their hook into the evaluation loop,
against the float64 definition of tests/_classical_def.py.

Gates.  A minimum is exact, the cut is an element of the plane, the airlight a pixel of the image, and t_raw one double multiply and
subtract rounded once: the dark channel (both channel sets), the cut, A and t_raw are held BIT FOR BIT.  M and J are a correctly
rounded double division (and an add) rounded once to fp32, so they are held to the definition's fp32 value or its neighbour; measured
on the MI355X: both meet the value itself, 0 elements differ in every case below.  The white-balance gains are held to 1e-11 relative
(the project's gate for fixed-order double sums against numpy's; measured 2.7e-16 at most, 0 at p = 1) and are exact at p = inf; its output is
the definition's fp32 value or its neighbour (measured: 0 elements differ).

The window minimum works on kTile x kTile = 32 x 32 output tiles with a halo of r = patch // 2 on every side: 75 x 101 is larger than
tile plus halo (46 at patch 15) on both sides and a multiple of neither.  Every test prints its figures before asserting."""
import functools
import gc
import math
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
from hdiff_amd import transfer as T  # noqa: E402
from hdiff_amd.diffusion import Evaluate as EV  # noqa: E402

import _classical_def as CD  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K_TILE = 32
SHAPES = ((1, 1), (3, 5), (8, 13), (75, 101))
PATCHES = (1, 3, 15)
BETA_1, BETA_T = 1e-4, 0.02


@pytest.fixture(scope="module", autouse=True)
def private_memory_pool():
    """Every allocation of this module comes from a pool of its own, released at the end: the caching allocator's default pool, whose
    leftover blocks later tests' memory accounting depends on (tests/test_gpu_fused_dropout.py), is left as this module found it."""
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool):
        yield
    small_sampler.cache_clear()
    images.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    del pool


def bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


@functools.lru_cache(maxsize=None)
def images(shape, n=3, levels=None, seed=0):
    """fp32 [n, 3, H, W] in [-0.1, 1.1] (the clip has work to do): a smooth colour field, so that dark channel and transmission vary
    over the image at every patch, under noise; with ``levels`` quantised to that many steps: long runs of ties."""
    rng = np.random.default_rng([seed, shape[0], shape[1], n, levels or 0])
    yy, xx = np.meshgrid(np.arange(shape[0], dtype=np.float64), np.arange(shape[1], dtype=np.float64), indexing="ij")
    field = np.stack([[0.5 + 0.45 * np.sin(yy / 9 + c + i) * np.cos(xx / 7 - c) for c in range(3)] for i in range(n)])
    x = (field + 0.3 * (rng.random((n, 3) + shape) - 0.5)).astype(np.float32)
    if levels:
        x = (np.round(x * levels) / np.float32(levels)).astype(np.float32)
    return x + np.float32(0.0)                     # no -0: numpy's maximum(-0, +0) is free to return either


@pytest.mark.parametrize("patch", PATCHES)
@pytest.mark.parametrize("shape", SHAPES)
def test_dark_channel_is_the_definition_bit_for_bit(shape, patch):
    x = images(shape)
    d = torch.from_numpy(x).to(DEV)
    for channels in ("rgb", "gb"):
        got = CL.dark_channel(d, patch=patch, channels=channels)
        want = np.stack([CD.dark_channel_def(CD.clipped(im), patch, channels) for im in x])
        assert tuple(got.shape) == (3,) + shape and np.array_equal(bits(got), bits(want)), channels
        one = CL.dark_channel(d[1:2], patch=patch, channels=channels)                  # a batch of 1 gives the same bits
        assert np.array_equal(bits(one[0]), bits(want[1]))


def check_dehaze(x, *, prior, patch, top, omega=0.95, t0=0.1, airlight=None):
    d = torch.from_numpy(x).to(DEV)
    a = None if airlight is None else torch.from_numpy(airlight).to(DEV)
    J, parts = CL.dehaze(d, prior=prior, patch=patch, omega=omega, t0=t0, top=top, refine=None, airlight=a, return_parts=True)
    differing = {"M": 0, "J": 0}
    for i, im in enumerate(x):
        want = CD.dehaze_def(im, prior=prior, patch=patch, omega=omega, t0=t0, top=top, refine=None,
                             airlight=None if airlight is None else airlight[i])
        assert np.array_equal(bits(parts["dark"][i]), bits(want["dark"])), ("dark", i)
        assert np.array_equal(bits(parts["A"][i]), bits(want["A"])), ("A", i, parts["A"][i], want["A"])
        if airlight is None:
            assert bits(parts["cut"][i]) == bits(want["cut"]), ("cut", i)
        else:
            assert parts["cut"] is None
        ok, n = CD.neighbours_ok(parts["M"][i].cpu().numpy(), want["M"])
        differing["M"] += n
        assert ok, ("M", i)
        assert np.array_equal(bits(parts["t_raw"][i]), bits(want["t_raw"])), ("t_raw", i)
        assert parts["t"] is parts["t_raw"]
        ok, n = CD.neighbours_ok(J[i].cpu().numpy(), want["J"])
        differing["J"] += n
        assert ok, ("J", i)
    return differing


@pytest.mark.parametrize("prior", ("dcp", "udcp", "inverted_dcp"))
@pytest.mark.parametrize("shape", SHAPES)
def test_dehaze_parts_against_the_definition(shape, prior):
    """n_top = 1 (top = 1e-4 on these sizes) on continuous images, and top = 0.3 on quantised ones, where the cut falls inside a run
    of equal dark-channel values and every tie is a candidate."""
    H, W = shape
    total = {"M": 0, "J": 0}
    for patch in PATCHES:
        for n in (1, 3):
            assert CD.n_top_of(1e-4, H, W) == 1
            for k, v in check_dehaze(images(shape, n), prior=prior, patch=patch, top=1e-4).items():
                total[k] += v
        tied = images(shape, 3, levels=4)
        if H * W >= 15:
            flat = np.sort(CD.dehaze_def(tied[0], prior=prior, patch=patch, top=0.3)["dark"].reshape(-1))
            cut_at = H * W - CD.n_top_of(0.3, H, W)
            assert flat[cut_at - 1] == flat[cut_at] or flat[cut_at + 1] == flat[cut_at], "the fixture must put the cut inside a run of ties"
        for k, v in check_dehaze(tied, prior=prior, patch=patch, top=0.3, omega=0.8, t0=0.25).items():
            total[k] += v
    print(f"dehaze {prior} {shape}: elements off the definition's fp32 value: M {total['M']}, J {total['J']}")


def test_airlight_override():
    x = images((8, 13))
    A = np.array([[0.9, 0.8, 0.7], [0.5, 1.0, 0.25], [1.0 / 3.0, 0.0, -0.5]], dtype=np.float32)      # 0 and -0.5: raised to 1 / 255
    for prior in ("dcp", "udcp", "inverted_dcp"):
        print(prior, check_dehaze(x, prior=prior, patch=3, top=1e-3, airlight=A))
    d = torch.from_numpy(x).to(DEV)
    floor = np.float32(1.0 / 255.0)
    got = CL.dehaze(d, patch=3, refine=None, airlight=torch.from_numpy(A).to(DEV), return_parts=True)[1]["A"]
    assert np.array_equal(bits(got), bits(np.maximum(A, floor)))
    nan_a = torch.full((3, 3), float("nan"), device=DEV)
    J, parts = CL.dehaze(d, patch=3, refine=None, airlight=nan_a, return_parts=True)
    assert np.array_equal(bits(parts["A"]), bits(np.full((3, 3), floor))) and bool(torch.isfinite(J).all())
    with pytest.raises(ValueError):
        CL.dehaze(d, airlight=torch.ones(2, 3, device=DEV))


def test_largest_patch_over_several_tiles():
    """patch 63: the halo of 31 the kernel's LDS arrays are sized for (a staged block of 94 x 94), on an image of 3 x 4 tiles."""
    x = images((75, 101))
    d = torch.from_numpy(x).to(DEV)
    for channels in ("rgb", "gb"):
        want = np.stack([CD.dark_channel_def(CD.clipped(im), 63, channels) for im in x])
        assert np.array_equal(bits(CL.dark_channel(d, patch=63, channels=channels)), bits(want)), channels
    print("patch 63:", check_dehaze(x, prior="dcp", patch=63, top=0.01))


def test_refinement_reads_a_nan_pixel_as_zero():
    """The guide of the refinement is X as every kernel reads it: a NaN pixel gives what a 0 in its place gives, bit for bit."""
    x = np.array(images((8, 13)))
    x[1, 2, 3, 4] = np.nan
    zero = np.array(x)
    zero[1, 2, 3, 4] = 0.0
    for prior in ("dcp", "inverted_dcp"):
        a = CL.dehaze(torch.from_numpy(x).to(DEV), prior=prior, patch=3, refine=(2, 1e-3), return_parts=True)
        b = CL.dehaze(torch.from_numpy(zero).to(DEV), prior=prior, patch=3, refine=(2, 1e-3), return_parts=True)
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]["t"]), bits(b[1]["t"])), prior
        assert bool(torch.isfinite(a[0]).all())


@pytest.mark.parametrize("prior", ("dcp", "inverted_dcp"))
def test_refinement_is_the_guided_filter_itself(prior):
    x = images((75, 101))
    d = torch.from_numpy(x).to(DEV)
    J, parts = CL.dehaze(d, prior=prior, patch=15, refine=(4, 1e-3), return_parts=True)
    raw = CL.dehaze(d, prior=prior, patch=15, refine=None, return_parts=True)[1]["t_raw"]
    assert np.array_equal(bits(parts["t_raw"]), bits(raw)) and float(raw.min()) < 0.9 < float(raw.max())
    guide = d.clamp(0, 1)
    if prior == "inverted_dcp":
        guide = 1.0 - guide
    coef = T.guided_fit(guide, raw[:, None].repeat(1, 3, 1, 1), radius=4, eps=1e-3)
    want_t = T.guided_apply(coef, guide, clamp=False)[:, 0]
    assert np.array_equal(bits(parts["t"]), bits(want_t))
    assert not np.array_equal(bits(parts["t"]), bits(raw))
    for i, im in enumerate(x):                     # and J is the definition's recovery under that t
        xi = CD.clipped(im)
        xi = np.float32(1.0) - xi if prior == "inverted_dcp" else xi
        want = CD.recover_def(xi, parts["A"][i].cpu().numpy(), want_t[i].cpu().numpy(), 0.1)
        want = np.float32(1.0) - want if prior == "inverted_dcp" else want
        ok, n = CD.neighbours_ok(J[i].cpu().numpy(), want)
        print(f"refined {prior} image {i}: {n} elements of J off the definition's fp32 value")
        assert ok


@pytest.mark.parametrize("p", (1.0, 6.0, math.inf))
@pytest.mark.parametrize("shape", SHAPES)
def test_white_balance_against_the_definition(shape, p):
    worst, off = 0.0, 0
    for n in (1, 3):
        x = images(shape, n, seed=2)
        out, gains = CL.white_balance(torch.from_numpy(x).to(DEV), p=p, return_gains=True)
        assert gains.dtype == torch.float64 and tuple(gains.shape) == (n, 3)
        for i, im in enumerate(x):
            want, g = CD.white_balance_def(im, p)
            got_g = gains[i].cpu().numpy()
            if math.isinf(p):
                assert np.array_equal(bits(got_g), bits(g))
            worst = max(worst, float(np.max(np.abs(got_g - g) / np.abs(g))))
            ok, k = CD.neighbours_ok(out[i].cpu().numpy(), want)
            off += k
            assert ok
    print(f"white balance p={p} {shape}: gains within {worst:.2e} relative; {off} output elements off the definition's fp32 value")
    assert worst <= 1e-11


def test_white_balance_of_a_large_plane_uses_every_partial():
    """More pixels than one workgroup's share (2048): the partial sums of several workgroups are added in index order."""
    x = images((75, 101), 1, seed=3)
    out, gains = CL.white_balance(torch.from_numpy(x).to(DEV), p=1.0, return_gains=True)
    m = CD.clipped(x[0]).astype(np.float64).reshape(3, -1).mean(axis=1)
    assert np.allclose(gains[0].cpu().numpy(), m.mean() / m, rtol=1e-11, atol=0)
    black = torch.zeros(1, 3, 8, 13, device=DEV)
    assert np.array_equal(bits(CL.white_balance(black)), bits(black))


def test_a_nan_pixel_stays_in_its_own_image():
    x = np.array(images((75, 101)))
    clean = torch.from_numpy(x).to(DEV)
    x[1, 1, 40, 50] = np.nan
    dirty = torch.from_numpy(x).to(DEV)
    for prior in ("dcp", "udcp", "inverted_dcp"):
        a = CL.dehaze(clean, prior=prior, patch=15, refine=(4, 1e-3))
        b = CL.dehaze(dirty, prior=prior, patch=15, refine=(4, 1e-3))
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[2]), bits(b[2])), prior
    a, ga = CL.white_balance(clean, p=6.0, return_gains=True)
    b, gb = CL.white_balance(dirty, p=6.0, return_gains=True)
    assert np.array_equal(bits(a[[0, 2]]), bits(b[[0, 2]])) and np.array_equal(bits(ga[[0, 2]]), bits(gb[[0, 2]]))


def test_results_repeat_and_do_not_depend_on_the_batch():
    x = torch.from_numpy(images((75, 101))).to(DEV)
    for prior in ("dcp", "udcp", "inverted_dcp"):
        first = CL.dehaze(x, prior=prior, patch=15, top=0.01, refine=(4, 1e-3), return_parts=True)
        again = CL.dehaze(x, prior=prior, patch=15, top=0.01, refine=(4, 1e-3), return_parts=True)
        alone = CL.dehaze(x[2:3], prior=prior, patch=15, top=0.01, refine=(4, 1e-3), return_parts=True)
        assert np.array_equal(bits(first[0]), bits(again[0])) and np.array_equal(bits(first[0][2]), bits(alone[0][0]))
        for k in ("dark", "A", "t_raw", "t", "M", "cut"):
            assert np.array_equal(bits(first[1][k]), bits(again[1][k])) and np.array_equal(bits(first[1][k][2]), bits(alone[1][k][0])), k
    for p in (1.0, 6.0, math.inf):
        first, again, alone = (CL.white_balance(v, p=p, return_gains=True) for v in (x, x, x[2:3]))
        for j in (0, 1):
            assert np.array_equal(bits(first[j]), bits(again[j])) and np.array_equal(bits(first[j][2]), bits(alone[j][0]))


def test_dehaze_and_white_balance_replay_from_a_captured_graph():
    x = torch.from_numpy(images((75, 101))).to(DEV)
    eager_j = CL.dehaze(x, prior="dcp", patch=15, refine=(4, 1e-3))
    eager_w = CL.white_balance(x, p=6.0)
    static = torch.zeros_like(x)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        out_j = CL.dehaze(static, prior="dcp", patch=15, refine=(4, 1e-3))
        out_w = CL.white_balance(static, p=6.0)
    static.copy_(x)
    for _ in range(2):                                               # the second replay starts from used workspaces
        out_j.zero_()
        out_w.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(out_j), bits(eager_j)) and np.array_equal(bits(out_w), bits(eager_w))


def test_cpu_tensors_and_bad_sizes_are_refused():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CL.dehaze(torch.zeros(1, 3, 8, 8))
    lib = hdiff_amd.lib()
    assert lib.hdiff_classical_window_min(None, 1, 8, 8, 4, 0, 0.0, None, None) == -1 and b"patch" in lib.hdiff_last_error()
    assert lib.hdiff_classical_airlight(None, None, 1, 8, 8, 0, 65, None, None, None, None) == -1 and b"n_top" in lib.hdiff_last_error()
    assert lib.hdiff_white_balance(None, 1, 8, 8, 0.5, None, None, None, None) == -1 and b"p =" in lib.hdiff_last_error()


# ---------------------------------------------------------------------------------------------------------------- evaluation loop
@functools.lru_cache(maxsize=None)
def small_sampler():
    from _tree_b_small import load_small_dyn_unet
    from hdiff_amd.diffusion.Diffusion import GaussianDiffusionSampler
    _, cfg, m, _ = load_small_dyn_unet()
    return GaussianDiffusionSampler(m.to(DEV), BETA_1, BETA_T, cfg["T"]).to(DEV)


def test_evaluate_scores_the_baselines_and_changes_nothing_else(tmp_path):
    sampler = small_sampler()
    g = torch.Generator().manual_seed(5)
    batches = [(torch.randint(0, 256, (2, 3, 32, 32), generator=g, dtype=torch.uint8),
                torch.randint(0, 256, (2, 3, 32, 32), generator=g, dtype=torch.uint8), [f"img_{2 * i}.png", f"img_{2 * i + 1}.png"])
               for i in range(2)]
    plain_dir, with_dir = str(tmp_path / "plain"), str(tmp_path / "with")
    names = ("input", "gray_world", "dcp")
    torch.manual_seed(21)
    plain = EV.evaluate(sampler, batches, ddim_step=2, save_dir=plain_dir)
    torch.manual_seed(21)
    res = EV.evaluate(sampler, batches, ddim_step=2, save_dir=with_dir, baselines=names)
    # without the argument: today's keys and today's six lines, nothing else
    assert set(plain) == {"n", "psnr", "ssim", "uiqm", "uicm", "uism", "uiconm", "per_image"}
    plain_txt = open(os.path.join(plain_dir, "res.txt"), "rb").read()
    assert [ln.split(":")[0] + ":" for ln in plain_txt.decode().split("\n")[1:]] == [k for k, _ in EV.RES_KEYS]
    # with it: the same result beside one new key, the same bytes in front of the new lines, the same images
    assert set(res) == set(plain) | {"baselines"} and list(res["baselines"]) == list(names)
    assert np.array_equal(bits(res["per_image"]), bits(plain["per_image"]))
    assert all(res[k] == plain[k] for k in plain if k != "per_image")
    with_txt = open(os.path.join(with_dir, "res.txt"), "rb").read()
    assert with_txt.startswith(plain_txt)
    tail = with_txt[len(plain_txt):].decode().split("\n")[1:]
    scores = [k for _, k in EV.RES_KEYS]
    assert [ln.split(":")[0] for ln in tail] == [f"{s}_{n}_avg" for n in names for s in scores]
    for ln in tail:
        key, value = ln.split(":")
        s, n = next((s, n) for n in names for s in scores if key == f"{s}_{n}_avg")
        assert value == str(res["baselines"][n][s])
    for name in os.listdir(plain_dir):
        if name != "res.txt":
            assert open(os.path.join(plain_dir, name), "rb").read() == open(os.path.join(with_dir, name), "rb").read(), name
    # every baseline's meter is the main meter's configuration fed fn(input / 255) against target / 255
    for n in names:
        meter = Q.QualityMeter()
        for b in batches:
            meter.update(CL.BASELINES[n](b[0].to(DEV).float() / 255), b[1].to(DEV).float() / 255)
        want = meter.compute()
        assert np.array_equal(bits(res["baselines"][n]["per_image"]), bits(want["per_image"])), n
        assert all(res["baselines"][n][k] == want[k] for k in want if k != "per_image")
    assert not np.array_equal(bits(res["baselines"]["dcp"]["per_image"]), bits(res["baselines"]["input"]["per_image"]))
    # a caller's own baseline, and the meter's configuration is copied
    torch.manual_seed(21)
    own = EV.evaluate(sampler, batches[:1], ddim_step=2, color=True, baselines=(("half", lambda x: x * 0.5), "udcp"))
    assert list(own["baselines"]) == ["half", "udcp"] and "ciede2000" in own["baselines"]["half"]
    with pytest.raises(ValueError):
        EV.evaluate(sampler, batches, ddim_step=2, baselines=("input", "clahe"))
