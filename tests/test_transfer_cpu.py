"""Host-side tests of the guided full-resolution transfer (no GPU): the float64 definitions the kernels are held to
(tests/_transfer_def.py) have the properties of a guided filter and of Pillow's resize, the tolerance the uint8 GPU test grants at
rounding ties is rare on its fixtures, the C ABI declares / exports / validates the six entries, and the Python layer checks its
arguments before it touches a device."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hdiff_amd  # noqa: E402
from hdiff_amd import _capi  # noqa: E402
import _transfer_def as TD  # noqa: E402

NEW_SYMBOLS = {"hdiff_resample_workspace", "hdiff_resample_u8", "hdiff_guided_workspace", "hdiff_guided_fit", "hdiff_guided_apply_f32",
               "hdiff_guided_apply_u8"}


def pair(h, w, seed=0):
    rng = np.random.default_rng(seed)
    I = rng.random((3, h, w)).astype(np.float32)
    p = np.clip(np.einsum("cj,jyx->cyx", TD.COLOUR_MATRIX, I.astype(np.float64)) + 0.05 * rng.standard_normal((3, h, w)), 0, 1)
    return I, p.astype(np.float32)


def clipped(y, x, h, w, r):
    return slice(max(y - r, 0), min(y + r, h - 1) + 1), slice(max(x - r, 0), min(x + r, w - 1) + 1)


def test_fit_is_the_ridge_regression_minimiser():
    """(a, b) before the second window mean minimises sum (a.I + b - p)^2 + n eps |a|^2 over the clipped window: solved independently
    with lstsq on the augmented system."""
    h, w, r, eps = 9, 11, 2, 1e-3
    I, p = pair(h, w, 1)
    ab = TD.fit_ab64(I, p, r, eps)
    rng = np.random.default_rng(2)
    for y, x in [(0, 0)] + [(int(rng.integers(h)), int(rng.integers(w))) for _ in range(3)]:
        ys, xs = clipped(y, x, h, w, r)
        Iw = I[:, ys, xs].reshape(3, -1).astype(np.float64).T
        n = Iw.shape[0]
        rows = np.concatenate([np.concatenate([Iw, np.ones((n, 1))], axis=1),
                               np.concatenate([np.sqrt(n * eps) * np.eye(3), np.zeros((3, 1))], axis=1)])
        for c in range(3):
            rhs = np.concatenate([p[c, ys, xs].reshape(-1).astype(np.float64), np.zeros(3)])
            want = np.linalg.lstsq(rows, rhs, rcond=None)[0]
            got = np.array([ab[3 * c, y, x], ab[3 * c + 1, y, x], ab[3 * c + 2, y, x], ab[9 + c, y, x]])
            assert np.abs(got - want).max() <= 1e-9, (y, x, c, got, want)


def test_constant_target_gives_zero_matrix_and_the_constant():
    I, _ = pair(12, 15, 3)
    const = np.array([0.25, 0.6180339887, 0.9], dtype=np.float32)
    p = np.broadcast_to(const[:, None, None], I.shape).copy()
    coef = TD.fit64(I, p, 3, 1e-3)
    assert np.abs(coef[:9]).max() <= 1e-9
    for c in range(3):
        assert np.abs(coef[9 + c] - float(const[c])).max() <= float(np.spacing(const[c]))


def test_a_radius_that_covers_the_image_gives_one_map():
    I, p = pair(7, 9, 4)
    coef = TD.fit(I, p, 9, 1e-3)
    assert np.isfinite(coef).all()
    assert (coef == coef[:, :1, :1]).all()


def test_equal_size_is_the_classical_guided_filter():
    """Brute force: per pixel np.mean over the clipped window and np.linalg.solve; q = mean(a) . I + mean(b)."""
    h, w, r, eps = 8, 10, 2, 1e-2
    I, p = pair(h, w, 5)
    I64, p64 = I.astype(np.float64), p.astype(np.float64)
    a = np.zeros((h, w, 3, 3))
    b = np.zeros((h, w, 3))
    for y in range(h):
        for x in range(w):
            ys, xs = clipped(y, x, h, w, r)
            Iw, pw = I64[:, ys, xs].reshape(3, -1), p64[:, ys, xs].reshape(3, -1)
            mI, mp = Iw.mean(axis=1), pw.mean(axis=1)
            sigma = Iw @ Iw.T / Iw.shape[1] - np.outer(mI, mI) + eps * np.eye(3)
            cov = Iw @ pw.T / Iw.shape[1] - np.outer(mI, mp)                     # [j][c]
            a[y, x] = np.linalg.solve(sigma, cov).T                                # [c][j]
            b[y, x] = mp - a[y, x] @ mI
    want = np.zeros((3, h, w))
    for y in range(h):
        for x in range(w):
            ys, xs = clipped(y, x, h, w, r)
            ma, mb = a[ys, xs].reshape(-1, 3, 3).mean(axis=0), b[ys, xs].reshape(-1, 3).mean(axis=0)
            want[:, y, x] = ma @ I64[:, y, x] + mb
    got, _ = TD.apply64(TD.fit64(I, p, r, eps), I64)
    assert np.abs(got - want).max() <= 1e-9


@pytest.mark.parametrize("h,w,r,eps", [(16, 19, 3, 1e-3), (33, 40, 8, 1e-3), (33, 40, 4, 1e-4), (24, 24, 2, 1e-2)])
def test_fit_does_not_depend_on_the_summation_order(h, w, r, eps):
    """The image flipped along both axes is summed in the opposite order: the fp32 coefficients are the same ones.  This is why the GPU
    test grants one rounding and no more."""
    I, p = pair(h, w, 6)
    flipped = TD.fit(I[:, ::-1, ::-1].copy(), p[:, ::-1, ::-1].copy(), r, eps)[:, ::-1, ::-1]
    assert np.array_equal(TD.fit(I, p, r, eps), flipped)


@pytest.mark.parametrize("big,small", [((7, 5), (3, 2)), ((20, 31), (32, 32)), ((97, 131), (33, 40)), ((403, 302), (32, 32)), ((64, 64), (64, 64))])
def test_resample_against_pillow(big, small):
    from PIL import Image
    img = np.random.default_rng(big[0]).integers(0, 256, size=big + (3,), dtype=np.uint8)
    got = TD.resample64(img, small)
    pillow = np.asarray(Image.fromarray(img).resize((small[1], small[0]), Image.BILINEAR)).astype(np.float64).transpose(2, 0, 1)
    gap = float(np.abs(got - pillow).max())
    print(f"{big} -> {small}: largest distance from Pillow {gap:.3f} levels")
    if big == small:
        assert np.array_equal(got, pillow)
    else:
        assert gap <= 1.0


@pytest.mark.parametrize("small,large", TD.APPLY_SIZES + TD.EXTRA_APPLY_SIZES)
def test_rounding_ties_are_rare_on_the_uint8_fixtures(small, large):
    """The uint8 GPU test excuses a byte off by one where the definition lies within 255 * 16 * 2^-24 * S of a half-integer.  For the
    reference alone: at most 0.5 % of the bytes of a fixture are such, and the fixtures keep max |A| <= 1.1 and S <= 1.2."""
    img, low, target = TD.u8_fixture(small, large)
    coef = TD.fit(low, target, TD.FIXTURE_RADIUS, TD.FIXTURE_EPS)
    v, S = TD.apply_u8_64(coef, img)
    share = float(TD.tie_excused(v, S).mean())
    print(f"{small} -> {large}: {100 * share:.3f} % of {v.size} bytes near a tie; max |A| {np.abs(coef[:9]).max():.3f}, max S {S.max():.3f}")
    assert np.abs(coef[:9]).max() <= 1.1 and S.max() <= 1.2
    assert share <= 0.005


def test_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "hdiff.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(hdiff_[a-z0-9_]+)\s*\(", text))
    assert NEW_SYMBOLS <= declared
    assert NEW_SYMBOLS <= set(_capi.EXPORTED_SYMBOLS)
    lib = hdiff_amd.lib()
    assert lib.hdiff_abi_version() == 6
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert NEW_SYMBOLS <= set(re.findall(r" T (hdiff_[a-z0-9_]+)", out))


def test_argument_validation_needs_no_gpu():
    lib = hdiff_amd.lib()
    need = C.c_int64(0)
    assert lib.hdiff_resample_workspace(3024, 4032, 256, 256, C.byref(need)) == 0
    assert need.value >= 3024 * 256 * 3 * 8                    # the [H][w][3] intermediate in double
    assert lib.hdiff_guided_workspace(1, 256, 256, C.byref(need)) == 0
    assert need.value >= (21 + 12) * 256 * 256 * 8
    three = C.c_int64(0)
    assert lib.hdiff_guided_workspace(3, 256, 256, C.byref(three)) == 0 and three.value > need.value
    one = 64         # any non-null address: validation returns before anything is read or launched

    def refused(rc, word):
        assert rc == -1
        assert word in lib.hdiff_last_error().decode(), lib.hdiff_last_error()

    for H, W in ((0, 8), (8, 0), (16385, 8), (8, 16385), (-1, 8)):
        refused(lib.hdiff_resample_workspace(H, W, 4, 4, C.byref(need)), "between 1 and 16384")
        refused(lib.hdiff_resample_u8(one, H, W, one, 4, 4, one, None), "between 1 and 16384")
        refused(lib.hdiff_guided_apply_u8(one, 4, 4, one, one, H, W, None), "between 1 and 16384")
        refused(lib.hdiff_guided_apply_f32(one, 4, 4, one, one, 1, H, W, 1, None), "between 1 and 16384")
    for h, w in ((0, 4), (4, 0), (4097, 4), (4, 4097)):
        refused(lib.hdiff_resample_workspace(8, 8, h, w, C.byref(need)), "between 1 and 4096")
        refused(lib.hdiff_resample_u8(one, 8, 8, one, h, w, one, None), "between 1 and 4096")
        refused(lib.hdiff_guided_workspace(1, h, w, C.byref(need)), "between 1 and 4096")
        refused(lib.hdiff_guided_fit(one, one, 1, h, w, 2, 1e-3, one, one, None), "between 1 and 4096")
        refused(lib.hdiff_guided_apply_u8(one, h, w, one, one, 8, 8, None), "between 1 and 4096")
        refused(lib.hdiff_guided_apply_f32(one, h, w, one, one, 1, 8, 8, 1, None), "between 1 and 4096")
    for N in (0, 65536, -2):
        refused(lib.hdiff_guided_workspace(N, 4, 4, C.byref(need)), f"N = {N}")
        refused(lib.hdiff_guided_fit(one, one, N, 4, 4, 2, 1e-3, one, one, None), f"N = {N}")
        refused(lib.hdiff_guided_apply_f32(one, 4, 4, one, one, N, 8, 8, 1, None), f"N = {N}")
    for r in (0, 129, -1):
        refused(lib.hdiff_guided_fit(one, one, 1, 4, 4, r, 1e-3, one, one, None), f"r = {r}")
    for eps in (0.0, -1e-3, float("inf"), float("nan")):
        refused(lib.hdiff_guided_fit(one, one, 1, 4, 4, 2, eps, one, one, None), "eps")
    refused(lib.hdiff_resample_workspace(8, 8, 4, 4, None), "null pointer")
    refused(lib.hdiff_guided_workspace(1, 4, 4, None), "null pointer")
    for k in range(3):
        img, out, scratch = (None if i == k else one for i in range(3))
        refused(lib.hdiff_resample_u8(img, 8, 8, out, 4, 4, scratch, None), "null pointer")
        coef, full, res = (None if i == k else one for i in range(3))
        refused(lib.hdiff_guided_apply_u8(coef, 4, 4, full, res, 8, 8, None), "null pointer")
        refused(lib.hdiff_guided_apply_f32(coef, 4, 4, full, res, 1, 8, 8, 0, None), "null pointer")
    for k in range(4):
        I, p, coef, scratch = (None if i == k else one for i in range(4))
        refused(lib.hdiff_guided_fit(I, p, 1, 4, 4, 2, 1e-3, coef, scratch, None), "null pointer")


def test_python_layer_checks_arguments_before_any_device():
    from hdiff_amd import transfer as T
    img = torch.zeros(8, 9, 3, dtype=torch.uint8)
    small = torch.rand(1, 3, 4, 4)
    for bad in (0, 4097, (4, 0), (4, 4, 4)):
        with pytest.raises((ValueError, TypeError)):
            T.resample(img, bad)
    with pytest.raises(TypeError):
        T.resample(img, 4.0)
    with pytest.raises(ValueError, match="uint8"):
        T.resample(img.float(), 4)
    with pytest.raises(ValueError, match="uint8"):
        T.resample(torch.zeros(3, 8, 9, dtype=torch.uint8), 4)
    with pytest.raises(RuntimeError, match="MI355X"):
        T.resample(img, 4)
    for kw in (dict(radius=0), dict(radius=129), dict(eps=0.0), dict(eps=float("nan")), dict(eps=float("inf")), dict(eps=-1.0)):
        with pytest.raises(ValueError):
            T.guided_fit(small, small, **kw)
    with pytest.raises(TypeError):
        T.guided_fit(small, small, radius=2.5)
    with pytest.raises(ValueError, match="same shape"):
        T.guided_fit(small, torch.rand(1, 3, 4, 5))
    with pytest.raises(ValueError):
        T.guided_fit(small[0], small[0])
    with pytest.raises(RuntimeError, match="MI355X"):
        T.guided_fit(small, small)
    coef = torch.zeros(12, 4, 4)
    with pytest.raises(ValueError):
        T.guided_apply(coef[None], img)                      # a uint8 image takes [12, h, w]
    with pytest.raises(ValueError):
        T.guided_apply(coef, torch.rand(1, 3, 8, 9))         # a float batch takes [N, 12, h, w]
    with pytest.raises(ValueError):
        T.guided_apply(coef, img, clamp=False)
    with pytest.raises(RuntimeError, match="MI355X"):
        T.guided_apply(coef, img)
    with pytest.raises(RuntimeError, match="MI355X"):
        T.guided_apply(coef[None], torch.rand(1, 3, 8, 9))
    with pytest.raises(ValueError):
        T.GuidedEnhancer(lambda *a, **k: None, radius=0)
    with pytest.raises(ValueError):
        T.GuidedEnhancer(lambda *a, **k: None, size=0)
    with pytest.raises(TypeError):
        T.GuidedEnhancer(None)
    enhancer = T.GuidedEnhancer(lambda *a, **k: None, size=32, ddim_step=5)
    assert enhancer.size == (32, 32) and enhancer.sampler_kwargs == {"ddim_step": 5} and (enhancer.radius, enhancer.eps) == (8, 1e-3)
    with pytest.raises(RuntimeError, match="MI355X"):
        enhancer(img)
    for text in (T.__doc__, T.GuidedEnhancer.__doc__):
        assert "image-quality figure" in text and "texture" in text


def test_evaluate_checks_transfer_before_sampling(tmp_path):
    from hdiff_amd.diffusion import Evaluate as EV
    calls = []

    def sampler(x, **kw):
        calls.append(kw)
        raise AssertionError("the sampler must not be reached")

    batch = (torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4), ["a.png"])
    with pytest.raises(ValueError, match="save_dir"):
        EV.evaluate(sampler, [batch], ddim_step=2, transfer=(2, 1e-3))
    for bad in ((0, 1e-3), (2, 0.0), (2,), {"radius": 2, "epsilon": 1e-3}, "yes"):
        with pytest.raises((ValueError, TypeError)):
            EV.evaluate(sampler, [batch], ddim_step=2, transfer=bad, save_dir=str(tmp_path / "x"))
    with pytest.raises(ValueError, match="originals"):
        EV.evaluate(sampler, [batch], ddim_step=2, transfer={"radius": 2, "eps": 1e-3}, save_dir=str(tmp_path / "y"))
    with pytest.raises(ValueError, match="originals"):
        EV.evaluate(sampler, [batch + ([],)], ddim_step=2, transfer=(2, 1e-3), save_dir=str(tmp_path / "y"))
    with pytest.raises(ValueError, match="uint8"):
        EV.evaluate(sampler, [batch + ([torch.zeros(5, 6, 3)],)], ddim_step=2, transfer=(2, 1e-3), save_dir=str(tmp_path / "y"))
    assert calls == []
    assert not os.path.exists(str(tmp_path / "x"))


def test_batched_adds_the_originals_on_request(tmp_path):
    from PIL import Image
    from hdiff_amd.diffusion import Evaluate as EV

    rng = np.random.default_rng(0)
    paths, sizes = [], ((9, 14), (21, 8), (5, 5))
    for i, (H, W) in enumerate(sizes):
        path = str(tmp_path / f"{i}.png")
        Image.fromarray(rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)).save(path)
        paths.append(path)

    class Data:
        paths_a = paths

        def __len__(self):
            return len(paths)

        def __getitem__(self, i):
            return torch.full((3, 4, 4), float(i)), torch.zeros(3, 4, 4)

    plain = list(EV._batched(Data(), 2))
    assert [len(b) for b in plain] == [3, 3]
    full = list(EV._batched(Data(), 2, full=True))
    assert [len(b) for b in full] == [4, 4] and [len(b[3]) for b in full] == [2, 1]
    got = [o for b in full for o in b[3]]
    for o, path, (H, W) in zip(got, paths, sizes):
        assert o.dtype == torch.uint8 and tuple(o.shape) == (H, W, 3)
        assert np.array_equal(o.numpy(), np.asarray(Image.open(path).convert("RGB")))
    for a, b in zip(plain, full):
        assert torch.equal(a[0], b[0]) and a[2] == b[2]
