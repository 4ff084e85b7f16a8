"""Host-side tests of the set-level scores (no GPU): the C ABI declares / exports / validates the three entries of
``csrc/distribution.hip``; ``res.txt`` keeps its keys and gains two; the float64 definitions (tests/_distribution_def.py) agree with
numpy's own covariance and with a direct matrix expression of KID; ``quality.frechet_from_moments`` against closed forms and against
the ``scipy.linalg.sqrtm`` route the reference's FID takes."""
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
from hdiff_amd import quality as Q  # noqa: E402
import _distribution_def as DD  # noqa: E402

NEW_SYMBOLS = {"hdiff_feat_moments", "hdiff_kid_workspace", "hdiff_kid_sums"}
DIMS = (8, 48, 384)


def rel(a, b):
    return 0.0 if a == b else abs(a - b) / abs(b)


def test_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "hdiff.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(hdiff_[a-z0-9_]+)\s*\(", text))
    assert NEW_SYMBOLS <= declared
    assert NEW_SYMBOLS <= set(_capi.EXPORTED_SYMBOLS)
    lib = hdiff_amd.lib()
    assert lib.hdiff_abi_version() == 6                                    # additions only
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert NEW_SYMBOLS <= set(re.findall(r" T (hdiff_[a-z0-9_]+)", out))


def test_argument_validation_needs_no_gpu():
    lib = hdiff_amd.lib()
    need, small = C.c_int64(0), C.c_int64(0)
    assert lib.hdiff_kid_workspace(1024, 1024, C.byref(need)) == 0
    tiles = 32 * 33 // 2                                                   # pairs of 32-row blocks, I <= J
    assert need.value >= 3 * tiles * 8
    assert lib.hdiff_kid_workspace(1, 1, C.byref(small)) == 0 and 0 < small.value < need.value
    assert lib.hdiff_kid_workspace(32768, 32768, C.byref(need)) == 0
    one = 8          # any non-null address: validation returns before anything is read or launched

    def refused(rc, word):
        assert rc == -1
        assert word in lib.hdiff_last_error().decode(), lib.hdiff_last_error()

    refused(lib.hdiff_kid_workspace(0, 4, C.byref(need)), "n = 0")
    refused(lib.hdiff_kid_workspace(4, 0, C.byref(need)), "m = 0")
    refused(lib.hdiff_kid_workspace(32769, 4, C.byref(need)), "n = 32769")
    refused(lib.hdiff_kid_workspace(4, 4, None), "null pointer")
    refused(lib.hdiff_feat_moments(one, 0, 4, 4, 1, one, one, None), "n = 0")
    refused(lib.hdiff_feat_moments(one, 32769, 4, 4, 1, one, one, None), "n = 32769")
    refused(lib.hdiff_feat_moments(one, 4, 0, 4, 1, one, one, None), "d = 0")
    refused(lib.hdiff_feat_moments(one, 4, 8193, 8193, 1, one, one, None), "d = 8193")
    refused(lib.hdiff_feat_moments(one, 4, 4, 0, 1, one, one, None), "strides")
    refused(lib.hdiff_feat_moments(one, 4, 4, 4, -1, one, one, None), "strides")
    for args in ((None, one, one), (one, None, one), (one, one, None)):
        refused(lib.hdiff_feat_moments(args[0], 4, 4, 4, 1, args[1], args[2], None), "null pointer")
    refused(lib.hdiff_kid_sums(one, 0, one, 4, 4, 4, 1, 4, 1, one, one, None), "n = 0")
    refused(lib.hdiff_kid_sums(one, 4, one, 0, 4, 4, 1, 4, 1, one, one, None), "m = 0")
    refused(lib.hdiff_kid_sums(one, 4, one, 4, 0, 4, 1, 4, 1, one, one, None), "d = 0")
    refused(lib.hdiff_kid_sums(one, 4, one, 4, 4, 4, 1, 0, 1, one, one, None), "strides of m")
    refused(lib.hdiff_kid_sums(one, 4, one, 4, 4, 4, 0, 4, 1, one, one, None), "strides of n")
    for k in range(4):
        ptrs = [one] * 4
        ptrs[k] = None
        refused(lib.hdiff_kid_sums(ptrs[0], 4, ptrs[1], 4, 4, 4, 1, 4, 1, ptrs[2], ptrs[3], None), "null pointer")


def test_module_refuses_cpu_tensors_and_an_empty_meter_is_nan():
    rows = torch.rand(4, 8)
    with pytest.raises(RuntimeError, match="MI355X"):
        Q.moments(rows)
    with pytest.raises(RuntimeError, match="MI355X"):
        Q.kid(rows, rows)
    meter = Q.DistributionMeter(lambda img: img.mean(dim=(2, 3)))
    with pytest.raises(RuntimeError, match="MI355X"):
        meter.update(torch.rand(2, 3, 16, 16))
    empty = meter.compute()
    assert set(empty) == {"n_pred", "n_ref", "fd", "kid", "features"}
    assert empty["n_pred"] == 0 and empty["n_ref"] == 0 and np.isnan(empty["fd"]) and np.isnan(empty["kid"])
    with pytest.raises(TypeError):
        Q.DistributionMeter(3)
    with pytest.raises(TypeError):
        Q.DinoFeatures(object())


def test_res_keys_are_unchanged_and_the_distribution_list_adds_two_lines():
    from hdiff_amd.diffusion import Evaluate as EV
    assert EV.RES_KEYS == (("psnr_orgin_avg:", "psnr"), ("ssim_orgin_avg:", "ssim"), ("uiqm_orgin_avg:", "uiqm"),
                           ("uism_orgin_avg:", "uism"), ("uicm_orgin_avg:", "uicm"), ("uiconm_orgin_avg:", "uiconm"))
    assert EV.RES_KEYS_UCIQE == EV.RES_KEYS[:3] + (("uciqe_orgin_avg:", "uciqe"),) + EV.RES_KEYS[3:]
    assert EV.RES_KEY_LPIPS == ("lpips_orgin_avg:", "lpips")
    assert EV.RES_KEYS_DISTRIBUTION == (("fd_orgin_avg:", "fd"), ("kid_orgin_avg:", "kid"))
    assert "RES_KEYS_DISTRIBUTION" in EV.__all__
    assert not any(k.startswith("fid") for k, _ in EV.RES_KEYS_DISTRIBUTION)          # a different quantity from the reference's


def test_definition_covariance_against_numpy():
    """fp32-valued rows whose mean is 1e3 times their spread, 65 x 48: within 1e-12 of the largest entry (measured 1.6e-16 when the
    change was made)."""
    x = DD.offset_features(65, 48, 3)
    mean, cov = DD.moments_def(x)
    want = np.cov(x.astype(np.float64), rowvar=False)
    gap = np.abs(cov - want).max() / np.abs(want).max()
    print(f"definition against np.cov: {gap:.1e} of the largest entry; mean {np.abs(mean - x.astype(np.float64).mean(axis=0)).max():.1e}")
    assert gap <= 1e-12
    assert np.array_equal(cov, cov.T)
    assert np.abs(mean - x.astype(np.float64).mean(axis=0)).max() <= 1e-12 * np.abs(mean).max()
    assert np.isnan(DD.moments_def(x[:1])[1]).all() and np.isfinite(DD.moments_def(x[:1])[0]).all()


@pytest.mark.parametrize("d", DIMS)
def test_frechet_commuting_full_rank(d):
    """Relative error at most 1e-11, the gate UCIQE uses (measured at most 6e-16 when the change was made)."""
    ma, ca, mb, cb, exact = DD.commuting_fixture(d, 10 + d)
    got = Q.frechet_from_moments(ma, ca, mb, cb)
    print(f"d = {d}: {got!r} exact {exact!r} rel {rel(got, exact):.1e}")
    assert rel(got, exact) <= 1e-11
    as_tensors = Q.frechet_from_moments(*(torch.from_numpy(v) for v in (ma, ca, mb, cb)))
    assert as_tensors == got


@pytest.mark.parametrize("d,rank", [(48, 20), (384, 90)])
def test_frechet_commuting_rank_deficient(d, rank):
    """Trailing eigenvalues of S_a exactly zero: the square root amplifies their rounding to about sqrt(eps) on either route, so the
    gate is the error of the ``sqrtm`` route on the same fixture, times the project's usual 4."""
    ma, ca, mb, cb, exact = DD.commuting_fixture(d, 20 + d, rank=rank)
    got, other = Q.frechet_from_moments(ma, ca, mb, cb), DD.frechet_sqrtm(ma, ca, mb, cb)
    print(f"rank {rank} of {d}: eigh route rel {rel(got, exact):.2e}, sqrtm route rel {rel(other, exact):.2e}, "
          f"ratio {abs(got - exact) / abs(other - exact):.2f}")
    assert np.isfinite(got)
    assert abs(got - exact) <= 4 * abs(other - exact)


@pytest.mark.parametrize("d", DIMS)
def test_frechet_generic_against_sqrtm(d):
    """Covariances of random data that do not commute: the two routes agree to 1e-11 relative (measured at most 5.1e-14)."""
    ma, ca, mb, cb = DD.generic_fixture(d, 30 + d)
    got, other = Q.frechet_from_moments(ma, ca, mb, cb), DD.frechet_sqrtm(ma, ca, mb, cb)
    print(f"d = {d}: eigh route {got!r} sqrtm route {other!r} rel {rel(got, other):.1e}")
    assert got > 0 and rel(got, other) <= 1e-11


@pytest.mark.parametrize("d", DIMS)
def test_frechet_of_identical_moments_is_zero(d):
    ma, ca, _, _ = DD.generic_fixture(d, 40 + d)
    got = Q.frechet_from_moments(ma, ca, ma, ca)
    print(f"d = {d}: {got:.2e} at trace {np.trace(ca):.3f}")
    assert abs(got) <= 1e-9 * np.trace(ca)


def test_frechet_refuses_bad_shapes_and_passes_nan_through():
    ma, ca, mb, cb = DD.generic_fixture(8, 1)
    with pytest.raises(ValueError):
        Q.frechet_from_moments(ma, ca[:4], mb, cb)
    bad = ca.copy()
    bad[2, 3] = np.nan
    assert np.isnan(Q.frechet_from_moments(ma, bad, mb, cb))
    assert np.isnan(Q.frechet_from_moments(ma, ca, mb, np.full_like(cb, np.nan)))


def test_definition_kid_against_a_matrix_expression():
    """90 x 48 against 70 x 48 standard normals: the definition agrees with a direct matrix expression within 1e-12 (of the three
    terms' size), and a shifted set scores higher than a redraw of the same distribution (measured 0.97 against 0.009)."""
    rng = np.random.default_rng(7)
    a = rng.standard_normal((90, 48)).astype(np.float32)
    redraw = rng.standard_normal((70, 48)).astype(np.float32)
    shifted = (rng.standard_normal((70, 48)) + 0.5).astype(np.float32)

    def direct(x, y):
        x, y = x.astype(np.float64), y.astype(np.float64)
        n, m, d = x.shape[0], y.shape[0], x.shape[1]
        kxx, kyy, kxy = (x @ x.T / d + 1) ** 3, (y @ y.T / d + 1) ** 3, (x @ y.T / d + 1) ** 3
        terms = ((kxx.sum() - np.trace(kxx)) / (n * (n - 1)), (kyy.sum() - np.trace(kyy)) / (m * (m - 1)), 2 * kxy.mean())
        return terms[0] + terms[1] - terms[2], sum(abs(t) for t in terms)

    scores = {}
    for name, b in (("redraw", redraw), ("shifted", shifted)):
        got = DD.kid_def(a, b)
        want, size = direct(a, b)
        print(f"{name}: definition {got!r} direct {want!r} gap {abs(got - want) / size:.1e} of the terms")
        assert abs(got - want) <= 1e-12 * size
        scores[name] = got
    assert scores["shifted"] > 10 * abs(scores["redraw"])
    assert np.isnan(DD.kid_def(a[:1], redraw)) and np.isnan(DD.kid_def(a, redraw[:1]))
    assert np.isnan(Q._kid_from_sums((1.0, 1.0, 1.0), 1, 5)) and np.isnan(Q._kid_from_sums((1.0, np.inf, 1.0), 4, 5))
    assert Q._kid_from_sums((6.0, 40.0, 30.0), 3, 5) == DD.kid_from_sums((6.0, 40.0, 30.0), 3, 5)
