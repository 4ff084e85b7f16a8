"""Host-side tests of the device NIQE (no GPU): properties of the float64 definition the kernels are held to (tests/_niqe_def.py), the
table margins of every fixture the GPU tests compare (which is what lets them demand an exactly equal ``alpha``), the host finish
``niqe_from_moments``, ``NIQEModel`` files, the C ABI's new entries and their argument checks, the meter's columns and the line order
of ``res.txt``.

Nothing here is compared with the authors' MATLAB release: there is none on the build machine, and the definition was written from
the paper and from memory of that release.  A constant non-zero block (a rounding residue for sigma: finite, rounding-dependent
features in any implementation) is in no fixture: every fixture carries noise on every pixel."""
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
from hdiff_amd.diffusion import Evaluate as EV  # noqa: E402
import _niqe_def as D  # noqa: E402

NEW_SYMBOLS = {"hdiff_niqe_workspace", "hdiff_niqe_features", "hdiff_niqe_moments", "hdiff_niqe_keep", "hdiff_niqe_pool_moments"}
MARGIN = 1e-9


# ---------------------------------------------------------------------------------------------------------------- definition
def test_window_and_reduction():
    w = D.g7()
    assert abs(w.sum() - 1.0) <= 1e-15 and np.array_equal(w, w[::-1]) and w.argmax() == 3
    # the kernel file holds the window as literals: they are this window
    text = open(os.path.join(os.path.dirname(_capi.LIB_PATH), "csrc", "niqe.hip")).read()
    held = re.search(r"kWin\[7\] = \{([^}]*)\}", text).group(1)
    assert [float(v) for v in held.split(",")] == w.tolist()
    held = re.search(r"kCubic\[8\] = \{([^}]*)\}", text).group(1)
    assert [float(v) for v in held.split(",")] == D.half_weights().tolist() and D.half_weights().sum() == 1.0
    const = np.full((12, 20), 37.25)
    assert np.array_equal(D.half(const), np.full((6, 10), 37.25))
    assert np.abs(D.filt(const) - 37.25).max() <= 1e-13
    y, x = np.mgrid[0:32, 0:48].astype(np.float64)
    ramp = 3.0 * x - 2.0 * y + 5.0
    got = D.half(ramp)
    oy, ox = np.mgrid[0:16, 0:24].astype(np.float64)
    want = 3.0 * (2 * ox + 0.5) - 2.0 * (2 * oy + 0.5) + 5.0          # the ramp at the output centres
    assert np.abs(got - want)[2:-2, 2:-2].max() <= 1e-12               # away from the clamped edges a cubic kernel keeps a line
    assert np.abs(got - want).max() > 1e-3                              # at the edges it does not


def generalised_gaussian(shape: float, n: int, seed: int) -> np.ndarray:
    """Samples of density ~ exp(-|x|^shape): sign * Gamma(1 / shape)^(1 / shape)."""
    rng = np.random.default_rng(seed)
    return rng.choice([-1.0, 1.0], n) * rng.gamma(1.0 / shape, 1.0, n) ** (1.0 / shape)


@pytest.mark.parametrize("shape", [1.0, 2.0, 4.0])
def test_aggd_recovers_the_shape(shape):
    alpha, bl, br, rn = D.aggd(generalised_gaussian(shape, 100000, 5)[None])
    print(f"shape {shape}: alpha {alpha[0]} bl {bl[0]} br {br[0]}")
    assert abs(alpha[0] - shape) <= 0.05
    assert abs(bl[0] - br[0]) <= 0.02 * br[0]                          # a symmetric density


def test_table_is_monotone_and_nan_has_no_answer():
    R = D.table()
    assert R.shape == (9801,) and (np.diff(R) > 0).all() and D.GAM[0] == 0.2 and abs(D.GAM[-1] - 10.0) < 1e-12
    assert abs(R[1800] - 2.0 / np.pi) <= 1e-12                         # a Gaussian: gamma = 2
    assert abs(R[800] - 0.5) <= 1e-12                                  # a Laplacian: gamma = 1
    alpha, _, _, _ = D.aggd(np.zeros((1, 16)))                         # neither negative nor positive values
    assert np.isnan(alpha[0])


def test_every_compared_fixture_keeps_its_table_margin():
    """What lets tests/test_gpu_niqe.py demand ``alpha`` exactly: no estimate of any compared fixture is within 1e-9 (relative) of
    the point where its table entry changes, and every compared row is finite."""
    worst = np.inf
    for seed, H, W, noise, patch, quantize in D.compared_fixtures():
        feats, sharp, margin = D.features(D.image(seed, H, W, noise), patch, quantize)
        assert np.isfinite(feats).all() and np.isfinite(sharp).all() and (sharp > 1.0).all(), (seed, H, W, noise, patch, quantize)
        assert margin.min() >= MARGIN, (seed, H, W, noise, patch, quantize, margin.min())
        worst = min(worst, margin.min())
    img = D.image(D.ZERO_SEED, 64, 160)
    img[:, :, :80] = 0.0
    feats, _, margin = D.features(img, 16)
    ok = D.valid_rows(feats)
    assert ok.reshape(4, 10).tolist() == [[False] * 5 + [True] * 5] * 4 and margin[ok].min() >= MARGIN
    print(f"smallest table margin over {len(D.compared_fixtures())} fixtures: {worst:.2e}")


def test_definition_separates_clean_from_noisy_and_survives_four_blocks():
    mu, cov, kept = D.fit([D.image(s, 96, 128, D.CLEAN_NOISE) for s in D.FIT_SEEDS], 16)
    assert all(k.sum() >= 1 for k in kept) and sum(int(k.sum()) for k in kept) > 36
    clean = D.niqe(D.image(D.SCORE_SEED, 96, 128, D.CLEAN_NOISE), mu, cov, 16)
    noisy = D.niqe(D.image(D.SCORE_SEED, 96, 128, D.NOISY_NOISE), mu, cov, 16)
    four = D.niqe(D.image(D.SCORE_SEED, 32, 32, D.CLEAN_NOISE), mu, cov, 16)
    print(f"clean {clean} noisy {noisy} four blocks {four}")
    assert np.isfinite([clean, noisy, four]).all() and clean < noisy
    spoiled = D.image(D.SCORE_SEED, 48, 64)
    spoiled[1, 5, 7] = np.nan
    assert np.isnan(D.features(spoiled, 16)[0]).all() and np.isnan(D.niqe(spoiled, mu, cov, 16))
    spoiled[1, 5, 7] = np.inf                                          # clipped to 1 like any other value
    assert np.isfinite(D.niqe(spoiled, mu, cov, 16))


# ---------------------------------------------------------------------------------------------------------------- host finish
def test_niqe_from_moments():
    rng = np.random.default_rng(3)
    a, b = rng.uniform(0.5, 2.0, 36), rng.uniform(0.5, 2.0, 36)
    mu, mean = rng.standard_normal(36), rng.standard_normal(36)
    model = Q.NIQEModel(mu, np.diag(a), patch=16)
    want = float(np.sqrt(np.sum((mu - mean) ** 2 / ((a + b) / 2))))
    got = Q.niqe_from_moments(model, mean, np.diag(b))
    assert abs(got - want) <= 1e-12 * want
    assert Q.niqe_from_moments(model, mu, np.diag(b)) == 0.0
    assert Q.niqe_from_moments(model, torch.from_numpy(mean), torch.from_numpy(np.diag(b))) == got
    rows = rng.standard_normal((4, 36))                                # four rows: a covariance of rank 3
    cov = np.cov(rows, rowvar=False)
    assert np.linalg.matrix_rank(cov) == 3
    low = Q.niqe_from_moments(Q.NIQEModel(mu, cov, patch=16), rows.mean(axis=0), cov, 4)
    assert np.isfinite(low) and low >= 0.0
    assert np.isnan(Q.niqe_from_moments(model, mean, np.full((36, 36), np.nan)))          # the kernel's covariance of one row
    assert np.isnan(Q.niqe_from_moments(model, mean, np.diag(b), 1))
    assert np.isnan(Q.niqe_from_moments(model, np.full(36, np.nan), np.diag(b), 0))
    assert D.score(mu, np.diag(a), mean, np.diag(b), 5) == got          # the definition's finish is the same expression
    with pytest.raises(ValueError, match="36"):
        Q.niqe_from_moments(model, mean[:35], np.diag(b))
    with pytest.raises(TypeError, match="NIQEModel"):
        Q.niqe_from_moments((mu, np.diag(a)), mean, np.diag(b))


def test_model_files(tmp_path):
    from scipy.io import savemat
    rng = np.random.default_rng(4)
    mu, root = rng.standard_normal(36), rng.standard_normal((36, 36))
    cov = root @ root.T
    model = Q.NIQEModel(mu, cov, patch=32, quantize=False)
    path = str(tmp_path / "pristine.npz")
    model.save(path)
    assert os.path.exists(path)
    back = Q.NIQEModel.load(path)
    assert back.patch == 32 and back.quantize is False
    assert np.array_equal(back.mean, mu) and np.array_equal(back.cov, cov)
    assert Q.NIQEModel.load(path, patch=32).patch == 32
    with pytest.raises(ValueError, match="patch = 32"):
        Q.NIQEModel.load(path, patch=96)
    mat = str(tmp_path / "modelparameters.mat")
    savemat(mat, {"mu_prisparam": mu.reshape(1, 36), "cov_prisparam": cov})
    released = Q.NIQEModel.load(mat)
    assert released.patch == 96 and released.quantize is True
    assert np.array_equal(released.mean, mu) and np.array_equal(released.cov, cov)
    with pytest.raises(ValueError, match="patch = 96"):
        Q.NIQEModel.load(mat, patch=32)
    savemat(mat, {"mu_prisparam": mu.reshape(1, 36)})
    with pytest.raises(ValueError, match="cov_prisparam"):
        Q.NIQEModel.load(mat)
    for bad in (dict(mean=mu[:30], cov=cov), dict(mean=mu, cov=cov[:30]), dict(mean=np.full(36, np.nan), cov=cov)):
        with pytest.raises(ValueError):
            Q.NIQEModel(bad["mean"], bad["cov"])
    for patch in (6, 7, 33, 514, 16.5, True):
        with pytest.raises(ValueError, match="patch"):
            Q.NIQEModel(mu, cov, patch=patch)


# ---------------------------------------------------------------------------------------------------------------- C ABI
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
    assert lib.hdiff_niqe_workspace(1, 3024, 4032, 96, C.byref(need)) == 0
    cropped = (3024 // 96 * 96) * (4032 // 96 * 96)
    assert 3.25 * 8 * cropped <= need.value <= 3.25 * 8 * cropped + 4096          # gray, its reduction, m and sigma; the flags
    two = C.c_int64(0)
    assert lib.hdiff_niqe_workspace(2, 3024, 4032, 96, C.byref(two)) == 0 and two.value > need.value
    assert lib.hdiff_niqe_workspace(1, 16384, 16384, 512, C.byref(need)) == 0
    assert lib.hdiff_niqe_workspace(1, 8, 8, 8, C.byref(need)) == 0 and need.value > 0
    one = 8          # any non-null address: validation returns before anything is read or launched

    def refused(rc, word):
        assert rc == -1
        assert word in lib.hdiff_last_error().decode(), lib.hdiff_last_error()

    for patch in (0, 6, 9, 97, 514, -8):
        refused(lib.hdiff_niqe_workspace(1, 1024, 1024, patch, C.byref(need)), "patch")
        refused(lib.hdiff_niqe_features(one, 1, 1024, 1024, patch, 1, one, one, one, None), "patch")
    refused(lib.hdiff_niqe_workspace(1, 95, 200, 96, C.byref(need)), "at least patch")
    refused(lib.hdiff_niqe_features(one, 1, 200, 95, 96, 1, one, one, one, None), "at least patch")
    refused(lib.hdiff_niqe_workspace(1, 16385, 200, 96, C.byref(need)), "too large")
    refused(lib.hdiff_niqe_features(one, 1, 200, 16385, 96, 1, one, one, one, None), "too large")
    refused(lib.hdiff_niqe_workspace(0, 200, 200, 96, C.byref(need)), "N = 0")
    refused(lib.hdiff_niqe_features(one, 65536, 200, 200, 96, 1, one, one, one, None), "N = 65536")
    refused(lib.hdiff_niqe_workspace(1, 200, 200, 96, None), "null pointer")
    for args in ((None, one, one, one), (one, None, one, one), (one, one, None, one), (one, one, one, None)):
        img, feats, sharp, scratch = args
        refused(lib.hdiff_niqe_features(img, 1, 200, 200, 96, 1, feats, sharp, scratch, None), "null pointer")
    for name in ("hdiff_niqe_moments", "hdiff_niqe_keep"):
        f = getattr(lib, name)
        refused(f(one, one, 0, 4, 0.0, one, None), "N = 0")
        refused(f(one, one, 1, 0, 0.0, one, None), "P = 0")
        refused(f(one, one, 1, (1 << 22) + 1, 0.0, one, None), "P = ")
        for t in (-0.1, 1.0, float("nan"), float("inf")):
            refused(f(one, one, 1, 4, t, one, None), "sharp_threshold")
        refused(f(None, one, 1, 4, 0.0, one, None), "null pointer")
        refused(f(one, one, 1, 4, 0.0, None, None), "null pointer")
        refused(f(one, None, 1, 4, 0.75, one, None), "null pointer")      # a threshold needs the sharpness
    refused(lib.hdiff_niqe_pool_moments(one, one, 0, one, None), "rows = 0")
    refused(lib.hdiff_niqe_pool_moments(one, one, (1 << 26) + 1, one, None), "rows = ")
    for args in ((None, one, one), (one, None, one), (one, one, None)):
        refused(lib.hdiff_niqe_pool_moments(args[0], args[1], 4, args[2], None), "null pointer")


def test_python_argument_checks():
    img = torch.rand(2, 3, 32, 32)
    model = Q.NIQEModel(np.zeros(36), np.eye(36), patch=16)
    with pytest.raises(RuntimeError, match="MI355X"):
        Q.niqe_features(img, patch=16)
    with pytest.raises(RuntimeError, match="MI355X"):
        Q.niqe(img, model)
    with pytest.raises(RuntimeError, match="MI355X"):
        Q.NIQEModel.fit([img], patch=16)
    with pytest.raises(RuntimeError, match="MI355X"):
        Q.QualityMeter(niqe=model).update(img)
    for patch in (6, 15, 1024, 16.5):
        with pytest.raises(ValueError, match="patch"):
            Q.niqe_features(img, patch=patch)
        with pytest.raises(ValueError, match="patch"):
            Q.NIQEModel.fit([img], patch=patch)
    for threshold in (-0.5, 1.0, float("nan")):
        with pytest.raises(ValueError, match="sharp_threshold"):
            Q.NIQEModel.fit([img], patch=16, sharp_threshold=threshold)
    with pytest.raises(ValueError, match="no images"):
        Q.NIQEModel.fit([], patch=16)
    with pytest.raises(TypeError, match="NIQEModel"):
        Q.niqe(img, (np.zeros(36), np.eye(36)))
    with pytest.raises(TypeError, match="NIQEModel"):
        Q.QualityMeter(niqe="pristine.npz")
    with pytest.raises(ValueError, match="patch = 16"):
        Q._niqe_blocks(15, 64, 16)
    assert Q._niqe_blocks(43, 61, 8) == 35 and Q._niqe_blocks(3024, 4032, 96) == 1302 and Q._niqe_blocks(256, 256, 96) == 4


# ---------------------------------------------------------------------------------------------------------------- meter, res.txt
def test_meter_columns():
    model = Q.NIQEModel(np.zeros(36), np.eye(36), patch=16)
    assert Q.NIQE_COLUMNS == ("niqe",) and Q.NIQE_MOMENTS == 1333
    assert Q.QualityMeter().columns == Q.COLUMNS
    assert Q.QualityMeter(niqe=model).columns == Q.COLUMNS + Q.NIQE_COLUMNS
    assert Q.QualityMeter(uciqe=True, niqe=model).columns == Q.COLUMNS + Q.UCIQE_COLUMNS + Q.NIQE_COLUMNS
    lpips = object.__new__(Q.LPIPS)                                    # the column order needs no weights
    assert Q.QualityMeter(lpips=lpips, niqe=model).columns == Q.COLUMNS + Q.LPIPS_COLUMNS + Q.NIQE_COLUMNS
    assert Q.QualityMeter(uciqe=True, lpips=lpips, niqe=model).columns == Q.COLUMNS + Q.UCIQE_COLUMNS + Q.LPIPS_COLUMNS + Q.NIQE_COLUMNS
    assert Q.QualityMeter(uciqe=True, lpips=lpips).columns == Q.COLUMNS + Q.UCIQE_COLUMNS + Q.LPIPS_COLUMNS
    empty = Q.QualityMeter(niqe=model).compute()
    assert set(empty) == {"n", "per_image", "niqe_undefined"} | set(Q.COLUMNS) | set(Q.NIQE_COLUMNS)
    assert empty["n"] == 0 and empty["per_image"].shape == (0, 7) and empty["niqe_undefined"] == 0 and np.isnan(empty["niqe"])
    plain = Q.QualityMeter().compute()
    assert set(plain) == {"n", "per_image"} | set(Q.COLUMNS) and plain["per_image"].shape == (0, 6)


class StubMeter:
    """Stands in for the quality meter: evaluate's bookkeeping and res.txt need no device."""

    def __init__(self):
        self.n = 0

    def update(self, pred01, target01):
        self.n += int(pred01.shape[0])

    def compute(self):
        res = {k: float(i) for i, k in enumerate(Q.COLUMNS + Q.UCIQE_COLUMNS + Q.LPIPS_COLUMNS + Q.NIQE_COLUMNS)}
        res.update(n=self.n, niqe_undefined=0)
        return res


def res_keys(path):
    return [ln.split(":")[0] + ":" for ln in open(path).read().split("\n") if ln]


def test_res_txt_line_order_on_a_stub_sampler(tmp_path):
    model = Q.NIQEModel(np.zeros(36), np.eye(36), patch=16)
    batches = [(torch.zeros(2, 3, 32, 32), torch.zeros(2, 3, 32, 32))]
    sampler = lambda inp, **kw: inp / 127.5 - 1                          # noqa: E731
    lpips = object.__new__(Q.LPIPS)
    base = [k for k, _ in EV.RES_KEYS]
    EV.evaluate(sampler, batches, ddim_step=2, save_dir=str(tmp_path / "a"), meter=StubMeter(), niqe=model)
    assert res_keys(str(tmp_path / "a" / "res.txt")) == base + ["niqe_orgin_avg:"]
    EV.evaluate(sampler, batches, ddim_step=2, save_dir=str(tmp_path / "b"), meter=StubMeter(), uciqe=True, lpips=lpips, niqe=model)
    assert res_keys(str(tmp_path / "b" / "res.txt")) == [k for k, _ in EV.RES_KEYS_UCIQE] + ["lpips_orgin_avg:", "niqe_orgin_avg:"]
    EV.evaluate(sampler, batches, ddim_step=2, save_dir=str(tmp_path / "c"), meter=StubMeter())
    assert res_keys(str(tmp_path / "c" / "res.txt")) == base
    path = str(tmp_path / "pristine.npz")
    model.save(path)
    res = EV.evaluate(sampler, batches, ddim_step=2, save_dir=str(tmp_path / "d"), meter=StubMeter(), niqe=path)      # a path is loaded
    assert res_keys(str(tmp_path / "d" / "res.txt")) == base + ["niqe_orgin_avg:"] and "niqe_full" not in res
    assert EV.RES_KEY_NIQE == ("niqe_orgin_avg:", "niqe") and EV.RES_KEY_NIQE_FULL == ("niqe_full_orgin_avg:", "niqe_full")
    assert "fit_niqe" in EV.__all__ and callable(EV.fit_niqe)
    with pytest.raises(ValueError, match="side"):
        EV.fit_niqe({}, out=str(tmp_path / "m.npz"), side="both")
