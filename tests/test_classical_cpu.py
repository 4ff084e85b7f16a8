"""The classical baselines without a GPU: the definition (tests/_classical_def.py) against closed forms and on the procedural scenes,
and the host-side argument checks of hdiff_amd.classical and Evaluate.evaluate(baselines=)."""
import math

import numpy as np
import pytest
import torch

import _classical_def as CD
from hdiff_amd import classical
from hdiff_amd.diffusion import Evaluate

f32, f64 = np.float32, np.float64


def test_closed_form_recovers_the_scene():
    """J with dark channel 0 at the patch scale under a constant t: t_raw = t, and J comes back."""
    rng = np.random.default_rng(3)
    H, W, patch = 24, 30, 5
    J = rng.random((3, H, W)).astype(f32)
    J[rng.integers(0, 3, (H, W)), np.arange(H)[:, None], np.arange(W)[None, :]] = 0.0     # a zero channel at EVERY pixel
    A = np.array([0.9, 0.8, 0.85], dtype=f32)
    t = 0.6
    I = (J.astype(f64) * t + A.astype(f64)[:, None, None] * (1.0 - t)).astype(f32)
    got = CD.dehaze_def(I, patch=patch, omega=1.0, t0=0.1, airlight=A, refine=None)
    # min_c I_c / A_c = 1 - t up to the roundings of I (2^-24 relative) and of the quotient: a few fp32 steps of 1
    assert np.abs(got["t_raw"].astype(f64) - t).max() <= 4 * 2.0 ** -24
    # J = (I - A) / t + A: the rounding of I and the error of t_raw, both divided by t
    assert np.abs(got["J"].astype(f64) - J).max() <= (2.0 ** -24 + 4 * 2.0 ** -24) / t + 2.0 ** -24
    assert got["t"] is got["t_raw"]


def test_borders_and_patch_size():
    rng = np.random.default_rng(4)
    x = rng.random((3, 5, 7)).astype(f32)
    assert np.array_equal(CD.dark_channel_def(x, 15), np.full((5, 7), x.min(), dtype=f32))          # the window covers the image
    assert np.array_equal(CD.dark_channel_def(x, 1), x.min(axis=0))
    assert np.array_equal(CD.dark_channel_def(x, 1, "gb"), x[1:].min(axis=0))
    d = CD.dark_channel_def(x, 3)
    assert d[0, 0] == x[:, :2, :2].min() and d[4, 6] == x[:, 3:, 5:].min() and d[2, 3] == x[:, 1:4, 2:5].min()
    # brute force over every pixel, a window that is clipped on some sides only
    want = np.array([[x[:, max(0, i - 2):i + 3, max(0, j - 2):j + 3].min() for j in range(7)] for i in range(5)], dtype=f32)
    assert np.array_equal(CD.dark_channel_def(x, 5), want)


def test_airlight_rule_on_a_two_level_image():
    """A constant dark channel makes every pixel a candidate; equal sums go to the lowest index."""
    H, W = 6, 8
    x = np.zeros((3, H, W), dtype=f32)
    x[0] = 0.25                                    # dark channel (min over channels) is 0 everywhere
    bright = [(1, 5), (3, 2), (4, 7)]
    for (i, j) in bright:
        x[:, i, j] = (0.75, 0.0, 0.5)
    dark = CD.dark_channel_def(x, 1)
    assert (dark == 0).all()
    A, cut, index = CD.airlight_def(x, dark, 1)
    assert cut == 0 and index == 1 * W + 5
    assert np.array_equal(A, np.array([0.75, 1.0 / 255.0, 0.5], dtype=f32))       # the floor of 1 / 255 on the zero channel
    x[:, 0, 3] = (0.5, 0.25, 0.5)                  # the same sum 1.25, earlier
    assert CD.airlight_def(x, dark * 0, 1)[2] == 3
    # n_top = 1 with distinct dark values: the single brightest-dark pixel, whatever its colour
    d2 = np.arange(H * W, dtype=f32).reshape(H, W) / (H * W)
    assert CD.airlight_def(x, d2, 1)[2] == H * W - 1
    assert CD.n_top_of(1e-3, 64, 64) == 4 and CD.n_top_of(1e-3, 8, 13) == 1


@pytest.fixture(scope="module")
def sets():
    return CD.scene_sets()


def test_dcp_lifts_the_haze_set(sets):
    """Measured with this definition: 11.31 -> 16.36 dB (+5.05), 7 of 8 scenes improved."""
    clean, deg = sets["haze"]
    before = [CD.psnr(deg[i], clean[i]) for i in range(8)]
    after = [CD.psnr(CD.dehaze_def(deg[i], prior="dcp", patch=7, refine=None)["J"], clean[i]) for i in range(8)]
    print("haze: PSNR", np.mean(before), "->", np.mean(after), "improved", sum(a > b for a, b in zip(after, before)))
    assert np.mean(after) - np.mean(before) >= 3.0
    assert sum(a > b for a, b in zip(after, before)) >= 6


def test_inverted_dcp_lifts_the_lowlight_set(sets):
    """Measured with this definition: 10.01 -> 14.42 dB (+4.41), 8 of 8."""
    clean, deg = sets["lowlight"]
    before = [CD.psnr(deg[i], clean[i]) for i in range(8)]
    after = [CD.psnr(CD.dehaze_def(deg[i], prior="inverted_dcp", patch=7, refine=None)["J"], clean[i]) for i in range(8)]
    print("lowlight: PSNR", np.mean(before), "->", np.mean(after), "improved", sum(a > b for a, b in zip(after, before)))
    assert np.mean(after) - np.mean(before) >= 2.0


def test_gray_world_cuts_the_underwater_cast(sets):
    """Measured with this definition: angular error 27.40 -> 14.03 degrees, 8 of 8."""
    clean, deg = sets["underwater"]
    before = [CD.angular_error(deg[i], clean[i]) for i in range(8)]
    after = [CD.angular_error(CD.white_balance_def(deg[i], 1.0)[0], clean[i]) for i in range(8)]
    print("underwater: angular", np.mean(before), "->", np.mean(after), "improved", sum(a < b for a, b in zip(after, before)))
    assert np.mean(after) <= np.mean(before) * 2.0 / 3.0
    assert sum(a < b for a, b in zip(after, before)) >= 7


def test_white_balance_definition():
    rng = np.random.default_rng(6)
    x = rng.random((3, 9, 11)).astype(f32)
    x[0] *= 0.3
    out, g = CD.white_balance_def(x, 1.0)
    m = x.astype(f64).reshape(3, -1).mean(axis=1)
    assert np.allclose(g, m.mean() / m, rtol=1e-14)
    scaled = x.astype(f64) * g[:, None, None]
    assert np.allclose(scaled.reshape(3, -1).mean(axis=1), m.mean(), rtol=1e-12)          # gray-world: equal channel means
    _, g_inf = CD.white_balance_def(x, math.inf)
    mx = x.reshape(3, -1).max(axis=1).astype(f64)
    assert np.array_equal(g_inf, ((mx[0] + mx[1]) + mx[2]) / 3.0 / mx)
    _, g6 = CD.white_balance_def(x, 6.0)
    m6 = (x.astype(f64).reshape(3, -1) ** 6).mean(axis=1) ** (1.0 / 6.0)                   # the Minkowski 6-norm of each channel
    assert np.allclose(g6, m6.mean() / m6, rtol=1e-13)
    assert np.all(m <= m6) and np.all(m6 <= mx)                                          # a power mean lies between mean and maximum
    black = np.zeros((3, 4, 4), dtype=f32)
    assert np.array_equal(CD.white_balance_def(black, 1.0)[0], black)                     # the floor of 1e-6: no division by zero


def test_argument_checks_come_before_any_device_work():
    cpu = torch.zeros(1, 3, 8, 8)
    for bad in (dict(patch=4), dict(patch=65), dict(patch=0), dict(top=0.0), dict(top=1.5), dict(refine=(0, 1e-3)),
                dict(refine=(4, 0.0)), dict(refine=(4,)), dict(prior="he"), dict(omega=1.5), dict(t0=0.0)):
        with pytest.raises(ValueError):
            classical.dehaze(cpu, **bad)
    with pytest.raises(TypeError):
        classical.dehaze(cpu, patch=7.0)
    for bad in (0.5, float("nan"), -1):
        with pytest.raises(ValueError):
            classical.white_balance(cpu, p=bad)
    with pytest.raises(ValueError):
        classical.dark_channel(cpu, patch=2)
    with pytest.raises(ValueError):
        classical.dark_channel(cpu, channels="rg")
    # good settings reach the tensor check: CPU tensors are refused, there is no fallback
    for call in (lambda: classical.dehaze(cpu), lambda: classical.white_balance(cpu), lambda: classical.dark_channel(cpu)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError):
        classical.dehaze(torch.zeros(1, 1, 8, 8))


def test_evaluate_rejects_bad_baselines_before_sampling():
    calls = []

    def sampler(*a, **k):
        calls.append(1)
        raise AssertionError("the sampler must not run")

    def batches():
        calls.append(1)
        yield None

    for bad, err in ((("input", "clahe"), ValueError), ("dcp", TypeError), (("dcp", "dcp"), ValueError), ((("mine", 3),), TypeError),
                     ((("my name", lambda x: x),), ValueError), ((7,), TypeError)):
        with pytest.raises(err):
            Evaluate.evaluate(sampler, batches(), ddim_step=2, baselines=bad)
    assert not calls
    assert set(classical.BASELINES) == {"input", "gray_world", "dcp", "udcp", "inverted_dcp"}
    assert [n for n, _ in classical.resolve_baselines(["udcp", ("mine", lambda x: x)])] == ["udcp", "mine"]


def test_baseline_res_lines_follow_every_other_line():
    result = {"psnr": 1.0, "ssim": 2.0, "uiqm": 3.0, "uism": 4.0, "uicm": 5.0, "uiconm": 6.0, "fd": 7.0, "kid": 8.0,
              "baselines": {"input": dict(psnr=.1, ssim=.2, uiqm=.3, uism=.4, uicm=.5, uiconm=.6),
                            "dcp": dict(psnr=.7, ssim=.8, uiqm=.9, uism=1., uicm=1.1, uiconm=1.2)}}
    keys = Evaluate.RES_KEYS + Evaluate.RES_KEYS_DISTRIBUTION
    flat, out = Evaluate.baseline_res_lines(result, keys, ("psnr", "ssim", "uiqm", "uicm", "uism", "uiconm"))
    assert out[:len(keys)] == keys
    labels = [k for k, _ in out[len(keys):]]
    assert labels == [f"{s}_{n}_avg:" for n in ("input", "dcp") for s in ("psnr", "ssim", "uiqm", "uism", "uicm", "uiconm")]
    assert flat["psnr_dcp_avg"] == .7 and "fd_input_avg" not in flat
