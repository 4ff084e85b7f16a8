"""Host-side tests of the device colour differences (no GPU): the float64 definition the kernels are held to (tests/_color_def.py)
against the published table of Sharma, Wu and Dalal (tests/golden/ciede2000_sharma.json), CIE76 and the angle on hand-made pixels, the
percentile index, the hue-branch margins of every fixture the GPU tests compare (which is what keeps a flipped branch from hiding behind
a tolerance), the C ABI's new entries and their argument checks, the meter's columns and the lines of ``res.txt``.

Agreement with scikit-image's ``deltaE_ciede2000`` is not pinned: there is none on the build machine.  The table is the stronger anchor."""
import ctypes as C
import json
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
import _color_def as D  # noqa: E402
import _uciqe_def as UD  # noqa: E402

NEW_SYMBOLS = {"hdiff_color_diff_workspace", "hdiff_color_diff", "hdiff_ciede2000_lab"}
TABLE_GATE = 6e-5          # the table is rounded to four decimals: 5e-5 plus slack
MARGIN = 1e-6              # degrees


def table():
    rows = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "ciede2000_sharma.json")))["pairs"], dtype=np.float64)
    assert rows.shape == (34, 7)
    return rows[:, :3], rows[:, 3:6], rows[:, 6]


def pixel(rgb):
    return np.asarray(rgb, dtype=np.float32).reshape(3, 1, 1)


# ---------------------------------------------------------------------------------------------------------------- definition
def test_definition_reproduces_the_published_table():
    lab1, lab2, want = table()
    got = D.ciede2000_lab_def(lab1, lab2)
    swapped = D.ciede2000_lab_def(lab2, lab1)
    for i in range(34):
        print(f"pair {i + 1}: definition {got[i]!r}  table {want[i]}  swapped {swapped[i]!r}")
    print("worst deviation from the table", float(np.abs(got - want).max()))
    assert np.abs(got - want).max() <= TABLE_GATE
    assert (np.abs(swapped - got) <= 1e-13 * got).all()


def test_lab_is_the_uciqe_definitions_by_import():
    assert D.lab_def is UD.lab_def and D.seq_sum is UD.seq_sum


def test_cie76_and_angle_on_hand_made_pixels():
    red, green = pixel((1, 0, 0)), pixel((0, 1, 0))
    de00, _, de76, angular = D.color_def(red, green)
    assert abs(angular - 90.0) <= 1e-13
    lab_r = [float(v[0, 0]) for v in UD.lab_def(red.astype(np.float64))]
    lab_g = [float(v[0, 0]) for v in UD.lab_def(green.astype(np.float64))]
    assert abs(de76 - np.sqrt(sum((a - b) ** 2 for a, b in zip(lab_r, lab_g)))) <= 1e-12 * de76 and de76 > 100 and 0 < de00 < de76
    colour = pixel((0.11, 0.37, 0.29))
    assert D.color_def(colour, colour * np.float32(2))[3] == 0.0                # its double, inside [0, 1]: parallel, exactly
    assert D.color_def(colour, colour * np.float32(8))[3] > 0.0                 # clipped: no longer parallel
    # black against anything is excluded: the mean runs over the other pixel alone
    p = np.concatenate([pixel((0, 0, 0)), red], axis=2)
    t = np.concatenate([green, green], axis=2)
    assert abs(D.color_def(p, t)[3] - 90.0) <= 1e-13 and abs(D.color_def(t, p)[3] - 90.0) <= 1e-13
    black = np.zeros((3, 4, 5), dtype=np.float32)
    scores = D.color_def(black, np.full((3, 4, 5), 0.5, dtype=np.float32))
    assert np.isnan(scores[3]) and all(np.isfinite(v) and v > 0 for v in scores[:3])
    assert np.isnan(D.color_def(pixel((-3, 0, 0)), green)[3])                   # clipped to black


def test_percentile_index():
    assert [D.p95_index(n) for n in (1, 19, 20, 21, 100, 104)] == [0, 18, 18, 19, 94, 98]


def test_identical_images_give_exactly_zero():
    for H, W, seed, near in D.FIXTURES[:2]:
        p, _ = D.fixture(H, W, seed, near)
        assert D.color_def(p, p.copy()) == (0.0, 0.0, 0.0, 0.0)


def test_a_non_finite_value_in_either_image_makes_all_four_nan():
    p, t = D.fixture(8, 13, 2000)
    for value in (np.nan, np.inf, -np.inf):
        bad = p.copy()
        bad[1, 3, 4] = value
        assert np.isnan(D.color_def(bad, t)).all() and np.isnan(D.color_def(t, bad)).all()


# The figures of the four fixtures named when the feature was specified: size, seed, near -> (min ||dh| - 180|, min |h1 + h2 - 360| among
# the wrapped pixels, wrapped, of them with sum < 360, with sum >= 360, pixels with C1' C2' > 1e-6)
RECORDED = {(8, 13, 2000, False): (0.105, 0.045, 25, 7, 18, 104), (33, 47, 2003, False): (0.549, 0.265, 411, 138, 273, 1551),
            (72, 120, 2001, False): (0.0143, 0.0478, 2454, 811, 1643, 8640), (72, 120, 2002, True): (2.34, 0.038, None, None, None, 8640)}


@pytest.mark.parametrize("H,W,seed,near", D.FIXTURES)
def test_every_compared_fixture_keeps_its_hue_margins(H, W, seed, near):
    p, t = D.fixture(H, W, seed, near)
    terms = D.pixels_def(p, t)[4]
    chromatic = terms["cc"] > 1e-6
    gap, total = np.abs(terms["h1"] - terms["h2"]), terms["h1"] + terms["h2"]
    wrapped = chromatic & (gap > 180.0)
    below, above = wrapped & (total < 360.0), wrapped & (total >= 360.0)
    to_180 = float(np.abs(gap[chromatic] - 180.0).min())
    to_360 = float(np.abs(total[wrapped] - 360.0).min())
    print(f"{H}x{W} seed {seed}: min ||dh| - 180| {to_180:.4g}, min |h1 + h2 - 360| among wrapped {to_360:.4g}, wrapped "
          f"{int(wrapped.sum())} of {int(chromatic.sum())}, sum < 360: {int(below.sum())}, sum >= 360: {int(above.sum())}")
    assert to_180 > MARGIN and to_360 > MARGIN
    assert (chromatic & ~wrapped).any() and below.any() and above.any()           # all three branches of the mean-hue rule
    if (H, W, seed, near) in RECORDED:
        r180, r360, n_wrapped, n_below, n_above, n_chromatic = RECORDED[(H, W, seed, near)]
        assert abs(to_180 - r180) <= 0.006 * r180 + 5e-5 and abs(to_360 - r360) <= 0.02 * r360
        assert int(chromatic.sum()) == n_chromatic
        if n_wrapped is not None:
            assert (int(wrapped.sum()), int(below.sum()), int(above.sum())) == (n_wrapped, n_below, n_above)


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
    need, two = C.c_int64(0), C.c_int64(0)
    assert lib.hdiff_color_diff_workspace(1, 256, 256, C.byref(need)) == 0
    assert 8 * 65536 + 6 * 2048 * 4 <= need.value <= 8 * 65536 + 65536          # the plane and six histograms; selects, flags, partials
    assert lib.hdiff_color_diff_workspace(2, 256, 256, C.byref(two)) == 0 and two.value > need.value
    assert lib.hdiff_color_diff_workspace(1, 1, 1, C.byref(need)) == 0 and need.value > 0
    assert lib.hdiff_color_diff_workspace(1, 32768, 32768, C.byref(need)) == 0 and need.value > 8 << 30
    one = 8          # any non-null address: validation returns before anything is read or launched

    def refused(rc, word):
        assert rc == -1
        assert word in lib.hdiff_last_error().decode(), lib.hdiff_last_error()

    refused(lib.hdiff_color_diff_workspace(0, 8, 8, C.byref(need)), "N = 0")
    refused(lib.hdiff_color_diff_workspace(65536, 8, 8, C.byref(need)), "N = 65536")
    refused(lib.hdiff_color_diff_workspace(1, 0, 8, C.byref(need)), "at least 1")
    refused(lib.hdiff_color_diff_workspace(1, 8, -1, C.byref(need)), "at least 1")
    refused(lib.hdiff_color_diff_workspace(1, 32768, 32769, C.byref(need)), "too large")
    refused(lib.hdiff_color_diff_workspace(1, 8, 8, None), "null pointer")
    refused(lib.hdiff_color_diff(one, one, 0, 8, 8, one, None, one, None), "N = 0")
    refused(lib.hdiff_color_diff(one, one, 1, 8, 0, one, None, one, None), "at least 1")
    refused(lib.hdiff_color_diff(one, one, 1, -8, 8, one, None, one, None), "at least 1")
    refused(lib.hdiff_color_diff(one, one, 1, 32769, 32768, one, None, one, None), "too large")
    for args in ((None, one, one, one), (one, None, one, one), (one, one, None, one), (one, one, one, None)):
        pred, target, out, scratch = args
        refused(lib.hdiff_color_diff(pred, target, 1, 8, 8, out, one, scratch, None), "null pointer")      # the map alone may be null
    for n in (0, -1, (1 << 30) + 1):
        refused(lib.hdiff_ciede2000_lab(one, one, n, one, None), "n = ")
    for args in ((None, one, one), (one, None, one), (one, one, None)):
        refused(lib.hdiff_ciede2000_lab(args[0], args[1], 4, args[2], None), "null pointer")


def test_python_argument_checks():
    img = torch.rand(2, 3, 8, 13)
    with pytest.raises(RuntimeError, match="MI355X"):
        Q.color_difference(img, img)
    with pytest.raises(TypeError, match="tensor"):
        Q.color_difference(img.numpy(), img)
    with pytest.raises(RuntimeError, match="MI355X"):
        Q.QualityMeter(color=True).update(img, img)
    lab = torch.zeros(4, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="MI355X"):
        Q.ciede2000_lab(lab, lab)
    with pytest.raises(TypeError, match="tensor"):
        Q.ciede2000_lab(lab.numpy(), lab)
    assert {"color_difference", "ciede2000_lab"} <= set(Q.__all__)


# ---------------------------------------------------------------------------------------------------------------- meter, res.txt
def test_meter_columns():
    assert Q.COLOR_COLUMNS == ("ciede2000", "ciede2000_p95", "deltae76", "angular")
    model = Q.NIQEModel(np.zeros(36), np.eye(36), patch=16)
    lpips = object.__new__(Q.LPIPS)                                    # the column order needs no weights
    assert Q.QualityMeter().columns == Q.COLUMNS
    assert Q.QualityMeter(color=True).columns == Q.COLUMNS + Q.COLOR_COLUMNS
    assert Q.QualityMeter(uciqe=True, color=True).columns == Q.COLUMNS + Q.UCIQE_COLUMNS + Q.COLOR_COLUMNS
    assert Q.QualityMeter(uciqe=True, lpips=lpips, niqe=model, color=True).columns == \
        Q.COLUMNS + Q.UCIQE_COLUMNS + Q.COLOR_COLUMNS + Q.LPIPS_COLUMNS + Q.NIQE_COLUMNS
    assert Q.QualityMeter(lpips=lpips, color=True).columns == Q.COLUMNS + Q.COLOR_COLUMNS + Q.LPIPS_COLUMNS
    assert Q.QualityMeter(niqe=model, color=True).columns == Q.COLUMNS + Q.COLOR_COLUMNS + Q.NIQE_COLUMNS
    empty = Q.QualityMeter(color=True).compute()
    assert set(empty) == {"n", "per_image"} | set(Q.COLUMNS) | set(Q.COLOR_COLUMNS)
    assert empty["n"] == 0 and empty["per_image"].shape == (0, 10) and all(np.isnan(empty[k]) for k in Q.COLOR_COLUMNS)
    plain = Q.QualityMeter().compute()
    assert set(plain) == {"n", "per_image"} | set(Q.COLUMNS) and plain["per_image"].shape == (0, 6)


class StubMeter:
    """Stands in for the quality meter: evaluate's bookkeeping and res.txt need no device."""

    def __init__(self):
        self.n = 0

    def update(self, pred01, target01):
        self.n += int(pred01.shape[0])

    def compute(self):
        res = {k: float(i) for i, k in enumerate(Q.COLUMNS + Q.UCIQE_COLUMNS + Q.COLOR_COLUMNS + Q.LPIPS_COLUMNS + Q.NIQE_COLUMNS)}
        res.update(n=self.n, niqe_undefined=0)
        return res


def res_keys(path):
    return [ln.split(":")[0] + ":" for ln in open(path).read().split("\n") if ln]


def test_res_txt_lines_on_a_stub_sampler(tmp_path):
    assert EV.RES_KEYS_COLOR == (("ciede2000_orgin_avg:", "ciede2000"), ("ciede2000_p95_orgin_avg:", "ciede2000_p95"),
                                 ("deltae76_orgin_avg:", "deltae76"), ("angular_orgin_avg:", "angular"))
    assert "RES_KEYS_COLOR" in EV.__all__
    colour = [k for k, _ in EV.RES_KEYS_COLOR]
    model = Q.NIQEModel(np.zeros(36), np.eye(36), patch=16)
    batches = [(torch.zeros(2, 3, 32, 32), torch.zeros(2, 3, 32, 32))]
    sampler = lambda inp, **kw: inp / 127.5 - 1                          # noqa: E731
    lpips = object.__new__(Q.LPIPS)
    base = [k for k, _ in EV.RES_KEYS]
    EV.evaluate(sampler, batches, ddim_step=2, save_dir=str(tmp_path / "a"), meter=StubMeter(), color=True)
    assert res_keys(str(tmp_path / "a" / "res.txt")) == base + colour
    EV.evaluate(sampler, batches, ddim_step=2, save_dir=str(tmp_path / "b"), meter=StubMeter(), uciqe=True, lpips=lpips, niqe=model,
                color=True)
    assert res_keys(str(tmp_path / "b" / "res.txt")) == [k for k, _ in EV.RES_KEYS_UCIQE] + ["lpips_orgin_avg:", "niqe_orgin_avg:"] + colour
    result = EV.evaluate(sampler, batches, ddim_step=2, save_dir=str(tmp_path / "c"), meter=StubMeter())
    text = open(str(tmp_path / "c" / "res.txt")).read()
    assert text == "".join("\n" + key + str(result[k]) for key, k in EV.RES_KEYS)      # without color=: the file of before, byte for byte


def test_sample_lines_carry_the_colour_scores():
    names = Q.COLUMNS + Q.COLOR_COLUMNS
    result = {k: 1.0 for k in names}
    result.update(samples=2, uncertainty=0.5, sample_avg={k: 2.0 for k in names}, sample_std={k: 3.0 for k in names})
    flat, keys = EV.sample_res_lines(result, EV.RES_KEYS + EV.RES_KEYS_COLOR)
    tail = [k for k, _ in keys][len(EV.RES_KEYS) + 4:]
    want = ["samples:"]
    for _, name in EV.RES_KEYS + EV.RES_KEYS_COLOR:
        want += [f"{name}_sample_avg:", f"{name}_sample_std:"]
    assert tail == want + ["uncertainty_avg:"] and flat["angular_sample_std"] == 3.0
