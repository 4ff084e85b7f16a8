"""Host-side tests of the device UCIQE (no GPU): the float64 definition the kernels are held to (tests/_uciqe_def.py) agrees with
``uw_metrics.nmetrics``, its colour conversion is anchored to the published CIE values of the sRGB primaries, the C ABI declares /
exports / validates the two entries, and the module refuses CPU tensors."""
import ctypes as C
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hdiff_amd  # noqa: E402
from hdiff_amd import _capi  # noqa: E402
from hdiff_amd import uw_metrics as U  # noqa: E402
import _uciqe_def as UD  # noqa: E402
import _uiqm_def as D  # noqa: E402

NEW_SYMBOLS = {"hdiff_uciqe_workspace", "hdiff_uciqe"}
HOST_GATE = 1e-11
SIZES = tuple(D.SIZES) + ((8, 13), (72, 120))


def rel(a, b):
    return 0.0 if a == b else abs(a - b) / abs(b)


def host_parts(hwc01: np.ndarray, scale: float):
    """(sc, conl, us) by numpy's own reductions on ``uw_metrics._srgb_to_lab``: the three terms ``nmetrics`` combines."""
    lab = U._srgb_to_lab(np.clip(hwc01, 0, 1).astype(np.float64) * scale)
    lum, chroma = lab[:, :, 0], np.sqrt(lab[:, :, 1] ** 2 + lab[:, :, 2] ** 2)
    top = int(np.round(0.01 * lum.size))
    sl = np.sort(lum, axis=None)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")                                # top == 0: numpy's "Mean of empty slice"
        satur =np.where((chroma == 0) | (lum == 0), 0.0, chroma / lum)
        return (float(np.sqrt(np.mean((chroma - chroma.mean()) ** 2))), float(np.mean(sl[::-1][:top]) - np.mean(sl[:top])),
                float(satur.mean()))


@pytest.mark.parametrize("scale", [1.0, 255.0])
@pytest.mark.parametrize("size", SIZES)
def test_definition_against_the_host_function(size, scale):
    """1e-11 relative: both sides work in double; what differs is the order of the sums (numpy's pairwise reductions and a BLAS
    product against left-to-right loops), at most H W 2^-53 = 1e-12 at the largest size."""
    H, W = size
    for kind, img in zip(D.KINDS, D.images(H, W)):
        want = U.nmetrics(np.clip(img, 0, 1).astype(np.float64) * scale)[1]
        sc, conl, us, got = UD.uciqe_def(np.ascontiguousarray(img.transpose(2, 0, 1)), scale)
        parts = host_parts(img, scale)
        gaps = [rel(got, want)] + [rel(a, b) for a, b in zip((sc, conl, us), parts)]
        print(f"{H}x{W} {kind} scale {scale:g}: uciqe {got!r} host {want!r}  rel (uciqe, sc, conl, us) {[f'{g:.1e}' for g in gaps]}")
        assert np.isfinite(want) and np.isfinite([sc, conl, us, got]).all()
        assert (10 < want < 50) if scale == 1.0 else (1000 < want < 5000), want      # tens on the colour range, thousands at 255
        assert max(gaps) <= HOST_GATE, (kind, gaps)


def test_fewer_than_fifty_pixels_have_no_tails():
    img = D.image("smooth", 7, 7)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")                                # numpy: "Mean of empty slice"
        assert np.isnan(U.nmetrics(img.astype(np.float64))[1])
    sc, conl, us, uciqe = UD.uciqe_def(np.ascontiguousarray(img.transpose(2, 0, 1)))
    assert np.isnan(conl) and np.isnan(uciqe) and np.isfinite(sc) and np.isfinite(us)
    want = host_parts(img, 1.0)
    assert rel(sc, want[0]) <= HOST_GATE and rel(us, want[2]) <= HOST_GATE
    assert UD.top_count(7, 7) == 0 and UD.top_count(8, 13) == 1 and UD.top_count(10, 25) == 2      # 2.5 rounds to even
    assert all(UD.top_count(h, w) == int(np.round(0.01 * h * w)) for h in range(1, 40) for w in range(1, 40))


PRIMARIES = (((1.0, 0.0, 0.0), (53.24, 80.09, 67.20)), ((0.0, 1.0, 0.0), (87.73, -86.18, 83.18)),
             ((0.0, 0.0, 1.0), (32.30, 79.19, -107.86)))


def test_colour_conversion_is_anchored_to_the_published_values():
    """CIE L*a*b* (D65) of the sRGB primaries, within 0.02; white is L = 100, black exactly (0, 0, 0): for the host function and for
    the definition's own conversion."""
    def host(rgb):
        return tuple(float(v) for v in U._srgb_to_lab(np.asarray(rgb, dtype=np.float64).reshape(1, 1, 3))[0, 0])

    def definition(rgb):
        return tuple(float(p[0, 0]) for p in UD.lab_def(np.asarray(rgb, dtype=np.float64).reshape(3, 1, 1)))

    for convert in (host, definition):
        for rgb, want in PRIMARIES:
            got = convert(rgb)
            print(convert.__name__, rgb, got)
            assert max(abs(g - w) for g, w in zip(got, want)) <= 0.02, (convert.__name__, rgb, got)
        white = convert((1.0, 1.0, 1.0))
        assert abs(white[0] - 100.0) <= 0.02 and abs(white[1]) <= 0.02 and abs(white[2]) <= 0.02, white
        assert convert((0.0, 0.0, 0.0)) == (0.0, 0.0, 0.0)


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
    assert lib.hdiff_uciqe_workspace(8, 256, 256, C.byref(need)) == 0
    assert need.value >= 8 * 256 * 256 * 8              # at least the L plane in double
    one_image = C.c_int64(0)
    assert lib.hdiff_uciqe_workspace(1, 256, 256, C.byref(one_image)) == 0
    assert 0 < one_image.value < need.value
    tiny = C.c_int64(0)
    assert lib.hdiff_uciqe_workspace(1, 1, 1, C.byref(tiny)) == 0 and tiny.value > 0
    quality = C.c_int64(0)                               # the other scores' workspace is what it was
    assert lib.hdiff_quality_workspace(8, 256, 256, C.byref(quality)) == 0 and quality.value < need.value
    one = 8          # any non-null address: validation returns before anything is read or launched

    def refused(rc, word):
        assert rc == -1
        assert word in lib.hdiff_last_error().decode(), lib.hdiff_last_error()

    refused(lib.hdiff_uciqe(one, 0, 32, 32, 1.0, one, one, None), "N = 0")
    refused(lib.hdiff_uciqe(one, 65536, 32, 32, 1.0, one, one, None), "N = 65536")
    refused(lib.hdiff_uciqe_workspace(0, 32, 32, C.byref(need)), "N = 0")
    refused(lib.hdiff_uciqe(one, 1, 0, 32, 1.0, one, one, None), "at least 1")
    refused(lib.hdiff_uciqe(one, 1, 32, 0, 1.0, one, one, None), "at least 1")
    refused(lib.hdiff_uciqe(one, 1, 32, -3, 1.0, one, one, None), "at least 1")
    refused(lib.hdiff_uciqe_workspace(1, 0, 32, C.byref(need)), "at least 1")
    refused(lib.hdiff_uciqe(one, 1, 32769, 32768, 1.0, one, one, None), "too large")
    refused(lib.hdiff_uciqe_workspace(1, 40000, 40000, C.byref(need)), "too large")
    refused(lib.hdiff_uciqe_workspace(1, 32, 32, None), "null pointer")
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        refused(lib.hdiff_uciqe(one, 1, 32, 32, scale, one, one, None), "scale")
    for args in ((None, one, one), (one, None, one), (one, one, None)):
        a, out, scratch = args
        refused(lib.hdiff_uciqe(a, 1, 32, 32, 1.0, out, scratch, None), "null pointer")
    assert lib.hdiff_uciqe_workspace(1, 32768, 32768, C.byref(need)) == 0          # 2^30 pixels are accepted
    assert need.value >= 2 ** 30 * 8


def test_module_refuses_cpu_tensors():
    from hdiff_amd import quality
    img = torch.rand(2, 3, 16, 16)
    with pytest.raises(RuntimeError, match="MI355X"):
        quality.uciqe(img)
    with pytest.raises(RuntimeError, match="MI355X"):
        quality.uciqe(img, scale=255.0)
    with pytest.raises(RuntimeError, match="MI355X"):
        quality.QualityMeter(uciqe=True).update(img, img)
    with pytest.raises(RuntimeError, match="MI355X"):
        quality.QualityMeter(uciqe=True, uciqe_scale=255.0).update(img)
    empty = quality.QualityMeter(uciqe=True).compute()
    assert empty["n"] == 0 and empty["per_image"].shape == (0, 10)
    assert set(empty) == {"n", "per_image"} | set(quality.COLUMNS) | set(quality.UCIQE_COLUMNS)
    assert quality.UCIQE_COLUMNS == ("uciqe", "uciqe_sc", "uciqe_conl", "uciqe_us")
    plain = quality.QualityMeter().compute()
    assert plain["per_image"].shape == (0, 6) and set(plain) == {"n", "per_image"} | set(quality.COLUMNS)


def test_res_keys_are_unchanged_and_the_extended_list_adds_one_line():
    from hdiff_amd.diffusion import Evaluate as EV
    assert EV.RES_KEYS == (("psnr_orgin_avg:", "psnr"), ("ssim_orgin_avg:", "ssim"), ("uiqm_orgin_avg:", "uiqm"),
                           ("uism_orgin_avg:", "uism"), ("uicm_orgin_avg:", "uicm"), ("uiconm_orgin_avg:", "uiconm"))
    keys = [k for k, _ in EV.RES_KEYS_UCIQE]
    assert keys.index("uciqe_orgin_avg:") == keys.index("uiqm_orgin_avg:") + 1
    assert [kv for kv in EV.RES_KEYS_UCIQE if kv[1] != "uciqe"] == list(EV.RES_KEYS)
    assert "inference" in EV.__all__ and callable(EV.inference)
