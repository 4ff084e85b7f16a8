"""Host-side tests of the device quality scores (no GPU): the C ABI declares / exports / validates the three entries, the float64-sum
definition the kernels are held to (tests/_uiqm_def.py) agrees with the pinned ``uw_metrics`` functions, the module refuses CPU
tensors, and the evaluation loop aggregates, names files and writes ``res.txt`` (stub sampler, stub meter)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hdiff_amd  # noqa: E402
from hdiff_amd import _capi  # noqa: E402
from hdiff_amd import uw_metrics as U  # noqa: E402
import _uiqm_def as D  # noqa: E402

NEW_SYMBOLS = {"hdiff_quality_workspace", "hdiff_psnr_ssim", "hdiff_uiqm"}


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
    assert lib.hdiff_quality_workspace(8, 256, 256, C.byref(need)) == 0
    assert need.value > 0
    one_image = C.c_int64(0)
    assert lib.hdiff_quality_workspace(1, 256, 256, C.byref(one_image)) == 0
    assert 0 < one_image.value < need.value
    one = 8          # any non-null address: validation returns before anything is read or launched

    def refused(rc, word):
        assert rc == -1
        assert word in lib.hdiff_last_error().decode(), lib.hdiff_last_error()

    refused(lib.hdiff_psnr_ssim(one, one, 1, 6, 32, one, one, None), "at least 7")
    refused(lib.hdiff_psnr_ssim(one, one, 1, 32, 6, one, one, None), "at least 7")
    refused(lib.hdiff_uiqm(one, 1, 7, 32, one, one, None), "at least 8")
    refused(lib.hdiff_uiqm(one, 1, 32, 7, one, one, None), "at least 8")
    refused(lib.hdiff_quality_workspace(1, 6, 32, C.byref(need)), "at least 7")
    refused(lib.hdiff_psnr_ssim(one, one, 0, 32, 32, one, one, None), "N = 0")
    refused(lib.hdiff_uiqm(one, 0, 32, 32, one, one, None), "N = 0")
    refused(lib.hdiff_quality_workspace(0, 32, 32, C.byref(need)), "N = 0")
    refused(lib.hdiff_psnr_ssim(one, one, 1, 32768, 32769, one, one, None), "too large")
    refused(lib.hdiff_uiqm(one, 1, 32769, 32768, one, one, None), "too large")
    refused(lib.hdiff_quality_workspace(1, 40000, 40000, C.byref(need)), "too large")
    refused(lib.hdiff_quality_workspace(1, 32, 32, None), "null pointer")
    for args in ((None, one, one, one), (one, None, one, one), (one, one, None, one), (one, one, one, None)):
        a, b, out, scratch = args
        refused(lib.hdiff_psnr_ssim(a, b, 1, 32, 32, out, scratch, None), "null pointer")
    for args in ((None, one, one), (one, None, one), (one, one, None)):
        a, out, scratch = args
        refused(lib.hdiff_uiqm(a, 1, 32, 32, out, scratch, None), "null pointer")


@pytest.mark.parametrize("size", D.SIZES)
def test_float64_sum_definition_against_the_pinned_functions(size):
    """UISM and UIConM equal; UICM within 1e-7 relative: four times the worst gap measured at these sizes (2.3e-8), which is the
    reference's own fp32 running sum of the kept samples."""
    H, W = size
    zero_blocks = 0
    for kind, img in zip(D.KINDS, D.images(H, W)):
        x = D.scaled(img)
        for c in range(3):
            for axis in (0, 1):
                assert np.array_equal(D.sobel_def(x[:, :, c], axis), ndimage.sobel(x[:, :, c], axis)), (kind, c, axis)
            zero_blocks += int((np.minimum.reduceat(np.minimum.reduceat(x[:, :, c], np.arange(0, H, 8), axis=0),
                                                    np.arange(0, W, 8), axis=1) == 0).sum())
        uicm, uism, uiconm, uiqm = D.uiqm_def(x)
        assert uism == U.uism(x), (kind, uism, U.uism(x))
        assert uiconm == U.uiconm(x, 8), (kind, uiconm, U.uiconm(x, 8))
        ref = U.uicm(x)
        print(f"{H}x{W} {kind}: uicm rel {abs(uicm - ref) / abs(ref):.2e}")
        assert abs(uicm - ref) <= 1e-7 * abs(ref), (kind, uicm, ref)
    assert zero_blocks > 0          # the "zero extremum becomes 1" branch is exercised at every size


def test_ties_image_has_many_samples_at_the_cut_values():
    x = D.scaled(D.image("ties", 40, 71))
    rg = np.sort((x[:, :, 0] - x[:, :, 1]).reshape(-1))
    K = rg.size
    lo, hi = rg[int(np.ceil(0.1 * K)) + 1], rg[K - int(np.floor(0.1 * K)) - 1]
    assert (rg == lo).sum() > 10 and (rg == hi).sum() > 10


def test_constant_channel_gives_nan_on_the_host():
    x = D.scaled(D.image("smooth", 16, 24)).copy()
    x[:, :, 1] = 100.0
    with np.errstate(all="ignore"):
        assert np.isnan(U.uism(x)) and np.isnan(U.getUIQM(x))
        uicm, uism, uiconm, uiqm = D.uiqm_def(x)
    assert np.isnan(uism) and np.isnan(uiqm) and np.isfinite(uicm) and np.isfinite(uiconm)


def test_module_refuses_cpu_tensors():
    from hdiff_amd import quality
    img = torch.rand(2, 3, 16, 16)
    with pytest.raises(RuntimeError, match="MI355X"):
        quality.psnr_ssim(img, img)
    with pytest.raises(RuntimeError, match="MI355X"):
        quality.uiqm(img)
    with pytest.raises(RuntimeError, match="MI355X"):
        quality.QualityMeter().update(img, img)
    with pytest.raises(RuntimeError, match="MI355X"):
        quality.QualityMeter().update(img)
    assert quality.QualityMeter().compute()["n"] == 0


class StubSampler:
    """Returns 2 * input / 255 - 1 (so that (out + 1) / 2 is the input image) and records its keyword arguments."""

    def __init__(self):
        self.calls = []

    def __call__(self, inp, **kw):
        self.calls.append(kw)
        return 2 * inp / 255 - 1


class StubMeter:
    """Scores on the host: psnr := mean |pred - target| * 100 per image, the rest constants times the image index."""

    def __init__(self):
        self.rows = []

    def update(self, pred01, target01=None):
        for p, t in zip(pred01, target01):
            i = len(self.rows)
            self.rows.append([float((p - t).abs().mean()) * 100, 0.5, 1.0 + i, 2.0 + i, 3.0 + i, 4.0 + i])

    def compute(self):
        per = np.asarray(self.rows, dtype=np.float64)
        res = {"n": len(self.rows), "per_image": per}
        for j, k in enumerate(("psnr", "ssim", "uiqm", "uicm", "uism", "uiconm")):
            res[k] = float(per[:, j].sum() / len(per))
        return res


def test_evaluate_aggregates_names_files_and_writes_res_txt(tmp_path):
    from hdiff_amd.diffusion import Evaluate as EV
    g = torch.Generator().manual_seed(3)
    inp = [torch.randint(0, 256, (2, 3, 8, 8), generator=g, dtype=torch.uint8) for _ in range(2)]
    tgt = [torch.randint(0, 256, (2, 3, 8, 8), generator=g, dtype=torch.uint8) for _ in range(2)]
    sampler, meter, collected = StubSampler(), StubMeter(), []
    save_dir = str(tmp_path / "named")
    res = EV.evaluate(sampler, [(inp[0], tgt[0], ["a.png", "b.png"]), (inp[1], tgt[1], ("c.png", "d.png"))], ddim_step=7, tile=16,
                      tile_overlap=2, tile_batch=3, save_dir=save_dir, collect=collected, meter=meter)
    assert sampler.calls == [dict(ddim=True, unconditional_guidance_scale=1, ddim_step=7, tile=16, tile_overlap=2, tile_batch=3)] * 2
    assert res["n"] == 4 and len(collected) == 2 and res["per_image"].shape == (4, 6)
    want = [float((i.float() / 255 - t.float() / 255).abs().mean()) * 100 for ib, tb in zip(inp, tgt) for i, t in zip(ib, tb)]
    assert np.allclose(res["per_image"][:, 0], want, rtol=1e-5)          # the target is scaled by 1 / 255, not clipped to a binary image
    assert res["uiqm"] == 2.5 and res["uiconm"] == 5.5
    text = open(os.path.join(save_dir, "res.txt")).read()
    lines = [ln for ln in text.split("\n") if ln]
    assert [ln.split(":")[0] + ":" for ln in lines] == ["psnr_orgin_avg:", "ssim_orgin_avg:", "uiqm_orgin_avg:", "uism_orgin_avg:",
                                                        "uicm_orgin_avg:", "uiconm_orgin_avg:"]
    parsed = {ln.split(":")[0]: float(ln.split(":")[1]) for ln in lines}
    assert parsed == {"psnr_orgin_avg": res["psnr"], "ssim_orgin_avg": 0.5, "uiqm_orgin_avg": 2.5, "uism_orgin_avg": 4.5,
                      "uicm_orgin_avg": 3.5, "uiconm_orgin_avg": 5.5}
    from PIL import Image
    for name, batch, i in (("a.png", 0, 0), ("b.png", 0, 1), ("c.png", 1, 0), ("d.png", 1, 1)):
        got = np.asarray(Image.open(os.path.join(save_dir, name)))
        assert np.array_equal(got, inp[batch][i].permute(1, 2, 0).numpy())      # uint8, rounded to nearest: the stub's image again
    # without names: the running index; without tile: no tiling keywords; without save_dir: nothing is written
    sampler2 = StubSampler()
    save2 = str(tmp_path / "indexed")
    EV.evaluate(sampler2, [(inp[0], tgt[0]), (inp[1], tgt[1])], ddim_step=5, save_dir=save2, meter=StubMeter())
    assert sampler2.calls == [dict(ddim=True, unconditional_guidance_scale=1, ddim_step=5)] * 2
    assert sorted(os.listdir(save2)) == ["00000.png", "00001.png", "00002.png", "00003.png", "res.txt"]
    before = set(os.listdir(tmp_path))
    EV.evaluate(StubSampler(), [(inp[0], tgt[0])], ddim_step=5, meter=StubMeter())
    assert set(os.listdir(tmp_path)) == before
