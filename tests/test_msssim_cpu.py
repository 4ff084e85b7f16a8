"""Host-side tests of the MS-SSIM + L1 loss (no GPU): the two torch forms of the definition (tests/_msssim_def.py) agree in
float64, the layouts differ, the C ABI declares / exports / validates, and the module refuses CPU tensors without importing kornia."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hdiff_amd  # noqa: E402
from hdiff_amd import _capi  # noqa: E402
import _msssim_def as D  # noqa: E402

NEW_SYMBOLS = {"hdiff_msssim_l1_workspace", "hdiff_msssim_l1_fwd", "hdiff_msssim_l1_bwd"}


def rel(a, b):
    return (a - b).abs().max().item() / b.abs().max().item()


@pytest.mark.parametrize("case", ["image", "odd", "tiny", "uniform"])
def test_dense_and_separable_forms_agree_in_float64(case):
    """<= 1e-12 relative in the loss and in the gradient (measured: 4e-14)."""
    x, y = {"image": lambda: D.image_like_pair(2, 64, 64, 1), "odd": lambda: D.image_like_pair(1, 40, 72, 2),
            "tiny": lambda: D.image_like_pair(2, 7, 5, 3), "uniform": lambda: D.uniform_pair(1, 48, 48, 4)}[case]()
    ld, gd = D.loss_and_grad(D.dense_loss, x, y, torch.float64)
    ls, gs = D.loss_and_grad(D.separable_loss, x, y, torch.float64, layout="kornia")
    assert abs(ld.item() - ls.item()) <= 1e-12 * abs(ld.item()), (ld.item(), ls.item())
    assert rel(gs, gd) <= 1e-12, rel(gs, gd)
    lsum, _ = D.loss_and_grad(D.separable_loss, x, y, torch.float64, layout="kornia", reduction="sum")
    assert abs(lsum.item() - ld.item() * x.shape[0] * x.shape[2] * x.shape[3]) <= 1e-10 * abs(lsum.item())


def test_identical_images_give_zero():
    x, _ = D.image_like_pair(2, 40, 40, 5)
    for fn, kw in ((D.dense_loss, {}), (D.separable_loss, {"layout": "kornia"}), (D.separable_loss, {"layout": "per_channel"})):
        loss, grad = D.loss_and_grad(fn, x, x.clone(), torch.float64, **kw)
        assert loss.item() == 0.0
        assert torch.isfinite(grad).all()


def test_layouts_differ_on_image_like_inputs():
    x, y = D.image_like_pair(2, 64, 64, 1)
    lk, gk = D.loss_and_grad(D.separable_loss, x, y, torch.float64, layout="kornia")
    lp, gp = D.loss_and_grad(D.separable_loss, x, y, torch.float64, layout="per_channel")
    assert abs(lk.item() - lp.item()) > 1e-4 * abs(lp.item())
    assert rel(gk, gp) > 1e-2


def test_pair_table_of_the_kornia_layout():
    """R:(0.5, 0.5, 0.5, 1, 1), G:(1, 2, 2, 2, 4), B:(4, 4, 8, 8, 8); lM = l(B, 8) cubed: seven distinct pairs with multiplicities."""
    from hdiff_amd.autograd import msssim_config
    cfg = msssim_config(layout="kornia")
    assert cfg.pairs == [(0, 0, 3, 0), (0, 1, 2, 0), (1, 1, 1, 0), (1, 2, 3, 0), (1, 3, 1, 0), (2, 3, 2, 0), (2, 4, 3, 3)]
    pairs, l_idx = D.layout_table("kornia")
    want = {}
    for i, p in enumerate(pairs):
        e = want.setdefault(p, [0, 0])
        e[0] += 1
        e[1] += int(i in l_idx)
    assert {(c, s): [m, lp] for c, s, m, lp in cfg.pairs} == want
    cfg = msssim_config(layout="per_channel")
    assert len(cfg.pairs) == 15 and sum(lp for *_, lp in cfg.pairs) == 3 and all(m == 1 for _, _, m, _ in cfg.pairs)
    assert cfg.window == 33 and abs(sum(cfg.weights[:33]) - 1.0) < 1e-6


def test_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "hdiff.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(hdiff_[a-z0-9_]+)\s*\(", text))
    assert NEW_SYMBOLS <= declared
    assert NEW_SYMBOLS <= set(_capi.EXPORTED_SYMBOLS)
    for name in NEW_SYMBOLS:
        assert len(_capi._PROTOS[name][1]) >= 3
    lib = hdiff_amd.lib()
    assert lib.hdiff_abi_version() == 6
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert NEW_SYMBOLS <= set(re.findall(r" T (hdiff_[a-z0-9_]+)", out))


def test_argument_validation_needs_no_gpu():
    from hdiff_amd.autograd import msssim_config
    lib = hdiff_amd.lib()
    cfg = msssim_config()
    sb, wb = C.c_int64(0), C.c_int64(0)
    d = cfg.desc(2, 3, 64, 64)
    assert lib.hdiff_msssim_l1_workspace(C.byref(d), C.byref(sb), C.byref(wb)) == 0
    assert sb.value == 2 * 64 * 64 * 7 * 5 * 4 and wb.value >= 2 * 64 * 64 * 7 * 3 * 4

    def refused(d, word):
        one = 8          # any non-null address: validation returns before anything is read or launched
        for rc in (lib.hdiff_msssim_l1_workspace(C.byref(d), C.byref(sb), C.byref(wb)),
                   lib.hdiff_msssim_l1_fwd(C.byref(d), one, one, one, one, one, None),
                   lib.hdiff_msssim_l1_bwd(C.byref(d), one, one, one, one, one, one, None)):
            assert rc == -1
            assert word in lib.hdiff_last_error().decode(), lib.hdiff_last_error()
    refused(cfg.desc(2, 4, 64, 64), "channels")
    d = cfg.desc(2, 3, 64, 64)
    d.nscales = 6
    refused(d, "scales")
    d = cfg.desc(2, 3, 64, 64)
    d.window = 35
    refused(d, "window")
    d = cfg.desc(2, 3, 64, 64)
    d.weights = None
    refused(d, "weight")
    d = cfg.desc(2, 3, 64, 64)
    assert lib.hdiff_msssim_l1_fwd(C.byref(d), None, None, None, None, None, None) == -1
    assert "null pointer" in lib.hdiff_last_error().decode()
    assert lib.hdiff_msssim_l1_bwd(C.byref(d), None, None, None, None, None, None, None) == -1
    assert "null pointer" in lib.hdiff_last_error().decode()


def test_module_refuses_cpu_tensors_and_unsupported_settings(monkeypatch):
    class NoKornia:
        def find_spec(self, fullname, path=None, target=None):
            if fullname == "kornia" or fullname.startswith("kornia."):
                raise AssertionError("kornia must not be imported")
            return None
    monkeypatch.setattr(sys, "meta_path", [NoKornia()] + sys.meta_path)
    monkeypatch.delitem(sys.modules, "kornia", raising=False)
    from hdiff_amd.Loss.loss import MSSSIMLoss
    m = MSSSIMLoss(id=3)
    assert m.name == "MSSSIMLoss" and m.id == 3 and MSSSIMLoss().id is None and m.layout == "kornia"
    img = torch.zeros(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match="MI355X"):
        m(img, img)
    with pytest.raises(ValueError, match="'mean' or 'sum'"):
        MSSSIMLoss(reduction="none")
    with pytest.raises(ValueError, match="limit of 8"):
        MSSSIMLoss(sigmas=(0.5, 1.0, 2.0, 4.0, 16.0))
    with pytest.raises(ValueError, match="layout"):
        MSSSIMLoss(layout="other")
    assert "kornia" not in sys.modules


def test_install_dropin_is_unchanged():
    """The loss module is passed to the trainer by the caller; the drop-in table does not grow."""
    names = [ref for ref, _ in hdiff_amd._DROPIN_MODULES + hdiff_amd._DROPIN_MODULES_TREE_B]
    assert not any(ref.split(".")[0] == "Loss" for ref in names)
