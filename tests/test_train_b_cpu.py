"""Host-side tests of the second tree's trainer (no GPU): the drop-in import of the reference's training driver, the
constructor's signature against the reference's, no pretrained-network loading, and the new C-ABI symbols."""
import ast
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hdiff_amd  # noqa: E402
from hdiff_amd import _capi  # noqa: E402
from hdiff_amd.diffusion import Diffusion as DB  # noqa: E402

NEW_SYMBOLS = {"hdiff_train_b_loss_workspace", "hdiff_train_b_loss_fwd", "hdiff_train_b_loss_bwd", "hdiff_avgpool_global_bwd",
               "hdiff_resize_nearest_bwd"}


def test_dropin_serves_the_training_driver_import():
    """utils/rotinas.py:17 of the reference, in a fresh interpreter started outside the repository."""
    code = "\n".join([
        f"import sys; sys.path.insert(0, {ROOT!r})",
        "import hdiff_amd; hdiff_amd.install_dropin()",
        "from diffusion.Diffusion import GaussianDiffusionSampler, GaussianDiffusionTrainer",
        "assert GaussianDiffusionTrainer.__module__ == 'hdiff_amd.diffusion.Diffusion'",
    ])
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd="/", timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]


def _reference_trainer_signature():
    from oracle import reference_loader as RL
    path = os.path.join(RL.REFERENCE_ROOT, "diffusion", "Diffusion.py")
    if not os.path.isfile(path):
        pytest.skip("the reference checkout is not available")
    tree = ast.parse(open(path).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "GaussianDiffusionTrainer")
    init = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "__init__")
    fwd = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "forward")
    defaults = [ast.literal_eval(d) for d in init.args.defaults]
    return [a.arg for a in init.args.args], defaults, [a.arg for a in fwd.args.args]


def test_constructor_signature_matches_the_reference():
    names, defaults, fwd = _reference_trainer_signature()
    import inspect
    ours = inspect.signature(DB.GaussianDiffusionTrainer.__init__)
    positional = [p for p in ours.parameters.values() if p.kind == p.POSITIONAL_OR_KEYWORD]
    assert [p.name for p in positional] == names
    assert [p.default for p in positional if p.default is not p.empty] == defaults
    kwonly = {p.name: p.default for p in ours.parameters.values() if p.kind == p.KEYWORD_ONLY}
    assert kwonly == {"dino_loss": None, "msssim_loss": None}
    fsig = inspect.signature(DB.GaussianDiffusionTrainer.forward)
    assert [p.name for p in fsig.parameters.values() if p.kind == p.POSITIONAL_OR_KEYWORD] == fwd


def test_constructor_loads_no_pretrained_network(monkeypatch):
    """The default model-name strings are recorded only: torch.hub is never called and kornia never imported."""
    def boom(*a, **k):
        raise AssertionError("torch.hub must not be used")
    for name in ("load", "load_state_dict_from_url", "list", "help"):
        monkeypatch.setattr(torch.hub, name, boom)

    class NoKornia:
        def find_spec(self, fullname, path=None, target=None):
            if fullname == "kornia" or fullname.startswith("kornia."):
                raise AssertionError("kornia must not be imported")
            return None
    monkeypatch.setattr(sys, "meta_path", [NoKornia()] + sys.meta_path)
    monkeypatch.delitem(sys.modules, "kornia", raising=False)
    model = torch.nn.Linear(1, 1)
    tr = DB.GaussianDiffusionTrainer(model, 1e-4, 0.02, 1000)
    assert tr.perceptual_dino == "dinov2_vits14" and tr.perceptual_vgg == "vgg16"
    assert tr.loss_perceptual_dino is None and tr.ms_ssim_loss is None
    assert tr.sqrt_alphas_bar.dtype == torch.float64 and tuple(tr.sqrt_alphas_bar.shape) == (1000,)
    assert "kornia" not in sys.modules


def test_trainer_refuses_cpu_images():
    tr = DB.GaussianDiffusionTrainer(torch.nn.Linear(1, 1), 1e-4, 0.02, 10)
    img = torch.zeros(1, 3, 8, 8, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="MI355X"):
        tr(img, img, 0)


def test_header_declares_the_new_symbols():
    text = open(os.path.join(ROOT, "include", "hdiff.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(hdiff_[a-z0-9_]+)\s*\(", text))
    assert NEW_SYMBOLS <= declared
    assert NEW_SYMBOLS <= set(_capi.EXPORTED_SYMBOLS)
    lib = hdiff_amd.lib()
    assert lib.hdiff_abi_version() == 6
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert NEW_SYMBOLS <= set(re.findall(r" T (hdiff_[a-z0-9_]+)", out))
