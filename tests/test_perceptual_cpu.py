"""Host-side tests of the VGG perceptual loss, the Charbonnier loss and LPIPS (no GPU): the class surface against the reference's, the
refusals that look at no device, the state-dict handling, the C ABI's declarations and argument checks, and the two properties of the
float64 fixtures that keep the GPU gradient test honest (tests/_perceptual_def.py holds the recipe)."""
import ast
import ctypes as C
import inspect
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
from hdiff_amd import _capi, perceptual, quality  # noqa: E402
from hdiff_amd.Loss.loss import CharbonnierLoss, MSSSIMLoss, PerceptualLoss_vgg  # noqa: E402
from hdiff_amd.diffusion import Diffusion as DB  # noqa: E402
import _perceptual_def as PD  # noqa: E402

NEW_SYMBOLS = {"hdiff_relu_fwd", "hdiff_relu_bwd", "hdiff_maxpool2_fwd", "hdiff_maxpool2_bwd", "hdiff_l1_mean_workspace",
               "hdiff_l1_mean_fwd", "hdiff_l1_mean_bwd", "hdiff_charbonnier_fwd", "hdiff_charbonnier_bwd",
               "hdiff_lpips_layer_workspace", "hdiff_lpips_layer", "hdiff_scale_input"}


# ------------------------------------------------------------------------------------------------------------ class surface
def _reference_init(cls_name):
    from oracle import reference_loader as RL
    path = os.path.join(RL.REFERENCE_ROOT, "Loss", "loss.py")
    if not os.path.isfile(path):
        pytest.skip("the reference checkout is not available")
    tree = ast.parse(open(path).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls_name)
    init = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "__init__")
    fwd = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "forward")
    layer_indices = None
    for node in ast.walk(init):
        if isinstance(node, ast.Assign) and isinstance(node.value, ast.Dict) and ast.unparse(node.targets[0]) == "self.layer_indices":
            layer_indices = ast.literal_eval(node.value)
    return ([a.arg for a in init.args.args], [ast.literal_eval(d) for d in init.args.defaults], [a.arg for a in fwd.args.args],
            layer_indices)


@pytest.mark.parametrize("cls", [PerceptualLoss_vgg, CharbonnierLoss])
def test_signatures_match_the_reference(cls):
    names, defaults, fwd, layer_indices = _reference_init(cls.__name__)
    ours = inspect.signature(cls.__init__)
    positional = [p for p in ours.parameters.values() if p.kind == p.POSITIONAL_OR_KEYWORD]
    assert [p.name for p in positional] == names
    assert [p.default for p in positional if p.default is not p.empty] == defaults
    kwonly = {p.name: p.default for p in ours.parameters.values() if p.kind == p.KEYWORD_ONLY}
    assert kwonly == ({"weights": None} if cls is PerceptualLoss_vgg else {"reduction": "none"})
    fsig = inspect.signature(cls.forward)
    assert [p.name for p in fsig.parameters.values() if p.kind == p.POSITIONAL_OR_KEYWORD] == fwd
    if cls is PerceptualLoss_vgg:
        with pytest.warns(RuntimeWarning, match="randomly initialised"):
            assert cls(model="vgg11").layer_indices == layer_indices


def test_names_ids_and_layer_indices():
    with pytest.warns(RuntimeWarning, match="randomly initialised") as rec:
        loss = PerceptualLoss_vgg(7, "vgg11")
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1          # one warning per instance
    assert loss.name == "PerceptualLoss_vgg_vgg11" and loss.id == 7
    assert isinstance(loss.perceptual, perceptual.VGGFeatures)
    assert loss.layer_indices["vgg16"] == [3, 8, 15, 22] and loss.layer_indices["vgg19"] == [3, 8, 17, 26, 35]
    assert loss.layer_indices["vgg11"] == [3, 8, 15, 22] and loss.layer_indices["alex"] == [3, 6, 8, 10, 12]
    assert all(not p.requires_grad for p in loss.parameters()) and len(list(loss.parameters())) == 16
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        custom = PerceptualLoss_vgg(model="vgg11", layer_indices=[1, 4])
    assert custom.layer_indices["vgg11"] == [1, 4] and custom.layer_indices["vgg16"] == [3, 8, 15, 22]
    charb = CharbonnierLoss(3)
    assert charb.name == "CharbonnierLoss" and charb.id == 3 and charb.reduction == "none" and CharbonnierLoss().id is None
    assert CharbonnierLoss(reduction="mean").reduction == "mean"
    assert MSSSIMLoss().name == "MSSSIMLoss"                                               # the sibling is where it was


def test_weights_are_loaded_without_a_warning(tmp_path):
    cfg = PD.VGG_CFGS["vgg11"]
    sd = PD.state_dict_of(cfg, PD.make_weights(cfg, 0))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        loss = PerceptualLoss_vgg(model="vgg11", weights=sd)
        path = os.path.join(tmp_path, "vgg11.pt")
        torch.save({"features." + k: v for k, v in sd.items()}, path)
        from_file = PerceptualLoss_vgg(model="vgg11", weights=path)
    for k, v in sd.items():
        assert torch.equal(loss.perceptual.state_dict()[k], v) and torch.equal(from_file.perceptual.state_dict()[k], v)


def test_refusals_look_at_no_device():
    for model in ("vgg11_bn", "vgg13_bn", "vgg16_bn", "vgg19_bn", "squeeze", "alex"):
        with pytest.raises(ValueError, match="not provided"):
            PerceptualLoss_vgg(model=model)
    with pytest.raises(ValueError, match="Unsupported perceptual model type. Choose from"):
        PerceptualLoss_vgg(model="resnet")
    with pytest.raises(ValueError, match="reduction"):
        CharbonnierLoss(reduction="median")
    with pytest.raises(ValueError):
        perceptual.VGGFeatures("vgg16_bn")
    with pytest.raises(ValueError):
        perceptual.VGGFeatures(cfg=["M", 8])
    x = torch.zeros(1, 3, 16, 16)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loss = PerceptualLoss_vgg(model="vgg11")
    with pytest.raises(RuntimeError, match="MI355X"):
        loss(x, x)
    with pytest.raises(RuntimeError, match="MI355X"):
        CharbonnierLoss()(x, x)
    with pytest.raises(RuntimeError, match="MI355X"):
        perceptual.VGGFeatures(cfg=[8])(x, [1])
    with pytest.raises(RuntimeError, match="MI355X"):
        perceptual.l1_mean(x, x)
    with pytest.raises(RuntimeError, match="MI355X"):
        perceptual.max_pool2(x)


def test_vgg_layer_lists_and_parameter_names():
    assert perceptual.VGG_CFGS == PD.VGG_CFGS and set(perceptual.VGG_CFGS) == {"vgg11", "vgg13", "vgg16", "vgg19"}
    assert [sum(1 for v in perceptual.VGG_CFGS[m] if v != "M") for m in ("vgg11", "vgg13", "vgg16", "vgg19")] == [8, 10, 13, 16]
    v16 = perceptual.VGGFeatures("vgg16")
    assert v16.conv_indices() == [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28]          # torchvision's vgg16.features
    assert list(v16.state_dict())[:4] == ["0.weight", "0.bias", "2.weight", "2.bias"]
    assert tuple(v16.state_dict()["28.weight"].shape) == (512, 512, 3, 3) and len(v16.layers) == 31
    assert all(not p.requires_grad for p in v16.parameters()) and not v16.training
    assert float(v16.state_dict()["0.bias"].abs().max()) == 0.0
    std = float(v16.state_dict()["10.weight"].std())
    assert abs(std / np.sqrt(2.0 / (256 * 9)) - 1) < 0.02                                   # fan-out Kaiming, ReLU gain
    small = perceptual.VGGFeatures(cfg=[8, 8, "M", 16])
    assert list(small.state_dict()) == ["0.weight", "0.bias", "2.weight", "2.bias", "5.weight", "5.bias"]
    assert tuple(small.state_dict()["5.weight"].shape) == (16, 8, 3, 3)


def test_load_torchvision_key_handling():
    cfg = [8, 8, "M", 16]
    sd = PD.state_dict_of(cfg, PD.make_weights(cfg, 1))
    m = perceptual.VGGFeatures(cfg=cfg)
    assert m.load_torchvision(sd) is m
    assert all(torch.equal(m.state_dict()[k], v) for k, v in sd.items())
    prefixed = {"features." + k: v + 1 for k, v in sd.items()}
    prefixed["classifier.0.weight"] = torch.zeros(4, 4)                                     # ignored
    prefixed["classifier.0.bias"] = torch.zeros(4)
    m.load_torchvision(prefixed)
    assert all(torch.equal(m.state_dict()[k], v + 1) for k, v in sd.items())
    assert all(not p.requires_grad for p in m.parameters())
    missing = {k: v for k, v in sd.items() if k != "5.bias"}
    with pytest.raises(RuntimeError, match="missing keys.*5.bias"):
        m.load_torchvision(missing)
    wrong = dict(sd)
    wrong["2.weight"] = torch.zeros(8, 4, 3, 3)
    with pytest.raises(RuntimeError, match="2.weight.*shape"):
        m.load_torchvision(wrong)
    with pytest.raises(RuntimeError, match="unexpected key"):
        m.load_torchvision({**sd, "7.weight": torch.zeros(1)})
    assert all(torch.equal(m.state_dict()[k], v + 1) for k, v in sd.items())               # a refused dict changed nothing


def test_extra_losses_validation():
    model = torch.nn.Linear(1, 1)

    def make(extra):
        return DB.GaussianDiffusionTrainer(model, 1e-4, 0.02, 10, extra_losses=extra)

    assert make(None).extra_losses == () and make([]).extra_losses == () and make(None).extra_terms == {}
    charb = CharbonnierLoss()
    tr = make([("charb", 0.5, charb), ("fn", 2, lambda a, b: (a - b).abs().mean())])
    assert [(n, w) for n, w, _ in tr.extra_losses] == [("charb", 0.5), ("fn", 2.0)] and tr.extra_losses[0][2] is charb
    assert charb in list(tr.modules())                                                       # travels with .to(device)
    assert not any(k.startswith("extra") for k in tr.state_dict())
    for bad, err in ((("a", 1.0, charb), ValueError), ([("a", 1.0)], ValueError), ([("", 1.0, charb)], ValueError),
                     ([(3, 1.0, charb)], ValueError), ([("a", "1", charb)], ValueError), ([("a", float("nan"), charb)], ValueError),
                     ([("a", True, charb)], ValueError), ([("a", 1.0, charb), ("a", 1.0, charb)], ValueError),
                     ([("a", 1.0, 3)], TypeError), ("vgg", TypeError), (5, TypeError)):
        with pytest.raises(err):
            make(bad)
    with pytest.raises(TypeError, match="unexpected keyword argument 'extra_loss'"):
        DB.GaussianDiffusionTrainer(model, 1e-4, 0.02, 10, extra_loss=None)


def test_lpips_construction_and_meter_columns():
    cfg = PD.VGG_CFGS["vgg16"]
    sd = PD.state_dict_of(cfg, PD.make_weights(cfg, 0))
    lin = PD.make_lin(0)
    metric = quality.LPIPS(sd, lin)
    assert metric.TAPS == (3, 8, 15, 22, 29) and [int(w.numel()) for w in metric.lin] == [64, 128, 256, 512, 512]
    assert torch.equal(metric.lin[2], lin[2].float().reshape(-1))
    by_key = quality.LPIPS(perceptual.VGGFeatures("vgg16").load_torchvision(sd), {f"lin{k}.model.1.weight": w for k, w in enumerate(lin)})
    assert all(torch.equal(a, b) for a, b in zip(by_key.lin, metric.lin))
    with pytest.raises(ValueError, match="lin3"):
        quality.LPIPS(metric.vgg, lin[:3] + [lin[2]] + lin[4:])
    with pytest.raises(ValueError, match="five"):
        quality.LPIPS(metric.vgg, lin[:4])
    with pytest.raises(ValueError, match="lack"):
        quality.LPIPS(metric.vgg, {"lin0.model.1.weight": lin[0]})
    with pytest.raises(ValueError, match="vgg16"):
        quality.LPIPS(perceptual.VGGFeatures("vgg11"), lin)
    img = torch.rand(1, 3, 16, 16)
    with pytest.raises(RuntimeError, match="MI355X"):
        metric.metric(img, img)
    assert quality.LPIPS_COLUMNS == ("lpips",)
    assert quality.QualityMeter(lpips=metric).columns == quality.COLUMNS + ("lpips",)
    both = quality.QualityMeter(uciqe=True, lpips=metric)
    assert both.columns == quality.COLUMNS + quality.UCIQE_COLUMNS + ("lpips",)
    empty = both.compute()
    assert empty["per_image"].shape == (0, 11) and np.isnan(empty["lpips"])
    assert quality.QualityMeter().columns == quality.COLUMNS and quality.QualityMeter(uciqe=True).compute()["per_image"].shape == (0, 10)
    with pytest.raises(TypeError):
        quality.QualityMeter(lpips=lambda a, b: a)
    from hdiff_amd.diffusion import Evaluate as EV
    assert EV.RES_KEY_LPIPS == ("lpips_orgin_avg:", "lpips") and "lpips" in inspect.signature(EV.evaluate).parameters


# ------------------------------------------------------------------------------------------------------------------ the C ABI
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
    one = 8          # any non-null address: validation returns before anything is read or launched
    two = 16
    f1 = C.c_float(1.0)

    def refused(rc, word):
        assert rc == -1
        assert word in lib.hdiff_last_error().decode(), lib.hdiff_last_error()

    for n in (0, -5, 2 ** 40 + 1):
        refused(lib.hdiff_relu_fwd(one, one, n, None), "n = ")
        refused(lib.hdiff_relu_bwd(one, one, two, n, None), "n = ")
        refused(lib.hdiff_l1_mean_fwd(one, one, n, one, one, None), "n = ")
        refused(lib.hdiff_l1_mean_bwd(one, one, one, n, one, None), "n = ")
        refused(lib.hdiff_charbonnier_fwd(one, one, one, n, None), "n = ")
        refused(lib.hdiff_charbonnier_bwd(one, one, one, 0, f1, one, n, None), "n = ")
    need = C.c_int64(0)
    refused(lib.hdiff_l1_mean_workspace(0, C.byref(need)), "n = 0")
    refused(lib.hdiff_l1_mean_workspace(64, None), "null pointer")
    assert lib.hdiff_l1_mean_workspace(1, C.byref(need)) == 0 and need.value >= 8
    small = need.value
    assert lib.hdiff_l1_mean_workspace(2 ** 31 + 5, C.byref(need)) == 0 and small <= need.value <= 256 * 8
    refused(lib.hdiff_relu_fwd(None, one, 4, None), "null pointer")
    refused(lib.hdiff_relu_fwd(one, None, 4, None), "null pointer")
    refused(lib.hdiff_relu_bwd(one, one, None, 4, None), "null pointer")
    refused(lib.hdiff_relu_bwd(one, two, one, 4, None), "alias")
    refused(lib.hdiff_relu_bwd(one, two, two, 4, None), "alias")
    refused(lib.hdiff_l1_mean_fwd(None, one, 4, one, one, None), "null pointer")
    refused(lib.hdiff_l1_mean_fwd(one, one, 4, None, one, None), "null pointer")
    refused(lib.hdiff_l1_mean_fwd(one, one, 4, one, None, None), "null pointer")
    refused(lib.hdiff_l1_mean_bwd(one, one, None, 4, one, None), "null pointer")
    refused(lib.hdiff_charbonnier_fwd(one, None, one, 4, None), "null pointer")
    refused(lib.hdiff_charbonnier_bwd(one, one, None, 0, f1, one, 4, None), "null pointer")
    refused(lib.hdiff_charbonnier_bwd(one, one, one, 2, f1, one, 4, None), "dy_is_scalar")
    for div in (0.5, 0.0, -1.0, float("inf"), float("nan")):
        refused(lib.hdiff_charbonnier_bwd(one, one, one, 1, C.c_float(div), one, 4, None), "divisor")
    for H, W in ((1, 8), (8, 1), (0, 0), (-2, 4)):
        refused(lib.hdiff_maxpool2_fwd(one, one, 1, H, W, None), "at least 2")
        refused(lib.hdiff_maxpool2_bwd(one, one, one, 1, H, W, None), "at least 2")
    refused(lib.hdiff_maxpool2_fwd(one, one, 0, 4, 4, None), "planes")
    refused(lib.hdiff_maxpool2_fwd(one, one, 2 ** 30, 2 ** 10, 2 ** 10, None), "too large")
    refused(lib.hdiff_maxpool2_bwd(one, one, one, 1, 40000, 40000, None), "too large")
    refused(lib.hdiff_maxpool2_fwd(None, one, 1, 4, 4, None), "null pointer")
    refused(lib.hdiff_maxpool2_bwd(one, one, None, 1, 4, 4, None), "null pointer")
    refused(lib.hdiff_lpips_layer(one, one, one, 0, 64, 8, 8, one, one, None), "N = 0")
    refused(lib.hdiff_lpips_layer(one, one, one, 65536, 64, 8, 8, one, one, None), "N = 65536")
    refused(lib.hdiff_lpips_layer(one, one, one, 1, 0, 8, 8, one, one, None), "C = 0")
    refused(lib.hdiff_lpips_layer(one, one, one, 1, 64, 0, 8, one, one, None), "at least 1")
    refused(lib.hdiff_lpips_layer(one, one, one, 1, 64, 40000, 40000, one, one, None), "too large")
    refused(lib.hdiff_lpips_layer(one, one, one, 65535, 65536, 2 ** 15, 2 ** 15, one, one, None), "too large")
    for args in ((None, one, one, one, one), (one, None, one, one, one), (one, one, None, one, one), (one, one, one, None, one),
                 (one, one, one, one, None)):
        f0, f1p, w, out, ws = args
        refused(lib.hdiff_lpips_layer(f0, f1p, w, 1, 64, 8, 8, out, ws, None), "null pointer")
    refused(lib.hdiff_lpips_layer_workspace(1, 64, 8, 8, None), "null pointer")
    refused(lib.hdiff_lpips_layer_workspace(0, 64, 8, 8, C.byref(need)), "N = 0")
    assert lib.hdiff_lpips_layer_workspace(1, 64, 256, 256, C.byref(need)) == 0 and need.value > 0
    per_image = need.value
    assert lib.hdiff_lpips_layer_workspace(8, 64, 256, 256, C.byref(need)) == 0 and need.value >= 8 * per_image - 8 * 256
    assert lib.hdiff_lpips_layer_workspace(1, 512, 1, 1, C.byref(need)) == 0 and need.value > 0
    refused(lib.hdiff_scale_input(one, one, one, f1, f1, one, 0, 3, 8, 8, None), "N = 0")
    refused(lib.hdiff_scale_input(one, one, one, f1, f1, one, 1, 0, 8, 8, None), "C = 0")
    refused(lib.hdiff_scale_input(one, None, one, f1, f1, one, 1, 3, 8, 8, None), "null pointer")
    refused(lib.hdiff_scale_input(one, one, one, f1, f1, None, 1, 3, 8, 8, None), "null pointer")


# ------------------------------------------------------------------------------------------------------- the fixtures' margins
@pytest.fixture(scope="module", params=PD.GRAD_FIXTURES, ids=lambda p: f"{p[0]}x{p[1]}-seed{p[2]}")
def fixture64(request):
    H, W, seed = request.param
    cfg = PD.VGG_CFGS["vgg16"]
    weights = PD.make_weights(cfg, seed)
    x, y = PD.make_images(seed, H, W)
    return cfg, weights, x, y


def test_gradient_fixtures_keep_their_margins(fixture64):
    """A ReLU net's gradient is discontinuous: an fp32 run may flip a mask that float64 does not, and one flip moves the gradient by
    far more than rounding.  So every pre-activation of the x pass, the lead of every pooling window's maximum (unless it is 0) and
    every non-zero tap difference stay DELTA = 2e-5 away from the switch, in float64 -- about 100x an fp32 error at the
    pre-activations' rms of 0.06 to 1.2.  Measured (pre, pool, tap): 8x8 seed 2: 5.7e-5, 3.9e-4, 2.6e-5; 8x8 seed 4: 4.2e-5, 5.3e-5,
    4.9e-5; 9x11 seed 2: 3.1e-5, 9.8e-5, 2.1e-5."""
    cfg, weights, x, y = fixture64
    pre, gap, tap = PD.margins(x, y, weights, cfg)
    print(f"min |pre-activation| {pre:.2e}  min pool gap {gap:.2e}  min tap gap {tap:.2e}")
    assert pre >= PD.DELTA and gap >= PD.DELTA and tap >= PD.DELTA
    # the GPU test evaluates its float64 reference on the fp32-rounded weights and images: the margins hold there too
    r = PD.margins(x.float().double(), y.float().double(), PD.rounded(weights), cfg)
    print("fp32-rounded fixture:", [f"{v:.2e}" for v in r])
    assert min(r) >= PD.DELTA


def test_no_tap_can_hide(fixture64):
    """Each of the four tap terms exceeds 1e-3 of the total in float64 (measured 0.12 / 0.11 / 0.04 / 0.002 of 0.28): an
    implementation that drops or mis-scales one cannot pass the value check."""
    cfg, weights, x, y = fixture64
    terms = [float(t) for t in PD.tap_terms(x, y, weights, cfg)]
    print("tap terms", [f"{t:.4f}" for t in terms], "total", f"{sum(terms):.4f}")
    assert len(terms) == 4 and all(t > 1e-3 * sum(terms) for t in terms)


# ------------------------------------------------------------------------------------------ the fp32 definitions themselves
def test_pooling_definition_rules():
    x = np.array([[[1, 1, 0, 0, 9], [1, 1, 0, 0, 9], [2, 3, -1, -2, 9], [3, 2, -2, -1, 9], [7, 7, 7, 7, 7]]], dtype=np.float32)
    assert PD.pool_fwd(x).tolist() == [[[1, 0], [3, -1]]]
    dy = np.array([[[10, 20], [30, 40]]], dtype=np.float32)
    dx = PD.pool_bwd(x, dy)
    assert dx[0].tolist() == [[10, 0, 20, 0, 0], [0, 0, 0, 0, 0], [0, 30, 40, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]]
    want = torch.nn.functional.max_pool2d(torch.from_numpy(x)[None], 2, 2)[0].numpy()
    assert np.array_equal(PD.pool_fwd(x), want)
    assert PD.l1_bwd([1, 2, 3], [1, 3, 2], 3.0).tolist() == [0.0, -1.0, 1.0]
    assert PD.relu_bwd([0.0, 2.0, 0.0], [5, 6, 7]).tolist() == [0.0, 6.0, 0.0]
