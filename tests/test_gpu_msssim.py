"""GPU tests of the MS-SSIM + L1 loss (csrc/msssim.hip through autograd.msssim_l1_loss and Loss.loss.MSSSIMLoss) against the
definition of tests/_msssim_def.py evaluated on the CPU.

Gate (the project's convention for the G10 trajectory): with r64 the definition in float64 and r32 the same definition in fp32 by
torch on the CPU (the dense grouped-33x33 form for the kornia layout, the separable form for per_channel, which has no dense
form), the HIP loss error and the HIP gradient's rms and max-abs errors against r64 are each at most 4x r32's, with a floor of
16 fp32 eps relative to |loss|, rms(grad), max|grad| (absolute 16 eps x compensation where the float64 loss is 0).

Measured on an MI355X (ratio = HIP error / max(r32 error, floor / 4), so the gate is ratio <= 4; worst over all cases):
  loss 0.94 (7x5, per_channel), gradient rms 1.78 and gradient max-abs 2.34 (both 7x5, kornia layout: 35 pixels, all border);
  on the image-like 64x64, 40x72 and 256x256 cases every ratio is between 0.00 and 1.03; uniform noise and the saturated
  trainer-like pair stay below 0.6.  x == y gives a loss of exactly 0.  The kornia-layout result is 1400 to 4700 gates away from
  the per_channel values (the sensitivity test asks for 100).
"""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hdiff_amd  # noqa: E402
from hdiff_amd import autograd as AG  # noqa: E402
from hdiff_amd.Loss.loss import MSSSIMLoss  # noqa: E402
from hdiff_amd.diffusion.Diffusion import GaussianDiffusionTrainer  # noqa: E402
import _msssim_def as D  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = float(np.finfo(np.float32).eps)
COMP = 200.0

CASES = {
    "img64": (lambda: D.image_like_pair(2, 64, 64, 11), ("kornia", "per_channel"), "mean"),
    "img40x72": (lambda: D.image_like_pair(2, 40, 72, 12), ("kornia", "per_channel"), "mean"),
    "small16": (lambda: D.image_like_pair(1, 16, 16, 13), ("kornia", "per_channel"), "mean"),
    "small7x5": (lambda: D.image_like_pair(2, 7, 5, 14), ("kornia", "per_channel"), "mean"),
    "uniform48": (lambda: D.uniform_pair(1, 48, 48, 15), ("kornia", "per_channel"), "mean"),
    "trainer_like": (lambda: D.trainer_like_pair(2, 32, 32, 16), ("kornia", "per_channel"), "mean"),
    "img256": (lambda: D.image_like_pair(2, 256, 256, 17), ("kornia",), "mean"),
    "sum40": (lambda: D.image_like_pair(1, 40, 40, 18), ("kornia", "per_channel"), "sum"),
}
IDS = [f"{name}-{lay}" for name, (_, lays, _) in CASES.items() for lay in lays]


def rms(a):
    return float(a.double().pow(2).mean().sqrt())


def references(x, y, layout, reduction, upstream=1.0):
    """-> (loss64, grad64, loss32, grad32) on the CPU."""
    l64, g64 = D.loss_and_grad(D.separable_loss, x, y, torch.float64, upstream, layout=layout, reduction=reduction)
    if layout == "kornia":
        l32, g32 = D.loss_and_grad(D.dense_loss, x, y, torch.float32, upstream, reduction=reduction)
    else:
        l32, g32 = D.loss_and_grad(D.separable_loss, x, y, torch.float32, upstream, layout=layout, reduction=reduction)
    return l64, g64, l32, g32


def hip(x, y, layout, reduction, upstream=1.0):
    xg = x.to(DEV).requires_grad_(True)
    loss = AG.msssim_l1_loss(xg, y.to(DEV), layout=layout, reduction=reduction)
    (loss * upstream).backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), xg.grad.detach().cpu()


def gates(l64, g64, l32, g32):
    """The three allowed errors: (loss, gradient rms, gradient max-abs)."""
    lf = 16 * EPS * abs(float(l64)) if float(l64) != 0.0 else 16 * EPS * COMP
    g64d = g64.double()
    return (max(4 * abs(float(l32) - float(l64)), lf),
            max(4 * rms(g32.double() - g64d), 16 * EPS * rms(g64d)),
            max(4 * float((g32.double() - g64d).abs().max()), 16 * EPS * float(g64d.abs().max())))


def errors(lh, gh, l64, g64):
    d = gh.double() - g64.double()
    return abs(float(lh) - float(l64)), rms(d), float(d.abs().max())


def check(tag, lh, gh, l64, g64, l32, g32):
    assert torch.isfinite(gh).all() and np.isfinite(float(lh))
    e, g = errors(lh, gh, l64, g64), gates(l64, g64, l32, g32)
    ratios = [4 * a / b for a, b in zip(e, g)]
    print(f"{tag}: loss {float(l64):.9g}  err/gate-unit  loss {ratios[0]:.2f}  grad rms {ratios[1]:.2f}  grad max {ratios[2]:.2f}"
          f"   (hip err {e[0]:.2e} {e[1]:.2e} {e[2]:.2e}; gate {g[0]:.2e} {g[1]:.2e} {g[2]:.2e})")
    for name, a, b in zip(("loss", "grad rms", "grad max-abs"), e, g):
        assert a <= b, (tag, name, a, b)
    return e, g


@pytest.mark.parametrize("case", IDS)
def test_forward_and_gradient_against_float64(case):
    name, layout = case.rsplit("-", 1)
    build, _, reduction = CASES[name]
    x, y = build()
    lh, gh = hip(x, y, layout, reduction)
    check(case, lh, gh, *references(x, y, layout, reduction))


def test_identical_images_give_zero_and_a_finite_gradient():
    x, _ = D.image_like_pair(2, 40, 40, 19)
    for layout in ("kornia", "per_channel"):
        lh, gh = hip(x, x.clone(), layout, "mean")
        print(f"x == y [{layout}]: loss {float(lh):.3e}, max |grad| {float(gh.abs().max()):.3e}")
        assert abs(float(lh)) <= 16 * EPS * COMP
        assert torch.isfinite(gh).all()


@pytest.mark.parametrize("name", ["img64", "img40x72"])
def test_a_wrong_pair_table_or_a_shifted_target_is_seen(name):
    """The kornia-layout HIP result is further from the float64 per_channel values than 100x its gates, and a target moved by one
    pixel changes the loss by more than the gate."""
    x, y = CASES[name][0]()
    lh, gh = hip(x, y, "kornia", "mean")
    _, g = check(name, lh, gh, *references(x, y, "kornia", "mean"))
    lp, gp = D.loss_and_grad(D.separable_loss, x, y, torch.float64, layout="per_channel")
    e = errors(lh, gh, lp, gp)
    print(f"{name}: distance to per_channel / gate: loss {e[0] / g[0]:.0f}  grad rms {e[1] / g[1]:.0f}  grad max {e[2] / g[2]:.0f}")
    for a, b in zip(e, g):
        assert a > 100 * b, (a, b)
    ls, _ = hip(x, torch.roll(y, 1, dims=3), "kornia", "mean")
    assert abs(float(ls) - float(lh)) > 100 * g[0], (float(ls), float(lh))


def test_bitwise_repeatable():
    x, y = D.image_like_pair(2, 40, 72, 20)
    for layout in ("kornia", "per_channel"):
        a, b = hip(x, y, layout, "mean"), hip(x, y, layout, "mean")
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_upstream_gradient_scales_the_gradient():
    """(0.0045 * loss).backward(), as the trainer weighs the term."""
    x, y = D.image_like_pair(2, 40, 72, 21)
    for layout in ("kornia", "per_channel"):
        lh, gh = hip(x, y, layout, "mean", upstream=0.0045)
        check(f"upstream-{layout}", lh, gh, *references(x, y, layout, "mean", upstream=0.0045))
        _, g1 = hip(x, y, layout, "mean")
        assert rms(gh.double() - 0.0045 * g1.double()) <= 16 * EPS * rms(gh)


def test_refusals_on_the_gpu():
    x, y = (t.to(DEV) for t in D.image_like_pair(1, 16, 16, 22))
    with pytest.raises(RuntimeError, match="only the prediction"):
        AG.msssim_l1_loss(x, y.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="3 channels"):
        AG.msssim_l1_loss(x[:, :2].contiguous(), y[:, :2].contiguous())
    with pytest.raises(RuntimeError, match="fp32"):
        AG.msssim_l1_loss(x.double(), y.double())


# ----------------------------------------------------------------------------------------------------------------------
# trainer level
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(params=["f32", "bf16x3"])
def mode(request):
    before = hdiff_amd.get_contraction_mode()
    hdiff_amd.set_contraction_mode(request.param)
    try:
        yield request.param
    finally:
        hdiff_amd.set_contraction_mode(before)


def dino_standin(y0, gt):
    return (y0 * gt).mean() * 40.0


def composite(y0, gt):
    return D.dense_loss(y0, gt)


def run_trainer(msssim, d, cz):
    from _tree_b_small import load_small_dyn_unet
    _, _, m, _ = load_small_dyn_unet()
    m = m.to(DEV).train()
    b1, bT = (float(v) for v in d["beta"])
    tr = GaussianDiffusionTrainer(m, b1, bT, 1000, dino_loss=dino_standin, msssim_loss=msssim).to(DEV)
    gt, inp, t, noise = (torch.from_numpy(np.asarray(d[f"uw/{k}"])).to(DEV) for k in ("gt", "input", "t", "noise"))
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        terms = tr(gt, inp, 0, t=t, noise=noise, context_zero=cz)
    assert not [w for w in caught if issubclass(w.category, RuntimeWarning) and "MS-SSIM" in str(w.message)]
    terms[0].mean().backward()
    torch.cuda.synchronize()
    return [v.detach().cpu() for v in terms], {n: (None if p.grad is None else p.grad.detach().cpu()) for n, p in m.named_parameters()}


@pytest.mark.parametrize("cz", [True, False])
def test_trainer_with_the_native_loss_matches_the_torch_composite(mode, cz):
    """Five terms and every parameter gradient within 1e-3 relative (floor: 1e-3 of the largest gradient), the bounds of
    tests/test_gpu_train_b.py::check_grads.  With the reference's own y_0_pred (its stray / 255) PIcs underflows and only the L1
    part carries gradient: this test covers the wiring, the op-level tests above the SSIM gradient."""
    d = np.load(os.path.join(ROOT, "tests", "golden", "dyn_trainer_small.npz"))
    th, gh = run_trainer(MSSSIMLoss(), d, cz)
    tc, gc = run_trainer(composite, d, cz)
    assert float(th[3].abs().max()) > 0
    for nm, a, b in zip(("loss", "mse_loss", "perceptual_dino", "msssim", "col_loss"), th, tc):
        assert tuple(a.shape) == tuple(b.shape)
        err = float((a - b).abs().max()) / (float(b.abs().max()) + 1e-12)
        assert err < 1e-3, (nm, err)
    largest = max(float(g.abs().max()) for g in gc.values() if g is not None)
    worst = 0.0
    for n, g in gc.items():
        assert (g is None) == (gh[n] is None), n
        if g is None:
            continue
        err = float((gh[n] - g).abs().max()) / max(float(g.abs().max()), 1e-3 * largest)
        worst = max(worst, err)
        assert err < 1e-3, (n, err)
    print(f"trainer [{mode}, context_zero={cz}]: msssim {float(th[3].mean()):.6g} vs {float(tc[3].mean()):.6g}, worst gradient "
          f"error {worst:.2e}")
