"""GPU checks of the perceptual pieces: csrc/perceptual.hip, hdiff_amd/perceptual.py, Loss.loss.PerceptualLoss_vgg / CharbonnierLoss, the
trainer's ``extra_losses`` and quality.LPIPS with its wiring.  tests/_perceptual_def.py holds the definitions.

Gates.  ReLU, pooling and the L1 backward: bit for bit against the fp32 definitions.  ``l1_mean``: 2 fp32 ulp of the float64 mean (the
terms are non-negative, each within 2^-24 relative, one final rounding).  Charbonnier: 4 * 2^-24 * (1 + |value|) absolute against float64
(four roundings; the ``- 1`` is exact below 2 and one more rounding above).  The loss end to end and LPIPS: the yardstick is torch's own
fp32 evaluation of the same definition on the CPU, measured in the test against float64 on the same fp32-rounded weights and images; the
HIP path gets 4x that (1.5 for the documented error class of the split-operand convs against the exact fp32 kernel, times 2 for a
k-ordered fp32 accumulation against blocked sums, rounded up).  Every test prints its figures before asserting; the values measured on
an MI355X are in profiles/perceptual.txt.

Measured on an MI355X, ratio of the HIP error to the fp32 CPU yardstick (gate 4): loss gradient 1.18 / 1.12 / 1.09 on the three
fixtures, loss value 1.00 / 0.47 / 1.00, the other shapes' values 0.52 to 1.85, LPIPS 0.08 / 0.91 (errors 9.2e-9 and 5.0e-8 against the
1e-5 floor).  The two contraction modes give the same figures at these sizes: below 192 tiles of 32x8 pixels x 64 channels both run the
exact fp32 conv kernel; test_trunk_wide_enough_for_the_split_operand_kernel is the case where they part."""
import ctypes as C
import functools
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
from hdiff_amd import _capi, perceptual as P, quality as Q  # noqa: E402
from hdiff_amd.Loss.loss import CharbonnierLoss, PerceptualLoss_vgg  # noqa: E402
from hdiff_amd.diffusion import Evaluate as EV  # noqa: E402

import _perceptual_def as PD  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
YARD = 4.0


@pytest.fixture(params=["f32", "bf16x3"])
def mode(request):
    before = hdiff_amd.get_contraction_mode()
    hdiff_amd.set_contraction_mode(request.param)
    try:
        yield request.param
    finally:
        hdiff_amd.set_contraction_mode(before)


def bits32(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().copy()


def same_bits(got, want):
    """fp32 device tensor against an fp32 numpy array, bit for bit (so -0 and +0 differ, NaNs compare by payload)."""
    want = np.ascontiguousarray(want, dtype=np.float32)
    return got.shape == want.shape and np.array_equal(bits32(got).reshape(-1), want.view(np.int32).reshape(-1))


def ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


# ---------------------------------------------------------------------------------------------------- 1. bit for bit
def test_relu_forward_and_backward_bit_for_bit():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 5, 33, 31, generator=g)
    x.view(-1)[:9] = torch.tensor([0.0, -0.0, 1e-45, -1e-45, 3.0, -3.0, float("inf"), -float("inf"), float("nan")])
    dy = torch.randn(x.shape, generator=g)
    xd = x.to(DEV).requires_grad_(True)
    y = P.relu(xd)
    y.backward(dy.to(DEV))
    want = PD.relu_fwd(x.numpy())
    assert same_bits(y, want) and same_bits(xd.grad, PD.relu_bwd(want, dy.numpy())) and bool(torch.isnan(y.view(-1)[8]))
    z = x.to(DEV)
    assert P.relu(z, inplace=True).data_ptr() == z.data_ptr() and same_bits(z, want)       # in place: y aliases x


@pytest.mark.parametrize("planes", [(1, 1), (2, 3)], ids=["bc1", "bc6"])
@pytest.mark.parametrize("size", [(2, 2), (5, 7), (8, 8), (9, 11)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_pooling_forward_and_backward_bit_for_bit(size, planes):
    """Values drawn from five levels: most windows hold equal entries, some are all zero; an odd last row / column gets no gradient."""
    H, W = size
    B, Cc = planes
    g = torch.Generator().manual_seed(17 * H + W + B)
    x = torch.randint(-2, 3, (B, Cc, H, W), generator=g).float() * 0.5
    x[0, 0, :2, :2] = 0.0
    noisy = x + (torch.rand(x.shape, generator=g) < 0.3) * torch.randn(x.shape, generator=g)
    dy = torch.randn(B, Cc, H // 2, W // 2, generator=g)
    for inp in (x, noisy):
        xd = inp.to(DEV).requires_grad_(True)
        y = P.max_pool2(xd)
        y.backward(dy.to(DEV))
        flat = inp.numpy().reshape(B * Cc, H, W)
        assert same_bits(y, PD.pool_fwd(flat).reshape(B, Cc, H // 2, W // 2))
        assert same_bits(xd.grad, PD.pool_bwd(flat, dy.numpy().reshape(B * Cc, H // 2, W // 2)).reshape(B, Cc, H, W))
        assert np.array_equal(y.detach().cpu().numpy(), torch.nn.functional.max_pool2d(inp, 2, 2).numpy())
    if H >= 4:                                                # a NaN is the maximum of its window and of no other
        bad = noisy.clone()
        bad[0, 0, 1, 1], bad[0, 0, 2, 3], bad[0, 0, 3, 2] = float("nan"), float("nan"), float("nan")
        y = P.max_pool2(bad.to(DEV))
        assert same_bits(y, PD.pool_fwd(bad.numpy().reshape(B * Cc, H, W)).reshape(B, Cc, H // 2, W // 2))
        assert int(torch.isnan(y).sum()) == 2 and bool(torch.isnan(y[0, 0, 0, 0])) and bool(torch.isnan(y[0, 0, 1, 1]))


def test_l1_backward_bit_for_bit_with_sign_zero():
    g = torch.Generator().manual_seed(5)
    a = torch.randn(3, 7, 5, 11, generator=g)
    b = torch.randn(a.shape, generator=g)
    b.view(-1)[::3] = a.view(-1)[::3]                      # a third of the differences are exactly 0
    ad, bd = a.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    out = P.l1_mean(ad, bd)
    out.backward(torch.tensor(1.7, device=DEV))
    want = PD.l1_bwd(a.numpy(), b.numpy(), np.float32(1.7))
    assert (want == 0).sum() >= a.numel() // 3
    assert same_bits(ad.grad, want) and bd.grad is None and out.dim() == 0


# ---------------------------------------------------------------------------------------------------- 2. the L1 mean
@pytest.mark.parametrize("n", [1, 63, 64, 65, 70001])
def test_l1_mean_forward_within_two_ulp(n):
    g = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g) * 3
    got = float(P.l1_mean(a.to(DEV), b.to(DEV)))
    want = float((a.double() - b.double()).abs().mean())
    print(f"n = {n}: device {got!r}  float64 {want!r}  gap {abs(got - want) / ulp32(want):.2f} ulp")
    assert abs(got - want) <= 2 * ulp32(want)
    again = P.l1_mean(a.to(DEV), b.to(DEV))
    assert float(again) == got                              # repeatable


# ---------------------------------------------------------------------------------------------------- 3. Charbonnier
@pytest.mark.parametrize("shape", [(1, 3, 5, 7), (2, 3, 16, 16)], ids=["1x3x5x7", "2x3x16x16"])
def test_charbonnier_forward_backward_and_reductions(shape):
    g = torch.Generator().manual_seed(sum(shape))
    n = int(np.prod(shape))
    mag = 10 ** (torch.rand(shape, generator=g, dtype=torch.float64) * (np.log10(4) + 4) - 4)         # |d| from 1e-4 to 4
    mag.view(-1)[0], mag.view(-1)[1] = 1e-4, 4.0
    d = mag * (torch.randint(0, 2, shape, generator=g) * 2 - 1)
    a = torch.randn(shape, generator=g)
    b = (a.double() - d).float()
    a64, b64 = a.double(), b.double()
    dy = (torch.rand(shape, generator=g) * 4 - 2)
    want, want_grad = PD.charbonnier_def(a64, b64), PD.charbonnier_grad_def(a64, b64, dy.double())
    assert float((a64 - b64).abs().min()) < 2e-4 and float((a64 - b64).abs().max()) > 3.9

    ad = a.to(DEV).requires_grad_(True)
    bd = b.to(DEV).requires_grad_(True)
    y = CharbonnierLoss()(ad, bd)
    y.backward(dy.to(DEV))
    err = (y.detach().cpu().double() - want).abs() / (4 * U * (1 + want))
    gerr = (ad.grad.cpu().double() - want_grad).abs() / (4 * U * (1 + want_grad.abs()))
    print(f"{shape}: forward {float(err.max()):.3f} of the bound, backward {float(gerr.max()):.3f} of the bound")
    assert y.shape == a.shape and float(err.max()) <= 1.0 and float(gerr.max()) <= 1.0 and bd.grad is None
    zero = CharbonnierLoss()(ad.detach(), ad.detach())
    assert float(zero.abs().max()) == 0.0                                                        # identical inputs: exactly 0

    own = y.detach().cpu().double()                                                              # the device's own map, reduced in double
    for reduction, ref, ref_def, scale in (("mean", own.mean(), want.mean(), 1.0 / n), ("sum", own.sum(), want.sum(), 1.0)):
        ad.grad = None
        r = CharbonnierLoss(reduction=reduction)(ad, bd)
        r.backward()
        got = float(r.detach())
        print(f"{shape} {reduction}: device {got!r}  float64 of the map {float(ref)!r}  gap {abs(got - float(ref)) / ulp32(float(ref)):.2f} ulp")
        assert r.dim() == 0 and abs(got - float(ref)) <= 2 * ulp32(float(ref))
        assert abs(got - float(ref_def)) <= 4 * U * (n if reduction == "sum" else 1) * (1 + float(want.mean())) + 2 * ulp32(float(ref))
        g_ref = PD.charbonnier_grad_def(a64, b64, torch.full(shape, scale, dtype=torch.float64))
        assert float(((ad.grad.cpu().double() - g_ref).abs() / (4 * U * (scale + g_ref.abs()))).max()) <= 1.0


# ---------------------------------------------------------------------------------------------------- 4. the loss end to end
@functools.lru_cache(maxsize=None)
def reference(H, W, seed, B=1, model="vgg16", taps=PD.LOSS_TAPS, grad=True):
    """The fp32-rounded fixture, its float64 value (and gradient) and the fp32 CPU yardstick's errors; computed once, never modified."""
    cfg = PD.VGG_CFGS[model]
    weights = PD.make_weights(cfg, seed)
    x, y = PD.make_images(seed, H, W, B)
    x32, y32, w64 = x.float(), y.float(), PD.rounded(weights)
    if grad:
        v64, g64 = PD.loss_and_grad(x32.double(), y32.double(), w64, cfg, taps)
        v32, g32 = PD.loss_and_grad(x32, y32, w64, cfg, taps, dtype=torch.float32)
        yard_g = float((g32 - g64).norm() / g64.norm())
    else:
        with torch.no_grad():
            v64 = float(PD.loss_def(x32.double(), y32.double(), w64, cfg, taps))
            v32 = float(PD.loss_def(x32, y32, w64, cfg, taps))
        g64, yard_g = None, None
    return dict(cfg=cfg, sd=PD.state_dict_of(cfg, weights), x=x32, y=y32, value=v64, grad=g64, yard_value=abs(v32 - v64) / abs(v64),
                yard_grad=yard_g)


def vgg_loss(model, sd):
    with warnings.catch_warnings():
        warnings.simplefilter("error")                     # weights are given: no warning
        return PerceptualLoss_vgg(model=model, weights=sd).to(DEV)


@pytest.mark.parametrize("fixture", PD.GRAD_FIXTURES, ids=lambda p: f"{p[0]}x{p[1]}-seed{p[2]}")
def test_loss_value_and_input_gradient_against_float64(mode, fixture):
    """Full-width vgg16, taps 3 / 8 / 15 / 22, on fixtures whose float64 pre-activations, pooling leads and tap differences stay 2e-5
    from a switch (tests/test_perceptual_cpu.py): an fp32 run takes the float64 run's branches, so the gradient is comparable."""
    ref = reference(*fixture)
    loss = vgg_loss("vgg16", ref["sd"])
    x = ref["x"].to(DEV).requires_grad_(True)
    y = ref["y"].to(DEV).requires_grad_(True)
    out = loss(x, y)
    out.backward()
    v_err = abs(float(out.detach()) - ref["value"]) / abs(ref["value"])
    g_err = float((x.grad.cpu().double() - ref["grad"]).norm() / ref["grad"].norm())
    print(f"{fixture} [{mode}]: value rel err {v_err:.3e} (fp32 CPU {ref['yard_value']:.3e}, ratio {v_err / ref['yard_value']:.2f})  "
          f"gradient rel L2 err {g_err:.3e} (fp32 CPU {ref['yard_grad']:.3e}, ratio {g_err / ref['yard_grad']:.2f})")
    assert out.dim() == 0 and y.grad is None
    assert all(p.grad is None for p in loss.parameters())
    assert v_err <= YARD * ref["yard_value"], (v_err, ref["yard_value"])
    assert g_err <= YARD * ref["yard_grad"], (g_err, ref["yard_grad"])


# ---------------------------------------------------------------------------------------------------- 5. route-table shapes
@pytest.mark.parametrize("case", [("vgg16", 2, 32, 32), ("vgg16", 1, 24, 44), ("vgg11", 1, 16, 16)], ids=lambda c: f"{c[0]}-{c[1]}x3x{c[2]}x{c[3]}")
def test_loss_value_at_other_shapes(mode, case):
    model, B, H, W = case
    ref = reference(H, W, 0, B, model, PD.LOSS_TAPS, False)
    loss = vgg_loss(model, ref["sd"])
    with torch.no_grad():
        got = float(loss(ref["x"].to(DEV), ref["y"].to(DEV)))
    v_err = abs(got - ref["value"]) / abs(ref["value"])
    print(f"{case} [{mode}]: value rel err {v_err:.3e} (fp32 CPU {ref['yard_value']:.3e}, ratio {v_err / ref['yard_value']:.2f})")
    assert v_err <= YARD * ref["yard_value"]
    if B == 2:                    # a batch of two is the mean of its samples run alone
        with torch.no_grad():
            alone = [float(loss(ref["x"][i:i + 1].to(DEV), ref["y"][i:i + 1].to(DEV))) for i in range(2)]
        gap = abs(got - sum(alone) / 2) / abs(ref["value"])
        print(f"  batch {got!r}  mean of the samples alone {sum(alone) / 2!r}  rel gap {gap:.3e}")
        assert gap <= YARD * ref["yard_value"]


def test_custom_trunk_with_narrow_channels(mode):
    """cfg = [8, 8, "M", 16] at 3x3x6x10: channel counts that are no multiple of 16, taps behind every ReLU and the pooling."""
    cfg, taps = [8, 8, "M", 16], (1, 3, 4, 6)
    weights = PD.make_weights(cfg, 0)
    x, y = (t.float() for t in PD.make_images(0, 6, 10, 3))
    w64 = PD.rounded(weights)
    with torch.no_grad():
        v64 = float(PD.loss_def(x.double(), y.double(), w64, cfg, taps))
        v32 = float(PD.loss_def(x, y, w64, cfg, taps))
    yard = abs(v32 - v64) / v64
    trunk = P.VGGFeatures(cfg=cfg).load_torchvision(PD.state_dict_of(cfg, weights)).to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    fx = trunk(xd, taps)
    with torch.no_grad():
        fy = trunk(y.to(DEV), taps)
    assert [tuple(f.shape) for f in fx] == [(3, 8, 6, 10), (3, 8, 6, 10), (3, 8, 3, 5), (3, 16, 3, 5)]
    out = sum(P.l1_mean(a, b) for a, b in zip(fx, fy))
    out.backward()
    v_err = abs(float(out.detach()) - v64) / v64
    print(f"custom trunk [{mode}]: value rel err {v_err:.3e} (fp32 CPU {yard:.3e}, ratio {v_err / yard:.2f})")
    assert v_err <= YARD * yard and xd.grad is not None and bool(torch.isfinite(xd.grad).all())
    conv_tap = trunk(x.to(DEV), [0, 1])                      # a tap on a conv's own output survives the ReLU behind it
    assert float(conv_tap[0].min()) < 0 and float(conv_tap[1].min()) == 0.0


def test_trunk_wide_enough_for_the_split_operand_kernel():
    """The shapes above are too small for the split-operand 3x3 kernel, which wants 192 tiles of 32x8 pixels x 64 output channels
    (both modes run the exact fp32 kernel there).  3x3x128x128 through cfg = [64, 64, "M", 128] puts the 64 -> 64 conv on it in the
    default mode: the features differ from the f32 mode's in their last bits, and the value holds the same rule in both -- 4x the
    fp32 CPU yardstick, or one fp32 ulp of the value where that is larger (the value is one fp32 number; the yardstick's own error
    can fall below its resolution by chance)."""
    cfg, taps = [64, 64, "M", 128], (1, 3, 4, 6)
    weights = PD.make_weights(cfg, 0)
    x, y = (t.float() for t in PD.make_images(0, 128, 128, 3))
    w64 = PD.rounded(weights)
    with torch.no_grad():
        v64 = float(PD.loss_def(x.double(), y.double(), w64, cfg, taps))
        v32 = float(PD.loss_def(x, y, w64, cfg, taps))
    yard = abs(v32 - v64) / v64
    gate = max(YARD * yard, ulp32(v64) / v64)
    trunk = P.VGGFeatures(cfg=cfg).load_torchvision(PD.state_dict_of(cfg, weights)).to(DEV)
    before = hdiff_amd.get_contraction_mode()
    feats = {}
    try:
        for m in ("f32", "bf16x3"):
            hdiff_amd.set_contraction_mode(m)
            xd = x.to(DEV).requires_grad_(True)
            fx = trunk(xd, taps)
            with torch.no_grad():
                fy = trunk(y.to(DEV), taps)
            out = sum(P.l1_mean(a, b).double() for a, b in zip(fx, fy)).float()
            out.backward()
            feats[m] = fx[1].detach()
            v_err = abs(float(out.detach()) - v64) / v64
            print(f"wide trunk [{m}]: value rel err {v_err:.3e} (fp32 CPU {yard:.3e}, gate {gate:.3e})")
            assert v_err <= gate and bool(torch.isfinite(xd.grad).all()) and float(xd.grad.abs().max()) > 0
    finally:
        hdiff_amd.set_contraction_mode(before)
    gap = float((feats["f32"] - feats["bf16x3"]).abs().max() / feats["f32"].abs().max())
    print(f"wide trunk: max |f32 - bf16x3| of the second conv's features, relative to their maximum: {gap:.3e}")
    assert 0 < gap < 1e-5                                   # another kernel ran, and it is the same conv


# ---------------------------------------------------------------------------------------------------- 6. the trainer
def test_trainer_adds_the_extra_terms():
    from _tree_b_small import load_small_dyn_unet
    from hdiff_amd.diffusion.Diffusion import GaussianDiffusionTrainer
    from tools.gen_golden_train_b import dino_standin, msssim_standin
    d = np.load(os.path.join(ROOT, "tests", "golden", "dyn_trainer_small.npz"))
    b1, bT = (float(v) for v in d["beta"])
    gt, inp, t, noise = (torch.from_numpy(np.asarray(d[f"uw/{k}"])).to(DEV) for k in ("gt", "input", "t", "noise"))
    ref = reference(8, 8, 2)
    vgg = vgg_loss("vgg16", ref["sd"])
    seen = {}

    def recording_msssim(y0, target):
        seen["y0"], seen["gt"] = y0.detach().clone(), target.detach().clone()
        return msssim_standin(y0, target)

    def run(**kw):
        _, _, m, _ = load_small_dyn_unet()
        m = m.to(DEV).train()
        tr = GaussianDiffusionTrainer(m, b1, bT, 1000, dino_loss=dino_standin, msssim_loss=recording_msssim, **kw).to(DEV)
        terms = tr(gt, inp, 0, t=t, noise=noise, context_zero=False)
        terms[0].mean().backward()
        return tr, m, terms

    tr0, m0, base = run()
    tr1, m1, none = run(extra_losses=None)
    assert tr1.extra_terms == {} and len(none) == 5
    for a, b in zip(base, none):
        assert torch.equal(a, b)
    for (na, pa), (nb, pb) in zip(m0.named_parameters(), m1.named_parameters()):
        assert na == nb and ((pa.grad is None and pb.grad is None) or torch.equal(pa.grad, pb.grad)), na

    tr2, m2, terms = run(extra_losses=[("vgg", 1.0, vgg), ("charb", 0.5, CharbonnierLoss())])
    assert len(terms) == 5 and set(tr2.extra_terms) == {"vgg", "charb"}
    for a, b in zip(base[1:], terms[1:]):
        assert torch.equal(a, b)                              # the four named terms are what they were
    with torch.no_grad():
        vgg_term = vgg(seen["y0"], seen["gt"]) * 1.0
        charb_term = CharbonnierLoss()(seen["y0"], seen["gt"]) * 0.5
    want = (base[0].detach() + vgg_term) + charb_term
    gap = float((terms[0].detach() - want).abs().max())
    print(f"loss with extras: max |got - (five terms + vgg + 0.5 charb)| = {gap:.3e}; vgg {float(vgg_term):.4e}, charb max {float(charb_term.max()):.4e}")
    assert terms[0].shape == want.shape and torch.equal(terms[0].detach(), want)
    assert torch.equal(tr2.extra_terms["vgg"], vgg_term) and torch.equal(tr2.extra_terms["charb"], charb_term)
    assert not tr2.extra_terms["vgg"].requires_grad and float(vgg_term) > 0
    changed = [n for (n, pa), (_, pb) in zip(m0.named_parameters(), m2.named_parameters())
               if pa.grad is not None and not torch.equal(pa.grad, pb.grad)]
    assert changed and all(bool(torch.isfinite(p.grad).all()) for p in m2.parameters() if p.grad is not None)
    assert all(p.grad is None for p in vgg.parameters())


# ---------------------------------------------------------------------------------------------------- 7. LPIPS
@functools.lru_cache(maxsize=None)
def lpips_fixture():
    cfg = PD.VGG_CFGS["vgg16"]
    weights = PD.make_weights(cfg, 1)
    lin = PD.make_lin(1)
    metric = Q.LPIPS(PD.state_dict_of(cfg, weights), lin).to(DEV)
    return metric, PD.rounded(weights), [w.float().double() for w in lin]


def lpips_images(N, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(N, 3, H, W, generator=g)
    b = (a + 0.2 * torch.randn(N, 3, H, W, generator=g)).clamp(0, 1)
    return a, b


@pytest.mark.parametrize("shape", [(2, 16, 16), (1, 19, 17)], ids=["2x3x16x16", "1x3x19x17"])
def test_lpips_against_the_float64_definition(mode, shape):
    metric, w64, lin64 = lpips_fixture()
    a, b = lpips_images(*shape, seed=sum(shape))
    with torch.no_grad():
        want = PD.lpips_def(a.double(), b.double(), w64, lin64)
        cpu32 = PD.lpips_def(a, b, w64, lin64).double()
    got = metric.metric(a.to(DEV), b.to(DEV))
    assert got.dtype == torch.float64 and tuple(got.shape) == (shape[0],) and got.is_cuda
    err = ((got.cpu() - want).abs() / want).max().item()
    yard = ((cpu32 - want).abs() / want).max().item()
    print(f"{shape} [{mode}]: lpips {got.cpu().tolist()}  rel err {err:.3e}  fp32 CPU rel err {yard:.3e}")
    assert float(want.min()) > 1e-3 and err <= max(1e-5, YARD * yard)


def bits64(t):
    return t.detach().cpu().contiguous().view(torch.int64).numpy().copy()


def test_lpips_properties():
    metric, _, _ = lpips_fixture()
    a, b = (t.to(DEV) for t in lpips_images(2, 19, 17, 9))
    both = metric.metric(a, b)
    assert np.array_equal(bits64(metric.metric(a, b)), bits64(both))                           # repeatable
    alone = torch.cat([metric.metric(a[i:i + 1], b[i:i + 1]) for i in range(2)])
    assert np.array_equal(bits64(alone), bits64(both))                                          # independent of the batch
    same = metric.metric(a, a.clone())
    assert same.cpu().tolist() == [0.0, 0.0]                                                    # identical images: exactly 0
    bad = a.clone()
    bad[1, 2, 7, 5] = float("nan")
    spoiled = metric.metric(bad, b).cpu()
    assert bool(torch.isnan(spoiled[1])) and np.array_equal(bits64(spoiled[:1]), bits64(both[:1]))
    with pytest.raises(ValueError, match="at least 16"):
        metric.metric(a[:, :, :15], b[:, :, :15])
    with pytest.raises(ValueError, match="same dimensions"):
        metric.metric(a, b[:1])


def test_lpips_is_legal_under_graph_capture():
    metric, _, _ = lpips_fixture()
    a, b = (t.to(DEV) for t in lpips_images(2, 16, 16, 4))
    c, d = (t.to(DEV) for t in lpips_images(2, 16, 16, 5))
    eager_ab, eager_cd = metric.metric(a, b), metric.metric(c, d)
    xa, xb = a.clone(), b.clone()
    out = torch.zeros(2, dtype=torch.float64, device=DEV)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        metric._into(xa, xb, out)
    for src, want in (((a, b), eager_ab), ((c, d), eager_cd), ((a, b), eager_ab)):
        xa.copy_(src[0])
        xb.copy_(src[1])
        out.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits64(out), bits64(want))


def test_meter_column_and_res_txt_line(tmp_path):
    metric, _, _ = lpips_fixture()
    a, b = (t.to(DEV) for t in lpips_images(3, 19, 27, 2))
    want = metric.metric(a, b).cpu().numpy()
    meter = Q.QualityMeter(capacity=2, uciqe=True, lpips=metric)
    meter.update(a, b)
    meter.update(a[:2])                                       # no target: NaN, left out of the mean
    res = meter.compute()
    assert meter.columns[-1] == "lpips" and res["per_image"].shape == (5, 11)
    assert np.array_equal(res["per_image"][:3, -1], want) and np.isnan(res["per_image"][3:, -1]).all()
    assert res["lpips"] == float(want.sum() / 3)
    plain = Q.QualityMeter(uciqe=True)
    plain.update(a, b)
    plain.update(a[:2])
    assert np.array_equal(plain.compute()["per_image"], res["per_image"][:, :10], equal_nan=True)      # the other columns are untouched

    g = torch.Generator().manual_seed(5)
    batches = [(torch.randint(0, 256, (2, 3, 32, 32), generator=g, dtype=torch.uint8),
                torch.randint(0, 256, (2, 3, 32, 32), generator=g, dtype=torch.uint8), [f"img_{2 * i}.png", f"img_{2 * i + 1}.png"])
               for i in range(2)]

    def sampler(inp, **kw):                                   # a stand-in: evaluate() scores whatever the sampler returns
        return (inp / 255.0) * 1.6 - 0.9

    with_dir, without_dir = str(tmp_path / "with"), str(tmp_path / "without")
    res = EV.evaluate(sampler, [tuple(t.to(DEV) if torch.is_tensor(t) else t for t in bt) for bt in batches], ddim_step=2,
                      save_dir=with_dir, lpips=metric)
    lines = [ln for ln in open(os.path.join(with_dir, "res.txt")).read().split("\n") if ln]
    assert [ln.split(":")[0] + ":" for ln in lines] == [k for k, _ in EV.RES_KEYS] + ["lpips_orgin_avg:"]
    assert float(lines[-1].split(":")[1]) == res["lpips"] and np.isfinite(res["lpips"]) and res["lpips"] > 0
    plain = EV.evaluate(sampler, [tuple(t.to(DEV) if torch.is_tensor(t) else t for t in bt) for bt in batches], ddim_step=2,
                        save_dir=without_dir)
    assert "lpips" not in plain
    # without the option res.txt is byte for byte what the code before this option wrote: its writer, restated here
    before = "".join("\n" + key + str(plain[k]) for key, k in
                     (("psnr_orgin_avg:", "psnr"), ("ssim_orgin_avg:", "ssim"), ("uiqm_orgin_avg:", "uiqm"), ("uism_orgin_avg:", "uism"),
                      ("uicm_orgin_avg:", "uicm"), ("uiconm_orgin_avg:", "uiconm")))
    assert open(os.path.join(without_dir, "res.txt")).read() == before
    assert open(os.path.join(with_dir, "res.txt")).read() == before + "\nlpips_orgin_avg:" + str(res["lpips"])
