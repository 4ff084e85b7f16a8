"""GPU tests of the second tree's training path: GaussianDiffusionTrainer (diffusion/Diffusion.py) through DynamicUNet's
autograd path, the fused loss tail and the new backward kernels (csrc/train_b_ops.hip), and the native AdamW on a model whose
middle blocks freeze and thaw.  Golden vectors: tests/golden/dyn_trainer_small.npz (tools/gen_golden_train_b.py, from the real
reference DynamicUNet and colour loss).  The parity tests run in both contraction modes, selected here."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hdiff_amd  # noqa: E402
from hdiff_amd import _capi  # noqa: E402
from hdiff_amd import autograd as AG  # noqa: E402
from hdiff_amd import optim as HO  # noqa: E402
from hdiff_amd.diffusion.Diffusion import GaussianDiffusionSampler, GaussianDiffusionTrainer  # noqa: E402
from hdiff_amd.diffusion.Model import DynamicUNet  # noqa: E402
from tools.gen_golden_train_b import dino_standin, msssim_standin, sample_idx  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TERMS = ("loss", "mse_loss", "perceptual_dino", "msssim", "col_loss")


@pytest.fixture(params=["f32", "bf16x3"])
def mode(request):
    before = hdiff_amd.get_contraction_mode()
    hdiff_amd.set_contraction_mode(request.param)
    try:
        yield request.param
    finally:
        hdiff_amd.set_contraction_mode(before)


def T(a):
    return torch.from_numpy(np.asarray(a))


def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "dyn_trainer_small.npz"))


def small_model():
    from _tree_b_small import load_small_dyn_unet
    _, cfg, m, _ = load_small_dyn_unet()
    return m.to(DEV).train(), cfg


def trainer_for(m, d):
    b1, bT = (float(v) for v in d["beta"])
    return GaussianDiffusionTrainer(m, b1, bT, 1000, dino_loss=dino_standin, msssim_loss=msssim_standin).to(DEV)


def batch(d, kind):
    return (T(d[f"{kind}/gt"]).to(DEV), T(d[f"{kind}/input"]).to(DEV), T(d[f"{kind}/t"]).to(DEV), T(d[f"{kind}/noise"]).to(DEV))


def rel_err(got, ref):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    return (got - ref).abs().max().item() / (ref.abs().max().item() + 1e-12)


def check_grads(m, d, tag):
    names = list(d["param_names"])
    gmax, samples = d[f"{tag}/gradmax"], d[f"{tag}/grad_samples"]
    params = dict(m.named_parameters())
    assert names == list(params.keys())
    # gradients that are zero analytically (e.g. the bias of a conv feeding a GroupNorm of one channel per group: the mean
    # subtraction removes it) are rounding noise on both sides; they are judged against a floor of 1e-3 of the largest gradient
    floor = 1e-3 * float(np.nanmax(gmax))
    off, worst = 0, 0.0
    for name, gm in zip(names, gmax):
        p = params[name]
        idx = sample_idx(p.numel())
        ref = samples[off:off + len(idx)]
        off += len(idx)
        if np.isnan(gm):
            assert p.grad is None, f"{tag}: {name} should have no gradient (frozen / unused), got one"
            continue
        assert p.grad is not None, f"{tag}: {name} has no gradient"
        got = p.grad.detach().reshape(-1)[torch.from_numpy(idx).to(DEV)].cpu().numpy()
        scale = max(float(gm), floor)
        err = np.abs(got - ref).max() / scale
        gfull = p.grad.detach().abs().max().item()
        err = max(err, abs(gfull - float(gm)) / scale)
        worst = max(worst, err)
        assert err < 1e-3, (tag, name, err)
    assert off == len(samples)
    return worst


@pytest.mark.parametrize("case", ["uw_cz1", "uw_cz0", "atm_cz1", "atm_cz0"])
def test_trainer_terms_and_gradients_match_reference(mode, case):
    """The five returned terms and every parameter gradient of loss.mean().backward() (reference rotinas.py:443) against the
    real reference model + colour loss; the gated-off middle blocks (and the unused image encoder with context_zero) have
    .grad None."""
    d = fixture()
    m, _ = small_model()
    tr = trainer_for(m, d)
    kind, cz = case.split("_")
    gt, inp, t, noise = batch(d, kind)
    terms = tr(gt, inp, 0, t=t, noise=noise, context_zero=cz == "cz1")
    assert len(terms) == 5 and terms[0].requires_grad
    for nm, v in zip(TERMS, terms):
        ref = T(d[f"case/{kind}_{cz}/{nm}"])
        assert tuple(v.shape) == tuple(ref.shape), (nm, v.shape, ref.shape)
        assert rel_err(v, ref) < 1e-3, (nm, rel_err(v, ref))
    terms[0].mean().backward()
    worst = check_grads(m, d, f"case/{kind}_{cz}")
    print(f"{case} [{mode}]: worst relative gradient error {worst:.2e}")


def test_three_step_trajectory_with_native_adamw(mode):
    """clip(1.0) + AdamW over three steps that alternate an underwater-like and an atmospheric-like pair: the middle blocks
    freeze and thaw, so their Adam step counts fall behind the others' (torch keeps one count per parameter).  Total norms and
    parameters after every step match the reference run with torch.optim.AdamW."""
    d = fixture()
    m, _ = small_model()
    tr = trainer_for(m, d)
    lr, wd = (float(v) for v in d["lr_wd"])
    opt = HO.AdamW(m.parameters(), lr=lr, weight_decay=wd)
    plan = [("uw", False), ("atm", True), ("uw", False)]
    for k, (kind, cz) in enumerate(plan):
        gt, inp, t, noise = batch(d, kind)
        opt.zero_grad()
        loss = tr(gt, inp, 0, t=t, noise=noise, context_zero=cz)[0]
        loss.mean().backward()
        total = opt.step(max_grad_norm=1.0).item()
        want = float(d[f"traj/{k}/total_norm"][0])
        assert abs(total - want) / want < 1e-3, (k, total, want)
        got = torch.cat([p.detach().reshape(-1)[torch.from_numpy(sample_idx(p.numel())).to(DEV)] for p in m.parameters()]).cpu()
        diff = (got - T(d[f"traj/{k}/param_samples"])).abs()
        # as in the tree-A trainer test (an Adam update is ~lr * g / (|g| + eps): ill-conditioned where g ~ eps), with a wider
        # share for the bulk: here some gradients are zero analytically (conv biases and projections feeding a GroupNorm of one
        # channel per group), so their updates are lr-sized noise on both sides (measured: 1.8 % of the samples above 2e-6 after
        # the first step, at most 2.2e-5).  A wrong step count moves every element of the affected blocks (> 10 % of samples).
        frac = (diff > 2e-6).float().mean().item()
        assert diff.max().item() < 2.5e-4 * (k + 1) and frac < 0.05, (k, diff.max().item(), frac)
    counts = {n: int(opt.state[p]["step"]) for n, p in m.named_parameters() if p in opt.state}
    assert counts["middleblocks.0.block1.2.weight"] == 2 and counts["middleblocks.1.block1.2.weight"] == 1
    assert counts["head.weight"] == 3


def _tail_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    B, H, W = 2, 5, 7
    npred = torch.randn(B, 3, H, W, generator=g)
    noise = torch.randn(B, 3, H, W, generator=g)
    y_t = torch.randn(B, 3, H, W, generator=g)
    gt = torch.rand(B, 3, H, W, generator=g) * 2 - 1
    # pixels whose y_0_pred is exactly zero and tiny (both eps branches of F.normalize / cosine_similarity), and a zero gt pixel
    npred[0, :, 0, 0] = 0.0; y_t[0, :, 0, 0] = 0.0
    npred[0, :, 0, 1] = 0.0; y_t[0, :, 0, 1] = torch.tensor([1e-15, -2e-15, 3e-15])
    npred[0, :, 0, 2] = 0.0; y_t[0, :, 0, 2] = torch.tensor([1e-21, 2e-21, -1e-21])
    npred[1, :, 1, 1] = 0.0; y_t[1, :, 1, 1] = torch.tensor([1e-9, 1e-9, -2e-9])
    gt[1, :, 2, 3] = 0.0
    t = torch.tensor([3, 870])
    betas = torch.linspace(1e-4, 0.02, 1000).double()
    ab = torch.cumprod(1 - betas, 0)
    return npred, noise, y_t, gt, t, ab.sqrt().float(), (1 - ab).sqrt().float(), g


def _run_tail(npred, noise, y_t, gt, t, sa, s1m, d_mse, d_y0, d_col):
    lib, s = _capi.lib(), torch.cuda.current_stream().cuda_stream
    B, _, H, W = npred.shape
    mse, y0, col = torch.empty_like(npred), torch.empty_like(npred), torch.empty((), device=DEV)
    nb = C.c_int64(0)
    _capi.check(lib.hdiff_train_b_loss_workspace(B * H * W, C.byref(nb)))
    ws = torch.empty(nb.value // 4, device=DEV)
    _capi.check(lib.hdiff_train_b_loss_fwd(npred.data_ptr(), noise.data_ptr(), y_t.data_ptr(), gt.data_ptr(), t.data_ptr(),
                                           sa.data_ptr(), s1m.data_ptr(), 1000, B, H * W, mse.data_ptr(), y0.data_ptr(),
                                           col.data_ptr(), ws.data_ptr(), s))
    d_np = torch.empty_like(npred)
    _capi.check(lib.hdiff_train_b_loss_bwd(npred.data_ptr(), noise.data_ptr(), y0.data_ptr(), gt.data_ptr(), t.data_ptr(),
                                           sa.data_ptr(), s1m.data_ptr(), 1000, B, H * W, d_mse.data_ptr(), d_y0.data_ptr(),
                                           d_col.data_ptr(), d_np.data_ptr(), s))
    torch.cuda.synchronize()
    return mse, y0, col, d_np


def test_loss_tail_kernel_against_float64_torch():
    """hdiff_train_b_loss_fwd / _bwd against float64 torch: mse, y_0_pred, the colour term 1 - mean(cosine_similarity(
    normalize(y0), normalize(gt))) and d noise_pred from all three incoming gradients, including pixels at and near zero.
    Two runs are bitwise identical."""
    npred, noise, y_t, gt, t, sa, s1m, g = _tail_inputs(0)
    d_mse = torch.randn(npred.shape, generator=g)
    d_y0 = torch.randn(npred.shape, generator=g) * 10
    d_col = torch.tensor(0.7)
    dev = [x.to(DEV) for x in (npred, noise, y_t, gt, t, sa, s1m, d_mse, d_y0, d_col)]
    mse, y0, col, d_np = _run_tail(*dev)
    mse2, y02, col2, d_np2 = _run_tail(*dev)
    assert torch.equal(mse, mse2) and torch.equal(y0, y02) and torch.equal(col, col2) and torch.equal(d_np, d_np2)
    # float64 reference; the colour term and its gradient start from the kernel's own y0 (the eps branches depend on the exact
    # value of y0, which the reference computes in fp32 too)
    r = (1.0 / sa.double()[t]).view(-1, 1, 1, 1)
    c = s1m.double()[t].view(-1, 1, 1, 1)
    np64 = npred.double()
    y0_64 = r * (y_t.double() - c * np64) / 255.0
    assert rel_err(mse, (np64 - noise.double()) ** 2) < 1e-6
    assert rel_err(y0, y0_64) < 1e-6
    assert (y0[0, :, 0, 0] == 0).all()
    u = y0.detach().cpu().double().requires_grad_(True)
    cos = F.cosine_similarity(F.normalize(u, p=2, dim=1), F.normalize(gt.double(), p=2, dim=1), dim=1)
    col64 = 1 - cos.mean()
    assert abs(col.item() - col64.item()) < 1e-6, (col.item(), col64.item())
    (gu,) = torch.autograd.grad(col64, u)
    want = d_mse.double() * 2 * (np64 - noise.double()) + (d_y0.double() + d_col.double() * gu) * (-(r * c) / 255.0)
    got = d_np.cpu().double()
    tol = 1e-4 * want.abs() + 1e-5 * want.abs().median()
    bad = (got - want).abs() > tol
    assert not bad.any(), (got[bad][:5], want[bad][:5])
    assert want[0, :, 0, 1].abs().min() > 1e6          # the tiny pixels really carry the large eps-branch gradients


@pytest.mark.parametrize("src,dst", [((5, 7), (9, 11)), ((9, 11), (5, 7)), ((3, 5), (6, 10)), ((7, 3), (7, 13))])
def test_resize_nearest_backward_matches_torch_autograd(src, dst):
    g = torch.Generator().manual_seed(sum(src) + sum(dst))
    x = torch.randn(2, 5, *src, generator=g).to(DEV).requires_grad_(True)
    dy = torch.randn(2, 5, *dst, generator=g).to(DEV)
    ours = AG._ResizeFn.apply(x, dst[0], dst[1])
    ref = F.interpolate(x, size=dst, mode="nearest")
    assert torch.equal(ours, ref)
    (gx,) = torch.autograd.grad(ours, x, dy)
    (gr,) = torch.autograd.grad(ref, x, dy)
    assert rel_err(gx, gr) < 1e-6
    (gx2,) = torch.autograd.grad(AG._ResizeFn.apply(x, dst[0], dst[1]), x, dy)
    assert torch.equal(gx, gx2)


def test_global_pool_backward_matches_torch_autograd():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 7, 9, 5, generator=g).to(DEV).requires_grad_(True)
    dy = torch.randn(3, 7, generator=g).to(DEV)
    ours = AG._PoolFn.apply(x)
    ref = F.adaptive_avg_pool2d(x, (1, 1)).flatten(1)
    assert rel_err(ours, ref) < 1e-6
    (gx,) = torch.autograd.grad(ours, x, dy)
    (gr,) = torch.autograd.grad(ref, x, dy)
    assert rel_err(gx, gr) < 1e-6


@pytest.mark.parametrize("cin,cout,hw", [(3, 8, (17, 16)), (8, 16, (9, 8)), (2, 4, (8, 8)), (16, 32, (5, 7))])
def test_image_encoder_strided_conv_backward(cin, cout, hw):
    """The image encoder's stride-2 3x3 convs (ConditionalEmbedding: Cin = 3, ch/16, ch/8) against torch autograd in float64,
    odd and even sizes: input, weight and bias gradients."""
    g = torch.Generator().manual_seed(cin * 100 + cout)
    x = torch.randn(2, cin, *hw, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) * 0.3
    b = torch.randn(cout, generator=g)
    dy = torch.randn(2, cout, (hw[0] - 1) // 2 + 1, (hw[1] - 1) // 2 + 1, generator=g)
    xs, ws, bs = (v.to(DEV).requires_grad_(True) for v in (x, w, b))
    out = AG._StridedConvFn.apply(xs, ws, bs)
    gx, gw, gb = torch.autograd.grad(out, (xs, ws, bs), dy.to(DEV))
    x64, w64, b64 = (v.double().requires_grad_(True) for v in (x, w, b))
    ref = F.conv2d(x64, w64, b64, stride=2, padding=1)
    rx, rw, rb = torch.autograd.grad(ref, (x64, w64, b64), dy.double())
    assert rel_err(out, ref) < 1e-4
    assert rel_err(gx, rx) < 1e-4 and rel_err(gw, rw) < 1e-4 and rel_err(gb, rb) < 1e-4


def test_frozen_middle_blocks_launch_no_weight_gradient_kernels(monkeypatch):
    d = fixture()
    m, _ = small_model()
    tr = trainer_for(m, d)
    gt, inp, t, noise = batch(d, "uw")
    calls = []
    real = AG._run_wgrad
    monkeypatch.setattr(AG, "_run_wgrad", lambda *a, **k: (calls.append(1), real(*a, **k))[1])

    def run():
        calls.clear()
        m.zero_grad(set_to_none=True)
        tr(gt, inp, 0, t=t, noise=noise, context_zero=False)[0].mean().backward()
        return len(calls)
    gated = run()
    assert all(p.grad is None for i in (1, 3) for p in m.middleblocks[i].parameters())
    assert all(p.grad is not None for i in (0, 2) for p in m.middleblocks[i].parameters())
    monkeypatch.setattr(m, "dynamic_forward", lambda x: [p.requires_grad_(True) for p in m.parameters()])
    everything = run()
    # a gated-off middle block has 4 weight-gradient launches: two 3x3 convs, the attention in- and out-projections
    assert everything - gated == 2 * 4, (everything, gated)


def test_train_mode_dropout_runs_and_reproduces():
    def run():
        torch.manual_seed(11)
        m = DynamicUNet(T=1000, ch=32, ch_mult=[1, 2, 2], num_res_blocks=1, dropout=0.15).to(DEV).train()
        tr = GaussianDiffusionTrainer(m, 1e-4, 0.02, 1000)
        g = torch.Generator().manual_seed(12)
        gt = torch.randint(0, 256, (2, 3, 16, 16), generator=g).float().to(DEV)
        inp = torch.randint(0, 256, (2, 3, 16, 16), generator=g).float().to(DEV)
        with pytest.warns(RuntimeWarning):
            loss = tr(gt, inp, 0)[0]
        loss.mean().backward()
        return loss.detach(), {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    l1, g1 = run()
    l2, g2 = run()
    assert torch.isfinite(l1).all() and all(torch.isfinite(v).all() for v in g1.values())
    assert torch.equal(l1, l2) and g1.keys() == g2.keys() and all(torch.equal(g1[k], g2[k]) for k in g1)


def test_sampler_uses_the_trained_weights():
    d = fixture()
    m, cfg = small_model()
    tr = trainer_for(m, d)
    samp = GaussianDiffusionSampler(m, 1e-4, 0.02, 1000)
    gt, inp, t, noise = batch(d, "uw")
    y_T = torch.randn(2, 3, 16, 16, generator=torch.Generator().manual_seed(5)).to(DEV)
    with torch.no_grad():
        before = samp(inp, ddim=True, ddim_step=5, y_T=y_T)
    opt = HO.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-4)
    for _ in range(3):
        opt.zero_grad()
        tr(gt, inp, 0, t=t, noise=noise, context_zero=False)[0].mean().backward()
        opt.step(max_grad_norm=1.0)
    with torch.no_grad():
        after = samp(inp, ddim=True, ddim_step=5, y_T=y_T)
    fresh = DynamicUNet(**cfg).to(DEV)
    fresh.load_state_dict(m.state_dict())
    with torch.no_grad():
        want = GaussianDiffusionSampler(fresh, 1e-4, 0.02, 1000)(inp, ddim=True, ddim_step=5, y_T=y_T)
    assert not torch.equal(before, after)
    assert torch.equal(after, want)


def test_reference_shaped_loop_256_decreases_the_loss():
    """loss = trainer(input, label, stage)[0]; loss.mean().backward(); opt.step(max_grad_norm=1.0) -- ten steps of the default
    tree-B configuration at 256^2, batch 2 (fixed t / noise, so that the trend is the model's, not the draws')."""
    torch.manual_seed(0)
    m = DynamicUNet(T=1000, ch=128, ch_mult=[1, 2, 2, 2], num_res_blocks=2, dropout=0.15).to(DEV).train()
    tr = GaussianDiffusionTrainer(m, 1e-4, 0.02, 1000)
    opt = HO.AdamW(m.parameters(), lr=1e-4, weight_decay=1e-4)
    g = torch.Generator().manual_seed(1)
    label = torch.randint(0, 256, (2, 3, 256, 256), generator=g).to(torch.uint8).to(DEV)
    inp = (label.float() * torch.tensor([0.4, 0.9, 1.0], device=DEV).view(1, 3, 1, 1)).to(torch.uint8)
    t = torch.tensor([150, 600], device=DEV)
    noise = torch.randn(2, 3, 256, 256, generator=g).to(DEV)
    losses = []
    with pytest.warns(RuntimeWarning):
        for _ in range(10):
            opt.zero_grad()
            loss = tr(label, inp, 0, t=t, noise=noise)[0]
            loss.mean().backward()
            opt.step(max_grad_norm=1.0)
            losses.append(loss.mean().item())
    print("losses", losses)
    assert all(np.isfinite(losses))
    assert np.mean(losses[5:]) < np.mean(losses[:5]) and losses[-1] < losses[0], losses
