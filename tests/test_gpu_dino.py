"""The DINOv2 perceptual loss on the GPU (hdiff_amd/dino.py, csrc/dino.hip) against tests/_dino_def.py.

Gates.  Unfold / fold, the token assembly and the tap's gradient: bit for bit against their fp32 definitions.  LayerNorm and GELU: error
against the float64 definition at most 4x that of torch's fp32 CPU operator on the same inputs (max and rms; LayerNorm per kind of
row, with a floor of one fp32 ulp of the rows' largest output, GELU per bucket).  The tap's forward: 2 fp32 ulp of the float64 value.
The whole trunk: loss within 4x the relative error of the definition evaluated in fp32 on the CPU (or one fp32 ulp of the value where
that is larger: the value is one fp32 number), gradient rms within 4x that arm's.  Every figure is printed before it is asserted;
profiles/dino.txt holds the measured ones.
"""
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _dino_def as D  # noqa: E402
import hdiff_amd  # noqa: E402
from hdiff_amd import dino  # noqa: E402
from hdiff_amd.Loss.loss import PerceptualLoss_dino  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]
DEV = "cuda:0"
YARD = 4.0


def ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


@pytest.fixture(params=["bf16x3", "f32"])
def mode(request):
    before = hdiff_amd.get_contraction_mode()
    hdiff_amd.set_contraction_mode(request.param)
    try:
        yield request.param
    finally:
        hdiff_amd.set_contraction_mode(before)


# ------------------------------------------------------------------------------------------------------------ unfold / fold
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", [(18, 18), (18, 32), (32, 46), (46, 32)])
def test_unfold_and_fold_bit_for_bit(H, W, B):
    g = torch.Generator().manual_seed(H * 100 + W + B)
    x = torch.randn(B, 3, H, W, generator=g)
    xc = x.clone().requires_grad_(True)
    want = D.unfold(D.crop(xc)).transpose(1, 2)                       # (B, 588, h*w): pure indexing
    xd = x.to(DEV).requires_grad_(True)
    got = dino.unfold_patches(xd)
    assert same_bits(got, want)
    dy = torch.randn(want.shape, generator=g)
    want.backward(dy)
    got.backward(dy.to(DEV))
    assert same_bits(xd.grad, xc.grad)
    gr = xd.grad.cpu()
    border = torch.ones(H, W, dtype=torch.bool)
    border[2:H - 2, 2:W - 2] = False
    assert torch.equal(bits(gr[:, :, border]), torch.zeros_like(bits(gr[:, :, border])))      # +0 exactly, not -0
    assert (gr[:, :, ~border] != 0).all()
    with pytest.raises(RuntimeError, match="19 x 18"):
        dino.unfold_patches(torch.zeros(1, 3, 19, 18, device=DEV))


# --------------------------------------------------------------------------------------------------------- token assembly
@pytest.mark.parametrize("B,C,P", [(1, 8, 1), (3, 48, 6), (2, 384, 324)])
def test_token_assembly_bit_for_bit(B, C, P):
    g = torch.Generator().manual_seed(C + P)
    patch, cls, pos = torch.randn(B, C, P, generator=g), torch.randn(C, generator=g), torch.randn(C, P + 1, generator=g)
    want = torch.cat([cls.view(1, C, 1).expand(B, C, 1), patch], dim=2) + pos
    pd = patch.to(DEV).requires_grad_(True)
    got = dino.assemble_tokens(pd, cls.to(DEV), pos.to(DEV))
    assert same_bits(got, want)
    dy = torch.randn(B, C, P + 1, generator=g)
    got.backward(dy.to(DEV))
    assert same_bits(pd.grad, dy[:, :, 1:])


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
KINDS = ("ordinary", "mean = 1e3 x spread", "constant", "1e4 x louder")


def ln_case(C, L):
    """(B = 4, C, L) input whose token (flat index b * L + l) 1 has mean = 1e3 x spread, 2 is constant, 3 is 1e4 times louder than its
    neighbours; everything else is ordinary.  -> x, the kind of every token"""
    g = torch.Generator().manual_seed(C * 1000 + L)
    B = 4
    x = torch.randn(B, L, C, generator=g)
    kind = torch.zeros(B * L, dtype=torch.long)
    flat = x.view(B * L, C)
    flat[1] = 1e3 + flat[1]
    flat[2] = 2.5
    flat[3] = 1e4 * flat[3]
    kind[1], kind[2], kind[3] = 1, 2, 3
    w, b, dy = torch.randn(C, generator=g), torch.randn(C, generator=g), torch.randn(B, L, C, generator=g)
    return x, kind.view(B, L), w, b, dy


@pytest.mark.parametrize("L", [1, 7, 65, 325])
@pytest.mark.parametrize("C", [8, 48, 384])
def test_layernorm_forward_and_backward_against_float64(C, L):
    x, kind, w, b, dy = ln_case(C, L)
    x64 = x.double().requires_grad_(True)
    y64 = D.layer_norm(x64, w.double(), b.double())
    y64.backward(dy.double())
    x32 = x.clone().requires_grad_(True)
    y32 = F.layer_norm(x32, (C,), w, b, eps=1e-6)
    y32.backward(dy)
    xd = x.transpose(1, 2).contiguous().to(DEV).requires_grad_(True)              # channel-major (B, C, L)
    yd = dino.layer_norm(xd, w.to(DEV), b.to(DEV))
    yd.backward(dy.transpose(1, 2).contiguous().to(DEV))
    got_y, got_dx = yd.detach().cpu().transpose(1, 2).double(), xd.grad.cpu().transpose(1, 2).double()
    assert torch.isfinite(got_dx).all() and torch.isfinite(got_y).all()
    for k, name in enumerate(KINDS):
        rows = kind == k
        for what, got, yard, ref in (("fwd", got_y, y32.detach().double(), y64.detach()), ("bwd", got_dx, x32.grad.double(), x64.grad)):
            e, ey, top = (got - ref)[rows].abs(), (yard - ref)[rows].abs(), float(ref[rows].abs().max())
            floor = ulp32(top)
            mx, rms, ymx, yrms = float(e.max()), float(e.pow(2).mean().sqrt()), float(ey.max()), float(ey.pow(2).mean().sqrt())
            print(f"C {C} L {L} {name} {what}: max {mx:.3e} (fp32 CPU {ymx:.3e}) rms {rms:.3e} (fp32 CPU {yrms:.3e}) ulp of the largest "
                  f"{floor:.3e}  ratios {mx / max(ymx, 1e-300):.2f} {rms / max(yrms, 1e-300):.2f}")
            assert mx <= max(YARD * ymx, floor) and rms <= max(YARD * yrms, floor), (C, L, name, what)
    const = yd.detach().cpu().transpose(1, 2)[kind == 2]
    assert same_bits(const, b.view(1, C).expand_as(const).contiguous())             # a constant row gives beta exactly
    # the loud row does not leak: with an ordinary row in its place every other token keeps its bits, forward and backward
    x2 = x.clone()
    x2.view(-1, C)[3] = torch.randn(C, generator=torch.Generator().manual_seed(5))
    xd2 = x2.transpose(1, 2).contiguous().to(DEV).requires_grad_(True)
    yd2 = dino.layer_norm(xd2, w.to(DEV), b.to(DEV))
    yd2.backward(dy.transpose(1, 2).contiguous().to(DEV))
    others = (kind != 3).view(-1)
    pick = lambda t: t.detach().cpu().transpose(1, 2).reshape(-1, C)[others]
    assert same_bits(pick(yd), pick(yd2)) and same_bits(pick(xd.grad), pick(xd2.grad))


# --------------------------------------------------------------------------------------------------------------------- GELU
def test_gelu_forward_and_backward_against_float64():
    x = torch.cat([torch.linspace(-10.0, 10.0, 400001), torch.tensor([0.0, -0.0, 3.0, -3.0, 10.0, -10.0])])
    x64 = x.double().requires_grad_(True)
    y64 = D.gelu(x64)
    y64.backward(torch.ones_like(y64))
    x32 = x.clone().requires_grad_(True)
    y32 = F.gelu(x32)
    y32.backward(torch.ones_like(y32))
    xd = x.to(DEV).requires_grad_(True)
    yd = dino.gelu(xd)
    yd.backward(torch.ones_like(yd))
    for name, rows in (("[-10, -3)", x < -3.0), ("[-3, 3]", (x >= -3.0) & (x <= 3.0)), ("(3, 10]", x > 3.0)):
        for what, got, yard, ref in (("fwd", yd.detach().cpu().double(), y32.detach().double(), y64.detach()),
                                     ("bwd", xd.grad.cpu().double(), x32.grad.double(), x64.grad)):
            e, ey = (got - ref)[rows].abs(), (yard - ref)[rows].abs()
            mx, rms, ymx, yrms = float(e.max()), float(e.pow(2).mean().sqrt()), float(ey.max()), float(ey.pow(2).mean().sqrt())
            print(f"gelu {name} {what}: max {mx:.3e} (fp32 CPU {ymx:.3e}) rms {rms:.3e} (fp32 CPU {yrms:.3e})  ratios "
                  f"{mx / max(ymx, 1e-300):.2f} {rms / max(yrms, 1e-300):.2f}")
            assert mx <= YARD * ymx and rms <= YARD * yrms, (name, what)
    sp = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan")])
    spd = sp.to(DEV).requires_grad_(True)
    out = dino.gelu(spd)
    out.backward(torch.ones_like(out))
    out, gr, ref = out.detach().cpu(), spd.grad.cpu(), F.gelu(sp)
    assert same_bits(out[:2], ref[:2]) and same_bits(gr[:2], torch.tensor([0.5, 0.5]))          # +0 and -0 as torch
    assert out[2] == float("inf") and gr[2] == 1.0
    assert out[3] == 0.0 and gr[3] == 0.0
    if ref[3] == 0.0:                                    # where torch's kernel returns a zero at -inf, the sign is torch's
        assert torch.signbit(out[3]) == torch.signbit(ref[3])
    assert torch.isnan(out[4]) and torch.isnan(gr[4])


# ---------------------------------------------------------------------------------------------------------- smooth-L1 tap
def tap_pair(n, seed, B=1):
    """a, b with a - b exact in fp32: differences on a grid of 1/64 over [-3, 3], with exactly 1, -1 and 0 among them"""
    g = torch.Generator().manual_seed(seed)
    b = torch.randint(-32, 33, (B, n), generator=g).float() / 4
    d = torch.randint(-192, 193, (B, n), generator=g).float() / 64
    for j, v in enumerate((1.0, -1.0, 0.0)):
        if j < n:
            d[:, j] = v
    return b + d, b, d


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, 325 * 384])
def test_smooth_l1_tap(n):
    a, b, d = tap_pair(n, n)
    assert torch.equal(a - b, d)
    want = float(D.smooth_l1(d.double()).mean())
    ad = a.to(DEV).requires_grad_(True)
    loss = dino.smooth_l1_taps(ad, b.to(DEV))
    (loss * 1.75).backward()
    got = float(loss)
    print(f"n = {n}: device {got!r}  float64 {want!r}  gap {abs(got - want) / ulp32(want):.2f} ulp")
    assert loss.dim() == 0 and loss.dtype == torch.float32 and abs(got - want) <= 2 * ulp32(want)
    coef = torch.tensor(1.75) * torch.tensor(1.0) / torch.tensor(float(n))
    assert same_bits(ad.grad, coef * d.clamp(-1.0, 1.0))
    # identical inputs: exactly 0 and a 0 gradient
    zd = a.to(DEV).requires_grad_(True)
    zero = dino.smooth_l1_taps(zd, a.to(DEV))
    zero.backward()
    assert float(zero) == 0.0 and not zd.grad.any()
    # the multiplicity scales exactly (2 is a power of two: every product is exact)
    a2 = a.to(DEV).requires_grad_(True)
    twice = dino.smooth_l1_taps(a2, b.to(DEV), 2.0)
    (twice * 1.75).backward()
    assert float(twice) == 2.0 * got and same_bits(a2.grad, 2.0 * ad.grad.cpu())
    thrice = dino.smooth_l1_taps(a.to(DEV), b.to(DEV), 3.0)
    assert abs(float(thrice) - 3.0 * want) <= 2 * ulp32(3.0 * want)


def test_smooth_l1_tap_keeps_a_nan_in_its_image():
    a, b, d = tap_pair(4097, 7, B=3)
    clean = a.to(DEV).requires_grad_(True)
    dino.smooth_l1_taps(clean, b.to(DEV)).backward()
    a[1, 11] = float("nan")
    ad = a.to(DEV).requires_grad_(True)
    loss = dino.smooth_l1_taps(ad, b.to(DEV))
    loss.backward()
    assert torch.isnan(loss)
    assert same_bits(ad.grad[0], clean.grad[0]) and same_bits(ad.grad[2], clean.grad[2]) and torch.isfinite(ad.grad[[0, 2]]).all()
    assert torch.isnan(ad.grad[1, 11]) and int(torch.isnan(ad.grad[1]).sum()) == 1


# -------------------------------------------------------------------------------------------------------------- whole trunk
@functools.lru_cache(maxsize=None)
def reference(name):
    """The fixture, its float64 loss and gradient, and the fp32-CPU arm's errors; computed once, never modified."""
    sd, xa, xb, c = D.fixture(name)
    quad, lin, gap = D.check_fixture(sd, xa, xb, c)
    assert quad >= 0.05 and lin >= 0.05 and gap > D.MARGIN, (name, quad, lin, gap)
    v64, g64 = D.loss_and_grad(sd, xa, xb, c["heads"], c["depth"])
    v32, g32 = D.loss_and_grad(sd, xa, xb, c["heads"], c["depth"], torch.float32)
    per64 = D.loss(sd, xa, xb, c["heads"], c["depth"], per_image=True)
    return dict(sd=sd, xa=xa, xb=xb, c=c, v64=float(v64), g64=g64, per64=per64, yard_value=abs(float(v32) - float(v64)) / float(v64),
                yard_grad=float((g32.double() - g64).pow(2).mean().sqrt()))


def trunk_for(ref):
    c = ref["c"]
    t = dino.DinoV2Features(embed_dim=c["embed"], depth=c["depth"], heads=c["heads"], pos_grid=c["pos_grid"])
    return t.load_dinov2(ref["sd"]).to(DEV)


def run(trunk, xa, xb):
    x = xa.to(DEV).requires_grad_(True)
    loss, per = dino.dino_perceptual(trunk, x, xb.to(DEV), return_per_image=True)
    loss.backward()
    return loss.detach().cpu(), per.cpu(), x.grad.cpu()


@pytest.mark.parametrize("name", list(D.FIXTURES))
def test_whole_trunk_loss_and_input_gradient_against_float64(mode, name):
    ref = reference(name)
    trunk = trunk_for(ref)
    loss, per, grad = run(trunk, ref["xa"], ref["xb"])
    v_err = abs(float(loss) - ref["v64"]) / ref["v64"]
    g_err = float((grad.double() - ref["g64"]).pow(2).mean().sqrt())
    gate = max(YARD * ref["yard_value"], ulp32(ref["v64"]) / ref["v64"])
    print(f"{name} [{mode}]: loss {float(loss)!r} float64 {ref['v64']!r} rel err {v_err:.3e} (fp32 CPU {ref['yard_value']:.3e}, gate {gate:.3e})"
          f"  grad rms err {g_err:.3e} (fp32 CPU {ref['yard_grad']:.3e}, ratio {g_err / ref['yard_grad']:.2f})")
    assert loss.dim() == 0 and loss.dtype == torch.float32
    assert v_err <= gate
    assert g_err <= YARD * ref["yard_grad"]
    assert float((per.double() - ref["per64"]).abs().max()) <= 1e-5 * ref["v64"] and abs(float(per.double().sum()) - float(loss)) <= 1e-5 * ref["v64"]
    # the 2-pixel border took part in nothing
    H, W = grad.shape[2:]
    border = torch.ones(H, W, dtype=torch.bool)
    border[2:H - 2, 2:W - 2] = False
    assert not grad[:, :, border].any() and (grad[:, :, ~border] != 0).all()
    # bitwise repeatable
    loss2, per2, grad2 = run(trunk, ref["xa"], ref["xb"])
    assert same_bits(loss, loss2) and same_bits(per, per2) and same_bits(grad, grad2)
    # image 0 does not see image 1
    g = torch.Generator().manual_seed(77)
    xa2, xb2 = ref["xa"].clone(), ref["xb"].clone()
    xa2[1], xb2[1] = torch.randn(xa2[1].shape, generator=g), torch.randn(xb2[1].shape, generator=g)
    loss3, per3, grad3 = run(trunk, xa2, xb2)
    assert same_bits(per[0], per3[0]) and same_bits(grad[0], grad3[0]) and not same_bits(per[1], per3[1])
    # the loss module gives the same numbers and keeps the shares
    mod = PerceptualLoss_dino(trunk=trunk)
    x = ref["xa"].to(DEV).requires_grad_(True)
    v = mod(x, ref["xb"].to(DEV))
    v.backward()
    assert same_bits(v, loss) and same_bits(x.grad, grad) and same_bits(mod.last_per_image, per)
    feats = trunk(ref["xa"].to(DEV))
    assert len(feats) == ref["c"]["depth"] * 10 + 4 and tuple(feats[-1].shape) == (2, ref["c"]["embed"])


def test_layers_selection_changes_the_loss_and_keeps_the_gradient_path():
    ref = reference("e32")
    trunk = trunk_for(ref)
    sd, c = ref["sd"], ref["c"]
    mod = PerceptualLoss_dino(trunk=trunk, layers=["blocks.0.attn", "blocks.0.attn.proj", "head"])
    x = ref["xa"].to(DEV).requires_grad_(True)
    v = mod(x, ref["xb"].to(DEV))
    v.backward()
    fa, fb = D.features(sd, ref["xa"], c["heads"], c["depth"]), D.features(sd, ref["xb"], c["heads"], c["depth"])
    want = 2 * D.smooth_l1(fa["0.proj"] - fb["0.proj"]).mean() + D.smooth_l1(fa["cls"] - fb["cls"]).mean()
    assert abs(float(v) - float(want)) <= 1e-5 * float(want) and x.grad.abs().max() > 0


# ----------------------------------------------------------------------------------------------------------- stream capture
def test_forward_and_backward_are_legal_under_stream_capture():
    ref = reference("e32")
    trunk = trunk_for(ref)
    eager_loss, _, eager_grad = run(trunk, ref["xa"], ref["xb"])            # also fills the position-embedding cache
    g = torch.Generator().manual_seed(5)
    other = torch.randn(ref["xa"].shape, generator=g)
    other_loss, _, other_grad = run(trunk, other, ref["xb"])
    xin = ref["xa"].to(DEV).requires_grad_(True)
    xb = ref["xb"].to(DEV)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        loss = dino.dino_perceptual(trunk, xin, xb)
        (grad,) = torch.autograd.grad(loss, xin)
    for src, want_loss, want_grad in ((ref["xa"], eager_loss, eager_grad), (other, other_loss, other_grad), (ref["xa"], eager_loss, eager_grad)):
        with torch.no_grad():
            xin.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(loss, want_loss) and same_bits(grad, want_grad)


# ------------------------------------------------------------------------------------------------------------------ trainer
def small_model():
    from _tree_b_small import load_small_dyn_unet
    _, _, m, _ = load_small_dyn_unet()
    return m.to(DEV).train()


def test_trainer_with_the_native_term():
    """32 x 32: the smallest size the small model (two halvings) and the trunk (H - 4 a multiple of 14) both accept."""
    from hdiff_amd.diffusion.Diffusion import GaussianDiffusionTrainer
    ref = reference("e32")
    g = torch.Generator().manual_seed(11)
    gt, inp = (torch.randint(0, 256, (2, 3, 32, 32), generator=g, dtype=torch.uint8).to(DEV) for _ in range(2))
    t, noise = torch.tensor([704, 50], device=DEV), torch.randn(2, 3, 32, 32, generator=g).to(DEV)

    def step(dino_loss):
        m = small_model()
        tr = GaussianDiffusionTrainer(m, 1e-4, 0.02, 1000, dino_loss=dino_loss).to(DEV)
        terms = tr(gt, inp, 0, t=t, noise=noise, context_zero=False)
        terms[0].mean().backward()
        return [v.detach().cpu() for v in terms], {n: p.grad.detach().cpu() for n, p in m.named_parameters() if p.grad is not None}

    seen = {}

    class Spy(PerceptualLoss_dino):
        def forward(self, input, target):
            seen["y0"], seen["gt"] = input.detach().clone(), target.detach().clone()
            return super().forward(input, target)

    terms_on, grads_on = step(Spy(trunk=trunk_for(ref)))
    terms_off, grads_off = step(None)
    alone = PerceptualLoss_dino(trunk=trunk_for(ref))(seen["y0"], seen["gt"]).cpu()
    assert float(terms_on[2]) != 0.0 and same_bits(terms_on[2], alone * 0.5)
    # loss = (mse + dino) + col against (mse + col) + dino: the same three numbers per element, added in another order
    assert terms_on[0].shape == terms_off[0].shape
    assert float((terms_on[0] - (terms_off[0] + terms_on[2])).abs().max()) <= 4 * ulp32(float(terms_on[0].abs().max()))
    assert float(terms_off[2]) == 0.0 and all(same_bits(terms_on[i], terms_off[i]) for i in (1, 3, 4))
    assert list(grads_on) == list(grads_off) and all(torch.isfinite(v).all() for v in grads_on.values())
    assert sum(int(not torch.equal(grads_on[n], grads_off[n])) for n in grads_on) > len(grads_on) // 2
    # dino_loss=None is bit for bit the old result: a second run without the term repeats the first
    terms_again, grads_again = step(None)
    assert all(same_bits(a, b) for a, b in zip(terms_off, terms_again))
    assert all(same_bits(grads_off[n], grads_again[n]) for n in grads_off)
    # "native" builds the module on the trainer's model name
    tr = GaussianDiffusionTrainer(small_model(), 1e-4, 0.02, 1000, dino_loss="native").to(DEV)
    assert tr.loss_perceptual_dino.perceptual.cls_token.is_cuda and not any(k.startswith("loss_perceptual") for k in tr.model.state_dict())


# ------------------------------------------------------------------------------------------------------------ the driver
def as_is(image):
    return {"image": torch.from_numpy(np.ascontiguousarray(image)).permute(2, 0, 1)}


def test_driver_passes_the_keys_and_resumes_bit_for_bit(tmp_path):
    """Train.train with dino_loss="native" (dinov2_vits14, random weights from the run's seed) at 32 x 32: the term is recorded, the
    checkpoints hold the model alone, and an interrupted and resumed run equals the uninterrupted one."""
    from PIL import Image
    from hdiff_amd.diffusion import Train as TR
    root = tmp_path / "data"
    rng = np.random.default_rng(9)
    for sub, ext, count in (("Train/low", "jpg", 2), ("Train/high", "jpg", 2), ("Test/low", "jpg", 2), ("Test/high", "jpg", 2),
                            ("Train/trainA_paired", "png", 2), ("Train/trainB_paired", "png", 2), ("Test/testA", "png", 2),
                            ("Test/testB", "png", 2)):
        os.makedirs(root / sub)
        for i in range(count):
            low = rng.integers(0, 256, (4, 4, 3), dtype=np.uint8)
            Image.fromarray(low).resize((32, 32), Image.BILINEAR).save(str(root / sub / f"img{i}.{ext}"))

    def config(out, **kw):
        base = dict(underwater_data_name="HICRD", atmospheric_data_name="LoLI", dataset_root=str(root), transforms=as_is, T=1000, channel=32,
                    channel_mult=[1, 2, 2], num_res_blocks=1, dropout=0.15, lr=1e-4, multiplier=2.5, beta_1=1e-4, beta_T=0.02, grad_clip=1.0,
                    batch_size=2, epochs_stage_1=2, epochs_stage_2=2, save_checkpoint=1, output_path=str(out), pretrained_path=None,
                    device_list=[DEV], num_workers=0, seed=3, ema_decay=0.9, max_val_batches=0, dino_loss="native", dino_weights=None)
        base.update(kw)
        return types.SimpleNamespace(**base)

    def tensors(out):
        ck = os.path.join(str(out), "ckpt")
        load = lambda n: torch.load(os.path.join(ck, n), map_location="cpu", weights_only=False)
        return load(TR.final_name(4, "HICRD", "LoLI")), load(TR.final_name(4, "HICRD", "LoLI", ema=True)), load(TR.STATE_FILE)

    full = TR.train(config(tmp_path / "full"))
    assert full["finished"] and all(v > 0 for v in full["losses"]["perceptual_dino"])
    part = TR.train(config(tmp_path / "run", max_epochs=2))
    assert not part["finished"]
    rest = TR.train(config(tmp_path / "run", resume=os.path.join(str(tmp_path / "run"), "ckpt", TR.STATE_FILE)))
    assert rest["finished"] and rest["losses"] == full["losses"]
    (fa, ea, sa), (fb, eb, sb) = tensors(tmp_path / "full"), tensors(tmp_path / "run")
    assert list(fa) == list(fb) and all(torch.equal(fa[k], fb[k]) for k in fa) and all(torch.equal(ea[k], eb[k]) for k in ea)
    from hdiff_amd.diffusion.Model import DynamicUNet
    plain = DynamicUNet(T=1000, ch=32, ch_mult=[1, 2, 2], num_res_blocks=1, dropout=0.15)
    assert list(fa) == list(plain.state_dict()) and list(ea) == list(plain.state_dict())       # the trunk is in no checkpoint ...
    assert len(sa["ema"]["shadow"]) == len(list(plain.parameters()))                            # ... nor in the EMA
    assert len(sa["ema"]["shadow"]) == len(sb["ema"]["shadow"]) and all(torch.equal(x, y) for x, y in zip(sa["ema"]["shadow"], sb["ema"]["shadow"]))
    assert sorted(os.listdir(os.path.join(str(tmp_path / "full"), "ckpt"))) == TR.expected_files(config(tmp_path / "full"))


# --------------------------------------------------------------------------------------------------------- full width, once
def test_full_width_vits14_at_256():
    torch.manual_seed(0)
    trunk = dino.DinoV2Features("dinov2_vits14")
    sd = {k: v.detach().clone() for k, v in trunk.state_dict().items()}
    trunk = trunk.to(DEV)
    g = torch.Generator().manual_seed(1)
    xa, xb = torch.rand(1, 3, 256, 256, generator=g) / 255.0, torch.rand(1, 3, 256, 256, generator=g) * 2 - 1       # the trainer's ranges
    feats = trunk(xa.to(DEV))
    assert len(feats) == 124 and tuple(feats[2].shape) == (1, 384, 325) and tuple(feats[-1].shape) == (1, 384)
    x = xa.to(DEV).requires_grad_(True)
    loss = dino.dino_perceptual(trunk, x, xb.to(DEV))
    loss.backward()
    assert torch.isfinite(loss) and torch.isfinite(x.grad).all() and x.grad.abs().max() > 0
    with torch.no_grad():
        v64 = float(D.loss(sd, xa, xb, 6, 12))
        v32 = float(D.loss(sd, xa, xb, 6, 12, torch.float32))
    yard, err = abs(v32 - v64) / v64, abs(float(loss) - v64) / v64
    gate = max(YARD * yard, ulp32(v64) / v64)
    print(f"dinov2_vits14 256 x 256: loss {float(loss)!r} float64 {v64!r} rel err {err:.3e} (fp32 CPU {yard:.3e}, gate {gate:.3e})")
    assert err <= gate
