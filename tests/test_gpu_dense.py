"""The token-axis dense layer on the GPU (hdiff_amd/dense.py, csrc/dense_tokens.hip) and the DINOv2 trunk on it (dense="tokens").

Gates.  The operator: error against the float64 definition at most 4x that of torch's fp32 CPU F.linear on the same inputs, rms and max
(tests/test_dense_cpu.py shows that this gate passes the kernel's arithmetic and fails it with any one piece product left out); nothing
outside x is read into a product, nothing outside y is written; dgrad, repeats, batch members, graph replays: bit for bit.  The trunk: the
gates of tests/test_gpu_dino.py's whole-trunk test, whose float64 reference is shared.  Everything runs in the "bf16x3" mode unless it says
otherwise; every figure is printed before it is asserted.
"""
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _dense_def as DD  # noqa: E402
import _dino_def as D  # noqa: E402
import test_gpu_dino as TD  # noqa: E402  (reference(), run(), ulp32: the whole-trunk test's own definitions and its cached float64 reference)
import hdiff_amd  # noqa: E402
from hdiff_amd import _capi, dense, dino  # noqa: E402
from hdiff_amd.Loss.loss import PerceptualLoss_dino  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]
DEV = "cuda:0"
YARD = 4.0
SENTINEL = -7777.25


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


@pytest.fixture(autouse=True)
def bf16x3():
    before = hdiff_amd.get_contraction_mode()
    hdiff_amd.set_contraction_mode("bf16x3")
    try:
        yield
    finally:
        hdiff_amd.set_contraction_mode(before)


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def launch_inside_buffers(x, w, bias):
    """The C entry on x and y that are slices of larger buffers -- x's filled with NaN, y's with a sentinel, more than a tile (64 channel
    rows and 64 tokens) on both sides, the slices only 4-byte aligned -> y, and whether both paddings of y kept the sentinel"""
    B, Cin, L = x.shape
    Cout = w.shape[0]
    pad = 64 * L + 2049
    xbuf = torch.full((2 * pad + x.numel(),), float("nan"), device=DEV)
    ybuf = torch.full((2 * pad + B * Cout * L,), SENTINEL, device=DEV)
    xbuf[pad:pad + x.numel()] = x.reshape(-1).to(DEV)
    wd = w.to(DEV)
    wp = torch.empty(dense.pack_words(Cout, Cin), dtype=torch.int32, device=DEV)
    lib = hdiff_amd.lib()
    _capi.check(lib.hdiff_dense_pack(wd.data_ptr(), wp.data_ptr(), Cout, Cin, 0, stream()), "dense_pack")
    bd = None if bias is None else bias.to(DEV)
    _capi.check(lib.hdiff_dense_tokens(xbuf.data_ptr() + 4 * pad, wp.data_ptr(), None if bd is None else bd.data_ptr(),
                                       ybuf.data_ptr() + 4 * pad, B, Cin, Cout, L, stream()), "dense_tokens")
    torch.cuda.synchronize()
    out = ybuf.cpu()
    y = out[pad:pad + B * Cout * L].view(B, Cout, L).clone()
    untouched = bool((out[:pad] == SENTINEL).all()) and bool((out[pad + B * Cout * L:] == SENTINEL).all())
    return y, untouched


# ------------------------------------------------------------------------------------------------------------------ the operator
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("shape", DD.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_operator_against_float64_inside_nan_and_sentinel_padding(shape, with_bias):
    w, bias, x = DD.case(*shape)
    bias = bias if with_bias else None
    ref = DD.linear64(x, w, bias)
    yr, ym = DD.errors(DD.yardstick(x, w, bias), ref)
    got, untouched = launch_inside_buffers(x, w, bias)
    finite = bool(torch.isfinite(got).all())
    er, em = DD.errors(got, ref) if finite else (float("nan"), float("nan"))
    print(f"{shape} bias {with_bias}: rms {er:.3e} max {em:.3e}; fp32 CPU rms {yr:.3e} max {ym:.3e}; ratios {er / yr:.2f} {em / ym:.2f}; "
          f"padding untouched {untouched}, finite {finite}")
    assert untouched                                   # no store outside y
    assert finite                                      # no NaN from outside x reached a product
    assert er <= YARD * yr and em <= YARD * ym
    # the public entry on the same numbers: the same bits
    pub = dense.linear_tokens(x.to(DEV), w.to(DEV), None if bias is None else bias.to(DEV))
    assert same_bits(pub, got)


@pytest.mark.parametrize("shape", DD.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_dgrad_is_the_forward_on_the_transposed_weight(shape):
    B, Cout, Cin, L = shape
    w, _, _ = DD.case(*shape)
    g = torch.Generator().manual_seed(B + Cout + Cin + L)
    dy = torch.randn(B, Cout, L, generator=g).to(DEV)
    wd = w.to(DEV)
    dx = dense.linear_tokens_dgrad(dy, wd)
    want = dense.linear_tokens(dy, wd.t().contiguous())
    assert tuple(dx.shape) == (B, Cin, L) and same_bits(dx, want)
    ref = torch.einsum("oc,bol->bcl", w.double(), dy.cpu().double())
    yard = torch.einsum("oc,bol->bcl", w, dy.cpu())
    (er, em), (yr, ym) = DD.errors(dx.cpu(), ref), DD.errors(yard, ref)
    print(f"{shape} dgrad: rms {er:.3e} max {em:.3e}; fp32 CPU rms {yr:.3e} max {ym:.3e}; ratios {er / yr:.2f} {em / ym:.2f}")
    assert er <= YARD * yr and em <= YARD * ym


@pytest.mark.parametrize("shape", [(3, 65, 17, 33), (3, 130, 64, 325)], ids=lambda s: "x".join(str(v) for v in s))
def test_repeatable_and_an_image_does_not_depend_on_its_batch(shape):
    w, bias, x = DD.case(*shape)
    xd, wd, bd = x.to(DEV), w.to(DEV), bias.to(DEV)
    y = dense.linear_tokens(xd, wd, bd)
    assert same_bits(dense.linear_tokens(xd, wd, bd), y)
    for b in range(shape[0]):
        assert same_bits(dense.linear_tokens(xd[b:b + 1].contiguous(), wd, bd), y[b:b + 1])
    dy = y.contiguous()
    dx = dense.linear_tokens_dgrad(dy, wd)
    assert same_bits(dense.linear_tokens_dgrad(dy, wd), dx)
    for b in range(shape[0]):
        assert same_bits(dense.linear_tokens_dgrad(dy[b:b + 1].contiguous(), wd), dx[b:b + 1])


@pytest.mark.parametrize("shape,b,l", [((2, 72, 48, 65), 1, 33), ((3, 65, 17, 33), 0, 32), ((2, 8, 12, 5), 1, 0)])
def test_a_nan_stays_in_its_column(shape, b, l):
    w, bias, x = DD.case(*shape)
    wd, bd = w.to(DEV), bias.to(DEV)
    clean = dense.linear_tokens(x.to(DEV), wd, bd).cpu()
    x2 = x.clone()
    x2[b, shape[2] // 2, l] = float("nan")
    got = dense.linear_tokens(x2.to(DEV), wd, bd).cpu()
    assert torch.isnan(got[b, :, l]).all()
    keep = torch.ones(got.shape, dtype=torch.bool)
    keep[b, :, l] = False
    assert torch.equal(bits(got)[keep], bits(clean)[keep]) and torch.isfinite(got[keep]).all()


def test_legal_under_stream_capture():
    shape = (2, 130, 64, 325)
    w, bias, x = DD.case(*shape)
    wd, bd = w.to(DEV), bias.to(DEV)
    other = torch.randn(x.shape, generator=torch.Generator().manual_seed(5))
    eager = [dense.linear_tokens(v.to(DEV), wd, bd).cpu() for v in (x, other)]                  # also builds the pack
    eager_dx = [dense.linear_tokens_dgrad(e.to(DEV), wd).cpu() for e in eager]
    xin = x.to(DEV).clone()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        y = dense.linear_tokens(xin, wd, bd)
        dx = dense.linear_tokens_dgrad(y, wd)
    for src, want, want_dx in ((x, eager[0], eager_dx[0]), (other, eager[1], eager_dx[1]), (x, eager[0], eager_dx[0])):
        xin.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(y, want) and same_bits(dx, want_dx)


def test_a_weight_updated_in_place_is_packed_again():
    shape = (2, 72, 48, 65)
    w, bias, x = DD.case(*shape)
    cache = dense.PackCache()
    xd, wd = x.to(DEV), w.to(DEV)
    y0 = dense.linear_tokens(xd, wd, cache=cache).cpu()
    dx0 = dense.linear_tokens_dgrad(xd.new_ones(2, 72, 65), wd, cache=cache).cpu()
    assert len(cache) == 2 and cache.nbytes() == 4 * (dense.pack_words(72, 48) + dense.pack_words(48, 72))
    version = wd._version
    assert same_bits(dense.linear_tokens(xd, wd, cache=cache), y0) and len(cache) == 2          # a hit: nothing new
    w2 = DD.case(2, 72, 48, 66)[0]
    wd.copy_(w2.to(DEV))
    assert wd._version != version
    y1 = dense.linear_tokens(xd, wd, cache=cache).cpu()
    dx1 = dense.linear_tokens_dgrad(xd.new_ones(2, 72, 65), wd, cache=cache).cpu()
    assert len(cache) == 2                                                                      # the same two slots
    assert not same_bits(y1, y0) and not same_bits(dx1, dx0)
    fresh = dense.linear_tokens(xd, w2.to(DEV), cache=dense.PackCache()).cpu()
    assert same_bits(y1, fresh)
    ref = DD.linear64(x, w2)
    (er, em), (yr, ym) = DD.errors(y1, ref), DD.errors(DD.yardstick(x, w2), ref)
    assert er <= YARD * yr and em <= YARD * ym


def test_refusals_of_the_python_entry():
    x, w = torch.zeros(1, 4, 3, device=DEV), torch.zeros(5, 4, device=DEV)
    with pytest.raises(RuntimeError, match="channels"):
        dense.linear_tokens(torch.zeros(1, 3, 3, device=DEV), w)
    with pytest.raises(RuntimeError, match="contiguous"):
        dense.linear_tokens(x, torch.zeros(4, 5, device=DEV).t())
    with pytest.raises(RuntimeError, match="bias"):
        dense.linear_tokens(x, w, torch.zeros(4, device=DEV))
    with pytest.raises(RuntimeError, match=r"\(B, C, L\)"):
        dense.linear_tokens_dgrad(torch.zeros(5, 3, device=DEV), w)


# --------------------------------------------------------------------------------------------------------------------- the trunk
def trunk_for(ref, **kw):
    c = ref["c"]
    t = dino.DinoV2Features(embed_dim=c["embed"], depth=c["depth"], heads=c["heads"], pos_grid=c["pos_grid"], **kw)
    return t.load_dinov2(ref["sd"]).to(DEV)


@pytest.mark.parametrize("name", list(D.FIXTURES))
def test_whole_trunk_on_the_token_kernel_against_float64(name):
    ref = TD.reference(name)
    trunk = trunk_for(ref, dense="tokens")
    loss, per, grad = TD.run(trunk, ref["xa"], ref["xb"])
    assert len(trunk._packs) == 2 * (1 + 4 * ref["c"]["depth"])                     # every dense layer, forward and transposed
    v_err = abs(float(loss) - ref["v64"]) / ref["v64"]
    g_err = float((grad.double() - ref["g64"]).pow(2).mean().sqrt())
    gate = max(YARD * ref["yard_value"], TD.ulp32(ref["v64"]) / ref["v64"])
    print(f"{name} [tokens]: loss {float(loss)!r} float64 {ref['v64']!r} rel err {v_err:.3e} (fp32 CPU {ref['yard_value']:.3e}, gate {gate:.3e})"
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
    loss2, per2, grad2 = TD.run(trunk, ref["xa"], ref["xb"])
    assert same_bits(loss, loss2) and same_bits(per, per2) and same_bits(grad, grad2)
    # image 0 does not see image 1
    g = torch.Generator().manual_seed(77)
    xa2, xb2 = ref["xa"].clone(), ref["xb"].clone()
    xa2[1], xb2[1] = torch.randn(xa2[1].shape, generator=g), torch.randn(xb2[1].shape, generator=g)
    loss3, per3, grad3 = TD.run(trunk, xa2, xb2)
    assert same_bits(per[0], per3[0]) and same_bits(grad[0], grad3[0]) and not same_bits(per[1], per3[1])
    # it is another program than the conv route, and the loss module runs it
    conv = TD.run(trunk_for(ref), ref["xa"], ref["xb"])
    assert not same_bits(conv[2], grad)
    mod = PerceptualLoss_dino(trunk=trunk)
    x = ref["xa"].to(DEV).requires_grad_(True)
    v = mod(x, ref["xb"].to(DEV))
    v.backward()
    assert same_bits(v, loss) and same_bits(x.grad, grad) and same_bits(mod.last_per_image, per)


def test_trunk_forward_and_backward_on_the_token_kernel_under_stream_capture():
    ref = TD.reference("e32")
    trunk = trunk_for(ref, dense="tokens")
    eager_loss, _, eager_grad = TD.run(trunk, ref["xa"], ref["xb"])            # also fills the position-embedding cache and the packs
    other = torch.randn(ref["xa"].shape, generator=torch.Generator().manual_seed(5))
    other_loss, _, other_grad = TD.run(trunk, other, ref["xb"])
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


def test_f32_mode_and_the_default_run_the_conv_route_bit_for_bit():
    ref = TD.reference("e32")
    tokens, conv, default = trunk_for(ref, dense="tokens"), trunk_for(ref, dense="conv"), trunk_for(ref)
    assert default.dense == "conv"
    a, b = TD.run(default, ref["xa"], ref["xb"]), TD.run(conv, ref["xa"], ref["xb"])            # bf16x3
    assert all(same_bits(u, v) for u, v in zip(a, b)) and len(default._packs) == 0 and len(conv._packs) == 0
    hdiff_amd.set_contraction_mode("f32")                                                        # (the fixture restores the mode)
    a, b = TD.run(tokens, ref["xa"], ref["xb"]), TD.run(conv, ref["xa"], ref["xb"])
    assert all(same_bits(u, v) for u, v in zip(a, b)) and len(tokens._packs) == 0
    hdiff_amd.set_contraction_mode("f16")
    TD.run(tokens, ref["xa"], ref["xb"])
    assert len(tokens._packs) > 0                                                                # there the token kernel runs


def test_loss_module_and_trainer_with_the_token_kernel():
    """32 x 32 as tests/test_gpu_dino.py's trainer test: dinov2_vits14 with random weights on 5 tokens."""
    from hdiff_amd.diffusion.Diffusion import GaussianDiffusionTrainer
    ref = TD.reference("e32")
    mod = PerceptualLoss_dino(trunk=trunk_for(ref, dense="tokens"))
    x = ref["xa"].to(DEV).requires_grad_(True)
    v = mod(x, ref["xb"].to(DEV))
    v.backward()
    assert torch.isfinite(v) and torch.isfinite(x.grad).all() and x.grad.abs().max() > 0
    g = torch.Generator().manual_seed(11)
    gt, inp = (torch.randint(0, 256, (2, 3, 32, 32), generator=g, dtype=torch.uint8).to(DEV) for _ in range(2))
    t, noise = torch.tensor([704, 50], device=DEV), torch.randn(2, 3, 32, 32, generator=g).to(DEV)
    m = TD.small_model()
    tr = GaussianDiffusionTrainer(m, 1e-4, 0.02, 1000, dino_loss="native", dino_dense="tokens").to(DEV)
    assert tr.loss_perceptual_dino.perceptual.dense == "tokens" and tr.loss_perceptual_dino.perceptual.cls_token.is_cuda
    terms = tr(gt, inp, 0, t=t, noise=noise, context_zero=False)
    terms[0].mean().backward()
    assert all(torch.isfinite(v).all() for v in terms) and float(terms[2]) > 0.0
    assert len(tr.loss_perceptual_dino.perceptual._packs) == 2 * 49
    grads = [p.grad for p in m.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(v).all() for v in grads)
    assert not any(k.startswith("loss_perceptual") for k in tr.model.state_dict())               # the checkpoint holds the model alone
