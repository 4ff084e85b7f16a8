"""Train-mode dropout fused into the GroupNorm-Swish conv (hdiff_dropout_keep_bits, hdiff_conv2d_fwd_dropout,
hdiff_conv2d_wgrad_dropout, hdiff_gn_swish_dropout_bwd and autograd.fused_conv(..., drop_p=)).

Reference of every error-class test: float64 on the GPU, the mask taken from hdiff_dropout_mask.  Baseline, measured in the same
test on the same inputs: the composite of the existing C entries that the fused form replaces (hdiff_gn_swish_apply ->
hdiff_dropout_mask -> hdiff_mul -> the conv / weight gradient without prologue; hdiff_gn_swish_bwd fed dA * mask).  Gate
(the ratios fixed for convolutions): rms error against float64 at most 1.5x the baseline's, worst element
at most 2x.  Every case runs in both contraction modes.
"""
import ctypes as C
import gc
import math

import pytest
import torch
import torch.nn.functional as F

import hdiff_amd
from hdiff_amd import _capi, autograd as A, engine as E

pytestmark = pytest.mark.gpu
both_modes = pytest.mark.parametrize("hdiff_contract", ("f32", "bf16x3"), indirect=True)

DEV = "cuda:0"
G = 32           # GroupNorm groups


def _s():
    return torch.cuda.current_stream().cuda_stream


def f32(v):
    return C.c_float(v).value


def inv_keep_of(keep):
    """the fp32 1.0f / keep that dropout_mask_kernel uses as its scale"""
    return f32(1.0 / f32(keep))


def dropout_mask(n, keep, seed, offset=0):
    m = torch.empty(n, device=DEV)
    _capi.check(_capi.lib().hdiff_dropout_mask(m.data_ptr(), n, C.c_float(keep), C.c_uint64(seed), C.c_uint64(offset), _s()), "mask")
    return m


def keep_bits(n, keep, seed, offset=0, before=0, after=0, fill=0):
    """ceil(n / 32) words, as a slice out of a larger buffer whose other words hold `fill`"""
    nw = (n + 31) // 32
    buf = torch.full((before + nw + after,), fill, dtype=torch.int32, device=DEV)
    words = buf[before:before + nw]
    _capi.check(_capi.lib().hdiff_dropout_keep_bits(words.data_ptr(), n, C.c_float(keep), C.c_uint64(seed), C.c_uint64(offset), _s()),
                "keep_bits")
    return words, buf


def unpack(words, n):
    sh = torch.arange(32, device=words.device, dtype=torch.int32)
    return ((words.view(-1, 1) >> sh) & 1).reshape(-1)[:n].bool()


# ----------------------------------------------------------------------------------------------------------------------
# 1. bits are the mask
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 7])
@pytest.mark.parametrize("seed", [1, 0x9E3779B97F4A7C15])
@pytest.mark.parametrize("keep", [0.5, 0.85, 1.0])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 4097, (1 << 20) + 5])
def test_keep_bits_are_the_mask(n, keep, seed, offset):
    mask = dropout_mask(n, keep, seed, offset)
    words, buf = keep_bits(n, keep, seed, offset, before=3, after=3, fill=0x5A5A5A5A)
    torch.cuda.synchronize()
    assert torch.equal(unpack(words, n), mask > 0)
    all_bits = unpack(words, 32 * words.numel())
    assert not all_bits[n:].any(), "unused bits of the last word must be 0"
    assert (buf[:3] == 0x5A5A5A5A).all() and (buf[-3:] == 0x5A5A5A5A).all(), "words outside ceil(n / 32) were written"
    if keep == 1.0:
        assert all_bits[:n].all()
    kept = mask[mask > 0]
    if kept.numel():
        assert kept.min().item() == kept.max().item() == inv_keep_of(keep)       # the scale the fused entries are handed


# ----------------------------------------------------------------------------------------------------------------------
# float64 references (plain matrix products: nothing here depends on a convolution library's float64 support)
# ----------------------------------------------------------------------------------------------------------------------
def gn_swish_f64(x, gamma, beta):
    B, Cc, H, W = x.shape
    xg = x.double().view(B, G, -1)
    mu, var = xg.mean(dim=2, keepdim=True), xg.var(dim=2, unbiased=False, keepdim=True)
    y = ((xg - mu) / torch.sqrt(var + 1e-5)).view(B, Cc, H, W) * gamma.double().view(1, -1, 1, 1) + beta.double().view(1, -1, 1, 1)
    return y * torch.sigmoid(y)


def conv3x3_f64(a, w, b=None):
    B, Cc, H, W = a.shape
    ap = F.pad(a, (1, 1, 1, 1))
    out = torch.zeros(B, w.shape[0], H, W, dtype=torch.float64, device=a.device)
    for ky in range(3):
        for kx in range(3):
            out += torch.einsum("oc,bchw->bohw", w[:, :, ky, kx].double(), ap[:, :, ky:ky + H, kx:kx + W])
    if b is not None:
        out += b.double().view(1, -1, 1, 1)
    return out


def wgrad3x3_f64(a, dy):
    B, Cc, H, W = a.shape
    ap = F.pad(a, (1, 1, 1, 1))
    dw = torch.empty(dy.shape[1], Cc, 3, 3, dtype=torch.float64, device=a.device)
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = torch.einsum("bohw,bchw->oc", dy.double(), ap[:, :, ky:ky + H, kx:kx + W])
    return dw


def rms(got, want):
    return (got.double() - want).pow(2).mean().sqrt().item()


def worst(got, want):
    return (got.double() - want).abs().max().item()


def gate(what, fused, base, want):
    r_f, r_b, w_f, w_b = rms(fused, want), rms(base, want), worst(fused, want), worst(base, want)
    print(f"{what}: rms vs float64 fused {r_f:.3e} composite {r_b:.3e} (x{r_f / max(r_b, 1e-300):.3f}); "
          f"worst fused {w_f:.3e} composite {w_b:.3e} (x{w_f / max(w_b, 1e-300):.3f})")
    assert r_f <= 1.5 * r_b, (what, r_f, r_b)
    assert w_f <= 2.0 * w_b, (what, w_f, w_b)


def make_case(C0, cout, H, W, B, seed):
    g = torch.Generator().manual_seed(seed)
    chan = torch.exp(torch.randn(1, C0, 1, 1, generator=g) * 1.0)
    x = (torch.randn(B, C0, H, W, generator=g) * chan + torch.randn(1, C0, 1, 1, generator=g) * 2).to(DEV)
    gamma = (torch.rand(C0, generator=g) * 1.5 + 0.25).to(DEV)
    beta = (torch.randn(C0, generator=g) * 0.5).to(DEV)
    w = (torch.randn(cout, C0, 3, 3, generator=g) / math.sqrt(C0 * 9)).to(DEV)
    b = torch.randn(cout, generator=g).to(DEV)
    return g, x, gamma, beta, w, b


def composite_activation(x, scale, shift, mask):
    """today's materialised tensor: gn_swish_apply -> (the mask) -> mul"""
    B, Cc, H, W = x.shape
    a = torch.empty_like(x)
    lib = _capi.lib()
    _capi.check(lib.hdiff_gn_swish_apply(x.data_ptr(), scale.data_ptr(), shift.data_ptr(), a.data_ptr(), B, Cc, H * W, _s()), "apply")
    _capi.check(lib.hdiff_mul(a.data_ptr(), mask.data_ptr(), a.data_ptr(), a.numel(), _s()), "mul")
    return a


def conv_fwd(x, w, b, out_shape, *, gn=None, act_range=None, dropout=None, residual=None):
    B, Cc, H, W = x.shape
    taps = E.conv_taps(3, 1)
    out = torch.empty(out_shape, device=DEV)
    A._run_conv(x, None, [(w, 0, taps.ky, taps.kx, 0)], taps, int(w.shape[0]), Cc, b, out, B=B, H=H, W=W, VH=H, VW=W, gn=gn,
                residual=residual, x3=(w, False), act_range=act_range, dropout=dropout)
    return out


# (C0, cout, H, W, B, residual epilogue, pairs): the dropout convs of the two default runs (256x256 / batch 2 and 32x32 / batch 80),
# one 20x40 plane, planes that start in the middle of a bit word (36 elements), a small launch (split-K in the f32 mode), planes four
# pixels wide (the 20-slot staging configuration of the fp32 kernel); pairs = False: the bf16-triple form in the bf16x3 mode
FWD_CASES = [
    (128, 128, 256, 256, 2, False, True), (256, 256, 128, 128, 2, False, True), (256, 256, 64, 64, 2, False, True),
    (256, 256, 32, 32, 2, True, True),
    (128, 128, 32, 32, 80, False, True), (256, 256, 32, 32, 80, False, True), (128, 128, 16, 16, 80, False, True),
    (256, 256, 16, 16, 80, True, True), (256, 256, 8, 8, 80, False, True), (256, 256, 4, 4, 80, False, True),
    (128, 128, 20, 40, 8, False, True), (32, 32, 6, 6, 3, True, True), (256, 256, 8, 8, 2, False, True),
    (32, 64, 256, 4, 2, False, True), (32, 32, 256, 4, 1, False, True),
    (256, 256, 32, 32, 80, False, False), (128, 128, 20, 40, 8, True, False), (64, 64, 64, 64, 16, False, False),
]


@both_modes
@pytest.mark.parametrize("C0,cout,H,W,B,res,pairs", FWD_CASES)
def test_fused_dropout_forward_error_class(C0, cout, H, W, B, res, pairs, hdiff_contract):
    keep, seed = 0.85, 1234 + C0 + H
    g, x, gamma, beta, w, b = make_case(C0, cout, H, W, B, seed)
    residual = torch.randn(B, cout, H, W, generator=g).to(DEV) if res else None
    n = x.numel()
    mask = dropout_mask(n, keep, seed).view_as(x)
    bits, _ = keep_bits(n, keep, seed)
    scale, shift, _, _ = A._gn_stats(x, None, gamma, beta, B, H * W)
    act_range = (gamma, beta, (C0 // G) * H * W, 1.0 / keep) if pairs else None
    shape = (B, cout, H, W)
    fused = conv_fwd(x, w, b, shape, gn=(scale, shift), act_range=act_range, dropout=(bits, inv_keep_of(keep)), residual=residual)
    base = conv_fwd(composite_activation(x, scale, shift, mask), w, b, shape, act_range=act_range, residual=residual)
    want = conv3x3_f64(gn_swish_f64(x, gamma, beta) * mask.double(), w, b)
    if res:
        want = want + residual.double()
    torch.cuda.synchronize()
    assert torch.isfinite(fused).all()
    undropped = conv_fwd(x, w, b, shape, gn=(scale, shift), act_range=act_range, residual=residual)
    assert worst(undropped, want) > 100 * worst(fused, want), "the reference does not tell a dropped input from an undropped one"
    gate(f"fwd {C0}->{cout} {H}x{W} B{B} {hdiff_contract} pairs={pairs}", fused, base, want)


# ----------------------------------------------------------------------------------------------------------------------
# 3. weight gradient and GroupNorm-Swish backward
# ----------------------------------------------------------------------------------------------------------------------
# wgrad3x3_applicable (W % 32 == 0, Cout % 128 == 0): the first three; the generic kernel: 16x16, 4x4, 20x40, 6x6
BWD_CASES = [(128, 128, 32, 32, 8), (256, 256, 64, 64, 2), (128, 128, 256, 256, 1), (256, 256, 16, 16, 16), (256, 256, 4, 4, 80),
             (128, 128, 20, 40, 4), (32, 32, 6, 6, 3)]


def run_wgrad(x, gn, dy, cout, dropout):
    B, Cc, H, W = x.shape
    taps = E.conv_taps(3, 1)
    dw = torch.empty(cout, Cc, 3, 3, device=DEV)
    A._run_wgrad(x, None, gn, dy, taps, cout, Cc, B=B, H=H, W=W, VH=H, VW=W, targets=[(dw, 0, taps.ky, taps.kx, 0)], dropout=dropout)
    return dw


@both_modes
@pytest.mark.parametrize("C0,cout,H,W,B", BWD_CASES)
def test_fused_dropout_weight_gradient_error_class(C0, cout, H, W, B, hdiff_contract):
    keep, seed = 0.85, 77 + C0 + W
    g, x, gamma, beta, w, b = make_case(C0, cout, H, W, B, seed)
    dy = torch.randn(B, cout, H, W, generator=g).to(DEV)
    n = x.numel()
    mask = dropout_mask(n, keep, seed).view_as(x)
    bits, _ = keep_bits(n, keep, seed)
    scale, shift, _, _ = A._gn_stats(x, None, gamma, beta, B, H * W)
    dropout = (bits, inv_keep_of(keep))
    fused = run_wgrad(x, (scale, shift), dy, cout, dropout)
    again = run_wgrad(x, (scale, shift), dy, cout, dropout)
    base = run_wgrad(composite_activation(x, scale, shift, mask), None, dy, cout, None)
    want = wgrad3x3_f64(gn_swish_f64(x, gamma, beta) * mask.double(), dy)
    torch.cuda.synchronize()
    assert torch.equal(fused, again), "two calls with the same inputs must be bitwise equal"
    undropped = run_wgrad(x, (scale, shift), dy, cout, None)
    assert worst(undropped, want) > 100 * worst(fused, want)
    gate(f"wgrad {C0}->{cout} {H}x{W} B{B}", fused, base, want)


def run_gn_bwd(x, dA, mean, rstd, gamma, beta, dropout):
    B, Cc, H, W = x.shape
    lib = _capi.lib()
    dx, dg, db = torch.empty_like(x), torch.empty_like(gamma), torch.empty_like(beta)
    ws = torch.empty(2 * B * Cc + 2 * B * G, device=DEV)
    if dropout is not None:
        _capi.check(lib.hdiff_gn_swish_dropout_bwd(x.data_ptr(), Cc, B, H * W, G, dA.data_ptr(), dropout[0].data_ptr(),
                                                   C.c_float(dropout[1]), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
                                                   beta.data_ptr(), ws.data_ptr(), dx.data_ptr(), dg.data_ptr(), db.data_ptr(), _s()),
                    "gn_swish_dropout_bwd")
    else:
        _capi.check(lib.hdiff_gn_swish_bwd(x.data_ptr(), None, Cc, 0, B, H * W, G, dA.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                           gamma.data_ptr(), beta.data_ptr(), ws.data_ptr(), dx.data_ptr(), None, dg.data_ptr(),
                                           db.data_ptr(), _s()), "gn_swish_bwd")
    return dx, dg, db


@both_modes
@pytest.mark.parametrize("C0,cout,H,W,B", BWD_CASES)
def test_fused_dropout_groupnorm_swish_backward_error_class(C0, cout, H, W, B, hdiff_contract):
    keep, seed = 0.85, 91 + C0 + W
    g, x, gamma, beta, w, b = make_case(C0, cout, H, W, B, seed)
    dA = torch.randn(B, C0, H, W, generator=g).to(DEV)
    n = x.numel()
    mask = dropout_mask(n, keep, seed).view_as(x)
    bits, _ = keep_bits(n, keep, seed)
    _, _, mean, rstd = A._gn_stats(x, None, gamma, beta, B, H * W)
    fused = run_gn_bwd(x, dA, mean, rstd, gamma, beta, (bits, inv_keep_of(keep)))
    again = run_gn_bwd(x, dA, mean, rstd, gamma, beta, (bits, inv_keep_of(keep)))
    dA_masked = torch.empty_like(dA)
    _capi.check(_capi.lib().hdiff_mul(dA.data_ptr(), mask.data_ptr(), dA_masked.data_ptr(), n, _s()), "mul")
    base = run_gn_bwd(x, dA_masked, mean, rstd, gamma, beta, None)
    xd, gd, bd = x.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    (gn_swish_f64(xd, gd, bd) * mask.double() * dA.double()).sum().backward()
    torch.cuda.synchronize()
    for name, f, a2, bs, want in zip(("dx", "dgamma", "dbeta"), fused, again, base, (xd.grad, gd.grad, bd.grad)):
        assert torch.equal(f, a2), name
        gate(f"gn-swish bwd {name} {C0} {H}x{W} B{B}", f, bs, want)


# ----------------------------------------------------------------------------------------------------------------------
# 4. autograd
# ----------------------------------------------------------------------------------------------------------------------
def close(got, ref, rel, abs_=1e-6, what=""):
    got, ref = got.detach().double(), ref.detach().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs().max().item()
    tol = rel * ref.abs().max().item() + abs_
    print(f"{what}: max err {err:.3e}, tol {tol:.3e}")
    assert err <= tol, f"{what}: max err {err:.3e} > tol {tol:.3e} (ref max {ref.abs().max().item():.3e})"


@both_modes
@pytest.mark.parametrize("C0,cout,H,W,B,s", [(32, 64, 16, 16, 2, 5), (128, 128, 32, 32, 2, 6), (256, 256, 16, 16, 24, 7),
                                             (128, 128, 64, 64, 4, 8)])
def test_fused_conv_with_dropout_matches_float64_autograd(C0, cout, H, W, B, s, hdiff_contract):
    """Tolerances: those of tests/test_gpu_backward.py::test_fused_conv_backward for the same op without dropout."""
    drop_p = 0.25
    g, x, gamma, beta, w, b = make_case(C0, cout, H, W, B, 300 + s)
    sc = torch.randn(B, cout, H, W, generator=g).to(DEV)
    dout = torch.randn(B, cout, H, W, generator=g).to(DEV)
    ins = [t.clone().requires_grad_(True) for t in (x, w, b, gamma, beta, sc)]
    torch.manual_seed(s)
    y = A.fused_conv(ins[0], None, ins[1], ins[2], ins[3], ins[4], residual=ins[5], k=3, drop_p=drop_p)
    y.backward(dout)
    # the seed as fused_conv draws it, and the mask it stands for
    torch.manual_seed(s)
    seed = int(torch.empty((), dtype=torch.int64).random_().item())
    mask = dropout_mask(x.numel(), 1.0 - drop_p, seed).view_as(x)
    ref = [t.double().clone().requires_grad_(True) for t in (x, w, b, gamma, beta, sc)]
    a = gn_swish_f64(ref[0], ref[3], ref[4]) * mask.double()
    y_ref = conv3x3_f64(a, ref[1], ref[2]) + ref[5]
    y_ref.backward(dout.double())
    close(y, y_ref, rel=3e-5, what="fwd")
    for name, t, r in zip(("dx", "dW", "dbias", "dgamma", "dbeta", "dres"), ins, ref):
        close(t.grad, r.grad, rel=1e-4 if name in ("dgamma", "dbeta", "dW") else 5e-5, what=name)


@both_modes
def test_fused_conv_without_dropout_runs_no_dropout_code(hdiff_contract):
    """drop_p = 0: bitwise the plain hdiff_conv2d_fwd with the same prologue."""
    C0, cout, H, W, B = 128, 128, 32, 32, 8
    g, x, gamma, beta, w, b = make_case(C0, cout, H, W, B, 17)
    sc = torch.randn(B, cout, H, W, generator=g).to(DEV)
    y = A.fused_conv(x, None, w, b, gamma, beta, residual=sc, k=3, drop_p=0.0)
    scale, shift, _, _ = A._gn_stats(x, None, gamma, beta, B, H * W)
    direct = conv_fwd(x, w, b, (B, cout, H, W), gn=(scale, shift), act_range=(gamma, beta, (C0 // G) * H * W, 1.0), residual=sc)
    assert torch.equal(y, direct)
    torch.manual_seed(3)
    assert not torch.equal(A.fused_conv(x, None, w, b, gamma, beta, residual=sc, k=3, drop_p=0.25), y)


# ----------------------------------------------------------------------------------------------------------------------
# 5. nothing is materialised
# ----------------------------------------------------------------------------------------------------------------------
def test_forward_keeps_bits_not_tensors():
    """What the forward leaves allocated, output alive: the output, ceil(n / 32) words of keep bits and a few kilobytes of
    per-(sample, channel) statistics -- arithmetic bound bytes(out) + bytes(x) / 8.  (A materialised mask and activation are
    2 * bytes(x).)"""
    g, x, gamma, beta, w, b = make_case(128, 128, 64, 64, 2, 23)
    ins = [t.requires_grad_(True) for t in (x, w, b, gamma, beta)]
    torch.manual_seed(1)
    A.fused_conv(ins[0], None, ins[1], ins[2], ins[3], ins[4], k=3, drop_p=0.15)     # first-use allocations of the library
    gc.collect()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    y = A.fused_conv(ins[0], None, ins[1], ins[2], ins[3], ins[4], k=3, drop_p=0.15)
    gc.collect()
    torch.cuda.synchronize()
    kept = torch.cuda.memory_allocated() - before
    nbytes = lambda t: t.numel() * t.element_size()
    print(f"kept {kept} bytes; out {nbytes(y)}, x {nbytes(x)}")
    assert kept <= nbytes(y) + nbytes(x) // 8, (kept, nbytes(y), nbytes(x))
    y.sum().backward()
    assert all(torch.isfinite(t.grad).all() for t in ins)


# ----------------------------------------------------------------------------------------------------------------------
# 6. hostile input
# ----------------------------------------------------------------------------------------------------------------------
def test_out_of_range_statistics_stay_loud_behind_the_dropout(hdiff_contract):
    """gn_scale / gn_shift that are not statistics of x (tests/test_gpu_ops.py, the out-of-range-is-loud case) through the dropout
    entry with keep = 1, so that nothing is dropped: inf / NaN, never a finite wrong number.  (The fp16-pair form: bf16x3 mode.)"""
    before = hdiff_amd.get_contraction_mode()
    hdiff_amd.set_contraction_mode("bf16x3")
    try:
        g = torch.Generator().manual_seed(12)
        B, Cc, H, W = 16, 64, 64, 64
        x = torch.randn(B, Cc, H, W, generator=g).to(DEV)
        gamma, beta = torch.ones(Cc, device=DEV), torch.zeros(Cc, device=DEV)
        w = (torch.randn(Cc, Cc, 3, 3, generator=g) / math.sqrt(Cc * 9)).to(DEV)
        bits, _ = keep_bits(x.numel(), 1.0, 5)
        scale, shift, _, _ = A._gn_stats(x, None, gamma, beta, B, H * W)
        act_range = (gamma, beta, (Cc // G) * H * W, 1.0)
        good = conv_fwd(x, w, None, (B, Cc, H, W), gn=(scale, shift), act_range=act_range, dropout=(bits, 1.0))
        plain = conv_fwd(x, w, None, (B, Cc, H, W), gn=(scale, shift), act_range=act_range)
        assert torch.isfinite(good).all() and torch.equal(good, plain)       # keep = 1: times 1.0f, every element kept
        scale.mul_(1.0e4)                  # "statistics" of some other tensor: values up to 4e4 where the bound says 128
        bad = conv_fwd(x, w, None, (B, Cc, H, W), gn=(scale, shift), act_range=act_range, dropout=(bits, 1.0))
        torch.cuda.synchronize()
        assert torch.isnan(bad).any()
        assert not torch.isfinite(bad).all()
    finally:
        hdiff_amd.set_contraction_mode(before)


@both_modes
@pytest.mark.parametrize("C0,cout,H,W,B", [(64, 128, 64, 64, 16), (32, 32, 6, 6, 3), (128, 128, 20, 40, 4)])
def test_nothing_outside_the_bit_slice_is_used(C0, cout, H, W, B, hdiff_contract):
    """The ceil(n / 32) words as a slice out of the middle of a larger buffer whose other words are all zeros in one run and all
    ones in the next: forward, weight gradient and GroupNorm-Swish backward are bitwise the same."""
    keep, seed = 0.85, 4
    g, x, gamma, beta, w, b = make_case(C0, cout, H, W, B, 55)
    dy = torch.randn(B, cout, H, W, generator=g).to(DEV)
    dA = torch.randn(B, C0, H, W, generator=g).to(DEV)
    scale, shift, mean, rstd = A._gn_stats(x, None, gamma, beta, B, H * W)
    act_range = (gamma, beta, (C0 // G) * H * W, 1.0 / keep)
    outs = []
    for fill in (0, -1):
        bits, buf = keep_bits(x.numel(), keep, seed, before=1021, after=1027, fill=fill)
        dropout = (bits, inv_keep_of(keep))
        y = conv_fwd(x, w, b, (B, cout, H, W), gn=(scale, shift), act_range=act_range, dropout=dropout)
        dw = run_wgrad(x, (scale, shift), dy, cout, dropout)
        dx, dg, db = run_gn_bwd(x, dA, mean, rstd, gamma, beta, dropout)
        torch.cuda.synchronize()
        assert (buf[:1021] == fill).all() and (buf[-1027:] == fill).all()
        outs.append((y, dw, dx, dg, db))
    for a, c in zip(*outs):
        assert torch.equal(a, c)
