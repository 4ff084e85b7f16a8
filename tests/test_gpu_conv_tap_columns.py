"""conv3x3_x3.hip walks its taps column by column: a patch row is read from LDS once per tap column and feeds every (tap row,
output row) pair that needs it.  What can go wrong is an index: (patch row, tap row, tap column, tap of the pack).

1. One-hot weights: ONE tap of the kernel is 2^k, everything else 0, the input a sparse field of powers of two.  Every output
   is one exact product, so the result equals the shifted input bit for bit, for every tap in turn and for every tap rectangle
   the launcher has: 3x3 (plain conv), 3x3 / 3x2 / 2x3 / 2x2 with an output map (UpSample's four phases) and with a strided input
   (DownSample's four parity planes).
2. Geometry: planes of 4x32, 5x33, 9x40, 16x64 (a wave without a valid row, with one valid row, edge tiles both ways), 16 / 32 / 48
   input channels (one chunk, two, three), a concat seam at 16 | 32, 64 / 80 / 128 output channels, with and without bias /
   vector / residual, plus 16x128 x 128 channels whose eight pixel tiles take the kernel's XCD remap.
   The dispatcher gives the kernel launches of at least 192 workgroups only, and these planes are one to eight tiles: the batch
   is the smallest that reaches the kernel (every case asserts that it did), never below 2.
3. Error class against float64 with the gates of tests/test_gpu_ops.py and tests/test_gpu_conv_range.py, through their own entry
   points: pairs behind GroupNorm, pairs by range word (UpSample, DownSample), triples.
4. Train-mode dropout in the prologue against float64 with the same keep mask.

Tolerance of 2 and 4: 1e-5 of max |ref| (+1e-6), the gate of _check_conv3x3_pairs / _check_conv3x3_split."""
import ctypes as C
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import hdiff_amd  # noqa: E402
from hdiff_amd import _capi, autograd as A, engine as E  # noqa: E402
import test_gpu_conv_range as RNG  # noqa: E402
import test_gpu_fused_dropout as DRP  # noqa: E402
import test_gpu_ops as OPS  # noqa: E402

DEV = "cuda:0"


@pytest.fixture(autouse=True)
def split_mode():
    before = hdiff_amd.get_contraction_mode()
    hdiff_amd.set_contraction_mode("bf16x3")
    try:
        yield
    finally:
        hdiff_amd.set_contraction_mode(before)


def blocks(cout, H, W, B):
    return OPS._split_launch_blocks(cout, H, W, B)


def smallest_batch(cout, H, W):
    per = blocks(cout, H, W, 1)
    return max(2, -(-192 // per))


X3_TRIPLES, X3_PAIRS_WORD = 3, 5          # HDIFF_CONV_ROUTE_* (include/hdiff.h)


def route_of_recorded_conv(plan):
    """the route the library gives the plan's one recorded forward conv, asked with the very descriptor the launch used"""
    (name, _, args), = [op for op in plan.ops if op[0] in ("hdiff_conv2d_fwd", "hdiff_conv2d_fwd_range")]
    d, r = args[0], (args[1] if name == "hdiff_conv2d_fwd_range" else None)
    route, tail = C.c_int(-1), C.c_int(-1)
    rc = hdiff_amd.lib().hdiff_conv2d_fwd_route(d, r, 0, C.byref(route), C.byref(tail))
    assert rc == 0, hdiff_amd.lib().hdiff_last_error().decode()
    return route.value


def conv_by_word(x0, x1, w, b, vec, res, form, check_route=True):
    """plain 3x3 through the plan: form = 'word' (fp16 pairs staged by the sample's range word) or 'triples'; the route is asserted,
    so that a fall from pairs to triples (or to the fp32 kernel), which passes every tolerance, fails here"""
    plan = E.Plan(DEV)
    B, C0, H, W = x0.shape
    dg = lambda t: None if t is None else t.to(DEV).contiguous()
    pk = E._std_pack(plan, w.to(DEV), 3, 1)
    out = plan.buf(B, w.shape[0], H, W)
    words = None
    if form == "word":
        xin = x0 if x1 is None else torch.cat([x0, x1], dim=1)
        words = RNG.words_of(xin.to(DEV))
    plan.conv(dg(x0), dg(x1), pk, dg(b), out, B=B, H=H, W=W, VH=H, VW=W, addvec=dg(vec), residual=dg(res), absmax_in=words)
    plan.pack_weights()
    plan.run()
    torch.cuda.synchronize()
    if check_route:
        assert route_of_recorded_conv(plan) == (X3_PAIRS_WORD if form == "word" else X3_TRIPLES), form
    return out.clone()


def sparse_powers(shape, seed):
    """about one element in 40 is +-2^e, e in [-3, 3]; the rest 0"""
    g = torch.Generator().manual_seed(seed)
    on = torch.rand(shape, generator=g) < 0.025
    e = torch.randint(-3, 4, shape, generator=g).float()
    s = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    return torch.where(on, s * torch.exp2(e), torch.zeros(shape))


# ---- 1. one-hot taps, exact --------------------------------------------------------------------------------------------------------
OH_C, OH_H, OH_W, OH_B = 16, 16, 1536, 2          # 2 x 48 tiles x 2 samples = 192 workgroups


def test_one_hot_taps_plain_3x3_exact():
    assert blocks(64, OH_H, OH_W, OH_B) == 192
    x = sparse_powers((OH_B, OH_C, OH_H, OH_W), 11)
    xd = F.pad(x.to(DEV), (1, 1, 1, 1))
    for form in ("word", "triples"):
        for ky in range(3):
            for kx in range(3):
                k = ky * 3 + kx - 4
                w = torch.zeros(64, OH_C, 3, 3)
                for co in range(64):
                    w[co, co % OH_C, ky, kx] = 2.0 ** k
                got = conv_by_word(x, None, w, None, None, None, form)
                want = (2.0 ** k) * xd[:, :, ky:ky + OH_H, kx:kx + OH_W].repeat(1, 4, 1, 1)
                assert torch.equal(got, want), (form, ky, kx, (got - want).abs().max().item())


def _identity3x3(Cc):
    w = torch.zeros(Cc, Cc, 3, 3)
    for c in range(Cc):
        w[c, c, 1, 1] = 1.0
    return w


def test_one_hot_taps_upsample_phases_exact():
    """ConvTranspose2d(5, stride 2, padding 2, output_padding 1): out[2 i - 2 + k] += x[i] w[k]; tap (ky, kx) belongs to phase
    (ky % 2, kx % 2), whose rectangle is 3x3, 3x2, 2x3 or 2x2.  UpSample's 3x3 behind it is the identity."""
    Cc, H, W, B = OH_C, OH_H, OH_W, OH_B
    x = sparse_powers((B, Cc, H, W), 12)
    xd = x.to(DEV)
    words = RNG.words_of(xd)
    zero = torch.zeros(Cc)
    iy, ix = torch.arange(H, device=DEV), torch.arange(W, device=DEV)
    for ky in range(5):
        for kx in range(5):
            k = (ky * 5 + kx) % 7 - 3
            wt = torch.zeros(Cc, Cc, 5, 5)
            for c in range(Cc):
                wt[c, c, ky, kx] = 2.0 ** k
            P = {"u.t.weight": wt, "u.t.bias": zero, "u.c.weight": _identity3x3(Cc), "u.c.bias": zero}
            got = RNG.run_up({n: v.to(DEV) for n, v in P.items()}, xd, words)
            oy, ox = 2 * iy - 2 + ky, 2 * ix - 2 + kx
            vy, vx = (oy >= 0) & (oy < 2 * H), (ox >= 0) & (ox < 2 * W)
            want = torch.zeros(B, Cc, 2 * H, 2 * W, device=DEV)
            want[:, :, oy[vy][:, None], ox[vx][None, :]] = (2.0 ** k) * xd[:, :, iy[vy][:, None], ix[vx][None, :]]
            assert torch.equal(got, want), (ky, kx, (got - want).abs().max().item())


def test_one_hot_taps_downsample_planes_exact():
    """5x5 / stride 2 / padding 2: out(y, x) = w(ky, kx) in(2 y + ky - 2, 2 x + kx - 2); tap (ky, kx) reads parity plane
    (ky % 2, kx % 2) of the input: 9, 6, 6 and 4 taps.  An odd input: the odd planes are one row / column shorter."""
    Cc, B = OH_C, OH_B
    H, W = 2 * OH_H - 1, 2 * OH_W - 1
    x = sparse_powers((B, Cc, H, W), 13)
    xd = x.to(DEV)
    words = RNG.words_of(xd)
    xp = F.pad(xd, (2, 3, 2, 3))
    zero = torch.zeros(Cc)
    for ky in range(5):
        for kx in range(5):
            k = (ky * 5 + kx) % 7 - 3
            w5 = torch.zeros(Cc, Cc, 5, 5)
            for c in range(Cc):
                w5[c, c, ky, kx] = 2.0 ** k
            P = {"d.c1.weight": torch.zeros(Cc, Cc, 3, 3), "d.c1.bias": zero, "d.c2.weight": w5, "d.c2.bias": zero}
            got = RNG.run_down({n: v.to(DEV) for n, v in P.items()}, xd, words)
            want = (2.0 ** k) * xp[:, :, ky:ky + 2 * OH_H:2, kx:kx + 2 * OH_W:2]
            assert got.shape == want.shape == (B, Cc, OH_H, OH_W)
            assert torch.equal(got, want), (ky, kx, (got - want).abs().max().item())


# ---- 2. geometry -------------------------------------------------------------------------------------------------------------------
# (H, W, C0, C1, cout, bias, vector, residual)
GEOMETRY = [(4, 32, 16, 0, 64, True, True, True), (4, 32, 16, 32, 128, False, False, False), (4, 32, 32, 0, 80, True, False, True),
            (5, 33, 32, 0, 80, True, True, True), (5, 33, 48, 0, 64, False, False, False), (5, 33, 16, 0, 128, False, True, False),
            (9, 40, 48, 0, 128, True, True, True), (9, 40, 16, 0, 80, False, False, False), (9, 40, 16, 32, 64, True, False, True),
            (16, 64, 16, 32, 64, True, True, True), (16, 64, 32, 0, 128, False, False, False), (16, 64, 48, 0, 80, False, True, False),
            (16, 128, 32, 0, 128, True, True, True)]


@pytest.fixture(scope="module")
def geometry_cases():
    """inputs and float64 references, computed once and never modified"""
    cases = {}
    for (H, W, C0, C1, cout, has_b, has_v, has_r) in GEOMETRY:
        B = smallest_batch(cout, H, W)
        g = torch.Generator().manual_seed(H * 1000 + W + C0 + cout)
        cin = C0 + C1
        x0 = torch.randn(B, C0, H, W, generator=g)
        x1 = torch.randn(B, C1, H, W, generator=g) if C1 else None
        w = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(cin * 9)
        b = torch.randn(cout, generator=g) if has_b else None
        vec = torch.randn(B, cout, generator=g) if has_v else None
        res = torch.randn(B, cout, H, W, generator=g) if has_r else None
        xin = (x0 if x1 is None else torch.cat([x0, x1], dim=1)).double()
        want = F.conv2d(xin, w.double(), None if b is None else b.double(), padding=1)
        if vec is not None:
            want = want + vec.double()[:, :, None, None]
        if res is not None:
            want = want + res.double()
        cases[(H, W, C0, C1, cout)] = (B, x0, x1, w, b, vec, res, want)
    return cases


@pytest.mark.parametrize("form", ["word", "triples"])
@pytest.mark.parametrize("H,W,C0,C1,cout,has_b,has_v,has_r", GEOMETRY)
def test_geometry_against_float64(H, W, C0, C1, cout, has_b, has_v, has_r, form, geometry_cases):
    B, x0, x1, w, b, vec, res, want = geometry_cases[(H, W, C0, C1, cout)]
    assert B >= 2 and blocks(cout, H, W, B) >= 192 and (B == 2 or blocks(cout, H, W, B - 1) < 192)
    if (H, W) == (16, 128):
        assert (-(-W // 32) * -(-H // 8)) % 8 == 0 and cout > 64, "the XCD remap needs eight tiles and two channel blocks"
    got = conv_by_word(x0, x1, w, b, vec, res, form)
    got_f32 = RNG.in_f32_mode(lambda: conv_by_word(x0, x1, w, b, vec, res, "triples", check_route=False))
    assert not torch.equal(got, got_f32), "the split-operand kernel did not run"
    OPS.close(got, want.float(), rel=1e-5, what=f"conv3x3 {form} {C0}+{C1}->{cout} {H}x{W} B={B}")


@pytest.mark.parametrize("H,W,C0,C1,cout", [(4, 32, 32, 0, 80), (5, 33, 32, 0, 80), (9, 40, 32, 32, 64), (16, 128, 32, 0, 128)])
def test_geometry_pairs_behind_groupnorm(H, W, C0, C1, cout):
    """the GroupNorm + Swish prologue (32 groups: channel counts that are multiples of 32) at the same planes"""
    B = smallest_batch(cout, H, W)
    g = torch.Generator().manual_seed(H + W + cout)
    cin = C0 + C1
    x0 = torch.randn(B, C0, H, W, generator=g)
    x1 = torch.randn(B, C1, H, W, generator=g) if C1 else None
    gamma, beta = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.5
    w = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(cin * 9)
    b, res = torch.randn(cout, generator=g), torch.randn(B, cout, H, W, generator=g)
    want = OPS._gn_swish_conv_f64(x0, x1, gamma, beta, w, b, None, res)
    got = OPS.run_conv_gn(x0, x1, gamma, beta, w, b, None, res)
    got_x3 = OPS.run_conv_gn(x0, x1, gamma, beta, w, b, None, res, pairs=False)
    assert not torch.equal(got, got_x3), "the fp16-pair kernel did not run"
    OPS.close(got, want.float(), rel=1e-5, what=f"conv3x3 pairs {cin}->{cout} {H}x{W} B={B}")
    OPS.close(got_x3, want.float(), rel=1e-5, what=f"conv3x3 triples {cin}->{cout} {H}x{W} B={B}")


# ---- 3. error class ----------------------------------------------------------------------------------------------------------------
def test_error_class_pairs_behind_groupnorm():
    """rms <= 1.5 x the fp32-MFMA kernel's, max <= 1e-5 of max |ref| (_check_conv3x3_pairs, unchanged)"""
    OPS._check_conv3x3_pairs(64, 32, 128, 16, 64, 24, _capi.lib())


def test_error_class_triples():
    OPS._check_conv3x3_split(64, 32, 128, 16, 64, 24, False, _capi.lib())
    OPS._check_conv3x3_split(32, 0, 64, 9, 40, 48, True, _capi.lib())


@pytest.mark.parametrize("kind", ["up", "down"])
def test_error_class_pairs_by_word(kind):
    """UpSample (four phases with an output map + its 3x3) and DownSample (four strided parity planes) staged by range words,
    samples 2^40 apart: per sample rms <= 1.5 x the f32 mode's (_gate_per_sample of tests/test_gpu_conv_range.py, unchanged)"""
    Cc, H, W = 32, 16, 1536
    assert blocks(Cc, H, W, 2) == 192
    if kind == "up":
        P, Pd = RNG.up_params(Cc, 21)
        x = RNG.ranged_input(2, Cc, H, W, 22)
        want, run = RNG.up_ref(P, x), RNG.run_up
    else:
        P, Pd = RNG.down_params(Cc, 23)
        x = RNG.ranged_input(2, Cc, 2 * H - 1, 2 * W - 1, 24)
        want, run = RNG.down_ref(P, x), RNG.run_down
    xd = x.to(DEV)
    got = run(Pd, xd, RNG.words_of(xd))
    got_f32 = RNG.in_f32_mode(lambda: run(Pd, xd))
    assert not torch.equal(got, got_f32), "the fp16-pair kernel did not run"
    RNG._gate_per_sample(got, got_f32, want, kind)
    for s in range(2):
        OPS.close(got[s], want[s].float(), rel=1e-5, abs_=0.0, what=f"{kind} sample {s}")


# ---- 4. dropout --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pairs", [True, False])
def test_dropout_fixed_mask_against_float64(pairs):
    C0, cout, H, W, B, keep, seed = 32, 64, 16, 64, 48, 0.85, 77
    assert blocks(cout, H, W, B) == 192
    g, x, gamma, beta, w, b = DRP.make_case(C0, cout, H, W, B, seed)
    mask = DRP.dropout_mask(x.numel(), keep, seed).view_as(x)
    bits, _ = DRP.keep_bits(x.numel(), keep, seed)
    scale, shift, _, _ = A._gn_stats(x, None, gamma, beta, B, H * W)
    act_range = (gamma, beta, (C0 // DRP.G) * H * W, 1.0 / keep) if pairs else None
    got = DRP.conv_fwd(x, w, b, (B, cout, H, W), gn=(scale, shift), act_range=act_range, dropout=(bits, DRP.inv_keep_of(keep)))
    undropped = DRP.conv_fwd(x, w, b, (B, cout, H, W), gn=(scale, shift), act_range=act_range)
    want = DRP.conv3x3_f64(DRP.gn_swish_f64(x, gamma, beta) * mask.double(), w, b)
    torch.cuda.synchronize()
    assert DRP.worst(undropped, want) > 100 * DRP.worst(got, want), "the reference does not tell a dropped input from an undropped one"
    OPS.close(got, want.float(), rel=1e-5, what=f"dropout conv pairs={pairs}")
