"""Per-sample range words (hdiff_conv2d_fwd_range): a producing kernel's epilogue leaves max |out[b]| in one word per sample, and the
fp16-pair form of the split-operand conv kernel takes its staging scale from such a word -- UpSample's four transposed-conv
phases and its 3x3, DownSample's 5x5 / stride 2 as four parity-plane convolutions.

Shapes: the split-operand kernels serve launches of at least 192 workgroups (64 channels x 8x32 pixels each), smaller ones keep the
fp32-input kernel; the cases here are the smallest that reach them with B = 2 -- 80 channels (a full and a partial 64-channel
block, five 16-channel chunks: both staging buffers and the two-ahead prefetch run) over 20 x 500 pixels (3 x 16 tiles, partial in
both directions) -- plus shapes below the threshold, which must take the other path and still fill the words.

Gate of the error-class tests (tests/test_gpu_ops.py, _check_upsample_phases): rms against float64 <= 1.5 x the f32-mode result's
rms + 1e-12."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import hdiff_amd  # noqa: E402
from hdiff_amd import engine as E  # noqa: E402

DEV = "cuda:0"
CC, PH, PW = 80, 20, 500          # channels and plane of the served Up / DownSample cases (see above)


@pytest.fixture(autouse=True)
def split_mode():
    before = hdiff_amd.get_contraction_mode()
    hdiff_amd.set_contraction_mode("bf16x3")
    try:
        yield
    finally:
        hdiff_amd.set_contraction_mode(before)


def in_f32_mode(fn):
    hdiff_amd.set_contraction_mode("f32")
    try:
        return fn()
    finally:
        hdiff_amd.set_contraction_mode("bf16x3")


def absmax_bits(t):
    """bits of max |t[b]| per sample, as the kernels leave them"""
    return t.detach().abs().flatten(1).amax(1).float().contiguous().view(torch.int32)


def words_of(x):
    """range words set by hand from a tensor on the device"""
    return absmax_bits(x).clone()


def rms(got, want):
    return (got.double().cpu() - want).pow(2).mean().sqrt().item()


def up_params(Cc, seed):
    g = torch.Generator().manual_seed(seed)
    P = {"u.t.weight": torch.randn(Cc, Cc, 5, 5, generator=g) / math.sqrt(Cc * 6.25), "u.t.bias": torch.randn(Cc, generator=g),
         "u.c.weight": torch.randn(Cc, Cc, 3, 3, generator=g) / math.sqrt(Cc * 9), "u.c.bias": torch.randn(Cc, generator=g)}
    return P, {k: v.to(DEV) for k, v in P.items()}


def down_params(Cc, seed):
    g = torch.Generator().manual_seed(seed)
    P = {"d.c1.weight": torch.randn(Cc, Cc, 3, 3, generator=g) / math.sqrt(Cc * 9), "d.c1.bias": torch.randn(Cc, generator=g),
         "d.c2.weight": torch.randn(Cc, Cc, 5, 5, generator=g) / math.sqrt(Cc * 25), "d.c2.bias": torch.randn(Cc, generator=g)}
    return P, {k: v.to(DEV) for k, v in P.items()}


def run_up(Pd, xd, words=None):
    B, Cc, H, W = xd.shape
    plan = E.Plan(DEV)
    y = E.emit_upsample(plan, Pd, "u", xd, B, Cc, H, W, x_absmax=words)
    plan.pack_weights()
    plan.run()
    torch.cuda.synchronize()
    return y.clone()


def run_down(Pd, xd, words=None):
    B, Cc, H, W = xd.shape
    plan = E.Plan(DEV)
    y = E.emit_downsample(plan, Pd, "d", xd, B, Cc, H, W, x_absmax=words)
    plan.pack_weights()
    plan.run()
    torch.cuda.synchronize()
    return y.clone()


def up_ref(P, x):
    u = F.conv_transpose2d(x.double(), P["u.t.weight"].double(), P["u.t.bias"].double(), stride=2, padding=2, output_padding=1)
    return F.conv2d(u, P["u.c.weight"].double(), P["u.c.bias"].double(), padding=1)


def down_ref(P, x):
    return F.conv2d(x.double(), P["d.c1.weight"].double(), P["d.c1.bias"].double(), stride=2, padding=1) + \
        F.conv2d(x.double(), P["d.c2.weight"].double(), P["d.c2.bias"].double(), stride=2, padding=2)


def ranged_input(B, Cc, H, W, seed):
    """sample 0 x 2^-20, sample 1 x 2^20, channels spanning 2^12"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cc, H, W, generator=g)
    x *= torch.exp2(12.0 * torch.arange(Cc) / (Cc - 1)).view(1, Cc, 1, 1)
    x[0] *= 2.0 ** -20
    x[1] *= 2.0 ** 20
    return x


# ---- the cases with a float64 reference, computed once (never modified) ---------------------------------------------------------
@pytest.fixture(scope="module")
def up_case():
    P, Pd = up_params(CC, 1)
    x = ranged_input(2, CC, PH, PW, 2)
    return P, Pd, x, up_ref(P, x)


@pytest.fixture(scope="module")
def down_case():
    """an odd 39 x 999 input: the planes with an odd row / column offset are one row / column shorter (output 20 x 500)"""
    P, Pd = down_params(CC, 3)
    x = ranged_input(2, CC, 2 * PH - 1, 2 * PW - 1, 4)
    return P, Pd, x, down_ref(P, x)


# ---- 1. the epilogue word is exact ---------------------------------------------------------------------------------------------
def _producer_plan(kind, scale):
    """One producer launch with absmax_out; sample 1's input is 2^10 larger than sample 0's (a launch-wide maximum would fail)."""
    g = torch.Generator().manual_seed(11)
    plan = E.Plan(DEV)
    B = 2
    words = plan.range_words(B)

    def inp(C_, H, W):
        x = torch.randn(B, C_, H, W, generator=g) * scale
        x[1] *= 2.0 ** 10
        return x.to(DEV)

    if kind == "pair3x3_gn_residual":            # 64 -> 96 (GroupNorm has 32 groups) over 44 x 250: 6 x 8 tiles x 2 channel blocks x 2 = 192 workgroups
        Cin, Cout, H, W = 64, 96, 44, 250
        x, res = inp(Cin, H, W), inp(Cout, H, W)
        w = (torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)).to(DEV)
        gamma, beta = (1 + 0.1 * torch.randn(Cin, generator=g)).to(DEV), (0.1 * torch.randn(Cin, generator=g)).to(DEV)
        sc = plan.gn_scale_shift(x, None, gamma, beta, B, H * W)
        pk = E._std_pack(plan, w, 3, 1)
        out = plan.buf(B, Cout, H, W)
        plan.conv(x, None, pk, None, out, B=B, H=H, W=W, VH=H, VW=W, gn=sc, residual=res, absmax_out=words)
        written = lambda: out
    elif kind in ("triple_phase", "four_phases"):
        Cc, H, W = CC, PH, PW
        x = inp(Cc, H, W)
        wt = (torch.randn(Cc, Cc, 5, 5, generator=g) / math.sqrt(Cc * 6.25)).to(DEV)
        bias = torch.randn(Cc, generator=g).to(DEV)
        u = plan.buf(B, Cc, 2 * H, 2 * W)
        plan.keep(u)
        phases = [(0, 1)] if kind == "triple_phase" else [(0, 0), (0, 1), (1, 0), (1, 1)]
        for py, px in phases:
            taps = E.tconv_phase_taps(py, px)
            pk = E._new_pack(plan, Cc, Cc, taps)
            pk.add_source(wt, 1, taps.ky, taps.kx, 0)
            pk.enable_x3_taps(wt, 1)
            plan.conv(x, None, pk, bias, u, B=B, H=H, W=W, VH=H, VW=W, out_map=(2, py, 2, px), absmax_out=words)
        written = (lambda: u[:, :, 0::2, 1::2]) if kind == "triple_phase" else (lambda: u)
    elif kind in ("conv1x1_x3", "conv1x1_small"):      # 128 x 128: the split-operand 1x1 GEMM; 16 x 16: below its threshold
        Cin, Cout, H, W = 32, 96, (128 if kind == "conv1x1_x3" else 16), (128 if kind == "conv1x1_x3" else 16)
        x = inp(Cin, H, W)
        w = (torch.randn(Cout, Cin, 1, 1, generator=g) / math.sqrt(Cin)).to(DEV)
        pk = E._std_pack(plan, w, 1, 0)
        out = plan.buf(B, Cout, H, W)
        plan.conv(x, None, pk, None, out, B=B, H=H, W=W, VH=H, VW=W, absmax_out=words)
        written = lambda: out
    else:                                        # "splitk": 128 -> 64 over 8 x 8, a small grid with a long channel loop
        assert kind == "splitk"
        Cin, Cout, H, W = 128, 64, 8, 8
        x = inp(Cin, H, W)
        w = (torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)).to(DEV)
        pk = E._std_pack(plan, w, 3, 1)
        out = plan.buf(B, Cout, H, W)
        plan.conv(x, None, pk, None, out, B=B, H=H, W=W, VH=H, VW=W, absmax_out=words)
        written = lambda: out
    plan.pack_weights()
    return plan, x, words, written


@pytest.mark.parametrize("kind", ["pair3x3_gn_residual", "triple_phase", "four_phases", "conv1x1_x3", "conv1x1_small", "splitk"])
def test_epilogue_word_is_the_exact_sample_maximum(kind):
    plan, x, words, written = _producer_plan(kind, 1.0)
    plan.run()
    torch.cuda.synchronize()
    big = words.clone()
    want = absmax_bits(written())
    assert torch.equal(big, want), (kind, big.tolist(), want.tolist())
    assert big[1] > big[0]                                   # per sample, not per launch
    # the same plan on smaller inputs: the smaller word (the plan zeroes its words before the first producer)
    x.mul_(2.0 ** -3)
    plan.run()
    torch.cuda.synchronize()
    want = absmax_bits(written())
    assert torch.equal(words, want), (kind, words.tolist(), want.tolist())
    if kind != "pair3x3_gn_residual":                        # (GroupNorm takes the scale out again)
        assert (words < big).all()


# ---- 2. / 3. error class and range ---------------------------------------------------------------------------------------------
def _gate_per_sample(got, got_f32, want, what):
    for b in range(want.shape[0]):
        r, r32 = rms(got[b], want[b]), rms(got_f32[b], want[b])
        print(f"{what} sample {b}: rms vs float64: pairs by word {r:.3e}, fp32-MFMA {r32:.3e} (output rms {want[b].pow(2).mean().sqrt().item():.3e})")
        assert r <= 1.5 * r32 + 1e-12, (what, b, r, r32)


def test_upsample_by_word_error_class_and_range(up_case):
    P, Pd, x, want = up_case
    xd = x.to(DEV)
    got = run_up(Pd, xd, words_of(xd))
    got_f32 = in_f32_mode(lambda: run_up(Pd, xd, words_of(xd)))
    assert not torch.equal(got, got_f32), "another program must have run"
    assert not torch.equal(got, run_up(Pd, xd)), "with the word the phases leave the bf16 triples"
    _gate_per_sample(got, got_f32, want, "upsample")


def test_downsample_by_word_error_class_and_range(down_case):
    P, Pd, x, want = down_case
    xd = x.to(DEV)
    got = run_down(Pd, xd, words_of(xd))
    got_f32 = in_f32_mode(lambda: run_down(Pd, xd, words_of(xd)))
    assert not torch.equal(got, got_f32), "another program must have run"
    assert torch.equal(run_down(Pd, xd), got_f32), "without the word the 5x5 / stride 2 keeps the fp32-input kernel"
    _gate_per_sample(got, got_f32, want, "downsample")


@pytest.mark.parametrize("H,W,B", [(32, 32, 2), (17, 23, 2)])
def test_downsample_small_planes(H, W, B):
    """Below the split-operand kernel's threshold (and an odd plane): served or not, the result is right."""
    P, Pd = down_params(32, 5)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(B, 32, H, W, generator=g)
    xd = x.to(DEV)
    want = down_ref(P, x)
    got = run_down(Pd, xd, words_of(xd))
    got_f32 = in_f32_mode(lambda: run_down(Pd, xd, words_of(xd)))
    _gate_per_sample(got, got_f32, want, f"downsample {H}x{W}")


def test_zero_sample_gives_exactly_the_bias(down_case):
    P, Pd, x, _ = down_case
    xd = x.to(DEV).clone()
    xd[0].zero_()
    got = run_down(Pd, xd, words_of(xd))
    bias = (Pd["d.c1.bias"] + Pd["d.c2.bias"]).view(-1, 1, 1)
    assert torch.equal(got[0], bias.expand_as(got[0]))
    assert torch.isfinite(got[1]).all()


def test_inf_stays_in_its_sample(up_case, down_case):
    for (P, Pd, x, _), run in ((up_case, run_up), (down_case, run_down)):
        xd = x.to(DEV).clone()
        clean = run(Pd, xd, words_of(xd))
        xd[0, 3, 7, 11] = float("inf")
        got = run(Pd, xd, words_of(xd))
        assert torch.isnan(got[0]).any() and not torch.isfinite(got[0]).all()
        assert torch.equal(got[1], clean[1])


def test_understated_word_is_loud(up_case, down_case):
    """A word 2^6 below the true maximum: the fp16 conversion overflows, every output that value reaches is NaN -- and what is
    finite is still right (never a finite wrong value; 1e-5 of the sample's largest output, the op-level tolerance of
    tests/test_gpu_ops.py for these convolutions)."""
    for (P, Pd, x, want), run in ((up_case, run_up), (down_case, run_down)):
        xd = x.to(DEV)
        low = absmax_bits(xd * 2.0 ** -6).clone()
        got = run(Pd, xd, low).cpu().double()
        assert not torch.isinf(got).any()
        for b in range(2):
            nan = torch.isnan(got[b])
            assert nan.any(), b
            err = (got[b] - want[b])[~nan].abs()
            assert err.numel() == 0 or err.max().item() <= 1e-5 * want[b].abs().max().item() + 1e-6, b


# ---- 4. batch independence -----------------------------------------------------------------------------------------------------
def test_a_sample_does_not_depend_on_its_batch():
    """20 x 1000 (Up) / 40 x 2000 (Down): 192 workgroups per launch already at B = 1, so both batch sizes run the same kernels."""
    H, W = PH, 2 * PW
    x = ranged_input(2, CC, H, W, 7).to(DEV)
    _, Pu = up_params(CC, 8)
    both = run_up(Pu, x, words_of(x))
    for b in range(2):
        alone = run_up(Pu, x[b:b + 1].contiguous(), words_of(x[b:b + 1]))
        assert torch.equal(both[b], alone[0]), ("upsample", b)
    x = ranged_input(2, CC, 2 * H, 2 * W, 9).to(DEV)
    _, Pdn = down_params(CC, 10)
    both = run_down(Pdn, x, words_of(x))
    assert not torch.equal(both, in_f32_mode(lambda: run_down(Pdn, x, words_of(x))))
    for b in range(2):
        alone = run_down(Pdn, x[b:b + 1].contiguous(), words_of(x[b:b + 1]))
        assert torch.equal(both[b], alone[0]), ("downsample", b)


# ---- 5. / 6. a plan: producer -> words -> consumers ----------------------------------------------------------------------------
class _Chain:
    """xin -> 3x3 conv (its epilogue fills the words of x) -> UpSample(x) and DownSample(x), each with the words or without"""

    def __init__(self, wired, H=2 * PH, W=2 * PW):
        g = torch.Generator().manual_seed(21)
        B, Cc = 2, CC
        plan = E.Plan(DEV)
        self.plan, self.xin = plan, plan.buf(B, Cc, H, W)
        w = (torch.randn(Cc, Cc, 3, 3, generator=g) / math.sqrt(Cc * 9)).to(DEV)
        _, Pu = up_params(Cc, 22)
        _, Pdn = down_params(Cc, 23)
        words = plan.range_words(B) if wired else None
        x = self.x = plan.buf(B, Cc, H, W)
        plan.conv(self.xin, None, E._std_pack(plan, w, 3, 1), None, x, B=B, H=H, W=W, VH=H, VW=W, absmax_out=words)
        self.up = E.emit_upsample(plan, Pu, "u", x, B, Cc, H, W, x_absmax=words)
        self.down = E.emit_downsample(plan, Pdn, "d", x, B, Cc, H, W, x_absmax=words)
        plan.keep((w, Pu, Pdn, x))
        plan.pack_weights()
        torch.cuda.synchronize()

    def outputs(self):
        torch.cuda.synchronize()
        return self.up.clone(), self.down.clone()


def _chain_input(scale):
    return (ranged_input(2, CC, 2 * PH, 2 * PW, 24) * scale).to(DEV)


def test_replay_starts_from_zeroed_words():
    a, small = _chain_input(1.0), _chain_input(2.0 ** -8)
    eager = _Chain(True)
    eager.xin.copy_(a)
    eager.plan.run()
    want_a = eager.outputs()
    graph = _Chain(True)
    graph.xin.copy_(a)
    graph.plan.capture()
    graph.plan.replay()
    got_a = graph.outputs()
    assert all(torch.equal(g_, w_) for g_, w_ in zip(got_a, want_a)), "graph != eager"
    graph.xin.copy_(small)
    graph.plan.replay()
    got_small = graph.outputs()
    fresh = _Chain(True)
    fresh.xin.copy_(small)
    fresh.plan.run()
    want_small = fresh.outputs()
    assert all(torch.equal(g_, w_) for g_, w_ in zip(got_small, want_small)), "a replay saw the words of the run before it"
    assert all(torch.isfinite(t).all() for t in got_small)
    # the words matter: without them the same chain computes other bits
    plain = _Chain(False)
    plain.xin.copy_(small)
    plain.plan.run()
    assert not any(torch.equal(g_, w_) for g_, w_ in zip(plain.outputs(), want_small))


def test_f32_mode_ignores_the_words():
    x = _chain_input(1.0)

    def run(wired):
        c = _Chain(wired)
        c.xin.copy_(x)
        c.plan.run()
        return c.outputs()

    with_words, without = in_f32_mode(lambda: run(True)), in_f32_mode(lambda: run(False))
    assert all(torch.equal(a, b) for a, b in zip(with_words, without))


def test_default_plan_route_histogram():
    """Which kernel each conv of the default model's plan runs on, asked of hdiff_conv2d_fwd_route for every kept descriptor -- the
    plan is built, not run.  128 x 128 with B = 2 is the smallest shape at which level 0 passes 192 workgroups (3x3: 64 tiles x
    2 channel blocks x 2 samples = 256; 1x1: 32 768 pixels) while every deeper level, the tail (one channel block: 128) and every
    Up / DownSample but the last UpSample's 3x3 (512) stay below.  The literals are what the predicate cascade of the commit before
    the route function answers for these same descriptors (profiles/conv_route_refactor.txt, section 5), that is per kernel:
    conv_igemm_kernel 77, conv3x3_x3_kernel<.., PAIR> 11, conv1x1_x3_kernel 7, conv_out_absmax_kernel 17; f32 mode:
    conv_igemm_kernel 88, conv1x1_direct_kernel 7.  Of the 11 pair launches one takes its range from a word (UpSample's 3x3 at
    level 0), ten from a GroupNorm (the 3x3 convs of level 0's two down and three up blocks)."""
    import collections
    import ctypes as C
    from hdiff_amd import _capi
    from hdiff_amd.DiffusionFreeGuidence.ModelCondition import UNet, _params_of
    m = UNet(T=500, num_labels=10, ch=128, ch_mult=[1, 2, 2, 2], num_res_blocks=2, dropout=0.15).to(DEV).eval()
    plan = E.UNetPlan(_params_of(m), m._shape, 2, 128, 128, torch.device(DEV)).plan
    convs = [k for k in plan._keep if isinstance(k, tuple) and k and isinstance(k[0], _capi.ConvDesc)]
    assert len(convs) == sum(name.startswith("hdiff_conv2d_fwd") for name, _, _ in plan.ops) == 95

    def histogram():
        hist, tails = collections.Counter(), 0
        for kept in convs:
            r = next((v for v in kept if isinstance(v, _capi.ConvRange)), None)
            route, tail = C.c_int(-1), C.c_int(-1)
            _capi.check(plan.lib.hdiff_conv2d_fwd_route(C.byref(kept[0]), None if r is None else C.byref(r), 0, C.byref(route),
                                                        C.byref(tail)), "conv2d_fwd_route")
            hist[route.value] += 1
            tails += tail.value
        return dict(hist), tails

    IGEMM, DIRECT_1X1, X3_1X1, X3_PAIRS_GN, X3_PAIRS_WORD = 0, 1, 2, 4, 5
    assert histogram() == ({IGEMM: 77, X3_1X1: 7, X3_PAIRS_GN: 10, X3_PAIRS_WORD: 1}, 17)
    assert in_f32_mode(histogram) == ({IGEMM: 88, DIRECT_1X1: 7}, 0)
