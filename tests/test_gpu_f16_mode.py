"""The opt-in "f16" contraction mode on the GPU (csrc/attention_f16.hip): the attention forward of inference on single fp16 pieces.

Yardstick: tests/_f16_attention_emul.py, an emulation of the FORMAT in float64 (never of the kernel), evaluated at the offsets k / 8
of the softmax reference inside a binade; the largest error over the offsets is the bound the kernel is held to, with the margins the
project uses for a kernel against its error class (1.25x rms, 2x worst; tests/test_gpu_ops.py).  Each test sets the mode itself and
restores the one it found."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import hdiff_amd  # noqa: E402
from hdiff_amd import _capi  # noqa: E402
import _f16_attention_emul as EM  # noqa: E402
from test_gpu_ops import MHA_H2_PAIRS, MHA_X3P_PAIRS, _flash, _flash_route, _h2_case, run_conv  # noqa: E402

DEV = "cuda:0"
GOLDEN = os.path.join(HERE, "golden")
H2_SEEDS = {"ramp": 1, "peaked": 2, "late-spikes": 3, "wide-v": 4, "tiny-v": 5, "quiet-neighbour": 6}


@pytest.fixture
def f16_mode():
    """the library in the f16 mode; the mode found is restored"""
    before = hdiff_amd.get_contraction_mode()
    hdiff_amd.set_contraction_mode("f16")
    yield _capi.lib()
    hdiff_amd.set_contraction_mode(before)


def _in_mode(mode, fn):
    before = hdiff_amd.get_contraction_mode()
    hdiff_amd.set_contraction_mode(mode)
    try:
        return fn()
    finally:
        hdiff_amd.set_contraction_mode(before)


def _gate(what, qkv, heads, out):
    """kernel error against float64 <= 1.25x (rms) / 2x (worst) of the yardstick, over all (sample, head) pairs and per pair"""
    d_qkv = qkv.to(DEV)
    ref = EM.exact(d_qkv, heads)
    y_rms, y_worst, y_rms_p, y_worst_p = EM.yardstick(d_qkv, heads, ref=ref)
    k_rms, k_worst, k_rms_p, k_worst_p = EM.errors(out, ref, per_pair_heads=heads)
    print(f"f16 {what}: kernel rms {k_rms:.3e} worst {k_worst:.3e} | yardstick rms {y_rms:.3e} worst {y_worst:.3e} | "
          f"ratio {k_rms / y_rms:.3f} / {k_worst / y_worst:.3f} | worst pair ratio "
          f"{max(a / b for a, b in zip(k_rms_p, y_rms_p)):.3f} / {max(a / b for a, b in zip(k_worst_p, y_worst_p)):.3f}")
    assert torch.isfinite(out).all(), what
    assert k_rms <= 1.25 * y_rms and k_worst <= 2.0 * y_worst, (what, k_rms, y_rms, k_worst, y_worst)
    for i, (a, b, c, e) in enumerate(zip(k_rms_p, y_rms_p, k_worst_p, y_worst_p)):
        assert a <= 1.25 * b and c <= 2.0 * e, (what, "pair", i, a, b, c, e)


def _case(name, d, L, B, heads=8):
    if name in H2_SEEDS:
        assert B == 1
        return _h2_case(name, d, L, torch.Generator().manual_seed(H2_SEEDS[name]))
    g = torch.Generator().manual_seed(1000 + d + L)
    qkv = torch.randn(B, 3 * heads * d, L, generator=g)
    if name == "x3":
        qkv[:, :2 * heads * d] *= 3.0
    elif name == "x0.05":
        qkv[:, :2 * heads * d] *= 0.05
    else:
        assert name == "gauss"
    return qkv


CASES = ([("gauss", 512, 2), ("gauss", 4096, 2), ("gauss", 16384, 1), ("x3", 4096, 1), ("x0.05", 4096, 1)] +
         [(n, 4096, 1) for n in H2_SEEDS])


# ---- 1. the kernel against the yardstick ------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [16, 32])
@pytest.mark.parametrize("name,L,B", CASES, ids=[f"{n}-L{L}-B{B}" for n, L, B in CASES])
def test_f16_kernel_within_the_format_error(name, L, B, d, f16_mode):
    qkv = _case(name, d, L, B)
    out, _ = _flash(f16_mode, qkv, 8, workspace=True)
    _gate(f"{name} d={d} L={L} B={B}", qkv, 8, out)


def test_f16_kernel_one_pair_at_L65536(f16_mode):
    """one whole (sample, head) at the longest sequence of a 256x256 forward, d_head 16"""
    g = torch.Generator().manual_seed(65536)
    qkv = torch.randn(1, 3 * 16, 65536, generator=g)
    out, _ = _flash(f16_mode, qkv, 1, workspace=True)
    _gate("gauss d=16 L=65536 one pair", qkv, 1, out)


# ---- 2. the rows stay in the kernel ------------------------------------------------------------------------------------------
def test_f16_keeps_every_row_in_the_kernel():
    """The _h2_case inputs with the check pass switched off (HDIFF_NO_CHECK_PASS, read once per process): no NaN anywhere -- the
    moving reference kept every P inside fp16, no row was handed to the fp32 kernel."""
    code = r'''
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch, hdiff_amd
import test_gpu_ops as T
lib = hdiff_amd.lib()
assert hdiff_amd.get_contraction_mode() == "f16"
for d in (16, 32):
    for i, name in enumerate(["ramp", "peaked", "late-spikes", "wide-v", "tiny-v", "quiet-neighbour"]):
        qkv = T._h2_case(name, d, 4096, torch.Generator().manual_seed(i + 1))
        o, _ = T._flash(lib, qkv, 8, workspace=True)
        assert torch.isfinite(o).all(), (name, d)
        ref = T.attention_core_ref(qkv, 8)
        # half-precision operands, and the rows are the kernel's own: far from the 1e-6 class, far from garbage
        assert ((o.cpu() - ref).abs().amax(dim=2) <= 0.1 * ref.abs().amax(dim=2) + 1e-30).all(), (name, d)
print("F16_ROWS_OK")
''' % (ROOT, HERE)
    env = dict(os.environ, HDIFF_NO_CHECK_PASS="1", HDIFF_CONTRACT="f16")
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0 and "F16_ROWS_OK" in res.stdout, res.stdout[-1500:] + res.stderr[-3000:]


# ---- 3. it is another program --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [16, 32])
def test_f16_is_another_program(d, f16_mode):
    """Same inputs in bf16x3 and f16: the outputs differ and the f16 error against float64 is at least 50x the pair kernels'
    (a dispatch that quietly ran the pair kernel fails here)."""
    lib = f16_mode
    qkv = _case("gauss", d, 4096, 2)
    o16, _ = _flash(lib, qkv, 8, workspace=True)
    ox3, _ = _in_mode("bf16x3", lambda: _flash(lib, qkv, 8, workspace=True))
    assert hdiff_amd.get_contraction_mode() == "f16"
    assert _flash_route(lib, qkv, 8, workspace=True) == 5      # HDIFF_MHA_FWD_ROUTE_F16_SINGLE
    assert not torch.equal(o16, ox3)
    ref = EM.exact(qkv.to(DEV), 8)
    e16, ex3 = EM.errors(o16, ref)[0], EM.errors(ox3, ref)[0]
    print(f"f16 / bf16x3 rms error against float64, d={d}: {e16:.3e} / {ex3:.3e} = {e16 / ex3:.0f}x")
    assert e16 >= 50.0 * ex3, (e16, ex3)


# ---- 4. everything else is untouched -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [16, 32])
def test_f16_forward_with_lse_is_the_default_forward(d, f16_mode):
    lib = f16_mode
    qkv = _case("gauss", d, 1024, 2)
    o16, l16 = _flash(lib, qkv, 8, want_lse=True, workspace=True)
    ox3, lx3 = _in_mode("bf16x3", lambda: _flash(lib, qkv, 8, want_lse=True, workspace=True))
    assert torch.equal(o16, ox3) and torch.equal(l16, lx3)
    assert _flash_route(lib, qkv, 8, want_lse=True, workspace=True) == (MHA_H2_PAIRS if d == 16 else MHA_X3P_PAIRS)
    assert not torch.equal(o16, _flash(lib, qkv, 8, workspace=True)[0])          # ... and without the lse the mode does act


@pytest.mark.parametrize("d,L,workspace", [(8, 1024, True), (16, 256, True), (32, 256, True), (16, 1024, False), (32, 1024, False)],
                         ids=["d8", "d16-L256", "d32-L256", "d16-no-ws", "d32-no-ws"])
def test_f16_uncovered_forward_is_the_default_forward(d, L, workspace, f16_mode):
    lib = f16_mode
    qkv = _case("gauss", d, L, 2)
    o16, _ = _flash(lib, qkv, 8, workspace=workspace)
    ox3, _ = _in_mode("bf16x3", lambda: _flash(lib, qkv, 8, workspace=workspace))
    assert torch.equal(o16, ox3)


@pytest.mark.parametrize("d", [16, 32])
def test_f16_attention_backward_is_the_default_backward(d):
    from _attn_bwd_cases import make_case, run_bwd
    lib = _capi.lib()
    qkv, d_o = make_case("plain", d, 1024, 2, 8, torch.Generator().manual_seed(40 + d))
    qkv, d_o = qkv.to(DEV), d_o.to(DEV)
    g16, gx3, g32 = run_bwd(lib, qkv, d_o, 8, 2), run_bwd(lib, qkv, d_o, 8, 1), run_bwd(lib, qkv, d_o, 8, 0)
    assert torch.isfinite(g16).all() and torch.equal(g16, gx3)
    assert not torch.equal(g16, g32), "the split-operand backward did not run in the f16 mode"


def test_f16_convolutions_are_the_default_convolutions(f16_mode):
    lib = f16_mode
    g = torch.Generator().manual_seed(77)
    B, cin, cout, H, W = 16, 64, 64, 64, 64          # sizes the split-operand 3x3 and 1x1 kernels take (tests/test_gpu_ops.py)
    x = torch.randn(B, cin, H, W, generator=g)
    w3 = torch.randn(cout, cin, 3, 3, generator=g) / 24
    w1 = torch.randn(cout, cin, 1, 1, generator=g) / 8
    b = torch.randn(cout, generator=g)
    gn = (torch.rand(B, cin, generator=g) + 0.5, torch.randn(B, cin, generator=g) * 0.3)
    run = lambda: (run_conv(x, None, w3, b, 3, 1, gn=gn), run_conv(x, None, w1, b, 1, 0))
    a3, a1 = run()
    b3, b1 = _in_mode("bf16x3", run)
    c3, c1 = _in_mode("f32", run)
    assert torch.equal(a3, b3) and torch.equal(a1, b1)
    assert not torch.equal(a3, c3), "the split-operand 3x3 convolution did not run in the f16 mode"
    assert not torch.equal(a1, c1), "the split-operand 1x1 convolution did not run in the f16 mode"


def test_f16_training_step_is_the_default_training_step():
    """One optimizer step of the default model at 32x32, batch 2: loss and every parameter bitwise equal in the two modes."""
    from golden_models import default32_trainer_model
    from hdiff_amd.DiffusionFreeGuidence import ModelCondition as MC
    from hdiff_amd import optim as HO

    def step():
        m, c, _ = default32_trainer_model(MC.UNet)
        m = m.to(DEV).train()
        opt = HO.AdamW(m.parameters(), lr=1e-4, weight_decay=1e-4)
        g = torch.Generator().manual_seed(5)
        x = torch.randn(2, 3, 32, 32, generator=g).to(DEV)
        noise = torch.randn(2, 3, 32, 32, generator=g).to(DEV)
        t = torch.tensor([17, 401], device=DEV)
        labels = torch.tensor([1, 3], device=DEV)
        loss = (m(x, t, labels) - noise).pow(2).mean()
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        return loss.detach().clone(), [p.detach().clone() for p in m.parameters()]

    l16, p16 = _in_mode("f16", step)
    lx3, px3 = _in_mode("bf16x3", step)
    assert torch.isfinite(l16) and torch.equal(l16, lx3)
    assert all(torch.equal(a, b) for a, b in zip(p16, px3))


# ---- 5. error behaviour --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [16, 32])
def test_f16_nan_and_inf_inputs_behave_like_the_default_mode(d, f16_mode):
    lib = f16_mode
    qkv = _case("gauss", d, 1024, 2)
    qkv[0, 2 * d + 3, 300] = float("nan")            # a query of head 2, sample 0
    qkv[1, 5 * d + 1, 777] = float("inf")            # a query of head 5, sample 1
    o16, _ = _flash(lib, qkv, 8, workspace=True)
    ox3, _ = _in_mode("bf16x3", lambda: _flash(lib, qkv, 8, workspace=True))
    assert torch.equal(torch.isnan(o16), torch.isnan(ox3))
    assert torch.isnan(o16).any() and torch.isfinite(o16[~torch.isnan(o16)]).all()
    ok = ~torch.isnan(ox3)
    assert (o16[ok] - ox3[ok]).abs().max().item() < 0.05 * ox3[ok].abs().max().item()


# ---- 6. network level ----------------------------------------------------------------------------------------------------------
def _default64():
    from hdiff_amd.DiffusionFreeGuidence import ModelCondition as MC
    from oracle import cpu_path as O
    d = np.load(os.path.join(GOLDEN, "unet_default64.npz"))
    c = json.loads(bytes(d["cfg_json"]).decode())
    torch.manual_seed(int(d["seed"][0]))
    m = MC.UNet(**c).eval()
    with torch.no_grad():
        m.time_embedding.timembedding[0].weight[417].copy_(torch.from_numpy(d["temb_row_417"]))
    cfg = O.UNetConfig(T=c["T"], num_labels=c["num_labels"], ch=c["ch"], ch_mult=tuple(c["ch_mult"]),
                       num_res_blocks=c["num_res_blocks"], dropout=c["dropout"])
    return m, c, cfg, d


def oracle_with_emulation(sd, cfg, x, t, labels, offset):
    """the CPU oracle's forward with its attention core replaced, where the mode acts, by the emulation of the format"""
    from oracle import cpu_path as O
    with EM.oracle_with_emulated_attention(offset), torch.no_grad():
        return O.unet_forward(sd, cfg, x, t, labels)


@pytest.mark.parametrize("which", ["golden", "randn1234"])
def test_f16_default_model_64_inside_the_emulated_envelope(which):
    from oracle import cpu_path as O
    m, c, cfg, d = _default64()
    if which == "golden":
        x, t, labels = torch.from_numpy(d["x"]), torch.from_numpy(d["t"]), torch.tensor([1])
    else:
        x = torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(1234))
        t, labels = torch.tensor([c["T"] - 1]), torch.tensor([1])
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    with torch.no_grad():
        exact = O.unet_forward(sd, cfg, x, t, labels).double()
    dep = []
    for off in EM.OFFSETS8:
        e = oracle_with_emulation(sd, cfg, x, t, labels, off).double() - exact
        dep.append((e.pow(2).mean().sqrt().item(), e.abs().max().item()))
    md = m.to(DEV)
    with torch.no_grad():
        run = lambda: md(x.to(DEV), t.to(DEV), labels.to(DEV)).double().cpu()
        y16 = _in_mode("f16", run)
        yx3 = _in_mode("bf16x3", run)
    e16 = y16 - exact
    rms16, worst16 = e16.pow(2).mean().sqrt().item(), e16.abs().max().item()
    lo, hi, hiw = min(r for r, _ in dep), max(r for r, _ in dep), max(w for _, w in dep)
    print(f"f16 default64 {which}: output rms {exact.pow(2).mean().sqrt().item():.3f}; hip f16 - exact oracle rms {rms16:.3e} worst "
          f"{worst16:.3e}; emulated departures rms {lo:.3e} .. {hi:.3e}, worst up to {hiw:.3e}; bf16x3 worst "
          f"{(yx3 - exact).abs().max().item():.3e}")
    assert 0.5 * lo <= rms16 <= 2.0 * hi, (rms16, lo, hi)
    assert worst16 < 3.0 * hiw, (worst16, hiw)
    assert (yx3 - exact).abs().max().item() < 7e-5


# ---- 7. samplers ---------------------------------------------------------------------------------------------------------------
def _quality(a, b):
    from hdiff_amd import metrics as M
    ia = ((a.cpu().clamp(-1, 1) * 0.5 + 0.5) * 255.0).permute(0, 2, 3, 1).numpy()
    ib = ((b.cpu().clamp(-1, 1) * 0.5 + 0.5) * 255.0).permute(0, 2, 3, 1).numpy()
    return (min(M.psnr(x, y, 255) for x, y in zip(ia, ib)), min(M.ssim(x, y, 255, channel_axis=2) for x, y in zip(ia, ib)))


def test_f16_tree_a_sampler():
    from hdiff_amd.DiffusionFreeGuidence import DiffusionCondition as DC, ModelCondition as MC
    T_, S, w, beta = 50, 64, 1.8, (1e-4, 0.028)
    torch.manual_seed(0)
    m = MC.UNet(T=T_, num_labels=10, ch=128, ch_mult=[1, 2, 2, 2], num_res_blocks=2, dropout=0.15).eval()
    with torch.no_grad():
        m.tail[2].weight.mul_(0.1)           # keep x O(1) (tests/test_gpu_end_to_end.py)
    g = torch.Generator().manual_seed(1234)
    x_T = torch.randn(1, 3, S, S, generator=g).to(DEV)
    labels = torch.tensor([1], device=DEV)
    noise = torch.randn(T_, 1, 3, S, S, generator=g).to(DEV)
    samp = DC.GaussianDiffusionSampler(m.to(DEV), beta[0], beta[1], T_, w=w).to(DEV)
    run = lambda: samp(x_T, labels, noise_by_step=noise).clone()
    before = hdiff_amd.get_contraction_mode()
    try:
        hdiff_amd.set_contraction_mode("bf16x3")
        first = run()
        hdiff_amd.set_contraction_mode("f16")
        second = run()
        again = run()
        samp.use_graph = False
        eager = run()
        samp.use_graph = True
        hdiff_amd.set_contraction_mode("bf16x3")
        third = run()
    finally:
        hdiff_amd.set_contraction_mode(before)
    sp = next(iter(samp._splans.values()))
    assert int(sp.nan_flag.item()) == 0
    assert torch.equal(second, again), "two f16 runs differ"
    assert torch.equal(second, eager), "hipGraph replay differs from eager launches"
    assert not torch.equal(first, second), "the f16 step ran the default kernels (graph not rebuilt?)"
    assert torch.equal(first, third), "back in bf16x3 the graph was not rebuilt"
    assert second.min().item() >= -1.0 and second.max().item() <= 1.0
    psnr, ssim = _quality(second, first)
    print(f"F16_SAMPLER tree A 64x64 T=50 w=1.8: f16 against bf16x3 image PSNR {psnr:.2f} dB SSIM {ssim:.5f} (not gated)")


def test_f16_tree_b_ddim_sampler():
    """DynamicUNet attends only in its four middle blocks, at 1/8 of the resolution: 256x256 is the size at which they reach the
    mode's shapes (L = 1024, d_head 32).  The untrained model saturates the clipped output (tests/test_gpu_end_to_end.py), so the
    comparisons also look at the pre-clip state the sampler ends with."""
    from hdiff_amd.diffusion.Diffusion import GaussianDiffusionSampler as SamplerB
    from hdiff_amd.diffusion.Model import DynamicUNet
    torch.manual_seed(0)
    m = DynamicUNet(T=1000, ch=128, ch_mult=[1, 2, 2, 2], num_res_blocks=2, dropout=0.0).eval()
    with torch.no_grad():
        m.tail[2].weight.mul_(2.0e4)         # tests/test_gpu_end_to_end.py: initialize() gives the tail gain 1e-5
    g = torch.Generator().manual_seed(7)
    S = 256
    img = torch.randint(0, 256, (1, 3, S, S), generator=g).float().to(DEV)
    y_T = torch.randn(1, 3, S, S, generator=g).to(DEV)
    samp = SamplerB(m.to(DEV), 1e-4, 0.02, 1000).to(DEV)

    def run(**kw):
        out = samp(img, ddim=True, unconditional_guidance_scale=1, ddim_step=10, y_T=y_T, **kw).clone()
        sp = next(iter(samp._plans.values()))
        assert int(sp.nan_flag.item()) == 0
        return out, sp.unet.y.clone()
    before = hdiff_amd.get_contraction_mode()
    try:
        hdiff_amd.set_contraction_mode("bf16x3")
        first = run()
        hdiff_amd.set_contraction_mode("f16")
        second = run()
        again = run()
        traj = []
        eager = run(trajectory=traj)
        hdiff_amd.set_contraction_mode("bf16x3")
        third = run()
    finally:
        hdiff_amd.set_contraction_mode(before)
    assert len(traj) == 10
    same = lambda a, b: torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert same(second, again), "two f16 runs differ"
    assert same(second, eager), "hipGraph replay differs from eager launches"
    assert not torch.equal(first[1], second[1]), "the f16 step ran the default kernels (graph not rebuilt?)"
    assert same(first, third), "back in bf16x3 the graph was not rebuilt"
    assert torch.isfinite(second[1]).all() and second[0].min().item() >= -1.0 and second[0].max().item() <= 1.0
    psnr, ssim = _quality(second[0], first[0])
    rel = ((second[1] - first[1]).abs().max() / first[1].abs().max()).item()
    print(f"F16_SAMPLER tree B 256x256 DDIM 10 steps: f16 against bf16x3 image PSNR {psnr:.2f} dB SSIM {ssim:.5f}, pre-clip state "
          f"relative difference {rel:.2e} (not gated)")
