"""GPU: the strided DDIM sampler of the label-conditioned tree -- the fused update kernel bit for bit against the fp32 definition
(tests/_ddim_a_def.py), its own noise, its loop bookkeeping, the whole loop against the CPU oracle's UNet, the tie to the pinned
ancestral path, seeding, and the eval harness.

New modules are not in conftest.py's mode list: a test that has to hold in both contraction modes selects them itself."""
import ctypes as C
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hdiff_amd  # noqa: E402
from hdiff_amd import _capi  # noqa: E402
from hdiff_amd.DiffusionFreeGuidence import DiffusionCondition as DC  # noqa: E402
from hdiff_amd.DiffusionFreeGuidence import ModelCondition as MC  # noqa: E402
from hdiff_amd.DiffusionFreeGuidence import TrainCondition as TC  # noqa: E402
from oracle import cpu_path as O  # noqa: E402

import _ddim_a_def as D  # noqa: E402

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def maxerr(got, ref):
    return (got.detach().cpu().double() - ref.detach().cpu().double()).abs().max().item()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _step(lib, x, ec, eu, z, out, tab, counter, S, w, clip, seed, flag, n):
    _capi.check(lib.hdiff_cfg_ddim_step(x.data_ptr(), ec.data_ptr(), eu.data_ptr(), None if z is None else z.data_ptr(),
                                        out.data_ptr(), tab.data_ptr(), counter.data_ptr(), S, C.c_double(w), int(clip),
                                        C.c_uint64(seed), flag.data_ptr(), n, _stream()), "cfg_ddim_step")


# ----------------------------------------------------------------------------------------------------------------------
# a. the update, bit for bit
# ----------------------------------------------------------------------------------------------------------------------
def test_update_bit_exact_nan_flag_and_counter_clamp():
    g = torch.Generator().manual_seed(2)
    n, T, S, w = 3 * 33 * 31, 50, 10, 1.8          # n % 4 == 3: the tail quad is taken
    x, ec, eu, z = [torch.randn(n, generator=g) for _ in range(4)]
    betas = torch.linspace(1e-4, 0.028, T).double()
    tau = D.timesteps(T, S)
    lib = _capi.lib()
    dx, dec, deu, dz = x.to(DEV), ec.to(DEV), eu.to(DEV), z.to(DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = torch.empty(n, device=DEV)
    clipped = 0
    for eta in (0.0, 0.7):
        tab = D.table(betas, tau, eta).float()
        dtab = tab.to(DEV).contiguous()
        for clip in (False, True):
            for k in (7, 0):
                ctr = torch.tensor([k], dtype=torch.int32, device=DEV)
                _step(lib, dx, dec, deu, dz, out, dtab, ctr, S, w, clip, 0, flag, n)
                ref = D.step(x, ec, eu, z, tab[k], k, w, clip)
                assert torch.equal(out.cpu(), ref), f"cfg_ddim_step not bit-exact at k={k} eta={eta} clip_x0={clip}"
                if clip:
                    x0 = (x - D.guided_eps(ec, eu, w) * tab[k][0]) / tab[k][1]
                    clipped += int((x0.abs() > 1).sum())
            # a counter outside the table is clamped, never an out-of-bounds read
            for bad, as_k in ((-7, 0), (10 ** 6, S - 1)):
                ctr = torch.tensor([bad], dtype=torch.int32, device=DEV)
                _step(lib, dx, dec, deu, dz, out, dtab, ctr, S, w, clip, 0, flag, n)
                assert torch.equal(out.cpu(), D.step(x, ec, eu, z, tab[as_k], as_k, w, clip)), (bad, eta, clip)
    assert clipped > 100                             # the clip branch really clamps values in this data
    assert flag.item() == 0
    # x and x_next may alias
    tab = D.table(betas, tau, 0.7).float()
    dtab, cur = tab.to(DEV).contiguous(), dx.clone()
    ctr = torch.tensor([7], dtype=torch.int32, device=DEV)
    _step(lib, cur, dec, deu, dz, cur, dtab, ctr, S, w, True, 0, flag, n)
    assert torch.equal(cur.cpu(), D.step(x, ec, eu, z, tab[7], 7, w, True))
    # one NaN in eps_c sets the flag, with and without the clip (the clamp must not swallow it)
    dec[5] = float("nan")
    for clip in (False, True):
        flag.zero_()
        _step(lib, dx, dec, deu, dz, out, dtab, ctr, S, w, clip, 0, flag, n)
        assert flag.item() == 1, clip
        assert bool(torch.isnan(out[5])) and int(torch.isnan(out).sum()) == 1


# ----------------------------------------------------------------------------------------------------------------------
# b. the kernel's own noise
# ----------------------------------------------------------------------------------------------------------------------
def test_own_noise_moments_and_determinism():
    n, T, S = 1 << 18, 50, 10
    betas = torch.linspace(1e-4, 0.028, T).double()
    tab = D.table(betas, D.timesteps(T, S), 1.0).float()
    dtab = tab.to(DEV).contiguous()
    zero = torch.zeros(n, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    lib = _capi.lib()

    def run(seed, k):
        out = torch.empty(n, device=DEV)
        ctr = torch.tensor([k], dtype=torch.int32, device=DEV)
        _step(lib, zero, zero, zero, None, out, dtab, ctr, S, 1.8, False, seed, flag, n)
        return out

    a, b, other_seed, other_k = run(42, 6), run(42, 6), run(43, 6), run(42, 5)
    assert torch.equal(a, b) and not torch.equal(a, other_seed)
    z = (a.double() / float(tab[6, D.SIGMA])).cpu()            # x = eps = 0: the output is sigma_k * z
    z5 = (other_k.double() / float(tab[5, D.SIGMA])).cpu()
    assert not torch.equal(z.float(), z5.float())
    mean, var = z.mean().item(), z.var(unbiased=False).item()
    print(f"own noise n={n}: mean {mean:+.3e} (bound {4 / math.sqrt(n):.3e})  var - 1 {var - 1:+.3e} (bound {4 * math.sqrt(2 / n):.3e})")
    assert torch.isfinite(z).all()
    assert abs(mean) < 4 / math.sqrt(n) and abs(var - 1) < 4 * math.sqrt(2 / n)
    assert bool((run(42, 0) == 0).all())                        # no noise at k = 0
    assert flag.item() == 0


def test_own_noise_is_the_randn_stream():
    """The step kernels draw element i of step k from the Philox counter that ``hdiff_randn(n, seed, offset=k)`` gives element i:
    with x = eps_c = eps_u = 0 and no injected noise each update is exactly ``0 + sigma_k * z``, bit for bit (the product formed by
    torch in fp32 on the device).  n = 4099: several workgroups, n % 4 == 3, so the tail quad is taken."""
    n, T, S, w, seed = 4099, 50, 10, 1.8, 42
    lib = _capi.lib()
    zero = torch.zeros(n, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)

    def randn(k):
        z = torch.empty(n, device=DEV)
        _capi.check(lib.hdiff_randn(z.data_ptr(), n, C.c_uint64(seed), C.c_uint64(k), _stream()), "randn")
        return z

    # the ancestral step: the sampler's own tables (DiffusionCondition.py: _SamplerPlan)
    betas = torch.linspace(1e-4, 0.028, T).double()
    alphas = 1. - betas
    alphas_bar = torch.cumprod(alphas, dim=0)
    alphas_bar_prev = torch.cat([torch.ones(1, dtype=torch.float64), alphas_bar[:-1]])
    coeff1 = torch.sqrt(1. / alphas)
    coeff2 = coeff1 * (1. - alphas) / torch.sqrt(1. - alphas_bar)
    var = torch.cat([(betas * (1. - alphas_bar_prev) / (1. - alphas_bar))[1:2], betas[1:]])
    c1, c2, sg = coeff1.float().to(DEV), coeff2.float().to(DEV), torch.sqrt(var.float()).to(DEV)

    def ddpm(step):
        out = torch.empty(n, device=DEV)
        ctr = torch.tensor([step], dtype=torch.int32, device=DEV)
        _capi.check(lib.hdiff_ddpm_step(zero.data_ptr(), zero.data_ptr(), zero.data_ptr(), None, out.data_ptr(), c1.data_ptr(),
                                        c2.data_ptr(), sg.data_ptr(), ctr.data_ptr(), T, C.c_double(w), C.c_uint64(seed),
                                        flag.data_ptr(), n, _stream()), "ddpm_step")
        return out

    assert torch.equal(ddpm(5), sg[5] * randn(5)), "ddpm_step: not sigma_5 * randn(seed, offset=5)"
    assert bool((ddpm(0) == 0).all())                           # no noise at step 0

    # the strided DDIM step with eta = 1
    dtab = D.table(betas, D.timesteps(T, S), 1.0).float().to(DEV).contiguous()

    def ddim(k):
        out = torch.empty(n, device=DEV)
        ctr = torch.tensor([k], dtype=torch.int32, device=DEV)
        _step(lib, zero, zero, zero, None, out, dtab, ctr, S, w, False, seed, flag, n)
        return out

    assert float(dtab[6, D.SIGMA]) > 0
    assert torch.equal(ddim(6), dtab[6, D.SIGMA] * randn(6)), "cfg_ddim_step: not sigma_6 * randn(seed, offset=6)"
    assert bool((ddim(0) == 0).all())                           # no noise at k = 0
    assert flag.item() == 0


# ----------------------------------------------------------------------------------------------------------------------
# c. the loop's bookkeeping
# ----------------------------------------------------------------------------------------------------------------------
def test_step_loop_bookkeeping():
    g = torch.Generator().manual_seed(3)
    B, per, T, w, eta = 3, 3 * 40 * 36, 50, 1.8, 0.5
    n = B * per
    tau = [3, 11, 19, 30, 49]
    S = len(tau)
    x, ec, eu, z = [torch.randn(n, generator=g) for _ in range(4)]
    tab = D.table(torch.linspace(1e-4, 0.028, T).double(), tau, eta).float()
    dtab, dtau = tab.to(DEV).contiguous(), torch.tensor(tau, dtype=torch.int64, device=DEV)
    dec, deu, dz = ec.to(DEV), eu.to(DEV), z.to(DEV)
    cur = x.to(DEV)
    ctr = torch.tensor([S - 1], dtype=torch.int32, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    done = torch.zeros(1, dtype=torch.int32, device=DEV)
    t_next = torch.full((2 * B,), -5, dtype=torch.int64, device=DEV)
    xin = torch.zeros(2 * n, device=DEV)
    d = _capi.CfgDdimLoopDesc()
    d.x, d.eps_c, d.eps_u, d.noise, d.x_next = cur.data_ptr(), dec.data_ptr(), deu.data_ptr(), dz.data_ptr(), cur.data_ptr()
    d.tab, d.t_tab, d.step_ptr, d.nsteps, d.clip_x0 = dtab.data_ptr(), dtau.data_ptr(), ctr.data_ptr(), S, 0
    d.w, d.seed, d.nan_flag, d.n = w, 0, flag.data_ptr(), n
    d.x_dup0, d.x_dup1, d.t_next, d.t_count = xin.data_ptr(), xin.data_ptr() + 4 * n, t_next.data_ptr(), 2 * B
    d.done_counter = done.data_ptr()
    lib = _capi.lib()
    want = x
    for k in range(S - 1, -1, -1):                   # five eager launches, no reset in between
        _capi.check(lib.hdiff_cfg_ddim_step_loop(C.byref(d), _stream()), "cfg_ddim_step_loop")
        torch.cuda.synchronize()
        want = D.step(want, ec, eu, z, tab[k], k, w, False)
        assert torch.equal(cur.cpu(), want), k
        assert torch.equal(xin[:n], cur) and torch.equal(xin[n:], cur), k
        assert int(ctr.item()) == k - 1
        assert t_next.tolist() == [tau[max(k - 1, 0)]] * (2 * B), k
        assert int(done.item()) == 0 and int(flag.item()) == 0          # the counter wrapped back by itself


# ----------------------------------------------------------------------------------------------------------------------
# d. the whole loop against the CPU oracle
# ----------------------------------------------------------------------------------------------------------------------
TRAJ = dict(T=100, num_labels=3, ch=32, ch_mult=[1, 2], num_res_blocks=1, dropout=0.0)
TRAJ_BETA, TRAJ_S = (1e-4, 0.028), 8


@functools.lru_cache(maxsize=None)
def _traj_model():
    torch.manual_seed(4100)
    m = MC.UNet(**TRAJ).eval()
    g = torch.Generator().manual_seed(4101)
    with torch.no_grad():
        for n, p in sorted(m.named_parameters()):      # torch zero-initialises the attention biases: exercise them
            if n.endswith("in_proj_bias") or n.endswith("out_proj.bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x_T = torch.randn(2, 3, 16, 16, generator=g)
    noise = torch.randn(TRAJ_S, 2, 3, 16, 16, generator=g)
    return m.to(DEV), sd, x_T, torch.tensor([1, 3]), noise


@functools.lru_cache(maxsize=None)
def _traj_reference(w, eta, clip):
    """The loop of the definition on the CPU, computed once per case and shared by both contraction modes: k = S-1 .. 0,
    t = tau_k for every sample, eps from the oracle's UNet and guidance, the helper's update."""
    _, sd, x_T, labels, noise = _traj_model()
    cfg = O.UNetConfig(T=TRAJ["T"], num_labels=TRAJ["num_labels"], ch=TRAJ["ch"], ch_mult=tuple(TRAJ["ch_mult"]),
                       num_res_blocks=TRAJ["num_res_blocks"])
    tau = D.timesteps(TRAJ["T"], TRAJ_S)
    tab = D.table(torch.linspace(*TRAJ_BETA, TRAJ["T"]).double(), tau, eta).float()
    x, states = x_T, []
    with torch.no_grad():
        for k in range(TRAJ_S - 1, -1, -1):
            t = torch.full((x.shape[0],), tau[k], dtype=torch.long)
            eps = O.cfg_eps(O.unet_forward(sd, cfg, x, t, labels), O.unet_forward(sd, cfg, x, t, torch.zeros_like(labels)), w)
            x = D.update(x, eps, noise[k], tab[k], k, clip)
            states.append(x)
    return tuple(states)


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("eta", [0.0, 1.0])
@pytest.mark.parametrize("w", [0.0, 1.8])
def test_trajectory_against_the_oracle(w, eta, clip, mode):
    """Max-abs error of every pre-clip state against the CPU loop.  Gate: 1e-4, the gate of
    test_sampler_small_teacher_forced_and_graph for the ancestral loop.  Measured on an MI355X (profiles/ddim_tree_a.txt has every
    step): the largest of the eight steps is 9.2e-6 ... 1.4e-5 at w = 0 and 2.7e-5 ... 3.7e-5 at w = 1.8, the same in both modes
    (at this size neither mode reaches a split-operand kernel)."""
    m, _, x_T, labels, noise = _traj_model()
    ref = _traj_reference(w, eta, clip)
    before = hdiff_amd.get_contraction_mode()
    hdiff_amd.set_contraction_mode(mode)
    try:
        samp = DC.GaussianDiffusionSampler(m, *TRAJ_BETA, TRAJ["T"], w=w).to(DEV)
        traj = []
        with torch.no_grad():
            kw = dict(ddim_steps=TRAJ_S, eta=eta, clip_x0=clip, noise_by_step=noise)
            y_eager = samp(x_T.to(DEV), labels.to(DEV), trajectory=traj, **kw)
            y_graph = samp(x_T.to(DEV), labels.to(DEV), **kw)
    finally:
        hdiff_amd.set_contraction_mode(before)
    assert len(traj) == TRAJ_S
    errs = [maxerr(got, want) for got, want in zip(traj, ref)]
    print(f"ddim trajectory w={w} eta={eta} clip_x0={clip} {mode}: per-step max err", ["%.2e" % e for e in errs])
    assert max(errs) < 1e-4
    assert float(y_graph.min()) >= -1 and float(y_graph.max()) <= 1
    assert torch.equal(y_eager, torch.clip(traj[-1], -1, 1))
    assert torch.equal(y_eager, y_graph), "graph replay must reproduce the eager launches bit for bit"


# ----------------------------------------------------------------------------------------------------------------------
# e. the tie to the pinned ancestral path
# ----------------------------------------------------------------------------------------------------------------------
def _golden_small_model():
    d = np.load(os.path.join(GOLDEN, "unet_small.npz"))
    c = json.loads(bytes(d["cfg_json"]).decode())
    m = MC.UNet(**c)
    m.load_state_dict({k[3:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("sd/")}, strict=True)
    return m.to(DEV).eval(), c


def test_stride_one_eta_one_equals_the_ancestral_mean():
    """With all-zero noise the ancestral loop is its posterior mean, and DDIM at stride 1, eta = 1 is the same mean written as
    san * x0 + c2 * eps: the two loops over the golden small model agree to 1e-4."""
    m, c = _golden_small_model()
    d = np.load(os.path.join(GOLDEN, "sampler_small.npz"))
    b1, bT = [float(v) for v in d["beta"]]
    x_T, labels = torch.from_numpy(d["x_T"]).to(DEV), torch.from_numpy(d["labels"]).to(DEV)
    zeros = torch.zeros(c["T"], *x_T.shape)
    for w in (0.0, 1.8):
        samp = DC.GaussianDiffusionSampler(m, b1, bT, c["T"], w=w).to(DEV)
        with torch.no_grad():
            anc = samp(x_T, labels, noise_by_step=zeros)
            ddim = samp(x_T, labels, ddim_steps=c["T"], eta=1.0, noise_by_step=zeros)
            again = samp(x_T, labels, noise_by_step=zeros)
        err = maxerr(ddim, anc)
        print(f"w={w}: ancestral mean vs ddim(stride 1, eta 1), zero noise: max abs {err:.2e}")
        assert err < 1e-4
        assert torch.equal(anc, again)               # the ancestral variant is rebuilt intact after a strided call


def test_strided_step_has_no_more_launches_than_the_ancestral_step():
    """Both captured steps are the 2B UNet's launch list plus ONE update call."""
    m, c = _golden_small_model()
    samp = DC.GaussianDiffusionSampler(m, 1e-4, 0.028, c["T"], w=1.8).to(DEV)
    sp = DC._SamplerPlan(samp, 2, 16, 16, torch.device(DEV))
    names = [op[0] for op in sp.variant(False, 1).ops]
    ddim_names = [op[0] for op in sp.variant(False, 1, ((1, 3, 7), 1.0, False)).ops]
    assert names[-1] == "hdiff_ddpm_step_loop" and ddim_names[-1] == "hdiff_cfg_ddim_step_loop"
    assert ddim_names[:-1] == names[:-1] and len(ddim_names) <= len(names)


# ----------------------------------------------------------------------------------------------------------------------
# f. seeds, the NaN contract, the f16 mode
# ----------------------------------------------------------------------------------------------------------------------
def test_seeds_nan_and_f16_mode():
    m, c = _golden_small_model()
    samp = DC.GaussianDiffusionSampler(m, 1e-4, 0.028, c["T"], w=1.8).to(DEV)
    x_T = torch.randn(3, 3, 16, 16, generator=torch.Generator().manual_seed(1)).to(DEV)
    labels = torch.tensor([1, 2, 3], device=DEV)
    with torch.no_grad():
        torch.manual_seed(7); a = samp(x_T, labels, ddim_steps=4, eta=1.0)
        torch.manual_seed(7); b = samp(x_T, labels, ddim_steps=4, eta=1.0)
        torch.manual_seed(8); other = samp(x_T, labels, ddim_steps=4, eta=1.0)
        assert torch.equal(a, b) and not torch.equal(a, other)
        torch.manual_seed(7); d7 = samp(x_T, labels, ddim_steps=4)
        state = torch.get_rng_state()
        samp(x_T, labels, ddim_steps=4)
        assert torch.equal(torch.get_rng_state(), state)             # eta = 0 draws no seed: the generator is where it was
        samp(x_T, labels, ddim_steps=4, eta=1.0)
        assert not torch.equal(torch.get_rng_state(), state)         # (eta > 0 does)
        torch.manual_seed(8); d8 = samp(x_T, labels, ddim_steps=4)
        assert torch.equal(d7, d8) and not torch.equal(d7, a)
        assert float(d7.min()) >= -1 and float(d7.max()) <= 1
    bad = x_T.clone()
    bad[0, 0, 0, 0] = float("nan")
    for kw in (dict(ddim_steps=4), dict(ddim_steps=4, eta=1.0, clip_x0=True)):
        with torch.no_grad(), pytest.raises(AssertionError, match="nan in tensor."):
            samp(bad, labels, **kw)
    # the opt-in f16 mode at a shape that reaches its attention kernel (d_head 16, L = 1024)
    torch.manual_seed(5)
    big = MC.UNet(T=20, num_labels=3, ch=128, ch_mult=[1, 2], num_res_blocks=1, dropout=0.0).eval().to(DEV)
    samp = DC.GaussianDiffusionSampler(big, 1e-4, 0.028, 20, w=1.8).to(DEV)
    x_T = torch.randn(1, 3, 32, 32, generator=torch.Generator().manual_seed(2)).to(DEV)
    before = hdiff_amd.get_contraction_mode()
    hdiff_amd.set_contraction_mode("f16")
    try:
        with torch.no_grad():
            y = samp(x_T, torch.tensor([2], device=DEV), ddim_steps=4)
    finally:
        hdiff_amd.set_contraction_mode(before)
    assert torch.isfinite(y).all() and float(y.min()) >= -1 and float(y.max()) <= 1 and float(y.abs().max()) > 0


# ----------------------------------------------------------------------------------------------------------------------
# g. the eval harness
# ----------------------------------------------------------------------------------------------------------------------
def test_eval_reads_the_ddim_keys(tmp_path, monkeypatch):
    cfg = {
        "state": "eval", "epoch": 10, "batch_size": 4, "T": 6, "channel": 32, "channel_mult": [1, 2], "num_res_blocks": 1,
        "dropout": 0.0, "lr": 2e-4, "multiplier": 2.5, "beta_1": 1e-4, "beta_T": 0.028, "img_size": 16, "grad_clip": 1.,
        "device": DEV, "w": 1.8, "save_dir": str(tmp_path / "ckpt"), "training_load_weight": None,
        "test_load_weight": "ckpt_0_.pt", "sampled_dir": str(tmp_path / "samples"),
        "sampledNoisyImgName": "noisy.png", "sampledImgName": "sampled.png", "nrow": 4,
        "dataset": "synthetic", "num_labels": 3, "num_workers": 0,
    }
    os.makedirs(cfg["save_dir"])
    torch.manual_seed(0)
    torch.save(TC._denoiser(cfg, "cpu").state_dict(), os.path.join(cfg["save_dir"], "ckpt_0_.pt"))
    seen = []

    class Recording(DC.GaussianDiffusionSampler):
        """A thin wrapper: records the keywords eval passes and, through `trajectory`, how many steps the loop ran."""
        def forward(self, x_T, labels, **kw):
            traj = []
            out = super().forward(x_T, labels, trajectory=traj, **kw)
            seen.append((kw, len(traj)))
            return out

    monkeypatch.setattr(TC, "GaussianDiffusionSampler", Recording)
    imgs = TC.eval(dict(cfg, ddim_steps=4))
    assert tuple(imgs.shape) == (4, 3, 16, 16) and float(imgs.min()) >= 0 and float(imgs.max()) <= 1
    assert os.path.isfile(os.path.join(cfg["sampled_dir"], "sampled.png"))
    assert os.path.isfile(os.path.join(cfg["sampled_dir"], "noisy.png"))
    assert seen == [(dict(ddim_steps=4, eta=0.0, clip_x0=False), 4)]
    TC.eval(dict(cfg, ddim_steps=3, ddim_eta=1.0, ddim_clip_x0=True))
    assert seen[-1] == (dict(ddim_steps=3, eta=1.0, clip_x0=True), 3)
    imgs = TC.eval(cfg)                              # without the keys: the T-step ancestral loop, called as before
    assert seen[-1] == ({}, cfg["T"]) and float(imgs.min()) >= 0 and float(imgs.max()) <= 1
