"""CPU-only checks of the strided DDIM sampler of the label-conditioned tree: the time-step rule, the float64 coefficient table and
its identities with the ancestral sampler's buffers, the C ABI's declarations and host-side argument checks, and the public
signature.  The definition is tests/_ddim_a_def.py."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest
import torch

import hdiff_amd
from hdiff_amd import _capi
from hdiff_amd.DiffusionFreeGuidence import DiffusionCondition as DC
from hdiff_amd.DiffusionFreeGuidence import ModelCondition as MC

import _ddim_a_def as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_timestep_rule():
    assert DC.ddim_timesteps(8, 8) == list(range(8)) and DC.ddim_timesteps(1000, 1000) == list(range(1000))
    assert DC.ddim_timesteps(1000, 50) == list(range(19, 1000, 20))
    assert DC.ddim_timesteps(100, 7) == [13, 27, 41, 56, 70, 84, 99]
    assert DC.ddim_timesteps(50, 1) == [49]
    for T in (1, 2, 7, 50, 100, 1000):
        for S in sorted({1, 2, 3, T // 3 + 1, T - 1, T} & set(range(1, T + 1))):
            tau = DC.ddim_timesteps(T, S)
            assert tau == D.timesteps(T, S) and len(tau) == S and tau[-1] == T - 1 and tau[0] >= 0
            assert all(b > a for a, b in zip(tau, tau[1:])), (T, S)
    for T, S in ((10, 0), (10, 11), (10, -3), (10, 4.5)):
        with pytest.raises(ValueError):
            DC.ddim_timesteps(T, S)


def _sampler(T, beta_T=0.028, w=1.8):
    m = MC.UNet(T=T, num_labels=3, ch=32, ch_mult=[1, 2], num_res_blocks=1, dropout=0.0).eval()
    return DC.GaussianDiffusionSampler(m, 1e-4, beta_T, T, w=w)


def _same_table(got, want):
    """The package's table against the definition's, to a few units in the last place of float64 (torch's sqrt may round its last
    bit differently between its vector and scalar paths)."""
    return got.shape == want.shape and bool(((got - want).abs() <= 8 * 2.0 ** -53 * want.abs()).all())


def test_table_rows_and_eta_zero():
    betas = torch.linspace(1e-4, 0.02, 100).double()
    for tau in (DC.ddim_timesteps(100, 7), [3, 11, 19, 30, 99], list(range(100))):
        tab = DC.ddim_table(betas, tau, 0.0)
        assert tab.dtype == torch.float64 and tuple(tab.shape) == (len(tau), 5)
        assert _same_table(tab, D.table(betas, tau, 0.0))
        ab = torch.cumprod(1.0 - betas, 0)
        ap = torch.cat([torch.ones(1, dtype=torch.float64), ab[torch.tensor(tau)][:-1]])
        assert torch.all(tab[:, D.SIGMA] == 0) and torch.equal(tab[:, D.C2], torch.sqrt(1.0 - ap))
    for eta in (0.0, 0.7, 1.0):
        tab = DC.ddim_table(betas, DC.ddim_timesteps(100, 7), eta)
        assert _same_table(tab, D.table(betas, DC.ddim_timesteps(100, 7), eta))
        assert tab[0, D.SAN] == 1.0 and tab[0, D.C2] == 0.0 and tab[0, D.SIGMA] == 0.0
        assert torch.isfinite(tab).all() and (eta == 0.0 or torch.all(tab[1:, D.SIGMA] > 0))


@pytest.mark.parametrize("T", [8, 100, 1000])
@pytest.mark.parametrize("beta_T", [0.02, 0.028])
def test_table_stride_one_eta_one_is_the_posterior_sampler(T, beta_T):
    """sigma^2 == posterior_var, san / sa == coeff1, c2 - san * s1m / sa == -coeff2 in float64 (measured <= 1.4e-15; gate 1e-12),
    and the argument of c2's square root is exactly 0 at k = 0 and never negative."""
    samp = _sampler(T, beta_T)
    tab = DC.ddim_table(samp.betas, range(T), 1.0)
    e_var = (tab[:, D.SIGMA] ** 2 - samp.posterior_var).abs().max().item()
    e_c1 = (tab[:, D.SAN] / tab[:, D.SA] - samp.coeff1).abs().max().item()
    e_c2 = (tab[:, D.C2] - tab[:, D.SAN] * tab[:, D.S1M] / tab[:, D.SA] + samp.coeff2).abs().max().item()
    print(f"T={T} beta_T={beta_T}: |sigma^2 - posterior_var| {e_var:.2e}  |san/sa - coeff1| {e_c1:.2e}  |c2 - san s1m/sa + coeff2| {e_c2:.2e}")
    assert e_var <= 1e-12 and e_c1 <= 1e-12 and e_c2 <= 1e-12
    arg = D.c2_sqrt_argument(samp.betas, range(T), 1.0)
    assert arg[0].item() == 0.0 and arg.min().item() >= 0.0


def test_table_argument_errors():
    betas = torch.linspace(1e-4, 0.02, 20).double()
    for bad in ([], [3, 3, 5], [5, 3], [-1, 4], [4, 20], [1.5, 3], iter([1.5, 3]), (t for t in [3, 9.5])):
        with pytest.raises(ValueError):
            DC.ddim_table(betas, bad, 0.0)
    assert torch.equal(DC.ddim_table(betas, (t for t in [3, 9]), 0.5), DC.ddim_table(betas, [3, 9], 0.5))   # a one-shot iterable is read once
    with pytest.raises(ValueError):
        DC.ddim_table(betas, [3, 9], -0.1)


def test_forward_signature_and_value_errors():
    sig = inspect.signature(DC.GaussianDiffusionSampler.forward)
    want = {"ddim_steps": None, "eta": 0.0, "timesteps": None, "clip_x0": False, "noise_by_step": None, "trajectory": None}
    for name, default in want.items():
        p = sig.parameters[name]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY, name
        assert p.default == default and type(p.default) is type(default), name
    assert [n for n, p in sig.parameters.items() if p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD] == ["self", "x_T", "labels"]
    samp = _sampler(8)
    x, lab = torch.zeros(1, 3, 16, 16), torch.ones(1, dtype=torch.long)
    bad_calls = [dict(ddim_steps=0), dict(ddim_steps=9), dict(ddim_steps=4, eta=-0.5), dict(ddim_steps=4, timesteps=[1, 3, 5, 7]),
                 dict(ddim_steps=4.5), dict(timesteps=iter([1.5, 3])),
                 dict(eta=1.0), dict(clip_x0=True), dict(eta=0.5, noise_by_step=torch.zeros(8, 1, 3, 16, 16)),      # eta / clip_x0 need a schedule
                 dict(timesteps=[1, 1, 7]), dict(timesteps=[5, 3]), dict(timesteps=[0, 8]), dict(timesteps=[-1, 7]),
                 dict(ddim_steps=4, noise_by_step=torch.zeros(8, 1, 3, 16, 16)),
                 dict(timesteps=[1, 3, 7], noise_by_step=torch.zeros(4, 1, 3, 16, 16))]
    for kw in bad_calls:
        with torch.no_grad(), pytest.raises(ValueError):
            samp(x, lab, **kw)
    # a CPU tensor is still refused, in both loops
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        samp(x, lab)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        samp(x, lab, ddim_steps=4)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        samp(x, lab, timesteps=[1, 3, 7], eta=1.0, clip_x0=True)


def test_symbols_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "hdiff.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(hdiff_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (hdiff_[a-z0-9_]+)", out))
    for name in ("hdiff_cfg_ddim_step", "hdiff_cfg_ddim_step_loop"):
        assert name in declared and name in exported and name in _capi.EXPORTED_SYMBOLS, name
    assert "hdiff_cfg_ddim_loop_desc" in text
    assert hdiff_amd.lib().hdiff_abi_version() == 6


def test_argument_validation_without_gpu():
    """Null pointers and zero sizes come back as HDIFF_ERR_INVALID from the host-side checks: nothing is launched."""
    lib = hdiff_amd.lib()
    p = 64      # any non-null value: the checks fail before a pointer is used
    assert lib.hdiff_cfg_ddim_step(None, p, p, None, p, p, p, 5, 1.8, 0, 0, p, 16, None) == -1
    assert b"cfg_ddim_step: null pointer" in lib.hdiff_last_error()
    assert lib.hdiff_cfg_ddim_step(p, p, p, None, p, None, p, 5, 1.8, 0, 0, p, 16, None) == -1
    assert lib.hdiff_cfg_ddim_step(p, p, p, None, p, p, p, 5, 1.8, 0, 0, None, 16, None) == -1
    assert lib.hdiff_cfg_ddim_step(p, p, p, None, p, p, p, 0, 1.8, 0, 0, p, 16, None) == -1
    assert b"bad sizes" in lib.hdiff_last_error()
    assert lib.hdiff_cfg_ddim_step(p, p, p, None, p, p, p, 5, 1.8, 0, 0, p, 0, None) == -1
    assert lib.hdiff_cfg_ddim_step_loop(None, None) == -1
    d = _capi.CfgDdimLoopDesc()
    assert lib.hdiff_cfg_ddim_step_loop(C.byref(d), None) == -1 and b"cfg_ddim_step_loop: null pointer" in lib.hdiff_last_error()
    d.x = d.eps_c = d.eps_u = d.x_next = d.tab = d.step_ptr = d.nan_flag = d.done_counter = p
    d.nsteps, d.n = 0, 16
    assert lib.hdiff_cfg_ddim_step_loop(C.byref(d), None) == -1 and b"bad sizes" in lib.hdiff_last_error()
    d.nsteps, d.n = 5, 0
    assert lib.hdiff_cfg_ddim_step_loop(C.byref(d), None) == -1
    d.n, d.t_count = 16, 4                        # a time vector to fill, but neither it nor the time-step table is given
    assert lib.hdiff_cfg_ddim_step_loop(C.byref(d), None) == -1
    d.t_next = p                                  # ... the table alone is missing
    assert lib.hdiff_cfg_ddim_step_loop(C.byref(d), None) == -1
    d.t_count = -1
    assert lib.hdiff_cfg_ddim_step_loop(C.byref(d), None) == -1
