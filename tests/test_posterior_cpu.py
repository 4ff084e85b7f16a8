"""CPU-only checks of multi-sample posterior sampling (``GaussianDiffusionSampler.posterior`` / ``forward(eta=)``): the per-sample seed
against its definition (tests/_posterior_def.py) and known answers, the table rows with ``eta``, the argument errors, the lines of
``res.txt`` under ``samples=``, and the agreement of header, library and binding."""
import math
import os
import re
import subprocess

import pytest
import torch

import hdiff_amd
from hdiff_amd import _capi
from hdiff_amd import schedules
from hdiff_amd.diffusion import Diffusion as DD
from hdiff_amd.diffusion import Evaluate as EV

import _posterior_def as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("hdiff_randn_rows", "hdiff_ddim_eta_step", "hdiff_sample_stats")
B1, BT, T = 1e-4, 0.02, 1000


def _sampler():
    return DD.GaussianDiffusionSampler(torch.nn.Identity(), B1, BT, T)


# ----------------------------------------------------------------------------------------------------------------------
# seeds
# ----------------------------------------------------------------------------------------------------------------------
def test_posterior_seed_known_answers():
    assert P.mix(0) == 0xE220A8397B1DCDAF                       # the first output of splitmix64 seeded with 0 (Vigna's reference)
    known = {(0, 0, 0): 0x238275BC38FCBE91, (0, 0, 1): 0x2F32A78496C67C60, (0, 1, 0): 0x44E5B98100C67FB0,
             (1, 0, 0): 0xB18A02F46D8D86C3, (2 ** 63 + 5, 4095, 63): 0x9C0FA3D317553285, (7, 123456789, 3): 0x60A64F0429879FD2}
    for args, want in known.items():
        assert schedules.posterior_seed(*args) == want == P.seed_of(*args), args
    assert DD.posterior_seed is schedules.posterior_seed and "posterior_seed" in DD.__all__
    for bad in ((0.5, 0, 0), (0, "1", 0), (0, 0, True)):
        with pytest.raises((ValueError, TypeError)):
            schedules.posterior_seed(*bad)


@pytest.mark.parametrize("seed", [0, 1, 2 ** 63 + 5])
def test_posterior_seed_distinct_over_images_and_replicas(seed):
    got = {schedules.posterior_seed(seed, i, r) for i in range(4096) for r in range(64)}
    assert len(got) == 4096 * 64
    assert all(0 <= v < 2 ** 64 for v in got)


def test_posterior_seed_distinct_over_seeds():
    got = {schedules.posterior_seed(s, i, r) for s in range(8) for i in range(256) for r in range(16)}
    assert len(got) == 8 * 256 * 16


# ----------------------------------------------------------------------------------------------------------------------
# the table
# ----------------------------------------------------------------------------------------------------------------------
EPS32 = 2.0 ** -24


def _bounds(betas, tau, eta):
    """Per entry, how far the fp32 program may land from the float64 formula.  Every ``1 - x`` of fp32 values is off by at most
    4 EPS32 in absolute terms (x rounded, its inputs rounded, the difference rounded; x <= 1); a product, quotient or square root adds
    a relative EPS32 each.  u = 1 - a / a', v = 1 - a', w = 1 - a;  c1 = eta sqrt(u v / w),  c2 = sqrt(v - c1^2)."""
    ab = torch.cumprod(1.0 - betas.double(), dim=0)
    out = []
    for k, t in enumerate(tau):
        a, an = float(ab[t + 1]), float(ab[tau[k - 1] + 1] if k > 0 else ab[0])
        u, v, w = 1 - a / an, 1 - an, 1 - a
        rel = lambda x: 4 * EPS32 / x                                                                # noqa: E731
        c1 = eta * math.sqrt(u * v / w)
        e_c1 = c1 * (0.5 * (rel(u) + rel(v) + rel(w)) + 6 * EPS32)
        c2sq = v - c1 * c1
        e_c2 = math.sqrt(c2sq) * (0.5 * (4 * EPS32 + 2 * c1 * e_c1 + 2 * EPS32 * c1 * c1 + EPS32 * c2sq) / c2sq + EPS32)
        out.append([math.sqrt(w) * (0.5 * rel(w) + EPS32), math.sqrt(a) * 2 * EPS32, math.sqrt(an) * 2 * EPS32, e_c1, e_c2])
    return torch.tensor(out, dtype=torch.float64)


@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("steps", [4, 10, "list"])
def test_eta_table_against_the_formula(eta, steps):
    s = _sampler()
    seq = [0, 3, 40, 500, 998] if steps == "list" else None
    tau = seq if seq is not None else list(range(0, 1000, int(1000 / steps)))
    tab, t_tab = DD._ddim_tables(s, None if seq else steps, "cpu", seq, eta)
    assert tab.dtype == torch.float32 and tuple(tab.shape) == (len(tau), 5) and t_tab.tolist() == tau
    want = P.eta_table(s.betas, tau, eta)
    err, lim = (tab.double() - want).abs(), _bounds(s.betas, tau, eta)
    assert bool((err <= lim).all()), (err / lim).max()
    if eta == 0:
        assert bool((tab[:, 3] == 0).all())


@pytest.mark.parametrize("steps", [4, 5, 10, "list"])
def test_eta_zero_rows_are_todays_bit_for_bit(steps):
    s = _sampler()
    seq = [0, 3, 40, 500, 998] if steps == "list" else None
    today, t_today = DD._ddim_tables(s, None if seq else steps, "cpu", seq)
    with_eta, t_eta = DD._ddim_tables(s, None if seq else steps, "cpu", seq, 0.0)
    assert tuple(today.shape) == (len(t_today), 4)
    assert torch.equal(with_eta[:, [0, 1, 2, 4]], today) and torch.equal(t_eta, t_today)
    if steps == 5:                          # and today's is the oracle's, as before
        from oracle import cpu_path_b as OB
        assert torch.equal(today.flip(0), OB.ddim_coefficients(OB.sampler_schedule(B1, BT, T), 5))


def test_eta_too_large_is_refused():
    with pytest.raises(ValueError, match="eta"):
        DD._ddim_tables(_sampler(), 4, "cpu", None, 50.0)


# ----------------------------------------------------------------------------------------------------------------------
# arguments (all refused before anything looks at a device)
# ----------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    s, img = _sampler(), torch.zeros(1, 3, 16, 16)
    kw = dict(ddim=True, ddim_step=4)
    with pytest.raises(ValueError, match="tile"):
        s(img, eta=0.5, tile=16, **kw)
    with pytest.raises(ValueError, match="tile"):
        s(img, seed=1, tile=16, **kw)
    with pytest.raises(ValueError, match="solver"):
        s(img, eta=0.5, solver="dpmpp2m", **kw)
    with pytest.raises(ValueError, match="ddim=True"):
        s(img, eta=0.5)
    with pytest.raises(ValueError, match="ddim=True"):
        s(img, seed=3)
    with pytest.raises(ValueError, match="seed"):
        s(img, image_ids=[0], **kw)
    for bad in (-0.1, float("nan"), float("inf"), -float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="eta"):
            s(img, eta=bad, **kw)
        with pytest.raises(ValueError, match="eta"):
            s.posterior(img, 2, ddim_step=4, eta=bad)
    for bad in (0, -1, 1.5, None, True):
        with pytest.raises(ValueError, match="samples"):
            s.posterior(img, bad, ddim_step=4)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="samples"):
            EV.evaluate(s, [], ddim_step=4, samples=bad)
    with pytest.raises(ValueError, match="solver"):
        s.posterior(img, 2, ddim_step=4, eta=0.5, solver="dpmpp2m")
    with pytest.raises(ValueError, match="sample_batch"):
        s.posterior(img, 2, ddim_step=4, sample_batch=0)
    with pytest.raises(ValueError, match="samples"):
        EV.evaluate(s, [], ddim_step=4, eta=0.5)
    with pytest.raises(ValueError, match="tile"):
        EV.evaluate(s, [], ddim_step=4, samples=2, tile=16)
    from hdiff_amd import transfer
    with pytest.raises(ValueError, match="samples"):
        transfer.GuidedEnhancer(s, samples=0)
    with pytest.raises(ValueError, match="samples"):
        transfer.GuidedEnhancer(s, eta=0.5)
    with pytest.raises(ValueError):
        DD._row_seeds(0, [0, 1, 2], 2)


def test_row_seeds_layout():
    rows = DD._row_seeds(5, [7, 9], 2, 3)
    assert rows == [P.as_int64(P.seed_of(5, i, r)) for i in (7, 9) for r in range(3)]
    assert DD._row_seeds(5, None, 2) == [P.as_int64(P.seed_of(5, i, 0)) for i in (0, 1)]
    assert DD._row_seeds(5, [(7, 2), 9], 2) == [P.as_int64(P.seed_of(5, 7, 2)), P.as_int64(P.seed_of(5, 9, 0))]
    assert all(-2 ** 63 <= v < 2 ** 63 for v in rows)


# ----------------------------------------------------------------------------------------------------------------------
# res.txt
# ----------------------------------------------------------------------------------------------------------------------
def test_res_txt_lines_in_order(tmp_path):
    cols = ("psnr", "ssim", "uiqm", "uicm", "uism", "uiconm")
    result = {c: float(i) for i, c in enumerate(cols)}
    result.update(samples=3, per_sample={c: [1.0, 2.0, 3.0] for c in cols}, sample_avg={c: 2.0 + i for i, c in enumerate(cols)},
                  sample_std={c: 0.5 + i for i, c in enumerate(cols)}, uncertainty=0.125, fd=9.0, kid=8.0)
    today = EV.RES_KEYS + EV.RES_KEYS_DISTRIBUTION
    flat, keys = EV.sample_res_lines(result, today)
    path = os.path.join(tmp_path, "res.txt")
    EV.write_res(path, flat, keys)
    lines = [ln for ln in open(path).read().split("\n") if ln]
    names = [ln[:ln.index(":") + 1] for ln in lines]
    want = P.res_keys([k for k, _ in EV.RES_KEYS])
    # the set-level scores keep their place among today's lines and have no per-sample twin
    want = want[:6] + ["fd_orgin_avg:", "kid_orgin_avg:"] + want[6:]
    assert names == want
    assert names[:8] == [k for k, _ in today]
    values = dict(zip(names, (ln[ln.index(":") + 1:] for ln in lines)))
    assert values["samples:"] == "3" and values["uncertainty_avg:"] == "0.125"
    assert values["ssim_sample_avg:"] == "3.0" and values["ssim_sample_std:"] == "1.5"
    assert values["psnr_orgin_avg:"] == "0.0"


# ----------------------------------------------------------------------------------------------------------------------
# header, library, binding
# ----------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "hdiff.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(hdiff_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (hdiff_[a-z0-9_]+)", out))
    for name in NEW_SYMBOLS:
        assert name in declared and name in exported and name in _capi.EXPORTED_SYMBOLS, name
    lib = hdiff_amd.lib()
    assert lib.hdiff_abi_version() == 6          # symbols were added, nothing changed
    # the host-side argument checks answer without a device
    assert lib.hdiff_randn_rows(None, 1, 4, None, 0, None) != 0
    assert lib.hdiff_sample_stats(None, 1, 1, 4, None, None, None) != 0
    assert lib.hdiff_ddim_eta_step(None, None, None, None, None, None, 4, None, 1, None, 1, None) != 0
    assert b"null pointer" in lib.hdiff_last_error()
