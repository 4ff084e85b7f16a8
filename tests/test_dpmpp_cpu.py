"""CPU-only checks of DPM-Solver++(2M) sampling (``solver="dpmpp2m"`` of both samplers): the logSNR time-step rule, the coefficient
table against its definition (tests/_dpmpp_def.py), the identity of a first-order row with the DDIM update, the order of
convergence on an analytic model in float64, the argument errors of both public interfaces, the host-side argument checks of the C
entry points, and the agreement of header, library and binding."""
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
from hdiff_amd.diffusion import Diffusion as DD

import _dpmpp_def as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("hdiff_cfg_dpmpp_step", "hdiff_cfg_dpmpp_step_loop", "hdiff_dpmpp_step", "hdiff_tile_dpmpp_step")
T = 1000
BETAS = torch.linspace(1e-4, 0.02, T).double()


# ----------------------------------------------------------------------------------------------------------------------
# the grid
# ----------------------------------------------------------------------------------------------------------------------
def test_one_implementation_in_both_trees():
    assert DD.logsnr_timesteps is DC.logsnr_timesteps and DD.dpmpp_table is DC.dpmpp_table
    assert {"logsnr_timesteps", "dpmpp_table"} <= set(DC.__all__) and {"logsnr_timesteps", "dpmpp_table"} <= set(DD.__all__)


def test_schedules_module_is_cpu_only_and_shared():
    """``hdiff_amd.schedules`` is the one home of the schedule functions: both sampler modules re-export its objects, and importing
    it (in a fresh interpreter) loads neither the native library nor the engine."""
    from hdiff_amd import schedules
    for name in ("ddim_timesteps", "ddim_table", "logsnr_timesteps", "dpmpp_table"):
        assert getattr(DC, name) is getattr(schedules, name), name
    for name in ("logsnr_timesteps", "dpmpp_table"):
        assert getattr(DD, name) is getattr(schedules, name), name
    code = ("import sys; import hdiff_amd.schedules as S; from hdiff_amd import _capi; "
            "assert _capi._lib is None, 'libhdiff.so was loaded'; "
            "assert 'hdiff_amd.engine' not in sys.modules, 'engine was imported'; "
            "print(S.ddim_timesteps(1000, 4))")
    res = subprocess.run([os.sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert res.returncode == 0, res.stderr
    assert res.stdout.strip() == "[249, 499, 749, 999]"


def test_logsnr_prefixes():
    assert DC.logsnr_timesteps(BETAS, 10)[:5] == [0, 5, 22, 73, 202]
    assert DC.logsnr_timesteps(BETAS, 10, shift=1)[:5] == [0, 7, 31, 94, 240]
    assert DC.logsnr_timesteps(BETAS, 10) == P.logsnr_steps(BETAS, 10)
    assert DC.logsnr_timesteps(BETAS.float(), 10, 1) == P.logsnr_steps(BETAS.float(), 10, 1)      # any dtype: float64 inside


@pytest.mark.parametrize("shift", [0, 1])
def test_logsnr_counts_ends_and_collisions(shift):
    hi = T - 1 - shift
    ab = P.alphas_bar(BETAS)
    lam = P.lam_of(ab[shift:])
    for S in (1, 2, 10, 40, 50, hi + 1):
        tau = DC.logsnr_timesteps(BETAS, S, shift)
        assert len(tau) == S and all(isinstance(t, int) for t in tau), S
        assert tau[-1] == hi and (S == 1 or tau[0] == 0), (S, tau[:3], tau[-3:])
        assert all(b > a for a, b in zip(tau, tau[1:])), S
        if S in (40, 50):
            # the nearest indices collide near t = 0 (lam falls fastest there): the two passes are what separates them
            near = [int((lam - (lam[0] + (lam[hi] - lam[0]) * k / (S - 1))).abs().argmin()) for k in range(S)]
            if shift == 0:                                   # (with shift = 1 the first interval is wider: S = 40 has no collision)
                assert len(set(near)) < S, S
            assert tau == P.logsnr_steps(BETAS, S, shift), S
    assert DC.logsnr_timesteps(BETAS, hi + 1, shift) == list(range(hi + 1))


def test_logsnr_value_errors():
    for S, shift in ((0, 0), (-3, 0), (T + 1, 0), (T, 1), (2.5, 0), (True, 0), (10, -1), (10, 0.5), (1, T)):
        with pytest.raises(ValueError):
            DC.logsnr_timesteps(BETAS, S, shift)
    assert DC.logsnr_timesteps(BETAS, 10.0) == DC.logsnr_timesteps(BETAS, 10)          # an integral float is an integer


# ----------------------------------------------------------------------------------------------------------------------
# the table
# ----------------------------------------------------------------------------------------------------------------------
def _cases():
    ab0 = float(P.alphas_bar(BETAS)[0])
    return [(DC.logsnr_timesteps(BETAS, 10), 0, 1.0), (DC.logsnr_timesteps(BETAS, 40), 0, 1.0),
            (DC.logsnr_timesteps(BETAS, 10, 1), 1, ab0), (DC.logsnr_timesteps(BETAS, 20, 1), 1, ab0),
            (DC.ddim_timesteps(T, 8), 0, 1.0), (list(range(0, 1000, 100)), 1, ab0), ([3, 400], 0, 1.0), ([998], 1, ab0), ([999], 0, 1.0)]


def test_table_equals_the_definition():
    for tau, shift, final in _cases():
        got = DC.dpmpp_table(BETAS, tau, shift=shift, final_alpha_bar=final)
        want = P.table(BETAS, tau, shift, final)
        S = len(tau)
        assert got.dtype == torch.float64 and tuple(got.shape) == (S, 5)
        rel = ((got - want).abs() / want.abs().clamp(min=1e-300)).max().item()
        assert rel <= 1e-15, (tau[:4], shift, rel)
        assert got[S - 1, P.C_] == 0 and got[0, P.C_] == 0
        if S > 2:
            assert bool((got[1:S - 1, P.C_] != 0).all())
        if final == 1.0:
            assert got[0, 2:].tolist() == [0.0, 1.0, 0.0]            # exact, h never formed
        else:
            assert 0 < got[0, P.A_] < 1 and 0 < got[0, P.B_] < 1
        assert torch.isfinite(got).all()


def test_table_value_errors():
    for tau, shift, final in (([], 0, 1.0), ([5, 5], 0, 1.0), ([7, 3], 0, 1.0), ([-1, 3], 0, 1.0), ([0, T], 0, 1.0), ([0, T - 1], 1, 1.0),
                              ([1.5], 0, 1.0), ([3], 0, 0.0), ([3], 0, 1.5), ([3], -1, 1.0)):
        with pytest.raises(ValueError):
            DC.dpmpp_table(BETAS, tau, shift=shift, final_alpha_bar=final)


def test_first_order_rows_are_the_ddim_update():
    """With every C forced to 0 and B = g, the update A x + B x0 equals DDIM's eta = 0 update sqrt(a') x0 + sqrt(1 - a') eps, to 1e-13
    in float64 -- the identity the solver rests on."""
    g = torch.Generator().manual_seed(0)
    ab = P.alphas_bar(BETAS)
    worst = 0.0
    for shift, final in ((0, 1.0), (1, float(ab[0]))):
        for S in (10, 40):
            tau = DC.logsnr_timesteps(BETAS, S, shift)
            # first-order rows of every step: two-entry tables (row 1 = k = S-1 has no history, so it is first order)
            for k in range(S):
                pair = [tau[k - 1], tau[k]] if k > 0 else [tau[0], tau[1]]
                row = DC.dpmpp_table(BETAS, pair, shift=shift, final_alpha_bar=final)[1 if k > 0 else 0]
                assert row[P.C_] == 0
                a = ab[tau[k] + shift]
                ap = ab[tau[k - 1] + shift] if k > 0 else torch.tensor(final, dtype=torch.float64)
                x, eps = torch.randn(64, generator=g, dtype=torch.float64), torch.randn(64, generator=g, dtype=torch.float64)
                v, x0 = P.update(x, eps, None, row, False)
                ddim = torch.sqrt(ap) * x0 + torch.sqrt(1.0 - ap) * eps
                worst = max(worst, (v - ddim).abs().max().item())
    print(f"first-order row vs the ddim update, float64: max abs {worst:.2e}")
    assert worst <= 1e-13


# ----------------------------------------------------------------------------------------------------------------------
# convergence on the analytic model
# ----------------------------------------------------------------------------------------------------------------------
def _endpoint_errors(S, shift):
    """-> (ddim error, 2M error): max over the four start values of |x_end - exact| in float64, the package's own steps and table."""
    ab = P.alphas_bar(BETAS)
    final = 1.0 if shift == 0 else float(ab[0])
    tau = DC.logsnr_timesteps(BETAS, S, shift)
    tab = DC.dpmpp_table(BETAS, tau, shift=shift, final_alpha_bar=final)
    a_start = float(ab[tau[-1] + shift])
    e_ddim = e_2m = 0.0
    for start in P.START:
        x1 = x2 = torch.tensor(start, dtype=torch.float64)
        x0_prev = None
        for k in range(S - 1, -1, -1):
            a = float(ab[tau[k] + shift])
            ap = float(ab[tau[k - 1] + shift]) if k > 0 else final
            eps = P.gauss_eps(x1, a)
            x1 = (ap ** 0.5) * ((x1 - eps * (1 - a) ** 0.5) / a ** 0.5) + ((1 - ap) ** 0.5) * eps
            x2, x0_prev = P.update(x2, P.gauss_eps(x2, a), x0_prev, tab[k], False)
        exact = P.gauss_flow(start, a_start, final)
        e_ddim, e_2m = max(e_ddim, abs(float(x1) - exact)), max(e_2m, abs(float(x2) - exact))
    return e_ddim, e_2m


@pytest.mark.parametrize("shift", [0, 1])
def test_second_order_convergence(shift):
    err = {S: _endpoint_errors(S, shift) for S in (10, 20, 40)}
    for S, (d, m) in err.items():
        print(f"shift={shift} S={S}: ddim {d:.4g}  dpmpp2m {m:.4g}  ratio {d / m:.2f}")
    print(f"shift={shift}: err2m(20) / err2m(40) = {err[20][1] / err[40][1]:.2f}   errddim(20) / errddim(40) = {err[20][0] / err[40][0]:.2f}")
    for S in (10, 20):
        assert err[S][1] <= err[S][0] / 4, (S, err[S])
    assert err[20][1] / err[40][1] >= 3, err


# ----------------------------------------------------------------------------------------------------------------------
# arguments of both forwards: raised before a device is looked at (the inputs are CPU tensors)
# ----------------------------------------------------------------------------------------------------------------------
def test_tree_a_forward_arguments():
    sig = inspect.signature(DC.GaussianDiffusionSampler.forward)
    assert sig.parameters["solver"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["solver"].default == "ddim"
    assert sig.parameters["spacing"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["spacing"].default is None
    samp = DC.GaussianDiffusionSampler(torch.nn.Identity(), 1e-4, 0.02, 100, w=1.8)
    x, labels = torch.zeros(2, 3, 16, 16), torch.tensor([1, 2])
    z = [torch.zeros(2, 3, 16, 16)] * 4
    bad_calls = [dict(solver="dpmpp2m"), dict(spacing="logsnr"), dict(spacing="uniform"),                 # without a schedule
                 dict(ddim_steps=4, solver="heun"), dict(ddim_steps=4, solver=None), dict(ddim_steps=4, spacing="cosine"),
                 dict(timesteps=[3, 50, 99], spacing="logsnr"), dict(timesteps=[3, 50, 99], solver="dpmpp2m", spacing="uniform"),
                 dict(ddim_steps=4, solver="dpmpp2m", eta=0.5), dict(ddim_steps=4, solver="dpmpp2m", noise_by_step=z),
                 dict(ddim_steps=101, solver="dpmpp2m"), dict(ddim_steps=0, spacing="logsnr")]
    for kw in bad_calls:
        with torch.no_grad(), pytest.raises(ValueError):
            samp(x, labels, **kw)
    for kw in (dict(ddim_steps=4, solver="dpmpp2m"), dict(ddim_steps=4, solver="dpmpp2m", spacing="uniform", clip_x0=True),
               dict(ddim_steps=4, spacing="logsnr"), dict(timesteps=[3, 50, 99], solver="dpmpp2m"), dict(ddim_steps=4, solver="ddim"),
               dict(solver="ddim")):
        with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
            samp(x, labels, **kw)
    # the default spacing of each solver
    assert samp._ddim_arguments(8, 0.0, None, False, None, "dpmpp2m", None)[0][0] == tuple(DC.logsnr_timesteps(samp.betas, 8))
    assert samp._ddim_arguments(8, 0.0, None, False, None, "ddim", None)[0][0] == tuple(DC.ddim_timesteps(100, 8))
    assert samp._ddim_arguments(8, 0.0, None, False, None, "dpmpp2m", "uniform") == ((tuple(DC.ddim_timesteps(100, 8)), 0.0, False), "dpmpp2m")


def test_tree_b_forward_arguments():
    sig = inspect.signature(DD.GaussianDiffusionSampler.forward)
    for name, default in (("solver", "ddim"), ("spacing", None), ("timesteps", None)):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[name].default == default, name
    samp = DD.GaussianDiffusionSampler(torch.nn.Identity(), 1e-4, 0.02, 1000)
    x = torch.zeros(1, 3, 24, 40)
    bad_calls = [dict(solver="dpmpp2m"), dict(spacing="logsnr"), dict(timesteps=[0, 5]), dict(ddim_step=5, solver="dpmpp2m"),   # ddim=False
                 dict(ddim=True, ddim_step=5, solver="heun"), dict(ddim=True, ddim_step=5, spacing="cosine"),
                 dict(ddim=True, solver="dpmpp2m"), dict(ddim=True, spacing="logsnr"),
                 dict(ddim=True, ddim_step=5, timesteps=[0, 5]), dict(ddim=True, timesteps=[0, 5], spacing="uniform"),
                 dict(ddim=True, timesteps=[0, 999], solver="dpmpp2m"), dict(ddim=True, timesteps=[5, 5], solver="dpmpp2m"),
                 dict(ddim=True, timesteps=[], solver="dpmpp2m"), dict(ddim=True, timesteps=[-1, 5]),
                 dict(ddim=True, ddim_step=1000, solver="dpmpp2m"), dict(ddim=True, ddim_step=0, solver="dpmpp2m"),
                 dict(ddim=True, ddim_step=5, solver="dpmpp2m", tile=16, tile_overlap=9)]
    for kw in bad_calls:
        with torch.no_grad(), pytest.raises(ValueError):
            samp(x, **kw)
    for kw in (dict(ddim_step=5, solver="dpmpp2m"), dict(ddim_step=5, solver="dpmpp2m", spacing="uniform"),
               dict(ddim_step=5, spacing="logsnr"), dict(timesteps=[0, 7, 998], solver="dpmpp2m"), dict(timesteps=[0, 7, 998]),
               dict(ddim_step=5, solver="dpmpp2m", tile=16, tile_overlap=8, tile_batch=7), dict(ddim_step=5, solver="ddim")):
        with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
            samp(x, ddim=True, **kw)
    assert samp._solver_arguments(True, 5, "dpmpp2m", None, None) == tuple(DC.logsnr_timesteps(samp.betas, 5, shift=1))
    assert samp._solver_arguments(True, 5, "ddim", None, None) is None and samp._solver_arguments(True, 5, "dpmpp2m", "uniform", None) is None


# ----------------------------------------------------------------------------------------------------------------------
# the C ABI
# ----------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "hdiff.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(hdiff_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (hdiff_[a-z0-9_]+)", out))
    for name in NEW_SYMBOLS:
        assert name in declared and name in exported and name in _capi.EXPORTED_SYMBOLS, name
    assert "hdiff_cfg_dpmpp_loop_desc" in text
    assert hdiff_amd.lib().hdiff_abi_version() == 6          # symbols were added, nothing changed
    # the descriptor binding has the header's fields in the header's order
    body = re.search(r"typedef struct hdiff_cfg_dpmpp_loop_desc \{(.*?)\} hdiff_cfg_dpmpp_loop_desc;", text, flags=re.S).group(1)
    fields = re.findall(r"(\w+)\s*[;]", body)
    assert fields == [f[0] for f in _capi.CfgDpmppLoopDesc._fields_]


def test_argument_validation_without_gpu():
    """Null pointers and bad sizes are refused on the host, before any launch."""
    lib = hdiff_amd.lib()
    p = 1 << 20                                                # never dereferenced: the calls below fail their argument checks
    assert lib.hdiff_cfg_dpmpp_step(p, p, p, p, None, p, p, 4, C.c_double(0.0), 0, p, 16, None) == -1          # no history
    assert b"cfg_dpmpp_step" in lib.hdiff_last_error()
    assert lib.hdiff_cfg_dpmpp_step(p, p, p, p, p, p, p, 0, C.c_double(0.0), 0, p, 16, None) == -1             # no table rows
    assert lib.hdiff_cfg_dpmpp_step(p, p, p, p, p, p, p, 4, C.c_double(0.0), 0, p, 0, None) == -1              # n = 0
    assert lib.hdiff_cfg_dpmpp_step_loop(None, None) == -1
    d = _capi.CfgDpmppLoopDesc()
    for name in ("x", "eps_c", "eps_u", "x_next", "x0_prev", "tab", "step_ptr", "nan_flag"):
        setattr(d, name, p)
    d.nsteps, d.n = 4, 16
    assert lib.hdiff_cfg_dpmpp_step_loop(C.byref(d), None) == -1 and b"null pointer" in lib.hdiff_last_error()    # no done_counter
    d.done_counter, d.t_count = p, 4
    assert lib.hdiff_cfg_dpmpp_step_loop(C.byref(d), None) == -1 and b"bad sizes" in lib.hdiff_last_error()       # t_count without t_next
    assert lib.hdiff_dpmpp_step(p, p, p, None, p, p, 4, 0, p, 16, None) == -1 and b"dpmpp_step" in lib.hdiff_last_error()
    assert lib.hdiff_dpmpp_step(p, p, p, p, p, p, 4, 0, p, 0, None) == -1
    tile = [p] * 13 + [4, 0, p]
    assert lib.hdiff_tile_dpmpp_step(*tile, 2, 3, 24, 44, 2, 5, 32, 16, None) == -1 and b"tile_dpmpp_step" in lib.hdiff_last_error()
    assert lib.hdiff_tile_dpmpp_step(*([p, p, None] + [p] * 10 + [4, 0, p]), 2, 3, 24, 44, 2, 5, 16, 16, None) == -1
