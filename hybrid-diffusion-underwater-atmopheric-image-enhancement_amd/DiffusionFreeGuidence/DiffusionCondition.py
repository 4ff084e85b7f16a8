"""Drop-in for the reference's ``DiffusionFreeGuidence/DiffusionCondition.py``: ``extract``, ``GaussianDiffusionTrainer``
(Algorithm 1) and ``GaussianDiffusionSampler`` (Algorithm 2, classifier-free guidance) with the same constructor /
``forward`` signatures, registered float64 buffers and error behaviour.

What differs underneath (reference lines in brackets):
  * the cond + uncond denoiser calls of one step [:76-77] run as ONE 2B-batched UNet plan (labels = [labels; 0]);
  * CFG combine, posterior mean, noise add and the NaN check [:78-79, :91-96] are one kernel (``hdiff_ddpm_step``);
  * one whole denoising step is captured into a hipGraph and replayed T times with a device-resident step counter
    [:87-96]; the per-step ``print`` [:88] is dropped and the per-step NaN ``assert`` [:96] is evaluated once after the
    loop from a device flag (same ``AssertionError("nan in tensor.")``);
  * per-step noise is drawn in-kernel (Philox4x32-10 + Box-Muller) from a seed taken from torch's default generator,
    so ``torch.manual_seed`` still makes sampling reproducible.

What is added to the reference's surface: ``GaussianDiffusionSampler.forward(..., ddim_steps=S)`` (or ``timesteps=[...]``) samples
in S <= T model evaluations with the strided DDIM update (Song et al. 2021) under the same guidance, from the same captured 2B step
with ``hdiff_cfg_ddim_step_loop`` as its one update kernel; ``ddim_timesteps`` and ``ddim_table`` are its schedule, usable on the CPU.
``solver="dpmpp2m"`` replaces that first-order update by DPM-Solver++(2M) (Lu et al. 2022: data prediction, multistep) -- still one
model evaluation and ONE update kernel per step (``hdiff_cfg_dpmpp_step_loop``), one more state tensor -- on the logSNR-uniform time
steps of ``logsnr_timesteps``, with the coefficients of ``dpmpp_table``.  The four schedule functions live in ``schedules.py``
(CPU-only, shared with the image-conditioned sampler) and are re-exported here; every update kernel of both samplers is in
``csrc/sampler_step.hip``.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F
import warnings

from .. import _capi
from .. import engine as E
from ..engine import gpu_input as _gpu_input, index_vector as _timesteps
from ..schedules import (_checked_timesteps, check_solver_spacing, ddim_table, ddim_timesteps, dpmpp_table, logsnr_timesteps,
                         spacing_of)


__all__ = ["extract", "GaussianDiffusionTrainer", "GaussianDiffusionSampler", "ddim_timesteps", "ddim_table", "logsnr_timesteps",
           "dpmpp_table"]

def extract(v, t, x_shape):
    """Coefficients at the given timesteps, cast float64 -> fp32 AFTER the gather, shaped [B,1,1,...] (reference :9-16)."""
    out = torch.gather(v, index=t, dim=0).float().to(t.device)
    return out.view([t.shape[0]] + [1] * (len(x_shape) - 1))


def _stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


class GaussianDiffusionTrainer(nn.Module):
    """forward(x_0, labels) -> unreduced squared error of the eps prediction (reference :19-46)."""

    def __init__(self, model, beta_1, beta_T, T):
        super().__init__()
        self.model = model
        self.T = T
        self.register_buffer('betas', torch.linspace(beta_1, beta_T, T).double())
        alphas_bar = torch.cumprod(1. - self.betas, dim=0)
        self.register_buffer('sqrt_alphas_bar', torch.sqrt(alphas_bar))
        self.register_buffer('sqrt_one_minus_alphas_bar', torch.sqrt(1. - alphas_bar))

    def forward(self, x_0, labels, *, t=None, noise=None):
        """``t`` / ``noise`` may be injected (parity tests); by default they are drawn exactly where the reference
        draws them (``torch.randint`` then ``torch.randn_like``, reference :41-42)."""
        x_0, labels = _gpu_input(x_0, "x_0"), _gpu_input(labels, "labels")
        lib = _capi.lib()
        B = int(x_0.shape[0])
        if t is None:
            t = torch.randint(self.T, size=(B,), device=x_0.device)     # in range by construction: no device->host read
        else:
            t = _timesteps(t, self.T, x_0.device)                        # a caller's vector is validated like torch.gather would
        if noise is None:
            noise = torch.randn_like(x_0)
        noise = _gpu_input(noise, "noise")
        assert noise.shape == x_0.shape
        sa, sb = self.sqrt_alphas_bar.float(), self.sqrt_one_minus_alphas_bar.float()
        x_t = torch.empty_like(x_0)
        with torch.cuda.device(x_0.device):
            s = _stream(x_0.device)
            _capi.check(lib.hdiff_q_sample(x_0.data_ptr(), noise.data_ptr(), t.data_ptr(), sa.data_ptr(), sb.data_ptr(),
                                           x_t.data_ptr(), B, x_0.numel() // B, self.T, s), "q_sample")
            eps_hat = self.model(x_t, t, labels)
            if eps_hat.requires_grad:
                from ..autograd import sq_err_with_grad
                return sq_err_with_grad(eps_hat, noise)
            loss = torch.empty_like(x_0)
            _capi.check(lib.hdiff_sq_err(eps_hat.data_ptr(), noise.data_ptr(), loss.data_ptr(), x_0.numel(), s), "sq_err")
            return loss


class _SamplerPlan:
    """One captured denoising step for a fixed (B, H, W): 2B UNet -> fused DDPM update (which also prepares the next step)."""

    def __init__(self, sampler: "GaussianDiffusionSampler", B: int, H: int, W: int, device):
        model = sampler.model
        self.unet = model.plan_for(2 * B, H, W, device)
        up = self.unet
        n = B * 3 * H * W
        dev = device
        self.x = torch.empty(B, 3, H, W, device=dev)
        self.noise = torch.empty(B, 3, H, W, device=dev)
        self.x0_prev = None                                              # the x0 history of solver="dpmpp2m", allocated on first use
        self.step = torch.zeros(1, dtype=torch.int32, device=dev)
        self.nan_flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self.done = torch.zeros(1, dtype=torch.int32, device=dev)       # finished-workgroup counter of the fused update
        var = torch.cat([sampler.posterior_var[1:2], sampler.betas[1:]])                 # reference :74
        self.c1 = sampler.coeff1.float().contiguous()                                     # extract(): f64 -> f32
        self.c2 = sampler.coeff2.float().contiguous()
        self.sigma = torch.sqrt(var.float()).contiguous()                                 # sqrt on the fp32 value (:95)
        self.seed = 0
        self.B, self.n = B, n
        self._variants = {}
        self._sampler = sampler

    def _loop_fields(self, d):
        """What the three loop descriptors share: the state and the two eps halves, guidance, the flags, and the bookkeeping --
        x_next into both halves of the UNet's input, the device-resident step, the next time vector."""
        up, n = self.unet, self.n
        eps = up.out
        d.x, d.eps_c, d.eps_u = self.x.data_ptr(), eps.data_ptr(), eps.data_ptr() + 4 * n
        d.x_next = self.x.data_ptr()
        d.step_ptr, d.w = self.step.data_ptr(), float(self._sampler.w)
        d.nan_flag, d.n = self.nan_flag.data_ptr(), n
        d.x_dup0, d.x_dup1 = up.x.data_ptr(), up.x.data_ptr() + 4 * n
        d.t_next, d.t_count = up.t.data_ptr(), 2 * self.B
        d.done_counter = self.done.data_ptr()
        return d

    def _noise_fields(self, d, inject_noise: bool):
        """The injected noise buffer (else the kernel draws its own from the seed) of the two descriptors that add noise."""
        d.noise, d.seed = (self.noise.data_ptr() if inject_noise else None), self.seed
        return d

    def _build(self, inject_noise: bool, ddim=None, solver: str = "ddim") -> E.Plan:
        """One denoising step = the 2B UNet launches + ONE fused update kernel.  The update also writes x_next into both
        halves of the UNet's input, decrements the device-resident step and refills the time vector, so nothing else has to run
        between two replays; `reset()` puts the loop state at its start.  Without ``ddim`` the ancestral step
        (hdiff_ddpm_step_loop: the counter is the time step).  With ``ddim = (timesteps, eta, clip_x0)`` the strided step: the
        counter is the position k in ``timesteps``, the time vector tau_k, the update hdiff_cfg_ddim_step_loop or, for
        ``solver="dpmpp2m"``, hdiff_cfg_dpmpp_step_loop -- whose x0 history (read from the second step on, and written) the plan owns."""
        dev = self.x.device
        p = E.Plan(dev)
        p.ops.extend(self.unet.plan.ops)
        if ddim is None:
            d = self._noise_fields(self._loop_fields(_capi.DdpmLoopDesc()), inject_noise)
            d.coeff1, d.coeff2, d.sigma = self.c1.data_ptr(), self.c2.data_ptr(), self.sigma.data_ptr()
            d.T = int(self._sampler.T)
            p.keep(d)
            p.call("hdiff_ddpm_step_loop", C.byref(d))
            return p
        timesteps, eta, clip_x0 = ddim
        dpmpp = solver == "dpmpp2m"
        tab = dpmpp_table(self._sampler.betas, timesteps) if dpmpp else ddim_table(self._sampler.betas, timesteps, eta)
        tab = tab.float().contiguous().to(dev)                          # f64 -> f32 once per entry
        t_tab = torch.tensor(timesteps, dtype=torch.int64, device=dev)
        if dpmpp:
            if self.x0_prev is None:
                self.x0_prev = torch.empty_like(self.x)
            d = self._loop_fields(_capi.CfgDpmppLoopDesc())
            d.x0_prev = self.x0_prev.data_ptr()
        else:
            d = self._noise_fields(self._loop_fields(_capi.CfgDdimLoopDesc()), inject_noise)
        d.tab, d.t_tab = tab.data_ptr(), t_tab.data_ptr()
        d.nsteps, d.clip_x0 = len(timesteps), int(bool(clip_x0))
        p.keep((d, tab, t_tab))                    # the tables live exactly as long as the step that reads them
        p.call("hdiff_cfg_dpmpp_step_loop" if dpmpp else "hdiff_cfg_ddim_step_loop", C.byref(d))
        return p

    def reset(self, x_T: torch.Tensor, labels: torch.Tensor, step: Optional[int] = None, t: Optional[int] = None) -> None:
        """Loop state at its start: x = x_T (also in both halves of the UNet input), labels = [labels; 0] (reference :76-77),
        the time vector and the device-resident step at T - 1 (or `step`), flags cleared.  The strided loop counts positions:
        `step` = S - 1 and the time vector at `t` = tau_(S-1)."""
        T = int(self._sampler.T)
        step = T - 1 if step is None else int(step)
        self.x.copy_(x_T)
        self.unet.x[:self.B].copy_(x_T)
        self.unet.x[self.B:].copy_(x_T)
        self.unet.labels.copy_(torch.cat([labels, torch.zeros_like(labels)], dim=0))
        self.unet.t.fill_(step if t is None else int(t))
        self.step.fill_(step)
        self.nan_flag.zero_()
        self.done.zero_()

    def variant(self, inject_noise: bool, seed: int, ddim=None, solver: str = "ddim") -> E.Plan:
        # the guidance weight is a launch argument of the fused update: the reference reads self.w on every step (:78), so
        # a changed sampler.w must rebuild the captured step.  ddim = (timesteps, eta, clip_x0) selects the strided step, solver
        # its update.
        key = (inject_noise, seed if not inject_noise else 0, _capi.lib().hdiff_get_contraction_mode(),
               float(self._sampler.w), ddim, solver)
        if key not in self._variants:
            self.seed = seed
            self._variants.clear()          # a graph bakes its seed (and the contraction mode): keep one live variant
            self._variants[key] = self._build(inject_noise, ddim, solver)
        return self._variants[key]


class GaussianDiffusionSampler(nn.Module):
    """forward(x_T, labels) -> x_0 clipped to [-1, 1] by T ancestral steps with classifier-free guidance (reference :49-98)."""

    def __init__(self, model, beta_1, beta_T, T, w=0.):
        super().__init__()
        self.model = model
        self.T = T
        self.w = w
        self.register_buffer('betas', torch.linspace(beta_1, beta_T, T).double())
        alphas = 1. - self.betas
        alphas_bar = torch.cumprod(alphas, dim=0)
        alphas_bar_prev = F.pad(alphas_bar, [1, 0], value=1)[:T]
        self.register_buffer('coeff1', torch.sqrt(1. / alphas))
        self.register_buffer('coeff2', self.coeff1 * (1. - alphas) / torch.sqrt(1. - alphas_bar))
        self.register_buffer('posterior_var', self.betas * (1. - alphas_bar_prev) / (1. - alphas_bar))
        self.use_graph = True
        self._splans = {}

    # -- single-step API of the reference -----------------------------------------------------------------------------
    def predict_xt_prev_mean_from_eps(self, x_t, t, eps):
        assert x_t.shape == eps.shape
        x_t, eps = _gpu_input(x_t, "x_t"), _gpu_input(eps, "eps")
        t = _timesteps(t, self.T, x_t.device)
        lib = _capi.lib()
        B = int(x_t.shape[0])
        c1 = self.coeff1.float()
        neg_c2 = -(self.coeff2.float())
        out = torch.empty_like(x_t)
        # coeff1[t]*x_t - coeff2[t]*eps  ==  coeff1[t]*x_t + (-coeff2[t])*eps with identical roundings
        with torch.cuda.device(x_t.device):
            _capi.check(lib.hdiff_q_sample(x_t.data_ptr(), eps.data_ptr(), t.data_ptr(), c1.data_ptr(), neg_c2.data_ptr(),
                                           out.data_ptr(), B, x_t.numel() // B, self.T, _stream(x_t.device)),
                        "posterior_mean")
        return out

    def _paired_eps(self, x_t, t, labels):
        """cond and uncond denoiser outputs from one 2B-batched launch sequence (reference :76-77)."""
        x2 = torch.cat([x_t, x_t], dim=0)
        t2 = torch.cat([t, t], dim=0)
        l2 = torch.cat([labels, torch.zeros_like(labels)], dim=0)
        e2 = self.model(x2, t2, l2)
        B = x_t.shape[0]
        return e2[:B], e2[B:]

    def p_mean_variance(self, x_t, t, labels):
        x_t, labels = _gpu_input(x_t, "x_t"), _gpu_input(labels, "labels")
        t = _timesteps(t, self.T, x_t.device)
        var = torch.cat([self.posterior_var[1:2], self.betas[1:]])
        var = extract(var, t, x_t.shape)
        eps_c, eps_u = self._paired_eps(x_t, t, labels)
        lib = _capi.lib()
        eps = torch.empty_like(x_t)
        with torch.cuda.device(x_t.device):
            _capi.check(lib.hdiff_axpby(C.c_float(1. + self.w), eps_c.contiguous().data_ptr(), C.c_float(-self.w),
                                        eps_u.contiguous().data_ptr(), eps.data_ptr(), x_t.numel(), _stream(x_t.device)),
                        "cfg_combine")
        return self.predict_xt_prev_mean_from_eps(x_t, t, eps=eps), var

    # -- the loop -----------------------------------------------------------------------------------------------------
    def forward(self, x_T, labels, *, ddim_steps: Optional[int] = None, eta: float = 0.0,
                timesteps: Optional[Sequence[int]] = None, clip_x0: bool = False, noise_by_step=None,
                trajectory: Optional[List[torch.Tensor]] = None, solver: str = "ddim", spacing: Optional[str] = None):
        """``noise_by_step[time_step]`` injects the per-step z (parity tests); ``trajectory`` collects the pre-clip
        x_t after every step.  Both default to the reference behaviour.

        ``ddim_steps=S`` (the time steps of ``ddim_timesteps(T, S)``) or an explicit strictly increasing ``timesteps`` list
        switches to the strided DDIM sampler: S model evaluations instead of T, same guidance, same 2B plan and graph replay.
        ``eta`` scales the step noise (0: deterministic, no seed is drawn; 1: posterior-variance ancestral steps -- ``ddim_table``),
        ``clip_x0`` clamps the predicted x_0 to [-1, 1] before it is used.  In this mode ``noise_by_step[k]`` is indexed by the
        POSITION k in the time-step list (S entries, entry 0 unused) and ``trajectory`` receives S states.  Without
        ``ddim_steps`` / ``timesteps`` the T-step ancestral loop of the reference runs.

        ``solver`` ("ddim" or "dpmpp2m") chooses the update of the strided sampler: "dpmpp2m" is DPM-Solver++(2M) (``dpmpp_table``),
        second order at the same one model evaluation per step; it is the deterministic solver, so it takes neither ``eta != 0``
        nor ``noise_by_step``.  ``spacing`` ("uniform": ``ddim_timesteps``; "logsnr": ``logsnr_timesteps(betas, S)``) chooses the
        time steps of ``ddim_steps=S``; ``None`` is uniform for "ddim" and logsnr for "dpmpp2m".  It does not go with an explicit
        ``timesteps`` list, and neither argument goes without ``ddim_steps`` / ``timesteps``."""
        ddim, solver = self._ddim_arguments(ddim_steps, eta, timesteps, clip_x0, noise_by_step, solver, spacing)
        x_T, labels = _gpu_input(x_T, "x_T"), _gpu_input(labels, "labels")
        if torch.is_grad_enabled():
            # The reference runs here too (DiffusionCondition.py:82-98) and records an autograd graph through all 2T model
            # evaluations, which nothing in its callers ever differentiates (TrainCondition.eval samples under no_grad).
            # The loop here is an inference loop: it runs without a graph and hands back a detached tensor.  A caller that
            # asks for a gradient with respect to x_T clearly expects that graph: refused; enabled autograd with trainable
            # parameters alone: said once per sampler instance.
            if x_T.requires_grad:
                raise RuntimeError("GaussianDiffusionSampler.forward: x_T requires grad, but the denoising loop runs under "
                                   "torch.no_grad() and cannot be differentiated (the reference would record a graph through all "
                                   "2T model evaluations); detach x_T or call under torch.no_grad()")
            if any(p.requires_grad for p in self.model.parameters()) and not getattr(self, "_warned_grad", False):
                self._warned_grad = True
                warnings.warn("GaussianDiffusionSampler.forward was called with autograd enabled: the denoising loop runs under "
                              "torch.no_grad() and returns a tensor without grad_fn (the reference would record a graph "
                              "through all 2T model evaluations)", RuntimeWarning, stacklevel=2)
        with torch.no_grad(), torch.cuda.device(x_T.device):
            return self._forward(x_T, labels, noise_by_step, trajectory, ddim, solver)

    def _ddim_arguments(self, ddim_steps, eta, timesteps, clip_x0, noise_by_step, solver="ddim", spacing=None):
        """-> (None for the ancestral loop, else the validated (timesteps, eta, clip_x0) of the strided one; its solver);
        ``ValueError`` otherwise.  Looks at no device."""
        check_solver_spacing(solver, spacing)
        if ddim_steps is None and timesteps is None:
            if float(eta) != 0.0 or clip_x0:
                raise ValueError("eta / clip_x0 belong to the strided sampler: give ddim_steps or timesteps with them")
            if solver != "ddim" or spacing is not None:
                raise ValueError("solver / spacing belong to the strided sampler: give ddim_steps or timesteps with them")
            return None, solver
        if ddim_steps is not None and timesteps is not None:
            raise ValueError("give ddim_steps or timesteps, not both")
        if timesteps is not None:
            if spacing is not None:
                raise ValueError("spacing chooses the time steps of ddim_steps: it does not go with an explicit timesteps list")
            tau = _checked_timesteps(timesteps, int(self.T))
        elif spacing_of(solver, spacing) == "logsnr":
            tau = tuple(logsnr_timesteps(self.betas, ddim_steps))
        else:
            tau = tuple(ddim_timesteps(self.T, ddim_steps))
        eta = float(eta)
        if not eta >= 0.0:
            raise ValueError(f"eta must be >= 0, got {eta}")
        if solver == "dpmpp2m" and (eta != 0.0 or noise_by_step is not None):
            raise ValueError("solver='dpmpp2m' is the deterministic solver: it takes neither eta != 0 nor noise_by_step")
        if noise_by_step is not None and len(noise_by_step) != len(tau):
            raise ValueError(f"noise_by_step has {len(noise_by_step)} entries for {len(tau)} time steps (one per position, "
                             "entry 0 unused)")
        return (tau, eta, bool(clip_x0)), solver

    def _forward(self, x_T, labels, noise_by_step, trajectory, ddim=None, solver="ddim"):
        lib = _capi.lib()
        B, Cx, H, W = (int(v) for v in x_T.shape)
        dev = x_T.device
        key = (B, H, W, str(dev))
        sp = self._splans.get(key)
        if sp is None or sp.unet is not self.model.plan_for(2 * B, H, W, dev):
            sp = _SamplerPlan(self, B, H, W, dev)
            self._splans = {key: sp}
        # One pack per call is nothing against T steps, and it closes the one hole of version-keyed staleness: a write through
        # ``p.data`` (EMA swaps, ``dist.broadcast(p.data)``) does not bump ``p._version``.
        sp.unet.plan.pack_weights()
        self.model.check_indices(torch.zeros_like(labels), labels)
        inject = noise_by_step is not None
        if ddim is None:
            seed = 0 if inject else int(torch.empty((), dtype=torch.int64).random_().item())
            plan = sp.variant(inject, seed)
            sp.reset(x_T, labels)
            steps = self.T
        else:
            tau, eta, _ = ddim
            # the deterministic sampler consumes no randomness: torch's generator is left where it was
            seed = 0 if inject or eta == 0.0 else int(torch.empty((), dtype=torch.int64).random_().item())
            plan = sp.variant(inject, seed, ddim, solver)
            steps = len(tau)
            sp.reset(x_T, labels, step=steps - 1, t=tau[-1])
        graphed = self.use_graph and trajectory is None
        if graphed:
            plan.capture()
        for time_step in reversed(range(steps)):          # the strided loop counts positions k in its time-step list
            if inject and time_step > 0:
                sp.noise.copy_(noise_by_step[time_step])
            if graphed:
                plan.replay()
            else:
                plan.run()
            if trajectory is not None:
                trajectory.append(sp.x.clone())
        assert int(sp.nan_flag.item()) == 0, "nan in tensor."
        out = torch.empty_like(x_T)
        _capi.check(lib.hdiff_clip(sp.x.data_ptr(), out.data_ptr(), C.c_float(-1.0), C.c_float(1.0), x_T.numel(),
                                   _stream(dev)), "clip")
        return out
