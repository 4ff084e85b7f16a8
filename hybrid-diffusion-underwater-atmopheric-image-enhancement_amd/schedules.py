"""The time steps and coefficient tables of the samplers' strided loops, shared by the label-conditioned sampler
(``DiffusionFreeGuidence.DiffusionCondition``) and the image-conditioned one (``diffusion.Diffusion``, which reads
``alphas_bar[t + 1]``: ``shift=1``): ``ddim_timesteps`` / ``ddim_table`` of the strided DDIM update (Song et al. 2021),
``logsnr_timesteps`` / ``dpmpp_table`` of DPM-Solver++(2M) (Lu et al. 2022), the validation of ``solver`` / ``spacing`` /
``timesteps`` both ``forward`` signatures share, ``posterior_seed``, the seed of one sample of a multi-sample run, and what the
image-conditioned tree's ``prediction`` / ``loss_weighting`` arguments may be, with ``min_snr_weights``.  Everything here runs on the CPU in float64 and loads no native library; both
sampler modules re-export the public names."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

__all__ = ["SOLVERS", "SPACINGS", "PREDICTIONS", "LOSS_WEIGHTINGS", "ddim_timesteps", "ddim_table", "logsnr_timesteps", "dpmpp_table",
           "posterior_seed", "min_snr_weights"]

SOLVERS = ("ddim", "dpmpp2m")
SPACINGS = ("uniform", "logsnr")


def check_solver_spacing(solver, spacing) -> None:
    """``ValueError`` for a ``solver`` / ``spacing`` argument that names none of ``SOLVERS`` / ``SPACINGS`` (``spacing`` may be None)."""
    if solver not in SOLVERS:
        raise ValueError(f"solver must be one of {SOLVERS}, got {solver!r}")
    if spacing is not None and spacing not in SPACINGS:
        raise ValueError(f"spacing must be None or one of {SPACINGS}, got {spacing!r}")


def spacing_of(solver: str, spacing: Optional[str]) -> str:
    """The spacing that ``spacing=None`` stands for: uniform for "ddim", logsnr for "dpmpp2m"."""
    return spacing or ("logsnr" if solver == "dpmpp2m" else "uniform")


def ddim_timesteps(T: int, S: int) -> List[int]:
    """The S time steps a strided sampler visits out of T: ``tau_k = ((k + 1) * T) // S - 1`` for k = 0 .. S-1 in integer
    arithmetic -- strictly increasing for 1 <= S <= T, always ending at T - 1 (the step x_T belongs to); S = T gives 0 .. T-1,
    (1000, 50) gives 19, 39, ..., 999.  ``ValueError`` for S outside [1, T] or not an integer."""
    if int(S) != S or int(T) != T:
        raise ValueError(f"ddim_steps and T must be integers, got {S!r} out of {T!r}")
    T, S = int(T), int(S)
    if not 1 <= S <= T:
        raise ValueError(f"ddim_steps must lie in [1, T = {T}], got {S}")
    return [((k + 1) * T) // S - 1 for k in range(S)]


def _checked_timesteps(timesteps: Sequence[int], T: int) -> Tuple[int, ...]:
    given = list(timesteps)                    # once: a generator is consumed by the first pass over it
    tau = tuple(int(t) for t in given)
    if len(tau) < 1 or any(a != b for a, b in zip(tau, given)):
        raise ValueError("timesteps must be a non-empty list of integers")
    if tau[0] < 0 or tau[-1] >= T or any(b <= a for a, b in zip(tau, tau[1:])):
        raise ValueError(f"timesteps must be strictly increasing and lie in [0, T = {T}), got {list(tau)[:8]}"
                         f"{' ...' if len(tau) > 8 else ''}")
    return tau


def ddim_table(betas: torch.Tensor, timesteps: Sequence[int], eta: float = 0.0) -> torch.Tensor:
    """Coefficients of the strided DDIM update, float64 ``[S, 5]``, row k = ``(s1m, sa, san, c2, sigma)`` for the step from
    ``tau_k`` to ``tau_(k-1)``.  With ``ab = cumprod(1 - betas)``, ``a = ab[tau_k]`` and ``a' = ab[tau_(k-1)]`` (``a' = 1`` at k = 0):

        sigma = eta * sqrt((1 - a') / (1 - a)) * sqrt(1 - a / a')
        s1m = sqrt(1 - a),  sa = sqrt(a),  san = sqrt(a'),  c2 = sqrt(max(1 - a' - sigma^2, 0))

    and one step is ``x0 = (x - eps * s1m) / sa ; x' = san * x0 + c2 * eps + sigma * z``.  ``eta = 0`` is the deterministic DDIM;
    ``eta = 1`` at stride 1 is the ancestral sampler with the POSTERIOR variance (``sigma^2 == posterior_var``,
    ``san / sa == coeff1``, ``san * s1m / sa - c2 == coeff2``), not the reference's fixed-large variance.  Computed on the CPU."""
    b = torch.as_tensor(betas).detach().to(device="cpu", dtype=torch.float64)
    tau = _checked_timesteps(timesteps, int(b.numel()))
    eta = float(eta)
    if not eta >= 0.0:
        raise ValueError(f"eta must be >= 0, got {eta}")
    ab = torch.cumprod(1.0 - b, dim=0)
    idx = torch.tensor(tau, dtype=torch.int64)
    a = ab[idx]
    a_prev = torch.cat([torch.ones(1, dtype=torch.float64), a[:-1]])
    sigma = eta * torch.sqrt((1.0 - a_prev) / (1.0 - a)) * torch.sqrt(1.0 - a / a_prev)
    c2 = torch.sqrt(torch.clamp(1.0 - a_prev - sigma * sigma, min=0.0))
    return torch.stack([torch.sqrt(1.0 - a), torch.sqrt(a), torch.sqrt(a_prev), c2, sigma], dim=1)


def _alphas_bar(betas) -> torch.Tensor:
    return torch.cumprod(1.0 - torch.as_tensor(betas).detach().to(device="cpu", dtype=torch.float64).reshape(-1), dim=0)


def _int_shift(shift) -> int:
    if isinstance(shift, bool) or int(shift) != shift or int(shift) < 0:
        raise ValueError(f"shift must be an integer >= 0, got {shift!r}")
    return int(shift)


def logsnr_timesteps(betas, S: int, shift: int = 0) -> List[int]:
    """S time steps spaced uniformly in the half log signal-to-noise ratio ``lam[t] = 0.5 * log(ab / (1 - ab))`` at
    ``ab = cumprod(1 - betas)[t + shift]``, t = 0 .. hi = T - 1 - shift (``shift = 1``: the image-conditioned sampler, which reads
    ``alphas_bar[t + 1]``): the index nearest to each of the S targets between ``lam[0]`` and ``lam[hi]`` (the lowest on a tie), then
    made strictly increasing by a forward pass ``idx_k >= idx_(k-1) + 1``, a cap of the last at hi and a backward pass
    ``idx_k <= idx_(k+1) - 1``.  Always S entries, from 0 to hi; ``S = 1`` gives ``[hi]``.  A multistep solver needs such steps: on
    index-uniform ones the last logSNR interval of a linear-beta schedule is several times the one before it.  ``ValueError`` for S
    outside [1, hi + 1] or not an integer.  Computed on the CPU in float64."""
    shift = _int_shift(shift)
    ab = _alphas_bar(betas)
    hi = int(ab.numel()) - 1 - shift
    if isinstance(S, bool) or int(S) != S:
        raise ValueError(f"the number of steps must be an integer, got {S!r}")
    S = int(S)
    if hi < 0 or not 1 <= S <= hi + 1:
        raise ValueError(f"the number of steps must lie in [1, {hi + 1}], got {S}")
    if S == 1:
        return [hi]
    v = ab[shift:]
    lam = 0.5 * torch.log(v / (1.0 - v))
    idx = []
    for k in range(S):
        d = (lam - (lam[0] + (lam[hi] - lam[0]) * k / (S - 1))).abs()
        idx.append(int((d == d.min()).nonzero()[0]))
    for k in range(1, S):
        idx[k] = max(idx[k], idx[k - 1] + 1)
    idx[S - 1] = min(idx[S - 1], hi)
    for k in range(S - 2, -1, -1):
        idx[k] = min(idx[k], idx[k + 1] - 1)
    return idx


def dpmpp_table(betas, timesteps: Sequence[int], shift: int = 0, final_alpha_bar: float = 1.0) -> torch.Tensor:
    """Coefficients of DPM-Solver++(2M), float64 ``[S, 5]``, row k = ``(s1m, sa, A, B, C)`` for the step from ``tau_k`` to
    ``tau_(k-1)`` (the loop runs k = S-1 down to 0).  With ``a = ab[tau_k + shift]``, ``a' = ab[tau_(k-1) + shift]`` (``a' =
    final_alpha_bar`` at k = 0), ``lam(v) = 0.5 * log(v / (1 - v))`` and ``h = lam(a') - lam(a)``:

        s1m = sqrt(1 - a),  sa = sqrt(a),  A = sqrt(1 - a') / sqrt(1 - a),  g = -sqrt(a') * expm1(-h)
        first order (k = S-1: no history yet; k = 0: the closing step):   B = g,  C = 0
        else, with r = h_(k+1) / h:                                        B = g * (1 + 1 / (2r)),  C = -g / (2r)

    and one step is ``x0 = (x - eps * s1m) / sa ; x' = A * x + B * x0 + C * x0_prev`` (``x0_prev``: the x0 of the step before).  A
    first-order row is the deterministic DDIM update written in x and x0.  Where ``a' = 1`` the row is exactly ``A = 0, B = 1, C = 0``
    (h is infinite and is not formed).  Computed on the CPU; the samplers cast each entry to fp32 once."""
    shift = _int_shift(shift)
    ab = _alphas_bar(betas)
    tau = _checked_timesteps(timesteps, int(ab.numel()) - shift)
    final = torch.tensor(float(final_alpha_bar), dtype=torch.float64)
    if not 0.0 < float(final) <= 1.0:
        raise ValueError(f"final_alpha_bar must lie in (0, 1], got {final_alpha_bar}")

    def lam(v):
        return 0.5 * torch.log(v / (1.0 - v))

    S = len(tau)
    rows, h_prev = [None] * S, None
    zero, one = torch.zeros((), dtype=torch.float64), torch.ones((), dtype=torch.float64)
    for k in range(S - 1, -1, -1):
        a = ab[tau[k] + shift]
        a_next = ab[tau[k - 1] + shift] if k > 0 else final
        if float(a_next) == 1.0:
            A, B, Cc, h = zero, one, zero, None
        else:
            h = lam(a_next) - lam(a)
            A = torch.sqrt(1.0 - a_next) / torch.sqrt(1.0 - a)
            g = -torch.sqrt(a_next) * torch.expm1(-h)
            if k == S - 1 or k == 0:
                B, Cc = g, zero
            else:
                r = h_prev / h
                B, Cc = g * (1.0 + 1.0 / (2.0 * r)), -g / (2.0 * r)
        rows[k] = torch.stack([torch.sqrt(1.0 - a), torch.sqrt(a), A, B, Cc])
        h_prev = h
    return torch.stack(rows)


PREDICTIONS = ("eps", "v")
LOSS_WEIGHTINGS = (None, "min_snr")


def check_prediction(prediction) -> str:
    """``ValueError`` for a ``prediction`` that names none of ``PREDICTIONS``: what the network's output stands for, the noise
    ("eps") or ``v = sqrt(ab) * noise - sqrt(1 - ab) * x_0`` (Salimans & Ho 2022)."""
    if not isinstance(prediction, str) or prediction not in PREDICTIONS:
        raise ValueError(f"prediction must be one of {PREDICTIONS}, got {prediction!r}")
    return prediction


def check_loss_weighting(loss_weighting):
    if loss_weighting is not None and (not isinstance(loss_weighting, str) or loss_weighting not in LOSS_WEIGHTINGS):
        raise ValueError(f"loss_weighting must be one of {LOSS_WEIGHTINGS}, got {loss_weighting!r}")
    return loss_weighting


def check_snr_gamma(gamma) -> float:
    if isinstance(gamma, bool) or not isinstance(gamma, (int, float)) or gamma != gamma or gamma in (float("inf"), -float("inf")) \
            or gamma <= 0:
        raise ValueError(f"snr_gamma must be a finite number > 0, got {gamma!r}")
    return float(gamma)


def min_snr_weights(betas, gamma: float = 5.0, prediction: str = "eps") -> torch.Tensor:
    """Min-SNR-gamma weights of the squared-error term (Hang et al. 2023), float64 ``[T]``: with ``ab = cumprod(1 - betas)`` and
    ``snr = ab / (1 - ab)``, ``w = min(snr, gamma) / snr`` for ``prediction="eps"`` and ``min(snr, gamma) / (snr + 1)`` for ``"v"``
    (the v target's own scale is ``snr + 1`` times the noise's).  ``ValueError`` for a ``gamma`` that is not a finite number > 0 or an
    unknown ``prediction``.  Computed on the CPU; the trainer casts each entry to fp32 once."""
    check_prediction(prediction)
    gamma = check_snr_gamma(gamma)
    ab = _alphas_bar(betas)
    snr = ab / (1.0 - ab)
    capped = torch.clamp(snr, max=float(gamma))
    return capped / snr if prediction == "eps" else capped / (snr + 1.0)


_M64 = (1 << 64) - 1


def _splitmix64(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def posterior_seed(seed: int, image_id: int, replica: int) -> int:
    """The Philox seed of sample ``(image_id, replica)`` of a posterior run under ``seed``, a uint64:
    ``mix(mix(mix(seed) ^ image_id) ^ replica)`` with ``mix`` the splitmix64 step, everything mod 2^64.  All noise of that sample is
    drawn under this one seed -- ``y_T`` is ``hdiff_randn(3HW, s, offset = 2^32 - 1)``, the noise of the step whose device counter reads
    k is ``hdiff_randn(3HW, s, offset = k)`` -- so it belongs to the image, not to a place in a batch.  Pure integer arithmetic."""
    for name, v in (("seed", seed), ("image_id", image_id), ("replica", replica)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"posterior_seed: {name} must be an integer, got {v!r}")
    return _splitmix64(_splitmix64(_splitmix64(int(seed) & _M64) ^ (int(image_id) & _M64)) ^ (int(replica) & _M64))


Y_T_OFFSET = (1 << 32) - 1      # the Philox offset of a posterior sample's y_T; the step noise uses offsets 0 .. n_steps - 1
