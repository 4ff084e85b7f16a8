"""Drop-in for the reference's ``diffusion/Diffusion.py``: ``extract`` (:16-23), ``GaussianDiffusionTrainer`` (:26-180) and
``GaussianDiffusionSampler`` (:182-269) -- the image-conditioned trainer, the ancestral sampler and the deterministic DDIM
sampler -- with the same constructor / ``forward`` signatures, registered float64 buffers and plain attributes.

Sampler underneath: one DynamicUNet evaluation + one fused update kernel per step, the whole step captured into a hipGraph and
replayed (device-resident step counter, time-step and coefficient tables); y_t is updated in place in the plan's buffer.

Kept as written in the reference, on purpose:
  * the model is called as ``model(input, t)``: no label, ``context_zero=True``;
  * with ``unconditional_guidance_scale != 1`` the reference evaluates that same function twice and forms
    ``eps_u + s * (eps - eps_u)`` (:254-257); both evaluations being identical, that is ``eps_u + s * 0 = eps`` exactly,
    so one evaluation is issued here;
  * DDIM lays its time steps over a literal 1000 and reads ``alphas_bar[t + 1]`` (:243-251); ``eta = 0`` makes the
    per-step ``c1 * randn`` term an exact zero (:260-263).

Added to the reference's surface: ``forward(..., tile=, tile_overlap=, tile_batch=)`` samples an image of any size through
overlapping model-sized windows (``tile_origins`` / ``tile_weights`` give the layout): every window is denoised at every step,
the noise estimates are blended where they overlap and ONE DDIM update is applied to the full image
(``csrc/sampler_step.hip``).  Without ``tile`` nothing changes.  ``forward(..., solver="dpmpp2m", spacing=, timesteps=)`` replaces the
first-order DDIM update by DPM-Solver++(2M) on logSNR-uniform time steps (``dpmpp_table`` / ``logsnr_timesteps`` of
``schedules`` with ``shift=1``: this sampler reads ``alphas_bar[t + 1]``) -- still one model evaluation and one update kernel per
step (the same file), untiled and over windows.  Without ``solver`` nothing changes.  ``forward(..., eta=, seed=, image_ids=)`` puts the
reference's ``c1 * randn`` term back with per-image Philox streams, and ``posterior(img, K, ...)`` draws K samples per image in one
plan and returns their mean and per-pixel spread (the same file: ``hdiff_ddim_eta_step``, ``hdiff_randn_rows``,
``hdiff_sample_stats``).  Without those arguments nothing changes.

Trainer underneath: q_sample and the 3 + 3 channel concat are HIP launches, the DynamicUNet runs its autograd path
(``autograd.dyn_unet_forward_with_grad``) and the loss tail -- the squared error, ``y_0_pred`` and the angular-colour term,
and their joint backward -- is one fused kernel pair (``csrc/train_b_ops.hip``).  The reference's two further terms are passed in as
callables (``dino_loss=``, ``msssim_loss=``); a term without one is returned as zero and left out of ``loss``.  Both have a native
form: ``dino_loss="native"`` builds ``Loss.loss.PerceptualLoss_dino`` (a frozen DINOv2 ViT on ``csrc/dino.hip`` and the package's
dense-layer and attention kernels; ``dino_weights=`` is the hub checkpoint's state dict, nothing is fetched), and
``Loss.loss.MSSSIMLoss()`` (``csrc/msssim.hip``) is what to pass as ``msssim_loss=``; nothing here imports torch.hub or kornia.

What the network predicts (an addition to the reference's surface): ``prediction="v"`` on the trainer makes the model's output
``v = sqrt(ab) * noise - sqrt(1 - ab) * x_0`` (Salimans & Ho 2022) -- the tail forms that target, ``y_0_pred = (sqrt(ab) * y_t -
sqrt(1 - ab) * v) / y0_divisor`` and its chain into the output in the same kernel pair -- and ``loss_weighting="min_snr"`` weights the
squared error by ``schedules.min_snr_weights`` (Hang et al. 2023).  The sampler takes the same ``prediction="v"``: one
``hdiff_v_to_eps`` launch behind the UNet turns the output into the noise estimate every update kernel takes, so all loops and
solvers serve both kinds of checkpoint.  Without those arguments nothing changes.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

import warnings

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _capi
from .. import engine as E
from ..engine import gpu_input as _gpu_input, index_vector as _timesteps
from ..schedules import (Y_T_OFFSET, _checked_timesteps, check_loss_weighting, check_prediction, check_snr_gamma, check_solver_spacing,
                         dpmpp_table, logsnr_timesteps, min_snr_weights, posterior_seed, spacing_of)

__all__ = ["extract", "GaussianDiffusionTrainer", "GaussianDiffusionSampler", "tile_origins", "tile_weights", "logsnr_timesteps",
           "dpmpp_table", "posterior_seed", "PosteriorSamples", "min_snr_weights"]


def extract(v, t, x_shape):
    """Coefficients at the given timesteps, cast to fp32 AFTER the gather, shaped [B,1,1,...] (reference :16-23)."""
    device = t.device
    out = torch.gather(v, index=t, dim=0).float().to(device)
    return out.view([t.shape[0]] + [1] * (len(x_shape) - 1))


def _checked_extra_losses(extra_losses):
    """-> a tuple of ``(name, weight, callable)``; ``ValueError`` / ``TypeError`` for anything else.  Looks at no device."""
    if extra_losses is None:
        return ()
    if isinstance(extra_losses, (str, bytes, dict)) or not hasattr(extra_losses, "__iter__"):
        raise TypeError("extra_losses must be a sequence of (name, weight, callable)")
    out, names = [], set()
    for entry in extra_losses:
        if not isinstance(entry, (tuple, list)) or len(entry) != 3:
            raise ValueError(f"extra_losses: every entry is (name, weight, callable), got {entry!r}")
        name, weight, fn = entry
        if not isinstance(name, str) or not name:
            raise ValueError(f"extra_losses: a term's name must be a non-empty string, got {name!r}")
        if name in names:
            raise ValueError(f"extra_losses: the name {name!r} appears twice")
        if isinstance(weight, bool) or not isinstance(weight, (int, float)) or weight != weight or weight in (float("inf"), -float("inf")):
            raise ValueError(f"extra_losses: the weight of {name!r} must be a finite number, got {weight!r}")
        if not callable(fn):
            raise TypeError(f"extra_losses: the term {name!r} is not callable")
        names.add(name)
        out.append((name, float(weight), fn))
    return tuple(out)


class GaussianDiffusionTrainer(nn.Module):
    """forward(gt_images, input_image, stage) -> [loss, mse_loss, perceptual_dino, msssim, col_loss] (reference :26-180).

    ``extra_losses``: a sequence of ``(name, weight, callable)``; each ``callable(y_0_pred, gt_images) * weight`` is added to ``loss``
    (an elementwise map broadcasts into it as it would in the reference's commented-out recipes, :111-136).  The returned list stays
    the reference's five entries; the detached weighted values of the last call are in ``trainer.extra_terms``, a dict by name.
    ``Loss.loss.PerceptualLoss_vgg`` and ``CharbonnierLoss`` are the package's own terms for it.  ``None`` or empty runs what ran
    before, bit for bit.

    ``perceptual_vgg`` / ``perceptual_dino`` are the reference's model names; they are recorded but never loaded (no
    ``torch.hub``, no kornia).  ``dino_loss`` / ``msssim_loss`` are callables ``(y_0_pred, gt) -> scalar tensor`` for those two
    terms; their gradient reaches the model through ``y_0_pred``.  ``msssim_loss=Loss.loss.MSSSIMLoss()`` is the package's own
    MS-SSIM + L1 loss on the HIP path; any other callable runs under torch autograd.  ``dino_loss="native"`` builds
    ``Loss.loss.PerceptualLoss_dino(perceptual_dino, weights=dino_weights)``, the package's own DINOv2 term (``dino_weights``: the hub
    checkpoint's state dict or its path; without it the trunk is random and warns; ``dino_dense="tokens"`` runs its dense layers on
    ``csrc/dense_tokens.hip``, default ``"conv"``).  The trunk is frozen and belongs to the trainer,
    not to ``model``: it is in no checkpoint, no EMA and no optimizer.

    Further keywords (not in the reference; each at its default runs what ran before, bit for bit):
      * ``prediction``: "eps" (the model's output is the noise) or "v" (it is ``a * noise - s * x_0`` with ``a = sqrt_alphas_bar[t]``,
        ``s = sqrt_one_minus_alphas_bar[t]``).  With "v" the squared error is taken against that target, ``y_0_pred = (a * y_t - s *
        out) / y0_divisor`` and its chain into the output is ``-s / y0_divisor``: bounded by 1 at every t, where the eps form's
        ``s / a`` reaches 157 at t = 999.  A checkpoint trained with "v" must be sampled with ``GaussianDiffusionSampler(...,
        prediction="v")``.
      * ``loss_weighting``: None, or "min_snr": ``mse_loss`` (the returned map and its share of ``loss``) is multiplied per sample by
        ``min_snr_weights(betas, snr_gamma, prediction)[t]``; the terms taken on ``y_0_pred`` are not weighted.  ``snr_gamma``
        (default 5.0): a finite number > 0.
      * ``y0_divisor`` (default 255.0, the reference's trailing ``/ 255.0``, :106-107): a finite number other than 0."""

    DINO_WEIGHT, MSSSIM_WEIGHT, COL_WEIGHT = 0.5, 0.0045, 1.0          # reference :165

    def __init__(self, model, beta_1, beta_T, T, perceptual_vgg: str = "vgg16", perceptual_dino: str = "dinov2_vits14", *,
                 dino_loss=None, msssim_loss=None, **more):
        super().__init__()
        # extra_losses arrives through **more: the NAMED keyword-only arguments stay the two callables of the reference's own terms
        # (tests/test_train_b_cpu.py holds the signature to that)
        extra_losses = more.pop("extra_losses", None)
        dino_weights = more.pop("dino_weights", None)
        dino_dense = more.pop("dino_dense", None)
        self.prediction = check_prediction(more.pop("prediction", "eps"))
        self.loss_weighting = check_loss_weighting(more.pop("loss_weighting", None))
        self.snr_gamma = check_snr_gamma(more.pop("snr_gamma", 5.0))
        self.y0_divisor = more.pop("y0_divisor", 255.0)
        if more:
            raise TypeError(f"GaussianDiffusionTrainer.__init__() got an unexpected keyword argument '{next(iter(more))}'")
        if isinstance(self.y0_divisor, bool) or not isinstance(self.y0_divisor, (int, float)) or self.y0_divisor != self.y0_divisor \
                or self.y0_divisor in (0, float("inf"), -float("inf")):
            raise ValueError(f"GaussianDiffusionTrainer: y0_divisor must be a finite number other than 0, got {self.y0_divisor!r}")
        self.extra_losses = _checked_extra_losses(extra_losses)
        self.extra_terms = {}
        held = [fn for _, _, fn in self.extra_losses if isinstance(fn, nn.Module)]
        if held:      # terms that are modules travel with the trainer's .to(device), as dino_loss / msssim_loss do by being attributes
            self.extra_loss_modules = nn.ModuleList(held)
        self.model = model
        self.T = T
        self.register_buffer('betas', torch.linspace(beta_1, beta_T, T).double())
        alphas_bar = torch.cumprod(1. - self.betas, dim=0)
        self.register_buffer('sqrt_alphas_bar', torch.sqrt(alphas_bar))
        self.register_buffer('sqrt_one_minus_alphas_bar', torch.sqrt(1. - alphas_bar))
        # min-SNR-gamma weights of the squared error: float64 -> fp32 once, here; travels with .to(device) but is in no state_dict (the
        # reference's trainer has no such buffer).  None: the tail multiplies by nothing
        self.register_buffer('mse_weights', None if self.loss_weighting is None else
                             min_snr_weights(self.betas, self.snr_gamma, self.prediction).float(), persistent=False)
        self.num = 0
        self.stage = 0
        self.perceptual_vgg, self.perceptual_dino = perceptual_vgg, perceptual_dino
        if isinstance(dino_loss, str):
            if dino_loss != "native":
                raise ValueError(f"GaussianDiffusionTrainer: dino_loss is a callable, None or 'native', got {dino_loss!r}")
            from ..Loss.loss import PerceptualLoss_dino
            dino_loss = PerceptualLoss_dino(perceptual_dino, weights=dino_weights, dense=dino_dense)
        elif dino_weights is not None:
            raise ValueError("GaussianDiffusionTrainer: dino_weights goes with dino_loss='native'")
        elif dino_dense is not None:
            raise ValueError("GaussianDiffusionTrainer: dino_dense goes with dino_loss='native'")
        self.loss_perceptual_dino = dino_loss
        self.ms_ssim_loss = msssim_loss
        self._warned_missing = False

    def _warn_missing(self):
        missing = [f"{name} (weight {w})" for name, fn, w in
                   (("the DINOv2 perceptual loss '" + str(self.perceptual_dino) + "'", self.loss_perceptual_dino, self.DINO_WEIGHT),
                    ("the MS-SSIM loss", self.ms_ssim_loss, self.MSSSIM_WEIGHT)) if fn is None]
        if missing and not self._warned_missing:
            self._warned_missing = True
            warnings.warn("GaussianDiffusionTrainer: no callable for " + " and ".join(missing) + "; the reference adds it to "
                          "the loss, here it is returned as zero and left out (pass dino_loss= / msssim_loss=)",
                          RuntimeWarning, stacklevel=3)

    def forward(self, gt_images, input_image, stage, *, t=None, noise=None, context_zero=None):
        """Images in [0, 255] (uint8 or float).  ``t`` / ``noise`` / ``context_zero`` inject the random draws (parity tests); by
        default they are drawn where the reference draws them: ``torch.randint`` and ``torch.randn_like`` on the device, then
        the host ``torch.rand(1) < 0.02`` (reference :50-67).  As there, a drawn False calls ``model(input, t, gt_images)``,
        whose default is ``context_zero=True``; an injected value is passed to the model as given."""
        self.stage = stage
        self._warn_missing()
        if not (gt_images.is_cuda and input_image.is_cuda):
            E.require_gpu_tensor(gt_images if not gt_images.is_cuda else input_image, "images")
        input_image = (input_image.float() / 255.0) * 2 - 1                                       # :46-47
        gt_images = (gt_images.float() / 255.0) * 2 - 1
        input_image = _gpu_input(input_image, "input_image")
        gt_images = _gpu_input(gt_images, "gt_images")
        if tuple(input_image.shape) != tuple(gt_images.shape) or int(gt_images.shape[1]) != 3:
            raise RuntimeError(f"GaussianDiffusionTrainer: expected two [B, 3, H, W] images, got {tuple(gt_images.shape)} and "
                               f"{tuple(input_image.shape)}")
        dev = gt_images.device
        B, _, H, W = (int(v) for v in gt_images.shape)
        if t is None:
            t = torch.randint(self.T, size=(B,), device=dev)                                       # :51
        else:
            t = _timesteps(t, self.T, dev)
        if noise is None:
            noise = torch.randn_like(gt_images, dtype=torch.float32)                               # :52
        noise = _gpu_input(noise, "noise")
        if tuple(noise.shape) != tuple(gt_images.shape):
            raise RuntimeError(f"GaussianDiffusionTrainer: noise has shape {tuple(noise.shape)}, expected {tuple(gt_images.shape)}")
        lib = _capi.lib()
        sa = self.sqrt_alphas_bar.float().to(dev).contiguous()            # extract(): the fp32 cast of the float64 schedule
        s1m = self.sqrt_one_minus_alphas_bar.float().to(dev).contiguous()
        with torch.cuda.device(dev):
            s = torch.cuda.current_stream(dev).cuda_stream
            y_t = torch.empty_like(gt_images)
            _capi.check(lib.hdiff_q_sample(gt_images.data_ptr(), noise.data_ptr(), t.data_ptr(), sa.data_ptr(), s1m.data_ptr(),
                                           y_t.data_ptr(), B, 3 * H * W, self.T, s), "q_sample")          # :53-55
            x6 = torch.empty(B, 6, H, W, device=dev)
            _capi.check(lib.hdiff_concat2(input_image.data_ptr(), y_t.data_ptr(), x6.data_ptr(), B, 3 * H * W, 3 * H * W, s),
                        "concat2")                                                                         # :57
            if context_zero is None:
                if torch.rand(1) < 0.02:                                                                   # :61-64
                    noise_pred = self.model(x6, t, gt_images, context_zero=True)
                else:
                    noise_pred = self.model(x6, t, gt_images)
            else:
                noise_pred = self.model(x6, t, gt_images, context_zero=bool(context_zero))
            from ..autograd import train_b_loss_tail
            # mse_loss (:102), y_0_pred with the reference's trailing / 255.0 (sic, :106-107: kept), colour term (:172)
            # (with prediction="v" `noise_pred` is the network's v: the tail forms its target and y_0_pred accordingly; with the three
            # arguments at their defaults it launches what it launched before they existed)
            w = None if self.mse_weights is None else self.mse_weights.to(dev)
            mse_loss, y_0_pred, col = train_b_loss_tail(noise_pred, noise, y_t, gt_images, t, sa, s1m, prediction=self.prediction,
                                                        weight_tab=w, y0_div=float(self.y0_divisor))
        zero = torch.zeros((), device=dev)
        loss = mse_loss
        perceptual_dino, msssim = zero, zero
        if self.loss_perceptual_dino is not None:
            perceptual_dino = self.loss_perceptual_dino(y_0_pred, gt_images) * self.DINO_WEIGHT           # :168-169
            loss = loss + perceptual_dino
        if self.ms_ssim_loss is not None:
            msssim = self.ms_ssim_loss(y_0_pred, gt_images) * self.MSSSIM_WEIGHT                          # :171-172
            loss = loss + msssim
        col_loss = col * self.COL_WEIGHT                                                                   # :174-175
        loss = loss + col_loss
        if self.extra_losses:
            terms = {}
            for name, weight, fn in self.extra_losses:
                term = fn(y_0_pred, gt_images) * weight
                loss = loss + term
                terms[name] = term.detach()
            self.extra_terms = terms
        return [loss, mse_loss, perceptual_dino, msssim, col_loss]


def _int_arg(name: str, v, lo: int) -> int:
    if isinstance(v, bool) or not isinstance(v, int):
        raise ValueError(f"{name} must be an integer, got {v!r}")
    if v < lo:
        raise ValueError(f"{name} must be >= {lo}, got {v}")
    return int(v)


def _tile_args(size, tile, overlap):
    size, tile, overlap = _int_arg("size", size, 1), _int_arg("tile", tile, 1), _int_arg("tile_overlap", overlap, 0)
    if overlap > tile // 2:
        raise ValueError(f"tile_overlap must be in [0, tile // 2] = [0, {tile // 2}], got {overlap}")
    return size, tile, overlap


def tile_origins(size: int, tile: int, overlap: int) -> List[int]:
    """Origins of the windows of length ``min(tile, size)`` along an axis of ``size`` positions: ``[0]`` if one window covers
    the axis, else ``0, s, 2s, ...`` with ``s = tile - overlap`` while the window ends before the axis does, then a last window
    flush with the end, at ``size - tile``.  Strictly increasing; at most 3 windows cover a position."""
    size, tile, overlap = _tile_args(size, tile, overlap)
    if size <= tile:
        return [0]
    s, origins, o = tile - overlap, [], 0
    while o + tile < size:
        origins.append(o)
        o += s
    origins.append(size - tile)
    return origins


def tile_weights(size: int, tile: int, overlap: int):
    """-> (first[int32, size], count[int32, size], weight[float64, size, 3]): position p is covered by the consecutive windows
    ``first[p] .. first[p] + count[p] - 1`` of ``tile_origins`` with the weights ``weight[p, :count[p]]`` (the rest is 0), which
    sum to 1.  The profile over a window of length t is ``w(i) = min(i + 1, t - i, max(overlap, 1))`` -- a linear cross-fade
    across a regular overlap -- normalised over the covering windows in float64 (the sampler casts it to fp32 once)."""
    origins = tile_origins(size, tile, overlap)
    size, tile, overlap = _tile_args(size, tile, overlap)
    t = min(tile, size)
    cap = max(overlap, 1)
    first = torch.zeros(size, dtype=torch.int32)
    count = torch.zeros(size, dtype=torch.int32)
    weight = torch.zeros(size, 3, dtype=torch.float64)
    lo = 0
    for p in range(size):
        while origins[lo] + t <= p:                      # origins increase: the first covering window only moves forward
            lo += 1
        ws = []
        k = lo
        while k < len(origins) and origins[k] <= p:
            i = p - origins[k]
            ws.append(min(i + 1, t - i, cap))
            k += 1
        if not 1 <= len(ws) <= 3:
            raise AssertionError(f"position {p} of {size} is covered by {len(ws)} windows (tile {tile}, overlap {overlap})")
        w = torch.tensor(ws, dtype=torch.float64)
        first[p], count[p] = lo, len(ws)
        weight[p, :len(ws)] = w / w.sum()
    return first, count, weight


def _uniform_sequence(ddim_step: int) -> List[int]:
    return list(range(0, 1000, int(1000 / ddim_step)))                                     # :243-247 (the 1000 is literal there)


def _dpmpp_tables(sampler: "GaussianDiffusionSampler", seq, device):
    """-> (tab[n, 5] fp32, t_tab[n] int32) of DPM-Solver++(2M) on the increasing time steps ``seq``: ``a = alphas_bar[t + 1]`` and
    the last step lands on ``alphas_bar[0]``, as the DDIM loop's does; float64 -> fp32 once per entry."""
    seq = list(seq)
    tab = dpmpp_table(sampler.betas, seq, shift=1, final_alpha_bar=float(sampler.alphas_bar[0]))
    return tab.float().contiguous().to(device), torch.tensor(seq, dtype=torch.int32, device=device)


def _ddim_tables(sampler: "GaussianDiffusionSampler", ddim_step: Optional[int], device, seq: Optional[List[int]] = None,
                 eta: Optional[float] = None):
    """-> (tab[n, 4] fp32, t_tab[n] int32), indexed by the down-counting step counter k (k = n - 1 first): the same fp32 ops as
    the reference's :250-262, on the reference's time steps or on the increasing list ``seq``.  With ``eta`` (a number, 0 included)
    the reference's ``eta = 0`` is replaced by it and the rows are ``[n, 5]`` = {sqrt(1 - at), sqrt(at), sqrt(at_next), c1, c2}, the
    rows of ``hdiff_ddim_eta_step``; ``eta=0`` gives the four columns of the call without it bit for bit, and c1 = 0."""
    seq = _uniform_sequence(ddim_step) if seq is None else list(seq)
    seq_next = [-1] + seq[:-1]
    ab = sampler.alphas_bar
    if seq[-1] + 1 >= ab.shape[0]:
        raise RuntimeError(f"index {seq[-1] + 1} is out of bounds for dimension 0 with size {ab.shape[0]}")
    ab = ab.to(device)
    at = ab[torch.tensor(seq, device=device) + 1].float()
    at_next = ab[torch.tensor(seq_next, device=device) + 1].float()
    c1 = (0 if eta is None else eta) * ((1 - at / at_next) * (1 - at_next) / (1 - at)).sqrt()
    c2 = ((1 - at_next) - c1 ** 2).sqrt()
    cols = [(1 - at).sqrt(), at.sqrt(), at_next.sqrt(), c2]
    if eta is not None:
        if not bool(torch.isfinite(c2).all()):
            raise ValueError(f"eta = {eta} is too large for these time steps: (1 - at_next) - c1^2 is negative at some step")
        cols.insert(3, c1)
    tab = torch.stack(cols, dim=1).contiguous()
    return tab, torch.tensor(seq, dtype=torch.int32, device=device)


def _loop_tables(sampler: "GaussianDiffusionSampler", B: int, H: int, W: int, device, ddim_step: Optional[int], seq, solver: str,
                 eta: Optional[float] = None):
    """-> (tab, t_tab, x0_prev) of the DDIM loop on the increasing time steps ``seq`` (None: the reference's, from ``ddim_step``).
    ``x0_prev`` is the full-size history solver="dpmpp2m" reads (from the second step on) and writes, else None."""
    if solver == "dpmpp2m":
        tab, t_tab = _dpmpp_tables(sampler, _uniform_sequence(ddim_step) if seq is None else seq, device)
        return tab, t_tab, torch.empty(B, 3, H, W, device=device)
    return _ddim_tables(sampler, ddim_step, device, seq, eta) + (None,)


def _checked_eta(eta) -> float:
    if isinstance(eta, bool) or not isinstance(eta, (int, float)) or eta != eta or eta in (float("inf"), -float("inf")) or eta < 0:
        raise ValueError(f"eta must be a finite number >= 0, got {eta!r}")
    return float(eta)


def _row_seeds(seed: int, image_ids, B: int, replicas: int = 1) -> List[int]:
    """The Philox seeds of a batch of ``B`` images x ``replicas`` samples, image-major, as the int64 bit patterns a torch tensor
    holds.  An entry of ``image_ids`` is an integer (replica r of it is ``posterior_seed(seed, id, r)``) or, for one row of a batch laid
    out by hand, an ``(image, replica)`` pair."""
    ids = list(range(B)) if image_ids is None else list(image_ids)
    if len(ids) != B:
        raise ValueError(f"image_ids names {len(ids)} images, the batch holds {B}")
    out = []
    for entry in ids:
        pair = isinstance(entry, (tuple, list))
        if pair and (len(entry) != 2 or replicas != 1):
            raise ValueError(f"image_ids: an entry is an integer or an (image, replica) pair of a single-sample call, got {entry!r}")
        for r in range(replicas):
            s = posterior_seed(seed, entry[0] if pair else entry, entry[1] if pair else r)
            out.append(s - (1 << 64) if s >= (1 << 63) else s)
    return out


class PosteriorSamples:
    """What ``GaussianDiffusionSampler.posterior`` returns: ``mean`` and ``std`` ``[B, 3, H, W]`` over the K clipped samples of every
    image (``hdiff_sample_stats``), and ``samples`` ``[B, K, 3, H, W]`` or None."""

    __slots__ = ("mean", "std", "samples")

    def __init__(self, mean: torch.Tensor, std: torch.Tensor, samples: Optional[torch.Tensor]):
        self.mean, self.std, self.samples = mean, std, samples


def _emit_v_to_eps(holder, p, sampler: "GaussianDiffusionSampler", up, rows: int, n_per: int, device) -> None:
    """With ``sampler.prediction == "v"``: one ``hdiff_v_to_eps`` on the UNet plan's output, reading the state the model saw
    (``up.y``) and the time vector it was called with (``up.t``), so that whatever follows takes a noise estimate.  The tables are
    the TRAINER's -- ``sqrt(alphas_bar)[t]`` and ``sqrt(1 - alphas_bar)[t]``, float64 -> fp32 once -- not the DDIM loop's
    ``alphas_bar[t + 1]``: the model was trained against the former.  ``holder`` (the step plan) keeps them alive.  With "eps"
    nothing is emitted."""
    if sampler.prediction != "v":
        return
    if not hasattr(holder, "v_sa"):
        holder.v_sa = torch.sqrt(sampler.alphas_bar).float().to(device).contiguous()
        holder.v_s1m = torch.sqrt(1. - sampler.alphas_bar).float().to(device).contiguous()
    p.call("hdiff_v_to_eps", up.out.data_ptr(), up.y.data_ptr(), up.t.data_ptr(), holder.v_sa.data_ptr(), holder.v_s1m.data_ptr(),
           int(sampler.T), rows, n_per)


class _StepPlan:
    """One captured sampling step for a fixed (B, H, W) and mode: fill t -> DynamicUNet [-> v to eps] -> update -> advance the
    counter."""

    def __init__(self, sampler: "GaussianDiffusionSampler", B: int, H: int, W: int, device, ddim_step: Optional[int],
                 inject_noise: bool = False, seed: int = 0, solver: str = "ddim", seq: Optional[List[int]] = None,
                 eta: Optional[float] = None):
        """``seq``: the increasing time steps of the DDIM / DPM-Solver++(2M) loop (None: the reference's, from ``ddim_step``).
        ``eta``: the DDIM loop with its stochastic term (``hdiff_ddim_eta_step``): row b draws under ``self.seeds[b]``, which the
        caller fills before a run, or reads ``self.noise`` with ``inject_noise``."""
        self.unet = sampler.model.plan_for(B, H, W, device, True)
        up = self.unet
        if up.out_hw != (H, W):
            raise RuntimeError(f"The size of tensor a ({W}) must match the size of tensor b ({up.out_hw[1]}) at non-singleton "
                               "dimension 3")
        n = B * 3 * H * W
        self.B, self.n = B, n
        self.n_slots, self.th, self.tw = B, H, W          # what the UNet plan was made for (the names of _TiledStepPlan)
        self.step = torch.zeros(1, dtype=torch.int32, device=device)
        self.nan_flag = torch.zeros(1, dtype=torch.int32, device=device)
        self.noise = torch.empty(B, 3, H, W, device=device)
        p = E.Plan(device)
        if ddim_step is None and seq is None:
            # ancestral (:224-236): t = the step counter itself; the first tree's fused update with w = 0 (eps_u := eps)
            var = torch.cat([sampler.posterior_var[1:2], sampler.betas[1:]])                      # :210
            self.c1 = sampler.coeff1.float().contiguous()
            self.c2 = sampler.coeff2.float().contiguous()
            self.sigma = torch.sqrt(var.float()).contiguous()
            self.n_steps = sampler.T
            p.call("hdiff_fill_t", up.t.data_ptr(), self.step.data_ptr(), B)
            p.ops.extend(up.plan.ops)
            _emit_v_to_eps(self, p, sampler, up, B, 3 * H * W, device)
            # noise: injected buffer (parity runs) or drawn in-kernel (Philox, counter = (seed, step, element))
            p.call("hdiff_ddpm_step", up.y.data_ptr(), up.out.data_ptr(), up.out.data_ptr(),
                   self.noise.data_ptr() if inject_noise else None, up.y.data_ptr(), self.c1.data_ptr(), self.c2.data_ptr(),
                   self.sigma.data_ptr(), self.step.data_ptr(), int(sampler.T), C.c_double(0.0), C.c_uint64(seed),
                   self.nan_flag.data_ptr(), n)
        else:
            self.tab, self.t_tab, self.x0_prev = _loop_tables(sampler, B, H, W, device, ddim_step, seq, solver, eta)
            self.n_steps = int(self.t_tab.numel())
            p.call("hdiff_fill_from_table", up.t.data_ptr(), self.t_tab.data_ptr(), self.step.data_ptr(), self.n_steps, B)
            p.ops.extend(up.plan.ops)
            _emit_v_to_eps(self, p, sampler, up, B, 3 * H * W, device)
            if solver == "dpmpp2m":         # the same step with the second-order update; the plan owns the x0 history
                p.call("hdiff_dpmpp_step", up.y.data_ptr(), up.out.data_ptr(), up.y.data_ptr(), self.x0_prev.data_ptr(),
                       self.tab.data_ptr(), self.step.data_ptr(), self.n_steps, 0, self.nan_flag.data_ptr(), n)
            elif eta is not None:           # the same step with c1 * z kept: one Philox stream per row, or the injected draws
                self.seeds = torch.zeros(B, dtype=torch.int64, device=device)
                p.call("hdiff_ddim_eta_step", up.y.data_ptr(), up.out.data_ptr(), self.noise.data_ptr() if inject_noise else None,
                       up.y.data_ptr(), self.tab.data_ptr(), self.seeds.data_ptr(), 3 * H * W, self.step.data_ptr(), self.n_steps,
                       self.nan_flag.data_ptr(), B)
            else:
                p.call("hdiff_ddim_step", up.y.data_ptr(), up.out.data_ptr(), up.y.data_ptr(), self.tab.data_ptr(),
                       self.step.data_ptr(), self.n_steps, self.nan_flag.data_ptr(), n)
        p.call("hdiff_step_decrement", self.step.data_ptr())
        self.plan = p


class _TiledStepPlan:
    """One captured DDIM step over overlapping windows for a fixed (B, H, W, tile, overlap, tile_batch): fill t -> per chunk of
    windows [gather cond, gather y, DynamicUNet, store eps] -> blend + update on the full image -> advance the counter.

    Every chunk runs the SAME window plan at batch ``n_slots``; a short final chunk is padded with repeats of the last window,
    whose estimates are not stored.  With a single chunk the blend reads the plan's output directly."""

    def __init__(self, sampler: "GaussianDiffusionSampler", B: int, H: int, W: int, device, ddim_step: Optional[int], tile: int,
                 overlap: int, tile_batch: Optional[int], solver: str = "ddim", seq: Optional[List[int]] = None):
        th, tw = min(tile, H), min(tile, W)
        oy, ox = tile_origins(H, tile, overlap), tile_origins(W, tile, overlap)
        ny, nx = len(oy), len(ox)
        n_windows = B * ny * nx
        n_slots = n_windows if tile_batch is None else min(tile_batch, n_windows)
        self.unet = sampler.model.plan_for(n_slots, th, tw, device, True)
        up = self.unet
        if up.out_hw != (th, tw):
            raise RuntimeError(f"The size of tensor a ({tw}) must match the size of tensor b ({up.out_hw[1]}) at non-singleton "
                               "dimension 3")
        self.B, self.n = B, B * 3 * H * W
        self.ny, self.nx, self.th, self.tw, self.n_windows, self.n_slots = ny, nx, th, tw, n_windows, n_slots
        self.chunks = [(w0, min(n_slots, n_windows - w0)) for w0 in range(0, n_windows, n_slots)]
        self.step = torch.zeros(1, dtype=torch.int32, device=device)
        self.nan_flag = torch.zeros(1, dtype=torch.int32, device=device)
        self.y = torch.empty(B, 3, H, W, device=device)
        self.cond = torch.empty(B, 3, H, W, device=device)
        self.eps = up.out if len(self.chunks) == 1 else torch.empty(n_windows, 3, th, tw, device=device)
        i32 = dict(dtype=torch.int32, device=device)
        self.oy, self.ox, self.zero = torch.tensor(oy, **i32), torch.tensor(ox, **i32), torch.zeros(1, **i32)
        fy, cy, wy = tile_weights(H, tile, overlap)
        fx, cx, wx = tile_weights(W, tile, overlap)
        self.fy, self.cy, self.wy = fy.to(device), cy.to(device), wy.float().to(device).contiguous()    # fp32 cast: once, here
        self.fx, self.cx, self.wx = fx.to(device), cx.to(device), wx.float().to(device).contiguous()
        self.tab, self.t_tab, self.x0_prev = _loop_tables(sampler, B, H, W, device, ddim_step, seq, solver)   # history: full-size, like y
        self.n_steps = int(self.t_tab.numel())
        p = E.Plan(device)
        p.call("hdiff_fill_from_table", up.t.data_ptr(), self.t_tab.data_ptr(), self.step.data_ptr(), self.n_steps, n_slots)
        for w0, valid in self.chunks:
            for src, dst in ((self.cond, up.cond), (self.y, up.y)):
                p.call("hdiff_tile_gather", src.data_ptr(), dst.data_ptr(), self.oy.data_ptr(), self.ox.data_ptr(), B, 3, H, W,
                       ny, nx, th, tw, w0, n_slots)
            p.ops.extend(up.plan.ops)
            _emit_v_to_eps(self, p, sampler, up, n_slots, 3 * th * tw, device)       # per chunk, on the gathered windows of y
            if self.eps is not up.out:
                # the plan's output is reused by the next chunk: keep this chunk's estimates (a gather whose windows are whole
                # samples is a copy; the padding slots are left behind)
                p.call("hdiff_tile_gather", up.out.data_ptr(), self.eps[w0].data_ptr(), self.zero.data_ptr(),
                       self.zero.data_ptr(), n_slots, 3, th, tw, 1, 1, th, tw, 0, valid)
        if solver == "dpmpp2m":
            p.call("hdiff_tile_dpmpp_step", self.y.data_ptr(), self.eps.data_ptr(), self.x0_prev.data_ptr(), self.fy.data_ptr(),
                   self.cy.data_ptr(), self.wy.data_ptr(), self.oy.data_ptr(), self.fx.data_ptr(), self.cx.data_ptr(),
                   self.wx.data_ptr(), self.ox.data_ptr(), self.tab.data_ptr(), self.step.data_ptr(), self.n_steps, 0,
                   self.nan_flag.data_ptr(), B, 3, H, W, ny, nx, th, tw)
        else:
            p.call("hdiff_tile_ddim_step", self.y.data_ptr(), self.eps.data_ptr(), self.fy.data_ptr(), self.cy.data_ptr(),
                   self.wy.data_ptr(), self.oy.data_ptr(), self.fx.data_ptr(), self.cx.data_ptr(), self.wx.data_ptr(),
                   self.ox.data_ptr(), self.tab.data_ptr(), self.step.data_ptr(), self.n_steps, self.nan_flag.data_ptr(), B, 3, H,
                   W, ny, nx, th, tw)
        p.call("hdiff_step_decrement", self.step.data_ptr())
        self.plan = p


class GaussianDiffusionSampler(nn.Module):
    """forward(input_image, ddim=False, unconditional_guidance_scale=1, ddim_step=None) -> enhanced image clipped to [-1, 1]
    (reference diffusion/Diffusion.py:182-269).  ``input_image`` is in [0, 255] (divided by 255 here, as there).
    ``tile=`` (not in the reference) samples an image of any size through overlapping model-sized windows: see ``forward``.
    ``prediction`` (not in the reference): "eps", or "v" for a model trained with ``GaussianDiffusionTrainer(..., prediction="v")`` --
    every step then runs one ``hdiff_v_to_eps`` behind the model (per chunk of windows with ``tile``), in front of whichever update the
    call asks for: the ancestral loop, DDIM, ``solver="dpmpp2m"``, ``eta`` / ``posterior`` and ``tile`` all take it.  Sampling a v
    checkpoint as "eps" (or the reverse) raises nothing and returns noise: ``Evaluate`` reads the ``prediction.json`` the training
    driver writes for that reason."""

    GRAPH_MIN_STEPS = 4

    def __init__(self, model, beta_1, beta_T, T, *, prediction: str = "eps"):
        super().__init__()
        self.model = model
        self.T = T
        self.prediction = check_prediction(prediction)
        self.register_buffer('betas', torch.linspace(beta_1, beta_T, T).double())
        alphas = 1. - self.betas
        alphas_bar = torch.cumprod(alphas, dim=0)
        alphas_bar_prev = F.pad(alphas_bar, [1, 0], value=1)[:T]
        self.sqrt_alphas_bar = alphas_bar                      # sic: the reference stores alphas_bar under this name (:193)
        self.sqrt_one_minus_alphas_bar = torch.sqrt(1. - alphas_bar)
        self.alphas_bar = alphas_bar
        self.one_minus_alphas_bar = (1. - alphas_bar)
        self.register_buffer('coeff1', torch.sqrt(1. / alphas))
        self.register_buffer('coeff2', self.coeff1 * (1. - alphas) / torch.sqrt(1. - alphas_bar))
        self.register_buffer('posterior_var', self.betas * (1. - alphas_bar_prev) / (1. - alphas_bar))
        self._plans = {}

    def predict_xt_prev_mean_from_eps(self, t, eps, y_t):
        assert y_t.shape == eps.shape
        E.require_gpu_tensor(y_t, "y_t")
        E.require_gpu_tensor(eps, "eps")
        lib = _capi.lib()
        out = torch.empty_like(y_t)
        c1, c2 = extract(self.coeff1, t, y_t.shape), extract(self.coeff2, t, y_t.shape)
        s = torch.cuda.current_stream(y_t.device).cuda_stream
        per = y_t.numel() // y_t.shape[0]
        for b in range(y_t.shape[0]):      # tiny helper path (the sampler itself uses the fused per-step kernel)
            _capi.check(lib.hdiff_axpby(C.c_float(float(c1[b])), y_t[b].data_ptr(), C.c_float(-float(c2[b])), eps[b].data_ptr(),
                                        out[b].data_ptr(), per, s), "axpby")
        return out

    def p_mean_variance(self, input, t, y_t):
        var = torch.cat([self.posterior_var[1:2], self.betas[1:]])
        var = extract(var, t, input.shape)
        eps = self.model(input, t)
        if self.prediction == "v":
            eps, y, tt, dev = eps.contiguous(), y_t.contiguous(), t.to(torch.int64).contiguous(), y_t.device
            sa, s1m = torch.sqrt(self.alphas_bar).float().to(dev), torch.sqrt(1. - self.alphas_bar).float().to(dev)
            _capi.check(_capi.lib().hdiff_v_to_eps(eps.data_ptr(), y.data_ptr(), tt.data_ptr(), sa.data_ptr(), s1m.data_ptr(),
                                                   int(self.T), int(y.shape[0]), y.numel() // int(y.shape[0]),
                                                   torch.cuda.current_stream(dev).cuda_stream), "v_to_eps")
        return self.predict_xt_prev_mean_from_eps(t, eps, y_t), var

    def forward(self, input_image, ddim=False, unconditional_guidance_scale=1, ddim_step=None, *, y_T=None,
                noise_by_step: Optional[List[torch.Tensor]] = None, trajectory: Optional[List[torch.Tensor]] = None,
                tile: Optional[int] = None, tile_overlap: Optional[int] = None, tile_batch: Optional[int] = None,
                solver: str = "ddim", spacing: Optional[str] = None, timesteps=None, eta: float = 0.0, seed: Optional[int] = None,
                image_ids=None):
        """``y_T`` / ``noise_by_step`` inject the random draws (parity runs; ``noise_by_step[k]`` is the k-th per-step draw of
        the ancestral loop, in call order); by default they come from torch's generator exactly where the reference draws
        them.  ``trajectory`` collects the pre-clip y_t after every step.  Called with autograd enabled (the reference would
        record a graph through every model evaluation, diffusion/Diffusion.py:217-269) the loop still runs without one and
        returns a detached tensor, with one RuntimeWarning per sampler instance; an input that requires grad is refused.

        Overlapping-window sampling (an addition to the reference's surface; DDIM only):
          * ``tile``: integer >= 1, the side of the square window handed to the model (``min(tile, size)`` on each axis); every
            window is denoised at every step, the noise estimates are averaged where windows overlap (``tile_weights``) and one
            DDIM update is applied to the full image.  ``None``: the whole image goes through the model in one piece, as in the
            reference.  A window size the model cannot take raises the same ``RuntimeError`` as such an image does.
          * ``tile_overlap``: integer in ``[0, tile // 2]``, the overlap of neighbouring windows; default ``tile // 8``.
          * ``tile_batch``: integer >= 1, the most windows per model evaluation (bounds memory); ``None`` evaluates all
            ``B * n_windows`` at once.
        ``y_T`` and ``trajectory`` are full-size ``[B, 3, H, W]``; ``dynamic_forward`` sees the full image.

        The solver of the DDIM loop (additions as well; ``ddim=True`` only, untiled and with ``tile``):
          * ``solver``: "ddim" (the reference's update) or "dpmpp2m", DPM-Solver++(2M) -- second order at the same one model
            evaluation per step (``dpmpp_table(betas, tau, shift=1, final_alpha_bar=alphas_bar[0])``).
          * ``spacing``: the ``ddim_step`` time steps tau -- "uniform", the reference's ``range(0, 1000, int(1000 / ddim_step))``, or
            "logsnr", ``logsnr_timesteps(betas, ddim_step, shift=1)``; ``None`` is uniform for "ddim" and logsnr for "dpmpp2m".
          * ``timesteps``: an explicit strictly increasing list in ``[0, T - 2]`` in place of ``ddim_step`` (and of ``spacing``).
        The model's time input at step k is ``tau_k``, as in the reference's loop.

        The reference's stochastic term and per-image noise (additions; ``ddim=True``, ``solver="ddim"``, untiled):
          * ``eta``: a finite number >= 0 in place of the ``eta = 0`` the reference has written in (:260): every step, the last
            included, adds ``c1 * z`` with ``c1 = eta * sqrt((1 - at / at_next) * (1 - at_next) / (1 - at))`` (``hdiff_ddim_eta_step``).
            ``z`` of row b at the step whose counter reads k is ``hdiff_randn(3HW, s_b, offset = k)``, or ``noise_by_step[j]`` for the
            j-th step in call order.  ``eta=0`` runs what ran before.
          * ``seed`` / ``image_ids``: ``s_b = posterior_seed(seed, image_ids[b], 0)`` (``image_ids`` defaults to ``range(B)``; an entry
            may be an ``(image, replica)`` pair).  With ``seed`` given and no ``y_T``, ``y_T`` of row b is ``hdiff_randn(3HW, s_b,
            offset = 2^32 - 1)``: the call then reads nothing of torch's generator, and a row's result does not depend on the batch
            it is in.  ``seed=None`` with ``eta > 0`` draws one int64 from torch's CPU generator, as the ancestral path does."""
        seq = self._solver_arguments(ddim, ddim_step, solver, spacing, timesteps)
        eta = _checked_eta(eta)
        if eta > 0 and (not ddim or solver != "ddim"):
            raise ValueError("eta > 0 needs ddim=True and solver='ddim': DPM-Solver++(2M) here is the deterministic multistep solver")
        if (eta > 0 or seed is not None or image_ids is not None) and tile is not None:
            raise ValueError("eta / seed / image_ids are not available with tile: the windowed loop is deterministic")
        if (seed is not None or image_ids is not None) and not ddim:
            raise ValueError("seed / image_ids need ddim=True")
        if image_ids is not None and seed is None and eta == 0:
            raise ValueError("image_ids was given without seed")
        if tile is None:
            if tile_overlap is not None or tile_batch is not None:
                raise ValueError("tile_overlap / tile_batch were given without tile")
        else:
            tile = _int_arg("tile", tile, 1)
            if not ddim:
                raise ValueError("tile needs ddim=True: the ancestral loop is not run over windows")
            tile_overlap = tile // 8 if tile_overlap is None else _int_arg("tile_overlap", tile_overlap, 0)
            if tile_overlap > tile // 2:
                raise ValueError(f"tile_overlap must be in [0, tile // 2] = [0, {tile // 2}], got {tile_overlap}")
            if tile_batch is not None:
                tile_batch = _int_arg("tile_batch", tile_batch, 1)
        if torch.is_grad_enabled():
            if input_image.requires_grad or (y_T is not None and torch.is_tensor(y_T) and y_T.requires_grad):
                raise RuntimeError("GaussianDiffusionSampler.forward: an input requires grad, but the sampling loop runs under "
                                   "torch.no_grad() and cannot be differentiated; detach it or call under torch.no_grad()")
            if any(p.requires_grad for p in self.model.parameters()) and not getattr(self, "_warned_grad", False):
                self._warned_grad = True
                warnings.warn("GaussianDiffusionSampler.forward was called with autograd enabled: the sampling loop runs under "
                              "torch.no_grad() and returns a tensor without grad_fn", RuntimeWarning, stacklevel=2)
        with torch.no_grad():
            if tile is not None:
                return self._forward_tiled(input_image, ddim_step, y_T, trajectory, tile, tile_overlap, tile_batch, solver, spacing,
                                           seq)
            return self._forward(input_image, ddim, unconditional_guidance_scale, ddim_step, y_T, noise_by_step, trajectory, solver,
                                 spacing, seq, eta, seed, image_ids)

    def _solver_arguments(self, ddim, ddim_step, solver, spacing, timesteps):
        """-> the time steps of the loop as a tuple, or None for the reference's own (``ValueError`` otherwise).  Looks at no
        device.  Plain ``ddim=True, ddim_step=n`` gives None: that call runs exactly what it ran before these arguments existed."""
        check_solver_spacing(solver, spacing)
        if not ddim:
            if solver != "ddim" or spacing is not None or timesteps is not None:
                raise ValueError("solver / spacing / timesteps need ddim=True: they choose the update and the steps of the DDIM loop")
            return None
        if timesteps is not None:
            if ddim_step is not None or spacing is not None:
                raise ValueError("an explicit timesteps list replaces ddim_step and spacing: give one or the other")
            return _checked_timesteps(timesteps, int(self.T) - 1)
        if spacing_of(solver, spacing) == "uniform":
            if ddim_step is None and solver != "ddim":
                raise ValueError("solver='dpmpp2m' needs ddim_step or timesteps")
            return None                                       # (ddim_step=None: the reference's TypeError, raised where it was)
        if ddim_step is None:
            raise ValueError("spacing='logsnr' needs ddim_step")
        return tuple(logsnr_timesteps(self.betas, ddim_step, shift=1))

    def _input(self, input_image, ddim, ddim_step, seq):
        """-> (the image in [0, 1] as the kernels need it, ``ddim_step`` as a plan key holds it: an int for the reference's own
        time steps of the DDIM loop, else None)."""
        img = _gpu_input(input_image, "input_image").float() / 255.0                               # :220
        B, Cx, H, W = (int(v) for v in img.shape)
        if Cx != 3:
            raise RuntimeError(f"expected input[{B}, {Cx + 3}, {H}, {W}] to have 6 channels")
        if ddim and ddim_step is None and seq is None:
            raise TypeError("unsupported operand type(s) for /: 'int' and 'NoneType'")             # :243 with ddim_step=None
        return img, (int(ddim_step) if ddim and seq is None else None)

    def _plan(self, key, device, make):
        """The one live step plan: a graph bakes its seed and contraction mode, and a rebuilt UNet plan retires it.  What the model
        predicts decides the launch list, so it is part of the key (for "eps" the key is the one it was)."""
        if self.prediction != "eps":
            key = key + (("prediction", self.prediction),)
        sp = self._plans.get(key)
        if sp is None or sp.unet is not self.model.plan_for(sp.n_slots, sp.th, sp.tw, device, True):
            sp = make()
            self._plans = {key: sp}
        sp.unet.plan.pack_weights()     # once per call: also catches writes through p.data, which p._version does not see
        return sp

    def _run(self, sp, y_buffer, n_steps, eager, noise_by_step, trajectory, noise_steps=None, out=None, n=None):
        """``n_steps`` runs (eager) or replays of the captured step on the state in ``y_buffer``, then the clip.
        ``noise_by_step[k]`` goes into the plan's noise buffer before step k (the last step adds none; ``noise_steps=n_steps``: every
        step does, the loop with ``eta``).  ``out`` / ``n``: clip the first ``n`` floats into ``out`` in place of a new tensor."""
        noise_steps = n_steps - 1 if noise_steps is None else noise_steps
        sp.step.fill_(n_steps - 1)
        sp.nan_flag.zero_()
        stream = torch.cuda.current_stream(y_buffer.device).cuda_stream
        if not eager:
            sp.plan.capture()
        for k in range(n_steps):
            if noise_by_step is not None and k < noise_steps:
                sp.noise.copy_(noise_by_step[k])
            if eager:
                sp.plan.run(stream)
            else:
                sp.plan.replay(stream)
            if trajectory is not None:
                trajectory.append(y_buffer.clone())
        if out is None:
            out, n = torch.empty_like(y_buffer), sp.n
        _capi.check(_capi.lib().hdiff_clip(y_buffer.data_ptr(), out.data_ptr(), C.c_float(-1.0), C.c_float(1.0), n, stream),
                    "clip")
        return out

    def _forward_tiled(self, input_image, ddim_step, y_T, trajectory, tile, overlap, tile_batch, solver="ddim", spacing=None,
                       seq=None):
        """The DDIM loop over overlapping windows.  ``unconditional_guidance_scale`` needs no handling: as in ``_forward`` its
        two evaluations are the same function, so the combine is eps exactly and one evaluation is issued."""
        img, ddim_step = self._input(input_image, True, ddim_step, seq)
        B, _, H, W = (int(v) for v in img.shape)
        dev = img.device
        mode = _capi.lib().hdiff_get_contraction_mode()
        sp = self._plan((B, H, W, str(dev), ddim_step, False, 0, mode, tile, overlap, tile_batch, solver, spacing, seq), dev,
                        lambda: _TiledStepPlan(self, B, H, W, dev, ddim_step, tile, overlap, tile_batch, solver, seq))
        self.model.dynamic_forward(torch.cat([img, img], dim=1))    # on the full image
        y = torch.randn_like(img) if y_T is None else y_T            # :239
        sp.cond.copy_(img)
        sp.y.copy_(y)
        eager = trajectory is not None or sp.n_steps < self.GRAPH_MIN_STEPS
        return self._run(sp, sp.y, sp.n_steps, eager, None, trajectory)

    def _step_plan(self, B, H, W, dev, ddim_step, inject, seed, solver, spacing, seq, eta):
        """The untiled plan of ``forward`` and ``posterior``.  Without ``eta`` the key and the launch list are those of the call
        before ``eta`` existed; with it the key gains one entry and the seeds live in the plan's device buffer, not in the key."""
        mode = _capi.lib().hdiff_get_contraction_mode()
        key = (B, H, W, str(dev), ddim_step, inject, seed, mode, None, None, None, solver, spacing, seq)   # the three None: tile, ...
        if eta > 0:
            return self._plan(key + (("eta", eta),), dev, lambda: _StepPlan(self, B, H, W, dev, ddim_step, inject, seed, solver, seq, eta))
        return self._plan(key, dev, lambda: _StepPlan(self, B, H, W, dev, ddim_step, inject, seed, solver, seq))

    def _forward(self, input_image, ddim, unconditional_guidance_scale, ddim_step, y_T, noise_by_step, trajectory, solver="ddim",
                 spacing=None, seq=None, eta=0.0, row_seed=None, image_ids=None):
        img, ddim_step = self._input(input_image, ddim, ddim_step, seq)
        B, _, H, W = (int(v) for v in img.shape)
        dev = img.device
        inject = ((not ddim) or eta > 0) and noise_by_step is not None
        seed = 0 if (ddim or inject) else int(torch.empty((), dtype=torch.int64).random_().item())
        seeds, drawn = None, row_seed is None       # per-row Philox seeds; a drawn seed leaves y_T to torch's generator, as before
        if row_seed is not None or (eta > 0 and not inject):
            if drawn:
                row_seed = int(torch.empty((), dtype=torch.int64).random_().item())
            seeds = torch.tensor(_row_seeds(row_seed, image_ids, B), dtype=torch.int64).to(dev)
        sp = self._step_plan(B, H, W, dev, ddim_step, inject, seed, solver, spacing, seq, eta)
        self.model.dynamic_forward(torch.cat([img, img], dim=1))    # the reference runs it on every call (requires_grad only)
        if y_T is None and seeds is not None and not drawn:
            y = torch.empty_like(img)
            _capi.check(_capi.lib().hdiff_randn_rows(y.data_ptr(), B, 3 * H * W, seeds.data_ptr(), C.c_uint64(Y_T_OFFSET),
                                                     torch.cuda.current_stream(dev).cuda_stream), "randn_rows")
        else:
            y = torch.randn_like(img) if y_T is None else y_T        # :226 / :239
        up = sp.unet
        up.cond.copy_(img)
        up.y.copy_(y)
        if eta > 0 and seeds is not None:
            sp.seeds.copy_(seeds)
        eager = inject or trajectory is not None or sp.n_steps < self.GRAPH_MIN_STEPS
        return self._run(sp, up.y, sp.n_steps, eager, noise_by_step if inject else None, trajectory,
                         sp.n_steps if eta > 0 else None)

    def posterior(self, input_image, samples, *, ddim_step=None, timesteps=None, spacing=None, solver="ddim", eta=0.0, seed=0,
                  image_ids=None, sample_batch=None, keep_samples=False) -> PosteriorSamples:
        """``samples`` = K draws of the DDIM loop per image, their mean and their per-pixel spread (an addition to the reference's
        surface).  Sample ``(b, r)`` is what ``forward`` returns for image b under the Philox seed ``posterior_seed(seed,
        image_ids[b], r)``: its ``y_T`` and, with ``eta > 0``, the noise of every step come from that one stream, so a sample depends
        on neither its batch, ``sample_batch`` nor K, and the first K samples of a larger run are the samples of the K run.
        ONE step plan at batch ``min(B * K, sample_batch)`` is looped over chunks of samples (the conditioning image repeated per
        replica, ``y_T`` from ``hdiff_randn_rows``; a short last chunk is padded with repeats of the last sample, whose results are
        dropped); every clipped sample lands in one ``[B, K, 3, H, W]`` buffer and one ``hdiff_sample_stats`` launch follows.
        ``solver="dpmpp2m"`` needs ``eta == 0``: the samples then differ through ``y_T`` alone.  The hipGraph policy is ``forward``'s
        (``GRAPH_MIN_STEPS``); nothing here synchronises.
        -> ``PosteriorSamples``: ``mean`` ``[B, 3, H, W]``, the mean of the clipped samples, in [-1, 1]; ``std``, the same shape,
        their unbiased standard deviation (0 for K = 1); ``samples`` with ``keep_samples``, else None."""
        K = _int_arg("samples", samples, 1)
        eta = _checked_eta(eta)
        if eta > 0 and solver != "ddim":
            raise ValueError("eta > 0 needs solver='ddim': DPM-Solver++(2M) here is the deterministic multistep solver")
        if sample_batch is not None:
            sample_batch = _int_arg("sample_batch", sample_batch, 1)
        _int_arg("seed", seed, -(1 << 63))
        seq = self._solver_arguments(True, ddim_step, solver, spacing, timesteps)
        if torch.is_grad_enabled() and input_image.requires_grad:
            raise RuntimeError("GaussianDiffusionSampler.posterior: the input requires grad, but the sampling loop runs under "
                               "torch.no_grad() and cannot be differentiated; detach it or call under torch.no_grad()")
        with torch.no_grad():
            img, ddim_step = self._input(input_image, True, ddim_step, seq)
            B, _, H, W = (int(v) for v in img.shape)
            dev, per = img.device, 3 * H * W
            R = B * K
            PB = R if sample_batch is None else min(R, sample_batch)
            chunks = [(r0, min(PB, R - r0)) for r0 in range(0, R, PB)]
            rows = _row_seeds(seed, image_ids, B, K)
            # one upload: the R seeds in order, then those of every chunk's slots (a padding slot repeats the last sample, as
            # hdiff_tile_gather does)
            table = torch.tensor(rows + [rows[min(r0 + s, R - 1)] for r0, _ in chunks for s in range(PB)], dtype=torch.int64).to(dev)
            seeds = table[R:]
            sp = self._step_plan(PB, H, W, dev, ddim_step, False, 0, solver, spacing, seq, eta)
            self.model.dynamic_forward(torch.cat([img, img], dim=1))
            lib, up = _capi.lib(), sp.unet
            stream = torch.cuda.current_stream(dev).cuda_stream
            cond = img.repeat_interleave(K, dim=0).contiguous()
            y_T = torch.empty(R, 3, H, W, device=dev)
            _capi.check(lib.hdiff_randn_rows(y_T.data_ptr(), R, per, table.data_ptr(), C.c_uint64(Y_T_OFFSET), stream), "randn_rows")
            out = torch.empty(B, K, 3, H, W, device=dev)
            zero = torch.zeros(1, dtype=torch.int32, device=dev)
            eager = sp.n_steps < self.GRAPH_MIN_STEPS
            for c, (r0, valid) in enumerate(chunks):
                for src, dst in ((cond, up.cond), (y_T, up.y)):       # samples r0 .. r0 + PB - 1, the last one repeated
                    _capi.check(lib.hdiff_tile_gather(src.data_ptr(), dst.data_ptr(), zero.data_ptr(), zero.data_ptr(), R, 3, H, W, 1, 1,
                                                      H, W, r0, PB, stream), "tile_gather")
                if eta > 0:
                    sp.seeds.copy_(seeds[c * PB:(c + 1) * PB])
                self._run(sp, up.y, sp.n_steps, eager, None, None, out=out.view(R, per)[r0], n=valid * per)
            mean, std = torch.empty(B, 3, H, W, device=dev), torch.empty(B, 3, H, W, device=dev)
            _capi.check(lib.hdiff_sample_stats(out.data_ptr(), B, K, per, mean.data_ptr(), std.data_ptr(), stream), "sample_stats")
        return PosteriorSamples(mean, std, out if keep_samples else None)
