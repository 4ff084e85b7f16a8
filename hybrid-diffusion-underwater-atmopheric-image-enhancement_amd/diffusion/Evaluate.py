"""The evaluation loops of the reference's second tree (``utils/rotinas.py:839-1085`` ``test``, which ``Main.py --state inference``
runs, and ``:1086`` ``inference``, which ``--state eval`` runs on the validation split): sample a set with the image-conditioned DDIM
sampler and score every result with PSNR, SSIM, UIQM and, when asked for, UCIQE.  Here the scores are taken on the device, where the
sampler leaves its output (``hdiff_amd.quality``); nothing is copied to the host per batch unless the images are to be saved.

Deliberate deviations from the reference:
  * the target is scaled by 1 / 255.  ``rotinas.py:919`` clips the 0-255 target to [0, 1] and so compares against a binary image; that
    is not copied.
  * the reference's FID (``rotinas.py:879, 914, 962-972``: an Inception distance between the 16 images of a batch, averaged over the
    batches) is not copied: there is no Inception trunk here, and a covariance of 16 samples in 2048 dimensions is singular.  In its
    place ``distribution=`` (a ``quality.DistributionMeter``, or a feature callable such as ``quality.DinoFeatures``; config keys
    ``distribution``, or ``fd_model`` with ``fd_weights``) scores the WHOLE set of outputs against the whole set of targets: the
    Frechet distance and KID over the features, on DINOv2 class tokens by default.  ``res.txt`` then ends with ``fd_orgin_avg:`` and
    ``kid_orgin_avg:`` -- deliberately not ``fid_orgin_avg:``, it is a different quantity.
  * LPIPS (``rotinas.py`` imports ``lpips``) is computed when the caller brings
    the weights: ``lpips=`` a ``quality.LPIPS`` (config key ``lpips``, or ``lpips_weights``, the path of a file holding
    ``{"vgg": <torchvision vgg16 state dict>, "lin": <the five lin weights>}``); ``res.txt`` then ends with ``lpips_orgin_avg:``.  Without
    it ``res.txt`` holds the reference's keys for what was measured and no others.
  * UCIQE (``uciqe=True``; the UCIQE part of ``nmetrics``, ``rotinas.py:923, 975-976``) is taken on the image's colour range by
    default.  The reference hands ``nmetrics`` a float image in [0, 255] (``:916``), which the colour conversion inside takes as being
    in [0, 1] already: ``uciqe_scale=255`` evaluates that, for comparing a ``res.txt`` with one of a reference run.
  * UIQM's parts are ``getUIQM``'s own (``quality.uiqm``); the reference reports the parts of ``nmetrics`` beside ``getUIQM``'s total.
  * images are written with Pillow, rounded to the nearest integer (``cv2.imwrite`` of a float image in the reference, which also
    swaps the red and blue channels on the way).
  * NIQE (``niqe=``; Mittal, Soundararajan, Bovik 2013) is not in the reference at all: it is the no-reference score for what UIQM and
    UCIQE, both underwater colour measures, say nothing about -- the atmospheric sets, and the full-size results of ``transfer=``,
    which have no target.  The pristine model comes from the caller (``quality.NIQEModel``; ``fit_niqe`` fits one on a set's targets);
    agreement with the authors' MATLAB release is unpinned, and rows with a non-finite feature leave mean and covariance alike
    (the release drops them per column for the mean).  ``res.txt`` then ends with ``niqe_orgin_avg:`` and, with ``transfer=``,
    ``niqe_full_orgin_avg:``.
  * the colour differences (``color=True``; ``quality.color_difference``) are not in the reference either: the mean CIEDE2000 of every
    result against its target, its 95th percentile over the pixels, the mean CIE76 and the mean angular error in degrees -- the
    scores dehazing and low-light benchmarks report beside PSNR and SSIM, and the only ones here that say how far the COLOUR is from
    the target's.  ``res.txt`` then ends with ``ciede2000_orgin_avg:``, ``ciede2000_p95_orgin_avg:``, ``deltae76_orgin_avg:`` and
    ``angular_orgin_avg:``.
  * ``test`` scores every image of a set: the reference's loader drops the last incomplete batch.  Its file names are those of the
    degraded images.  ``inference`` does the same on the validation split, and its means are ``sum / len``: the reference's
    ``(sum + 1) / (len + 1)`` (``:1204-1211``) is not copied.
"""
from __future__ import annotations

import os
from typing import Dict, Iterable, Iterator, List, Optional, Sequence

import torch

from .. import quality

__all__ = ["evaluate", "test", "inference", "fit_niqe", "RES_KEYS", "RES_KEYS_UCIQE", "RES_KEY_LPIPS", "RES_KEYS_DISTRIBUTION",
           "RES_KEY_NIQE", "RES_KEY_NIQE_FULL", "RES_KEYS_COLOR", "baseline_res_lines", "PREDICTION_FILE", "read_prediction", "resolve_prediction"]

# res.txt: the reference's key for each measured score, in the reference's order (rotinas.py:967-982)
RES_KEYS = (("psnr_orgin_avg:", "psnr"), ("ssim_orgin_avg:", "ssim"), ("uiqm_orgin_avg:", "uiqm"), ("uism_orgin_avg:", "uism"),
            ("uicm_orgin_avg:", "uicm"), ("uiconm_orgin_avg:", "uiconm"))
# with UCIQE: its line directly after UIQM's, the reference's position (rotinas.py:973-976)
RES_KEYS_UCIQE = RES_KEYS[:3] + (("uciqe_orgin_avg:", "uciqe"),) + RES_KEYS[3:]
# with LPIPS: one last line, behind whichever list is in use
RES_KEY_LPIPS = ("lpips_orgin_avg:", "lpips")
# with the set-level scores: two last lines, behind LPIPS's where both are on
RES_KEYS_DISTRIBUTION = (("fd_orgin_avg:", "fd"), ("kid_orgin_avg:", "kid"))
# with NIQE: one last line, behind all of the above; with transfer= as well, one more for the full-size results
RES_KEY_NIQE = ("niqe_orgin_avg:", "niqe")
RES_KEY_NIQE_FULL = ("niqe_full_orgin_avg:", "niqe_full")
# with the colour differences: four last lines, behind all of the above
RES_KEYS_COLOR = (("ciede2000_orgin_avg:", "ciede2000"), ("ciede2000_p95_orgin_avg:", "ciede2000_p95"),
                  ("deltae76_orgin_avg:", "deltae76"), ("angular_orgin_avg:", "angular"))


def _device_of(sampler) -> Optional[torch.device]:
    """Where the sampler's tensors live; None (batches stay where they are) for a callable that holds none."""
    if isinstance(sampler, torch.nn.Module):
        for t in list(sampler.buffers()) + list(sampler.parameters()):
            return t.device
    return None


def _save_batch(images01: torch.Tensor, names: Sequence[str], save_dir: str) -> None:
    from PIL import Image
    arr = (images01.detach().float().clamp(0, 1) * 255.0).round().to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()
    for img, name in zip(arr, names):
        Image.fromarray(img).save(os.path.join(save_dir, name))


def write_res(path: str, result: Dict[str, object], keys=RES_KEYS) -> None:
    with open(path, "w+") as f:
        for key, k in keys:
            f.write("\n" + key)
            f.write(str(result[k]))


def evaluate(sampler, batches: Iterable, *, ddim_step: int, tile: Optional[int] = None, tile_overlap: Optional[int] = None,
             tile_batch: Optional[int] = None, save_dir: Optional[str] = None, collect: Optional[List[torch.Tensor]] = None,
             meter=None, solver: Optional[str] = None, spacing: Optional[str] = None, uciqe: bool = False,
             uciqe_scale: float = 1.0, lpips=None, distribution=None, transfer=None, niqe=None, samples: Optional[int] = None,
             eta: float = 0.0, sample_seed: int = 0, sample_batch: Optional[int] = None, std_gain: float = 4.0,
             color: bool = False, baselines=None) -> Dict[str, object]:
    """Samples and scores a set.  ``batches`` yields ``(input, target)`` or ``(input, target, names)``: CHW images in [0, 255] as
    ``Underwater_Dataset`` / ``Atmospheric_Dataset`` produce them, batched.  Per batch: ``out = sampler(input, ddim=True,
    unconditional_guidance_scale=1, ddim_step=ddim_step, tile=...)`` (rotinas.py:907), then ``(out + 1) / 2`` is scored against
    ``target / 255``.  ``collect``, a list, receives every ``out``.  With ``save_dir`` each result is written under its name
    (``<running index>.png`` without one) as uint8, and ``res.txt`` beside them.  ``meter``: a ``quality.QualityMeter`` to go on
    filling (a new one by default).  ``solver`` / ``spacing`` are the sampler's (``solver="dpmpp2m"``: DPM-Solver++(2M) on logSNR
    time steps); ``None`` leaves the argument out of the call.  ``uciqe=True``: the default meter also scores UCIQE of
    ``clip((out + 1) / 2, 0, 1) * uciqe_scale`` (``quality.QualityMeter(uciqe=True)``; a ``meter`` passed in must report "uciqe"
    itself) and ``res.txt`` gets ``uciqe_orgin_avg:`` after UIQM's line.  ``lpips``: a ``quality.LPIPS``; the default meter also scores the
    LPIPS distance of ``(out + 1) / 2`` from ``target / 255`` (a ``meter`` passed in must report "lpips" itself), the result gains
    ``"lpips"`` and ``res.txt`` a last line ``lpips_orgin_avg:``.  ``distribution``: a ``quality.DistributionMeter`` to go on filling, or
    a feature callable (``quality.DinoFeatures``) from which one is made; it is updated beside the quality meter with the same
    ``(out + 1) / 2`` and ``target / 255``, the result gains ``"fd"`` and ``"kid"`` (of ALL the images the meter holds) and ``res.txt``
    two last lines, ``fd_orgin_avg:`` and ``kid_orgin_avg:``.  Without it nothing of that is constructed, launched or written.
    ``transfer``: a ``(radius, eps)`` pair or a dict with those keys (``hdiff_amd.transfer``: guided full-resolution transfer); it needs
    ``save_dir``, and every batch must then carry a FOURTH element, the list of its full-size uint8 ``[H_i, W_i, 3]`` originals (host
    or device tensors, or arrays).  Each image's colour map is fitted from the batch's own ``input / 255`` (exactly what the model saw)
    and ``clamp((out + 1) / 2, 0, 1)``, applied to its original and written to ``<save_dir>/full/<name>`` at the original's size.  The
    scores, ``res.txt`` and the model-sized images are what they are without it; ``transfer`` without ``save_dir``, or a batch without
    originals, raises ``ValueError`` before anything is sampled.
    ``niqe``: a ``quality.NIQEModel`` or the path of one (``NIQEModel.load``); the default meter also scores NIQE of ``(out + 1) / 2``
    at the model's ``patch`` (a ``meter`` passed in must report "niqe" itself), the result gains ``"niqe"`` (the mean over the images
    whose score is defined) and ``"niqe_undefined"``, and ``res.txt`` a last line ``niqe_orgin_avg:``.  A model-sized image smaller than
    ``patch`` raises ``ValueError``.  With ``transfer=`` as well every full-size result is scored once, at its own size, before it is
    written (one synchronisation per image, beside the one of the file): the result gains ``"niqe_full"`` (the same mean),
    ``"niqe_full_per_image"`` and ``"niqe_full_undefined"``, and ``res.txt`` one more line, ``niqe_full_orgin_avg:``.  Without it
    nothing of that is loaded, launched or written.
    ``color=True``: the default meter also scores the colour differences of ``(out + 1) / 2`` from ``target / 255``
    (``quality.QualityMeter(color=True)``; a ``meter`` passed in must report them itself), the result gains ``"ciede2000"``,
    ``"ciede2000_p95"``, ``"deltae76"`` and ``"angular"``, and ``res.txt`` four lines behind every other one: ``ciede2000_orgin_avg:``,
    ``ciede2000_p95_orgin_avg:``, ``deltae76_orgin_avg:`` and ``angular_orgin_avg:`` (under ``samples=`` their ``_sample_avg:`` /
    ``_sample_std:`` lines follow like the other per-image scores').  Without it nothing of that is launched or written.
    ``baselines``: a sequence of names out of ``hdiff_amd.classical.BASELINES`` (``"input"``, ``"gray_world"``, ``"dcp"``, ``"udcp"``,
    ``"inverted_dcp"``) or ``classical.CONTRAST_BASELINES`` (``"clahe_lab"``, ``"clahe_rgb"``, ``"equalize"``; there is no bare
    ``"clahe"``: the name says which planes were enhanced) or ``(name, callable)`` pairs, a callable taking the ``[0, 1]`` input batch to an image batch of the same shape.
    Per baseline a second meter of the main meter's configuration (a ``quality.QualityMeter``) is updated per batch with
    ``fn(input / 255)`` against ``target / 255``; the result gains ``"baselines": {name: that meter's compute() dict}`` and ``res.txt``,
    behind every other line (the ``samples=`` lines included), one line ``<score>_<name>_avg:`` per baseline in the order given, for
    every per-image score the main meter reports (the set-level ``fd`` / ``kid`` and ``niqe_full`` have none).  An unknown name raises
    before anything is sampled.  Without it nothing of that is constructed, launched or written.
    ``samples=K`` (an integer >= 1): every batch goes through ``sampler.posterior(input, K, eta=eta, seed=sample_seed,
    image_ids=<the running indices of its images in the set>, sample_batch=sample_batch, ...)`` in place of one ``sampler`` call.  The
    MEAN of the K clipped samples is the image that is scored, saved, and handed to ``distribution`` and ``transfer``; a second meter
    of the same configuration scores every replica, and the result gains ``"samples"`` (K), ``"per_sample"`` (``{column: [the set
    mean of replica 0, 1, ...]}``), ``"sample_avg"`` / ``"sample_std"`` (``{column: mean / unbiased std of those K set means}``; the
    spread is 0 for K = 1) and ``"uncertainty"`` (the mean of ``std / 2``, the per-pixel spread on the [0, 1] scale, over the set).
    ``res.txt`` keeps its lines and gains, behind them, ``samples:``, for every per-image score ``<name>_sample_avg:`` and
    ``<name>_sample_std:`` (``psnr_sample_avg:`` ...; the set-level ``fd`` / ``kid`` and ``niqe_full`` have none), and
    ``uncertainty_avg:``.  With ``save_dir``, ``<save_dir>/std/<name>`` holds ``rint(255 * clamp(std_gain * std / 2, 0, 1))``;
    ``std_gain`` is a display constant and nothing backs its default.  The noise of an image belongs to its index in the set: the
    result depends on neither torch's generator nor the batch size.  ``tile`` cannot be combined with it.  Without ``samples`` (and
    with ``eta == 0``) nothing of this is constructed, launched or written; ``eta`` without ``samples`` is refused.
    Returns ``QualityMeter.compute()``'s dict."""
    if samples is None and eta != 0:
        raise ValueError("evaluate: eta= goes with samples=")
    if samples is not None:
        if isinstance(samples, bool) or not isinstance(samples, int) or samples < 1:
            raise ValueError(f"evaluate: samples must be an integer >= 1, got {samples!r}")
        if tile is not None:
            raise ValueError("evaluate: samples= cannot be combined with tile=")
        if not hasattr(sampler, "posterior"):
            raise TypeError("evaluate: samples= needs a sampler with a posterior() method (diffusion.Diffusion.GaussianDiffusionSampler)")
    if baselines is not None:
        from ..classical import resolve_baselines
        baselines = resolve_baselines(baselines)
        if meter is not None and not isinstance(meter, quality.QualityMeter):
            raise ValueError("evaluate: baselines= needs a quality.QualityMeter (its configuration is copied for every baseline)")
    transfer = _transfer_settings(transfer)
    if transfer is not None and save_dir is None:
        raise ValueError("evaluate: transfer= writes full-size images and needs save_dir=")
    if distribution is not None and not isinstance(distribution, quality.DistributionMeter):
        distribution = quality.DistributionMeter(distribution)
    if niqe is not None and not isinstance(niqe, quality.NIQEModel):
        niqe = quality.NIQEModel.load(niqe)
    full_scores: List[float] = []
    if meter is None and color:
        meter = quality.QualityMeter(uciqe=bool(uciqe), uciqe_scale=uciqe_scale, lpips=lpips, niqe=niqe, color=True)
    if meter is None and niqe is not None:
        meter = quality.QualityMeter(uciqe=bool(uciqe), uciqe_scale=uciqe_scale, lpips=lpips, niqe=niqe)
    if meter is None:
        if lpips is not None:
            meter = quality.QualityMeter(uciqe=bool(uciqe), uciqe_scale=uciqe_scale, lpips=lpips)
        else:
            meter = quality.QualityMeter(uciqe=True, uciqe_scale=uciqe_scale) if uciqe else quality.QualityMeter()
    dev = _device_of(sampler)
    if save_dir is not None:
        os.makedirs(save_dir, exist_ok=True)
        if transfer is not None:
            os.makedirs(os.path.join(save_dir, "full"), exist_ok=True)
    tile_kw = {} if tile is None else dict(tile=tile, tile_overlap=tile_overlap, tile_batch=tile_batch)
    tile_kw.update({k: v for k, v in (("solver", solver), ("spacing", spacing)) if v is not None})
    replicas = None
    if samples is not None:
        replicas = _ReplicaScores(meter, samples)
        if save_dir is not None:
            os.makedirs(os.path.join(save_dir, "std"), exist_ok=True)
    baseline_meters = None if baselines is None else [(name, fn, _meter_like(meter)) for name, fn in baselines]
    done = 0
    with torch.no_grad():
        for batch in batches:
            inp, target = batch[0], batch[1]
            names = list(batch[2]) if len(batch) > 2 else [f"{done + i:05d}.png" for i in range(int(inp.shape[0]))]
            originals = _originals(batch, int(inp.shape[0])) if transfer is not None else None
            inp = (inp if dev is None else inp.to(dev)).float()
            target = (target if dev is None else target.to(dev)).float()
            if replicas is None:
                out = sampler(inp, ddim=True, unconditional_guidance_scale=1, ddim_step=ddim_step, **tile_kw)
            else:
                post = sampler.posterior(inp, samples, ddim_step=ddim_step, eta=eta, seed=sample_seed, sample_batch=sample_batch,
                                         image_ids=range(done, done + int(inp.shape[0])), keep_samples=True, **tile_kw)
                out = post.mean
                replicas.update(post, target / 255)
                if save_dir is not None:
                    _save_batch(std_gain * post.std / 2, names, os.path.join(save_dir, "std"))
            pred01 = (out + 1) / 2                                                        # :912
            meter.update(pred01, target / 255)
            if baseline_meters is not None:
                for _, fn, other in baseline_meters:
                    other.update(fn(inp / 255), target / 255)
            if distribution is not None:
                distribution.update(pred01, target / 255)
            if collect is not None:
                collect.append(out)
            if save_dir is not None:
                _save_batch(pred01, names, save_dir)
            if transfer is not None:
                full_scores += _save_full(inp, pred01, originals, names, os.path.join(save_dir, "full"), transfer, niqe)
            done += int(inp.shape[0])
    result = meter.compute()
    if distribution is not None:
        scores = distribution.compute()
        result["fd"], result["kid"] = scores["fd"], scores["kid"]
    if niqe is not None and transfer is not None:
        defined = [v for v in full_scores if v == v and abs(v) != float("inf")]
        result["niqe_full"] = sum(defined) / len(defined) if defined else float("nan")
        result["niqe_full_per_image"] = list(full_scores)
        result["niqe_full_undefined"] = len(full_scores) - len(defined)
    if replicas is not None:
        result.update(replicas.compute())
    if baseline_meters is not None:
        result["baselines"] = {name: other.compute() for name, _, other in baseline_meters}
    if save_dir is not None:
        keys = RES_KEYS_UCIQE if uciqe else RES_KEYS
        if lpips is not None:
            keys = keys + (RES_KEY_LPIPS,)
        if distribution is not None:
            keys = keys + RES_KEYS_DISTRIBUTION
        if niqe is not None:
            keys = keys + (RES_KEY_NIQE,) + ((RES_KEY_NIQE_FULL,) if transfer is not None else ())
        if color:
            keys = keys + RES_KEYS_COLOR
        flat = result
        if replicas is not None:
            flat, keys = sample_res_lines(result, keys)
        if baseline_meters is not None:
            flat, keys = baseline_res_lines(flat, keys, meter.columns)
        write_res(os.path.join(save_dir, "res.txt"), flat, keys)
    return result


def _meter_like(meter):
    """A new ``quality.QualityMeter`` of ``meter``'s configuration."""
    return quality.QualityMeter(uciqe=meter._uciqe, uciqe_scale=meter._uciqe_scale, lpips=meter._lpips, niqe=meter._niqe,
                                color=meter._color)


def baseline_res_lines(result: Dict[str, object], keys, columns):
    """-> (flat result, keys) for ``write_res`` under ``baselines=``: ``keys`` in their order, then per baseline in the order given one
    ``<score>_<name>_avg:`` for each of today's ``*_orgin_avg:`` lines whose score is a column of the meter."""
    flat = dict(result)
    keys = tuple(keys)
    scores = [k for label, k in keys if label.endswith("_orgin_avg:") and k in columns]
    for name, scored in result["baselines"].items():
        for k in scores:
            flat[f"{k}_{name}_avg"] = scored[k]
            keys += ((f"{k}_{name}_avg:", f"{k}_{name}_avg"),)
    return flat, keys


def sample_res_lines(result: Dict[str, object], keys):
    """-> (flat result, keys) for ``write_res`` under ``samples=``: today's ``keys`` in their order, then ``samples:``, then for each of
    them that the replicas were scored for ``<name>_sample_avg:`` and ``<name>_sample_std:``, then ``uncertainty_avg:``."""
    flat = dict(result)
    keys = tuple(keys) + (("samples:", "samples"),)
    for _, name in keys[:-1]:
        if name in result["sample_avg"]:
            flat[f"{name}_sample_avg"], flat[f"{name}_sample_std"] = result["sample_avg"][name], result["sample_std"][name]
            keys += ((f"{name}_sample_avg:", f"{name}_sample_avg"), (f"{name}_sample_std:", f"{name}_sample_std"))
    return flat, keys + (("uncertainty_avg:", "uncertainty"),)


class _ReplicaScores:
    """The per-replica side of ``evaluate(samples=K)``: a second meter of ``meter``'s configuration, updated with every replica of every
    batch, and the running sum of ``std / 2`` on the device.  Nothing here synchronises before ``compute``."""

    def __init__(self, meter, K: int):
        if not isinstance(meter, quality.QualityMeter):
            raise ValueError("evaluate: samples= needs a quality.QualityMeter (its configuration is copied for the replicas)")
        self.K = K
        self.meter = _meter_like(meter)
        self.replica_of_update: List[int] = []
        self.spread = None          # [sum of std / 2, elements] as a float64 device pair

    def update(self, post, target01: torch.Tensor) -> None:
        for r in range(self.K):
            self.meter.update((post.samples[:, r] + 1) / 2, target01)
            self.replica_of_update.append(r)
        part = torch.stack([(post.std.double() / 2).sum(), torch.tensor(float(post.std.numel()), dtype=torch.float64,
                                                                          device=post.std.device)])
        self.spread = part if self.spread is None else self.spread + part

    def compute(self) -> Dict[str, object]:
        import numpy as np
        scores = self.meter.compute()
        per = np.asarray(scores["per_image"], dtype=np.float64)
        replica = np.concatenate([np.full(n, r) for (_, n, _), r in zip(self.meter._updates, self.replica_of_update)]) \
            if self.replica_of_update else np.zeros(0)
        per_sample: Dict[str, List[float]] = {}
        for j, name in enumerate(self.meter.columns):
            cols = [per[replica == r, j] for r in range(self.K)]
            if name == "niqe":          # the meter's own rule for this column: over the images whose score is finite
                cols = [c[np.isfinite(c)] for c in cols]
            per_sample[name] = [float(c.mean()) if c.size else float("nan") for c in cols]
        avg = {name: float(np.mean(v)) for name, v in per_sample.items()}
        std = {name: float(np.std(v, ddof=1)) if self.K > 1 else 0.0 for name, v in per_sample.items()}
        total, count = (0.0, 0.0) if self.spread is None else self.spread.tolist()
        return {"samples": self.K, "per_sample": per_sample, "sample_avg": avg, "sample_std": std,
                "uncertainty": total / count if count else float("nan")}


def _transfer_settings(transfer):
    """``evaluate``'s ``transfer=`` as a checked ``(radius, eps)``, or None."""
    if transfer is None:
        return None
    from ..transfer import transfer_settings
    if isinstance(transfer, dict):
        unknown = set(transfer) - {"radius", "eps"}
        if unknown:
            raise ValueError(f"evaluate: transfer= has unknown keys {sorted(unknown)}; it takes 'radius' and 'eps'")
        return transfer_settings(transfer.get("radius", 8), transfer.get("eps", 1e-3))
    if not isinstance(transfer, (tuple, list)) or len(transfer) != 2:
        raise ValueError(f"evaluate: transfer= must be a (radius, eps) pair or a dict, got {transfer!r}")
    return transfer_settings(transfer[0], transfer[1])


def _originals(batch, count: int) -> list:
    """The fourth element of a batch under ``transfer=``: one uint8 [H, W, 3] image per sample."""
    if len(batch) < 4 or batch[3] is None:
        raise ValueError("evaluate: with transfer= every batch is (input, target, names, originals); this one has no originals")
    originals = [torch.as_tensor(o) for o in batch[3]]
    if len(originals) != count:
        raise ValueError(f"evaluate: the batch holds {count} images and {len(originals)} originals")
    for o in originals:
        if o.dtype != torch.uint8 or o.dim() != 3 or o.shape[2] != 3:
            raise ValueError(f"evaluate: an original has dtype {o.dtype} and shape {tuple(o.shape)}; it must be a uint8 [H, W, 3] image")
    return originals


def _save_full(inp: torch.Tensor, pred01: torch.Tensor, originals: list, names: Sequence[str], full_dir: str, settings,
               niqe=None) -> List[float]:
    """Writes the full-size results; with a ``quality.NIQEModel`` returns the NIQE of each, taken from the uint8 image that is written."""
    from PIL import Image
    from .. import transfer as T
    coef = T.guided_fit(inp / 255, pred01.clamp(0, 1), radius=settings[0], eps=settings[1])
    scores: List[float] = []
    for i, (orig, name) in enumerate(zip(originals, names)):
        out = T.guided_apply(coef[i], orig.to(inp.device))
        if niqe is not None:
            scores.append(float(quality.niqe(out.permute(2, 0, 1).unsqueeze(0).float() / 255, niqe)[0]))
        Image.fromarray(out.cpu().numpy()).save(os.path.join(full_dir, name))
    return scores


def _cfg(config, key: str, *default):
    if isinstance(config, dict):
        if key in config:
            return config[key]
    elif hasattr(config, key):
        return getattr(config, key)
    if default:
        return default[0]
    raise KeyError(f"the configuration has no '{key}'")


PREDICTION_FILE = "prediction.json"      # what Train.train leaves beside the checkpoints of a run whose prediction is not "eps"


def read_prediction(path: str) -> Dict[str, object]:
    """The four values of a ``prediction.json``: ``prediction``, ``loss_weighting``, ``snr_gamma``, ``y0_divisor``."""
    import json
    with open(path) as f:
        held = json.load(f)
    if not isinstance(held, dict) or "prediction" not in held:
        raise ValueError(f"{path} holds no 'prediction'")
    return held


def resolve_prediction(config, pretrained_path: str) -> str:
    """What the checkpoint at ``pretrained_path`` predicts: the configuration's ``prediction`` key, else the ``prediction.json`` lying
    beside the checkpoint, else "eps".  When both are present and disagree this raises: a v checkpoint sampled as eps (or the reverse)
    fails nowhere and returns noise."""
    from ..schedules import check_prediction
    given = _cfg(config, "prediction", None)
    beside = os.path.join(os.path.dirname(os.path.abspath(pretrained_path)), PREDICTION_FILE)
    recorded = read_prediction(beside)["prediction"] if os.path.isfile(beside) else None
    if given is not None and recorded is not None and given != recorded:
        raise ValueError(f"the configuration says prediction = {given!r}, but {beside} records that the checkpoints of that run were "
                         f"trained with prediction = {recorded!r}")
    return check_prediction(given if given is not None else (recorded if recorded is not None else "eps"))


def _batched(dataset, batch_size: int, full: bool = False) -> Iterator:
    """(input [B,3,H,W], target [B,3,H,W], file names of the degraded images) in order, the last batch as short as it comes.  ``full``
    adds a fourth element: the degraded files at their own size, uint8 [H_i, W_i, 3] host tensors (``datasets.load_image``)."""
    for start in range(0, len(dataset), batch_size):
        idx = range(start, min(start + batch_size, len(dataset)))
        items = [dataset[i] for i in idx]
        batch = (torch.stack([it[0] for it in items]), torch.stack([it[1] for it in items]),
                 [os.path.basename(dataset.paths_a[i]) for i in idx])
        if full:
            from ..datasets import load_image
            batch = batch + ([torch.from_numpy(load_image(dataset.paths_a[i]).copy()) for i in idx],)
        yield batch


def _run_sets(config, task: str) -> Dict[str, Dict[str, object]]:
    """The body ``test`` and ``inference`` share; ``task`` is the split both sets are opened with."""
    from ..datasets import Atmospheric_Dataset, Underwater_Dataset
    from .Diffusion import GaussianDiffusionSampler
    from .Model import DynamicUNet

    u_name, a_name = _cfg(config, "underwater_data_name"), _cfg(config, "atmospheric_data_name")
    root = _cfg(config, "dataset_root", None)

    def root_of(name):
        return root.get(name) if isinstance(root, dict) else root

    transforms = _cfg(config, "transforms", None)
    sets = ((u_name, Underwater_Dataset(u_name, transforms=transforms, task=task, root=root_of(u_name))),
            (a_name, Atmospheric_Dataset(a_name, transforms=transforms, task=task, root=root_of(a_name))))
    devices = _cfg(config, "device_list", None)
    device = torch.device(devices[0] if devices else "cuda:0")
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())

    model = DynamicUNet(T=_cfg(config, "T"), ch=_cfg(config, "channel"), ch_mult=_cfg(config, "channel_mult"),
                        num_res_blocks=_cfg(config, "num_res_blocks"), dropout=0.)
    path = _cfg(config, "pretrained_path")
    prediction = resolve_prediction(config, path)
    ckpt = torch.load(path, map_location="cpu")
    model.load_state_dict({k.replace("module.", ""): v for k, v in ckpt.items()})
    model.eval()
    sampler = GaussianDiffusionSampler(model, _cfg(config, "beta_1"), _cfg(config, "beta_T"), _cfg(config, "T"),
                                       **({} if prediction == "eps" else {"prediction": prediction})).to(device)

    base = os.path.join(_cfg(config, "result_root", os.path.join("output", "result")), os.path.basename(path))
    extra = {}
    if _cfg(config, "uciqe", False):
        extra = dict(uciqe=True, uciqe_scale=float(_cfg(config, "uciqe_scale", 1.0)))
    lpips = _cfg(config, "lpips", None)
    if lpips is None and _cfg(config, "lpips_weights", None) is not None:
        held = torch.load(_cfg(config, "lpips_weights"), map_location="cpu")
        lpips = quality.LPIPS(held["vgg"], held["lin"])
    if lpips is not None:
        extra["lpips"] = lpips.to(device)
    features = _cfg(config, "distribution", None)
    if features is None and _cfg(config, "fd_model", None) is not None:
        from ..dino import DinoV2Features
        trunk = DinoV2Features(_cfg(config, "fd_model"), dense=_cfg(config, "fd_dense", "conv"))
        if _cfg(config, "fd_weights", None) is not None:
            trunk.load_dinov2(torch.load(_cfg(config, "fd_weights"), map_location="cpu"))
        features = quality.DinoFeatures(trunk).to(device)
    full = bool(_cfg(config, "full_resolution", False))
    if full:
        extra["transfer"] = (_cfg(config, "transfer_radius", 8), _cfg(config, "transfer_eps", 1e-3))
    niqe_model = _cfg(config, "niqe_model", None)
    if _cfg(config, "niqe", False) or niqe_model is not None:
        if niqe_model is None:
            raise ValueError("the configuration asks for niqe and names no 'niqe_model': fit one with fit_niqe, or load the release's")
        extra["niqe"] = niqe_model if isinstance(niqe_model, quality.NIQEModel) else quality.NIQEModel.load(niqe_model)
    if _cfg(config, "color", False):
        extra["color"] = True
    if _cfg(config, "samples", None) is not None:
        extra.update(samples=_cfg(config, "samples"), eta=_cfg(config, "ddim_eta", 0.0), sample_seed=_cfg(config, "sample_seed", 0),
                     sample_batch=_cfg(config, "sample_batch", None))
    elif any(_cfg(config, k, None) is not None for k in ("ddim_eta", "sample_seed", "sample_batch")):
        raise ValueError("the configuration gives ddim_eta / sample_seed / sample_batch without 'samples'")
    if _cfg(config, "baselines", None) is not None:
        extra["baselines"] = _cfg(config, "baselines")
    results = {}
    for name, data in sets:
        if features is not None:      # one meter per set; a DistributionMeter from the configuration goes on filling across both
            extra["distribution"] = features if isinstance(features, quality.DistributionMeter) else quality.DistributionMeter(features)
        results[name] = evaluate(sampler, _batched(data, int(_cfg(config, "batch_size")), full), ddim_step=_cfg(config, "ddim_step"),
                                 tile=_cfg(config, "tile", None), tile_overlap=_cfg(config, "tile_overlap", None),
                                 tile_batch=_cfg(config, "tile_batch", None), save_dir=os.path.join(base, name),
                                 solver=_cfg(config, "solver", None), spacing=_cfg(config, "spacing", None), **extra)
    return results


def test(config, epoch=None) -> Dict[str, Dict[str, object]]:
    """``rotinas.test(config, epoch)``: the test split of ``config.underwater_data_name`` and of ``config.atmospheric_data_name``
    through ``DynamicUNet`` (``config.T / channel / channel_mult / num_res_blocks``) loaded from ``config.pretrained_path`` (a
    state dict; ``module.`` prefixes are stripped), ``config.ddim_step`` DDIM steps, results under
    ``output/result/<checkpoint file>/<set>/`` (``config.result_root`` replaces ``output/result``).  Optional keys: ``tile``,
    ``tile_overlap``, ``tile_batch`` (overlapping-window sampling), ``solver``, ``spacing`` (the sampler's; absent: the reference's DDIM), ``dataset_root`` (one root for both sets, or a dict by set
    name), ``transforms`` (the sets' ``transforms=``; default: their 256 x 256 resize), ``device_list`` (the first entry is used; default ``cuda:0``),
    ``uciqe``, ``uciqe_scale`` (``evaluate``'s; absent: no UCIQE, ``res.txt`` as before), ``lpips`` (a ``quality.LPIPS``) or
    ``lpips_weights`` (the path of a file holding ``{"vgg": ..., "lin": ...}``; absent: no LPIPS, ``res.txt`` as before),
    ``distribution`` (a feature callable such as ``quality.DinoFeatures``, or a ``quality.DistributionMeter``) or ``fd_model``
    (``"dinov2_vits14"`` / ``vitb14`` / ``vitl14``) with ``fd_weights`` (the path of the hub state dict, loaded with ``load_dinov2``) and ``fd_dense`` (``"conv"``, the default, or
    ``"tokens"``: the trunk's dense-layer route;
    the images must fit the trunk: ``H - 4`` and ``W - 4`` multiples of 14; absent: no set-level scores, ``res.txt`` as before),
    ``full_resolution`` (bool: every degraded file is also enhanced at its OWN size by guided transfer of the model-sized result and
    written to ``<set>/full/<name>``, ``evaluate``'s ``transfer=``) with ``transfer_radius`` (default 8) and ``transfer_eps`` (default
    1e-3; neither is backed by an image-quality figure; absent: nothing of it is loaded, launched or written),
    ``niqe`` (bool) with ``niqe_model`` (the path of a ``quality.NIQEModel`` file, ``.npz`` or the release's ``.mat``, or a model;
    ``evaluate``'s ``niqe=``: NIQE of every result at the model's ``patch``, and of every full-size result under ``full_resolution``;
    absent: no NIQE, ``res.txt`` as before),
    ``color`` (bool: ``evaluate``'s ``color=``, CIEDE2000 with its 95th percentile, CIE76 and the angular error of every result against
    its target; absent: none of them, ``res.txt`` as before),
    ``samples`` (K >= 1: ``evaluate``'s ``samples=``, the mean of K posterior samples per image is scored and saved, the per-pixel spread
    goes to ``<set>/std/<name>`` and ``res.txt`` gains the draw-to-draw spread of every score) with ``ddim_eta`` (default 0),
    ``sample_seed`` (default 0) and ``sample_batch`` (the most samples per model evaluation; absent: one draw from torch's generator
    per image, ``res.txt`` as before),
    ``baselines`` (``evaluate``'s ``baselines=``: names out of ``classical.BASELINES`` or ``classical.CONTRAST_BASELINES``, or ``(name,
    callable)`` pairs, each scored on ``input / 255`` against the targets beside the model, ``res.txt`` gains ``<score>_<name>_avg:`` lines; absent: nothing of it is
    constructed, launched or written),
    ``prediction`` ("eps" or "v": what the checkpoint's network predicts, the sampler's ``prediction=``; absent: read from the
    ``prediction.json`` beside ``pretrained_path`` if ``Train.train`` left one, else "eps"; present and different from that file:
    ``ValueError``, see ``resolve_prediction``).
    ``epoch`` is accepted and unused, as in the reference.  Returns ``{set name: evaluate()'s dict}``."""
    return _run_sets(config, "test")


def inference(config, epoch=None) -> Dict[str, Dict[str, object]]:
    """``rotinas.inference(config, epoch)`` (``:1086``, ``Main.py --state eval``): the same loop on the validation split
    (``task="val"``) of both sets, with ``test``'s keys (``full_resolution``, ``transfer_radius``, ``transfer_eps`` among them), results under the same ``<result_root>/<checkpoint file>/<set>/``.  Every image
    is scored, under the file name of its degraded image, and the means are ``sum / len``."""
    return _run_sets(config, "val")


def fit_niqe(config, *, out: str, split: str = "train", side: str = "target", patch: int = 96, sharp_threshold: float = 0.75,
             quantize: bool = True):
    """Fits NIQE's pristine model (``quality.NIQEModel.fit``) on the images of one side of ``config.underwater_data_name`` and
    ``config.atmospheric_data_name``, opened the way ``test`` opens them (``dataset_root``, ``transforms``, ``batch_size``,
    ``device_list``) with ``task=split``, and writes it to ``out`` (an ``.npz``).  ``side``: ``"target"`` (the clean images: what a
    pristine model is meant to describe) or ``"input"``.  A set named ``None`` is left out.  Returns the model."""
    from ..datasets import Atmospheric_Dataset, Underwater_Dataset
    if side not in ("target", "input"):
        raise ValueError(f"fit_niqe: side = {side!r}; 'target' or 'input'")
    root = _cfg(config, "dataset_root", None)
    transforms = _cfg(config, "transforms", None)
    devices = _cfg(config, "device_list", None)
    device = torch.device(devices[0] if devices else "cuda:0")
    sets = []
    for key, cls in (("underwater_data_name", Underwater_Dataset), ("atmospheric_data_name", Atmospheric_Dataset)):
        name = _cfg(config, key, None)
        if name is not None:
            sets.append(cls(name, transforms=transforms, task=split, root=root.get(name) if isinstance(root, dict) else root))
    if not sets:
        raise ValueError("fit_niqe: the configuration names no set")
    pick = 1 if side == "target" else 0

    def images():
        for data in sets:
            for batch in _batched(data, int(_cfg(config, "batch_size", 8))):
                yield batch[pick].to(device).float() / 255

    model = quality.NIQEModel.fit(images(), patch=patch, sharp_threshold=sharp_threshold, quantize=quantize)
    model.save(out)
    return model
