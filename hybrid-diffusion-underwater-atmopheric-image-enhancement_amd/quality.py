"""PSNR / SSIM / UIQM (``csrc/quality.hip``), UCIQE (``csrc/uciqe.hip``) and the colour differences (``csrc/color_diff.hip``) on the
device: the per-image scores of the reference's evaluation (``utils/rotinas.py:916-931``) taken where the sampler leaves its output,
without a copy to the host per batch.

Inputs are ``[N, 3, H, W]`` device tensors with nominal range [0, 1]; the kernels score ``clip(x, 0, 1) * 255`` as an fp32 image,
which is what ``np.clip(img, 0, 1) * 255`` hands the reference's metric calls.  Definitions:

  * ``psnr_ssim`` is ``metrics.psnr`` / ``metrics.ssim(..., channel_axis=2)`` (data range 255, 7x7 uniform window, moments in double);
  * ``uiqm`` is ``uw_metrics.getUIQM`` with its parts (pinned to the reference's functions by ``tests/golden/uw_metrics.npz``), with
    ONE deliberate difference: the trimmed means of UICM add the kept samples in double, not in an fp32 running sum.  An image with a
    constant channel has ``uism = uiqm = NaN``, as on the host.
  * ``uciqe`` is the UCIQE part of ``uw_metrics.nmetrics`` (CIE L*a*b* from sRGB in double; ``tests/_uciqe_def.py`` is the definition the
    kernels are held to) of ``clip(x, 0, 1) * scale``.  ``scale=1`` scores the image on its colour range; ``scale=255`` evaluates what
    the reference's call evaluates (a float image in [0, 255] handed to a conversion that takes floats as [0, 1]).  An image of fewer
    than 50 pixels has ``conl = uciqe = NaN``, as on the host.

``color_difference`` scores what none of the above measures: how far a prediction's COLOUR is from its target's.  Per pixel, CIE L*a*b*
of both images (the conversion of ``uciqe`` at ``scale=1``), CIEDE2000 after Sharma, Wu and Dalal 2005 with ``kL = kC = kH = 1``, CIE76,
and the angle between the two clipped RGB vectors; per image the mean and the nearest-rank 95th percentile of CIEDE2000, the mean CIE76
and the mean angle in degrees over the pixels where neither image is black (``tests/_color_def.py`` is the definition the kernels are
held to; ``tests/golden/ciede2000_sharma.json``, the published table, pins the formula).  The reference has no such score.

A non-finite input value makes the scores of its image NaN and leaves the rest of the batch alone.  Results are bitwise repeatable
and do not depend on the batch an image is scored in.

``LPIPS(vgg, lin)`` is the LPIPS v0.1 VGG distance between two images (Zhang et al., "The Unreasonable Effectiveness of Deep Features
as a Perceptual Metric"): the VGG16 trunk of ``hdiff_amd.perceptual`` tapped behind its five conv blocks, and per layer the mean over
the pixels of the weighted squared difference of the channel-normalised features (``hdiff_lpips_layer``, in double).  The weights come
from the caller -- a torchvision ``vgg16`` state dict and the five ``lin`` layers of the ``lpips`` package; none ship, none are fetched.
Scaling constants, taps and formula were written from memory of that package: agreement with it is unpinned.  The other parts of ``nmetrics`` (its own UIQM variant) and the 8-bit OpenCV
``uw_metrics.uciqe``, which the reference never calls, stay on the host.  There is no CPU fallback: CPU tensors are refused.

``niqe`` is the no-reference NIQE (Mittal, Soundararajan, Bovik 2013; ``csrc/niqe.hip``; ``tests/_niqe_def.py`` is the definition the
kernels are held to): the distance between the Gaussian fitted to the 36 AGGD features of an image's blocks and a "pristine" model
(``NIQEModel``: fitted on the device over clean images, or loaded).  It is the score for what UIQM and UCIQE, both underwater colour
measures, do not cover.  Agreement with the authors' MATLAB release is unpinned; rows with a non-finite feature (blocks over a
constant area) leave mean and covariance alike, where the release drops them per column for the mean, and the pseudo-inverse is
numpy's on the host.

The scores above are per image.  ``DistributionMeter`` scores a SET of outputs against a set of targets (``csrc/distribution.hip``): the
Frechet distance between the Gaussians fitted to the two sets' features, and KID, the unbiased estimate of the squared maximum mean
discrepancy under the kernel ``(x.y / d + 1)^3`` (Binkowski et al. 2018, "Demystifying MMD GANs").  With ``DinoFeatures`` the features
are the normalised class token of a DINOv2 trunk (``hdiff_amd.dino``), which makes the first one FD-DINOv2 (Stein et al. 2023,
"Exposing flaws of generative model evaluation metrics", who recommend it over the Inception FID).  This is NOT the reference's
``fid_orgin_avg`` (``utils/rotinas.py:879, 914, 962-972``): that one averages, over batches, a distance between 16 images in 2048
Inception dimensions.  The Frechet distance is strongly biased on sets smaller than the feature width -- the normal case for a test
set of a few hundred images -- and KID is the score that stays meaningful there.  No value of either has been measured on hub weights
or on trained models.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _capi
from . import engine as E

__all__ = ["psnr_ssim", "uiqm", "uciqe", "color_difference", "ciede2000_lab", "LPIPS", "QualityMeter", "moments", "kid_sums", "kid",
           "frechet_from_moments", "DinoFeatures", "DistributionMeter", "niqe_features", "NIQEModel", "niqe_from_moments", "niqe"]

COLUMNS = ("psnr", "ssim", "uiqm", "uicm", "uism", "uiconm")      # the columns of QualityMeter's per-image rows
UCIQE_COLUMNS = ("uciqe", "uciqe_sc", "uciqe_conl", "uciqe_us")   # the four more of QualityMeter(uciqe=True)
COLOR_COLUMNS = ("ciede2000", "ciede2000_p95", "deltae76", "angular")      # four more with QualityMeter(color=True), behind UCIQE's
LPIPS_COLUMNS = ("lpips",)                                        # the last one of QualityMeter(lpips=metric)
NIQE_COLUMNS = ("niqe",)                                          # the last one of QualityMeter(niqe=model), behind LPIPS's
NIQE_ROW = 36                                                     # features of a block: 18 per scale
NIQE_MOMENTS = NIQE_ROW + NIQE_ROW * NIQE_ROW + 1                 # mean, covariance, count of valid rows: per image


def _image_batch(t: torch.Tensor, name: str) -> torch.Tensor:
    if not torch.is_tensor(t):
        raise TypeError(f"hdiff: '{name}' must be a tensor, got {type(t).__name__}")
    if t.is_cuda:
        if t.is_floating_point() and t.dtype != torch.float32:
            t = t.float()
        if not t.is_contiguous():
            t = t.contiguous()
    E.require_gpu_tensor(t, name)
    if t.dtype != torch.float32:
        raise RuntimeError(f"hdiff: '{name}' has dtype {t.dtype}; the quality scores take floating-point images in [0, 1]")
    if t.dim() != 4 or t.shape[1] != 3:
        raise RuntimeError(f"hdiff: '{name}' has shape {tuple(t.shape)}; the quality scores take [N, 3, H, W] images")
    return t


def _scratch(N: int, H: int, W: int, dev) -> torch.Tensor:
    need = C.c_int64(0)
    _capi.check(_capi.lib().hdiff_quality_workspace(N, H, W, C.byref(need)), "quality_workspace")
    return torch.empty(need.value, dtype=torch.uint8, device=dev)


def _uciqe_scratch(N: int, H: int, W: int, dev) -> torch.Tensor:
    need = C.c_int64(0)
    _capi.check(_capi.lib().hdiff_uciqe_workspace(N, H, W, C.byref(need)), "uciqe_workspace")
    return torch.empty(need.value, dtype=torch.uint8, device=dev)


def _color_scratch(N: int, H: int, W: int, dev) -> torch.Tensor:
    need = C.c_int64(0)
    _capi.check(_capi.lib().hdiff_color_diff_workspace(N, H, W, C.byref(need)), "color_diff_workspace")
    return torch.empty(need.value, dtype=torch.uint8, device=dev)


def _stream(dev) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def _psnr_ssim_into(pred: torch.Tensor, target: torch.Tensor, out: torch.Tensor, scratch: torch.Tensor) -> None:
    N, _, H, W = (int(v) for v in pred.shape)
    _capi.check(_capi.lib().hdiff_psnr_ssim(target.data_ptr(), pred.data_ptr(), N, H, W, out.data_ptr(), scratch.data_ptr(),
                                            _stream(pred.device)), "psnr_ssim")


def _uiqm_into(img: torch.Tensor, out: torch.Tensor, scratch: torch.Tensor) -> None:
    N, _, H, W = (int(v) for v in img.shape)
    _capi.check(_capi.lib().hdiff_uiqm(img.data_ptr(), N, H, W, out.data_ptr(), scratch.data_ptr(), _stream(img.device)), "uiqm")


def _uciqe_into(img: torch.Tensor, scale: float, out: torch.Tensor, scratch: torch.Tensor) -> None:
    N, _, H, W = (int(v) for v in img.shape)
    _capi.check(_capi.lib().hdiff_uciqe(img.data_ptr(), N, H, W, float(scale), out.data_ptr(), scratch.data_ptr(),
                                        _stream(img.device)), "uciqe")


def _color_into(pred: torch.Tensor, target: torch.Tensor, out: torch.Tensor, scratch: torch.Tensor,
                map_out: Optional[torch.Tensor] = None) -> None:
    N, _, H, W = (int(v) for v in pred.shape)
    _capi.check(_capi.lib().hdiff_color_diff(pred.data_ptr(), target.data_ptr(), N, H, W, out.data_ptr(),
                                             None if map_out is None else map_out.data_ptr(), scratch.data_ptr(),
                                             _stream(pred.device)), "color_diff")


def psnr_ssim(pred01: torch.Tensor, target01: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (psnr[N], ssim[N]), float64 device tensors.  PSNR is +inf for identical images."""
    pred, target = _image_batch(pred01, "pred01"), _image_batch(target01, "target01")
    if pred.shape != target.shape or pred.device != target.device:
        raise ValueError("Input images must have the same dimensions.")
    N, _, H, W = (int(v) for v in pred.shape)
    out = torch.empty(N, 2, dtype=torch.float64, device=pred.device)
    with torch.cuda.device(pred.device):
        _psnr_ssim_into(pred, target, out, _scratch(N, H, W, pred.device))
    return out[:, 0], out[:, 1]


def uiqm(img01: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """-> (uicm[N], uism[N], uiconm[N], uiqm[N]), float64 device tensors."""
    img = _image_batch(img01, "img01")
    N, _, H, W = (int(v) for v in img.shape)
    out = torch.empty(N, 4, dtype=torch.float64, device=img.device)
    with torch.cuda.device(img.device):
        _uiqm_into(img, out, _scratch(N, H, W, img.device))
    return out[:, 0], out[:, 1], out[:, 2], out[:, 3]


def uciqe(img01: torch.Tensor, *, scale: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """-> (sc[N], conl[N], us[N], uciqe[N]), float64 device tensors: chroma spread, luminance contrast (mean of the 1 % largest L minus
    mean of the 1 % smallest), mean saturation, and ``0.4680 sc + 0.2745 conl + 0.2576 us``, of ``clip(img01, 0, 1) * scale``."""
    img = _image_batch(img01, "img01")
    N, _, H, W = (int(v) for v in img.shape)
    out = torch.empty(N, 4, dtype=torch.float64, device=img.device)
    with torch.cuda.device(img.device):
        _uciqe_into(img, scale, out, _uciqe_scratch(N, H, W, img.device))
    return out[:, 0], out[:, 1], out[:, 2], out[:, 3]


def color_difference(pred01: torch.Tensor, target01: torch.Tensor, *, with_map: bool = False):
    """-> (de00[N], de00_p95[N], de76[N], angular[N]), float64 device tensors: the mean CIEDE2000 between ``clip(pred01, 0, 1)`` and
    ``clip(target01, 0, 1)``, its nearest-rank 95th percentile over the pixels, the mean CIE76, and the mean angle in degrees between
    the RGB vectors over the pixels where neither is black (NaN when there is none).  ``with_map``: a fifth element, the per-pixel
    CIEDE2000 as an fp32 ``[N, 1, H, W]`` tensor.  Never synchronises."""
    pred, target = _image_batch(pred01, "pred01"), _image_batch(target01, "target01")
    if pred.shape != target.shape or pred.device != target.device:
        raise ValueError("Input images must have the same dimensions.")
    N, _, H, W = (int(v) for v in pred.shape)
    out = torch.empty(N, 4, dtype=torch.float64, device=pred.device)
    de_map = torch.empty(N, 1, H, W, dtype=torch.float32, device=pred.device) if with_map else None
    with torch.cuda.device(pred.device):
        _color_into(pred, target, out, _color_scratch(N, H, W, pred.device), de_map)
    scores = (out[:, 0], out[:, 1], out[:, 2], out[:, 3])
    return scores + (de_map,) if with_map else scores


def ciede2000_lab(lab1: torch.Tensor, lab2: torch.Tensor) -> torch.Tensor:
    """-> float64 ``[n]`` on the device: CIEDE2000 (``kL = kC = kH = 1``) between the rows of two float64 ``[n, 3]`` device tensors of
    (L, a, b), through the device function ``color_difference`` uses.  For data that is Lab already."""
    for t, name in ((lab1, "lab1"), (lab2, "lab2")):
        if not torch.is_tensor(t):
            raise TypeError(f"hdiff: '{name}' must be a tensor, got {type(t).__name__}")
        if not t.is_cuda:                           # engine.require_gpu_tensor's refusal; its dtype rule does not apply to Lab rows
            raise RuntimeError(f"hdiff: '{name}' lives on {t.device}; the HIP path needs an MI355X device tensor "
                               "(there is deliberately no CPU fallback)")
    a, b = lab1.detach().contiguous(), lab2.detach().contiguous()
    if a.dtype != torch.float64 or b.dtype != torch.float64 or a.dim() != 2 or a.shape[1] != 3 or a.shape[0] < 1:
        raise RuntimeError(f"hdiff: ciede2000_lab takes float64 [n, 3] rows, got {a.dtype} {tuple(a.shape)} and {b.dtype} "
                           f"{tuple(b.shape)}")
    if a.shape != b.shape or a.device != b.device:
        raise ValueError("ciede2000_lab: the two sets of rows must have the same shape and device")
    out = torch.empty(int(a.shape[0]), dtype=torch.float64, device=a.device)
    with torch.cuda.device(a.device):
        _capi.check(_capi.lib().hdiff_ciede2000_lab(a.data_ptr(), b.data_ptr(), int(a.shape[0]), out.data_ptr(), _stream(a.device)),
                    "ciede2000_lab")
    return out


class LPIPS:
    """``metric(a01, b01)`` -> float64 ``[N]`` on the device: the LPIPS v0.1 VGG distance of images in [0, 1].

    ``vgg``: a ``perceptual.VGGFeatures("vgg16")``, a torchvision ``vgg16`` state dict, or the path of a file holding one.  ``lin``: five
    tensors ``[1, C, 1, 1]`` (C = 64, 128, 256, 512, 512), a dict with the keys ``lin<k>.model.1.weight``, or the path of one.  Inputs
    are mapped to [-1, 1], scaled per channel (``hdiff_scale_input``: one kernel, not folded into the first conv, whose zero padding
    would see the shift), run through the trunk without a graph, and the five layer distances are added in layer order.  The tensors
    follow the images' device on first use."""

    TAPS = (3, 8, 15, 22, 29)
    CHANNELS = (64, 128, 256, 512, 512)
    SHIFT = (-0.030, -0.088, -0.188)
    SCALE = (0.458, 0.448, 0.450)
    MIN_SIDE = 16

    def __init__(self, vgg, lin):
        from .perceptual import VGGFeatures
        if isinstance(vgg, VGGFeatures):
            if list(vgg.cfg) != list(VGGFeatures("vgg16").cfg):
                raise ValueError("LPIPS: the trunk must be VGGFeatures('vgg16')")
            self.vgg = vgg
        else:
            if not isinstance(vgg, dict):
                vgg = torch.load(vgg, map_location="cpu")
            self.vgg = VGGFeatures("vgg16").load_torchvision(vgg)
        if not isinstance(lin, (dict, list, tuple)):
            lin = torch.load(lin, map_location="cpu")
        if isinstance(lin, dict):
            missing = [f"lin{k}.model.1.weight" for k in range(5) if f"lin{k}.model.1.weight" not in lin]
            if missing:
                raise ValueError(f"LPIPS: the lin weights lack {missing}")
            lin = [lin[f"lin{k}.model.1.weight"] for k in range(5)]
        if len(lin) != 5:
            raise ValueError(f"LPIPS: five lin layers are needed, got {len(lin)}")
        self.lin = []
        for k, (w, c) in enumerate(zip(lin, self.CHANNELS)):
            if not torch.is_tensor(w) or w.numel() != c:
                raise ValueError(f"LPIPS: lin{k} must hold {c} weights ([1, {c}, 1, 1])")
            self.lin.append(w.detach().to(dtype=torch.float32).reshape(c).contiguous())
        self.shift = torch.tensor(self.SHIFT, dtype=torch.float32)
        self.scale = torch.tensor(self.SCALE, dtype=torch.float32)

    def to(self, device) -> "LPIPS":
        self.vgg.to(device)
        self.lin = [w.to(device) for w in self.lin]
        self.shift, self.scale = self.shift.to(device), self.scale.to(device)
        return self

    def _scaled(self, img: torch.Tensor) -> torch.Tensor:
        N, _, H, W = (int(v) for v in img.shape)
        out = torch.empty_like(img)
        _capi.check(_capi.lib().hdiff_scale_input(img.data_ptr(), self.shift.data_ptr(), self.scale.data_ptr(), C.c_float(2.0),
                                                  C.c_float(-1.0), out.data_ptr(), N, 3, H, W, _stream(img.device)), "scale_input")
        return out

    def _into(self, a: torch.Tensor, b: torch.Tensor, out: torch.Tensor) -> None:
        """Zeroes ``out`` (float64 ``[N]``, contiguous) and adds the five layers; the caller holds the device context."""
        lib = _capi.lib()
        if self.shift.device != a.device:
            self.to(a.device)
        with torch.no_grad():
            f0 = self.vgg(self._scaled(a), self.TAPS)
            f1 = self.vgg(self._scaled(b), self.TAPS)
        out.zero_()
        for u, v, w in zip(f0, f1, self.lin):
            N, Cc, H, W = (int(s) for s in u.shape)
            need = C.c_int64(0)
            _capi.check(lib.hdiff_lpips_layer_workspace(N, Cc, H, W, C.byref(need)), "lpips_layer_workspace")
            ws = torch.empty(need.value, dtype=torch.uint8, device=a.device)
            _capi.check(lib.hdiff_lpips_layer(u.data_ptr(), v.data_ptr(), w.data_ptr(), N, Cc, H, W, out.data_ptr(), ws.data_ptr(),
                                              _stream(a.device)), "lpips_layer")

    def _checked(self, a01, b01):
        a, b = _image_batch(a01, "a01"), _image_batch(b01, "b01")
        if a.shape != b.shape or a.device != b.device:
            raise ValueError("Input images must have the same dimensions.")
        if min(int(a.shape[2]), int(a.shape[3])) < self.MIN_SIDE:
            raise ValueError(f"LPIPS: images of {int(a.shape[2])} x {int(a.shape[3])}; each side must be at least {self.MIN_SIDE} "
                             "(four poolings lie in front of the last tap)")
        return a, b

    def metric(self, a01: torch.Tensor, b01: torch.Tensor) -> torch.Tensor:
        a, b = self._checked(a01, b01)
        out = torch.empty(int(a.shape[0]), dtype=torch.float64, device=a.device)
        with torch.cuda.device(a.device):
            self._into(a, b, out)
        return out

    __call__ = metric


class QualityMeter:
    """Accumulates per-image scores on the device: ``update`` per batch (never synchronises), ``compute`` once at the end (one copy).

    Rows are ``COLUMNS`` = (psnr, ssim, uiqm, uicm, uism, uiconm); psnr / ssim are NaN for the images of an ``update`` without a
    target, and the means of those two are taken over the images that had one.  With ``uciqe=True`` every row gains
    ``UCIQE_COLUMNS`` = (uciqe, uciqe_sc, uciqe_conl, uciqe_us) of ``clip(pred, 0, 1) * uciqe_scale`` (``quality.uciqe``); without it
    the rows, the launches and ``compute``'s dict are those of the six columns alone.  With ``color=True`` every row gains
    ``COLOR_COLUMNS`` = (ciede2000, ciede2000_p95, deltae76, angular) of the prediction against its target (``color_difference``),
    behind UCIQE's where both are on and in front of LPIPS's and NIQE's: NaN for the images of an ``update`` without a target, and
    their means are taken like PSNR's; without it nothing of it is allocated, launched or reported.  With ``lpips=metric`` (an ``LPIPS``) every row
    gains ``LPIPS_COLUMNS`` = (lpips,) as its LAST column, behind UCIQE's where both are on: the distance of the prediction from its
    target, NaN for the images of an ``update`` without one, and its mean is taken like PSNR's.  With ``niqe=model`` (a ``NIQEModel``)
    every row gains ``NIQE_COLUMNS`` = (niqe,) as its LAST column, behind LPIPS's where both are on: ``update`` leaves the
    ``NIQE_MOMENTS`` doubles of each image (``hdiff_niqe_moments``) in a second device bank and never synchronises, ``compute`` copies
    that bank once and finishes every score on the host (``niqe_from_moments``).  The mean of the column is taken over the images
    whose score is finite; ``"niqe_undefined"`` counts the others (fewer than two valid blocks, a NaN pixel).  An image smaller than
    the model's ``patch`` is refused before a row is written.  Without ``niqe=`` nothing of it is allocated, launched or reported."""

    def __init__(self, capacity: int = 64, *, uciqe: bool = False, uciqe_scale: float = 1.0, lpips: Optional[LPIPS] = None,
                 niqe: Optional["NIQEModel"] = None, color: bool = False):
        self._capacity = max(1, int(capacity))
        self._uciqe, self._uciqe_scale = bool(uciqe), float(uciqe_scale)
        if lpips is not None and not isinstance(lpips, LPIPS):
            raise TypeError(f"QualityMeter: lpips must be a quality.LPIPS, got {type(lpips).__name__}")
        self._lpips = lpips
        self._color = bool(color)
        self.columns = COLUMNS + UCIQE_COLUMNS if self._uciqe else COLUMNS
        if self._color:
            self.columns = self.columns + COLOR_COLUMNS
        if lpips is not None:
            self.columns = self.columns + LPIPS_COLUMNS
        if niqe is not None and not isinstance(niqe, NIQEModel):
            raise TypeError(f"QualityMeter: niqe must be a quality.NIQEModel, got {type(niqe).__name__}")
        self._niqe = niqe
        if niqe is not None:
            self.columns = self.columns + NIQE_COLUMNS
        self._niqe_bank: Optional[torch.Tensor] = None   # [capacity, NIQE_MOMENTS] float64 beside the rows
        self._rows: Optional[torch.Tensor] = None      # [capacity, 6 or 10] float64 on the device of the first update
        self._n = 0
        self._updates = []                             # (first row, rows, had a target): host bookkeeping

    def __len__(self) -> int:
        return self._n

    def _reserve(self, extra: int, dev) -> None:
        if self._rows is None:
            while self._capacity < extra:
                self._capacity *= 2
            self._rows = torch.empty(self._capacity, len(self.columns), dtype=torch.float64, device=dev)
            if self._niqe is not None:
                self._niqe_bank = torch.empty(self._capacity, NIQE_MOMENTS, dtype=torch.float64, device=dev)
            return
        if self._rows.device != dev:
            raise RuntimeError(f"hdiff: QualityMeter holds rows on {self._rows.device}, the update is on {dev}")
        if self._n + extra > self._capacity:
            while self._capacity < self._n + extra:
                self._capacity *= 2
            grown = torch.empty(self._capacity, len(self.columns), dtype=torch.float64, device=dev)
            grown[:self._n].copy_(self._rows[:self._n])
            self._rows = grown
            if self._niqe is not None:
                bank = torch.empty(self._capacity, NIQE_MOMENTS, dtype=torch.float64, device=dev)
                bank[:self._n].copy_(self._niqe_bank[:self._n])
                self._niqe_bank = bank

    def update(self, pred01: torch.Tensor, target01: Optional[torch.Tensor] = None) -> None:
        pred = _image_batch(pred01, "pred01")
        target = None if target01 is None else _image_batch(target01, "target01")
        if target is not None and (pred.shape != target.shape or pred.device != target.device):
            raise ValueError("Input images must have the same dimensions.")
        if self._lpips is not None and target is not None:
            self._lpips._checked(pred, target)                    # a size LPIPS cannot take is refused before a row is written
        N, _, H, W = (int(v) for v in pred.shape)
        if self._niqe is not None:
            _niqe_blocks(H, W, self._niqe.patch)                  # an image smaller than patch likewise
        dev = pred.device
        self._reserve(N, dev)
        with torch.cuda.device(dev):
            scratch = _scratch(N, H, W, dev)
            rows = self._rows[self._n:self._n + N]
            pair = torch.empty(N, 2, dtype=torch.float64, device=dev)
            four = torch.empty(N, 4, dtype=torch.float64, device=dev)
            if target is not None:
                _psnr_ssim_into(pred, target, pair, scratch)
                rows[:, 0:2].copy_(pair)
            else:
                rows[:, 0:2].fill_(float("nan"))
            _uiqm_into(pred, four, scratch)             # same stream: the scratch is reused in order
            rows[:, 2].copy_(four[:, 3])
            rows[:, 3:6].copy_(four[:, 0:3])
            if self._uciqe:
                _uciqe_into(pred, self._uciqe_scale, four, _uciqe_scratch(N, H, W, dev))
                rows[:, 6].copy_(four[:, 3])
                rows[:, 7:10].copy_(four[:, 0:3])
            if self._color:
                at = 10 if self._uciqe else 6
                if target is not None:
                    _color_into(pred, target, four, _color_scratch(N, H, W, dev))
                    rows[:, at:at + 4].copy_(four)
                else:
                    rows[:, at:at + 4].fill_(float("nan"))
            if self._lpips is not None:
                at = len(self.columns) - 1 - (1 if self._niqe is not None else 0)
                if target is not None:
                    dist = torch.empty(N, dtype=torch.float64, device=dev)
                    self._lpips._into(pred, target, dist)
                    rows[:, at].copy_(dist)
                else:
                    rows[:, at].fill_(float("nan"))
            if self._niqe is not None:
                feats, sharp = _niqe_features_checked(pred, self._niqe.patch, self._niqe.quantize)
                _niqe_moments_into(feats, sharp, 0.0, self._niqe_bank[self._n:self._n + N])
                rows[:, -1].fill_(float("nan"))                   # filled by compute(), on the host
        self._updates.append((self._n, N, target is not None))
        self._n += N

    def compute(self) -> Dict[str, object]:
        """{"n", "psnr", "ssim", "uiqm", "uicm", "uism", "uiconm"} as float means over the images (an infinite PSNR makes the mean
        infinite, as the reference's ``sum(list) / len(list)`` does) and "per_image", the ``[n, 6]`` float64 rows; with ``uciqe=True``
        also the means of ``UCIQE_COLUMNS``, and "per_image" is ``[n, 10]``; with ``color=True`` also the means of ``COLOR_COLUMNS`` (over the images that had a
        target) and four more columns; with ``lpips=`` also "lpips" (likewise) and one more column; with ``niqe=`` also "niqe" (over the images whose score is finite), "niqe_undefined" (how many
        are not) and one more column."""
        per = np.empty((0, len(self.columns))) if self._rows is None else self._rows[:self._n].cpu().numpy()
        if self._niqe is not None and self._n:
            per[:, -1] = _niqe_scores(self._niqe, self._niqe_bank[:self._n].cpu().numpy())
        paired = np.zeros(self._n, dtype=bool)
        for start, count, has_target in self._updates:
            paired[start:start + count] = has_target
        res: Dict[str, object] = {"n": int(self._n)}
        for j, k in enumerate(self.columns):
            col = per[paired, j] if k in ("psnr", "ssim", "lpips") or k in COLOR_COLUMNS else per[:, j]
            res[k] = float(np.sum(col) / col.size) if col.size else float("nan")
        if self._niqe is not None:
            col = per[:, -1]
            defined = col[np.isfinite(col)]
            res["niqe"] = float(np.sum(defined) / defined.size) if defined.size else float("nan")
            res["niqe_undefined"] = int(col.size - defined.size)
        res["per_image"] = per
        return res


# ----------------------------------------------------------------------------------------------------------------------
# set-level scores: feature moments, the Frechet distance, KID (csrc/distribution.hip)
# ----------------------------------------------------------------------------------------------------------------------
def _feature_rows(t: torch.Tensor, name: str) -> torch.Tensor:
    """``[n, d]`` fp32 on the device, addressed in place by its two strides where they are positive."""
    if not torch.is_tensor(t):
        raise TypeError(f"hdiff: '{name}' must be a tensor, got {type(t).__name__}")
    if t.is_cuda and t.is_floating_point() and t.dtype != torch.float32:
        t = t.float()
    if not t.is_cuda:                               # engine.require_gpu_tensor's refusal; its contiguity rule does not apply to a view
        raise RuntimeError(f"hdiff: '{name}' lives on {t.device}; the HIP path needs an MI355X device tensor "
                           "(there is deliberately no CPU fallback)")
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise RuntimeError(f"hdiff: '{name}' has dtype {t.dtype} and shape {tuple(t.shape)}; features are floating-point [n, d] rows")
    if min(t.stride()) < 1:
        t = t.contiguous()
    return t.detach()


def moments(feats: torch.Tensor) -> Tuple[int, torch.Tensor, torch.Tensor]:
    """-> (n, mean[d], cov[d, d]), float64 device tensors, of ``feats`` ``[n, d]`` (any positive strides: a class-token view is read in
    place).  ``cov`` is the unbiased sample covariance (divided by ``n - 1``; NaN for ``n = 1``), two passes in double, symmetric bit
    for bit.  The raw kernel call: a non-finite feature spoils what it touches and raises nothing."""
    f = _feature_rows(feats, "feats")
    n, d = int(f.shape[0]), int(f.shape[1])
    mean = torch.empty(d, dtype=torch.float64, device=f.device)
    cov = torch.empty(d, d, dtype=torch.float64, device=f.device)
    with torch.cuda.device(f.device):
        _capi.check(_capi.lib().hdiff_feat_moments(f.data_ptr(), n, d, f.stride(0), f.stride(1), mean.data_ptr(), cov.data_ptr(),
                                                   _stream(f.device)), "feat_moments")
    return n, mean, cov


def kid_sums(feats_a: torch.Tensor, feats_b: torch.Tensor) -> torch.Tensor:
    """-> float64 ``[3]`` on the device: the sum of ``k(a_i, a_j)`` over ``i != j``, the same over ``b``, and the sum of ``k(a_i, b_j)``
    over all pairs, ``k(x, y) = (x.y / d + 1)^3`` in double.  Swapping the arguments swaps the first two sums, bit for bit."""
    a, b = _feature_rows(feats_a, "feats_a"), _feature_rows(feats_b, "feats_b")
    if a.shape[1] != b.shape[1] or a.device != b.device:
        raise ValueError(f"kid: the two sets must share their feature width and device, got {tuple(a.shape)} on {a.device} and "
                         f"{tuple(b.shape)} on {b.device}")
    n, m, d = int(a.shape[0]), int(b.shape[0]), int(a.shape[1])
    need = C.c_int64(0)
    _capi.check(_capi.lib().hdiff_kid_workspace(n, m, C.byref(need)), "kid_workspace")
    out = torch.empty(3, dtype=torch.float64, device=a.device)
    with torch.cuda.device(a.device):
        scratch = torch.empty(need.value, dtype=torch.uint8, device=a.device)
        _capi.check(_capi.lib().hdiff_kid_sums(a.data_ptr(), n, b.data_ptr(), m, d, a.stride(0), a.stride(1), b.stride(0), b.stride(1),
                                               out.data_ptr(), scratch.data_ptr(), _stream(a.device)), "kid_sums")
    return out


def _kid_from_sums(sums, n: int, m: int) -> float:
    s = [float(v) for v in sums]
    if n < 2 or m < 2 or not np.isfinite(s).all():
        return float("nan")
    return s[0] / (n * (n - 1)) + s[1] / (m * (m - 1)) - 2 * s[2] / (n * m)


def kid(feats_a: torch.Tensor, feats_b: torch.Tensor) -> float:
    """The unbiased estimate of the squared MMD between the two sets under ``k(x, y) = (x.y / d + 1)^3``:
    ``sum_{i != j} k(a_i, a_j) / (n (n - 1)) + sum_{i != j} k(b_i, b_j) / (m (m - 1)) - 2 sum_{i, j} k(a_i, b_j) / (n m)`` over the WHOLE
    sets.  There is no subset resampling: the customary mean over 100 subsets of 1000 bounds the cost on sets of tens of thousands,
    and on sets of a few hundred images the full estimate is the one with the lower variance.  It can come out slightly negative for
    two samples of one distribution.  NaN if ``n < 2`` or ``m < 2`` or a feature is not finite."""
    sums = kid_sums(feats_a, feats_b).cpu().numpy()
    return _kid_from_sums(sums, int(feats_a.shape[0]), int(feats_b.shape[0]))


def _host64(v) -> np.ndarray:
    if torch.is_tensor(v):
        v = v.detach().cpu().numpy()
    return np.asarray(v, dtype=np.float64)


def frechet_from_moments(mean_a, cov_a, mean_b, cov_b) -> float:
    """``|mu_a - mu_b|^2 + tr S_a + tr S_b - 2 tr (S_a^1/2 S_b S_a^1/2)^1/2`` on the host in float64 (tensors are copied once; ``d`` is at
    most a thousand or so, once per set).  ``R = S_a^1/2`` comes from ``eigh(S_a)`` with negative eigenvalues clamped to 0, the last
    trace is the sum of the square roots of the eigenvalues of the symmetrised ``R S_b R``, clamped to 0 likewise.  No ``sqrtm``: the
    route stays real on rank-deficient covariances (fewer rows than dimensions), which the reference patches with a ``1e-6`` offset.
    NaN if a moment is not finite."""
    ma, ca, mb, cb = _host64(mean_a), _host64(cov_a), _host64(mean_b), _host64(cov_b)
    d = ma.shape[0]
    if ma.shape != (d,) or mb.shape != (d,) or ca.shape != (d, d) or cb.shape != (d, d):
        raise ValueError(f"frechet_from_moments: shapes {ma.shape}, {ca.shape}, {mb.shape}, {cb.shape}; means [d] and covariances [d, d]")
    if not (np.isfinite(ma).all() and np.isfinite(mb).all() and np.isfinite(ca).all() and np.isfinite(cb).all()):
        return float("nan")
    lam_a, vec = np.linalg.eigh(ca)
    root = (vec * np.sqrt(np.maximum(lam_a, 0.0))) @ vec.T
    inner = root @ cb @ root
    lam = np.maximum(np.linalg.eigvalsh((inner + inner.T) / 2), 0.0)
    diff = ma - mb
    return float(diff @ diff + np.trace(ca) + np.trace(cb) - 2.0 * np.sqrt(lam).sum())


class DinoFeatures:
    """``features(images01)`` -> the class-token features ``[N, d]`` of images in [0, 1], ``[N, 3, H, W]``: the ``head`` tap of a
    ``dino.DinoV2Features`` (the class token behind the last LayerNorm), returned as the strided view ``nf[:, :, 0]`` of the trunk's
    ``(N, d, L)`` output.  With ``normalize`` the images first get ImageNet's mean and std (``hdiff_scale_input``, one kernel).  The
    trunk's own size rule applies: 2 pixels come off every edge and the rest must be whole 14 x 14 patches (256 -> 252).  Runs under
    ``no_grad``.  A trunk without loaded weights warns once (the trunk's own ``RuntimeWarning``): its scores are not FD-DINOv2."""

    MEAN = (0.485, 0.456, 0.406)
    STD = (0.229, 0.224, 0.225)

    def __init__(self, trunk, *, normalize: bool = True):
        from .dino import DinoV2Features
        if not isinstance(trunk, DinoV2Features):
            raise TypeError(f"DinoFeatures: trunk must be a dino.DinoV2Features, got {type(trunk).__name__}")
        self.trunk, self.normalize = trunk, bool(normalize)
        self.name = str(trunk.model_name)
        self.shift = torch.tensor(self.MEAN, dtype=torch.float32)
        self.scale = torch.tensor(self.STD, dtype=torch.float32)

    def to(self, device) -> "DinoFeatures":
        self.trunk.to(device)
        self.shift, self.scale = self.shift.to(device), self.scale.to(device)
        return self

    def scaled(self, images01: torch.Tensor) -> torch.Tensor:
        """``(x - mean[c]) / std[c]`` in fp32: what the trunk is fed when ``normalize`` is on."""
        img = _image_batch(images01, "images01")
        if self.shift.device != img.device:
            self.shift, self.scale = self.shift.to(img.device), self.scale.to(img.device)
        N, _, H, W = (int(v) for v in img.shape)
        out = torch.empty_like(img)
        with torch.cuda.device(img.device):
            _capi.check(_capi.lib().hdiff_scale_input(img.data_ptr(), self.shift.data_ptr(), self.scale.data_ptr(), C.c_float(1.0),
                                                      C.c_float(0.0), out.data_ptr(), N, 3, H, W, _stream(img.device)), "scale_input")
        return out

    def __call__(self, images01: torch.Tensor) -> torch.Tensor:
        img = _image_batch(images01, "images01")
        with torch.no_grad():
            return self.trunk(self.scaled(img) if self.normalize else img, ["head"])[0]


class DistributionMeter:
    """Collects the features of two image sets on the device and scores one set against the other: ``update`` per batch (never
    synchronises), ``compute`` once at the end.

    ``features``: a callable that maps ``[N, 3, H, W]`` images in [0, 1] to ``[N, d]`` fp32 features on the device -- a
    ``DinoFeatures``, or any other extractor (a caller who has an Inception trunk gets an FID out of the same machinery).
    ``update(pred01, target01)`` appends the features of both batches to two growing fp32 banks (they double from ``capacity`` rows,
    as ``QualityMeter``'s rows do); ``update(pred01)`` fills the prediction bank only and ``add_reference(images01)`` the other one, so
    the two sets need neither pairing nor equal sizes.  ``compute()`` -> ``{"n_pred", "n_ref", "fd", "kid", "features"}``: the Frechet
    distance between the two banks' moments (``moments``, ``frechet_from_moments``), ``kid`` over the whole banks, and the extractor's
    name.  A non-finite feature in either bank makes BOTH scores NaN; so does an empty bank, and a bank of one row (no covariance, no
    off-diagonal pair)."""

    def __init__(self, features, capacity: int = 64):
        if not callable(features):
            raise TypeError(f"DistributionMeter: features must be callable, got {type(features).__name__}")
        self.features = features
        self.name = str(getattr(features, "name", None) or getattr(features, "__name__", type(features).__name__))
        self._capacity = [max(1, int(capacity))] * 2
        self._bank = [None, None]                      # [capacity, d] fp32: predictions, references
        self._n = [0, 0]

    def _append(self, which: int, images01: torch.Tensor, name: str) -> None:
        img = _image_batch(images01, name)
        N = int(img.shape[0])
        f = self.features(img)
        if not torch.is_tensor(f) or not f.is_cuda or f.dim() != 2 or int(f.shape[0]) != N or f.device != img.device:
            raise RuntimeError(f"DistributionMeter: the feature extractor must return [N, d] device tensors; got "
                               f"{tuple(f.shape) if torch.is_tensor(f) else type(f).__name__} for {N} images")
        d = int(f.shape[1])
        other = self._bank[1 - which]
        if other is not None and (int(other.shape[1]) != d or other.device != f.device):
            raise RuntimeError(f"DistributionMeter: features of width {d} on {f.device}; the other set holds width "
                               f"{int(other.shape[1])} on {other.device}")
        bank, n = self._bank[which], self._n[which]
        if bank is not None and (int(bank.shape[1]) != d or bank.device != f.device):
            raise RuntimeError(f"DistributionMeter: features of width {d} on {f.device}; the bank holds width {int(bank.shape[1])} on "
                               f"{bank.device}")
        if bank is None or n + N > self._capacity[which]:
            while self._capacity[which] < n + N:
                self._capacity[which] *= 2
            grown = torch.empty(self._capacity[which], d, dtype=torch.float32, device=f.device)
            if bank is not None:
                grown[:n].copy_(bank[:n])
            self._bank[which] = bank = grown
        bank[n:n + N].copy_(f.detach())
        self._n[which] = n + N

    def update(self, pred01: torch.Tensor, target01: Optional[torch.Tensor] = None) -> None:
        self._append(0, pred01, "pred01")
        if target01 is not None:
            self._append(1, target01, "target01")

    def add_reference(self, images01: torch.Tensor) -> None:
        self._append(1, images01, "images01")

    def compute(self) -> Dict[str, object]:
        n, m = self._n
        res: Dict[str, object] = {"n_pred": int(n), "n_ref": int(m), "fd": float("nan"), "kid": float("nan"), "features": self.name}
        if n < 1 or m < 1:
            return res
        a, b = self._bank[0][:n], self._bank[1][:m]
        _, mean_a, cov_a = moments(a)
        _, mean_b, cov_b = moments(b)
        sums = kid_sums(a, b).cpu().numpy()
        fd = frechet_from_moments(mean_a, cov_a, mean_b, cov_b)        # NaN moments (a non-finite feature, a bank of one row) -> NaN
        if np.isfinite(sums).all() and np.isfinite(fd):
            res["fd"], res["kid"] = fd, _kid_from_sums(sums, n, m)
        return res


# ----------------------------------------------------------------------------------------------------------------------
# NIQE: the no-reference score (csrc/niqe.hip; tests/_niqe_def.py is the definition)
# ----------------------------------------------------------------------------------------------------------------------
def _niqe_patch(patch) -> int:
    if isinstance(patch, bool) or int(patch) != patch or int(patch) % 2 or not 8 <= int(patch) <= 512:
        raise ValueError(f"niqe: patch = {patch!r}; the block side must be an even integer between 8 and 512")
    return int(patch)


def _niqe_blocks(H: int, W: int, patch: int) -> int:
    """Whole blocks of ``patch`` x ``patch`` in an image of H x W; refuses an image that holds none."""
    if H < patch or W < patch:
        raise ValueError(f"niqe: an image of {H} x {W} holds no block of patch = {patch}; both sides must be at least patch")
    if H > 16384 or W > 16384:
        raise ValueError(f"niqe: an image of {H} x {W}; sides of at most 16384")
    return (H // patch) * (W // patch)


def _niqe_features_checked(img: torch.Tensor, patch: int, quantize: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    N, _, H, W = (int(v) for v in img.shape)
    P = _niqe_blocks(H, W, patch)
    lib = _capi.lib()
    need = C.c_int64(0)
    _capi.check(lib.hdiff_niqe_workspace(N, H, W, patch, C.byref(need)), "niqe_workspace")
    with torch.cuda.device(img.device):
        feats = torch.empty(N, P, NIQE_ROW, dtype=torch.float64, device=img.device)
        sharp = torch.empty(N, P, dtype=torch.float64, device=img.device)
        scratch = torch.empty(need.value, dtype=torch.uint8, device=img.device)
        _capi.check(lib.hdiff_niqe_features(img.data_ptr(), N, H, W, patch, int(bool(quantize)), feats.data_ptr(), sharp.data_ptr(),
                                            scratch.data_ptr(), _stream(img.device)), "niqe_features")
    return feats, sharp


def _niqe_moments_into(feats: torch.Tensor, sharp: torch.Tensor, threshold: float, out: torch.Tensor) -> None:
    """``out``: a contiguous ``[N, NIQE_MOMENTS]`` float64 slice on the features' device."""
    N, P = int(feats.shape[0]), int(feats.shape[1])
    with torch.cuda.device(feats.device):
        _capi.check(_capi.lib().hdiff_niqe_moments(feats.data_ptr(), sharp.data_ptr(), N, P, float(threshold), out.data_ptr(),
                                                   _stream(feats.device)), "niqe_moments")


def niqe_features(img01: torch.Tensor, *, patch: int = 96, quantize: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (feats ``[N, P, 36]``, sharp ``[N, P]``), float64 device tensors; never synchronises.  ``P`` is the number of whole
    ``patch`` x ``patch`` blocks of the image, counted from its top-left corner (``patch`` even, 8 to 512; both sides at least
    ``patch``).  A row holds the 18 AGGD features of a block of the contrast-normalised gray plane and the 18 of its counterpart on the
    plane reduced by two; ``sharp`` is the mean local deviation of the block.  ``quantize`` rounds channels and gray to 8-bit values
    first, as a written file holds them.  A block over a constant area has non-finite features; an image with a NaN pixel has NaN
    everywhere."""
    patch = _niqe_patch(patch)
    return _niqe_features_checked(_image_batch(img01, "img01"), patch, quantize)


class NIQEModel:
    """The "pristine" model NIQE measures against: the mean ``[36]`` and covariance ``[36, 36]`` of the rows of sharp blocks of clean
    images, with the ``patch`` and ``quantize`` they were taken at (host float64).  None ships and none is fetched: ``fit`` one on the
    targets of a paired set, or ``load`` the parameters of the authors' release (agreement with that release is unpinned)."""

    def __init__(self, mean, cov, *, patch: int = 96, quantize: bool = True):
        self.patch, self.quantize = _niqe_patch(patch), bool(quantize)
        self.mean = np.ascontiguousarray(_host64(mean).reshape(-1))
        self.cov = np.ascontiguousarray(_host64(cov))
        if self.mean.shape != (NIQE_ROW,) or self.cov.shape != (NIQE_ROW, NIQE_ROW):
            raise ValueError(f"NIQEModel: mean of shape {_host64(mean).shape} and cov of shape {self.cov.shape}; [36] and [36, 36]")
        if not (np.isfinite(self.mean).all() and np.isfinite(self.cov).all()):
            raise ValueError("NIQEModel: the mean and the covariance must be finite")

    def save(self, path: str) -> None:
        """Writes an ``.npz`` with ``mean``, ``cov``, ``patch`` and ``quantize`` (to ``path`` as given: no suffix is appended)."""
        with open(path, "wb") as f:
            np.savez(f, mean=self.mean, cov=self.cov, patch=np.int64(self.patch), quantize=np.bool_(self.quantize))

    @classmethod
    def load(cls, path: str, *, patch: Optional[int] = None) -> "NIQEModel":
        """An ``.npz`` written by ``save``, or a ``.mat`` holding ``mu_prisparam`` / ``cov_prisparam`` (the release's file, read with
        ``scipy.io.loadmat``; those were taken at ``patch=96`` on 8-bit images).  ``patch``: the block side the caller is going to
        use; a file that holds another one raises ``ValueError``."""
        if str(path).lower().endswith(".mat"):
            from scipy.io import loadmat
            held = loadmat(str(path))
            missing = [k for k in ("mu_prisparam", "cov_prisparam") if k not in held]
            if missing:
                raise ValueError(f"NIQEModel.load: {path} lacks {missing}")
            model = cls(held["mu_prisparam"], held["cov_prisparam"], patch=96, quantize=True)
        else:
            with np.load(str(path)) as held:
                missing = [k for k in ("mean", "cov", "patch") if k not in held.files]
                if missing:
                    raise ValueError(f"NIQEModel.load: {path} lacks {missing}")
                model = cls(held["mean"], held["cov"], patch=int(held["patch"]),
                            quantize=bool(held["quantize"]) if "quantize" in held.files else True)
        if patch is not None and int(patch) != model.patch:
            raise ValueError(f"NIQEModel.load: {path} was fitted at patch = {model.patch}, not at patch = {patch}")
        return model

    @classmethod
    def fit(cls, batches, *, patch: int = 96, sharp_threshold: float = 0.75, quantize: bool = True) -> "NIQEModel":
        """Fits the model on ``batches``: an iterable of ``[N, 3, H, W]`` (or ``[3, H, W]``) device images in [0, 1], of any sizes.  From
        each image the finite rows whose ``sharp`` exceeds ``sharp_threshold * max(sharp of that image)`` are kept
        (``hdiff_niqe_keep``); rows and selection stay in a device bank that doubles as it fills, and the mean and unbiased covariance
        of the kept rows are taken by ``hdiff_niqe_pool_moments`` in bank order, so the result does not depend on how the set was cut
        into batches.  Nothing synchronises before the one copy of the result.  Fewer than two kept rows raise ``ValueError``."""
        patch = _niqe_patch(patch)
        if not 0.0 <= float(sharp_threshold) < 1.0:
            raise ValueError(f"NIQEModel.fit: sharp_threshold = {sharp_threshold!r}; in [0, 1)")
        if torch.is_tensor(batches):
            batches = [batches]
        lib = _capi.lib()
        bank = keep = None
        n = 0
        for batch in batches:
            if torch.is_tensor(batch) and batch.dim() == 3:
                batch = batch.unsqueeze(0)
            img = _image_batch(batch, "batches")
            feats, sharp = _niqe_features_checked(img, patch, quantize)
            N, P = int(feats.shape[0]), int(feats.shape[1])
            dev = img.device
            if bank is not None and bank.device != dev:
                raise RuntimeError(f"hdiff: NIQEModel.fit holds rows on {bank.device}, a batch is on {dev}")
            if bank is None or n + N * P > int(bank.shape[0]):
                capacity = 1024 if bank is None else int(bank.shape[0])
                while capacity < n + N * P:
                    capacity *= 2
                grown, grown_keep = (torch.empty(capacity, NIQE_ROW, dtype=torch.float64, device=dev),
                                     torch.empty(capacity, dtype=torch.int32, device=dev))
                if bank is not None:
                    grown[:n].copy_(bank[:n])
                    grown_keep[:n].copy_(keep[:n])
                bank, keep = grown, grown_keep
            bank[n:n + N * P].copy_(feats.view(N * P, NIQE_ROW))
            with torch.cuda.device(dev):
                _capi.check(lib.hdiff_niqe_keep(feats.data_ptr(), sharp.data_ptr(), N, P, float(sharp_threshold),
                                                keep[n:n + N * P].data_ptr(), _stream(dev)), "niqe_keep")
            n += N * P
        if bank is None:
            raise ValueError("NIQEModel.fit: no images")
        out = torch.empty(NIQE_MOMENTS, dtype=torch.float64, device=bank.device)
        with torch.cuda.device(bank.device):
            _capi.check(lib.hdiff_niqe_pool_moments(bank.data_ptr(), keep.data_ptr(), n, out.data_ptr(), _stream(bank.device)),
                        "niqe_pool_moments")
        host = out.cpu().numpy()
        if host[-1] < 2:
            raise ValueError(f"NIQEModel.fit: {int(host[-1])} of {n} rows are finite and sharp enough; at least two are needed")
        return cls(host[:NIQE_ROW], host[NIQE_ROW:-1].reshape(NIQE_ROW, NIQE_ROW), patch=patch, quantize=quantize)


def niqe_from_moments(model: NIQEModel, mean, cov, count: Optional[float] = None) -> float:
    """``sqrt(d . pinv((cov_pris + cov) / 2) . d)`` with ``d = mu_pris - mean``, on the host in float64;
    ``numpy.linalg.pinv(hermitian=True)`` at its default cutoff (the release's ``pinv`` uses MATLAB's tolerance).  NaN where the
    image's moments are undefined: a non-finite entry (the kernel's covariance of fewer than two rows is NaN) or ``count`` < 2."""
    if not isinstance(model, NIQEModel):
        raise TypeError(f"niqe: model must be a quality.NIQEModel, got {type(model).__name__}")
    m, c = _host64(mean).reshape(-1), _host64(cov)
    if m.shape != (NIQE_ROW,) or c.shape != (NIQE_ROW, NIQE_ROW):
        raise ValueError(f"niqe_from_moments: mean of shape {m.shape} and cov of shape {c.shape}; [36] and [36, 36]")
    if (count is not None and count < 2) or not (np.isfinite(m).all() and np.isfinite(c).all()):
        return float("nan")
    d = model.mean - m
    return float(np.sqrt(d @ np.linalg.pinv((model.cov + c) / 2.0, hermitian=True) @ d))


def _niqe_scores(model: NIQEModel, rows: np.ndarray) -> np.ndarray:
    """``[n, NIQE_MOMENTS]`` host rows -> ``[n]`` scores."""
    return np.array([niqe_from_moments(model, r[:NIQE_ROW], r[NIQE_ROW:-1].reshape(NIQE_ROW, NIQE_ROW), r[-1]) for r in rows],
                    dtype=np.float64).reshape(-1)


def niqe(img01: torch.Tensor, model: NIQEModel) -> torch.Tensor:
    """-> float64 ``[N]`` on the images' device: the NIQE of each image against ``model``, at the model's ``patch`` and ``quantize``;
    lower is better.  The features and the per-image moments of the finite rows are taken on the device; then ONE copy of the
    ``N x 1333`` doubles and the finish on the host (``niqe_from_moments``): this call SYNCHRONISES once.  NaN for an image with fewer
    than two finite rows or with a NaN pixel."""
    if not isinstance(model, NIQEModel):
        raise TypeError(f"niqe: model must be a quality.NIQEModel, got {type(model).__name__}")
    img = _image_batch(img01, "img01")
    feats, sharp = _niqe_features_checked(img, model.patch, model.quantize)
    out = torch.empty(int(img.shape[0]), NIQE_MOMENTS, dtype=torch.float64, device=img.device)
    _niqe_moments_into(feats, sharp, 0.0, out)
    return torch.from_numpy(_niqe_scores(model, out.cpu().numpy())).to(img.device)
