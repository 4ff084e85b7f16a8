"""PSNR / SSIM / UIQM (``csrc/quality.hip``) and UCIQE (``csrc/uciqe.hip``) on the device: the per-image scores of the reference's
evaluation (``utils/rotinas.py:916-931``) taken where the sampler leaves its output, without a copy to the host per batch.

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

A non-finite input value makes the scores of its image NaN and leaves the rest of the batch alone.  Results are bitwise repeatable
and do not depend on the batch an image is scored in.

``LPIPS(vgg, lin)`` is the LPIPS v0.1 VGG distance between two images (Zhang et al., "The Unreasonable Effectiveness of Deep Features
as a Perceptual Metric"): the VGG16 trunk of ``hdiff_amd.perceptual`` tapped behind its five conv blocks, and per layer the mean over
the pixels of the weighted squared difference of the channel-normalised features (``hdiff_lpips_layer``, in double).  The weights come
from the caller -- a torchvision ``vgg16`` state dict and the five ``lin`` layers of the ``lpips`` package; none ship, none are fetched.
Scaling constants, taps and formula were written from memory of that package: agreement with it is unpinned.  The other parts of ``nmetrics`` (its own UIQM variant) and the 8-bit OpenCV
``uw_metrics.uciqe``, which the reference never calls, stay on the host.  There is no CPU fallback: CPU tensors are refused.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _capi
from . import engine as E

__all__ = ["psnr_ssim", "uiqm", "uciqe", "LPIPS", "QualityMeter"]

COLUMNS = ("psnr", "ssim", "uiqm", "uicm", "uism", "uiconm")      # the columns of QualityMeter's per-image rows
UCIQE_COLUMNS = ("uciqe", "uciqe_sc", "uciqe_conl", "uciqe_us")   # the four more of QualityMeter(uciqe=True)
LPIPS_COLUMNS = ("lpips",)                                        # the last one of QualityMeter(lpips=metric)


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
    the rows, the launches and ``compute``'s dict are those of the six columns alone.  With ``lpips=metric`` (an ``LPIPS``) every row
    gains ``LPIPS_COLUMNS`` = (lpips,) as its LAST column, behind UCIQE's where both are on: the distance of the prediction from its
    target, NaN for the images of an ``update`` without one, and its mean is taken like PSNR's."""

    def __init__(self, capacity: int = 64, *, uciqe: bool = False, uciqe_scale: float = 1.0, lpips: Optional[LPIPS] = None):
        self._capacity = max(1, int(capacity))
        self._uciqe, self._uciqe_scale = bool(uciqe), float(uciqe_scale)
        if lpips is not None and not isinstance(lpips, LPIPS):
            raise TypeError(f"QualityMeter: lpips must be a quality.LPIPS, got {type(lpips).__name__}")
        self._lpips = lpips
        self.columns = COLUMNS + UCIQE_COLUMNS if self._uciqe else COLUMNS
        if lpips is not None:
            self.columns = self.columns + LPIPS_COLUMNS
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
            return
        if self._rows.device != dev:
            raise RuntimeError(f"hdiff: QualityMeter holds rows on {self._rows.device}, the update is on {dev}")
        if self._n + extra > self._capacity:
            while self._capacity < self._n + extra:
                self._capacity *= 2
            grown = torch.empty(self._capacity, len(self.columns), dtype=torch.float64, device=dev)
            grown[:self._n].copy_(self._rows[:self._n])
            self._rows = grown

    def update(self, pred01: torch.Tensor, target01: Optional[torch.Tensor] = None) -> None:
        pred = _image_batch(pred01, "pred01")
        target = None if target01 is None else _image_batch(target01, "target01")
        if target is not None and (pred.shape != target.shape or pred.device != target.device):
            raise ValueError("Input images must have the same dimensions.")
        if self._lpips is not None and target is not None:
            self._lpips._checked(pred, target)                    # a size LPIPS cannot take is refused before a row is written
        N, _, H, W = (int(v) for v in pred.shape)
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
            if self._lpips is not None:
                if target is not None:
                    dist = torch.empty(N, dtype=torch.float64, device=dev)
                    self._lpips._into(pred, target, dist)
                    rows[:, -1].copy_(dist)
                else:
                    rows[:, -1].fill_(float("nan"))
        self._updates.append((self._n, N, target is not None))
        self._n += N

    def compute(self) -> Dict[str, object]:
        """{"n", "psnr", "ssim", "uiqm", "uicm", "uism", "uiconm"} as float means over the images (an infinite PSNR makes the mean
        infinite, as the reference's ``sum(list) / len(list)`` does) and "per_image", the ``[n, 6]`` float64 rows; with ``uciqe=True``
        also the means of ``UCIQE_COLUMNS``, and "per_image" is ``[n, 10]``; with ``lpips=`` also "lpips" (over the images that had a
        target) and one more column."""
        per = np.empty((0, len(self.columns))) if self._rows is None else self._rows[:self._n].cpu().numpy()
        paired = np.zeros(self._n, dtype=bool)
        for start, count, has_target in self._updates:
            paired[start:start + count] = has_target
        res: Dict[str, object] = {"n": int(self._n)}
        for j, k in enumerate(self.columns):
            col = per[paired, j] if k in ("psnr", "ssim", "lpips") else per[:, j]
            res[k] = float(np.sum(col) / col.size) if col.size else float("nan")
        res["per_image"] = per
        return res
