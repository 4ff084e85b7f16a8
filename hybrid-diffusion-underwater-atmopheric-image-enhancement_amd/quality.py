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
and do not depend on the batch an image is scored in.  The other parts of ``nmetrics`` (its own UIQM variant) and the 8-bit OpenCV
``uw_metrics.uciqe``, which the reference never calls, stay on the host.  There is no CPU fallback: CPU tensors are refused.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _capi
from . import engine as E

__all__ = ["psnr_ssim", "uiqm", "uciqe", "QualityMeter"]

COLUMNS = ("psnr", "ssim", "uiqm", "uicm", "uism", "uiconm")      # the columns of QualityMeter's per-image rows
UCIQE_COLUMNS = ("uciqe", "uciqe_sc", "uciqe_conl", "uciqe_us")   # the four more of QualityMeter(uciqe=True)


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


class QualityMeter:
    """Accumulates per-image scores on the device: ``update`` per batch (never synchronises), ``compute`` once at the end (one copy).

    Rows are ``COLUMNS`` = (psnr, ssim, uiqm, uicm, uism, uiconm); psnr / ssim are NaN for the images of an ``update`` without a
    target, and the means of those two are taken over the images that had one.  With ``uciqe=True`` every row gains
    ``UCIQE_COLUMNS`` = (uciqe, uciqe_sc, uciqe_conl, uciqe_us) of ``clip(pred, 0, 1) * uciqe_scale`` (``quality.uciqe``); without it
    the rows, the launches and ``compute``'s dict are those of the six columns alone."""

    def __init__(self, capacity: int = 64, *, uciqe: bool = False, uciqe_scale: float = 1.0):
        self._capacity = max(1, int(capacity))
        self._uciqe, self._uciqe_scale = bool(uciqe), float(uciqe_scale)
        self.columns = COLUMNS + UCIQE_COLUMNS if self._uciqe else COLUMNS
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
        self._updates.append((self._n, N, target is not None))
        self._n += N

    def compute(self) -> Dict[str, object]:
        """{"n", "psnr", "ssim", "uiqm", "uicm", "uism", "uiconm"} as float means over the images (an infinite PSNR makes the mean
        infinite, as the reference's ``sum(list) / len(list)`` does) and "per_image", the ``[n, 6]`` float64 rows; with ``uciqe=True``
        also the means of ``UCIQE_COLUMNS``, and "per_image" is ``[n, 10]``."""
        per = np.empty((0, len(self.columns))) if self._rows is None else self._rows[:self._n].cpu().numpy()
        paired = np.zeros(self._n, dtype=bool)
        for start, count, has_target in self._updates:
            paired[start:start + count] = has_target
        res: Dict[str, object] = {"n": int(self._n)}
        for j, k in enumerate(self.columns):
            col = per[paired, j] if k in ("psnr", "ssim") else per[:, j]
            res[k] = float(np.sum(col) / col.size) if col.size else float("nan")
        res["per_image"] = per
        return res
