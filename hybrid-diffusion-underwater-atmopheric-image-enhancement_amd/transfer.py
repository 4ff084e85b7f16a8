"""Guided full-resolution transfer (``csrc/transfer.hip``): let the model decide what the enhancement IS at its own 256 x 256 and carry
that decision to the file at its own size.  Per pixel neighbourhood of the small pair (degraded, enhanced) the affine colour map that
takes one to the other is fitted -- He et al.'s guided filter with a colour guide, in its "fast" form -- and the smoothly upsampled map
is applied to the full-size original: detail comes from the original; colour, contrast and haze removal come from the diffusion sample.
The cost is one model-sized sampling run plus one pass over the large image.

    from hdiff_amd import transfer
    enhance = transfer.GuidedEnhancer(sampler, ddim_step=20)
    out_u8 = enhance(img_u8)                      # uint8 [H, W, 3] on the device, in and out

or by hand: ``low = resample(img, 256)``, ``coef = guided_fit(low[None] / 255, pred01)``, ``guided_apply(coef[0], img)``.

What is NOT pinned.  The defaults ``radius=8``, ``eps=1e-3`` are the usual range of the guided-filter literature for a 256-pixel grid;
no image-quality figure backs them (there are no trained weights here), nor any other claim about how the output looks.  By design the
diffusion sample's own fine texture does not survive the fit: within a window the output is an affine function of the original's
colours, so only what the original holds at that scale can appear.  ``resample`` agrees with Pillow's ``BILINEAR`` resize to within one
8-bit level (it skips Pillow's 8-bit rounding between the passes), not beyond.

Everything runs on the current stream, allocates through torch's caching allocator and never synchronises; there is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Tuple, Union

import torch

from . import _capi
from . import engine as E

__all__ = ["resample", "guided_fit", "guided_apply", "GuidedEnhancer", "transfer_settings"]

MAX_SIDE, MAX_SMALL_SIDE, MAX_RADIUS = 16384, 4096, 128


def _stream(dev) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def _size_pair(size) -> Tuple[int, int]:
    if isinstance(size, bool) or not isinstance(size, (int, tuple, list)):
        raise TypeError(f"hdiff: 'size' must be an int or an (h, w) pair, got {size!r}")
    pair = (size, size) if isinstance(size, int) else tuple(size)
    if len(pair) != 2 or any(isinstance(v, bool) or not isinstance(v, int) for v in pair):
        raise TypeError(f"hdiff: 'size' must be an int or an (h, w) pair of ints, got {size!r}")
    if not all(1 <= v <= MAX_SMALL_SIDE for v in pair):
        raise ValueError(f"hdiff: 'size' = {size!r}; each side must be between 1 and {MAX_SMALL_SIDE}")
    return int(pair[0]), int(pair[1])


def transfer_settings(radius, eps) -> Tuple[int, float]:
    """``(radius, eps)`` checked: an int in [1, 128] and a finite positive float."""
    if isinstance(radius, bool) or not isinstance(radius, int):
        raise TypeError(f"hdiff: 'radius' must be an int, got {radius!r}")
    if not 1 <= radius <= MAX_RADIUS:
        raise ValueError(f"hdiff: 'radius' = {radius}; it must be between 1 and {MAX_RADIUS}")
    if isinstance(eps, bool) or not isinstance(eps, (int, float)):
        raise TypeError(f"hdiff: 'eps' must be a number, got {eps!r}")
    eps = float(eps)
    if not (math.isfinite(eps) and eps > 0.0):
        raise ValueError(f"hdiff: 'eps' = {eps!r}; it must be finite and positive")
    return radius, eps


def _image_u8(t, name: str) -> torch.Tensor:
    if not torch.is_tensor(t):
        raise TypeError(f"hdiff: '{name}' must be a tensor, got {type(t).__name__}")
    if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
        raise ValueError(f"hdiff: '{name}' has dtype {t.dtype} and shape {tuple(t.shape)}; it must be a uint8 [H, W, 3] image")
    H, W = int(t.shape[0]), int(t.shape[1])
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f"hdiff: '{name}' is {H} x {W}; each side must be between 1 and {MAX_SIDE}")
    if not t.is_cuda:
        raise RuntimeError(f"hdiff: '{name}' lives on {t.device}; the HIP path needs an MI355X device tensor "
                           "(there is deliberately no CPU fallback)")
    return t if t.is_contiguous() else t.contiguous()


def _planes_f32(t, name: str, channels: int, dims: int) -> torch.Tensor:
    if not torch.is_tensor(t):
        raise TypeError(f"hdiff: '{name}' must be a tensor, got {type(t).__name__}")
    if not t.is_floating_point() or t.dim() != dims or t.shape[dims - 3] != channels:
        lead = "N, " if dims == 4 else ""
        raise ValueError(f"hdiff: '{name}' has dtype {t.dtype} and shape {tuple(t.shape)}; it must be a float [{lead}{channels}, H, W] "
                         "tensor")
    if t.is_cuda:
        if t.dtype != torch.float32:
            t = t.float()
        if not t.is_contiguous():
            t = t.contiguous()
    E.require_gpu_tensor(t, name)
    return t


def _same_device(a: torch.Tensor, b: torch.Tensor, name_a: str, name_b: str) -> None:
    if a.device != b.device:
        raise ValueError(f"hdiff: '{name_a}' lives on {a.device} and '{name_b}' on {b.device}; both must be on one device")


def _resample_scratch(H: int, W: int, h: int, w: int, dev) -> torch.Tensor:
    need = C.c_int64(0)
    _capi.check(_capi.lib().hdiff_resample_workspace(H, W, h, w, C.byref(need)), "resample_workspace")
    return torch.empty(need.value, dtype=torch.uint8, device=dev)


def _fit_scratch(N: int, h: int, w: int, dev) -> torch.Tensor:
    need = C.c_int64(0)
    _capi.check(_capi.lib().hdiff_guided_workspace(N, h, w, C.byref(need)), "guided_workspace")
    return torch.empty(need.value, dtype=torch.uint8, device=dev)


def _resample_into(img: torch.Tensor, out: torch.Tensor, scratch: torch.Tensor) -> None:
    _capi.check(_capi.lib().hdiff_resample_u8(img.data_ptr(), int(img.shape[0]), int(img.shape[1]), out.data_ptr(), int(out.shape[1]),
                                              int(out.shape[2]), scratch.data_ptr(), _stream(img.device)), "resample_u8")


def _fit_into(I: torch.Tensor, p: torch.Tensor, radius: int, eps: float, coef: torch.Tensor, scratch: torch.Tensor) -> None:
    N, _, h, w = (int(v) for v in I.shape)
    _capi.check(_capi.lib().hdiff_guided_fit(I.data_ptr(), p.data_ptr(), N, h, w, radius, eps, coef.data_ptr(), scratch.data_ptr(),
                                             _stream(I.device)), "guided_fit")


def _apply_u8_into(coef: torch.Tensor, full: torch.Tensor, out: torch.Tensor) -> None:
    _capi.check(_capi.lib().hdiff_guided_apply_u8(coef.data_ptr(), int(coef.shape[1]), int(coef.shape[2]), full.data_ptr(), out.data_ptr(),
                                                  int(full.shape[0]), int(full.shape[1]), _stream(full.device)), "guided_apply_u8")


def resample(image_u8_hwc: torch.Tensor, size: Union[int, Tuple[int, int]]) -> torch.Tensor:
    """uint8 ``[H, W, 3]`` -> float ``[3, h, w]`` in [0, 255]: the triangle filter of Pillow's ``BILINEAR`` resize (support
    ``max(in / out, 1)`` per axis, horizontal pass first), in double with one rounding; within one 8-bit level of Pillow."""
    h, w = _size_pair(size)
    img = _image_u8(image_u8_hwc, "image_u8_hwc")
    out = torch.empty(3, h, w, dtype=torch.float32, device=img.device)
    with torch.cuda.device(img.device):
        _resample_into(img, out, _resample_scratch(int(img.shape[0]), int(img.shape[1]), h, w, img.device))
    return out


def guided_fit(low_in01: torch.Tensor, low_out01: torch.Tensor, *, radius: int = 8, eps: float = 1e-3) -> torch.Tensor:
    """``low_in01`` (guide), ``low_out01`` (target): float ``[N, 3, h, w]`` in [0, 1] units -> ``coef`` float ``[N, 12, h, w]``: per pixel
    the 3 x 3 matrix (planes 0-8, row by row) and offset (planes 9-11) of the ridge-regularised affine map fitted over the clipped
    ``(2 radius + 1)^2`` window and averaged over the same window (module docstring: the defaults are unpinned)."""
    radius, eps = transfer_settings(radius, eps)
    if torch.is_tensor(low_in01) and torch.is_tensor(low_out01) and low_in01.shape != low_out01.shape:
        raise ValueError(f"hdiff: guide {tuple(low_in01.shape)} and target {tuple(low_out01.shape)} must have the same shape")
    I, p = _planes_f32(low_in01, "low_in01", 3, 4), _planes_f32(low_out01, "low_out01", 3, 4)
    _same_device(I, p, "low_in01", "low_out01")
    N, _, h, w = (int(v) for v in I.shape)
    coef = torch.empty(N, 12, h, w, dtype=torch.float32, device=I.device)
    with torch.cuda.device(I.device):
        _fit_into(I, p, radius, eps, coef, _fit_scratch(N, h, w, I.device))
    return coef


def guided_apply(coef: torch.Tensor, full: torch.Tensor, *, clamp: bool = True) -> torch.Tensor:
    """The map at the image's own size.  ``full`` uint8 ``[H, W, 3]`` with ``coef`` ``[12, h, w]``: -> uint8 ``[H, W, 3]``,
    ``rint(255 clamp(q, 0, 1))``.  ``full`` float ``[N, 3, H, W]`` in [0, 1] units with ``coef`` ``[N, 12, h, w]``: -> float
    ``[N, 3, H, W]``, clamped to [0, 1] unless ``clamp=False``."""
    if not torch.is_tensor(full):
        raise TypeError(f"hdiff: 'full' must be a tensor, got {type(full).__name__}")
    if full.dtype == torch.uint8:
        if not clamp:
            raise ValueError("hdiff: a uint8 image is always clamped; clamp=False needs a float image")
        c = _planes_f32(coef, "coef", 12, 3)
        img = _image_u8(full, "full")
        _same_device(c, img, "coef", "full")
        out = torch.empty_like(img)
        with torch.cuda.device(img.device):
            _apply_u8_into(c, img, out)
        return out
    c = _planes_f32(coef, "coef", 12, 4)
    img = _planes_f32(full, "full", 3, 4)
    if img.shape[0] != c.shape[0]:
        raise ValueError(f"hdiff: 'coef' holds {c.shape[0]} images, 'full' {img.shape[0]}")
    _same_device(c, img, "coef", "full")
    N, _, H, W = (int(v) for v in img.shape)
    out = torch.empty_like(img)
    with torch.cuda.device(img.device):
        _capi.check(_capi.lib().hdiff_guided_apply_f32(c.data_ptr(), int(c.shape[2]), int(c.shape[3]), img.data_ptr(), out.data_ptr(), N, H,
                                                       W, int(bool(clamp)), _stream(img.device)), "guided_apply_f32")
    return out


class GuidedEnhancer:
    """``enhance(img)``: one uint8 ``[H, W, 3]`` device image -> the enhanced uint8 ``[H, W, 3]``.

      1. ``low = resample(img, size)``
      2. ``out = sampler(low[None], ddim=True, **sampler_kwargs)`` (``ddim_step``, ``solver``, ``spacing``, ``y_T`` pass through); with
         ``samples=K``: ``out = sampler.posterior(low[None], K, eta=eta, seed=seed, **sampler_kwargs).mean``, the mean of K samples --
         the better target for a fit that discards a sample's own texture anyway (``sample_batch`` passes through)
      3. ``pred01 = clamp((out + 1) / 2, 0, 1)``
      4. ``coef = guided_fit(low[None] / 255, pred01, radius=radius, eps=eps)``
      5. ``guided_apply(coef[0], img)``

    Workspaces are cached per shape; the call synchronises only where the sampler does.  ``radius=8``, ``eps=1e-3`` are the usual range
    of the guided-filter literature for a 256-pixel grid and NO image-quality figure backs them; the diffusion sample's own fine texture
    does not survive the fit, by design (module docstring)."""

    def __init__(self, sampler, *, size: Union[int, Tuple[int, int]] = 256, radius: int = 8, eps: float = 1e-3,
                 samples: Optional[int] = None, eta: float = 0.0, seed: int = 0, **sampler_kwargs):
        if not callable(sampler):
            raise TypeError("hdiff: GuidedEnhancer needs a callable sampler")
        if samples is None and eta != 0:
            raise ValueError("hdiff: GuidedEnhancer: eta= goes with samples=")
        if samples is not None:
            if isinstance(samples, bool) or not isinstance(samples, int) or samples < 1:
                raise ValueError(f"hdiff: GuidedEnhancer: samples must be an integer >= 1, got {samples!r}")
            if not hasattr(sampler, "posterior"):
                raise TypeError("hdiff: GuidedEnhancer(samples=) needs a sampler with a posterior() method")
        self.samples, self.eta, self.seed = samples, eta, seed
        self.sampler = sampler
        self.size = _size_pair(size)
        self.radius, self.eps = transfer_settings(radius, eps)
        self.sampler_kwargs = dict(sampler_kwargs)
        self._resample_ws: Dict[tuple, torch.Tensor] = {}
        self._fit_ws: Dict[tuple, torch.Tensor] = {}

    def __call__(self, image_u8_hwc: torch.Tensor) -> torch.Tensor:
        img = _image_u8(image_u8_hwc, "image_u8_hwc")
        h, w = self.size
        H, W, dev = int(img.shape[0]), int(img.shape[1]), img.device
        with torch.cuda.device(dev), torch.no_grad():
            key = (H, W, dev)
            if key not in self._resample_ws:
                self._resample_ws[key] = _resample_scratch(H, W, h, w, dev)
            if dev not in self._fit_ws:
                self._fit_ws[dev] = _fit_scratch(1, h, w, dev)
            low = torch.empty(3, h, w, dtype=torch.float32, device=dev)
            _resample_into(img, low, self._resample_ws[key])
            if self.samples is None:
                out = self.sampler(low[None], ddim=True, **self.sampler_kwargs)
            else:
                out = self.sampler.posterior(low[None], self.samples, eta=self.eta, seed=self.seed, **self.sampler_kwargs).mean
            pred01 = ((out + 1) / 2).clamp(0, 1)
            if pred01.shape != (1, 3, h, w) or pred01.device != dev:
                raise RuntimeError(f"hdiff: the sampler returned {tuple(out.shape)} on {out.device} for a (1, 3, {h}, {w}) input on {dev}")
            coef = torch.empty(1, 12, h, w, dtype=torch.float32, device=dev)
            _fit_into(low[None] / 255, pred01.float().contiguous(), self.radius, self.eps, coef, self._fit_ws[dev])
            result = torch.empty_like(img)
            _apply_u8_into(coef[0], img, result)
        return result
