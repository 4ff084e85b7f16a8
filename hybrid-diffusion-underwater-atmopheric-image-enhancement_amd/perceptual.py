"""A VGG feature trunk on the HIP path, and the loss arithmetic that sits on its taps (``csrc/perceptual.hip``).

``VGGFeatures`` is torchvision's ``vgg11 / vgg13 / vgg16 / vgg19`` ``.features`` Sequential (no batch norm) with frozen weights:
its 3x3 convs run through ``autograd.fused_conv`` (the split-operand kernels in the default contraction mode, the exact fp32 kernel
in the other; the input gradient is the same kernels' dgrad route, and no weight gradient is ever launched), ReLU and 2x2
max-pooling are the kernels of ``csrc/perceptual.hip`` with their hand-written backward.  ``l1_mean`` and ``charbonnier`` are the two
reductions / maps the losses of ``Loss/loss.py`` are made of.  Nothing here runs in ATen but the sum of a handful of scalars.

No pretrained weights ship with the package and none are fetched: ``load_torchvision`` takes a torchvision state dict from the
caller.  The layer lists and the initialisation (Kaiming-normal, fan-out, ReLU gain; zero bias) are written from memory of
torchvision, which is not a dependency: agreement with torchvision itself is unpinned.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Iterable, List, Optional, Sequence

import torch
import torch.nn as nn
from torch.autograd import Function

from . import _capi
from . import engine as E

__all__ = ["VGG_CFGS", "VGGFeatures", "relu", "max_pool2", "l1_mean", "charbonnier"]

VGG_CFGS: Dict[str, List] = {
    "vgg11": [64, "M", 128, "M", 256, 256, "M", 512, 512, "M", 512, 512, "M"],
    "vgg13": [64, 64, "M", 128, 128, "M", 256, 256, "M", 512, 512, "M", 512, 512, "M"],
    "vgg16": [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"],
    "vgg19": [64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512, 512, 512, 512, "M"],
}


def _stream(dev) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def _fp32_gpu(t: torch.Tensor, name: str) -> torch.Tensor:
    if not torch.is_tensor(t):
        raise TypeError(f"hdiff: '{name}' must be a tensor, got {type(t).__name__}")
    t = E.gpu_input(t, name)
    if t.dtype != torch.float32:
        raise RuntimeError(f"hdiff: '{name}' has dtype {t.dtype}; the perceptual path computes in fp32")
    return t


def _pair(a: torch.Tensor, b: torch.Tensor, who: str):
    a, b = _fp32_gpu(a, "input"), _fp32_gpu(b, "target")
    if a.shape != b.shape or a.device != b.device:
        raise RuntimeError(f"{who}: input and target must have one shape and one device, got {tuple(a.shape)} on {a.device} and "
                           f"{tuple(b.shape)} on {b.device}")
    if a.numel() == 0:
        raise RuntimeError(f"{who}: empty tensors")
    return a, b


# ----------------------------------------------------------------------------------------------------------------------
# autograd functions on the kernels
# ----------------------------------------------------------------------------------------------------------------------
class _ReluFn(Function):
    @staticmethod
    def forward(ctx, x, inplace: bool):
        y = x if inplace else torch.empty_like(x)
        with torch.cuda.device(x.device):
            _capi.check(_capi.lib().hdiff_relu_fwd(x.data_ptr(), y.data_ptr(), x.numel(), _stream(x.device)), "relu_fwd")
        if inplace:
            ctx.mark_dirty(x)
        ctx.save_for_backward(y)            # the backward reads the OUTPUT: nothing of the input needs to survive
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(y)
        with torch.cuda.device(y.device):
            _capi.check(_capi.lib().hdiff_relu_bwd(y.data_ptr(), dy.data_ptr(), dx.data_ptr(), y.numel(), _stream(y.device)),
                        "relu_bwd")
        return dx, None


class _MaxPool2Fn(Function):
    @staticmethod
    def forward(ctx, x):
        B, Cc, H, W = (int(v) for v in x.shape)
        if H < 2 or W < 2:
            raise RuntimeError(f"max_pool2: the input is {H} x {W}; a 2x2 window needs at least 2 x 2 (Output size is too small)")
        y = torch.empty(B, Cc, H // 2, W // 2, device=x.device)
        with torch.cuda.device(x.device):
            _capi.check(_capi.lib().hdiff_maxpool2_fwd(x.data_ptr(), y.data_ptr(), B * Cc, H, W, _stream(x.device)), "maxpool2_fwd")
        ctx.save_for_backward(x)            # the choice is recomputed from the input: no index tensor
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        B, Cc, H, W = (int(v) for v in x.shape)
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _capi.check(_capi.lib().hdiff_maxpool2_bwd(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), B * Cc, H, W, _stream(x.device)),
                        "maxpool2_bwd")
        return dx


def _l1_mean_into(a: torch.Tensor, b: Optional[torch.Tensor], out: torch.Tensor) -> None:
    n = a.numel()
    need = C.c_int64(0)
    _capi.check(_capi.lib().hdiff_l1_mean_workspace(n, C.byref(need)), "l1_mean_workspace")
    ws = torch.empty(need.value, dtype=torch.uint8, device=a.device)
    _capi.check(_capi.lib().hdiff_l1_mean_fwd(a.data_ptr(), None if b is None else b.data_ptr(), n, out.data_ptr(), ws.data_ptr(),
                                              _stream(a.device)), "l1_mean_fwd")


class _L1MeanFn(Function):
    @staticmethod
    def forward(ctx, a, b):
        out = torch.empty((), device=a.device)
        with torch.cuda.device(a.device):
            _l1_mean_into(a, b, out)
        ctx.save_for_backward(a, b)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = g.contiguous()
        da = torch.empty_like(a)
        with torch.cuda.device(a.device):
            _capi.check(_capi.lib().hdiff_l1_mean_bwd(a.data_ptr(), b.data_ptr(), g.data_ptr(), a.numel(), da.data_ptr(),
                                                      _stream(a.device)), "l1_mean_bwd")
        return da, None


class _CharbonnierFn(Function):
    @staticmethod
    def forward(ctx, a, b, reduction: str):
        lib = _capi.lib()
        n = a.numel()
        with torch.cuda.device(a.device):
            s = _stream(a.device)
            y = torch.empty_like(a)
            _capi.check(lib.hdiff_charbonnier_fwd(a.data_ptr(), b.data_ptr(), y.data_ptr(), n, s), "charbonnier_fwd")
            if reduction != "none":
                # the map is non-negative: its mean is the L1 mean against nothing, in the same fixed order
                mean = torch.empty((), device=a.device)
                _l1_mean_into(y, None, mean)
                y = mean
                if reduction == "sum":
                    y = torch.empty((), device=a.device)
                    _capi.check(lib.hdiff_axpby(C.c_float(float(n)), mean.data_ptr(), C.c_float(0.0), None, y.data_ptr(), 1, s),
                                "axpby")
        ctx.reduction = reduction
        ctx.save_for_backward(a, b)
        return y

    @staticmethod
    def backward(ctx, dy):
        a, b = ctx.saved_tensors
        dy = dy.contiguous()
        n = a.numel()
        da = torch.empty_like(a)
        scalar = ctx.reduction != "none"
        with torch.cuda.device(a.device):
            _capi.check(_capi.lib().hdiff_charbonnier_bwd(a.data_ptr(), b.data_ptr(), dy.data_ptr(), 1 if scalar else 0,
                                                          C.c_float(float(n) if ctx.reduction == "mean" else 1.0), da.data_ptr(), n,
                                                          _stream(a.device)), "charbonnier_bwd")
        return da, None, None


def relu(x: torch.Tensor, inplace: bool = False) -> torch.Tensor:
    """``max(x, 0)`` (``hdiff_relu_fwd``); ``inplace=True`` overwrites ``x`` -- the backward needs the output alone."""
    return _ReluFn.apply(_fp32_gpu(x, "x"), bool(inplace))


def max_pool2(x: torch.Tensor) -> torch.Tensor:
    """``nn.MaxPool2d(kernel_size=2, stride=2)`` on ``[B, C, H, W]``: floor mode, a last odd row / column is dropped."""
    x = _fp32_gpu(x, "x")
    if x.dim() != 4:
        raise RuntimeError(f"max_pool2: expected [B, C, H, W], got {tuple(x.shape)}")
    return _MaxPool2Fn.apply(x)


def l1_mean(input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """``mean |input - target|`` as a 0-dim tensor (``F.l1_loss(..., reduction='mean')``): terms rounded to fp32, summed in double in a
    fixed order.  ``input`` is differentiated (``g * sign(input - target) / n``, ``sign(0) = 0``); ``target`` is a constant."""
    a, b = _pair(input, target, "l1_mean")
    return _L1MeanFn.apply(a, b.detach())


def charbonnier(input: torch.Tensor, target: torch.Tensor, reduction: str = "none") -> torch.Tensor:
    """``sqrt((input - target)^2 + 1) - 1`` elementwise ('none'), or its 'mean' / 'sum'.  ``input`` is differentiated; ``target`` is a
    constant."""
    if reduction not in ("none", "mean", "sum"):
        raise ValueError(f"Invalid reduction mode: {reduction}. Expected one of 'none', 'mean', 'sum'.")
    a, b = _pair(input, target, "charbonnier")
    return _CharbonnierFn.apply(a, b.detach(), reduction)


# ----------------------------------------------------------------------------------------------------------------------
# the trunk
# ----------------------------------------------------------------------------------------------------------------------
class _Conv3x3(nn.Module):
    """Holds ``weight [cout, cin, 3, 3]`` and ``bias [cout]`` under the Sequential index of the conv; frozen."""

    def __init__(self, cin: int, cout: int):
        super().__init__()
        w = torch.empty(cout, cin, 3, 3)
        nn.init.normal_(w, 0.0, math.sqrt(2.0 / (cout * 9)))          # kaiming_normal_(mode="fan_out", nonlinearity="relu")
        self.weight = nn.Parameter(w, requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(cout), requires_grad=False)


def _layers_of(cfg: Sequence) -> List:
    """The Sequential as a list: ("conv", cin, cout) / ("relu",) / ("pool",) at its index."""
    layers, cin = [], 3
    for v in cfg:
        if v == "M":
            layers.append(("pool",))
        else:
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"VGGFeatures: a layer list holds channel counts and 'M', got {v!r}")
            layers += [("conv", cin, int(v)), ("relu",)]
            cin = int(v)
    if not layers or layers[0][0] != "conv":
        raise ValueError("VGGFeatures: the layer list must start with a conv")
    return layers


class VGGFeatures(nn.Module):
    """``torchvision.models.<model>(...).features`` on the HIP path.  Parameters are named as in that Sequential (``0.weight``,
    ``0.bias``, ``2.weight``, ...) and have ``requires_grad=False``.  ``cfg`` replaces the layer list of ``model`` by a custom one
    such as ``[8, 8, "M", 16]``.  ``forward(x, taps)`` returns the activations at the Sequential indices ``taps``."""

    def __init__(self, model: str = "vgg16", cfg: Optional[Sequence] = None):
        super().__init__()
        if cfg is None:
            if model not in VGG_CFGS:
                raise ValueError(f"VGGFeatures: no layer list for {model!r}; one of {sorted(VGG_CFGS)} or cfg=")
            cfg = VGG_CFGS[model]
        self.model_name, self.cfg = model, list(cfg)
        self.layers = _layers_of(self.cfg)
        for i, layer in enumerate(self.layers):
            if layer[0] == "conv":
                self.add_module(str(i), _Conv3x3(layer[1], layer[2]))
        self.eval()

    def conv_indices(self) -> List[int]:
        return [i for i, layer in enumerate(self.layers) if layer[0] == "conv"]

    def load_torchvision(self, state) -> "VGGFeatures":
        """Copies a torchvision VGG state dict in: keys ``features.<i>.weight`` / ``<i>.weight`` (and ``.bias``); ``classifier.*`` is
        ignored.  A missing key, a shape mismatch or a key of a layer this trunk does not have raises ``RuntimeError``."""
        own = dict(self.named_parameters())
        seen = set()
        for key, value in state.items():
            if key.startswith("classifier."):
                continue
            name = key[len("features."):] if key.startswith("features.") else key
            if name not in own:
                raise RuntimeError(f"VGGFeatures.load_torchvision: unexpected key {key!r} for {self.model_name} {self.cfg}")
            if tuple(value.shape) != tuple(own[name].shape):
                raise RuntimeError(f"VGGFeatures.load_torchvision: {key!r} has shape {tuple(value.shape)}, expected "
                                   f"{tuple(own[name].shape)}")
            seen.add(name)
        missing = sorted(set(own) - seen)
        if missing:
            raise RuntimeError(f"VGGFeatures.load_torchvision: missing keys {missing}")
        with torch.no_grad():
            for key, value in state.items():
                if not key.startswith("classifier."):
                    name = key[len("features."):] if key.startswith("features.") else key
                    own[name].copy_(value.detach().to(dtype=torch.float32))
        return self

    def forward(self, x: torch.Tensor, taps: Iterable[int]) -> List[torch.Tensor]:
        """-> the outputs of the layers at the Sequential indices ``taps``, in index order; runs no layer behind the largest.  An index
        past the end of the Sequential yields nothing, as iterating the Sequential would.  ``x``: ``[B, 3, H, W]`` fp32 on the GPU,
        each side at least ``2 ** (poolings in front of the last tap)``."""
        from .autograd import fused_conv
        want = sorted({int(t) for t in taps})
        if any(t < 0 for t in want):
            raise ValueError(f"VGGFeatures: tap indices are Sequential indices >= 0, got {want}")
        want = [t for t in want if t < len(self.layers)]
        x = _fp32_gpu(x, "x")
        if x.dim() != 4 or int(x.shape[1]) != 3:
            raise RuntimeError(f"VGGFeatures: expected [B, 3, H, W] images, got {tuple(x.shape)}")
        if not want:
            return []
        first = getattr(self, "0").weight
        if first.device != x.device:
            raise RuntimeError(f"VGGFeatures: the weights live on {first.device}, the images on {x.device}; move the module first")
        out = []
        with torch.cuda.device(x.device):
            for i, layer in enumerate(self.layers[:want[-1] + 1]):
                if layer[0] == "conv":
                    conv = getattr(self, str(i))
                    x = fused_conv(x, None, conv.weight, conv.bias)
                elif layer[0] == "relu":
                    x = _ReluFn.apply(x, (i - 1) not in want)      # in place behind the conv, unless the conv's output is a tap
                else:
                    x = max_pool2(x)
                if i in want:
                    out.append(x)
        return out
