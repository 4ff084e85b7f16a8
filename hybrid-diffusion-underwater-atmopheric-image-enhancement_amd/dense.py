"""Dense layers along a token axis on the HIP path (``csrc/dense_tokens.hip``).

``linear_tokens(x, weight, bias)`` is ``nn.Linear`` over the channels of a channel-major ``(B, Cin, L)`` fp32 tensor: ``y[b, co, l] = bias[co] +
sum_ci weight[co, ci] x[b, ci, l]``, any ``Cin, Cout, L >= 1``.  ``linear_tokens_dgrad(dy, weight)`` is its input gradient ``dx = weight^T dy``:
the same kernel on the transposed pack.  Both contract on bf16 triples (six piece products with ``i + j <= 2``, fp32 accumulation: fp32-class
error) whatever the package's contraction mode is; ``dino.dense_route`` is where the trunk chooses between this and the conv route.  There is
no weight gradient and no autograd graph: callers that differentiate call the two functions themselves, as ``dino._DinoLossFn`` does.

The packs.  The kernel reads the weight pre-split (``hdiff_dense_pack``): 6 bytes per weight, K padded to 16 and the channels to 64.  A pack is
built on first use and kept in a ``PackCache`` (the module's own, or the caller's ``cache=``: a ``DinoV2Features`` has one, which dies with
it) under ``(data_ptr, device, transposed, shape)`` of the weight together with the weight's ``_version``: an in-place update moves the version and the next call packs again, into the same slot.  The transposed pack is built by the first
``linear_tokens_dgrad``, so a trunk that is never differentiated holds one pack per layer.  Memory: ``dinov2_vits14``'s dense layers have 21.5 M
weights, about 130 MB per pack (forward, and again transposed once a backward ran); ``dinov2_vitl14`` about 1.8 GB per pack.  An entry holds a
reference to its weight, so the address it is keyed on cannot be handed to another tensor while the entry lives; ``clear_packs()`` drops them all.
A pack built outside a stream capture is what a captured launch reads: run once eagerly before capturing, as with the trunk's position
embedding.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import torch

from . import _capi
from .perceptual import _fp32_gpu, _stream

__all__ = ["linear_tokens", "linear_tokens_dgrad", "pack_words", "PackCache", "clear_packs"]


class PackCache:
    """``key -> (the weight's _version, pack, the weight)``; one per owner of weights (a ``DinoV2Features`` has its own, which dies with it)."""

    def __init__(self):
        self.entries: Dict[Tuple, Tuple] = {}

    def clear(self) -> None:
        self.entries.clear()

    def __len__(self) -> int:
        return len(self.entries)

    def nbytes(self) -> int:
        return sum(4 * e[1].numel() for e in self.entries.values())

    def get(self, w: torch.Tensor, transposed: bool) -> torch.Tensor:
        Cout, Cin = (int(v) for v in w.shape)
        key = (w.data_ptr(), str(w.device), bool(transposed), (Cout, Cin))
        hit = self.entries.get(key)
        if hit is not None and hit[0] == w._version:
            return hit[1]
        words = pack_words(Cin, Cout) if transposed else pack_words(Cout, Cin)
        with torch.cuda.device(w.device):
            wp = torch.empty(words, dtype=torch.int32, device=w.device)
            _capi.check(_capi.lib().hdiff_dense_pack(w.data_ptr(), wp.data_ptr(), Cout, Cin, int(bool(transposed)), _stream(w.device)),
                        "dense_pack")
        self.entries[key] = (w._version, wp, w)
        return wp


_PACKS = PackCache()                     # what calls without cache= use


def clear_packs() -> None:
    """Forgets every pack of the default cache (and the weights they hold on to)."""
    _PACKS.clear()


def pack_words(Cout: int, Cin: int) -> int:
    """32-bit words of the pack of a GEMM with ``Cout`` outputs and ``Cin`` inputs (``hdiff_dense_pack_words``)."""
    n = C.c_int64(0)
    _capi.check(_capi.lib().hdiff_dense_pack_words(int(Cout), int(Cin), C.byref(n)), "dense_pack_words")
    return n.value


def _weight(weight, name="weight"):
    # (checked before _fp32_gpu, which would copy a strided weight: a pack keyed on a temporary)
    if torch.is_tensor(weight) and (weight.dim() != 2 or not weight.is_contiguous()):
        raise RuntimeError(f"hdiff: '{name}' must be a contiguous (Cout, Cin) matrix, got {tuple(weight.shape)} with strides "
                           f"{weight.stride()}")
    return _fp32_gpu(weight, name).detach()


def _bcl(x, name, C_want, wname):
    x = _fp32_gpu(x, name)
    if x.dim() != 3:
        raise RuntimeError(f"hdiff: '{name}' must be channel-major (B, C, L), got {tuple(x.shape)}")
    if int(x.shape[1]) != C_want:
        raise RuntimeError(f"hdiff: '{name}' has {int(x.shape[1])} channels, '{wname}' wants {C_want}")
    if x.numel() == 0:
        raise RuntimeError(f"hdiff: '{name}' is empty: {tuple(x.shape)}")
    return x


def _launch(x, wp, bias, Cout: int):
    B, Cin, L = (int(v) for v in x.shape)
    with torch.cuda.device(x.device):
        y = torch.empty(B, Cout, L, device=x.device)
        _capi.check(_capi.lib().hdiff_dense_tokens(x.data_ptr(), wp.data_ptr(), None if bias is None else bias.data_ptr(), y.data_ptr(), B, Cin,
                                                   Cout, L, _stream(x.device)), "dense_tokens")
    return y


def linear_tokens(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, *, cache: Optional[PackCache] = None) -> torch.Tensor:
    """``(B, Cin, L)`` against ``(Cout, Cin)`` [and ``(Cout,)``] -> ``(B, Cout, L)``.  Nothing is differentiated.  ``cache``: where the pack is
    kept (default: the module's own)."""
    w = _weight(weight)
    x = _bcl(x, "x", int(w.shape[1]), "weight")
    if w.device != x.device:
        raise RuntimeError(f"hdiff: 'weight' lives on {w.device}, 'x' on {x.device}")
    if bias is not None:
        bias = _fp32_gpu(bias, "bias").detach()
        if tuple(bias.shape) != (int(w.shape[0]),) or not bias.is_contiguous() or bias.device != x.device:
            raise RuntimeError(f"hdiff: 'bias' must be {int(w.shape[0])} contiguous values on {x.device}, got {tuple(bias.shape)} on {bias.device}")
    return _launch(x.detach(), (_PACKS if cache is None else cache).get(w, False), bias, int(w.shape[0]))


def linear_tokens_dgrad(dy: torch.Tensor, weight: torch.Tensor, *, cache: Optional[PackCache] = None) -> torch.Tensor:
    """``dx = weight^T dy``: ``(B, Cout, L)`` against ``(Cout, Cin)`` -> ``(B, Cin, L)``, bit for bit ``linear_tokens(dy, weight.t().contiguous())``."""
    w = _weight(weight)
    dy = _bcl(dy, "dy", int(w.shape[0]), "weight")
    if w.device != dy.device:
        raise RuntimeError(f"hdiff: 'weight' lives on {w.device}, 'dy' on {dy.device}")
    return _launch(dy.detach(), (_PACKS if cache is None else cache).get(w, True), None, int(w.shape[1]))
