"""A frozen DINOv2 ViT trunk on the HIP path, and the smooth-L1 perceptual loss that sits on its taps (``csrc/dino.hip``).

``DinoV2Features`` is the hub model ``dinov2_vits14 / vitb14 / vitl14`` in ``eval()``: patch 14, d_head 64, MLP ratio 4, exact GELU,
``LayerNorm(eps=1e-6)``, a LayerScale behind the attention and behind the MLP, a class token, a learned position embedding of
1 + 37 x 37 entries, no register tokens.  Activations are fp32, channel-major ``(B, C, L)`` with ``L = 1 + h * w`` and the class
token at position 0.  The dense layers (patch embedding on the unfolded 588-row columns, qkv, proj, fc1, fc2) are
``autograd.fused_conv(k=1)`` calls on the ``L`` positions viewed as a plane (``plane_of``), the attention core is
``hdiff_mha_flash_fwd / _bwd`` on the ``(B, 3C, L)`` qkv -- whose row order ``[Q | K | V]``, head ``h`` on rows ``h * d .. h * d + d - 1`` of each third, IS DINOv2's
``reshape(B, N, 3, heads, D)``: no row of ``qkv.weight`` is permuted -- and everything else is a kernel of ``csrc/dino.hip``.
``DinoV2Features(dense="tokens")`` runs the dense layers and their input gradients on ``csrc/dense_tokens.hip`` instead
(``hdiff_amd.dense``; ``dense_route`` decides; the default ``"conv"`` is the route just described).
``dino_perceptual`` adds ``smooth_l1_loss(..., 'mean')`` over the taps; its backward is written out by hand (no autograd graph inside
the trunk): every tap adds ``g * weight / n * clamp(a - b, -1, 1)`` to the gradient already flowing into its tensor, the dense layers
run their dgrad route and no weight gradient exists.  Nothing here runs in ATen.

The taps.  The reference hooks every module of the hub model and adds the loss of every hooked output; several modules return the
same tensor, so a tap carries a multiplicity (``default_taps``).  The attention probabilities (``attn.attn_drop``) are NOT a tap:
dinov2 runs its memory-efficient attention when xformers is present, and that path never calls the module.  ``drop_path1/2`` are not
called in ``eval()``.

Written from memory of the dinov2 code, which is not a dependency: the tap list, the position-embedding rule
(``resize_pos_embed``) and the initialisation.  No pretrained weights ship and none are fetched; ``load_dinov2`` takes the hub
checkpoint's state dict from the caller.  Agreement with the hub model is unpinned.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
import warnings
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn
from torch.autograd import Function

from . import _capi
from . import engine as E
from .perceptual import _fp32_gpu, _stream

__all__ = ["DINO_CFGS", "DinoV2Features", "dense_route", "default_taps", "select_taps", "resize_pos_embed", "dino_perceptual", "layer_norm",
           "gelu", "layer_scale","unfold_patches", "assemble_tokens", "smooth_l1_taps"]

DINO_CFGS: Dict[str, Dict[str, int]] = {
    "dinov2_vits14": dict(embed_dim=384, depth=12, heads=6),
    "dinov2_vitb14": dict(embed_dim=768, depth=12, heads=12),
    "dinov2_vitl14": dict(embed_dim=1024, depth=24, heads=16),
}
PATCH, CROP, POS_GRID, LN_EPS, INTERPOLATE_OFFSET = 14, 2, 37, 1e-6, 0.1
_HEAD_DIMS = (4, 8, 12, 16, 24, 32, 48, 64)          # what hdiff_mha_flash_* accepts


def check_model_name(model: str, version: str = "dinov2") -> None:
    """``ValueError`` for what is not provided: ``version='dino'``, the SwiGLU giant, the register-token variants."""
    have = f"provided: version 'dinov2' with {sorted(DINO_CFGS)}"
    if version != "dinov2":
        raise ValueError(f"PerceptualLoss_dino: version {version!r} is not provided ({have})")
    if model not in DINO_CFGS:
        why = "SwiGLU MLP" if "vitg" in str(model) else ("register tokens" if str(model).endswith("_reg") else "unknown")
        raise ValueError(f"PerceptualLoss_dino: model {model!r} is not provided ({why}; {have})")


# ----------------------------------------------------------------------------------------------------------------------
# taps
# ----------------------------------------------------------------------------------------------------------------------
_BLOCK_TAPS = ((("norm1",), "norm1"), (("attn.qkv",), "qkv"), (("attn.proj", "attn.proj_drop", "attn"), "proj"), (("ls1",), "ls1"),
               (("norm2",), "norm2"), (("mlp.fc1",), "fc1"), (("mlp.act", "mlp.drop"), "act"), (("mlp.fc2", "mlp.drop", "mlp"), "fc2"),
               (("ls2",), "ls2"), (("",), "out"))


def default_taps(depth: int) -> List[Tuple[Tuple[str, ...], str, int]]:
    """``[(module names, tensor key, multiplicity)]`` in forward order: what ``layers=None`` hooks.  ``mlp.drop`` is called twice per
    block and so names two tensors; the root module is ``""``; ``head`` is an Identity on the class token of ``norm``."""
    taps = [(("patch_embed.proj",), "patch", 1), (("patch_embed.norm", "patch_embed"), "patch", 2)]
    for i in range(depth):
        for names, key in _BLOCK_TAPS:
            full = tuple(f"blocks.{i}.{n}" if n else f"blocks.{i}" for n in names)
            taps.append((full, f"{i}.{key}", len(full)))
    taps += [(("norm",), "norm", 1), (("head", ""), "cls", 2)]
    return taps


def select_taps(depth: int, layers: Optional[Sequence[str]]):
    """The taps whose module names are listed, with multiplicity = the number of listed names on that tensor."""
    taps = default_taps(depth)
    if layers is None:
        return taps
    if isinstance(layers, (str, bytes)):
        raise TypeError("layers must be a sequence of module names")
    want = list(layers)
    known = {n for names, _, _ in taps for n in names}
    unknown = [n for n in want if n not in known]
    if unknown:
        raise ValueError(f"PerceptualLoss_dino: unknown module names {unknown}; the hooked modules are patch_embed[.proj|.norm], "
                         f"blocks.i[.norm1|.attn|.attn.qkv|.attn.proj|.attn.proj_drop|.ls1|.norm2|.mlp|.mlp.fc1|.mlp.act|.mlp.drop|"
                         f".mlp.fc2|.ls2], norm, head and '' (the root)")
    out = []
    for names, key, _ in taps:
        m = sum(1 for n in names if n in want)
        if m:
            out.append((tuple(n for n in names if n in want), key, m))
    if not out:
        raise ValueError("PerceptualLoss_dino: layers selects no tap")
    return out


# ----------------------------------------------------------------------------------------------------------------------
# position embedding
# ----------------------------------------------------------------------------------------------------------------------
def resize_pos_embed(pos_embed: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """``(1, 1 + M*M, C)`` -> ``(1, 1 + h*w, C)``: the class entry as it is, the patch grid resized bicubically
    (``align_corners=False``, no antialias) with DINOv2's ``interpolate_offset = 0.1`` in its scale-factor form,
    ``F.interpolate(grid, scale_factor=((h + 0.1) / M, (w + 0.1) / M), mode="bicubic")``; ``h == w == M`` returns the embedding
    unchanged.  Written from memory of dinov2's ``interpolate_pos_encoding``; runs on the host, once per size."""
    n = int(pos_embed.shape[1]) - 1
    M = int(round(math.sqrt(n)))
    if M * M != n:
        raise ValueError(f"resize_pos_embed: {n} patch entries are not a square grid")
    if h == M and w == M:
        return pos_embed
    Cc = int(pos_embed.shape[2])
    p = pos_embed.detach().to(device="cpu")
    grid = p[:, 1:].reshape(1, M, M, Cc).permute(0, 3, 1, 2)
    sf = (float(h + INTERPOLATE_OFFSET) / M, float(w + INTERPOLATE_OFFSET) / M)
    out = torch.nn.functional.interpolate(grid, scale_factor=sf, mode="bicubic", align_corners=False, antialias=False)
    if tuple(out.shape[-2:]) != (h, w):
        raise RuntimeError(f"resize_pos_embed: the resize gave {tuple(out.shape[-2:])}, expected {(h, w)}")
    out = out.permute(0, 2, 3, 1).reshape(1, h * w, Cc)
    return torch.cat([p[:, :1], out], dim=1)


# ----------------------------------------------------------------------------------------------------------------------
# launches
# ----------------------------------------------------------------------------------------------------------------------
def _lib():
    return _capi.lib()


def grid_of(H: int, W: int) -> Tuple[int, int]:
    """The patch grid of an ``H x W`` image: 2 pixels come off every edge (the reference's ``_crop_tensor``), then 14 x 14 patches."""
    if H - 2 * CROP <= 0 or W - 2 * CROP <= 0 or (H - 2 * CROP) % PATCH or (W - 2 * CROP) % PATCH:
        raise RuntimeError(f"DinoV2Features: images are {H} x {W}; H - 4 = {H - 4} and W - 4 = {W - 4} must be positive multiples of "
                           f"{PATCH} (2 pixels are cropped from every edge, e.g. 256 -> 252 = 18 x 14)")
    return (H - 2 * CROP) // PATCH, (W - 2 * CROP) // PATCH


def _unfold(x):
    B, _, H, W = (int(v) for v in x.shape)
    h, w = grid_of(H, W)
    cols = torch.empty(B, 3 * PATCH * PATCH, h * w, device=x.device)
    _capi.check(_lib().hdiff_dino_unfold(x.data_ptr(), cols.data_ptr(), B, H, W, _stream(x.device)), "dino_unfold")
    return cols


def _fold(dcols, B, H, W):
    dx = torch.empty(B, 3, H, W, device=dcols.device)
    _capi.check(_lib().hdiff_dino_fold(dcols.data_ptr(), dx.data_ptr(), B, H, W, _stream(dcols.device)), "dino_fold")
    return dx


def _tokens(patch, cls, pos):
    B, Cc, P = (int(v) for v in patch.shape)
    tok = torch.empty(B, Cc, P + 1, device=patch.device)
    _capi.check(_lib().hdiff_dino_tokens_fwd(patch.data_ptr(), cls.data_ptr(), pos.data_ptr(), tok.data_ptr(), B, Cc, P + 1,
                                             _stream(patch.device)), "dino_tokens_fwd")
    return tok


def _tokens_bwd(dtok):
    B, Cc, L = (int(v) for v in dtok.shape)
    dp = torch.empty(B, Cc, L - 1, device=dtok.device)
    _capi.check(_lib().hdiff_dino_tokens_bwd(dtok.data_ptr(), dp.data_ptr(), B, Cc, L, _stream(dtok.device)), "dino_tokens_bwd")
    return dp


def _ln(x, weight, bias, keep: bool, eps: float = LN_EPS):
    B, Cc, L = (int(v) for v in x.shape)
    y = torch.empty_like(x)
    mean = torch.empty(B, L, dtype=torch.float64, device=x.device) if keep else None
    rstd = torch.empty(B, L, dtype=torch.float64, device=x.device) if keep else None
    _capi.check(_lib().hdiff_layernorm_fwd(x.data_ptr(), weight.data_ptr(), bias.data_ptr(), C.c_float(eps), y.data_ptr(),
                                           None if mean is None else mean.data_ptr(), None if rstd is None else rstd.data_ptr(), B, Cc, L,
                                           _stream(x.device)), "layernorm_fwd")
    return y, mean, rstd


def _ln_bwd(x, weight, mean, rstd, dy, add):
    """-> add + dLN/dx(dy), written into ``add`` when there is one"""
    B, Cc, L = (int(v) for v in x.shape)
    dx = add if add is not None else torch.empty_like(x)
    _capi.check(_lib().hdiff_layernorm_bwd(x.data_ptr(), weight.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dy.data_ptr(),
                                           None if add is None else add.data_ptr(), dx.data_ptr(), B, Cc, L, _stream(x.device)),
                "layernorm_bwd")
    return dx


def _gelu(x):
    y = torch.empty_like(x)
    _capi.check(_lib().hdiff_gelu_fwd(x.data_ptr(), y.data_ptr(), x.numel(), _stream(x.device)), "gelu_fwd")
    return y


def _gelu_bwd(x, dy, out=None):
    out = dy if out is None else out
    _capi.check(_lib().hdiff_gelu_bwd(x.data_ptr(), dy.data_ptr(), out.data_ptr(), x.numel(), _stream(x.device)), "gelu_bwd")
    return out


def _ls(x, gamma, res, want_s: bool = True):
    B, Cc, L = (int(v) for v in x.shape)
    s = torch.empty_like(x) if want_s else None
    y = torch.empty_like(x)
    _capi.check(_lib().hdiff_layerscale_fwd(x.data_ptr(), gamma.data_ptr(), res.data_ptr(), None if s is None else s.data_ptr(),
                                            y.data_ptr(), B, Cc, L, _stream(x.device)), "layerscale_fwd")
    return s, y


def _ls_bwd(ds, gamma):
    B, Cc, L = (int(v) for v in ds.shape)
    dx = torch.empty_like(ds)
    _capi.check(_lib().hdiff_layerscale_bwd(ds.data_ptr(), gamma.data_ptr(), dx.data_ptr(), B, Cc, L, _stream(ds.device)),
                "layerscale_bwd")
    return dx


def plane_of(L: int) -> Tuple[int, int]:
    """The ``(rows, columns)`` the ``L`` positions of a token axis are shown to the one-tap conv as.  A 1x1 conv does not care how its
    positions are arranged, but the kernel that runs it here does: the direct 1x1 GEMM routes refuse these shapes (they want
    ``H * W`` a multiple of 128 and ``B * H * W >= 32768``; ``L = 325`` is neither), so the launch falls to the implicit-GEMM kernel,
    which cuts a plane into tiles of ``2^min(5, ceil log2 W)`` columns by ``128 / columns`` rows (256 / columns from 1024 positions
    on).  A ``1 x 325`` plane fills a quarter of every tile; ``13 x 25`` fills 63 %.  This picks the factorisation of ``L`` whose
    tiles cover the fewest positions among those at least 16 columns wide; a prime ``L`` stays ``1 x L``."""
    def covered(rows, cols):
        tw = 1 << min(5, max(0, (cols - 1).bit_length()))
        th = (256 if rows * cols >= 1024 else 128) // tw
        return -(-cols // tw) * tw * -(-rows // th) * th
    best = (covered(1, L), 1, L)
    for r in range(2, int(math.isqrt(L)) + 1):
        if L % r == 0:
            for rows, cols in ((r, L // r), (L // r, r)):
                if cols >= 16:
                    best = min(best, (covered(rows, cols), rows, cols))
    return best[1], best[2]


DENSE_ROUTES = ("conv", "tokens")
_MODE_NAMES = {0: "f32", 1: "bf16x3", 2: "f16"}


def dense_route(dense: str, mode: str) -> str:
    """Which kernel family runs the trunk's dense layers, forward and input gradient: ``"conv"`` -- ``autograd.fused_conv(k=1)`` on the
    token axis shown as a plane (``plane_of``) -- or ``"tokens"`` -- ``dense.linear_tokens`` / ``linear_tokens_dgrad``
    (``csrc/dense_tokens.hip``).  ``dense`` is the trunk's ``dense=`` argument, ``mode`` the contraction mode's name.  The token kernel
    contracts on bf16 triples only, so ``dense="tokens"`` in mode ``"f32"`` runs the conv route: the exact-fp32 arm stays one switch
    away, bit for bit what ``dense="conv"`` runs there."""
    if dense not in DENSE_ROUTES:
        raise ValueError(f"DinoV2Features: dense must be one of {DENSE_ROUTES}, got {dense!r}")
    if mode not in _MODE_NAMES.values():
        raise ValueError(f"dense_route: contraction mode must be one of {sorted(_MODE_NAMES.values())}, got {mode!r}")
    return "tokens" if dense == "tokens" and mode != "f32" else "conv"


def _dense(x, weight, bias, route: str = "conv", packs=None):
    """``nn.Linear`` over the channels of ``(B, Cin, L)``: the token kernel, or a one-tap conv on ``(B, Cin, rows, columns)``
    (``plane_of``)."""
    if route == "tokens":
        from .dense import linear_tokens
        return linear_tokens(x, weight, bias, cache=packs)
    from .autograd import fused_conv
    B, Cin, L = (int(v) for v in x.shape)
    Cout = int(weight.shape[0])
    rows, cols = plane_of(L)
    with torch.no_grad():
        return fused_conv(x.view(B, Cin, rows, cols), None, weight.view(Cout, Cin, 1, 1), bias, k=1).view(B, Cout, L)


def _dense_dgrad(dy, weight, route: str = "conv", packs=None):
    """The input gradient of ``_dense``: the token kernel on the transposed pack, or ``autograd._FusedConv.backward``'s dgrad launch
    (the forward kernels on the weight read as ``[in = Cout][out = Cin]``); the weight is frozen, so there is nothing else."""
    if route == "tokens":
        from .dense import linear_tokens_dgrad
        return linear_tokens_dgrad(dy, weight, cache=packs)
    from .autograd import _run_conv
    B, Cout, L = (int(v) for v in dy.shape)
    Cin = int(weight.shape[1])
    w4 = weight.view(Cout, Cin, 1, 1)
    taps = E.conv_taps(1, 0)
    dtaps = E.TapSet(taps.dy, taps.dx, [0 - v for v in taps.dy], [0 - v for v in taps.dx])
    rows, cols = plane_of(L)
    dx = torch.empty(B, Cin, rows, cols, device=dy.device)
    _run_conv(dy.view(B, Cout, rows, cols), None, [(w4, 1, dtaps.ky, dtaps.kx, 0)], dtaps, Cin, Cout, None, dx, B=B, H=rows, W=cols,
              VH=rows, VW=cols, x3=(w4, True))
    return dx.view(B, Cin, L)


def _flash_fwd(qkv, heads: int, want_lse: bool):
    lib = _lib()
    B, C3, L = (int(v) for v in qkv.shape)
    Cc = C3 // 3
    o = torch.empty(B, Cc, L, device=qkv.device)
    lse = torch.empty(B, heads, L, device=qkv.device) if want_lse else None
    need = C.c_int64(0)
    _capi.check(lib.hdiff_mha_flash_fwd_workspace(B, Cc, heads, L, C.byref(need)), "mha_flash_fwd_workspace")
    ws = torch.empty(need.value // 4 + 1, device=qkv.device) if need.value > 0 and lib.hdiff_get_contraction_mode() != 0 else None
    _capi.check(lib.hdiff_mha_flash_fwd_ws(qkv.data_ptr(), o.data_ptr(), None if lse is None else lse.data_ptr(), B, Cc, heads, L,
                                           None if ws is None else ws.data_ptr(), 0 if ws is None else need.value,
                                           _stream(qkv.device)), "mha_flash_fwd")
    return o, lse


def _flash_bwd(qkv, o, lse, d_o, heads: int):
    lib = _lib()
    B, C3, L = (int(v) for v in qkv.shape)
    Cc = C3 // 3
    delta = torch.empty(B, heads, L, device=qkv.device)
    dqkv = torch.empty_like(qkv)
    need = C.c_int64(0)
    _capi.check(lib.hdiff_mha_flash_bwd_workspace(B, Cc, heads, L, C.byref(need)), "mha_flash_bwd_workspace")
    ws = torch.empty(need.value, dtype=torch.float32, device=qkv.device) if need.value else None
    _capi.check(lib.hdiff_mha_flash_bwd(qkv.data_ptr(), o.data_ptr(), d_o.data_ptr(), lse.data_ptr(), delta.data_ptr(), dqkv.data_ptr(),
                                        None if ws is None else ws.data_ptr(), B, Cc, heads, L, _stream(qkv.device)), "mha_flash_bwd")
    return dqkv


class _Feat:
    """A tap's tensor as the tap kernels address it: ``B`` images of ``n_img`` elements, element ``j`` of image ``b`` at
    ``[b * img_stride + j * stride]`` of ``base``; ``view`` is the same numbers as a torch tensor."""
    __slots__ = ("base", "B", "n_img", "stride", "img_stride", "view")

    def __init__(self, base, B, n_img, stride, img_stride, view):
        self.base, self.B, self.n_img, self.stride, self.img_stride, self.view = base, B, n_img, stride, img_stride, view


def _feat(t):
    B = int(t.shape[0])
    n = t.numel() // B
    return _Feat(t, B, n, 1, n, t)


def _tap_fwd(a: _Feat, b: _Feat, weight: float, slot_ptr: int, ws):
    _capi.check(_lib().hdiff_smooth_l1_tap_fwd(a.base.data_ptr(), b.base.data_ptr(), a.B, a.n_img, a.stride, a.img_stride,
                                               C.c_double(float(weight)), slot_ptr, ws.data_ptr(), _stream(a.base.device)),
                "smooth_l1_tap_fwd")


def _tap_ws(feats: Sequence[_Feat]):
    need, top = C.c_int64(0), 0
    for f in feats:
        _capi.check(_lib().hdiff_smooth_l1_tap_workspace(f.B, f.n_img, C.byref(need)), "smooth_l1_tap_workspace")
        top = max(top, need.value)
    return torch.empty(top, dtype=torch.uint8, device=feats[0].base.device)


def _tap_bwd(a: _Feat, b: _Feat, g, weight: float, da_in, da_out):
    _capi.check(_lib().hdiff_smooth_l1_tap_bwd(a.base.data_ptr(), b.base.data_ptr(), g.data_ptr(), a.B, a.n_img, a.stride, a.img_stride,
                                               C.c_float(float(weight)), None if da_in is None else da_in.data_ptr(), da_out.data_ptr(),
                                               _stream(a.base.device)), "smooth_l1_tap_bwd")


# ----------------------------------------------------------------------------------------------------------------------
# the trunk
# ----------------------------------------------------------------------------------------------------------------------
def _trunc(shape):
    w = torch.empty(*shape)
    nn.init.trunc_normal_(w, std=0.02)
    return nn.Parameter(w, requires_grad=False)


class _Affine(nn.Module):
    def __init__(self, n: int, m: Optional[Sequence[int]] = None):
        super().__init__()
        if m is None:                                    # a LayerNorm
            self.weight = nn.Parameter(torch.ones(n), requires_grad=False)
        else:                                            # a Linear / the patch conv
            self.weight = _trunc((n, *m))
        self.bias = nn.Parameter(torch.zeros(n), requires_grad=False)


class _Gamma(nn.Module):
    def __init__(self, n: int):
        super().__init__()
        self.gamma = nn.Parameter(torch.ones(n), requires_grad=False)


class _Attn(nn.Module):
    def __init__(self, Cc: int):
        super().__init__()
        self.qkv, self.proj = _Affine(3 * Cc, (Cc,)), _Affine(Cc, (Cc,))


class _Mlp(nn.Module):
    def __init__(self, Cc: int):
        super().__init__()
        self.fc1, self.fc2 = _Affine(4 * Cc, (Cc,)), _Affine(Cc, (4 * Cc,))


class _Block(nn.Module):
    def __init__(self, Cc: int):
        super().__init__()
        self.norm1, self.attn, self.ls1 = _Affine(Cc), _Attn(Cc), _Gamma(Cc)
        self.norm2, self.mlp, self.ls2 = _Affine(Cc), _Mlp(Cc), _Gamma(Cc)


class _PatchEmbed(nn.Module):
    def __init__(self, Cc: int, patch: int):
        super().__init__()
        self.proj = _Affine(Cc, (3, patch, patch))


class DinoV2Features(nn.Module):
    """The hub model ``model`` on the HIP path, frozen, ``state_dict()`` keyed as the hub checkpoint (``cls_token``, ``pos_embed``,
    ``mask_token``, ``patch_embed.proj.*``, ``blocks.N.*``, ``norm.*``).  ``DinoV2Features(embed_dim=, depth=, heads=, patch=14,
    pos_grid=)`` builds a small trunk of the same architecture (tests); its head dim is any the attention kernels accept.  Without
    ``load_dinov2`` the weights are random (truncated normal 0.02, LayerScale 1, zero biases) and one ``RuntimeWarning`` says so.
    ``forward(x, layers=None)`` -> the tap tensors in ``select_taps`` order (``(B, C, L)``; the patch embedding ``(B, C, h*w)``; the
    class token ``(B, C)``).  ``dense="tokens"`` runs every dense layer and every input gradient on ``csrc/dense_tokens.hip`` instead of the
    one-tap conv (``dense_route``; the default ``"conv"`` launches what it always did; ``hdiff_amd.dense`` has the memory of the packs)."""

    def __init__(self, model: Optional[str] = "dinov2_vits14", *, embed_dim: Optional[int] = None, depth: Optional[int] = None,
                 heads: Optional[int] = None, patch: int = PATCH, pos_grid: int = POS_GRID, version: str = "dinov2", dense: str = "conv"):
        super().__init__()
        dense_route(dense, "f32")                        # raises for an unknown name
        self.dense = dense
        from .dense import PackCache
        self._packs = PackCache()
        if embed_dim is None:
            check_model_name(model, version)
            cfg = DINO_CFGS[model]
            embed_dim, depth, heads = cfg["embed_dim"], cfg["depth"], cfg["heads"]
        else:
            model = f"vit(embed_dim={embed_dim}, depth={depth}, heads={heads})"
        if patch != PATCH:
            raise ValueError(f"DinoV2Features: the unfold kernel cuts {PATCH} x {PATCH} patches, got patch={patch}")
        if not (isinstance(depth, int) and depth >= 1 and isinstance(heads, int) and heads >= 1 and embed_dim % heads == 0
                and embed_dim // heads in _HEAD_DIMS):
            raise ValueError(f"DinoV2Features: embed_dim={embed_dim}, depth={depth}, heads={heads}: the head dim must be one of "
                             f"{_HEAD_DIMS}")
        self.model_name, self.embed_dim, self.depth, self.heads, self.pos_grid = model, int(embed_dim), depth, heads, int(pos_grid)
        Cc = self.embed_dim
        self.cls_token = _trunc((1, 1, Cc))
        self.pos_embed = _trunc((1, 1 + self.pos_grid ** 2, Cc))
        self.mask_token = nn.Parameter(torch.zeros(1, Cc), requires_grad=False)        # kept for the checkpoint's sake, never read
        self.patch_embed = _PatchEmbed(Cc, patch)
        self.blocks = nn.ModuleList([_Block(Cc) for _ in range(depth)])
        self.norm = _Affine(Cc)
        self._pos_cache: Dict = {}
        self.pretrained = False
        self._warned_random = False
        self.eval()

    def load_dinov2(self, state) -> "DinoV2Features":
        """Copies a hub state dict in.  Strict: a missing key, an unexpected key or a shape mismatch raises ``RuntimeError``.  The
        attention kernels read the qkv rows in the checkpoint's own order, so nothing is permuted."""
        own = dict(self.named_parameters())
        unexpected = [k for k in state if k not in own]
        missing = [k for k in own if k not in state]
        if unexpected or missing:
            raise RuntimeError(f"DinoV2Features.load_dinov2 ({self.model_name}): missing keys {missing}, unexpected keys {unexpected}")
        for k, v in state.items():
            if tuple(v.shape) != tuple(own[k].shape):
                raise RuntimeError(f"DinoV2Features.load_dinov2: {k!r} has shape {tuple(v.shape)}, expected {tuple(own[k].shape)}")
        with torch.no_grad():
            for k, v in state.items():
                own[k].copy_(v.detach().to(dtype=torch.float32))
        self.pretrained = True
        return self

    def _pos(self, h: int, w: int, dev) -> torch.Tensor:
        """The position embedding at ``h x w`` as the token kernel reads it, ``(C, L)`` on the device; resized once per size and per
        version of the parameter."""
        key = (h, w, str(dev), self.pos_embed._version, self.pos_embed.data_ptr())
        if key not in self._pos_cache:
            self._pos_cache.clear()
            pe = resize_pos_embed(self.pos_embed, h, w)
            self._pos_cache[key] = pe[0].t().contiguous().to(device=dev, dtype=torch.float32)
        return self._pos_cache[key]

    def _route(self) -> str:
        """``dense_route`` at the contraction mode of this moment"""
        if self.dense == "conv":
            return "conv"
        return dense_route(self.dense, _MODE_NAMES[_lib().hdiff_get_contraction_mode()])

    def _check(self, x):
        x = _fp32_gpu(x, "x")
        if x.dim() != 4 or int(x.shape[1]) != 3:
            raise RuntimeError(f"DinoV2Features: expected [B, 3, H, W] images, got {tuple(x.shape)}")
        grid_of(int(x.shape[2]), int(x.shape[3]))
        if self.cls_token.device != x.device:
            raise RuntimeError(f"DinoV2Features: the weights live on {self.cls_token.device}, the images on {x.device}; move the module "
                               "first")
        if not self.pretrained and not self._warned_random:
            self._warned_random = True
            warnings.warn(f"DinoV2Features({self.model_name}): no weights were loaded (load_dinov2); the trunk is randomly initialised "
                          "and its loss is not the pretrained perceptual loss", RuntimeWarning, stacklevel=3)
        return x

    def _run(self, x, keep: bool):
        """-> (features by key as ``_Feat``, what the backward needs when ``keep``)"""
        B, _, H, W = (int(v) for v in x.shape)
        h, w = grid_of(H, W)
        Cc = self.embed_dim
        f: Dict[str, _Feat] = {}
        saved = []
        route = self._route()
        with torch.cuda.device(x.device):
            pos = self._pos(h, w, x.device)
            pw = self.patch_embed.proj.weight
            patch = _dense(_unfold(x), pw.view(Cc, -1), self.patch_embed.proj.bias, route, self._packs)
            f["patch"] = _feat(patch)
            t = _tokens(patch, self.cls_token, pos)
            L = h * w + 1
            for i, blk in enumerate(self.blocks):
                n1, m1, r1 = _ln(t, blk.norm1.weight, blk.norm1.bias, keep)
                qkv = _dense(n1, blk.attn.qkv.weight, blk.attn.qkv.bias, route, self._packs)
                o, lse = _flash_fwd(qkv, self.heads, keep)
                p = _dense(o, blk.attn.proj.weight, blk.attn.proj.bias, route, self._packs)
                s1, t1 = _ls(p, blk.ls1.gamma, t)
                n2, m2, r2 = _ln(t1, blk.norm2.weight, blk.norm2.bias, keep)
                fc1 = _dense(n2, blk.mlp.fc1.weight, blk.mlp.fc1.bias, route, self._packs)
                act = _gelu(fc1)
                fc2 = _dense(act, blk.mlp.fc2.weight, blk.mlp.fc2.bias, route, self._packs)
                s2, t2 = _ls(fc2, blk.ls2.gamma, t1)
                for key, val in (("norm1", n1), ("qkv", qkv), ("proj", p), ("ls1", s1), ("norm2", n2), ("fc1", fc1), ("act", act),
                                 ("fc2", fc2), ("ls2", s2), ("out", t2)):
                    f[f"{i}.{key}"] = _feat(val)
                if keep:
                    saved.append((t, m1, r1, qkv, o, lse, t1, m2, r2, fc1))
                t = t2
            nf, mf, rf = _ln(t, self.norm.weight, self.norm.bias, keep)
            f["norm"] = _feat(nf)
            f["cls"] = _Feat(nf, B, Cc, L, Cc * L, nf[:, :, 0])
        return f, (saved, t, mf, rf, (B, H, W)) if keep else None

    def forward(self, x: torch.Tensor, layers: Optional[Sequence[str]] = None) -> List[torch.Tensor]:
        taps = select_taps(self.depth, layers)
        x = self._check(x)
        with torch.no_grad():
            f, _ = self._run(x, False)
        return [f[key].view for _, key, _ in taps]


# ----------------------------------------------------------------------------------------------------------------------
# the loss on the taps
# ----------------------------------------------------------------------------------------------------------------------
def _loss_forward(fa: Dict[str, _Feat], fb: Dict[str, _Feat], taps):
    dev = fa[taps[0][1]].base.device
    B = fa[taps[0][1]].B
    slots = torch.empty(len(taps) * B, dtype=torch.float64, device=dev)
    out, per_image = torch.empty((), device=dev), torch.empty(B, device=dev)
    with torch.cuda.device(dev):
        ws = _tap_ws([fa[key] for _, key, _ in taps])
        for k, (_, key, mult) in enumerate(taps):
            _tap_fwd(fa[key], fb[key], mult, slots.data_ptr() + 8 * k * B, ws)
        _capi.check(_lib().hdiff_smooth_l1_tap_total(slots.data_ptr(), len(taps), B, out.data_ptr(), per_image.data_ptr(), _stream(dev)),
                    "smooth_l1_tap_total")
    return out, per_image


class _DinoLossFn(Function):
    """forward: the trunk on ``x`` (keeping what the backward reads), the tap sums against the target's features.  backward: the
    trunk walked in reverse by hand."""

    @staticmethod
    def forward(ctx, x, trunk, fb, taps, box):
        keep = bool(ctx.needs_input_grad[0])
        fa, saved = trunk._run(x, keep)
        out, per_image = _loss_forward(fa, fb, taps)
        box["per_image"] = per_image
        if keep:
            ctx.trunk, ctx.fa, ctx.fb, ctx.saved = trunk, fa, fb, saved
            ctx.mult = {}
            for _, key, m in taps:
                ctx.mult.setdefault(key, []).append(m)
        return out

    @staticmethod
    def backward(ctx, g):
        trunk, fa, fb = ctx.trunk, ctx.fa, ctx.fb
        blocks_saved, t_last, mf, rf, (B, H, W) = ctx.saved
        dev = t_last.device
        g = g.contiguous()
        route = trunk._route()

        def tap(key, grad):
            """the taps of ``key`` added to ``grad`` in place (a new tensor when nothing flows yet)"""
            for m in ctx.mult.get(key, ()):
                a = fa[key]
                if grad is None:
                    if a.stride == 1:
                        grad = torch.empty_like(a.base)
                        _tap_bwd(a, fb[key], g, m, None, grad)
                        continue
                    grad = torch.zeros_like(a.base)
                _tap_bwd(a, fb[key], g, m, grad, grad)
            return grad

        def tap_apart(key, grad):
            """the same into a tensor of its own: ``grad`` goes on as the residual stream's gradient"""
            ms = ctx.mult.get(key, ())
            if not ms or grad is None:
                return tap(key, grad)
            out = torch.empty_like(grad)
            _tap_bwd(fa[key], fb[key], g, ms[0], grad, out)
            for m in ms[1:]:
                _tap_bwd(fa[key], fb[key], g, m, out, out)
            return out

        with torch.cuda.device(dev):
            dn = tap("cls", tap("norm", None))
            G = None if dn is None else _ln_bwd(t_last, trunk.norm.weight, mf, rf, dn, None)
            for i in reversed(range(trunk.depth)):
                blk = trunk.blocks[i]
                t, m1, r1, qkv, o, lse, t1, m2, r2, fc1 = blocks_saved[i]
                G = tap(f"{i}.out", G)
                d = tap_apart(f"{i}.ls2", G)
                d = tap(f"{i}.fc2", None if d is None else _ls_bwd(d, blk.ls2.gamma))
                d = tap(f"{i}.act", None if d is None else _dense_dgrad(d, blk.mlp.fc2.weight, route, trunk._packs))
                d = tap(f"{i}.fc1", None if d is None else _gelu_bwd(fc1, d))
                d = tap(f"{i}.norm2", None if d is None else _dense_dgrad(d, blk.mlp.fc1.weight, route, trunk._packs))
                if d is not None:
                    G = _ln_bwd(t1, blk.norm2.weight, m2, r2, d, G)
                d = tap_apart(f"{i}.ls1", G)
                d = tap(f"{i}.proj", None if d is None else _ls_bwd(d, blk.ls1.gamma))
                d = None if d is None else _flash_bwd(qkv, o, lse, _dense_dgrad(d, blk.attn.proj.weight, route, trunk._packs), trunk.heads)
                d = tap(f"{i}.qkv", d)
                d = tap(f"{i}.norm1", None if d is None else _dense_dgrad(d, blk.attn.qkv.weight, route, trunk._packs))
                if d is not None:
                    G = _ln_bwd(t, blk.norm1.weight, m1, r1, d, G)
            d = tap("patch", None if G is None else _tokens_bwd(G))
            if d is None:
                return torch.zeros(B, 3, H, W, device=dev), None, None, None, None
            Cc = trunk.embed_dim
            dx = _fold(_dense_dgrad(d, trunk.patch_embed.proj.weight.view(Cc, -1), route, trunk._packs), B, H, W)
        return dx, None, None, None, None


def dino_perceptual(trunk: DinoV2Features, input: torch.Tensor, target: torch.Tensor, taps=None, return_per_image: bool = False):
    """``sum over taps of multiplicity * smooth_l1_loss(feature(input), feature(target), 'mean')`` as a 0-dim fp32 tensor.  ``input`` is
    differentiated; ``target``'s features are taken without a graph, in a pass of their own (nothing is batched across the two, and
    nothing across images).  ``return_per_image`` adds the ``(B,)`` per-image shares, which sum to the loss."""
    taps = select_taps(trunk.depth, None) if taps is None else taps
    a, b = trunk._check(input), trunk._check(target)
    if a.shape != b.shape or a.device != b.device:
        raise RuntimeError(f"PerceptualLoss_dino: input and target must have one shape and one device, got {tuple(a.shape)} on "
                           f"{a.device} and {tuple(b.shape)} on {b.device}")
    if int(a.shape[0]) > 256:
        raise RuntimeError(f"PerceptualLoss_dino: at most 256 images per call, got {int(a.shape[0])}")
    with torch.no_grad():
        fb, _ = trunk._run(b.detach(), False)
    box: Dict = {}
    loss = _DinoLossFn.apply(a, trunk, fb, taps, box)
    return (loss, box["per_image"]) if return_per_image else loss


# ----------------------------------------------------------------------------------------------------------------------
# the kernels one by one (tests, and callers who want the pieces); each carries its hand-written backward
# ----------------------------------------------------------------------------------------------------------------------
class _LayerNormFn(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        with torch.cuda.device(x.device):
            y, mean, rstd = _ln(x, weight, bias, True, eps)
        ctx.save_for_backward(x, weight, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, mean, rstd = ctx.saved_tensors
        with torch.cuda.device(x.device):
            return _ln_bwd(x, weight, mean, rstd, dy.contiguous(), None), None, None, None


class _GeluFn(Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        with torch.cuda.device(x.device):
            return _gelu(x)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        with torch.cuda.device(x.device):
            return _gelu_bwd(x, dy.contiguous(), torch.empty_like(x))


class _LayerScaleFn(Function):
    @staticmethod
    def forward(ctx, x, gamma, res):
        ctx.save_for_backward(gamma)
        with torch.cuda.device(x.device):
            return _ls(x, gamma, res, False)[1]

    @staticmethod
    def backward(ctx, dy):
        (gamma,) = ctx.saved_tensors
        dy = dy.contiguous()
        with torch.cuda.device(dy.device):
            return _ls_bwd(dy, gamma), None, dy


class _UnfoldFn(Function):
    @staticmethod
    def forward(ctx, x):
        ctx.shape = tuple(int(v) for v in x.shape)
        with torch.cuda.device(x.device):
            return _unfold(x)

    @staticmethod
    def backward(ctx, dcols):
        B, _, H, W = ctx.shape
        with torch.cuda.device(dcols.device):
            return _fold(dcols.contiguous(), B, H, W)


class _TokensFn(Function):
    @staticmethod
    def forward(ctx, patch, cls, pos):
        with torch.cuda.device(patch.device):
            return _tokens(patch, cls, pos)

    @staticmethod
    def backward(ctx, dtok):
        with torch.cuda.device(dtok.device):
            return _tokens_bwd(dtok.contiguous()), None, None


class _SmoothL1Fn(Function):
    @staticmethod
    def forward(ctx, a, b, weight):
        fa, fb = _feat(a), _feat(b)
        out, _ = _loss_forward({"t": fa}, {"t": fb}, [((), "t", weight)])
        ctx.save_for_backward(a, b)
        ctx.weight = weight
        return out

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        da = torch.empty_like(a)
        with torch.cuda.device(a.device):
            _tap_bwd(_feat(a), _feat(b), g.contiguous(), ctx.weight, None, da)
        return da, None, None


def _bcl(x, name):
    x = _fp32_gpu(x, name)
    if x.dim() != 3:
        raise RuntimeError(f"hdiff: '{name}' must be channel-major (B, C, L), got {tuple(x.shape)}")
    return x


def layer_norm(x, weight, bias, eps: float = LN_EPS):
    """``nn.LayerNorm(C, eps)`` over the channels of a channel-major ``(B, C, L)`` tensor; ``x`` is differentiated, the affine is not."""
    return _LayerNormFn.apply(_bcl(x, "x"), _fp32_gpu(weight, "weight").detach(), _fp32_gpu(bias, "bias").detach(), float(eps))


def gelu(x):
    """Exact GELU ``x * Phi(x)``."""
    return _GeluFn.apply(_fp32_gpu(x, "x"))


def layer_scale(x, gamma, res):
    """``res + gamma[c] * x`` on ``(B, C, L)``; ``x`` and ``res`` are differentiated."""
    return _LayerScaleFn.apply(_bcl(x, "x"), _fp32_gpu(gamma, "gamma").detach(), _bcl(res, "res"))


def unfold_patches(x):
    """``(B, 3, H, W)`` -> ``(B, 588, h*w)``: the 14 x 14 patches of the image without its 2-pixel border."""
    x = _fp32_gpu(x, "x")
    if x.dim() != 4 or int(x.shape[1]) != 3:
        raise RuntimeError(f"unfold_patches: expected [B, 3, H, W] images, got {tuple(x.shape)}")
    grid_of(int(x.shape[2]), int(x.shape[3]))
    return _UnfoldFn.apply(x)


def assemble_tokens(patch, cls, pos):
    """``(B, C, P)`` patches, ``cls`` of C values, ``pos (C, P + 1)`` -> ``(B, C, P + 1)`` tokens; ``patch`` is differentiated."""
    return _TokensFn.apply(_bcl(patch, "patch"), _fp32_gpu(cls, "cls").detach(), _fp32_gpu(pos, "pos").detach())


def smooth_l1_taps(input, target, weight: float = 1.0):
    """``weight * smooth_l1_loss(input, target, 'mean')`` (beta = 1) through the tap kernels; the first dim is the batch."""
    a, b = _fp32_gpu(input, "input"), _fp32_gpu(target, "target")
    if a.shape != b.shape or a.dim() < 1 or a.numel() == 0:
        raise RuntimeError(f"smooth_l1_taps: input and target must have one non-empty shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    return _SmoothL1Fn.apply(a, b.detach(), float(weight))
