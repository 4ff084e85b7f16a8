"""Classical baselines on the device (``csrc/classical.hip``): what an enhancement method has to beat.  The dark-channel prior of
He, Sun and Tang (``prior="dcp"``), its underwater variant over G and B of Drews et al. (``"udcp"``), Dong et al.'s inverted-image
form for low light (``"inverted_dcp"``) -- the classical inverses of ``I = J T + B (1 - T)``, the model ``hdiff_amd.synth`` degrades
with -- and gray-world / shades-of-gray white balance.

    from hdiff_amd import classical
    J = classical.dehaze(img01)                               # float [N, 3, H, W] in [0, 1], in and out
    J, parts = classical.dehaze(img01, prior="udcp", return_parts=True)   # parts: dark, A, t_raw, t (and M, cut)
    out = classical.white_balance(img01, p=6.0)               # shades of gray; p=1 is gray-world, p=inf max-RGB
    Evaluate.evaluate(sampler, batches, ddim_step=20, baselines=("input", "gray_world", "dcp"))

``tests/_classical_def.py`` is the definition, every operation and its order written out.  The dark channel, the candidate cut, the
airlight and the raw transmission equal it bit for bit; the refinement is ``transfer.guided_fit`` / ``guided_apply`` themselves.

What is NOT pinned.  Every default -- ``patch=15``, ``omega=0.95``, ``t0=0.1``, ``top=1e-3`` (the papers' values, stated for
photographs of several hundred pixels), ``refine=(16, 1e-3)`` (a choice for 256-pixel images), ``p=1`` -- and agreement with any
published implementation of the dark-channel prior; nor any figure on real photographs.  The README records what the definition
gives on this repository's own procedural scenes.

Contrast from the histogram (``csrc/contrast.hip``), the family that raises the no-reference scores without inverting anything:

    out = classical.clahe(img01, clip_limit=2.0, grid=(8, 8), space="lab")   # CLAHE on 8-bit planes: CIE L* alone, or "rgb": each channel
    out = classical.equalize(img01, space="rgb")                              # global equalisation, the rule of Pillow's ImageOps.equalize
    Evaluate.evaluate(sampler, batches, ddim_step=20, baselines=("input", "clahe_lab", "equalize"))      # CONTRAST_BASELINES

``tests/_contrast_def.py`` is their definition; the quantised planes, every table and the ``"rgb"`` output equal it bit for bit, the
``"lab"`` output of ``clahe`` is its fp32 value or the neighbour, and ``equalize`` equals it bit for bit in both spaces and is
Pillow's byte for byte in ``"rgb"``.  NOT pinned: agreement with OpenCV's
``createCLAHE`` (the algorithm is written from memory, none is installed to compare with, and the padding knowingly differs: the
plane is padded to the next multiple of the grid and no further), the defaults ``clip_limit=2.0`` and ``grid=(8, 8)``, any figure on
real photographs.

Everything runs on the current stream, allocates through torch's caching allocator and never synchronises; there is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import math
from typing import Callable, Dict, Optional, Sequence, Tuple

import torch

from . import _capi
from . import engine as E

__all__ = ["dark_channel", "dehaze", "white_balance", "clahe", "equalize", "BASELINES", "CONTRAST_BASELINES", "resolve_baselines",
           "dehaze_settings", "PRIORS"]

PRIORS = {"dcp": ("rgb", False), "udcp": ("gb", False), "inverted_dcp": ("rgb", True)}      # the prior's channel set; inverted image
_CHANNELS = {"rgb": 3, "gb": 2}
MAX_PATCH = 63


def _stream(dev) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def _number(name: str, v) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise TypeError(f"hdiff: '{name}' must be a number, got {v!r}")
    return float(v)


def _patch(patch) -> int:
    if isinstance(patch, bool) or not isinstance(patch, int):
        raise TypeError(f"hdiff: 'patch' must be an int, got {patch!r}")
    if not 1 <= patch <= MAX_PATCH or patch % 2 == 0:
        raise ValueError(f"hdiff: 'patch' = {patch}; it must be odd, between 1 and {MAX_PATCH}")
    return patch


def _channels(channels) -> int:
    if channels not in _CHANNELS:
        raise ValueError(f"hdiff: 'channels' = {channels!r}; 'rgb' or 'gb'")
    return _CHANNELS[channels]


def _power(p) -> float:
    p = _number("p", p)
    if not p >= 1.0:          # NaN fails the comparison
        raise ValueError(f"hdiff: 'p' = {p!r}; it must be at least 1 (inf: the maximum)")
    return p


def dehaze_settings(*, prior="dcp", patch=15, omega=0.95, t0=0.1, top=1e-3, refine=(16, 1e-3)):
    """The settings of ``dehaze`` checked, on the host: ``(prior, patch, omega, t0, top, refine)`` with ``refine`` None or a checked
    ``(radius, eps)``."""
    if prior not in PRIORS:
        raise ValueError(f"hdiff: 'prior' = {prior!r}; one of {sorted(PRIORS)}")
    patch = _patch(patch)
    omega, t0, top = _number("omega", omega), _number("t0", t0), _number("top", top)
    if not 0.0 <= omega <= 1.0:
        raise ValueError(f"hdiff: 'omega' = {omega!r}; it must be in [0, 1]")
    if not 0.0 < t0 <= 1.0:
        raise ValueError(f"hdiff: 't0' = {t0!r}; it must be in (0, 1]")
    if not 0.0 < top <= 1.0:
        raise ValueError(f"hdiff: 'top' = {top!r}; it must be a fraction in (0, 1]")
    if refine is not None:
        from .transfer import transfer_settings
        if not isinstance(refine, (tuple, list)) or len(refine) != 2:
            raise ValueError(f"hdiff: 'refine' must be None or a (radius, eps) pair, got {refine!r}")
        refine = transfer_settings(refine[0], refine[1])
    return prior, patch, omega, t0, top, refine


def _images(t, name: str = "img01") -> torch.Tensor:
    if not torch.is_tensor(t):
        raise TypeError(f"hdiff: '{name}' must be a tensor, got {type(t).__name__}")
    if not t.is_floating_point() or t.dim() != 4 or t.shape[1] != 3 or t.shape[0] < 1 or t.shape[2] < 1 or t.shape[3] < 1:
        raise ValueError(f"hdiff: '{name}' has dtype {t.dtype} and shape {tuple(t.shape)}; it must be a float [N, 3, H, W] tensor")
    if t.is_cuda:
        if t.dtype != torch.float32:
            t = t.float()
        if not t.is_contiguous():
            t = t.contiguous()
    E.require_gpu_tensor(t, name)
    return t


def _point_min(x: torch.Tensor, channels: int, invert: bool, airlight: Optional[torch.Tensor]) -> torch.Tensor:
    N, _, H, W = (int(v) for v in x.shape)
    out = torch.empty(N, H, W, dtype=torch.float32, device=x.device)
    _capi.check(_capi.lib().hdiff_classical_point_min(x.data_ptr(), N, H, W, channels, int(invert),
                                                      None if airlight is None else airlight.data_ptr(), out.data_ptr(),
                                                      _stream(x.device)), "classical_point_min")
    return out


def _window_min(plane: torch.Tensor, patch: int, omega: Optional[float] = None) -> torch.Tensor:
    N, H, W = (int(v) for v in plane.shape)
    out = torch.empty_like(plane)
    _capi.check(_capi.lib().hdiff_classical_window_min(plane.data_ptr(), N, H, W, patch, int(omega is not None),
                                                       0.0 if omega is None else omega, out.data_ptr(), _stream(plane.device)),
                "classical_window_min")
    return out


def _airlight(x: torch.Tensor, dark: torch.Tensor, invert: bool, n_top: int) -> Tuple[torch.Tensor, torch.Tensor]:
    N, _, H, W = (int(v) for v in x.shape)
    need = C.c_int64(0)
    _capi.check(_capi.lib().hdiff_classical_airlight_workspace(N, H, W, C.byref(need)), "classical_airlight_workspace")
    scratch = torch.empty(need.value, dtype=torch.uint8, device=x.device)
    A = torch.empty(N, 3, dtype=torch.float32, device=x.device)
    cut = torch.empty(N, dtype=torch.float32, device=x.device)
    _capi.check(_capi.lib().hdiff_classical_airlight(x.data_ptr(), dark.data_ptr(), N, H, W, int(invert), n_top, A.data_ptr(),
                                                     cut.data_ptr(), scratch.data_ptr(), _stream(x.device)), "classical_airlight")
    return A, cut


def dark_channel(img01: torch.Tensor, *, patch: int = 15, channels: str = "rgb") -> torch.Tensor:
    """float ``[N, 3, H, W]`` -> float ``[N, H, W]``: the minimum of ``clip(img01, 0, 1)`` over the channel set (``"rgb"``, or
    ``"gb"``: the underwater prior's) and the ``patch x patch`` window clipped at the border.  ``patch`` odd, 1 to 63."""
    patch, ch = _patch(patch), _channels(channels)
    x = _images(img01)
    with torch.cuda.device(x.device):
        return _window_min(_point_min(x, ch, False, None), patch)


def dehaze(img01: torch.Tensor, *, prior: str = "dcp", patch: int = 15, omega: float = 0.95, t0: float = 0.1, top: float = 1e-3,
           refine: Optional[Tuple[int, float]] = (16, 1e-3), airlight: Optional[torch.Tensor] = None, return_parts: bool = False):
    """float ``[N, 3, H, W]`` in [0, 1] units -> the recovered ``J``, the same shape.

      1. ``dark`` = the dark channel of ``X = clip(img01, 0, 1)`` over the prior's channel set (``"inverted_dcp"``: ``X = 1 - clip``)
      2. ``A`` = the colour of the brightest pixel (largest R + G + B) among the ``max(1, floor(top H W))`` pixels of largest ``dark``,
         ties at the cut included, each channel at least 1 / 255; or ``airlight``, a float ``[N, 3]``, held to the same floor
         (``max(airlight, 1 / 255)`` in fp32, a NaN entry counting as 0)
      3. ``t_raw = 1 - omega windowmin(min_c X_c / A_c)``
      4. ``t`` = plane 0 of ``transfer.guided_apply(transfer.guided_fit(X, t_raw on three planes, radius, eps), X, clamp=False)``
         with ``refine=(radius, eps)``; ``t_raw`` itself with ``refine=None``
      5. ``J = clip((X - A) / max(t, t0) + A, 0, 1)`` (``"inverted_dcp"``: ``1 -`` that)

    With ``return_parts`` -> ``(J, parts)``, ``parts`` a dict of ``dark`` ``[N, H, W]``, ``A`` ``[N, 3]``, ``t_raw``, ``t`` ``[N, H, W]``,
    ``M`` (``min_c X_c / A_c``) and ``cut`` (``[N]``, the dark-channel value at the candidates' edge; None under ``airlight=``).  No
    default is backed by an image-quality figure on photographs (module docstring)."""
    prior, patch, omega, t0, top, refine = dehaze_settings(prior=prior, patch=patch, omega=omega, t0=t0, top=top, refine=refine)
    x = _images(img01)
    N, _, H, W = (int(v) for v in x.shape)
    ch, invert = _CHANNELS[PRIORS[prior][0]], PRIORS[prior][1]
    if airlight is not None:
        if not torch.is_tensor(airlight) or not airlight.is_floating_point() or tuple(airlight.shape) != (N, 3):
            raise ValueError(f"hdiff: 'airlight' must be a float [{N}, 3] tensor")
        if airlight.device != x.device:
            raise ValueError(f"hdiff: 'airlight' lives on {airlight.device} and 'img01' on {x.device}; both must be on one device")
        airlight = torch.nan_to_num(airlight.float(), nan=0.0).clamp_min(1.0 / 255.0).contiguous()      # step 2's floor: A_c > 0
    with torch.cuda.device(x.device):
        dark = _window_min(_point_min(x, ch, invert, None), patch)
        if airlight is None:
            A, cut = _airlight(x, dark, invert, max(1, int(math.floor(top * H * W))))
        else:
            A, cut = airlight, None
        M = _point_min(x, ch, invert, A)
        t_raw = _window_min(M, patch, omega)
        t = t_raw
        if refine is not None:
            from . import transfer as T
            guide = torch.nan_to_num(x, nan=0.0).clamp(0, 1)          # X as the kernels read it: a NaN clips to 0
            if invert:
                guide = 1.0 - guide
            coef = T.guided_fit(guide, t_raw[:, None].expand(N, 3, H, W).contiguous(), radius=refine[0], eps=refine[1])
            t = T.guided_apply(coef, guide, clamp=False)[:, 0].contiguous()
        J = torch.empty_like(x)
        _capi.check(_capi.lib().hdiff_classical_recover(x.data_ptr(), t.data_ptr(), A.data_ptr(), N, H, W, int(invert), t0, J.data_ptr(),
                                                        _stream(x.device)), "classical_recover")
    if return_parts:
        return J, {"dark": dark, "A": A, "t_raw": t_raw, "t": t, "M": M, "cut": cut}
    return J


def white_balance(img01: torch.Tensor, *, p: float = 1.0, return_gains: bool = False):
    """float ``[N, 3, H, W]`` -> ``clip(X_c g_c, 0, 1)`` with ``X = clip(img01, 0, 1)``, ``m_c = (mean X_c^p)^(1 / p)`` per image and
    ``g_c = mean(m) / max(m_c, 1e-6)``: gray-world at ``p=1``, shades of gray at ``p=6``, max-RGB at ``p=inf``.  With ``return_gains``
    -> ``(out, gains)``, ``gains`` float64 ``[N, 3]``."""
    p = _power(p)
    x = _images(img01)
    N, _, H, W = (int(v) for v in x.shape)
    need = C.c_int64(0)
    _capi.check(_capi.lib().hdiff_white_balance_workspace(N, H, W, C.byref(need)), "white_balance_workspace")
    with torch.cuda.device(x.device):
        scratch = torch.empty(need.value, dtype=torch.uint8, device=x.device)
        gains = torch.empty(N, 3, dtype=torch.float64, device=x.device)
        out = torch.empty_like(x)
        _capi.check(_capi.lib().hdiff_white_balance(x.data_ptr(), N, H, W, p, gains.data_ptr(), out.data_ptr(), scratch.data_ptr(),
                                                    _stream(x.device)), "white_balance")
    return (out, gains) if return_gains else out


# ---------------------------------------------------------------------------------------------------------------- contrast
_SPACES = {"rgb": 3, "lab": 1}         # the 8-bit planes a space is enhanced on: each channel, or CIE L* alone
_MAX_TILES = 16


def _f32(v: float) -> float:
    """One rounding to fp32.  A quotient of two fp32 values taken in double and rounded here is the fp32 quotient (53 >= 2 * 24 + 2)."""
    return C.c_float(v).value


def _space(space) -> int:
    if space not in _SPACES:
        raise ValueError(f"hdiff: 'space' = {space!r}; one of {sorted(_SPACES)}")
    return _SPACES[space]


def _grid(grid) -> Tuple[int, int]:
    if not isinstance(grid, (tuple, list)) or len(grid) != 2 or any(isinstance(g, bool) or not isinstance(g, int) for g in grid):
        raise ValueError(f"hdiff: 'grid' must be a (tiles_y, tiles_x) pair of ints, got {grid!r}")
    ty, tx = grid
    if not (1 <= ty <= _MAX_TILES and 1 <= tx <= _MAX_TILES):
        raise ValueError(f"hdiff: 'grid' = {tuple(grid)!r}; each value between 1 and {_MAX_TILES}")
    return ty, tx


def _clip_limit(clip_limit) -> float:
    clip_limit = _number("clip_limit", clip_limit)
    if not clip_limit >= 0.0:          # NaN fails the comparison
        raise ValueError(f"hdiff: 'clip_limit' = {clip_limit!r}; it must be at least 0 (0: no clipping)")
    return clip_limit


def _fits(H: int, W: int, ty: int, tx: int) -> None:
    if H < ty or W < tx:
        raise ValueError(f"hdiff: a {H} x {W} image cannot be cut into a ({ty}, {tx}) grid; it needs H >= tiles_y and W >= tiles_x")


def _tile_constants(H: int, W: int, ty: int, tx: int, clip_limit: float):
    """What the kernels are handed for an ``H x W`` plane: ``(clip, scale, inv_th, inv_tw)`` -- the count a tile's bin is cut at (the
    tile's area where nothing is cut) and the three fp32 constants, each one division on the host."""
    th, tw = -(-H // ty), -(-W // tx)
    area = th * tw
    clip = area
    if clip_limit > 0.0:
        c = clip_limit * float(area) / 256.0
        clip = area if c >= area else max(1, int(math.floor(c)))      # a clip above the area cuts nothing, like the area itself
    return clip, _f32(255.0 / _f32(area)), _f32(1.0 / _f32(th)), _f32(1.0 / _f32(tw))


def _quantise(x: torch.Tensor, planes: int) -> torch.Tensor:
    N, _, H, W = (int(v) for v in x.shape)
    q = torch.empty(N, planes, H, W, dtype=torch.uint8, device=x.device)
    _capi.check(_capi.lib().hdiff_contrast_quantise(x.data_ptr(), N, H, W, int(planes == 1), q.data_ptr(), _stream(x.device)),
                "contrast_quantise")
    return q


def _apply(x: torch.Tensor, q: torch.Tensor, lut: torch.Tensor, ty: int, tx: int, inv_th: float, inv_tw: float) -> torch.Tensor:
    N, _, H, W = (int(v) for v in x.shape)
    out = torch.empty_like(x)
    _capi.check(_capi.lib().hdiff_contrast_apply(x.data_ptr(), q.data_ptr(), lut.data_ptr(), N, H, W, int(q.shape[1] == 1), ty, tx,
                                                 inv_th, inv_tw, out.data_ptr(), _stream(x.device)), "contrast_apply")
    return out


def clahe(img01: torch.Tensor, *, clip_limit: float = 2.0, grid: Tuple[int, int] = (8, 8), space: str = "lab",
          return_parts: bool = False):
    """float ``[N, 3, H, W]`` in [0, 1] units -> float32, the same shape: contrast-limited adaptive histogram equalisation of the
    8-bit planes of ``space`` (``"rgb"``: each channel as its own plane; ``"lab"``: CIE L* alone, a and b kept).

      1. ``q`` = the planes quantised to bytes (``floor(X 255 + 0.5)``, or ``floor(L 2.55 + 0.5)``), ``X = clip(img01, 0, 1)``
      2. per tile of the ``grid = (tiles_y, tiles_x)`` (1 to 16 each; the plane padded right and bottom to a multiple by reflection): the
         256-bin histogram, cut at ``max(1, floor(clip_limit area / 256))`` with the excess spread over the bins in one pass
         (``clip_limit=0``: no cut, plain adaptive equalisation), and its cumulative sum scaled to 0..255: the tile's table
      3. every pixel through the four tables around it, blended bilinearly in fp32, rounded to a byte
      4. back to float: ``q' / 255``, or ``lab_to_srgb(q' / 2.55, a, b)`` clipped to [0, 1]

    ``tests/_contrast_def.py`` writes every operation out; ``q``, the tables and the ``"rgb"`` output equal it bit for bit.  With
    ``return_parts`` -> ``(out, parts)``, ``parts`` a dict of ``q`` (uint8 ``[N, P, H, W]``, ``P`` = 3 or 1) and ``lut`` (uint8
    ``[N, P, tiles_y, tiles_x, 256]``).  Neither default is backed by a figure on photographs (module docstring)."""
    planes, (ty, tx), clip_limit = _space(space), _grid(grid), _clip_limit(clip_limit)
    if torch.is_tensor(img01) and img01.dim() == 4:      # a grid too fine for the image is a ValueError wherever the tensor lives:
        _fits(int(img01.shape[2]), int(img01.shape[3]), ty, tx)      # ahead of `_images`, which refuses a CPU tensor
    x = _images(img01)
    N, _, H, W = (int(v) for v in x.shape)
    clip, scale, inv_th, inv_tw = _tile_constants(H, W, ty, tx, clip_limit)
    with torch.cuda.device(x.device):
        q = _quantise(x, planes)
        lut = torch.empty(N, planes, ty, tx, 256, dtype=torch.uint8, device=x.device)
        _capi.check(_capi.lib().hdiff_clahe_luts(q.data_ptr(), N, planes, H, W, ty, tx, clip, scale, lut.data_ptr(), _stream(x.device)),
                    "clahe_luts")
        out = _apply(x, q, lut, ty, tx, inv_th, inv_tw)
    return (out, {"q": q, "lut": lut}) if return_parts else out


def equalize(img01: torch.Tensor, *, space: str = "rgb", return_parts: bool = False):
    """float ``[N, 3, H, W]`` in [0, 1] units -> float32, the same shape: global histogram equalisation of the 8-bit planes of
    ``space`` by the rule of Pillow's ``ImageOps.equalize`` -- ``lut[i] = (step // 2 + sum(h[:i])) // step`` with ``step = (H W - the
    last filled bin's count) // 255``, at most 255; a plane with fewer than two filled bins, or with ``step == 0``, is left as it is.
    With ``return_parts`` -> ``(out, parts)``, ``parts`` a dict of ``q`` (uint8 ``[N, P, H, W]``) and ``lut`` (uint8 ``[N, P, 256]``)."""
    planes = _space(space)
    x = _images(img01)
    N, _, H, W = (int(v) for v in x.shape)
    need = C.c_int64(0)
    _capi.check(_capi.lib().hdiff_equalize_luts_workspace(N, planes, H, W, C.byref(need)), "equalize_luts_workspace")
    with torch.cuda.device(x.device):
        q = _quantise(x, planes)
        scratch = torch.empty(need.value, dtype=torch.uint8, device=x.device)
        lut = torch.empty(N, planes, 256, dtype=torch.uint8, device=x.device)
        _capi.check(_capi.lib().hdiff_equalize_luts(q.data_ptr(), N, planes, H, W, lut.data_ptr(), scratch.data_ptr(), _stream(x.device)),
                    "equalize_luts")
        out = _apply(x, q, lut, 0, 0, 1.0, 1.0)
    return (out, {"q": q, "lut": lut}) if return_parts else out


def _identity(img01: torch.Tensor) -> torch.Tensor:
    return img01


# name -> callable on a float [N, 3, H, W] batch in [0, 1], each with the defaults above
BASELINES: Dict[str, Callable[[torch.Tensor], torch.Tensor]] = {
    "input": _identity,
    "gray_world": lambda img01: white_balance(img01, p=1.0),
    "dcp": lambda img01: dehaze(img01, prior="dcp"),
    "udcp": lambda img01: dehaze(img01, prior="udcp"),
    "inverted_dcp": lambda img01: dehaze(img01, prior="inverted_dcp"),
}


# the contrast family, each with the defaults above.  A table of its own: ``BASELINES`` is the set of inverses of the image-formation
# model and stays as it is; and there is no bare "clahe" -- the name has to say which planes were enhanced, the two differ in every score
CONTRAST_BASELINES: Dict[str, Callable[[torch.Tensor], torch.Tensor]] = {
    "clahe_lab": lambda img01: clahe(img01, space="lab"),
    "clahe_rgb": lambda img01: clahe(img01, space="rgb"),
    "equalize": lambda img01: equalize(img01, space="rgb"),
}


def resolve_baselines(baselines) -> Sequence[Tuple[str, Callable]]:
    """``evaluate``'s ``baselines=`` as a list of ``(name, callable)``: names out of ``BASELINES``, then out of ``CONTRAST_BASELINES``, or
    pairs of the caller's own.  Raises on an unknown name, a name that is not a plain word, a duplicate, or something that cannot be
    called -- on the host."""
    if isinstance(baselines, (str, bytes)) or not isinstance(baselines, (tuple, list)):
        raise TypeError(f"hdiff: 'baselines' must be a sequence of names or (name, callable) pairs, got {baselines!r}")
    out = []
    for b in baselines:
        if isinstance(b, str):
            if b in BASELINES:
                name, fn = b, BASELINES[b]
            elif b in CONTRAST_BASELINES:
                name, fn = b, CONTRAST_BASELINES[b]
            else:
                raise ValueError(f"hdiff: unknown baseline {b!r}; one of {sorted(BASELINES)} or {sorted(CONTRAST_BASELINES)}, or a "
                                 "(name, callable) pair")
        elif isinstance(b, (tuple, list)) and len(b) == 2 and isinstance(b[0], str) and callable(b[1]):
            name, fn = b
        else:
            raise TypeError(f"hdiff: a baseline must be a name or a (name, callable) pair, got {b!r}")
        if not name or not all(c.isalnum() or c == "_" for c in name):
            raise ValueError(f"hdiff: the baseline name {name!r} must be letters, digits and '_' (it becomes part of a res.txt key)")
        if name in (n for n, _ in out):
            raise ValueError(f"hdiff: the baseline {name!r} is given twice")
        out.append((name, fn))
    return out
