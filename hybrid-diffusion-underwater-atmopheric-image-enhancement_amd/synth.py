"""Synthetic degradation on the device (``csrc/synth_degrade.hip``): the degraded input of a training pair drawn from its clean target.

Most paired underwater, haze and low-light sets in the literature are synthesised from clean images by the image-formation model.  This
module does that behind ``hdiff_batch_assemble``: the input of sample ``i`` at epoch ``e`` is a function of ``(label, seed, e, i)``
alone, drawn from counter-based Philox words that the geometric augmentation never uses, so a run repeats and resumes bit for bit and no
host work is done per batch.  ``tests/_synth_def.py`` is the definition: the parameter table matches it bit for bit, the bytes
everywhere.

Per sample a parameter row is drawn (``hdiff_synth_params``; the columns are ``COLUMNS``), then per pixel, in float64
(``hdiff_synth_apply``):

  1. range:    a smooth field ``s`` in [0, 1] -- a mean, a linear ramp and three low-frequency cosines -- scaled to ``d`` in metres;
  2. medium:   ``T_c = exp(-beta_c d)``, ``I_c = J_c T_c + B_c (1 - T_c)`` (underwater and haze share the formula);
  3. exposure: ``I_c = gain * I_c ** gamma``;
  4. noise:    ``I_c += sqrt(max(shot I_c, 0) + read^2) z`` with ``z`` the sample's own ``hdiff_randn_rows`` stream;
  5. quantise: ``floor(255 clamp01(I_c) + 0.5)``.

  * ``Synth(...)`` holds validated settings; ``Synth.underwater()``, ``Synth.haze()``, ``Synth.lowlight()`` are the named presets.
  * ``params`` / ``apply`` are the two launches; ``degrade(label, idx, synth=, seed=, epoch=, prob=)`` makes both.
  * ``noise_seed(seed, index, epoch)`` is the Philox seed of a sample's sensor noise.
  * ``procedural_scenes(n, H, W, seed)`` draws clean images on the host from integers alone: no files are involved.

``WATER_TYPES`` -- the per-metre transmission ``N(red, green, blue)`` of the ten Jerlov water types as the UWCNN paper tabulates them --
is UNPINNED: the values were written down from memory and nothing in this repository confirms them.  Override them with
``water_types={"name": (Nr, Ng, Nb), ...}``.  Nothing here claims that a preset matches a real water body or a real sensor.
"""
from __future__ import annotations

import ctypes as C
import math
from fractions import Fraction
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _capi
from .device_data import MAX_SIDE, _threshold
from .schedules import _splitmix64

__all__ = ["Synth", "WATER_TYPES", "COLUMNS", "N_PARAMS", "MAX_TYPES", "Z_OFFSET", "COUNTER_BASE", "noise_seed", "params", "apply",
           "degrade", "procedural_scenes"]

# UNPINNED (recalled, not checked against the paper): N(red, green, blue) per metre
WATER_TYPES: Dict[str, Tuple[float, float, float]] = {
    "I": (0.805, 0.961, 0.982), "IA": (0.804, 0.955, 0.975), "IB": (0.830, 0.950, 0.968), "II": (0.800, 0.925, 0.940),
    "III": (0.750, 0.885, 0.890), "1": (0.750, 0.885, 0.875), "3": (0.710, 0.820, 0.800), "5": (0.670, 0.730, 0.670),
    "7": (0.620, 0.610, 0.500), "9": (0.550, 0.460, 0.290),
}

MAX_TYPES = 16
N_PARAMS = 29
# the first column of each entry of a parameter row (include/hdiff.h, HDIFF_SYNTH_*); amp, fx, fy, phi, beta and veil take three
COLUMNS = {"selected": 0, "type": 1, "m": 2, "gx": 3, "gy": 4, "amp": 5, "fx": 8, "fy": 11, "phi": 14, "d_lo": 17, "d_hi": 18, "beta": 19,
           "veil": 22, "gamma": 25, "gain": 26, "shot": 27, "read": 28}
Z_OFFSET = 1 << 33             # the Philox offset of the sensor noise in a sample's stream
COUNTER_BASE = 1 << 32         # sample i at epoch e reads the counters COUNTER_BASE + 8 e + k, k < 8
_SEED_TAG = 0x73796E74685F7A31
_M64 = (1 << 64) - 1


class _Settings(C.Structure):
    _fields_ = [("n_types", C.c_int), ("type_beta", (C.c_double * 3) * MAX_TYPES), ("beta", C.c_double * 2), ("airlight", C.c_double * 2),
                ("veil", (C.c_double * 2) * 3), ("depth", C.c_double * 2), ("field_mean", C.c_double * 2),
                ("field_grad", C.c_double * 2), ("field_amp", C.c_double * 2), ("gamma", C.c_double * 2), ("gain", C.c_double * 2),
                ("shot", C.c_double * 2), ("read", C.c_double * 2)]


def _number(name: str, v) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float, Fraction)) or not math.isfinite(v):
        raise ValueError(f"Synth: {name} = {v!r}; a finite number")
    return float(v)


def _range(name: str, r, lo: Optional[float] = None, hi: Optional[float] = None, open_lo: bool = False) -> Tuple[float, float]:
    """``(lo, hi)`` from a pair or a single number, finite, ordered and inside the stated bounds."""
    if isinstance(r, (int, float, Fraction)) and not isinstance(r, bool):
        r = (r, r)
    if not isinstance(r, (tuple, list)) or len(r) != 2:
        raise ValueError(f"Synth: {name} = {r!r}; a (lo, hi) pair or one number")
    a, b = _number(name, r[0]), _number(name, r[1])
    if not a <= b:
        raise ValueError(f"Synth: {name} = ({a}, {b}); lo <= hi")
    if lo is not None and (a <= lo if open_lo else a < lo):
        raise ValueError(f"Synth: {name} = ({a}, {b}); {'above' if open_lo else 'at least'} {lo}")
    if hi is not None and b > hi:
        raise ValueError(f"Synth: {name} = ({a}, {b}); at most {hi}")
    return a, b


def _probability(name: str, p):
    if isinstance(p, bool) or not isinstance(p, (int, float, Fraction)) or not (0 <= p <= 1):      # NaN fails the comparison
        raise ValueError(f"Synth: {name} = {p!r}; a probability in [0, 1]")
    return p


class Synth:
    """The settings of the synthetic degradation.  Every range is a ``(lo, hi)`` pair (or one number) drawn uniformly per sample.

    ``water_types``: ``None`` (the medium's ``beta`` is drawn from ``beta``, one value for the three channels), or names out of
    ``WATER_TYPES``, or ``{"name": (Nr, Ng, Nb)}`` with per-metre transmissions in (0, 1]: a type is drawn per sample and
    ``beta_c = -ln N_c``.  ``airlight`` is the common part of the veiling light ``B`` and ``veil`` its per-channel part (one range, or
    three): ``B_c = clamp01(airlight + veil_c)``.  ``range_m``: two draws per sample span the scene's range in metres.
    ``field_mean`` / ``field_grad`` / ``field_amp``: the range field's mean, ramp and cosine amplitudes.  ``gamma`` / ``gain``: the
    exposure curve.  ``shot`` / ``read``: the sensor noise.  ``p_medium`` / ``p_exposure`` / ``p_noise``: the probability that a
    sample gets the stage at all."""

    def __init__(self, *, water_types=None, beta=(0.0, 0.0), airlight=(0.0, 0.0), veil=(0.0, 0.0), range_m=(0.0, 0.0),
                 field_mean=(0.3, 0.7), field_grad=(-0.5, 0.5), field_amp=(0.0, 0.15), gamma=(1.0, 1.0), gain=(1.0, 1.0),
                 shot=(0.0, 0.0), read=(0.0, 0.0), p_medium=1.0, p_exposure=1.0, p_noise=1.0):
        if water_types is None:
            types = None
        else:
            if isinstance(water_types, dict):
                items = list(water_types.items())
            elif isinstance(water_types, (tuple, list)):
                unknown = [t for t in water_types if not isinstance(t, str) or t not in WATER_TYPES]
                if unknown:
                    raise ValueError(f"Synth: unknown water types {unknown!r}; the table has {sorted(WATER_TYPES)}")
                items = [(t, WATER_TYPES[t]) for t in water_types]
            else:
                raise ValueError(f"Synth: water_types = {water_types!r}; names, a dict of name -> (Nr, Ng, Nb), or None")
            if not 1 <= len(items) <= MAX_TYPES:
                raise ValueError(f"Synth: {len(items)} water types; between 1 and {MAX_TYPES}")
            types = {}
            for name, N in items:
                if not isinstance(name, str) or not isinstance(N, (tuple, list)) or len(N) != 3:
                    raise ValueError(f"Synth: water type {name!r} = {N!r}; a name and (Nr, Ng, Nb)")
                N = tuple(_number(f"water type {name!r}", v) for v in N)
                if not all(0 < v <= 1 for v in N):
                    raise ValueError(f"Synth: water type {name!r} = {N}; transmissions per metre in (0, 1]")
                types[name] = N
        self.water_types = types
        self.beta = _range("beta", beta, lo=0.0)
        self.airlight = _range("airlight", airlight)
        veil = list(veil) if isinstance(veil, (tuple, list)) and len(veil) == 3 and all(isinstance(v, (tuple, list)) for v in veil) \
            else [veil] * 3
        self.veil = tuple(_range("veil", v) for v in veil)
        self.range_m = _range("range_m", range_m, lo=0.0)
        self.field_mean = _range("field_mean", field_mean)
        self.field_grad = _range("field_grad", field_grad)
        self.field_amp = _range("field_amp", field_amp)
        self.gamma = _range("gamma", gamma, lo=0.0, open_lo=True)
        self.gain = _range("gain", gain, lo=0.0)
        self.shot = _range("shot", shot, lo=0.0)
        self.read = _range("read", read, lo=0.0)
        self.p_medium = _probability("p_medium", p_medium)
        self.p_exposure = _probability("p_exposure", p_exposure)
        self.p_noise = _probability("p_noise", p_noise)

    # -- the named presets ---------------------------------------------------------------------------------------------------------
    @classmethod
    def underwater(cls, water_types=tuple(WATER_TYPES), range_m=(0.5, 15.0), veil=((0.0, 0.25), (0.25, 0.75), (0.3, 0.85)), **kw):
        """A Jerlov water type per sample (``beta_c = -ln N_c``), a veiling light drawn per channel, blue-green by default."""
        return cls(water_types=water_types, range_m=range_m, veil=veil, **kw)

    @classmethod
    def haze(cls, beta=(0.4, 1.6), airlight=(0.7, 1.0), tint=0.05, range_m=(0.3, 3.0), **kw):
        """One ``beta`` for the three channels and a near-grey airlight: ``B_c = airlight + U(-tint, tint)``."""
        tint = _number("tint", tint)
        if tint < 0:
            raise ValueError(f"Synth: tint = {tint}; at least 0")
        return cls(beta=beta, airlight=airlight, veil=(-tint, tint), range_m=range_m, **kw)

    @classmethod
    def lowlight(cls, gamma=(1.5, 3.0), gain=(0.3, 0.9), shot=(0.0, 0.01), read=(0.0, 0.02), **kw):
        """Darkened and noised: the exposure curve and the sensor noise, no medium."""
        return cls(gamma=gamma, gain=gain, shot=shot, read=read, p_medium=0.0, **kw)

    # -- what the kernels take -----------------------------------------------------------------------------------------------------
    def type_betas(self):
        """``[(name, (beta_r, beta_g, beta_b)), ...]`` in the order a sample's type index counts: ``beta_c = -ln N_c``."""
        return [] if self.water_types is None else [(k, tuple(-math.log(v) for v in N)) for k, N in self.water_types.items()]

    def settings(self) -> _Settings:
        S = _Settings()
        betas = self.type_betas()
        S.n_types = len(betas)
        for t, (_, b) in enumerate(betas):
            for c in range(3):
                S.type_beta[t][c] = b[c]
        for name, r in (("beta", self.beta), ("airlight", self.airlight), ("depth", self.range_m), ("field_mean", self.field_mean),
                        ("field_grad", self.field_grad), ("field_amp", self.field_amp), ("gamma", self.gamma), ("gain", self.gain),
                        ("shot", self.shot), ("read", self.read)):
            getattr(S, name)[0], getattr(S, name)[1] = r
        for c in range(3):
            S.veil[c][0], S.veil[c][1] = self.veil[c]
        return S

    def thresholds(self, prob=1.0) -> Dict[str, int]:
        """``{"th_select", "th_medium", "th_exposure", "th_noise"}``: the integers ``hdiff_synth_params`` takes."""
        return {"th_select": _threshold(_probability("prob", prob)), "th_medium": _threshold(self.p_medium),
                "th_exposure": _threshold(self.p_exposure), "th_noise": _threshold(self.p_noise)}

    def as_dict(self) -> Dict[str, object]:
        return {"water_types": None if self.water_types is None else {k: list(v) for k, v in self.water_types.items()},
                "beta": list(self.beta), "airlight": list(self.airlight), "veil": [list(v) for v in self.veil],
                "range_m": list(self.range_m), "field_mean": list(self.field_mean), "field_grad": list(self.field_grad),
                "field_amp": list(self.field_amp), "gamma": list(self.gamma), "gain": list(self.gain), "shot": list(self.shot),
                "read": list(self.read), "p_medium": self.p_medium, "p_exposure": self.p_exposure, "p_noise": self.p_noise}

    @classmethod
    def from_dict(cls, d) -> "Synth":
        if isinstance(d, Synth):
            return d
        if not isinstance(d, dict):
            raise TypeError(f"Synth.from_dict: a Synth or its dict, got {type(d).__name__}")
        return cls(**d)

    def __repr__(self) -> str:
        return "Synth(" + ", ".join(f"{k}={v!r}" for k, v in self.as_dict().items()) + ")"

    def __eq__(self, other) -> bool:
        return isinstance(other, Synth) and self.as_dict() == other.as_dict()

    __hash__ = None


def noise_seed(seed: int, index: int, epoch: int) -> int:
    """The Philox seed of the sensor noise of sample ``index`` at ``epoch``: ``mix(mix(mix(mix(tag) ^ seed) ^ index) ^ epoch)`` with
    ``mix`` the splitmix64 step and a tag of this module's own, everything mod 2^64.  The noise is
    ``hdiff_randn_rows(3 H W, this seed, offset = Z_OFFSET)``: it belongs to the sample, not to a place in a batch."""
    for name, v in (("seed", seed), ("index", index), ("epoch", epoch)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"noise_seed: {name} must be an integer, got {v!r}")
    return _splitmix64(_splitmix64(_splitmix64(_splitmix64(_SEED_TAG) ^ (int(seed) & _M64)) ^ (int(index) & _M64)) ^ (int(epoch) & _M64))


def _on_device(name: str, t, dtype) -> None:
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"hdiff: '{name}' lives on {t.device if torch.is_tensor(t) else 'the host'}; the degradation runs on an MI355X "
                           "device tensor (there is deliberately no CPU fallback)")
    if t.dtype != dtype or not t.is_contiguous():
        raise RuntimeError(f"hdiff: '{name}' must be a contiguous {dtype} tensor, got {t.dtype}")


def params(idx: torch.Tensor, *, synth: Synth, seed: int, epoch: int, prob=1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """One ``hdiff_synth_params`` launch on the current stream: ``(table, zseeds)``, float64 ``[B, N_PARAMS]`` and the noise seeds as
    int64 ``[B]`` (the bits of the uint64)."""
    if not isinstance(synth, Synth):
        raise TypeError(f"hdiff: synth must be a Synth, got {type(synth).__name__}")
    _on_device("idx", idx, torch.int64)
    if idx.dim() != 1 or idx.shape[0] < 1:
        raise ValueError(f"hdiff: idx is a 1-d index of at least one sample, got {tuple(idx.shape)}")
    B = int(idx.shape[0])
    table = torch.empty((B, N_PARAMS), dtype=torch.float64, device=idx.device)
    zseeds = torch.empty((B,), dtype=torch.int64, device=idx.device)
    S = synth.settings()
    th = synth.thresholds(prob)
    with torch.cuda.device(idx.device):
        _capi.check(_capi.lib().hdiff_synth_params(
            idx.data_ptr(), B, int(seed) & _M64, int(epoch), C.addressof(S), th["th_select"], th["th_medium"], th["th_exposure"],
            th["th_noise"], table.data_ptr(), zseeds.data_ptr(), torch.cuda.current_stream(idx.device).cuda_stream), "synth_params")
    return table, zseeds


def apply(label: torch.Tensor, table: torch.Tensor, zseeds: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """One ``hdiff_synth_apply`` launch on the current stream: the selected samples of ``out`` are overwritten, the others kept."""
    _on_device("label", label, torch.uint8)
    _on_device("out", out, torch.uint8)
    _on_device("table", table, torch.float64)
    _on_device("zseeds", zseeds, torch.int64)
    if label.dim() != 4 or label.shape[1] != 3 or out.shape != label.shape or out.data_ptr() == label.data_ptr():
        raise ValueError(f"hdiff: label and out are two [B, 3, H, W] arrays of one shape, got {tuple(label.shape)}, {tuple(out.shape)}")
    B, _, H, W = (int(v) for v in label.shape)
    if tuple(table.shape) != (B, N_PARAMS) or tuple(zseeds.shape) != (B,) or B < 1 or not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f"hdiff: {B} images of {H} x {W} take a [{B}, {N_PARAMS}] table and {B} seeds (sides between 1 and {MAX_SIDE}), "
                         f"got {tuple(table.shape)}, {tuple(zseeds.shape)}")
    if not (label.device == out.device == table.device == zseeds.device):
        raise ValueError("hdiff: label, out, table and zseeds live on one device")
    with torch.cuda.device(label.device):
        _capi.check(_capi.lib().hdiff_synth_apply(label.data_ptr(), table.data_ptr(), zseeds.data_ptr(), B, H, W, out.data_ptr(),
                                                  torch.cuda.current_stream(label.device).cuda_stream), "synth_apply")
    return out


def degrade(label_u8: torch.Tensor, idx: torch.Tensor, *, synth: Synth, seed: int, epoch: int, prob=1.0,
            out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(inp_u8, params)``: the two launches on the current stream.  ``label_u8`` is the assembled (and augmented) target batch,
    ``idx`` the samples' indices in the cache.  A sample is synthesised with probability ``prob``; the others keep what ``out`` held
    (a copy of the label when ``out`` is not given)."""
    _on_device("label", label_u8, torch.uint8)
    if torch.is_tensor(idx) and idx.dim() == 1 and int(idx.shape[0]) != int(label_u8.shape[0]):
        raise ValueError(f"hdiff: {int(idx.shape[0])} indices for {int(label_u8.shape[0])} images")
    if out is None:
        out = label_u8.clone()
    table, zseeds = params(idx, synth=synth, seed=seed, epoch=epoch, prob=prob)
    apply(label_u8, table, zseeds, out)
    return out, table


# -- clean images without files --------------------------------------------------------------------------------------------------------
def _bilinear_int(grid: np.ndarray, H: int, W: int) -> np.ndarray:
    """An integer grid ``[..., gh, gw]`` stretched corner to corner over H x W, in integers (round half up)."""
    gh, gw = grid.shape[-2:]
    Dy, Dx = max(H - 1, 1), max(W - 1, 1)
    ny, nx = np.arange(H, dtype=np.int64) * (gh - 1), np.arange(W, dtype=np.int64) * (gw - 1)
    y0, x0 = np.minimum(ny // Dy, gh - 2), np.minimum(nx // Dx, gw - 2)
    fy, fx = (ny - y0 * Dy)[:, None], (nx - x0 * Dx)[None, :]
    g = grid.astype(np.int64)
    p00, p01 = g[..., y0[:, None], x0[None, :]], g[..., y0[:, None], x0[None, :] + 1]
    p10, p11 = g[..., y0[:, None] + 1, x0[None, :]], g[..., y0[:, None] + 1, x0[None, :] + 1]
    acc = (Dy - fy) * ((Dx - fx) * p00 + fx * p01) + fy * ((Dx - fx) * p10 + fx * p11)
    return (2 * acc + Dy * Dx) // (2 * Dy * Dx)


def procedural_scenes(n: int, H: int, W: int, seed: int) -> np.ndarray:
    """``n`` clean images, uint8 ``[n, 3, H, W]``, on the host: a smooth colour gradient between four corner colours, three to six
    filled ellipses and rectangles, and a band-limited texture (a coarse random grid stretched bilinearly).  Integers and a private
    ``numpy`` ``Generator`` per image, keyed on ``(seed, i)``: image ``i`` does not depend on ``n``, and no file is read."""
    n, H, W, seed = int(n), int(H), int(W), int(seed)
    if n < 0 or H < 1 or W < 1 or seed < 0:
        raise ValueError(f"procedural_scenes: n = {n}, H = {H}, W = {W}, seed = {seed}")
    out = np.empty((n, 3, H, W), dtype=np.uint8)
    yy, xx = np.arange(H, dtype=np.int64)[:, None], np.arange(W, dtype=np.int64)[None, :]
    for i in range(n):
        g = np.random.default_rng([seed, i])
        img = _bilinear_int(g.integers(30, 226, (3, 2, 2)), H, W)
        for _ in range(int(g.integers(3, 7))):
            kind = int(g.integers(0, 2))
            cy, cx = int(g.integers(0, H)), int(g.integers(0, W))
            ry, rx = int(g.integers(1, max(H // 3, 1) + 1)), int(g.integers(1, max(W // 3, 1) + 1))
            colour = g.integers(0, 256, 3)
            if kind == 0:
                inside = (xx - cx) ** 2 * ry * ry + (yy - cy) ** 2 * rx * rx <= rx * rx * ry * ry
            else:
                inside = (np.abs(yy - cy) <= ry) & (np.abs(xx - cx) <= rx)
            img = np.where(inside[None], colour[:, None, None], img)
        img = img + _bilinear_int(g.integers(-20, 21, (3, 6, 6)), H, W)
        out[i] = np.clip(img, 0, 255).astype(np.uint8)
    return out
