"""A device-resident cache of a paired image set and a loader that assembles every batch on the device (``csrc/batch_assemble.hip``).

The paired sets are small (LoLI: 485 training pairs, UIEB: 890 images, LSUI: 4 279 pairs = 1.7 GB at 256 x 256), so a split is decoded
and resized ONCE, kept on the card as ``uint8``, and a batch is one kernel launch: a gather of ``idx`` with one geometric transform per
pair -- random crop resized back, horizontal flip, vertical flip, quarter turns -- applied to the degraded image and its reference
alike.  The host path cannot do that: ``datasets._PairedSet.__getitem__`` calls ``transforms`` once per image, so a random transform
given there flips or crops the two images of a pair independently.

The transform of sample ``i`` at epoch ``e`` is drawn from the counter-based Philox generator keyed on ``(seed, e, i)``
(``tests/_augment_def.py`` is the definition, the kernel matches it bit for bit): it does not depend on the batch the sample lands in,
on the batch size or on what ran before, so runs repeat and resume bit for bit.  Colour and intensity are never touched: that would
change the mapping the model is to learn.

  * ``Augment(hflip, vflip, rot90, crop, crop_min)``: validated settings; ``thresholds(H)`` are the integers the kernel takes.
  * ``build_cache(dataset, path=None)`` -> ``PairCache`` (``a``, ``b``, ``names``, ``fingerprint``; ``.to(device)``).
  * ``epoch_indices(n, batch_size, epoch=, seed=, shuffle=, drop_last=)``: the batches of one epoch, on the host.
  * ``DeviceLoader(cache, batch_size, shuffle=, drop_last=, augment=, seed=, synth=, synth_prob=, synth_epoch=)``: ``len``,
    ``set_epoch``, iteration.  ``synth`` (``hdiff_amd/synth.py``) replaces the INPUT of a pair by a synthetic degradation of its
    augmented target: that is not a colour augmentation of a real pair, it is how clean images alone become pairs.
"""
from __future__ import annotations

import copy
import hashlib
import math
import os
from fractions import Fraction
from typing import Dict, List, Optional, Tuple

import torch

from . import _capi

__all__ = ["Augment", "PairCache", "build_cache", "epoch_indices", "DeviceLoader", "assemble", "MAX_SIDE"]

MAX_SIDE = 4096
_ONE = 1 << 32


def _threshold(p) -> int:
    """min(2^32, floor(p 2^32)) in exact integer arithmetic (a float is the rational it stores)."""
    return min(_ONE, math.floor(Fraction(p) * _ONE))


class Augment:
    """The geometric augmentation of a pair: ``hflip`` / ``vflip`` / ``crop`` are probabilities in [0, 1]; ``rot90`` turns the (square)
    pair by a uniformly drawn multiple of 90 degrees; a crop keeps between ``crop_min`` and 1 of the height, uniformly, at the image's
    aspect ratio, at a uniform position, and is magnified back to the full size.  Fractions become integers here and nowhere else."""

    def __init__(self, hflip: float = 0.0, vflip: float = 0.0, rot90: bool = False, crop: float = 0.0, crop_min: float = 1.0):
        for name, p in (("hflip", hflip), ("vflip", vflip), ("crop", crop)):
            if isinstance(p, bool) or not isinstance(p, (int, float, Fraction)) or not (0 <= p <= 1):      # NaN fails the comparison
                raise ValueError(f"Augment: {name} = {p!r}; a probability in [0, 1]")
        if not isinstance(rot90, (bool, int)) or rot90 not in (0, 1):
            raise ValueError(f"Augment: rot90 = {rot90!r}; True or False")
        if isinstance(crop_min, bool) or not isinstance(crop_min, (int, float, Fraction)) or not (0 < crop_min <= 1):
            raise ValueError(f"Augment: crop_min = {crop_min!r}; a fraction of the height in (0, 1]")
        self.hflip, self.vflip, self.rot90, self.crop, self.crop_min = hflip, vflip, bool(rot90), crop, crop_min

    def thresholds(self, H: int) -> Dict[str, int]:
        """``{"th_hflip", "th_vflip", "rot90", "th_crop", "crop_lo_h"}`` for images of height ``H``: what ``hdiff_batch_assemble`` takes."""
        H = int(H)
        if H < 1:
            raise ValueError(f"Augment.thresholds: H = {H}")
        lo_h = min(H, max(1, math.ceil(Fraction(self.crop_min) * H)))
        return {"th_hflip": _threshold(self.hflip), "th_vflip": _threshold(self.vflip), "rot90": int(self.rot90),
                "th_crop": _threshold(self.crop), "crop_lo_h": lo_h}

    def as_dict(self) -> Dict[str, object]:
        return {"hflip": self.hflip, "vflip": self.vflip, "rot90": self.rot90, "crop": self.crop, "crop_min": self.crop_min}

    def __repr__(self) -> str:
        return "Augment(" + ", ".join(f"{k}={v!r}" for k, v in self.as_dict().items()) + ")"

    def __eq__(self, other) -> bool:
        return isinstance(other, Augment) and self.as_dict() == other.as_dict()


_NO_AUGMENT = {"th_hflip": 0, "th_vflip": 0, "rot90": 0, "th_crop": 0}


class PairCache:
    """``a``, ``b``: uint8 ``[N, 3, H, W]`` (``b is a`` when both sides of the set are the same files, or the set is unsupervised);
    ``names``: the file names of the underwater validation split, else ``None``; ``fingerprint``: see ``build_cache``."""

    def __init__(self, a: torch.Tensor, b: torch.Tensor, names: Optional[List[str]], fingerprint: str):
        for t in (a, b):
            if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[1] != 3:
                raise ValueError(f"PairCache: uint8 [N, 3, H, W] arrays, got {t.dtype} {tuple(t.shape)}")
        if a.shape != b.shape or a.device != b.device:
            raise ValueError("PairCache: the two sides differ in shape or device")
        if names is not None and len(names) != a.shape[0]:
            raise ValueError("PairCache: one name per pair")
        self.a, self.b, self.names, self.fingerprint = a, b, names, fingerprint

    def __len__(self) -> int:
        return int(self.a.shape[0])

    def to(self, device) -> "PairCache":
        a = self.a.to(device).contiguous()
        b = a if self.b is self.a else self.b.to(device).contiguous()
        return PairCache(a, b, self.names, self.fingerprint)


def _transform_name(dataset) -> str:
    t = getattr(dataset, "transforms", None)
    if t is None:
        return "default"
    named = t if hasattr(t, "__qualname__") else type(t)
    return f"{getattr(named, '__module__', '?')}.{named.__qualname__}"


def _fingerprint(dataset, shape: Tuple[int, ...]) -> str:
    """sha1 over the two path lists, each file's size and mtime, the item shape and the repr of the transform's qualified name."""
    h = hashlib.sha1()
    for side in (dataset.paths_a, dataset.paths_b if dataset.supervised else dataset.paths_a):
        h.update(f"{len(side)}\n".encode())
        for p in side:
            st = os.stat(p)
            h.update(f"{p}\0{st.st_size}\0{st.st_mtime_ns}\n".encode())
    h.update(repr(tuple(int(v) for v in shape)).encode())
    h.update(repr(_transform_name(dataset)).encode())
    return h.hexdigest()


def _check_item(img, dataset, k: int, side: str, shape) -> None:
    path = (dataset.paths_a if side == "a" else dataset.paths_b)[k]
    if not torch.is_tensor(img) or img.dtype != torch.uint8 or img.dim() != 3 or img.shape[0] != 3:
        what = f"{img.dtype} {tuple(img.shape)}" if torch.is_tensor(img) else type(img).__name__
        raise ValueError(f"build_cache: every item must be a uint8 CHW tensor with 3 channels; {path} gave {what}")
    if shape is not None and tuple(img.shape) != tuple(shape):
        raise ValueError(f"build_cache: every item must have one shape; {path} is {tuple(img.shape)}, the items before it {tuple(shape)}")


def build_cache(dataset, path: Optional[str] = None, *, num_workers: int = 4) -> PairCache:
    """Decode a split once: the items of an ``Underwater_Dataset`` / ``Atmospheric_Dataset``, in order, stacked into a CPU ``PairCache``.

    The set is iterated through a plain ``DataLoader`` (``shuffle=False``, ``drop_last=False``) inside ``torch.random.fork_rng``, so the
    cache holds exactly what the host path yields, whatever ``transforms=`` the set carries, and the caller's random stream does not
    move.  A RANDOM host transform is therefore frozen into the cache: every epoch sees the one draw made here.  Use ``Augment`` for
    augmentation.  When both sides list the same files (UIEB, RUIE, TM-DIED), or the set is unsupervised, each file is decoded once
    and one array is stored (``b is a``).

    With ``path`` the cache is saved there (``torch.save``) and reused by the next call if the fingerprint still matches: a sha1 over
    the two path lists, each file's size and mtime, the item shape (of item 0, decoded for the check) and the transform's qualified
    name.  A stale or unreadable file is rebuilt and overwritten.  Items that are not ``uint8`` CHW of one shape raise ``ValueError``
    naming the first offending file."""
    from torch.utils.data import DataLoader

    n = len(dataset)
    if n < 1:
        raise ValueError(f"build_cache: the set is empty (root '{getattr(dataset, 'root', '?')}')")
    one_sided = (not dataset.supervised) or list(dataset.paths_a) == list(dataset.paths_b)
    with_names = bool(getattr(dataset, "_NAME_WITH_VAL", False)) and dataset.supervised and dataset.task not in ("train", "test")
    names = [p.split("/")[-1] for p in dataset.paths_a] if with_names else None

    one_image = copy.copy(dataset)               # the degraded side alone: each file is decoded once
    one_image.supervised = False
    with torch.random.fork_rng(devices=[]):
        first = one_image[0][0]
        _check_item(first, dataset, 0, "a", None)
        shape = tuple(first.shape)
        fingerprint = _fingerprint(dataset, shape)
        if path is not None and os.path.isfile(path):
            try:
                saved = torch.load(path, map_location="cpu", weights_only=True)
                if saved["fingerprint"] == fingerprint:
                    a = saved["a"]
                    return PairCache(a, a if saved["b"] is None else saved["b"], saved["names"], fingerprint)
            except Exception:       # noqa: BLE001 -- an unreadable cache file is a stale one
                pass
        source = one_image if one_sided else dataset
        a =torch.empty((n,) + shape, dtype=torch.uint8)
        b = a if one_sided else torch.empty((n,) + shape, dtype=torch.uint8)
        loader = DataLoader(source, batch_size=None, shuffle=False, drop_last=False, num_workers=int(num_workers))
        for k, item in enumerate(loader):
            _check_item(item[0], dataset, k, "a", shape)
            a[k] = item[0]
            if not one_sided:
                _check_item(item[1], dataset, k, "b", shape)
                b[k] = item[1]
    cache = PairCache(a, b, names, fingerprint)
    if path is not None:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        torch.save({"a": a, "b": None if b is a else b, "names": names, "fingerprint": fingerprint}, path)
    return cache


def epoch_indices(n: int, batch_size: int, *, epoch: int, seed: int, shuffle: bool, drop_last: bool) -> List[torch.Tensor]:
    """The int64 index batches of one epoch over ``n`` samples, on the host: ``arange`` in order, or with ``shuffle`` a permutation from
    a private ``torch.Generator`` seeded from ``(seed, epoch)``.  The global generators are never touched."""
    n, batch_size = int(n), int(batch_size)
    if n < 0 or batch_size < 1:
        raise ValueError(f"epoch_indices: n = {n}, batch_size = {batch_size}")
    if shuffle:
        g = torch.Generator(device="cpu")
        key = hashlib.sha1(f"hdiff_amd.device_data:{int(seed)}:{int(epoch)}".encode()).digest()
        g.manual_seed(int.from_bytes(key[:8], "little") & (2 ** 63 - 1))
        order = torch.randperm(n, generator=g, dtype=torch.int64)
    else:
        order = torch.arange(n, dtype=torch.int64)
    stop = n - n % batch_size if drop_last else n
    return [order[s:min(s + batch_size, stop)] for s in range(0, stop, batch_size)]


def assemble(a: torch.Tensor, b: torch.Tensor, idx: torch.Tensor, *, seed: int = 0, epoch: int = 0, th_hflip: int = 0, th_vflip: int = 0,
             rot90: int = 0, th_crop: int = 0, crop_lo_h: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """One ``hdiff_batch_assemble`` launch on the current stream: ``(out_a, out_b)``, uint8 ``[len(idx), 3, H, W]``.  ``idx`` is an int64
    device tensor whose entries the CALLER keeps inside ``[0, N)``: the kernel does not check them."""
    for name, t, dtype in (("a", a, torch.uint8), ("b", b, torch.uint8), ("idx", idx, torch.int64)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError(f"hdiff: '{name}' lives on {t.device if torch.is_tensor(t) else 'the host'}; the batch is assembled on an "
                               "MI355X device tensor (there is deliberately no CPU fallback)")
        if t.dtype != dtype or not t.is_contiguous():
            raise RuntimeError(f"hdiff: '{name}' must be a contiguous {dtype} tensor, got {t.dtype}")
    if a.dim() != 4 or a.shape[1] != 3 or a.shape != b.shape or idx.dim() != 1 or not (a.device == b.device == idx.device):
        raise ValueError(f"hdiff: assemble takes [N, 3, H, W] arrays of one shape and device and a 1-d index, got {tuple(a.shape)}, "
                         f"{tuple(b.shape)}, {tuple(idx.shape)}")
    N, _, H, W = (int(v) for v in a.shape)
    B = int(idx.shape[0])
    out_a = torch.empty((B, 3, H, W), dtype=torch.uint8, device=a.device)
    out_b = torch.empty_like(out_a)
    with torch.cuda.device(a.device):
        _capi.check(_capi.lib().hdiff_batch_assemble(
            a.data_ptr(), b.data_ptr(), idx.data_ptr(), B, N, H, W, int(seed) & (2 ** 64 - 1), int(epoch), int(th_hflip), int(th_vflip),
            int(rot90), int(th_crop), H if crop_lo_h is None else int(crop_lo_h), out_a.data_ptr(), out_b.data_ptr(),
            torch.cuda.current_stream(a.device).cuda_stream), "batch_assemble")
    return out_a, out_b


class DeviceLoader:
    """Batches of a device-resident ``PairCache``: iteration yields ``[inp, label]`` uint8 device tensors (``[inp, label, names]`` for a
    cache with names) -- the structure, the order and the bytes that ``DataLoader(dataset, batch_size, drop_last=...)`` over the same
    set yields after ``.to(device)``; with ``augment`` each pair additionally gets its transform of ``(seed, epoch, sample index)``.
    ``augment=None`` still goes through the kernel, with all thresholds 0.  ``set_epoch(e)`` selects the epoch (the shuffle and the
    transforms are functions of it): a resumed run that sets the epoch it continues with draws what the uninterrupted run draws.

    ``__iter__`` draws one ``int64`` from torch's default CPU generator and discards it.  ``DataLoader.__iter__`` does exactly that for
    its base seed, with any ``num_workers``; matching it is what makes a run identical bit for bit when only the loader is switched.

    ``synth`` (a ``synth.Synth``): after the batch is assembled, the input of each sample selected with probability ``synth_prob`` is
    overwritten by the degradation of its (augmented) label, two more launches per batch; the draw is a function of ``(seed, epoch,
    sample index)`` like the transform.  ``synth_epoch`` fixes the epoch of that draw (a validation split is degraded the same way at
    every checkpoint).  With ``synth=None`` the loader makes exactly the launches it makes without the option."""

    def __init__(self, cache: PairCache, batch_size: int, *, shuffle: bool = False, drop_last: bool = True,
                 augment: Optional[Augment] = None, seed: int = 0, synth=None, synth_prob=1.0, synth_epoch: Optional[int] = None):
        if not cache.a.is_cuda:
            raise RuntimeError(f"hdiff: DeviceLoader needs a cache on the MI355X (cache.to(device)); this one lives on {cache.a.device} "
                               "(there is deliberately no CPU fallback)")
        if augment is not None and not isinstance(augment, Augment):
            raise TypeError(f"DeviceLoader: augment must be an Augment or None, got {type(augment).__name__}")
        N, _, H, W = (int(v) for v in cache.a.shape)
        if N < 1 or not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
            raise ValueError(f"DeviceLoader: {N} images of {H} x {W}; at least one, sides between 1 and {MAX_SIDE}")
        if int(batch_size) < 1:
            raise ValueError(f"DeviceLoader: batch_size = {batch_size}")
        self.cache, self.batch_size, self.shuffle, self.drop_last = cache, int(batch_size), bool(shuffle), bool(drop_last)
        self.augment, self.seed, self.epoch = augment, int(seed), 0
        self._settings = dict(_NO_AUGMENT, crop_lo_h=H) if augment is None else augment.thresholds(H)
        if self._settings["rot90"] and H != W:
            raise ValueError(f"DeviceLoader: rot90 needs square images, the cache holds {H} x {W}")
        if synth is not None:
            from .synth import Synth
            if not isinstance(synth, Synth):
                raise TypeError(f"DeviceLoader: synth must be a Synth or None, got {type(synth).__name__}")
            synth.thresholds(synth_prob)                      # refuses a probability outside [0, 1]
            if synth_epoch is not None and not 0 <= int(synth_epoch) < 2 ** 31:
                raise ValueError(f"DeviceLoader: synth_epoch = {synth_epoch}; between 0 and 2^31 - 1")
        self.synth, self.synth_prob = synth, synth_prob
        self.synth_epoch = None if synth_epoch is None else int(synth_epoch)

    def __len__(self) -> int:
        n = len(self.cache)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def set_epoch(self, epoch: int) -> None:
        if not 0 <= int(epoch) < 2 ** 31:
            raise ValueError(f"DeviceLoader.set_epoch: epoch = {epoch}; between 0 and 2^31 - 1")
        self.epoch = int(epoch)

    def __iter__(self):
        torch.empty((), dtype=torch.int64).random_()          # what DataLoader.__iter__ draws for its base seed
        epoch = self.epoch
        batches = epoch_indices(len(self.cache), self.batch_size, epoch=epoch, seed=self.seed, shuffle=self.shuffle,
                                drop_last=self.drop_last)
        if not batches:
            return
        order = torch.cat(batches)                              # every index is inside [0, N): a permutation or arange
        on_device = order.to(self.cache.a.device)
        start = 0
        for batch in batches:
            idx = on_device[start:start + len(batch)]
            start += len(batch)
            out_a, out_b = assemble(self.cache.a, self.cache.b, idx, seed=self.seed, epoch=epoch, **self._settings)
            if self.synth is not None:
                from .synth import degrade
                degrade(out_b, idx, synth=self.synth, seed=self.seed, epoch=epoch if self.synth_epoch is None else self.synth_epoch,
                        prob=self.synth_prob, out=out_a)
            if self.cache.names is None:
                yield [out_a, out_b]
            else:
                yield [out_a, out_b, tuple(self.cache.names[i] for i in batch.tolist())]      # default_collate keeps a tuple
