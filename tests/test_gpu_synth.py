"""The synthetic degradation on the GPU (csrc/synth_degrade.hip, hdiff_amd/synth.py) against its definition (tests/_synth_def.py): the
parameter table and the noise seeds bit for bit, the noise equal to hdiff_randn_rows', the bytes equal everywhere (no excluded pixels:
every fixture keeps a rounding margin of 1e-9, far above what a double exp, pow or cos a few ulp off can move); selection, the aliased
cache, sample independence, stream capture and DeviceLoader with and without the option."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hdiff_amd  # noqa: E402
from hdiff_amd import _capi  # noqa: E402
from hdiff_amd import device_data as DD  # noqa: E402
from hdiff_amd import synth as SY  # noqa: E402
import _synth_def as SD  # noqa: E402
import _synth_fixtures as FX  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning"), pytest.mark.filterwarnings("ignore::UserWarning")]
DEV = "cuda:0"
ONE = 1 << 32
M64 = (1 << 64) - 1


def dev_idx(values):
    return torch.tensor(list(values), dtype=torch.int64, device=DEV)


def noise_rows(zseeds: torch.Tensor, n_per: int) -> np.ndarray:
    """hdiff_randn_rows under the given seeds at the degradation's offset: float32 [B, n_per]."""
    out = torch.empty(zseeds.numel(), n_per, dtype=torch.float32, device=DEV)
    _capi.check(_capi.lib().hdiff_randn_rows(out.data_ptr(), int(zseeds.numel()), n_per, zseeds.data_ptr(), C.c_uint64(SY.Z_OFFSET),
                                             torch.cuda.current_stream().cuda_stream), "randn_rows")
    return out.cpu().numpy()


def bits(x: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


# -- 1. the kernels against the definition --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixture", FX.fixtures(), ids=lambda f: f[0])
def test_kernels_equal_the_definition(fixture):
    name, variant, H, W, idx, epoch = fixture
    s = FX.VARIANTS[variant]
    a = FX.cache_images(H, W)
    da = torch.from_numpy(a).to(DEV)
    didx = dev_idx(idx)
    inp, label = DD.assemble(da, da, didx, seed=FX.SEED, epoch=epoch)                   # a clean-only cache: b is a
    assert np.array_equal(label.cpu().numpy(), a[list(idx)])

    table, zseeds = SY.params(didx, synth=s, seed=FX.SEED, epoch=epoch)
    want_table = SD.param_table(FX.SEED, epoch, idx, FX.settings_of(s), **s.thresholds())
    assert np.array_equal(bits(table.cpu().numpy()), bits(want_table)), name                           # bit for bit
    assert [int(v) & M64 for v in zseeds.tolist()] == [SD.noise_seed(FX.SEED, i, epoch) for i in idx]

    z = noise_rows(zseeds, 3 * H * W).reshape(len(idx), 3, H, W)
    want, margin = SD.degrade(a[list(idx)], want_table, a[list(idx)], z)
    if variant in FX.NOISY:                     # the noise-free fixtures are checked on the host; these need the device's z
        assert margin >= FX.MARGIN, (name, margin)
    SY.apply(label, table, zseeds, inp)
    got = inp.cpu().numpy()
    assert np.array_equal(got, want), (name, int((got != want).sum()))
    assert np.array_equal(label.cpu().numpy(), a[list(idx)])                            # the label is read, never written
    if H * W >= 15:
        assert not np.array_equal(got, a[list(idx)])                                    # and the stage did something
    # the two launches in one call
    both, table2 = SY.degrade(label, didx, synth=s, seed=FX.SEED, epoch=epoch)
    assert np.array_equal(both.cpu().numpy(), want) and torch.equal(table2, table)


def test_noise_is_the_sample_stream_of_randn_rows():
    """With J = 128/255, no medium, unit exposure, shot = 0 and read = 1/255 the byte is floor(128.5 + z): every z is read back to within
    the rounding, so a wrong element, quad or seed cannot hide, and only +, *, / and sqrt are involved, which round alike everywhere.
    W = 13 puts every row's start at another place in a quad.  The seeds are the host's, not the kernel's."""
    H, W, idx, epoch = 8, 13, FX.IDX7, 2 ** 31 - 1
    r = 1.0 / 255.0
    s = SY.Synth(read=r)
    didx = dev_idx(idx)
    label = torch.full((len(idx), 3, H, W), 128, dtype=torch.uint8, device=DEV)
    out, table = SY.degrade(label, didx, synth=s, seed=5, epoch=epoch)
    seeds = [SY.noise_seed(5, i, epoch) for i in idx]
    zseeds = torch.tensor([v - (1 << 64) if v >= 1 << 63 else v for v in seeds], dtype=torch.int64, device=DEV)
    z = noise_rows(zseeds, 3 * H * W).reshape(len(idx), 3, H, W).astype(np.float64)
    want = np.floor(255.0 * np.clip(128.0 / 255.0 + np.sqrt(r * r) * z, 0.0, 1.0) + 0.5).astype(np.uint8)
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(out[1].cpu().numpy(), out[3].cpu().numpy()) and len(np.unique(want)) > 4       # idx[1] == idx[3]


# -- 2. selection ---------------------------------------------------------------------------------------------------------------------
def test_selection_keeps_or_replaces_whole_samples():
    H, W, epoch = 8, 13, 1
    rng = np.random.default_rng(3)
    a, b = (rng.integers(0, 256, (FX.N_CACHE, 3, H, W), dtype=np.uint8) for _ in range(2))
    da, db = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    idx = tuple(range(FX.N_CACHE)) + FX.IDX7
    didx = dev_idx(idx)
    s = FX.VARIANTS["all"]
    inp0, label = DD.assemble(da, db, didx, seed=FX.SEED, epoch=epoch)
    kept, table = SY.degrade(label, didx, synth=s, seed=FX.SEED, epoch=epoch, prob=0.0, out=inp0.clone())
    assert torch.equal(kept, inp0) and not table[:, 0].any()                             # prob = 0: the bytes of assemble
    mixed, table = SY.degrade(label, didx, synth=s, seed=FX.SEED, epoch=epoch, prob=0.5, out=inp0.clone())
    want_table = SD.param_table(FX.SEED, epoch, idx, FX.settings_of(s), **s.thresholds(0.5))
    assert np.array_equal(bits(table.cpu().numpy()), bits(want_table))
    selected = want_table[:, SD.SELECTED] != 0
    assert 0 < selected.sum() < len(idx)
    full, _ = SY.degrade(label, didx, synth=s, seed=FX.SEED, epoch=epoch, prob=1.0, out=inp0.clone())
    for j in range(len(idx)):
        assert torch.equal(mixed[j], full[j] if selected[j] else inp0[j]), j
        assert not torch.equal(full[j], inp0[j])
    assert torch.equal(label, db[didx])


# -- 3. sample independence, stream capture -------------------------------------------------------------------------------------------
def test_a_sample_does_not_depend_on_its_batch_and_the_launches_are_capturable():
    H, W, epoch = 8, 13, 2
    a = FX.cache_images(H, W)
    da = torch.from_numpy(a).to(DEV)
    s = FX.VARIANTS["mixed"]

    def run(values):
        didx = dev_idx(values)
        inp, label = DD.assemble(da, da, didx, seed=11, epoch=epoch)
        return SY.degrade(label, didx, synth=s, seed=11, epoch=epoch, out=inp)[0].cpu().numpy()

    alone, first, last = run([3]), run([3, 0, 1, 2, 4, 0, 1]), run([0, 1, 2, 4, 0, 1, 3])
    assert np.array_equal(alone[0], first[0]) and np.array_equal(alone[0], last[6]) and np.array_equal(first[1], last[0])
    assert np.array_equal(last, run([0, 1, 2, 4, 0, 1, 3]))

    # both launches captured once and replayed twice (everything allocated before the capture)
    lib = hdiff_amd.lib()
    didx = dev_idx([0, 1, 2, 4, 0, 1, 3])
    label = da[didx].contiguous()
    out = torch.zeros_like(label)
    table = torch.zeros(7, SY.N_PARAMS, dtype=torch.float64, device=DEV)
    zseeds = torch.zeros(7, dtype=torch.int64, device=DEV)
    S, th = s.settings(), s.thresholds()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        stream = torch.cuda.current_stream().cuda_stream
        _capi.check(lib.hdiff_synth_params(didx.data_ptr(), 7, 11, epoch, C.addressof(S), th["th_select"], th["th_medium"],
                                           th["th_exposure"], th["th_noise"], table.data_ptr(), zseeds.data_ptr(), stream), "synth_params")
        _capi.check(lib.hdiff_synth_apply(label.data_ptr(), table.data_ptr(), zseeds.data_ptr(), 7, H, W, out.data_ptr(), stream),
                    "synth_apply")
    for _ in range(2):
        out.copy_(label)
        table.zero_()
        zseeds.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), last)


# -- 4. the loader --------------------------------------------------------------------------------------------------------------------
def test_device_loader_with_synth_repeats_within_an_epoch_and_moves_between_epochs():
    H, W = 8, 13
    a = FX.cache_images(H, W)
    clean = torch.from_numpy(a)
    cache = DD.PairCache(clean, clean, None, "x").to(DEV)
    assert cache.b is cache.a
    s = FX.VARIANTS["all"]
    loader = DD.DeviceLoader(cache, 4, shuffle=True, drop_last=False, augment=DD.Augment(hflip=0.5, vflip=0.5), seed=21, synth=s)
    loader.set_epoch(3)
    once, twice = [[t.cpu().numpy() for t in batch] for batch in loader], [[t.cpu().numpy() for t in batch] for batch in loader]
    assert len(once) == len(twice) == 3
    batches = DD.epoch_indices(FX.N_CACHE, 4, epoch=3, seed=21, shuffle=True, drop_last=False)
    for (inp, label), (inp2, label2), idx in zip(once, twice, batches):
        assert np.array_equal(inp, inp2) and np.array_equal(label, label2)
        assert not np.array_equal(inp, label)
        plain_inp, plain_label = DD.assemble(cache.a, cache.b, idx.to(DEV), seed=21, epoch=3, **loader._settings)
        assert np.array_equal(label, plain_label.cpu().numpy())                          # the target is the augmented clean image ...
        want, _ = SY.degrade(plain_label, idx.to(DEV), synth=s, seed=21, epoch=3)
        assert np.array_equal(inp, want.cpu().numpy())                                   # ... and the input is drawn from it
    assert torch.equal(cache.a.cpu(), torch.from_numpy(a))                               # the cache itself is never written
    # one sample under one transform-free loader: its input differs between two epochs, and a fixed synth_epoch pins it
    free = DD.DeviceLoader(cache, FX.N_CACHE, seed=21, synth=s)
    pinned = DD.DeviceLoader(cache, FX.N_CACHE, seed=21, synth=s, synth_epoch=0)
    got = {}
    for e in (0, 1):
        free.set_epoch(e)
        pinned.set_epoch(e)
        got[e] = (next(iter(free))[0].cpu().numpy(), next(iter(pinned))[0].cpu().numpy())
    assert not np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]) and np.array_equal(got[0][0], got[0][1])
    with pytest.raises(TypeError):
        DD.DeviceLoader(cache, 2, synth=s.as_dict())
    with pytest.raises(ValueError):
        DD.DeviceLoader(cache, 2, synth=s, synth_prob=1.5)
    with pytest.raises(ValueError):
        DD.DeviceLoader(cache, 2, synth=s, synth_epoch=2 ** 31)


def test_device_loader_without_synth_yields_the_bytes_of_assemble():
    H, W = 8, 13
    rng = np.random.default_rng(5)
    a, b = (rng.integers(0, 256, (FX.N_CACHE, 3, H, W), dtype=np.uint8) for _ in range(2))
    cache = DD.PairCache(torch.from_numpy(a), torch.from_numpy(b), None, "x").to(DEV)
    aug = DD.Augment(hflip=0.5, vflip=0.5, crop=0.5, crop_min=0.5)
    for kw in (dict(), dict(synth=None), dict(synth=FX.VARIANTS["all"], synth_prob=0.0)):
        loader = DD.DeviceLoader(cache, 4, shuffle=True, drop_last=True, augment=aug, seed=8, **kw)
        loader.set_epoch(2)
        batches = DD.epoch_indices(FX.N_CACHE, 4, epoch=2, seed=8, shuffle=True, drop_last=True)
        got = list(loader)
        assert len(got) == len(batches) == 2
        for (inp, label), idx in zip(got, batches):
            want_a, want_b = DD.assemble(cache.a, cache.b, idx.to(DEV), seed=8, epoch=2, **aug.thresholds(H))
            assert torch.equal(inp, want_a) and torch.equal(label, want_b)
