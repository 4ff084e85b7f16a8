"""Host-side tests of the device-resident paired cache (hdiff_amd/device_data.py, csrc/batch_assemble.hip; no GPU): the Philox
transcription, the integer definition of the augmentation (tests/_augment_def.py), the parameters drawn per sample, what the C entry
refuses, the cache and its fingerprint, the epoch's index batches and the driver's data plan."""
import ctypes as C
import os
import re
import subprocess
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
from hdiff_amd.datasets import Atmospheric_Dataset, Underwater_Dataset  # noqa: E402
from hdiff_amd.diffusion import Train as TR  # noqa: E402
import _augment_def as AD  # noqa: E402

ONE = 1 << 32


# -- 1. Philox ----------------------------------------------------------------------------------------------------------------------
PHILOX_VECTORS = (
    ((0, 0), (0, 0, 0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 2, (0xffffffff,) * 4, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0xa4093822, 0x299f31d0), (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


@pytest.mark.parametrize("key,counter,want", PHILOX_VECTORS)
def test_philox_vectors(key, counter, want):
    assert AD.philox_raw(key, counter) == want
    seed = key[0] | (key[1] << 32)                     # the layout of csrc/philox.h: key = the halves of the seed, counter = two words
    assert AD.philox4x32_10(seed, counter[0] | (counter[1] << 32), counter[2] | (counter[3] << 32)) == want


# -- 2. the library ---------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hdiff.h")).read(), flags=re.S)
    assert "hdiff_batch_assemble" in set(re.findall(r"\b(hdiff_[a-z0-9_]+)\s*\(", text))
    assert "hdiff_batch_assemble" in _capi.EXPORTED_SYMBOLS
    lib = hdiff_amd.lib()
    assert lib.hdiff_abi_version() == 6
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "hdiff_batch_assemble" in set(re.findall(r" T (hdiff_[a-z0-9_]+)", out))


def test_argument_validation_needs_no_gpu():
    lib = hdiff_amd.lib()
    p = 8          # any non-null address: validation returns before anything is read or launched

    def call(a=p, b=p, idx=p, B=2, N=5, H=16, W=16, seed=0, epoch=0, th_h=0, th_v=0, rot90=0, th_c=0, lo_h=16, out_a=p, out_b=p):
        return lib.hdiff_batch_assemble(a, b, idx, B, N, H, W, seed, epoch, th_h, th_v, rot90, th_c, lo_h, out_a, out_b, None)

    def refused(rc, word):
        assert rc == -1
        assert word in lib.hdiff_last_error().decode(), lib.hdiff_last_error()

    for name in ("a", "b", "idx", "out_a", "out_b"):
        refused(call(**{name: None}), "null pointer")
    refused(call(B=0), "B = 0")
    refused(call(B=-2), "B = -2")
    refused(call(N=0), "N = 0")
    for bad in (dict(H=0, lo_h=1), dict(H=4097, lo_h=1), dict(W=0), dict(W=4097), dict(W=-1)):
        refused(call(**bad), "between 1 and 4096")
    for name in ("th_h", "th_v", "th_c"):
        refused(call(**{name: ONE + 1}), "at most 2^32")
    refused(call(lo_h=0), "crop_lo_h = 0")
    refused(call(lo_h=17), "crop_lo_h = 17")
    refused(call(H=16, W=20, rot90=1), "square")
    refused(call(epoch=2 ** 31), "below 2^31")
    refused(call(epoch=2 ** 32 - 1), "below 2^31")


def test_module_refuses_cpu_tensors():
    a = torch.zeros(2, 3, 4, 4, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="MI355X"):
        DD.assemble(a, a, torch.zeros(1, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="MI355X"):
        DD.DeviceLoader(DD.PairCache(a, a, None, "x"), 2)


# -- 3. the definition --------------------------------------------------------------------------------------------------------------
def image(H, W, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (3, H, W), dtype=np.uint8)


def whole(H, W, **kw):
    return AD.Params(**{**dict(hflip=False, vflip=False, k=0, cropped=False, y0=0, x0=0, ch=H, cw=W), **kw})


def test_definition_identity_flips_and_turns():
    for H, W in ((1, 1), (5, 7), (13, 20), (16, 16)):
        img = image(H, W)
        assert np.array_equal(AD.apply(img, whole(H, W)), img)
        assert np.array_equal(AD.apply(img, whole(H, W, hflip=True)), np.flip(img, 2))
        assert np.array_equal(AD.apply(img, whole(H, W, vflip=True)), np.flip(img, 1))
        out_a, out_b = AD.assemble_def(img[None], img[None, :, ::-1].copy(), [0, 0], seed=3, epoch=1)       # all thresholds 0
        assert np.array_equal(out_a, np.stack([img, img])) and np.array_equal(out_b, np.stack([img[:, ::-1]] * 2))
    img = image(16, 16)
    for k in (1, 2, 3):
        assert np.array_equal(AD.apply(img, whole(16, 16, k=k)), np.rot90(img, k, axes=(1, 2)))
        both = AD.apply(img, whole(16, 16, hflip=True, vflip=True, k=k))
        assert np.array_equal(both, np.rot90(np.flip(np.flip(img, 2), 1), k, axes=(1, 2)))
    # all four together: crop-resize, hflip, vflip, then the turn
    p = whole(16, 16, hflip=True, vflip=True, k=3, cropped=True, y0=2, x0=5, ch=9, cw=9)
    want = np.rot90(AD.crop_resize(img, 2, 5, 9, 9)[:, :, ::-1][:, ::-1, :], 3, axes=(1, 2))
    assert np.array_equal(AD.apply(img, p), want)
    assert not np.array_equal(want, np.rot90(AD.crop_resize(img[:, ::-1, ::-1], 2, 5, 9, 9), 3, axes=(1, 2)))   # the order matters


def test_definition_crop_resize():
    for H, W in ((1, 1), (5, 7), (13, 20), (16, 16)):
        img = image(H, W, 1)
        assert np.array_equal(AD.crop_resize(img, 0, 0, H, W), img)                    # a box that is the image: exactly the identity
    row = np.zeros((1, 8), dtype=np.uint8)
    row[0, 2:6] = (0, 100, 200, 40)
    assert AD.crop_resize(row, 0, 2, 1, 4).tolist() == [[0, 25, 75, 125, 175, 160, 80, 40]]
    col = np.ascontiguousarray(row.T)
    assert AD.crop_resize(col, 2, 0, 4, 1)[:, 0].tolist() == [0, 25, 75, 125, 175, 160, 80, 40]
    img = image(13, 20, 2)
    assert np.array_equal(AD.crop_resize(img, 4, 11, 1, 1), np.broadcast_to(img[:, 4:5, 11:12], img.shape))      # a 1 x 1 box
    rng = np.random.default_rng(3)
    for _ in range(50):                                                                  # within the min and max of the box
        ch, cw = int(rng.integers(1, 14)), int(rng.integers(1, 21))
        y0, x0 = int(rng.integers(0, 13 - ch + 1)), int(rng.integers(0, 20 - cw + 1))
        out = AD.crop_resize(img, y0, x0, ch, cw)
        box = img[:, y0:y0 + ch, x0:x0 + cw]
        assert (out >= box.min(axis=(1, 2), keepdims=True)).all() and (out <= box.max(axis=(1, 2), keepdims=True)).all()
    # the floor of a negative numerator is a true floor: the first output of a small box sits on the box's first source, weight 0 of
    # the (clamped) tap before it
    t0, t1, f = AD.axis(8, 2, 3)
    assert t0[0] == t1[0] == 3 and 0 < f[0] < 16 and t0[-1] == t1[-1] == 4
    # 64 bits: the largest accumulator of a 4096-wide image does not fit 32
    assert (2 * 4096) ** 2 * 255 > 2 ** 32


def test_a_constant_image_stays_constant():
    flat = np.full((3, 13, 13), 77, dtype=np.uint8)
    for i in range(200):
        p = AD.draw(11, i % 4, i, 13, 13, ONE // 2, ONE // 2, True, ONE // 2, 1)
        assert (AD.apply(flat, p) == 77).all(), p


# -- 4. the parameters --------------------------------------------------------------------------------------------------------------
def test_parameters_stay_inside_the_image():
    for H in (1, 5, 13, 16, 20):
        for W in (1, 5, 13, 16, 20):
            for lo_h in (1, H):
                seen = set()
                for i in range(1000):
                    p = AD.draw(7, 2, i, H, W, 0, 0, False, ONE, lo_h)
                    assert p.cropped and lo_h <= p.ch <= H and 1 <= p.cw <= W
                    assert 0 <= p.y0 <= H - p.ch and 0 <= p.x0 <= W - p.cw
                    assert p.cw == min(max((2 * p.ch * W + H) // (2 * H), 1), W)
                    seen.add(p.ch)
                assert seen == set(range(lo_h, H + 1))                                  # every height is drawn


def test_probabilities_one_and_zero_and_the_key():
    always = [AD.draw(1, 0, i, 16, 16, ONE, ONE, True, ONE, 8) for i in range(300)]
    assert all(p.hflip and p.vflip and p.cropped for p in always) and {p.k for p in always} == {0, 1, 2, 3}
    never = [AD.draw(1, 0, i, 16, 16, 0, 0, False, 0, 8) for i in range(300)]
    assert all(p == whole(16, 16) for p in never)
    half = [AD.draw(1, 0, i, 16, 16, ONE // 2, ONE // 2, True, ONE // 2, 8) for i in range(1000)]
    for field in ("hflip", "vflip", "cropped"):
        assert 400 < sum(getattr(p, field) for p in half) < 600                         # 6 sigma of a fair coin is 95
    s = 0x1234
    def params(seed, epoch):
        return [AD.draw(seed, epoch, i, 16, 16, ONE // 2, ONE // 2, True, ONE // 2, 8) for i in range(64)]
    assert params(s, 0) == params(s, 0)
    assert params(s, 0) != params(s, 1)
    assert params(s, 0) != params(s + 2 ** 32, 0)                                      # the high key word is used
    assert AD.draw(s, 2 ** 31 - 1, 5, 16, 16, ONE, 0, False, 0, 16).hflip


def test_augment_thresholds_and_validation():
    th = DD.Augment(hflip=0.5, vflip=1.0, rot90=True, crop=0.25, crop_min=0.5).thresholds(13)
    assert th == {"th_hflip": ONE // 2, "th_vflip": ONE, "rot90": 1, "th_crop": ONE // 4, "crop_lo_h": 7}
    assert DD.Augment().thresholds(16) == {"th_hflip": 0, "th_vflip": 0, "rot90": 0, "th_crop": 0, "crop_lo_h": 16}
    assert DD.Augment(hflip=0.1).thresholds(4)["th_hflip"] == int(0.1 .as_integer_ratio()[0] * ONE // 0.1 .as_integer_ratio()[1])
    assert DD.Augment(crop_min=1e-9).thresholds(5)["crop_lo_h"] == 1 and DD.Augment(crop_min=0.2).thresholds(5)["crop_lo_h"] == 2
    for bad in (dict(hflip=-0.1), dict(vflip=1.5), dict(crop=float("nan")), dict(crop_min=0.0), dict(crop_min=1.01), dict(rot90=2),
                dict(hflip="0.5"), dict(crop=True)):
        with pytest.raises(ValueError):
            DD.Augment(**bad)


# -- 5. the cache -----------------------------------------------------------------------------------------------------------------
def as_is(image):
    """The sets' ``transforms=`` without the 256 x 256 resize: HWC uint8 array -> {"image": CHW uint8 tensor}."""
    return {"image": torch.from_numpy(np.ascontiguousarray(image)).permute(2, 0, 1)}


def write_image(path, rng, size=16):
    from PIL import Image
    low = rng.integers(0, 256, (4, 4, 3), dtype=np.uint8)
    Image.fromarray(low).resize((size, size), Image.BILINEAR).save(str(path))


@pytest.fixture()
def data_root(tmp_path):
    """HICRD + LoLI + UIEB in the reference's layout, 16 x 16: 4 train / 2 test / 3 val pairs of HICRD, 4 / 2 of LoLI, 10 UIEB files."""
    root = tmp_path / "data"
    rng = np.random.default_rng(9)
    for sub, ext, count in (("Train/low", "jpg", 4), ("Train/high", "jpg", 4), ("Test/low", "jpg", 2), ("Test/high", "jpg", 2),
                            ("Train/trainA_paired", "png", 4), ("Train/trainB_paired", "png", 4), ("Test/testA", "png", 2),
                            ("Test/testB", "png", 2), ("Val/valA", "png", 3), ("Val/valB", "png", 3), ("train", "png", 10)):
        os.makedirs(root / sub)
        for i in range(count):
            write_image(root / sub / f"img{i}.{ext}", rng)
    return str(root)


def stacked(dataset):
    items = [dataset[i] for i in range(len(dataset))]
    return torch.stack([it[0] for it in items]), torch.stack([it[1] for it in items])


def test_cache_equals_the_items_is_reused_and_rebuilt(data_root, tmp_path):
    for data in (Underwater_Dataset("HICRD", transforms=as_is, task="train", root=data_root),
                 Atmospheric_Dataset("LoLI", transforms=as_is, task="test", root=data_root)):
        want_a, want_b = stacked(data)
        path = str(tmp_path / "cache" / f"{len(data)}.pt")
        state = torch.get_rng_state()
        cache = DD.build_cache(data, path, num_workers=0)
        assert torch.equal(torch.get_rng_state(), state)                                # the caller's stream did not move
        assert cache.a.dtype == torch.uint8 and tuple(cache.a.shape) == (len(data), 3, 16, 16) and cache.b is not cache.a
        assert torch.equal(cache.a, want_a) and torch.equal(cache.b, want_b) and not torch.equal(cache.a, cache.b)
        assert cache.names is None and len(cache) == len(data) and re.fullmatch(r"[0-9a-f]{40}", cache.fingerprint)
        written = os.path.getmtime(path)
        again = DD.build_cache(data, path, num_workers=0)                                # reloaded, not rebuilt
        assert torch.equal(again.a, want_a) and torch.equal(again.b, want_b) and again.fingerprint == cache.fingerprint
        assert os.path.getmtime(path) == written
        with_workers = DD.build_cache(data, num_workers=2)                               # no file; worker processes give the same
        assert torch.equal(with_workers.a, want_a) and torch.equal(with_workers.b, want_b)
        assert torch.equal(torch.get_rng_state(), state)
        # one source file rewritten: another fingerprint, the cache rebuilt and the file overwritten
        victim = data.paths_b[1]
        write_image(victim, np.random.default_rng(77))
        st = os.stat(victim)
        os.utime(victim, ns=(st.st_atime_ns, st.st_mtime_ns + 5_000_000_000))
        fresh = DD.build_cache(data, path, num_workers=0)
        new_a, new_b = stacked(data)
        assert fresh.fingerprint != cache.fingerprint and not torch.equal(new_b, want_b)
        assert torch.equal(fresh.a, new_a) and torch.equal(fresh.b, new_b)
        assert torch.load(path, weights_only=True)["fingerprint"] == fresh.fingerprint


def test_cache_of_a_one_sided_set_stores_one_array_and_the_validation_split_has_names(data_root):
    uieb = Underwater_Dataset("UIEB", transforms=as_is, task="train", root=data_root)
    cache = DD.build_cache(uieb, num_workers=0)
    assert cache.b is cache.a and len(cache) == len(uieb) == 7 and torch.equal(cache.a, stacked(uieb)[0])
    unsup = Atmospheric_Dataset("LoLI", transforms=as_is, task="train", supervised=False, root=data_root)
    cache = DD.build_cache(unsup, num_workers=0)
    assert cache.b is cache.a and torch.equal(cache.a, stacked(unsup)[0])
    val = Underwater_Dataset("HICRD", transforms=as_is, task="val", root=data_root)
    cache = DD.build_cache(val, num_workers=0)
    assert cache.names == [val[i][2] for i in range(len(val))] == ["img0.png", "img1.png", "img2.png"]
    assert DD.build_cache(Underwater_Dataset("HICRD", transforms=as_is, task="test", root=data_root), num_workers=0).names is None
    moved = cache.to("cpu")
    assert torch.equal(moved.a, cache.a) and moved.names == cache.names and moved.fingerprint == cache.fingerprint


def other_transform(image):
    return as_is(image)


def test_cache_fingerprint_names_the_transform_and_mixed_shapes_name_a_file(data_root, tmp_path):
    data = Atmospheric_Dataset("LoLI", transforms=as_is, task="train", root=data_root)
    same = Atmospheric_Dataset("LoLI", transforms=other_transform, task="train", root=data_root)
    assert DD.build_cache(data, num_workers=0).fingerprint != DD.build_cache(same, num_workers=0).fingerprint
    write_image(data.paths_b[2], np.random.default_rng(5), size=12)
    with pytest.raises(ValueError, match=re.escape(data.paths_b[2])):
        DD.build_cache(data, str(tmp_path / "c.pt"), num_workers=0)
    assert not os.path.exists(tmp_path / "c.pt")
    floats = Atmospheric_Dataset("LoLI", transforms=lambda image: {"image": as_is(image)["image"].float()}, task="test", root=data_root)
    with pytest.raises(ValueError, match=re.escape(floats.paths_a[0])):
        DD.build_cache(floats, num_workers=0)


# -- 6. epoch_indices -------------------------------------------------------------------------------------------------------------
def test_epoch_indices():
    state = torch.get_rng_state()
    got = DD.epoch_indices(7, 3, epoch=0, seed=0, shuffle=False, drop_last=True)
    assert [b.tolist() for b in got] == [[0, 1, 2], [3, 4, 5]] and all(b.dtype == torch.int64 for b in got)
    got = DD.epoch_indices(7, 3, epoch=4, seed=9, shuffle=False, drop_last=False)
    assert [b.tolist() for b in got] == [[0, 1, 2], [3, 4, 5], [6]]
    assert DD.epoch_indices(2, 3, epoch=0, seed=0, shuffle=False, drop_last=True) == []
    flat = lambda **kw: torch.cat(DD.epoch_indices(50, 4, drop_last=False, shuffle=True, **kw)).tolist()      # noqa: E731
    first = flat(epoch=0, seed=1)
    assert sorted(first) == list(range(50)) and first != list(range(50))
    assert flat(epoch=0, seed=1) == first and flat(epoch=1, seed=1) != first and flat(epoch=0, seed=2) != first
    dropped = DD.epoch_indices(50, 4, epoch=0, seed=1, shuffle=True, drop_last=True)
    assert len(dropped) == 12 and torch.cat(dropped).tolist() == first[:48]
    assert torch.equal(torch.get_rng_state(), state)                                    # the global generator is left alone


# -- 7. the driver's data plan ----------------------------------------------------------------------------------------------------
def test_data_plan():
    base = dict(output_path="out", seed=3)
    plan = TR.data_plan(base)
    assert plan == {"device_cache": False, "cache_dir": os.path.join("out", "cache"), "augment": None, "shuffle": False, "data_seed": 3}
    assert TR.data_plan(dict(output_path="out"))["data_seed"] == 0 and TR.data_plan(dict(output_path="out", seed=None))["data_seed"] == 0
    full = TR.data_plan(dict(base, device_cache=True, cache_dir="elsewhere", shuffle=True, data_seed=2 ** 63 + 5,
                             augment=dict(hflip=0.5, vflip=0.5, rot90=True, crop=0.5, crop_min=0.5)))
    assert full["device_cache"] and full["cache_dir"] == "elsewhere" and full["shuffle"] and full["data_seed"] == 2 ** 63 + 5
    assert full["augment"] == DD.Augment(hflip=0.5, vflip=0.5, rot90=True, crop=0.5, crop_min=0.5)
    given = DD.Augment(hflip=1.0)
    assert TR.data_plan(dict(base, device_cache=True, augment=given))["augment"] is given
    for bad in (dict(augment=dict(hflip=0.5)), dict(augment=DD.Augment()), dict(shuffle=True)):
        with pytest.raises(ValueError, match="host transforms cannot be paired"):
            TR.data_plan(dict(base, **bad))
    with pytest.raises(ValueError, match="hflip"):
        TR.data_plan(dict(base, device_cache=True, augment=dict(hflip=2.0)))
    with pytest.raises(ValueError, match="crop_min"):
        TR.data_plan(dict(base, device_cache=True, augment=dict(crop=0.5, crop_min=0.0)))
    with pytest.raises(TypeError):
        TR.data_plan(dict(base, device_cache=True, augment="flip"))
    with pytest.raises(ValueError, match="data_seed"):
        TR.data_plan(dict(base, data_seed=-1))
    with pytest.raises(ValueError, match="host transforms cannot be paired"):            # refused before anything touches a device
        TR.train(dict(base, shuffle=True))
