"""The device-resident paired cache on the GPU: hdiff_batch_assemble (csrc/batch_assemble.hip) against its integer definition
(tests/_augment_def.py) bit for bit, sample independence and stream capture, DeviceLoader against the DataLoader it replaces, and
hdiff_amd.diffusion.Train.train with ``device_cache`` / ``augment`` / ``shuffle``: equal to the host-loader run when only the loader is
switched, repeatable and resumable with augmentation."""
import os
import sys
import types

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

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning"), pytest.mark.filterwarnings("ignore::UserWarning")]
DEV = "cuda:0"
ONE = 1 << 32
SHAPES = ((1, 1), (5, 7), (13, 20), (16, 16), (32, 32))        # widths below, and not a multiple of, the 4-pixel store
N, IDX = 5, (4, 0, 2, 2, 1, 4, 3)                              # B = 7: repeated and out of order
EPOCHS_K, SEEDS = (0, 1, 2 ** 31 - 1), (0, 2 ** 63 + 5)


def arrays(H, W):
    rng = np.random.default_rng(1000 * H + W)
    return rng.integers(0, 256, (N, 3, H, W), dtype=np.uint8), rng.integers(0, 256, (N, 3, H, W), dtype=np.uint8)


def run(a, b, idx, **kw):
    out_a, out_b = DD.assemble(a, b, idx, **kw)
    return out_a.cpu().numpy(), out_b.cpu().numpy()


# -- 1. the kernel against the definition -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_equals_the_definition_bit_for_bit(shape):
    H, W = shape
    a, b = arrays(H, W)
    da, db = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    idx = torch.tensor(IDX, dtype=torch.int64, device=DEV)
    square = H == W
    cases = [dict(), dict(th_h=ONE), dict(th_v=ONE), dict(th_c=ONE, lo_h=1), dict(th_c=ONE, lo_h=H), dict(th_c=ONE, lo_h=(H + 1) // 2)]
    if square:
        cases.append(dict(rot90=True))
    cases += [dict(th_h=ONE // 2, th_v=ONE // 2, rot90=square, th_c=ONE // 2, lo_h=lo) for lo in (1, (H + 1) // 2)]
    checked = 0
    for case in cases:
        heavy = len(case) == 5                        # everything at p = 0.5: every epoch and seed; a switch alone: two keys
        keys = [(s, e) for s in SEEDS for e in EPOCHS_K] if heavy else [(SEEDS[0], 1), (SEEDS[1], EPOCHS_K[2])]
        for seed, epoch in keys:
            lo_h = case.get("lo_h", H)
            want_a, want_b = AD.assemble_def(a, b, IDX, seed=seed, epoch=epoch, th_h=case.get("th_h", 0), th_v=case.get("th_v", 0),
                                             rot90=case.get("rot90", False), th_c=case.get("th_c", 0), lo_h=lo_h)
            got_a, got_b = run(da, db, idx, seed=seed, epoch=epoch, th_hflip=case.get("th_h", 0), th_vflip=case.get("th_v", 0),
                               rot90=int(case.get("rot90", False)), th_crop=case.get("th_c", 0), crop_lo_h=lo_h)
            assert np.array_equal(got_a, want_a), (shape, case, seed, epoch, "a")
            assert np.array_equal(got_b, want_b), (shape, case, seed, epoch, "b")
            if not case:                              # all thresholds 0: the source bytes
                assert np.array_equal(got_a, a[list(IDX)]) and np.array_equal(got_b, b[list(IDX)])
            checked += 1
    assert checked >= 2 * 6 + 6 * 2
    # b aliasing a
    kw = dict(seed=7, epoch=3, th_hflip=ONE // 2, th_vflip=ONE // 2, rot90=int(square), th_crop=ONE // 2, crop_lo_h=1)
    alias_a, alias_b = run(da, da, idx, **kw)
    assert np.array_equal(alias_a, alias_b) and np.array_equal(alias_a, run(da, db, idx, **kw)[0])
    if H * W > 1:                                     # the switches did something
        assert not np.array_equal(alias_a, a[list(IDX)])


def test_augment_thresholds_drive_the_kernel_like_the_definition():
    """Augment -> thresholds -> kernel, through DeviceLoader's own path, at the driver test's settings."""
    a, b = arrays(16, 16)
    aug = DD.Augment(hflip=0.5, vflip=0.5, rot90=True, crop=0.5, crop_min=0.5)
    th = aug.thresholds(16)
    cache = DD.PairCache(torch.from_numpy(a), torch.from_numpy(b), None, "x").to(DEV)
    loader = DD.DeviceLoader(cache, 2, shuffle=True, drop_last=False, augment=aug, seed=2 ** 63 + 5)
    assert len(loader) == 3
    for epoch in (0, 6):
        loader.set_epoch(epoch)
        batches = DD.epoch_indices(N, 2, epoch=epoch, seed=2 ** 63 + 5, shuffle=True, drop_last=False)
        got = list(loader)
        assert len(got) == len(batches) == 3
        for (inp, label), idx in zip(got, batches):
            want_a, want_b = AD.assemble_def(a, b, idx.tolist(), seed=2 ** 63 + 5, epoch=epoch, th_h=th["th_hflip"], th_v=th["th_vflip"],
                                             rot90=True, th_c=th["th_crop"], lo_h=th["crop_lo_h"])
            assert np.array_equal(inp.cpu().numpy(), want_a) and np.array_equal(label.cpu().numpy(), want_b)
    with pytest.raises(ValueError, match="square"):
        DD.DeviceLoader(DD.PairCache(cache.a[:, :, :8].contiguous(), cache.b[:, :, :8].contiguous(), None, "x"), 2, augment=aug)


# -- 2. sample independence, stream capture ---------------------------------------------------------------------------------------
def test_a_sample_does_not_depend_on_its_batch_and_the_launch_is_capturable():
    H, W = 13, 20
    a, b = arrays(H, W)
    da, db = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    kw = dict(seed=11, epoch=2, th_hflip=ONE // 2, th_vflip=ONE // 2, rot90=0, th_crop=ONE, crop_lo_h=3)

    def dev_idx(values):
        return torch.tensor(values, dtype=torch.int64, device=DEV)

    alone = run(da, db, dev_idx([3]), **kw)
    first = run(da, db, dev_idx([3, 0, 1, 2, 4, 0, 1]), **kw)
    last = run(da, db, dev_idx([0, 1, 2, 4, 0, 1, 3]), **kw)
    again = run(da, db, dev_idx([0, 1, 2, 4, 0, 1, 3]), **kw)
    for side in (0, 1):
        assert np.array_equal(alone[side][0], first[side][0]) and np.array_equal(alone[side][0], last[side][6])
        assert np.array_equal(last[side], again[side])
    # one captured launch, replayed twice (outputs and indices allocated before the capture)
    lib = hdiff_amd.lib()
    idx = dev_idx([0, 1, 2, 4, 0, 1, 3])
    out_a = torch.zeros(7, 3, H, W, dtype=torch.uint8, device=DEV)
    out_b = torch.zeros_like(out_a)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        s = torch.cuda.current_stream().cuda_stream
        _capi.check(lib.hdiff_batch_assemble(da.data_ptr(), db.data_ptr(), idx.data_ptr(), 7, N, H, W, kw["seed"], kw["epoch"],
                                             kw["th_hflip"], kw["th_vflip"], 0, kw["th_crop"], kw["crop_lo_h"], out_a.data_ptr(),
                                             out_b.data_ptr(), s), "batch_assemble")
    for _ in range(2):
        out_a.zero_()
        out_b.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out_a.cpu().numpy(), last[0]) and np.array_equal(out_b.cpu().numpy(), last[1])


# -- 3. the loader against the DataLoader it replaces -----------------------------------------------------------------------------
def as_is(image):
    """The sets' ``transforms=`` without the 256 x 256 resize: HWC uint8 array -> {"image": CHW uint8 tensor}."""
    return {"image": torch.from_numpy(np.ascontiguousarray(image)).permute(2, 0, 1)}


@pytest.fixture(scope="module")
def data_root(tmp_path_factory):
    """HICRD + LoLI in the reference's layout (as tests/test_gpu_train_b_driver.py builds its own): 4 train and 2 test pairs per set,
    16 x 16, and 5 validation pairs of HICRD."""
    from PIL import Image
    root = tmp_path_factory.mktemp("data")
    rng = np.random.default_rng(9)
    for sub, ext, count in (("Train/low", "jpg", 4), ("Train/high", "jpg", 4), ("Test/low", "jpg", 2), ("Test/high", "jpg", 2),
                            ("Train/trainA_paired", "png", 4), ("Train/trainB_paired", "png", 4), ("Test/testA", "png", 2),
                            ("Test/testB", "png", 2), ("Val/valA", "png", 5), ("Val/valB", "png", 5)):
        os.makedirs(root / sub)
        for i in range(count):
            low = rng.integers(0, 256, (4, 4, 3), dtype=np.uint8)            # a few colour patches, enlarged
            Image.fromarray(low).resize((16, 16), Image.BILINEAR).save(str(root / sub / f"img{i}.{ext}"))
    return str(root)


def test_device_loader_yields_what_the_dataloader_yields(data_root):
    from torch.utils.data import DataLoader
    sets = (Underwater_Dataset("HICRD", transforms=as_is, task="train", root=data_root),
            Atmospheric_Dataset("LoLI", transforms=as_is, task="train", root=data_root),
            Underwater_Dataset("HICRD", transforms=as_is, task="val", root=data_root))
    for data in sets:
        cache = DD.build_cache(data, num_workers=0).to(DEV)
        torch.manual_seed(5)
        want = list(DataLoader(data, batch_size=2, drop_last=True))
        after_host = torch.get_rng_state()
        torch.manual_seed(5)
        loader = DD.DeviceLoader(cache, 2)
        got = list(loader)
        assert torch.equal(torch.get_rng_state(), after_host)                # the one draw DataLoader.__iter__ makes
        assert len(got) == len(want) == len(loader) == len(data) // 2 and len(got) >= 2
        for g, w in zip(got, want):
            assert type(g) is type(w) and len(g) == len(w)
            assert g[0].dtype == torch.uint8 and g[0].device == torch.device(DEV)
            assert torch.equal(g[0], w[0].to(DEV)) and torch.equal(g[1], w[1].to(DEV))
            if len(w) == 3:
                assert type(g[2]) is type(w[2]) and list(g[2]) == list(w[2])
        assert (len(want[0]) == 3) == (data.task == "val")
        short = list(DD.DeviceLoader(cache, 2, drop_last=False))
        want_short = list(DataLoader(data, batch_size=2, drop_last=False))
        assert len(short) == len(want_short) and torch.equal(short[-1][0], want_short[-1][0].to(DEV))


# -- 4. the driver ----------------------------------------------------------------------------------------------------------------
MODEL = dict(T=1000, ch=32, ch_mult=[1, 2, 2], num_res_blocks=1)
EPOCHS = (2, 2)
AUGMENT = dict(hflip=0.5, vflip=0.5, rot90=True, crop=0.5, crop_min=0.5)


def config(data_root, out, **kw):
    """The tiny configuration of tests/test_gpu_train_b_driver.py."""
    base = dict(underwater_data_name="HICRD", atmospheric_data_name="LoLI", dataset_root=data_root, transforms=as_is,
                T=MODEL["T"], channel=MODEL["ch"], channel_mult=MODEL["ch_mult"], num_res_blocks=MODEL["num_res_blocks"], dropout=0.15,
                lr=1e-4, multiplier=2.5, beta_1=1e-4, beta_T=0.02, grad_clip=1.0, batch_size=2, epochs_stage_1=EPOCHS[0],
                epochs_stage_2=EPOCHS[1], save_checkpoint=1, output_path=str(out), pretrained_path=None, device_list=[DEV],
                num_workers=0, seed=3, ema_decay=0.9, max_val_batches=1)
    base.update(kw)
    return types.SimpleNamespace(**base)


def load(path):
    return torch.load(path, map_location="cpu", weights_only=False)


def final_tensors(out):
    """(final weights, final averaged weights) of a finished run."""
    ck = os.path.join(str(out), "ckpt")
    return (load(os.path.join(ck, TR.final_name(sum(EPOCHS), "HICRD", "LoLI"))),
            load(os.path.join(ck, TR.final_name(sum(EPOCHS), "HICRD", "LoLI", ema=True))))


def same(x, y):
    return all(list(p) == list(q) and all(torch.equal(p[k], q[k]) for k in p) for p, q in zip(x, y))


@pytest.fixture(scope="module")
def host_run(data_root, tmp_path_factory):
    out = tmp_path_factory.mktemp("host")
    return out, TR.train(config(data_root, out))


@pytest.fixture(scope="module")
def augmented_run(data_root, tmp_path_factory):
    out = tmp_path_factory.mktemp("augmented")
    return out, TR.train(config(data_root, out, device_cache=True, augment=AUGMENT, shuffle=True))


def test_driver_with_the_device_cache_equals_the_host_loader_run(host_run, data_root, tmp_path):
    out, result = host_run
    got = TR.train(config(data_root, tmp_path / "cached", device_cache=True))
    assert got["finished"] and got["steps"] == result["steps"] == 2 * sum(EPOCHS)
    assert same(final_tensors(out), final_tensors(tmp_path / "cached")), "switching the loader changed the weights"
    assert got["losses"] == result["losses"] and got["validation"] == result["validation"] and got["lr"] == result["lr"]
    assert sorted(os.listdir(tmp_path / "cached" / "cache")) == ["HICRD_test.pt", "HICRD_train.pt", "LoLI_test.pt", "LoLI_train.pt"]
    assert sorted(os.listdir(tmp_path / "cached" / "ckpt")) == sorted(os.listdir(os.path.join(str(out), "ckpt")))
    elsewhere = TR.train(config(data_root, tmp_path / "again", device_cache=True, cache_dir=str(tmp_path / "cached" / "cache")))
    assert same(final_tensors(out), final_tensors(tmp_path / "again")) and not os.path.exists(tmp_path / "again" / "cache")


def test_augmented_run_differs_from_the_plain_one_and_repeats(host_run, augmented_run, data_root, tmp_path):
    out, result = augmented_run
    assert result["finished"] and all(np.isfinite(result["losses"][k]).all() for k in TR.TERMS)
    assert not same(final_tensors(host_run[0]), final_tensors(out)) and result["losses"] != host_run[1]["losses"]
    again = TR.train(config(data_root, tmp_path / "again", device_cache=True, augment=DD.Augment(**AUGMENT), shuffle=True))
    assert same(final_tensors(out), final_tensors(tmp_path / "again")), "two augmented runs differ"
    assert again["losses"] == result["losses"] and again["validation"] == result["validation"]


@pytest.mark.parametrize("max_epochs", [1, 2], ids=["inside_stage_0", "at_the_boundary"])
def test_augmented_run_interrupted_and_resumed_equals_uninterrupted(augmented_run, data_root, tmp_path, max_epochs):
    out, result = augmented_run
    extra = dict(device_cache=True, augment=AUGMENT, shuffle=True)
    part = TR.train(config(data_root, tmp_path / "run", max_epochs=max_epochs, **extra))
    assert not part["finished"] and part["epochs"] == max_epochs
    state = os.path.join(str(tmp_path / "run"), "ckpt", TR.STATE_FILE)
    rest = TR.train(config(data_root, tmp_path / "run", resume=state, **extra))
    assert rest["finished"] and rest["epochs"] == sum(EPOCHS)
    assert same(final_tensors(out), final_tensors(tmp_path / "run")), "the resumed run ends elsewhere"
    assert rest["losses"] == result["losses"] and rest["validation"] == result["validation"]
