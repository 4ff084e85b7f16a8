"""hdiff_amd.diffusion.Train.train with ``synthetic`` / ``synthetic_prob`` / ``synthetic_val`` on the GPU: the tiny on-disk sets and
the configuration of tests/test_gpu_train_b_driver.py.  A synthetic run repeats bit for bit (weights, averaged weights, losses,
validation records), resumes bit for bit inside a stage and across the stage boundary, refuses a resume under other settings and a
run without the device cache, and on a clean-only cache gives the model an input that is not its label."""
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hdiff_amd  # noqa: E402,F401
from hdiff_amd import device_data as DD  # noqa: E402
from hdiff_amd import synth as SY  # noqa: E402
from hdiff_amd.datasets import Underwater_Dataset  # noqa: E402
from hdiff_amd.diffusion import Train as TR  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning"), pytest.mark.filterwarnings("ignore::UserWarning")]
DEV = "cuda:0"
MODEL = dict(T=1000, ch=32, ch_mult=[1, 2, 2], num_res_blocks=1)
EPOCHS = (2, 2)
SYNTHETIC = {"atmospheric": SY.Synth.lowlight().as_dict(), "underwater": SY.Synth.underwater(shot=(0.0, 0.01), read=(0.0, 0.02))}
EXTRA = dict(device_cache=True, shuffle=True, augment=dict(hflip=0.5, vflip=0.5), synthetic=SYNTHETIC, synthetic_prob=0.75,
             synthetic_val=True)


def as_is(image):
    """The sets' ``transforms=`` without the 256 x 256 resize: HWC uint8 array -> {"image": CHW uint8 tensor}."""
    return {"image": torch.from_numpy(np.ascontiguousarray(image)).permute(2, 0, 1)}


@pytest.fixture(scope="module")
def data_root(tmp_path_factory):
    """HICRD + LoLI in the reference's layout (as tests/test_gpu_train_b_driver.py builds its own): 4 train and 2 test pairs per set,
    16 x 16."""
    from PIL import Image
    root = tmp_path_factory.mktemp("data")
    rng = np.random.default_rng(9)
    for sub, ext, count in (("Train/low", "jpg", 4), ("Train/high", "jpg", 4), ("Test/low", "jpg", 2), ("Test/high", "jpg", 2),
                            ("Train/trainA_paired", "png", 4), ("Train/trainB_paired", "png", 4), ("Test/testA", "png", 2),
                            ("Test/testB", "png", 2)):
        os.makedirs(root / sub)
        for i in range(count):
            low = rng.integers(0, 256, (4, 4, 3), dtype=np.uint8)            # a few colour patches, enlarged
            Image.fromarray(low).resize((16, 16), Image.BILINEAR).save(str(root / sub / f"img{i}.{ext}"))
    return str(root)


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
def synthetic_run(data_root, tmp_path_factory):
    out = tmp_path_factory.mktemp("synthetic")
    return out, TR.train(config(data_root, out, **EXTRA))


@pytest.fixture(scope="module")
def augmented_run(data_root, tmp_path_factory):
    """The same run without the synthetic keys: what the option must move away from."""
    out = tmp_path_factory.mktemp("augmented")
    return out, TR.train(config(data_root, out, **{k: v for k, v in EXTRA.items() if not k.startswith("synthetic")}))


def test_synthetic_run_repeats_and_differs_from_the_plain_one(synthetic_run, augmented_run, data_root, tmp_path):
    out, result = synthetic_run
    assert result["finished"] and result["steps"] == 2 * sum(EPOCHS)
    assert all(np.isfinite(result["losses"][k]).all() for k in TR.TERMS) and len(result["validation"]) == sum(EPOCHS)
    again = TR.train(config(data_root, tmp_path / "again", **dict(EXTRA, synthetic={k: SY.Synth.from_dict(v) for k, v in SYNTHETIC.items()})))
    assert same(final_tensors(out), final_tensors(tmp_path / "again")), "two synthetic runs differ"
    assert again["losses"] == result["losses"] and again["lr"] == result["lr"]
    assert again["validation"] == result["validation"]                   # synthetic_val: the same records at every checkpoint
    assert not same(final_tensors(out), final_tensors(augmented_run[0])) and result["losses"] != augmented_run[1]["losses"]
    assert result["validation"] != augmented_run[1]["validation"]
    state = load(os.path.join(str(out), "ckpt", TR.STATE_FILE))
    assert state["synthetic"] == {"synthetic": {"atmospheric": SY.Synth.lowlight().as_dict(), "underwater": SYNTHETIC["underwater"].as_dict()},
                                  "synthetic_prob": 0.75, "synthetic_val": True}
    assert "synthetic" not in load(os.path.join(str(augmented_run[0]), "ckpt", TR.STATE_FILE))      # a run without the keys: as before
    assert sorted(os.listdir(os.path.join(str(out), "ckpt"))) == sorted(os.listdir(os.path.join(str(augmented_run[0]), "ckpt")))


@pytest.mark.parametrize("max_epochs", [1, 2], ids=["inside_stage_0", "at_the_boundary"])
def test_synthetic_run_interrupted_and_resumed_equals_uninterrupted(synthetic_run, data_root, tmp_path, max_epochs):
    out, result = synthetic_run
    part = TR.train(config(data_root, tmp_path / "run", max_epochs=max_epochs, **EXTRA))
    assert not part["finished"] and part["epochs"] == max_epochs
    state = os.path.join(str(tmp_path / "run"), "ckpt", TR.STATE_FILE)
    rest = TR.train(config(data_root, tmp_path / "run", resume=state, **EXTRA))
    assert rest["finished"] and rest["epochs"] == sum(EPOCHS)
    assert same(final_tensors(out), final_tensors(tmp_path / "run")), "the resumed run ends elsewhere"
    assert rest["losses"] == result["losses"] and rest["validation"] == result["validation"]


def test_resume_under_other_settings_and_a_run_without_the_cache_are_refused(synthetic_run, augmented_run, data_root, tmp_path):
    state = os.path.join(str(synthetic_run[0]), "ckpt", TR.STATE_FILE)
    for other in (dict(synthetic_prob=0.5), dict(synthetic_val=False), dict(synthetic=SY.Synth.haze()),
                  dict(synthetic=dict(SYNTHETIC, atmospheric=None)), dict(synthetic=None, synthetic_prob=None, synthetic_val=None)):
        with pytest.raises(RuntimeError, match="synthetic"):
            TR.train(config(data_root, tmp_path / "other", resume=state, **dict(EXTRA, **other)))
    with pytest.raises(RuntimeError, match="synthetic"):                    # and a plain run's state does not continue as a synthetic one
        TR.train(config(data_root, tmp_path / "other", resume=os.path.join(str(augmented_run[0]), "ckpt", TR.STATE_FILE), **EXTRA))
    with pytest.raises(ValueError, match="device_cache=True"):
        TR.train(config(data_root, tmp_path / "host", synthetic=SY.Synth.haze()))
    with pytest.raises(ValueError, match="without synthetic"):
        TR.train(config(data_root, tmp_path / "host", device_cache=True, synthetic_prob=0.5))
    with pytest.raises(ValueError, match="probability"):
        TR.train(config(data_root, tmp_path / "host", device_cache=True, synthetic=SY.Synth.haze(), synthetic_prob=2.0))
    with pytest.raises(TypeError):
        TR.train(config(data_root, tmp_path / "host", device_cache=True, synthetic="haze"))


def test_a_clean_only_cache_feeds_an_input_that_is_not_its_label(data_root, tmp_path):
    """The loader the driver builds, over a cache whose two sides are one array (a clean-only set): without the option the first
    batch is an identity pair, with it (``synthetic_prob=1``) the input differs from the label and the label is the clean image."""
    plan = TR.synthetic_plan(config(data_root, tmp_path, device_cache=True, synthetic=SY.Synth.underwater(), synthetic_prob=1))
    assert plan["synthetic"]["underwater"] == plan["synthetic"]["atmospheric"] == SY.Synth.underwater() and not plan["synthetic_val"]
    pairs = DD.build_cache(Underwater_Dataset("HICRD", transforms=as_is, task="train", root=data_root), num_workers=0)
    clean = DD.PairCache(pairs.b, pairs.b, None, pairs.fingerprint).to(DEV)
    assert clean.b is clean.a
    inp, label = next(iter(DD.DeviceLoader(clean, 2, drop_last=True, seed=3)))
    assert torch.equal(inp, label)
    inp, label = next(iter(DD.DeviceLoader(clean, 2, drop_last=True, seed=3, synth=plan["synthetic"]["underwater"],
                                           synth_prob=plan["synthetic_prob"])))
    assert torch.equal(label, clean.a[:2]) and all(not torch.equal(inp[j], label[j]) for j in range(2))
