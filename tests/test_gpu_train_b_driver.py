"""hdiff_amd.diffusion.Train.train (reference utils/rotinas.py:571-732) end to end on a tiny two-stage run: the files it writes, the
EMA it keeps, the learning rates, the validation pass that leaves the training stream alone, interruption and resume, and the
evaluation of the averaged checkpoint by diffusion.Evaluate.test."""
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hdiff_amd  # noqa: E402
from hdiff_amd.Scheduler import GradualWarmupScheduler  # noqa: E402
from hdiff_amd.diffusion import Evaluate as EV  # noqa: E402
from hdiff_amd.diffusion import Train as TR  # noqa: E402
from hdiff_amd.diffusion.Model import DynamicUNet  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning"), pytest.mark.filterwarnings("ignore::UserWarning")]
DEV = "cuda:0"
MODEL = dict(T=1000, ch=32, ch_mult=[1, 2, 2], num_res_blocks=1)
DECAY, SEED = 0.9, 3
STEPS_PER_EPOCH, EPOCHS = 2, (2, 2)          # 4 train pairs, batch 2, drop_last
TOTAL_STEPS = STEPS_PER_EPOCH * sum(EPOCHS)


def as_is(image):
    """The sets' ``transforms=`` without the 256 x 256 resize: HWC uint8 array -> {"image": CHW uint8 tensor}."""
    return {"image": torch.from_numpy(np.ascontiguousarray(image)).permute(2, 0, 1)}


@pytest.fixture(scope="module")
def data_root(tmp_path_factory):
    """HICRD + LoLI in the reference's layout (as tests/test_gpu_quality.py builds its own): 4 train and 2 test pairs per set, 16 x 16."""
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
    base = dict(underwater_data_name="HICRD", atmospheric_data_name="LoLI", dataset_root=data_root, transforms=as_is,
                T=MODEL["T"], channel=MODEL["ch"], channel_mult=MODEL["ch_mult"], num_res_blocks=MODEL["num_res_blocks"], dropout=0.15,
                lr=1e-4, multiplier=2.5, beta_1=1e-4, beta_T=0.02, grad_clip=1.0, batch_size=2, epochs_stage_1=EPOCHS[0],
                epochs_stage_2=EPOCHS[1], save_checkpoint=1, output_path=str(out), pretrained_path=None, device_list=[DEV],
                num_workers=0, seed=SEED, ema_decay=DECAY, max_val_batches=1)
    base.update(kw)
    return types.SimpleNamespace(**base)


def load(path):
    return torch.load(path, map_location="cpu", weights_only=False)


def final_tensors(out):
    """(final weights, final averaged weights, the state file's shadow list) of a finished run."""
    ck = os.path.join(str(out), "ckpt")
    return (load(os.path.join(ck, TR.final_name(sum(EPOCHS), "HICRD", "LoLI"))),
            load(os.path.join(ck, TR.final_name(sum(EPOCHS), "HICRD", "LoLI", ema=True))), load(os.path.join(ck, TR.STATE_FILE))["ema"]["shadow"])


def same(a, b):
    if isinstance(a, dict):
        return list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def full_run(data_root, tmp_path_factory):
    """The uninterrupted run every test compares against, with the weights after every optimizer step."""
    out = tmp_path_factory.mktemp("full")
    trail = []
    cfg = config(data_root, out, on_step=lambda num, model: trail.append([p.detach().double().cpu() for p in model.parameters()]))
    result = TR.train(cfg)
    return out, cfg, result, trail


def test_files_checkpoints_and_the_average(full_run):
    out, cfg, result, trail = full_run
    ck = os.path.join(str(out), "ckpt")
    assert sorted(os.listdir(ck)) == TR.expected_files(cfg) == sorted(
        [f"ckpt_{g}_{stage}_HICRDLoLI{suffix}.pt" for g, stage in ((0, "Atmosferic"), (1, "Atmosferic"), (2, "Underwater"),
                                                                   (3, "Underwater"), (4, "final")) for suffix in ("", "_ema")]
        + ["state_last.pt"])
    assert sorted(result["files"]) == sorted(os.path.join(ck, n) for n in os.listdir(ck))
    assert result["finished"] and result["steps"] == TOTAL_STEPS == len(trail) and result["epochs"] == sum(EPOCHS)
    for name in os.listdir(ck):
        if name == TR.STATE_FILE:
            continue
        sd = torch.load(os.path.join(ck, name), map_location="cpu")              # a plain state dict: loads with weights_only
        DynamicUNet(**MODEL, dropout=0.15).load_state_dict(sd, strict=True)
        if name.endswith("_ema.pt"):
            raw = load(os.path.join(ck, name[:-len("_ema.pt")] + ".pt"))
            assert list(raw) == list(sd) and any(not torch.equal(raw[k], sd[k]) for k in sd)
    # losses and validation records
    assert all(len(result["losses"][k]) == sum(EPOCHS) and np.isfinite(result["losses"][k]).all() for k in TR.TERMS)
    assert all(v > 0 for v in result["losses"]["msssim"])                        # the package's MS-SSIM + L1 term is on by default
    assert [(v["epoch"], v["stage"]) for v in result["validation"]] == [(0, "Atmosferic"), (1, "Atmosferic"), (2, "Underwater"),
                                                                          (3, "Underwater")]
    for v in result["validation"]:
        assert v["raw"]["batches"] == v["ema"]["batches"] == 1
        assert all(np.isfinite(v[kind][k]) for kind in ("raw", "ema") for k in TR.TERMS) and v["raw"]["loss"] != v["ema"]["loss"]
    # the optimizer was rebuilt at the stage boundary, the EMA was not
    state = load(os.path.join(ck, TR.STATE_FILE))
    counts = {int(st["step"]) for st in state["optimizer"]["state"].values()}
    assert max(counts) == STEPS_PER_EPOCH * EPOCHS[1] and state["ema"]["num_updates"] == TOTAL_STEPS == state["num"]
    assert state["ema"]["decay"] == DECAY


def test_the_average_is_the_float64_average_of_the_per_step_weights(full_run):
    """shadow_0 = the initial weights, shadow_k = shadow_{k-1} + (p_k - shadow_{k-1}) * float32(1 - decay) in float64 from the weights
    after every step.  The kernel rounds three fp32 operations per element and step, each by at most 2^-24 of a value no larger than
    2 M (M: the largest |weight| or |shadow| of the tensor), and an earlier error is carried on with a factor below 1: after N steps
    the distance is at most N * 3 * 2^-24 * 2 M."""
    out, cfg, result, trail = full_run
    torch.manual_seed(SEED)
    start = [p.detach().double() for p in DynamicUNet(**MODEL, dropout=0.15).parameters()]      # what the driver built from its seed
    w = float(np.float32(1.0 - DECAY))
    shadow, peak = [s.clone() for s in start], [s.abs().max().item() for s in start]
    for weights in trail:
        shadow = [s + (p - s) * w for s, p in zip(shadow, weights)]
        peak = [max(m, p.abs().max().item()) for m, p in zip(peak, weights)]
    final, final_ema, state_shadow = final_tensors(out)
    names = [n for n, _ in DynamicUNet(**MODEL, dropout=0.15).named_parameters()]
    assert all(torch.equal(final[n], p.float()) for n, p in zip(names, trail[-1]))              # the hook saw the real weights
    assert len(names) == len(shadow) == len(state_shadow)
    moved = 0
    for name, want, got, m in zip(names, shadow, state_shadow, peak):
        assert torch.equal(final_ema[name], got), name                                          # the file holds the shadow
        err = (got.double() - want).abs().max().item()
        assert err <= TOTAL_STEPS * 3 * 2.0 ** -24 * 2 * m, (name, err, m)
        moved += int(not torch.equal(got, final[name]))
    assert moved > len(names) // 2


def scheduler_lrs(lr, multiplier, epochs):
    opt = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(2))], lr=lr, weight_decay=1e-4)
    cos = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer=opt, T_max=epochs, eta_min=0, last_epoch=-1)
    warm = GradualWarmupScheduler(optimizer=opt, multiplier=multiplier, warm_epoch=epochs // 10, after_scheduler=cos)
    out = []
    for _ in range(epochs):
        out.append(opt.param_groups[0]["lr"])
        opt.step()
        warm.step()
    return out


def test_learning_rates_are_the_schedulers(full_run):
    _, cfg, result, _ = full_run
    assert result["lr"] == scheduler_lrs(cfg.lr, cfg.multiplier, EPOCHS[0]) + scheduler_lrs(cfg.lr, cfg.multiplier, EPOCHS[1])
    assert result["lr"] == TR.lr_sequence(cfg.lr, cfg.multiplier, EPOCHS[0]) + TR.lr_sequence(cfg.lr, cfg.multiplier, EPOCHS[1])


def test_runs_repeat_bit_for_bit_and_validation_leaves_the_training_stream_alone(full_run, data_root, tmp_path):
    out, _, result, _ = full_run
    again = TR.train(config(data_root, tmp_path / "again"))
    assert all(same(a, b) for a, b in zip(final_tensors(out), final_tensors(tmp_path / "again"))), "two uninterrupted runs differ"
    assert again["losses"] == result["losses"] and again["validation"] == result["validation"]
    blind = TR.train(config(data_root, tmp_path / "blind", max_val_batches=0))
    assert all(v["raw"]["batches"] == 0 for v in blind["validation"])
    assert all(same(a, b) for a, b in zip(final_tensors(out), final_tensors(tmp_path / "blind"))), "validation moved the training stream"
    assert blind["losses"] == result["losses"]


@pytest.mark.parametrize("max_epochs", [1, 2, 3], ids=["inside_stage_0", "at_the_boundary", "inside_stage_1"])
def test_interrupted_and_resumed_equals_uninterrupted(full_run, data_root, tmp_path, max_epochs):
    out, _, result, _ = full_run
    part = TR.train(config(data_root, tmp_path / "run", max_epochs=max_epochs))
    assert not part["finished"] and part["epochs"] == max_epochs and part["steps"] == STEPS_PER_EPOCH * max_epochs
    ck = os.path.join(str(tmp_path / "run"), "ckpt")
    assert TR.final_name(sum(EPOCHS), "HICRD", "LoLI") not in os.listdir(ck)
    rest = TR.train(config(data_root, tmp_path / "run", resume=os.path.join(ck, TR.STATE_FILE)))
    assert rest["finished"] and rest["steps"] == TOTAL_STEPS and rest["epochs"] == sum(EPOCHS)
    assert all(same(a, b) for a, b in zip(final_tensors(out), final_tensors(tmp_path / "run")))
    assert rest["losses"] == result["losses"] and rest["lr"] == result["lr"] and rest["validation"] == result["validation"]
    assert sorted(os.listdir(ck)) == sorted(os.listdir(os.path.join(str(out), "ckpt")))
    state = load(os.path.join(ck, TR.STATE_FILE))
    assert max(int(st["step"]) for st in state["optimizer"]["state"].values()) == STEPS_PER_EPOCH * EPOCHS[1]
    assert state["ema"]["num_updates"] == TOTAL_STEPS


def test_evaluate_takes_the_averaged_checkpoint(full_run, data_root, tmp_path):
    """Evaluate.test(pretrained_path=<final _ema.pt>) scores and writes what a sampler built by hand on the shadow weights returns."""
    from PIL import Image
    from hdiff_amd.datasets import Atmospheric_Dataset, Underwater_Dataset
    from hdiff_amd.diffusion.Diffusion import GaussianDiffusionSampler
    out, cfg, _, _ = full_run
    path = os.path.join(str(out), "ckpt", TR.final_name(sum(EPOCHS), "HICRD", "LoLI", ema=True))
    ev = types.SimpleNamespace(**{**vars(cfg), "pretrained_path": path, "ddim_step": 2, "result_root": str(tmp_path / "result")})
    torch.manual_seed(4)
    results = EV.test(ev, None)
    shadow = load(os.path.join(str(out), "ckpt", TR.STATE_FILE))["ema"]["shadow"]
    torch.manual_seed(4)                      # as above: Evaluate.test builds its model, which draws from the CPU stream, then samples
    model = DynamicUNet(**MODEL, dropout=0.).eval()
    with torch.no_grad():
        for p, s in zip(model.parameters(), shadow):
            p.copy_(s)
    sampler = GaussianDiffusionSampler(model, cfg.beta_1, cfg.beta_T, cfg.T).to(DEV)
    for name, data in (("HICRD", Underwater_Dataset("HICRD", transforms=as_is, task="test", root=data_root)),
                       ("LoLI", Atmospheric_Dataset("LoLI", transforms=as_is, task="test", root=data_root))):
        outs = []
        want = EV.evaluate(sampler, EV._batched(data, 2), ddim_step=2, collect=outs)
        got = results[name]
        assert got["n"] == want["n"] == 2 and np.array_equal(got["per_image"], want["per_image"]), name
        folder = os.path.join(str(tmp_path / "result"), os.path.basename(path), name)
        images = ((torch.cat(outs) + 1) / 2).clamp(0, 1).mul(255.0).round().to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()
        for img, file in zip(images, sorted(f for f in os.listdir(folder) if f != "res.txt")):
            if file.endswith(".png"):                                               # lossless: the sampler's output as written
                assert np.array_equal(np.asarray(Image.open(os.path.join(folder, file))), img), (name, file)
