"""The training driver of the reference's second tree (``utils/rotinas.py:571-732`` ``train``, which ``Main.py --state train`` runs):
two stages over the image-conditioned ``DynamicUNet`` -- stage 0 "Atmosferic" on the atmospheric set for ``epochs_stage_1`` epochs,
stage 1 "Underwater" on the underwater set for ``epochs_stage_2`` -- each with a NEW ``AdamW(lr, weight_decay=1e-4)`` and a new
``CosineAnnealingLR(T_max=epochs)`` behind ``GradualWarmupScheduler(multiplier, warm_epoch=epochs // 10)`` stepped once per epoch.
Per batch (``rotinas.py:427-448``): ``loss = trainer(input, label, stage_number)[0]; loss.mean().backward()``, then the clip and the
step, here ``opt.step(max_grad_norm=grad_clip)`` of ``hdiff_amd.optim.AdamW``.  Weights-only checkpoints go to
``<output_path>/ckpt/ckpt_<global epoch>_<stage name>_<u_name><a_name>.pt`` and, at the end, ``ckpt_<total>_final_<u_name><a_name>.pt``:
plain state dicts that the reference and ``Evaluate.test(pretrained_path=...)`` load.

Keys read as the reference reads them: ``underwater_data_name``, ``atmospheric_data_name``, ``T``, ``channel``, ``channel_mult``,
``num_res_blocks``, ``dropout``, ``lr``, ``multiplier``, ``beta_1``, ``beta_T``, ``grad_clip``, ``batch_size``, ``epochs_stage_1``,
``epochs_stage_2``, ``save_checkpoint``, ``output_path``, ``pretrained_path``, ``device_list``.

Deliberate deviations from the reference:
  * checkpoints: the reference's second condition compares the GLOBAL epoch with the stage's length (``rotinas.py:700``); here a
    checkpoint is written when ``global_epoch % save_checkpoint == 0`` and also at the last epoch of each stage.
  * validation: the reference's is unreachable (it names an undefined ``dataloaders_test``, ``:712``) and would step the optimizer
    (``process_batch``).  Here it is the five loss terms of the trainer on the stage's test loader, under ``no_grad`` with the model in
    ``eval()``, no optimizer involved, at most ``max_val_batches`` batches, inside ``torch.random.fork_rng`` with a fixed seed: it
    draws the same ``t`` / noise at every checkpoint and does not move the training stream.
  * a stage shorter than 10 epochs has ``warm_epoch = 0``, at which the reference's scheduler divides by zero; here such a stage
    starts at ``lr * multiplier`` (``Scheduler.GradualWarmupScheduler``: a warm-up of no epochs is over at epoch 0).
  * wandb is not wired: ``wandb=True`` warns once.
  * data-parallel training is out of scope: ``WORLD_SIZE > 1`` or ``DDP=True`` raises (the per-batch gating of the middle blocks does
    not fit ``parallel.FlatGradients`` as it stands); of ``device_list`` the first entry is used.
  * ``msssim_loss`` defaults to the package's ``Loss.loss.MSSSIMLoss()``; ``dino_loss`` is optional -- a callable, or ``"native"`` for
    the package's own ``Loss.loss.PerceptualLoss_dino`` with ``dino_weights`` (the hub checkpoint's state dict or its path; no weights
    ship and none are fetched) and ``dino_dense`` (``"conv"``, the default, or ``"tokens"``: the trunk's dense-layer route) -- and the trainer's warning stands when it is absent.  The trunk is frozen and belongs to the trainer:
    ``TERMS``, the records, the checkpoints, the EMA and the optimizer are the same with and without it.

Additions, all optional (with none of them set the run is the loop above): ``dataset_root`` (one root for both sets, or a dict by
set name), ``transforms`` (the sets' ``transforms=``), ``num_workers`` (4), ``seed`` (``torch.manual_seed`` before the model is
built), ``max_steps_per_epoch``, ``max_val_batches``, ``max_epochs`` (stop after this many global epochs, having written the state
file: a clean interruption), ``ema_decay`` (``None``: no EMA), ``resume`` (a state file to continue from), ``on_step`` (a callable
``(step number, model)`` run after every optimizer step, for logging), ``extra_losses`` (handed to the trainer unchanged: a sequence
of ``(name, weight, callable)`` added to ``loss``, e.g. ``Loss.loss.PerceptualLoss_vgg`` / ``CharbonnierLoss``; ``TERMS``, the records
and the checkpoints are the same with and without it), and the data keys ``device_cache``, ``cache_dir``, ``augment``,
``shuffle``, ``data_seed``, ``synthetic``, ``synthetic_prob``, ``synthetic_val`` (below).

With ``device_cache=True`` each of the four splits is decoded once (``device_data.build_cache``, stored under ``cache_dir``, default
``<output_path>/cache``, and reused while the files' fingerprint holds), kept on the device as ``uint8``, and every batch is assembled
there by one kernel (``device_data.DeviceLoader``).  Without ``augment`` and ``shuffle`` such a run computes what the host-loader run
computes, bit for bit.  ``augment`` (an ``Augment`` or a dict of its arguments: ``hflip``, ``vflip``, ``rot90``, ``crop``, ``crop_min``)
gives each training pair ONE geometric transform, drawn from ``(data_seed, global epoch, sample index)``; ``shuffle`` permutes the
training set per epoch from the same key.  ``data_seed`` defaults to ``seed or 0``.  Test loaders never shuffle or augment.  Before
every training epoch the driver calls ``set_epoch(global epoch)``, so a resumed run draws what the uninterrupted one draws.
``augment`` or ``shuffle`` without ``device_cache`` raises: the sets' host ``transforms`` run once per image and cannot be paired.

``synthetic`` (a ``synth.Synth``, its ``as_dict()``, or ``{"atmospheric": ..., "underwater": ...}`` for one per stage, ``None`` for a
stage without) draws the INPUT of a training pair from its augmented target on the device (``hdiff_amd/synth.py``): with probability
``synthetic_prob`` (1.0) per sample, from ``(data_seed, global epoch, sample index)``.  That is how a clean-only set, whose cache
holds ``b is a``, trains anything but the identity.  ``synthetic_val`` (False) degrades the stage's test loader too, under a key that
does not move with the epoch: the only validation a clean-only set can have.  ``synthetic`` without ``device_cache`` raises.  The
state file records the three values (``synthetic_plan``) and ``resume`` under other values raises; a run without the keys builds and
writes what it did before.

With ``ema_decay`` an ``optim.EMA`` of all weights is updated after every optimizer step and lives across the stage boundary (the
optimizer does not); every checkpoint gets a sibling ``..._ema.pt`` (``EMA.shadow_state_dict``: the same keys, so ``Evaluate.test``
evaluates it unchanged) and validation reports the raw and the averaged weights.

Whenever a checkpoint is written so is ``<output_path>/ckpt/state_last.pt``: model, EMA, optimizer and both schedulers' state
dicts, stage index, epoch within the stage, step counter, the torch CPU and device RNG states and the records so far.  ``resume``
restores all of it and continues at the next epoch; across a stage boundary it begins stage 1 with a fresh optimizer, as the
uninterrupted run does.

``prediction`` ("eps", the default, or "v"), ``loss_weighting`` (None or "min_snr"), ``snr_gamma`` (5.0) and ``y0_divisor`` (255.0) are
the trainer's keywords of those names (``prediction_settings``).  The state file records the four values and ``resume`` under other
values raises.  When ``prediction`` is not "eps" the driver also writes ``<output_path>/ckpt/prediction.json`` with them -- the
checkpoints stay plain state dicts, and ``Evaluate.test`` reads that file so that such a checkpoint is not sampled as eps.  A run
without the keys writes the files it wrote before.

Returns ``{"losses": {term: [mean per epoch]}, "lr": [per epoch], "validation": [records], "files": [paths written], "steps": n,
"epochs": global epochs done, "finished": bool}``.
"""
from __future__ import annotations

import os
import warnings
from typing import Dict, List, Optional, Tuple

import torch

from .Evaluate import PREDICTION_FILE, _cfg

__all__ = ["train", "data_plan", "synthetic_plan", "stage_plan", "checkpoint_epochs", "checkpoint_name", "final_name", "expected_files", "lr_sequence",
           "TERMS", "STATE_FILE", "PREDICTION_FILE", "prediction_settings", "write_prediction_file"]

TERMS = ("loss", "mse_loss", "perceptual_dino", "msssim", "col_loss")       # the trainer's return order (rotinas.py:439)
WEIGHT_DECAY = 1e-4                                                          # rotinas.py:660
STATE_FILE = "state_last.pt"
VALIDATION_SEED = 0x5eed


# -- host-only pieces: the stage plan, which epochs checkpoint, the file names, the LR sequence ----------------------------------
def stage_plan(config) -> List[Dict[str, object]]:
    """rotinas.py:643-646, with the set each stage trains on (:668-673)."""
    lr = _cfg(config, "lr")
    return [{"name": "Atmosferic", "lr": lr, "epochs": int(_cfg(config, "epochs_stage_1")), "number": 0, "data": "atmospheric"},
            {"name": "Underwater", "lr": lr, "epochs": int(_cfg(config, "epochs_stage_2")), "number": 1, "data": "underwater"}]


def checkpoint_epochs(epochs_stage_1: int, epochs_stage_2: int, save_checkpoint: int) -> List[Tuple[int, int, int]]:
    """[(global epoch, stage index, epoch within the stage)] of every checkpoint but the final one: ``global % save_checkpoint == 0``
    or the last epoch of a stage."""
    out, start = [], 0
    for si, epochs in enumerate((int(epochs_stage_1), int(epochs_stage_2))):
        for e in range(epochs):
            if (start + e) % int(save_checkpoint) == 0 or e == epochs - 1:
                out.append((start + e, si, e))
        start += epochs
    return out


def checkpoint_name(global_epoch: int, stage_name: str, u_name: str, a_name: str, ema: bool = False) -> str:
    """rotinas.py:559 with ``dataset_name = u_name + a_name`` (:706); ``ema``: the averaged weights' sibling."""
    return f"ckpt_{global_epoch}_{stage_name}_{u_name}{a_name}{'_ema' if ema else ''}.pt"


def final_name(total_epochs: int, u_name: str, a_name: str, ema: bool = False) -> str:
    return checkpoint_name(total_epochs, "final", u_name, a_name, ema)


def expected_files(config) -> List[str]:
    """Every file name a complete run leaves under ``<output_path>/ckpt``, sorted."""
    u, a = _cfg(config, "underwater_data_name"), _cfg(config, "atmospheric_data_name")
    plan = stage_plan(config)
    kinds = (False, True) if _cfg(config, "ema_decay", None) is not None else (False,)
    names = [checkpoint_name(g, plan[si]["name"], u, a, k)
             for g, si, _ in checkpoint_epochs(plan[0]["epochs"], plan[1]["epochs"], _cfg(config, "save_checkpoint")) for k in kinds]
    names += [final_name(plan[0]["epochs"] + plan[1]["epochs"], u, a, k) for k in kinds]
    if prediction_settings(config)["prediction"] != "eps":
        names.append(PREDICTION_FILE)
    return sorted(names + [STATE_FILE])


def prediction_settings(config) -> Dict[str, object]:
    """What the network is asked to predict and how the squared error is weighted, validated on the host: ``{"prediction",
    "loss_weighting", "snr_gamma", "y0_divisor"}`` -- the trainer's keywords of those names, the state file's record of them and the
    content of ``prediction.json``.  With none of the keys set: the reference's eps-prediction, unweighted, ``/ 255``."""
    from ..schedules import check_loss_weighting, check_prediction, check_snr_gamma
    y0_divisor = _cfg(config, "y0_divisor", 255.0)
    if isinstance(y0_divisor, bool) or not isinstance(y0_divisor, (int, float)) or y0_divisor != y0_divisor \
            or y0_divisor in (0, float("inf"), -float("inf")):
        raise ValueError(f"hdiff_amd.diffusion.Train: y0_divisor = {y0_divisor!r}; a finite number other than 0")
    return {"prediction": check_prediction(_cfg(config, "prediction", "eps")),
            "loss_weighting": check_loss_weighting(_cfg(config, "loss_weighting", None)),
            "snr_gamma": check_snr_gamma(_cfg(config, "snr_gamma", 5.0)), "y0_divisor": float(y0_divisor)}


def write_prediction_file(ckpt_dir: str, settings: Dict[str, object]) -> str:
    """``<ckpt_dir>/prediction.json`` with the four values; ``Evaluate.resolve_prediction`` reads it.  -> its path."""
    import json
    path = os.path.join(ckpt_dir, PREDICTION_FILE)
    with open(path, "w") as f:
        json.dump(settings, f, indent=1, sort_keys=True)
        f.write("\n")
    return path


def data_plan(config) -> Dict[str, object]:
    """What feeds the run, validated on the host: ``{"device_cache", "cache_dir", "augment" (an ``Augment`` or None), "shuffle",
    "data_seed"}``.  With none of the keys set this is the reference's plan: host ``DataLoader``s, in order, no augmentation."""
    from ..device_data import Augment
    device_cache = bool(_cfg(config, "device_cache", False))
    augment = _cfg(config, "augment", None)
    if isinstance(augment, dict):
        augment = Augment(**augment)
    elif augment is not None and not isinstance(augment, Augment):
        raise TypeError(f"hdiff_amd.diffusion.Train: augment must be an Augment or a dict of its arguments, got {type(augment).__name__}")
    shuffle = bool(_cfg(config, "shuffle", False))
    if (augment is not None or shuffle) and not device_cache:
        raise ValueError("hdiff_amd.diffusion.Train: augment / shuffle need device_cache=True: host transforms cannot be paired (the "
                         "sets call `transforms` once per image, so the two images of a pair would be flipped or cropped independently)")
    data_seed = _cfg(config, "data_seed", None)
    if data_seed is None:
        data_seed = _cfg(config, "seed", None) or 0
    if isinstance(data_seed, bool) or not isinstance(data_seed, int) or not 0 <= data_seed < 2 ** 64:
        raise ValueError(f"hdiff_amd.diffusion.Train: data_seed = {data_seed!r}; an integer in [0, 2^64)")
    cache_dir = _cfg(config, "cache_dir", None)
    if cache_dir is None:
        cache_dir = os.path.join(str(_cfg(config, "output_path")), "cache")
    return {"device_cache": device_cache, "cache_dir": str(cache_dir), "augment": augment, "shuffle": shuffle, "data_seed": data_seed}


def synthetic_plan(config) -> Optional[Dict[str, object]]:
    """The synthetic degradation of the run, validated on the host: ``None`` without the ``synthetic`` key, else ``{"synthetic":
    {"atmospheric": Synth or None, "underwater": Synth or None}, "synthetic_prob", "synthetic_val"}``."""
    from ..synth import Synth
    given = _cfg(config, "synthetic", None)
    if given is None:
        for key in ("synthetic_prob", "synthetic_val"):
            if _cfg(config, key, None) is not None:
                raise ValueError(f"hdiff_amd.diffusion.Train: {key} without synthetic")
        return None
    if not bool(_cfg(config, "device_cache", False)):
        raise ValueError("hdiff_amd.diffusion.Train: synthetic needs device_cache=True: the degradation is drawn on the device, behind "
                         "the batch assembly")
    kinds = ("atmospheric", "underwater")
    if isinstance(given, dict) and given and set(given) <= set(kinds):
        per_stage = {k: None if given.get(k) is None else Synth.from_dict(given[k]) for k in kinds}
    else:
        per_stage = {k: Synth.from_dict(given) for k in kinds}
    if all(v is None for v in per_stage.values()):
        raise ValueError("hdiff_amd.diffusion.Train: synthetic names no stage")
    prob = _cfg(config, "synthetic_prob", None)
    prob = 1.0 if prob is None else prob
    next(v for v in per_stage.values() if v is not None).thresholds(prob)          # refuses a probability outside [0, 1]
    return {"synthetic": per_stage, "synthetic_prob": prob, "synthetic_val": bool(_cfg(config, "synthetic_val", False))}


def _synthetic_record(plan) -> Optional[Dict[str, object]]:
    """What the state file keeps of a ``synthetic_plan``: plain values, comparable with ``==``."""
    if plan is None:
        return None
    return {"synthetic": {k: None if v is None else v.as_dict() for k, v in plan["synthetic"].items()},
            "synthetic_prob": plan["synthetic_prob"], "synthetic_val": plan["synthetic_val"]}


def _schedulers(optimizer, multiplier: float, epochs: int):
    from ..Scheduler import GradualWarmupScheduler
    cosine = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer=optimizer, T_max=epochs, eta_min=0, last_epoch=-1)      # :661-662
    warm = GradualWarmupScheduler(optimizer=optimizer, multiplier=multiplier, warm_epoch=epochs // 10, after_scheduler=cosine)
    return warm, cosine


def lr_sequence(lr: float, multiplier: float, epochs: int) -> List[float]:
    """The learning rate of every epoch of one stage: the driver's schedulers on a dummy CPU optimizer, stepped once per epoch."""
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr)
    warm, _ = _schedulers(opt, multiplier, epochs)
    out = []
    for _ in range(epochs):
        out.append(opt.param_groups[0]["lr"])
        opt.step()
        warm.step()
    return out


def _refuse_data_parallel(config) -> None:
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 or bool(_cfg(config, "DDP", False)):
        raise RuntimeError("hdiff_amd.diffusion.Train.train: data-parallel training of the image-conditioned tree is out of scope "
                           "(WORLD_SIZE > 1 or DDP=True): run one process on one GPU")


def _device(config) -> torch.device:
    devices = _cfg(config, "device_list", None)
    first = devices[0] if devices else "cuda:0"
    device = torch.device("cuda", first) if isinstance(first, int) else torch.device(first)
    if device.type != "cuda":
        raise RuntimeError(f"hdiff_amd.diffusion.Train.train runs on the GPU in fp32 only (there is no CPU path), got device '{device}'")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def _sched_state(warm, cosine) -> Dict[str, dict]:
    return {"warmup": {k: v for k, v in warm.state_dict().items() if k != "after_scheduler"}, "cosine": cosine.state_dict()}


# -- the driver ----------------------------------------------------------------------------------------------------------------
def _validate(trainer, model, loader, device, stage_number: int, max_batches: Optional[int], ema) -> Dict[str, Dict[str, float]]:
    """Mean of the five loss terms over the stage's test loader, for the raw weights and, with an EMA, the averaged ones.  The
    caller's RNG streams (CPU and device) are the same after the call as before it."""
    def one_pass() -> Dict[str, float]:
        torch.manual_seed(VALIDATION_SEED)
        total, n = torch.zeros(len(TERMS), dtype=torch.float64, device=device), 0
        for it, (inp, label) in enumerate(loader):
            if max_batches is not None and it >= max_batches:
                break
            terms = trainer(inp.to(device), label.to(device), stage_number)
            total += torch.stack([v.detach().double().mean() for v in terms])
            n += 1
        vals = (total / max(n, 1)).tolist()
        return {"batches": n, **{k: (v if n else float("nan")) for k, v in zip(TERMS, vals)}}

    was_training = model.training
    model.eval()
    try:
        with torch.random.fork_rng(devices=[device]), torch.no_grad():
            out = {"raw": one_pass()}
            if ema is not None:
                with ema.average_parameters():
                    out["ema"] = one_pass()
    finally:
        model.train(was_training)
    return out


def train(config) -> Dict[str, object]:
    from torch.utils.data import DataLoader
    from .. import optim as hdiff_optim
    from ..datasets import Atmospheric_Dataset, Underwater_Dataset
    from .Diffusion import GaussianDiffusionTrainer
    from .Model import DynamicUNet

    _refuse_data_parallel(config)
    plan = data_plan(config)
    synthetic = synthetic_plan(config)
    predict = prediction_settings(config)
    default_predict = predict == prediction_settings({})
    device = _device(config)
    if _cfg(config, "wandb", False):
        warnings.warn("hdiff_amd.diffusion.Train.train: wandb is not wired; nothing is logged there", RuntimeWarning, stacklevel=2)

    u_name, a_name = _cfg(config, "underwater_data_name"), _cfg(config, "atmospheric_data_name")
    root = _cfg(config, "dataset_root", None)

    def root_of(name):
        return root.get(name) if isinstance(root, dict) else root

    transforms = _cfg(config, "transforms", None)
    batch_size, workers = int(_cfg(config, "batch_size")), int(_cfg(config, "num_workers", 4))

    def loader(data, name, task, kind):                                                             # :602-605
        if not plan["device_cache"]:
            return DataLoader(data, batch_size=batch_size, num_workers=workers, drop_last=True, pin_memory=True)
        from ..device_data import DeviceLoader, build_cache
        cache = build_cache(data, os.path.join(plan["cache_dir"], f"{name}_{task}.pt"), num_workers=workers).to(device)
        train_side = task == "train"
        extra = {}
        if synthetic is not None and synthetic["synthetic"][kind] is not None and (train_side or synthetic["synthetic_val"]):
            extra = dict(synth=synthetic["synthetic"][kind], synth_prob=synthetic["synthetic_prob"],
                         synth_epoch=None if train_side else 0)
        return DeviceLoader(cache, batch_size, shuffle=plan["shuffle"] and train_side, drop_last=True,
                            augment=plan["augment"] if train_side else None, seed=plan["data_seed"], **extra)

    loaders = {(kind, task): loader(cls(name, transforms=transforms, task=task, root=root_of(name)), name, task, kind)
               for kind, cls, name in (("underwater", Underwater_Dataset, u_name), ("atmospheric", Atmospheric_Dataset, a_name))
               for task in ("train", "test")}

    seed = _cfg(config, "seed", None)
    if seed is not None:
        torch.manual_seed(int(seed))
    model = DynamicUNet(T=_cfg(config, "T"), ch=_cfg(config, "channel"), ch_mult=_cfg(config, "channel_mult"),
                        num_res_blocks=_cfg(config, "num_res_blocks"), dropout=_cfg(config, "dropout"))          # :611-612
    pretrained = _cfg(config, "pretrained_path", None)
    if pretrained is not None:
        ckpt = torch.load(pretrained, map_location="cpu")
        model.load_state_dict({k.replace("module.", ""): v for k, v in ckpt.items()})                           # :614-616
    model.to(device).train()
    msssim_loss = _cfg(config, "msssim_loss", None)
    if msssim_loss is None:
        from ..Loss.loss import MSSSIMLoss
        msssim_loss = MSSSIMLoss()
    trainer = GaussianDiffusionTrainer(model, _cfg(config, "beta_1"), _cfg(config, "beta_T"), _cfg(config, "T"),
                                       dino_loss=_cfg(config, "dino_loss", None), msssim_loss=msssim_loss,
                                       extra_losses=_cfg(config, "extra_losses", None),
                                       dino_weights=_cfg(config, "dino_weights", None),
                                       dino_dense=_cfg(config, "dino_dense", None),
                                       **({} if default_predict else predict)).to(device)                       # :629
    ema_decay = _cfg(config, "ema_decay", None)
    ema = hdiff_optim.EMA(model.parameters(), decay=ema_decay) if ema_decay is not None else None

    ckpt_dir = os.path.join(_cfg(config, "output_path"), "ckpt")
    os.makedirs(os.path.join(_cfg(config, "output_path"), "logs"), exist_ok=True)                               # :631-635
    os.makedirs(ckpt_dir, exist_ok=True)
    state_path = os.path.join(ckpt_dir, STATE_FILE)

    stages = stage_plan(config)
    total_epochs = sum(s["epochs"] for s in stages)
    save_every, grad_clip = int(_cfg(config, "save_checkpoint")), _cfg(config, "grad_clip")
    multiplier = _cfg(config, "multiplier")
    step_cap, val_cap = _cfg(config, "max_steps_per_epoch", None), _cfg(config, "max_val_batches", None)
    max_epochs, on_step = _cfg(config, "max_epochs", None), _cfg(config, "on_step", None)

    record = {"losses": {k: [] for k in TERMS}, "lr": [], "validation": [], "files": []}
    num, first_stage, first_epoch, resumed = 0, 0, 0, None
    resume = _cfg(config, "resume", None)
    if resume is not None:
        resumed = torch.load(resume, map_location="cpu", weights_only=False)
        was = resumed.get("prediction", prediction_settings({}))       # a state file from before the keys existed: their defaults
        if was != predict:
            raise RuntimeError(f"hdiff_amd.diffusion.Train.train: the state file was written with {was} and the configuration asks for "
                               f"{predict}: a network goes on being trained for what it was trained for")
        if resumed.get("synthetic", None) != _synthetic_record(synthetic):
            raise RuntimeError(f"hdiff_amd.diffusion.Train.train: the state file was written with synthetic = {resumed.get('synthetic')} "
                               f"and the configuration asks for {_synthetic_record(synthetic)}: a resumed run draws what the "
                               "uninterrupted one draws")
        model.load_state_dict(resumed["model"])
        if (ema is None) != (resumed["ema"] is None):
            raise RuntimeError("hdiff_amd.diffusion.Train.train: the state file and the configuration disagree about ema_decay")
        if ema is not None:
            ema.load_state_dict(resumed["ema"])
        num, record = int(resumed["num"]), resumed["record"]
        first_stage, first_epoch = int(resumed["stage"]), int(resumed["epoch"]) + 1
        if first_stage < len(stages) and first_epoch >= stages[first_stage]["epochs"]:
            first_stage, first_epoch = first_stage + 1, 0          # the next stage starts with a fresh optimizer, as it would have

    def write(name: str, obj) -> None:
        path = os.path.join(ckpt_dir, name)
        torch.save(obj, path)
        if path not in record["files"]:
            record["files"].append(path)

    def write_weights(global_epoch: int, stage_name: str) -> None:
        write(checkpoint_name(global_epoch, stage_name, u_name, a_name), model.state_dict())                    # :555-564
        if ema is not None:
            write(checkpoint_name(global_epoch, stage_name, u_name, a_name, ema=True), ema.shadow_state_dict(model))

    def write_state(si: int, e: int, opt, warm, cosine) -> None:
        if state_path not in record["files"]:
            record["files"].append(state_path)
        torch.cuda.synchronize(device)
        torch.save({"model": model.state_dict(), "ema": None if ema is None else ema.state_dict(),
                    "optimizer": None if opt is None else opt.state_dict(),
                    "schedulers": None if opt is None else _sched_state(warm, cosine),
                    "stage": si, "epoch": e, "num": num, "record": record, "prediction": predict,
                    **({} if synthetic is None else {"synthetic": _synthetic_record(synthetic)}),
                    "rng_cpu": torch.get_rng_state(), "rng_device": torch.cuda.get_rng_state(device)}, state_path)

    if predict["prediction"] != "eps":          # beside the checkpoints, which stay plain state dicts: Evaluate reads it
        path = write_prediction_file(ckpt_dir, predict)
        if path not in record["files"]:
            record["files"].append(path)
    done_epochs = sum(s["epochs"] for s in stages[:first_stage]) + first_epoch
    stopped, opt, warm, cosine = False, None, None, None
    for si in range(first_stage, len(stages)):
        stage = stages[si]
        start = sum(s["epochs"] for s in stages[:si])
        opt = hdiff_optim.AdamW(model.parameters(), lr=stage["lr"], weight_decay=WEIGHT_DECAY)                  # :660
        warm, cosine = _schedulers(opt, multiplier, stage["epochs"])                                            # :661-665
        e0 = 0
        if resumed is not None and si == first_stage:
            if first_epoch > 0:
                opt.load_state_dict(resumed["optimizer"])
                cosine.load_state_dict(resumed["schedulers"]["cosine"])
                warm.load_state_dict(resumed["schedulers"]["warmup"])
                e0 = first_epoch
            torch.set_rng_state(resumed["rng_cpu"])
            torch.cuda.set_rng_state(resumed["rng_device"], device)
            resumed = None
        train_loader, test_loader = loaders[(stage["data"], "train")], loaders[(stage["data"], "test")]
        for e in range(e0, stage["epochs"]):
            current = start + e
            if plan["device_cache"]:
                train_loader.set_epoch(current)
            record["lr"].append(opt.param_groups[0]["lr"])
            sums, steps = torch.zeros(len(TERMS), dtype=torch.float64, device=device), 0
            for it, (inp, label) in enumerate(train_loader):
                if step_cap is not None and it >= step_cap:
                    break
                inp, label = inp.to(device), label.to(device)
                opt.zero_grad()
                terms = trainer(inp, label, stage["number"])                                                     # :439
                terms[0].mean().backward()                                                                       # :443
                opt.step(max_grad_norm=grad_clip)                                                                # :444-445
                if ema is not None:
                    ema.update()
                sums += torch.stack([v.detach().double().mean() for v in terms])
                steps += 1
                num += 1
                if on_step is not None:
                    on_step(num, model)
            means = (sums / max(steps, 1)).tolist()
            for k, v in zip(TERMS, means):
                record["losses"][k].append(v if steps else float("nan"))
            warm.step()                                                                                          # :697
            done_epochs = current + 1
            wrote = False
            if current % save_every == 0 or e == stage["epochs"] - 1:
                write_weights(current, stage["name"])
                val = _validate(trainer, model, test_loader, device, stage["number"], val_cap, ema)
                record["validation"].append({"epoch": current, "stage": stage["name"], **val})
                write_state(si, e, opt, warm, cosine)
                wrote = True
            if max_epochs is not None and done_epochs >= int(max_epochs) and done_epochs < total_epochs:
                if not wrote:
                    write_state(si, e, opt, warm, cosine)
                stopped = True
                break
        if stopped:
            break
    if not stopped:
        write_weights(total_epochs, "final")                                                                     # :731
        write_state(len(stages), -1, opt, warm, cosine)
    return {**record, "steps": num, "epochs": done_epochs, "finished": not stopped}
