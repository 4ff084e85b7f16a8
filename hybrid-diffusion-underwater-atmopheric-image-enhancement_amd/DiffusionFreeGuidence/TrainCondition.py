"""Drop-in for the reference's ``DiffusionFreeGuidence/TrainCondition.py``: ``train(modelConfig)`` and ``eval(modelConfig)``
driven by the same config dict (keys of MainCondition.py:5-29) with the same loop semantics:

  train: AdamW(lr, weight_decay=1e-4); CosineAnnealingLR(T_max=epoch) behind GradualWarmupScheduler(multiplier,
         warm_epoch=epoch//10), stepped per epoch; labels + 1; with probability 0.1 the WHOLE batch's labels are zeroed
         (host numpy RNG); loss = trainer(x_0, labels).sum() / b**2; clip_grad_norm_(grad_clip); one weights-only
         checkpoint ckpt_<e>_.pt per epoch (plain state_dict, loadable by the reference)            [reference :20-72]
  eval:  labels in batch_size//10 contiguous groups (+1); strict load of test_load_weight; sampler from x_T ~ N(0, I);
         noisy and sampled grids saved as PNG (x*0.5+0.5)                                             [reference :75-108]

Differences: the data set.  The reference hard-codes torchvision CIFAR10; here ``modelConfig["dataset"]`` selects
"folder" (``data_dir/<domain>/*.png``: clean image = x_0, domain index = label), "reference_sets" (the reference's own
``data/`` tree of underwater / atmospheric sets, ``hdiff_amd.datasets``), "synthetic", or "cifar10" (only if torchvision is
installed).  Optional keys, all with reference-equivalent defaults: ``num_labels`` (10), ``num_workers`` (4),
``max_steps_per_epoch``; for ``eval`` alone ``ddim_steps`` (absent / None: the reference's T-step ancestral loop; S: the strided DDIM
sampler of ``GaussianDiffusionSampler.forward`` in S model evaluations), ``ddim_eta`` (0.0), ``ddim_clip_x0`` (False), and with ``ddim_steps`` ``ddim_solver`` ("ddim" / "dpmpp2m": DPM-Solver++(2M)) and
``ddim_spacing`` ("uniform" / "logsnr"), passed on as ``solver=`` / ``spacing=`` only when present.  Under ``torch.distributed.run`` (WORLD_SIZE > 1) training is data-parallel: replicated weights,
per-rank shard of every epoch, ONE mean all-reduce of the gradients per step (hdiff_amd.parallel), rank-0 checkpoints.
"""
import os
from typing import Dict, List

import numpy as np
import torch
from torch.utils.data import DataLoader, Subset

from .. import optim as hdiff_optim
from .. import parallel
from ..Scheduler import GradualWarmupScheduler
from ..imageio import ImageDomainFolder, SyntheticDomains, save_image
from .DiffusionCondition import GaussianDiffusionSampler, GaussianDiffusionTrainer
from .ModelCondition import UNet

try:
    from tqdm import tqdm
except Exception:  # pragma: no cover
    def tqdm(it, **_):
        return it

WEIGHT_DECAY = 1e-4          # reference :39-40
LABEL_DROP_PROBABILITY = 0.1  # reference :57: classifier-free guidance trains the unconditional branch on 10 % of the batches
EVAL_LABEL_GROUPS = 10       # reference :79


def _dataset(cfg: Dict):
    kind = cfg.get("dataset", "folder" if cfg.get("data_dir") else "synthetic")
    if kind == "folder":
        return ImageDomainFolder(cfg["data_dir"], cfg["img_size"])
    if kind == "synthetic":
        return SyntheticDomains(cfg.get("synthetic_size", 512), cfg["img_size"], cfg.get("num_labels", 10))
    if kind == "reference_sets":
        # the reference's own data/ tree (utils/utils.py:309-473): reference images of the named underwater and / or
        # atmospheric sets, label = 0 for underwater, 1 for atmospheric
        from ..datasets import (ATMOSPHERIC_DOMAIN, UNDERWATER_DOMAIN, Atmospheric_Dataset, ReferenceImagesWithDomain,
                                Underwater_Dataset)
        sets = []                                     # (set, domain id): the id is fixed per kind, whatever else is configured
        if cfg.get("underwater_dataset"):
            sets.append((Underwater_Dataset(cfg["underwater_dataset"], task="train", root=cfg.get("underwater_root")),
                         UNDERWATER_DOMAIN))
        if cfg.get("atmospheric_dataset"):
            sets.append((Atmospheric_Dataset(cfg["atmospheric_dataset"], task="train", root=cfg.get("atmospheric_root")),
                         ATMOSPHERIC_DOMAIN))
        if not sets:
            raise ValueError("dataset 'reference_sets' needs underwater_dataset and / or atmospheric_dataset")
        return ReferenceImagesWithDomain(sets, cfg["img_size"])
    if kind == "cifar10":
        from torchvision import transforms
        from torchvision.datasets import CIFAR10
        to_unit_range = transforms.Compose([transforms.ToTensor(), transforms.Normalize((0.5,) * 3, (0.5,) * 3)])
        return CIFAR10(root="./CIFAR10", train=True, download=True, transform=to_unit_range)
    raise ValueError(f"unknown dataset kind {kind!r}")


def _epoch_indices(n: int, epoch: int, rank: int, world: int, seed: int = 0):
    """DistributedSampler semantics: one permutation per epoch shared by all ranks, padded to a multiple of world, strided."""
    g = torch.Generator().manual_seed(seed + epoch)
    perm = torch.randperm(n, generator=g).tolist()
    if world > 1:
        total = (n + world - 1) // world * world
        perm = (perm + perm[: total - n])[rank:total:world]
    return perm


def _denoiser(cfg: Dict, device) -> UNet:
    return UNet(T=cfg["T"], num_labels=cfg.get("num_labels", 10), ch=cfg["channel"], ch_mult=cfg["channel_mult"],
                num_res_blocks=cfg["num_res_blocks"], dropout=cfg["dropout"]).to(device)


def _weights_path(cfg: Dict, name: str) -> str:
    return os.path.join(cfg["save_dir"], name)


def _eval_labels(batch: int, num_labels: int) -> torch.Tensor:
    """Sample i gets class min(i // (batch // 10), classes - 1), then + 1 because 0 is the unconditional label (:79-87)."""
    width = max(1, batch // EVAL_LABEL_GROUPS)
    top = min(EVAL_LABEL_GROUPS, num_labels) - 1
    return torch.tensor([min(i // width, top) for i in range(batch)], dtype=torch.long) + 1


def train(modelConfig: Dict) -> List[float]:
    cfg = modelConfig
    rank, local, world = parallel.init_from_env()
    device = torch.device(cfg["device"]) if world == 1 else torch.device("cuda", local)
    data = _dataset(cfg)

    net = _denoiser(cfg, device)
    if cfg["training_load_weight"] is not None:
        net.load_state_dict(torch.load(_weights_path(cfg, cfg["training_load_weight"]), map_location=device), strict=False)
        print("Model weight load down.")
    parallel.broadcast_parameters_(net.parameters())
    weights = list(net.parameters())
    # AdamW(lr, weight_decay = 1e-4) as the reference builds it (TrainCondition.py:39-40): on the GPU the native optimizer, which takes the clip of
    # :61-62 into the same three launches (hdiff_amd/optim.py); the class is a torch.optim.Optimizer, the schedulers below drive it unchanged
    opt = hdiff_optim.AdamW(weights, lr=cfg["lr"], weight_decay=WEIGHT_DECAY)
    flat_grads = parallel.FlatGradients(weights, world, overlap=True) if world > 1 else None   # views of one exchange buffer; bucket reduce-scatters start during backward
    schedule = GradualWarmupScheduler(
        optimizer=opt, multiplier=cfg["multiplier"], warm_epoch=cfg["epoch"] // 10,
        after_scheduler=torch.optim.lr_scheduler.CosineAnnealingLR(optimizer=opt, T_max=cfg["epoch"], eta_min=0, last_epoch=-1))
    objective = GaussianDiffusionTrainer(net, cfg["beta_1"], cfg["beta_T"], cfg["T"]).to(device)
    os.makedirs(cfg["save_dir"], exist_ok=True)
    step_cap = cfg.get("max_steps_per_epoch", 1 << 30)
    losses: List[float] = []

    for epoch in range(cfg["epoch"]):
        shard = Subset(data, _epoch_indices(len(data), epoch, rank, world))
        batches = DataLoader(shard, batch_size=cfg["batch_size"], shuffle=False, num_workers=cfg.get("num_workers", 4),
                             drop_last=True, pin_memory=True)
        progress = tqdm(batches, dynamic_ncols=True, disable=rank != 0)
        for it, (images, domains) in enumerate(progress):
            if it >= step_cap:
                break
            x_0 = images.to(device)
            labels = torch.as_tensor(domains).to(device) + 1
            if np.random.rand() < LABEL_DROP_PROBABILITY:          # one draw per batch, on the host, like the reference
                labels = torch.zeros_like(labels)
            if flat_grads is not None:
                flat_grads.zero_()
            else:
                opt.zero_grad()
            loss = objective(x_0, labels).sum() / x_0.shape[0] ** 2.
            loss.backward()
            if flat_grads is not None:
                flat_grads.exchange_mean_()                        # the one collective of a step (mean over ranks)
            opt.step(max_grad_norm=cfg["grad_clip"])               # clip_grad_norm_(weights, grad_clip); opt.step()
            losses.append(loss.item())
            if hasattr(progress, "set_postfix"):
                progress.set_postfix(ordered_dict={"epoch": epoch, "loss: ": losses[-1], "img shape: ": tuple(x_0.shape),
                                                   "LR": opt.param_groups[0]["lr"]})
        schedule.step()
        if rank == 0:
            torch.save(net.state_dict(), _weights_path(cfg, f"ckpt_{epoch}_.pt"))
    return losses


def eval(modelConfig: Dict) -> torch.Tensor:
    cfg = modelConfig
    device = torch.device(cfg["device"])
    batch, side = cfg["batch_size"], cfg["img_size"]
    with torch.no_grad():
        labels = _eval_labels(batch, cfg.get("num_labels", 10)).to(device)
        print("labels: ", labels)
        net = _denoiser(cfg, device)
        net.load_state_dict(torch.load(_weights_path(cfg, cfg["test_load_weight"]), map_location=device))
        print("model load weight done.")
        net.eval()
        sampler = GaussianDiffusionSampler(net, cfg["beta_1"], cfg["beta_T"], cfg["T"], w=cfg["w"]).to(device)
        x_T = torch.randn(size=[batch, 3, side, side], device=device)
        save_image(torch.clamp(x_T * 0.5 + 0.5, 0, 1), os.path.join(cfg["sampled_dir"], cfg["sampledNoisyImgName"]),
                   nrow=cfg["nrow"])
        if cfg.get("ddim_steps") is None:
            images = sampler(x_T, labels) * 0.5 + 0.5               # [-1, 1] -> [0, 1]
        else:
            solver_kw = {kw: cfg[key] for kw, key in (("solver", "ddim_solver"), ("spacing", "ddim_spacing"))
                         if cfg.get(key) is not None}
            images = sampler(x_T, labels, ddim_steps=int(cfg["ddim_steps"]), eta=float(cfg.get("ddim_eta", 0.0)),
                             clip_x0=bool(cfg.get("ddim_clip_x0", False)), **solver_kw) * 0.5 + 0.5
        save_image(images, os.path.join(cfg["sampled_dir"], cfg["sampledImgName"]), nrow=cfg["nrow"])
        return images
