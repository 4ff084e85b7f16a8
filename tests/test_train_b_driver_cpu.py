"""Host-only pieces of the second tree's training driver (hdiff_amd.diffusion.Train, reference utils/rotinas.py:571-732): the stage
plan, which epochs checkpoint, the file names, the learning-rate sequence, and what the driver and optim.EMA refuse."""
import math
import os
import re
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hdiff_amd  # noqa: E402
from hdiff_amd import _capi  # noqa: E402
from hdiff_amd import optim as HO  # noqa: E402
from hdiff_amd.Scheduler import GradualWarmupScheduler  # noqa: E402
from hdiff_amd.diffusion import Train as TR  # noqa: E402


def config(**kw):
    base = dict(underwater_data_name="HICRD", atmospheric_data_name="LoLI", T=1000, channel=32, channel_mult=[1, 2, 2],
                num_res_blocks=1, dropout=0.15, lr=1e-4, multiplier=2.5, beta_1=1e-4, beta_T=0.02, grad_clip=1.0, batch_size=2,
                epochs_stage_1=2, epochs_stage_2=2, save_checkpoint=1, output_path="unused", pretrained_path=None,
                device_list=["cuda:0"])
    base.update(kw)
    return base


def test_stage_plan_names_numbers_and_sets():
    for cfg in (config(epochs_stage_1=3, epochs_stage_2=5, lr=2e-5), types.SimpleNamespace(**config(epochs_stage_1=3, epochs_stage_2=5,
                                                                                                    lr=2e-5))):
        plan = TR.stage_plan(cfg)
        assert [(s["name"], s["number"], s["epochs"], s["lr"], s["data"]) for s in plan] == \
            [("Atmosferic", 0, 3, 2e-5, "atmospheric"), ("Underwater", 1, 5, 2e-5, "underwater")]      # rotinas.py:643-646, 668-673


def test_checkpoint_epochs():
    """global % save_checkpoint == 0, or the last epoch of a stage: (global epoch, stage, epoch within the stage)."""
    assert TR.checkpoint_epochs(3, 2, 2) == [(0, 0, 0), (2, 0, 2), (4, 1, 1)]
    assert TR.checkpoint_epochs(1, 1, 200) == [(0, 0, 0), (1, 1, 0)]
    assert TR.checkpoint_epochs(10, 10, 4) == [(0, 0, 0), (4, 0, 4), (8, 0, 8), (9, 0, 9), (12, 1, 2), (16, 1, 6), (19, 1, 9)]


def test_file_names():
    assert TR.checkpoint_name(7, "Atmosferic", "HICRD", "LoLI") == "ckpt_7_Atmosferic_HICRDLoLI.pt"            # rotinas.py:559, :706
    assert TR.checkpoint_name(7, "Underwater", "LSUI", "HDR", ema=True) == "ckpt_7_Underwater_LSUIHDR_ema.pt"
    assert TR.final_name(20, "HICRD", "LoLI") == "ckpt_20_final_HICRDLoLI.pt"                                   # :731
    assert TR.final_name(20, "HICRD", "LoLI", ema=True) == "ckpt_20_final_HICRDLoLI_ema.pt"
    assert TR.STATE_FILE == "state_last.pt"
    assert TR.expected_files(config(epochs_stage_1=3, epochs_stage_2=2, save_checkpoint=2)) == sorted(
        ["ckpt_0_Atmosferic_HICRDLoLI.pt", "ckpt_2_Atmosferic_HICRDLoLI.pt", "ckpt_4_Underwater_HICRDLoLI.pt",
         "ckpt_5_final_HICRDLoLI.pt", "state_last.pt"])
    with_ema = TR.expected_files(config(epochs_stage_1=1, epochs_stage_2=1, save_checkpoint=200, ema_decay=0.99))
    assert with_ema == sorted(["ckpt_0_Atmosferic_HICRDLoLI.pt", "ckpt_0_Atmosferic_HICRDLoLI_ema.pt", "ckpt_1_Underwater_HICRDLoLI.pt",
                               "ckpt_1_Underwater_HICRDLoLI_ema.pt", "ckpt_2_final_HICRDLoLI.pt", "ckpt_2_final_HICRDLoLI_ema.pt",
                               "state_last.pt"])


def reference_lrs(lr, multiplier, epochs):
    """torch's CosineAnnealingLR behind Scheduler.GradualWarmupScheduler on a dummy CPU optimizer, as rotinas.py:660-665, 697."""
    opt = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(2))], lr=lr, weight_decay=1e-4)
    cos = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer=opt, T_max=epochs, eta_min=0, last_epoch=-1)
    warm = GradualWarmupScheduler(optimizer=opt, multiplier=multiplier, warm_epoch=epochs // 10, after_scheduler=cos)
    out = []
    for _ in range(epochs):
        out.append(opt.state_dict()["param_groups"][0]["lr"])
        opt.step()
        warm.step()
    return out


@pytest.mark.parametrize("epochs", [1, 2, 3, 10, 25])
def test_lr_sequence_of_a_stage(epochs):
    got = TR.lr_sequence(1e-4, 2.5, epochs)
    assert got == reference_lrs(1e-4, 2.5, epochs) and len(got) == epochs
    warm = epochs // 10
    # the ramp: base at epoch 0, base * multiplier at epoch warm_epoch; a warm-up of no epochs starts at the peak
    assert got[0] == pytest.approx(1e-4 if warm else 2.5e-4, rel=1e-12)
    assert got[warm] == pytest.approx(2.5e-4, rel=1e-12)
    for e in range(warm):
        assert got[e] == pytest.approx(1e-4 * (1 + 1.5 * e / warm), rel=1e-12)
    assert all(math.isfinite(v) and v > 0 for v in got)


def test_both_stages_restart_the_schedule():
    cfg = config(epochs_stage_1=10, epochs_stage_2=25)
    seqs = [TR.lr_sequence(s["lr"], cfg["multiplier"], s["epochs"]) for s in TR.stage_plan(cfg)]
    assert seqs[0] == reference_lrs(1e-4, 2.5, 10) and seqs[1] == reference_lrs(1e-4, 2.5, 25)
    assert seqs[0][0] == seqs[1][0] == 1e-4


def test_data_parallel_is_refused(monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="data-parallel training .* out of scope"):
        TR.train(config())
    monkeypatch.setenv("WORLD_SIZE", "1")
    with pytest.raises(RuntimeError, match="data-parallel training .* out of scope"):
        TR.train(config(DDP=True))


def test_driver_and_ema_refuse_the_cpu(monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(RuntimeError, match="GPU in fp32 only .*no CPU path"):
        TR.train(config(device_list=["cpu"]))
    p = torch.nn.Parameter(torch.randn(8))
    with pytest.raises(RuntimeError, match=re.escape("hdiff_amd.optim.EMA runs on the GPU in fp32 only (there is no CPU path)")):
        HO.EMA([p], decay=0.9)
    with pytest.raises(ValueError, match="decay"):
        HO.EMA([p], decay=1.5)


def test_ema_entry_point_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "hdiff.h")).read()
    assert re.search(r"\bint\s+hdiff_ema_update\s*\(\s*const\s+hdiff_ema_tensor\s*\*", header)
    assert re.search(r"typedef\s+struct\s*\{\s*float\s*\*\s*avg;\s*const\s+float\s*\*\s*p;\s*long\s+long\s+n;\s*\}\s*hdiff_ema_tensor;", header)
    assert "hdiff_ema_update" in _capi._PROTOS
    assert hasattr(hdiff_amd.lib(), "hdiff_ema_update")
    assert "#define HDIFF_ABI_VERSION 6" in header or hdiff_amd.lib().hdiff_abi_version() == 6      # an addition only
