"""The DINOv2 perceptual loss without a GPU: the definition (tests/_dino_def.py) against torch's own operators in float64, the tap
list, the checkpoint's names, the position-embedding resize, and what is refused."""
import json
import os
import sys
import warnings

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _dino_def as D  # noqa: E402
import hdiff_amd  # noqa: F401,E402
from hdiff_amd import dino  # noqa: E402
from hdiff_amd.Loss import loss as L  # noqa: E402
from hdiff_amd.diffusion import Diffusion as DB  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
RTOL = 1e-12


def close(a, b):
    return float((a - b).abs().max()) <= RTOL * float(b.abs().max())


def test_definition_pieces_agree_with_torch_in_float64():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 7, 48, generator=g, dtype=torch.float64) * 3 + 1
    ln = nn.LayerNorm(48, eps=1e-6).double()
    with torch.no_grad():
        ln.weight.copy_(torch.randn(48, generator=g, dtype=torch.float64))
        ln.bias.copy_(torch.randn(48, generator=g, dtype=torch.float64))
        assert close(D.layer_norm(x, ln.weight, ln.bias), ln(x))
    assert close(D.gelu(x), F.gelu(x))
    qkv = torch.randn(2, 7, 3 * 48, generator=g, dtype=torch.float64)
    q, k, v = qkv.reshape(2, 7, 3, 3, 16).permute(2, 0, 3, 1, 4)
    want = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(2, 7, 48)
    assert close(D.attention(qkv, 3), want)
    img = torch.randn(2, 3, 32, 46, generator=g, dtype=torch.float64)
    conv = nn.Conv2d(3, 8, 14, 14).double()
    with torch.no_grad():
        want = conv(D.crop(img)).flatten(2).transpose(1, 2)
        got = D.unfold(D.crop(img)) @ conv.weight.reshape(8, -1).t() + conv.bias
    assert tuple(D.crop(img).shape) == (2, 3, 28, 42) and close(got, want)
    a, b = torch.randn(500, generator=g, dtype=torch.float64) * 2, torch.randn(500, generator=g, dtype=torch.float64)
    assert abs(float(D.smooth_l1(a - b).mean()) - float(F.smooth_l1_loss(a, b))) <= RTOL * float(F.smooth_l1_loss(a, b))


def test_tap_list_counts_selection_and_unknown_names():
    taps = dino.default_taps(2)
    assert len(taps) == 2 * 10 + 4 and sum(m for _, _, m in taps) == 2 * 15 + 6
    assert all(m == len(names) for names, _, m in taps)
    assert [(k, m) for _, k, m in taps] == D.tap_list(2)
    assert len(dino.default_taps(12)) == 124
    names = [n for ns, _, _ in taps for n in ns]
    assert "" in names and "head" in names and not any("attn_drop" in n or "drop_path" in n for n in names)
    assert names.count("blocks.0.mlp.drop") == 2                       # called twice per block: two tensors
    sel = dino.select_taps(2, ["blocks.1.attn", "blocks.1.attn.proj", "norm", "blocks.0.mlp.drop"])
    assert [(k, m) for _, k, m in sel] == [("0.act", 1), ("0.fc2", 1), ("1.proj", 2), ("norm", 1)]
    with pytest.raises(ValueError, match="unknown module names"):
        dino.select_taps(2, ["blocks.2.norm1"])
    with pytest.raises(ValueError, match="unknown module names"):
        dino.select_taps(2, ["blocks.0.attn.attn_drop"])
    with pytest.raises(ValueError):
        L.PerceptualLoss_dino(layers=["nope"], trunk=dino.DinoV2Features(embed_dim=16, depth=1, heads=1, pos_grid=3))


def test_state_dict_names_order_and_shapes_and_strict_loading():
    want = json.load(open(os.path.join(GOLDEN, "state_dict_dinov2_vits14.json")))
    trunk = dino.DinoV2Features("dinov2_vits14")
    sd = trunk.state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == want
    assert [k for k, _ in want] == D.state_names(12)
    assert not any(p.requires_grad for p in trunk.parameters()) and not trunk.training
    assert {k: dino.DINO_CFGS[k] for k in dino.DINO_CFGS} == {
        "dinov2_vits14": dict(embed_dim=384, depth=12, heads=6), "dinov2_vitb14": dict(embed_dim=768, depth=12, heads=12),
        "dinov2_vitl14": dict(embed_dim=1024, depth=24, heads=16)}
    small = dino.DinoV2Features(embed_dim=32, depth=2, heads=2, pos_grid=5)
    state = D.make_state(32, 2, 5, seed=1)
    assert list(small.state_dict()) == list(state)
    small.load_dinov2(state)
    assert small.pretrained and all(torch.equal(small.state_dict()[k], state[k]) for k in state)
    # the attention kernels read the qkv rows in the checkpoint's order ([Q | K | V], head-major inside each): nothing is permuted
    assert torch.equal(small.blocks[0].attn.qkv.weight, state["blocks.0.attn.qkv.weight"])
    for bad, what in (({k: v for k, v in state.items() if k != "norm.bias"}, "missing keys"),
                      ({**state, "blocks.2.ls1.gamma": torch.zeros(32)}, "unexpected keys"),
                      ({**state, "register_tokens": torch.zeros(1, 4, 32)}, "unexpected keys"),
                      ({**state, "cls_token": torch.zeros(1, 1, 16)}, "has shape")):
        with pytest.raises(RuntimeError, match=what):
            dino.DinoV2Features(embed_dim=32, depth=2, heads=2, pos_grid=5).load_dinov2(bad)


def test_position_embedding_resize():
    g = torch.Generator().manual_seed(3)
    pos = torch.randn(1, 1 + 37 * 37, 8, generator=g)
    assert dino.resize_pos_embed(pos, 37, 37) is pos                      # identity at the native grid
    got = dino.resize_pos_embed(pos, 18, 18)
    grid = pos[:, 1:].reshape(1, 37, 37, 8).permute(0, 3, 1, 2)
    want = F.interpolate(grid, scale_factor=((18 + 0.1) / 37, (18 + 0.1) / 37), mode="bicubic", align_corners=False, antialias=False)
    assert tuple(got.shape) == (1, 1 + 18 * 18, 8) and torch.equal(got[:, 0], pos[:, 0])
    assert torch.equal(got[:, 1:], want.permute(0, 2, 3, 1).reshape(1, 324, 8))
    assert torch.equal(got, D.resize_pos(pos, 18, 18))
    rect = dino.resize_pos_embed(pos, 2, 3)
    assert tuple(rect.shape) == (1, 7, 8) and torch.equal(rect, D.resize_pos(pos, 2, 3))


def test_refusals():
    for H, W in ((256, 255), (17, 18), (4, 18), (30, 32)):
        with pytest.raises(RuntimeError, match=f"{H} x {W}"):
            dino.grid_of(H, W)
    assert dino.grid_of(256, 256) == (18, 18) and dino.grid_of(18, 32) == (1, 2)
    for name in ("dinov2_vitg14", "dinov2_vits14_reg", "dinov2_vitb14_reg", "vit_small"):
        with pytest.raises(ValueError, match="dinov2_vits14"):
            L.PerceptualLoss_dino(name)
        with pytest.raises(ValueError, match="dinov2_vits14"):
            dino.DinoV2Features(name)
    with pytest.raises(ValueError, match="version 'dino'"):
        L.PerceptualLoss_dino("dino_vits16", version="dino")
    with pytest.raises(NotImplementedError, match="normalize_inputs"):
        L.PerceptualLoss_dino(normalize_inputs=True)
    with pytest.raises(ValueError, match="head dim"):
        dino.DinoV2Features(embed_dim=30, depth=1, heads=3)
    assert "PerceptualLoss_dino" in L.__all__


def test_native_loss_names_the_device_requirement_on_the_cpu():
    trunk = dino.DinoV2Features(embed_dim=16, depth=1, heads=1, pos_grid=3)
    loss = L.PerceptualLoss_dino(trunk=trunk)
    with pytest.raises(RuntimeError, match="MI355X"):
        loss(torch.zeros(1, 3, 18, 18), torch.zeros(1, 3, 18, 18))
    tr = DB.GaussianDiffusionTrainer(nn.Linear(1, 1), 1e-4, 0.02, 10, dino_loss="native")
    assert isinstance(tr.loss_perceptual_dino, L.PerceptualLoss_dino) and tr.loss_perceptual_dino.perceptual.model_name == "dinov2_vits14"
    assert len(tr.loss_perceptual_dino.taps) == 124
    assert not any(p.requires_grad for p in tr.loss_perceptual_dino.parameters())
    img = torch.zeros(1, 3, 18, 18, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="MI355X"):
        tr(img, img, 0)
    with pytest.raises(ValueError, match="native"):
        DB.GaussianDiffusionTrainer(nn.Linear(1, 1), 1e-4, 0.02, 10, dino_loss="hub")
    with pytest.raises(ValueError, match="dino_weights"):
        DB.GaussianDiffusionTrainer(nn.Linear(1, 1), 1e-4, 0.02, 10, dino_weights={})
    with pytest.raises(ValueError, match="dinov2_vits14"):
        DB.GaussianDiffusionTrainer(nn.Linear(1, 1), 1e-4, 0.02, 10, "vgg16", "dinov2_vitg14", dino_loss="native")


def test_without_the_new_arguments_the_trainer_is_what_it_was():
    tr = DB.GaussianDiffusionTrainer(nn.Linear(1, 1), 1e-4, 0.02, 10)
    assert tr.loss_perceptual_dino is None and tr.ms_ssim_loss is None and tr.extra_losses == () and tr.perceptual_dino == "dinov2_vits14"
    assert [n for n, _ in tr.named_children()] == ["model"]
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        tr._warn_missing()
        tr._warn_missing()
    assert len(seen) == 1 and issubclass(seen[0].category, RuntimeWarning)
    text = str(seen[0].message)
    assert "the DINOv2 perceptual loss 'dinov2_vits14' (weight 0.5)" in text and "the MS-SSIM loss (weight 0.0045)" in text
    assert "pass dino_loss= / msssim_loss=" in text
    with pytest.raises(TypeError, match="unexpected keyword argument 'dino'"):
        DB.GaussianDiffusionTrainer(nn.Linear(1, 1), 1e-4, 0.02, 10, dino=1)


def test_fixtures_hold_their_conditions():
    """From the definition alone: at least 5 % of the tap elements in each smooth-L1 branch, no |a - b| within 2e-5 of 1."""
    for name in D.FIXTURES:
        quad, lin, gap = D.check_fixture(*D.fixture(name))
        assert quad >= 0.05 and lin >= 0.05 and gap > D.MARGIN, (name, quad, lin, gap)
