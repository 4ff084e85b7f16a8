"""Models whose weights are not stored with their golden vectors but rebuilt from the seed recipe of oracle/gen_golden.py
(the build's UNet initialises bit-identically to the reference under the same torch seed; checksums pin it)."""
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def state_checksums(sd):
    names = sorted(sd.keys())
    rows = []
    for n in names:
        bits = sd[n].detach().float().contiguous().reshape(-1).view(torch.int32).to(torch.int64)
        rows.append([int(bits.sum().item()), bits.numel(), int(bits[0].item()), int(bits[-1].item())])
    return names, np.array(rows, dtype=np.int64)


def wide_model(UNet):
    """G3c (tests/golden/unet_wide.npz): ch = 32, ch_mult = [1, 2, 3, 4] -> attention heads of 4 / 8 / 12 / 16 channels.
    Returns (model on the CPU in eval mode, config dict, npz)."""
    d = np.load(os.path.join(GOLDEN, "unet_wide.npz"))
    c = json.loads(bytes(d["cfg_json"]).decode())
    seed = int(d["seed"][0])
    torch.manual_seed(seed)
    m = UNet(**c)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in sorted(m.named_parameters()):
            if n.endswith("in_proj_bias") or n.endswith("out_proj.bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
        table = "time_embedding.timembedding.0.weight"      # sin/cos table: last-bit differences between CPU generations
        assert (m.state_dict()[table] - torch.from_numpy(d["temb_rows"])).abs().max().item() < 1e-5
        m.time_embedding.timembedding[0].weight.copy_(torch.from_numpy(d["temb_rows"]))
    names, sums = state_checksums(m.state_dict())
    assert list(d["weight_names"]) == names
    bad = [n for n, a, b in zip(names, sums, d["weight_checksums"]) if not np.array_equal(a, b)]
    assert not bad, f"seed recipe no longer reproduces the reference init for {bad[:8]} ({len(bad)} tensors)"
    return m.eval(), c, d


def default_trainer_model(UNet):
    """G6b (tests/golden/trainer_default64.npz): the default configuration with dropout 0, weights from the seed recipe of G4
    (torch.manual_seed(seed); the checksums of G4 pin that init) plus the seeded MHA-bias perturbation; the sinusoidal rows
    the recorded time steps use come from the fixture (last-bit differences between CPU generations).
    Returns (model on the CPU in train mode, config dict, npz)."""
    d = np.load(os.path.join(GOLDEN, "trainer_default64.npz"))
    c = json.loads(bytes(d["cfg_json"]).decode())
    seed = int(d["seed"][0])
    torch.manual_seed(seed)
    m = UNet(**c)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in sorted(m.named_parameters()):
            if n.endswith("in_proj_bias") or n.endswith("out_proj.bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
        rows = torch.from_numpy(d["temb_rows"])
        for i, t in enumerate(d["t"].tolist()):
            assert (m.time_embedding.timembedding[0].weight[t] - rows[i]).abs().max().item() < 1e-3
            m.time_embedding.timembedding[0].weight[t].copy_(rows[i])
    return m.train(), c, d



def reference_schedules(d, i):
    """The schedule buffers of the reference's trainer and sampler (DiffusionCondition.py:26-35, 60-66) for config `i` of
    schedules.npz, evaluated in float64 from the fixture's betas in the reference's order of operations, with torch's sqrt:
    what the reference computes on THIS host.  torch's float64 sqrt is not correctly rounded and its last bit depends on the
    host CPU, so the stored buffers carry the bits of the CPU that generated them."""
    betas = np.asarray(d[f"cfg{i}/trainer/betas"], dtype=np.float64)

    def sqrt(a):
        return torch.sqrt(torch.from_numpy(np.ascontiguousarray(a))).numpy()
    alphas = 1.0 - betas
    alphas_bar = np.cumprod(alphas)
    alphas_bar_prev = np.concatenate([[1.0], alphas_bar[:-1]])
    coeff1 = sqrt(1.0 / alphas)
    return {"trainer": {"betas": betas, "sqrt_alphas_bar": sqrt(alphas_bar), "sqrt_one_minus_alphas_bar": sqrt(1.0 - alphas_bar)},
            "sampler": {"betas": betas, "coeff1": coeff1, "coeff2": coeff1 * (1.0 - alphas) / sqrt(1.0 - alphas_bar),
                        "posterior_var": betas * (1.0 - alphas_bar_prev) / (1.0 - alphas_bar)}}


def assert_schedule_buffer(got, host, stored, what):
    """`got` (the code under test) must equal the reference's formula on this host (`host`, reference_schedules) bit for bit,
    and that must equal the stored buffer bit for bit -- or, on a host whose torch sqrt rounds differently from the generating
    CPU's, lie within four units in the last place of it (coeff2 holds two square roots, each up to one unit apart between
    hosts, and a product and a quotient that round once more each)."""
    got, host, stored = np.asarray(got), np.asarray(host), np.asarray(stored)
    assert got.dtype == stored.dtype and got.shape == stored.shape, what
    assert np.array_equal(got, host), what
    if not np.array_equal(host, stored):
        assert (np.abs(host - stored) <= 4 * np.spacing(np.abs(stored))).all(), what


def default32_trainer_model(UNet, peaked=False):
    """G10 (tests/golden/trainer_default32_b80.npz): the default configuration at T = 500 with dropout 0 from G6b's seed recipe;
    the tensors a host's CPU could round differently (sinusoidal table, label embedding, perturbed MHA biases) come from the
    fixture, every tensor is then pinned by its checksum.  ``peaked``: the fixture's second variant (q and k rows of every
    in_proj_weight times sqrt(3)).  Returns (model on the CPU in train mode, config dict, npz)."""
    from oracle.gen_golden import g10_peaked_
    d = np.load(os.path.join(GOLDEN, "trainer_default32_b80.npz"))
    c = json.loads(bytes(d["cfg_json"]).decode())
    torch.manual_seed(int(d["seed"][0]))
    m = UNet(**c)
    with torch.no_grad():
        sd = m.state_dict()
        for n in d["stored_names"]:
            sd[str(n)].copy_(torch.from_numpy(d[f"init/{n}"]))
        # the sinusoidal table: its low bits depend on the host's vectorised sin / cos (as in G6b: up to ~1e-4 at large
        # positions); the rows the recorded time steps read are stored
        table = "time_embedding.timembedding.0.weight"
        idx, rows = torch.from_numpy(d["temb_t"]), torch.from_numpy(d["temb_rows"])
        assert (sd[table][idx] - rows).abs().max().item() < 1e-3
        sd[table][idx] = rows
    names, sums = state_checksums(m.state_dict())
    assert list(d["weight_names"]) == names
    bad = [n for n, a, b in zip(names, sums, d["weight_checksums"]) if n != table and not np.array_equal(a, b)]
    assert not bad, f"seed recipe no longer reproduces the reference init for {bad[:8]} ({len(bad)} tensors)"
    if peaked:
        g10_peaked_(m)
    return m.train(), c, d
