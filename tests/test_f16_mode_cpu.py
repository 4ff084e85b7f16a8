"""The opt-in "f16" contraction mode without a GPU: the switch through every layer, the yardstick of its error class
(tests/_f16_attention_emul.py) on the seeded cases of its table, and the error class at network level through the CPU oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import hdiff_amd  # noqa: E402
import _f16_attention_emul as EM  # noqa: E402
from test_gpu_ops import _h2_case  # noqa: E402   (inputs only: nothing of that module runs here)

GOLDEN = os.path.join(HERE, "golden")


def test_mode_2_through_the_c_abi_and_python():
    hdiff_amd.build()
    lib = hdiff_amd.lib()
    start = lib.hdiff_get_contraction_mode()
    try:
        assert lib.hdiff_set_contraction_mode(2) == 0 and lib.hdiff_get_contraction_mode() == 2
        assert hdiff_amd.get_contraction_mode() == "f16"
        assert lib.hdiff_set_contraction_mode(7) != 0 and b"unknown mode" in lib.hdiff_last_error()
        assert lib.hdiff_set_contraction_mode(3) != 0 and lib.hdiff_get_contraction_mode() == 2
        hdiff_amd.set_contraction_mode("bf16x3")
        assert lib.hdiff_get_contraction_mode() == 1
        hdiff_amd.set_contraction_mode("f16")
        assert lib.hdiff_get_contraction_mode() == 2
        with pytest.raises(ValueError):
            hdiff_amd.set_contraction_mode("fp8")
        assert hdiff_amd.get_contraction_mode() == "f16"
    finally:
        lib.hdiff_set_contraction_mode(start)
    assert lib.hdiff_abi_version() == 6


def test_environment_variable_selects_the_mode_at_start():
    hdiff_amd.build()
    code = "import sys; sys.path.insert(0, %r); import hdiff_amd; print('MODE', hdiff_amd.lib().hdiff_get_contraction_mode())" % ROOT
    for value, want in (("f16", 2), (None, 1)):
        env = {k: v for k, v in os.environ.items() if k != "HDIFF_CONTRACT"}
        if value is not None:
            env["HDIFF_CONTRACT"] = value
        res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
        assert res.returncode == 0 and f"MODE {want}" in res.stdout, (value, res.stdout[-500:], res.stderr[-2000:])


# rms of the emulation against exact float64 attention (heads 8, one sample, L = 2048; error divided by each channel row's largest
# output; offsets 0, 1/4, 1/2, 3/4), as tabulated with the mode's definition: (d_head 16, d_head 32)
TABLE_RMS = {"ramp": (2.0e-4, 1.8e-4), "peaked": (3.4e-4, 3.0e-4), "late-spikes": (4.9e-4, 5.4e-4), "wide-v": (7.0e-5, 6.5e-5),
             "tiny-v": (1.1e-4, 1.1e-4), "quiet-neighbour": (2.0e-4, 1.8e-4), "uniform": (3.1e-3, 3.6e-3)}
SEEDS = {"ramp": 1, "peaked": 2, "late-spikes": 3, "wide-v": 4, "tiny-v": 5, "quiet-neighbour": 6, "uniform": 7}


@pytest.mark.parametrize("d", [16, 32])
@pytest.mark.parametrize("name", list(TABLE_RMS))
def test_yardstick_reproduces_its_table(name, d):
    """a broken yardstick must not wave a broken kernel through: finite, and each rms within 0.5x .. 2x of the table's"""
    g = torch.Generator().manual_seed(SEEDS[name])
    if name == "uniform":
        qkv = torch.randn(1, 3 * 8 * d, 2048, generator=g)
        qkv[:, :2 * 8 * d] *= 0.05
    else:
        qkv = _h2_case(name, d, 2048, g)
    ref = EM.exact(qkv, 8)
    want = TABLE_RMS[name][0 if d == 16 else 1]
    for off in (0.0, 0.25, 0.5, 0.75):
        out = EM.emulate(qkv, 8, off)
        assert torch.isfinite(out).all()
        rms, worst = EM.errors(out, ref)
        print(f"emulation {name} d={d} offset {off}: rms {rms:.3e} worst {worst:.3e}")
        assert 0.5 * want <= rms <= 2.0 * want, (name, d, off, rms, want)


def test_round_sig11_is_fp16_rounding_on_normal_numbers():
    g = torch.Generator().manual_seed(0)
    p = torch.exp2(torch.rand(100000, generator=g) * 28 - 13)       # fp32 values in 2^-13 .. 2^15: normal fp16 numbers
    assert torch.equal(EM.round_sig11(p.double()), p.half().double())


def test_network_level_error_class_default64():
    """The default model at 64x64 through the CPU oracle with the emulated attention core: every offset's rms departure from the
    exact oracle stays inside [2e-5, 3e-4] (output rms 0.32).  Offsets differ from each other by as much as either departs: at
    network level only the error class can be compared, never elements."""
    from hdiff_amd.DiffusionFreeGuidence import ModelCondition as MC
    from oracle import cpu_path as O
    d = np.load(os.path.join(GOLDEN, "unet_default64.npz"))
    c = json.loads(bytes(d["cfg_json"]).decode())
    torch.manual_seed(int(d["seed"][0]))
    m = MC.UNet(**c).eval()
    with torch.no_grad():
        m.time_embedding.timembedding[0].weight[417].copy_(torch.from_numpy(d["temb_row_417"]))
    cfg = O.UNetConfig(T=c["T"], num_labels=c["num_labels"], ch=c["ch"], ch_mult=tuple(c["ch_mult"]),
                       num_res_blocks=c["num_res_blocks"], dropout=c["dropout"])
    sd = dict(m.state_dict())
    x, t, labels = torch.from_numpy(d["x"]), torch.from_numpy(d["t"]), torch.tensor([1])
    with torch.no_grad():
        exact = O.unet_forward(sd, cfg, x, t, labels)
        assert torch.allclose(exact, torch.from_numpy(d["eps_label1"]), atol=1e-4)
        exact = exact.double()
        for off in EM.OFFSETS8:
            with EM.oracle_with_emulated_attention(off):
                y = O.unet_forward(sd, cfg, x, t, labels).double()
            assert O.mha_self_attention.__module__ == "oracle.cpu_path"
            rms, worst = (y - exact).pow(2).mean().sqrt().item(), (y - exact).abs().max().item()
            print(f"default64 with emulated attention, offset {off}: rms departure {rms:.3e}, worst {worst:.3e}")
            assert 2e-5 <= rms <= 3e-4, (off, rms)
