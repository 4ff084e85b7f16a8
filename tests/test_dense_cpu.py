"""The token-axis dense layer without a GPU: the symbols, the pack arithmetic, what the launcher refuses, the route decision, and the
proof that the accuracy gate of tests/test_gpu_dense.py bites -- the kernel's arithmetic emulated in numpy (tests/_dense_def.py) passes
it, the same arithmetic with any ONE of the six piece products left out does not."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _dense_def as DD  # noqa: E402
import hdiff_amd  # noqa: E402
from hdiff_amd import _capi, dino  # noqa: E402
from hdiff_amd.Loss import loss as L  # noqa: E402
from hdiff_amd.diffusion import Diffusion as DB  # noqa: E402

NEW_SYMBOLS = {"hdiff_dense_pack_words", "hdiff_dense_pack", "hdiff_dense_tokens"}
YARD = 4.0


def test_symbols_are_declared_exported_and_bound_with_abi_6():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hdiff.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(hdiff_[a-z0-9_]+)\s*\(", text))
    assert NEW_SYMBOLS <= declared
    assert NEW_SYMBOLS <= set(_capi.EXPORTED_SYMBOLS)
    lib = hdiff_amd.lib()
    assert lib.hdiff_abi_version() == 6                                    # additions only
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert NEW_SYMBOLS <= set(re.findall(r" T (hdiff_[a-z0-9_]+)", out))
    for name in NEW_SYMBOLS:
        assert getattr(lib, name).restype is C.c_int


@pytest.mark.parametrize("Cout,Cin,want", [(1, 1, 1 * 3 * 64 * 8), (64, 16, 1 * 3 * 64 * 8), (65, 17, 2 * 3 * 128 * 8), (8, 12, 1536),
                                           (384, 588, 37 * 3 * 384 * 8), (588, 384, 24 * 3 * 640 * 8), (1536, 384, 24 * 3 * 1536 * 8)])
def test_pack_words(Cout, Cin, want):
    """ceil(Cin / 16) chunks x 3 pieces x the channels padded to 64 x 8 words: 6 bytes per padded weight"""
    n = C.c_int64(-1)
    assert hdiff_amd.lib().hdiff_dense_pack_words(Cout, Cin, C.byref(n)) == 0
    assert n.value == want == -(-Cin // 16) * 16 * -(-Cout // 64) * 64 * 6 // 4
    from hdiff_amd import dense
    assert dense.pack_words(Cout, Cin) == want


def test_bad_arguments_return_an_error_and_launch_nothing():
    lib = hdiff_amd.lib()
    n = C.c_int64(0)
    p = 4096                                   # a non-null, 16-byte aligned address that is never dereferenced: every call below is refused

    def refused(rc, text):
        assert rc == -1 and text in lib.hdiff_last_error().decode(), (rc, lib.hdiff_last_error())

    refused(lib.hdiff_dense_pack_words(0, 4, C.byref(n)), "at least 1")
    refused(lib.hdiff_dense_pack_words(4, -1, C.byref(n)), "at least 1")
    refused(lib.hdiff_dense_pack_words(4, 4, None), "null pointer")
    refused(lib.hdiff_dense_pack(None, p, 4, 4, 0, None), "null pointer")
    refused(lib.hdiff_dense_pack(p, None, 4, 4, 1, None), "null pointer")
    refused(lib.hdiff_dense_pack(p, p, 0, 4, 0, None), "at least 1")
    refused(lib.hdiff_dense_pack(p, p + 4, 4, 4, 0, None), "16-byte")
    refused(lib.hdiff_dense_tokens(None, p, None, p, 1, 4, 4, 4, None), "null pointer")
    refused(lib.hdiff_dense_tokens(p, None, None, p, 1, 4, 4, 4, None), "null pointer")
    refused(lib.hdiff_dense_tokens(p, p, None, None, 1, 4, 4, 4, None), "null pointer")
    refused(lib.hdiff_dense_tokens(p, p, None, p, 0, 4, 4, 4, None), "at least 1 image")
    refused(lib.hdiff_dense_tokens(p, p, None, p, 1, 0, 4, 4, None), "at least 1")
    refused(lib.hdiff_dense_tokens(p, p, None, p, 1, 4, -3, 4, None), "at least 1")
    refused(lib.hdiff_dense_tokens(p, p, None, p, 1, 4, 4, 0, None), "at least 1 token")
    refused(lib.hdiff_dense_tokens(p, p, None, p, 1, 4, 4, 1 << 30, None), "31 bits")
    refused(lib.hdiff_dense_tokens(p, p + 8, None, p, 1, 4, 4, 4, None), "16-byte")


def test_dense_route_for_every_choice_and_mode():
    assert dino.DENSE_ROUTES == ("conv", "tokens")
    want = {("conv", "f32"): "conv", ("conv", "bf16x3"): "conv", ("conv", "f16"): "conv",
            ("tokens", "f32"): "conv", ("tokens", "bf16x3"): "tokens", ("tokens", "f16"): "tokens"}
    for (dense, mode), route in want.items():
        assert dino.dense_route(dense, mode) == route, (dense, mode)
    for bad in ("Tokens", "gemm", None, 1):
        with pytest.raises(ValueError, match="dense must be one of"):
            dino.dense_route(bad, "bf16x3")
    with pytest.raises(ValueError, match="contraction mode"):
        dino.dense_route("tokens", "bf16")


def test_unknown_choices_raise_and_the_defaults_are_conv():
    small = dict(embed_dim=16, depth=1, heads=1, pos_grid=3)
    assert dino.DinoV2Features(**small).dense == "conv"
    assert dino.DinoV2Features(dense="tokens", **small).dense == "tokens"
    with pytest.raises(ValueError, match="dense must be one of"):
        dino.DinoV2Features(dense="gemm", **small)
    with pytest.raises(ValueError, match="dense must be one of"):
        L.PerceptualLoss_dino(dense="gemm")
    assert L.PerceptualLoss_dino().perceptual.dense == "conv"
    assert L.PerceptualLoss_dino(dense="tokens").perceptual.dense == "tokens"
    trunk = dino.DinoV2Features(dense="tokens", **small)
    assert L.PerceptualLoss_dino(trunk=trunk).perceptual.dense == "tokens"               # the trunk's own choice stands
    with pytest.raises(ValueError, match="built with dense='tokens'"):
        L.PerceptualLoss_dino(trunk=trunk, dense="conv")
    tr = DB.GaussianDiffusionTrainer(nn.Linear(1, 1), 1e-4, 0.02, 10, dino_loss="native")
    assert tr.loss_perceptual_dino.perceptual.dense == "conv"
    tr = DB.GaussianDiffusionTrainer(nn.Linear(1, 1), 1e-4, 0.02, 10, dino_loss="native", dino_dense="tokens")
    assert tr.loss_perceptual_dino.perceptual.dense == "tokens"
    with pytest.raises(ValueError, match="dense must be one of"):
        DB.GaussianDiffusionTrainer(nn.Linear(1, 1), 1e-4, 0.02, 10, dino_loss="native", dino_dense="gemm")
    for dino_loss in (None, lambda a, b: (a - b).abs().mean()):
        with pytest.raises(ValueError, match="dino_dense goes with dino_loss='native'"):
            DB.GaussianDiffusionTrainer(nn.Linear(1, 1), 1e-4, 0.02, 10, dino_loss=dino_loss, dino_dense="tokens")


def test_the_emulation_splits_exactly_and_matches_float64_on_exact_inputs():
    """Small integers: every piece product and every sum is exact, so the emulation equals the definition to the last bit."""
    g = torch.Generator().manual_seed(0)
    w = torch.randint(-8, 9, (5, 19), generator=g).float()
    x = torch.randint(-8, 9, (2, 19, 7), generator=g).float()
    b = torch.randint(-8, 9, (5,), generator=g).float()
    assert torch.equal(DD.emulate(x, w, b).double(), DD.linear64(x, w, b))
    assert torch.equal(DD.yardstick(x, w, b).double(), DD.linear64(x, w, b))


@pytest.mark.parametrize("shape", DD.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_the_gate_passes_the_scheme_and_fails_every_dropped_term(shape):
    """On the GPU test's own seeded inputs: the full six-term scheme stays within 4x torch's fp32 CPU F.linear error (rms and max); with
    any single term left out the rms error alone is beyond it."""
    w, bias, x = DD.case(*shape)
    ref = DD.linear64(x, w, bias)
    yr, ym = DD.errors(DD.yardstick(x, w, bias), ref)
    er, em = DD.errors(DD.emulate(x, w, bias), ref)
    print(f"{shape}: emulation rms {er:.3e} max {em:.3e}; fp32 CPU rms {yr:.3e} max {ym:.3e}; ratios {er / yr:.2f} {em / ym:.2f}")
    assert yr > 0 and ym > 0
    assert er <= YARD * yr and em <= YARD * ym
    for t in range(6):
        dr, dm = DD.errors(DD.emulate(x, w, bias, drop=t), ref)
        print(f"  term {DD.TERMS[t]} dropped: rms {dr:.3e} max {dm:.3e}; ratios {dr / yr:.1f} {dm / ym:.1f}")
        assert dr > YARD * yr, (shape, t)
