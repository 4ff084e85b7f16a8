"""CPU-only checks of overlapping-window DDIM sampling (``GaussianDiffusionSampler.forward(tile=...)`` of the image-conditioned
tree): the window layout and its weights, the argument errors of the public interface, the host-side argument checks of the two
C entry points, and the agreement of header, library and binding.  The definition of the loop is tests/_tiled_def.py."""
import inspect
import os
import re
import subprocess

import pytest
import torch

import hdiff_amd
from hdiff_amd import _capi
from hdiff_amd.diffusion import Diffusion as DD
from hdiff_amd.diffusion.Model import DynamicUNet

import _tiled_def as TD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("hdiff_tile_gather", "hdiff_tile_ddim_step")


def test_origins_rule():
    assert DD.tile_origins(44, 16, 8) == [0, 8, 16, 24, 28]
    assert DD.tile_origins(24, 16, 8) == [0, 8]
    assert DD.tile_origins(16, 16, 8) == [0] and DD.tile_origins(7, 16, 2) == [0]
    assert DD.tile_origins(512, 256, 32) == [0, 224, 256]
    assert DD.tile_origins(5, 1, 0) == [0, 1, 2, 3, 4]
    first, count, weight = DD.tile_weights(44, 16, 8)
    assert first.dtype == torch.int32 and count.dtype == torch.int32 and weight.dtype == torch.float64
    assert tuple(first.shape) == (44,) and tuple(count.shape) == (44,) and tuple(weight.shape) == (44, 3)
    assert [p for p in range(44) if count[p] == 3] == [28, 29, 30, 31]
    # position 28: windows 2 (i = 12), 3 (i = 4), 4 (i = 0) with profile min(i + 1, 16 - i, 8) = 4, 5, 1
    assert first[28] == 2 and torch.equal(weight[28], torch.tensor([0.4, 0.5, 0.1], dtype=torch.float64))


def test_layout_properties_sweep():
    """Strictly increasing origins; consecutive covering windows, at most 3 per axis; fp32 weights sum to 1 within 2e-7; a
    position covered once weighs exactly 1.0; size <= tile is one window of weight 1.  (A reduced sweep of tile 2..40, every
    overlap, size 1..129.)"""
    worst = 0.0
    for tile in (2, 3, 5, 8, 16, 17, 40):
        for overlap in range(tile // 2 + 1):
            for size in list(range(1, 50)) + [63, 64, 65, 97, 128, 129]:
                o = DD.tile_origins(size, tile, overlap)
                t = min(tile, size)
                assert o[0] == 0 and o[-1] == size - t and all(b > a for a, b in zip(o, o[1:])), (size, tile, overlap)
                first, count, weight = DD.tile_weights(size, tile, overlap)
                w32 = weight.float()
                if size <= tile:
                    assert o == [0] and torch.all(count == 1) and torch.all(weight[:, 0] == 1.0)
                for p in range(size):
                    cover = [k for k, v in enumerate(o) if v <= p < v + t]
                    assert cover == list(range(int(first[p]), int(first[p]) + int(count[p]))), (size, tile, overlap, p)
                    assert 1 <= len(cover) <= 3
                    prof = [min(p - o[k] + 1, t - (p - o[k]), max(overlap, 1)) for k in cover]
                    assert torch.equal(weight[p, :len(cover)], torch.tensor(prof, dtype=torch.float64) / sum(prof))
                    assert torch.all(weight[p, len(cover):] == 0)
                    if len(cover) == 1:
                        assert w32[p, 0].item() == 1.0
                worst = max(worst, (w32.sum(dim=1, dtype=torch.float32) - 1).abs().max().item(),
                            (w32.double().sum(dim=1) - 1).abs().max().item())
    print(f"largest |sum of a position's fp32 weights - 1| = {worst:.2e}")
    assert worst <= 2e-7


def test_helper_argument_errors():
    for bad in ((0, 16, 2), (44, 0, 0), (44, 16, 9), (44, 16, -1), (44.0, 16, 2), (44, 16.0, 2), (44, 16, 2.0), (44, True, 0),
                (44, 1, 1)):
        with pytest.raises(ValueError):
            DD.tile_origins(*bad)
        with pytest.raises(ValueError):
            DD.tile_weights(*bad)


def test_definition_blend_is_a_partition_of_unity():
    """tests/_tiled_def.py: blending the windows of an image gives the image back (to fp32 rounding of the weights' sum), the
    plain average too, and one window is the identity bit for bit."""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 3, 24, 44, generator=g)
    lay = TD.Layout(24, 44, 16, 8)
    w = TD.windows(x, lay)
    assert tuple(w.shape) == (20, 3, 16, 16) and torch.equal(w[17], x[1, :, 8:24, 16:32])      # (b, iy, ix) = (1, 1, 2)
    assert (TD.blend(w, 2, lay) - x).abs().max().item() <= 4 * 2.0 ** -23 * x.abs().max().item()
    assert (TD.blend(w, 2, lay, weighted=False) - x).abs().max().item() <= 4 * 2.0 ** -23 * x.abs().max().item()
    lay1 = TD.Layout(7, 5, 16, 2)
    x1 = torch.randn(2, 3, 7, 5, generator=g)
    assert torch.equal(TD.blend(TD.windows(x1, lay1), 2, lay1), x1)


def test_forward_signature_and_value_errors():
    sig = inspect.signature(DD.GaussianDiffusionSampler.forward)
    for name in ("tile", "tile_overlap", "tile_batch"):
        p = sig.parameters[name]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, name
    assert [n for n, p in sig.parameters.items() if p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD] == \
        ["self", "input_image", "ddim", "unconditional_guidance_scale", "ddim_step"]
    torch.manual_seed(0)
    m = DynamicUNet(T=1000, ch=32, ch_mult=[1, 2], num_res_blocks=1, dropout=0.0).eval()
    samp = DD.GaussianDiffusionSampler(m, 1e-4, 0.02, 1000)
    x = torch.zeros(1, 3, 24, 44)
    bad_calls = [dict(tile=16),                                                    # tile with the ancestral loop
                 dict(tile=16, ddim=False, ddim_step=5),
                 dict(ddim=True, ddim_step=5, tile_overlap=2), dict(ddim=True, ddim_step=5, tile_batch=4),     # without tile
                 dict(tile_overlap=2), dict(tile_batch=4),
                 dict(ddim=True, ddim_step=5, tile=0), dict(ddim=True, ddim_step=5, tile=-16),
                 dict(ddim=True, ddim_step=5, tile=16.0), dict(ddim=True, ddim_step=5, tile="16"),
                 dict(ddim=True, ddim_step=5, tile=True),
                 dict(ddim=True, ddim_step=5, tile=16, tile_overlap=9), dict(ddim=True, ddim_step=5, tile=16, tile_overlap=-1),
                 dict(ddim=True, ddim_step=5, tile=16, tile_overlap=4.0), dict(ddim=True, ddim_step=5, tile=17, tile_overlap=9),
                 dict(ddim=True, ddim_step=5, tile=16, tile_batch=0), dict(ddim=True, ddim_step=5, tile=16, tile_batch=2.5)]
    for kw in bad_calls:
        with torch.no_grad(), pytest.raises(ValueError):
            samp(x, **kw)
    # valid arguments: a CPU tensor is still refused, only after the checks above
    for kw in (dict(tile=16), dict(tile=16, tile_overlap=8, tile_batch=7), dict(tile=17, tile_overlap=8), dict(tile=1, tile_overlap=0)):
        with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
            samp(x, ddim=True, ddim_step=5, **kw)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        samp(x, ddim=True, ddim_step=5)


def test_symbols_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "hdiff.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(hdiff_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (hdiff_[a-z0-9_]+)", out))
    for name in NEW_SYMBOLS:
        assert name in declared and name in exported and name in _capi.EXPORTED_SYMBOLS, name
    assert hdiff_amd.lib().hdiff_abi_version() == 6          # symbols were added, nothing changed


def test_argument_validation_without_gpu():
    """Null pointers and non-positive sizes come back as -1 with a message from the host-side checks: nothing is launched."""
    lib = hdiff_amd.lib()
    p = 64      # any non-null value: the checks fail before a pointer is used
    ok = [2, 3, 24, 44, 2, 5, 16, 16, 0, 7]                  # B C H W ny nx th tw w0 n_slots
    for k in range(4):
        ptrs = [p] * 4
        ptrs[k] = None
        assert lib.hdiff_tile_gather(*ptrs, *ok, None) == -1
        assert b"tile_gather: null pointer" in lib.hdiff_last_error()
    for k in range(10):
        for v in (0, -1):
            if k == 8 and v == 0:
                continue                                     # w0 = 0 is the first window
            sizes = list(ok)
            sizes[k] = v
            assert lib.hdiff_tile_gather(p, p, p, p, *sizes, None) == -1, (k, v)
            assert b"tile_gather: bad sizes" in lib.hdiff_last_error()
    for sizes in ([2, 3, 24, 44, 2, 5, 25, 16, 0, 7], [2, 3, 24, 44, 2, 5, 16, 45, 0, 7],       # a window larger than the tensor
                  [2, 3, 24, 44, 2, 5, 16, 16, 20, 7]):                                         # w0 past the last window
        assert lib.hdiff_tile_gather(p, p, p, p, *sizes, None) == -1
        assert b"tile_gather: bad sizes" in lib.hdiff_last_error()

    def step(ptrs, nsteps, sizes):
        return lib.hdiff_tile_ddim_step(*ptrs[:12], nsteps, ptrs[12], *sizes, None)

    ok = [2, 3, 24, 44, 2, 5, 16, 16]                        # B C H W ny nx th tw
    for k in range(13):
        ptrs = [p] * 13
        ptrs[k] = None
        assert step(ptrs, 5, ok) == -1, k
        assert b"tile_ddim_step: null pointer" in lib.hdiff_last_error()
    assert step([p] * 13, 0, ok) == -1 and b"tile_ddim_step: bad sizes" in lib.hdiff_last_error()
    for k in range(8):
        for v in (0, -1):
            sizes = list(ok)
            sizes[k] = v
            assert step([p] * 13, 5, sizes) == -1, (k, v)
            assert b"tile_ddim_step: bad sizes" in lib.hdiff_last_error()
    assert step([p] * 13, 5, [2, 3, 24, 44, 2, 5, 25, 16]) == -1 and step([p] * 13, 5, [2, 3, 24, 44, 2, 5, 16, 45]) == -1
