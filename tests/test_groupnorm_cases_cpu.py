"""The references and gates of tests/_groupnorm_cases.py, checked without a GPU: ref_bwd against float64 autograd, and every
forward gate against a two-pass fp32 computation -- so a GPU test that misses a gate shows a defect of the kernel, not a
bound that fp32 cannot meet."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _groupnorm_cases as GC  # noqa: E402


@pytest.mark.parametrize("swish", [True, False])
@pytest.mark.parametrize("C,HW,B", [(96, 25, 2), (384, 64, 2)])
def test_ref_bwd_equals_float64_autograd(C, HW, B, swish):
    """With the unrounded float64 mean and rstd, ref_bwd IS the gradient of F.group_norm (then y * sigmoid(y))."""
    x = GC.make_x("channel-steps", B, C, HW, seed=C + HW)
    gamma, beta = GC.make_affine(C, seed=C)
    dA = GC.make_dA("randn", B, C, HW, seed=HW)
    st = GC.ref_stats(x, GC.G, GC.EPS, gamma, beta)
    ref = GC.ref_bwd(x, dA, st["mean"], st["rstd"], gamma, beta, swish)
    x64 = x.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = F.group_norm(x64, GC.G, g64, b64, GC.EPS)
    (y * torch.sigmoid(y) if swish else y).backward(dA.double())
    for name, want in (("dx", x64.grad), ("dgamma", g64.grad), ("dbeta", b64.grad)):
        err = (ref[name] - want).abs().max().item()
        assert err <= 1e-9 * want.abs().max().item(), (name, err, want.abs().max().item())
    # T bounds dx term by term, and the absolute sums bound the signed ones
    assert (ref["dx"].abs() <= ref["T"] * (1 + 1e-12)).all()
    assert (ref["dbeta"].abs() <= ref["sum_abs_dy"] * (1 + 1e-12)).all()
    assert (ref["dgamma"].abs() <= ref["sum_abs_dyx"] * (1 + 1e-12)).all()


def test_pivot_indices_follow_the_kernel_slices():
    assert GC.slices(8192, 2) == [(0, 4096), (4096, 4096)]
    assert GC.slices(100, 3) == [(0, 100), (None, 0), (None, 0)]        # a split covers >= 4096 elements of a plane
    assert GC.slices(8, 4) == [(0, 8)] + [(None, 0)] * 3
    assert GC.slices(6000, 2) == [(0, 4096), (4096, 1904)] and GC.slices(8190, 2) == [(0, 4096), (4096, 4094)]
    assert GC.slices(8192, 3) == [(0, 4096), (4096, 4096), (None, 0)]
    assert GC.slices(65536, 16) == [(4096 * s, 4096) for s in range(16)] and GC.slices(9216, 2) == [(0, 4608), (4608, 4608)]
    assert GC.pivot_indices(8190, 2) == [0, 4096]
    x = GC.make_x("pivot-spike-3000", 1, 64, 6000, nsplit=2)
    assert (x[:, 0::2, [0, 4096]] == 3000.0).all() and (x == 3000.0).sum().item() == 32 * 2
    x = GC.make_x("constant-but-one", 1, 96, 25)
    assert (x.view(1, 32, -1) == 4.25).sum(-1).eq(1).all() and ((x == 3.25) | (x == 4.25)).all()


@pytest.mark.parametrize("shape", GC.SHAPES, ids=GC.shape_id)
@pytest.mark.parametrize("family", GC.FAMILIES)
def test_forward_gates_are_reachable_in_fp32(family, shape):
    C0, C1, HW, B, nsplit = shape
    C = C0 + C1
    x = GC.make_x(family, B, C, HW, seed=C + HW, nsplit=nsplit)
    gamma, beta = GC.make_affine(C, seed=C + HW)
    ref = GC.ref_stats(x, GC.G, GC.EPS, gamma, beta)
    fails, ratios = GC.forward_gate_report(GC.two_pass_fp32(x, gamma, beta), ref, beta, constant=family == "constant")
    assert not fails, (family, shape, fails)
