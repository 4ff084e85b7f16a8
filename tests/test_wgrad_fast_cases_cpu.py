"""tests/_wgrad_fast_cases.py without a GPU: the cases take the routes, tile counts and split counts they name; the probe tables
leave no tile corner out; the probe formulas ARE the weight gradient (autograd of F.conv2d in float64, torch.equal -- a single
product of powers of two and zeros is exact there), the zero padding of the activated tensor included; and the gates that
tests/test_gpu_wgrad_fast.py applies reject four defects a kernel could have, each simulated in float64 from the exact formula."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from hdiff_amd import autograd as A  # noqa: E402
import _strided_geometry_cases as K  # noqa: E402
import _wgrad_fast_cases as W  # noqa: E402
from test_wgrad_route_cpu import workspace_of  # noqa: E402

SEED = 2024


def prologue(c, seed, dropout):
    """a GroupNorm-like per-(sample, channel) scale and shift and, for the dropout form, keep decisions: any values serve here"""
    g = torch.Generator().manual_seed(seed)
    scale = torch.randn(c.B, W.cin_of(c), generator=g) * 0.5 + 1
    shift = torch.randn(c.B, W.cin_of(c), generator=g) * 0.3
    keep = (torch.rand(c.B, W.cin_of(c), c.H, c.W, generator=g) < 1 - W.DROP_P) if dropout else None
    return scale, shift, keep, (A._inv_keep(W.DROP_P) if dropout else 1.0)


def test_the_table_of_cases():
    assert W.CASE_IDS == ["3x3-2x32", "3x3-4x64", "3x3-6x96", "1x1-8x8", "1x1-seam", "1x1-160"]
    assert [(c.C0, c.C1, c.cout, c.H, c.W, c.B, c.tiles, c.odd) for c in W.CASES] == [
        (32, 0, 256, 2, 32, 3, 3, 2), (64, 32, 128, 4, 64, 3, 12, 5), (32, 0, 128, 6, 96, 2, 18, 7),
        (32, 0, 128, 8, 8, 5, 5, 2), (40, 24, 128, 8, 16, 3, 6, 4), (96, 64, 256, 16, 16, 2, 8, 3)]


@pytest.mark.parametrize("cid", W.CASE_IDS)
def test_case_takes_its_route_tile_count_and_split_count(cid):
    c = W.case(cid)
    for gn in ((False, True) if c.k == 3 else (False,)):
        assert K.route_of(W.desc(c, gn)) == c.route
    if cid in W.CASES_DROPOUT:
        assert K.route_of(W.desc(c, True), dropout=1) == c.route
    assert c.B * W.tiles_per_image(c) == c.tiles
    ns, floats = workspace_of(W.desc(c))
    assert ns == c.tiles == W.nsplit_of(c, "all"), "the library's own split count is one tile per split at these sizes"
    assert floats == ns * c.k * c.k * W.cin_of(c) * c.cout
    # the split that does not divide: the workgroups walk different numbers of tiles, so the last `more` is false at different
    # depths; the deepest uses both buffers, and walks three tiles or more wherever a non-dividing count with such a split exists
    # (none does for 3 and for 6 tiles: 2 gives 2 + 1, 4 gives 2 + 2 + 1 + 1, 5 gives 2 + 1 + 1 + 1 + 1)
    assert 1 < c.odd < c.tiles and c.tiles % c.odd != 0
    depth = [len(W.tiles_of_split(c, c.odd, s)) for s in range(c.odd)]
    assert max(depth) >= (2 if c.tiles in (3, 6) else 3) and min(depth) < max(depth) and sum(depth) == c.tiles
    assert W.longest_split(c, c.odd) == max(depth) and W.longest_split(c, 1) == c.tiles and W.longest_split(c, c.tiles) == 1
    # nsplit = 1 walks from one image into the next
    assert c.tiles > W.tiles_per_image(c)


@pytest.mark.parametrize("cid", W.CASE_IDS)
def test_probe_tables_leave_no_tile_corner_out(cid):
    c = W.case(cid)
    for probes, nchan in ((W.dy_probes(c, SEED), c.cout), (W.x_probes(c, SEED), W.cin_of(c))):
        tabs = [p.table for p in probes]
        assert len(tabs) == -(-5 * c.tiles // nchan)
        assert W.uncovered(c, tabs) == []
        for t in tabs:
            assert set(t.v.abs().log2().tolist()) <= {float(e) for e in range(-3, 4)} and len(t.v) == nchan
    # the condition has teeth: a table set short of one round, or with one probe moved, is reported
    t = W.dy_probes(c, SEED)[0].table
    b, ti = c.B - 1, W.tiles_per_image(c) - 1
    y, x = W.tile_pixels(c, ti)[63]
    moved = t._replace(y=torch.where((t.b == b) & (t.y == y) & (t.x == x), t.y - 1, t.y))
    assert (b, ti, "pixel 63") in W.uncovered(c, [moved])


def test_the_tile_walk_of_the_cases():
    c = W.case("3x3-6x96")
    assert W.tile_pixels(c, 4)[0] == (2, 32) and W.tile_pixels(c, 4)[63] == (3, 63)      # the interior tile
    c = W.case("1x1-seam")
    assert W.tile_pixels(c, 1)[0] == (4, 0) and W.tile_pixels(c, 1)[63] == (7, 15)
    assert W.tiles_of_split(W.case("3x3-4x64"), 5, 1) == [1, 6, 11] and W.tiles_of_split(W.case("1x1-8x8"), 2, 1) == [1, 3]


def conv_autograd_f64(c, act, dy):
    w = torch.zeros(c.cout, W.cin_of(c), c.k, c.k, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(act.double(), w, padding=c.k // 2)
    return torch.autograd.grad(y, w, dy.double())[0]


@pytest.mark.parametrize("cid", W.CASE_IDS)
def test_probe_formulas_are_the_float64_weight_gradient(cid):
    c = W.case(cid)
    for p in W.dy_probes(c, SEED):
        want = W.expected_dy_probe(c, W.cat(p.x0, p.x1), p.table)
        assert torch.equal(conv_autograd_f64(c, W.cat(p.x0, p.x1), p.dy), want)
        assert torch.equal(want.float().double(), want), "one product of a float and a power of two is a float"
    for p in W.x_probes(c, SEED):
        want = W.expected_x_probe(c, p.dy, p.table)
        assert torch.equal(conv_autograd_f64(c, W.cat(p.x0, p.x1), p.dy), want)
        assert torch.equal(want.float().double(), want)
        assert torch.equal(W.wgrad_f64(c, W.cat(p.x0, p.x1), p.dy), want)
    x0, x1, dy = W.dense_inputs(c, SEED)
    assert torch.allclose(W.wgrad_f64(c, W.cat(x0, x1), dy), conv_autograd_f64(c, W.cat(x0, x1), dy), rtol=0, atol=1e-11)


@pytest.mark.parametrize("cid,dropout", [(cid, False) for cid in W.CASES_3X3] + [(cid, True) for cid in W.CASES_DROPOUT])
def test_probe_formula_behind_the_prologue_pads_the_activated_tensor(cid, dropout):
    c = W.case(cid)
    scale, shift, keep, inv_keep = prologue(c, SEED + 5, dropout)
    for p in W.dy_probes(c, SEED):
        act, v = W.activation_f64(W.cat(p.x0, p.x1), scale, shift, keep, inv_keep)
        want = W.expected_dy_probe(c, act, p.table)
        assert torch.equal(conv_autograd_f64(c, act, p.dy), want)
        vabs = W.expected_dy_probe(c, v.abs(), p.table._replace(v=torch.ones_like(p.table.v)))
        ratio, zeros_exact = W.activation_ratio(want.float(), want, vabs)
        assert ratio <= 1 / 8 and zeros_exact, "rounding the float64 value to a float is 2^-24 of it at the most, the gate 8 x that at the least"
        if dropout:
            assert (want == 0).sum() > (W.expected_dy_probe(c, W.activation_f64(W.cat(p.x0, p.x1), scale, shift)[0], p.table) == 0).sum()


def defect_cases(ids):
    """every defect on every case; the batch-stride one needs a concat input"""
    return [(cid, d) for cid in ids for d in W.DEFECTS if d != "stride" or cid in W.CASES_CONCAT]


@pytest.mark.parametrize("cid,defect", defect_cases(W.CASE_IDS))
def test_the_probe_gates_reject_a_simulated_defect(cid, defect):
    """parts a and b of the GPU test: torch.equal on every round.  `skip` and `twice` act on the last tile split 0 walks: with one
    split that is the last tile of the last image, with the non-dividing count a tile in the middle of an image."""
    c = W.case(cid)
    for which in W.SPLITS if defect in ("skip", "twice") else ("one",):
        ns = W.nsplit_of(c, which)
        for probes, expected in ((W.dy_probes(c, SEED), lambda p: W.expected_dy_probe(c, W.cat(p.x0, p.x1), p.table)),
                                 (W.x_probes(c, SEED), lambda p: W.expected_x_probe(c, p.dy, p.table))):
            good = [W.exact(W.simulate(c, W.cat(p.x0, p.x1), p.dy).float(), expected(p)) for p in probes]
            bad = [W.exact(W.simulate(c, W.cat(p.x0, p.x1), p.dy, defect, ns).float(), expected(p)) for p in probes]
            assert all(good), "the formula without a defect passes"
            assert not all(bad), (cid, defect, which)


@pytest.mark.parametrize("cid,defect", defect_cases(W.CASES_3X3))
def test_the_activation_gate_rejects_a_simulated_defect(cid, defect):
    """part c: dy_probes behind the prologue, the per-element gate and the exact zeros"""
    c = W.case(cid)
    dropout = cid in W.CASES_DROPOUT
    scale, shift, keep, inv_keep = prologue(c, SEED + 5, dropout)
    rejected = []
    for p in W.dy_probes(c, SEED):
        act, v = W.activation_f64(W.cat(p.x0, p.x1), scale, shift, keep, inv_keep)
        ref = W.expected_dy_probe(c, act, p.table)
        vabs = W.expected_dy_probe(c, v.abs(), p.table._replace(v=torch.ones_like(p.table.v)))
        ratio, zeros_exact = W.activation_ratio(W.simulate(c, act, p.dy).float(), ref, vabs)
        assert ratio <= 1.0 and zeros_exact
        ratio, zeros_exact = W.activation_ratio(W.simulate(c, act, p.dy, defect, c.odd).float(), ref, vabs)
        rejected.append(ratio > 1.0 or not zeros_exact)
    assert any(rejected), (cid, defect)


@pytest.mark.parametrize("cid,defect", defect_cases(W.CASE_IDS))
def test_both_dense_gates_reject_a_simulated_defect(cid, defect):
    """part e: a skipped or doubled tile is a whole tile's contribution, far outside the per-op gate and the summation bound alike"""
    c = W.case(cid)
    x0, x1, dy = W.dense_inputs(c, SEED)
    act = W.cat(x0, x1)
    ref, abs_sum = W.wgrad_f64(c, act, dy), W.wgrad_f64(c, act.abs(), dy.abs())
    for which in W.SPLITS:
        ns = W.nsplit_of(c, which)
        r_op, r_sum = W.dense_ratios(c, W.simulate(c, act, dy).float(), ref, abs_sum, ns)
        assert r_op <= 1.0 and r_sum <= 1.0
        r_op, r_sum = W.dense_ratios(c, W.simulate(c, act, dy, defect, ns).float(), ref, abs_sum, ns)
        assert r_op > 1.0 and r_sum > 1.0, (cid, defect, which, r_op, r_sum)
