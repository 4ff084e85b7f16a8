"""tests/_attn_f32_cases.py without a GPU: the case table reaches every fp32-input attention program that a shape can reach (asked of
hdiff_mha_flash_fwd_route / hdiff_mha_flash_bwd_route in f32 mode, nothing launched), the input families have the properties they
are named for (from float64 scores), and gate() accepts the fp32 CPU definition while rejecting each model of a kernel defect on a
(case, family) that tests/test_gpu_attention_f32.py runs."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import hdiff_amd  # noqa: E402
import _attn_f32_cases as F  # noqa: E402


@pytest.fixture
def f32_lib():
    lib = hdiff_amd.lib()
    before = lib.hdiff_get_contraction_mode()
    assert lib.hdiff_set_contraction_mode(0) == 0
    yield lib
    lib.hdiff_set_contraction_mode(before)


def test_the_table_reaches_every_reachable_program(f32_lib):
    lib = f32_lib
    fwd, bwd, nsplits, short_last_range = set(), set(), set(), False
    for c in F.CASES:
        assert F.fwd_route(lib, c) == c.fwd, c
        route, nk, aligned, nsplit = F.bwd_route(lib, c)
        assert (route, nk, aligned, nsplit) == (0,) + c.bwd, c
        fwd.add((c.D,) + c.fwd[:2]); bwd.add((c.D, nk, aligned)); nsplits.add(nsplit)
        blocks = -(-c.L // (64 * nk))                  # key blocks; per range ceil(blocks / ranges) as key_ranges() cuts them
        per = -(-blocks // nsplit)
        short_last_range |= per >= 2 and blocks - (nsplit - 1) * per < per
        # hdiff_mha_flash_bwd_workspace answers for either mode: exactly the fp32 kernel's slabs unless the split-operand backward
        # covers the shape too (d_head 16 / 32, L % 256 == 0), which needs more
        slabs = nsplit * c.B * c.heads * c.D * c.L if nsplit > 1 else 0
        lib.hdiff_set_contraction_mode(1)
        covered = F.bwd_route(lib, c)[0] != 0
        lib.hdiff_set_contraction_mode(0)
        need = F.bwd_workspace(lib, c)
        assert need == slabs if not covered else need >= slabs, (c, need, slabs)
    small = [d for d in F.ALL_D if d < 48]
    assert fwd == ({(d, F.RUNNING_MAX, 1) for d in F.ALL_D} | {(d, F.RUNNING_MAX, 4) for d in small}
                   | {(d, F.FAST_F32, 4) for d in small})
    want_bwd = ({(d, 1, a) for d in F.ALL_D for a in (0, 1)} | {(d, 2, 1) for d in (24, 32)} | {(d, 4, 1) for d in (4, 8, 12, 16)})
    assert len(want_bwd) == 22 and bwd == want_bwd
    assert 1 in nsplits and max(nsplits) > 1 and short_last_range
    assert not any(F.bwd_route(lib, c)[0] != 0 for c in F.CASES)
    # plain runs on every case; the other families where the table says
    assert {c for c, f in F.RUNS if f == "plain"} == set(F.CASES)
    for f in F.FAMILIES[1:]:
        assert {(c.L, c.D) for c, g in F.RUNS if g == f} >= {(L, d) for L in (576, 600) for d in (8, 16, 32, 64)}, f
    for f in F.NEW_FAMILIES:
        assert {c.bwd[0] for c, g in F.RUNS if g == f} == {1, 2, 4}, f
    assert len(set(F.RUNS)) == len(F.RUNS)


def test_every_pair_of_a_batch_is_a_copy_of_its_base_pair():
    c = F.Case(100, 2, 8, 12, F.RM1, (1, 0, 2))
    qkv3, do3 = F.base_pairs("plain", c.D, c.L)
    qkv, d_o = F.make_batch(c, "plain")
    assert qkv.shape == (2, 3 * 96, 100) and d_o.shape == (2, 96, 100)
    idx = F.pair_index(c.B, c.heads)
    assert idx[0, 0] != idx[0, 1] != idx[0, 2] and idx[1, 0] == (8 % 3)
    for b in range(c.B):
        for h in range(c.heads):
            p = int(idx[b, h])
            for third in range(3):
                rows = slice(third * 96 + h * 12, third * 96 + (h + 1) * 12)
                assert torch.equal(qkv[b, rows], qkv3[p, third * 12:(third + 1) * 12])
            assert torch.equal(d_o[b, h * 12:(h + 1) * 12], do3[p])


@pytest.mark.parametrize("D", [8, 16, 32, 64])
@pytest.mark.parametrize("L", [576, 600])
def test_the_families_do_what_they_claim(D, L):
    """From float64 scores in the kernels' log2 domain (s2 = q . k * log2(e) / sqrt(D))."""
    first, last = slice(0, 64), slice(F.last_tile(L), L)
    for p in range(3):
        assert F.scores64("all-negative", D, L, p).amax(1).max().item() < -15.0, (D, L, p)
        s2 = F.scores64("late-spike", D, L, p)
        lead = s2[:, last].amax(1) - s2[:, first].amax(1)
        for q in F.SPIKE_ROWS(L):
            assert lead[q].item() > 128.0, (D, L, p, q, lead[q].item())
        assert (s2[:, last].amax(1) == s2.amax(1))[list(F.SPIKE_ROWS(L))].all()
        assert F.scores64("peaked", D, L, p).abs().max().item() >= 30.0 * F.LOG2E, (D, L, p)      # |scores| >= 30 nats
        _, d_o = F.base_pairs("one-hot-dO", D, L)
        nz = d_o[p].nonzero()
        assert nz.shape[0] == 1 and nz[0, 1].item() >= F.last_tile(L)
    assert F.base_pairs("zero-dO-head", D, L)[1][2].abs().max().item() == 0.0


def _slab(c):
    """(first key, keys) of the second key range of a case: one whole dQ slab"""
    nk, _, nsplit = c.bwd
    per = -(-(-(-c.L // (64 * nk))) // nsplit)
    return per * 64 * nk, per * 64 * nk


GATE_SHAPES = {(16, 100): next(c for c in F.CASES if (c.D, c.L) == (16, 100)),
               (64, 600): next(c for c in F.CASES if (c.D, c.L, c.heads) == (64, 600, 8))}


@pytest.mark.parametrize("shape", sorted(GATE_SHAPES))
def test_the_gate_accepts_the_fp32_cpu_definition(shape):
    D, L = shape
    for f in sorted({f for c, f in F.RUNS if (c.D, c.L) == shape}):
        ref, yard = F.references(f, D, L)
        for p in range(3):
            rep = F.gate(yard[p], ref[p], yard[p], f)
            assert set(rep) == set(F.TENSORS)
            assert all(v["max_x"] <= 1.0 and v["rms_x"] <= 1.0 for v in rep.values())


def _rejected(defect, shape, family):
    """gate() turns the float64 result with the defect down, on every base pair that has anything to lose"""
    D, L = shape
    assert (GATE_SHAPES[shape], family) in F.RUNS, "not a (case, family) the GPU module runs"
    ref, yard = F.references(family, D, L)
    qkv, d_o = F.base_pairs(family, D, L)
    hit = 0
    for p in range(3):
        bad = F.definition(*F.split_pair(qkv, d_o, p), torch.float64, defect=defect, slab=_slab(GATE_SHAPES[shape]))
        try:
            F.gate(bad, ref[p], yard[p], family)
        except AssertionError:
            hit += 1
    return hit


@pytest.mark.parametrize("defect,shape,family,pairs", [
    ("pad0", (16, 100), "plain", 3),
    ("pad0", (64, 600), "all-negative", 3),
    ("skip-last-query-tile", (16, 100), "plain", 3),
    ("skip-last-query-tile", (64, 600), "one-hot-dO", 3),
    ("skip-last-key-block-dQ", (16, 100), "plain", 3),
    ("skip-last-key-block-dQ", (64, 600), "late-spike", 3),
    ("drop-slab", (16, 100), "plain", 3),
    ("drop-slab", (64, 600), "plain", 3),
    ("dK-unscaled-channel", (16, 100), "plain", 3),
    ("dK-unscaled-channel", (64, 600), "tiny-dO", 3),
    ("dK-unscaled-channel", (64, 600), "zero-dO-head", 2),      # the silent pair has no dK to scale
    ("lse2-off", (16, 100), "plain", 3),
    ("lse2-off", (64, 600), "peaked", 3),
    ("lse2-off", (64, 600), "all-negative", 3),
])
def test_the_gate_rejects_each_defect_model(defect, shape, family, pairs):
    assert defect in F.DEFECTS
    assert _rejected(defect, shape, family) == pairs
    assert {d for d in F.DEFECTS} == {"pad0", "skip-last-query-tile", "skip-last-key-block-dQ", "drop-slab", "dK-unscaled-channel",
                                      "lse2-off"}


def test_padded_keys_at_score_zero_hide_on_peaked_rows_and_ruin_all_negative_ones():
    """The defect that randn-like inputs of large scores cannot see: on the peaked family every tensor moves by less than the fp32 CPU
    definition's own error (gate() lets it pass: nothing to hold against a kernel there), on the all-negative family by its
    whole magnitude."""
    D, L = 64, 600
    for family, total in (("peaked", False), ("all-negative", True)):
        ref, yard = F.references(family, D, L)
        qkv, d_o = F.base_pairs(family, D, L)
        for p in range(3):
            bad = F.definition(*F.split_pair(qkv, d_o, p), torch.float64, defect="pad0")
            for n in F.TENSORS:
                if n == "lse2":
                    continue
                mag = ref[p][n].abs().max().item()
                err = (bad[n] - ref[p][n]).abs().max().item() / mag
                yerr = (yard[p][n].double() - ref[p][n]).abs().max().item() / mag
                assert (err > 0.5) if total else (err < yerr), (family, p, n, err, yerr)


def test_no_margin_is_below_the_projects_and_each_comes_from_a_measurement():
    assert set(F.MEASURED) == set(F.FAMILIES) and all(set(v) == set(F.TENSORS) for v in F.MEASURED.values())
    for f in F.FAMILIES:
        for n in F.TENSORS:
            assert F.margin_of(f, n) == max(F.YARD, 1.5 * F.MEASURED[f][n])
        assert F.margin_of(f, "lse2") <= 1.5 * F.YARD      # lse2 is no cell that needed room: a shift by 2^-12 stays far outside


def test_a_silent_pair_must_be_exactly_zero():
    ref, yard = F.references("zero-dO-head", 64, 600)
    for n in ("dQ", "dK", "dV"):
        assert ref[2][n].abs().max().item() == 0.0 and yard[2][n].abs().max().item() == 0.0
    F.gate(yard[2], ref[2], yard[2], "zero-dO-head")
    got = dict(yard[2]); got["dK"] = yard[2]["dK"].clone(); got["dK"][3, 17] = 1e-38
    with pytest.raises(AssertionError, match="dK"):
        F.gate(got, ref[2], yard[2], "zero-dO-head")


def test_wide_v_gates_o_per_channel_row():
    """An error of 1e-3 of the QUIETEST channel's magnitude is 1e-12 of the tensor's: only a per-row gate sees it."""
    ref, yard = F.references("wide-V", 16, 600)
    got = {n: t.clone() for n, t in yard[0].items()}
    row = ref[0]["O"].abs().amax(1).argmin().item()
    got["O"][row] *= 1.001
    with pytest.raises(AssertionError, match=r"O\[row %d\]" % row):
        F.gate(got, ref[0], yard[0], "wide-V")
    F.gate(got, ref[0], yard[0], "plain")       # the whole-tensor statistic does not
