"""tests/_attn_bwd_h2_cases.py without a GPU: every case reaches the key-range geometry it is named for (asked of
hdiff_mha_flash_bwd_route, nothing launched), the families have the properties they claim (from float64 scores), and gate() accepts
the fp32 CPU definition on every (case, family) that tests/test_gpu_attn_bwd_h2.py runs while rejecting each model of what a block
behind the first of its key range can get wrong."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import hdiff_amd  # noqa: E402
import _attn_f32_cases as F  # noqa: E402
import _attn_bwd_h2_cases as H  # noqa: E402

SLAB_CAP_SET = "HDIFF_BWD_SLAB_GIB" in os.environ      # it moves nsplit of H2_PAIRS


@pytest.fixture
def mode(request):
    before = hdiff_amd.get_contraction_mode()
    hdiff_amd.set_contraction_mode(request.param)
    yield request.param
    hdiff_amd.set_contraction_mode(before)


@pytest.mark.parametrize("mode", ["bf16x3", "f16", "f32"], indirect=True)
def test_every_case_reaches_the_key_ranges_of_the_table(mode):
    lib = hdiff_amd.lib()
    for c in H.CASES:
        route, nk, aligned, nsplit = H.bwd_route(lib, c)
        if mode == "f32":
            assert route == H.FUSED_F32, c
            continue
        assert (route, aligned) == (H.H2_PAIRS, 1), c
        if SLAB_CAP_SET:
            continue
        assert nsplit == c.nsplit and -(-H.blocks(c) // nsplit) == c.per, (c, nsplit)


def test_the_table_is_the_issues():
    """blocks, blocks per range, ranges, and what each case is there for"""
    rows = {(c.name, c.D): (c.L, c.B, c.heads, H.blocks(c), c.per, c.nsplit) for c in H.CASES}
    want = {"seam2": (4352, 8, 8, 17, 2, 9), "seam3": (8448, 8, 8, 33, 3, 11), "seam4": (12544, 8, 8, 49, 4, 13),
            "alone": (4352, 1, 8, 17, 1, 17)}
    assert rows == {**{(n, d): v for n, v in want.items() for d in (16, 32)}, ("one-head", 32): (4352, 64, 1, 17, 2, 9)}
    last = {c.name: H.blocks(c) - (c.nsplit - 1) * c.per for c in H.CASES}      # blocks of the last range
    assert last == {"seam2": 1, "seam3": 3, "seam4": 1, "alone": 1, "one-head": 1}
    assert all(c.B * c.heads >= 64 for c in H.CASES if c.name != "alone")         # 16 ranges wanted, not ceil(1024 / (B heads))
    # plain everywhere, every family at seam2 (both head widths) and one-head, three referenced pairs but at seam4
    assert {c for c, f in H.RUNS if f == "plain"} == set(H.CASES)
    for f in H.FAMILIES[1:]:
        assert {H.case_id(c) for c, g in H.RUNS if g == f} == {"seam2-d16", "seam2-d32", "one-head-d32"}, f
    assert len(set(H.RUNS)) == len(H.RUNS) == 9 + 3 * 7
    assert [H.ref_pairs(c) for c in H.CASES if c.name == "seam4"] == [(0,), (0,)]
    # block-seam's keys sit on the seams of the per = 2 geometry at L = 4352
    c = H.find("seam2", 16)
    span = c.per * H.KB
    k0, k1, k2, k3 = H.SEAM_KEYS
    assert k0 // span == k1 // span == 0 and k0 // H.KB == 0 and k1 // H.KB == 1 and k1 % H.KB == 0
    assert k2 // span == c.nsplit - 2 and (k2 + 1) % span == 0 and k3 // span == c.nsplit - 1 and k3 % span == 0
    assert H.seam_rows(c.L) == (0, 31, 32, c.L - 33, c.L - 1)


def test_every_pair_of_a_batch_is_a_copy_of_its_base_pair():
    for c in (H.find("seam2", 16), H.find("one-head", 32)):
        qkv3, do3 = H.base_pairs("block-seam", c.D, c.L)
        qkv, d_o = H.make_batch(c, "block-seam")
        Cc = c.heads * c.D
        assert qkv.shape == (c.B, 3 * Cc, c.L) and d_o.shape == (c.B, Cc, c.L)
        idx = F.pair_index(c.B, c.heads)
        for b in (0, 1, c.B - 1):
            for h in range(c.heads):
                p = int(idx[b, h])
                for third in range(3):
                    rows = slice(third * Cc + h * c.D, third * Cc + (h + 1) * c.D)
                    assert torch.equal(qkv[b, rows], qkv3[p, third * c.D:(third + 1) * c.D])
                assert torch.equal(d_o[b, h * c.D:(h + 1) * c.D], do3[p])


@pytest.mark.parametrize("D", [16, 32])
def test_the_families_do_what_they_claim(D):
    L = 4352
    first, last = slice(0, 64), slice(F.last_tile(L), L)
    rows = list(H.seam_rows(L))
    quiet = [q for q in range(L) if q not in rows]
    for p in range(3):
        # block-seam: the four seam keys together own more than half of the softmax mass of every row that carries dO, no single
        # one of them owns it all (dS = P o (dP - delta) lives there), and no other row has any dO
        mass = H.seam_mass(D, L, p)
        assert mass.min().item() > 0.5, (D, p, mass.tolist())
        qkv, d_o = H.base_pairs("block-seam", D, L)
        q, k, _, _ = F.split_pair(qkv, d_o, p)
        P = torch.softmax((q.double().t()[rows] @ k.double()) / D ** 0.5, dim=-1)[:, list(H.SEAM_KEYS)]
        assert P.max().item() < 0.5 and P.min().item() > 0.1, (D, p)
        assert d_o[p][:, quiet].abs().max().item() == 0.0 and d_o[p][:, rows].abs().amax(0).min().item() > 0.0
        # late-spike: key L - 3 owns more than half (all, to 1e-30) of the mass of the rows made to see it
        s2 = F.scores64("late-spike", D, L, p)
        for qrow in F.SPIKE_ROWS(L):
            assert torch.softmax(s2[qrow] / F.LOG2E, dim=-1)[L - 3].item() > 0.5, (D, p, qrow)
            assert (s2[qrow, last].max() - s2[qrow, first].max()).item() > 128.0
        assert F.scores64("peaked", D, L, p).abs().max().item() >= 30.0 * F.LOG2E, (D, p)
        nz = H.base_pairs("one-hot-dO", D, L)[1][p].nonzero()
        assert nz.shape[0] == 1 and nz[0, 1].item() >= F.last_tile(L)
        v = H.base_pairs("wide-V", D, L)[0][p, 2 * D:]
        assert (v.abs().amax(1).max() / v.abs().amax(1).min()).item() > 2.0 ** 26
        d_loud = H.base_pairs("loud-dO-pixel", D, L)[1][p].abs().amax(0)
        assert d_loud.argmax().item() == L // 3 and (d_loud.max() / d_loud.median()).item() > 1e3
    assert H.base_pairs("zero-dO-head", D, L)[1][2].abs().max().item() == 0.0
    assert H.base_pairs("zero-dO-head", D, L)[1][:2].abs().amax((1, 2)).min().item() > 0.0


def _sets(case, family, defect=None):
    ps = H.ref_pairs(case)
    ref = [H.reference(family, case.D, case.L, p) for p in ps]
    yard = [H.yard32(family, case.D, case.L, p) for p in ps]
    if defect is None:
        return yard, yard, ref
    qkv, d_o = H.base_pairs(family, case.D, case.L)
    o, lse2 = H.forwards(family, case.D, case.L)
    bad = [H.backward(*F.split_pair(qkv, d_o, p), o[p], lse2[p], torch.float32, defect=defect, per=case.per) for p in ps]
    return bad, yard, ref


@pytest.mark.parametrize("case,f", H.RUNS, ids=[H.case_id(c) + "-" + f for c, f in H.RUNS])
def test_the_gate_accepts_the_fp32_cpu_definition(case, f):
    rep = H.gate(*_sets(case, f), f)
    assert set(rep) == set(H.TENSORS)
    for name, r in rep.items():
        assert all(r[ch] in (0.0, 1.0) for ch in ("all-rms", "all-worst", "pair-rms", "pair-worst")), (f, name, r)
        assert r["worst-of-mag"] <= H.WORST_OF_MAG, (f, name, r)
    # float64 is the reference of what the kernels are fed: O and lse2 are fp32 values
    o, lse2 = H.forwards("plain", case.D, case.L)
    assert o.dtype == lse2.dtype == torch.float32 and o.shape == (3, case.D, case.L) and lse2.shape == (3, case.L)


# tensors that each defect model must turn the gate down on (at least): what the defect touches
TOUCHES = {"dQ-drops-later-blocks": {"dQ"}, "dQ-block-twice": {"dQ"}, "stale-KV": {"dK", "dV"}, "no-reset": {"dK", "dV"},
           "skip-last-range": {"dQ", "dK", "dV"}}


@pytest.mark.parametrize("defect", H.DEFECTS)
@pytest.mark.parametrize("where", [("seam2", 16, "plain"), ("seam2", 32, "block-seam"), ("one-head", 32, "plain"),
                                   ("one-head", 32, "late-spike")], ids=lambda w: "%s-d%d-%s" % w)
def test_the_gate_rejects_each_defect_model(defect, where):
    name, D, family = where
    case = H.find(name, D)
    assert (case, family) in H.RUNS, "not a (case, family) the GPU module runs"
    assert set(TOUCHES) == set(H.DEFECTS)
    with pytest.raises(AssertionError) as e:
        H.gate(*_sets(case, family, defect), family)
    msg = str(e.value)
    for t in H.TENSORS:
        assert ((t + " ") in msg) == (t in TOUCHES[defect]), (defect, t, msg)      # named, and nothing the defect leaves alone


def test_each_defect_alone_on_one_pair_is_rejected_too():
    """one damaged pair among three: the per-pair and the all-pairs checks both see it"""
    case = H.find("seam2", 16)
    yard, _, ref = _sets(case, "plain")
    bad, _, _ = _sets(case, "plain", "dQ-block-twice")
    mixed = [yard[0], bad[1], yard[2]]
    with pytest.raises(AssertionError, match=r"dQ pair-rms \(pair 1\)"):
        H.gate(mixed, yard, ref, "plain")
    assert H.gate(mixed, yard, ref, "plain", enforce=False)["dQ"]["all-rms"] > 1e3


def test_a_silent_pair_must_be_exactly_zero():
    case = H.find("seam2", 16)
    yard, _, ref = _sets(case, "zero-dO-head")
    for n in H.TENSORS:
        assert ref[2][n].abs().max().item() == 0.0 and yard[2][n].abs().max().item() == 0.0
    got = [dict(y) for y in yard]
    got[2]["dK"] = yard[2]["dK"].clone(); got[2]["dK"][3, 300] = 1e-38
    with pytest.raises(AssertionError, match=r"dK pair-rms \(pair 2\)"):
        H.gate(got, yard, ref, "zero-dO-head")


def test_the_margins_are_the_contract_unless_a_measurement_says_otherwise():
    contract = {"all-rms": 1.25, "all-worst": 3.0, "pair-rms": 4.0, "pair-worst": None, "worst-of-mag": 2e-5}
    plain = dict(contract, **{"pair-rms": 1.25, "pair-worst": 4.0, "worst-of-mag": None})
    for f in H.FAMILIES:
        for n in H.TENSORS:
            for ch in H.CHECKS:
                base = (plain if f == "plain" else contract)[ch]
                m = H.MEASURED.get((f, n, ch))
                assert H.margin_of(f, n, ch) == (base if m is None else max(base, 1.5 * m)), (f, n, ch)
    assert all(f in H.UNMEASURED and n in H.TENSORS and ch in H.CHECKS and contract[ch] is not None for f, n, ch in H.MEASURED)
