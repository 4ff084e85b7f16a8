"""The split-operand attention backward (csrc/attention_bwd_h2.hip) against float64 where a workgroup walks SEVERAL key blocks: the
blocks behind the first of a key range run sweep<false> of mha_bwd_h2p_kernel (d_head 16) / the !first_kb path of
mha_bwd_h2_kernel<32> (d_head 32), which add to the dQ slab in L2 where the first block stores, reuse the LDS tile buffers, reload
the stationary operands and reset the dK / dV accumulators.  tests/_attn_bwd_h2_cases.py has the cases (2, 3 and 4 blocks per range,
the one-block partner, one head), the families, the references and the gate; tests/test_attn_bwd_h2_cases_cpu.py shows that the cases
reach that geometry and that the gate turns down each defect model.

Everything goes through the C ABI, the backward ALONE: O and lse2 are the float64 definition's, rounded to fp32, and the float64
reference consumes the same rounded values.  dqkv, delta and the workspace (exactly hdiff_mha_flash_bwd_workspace floats: the call
takes no size) lie between canaries, dqkv and the workspace pre-filled with NaN -- a slab word that is added to before it was stored
comes out NaN.  The yardstick of every ratio is the fp32-input kernel (contraction mode 0) on the same inputs, itself held by
tests/test_gpu_attention_f32.py."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import hdiff_amd  # noqa: E402
import _attn_f32_cases as F  # noqa: E402
import _attn_bwd_h2_cases as H  # noqa: E402

pytestmark = pytest.mark.gpu
SLAB_CAP_SET = "HDIFF_BWD_SLAB_GIB" in os.environ      # it moves nsplit: the geometry is not asserted then


def h2_call(lib, case, inputs):
    """the split-operand backward of a case, after asserting that the call takes the route and the key ranges of the table"""
    before = lib.hdiff_get_contraction_mode()
    try:
        assert lib.hdiff_set_contraction_mode(1) == 0
        route, _, aligned, nsplit = H.bwd_route(lib, case)
    finally:
        lib.hdiff_set_contraction_mode(before)
    assert (route, aligned) == (H.H2_PAIRS, 1), (case, route, aligned)
    if not SLAB_CAP_SET:
        assert nsplit == case.nsplit and -(-H.blocks(case) // nsplit) == case.per, (case, nsplit)
    return H.run_bwd(lib, case, *inputs, 1)


def copies_agree(res, case):
    """every (sample, head) pair equals its base pair's result bit for bit, dQ included: batch and head strides, and the fixed order
    of the L2 adds whatever the order the workgroups ran in.  -> {name: [3, D, L]} of the base pairs"""
    idx = F.pair_index(case.B, case.heads).flatten().to(H.DEV)
    assert idx[:3].tolist() == [0, 1, 2]
    base = {}
    for n, flat in res.items():
        base[n] = flat[:3]
        same = (flat == base[n][idx]).flatten(1).all(1)
        assert bool(same.all()), f"{n}: pairs {(~same).nonzero().flatten().tolist()[:8]} (b * heads + h) differ from their base pair"
    return base


def check_run(lib, case, family):
    inputs = H.device_inputs(case, family)
    h2 = copies_agree(H.pairs_of(h2_call(lib, case, inputs), case), case)
    f32 = H.pairs_of(H.run_bwd(lib, case, *inputs, 0), case)
    ps = H.ref_pairs(case)
    ref = [H.reference(family, case.D, case.L, p, H.DEV) for p in ps]
    got = [{n: h2[n][p] for n in H.TENSORS} for p in ps]
    yard = [{n: f32[n][p] for n in H.TENSORS} for p in ps]
    assert not any(torch.equal(g[n], y[n]) for g, y in zip(got, yard) for n in H.TENSORS if bool(y[n].any())), \
        "the split-operand backward did not run"
    rep = H.gate(got, yard, ref, family, enforce=False)
    for n, r in rep.items():
        print(H.case_id(case), family, n, " ".join(f"{ch} x{r[ch]:.3g}" for ch in H.CHECKS), f"mag {r['mag']:.3g}")
    H.gate(got, yard, ref, family)
    lifted = [(n, ch) for (f, n, ch) in H.MEASURED if f == family]
    if lifted:          # where the fp32-input kernel's margin was given room, the fp32 CPU definition holds the cell as well
        cpu = lambda ts: [{n: t[n].cpu() for n in H.TENSORS} for t in ts]
        rep = H.gate(cpu(got), [H.yard32(family, case.D, case.L, p) for p in ps], cpu(ref), family, enforce=False)
        for n, ch in lifted:
            print(H.case_id(case), family, n, ch, f"x{rep[n][ch]:.3g} of the fp32 CPU definition's")
            assert rep[n][ch] <= H.YARD, (n, ch, rep[n][ch])
    if family == "zero-dO-head":
        for n in H.TENSORS:
            assert h2[n][2].abs().max().item() == 0.0, n


PLAIN = [c for c, f in H.RUNS if f == "plain"]
OTHERS = [(c, f) for c, f in H.RUNS if f != "plain"]


@pytest.mark.parametrize("case", PLAIN, ids=[H.case_id(c) + "-plain" for c in PLAIN])
def test_multiblock_error_class(case):
    """plain inputs at every case: over the referenced pairs rms <= 1.25x and worst <= 3x the fp32-input kernel's, per pair rms <=
    1.25x and worst <= 4x -- the constants of test_attention_backward_fp16_pairs_error_class_every_pair (tests/test_gpu_backward.py),
    on launches whose ranges hold 2 (seam2, one-head), 3 (seam3), 4 (seam4) and 1 (alone) blocks.  tests/test_gpu_mutation.py runs
    seam2 on the mutant libraries: it must turn red at both head widths."""
    check_run(hdiff_amd.lib(), case, "plain")


@pytest.mark.parametrize("case,family", OTHERS, ids=[H.case_id(c) + "-" + f for c, f in OTHERS])
def test_multiblock_ranges(case, family):
    """The range families at two blocks per range (seam2 at both head widths, one-head): over the referenced pairs rms <= 1.25x and
    worst <= 3x the fp32-input kernel's, worst <= 2e-5 of the tensor's magnitude, per pair rms <= 4x -- the constants of
    test_attention_backward_fp16_pairs_ranges; a silent pair is exactly zero.  late-spike, one-hot-dO and block-seam had no measured
    ratio on this kernel.  one-hot-dO keeps every constant.  Five cells need room (_attn_bwd_h2_cases.MEASURED: margin = max(contract,
    1.5 x measured); every figure in profiles/attention_bwd_h2_multiblock_error_ratio.txt), none through a defect -- in each the
    kernel's error is BELOW the fp32 CPU definition's on all pairs (<= 0.77x), which the test asserts too (<= 4x, the project's margin
    over an fp32 definition, per pair as well); it is the fp32-input kernel that is unusually exact there:
      block-seam dK, dV   rms over all pairs 3.19x / 3.34x, one pair 7.70x / 4.70x the fp32-input kernel's (d_head 16; 32: less).
                          Five query rows carry dO, so an element of dK or dV is a sum of five products: nothing accumulates and
                          nothing averages.  The fp32-input kernel's operands are exact, its error is the rounding of P and of five
                          terms (0.2x the fp32 CPU definition's); the pair kernel's is its operand representation, 2^-22 against
                          2^-24 -- the factor of 4 that test_attention_backward_fp16_pairs_error_class_every_pair's docstring
                          derives for single elements -- on every element here.  <= 8.5e-7 of the tensor's magnitude.
      late-spike dV       rms over all pairs 1.34x at d_head 32 (1.15x at 16).  Keys 5 and L - 3 carry 10 and 45 sqrt(D): they dominate
                          every row whose q0 is above a few tenths, so dV is carried by P = exp2(s2 - lse2) of scores tens to
                          hundreds of log2 units large, where the error of P is the recomputed score's own rounding: again the pairs'
                          operand representation against exact fp32 operands, for the rows that make up the tensor.  0.46x the
                          fp32 CPU definition's error, 4.9e-6 of the magnitude."""
    check_run(hdiff_amd.lib(), case, family)


@pytest.mark.parametrize("D", [16, 32])
@pytest.mark.parametrize("name", ["seam2", "seam3"])
def test_multiblock_backward_repeats_bit_for_bit(name, D):
    """"fire-and-forget L2 float adds in a fixed order": one slab word is added to by ONE workgroup, block after block.  The whole call
    repeats bit for bit on launches that do issue the adds (one per word at seam2, two at seam3)."""
    lib, case = hdiff_amd.lib(), H.find(name, D)
    inputs = H.device_inputs(case, "plain")
    first = h2_call(lib, case, inputs).clone()
    again = h2_call(lib, case, inputs)
    assert torch.equal(first, again), "not bitwise reproducible"


@pytest.mark.parametrize("D", [16, 32])
@pytest.mark.parametrize("family", ["plain", "block-seam"])
def test_two_blocks_per_range_against_one(family, D):
    """seam2 (B = 8: 9 ranges of two blocks) and alone (B = 1: 17 ranges of one) run the same base pairs.  dK and dV of a key block
    do not depend on where in a range it sits -- the FIRST tag selects only the slab store --: equal in bits.  dQ is summed in
    another order (8 adds in L2 and 9 slabs in the reduce kernel, against 17 slabs): plain within 2e-6 of max |dQ|, the bound of
    test_attention_backward_slab_cap_setting.  block-seam is outside that bound's premise: the four seam keys share one K row and the
    dS of a row sum to zero, so the per-block terms of dQ cancel to 1 / 60 ... 1 / 220 of their absolute sum, and two orders of
    the SAME 17 fp32 terms differ by 2e-6 ... 7e-6 of max |dQ| in plain torch float32 already (measured on the kernel: 4.9e-6 at
    d_head 32).  There each element is held to the two orders' summation bound, 2 x 16 x 2^-24 x sum_b |dQ_b| from float64
    (_attn_bwd_h2_cases.dq_block_terms; the torch emulation reaches 0.12 of it, a dropped or doubled block is its whole |dQ_b|)."""
    lib = hdiff_amd.lib()
    out = {}
    for name in ("seam2", "alone"):
        case = H.find(name, D)
        out[name] = copies_agree(H.pairs_of(h2_call(lib, case, H.device_inputs(case, family)), case), case)
    for n in ("dK", "dV"):
        diff = out["seam2"][n] != out["alone"][n]
        assert not bool(diff.any()), (n, int(diff.sum()), (out["seam2"][n] - out["alone"][n]).abs().max().item())
    dq2, dq1 = out["seam2"]["dQ"], out["alone"]["dQ"]
    err, mag = (dq2 - dq1).abs().max().item(), dq1.abs().max().item()
    print(f"d{D} {family}: dQ of two blocks per range against one: {err:.3e} of max |dQ| {mag:.3e} = {err / mag:.2e}")
    if family == "plain":
        assert err <= 2e-6 * mag, (err, mag)
    else:
        terms = torch.stack([H.dq_block_terms(family, D, H.find("seam2", D).L, p, H.DEV) for p in range(3)])
        used = ((dq2 - dq1).abs().double() / (32 * 2.0 ** -24 * terms).clamp_min(1e-300)).max().item()
        print(f"d{D} {family}: {used:.3f} of the summation bound")
        assert used <= 1.0, used
