"""The fp32-input attention kernels against float64, per tensor, on every instantiation as the main kernel and on ragged sequences
(tests/_attn_f32_cases.py: the case table, the input families, the references, the gate; tests/test_attn_f32_cases_cpu.py shows
that the table is complete and that the gate turns down each defect model).  Per (case, family), in f32 mode through the C ABI:
the routes of the call are the table's; o, lse2, delta, dqkv and the workspace lie between canaries and are written completely
and nowhere else; every (sample, head) pair equals its base pair's result bit for bit; the three base pairs pass gate() against
float64 with the fp32 CPU definition as the yardstick; a second call repeats bit for bit.

Measured on the MI355X (tools/attn_f32_error_ratio.py, profiles/attention_f32_error_ratio.txt), worst ratio of the kernels' error to
the fp32 CPU definition's over all runs, the larger of max and rms, as O / lse2 / dQ / dK / dV:
    plain 4.13 / 3.13 / 6.07 / 7.17 / 6.13        peaked 1.62 / 1.40 / 4.83 / 4.36 / 9.35       wide-V 6.21 / 1.60 / 4.07 / 3.91 / 3.16
    loud-dO-pixel 1.66 / 1.11 / 4.72 / 4.94 / 3.85   tiny-dO 2.58 / 1.52 / 2.92 / 3.61 / 5.64   zero-dO-head 2.91 / 1.87 / 3.48 / 2.69 / 4.34
    all-negative 2.88 / 1.13 / 24.11 / 1.69 / 1.75   late-spike 2.67 / 2.42 / 3.35 / 2.47 / 69.34   one-hot-dO 6.17 / 1.19 / 7.15 / 24.48 / 15.53
Above YARD = 4 in several cells with errors of at most 3e-4 (all-negative dQ; 2e-5 elsewhere) of the tensor's magnitude: an honest
kernel, _attn_f32_cases.MEASURED says which terms carry it.  A cell's margin is max(4, 1.5 x its figure above)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import hdiff_amd  # noqa: E402
import _attn_f32_cases as F  # noqa: E402

pytestmark = pytest.mark.gpu


def check_run(lib, case, family):
    """-> [report of gate() per base pair]"""
    qkv, d_o = F.make_batch(case, family, F.DEV)
    out = F.run_f32(lib, case, qkv, d_o)
    again = F.run_f32(lib, case, qkv, d_o)
    for n in out:
        assert torch.equal(out[n], again[n]), f"{n}: the second call differs"
    idx = F.pair_index(case.B, case.heads).flatten().to(F.DEV)
    assert idx[:3].tolist() == [0, 1, 2]
    res = F.pairs_of(out, case)
    base = {}
    for n, t in res.items():
        flat = t.reshape(case.B * case.heads, *t.shape[2:])
        base[n] = flat[:3]
        same = (flat == base[n][idx]).flatten(1).all(1)
        assert bool(same.all()), f"{n}: pairs {(~same).nonzero().flatten().tolist()[:8]} (b * heads + h) differ from their base pair"
    ref, yard = F.references(family, case.D, case.L)
    reports = []
    for p in range(3):
        reports.append(F.gate({n: base[n][p].cpu() for n in F.TENSORS}, ref[p], yard[p], family))
        if family == "zero-dO-head" and p == 2:
            for n in ("dQ", "dK", "dV"):
                assert base[n][p].abs().max().item() == 0.0, n
    return reports


@pytest.mark.parametrize("case,family", F.RUNS, ids=[F.case_id(c) + "-" + f for c, f in F.RUNS])
def test_fp32_attention_against_float64(case, family):
    reports = check_run(hdiff_amd.lib(), case, family)
    for p, rep in enumerate(reports):
        print(F.case_id(case), family, "pair", p, " ".join(f"{n} max x{v['max_x']:.2f} rms x{v['rms_x']:.2f}" for n, v in rep.items()))


def test_the_gate_rejects_the_real_backward_fed_a_shifted_lse2():
    """The negative control on the real kernel: the backward given lse2 + 1e-3 (every probability 0.07 % low) is turned down."""
    case = next(c for c in F.CASES if (c.D, c.L, c.heads) == (16, 600, 8))
    qkv, d_o = F.make_batch(case, "plain", F.DEV)
    ref, yard = F.references("plain", case.D, case.L)
    for shift, ok in ((0.0, True), (1e-3, False)):
        res = F.pairs_of(F.run_f32(hdiff_amd.lib(), case, qkv, d_o, lse_shift=shift), case)
        got = {n: res[n][0, 0].cpu() for n in F.TENSORS}
        if ok:
            F.gate(got, ref[0], yard[0], "plain")
        else:
            with pytest.raises(AssertionError, match="dV"):
                F.gate(got, ref[0], yard[0], "plain")
