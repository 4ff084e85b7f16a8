"""conv_wgrad3x3_kernel<false>, <true>, <true, true> and conv_wgrad1x1_kernel (conv_wgrad3x3.hip) at every tile seam and every
split count, through hdiff_conv2d_wgrad / hdiff_conv2d_wgrad_dropout with the split count as an ARGUMENT (autograd._run_wgrad only
ever passes the library's own answer) and hdiff_conv_wgrad_unpack.  tests/_wgrad_fast_cases.py holds the cases, the probes, the
float64 references and the gates with their derivation; tests/test_wgrad_fast_cases_cpu.py shows without a GPU that the references
are the weight gradient and that the gates reject a shifted patch, a skipped tile, a doubled tile and a wrong batch stride.

  a  dy_probes, no prologue: torch.equal.  The activation staging: halo rows and columns, the four border masks, the in-image
     substitute address of a padding element, the x0 / x1 choice and batch stride, the image index while one workgroup walks on.
  b  x_probes, no prologue: torch.equal.  The dY tile: 16-byte loads, pixel-major stores, the second output-channel workgroup's
     offset; 1x1: both operands' shared staging, and the dead input columns (nothing of them may reach a live channel).
  c  dy_probes behind GroupNorm + Swish and behind dropout, scale / shift from A._gn_stats on the device and used by the reference
     too (GroupNorm's own statistics error is out of the picture): the per-element activation gate, padding and dropped elements 0.
  d  the result at every split count is bit-identical to nsplit = 1 (one product plus zeros), and a second call is bit-identical.
  e  dense randn operands against float64: the per-op gate of tests/test_gpu_backward.py and the fp32 summation bound.

Every launch asserts its route; slabs and dW start as NaN, so an element no workgroup wrote is seen.
HDIFF_WGRAD_FAST_REPORT=<file> appends the measured error / gate ratios of c and e (profiles/wgrad_fast.txt)."""
import ctypes as C
import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from hdiff_amd import _capi  # noqa: E402
from hdiff_amd import autograd as A  # noqa: E402
from hdiff_amd import engine as E  # noqa: E402
import _strided_geometry_cases as K  # noqa: E402
import _wgrad_fast_cases as W  # noqa: E402

DEV = "cuda:0"
SEED = 2024
INSTANCES = [(cid, "plain") for cid in W.CASE_IDS] + [(cid, "gn") for cid in W.CASES_3X3] + [(cid, "drop") for cid in W.CASES_DROPOUT]
PROLOGUES = [(cid, inst) for cid, inst in INSTANCES if inst != "plain"]


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


def wgrad(case, x0, x1, gn, dy, nsplit, dropout):
    """The launch group of autograd._run_wgrad on device tensors, with nsplit slabs instead of the library's count.
    gn = (scale, shift) or None, dropout = (keep bits, 1 / keep) or None -> dW [cout, cin, k, k]."""
    lib = _capi.lib()
    c, cin = case, W.cin_of(case)
    taps = E.conv_taps(c.k, c.k // 2)
    n = len(taps.dy)
    d = _capi.WgradDesc()
    d.x0, d.x1, d.C0, d.C1, d.B, d.H, d.W = A._p(x0), A._p(x1), c.C0, c.C1, c.B, c.H, c.W
    d.gn_scale, d.gn_shift = (A._p(gn[0]), A._p(gn[1])) if gn is not None else (None, None)
    d.dy, d.Cout, d.CinPad, d.CoutPad = dy.data_ptr(), c.cout, E._pad(cin, 8), E._pad(c.cout, 64)
    d.OH, d.OW, d.VH, d.VW, d.in_stride = c.H, c.W, c.H, c.W, 1
    d.out_sy, d.out_oy, d.out_sx, d.out_ox = 1, 0, 1, 0
    d.ntaps = n
    for i in range(n):
        d.tap_dy[i], d.tap_dx[i] = taps.dy[i], taps.dx[i]
    assert tuple(x0.shape) == (c.B, c.C0, c.H, c.W) and tuple(dy.shape) == (c.B, c.cout, c.H, c.W)
    assert (x1 is None) == (c.C1 == 0) and 1 <= nsplit <= c.tiles
    assert K.route_of(d, 1 if dropout is not None else 0) == c.route, (c.id, "weight-gradient route")
    slab = n * d.CinPad * d.CoutPad
    ws = torch.full((nsplit * slab,), float("nan"), device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    if dropout is not None:
        _capi.check(lib.hdiff_conv2d_wgrad_dropout(C.byref(d), dropout[0].data_ptr(), C.c_float(dropout[1]), ws.data_ptr(), nsplit, s),
                    "conv2d_wgrad_dropout")
    else:
        _capi.check(lib.hdiff_conv2d_wgrad(C.byref(d), ws.data_ptr(), nsplit, s), "conv2d_wgrad")
    dw = torch.full((c.cout, cin, c.k, c.k), float("nan"), device=DEV)
    a_ky, a_kx = (C.c_int * n)(*taps.ky), (C.c_int * n)(*taps.kx)
    _capi.check(lib.hdiff_conv_wgrad_unpack(ws.data_ptr(), nsplit, dw.data_ptr(), 0, c.cout, cin, c.k, c.k, n, a_ky, a_kx, d.CinPad,
                                            d.CoutPad, 0, s), "wgrad_unpack")
    return dw


def run(c, p, nsplit, pro=None):
    """one probe (or dense triple) through the instantiation pro belongs to"""
    gn, dropout = (pro["gn"], pro["dropout"]) if pro is not None else (None, None)
    return wgrad(c, dev(p.x0), dev(p.x1), gn, dev(p.dy), nsplit, dropout)


# ---- references, computed once and never modified ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dy_probe_set(cid):
    c = W.case(cid)
    probes = W.dy_probes(c, SEED)
    return probes, [W.expected_dy_probe(c, W.cat(p.x0, p.x1), p.table) for p in probes]


@functools.lru_cache(maxsize=None)
def x_probe_set(cid):
    c = W.case(cid)
    probes = W.x_probes(c, SEED)
    return probes, [W.expected_x_probe(c, p.dy, p.table) for p in probes]


@functools.lru_cache(maxsize=None)
def dense_set(cid):
    c = W.case(cid)
    x0, x1, dy = W.dense_inputs(c, SEED)
    return W.Probe(x0, x1, dy, None)


@functools.lru_cache(maxsize=None)
def prologue(cid, inst):
    """GroupNorm + Swish (+ dropout, keep 0.85) of the case's dense input (dy_probes and the dense test share it): the device scale
    and shift, the keep bits, and the float64 activation formed from THOSE scale / shift values with its pre-activation."""
    c, cin = W.case(cid), W.cin_of(W.case(cid))
    x0, x1, _ = W.dense_inputs(c, SEED)
    g = torch.Generator().manual_seed(SEED + 11 + W.CASE_IDS.index(cid))
    gamma, beta = torch.randn(cin, generator=g) * 0.5 + 1, torch.randn(cin, generator=g) * 0.3
    scale, shift, _, _ = A._gn_stats(dev(x0), dev(x1), dev(gamma), dev(beta), c.B, c.H * c.W)
    dropout = keep = None
    inv_keep = 1.0
    if inst == "drop":
        n = x0.numel()
        bits = torch.empty((n + 31) // 32, dtype=torch.int32, device=DEV)
        _capi.check(_capi.lib().hdiff_dropout_keep_bits(bits.data_ptr(), n, C.c_float(1.0 - W.DROP_P), C.c_uint64(SEED + 13), C.c_uint64(0),
                                                        torch.cuda.current_stream().cuda_stream), "keep_bits")
        sh = torch.arange(32, device=DEV, dtype=torch.int32)
        keep = ((bits.view(-1, 1) >> sh) & 1).reshape(-1)[:n].view_as(x0).cpu()
        inv_keep = A._inv_keep(W.DROP_P)
        dropout = (bits, inv_keep)
        assert 0.7 < keep.double().mean().item() < 0.95
    torch.cuda.synchronize()
    act, v = W.activation_f64(W.cat(x0, x1), scale.cpu(), shift.cpu(), keep, inv_keep)
    return {"gn": (scale, shift), "dropout": dropout, "act": act, "v": v}


def report(line):
    print(line)
    path = os.environ.get("HDIFF_WGRAD_FAST_REPORT")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


# ---- a, b: exact probes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", W.SPLITS)
@pytest.mark.parametrize("cid", W.CASE_IDS)
def test_dy_probes_come_back_bit_for_bit(cid, which):
    c = W.case(cid)
    probes, wants = dy_probe_set(cid)
    for r, (p, want) in enumerate(zip(probes, wants)):
        got = run(c, p, W.nsplit_of(c, which))
        assert W.exact(got, want), (cid, which, r, (got.cpu().double() - want).abs().max().item())


@pytest.mark.parametrize("which", W.SPLITS)
@pytest.mark.parametrize("cid", W.CASE_IDS)
def test_x_probes_come_back_bit_for_bit(cid, which):
    c = W.case(cid)
    probes, wants = x_probe_set(cid)
    for r, (p, want) in enumerate(zip(probes, wants)):
        got = run(c, p, W.nsplit_of(c, which))
        assert W.exact(got, want), (cid, which, r, (got.cpu().double() - want).abs().max().item())


# ---- c: the probes behind the prologue --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", W.SPLITS)
@pytest.mark.parametrize("cid,inst", PROLOGUES)
def test_dy_probes_behind_the_prologue(cid, inst, which):
    c = W.case(cid)
    pro = prologue(cid, inst)
    worst = 0.0
    for p in dy_probe_set(cid)[0]:
        ref = W.expected_dy_probe(c, pro["act"], p.table)
        vabs = W.expected_dy_probe(c, pro["v"].abs(), p.table._replace(v=torch.ones_like(p.table.v)))
        got = run(c, p, W.nsplit_of(c, which), pro)
        ratio, zeros_exact = W.activation_ratio(got, ref, vabs)
        assert zeros_exact, (cid, inst, which, "a padding or dropped element is not exactly 0")
        worst = max(worst, ratio)
    report(f"c {cid:9s} {inst:5s} nsplit={W.nsplit_of(c, which):<2d} err/gate={worst:.3f}")
    assert worst <= 1.0, f"{cid} {inst} {which}: an element is {worst:.3f} x its gate"


# ---- d: split invariance ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,inst", INSTANCES)
def test_probe_results_do_not_depend_on_the_split_count(cid, inst):
    c = W.case(cid)
    pro = prologue(cid, inst) if inst != "plain" else None
    probes = list(dy_probe_set(cid)[0]) + (list(x_probe_set(cid)[0]) if inst == "plain" else [])
    for r, p in enumerate(probes):
        one = run(c, p, 1, pro)
        assert torch.isfinite(one).all()
        for which in W.SPLITS:
            got = run(c, p, W.nsplit_of(c, which), pro)
            assert torch.equal(got, one), (cid, inst, which, r, "differs from nsplit = 1")
            assert torch.equal(run(c, p, W.nsplit_of(c, which), pro), got), (cid, inst, which, r, "a second call differs")


# ---- e: dense operands ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dense_reference(cid, inst):
    c, p = W.case(cid), dense_set(cid)
    if inst == "plain":
        act, act_sum = W.cat(p.x0, p.x1).double(), None
    else:
        pro = prologue(cid, inst)
        act = pro["act"]
        act_sum = W.wgrad_f64(c, (8 + 4 * pro["v"].abs()) * act.abs(), p.dy.abs())
    return W.wgrad_f64(c, act, p.dy), W.wgrad_f64(c, act.abs(), p.dy.abs()), act_sum


@pytest.mark.parametrize("which", W.SPLITS)
@pytest.mark.parametrize("cid,inst", INSTANCES)
def test_dense_operands_against_float64(cid, inst, which):
    c, ns = W.case(cid), W.nsplit_of(W.case(cid), which)
    pro = prologue(cid, inst) if inst != "plain" else None
    ref, abs_sum, act_sum = dense_reference(cid, inst)
    got = run(c, dense_set(cid), ns, pro)
    assert torch.equal(run(c, dense_set(cid), ns, pro), got), (cid, inst, which, "a second call differs")
    r_op, r_sum = W.dense_ratios(c, got, ref, abs_sum, ns, act_sum)
    report(f"e {cid:9s} {inst:5s} nsplit={ns:<2d} err/per-op-gate={r_op:.3f} err/bound={r_sum:.3f}")
    assert r_op <= 1.0, f"{cid} {inst} {which}: error is {r_op:.3f} x 1e-4 max |ref| + 1e-6"
    assert r_sum <= 1.0, f"{cid} {inst} {which}: an element is {r_sum:.3f} x its fp32 summation bound"
