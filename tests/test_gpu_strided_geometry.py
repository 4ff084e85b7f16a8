"""The stride-2 and output-parity convolutions at 32-wide tiles, the generic weight gradient on planes shorter than its tile, and
fused_conv at small planes of several 32-wide tiles that take the fast weight-gradient kernels ("-fast": the 3x3 behind GroupNorm + Swish,
with dropout and without a prologue, and the 1x1), through the autograd entry points the trainers use (A._DownFn, A._TConvFn,
A._StridedConvFn, A.fused_conv).

tests/test_gpu_backward.py runs these ops on planes whose virtual output is at most 16 wide; both launchers pick another program
above that (tests/_strided_geometry_cases.py lists the cases and what each reaches).  Every case here

  * names the weight-gradient route of each of its launches (hdiff_conv2d_wgrad_route): a shape that falls to another kernel
    turns red instead of passing on the wrong one;
  * agrees with torch on the CPU in float64 (F.conv2d / F.conv_transpose2d and autograd of them) within the per-op gates of
    tests/test_gpu_backward.py: forward 3e-5, dX 5e-5, dW / bias (and GroupNorm weight) gradients 1e-4, each of max |ref|, plus 1e-6;
  * has finite gradients, and a second backward on the same inputs gives bitwise the same ones (the weight gradient sums its
    splits in a fixed order, no atomics: whatever a kernel read beyond its staged patch would break this on a short plane);
  * runs twice: dy = "randn", and dy = "edge", where dY is zero except in the last live row and the last live column of the
    launches' virtual output grid and, where a row has several 32-wide tiles, the first column of the last tile (for _TConvFn:
    of each phase's grid, that is two rows / columns of the doubled output).  dW and dX are then made of edge pixels alone: a dropped
    or misplaced one is an error of the size of the result, not one term among hundreds; the gates are relative to that
    reference's own maximum.

HDIFF_STRIDED_GEOMETRY_REPORT=<file> appends the measured error / gate ratio of every tensor (profiles/strided_geometry.txt)."""
import ctypes as C
import functools
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))      # _strided_geometry_cases

from hdiff_amd import _capi  # noqa: E402
from hdiff_amd import autograd as A  # noqa: E402
import _strided_geometry_cases as K  # noqa: E402

DEV = "cuda:0"
B = K.B
DROP_P = 0.25
GATES = {"fwd": 3e-5, "dx": 5e-5}      # everything else (dW, bias and GroupNorm weight gradients): 1e-4


def ratio(got, ref, rel):
    """error / gate, the gate of tests/test_gpu_backward.py::close: rel * max |ref| + 1e-6"""
    got, ref = got.detach().cpu().double(), ref.detach().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return (got - ref).abs().max().item() / (rel * ref.abs().max().item() + 1e-6)


@functools.lru_cache(maxsize=None)
def inputs(cid):
    """Seeded randn inputs of a case (weights scaled by 1 / sqrt(fan_in)), the same for both dy modes: name -> float32 CPU tensor."""
    _, kind, (cin, cout, H, W), _, _ = K.CASES[K.CASE_IDS.index(cid)]
    g = torch.Generator().manual_seed(1000 + K.CASE_IDS.index(cid))
    rn = lambda *s: torch.randn(*s, generator=g)
    t = {"x": rn(B, cin, H, W)}
    if kind == "down":
        t.update(w1=rn(cout, cin, 3, 3) / math.sqrt(cin * 9), b1=rn(cout), w2=rn(cout, cin, 5, 5) / math.sqrt(cin * 25), b2=rn(cout))
    elif kind == "tconv":
        t.update(wt=rn(cin, cout, 5, 5) / math.sqrt(cin * 25), bt=rn(cout))
    elif kind == "strided":
        t.update(w=rn(cout, cin, 3, 3) / math.sqrt(cin * 9), b=rn(cout))
    else:
        k = 1 if kind == "conv1" else 3
        t.update(w=rn(cout, cin, k, k) / math.sqrt(cin * k * k), b=rn(cout))
        if kind not in ("conv1", "conv3"):
            t.update(gamma=rn(cin) * 0.5 + 1, beta=rn(cin) * 0.3)
    t["dy_randn"] = rn(*out_shape(kind, cout, H, W))
    return t


def out_shape(kind, cout, H, W):
    if kind in ("down", "strided"):
        return B, cout, (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return (B, cout, 2 * H, 2 * W) if kind == "tconv" else (B, cout, H, W)


def edge_mask(kind, shape):
    """1 on the output pixels of the virtual grid's last row, last column and (several x tiles) the last tile's first column."""
    VH, VW, sy, sx = K.virtual_grid(kind, shape)
    m = torch.zeros(VH, VW)
    m[VH - 1, :] = 1
    m[:, VW - 1] = 1
    if VW > 32:
        m[:, (VW - 1) // 32 * 32] = 1
    return m.repeat_interleave(sy, 0).repeat_interleave(sx, 1)


def hip_op(kind, t, seed):
    if kind == "down":
        return A._DownFn.apply(t["x"], t["w1"], t["b1"], t["w2"], t["b2"])
    if kind == "tconv":
        return A._TConvFn.apply(t["x"], t["wt"], t["bt"])
    if kind == "strided":
        return A._StridedConvFn.apply(t["x"], t["w"], t["b"])
    if kind == "conv1":
        return A.fused_conv(t["x"], None, t["w"], t["b"], k=1)
    if kind == "conv3":
        return A.fused_conv(t["x"], None, t["w"], t["b"], k=3)
    if kind == "conv3-gn":
        return A.fused_conv(t["x"], None, t["w"], t["b"], t["gamma"], t["beta"], k=3)
    torch.manual_seed(seed)          # fused_conv draws the dropout seed from torch's generator
    return A.fused_conv(t["x"], None, t["w"], t["b"], t["gamma"], t["beta"], k=3, drop_p=DROP_P)


def keep_mask(n, seed):
    """The forward's keep decisions from the C ABI (hdiff_dropout_keep_bits, one bit per element) times its fp32 1 / keep, as float64
    on the CPU: the reference construction of tests/test_gpu_fused_dropout.py."""
    torch.manual_seed(seed)
    drawn = int(torch.empty((), dtype=torch.int64).random_().item())           # the seed as fused_conv draws it
    words = torch.empty((n + 31) // 32, dtype=torch.int32, device=DEV)
    _capi.check(_capi.lib().hdiff_dropout_keep_bits(words.data_ptr(), n, C.c_float(1.0 - DROP_P), C.c_uint64(drawn), C.c_uint64(0),
                                                    torch.cuda.current_stream().cuda_stream), "keep_bits")
    sh = torch.arange(32, device=DEV, dtype=torch.int32)
    bits = ((words.view(-1, 1) >> sh) & 1).reshape(-1)[:n]
    return bits.cpu().double() * A._inv_keep(DROP_P)


def ref_op(kind, t, mask):
    if kind == "down":
        return F.conv2d(t["x"], t["w1"], t["b1"], stride=2, padding=1) + F.conv2d(t["x"], t["w2"], t["b2"], stride=2, padding=2)
    if kind == "tconv":
        return F.conv_transpose2d(t["x"], t["wt"], t["bt"], stride=2, padding=2, output_padding=1)
    if kind == "strided":
        return F.conv2d(t["x"], t["w"], t["b"], stride=2, padding=1)
    if kind == "conv1":
        return F.conv2d(t["x"], t["w"], t["b"])
    if kind == "conv3":
        return F.conv2d(t["x"], t["w"], t["b"], padding=1)
    a = F.group_norm(t["x"], 32, t["gamma"], t["beta"], 1e-5)
    a = a * torch.sigmoid(a)
    if mask is not None:
        a = a * mask.view_as(a)
    return F.conv2d(a, t["w"], t["b"], padding=1)


def report(cid, dy, ratios):
    line = f"{cid:32s} dy={dy:5s} " + " ".join(f"{n}={r:.3f}" for n, r in ratios.items())
    print(line)
    path = os.environ.get("HDIFF_STRIDED_GEOMETRY_REPORT")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


@pytest.mark.parametrize("dy", ["randn", "edge"])
@pytest.mark.parametrize("cid", K.CASE_IDS)
def test_strided_geometry_matches_float64(cid, dy):
    _, kind, shape, route, _ = K.CASES[K.CASE_IDS.index(cid)]
    for d, dropout in K.case_descs(kind, shape):
        assert K.route_of(d, dropout) == route, (cid, "weight-gradient route")
    t = inputs(cid)
    names = [n for n in t if n != "dy_randn"]
    dout = t["dy_randn"] * edge_mask(kind, shape) if dy == "edge" else t["dy_randn"]
    assert dout.abs().max().item() > 0
    seed = 77

    hip = {n: t[n].to(DEV).requires_grad_(True) for n in names}
    y = hip_op(kind, hip, seed)
    first = torch.autograd.grad(y, [hip[n] for n in names], dout.to(DEV), retain_graph=True)
    again = torch.autograd.grad(y, [hip[n] for n in names], dout.to(DEV))

    mask = keep_mask(t["x"].numel(), seed) if kind == "conv3-gn-drop" else None
    ref = {n: t[n].double().requires_grad_(True) for n in names}
    y_ref = ref_op(kind, ref, mask)
    g_ref = torch.autograd.grad(y_ref, [ref[n] for n in names], dout.double())

    ratios = {"fwd": ratio(y, y_ref, GATES["fwd"])}
    for n, g in zip(names, first):
        ratios["d" + n] = ratio(g, g_ref[names.index(n)], GATES.get("d" + n, 1e-4))
    report(cid, dy, ratios)
    for n, g, g2 in zip(names, first, again):
        assert torch.isfinite(g).all(), (cid, dy, "d" + n, "not finite")
        assert torch.equal(g, g2), (cid, dy, "d" + n, "a second backward on the same inputs differs")
    for n, r in ratios.items():
        assert r <= 1.0, f"{cid} dy={dy} {n}: error is {r:.3f} x its gate"
