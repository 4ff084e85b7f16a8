"""The fused-dropout entries of the C ABI without a GPU: declared in include/hdiff.h, exported by libhdiff.so, bound by
_capi.py, ABI still 6 -- and every validation rule answers with an error code and a message before anything is launched
(there is no device here to launch on: a call that got past its checks would fail with a launch error, not HDIFF_ERR_INVALID)."""
import ctypes as C
import math
import os
import re
import subprocess

import hdiff_amd
from hdiff_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hdiff_dropout_keep_bits", "hdiff_conv2d_fwd_dropout", "hdiff_conv2d_wgrad_dropout", "hdiff_gn_swish_dropout_bwd")
KEPT = ("hdiff_gn_swish_apply", "hdiff_dropout_mask", "hdiff_mul", "hdiff_conv2d_fwd", "hdiff_conv2d_wgrad", "hdiff_gn_swish_bwd")
INVALID = -1
P = 0x1000            # a non-null "pointer": never dereferenced by a call that is refused on the host


def test_new_entries_are_declared_exported_and_bound():
    lib = hdiff_amd.lib()
    assert lib.hdiff_abi_version() == 6
    header = open(os.path.join(ROOT, "include", "hdiff.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (hdiff_[a-z0-9_]+)", nm))
    for name in NEW + KEPT:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in exported, name
        assert name in _capi.EXPORTED_SYMBOLS, name
        assert getattr(lib, name).restype is C.c_int


def conv_desc(**over):
    d = _capi.ConvDesc()
    d.x0, d.x1, d.C0, d.C1, d.B, d.H, d.W = P, None, 64, 0, 2, 16, 16
    d.wp, d.bias, d.Cout, d.CinPad, d.CoutPad = P, None, 64, 64, 64
    d.gn_scale, d.gn_shift, d.out, d.OH, d.OW = P, P, P, 16, 16
    d.VH, d.VW, d.in_stride = 16, 16, 1
    d.out_sy, d.out_oy, d.out_sx, d.out_ox = 1, 0, 1, 0
    d.ntaps = 9
    for t in range(9):
        d.tap_dy[t], d.tap_dx[t] = t // 3 - 1, t % 3 - 1
    for k, v in over.items():
        setattr(d, k, v)
    return d


def wgrad_desc(**over):
    d = _capi.WgradDesc()
    d.x0, d.x1, d.C0, d.C1, d.B, d.H, d.W = P, None, 64, 0, 2, 16, 16
    d.gn_scale, d.gn_shift, d.dy = P, P, P
    d.Cout, d.CinPad, d.CoutPad, d.OH, d.OW = 64, 64, 64, 16, 16
    d.VH, d.VW, d.in_stride = 16, 16, 1
    d.out_sy, d.out_oy, d.out_sx, d.out_ox = 1, 0, 1, 0
    d.ntaps = 9
    for t in range(9):
        d.tap_dy[t], d.tap_dx[t] = t // 3 - 1, t % 3 - 1
    for k, v in over.items():
        setattr(d, k, v)
    return d


def refused(rc, *words):
    msg = hdiff_amd.lib().hdiff_last_error().decode()
    assert rc == INVALID, (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


def test_keep_bits_validation():
    lib = hdiff_amd.lib()
    refused(lib.hdiff_dropout_keep_bits(None, 64, 0.5, 1, 0, None), "dropout_keep_bits", "null")
    refused(lib.hdiff_dropout_keep_bits(P, 0, 0.5, 1, 0, None), "dropout_keep_bits")
    refused(lib.hdiff_dropout_keep_bits(P, -5, 0.5, 1, 0, None), "dropout_keep_bits")
    for keep in (0.0, -0.25, 1.0000001, math.nan, math.inf):
        refused(lib.hdiff_dropout_keep_bits(P, 64, keep, 1, 0, None), "keep")


BAD_INV_KEEP = (math.nan, math.inf, -math.inf, 0.0, 0.5, -2.0)


def test_conv_forward_dropout_validation():
    lib = hdiff_amd.lib()
    fwd = lib.hdiff_conv2d_fwd_dropout
    refused(fwd(None, P, 2.0, None), "conv2d_fwd_dropout", "null")
    refused(fwd(conv_desc(), None, 2.0, None), "conv2d_fwd_dropout", "null")
    for v in BAD_INV_KEEP:
        refused(fwd(conv_desc(), P, v, None), "inv_keep")
    refused(fwd(conv_desc(x1=P, C1=64, CinPad=128), P, 2.0, None), "x1")
    refused(fwd(conv_desc(gn_scale=None, gn_shift=None), P, 2.0, None), "prologue")
    refused(fwd(conv_desc(gn_shift=None), P, 2.0, None), "prologue")
    # not a plain 3x3 / stride 1 / pad 1: a 1x1, a strided conv, a transposed-conv phase, taps in another order, another grid
    one = conv_desc(ntaps=1)
    one.tap_dy[0] = one.tap_dx[0] = 0
    refused(fwd(one, P, 2.0, None), "plain 3x3")
    refused(fwd(conv_desc(in_stride=2, VH=8, VW=8, OH=8, OW=8), P, 2.0, None), "plain 3x3")
    refused(fwd(conv_desc(out_sy=2, out_sx=2, OH=32, OW=32), P, 2.0, None), "plain 3x3")
    swapped = conv_desc()
    swapped.tap_dx[0], swapped.tap_dx[2] = 1, -1
    refused(fwd(swapped, P, 2.0, None), "plain 3x3")
    refused(fwd(conv_desc(VH=8), P, 2.0, None), "plain 3x3")
    refused(fwd(conv_desc(C0=60, CinPad=64), P, 2.0, None), "multiple of 8")
    refused(fwd(conv_desc(B=1 << 14, H=512, W=512, VH=512, VW=512, OH=512, OW=512), P, 2.0, None), "2^31")
    # the rules of hdiff_conv2d_fwd itself still hold behind them
    refused(fwd(conv_desc(x0=None), P, 2.0, None), "null")
    refused(fwd(conv_desc(CoutPad=48), P, 2.0, None), "padded channel counts")


def test_conv_wgrad_dropout_validation():
    lib = hdiff_amd.lib()
    wg = lib.hdiff_conv2d_wgrad_dropout
    refused(wg(None, P, 2.0, P, 1, None), "conv2d_wgrad_dropout", "null")
    refused(wg(wgrad_desc(), None, 2.0, P, 1, None), "conv2d_wgrad_dropout", "null")
    refused(wg(wgrad_desc(), P, 2.0, None, 1, None), "conv2d_wgrad_dropout", "null")
    for v in BAD_INV_KEEP:
        refused(wg(wgrad_desc(), P, v, P, 1, None), "inv_keep")
    refused(wg(wgrad_desc(x1=P, C1=64, CinPad=128), P, 2.0, P, 1, None), "x1")
    refused(wg(wgrad_desc(gn_scale=None, gn_shift=None), P, 2.0, P, 1, None), "prologue")
    refused(wg(wgrad_desc(in_stride=2, VH=8, VW=8, OH=8, OW=8), P, 2.0, P, 1, None), "plain 3x3")
    five = wgrad_desc(ntaps=25)
    refused(wg(five, P, 2.0, P, 1, None), "plain 3x3")
    refused(wg(wgrad_desc(B=1 << 14, H=512, W=512, VH=512, VW=512, OH=512, OW=512), P, 2.0, P, 1, None), "2^31")
    refused(wg(wgrad_desc(x0=None), P, 2.0, P, 1, None), "null")
    refused(wg(wgrad_desc(), P, 2.0, P, 0, None), "bad geometry")


def test_groupnorm_swish_dropout_backward_validation():
    lib = hdiff_amd.lib()
    bwd = lib.hdiff_gn_swish_dropout_bwd
    good = dict(x=P, C=64, B=2, HW=256, G=32, dA=P, keep_bits=P, inv_keep=2.0, mean=P, rstd=P, gamma=P, beta=P, ws=P, dx=P, dgamma=P,
                dbeta=P)

    def call(**over):
        a = dict(good, **over)
        return bwd(a["x"], a["C"], a["B"], a["HW"], a["G"], a["dA"], a["keep_bits"], a["inv_keep"], a["mean"], a["rstd"], a["gamma"],
                   a["beta"], a["ws"], a["dx"], a["dgamma"], a["dbeta"], None)

    for name in ("x", "dA", "keep_bits", "mean", "rstd", "gamma", "beta", "ws", "dx", "dgamma", "dbeta"):
        refused(call(**{name: None}), "gn_swish_dropout_bwd", "null")
    for v in BAD_INV_KEEP:
        refused(call(inv_keep=v), "inv_keep")
    refused(call(C=48), "bad sizes")
    refused(call(B=0), "bad sizes")
    refused(call(HW=0), "bad sizes")
    refused(call(G=0), "bad sizes")


def test_python_side_derives_the_kernel_scale():
    """autograd._inv_keep: the fp32 quotient 1.0f / (float)keep, for every dropout rate in steps of 1 / 200."""
    import numpy as np
    from hdiff_amd import autograd as A
    for i in range(1, 200):
        p = i / 200.0
        keep = np.float32(1.0 - p)
        assert A._inv_keep(p) == float(np.float32(1.0) / keep), p
