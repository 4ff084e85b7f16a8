"""The range-word entries of the C ABI without a GPU: declared in include/hdiff.h, exported by libhdiff.so, bound by _capi.py,
ABI still 6 -- and every validation rule answers HDIFF_ERR_INVALID with a message before anything is launched (there is no device
here: a call that got past its checks would fail with a launch error instead)."""
import ctypes as C
import os
import re
import subprocess

import hdiff_amd
from hdiff_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hdiff_conv2d_fwd_range", "hdiff_range_words_zero", "hdiff_pack_conv_weight_h2_taps_words", "hdiff_pack_conv_weight_h2_taps",
       "hdiff_pack_conv_weight_h2_s2_words", "hdiff_pack_conv_weight_h2_s2")
KEPT = ("hdiff_conv2d_fwd", "hdiff_conv2d_fwd_dropout", "hdiff_conv2d_fwd_workspace", "hdiff_pack_conv_weight_h2",
        "hdiff_pack_conv_weight_x3_taps")
INVALID = -1
P = 0x1000            # a non-null, word-aligned "pointer": never dereferenced by a call that is refused on the host


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
    assert re.search(r"typedef struct hdiff_conv_range \{[^}]*absmax_out;[^}]*absmax_in;[^}]*wp_h2_taps;[^}]*wp_h2_s2;[^}]*\}", header)
    assert C.sizeof(_capi.ConvRange) == 4 * C.sizeof(C.c_void_p)


def test_the_descriptor_is_what_it_was():
    """hdiff_conv_desc did not grow: the new fields live in a struct of their own."""
    assert len(_capi.ConvDesc._fields_) == 34 and C.sizeof(_capi.ConvDesc) == 392
    assert [n for n, _ in _capi.ConvDesc._fields_][-3:] == ["wp_x3", "wp_h2", "act_scale"]


def conv_desc(**over):
    d = _capi.ConvDesc()
    d.x0, d.x1, d.C0, d.C1, d.B, d.H, d.W = P, None, 64, 0, 2, 16, 16
    d.wp, d.bias, d.Cout, d.CinPad, d.CoutPad = P, None, 64, 64, 64
    d.gn_scale, d.gn_shift, d.out, d.OH, d.OW = None, None, P, 16, 16
    d.VH, d.VW, d.in_stride = 16, 16, 1
    d.out_sy, d.out_oy, d.out_sx, d.out_ox = 1, 0, 1, 0
    d.ntaps = 9
    for t in range(9):
        d.tap_dy[t], d.tap_dx[t] = t // 3 - 1, t % 3 - 1
    for k, v in over.items():
        setattr(d, k, v)
    return d


def rng(**kw):
    r = _capi.ConvRange()
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def refused(rc, *words):
    msg = hdiff_amd.lib().hdiff_last_error().decode()
    assert rc == INVALID, (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


def test_conv_forward_range_validation():
    fwd = hdiff_amd.lib().hdiff_conv2d_fwd_range
    refused(fwd(None, rng(absmax_out=P), None), "conv2d_fwd_range", "null")
    refused(fwd(conv_desc(), None, None), "conv2d_fwd_range", "null")
    refused(fwd(conv_desc(), rng(absmax_out=P + 2), None), "aligned")
    refused(fwd(conv_desc(), rng(absmax_in=P + 1), None), "aligned")
    refused(fwd(conv_desc(), rng(absmax_out=P, absmax_in=P), None), "same words")
    refused(fwd(conv_desc(gn_scale=P, gn_shift=P), rng(absmax_in=P), None), "prologue")
    refused(fwd(conv_desc(), rng(wp_h2_taps=P), None), "wp_h2_taps without absmax_in")
    refused(fwd(conv_desc(), rng(wp_h2_s2=P), None), "wp_h2_s2 without absmax_in")
    five = conv_desc(ntaps=25)
    refused(fwd(five, rng(absmax_in=P, wp_h2_taps=P), None), "at most 9 taps")
    refused(fwd(conv_desc(), rng(absmax_in=P, wp_h2_s2=P), None), "25-tap stride-2")
    refused(fwd(conv_desc(ntaps=25), rng(absmax_in=P, wp_h2_s2=P), None), "25-tap stride-2")        # stride 1
    # the rules of hdiff_conv2d_fwd itself still hold behind them
    refused(fwd(conv_desc(x0=None), rng(absmax_out=P), None), "null")
    refused(fwd(conv_desc(CoutPad=48), rng(absmax_out=P), None), "padded channel counts")
    refused(fwd(conv_desc(gn_scale=P), rng(absmax_out=P), None), "gn_scale/gn_shift")


def test_packers_and_zeroing_validation():
    lib = hdiff_amd.lib()
    words = C.c_int64(-1)
    assert lib.hdiff_pack_conv_weight_h2_taps_words(96, 48, 128, 6, C.byref(words)) == 0
    assert words.value == 3 * 6 * 2 * 128 * 8 + 4
    assert lib.hdiff_pack_conv_weight_h2_s2_words(96, 48, 128, C.byref(words)) == 0
    assert words.value == 3 * 25 * 2 * 128 * 8 + 4
    refused(lib.hdiff_pack_conv_weight_h2_taps_words(96, 48, 128, 6, None), "pack_conv_weight_h2_taps_words", "null")
    refused(lib.hdiff_pack_conv_weight_h2_taps_words(96, 40, 128, 6, C.byref(words)), "Cin %")
    refused(lib.hdiff_pack_conv_weight_h2_taps_words(96, 48, 96, 6, C.byref(words)), "CoutPad %")
    refused(lib.hdiff_pack_conv_weight_h2_taps_words(96, 48, 128, 10, C.byref(words)), "ntaps")
    refused(lib.hdiff_pack_conv_weight_h2_s2_words(96, 48, 128, None), "pack_conv_weight_h2_s2_words", "null")
    refused(lib.hdiff_pack_conv_weight_h2_s2_words(96, 40, 128, C.byref(words)), "Cin %")
    ky, kx = (C.c_int * 4)(1, 1, 3, 3), (C.c_int * 4)(1, 3, 1, 3)
    pack = lib.hdiff_pack_conv_weight_h2_taps
    refused(pack(None, P, 1, 64, 64, 5, 5, 4, ky, kx, 64, None), "pack_conv_weight_h2_taps", "null")
    refused(pack(P, P, 1, 64, 64, 5, 5, 4, None, kx, 64, None), "pack_conv_weight_h2_taps", "null")
    refused(pack(P, P, 2, 64, 64, 5, 5, 4, ky, kx, 64, None), "mode")
    refused(pack(P, P, 1, 64, 60, 5, 5, 4, ky, kx, 64, None), "Cin %")
    refused(pack(P, P, 1, 64, 64, 5, 5, 0, ky, kx, 64, None), "ntaps")
    refused(pack(P, P, 1, 64, 64, 3, 3, 4, ky, kx, 64, None), "tap 1 reads kernel element (1, 3)")
    s2 = lib.hdiff_pack_conv_weight_h2_s2
    refused(s2(None, P, 64, 64, 64, 64, None), "pack_conv_weight_h2_s2", "null")
    refused(s2(P, None, 64, 64, 64, 64, None), "pack_conv_weight_h2_s2", "null")
    refused(s2(P, P, 64, 72, 72, 64, None), "Cin %")
    refused(s2(P, P, 64, 64, 60, 64, None), "CinPad")
    refused(s2(P, P, 96, 64, 64, 96, None), "CoutPad")
    refused(lib.hdiff_range_words_zero(None, 4, None), "range_words_zero", "null")
    refused(lib.hdiff_range_words_zero(P, 0, None), "range_words_zero")
