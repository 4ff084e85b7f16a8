"""The forward conv's dispatch without a GPU: hdiff_conv2d_fwd_route answers, for a descriptor (fake non-null pointers, nothing
launched), which kernel the three forward entries run it on.  The table below lists every conv kind of the default model
(ch 128, ch_mult 1-2-2-2) at a launch that fills the chip and at one just under the threshold, and the descriptors the split-operand
kernels refuse.  The expected values were recorded from the predicate cascade this function replaced (the commit before it),
not from the function: a conv that falls from pairs to triples or to the fp32 kernel passes every tolerance test and only costs time."""
import ctypes as C
import os
import re
import subprocess

import pytest

import hdiff_amd
from hdiff_amd import _capi
from hdiff_amd.engine import conv_taps, tconv_phase_taps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
P = 0x1000            # a non-null, word-aligned "pointer": the route function dereferences none
IGEMM, DIRECT_1X1, X3_1X1, X3_TRIPLES, X3_PAIRS_GN, X3_PAIRS_WORD, S2_PAIRS_WORD = range(7)
PAIR_FIELDS = ("wp_h2", "wp_h2_taps", "wp_h2_s2")


def conv_desc(taps, C0, Cout, B, H, W, C1=0, stride=1, out_map=(1, 0, 1, 0), **over):
    d = _capi.ConvDesc()
    d.x0, d.x1, d.C0, d.C1, d.B, d.H, d.W = P, (P if C1 else None), C0, C1, B, H, W
    d.wp, d.Cout, d.CinPad, d.CoutPad, d.out = P, Cout, (C0 + C1 + 7) // 8 * 8, (Cout + 63) // 64 * 64, P
    d.in_stride, d.VH, d.VW = stride, (H - 1) // stride + 1, (W - 1) // stride + 1
    d.out_sy, d.out_oy, d.out_sx, d.out_ox = out_map
    d.OH, d.OW = d.VH * out_map[0], d.VW * out_map[2]
    d.ntaps = len(taps.dy)
    for t in range(d.ntaps):
        d.tap_dy[t], d.tap_dx[t] = taps.dy[t], taps.dx[t]
    for k, v in over.items():
        setattr(d, k, v)
    return d


def rng(**kw):
    r = _capi.ConvRange()
    for k, v in kw.items():
        setattr(r, k, v)
    return r


T3, T1, T5 = conv_taps(3, 1), conv_taps(1, 0), conv_taps(5, 2)
GN = dict(gn_scale=P, gn_shift=P)
PAIRS = dict(wp_x3=P, wp_h2=P, act_scale=P)          # what Plan.conv sets for a plain 3x3 behind a GroupNorm it knows


def _permuted():
    t = conv_taps(3, 1)
    t.dy[0], t.dy[8], t.dx[0], t.dx[8] = t.dy[8], t.dy[0], t.dx[8], t.dx[0]
    return t


def _repeated():
    t = conv_taps(3, 1)
    t.dy[4], t.dx[4] = t.dy[3], t.dx[3]
    return t


def _phase(py, px, B, residual=None, **r):
    return conv_desc(tconv_phase_taps(py, px), 256, 256, B, 32, 32, out_map=(2, py, 2, px), bias=P, wp_x3=P, residual=residual), rng(**r)


WORDS = dict(absmax_out=0x2000, absmax_in=0x3000)
# name: (descriptor, range struct or None, dropout, (route, pair pack, absmax tail) in the split-operand modes, the same in f32).
# 3x3-neighbourhood launches of 32 x 32 pixels: 4 x cdiv(Cout, 64) workgroups per sample, 192 is the threshold.
TABLE = {
    "head fills": (conv_desc(T3, 3, 128, 24, 32, 32, bias=P), None, 0, (IGEMM, None, 0), (IGEMM, None, 0)),
    "head under": (conv_desc(T3, 3, 128, 23, 32, 32, bias=P), None, 0, (IGEMM, None, 0), (IGEMM, None, 0)),
    "block1 fills": (conv_desc(T3, 128, 128, 24, 32, 32, bias=P, addvec=P, **GN, **PAIRS), None, 0, (X3_PAIRS_GN, "wp_h2", 0), (IGEMM, None, 0)),
    "block1 under": (conv_desc(T3, 128, 128, 23, 32, 32, bias=P, addvec=P, **GN, **PAIRS), None, 0, (IGEMM, None, 0), (IGEMM, None, 0)),
    "block1 concat fills": (conv_desc(T3, 256, 256, 12, 32, 32, C1=128, bias=P, addvec=P, **GN, **PAIRS), None, 0, (X3_PAIRS_GN, "wp_h2", 0), (IGEMM, None, 0)),
    "block1 concat under": (conv_desc(T3, 256, 256, 11, 32, 32, C1=128, bias=P, addvec=P, **GN, **PAIRS), None, 0, (IGEMM, None, 0), (IGEMM, None, 0)),
    "block2 fills": (conv_desc(T3, 128, 128, 24, 32, 32, bias=P, residual=P, **GN, **PAIRS), rng(absmax_out=0x2000), 0, (X3_PAIRS_GN, "wp_h2", 0), (IGEMM, None, 0)),
    "block2 under": (conv_desc(T3, 128, 128, 23, 32, 32, bias=P, residual=P, **GN, **PAIRS), rng(absmax_out=0x2000), 0, (IGEMM, None, 1), (IGEMM, None, 0)),
    "block2 dropout fills": (conv_desc(T3, 128, 128, 24, 32, 32, bias=P, residual=P, **GN, **PAIRS), None, 1, (X3_PAIRS_GN, "wp_h2", 0), (IGEMM, None, 0)),
    "block2 dropout under": (conv_desc(T3, 128, 128, 23, 32, 32, bias=P, residual=P, **GN, **PAIRS), None, 1, (IGEMM, None, 0), (IGEMM, None, 0)),
    "block2 triples (range unknown)": (conv_desc(T3, 128, 128, 24, 32, 32, bias=P, residual=P, wp_x3=P, **GN), None, 0, (X3_TRIPLES, None, 0), (IGEMM, None, 0)),
    # 1x1: B * H * W >= 32768 pixels is the threshold
    "shortcut fills": (conv_desc(T1, 128, 256, 32, 32, 32, C1=128, bias=P, wp_x3=P), None, 0, (X3_1X1, None, 0), (DIRECT_1X1, None, 0)),
    "shortcut under": (conv_desc(T1, 128, 256, 31, 32, 32, C1=128, bias=P, wp_x3=P), None, 0, (IGEMM, None, 0), (IGEMM, None, 0)),
    "attention in-projection fills": (conv_desc(T1, 128, 384, 32, 32, 32, bias=P, wp_x3=P), None, 0, (X3_1X1, None, 0), (DIRECT_1X1, None, 0)),
    "attention in-projection under": (conv_desc(T1, 128, 384, 31, 32, 32, bias=P, wp_x3=P), None, 0, (IGEMM, None, 0), (IGEMM, None, 0)),
    "attention out-projection fills": (conv_desc(T1, 128, 128, 32, 32, 32, bias=P, wp_x3=P), rng(absmax_out=0x2000), 0, (X3_1X1, None, 0), (DIRECT_1X1, None, 0)),
    "attention out-projection under": (conv_desc(T1, 128, 128, 31, 32, 32, bias=P, wp_x3=P), rng(absmax_out=0x2000), 0, (IGEMM, None, 1), (IGEMM, None, 0)),
    "1x1 without a triple pack": (conv_desc(T1, 128, 128, 32, 32, 32, bias=P), rng(absmax_out=0x2000), 0, (DIRECT_1X1, None, 1), (DIRECT_1X1, None, 0)),
    # DownSample: 16 x 16 outputs, 4 workgroups per sample
    "DownSample by word fills": (conv_desc(T5, 128, 128, 48, 32, 32, stride=2, bias=P), rng(absmax_in=0x3000, wp_h2_s2=P), 0, (S2_PAIRS_WORD, "wp_h2_s2", 0), (IGEMM, None, 0)),
    "DownSample by word under": (conv_desc(T5, 128, 128, 47, 32, 32, stride=2, bias=P), rng(absmax_in=0x3000, wp_h2_s2=P), 0, (IGEMM, None, 0), (IGEMM, None, 0)),
    "DownSample without words": (conv_desc(T5, 128, 128, 48, 32, 32, stride=2, bias=P), None, 0, (IGEMM, None, 0), (IGEMM, None, 0)),
    # UpSample: the phases at 32 x 32 with 256 channels (16 workgroups per sample), its 3x3 on the 64 x 64 result
    "phase (0, 0) by word": (*_phase(0, 0, 12, wp_h2_taps=P, **WORDS), 0, (X3_PAIRS_WORD, "wp_h2_taps", 0), (IGEMM, None, 0)),
    "phase (0, 1) by word": (*_phase(0, 1, 12, wp_h2_taps=P, **WORDS), 0, (X3_PAIRS_WORD, "wp_h2_taps", 0), (IGEMM, None, 0)),
    "phase (1, 0) by word": (*_phase(1, 0, 12, wp_h2_taps=P, **WORDS), 0, (X3_PAIRS_WORD, "wp_h2_taps", 0), (IGEMM, None, 0)),
    "phase (1, 1) by word": (*_phase(1, 1, 12, wp_h2_taps=P, **WORDS), 0, (X3_PAIRS_WORD, "wp_h2_taps", 0), (IGEMM, None, 0)),
    "phase (1, 1) by word under": (*_phase(1, 1, 11, wp_h2_taps=P, **WORDS), 0, (IGEMM, None, 1), (IGEMM, None, 0)),
    "phase (0, 0) without input words": (*_phase(0, 0, 12, absmax_out=0x2000), 0, (X3_TRIPLES, None, 0), (IGEMM, None, 0)),
    "phase (0, 1) without input words": (*_phase(0, 1, 12, absmax_out=0x2000), 0, (X3_TRIPLES, None, 0), (IGEMM, None, 0)),
    "phase (1, 0) without input words": (*_phase(1, 0, 12, absmax_out=0x2000), 0, (X3_TRIPLES, None, 0), (IGEMM, None, 0)),
    "phase (1, 1) without input words": (*_phase(1, 1, 12, absmax_out=0x2000), 0, (X3_TRIPLES, None, 0), (IGEMM, None, 0)),
    "UpSample 3x3 by word fills": (conv_desc(T3, 256, 256, 3, 64, 64, bias=P, wp_x3=P, wp_h2=P), rng(absmax_in=0x3000), 0, (X3_PAIRS_WORD, "wp_h2", 0), (IGEMM, None, 0)),
    "UpSample 3x3 by word under": (conv_desc(T3, 256, 256, 2, 64, 64, bias=P, wp_x3=P, wp_h2=P), rng(absmax_in=0x3000), 0, (IGEMM, None, 0), (IGEMM, None, 0)),
    "tail fills": (conv_desc(T3, 128, 3, 48, 32, 32, bias=P, **GN, **PAIRS), None, 0, (X3_PAIRS_GN, "wp_h2", 0), (IGEMM, None, 0)),
    "tail under": (conv_desc(T3, 128, 3, 47, 32, 32, bias=P, **GN, **PAIRS), None, 0, (IGEMM, None, 0), (IGEMM, None, 0)),
    # refused by the split-operand kernels: the fp32 kernel runs them
    "permuted tap list": (conv_desc(_permuted(), 128, 128, 24, 32, 32, **GN, **PAIRS), None, 0, (IGEMM, None, 0), (IGEMM, None, 0)),
    "repeated tap": (conv_desc(_repeated(), 128, 128, 24, 32, 32, **GN, **PAIRS), None, 0, (IGEMM, None, 0), (IGEMM, None, 0)),
    "Cin % 16 != 0": (conv_desc(T3, 24, 128, 24, 32, 32, **GN, **PAIRS), None, 0, (IGEMM, None, 0), (IGEMM, None, 0)),
    "concat with C0 % 16 != 0": (conv_desc(T3, 40, 128, 24, 32, 32, C1=24, **GN, **PAIRS), None, 0, (IGEMM, None, 0), (IGEMM, None, 0)),
    "phase with a residual": (*_phase(1, 0, 12, residual=P, wp_h2_taps=P, **WORDS), 0, (IGEMM, None, 1), (IGEMM, None, 0)),
}


def route_of(d, r, dropout):
    route, tail = C.c_int(-1), C.c_int(-1)
    rc = hdiff_amd.lib().hdiff_conv2d_fwd_route(d, r, dropout, C.byref(route), C.byref(tail))
    assert rc == 0, hdiff_amd.lib().hdiff_last_error().decode()
    return route.value, tail.value


def pair_pack_of(d, r, dropout):
    """The pair pack a route reads, observed from outside: the one pointer whose removal changes the route."""
    route = route_of(d, r, dropout)[0]
    found = []
    for field in PAIR_FIELDS:
        owner = d if field == "wp_h2" else r
        if owner is None or not getattr(owner, field):
            continue
        setattr(owner, field, None)
        if route_of(d, r, dropout)[0] != route:
            found.append(field)
        setattr(owner, field, P)
    assert len(found) <= 1, found
    return found[0] if found else None


@pytest.fixture
def mode(request):
    before = hdiff_amd.get_contraction_mode()
    hdiff_amd.set_contraction_mode(request.param)
    yield request.param
    hdiff_amd.set_contraction_mode(before)


@pytest.mark.parametrize("mode", ["bf16x3", "f16", "f32"], indirect=True)
def test_every_conv_kind_takes_the_route_it_took(mode):
    for name, (d, r, dropout, split, f32) in TABLE.items():
        want = f32 if mode == "f32" else split
        route, tail = route_of(d, r, dropout)
        assert (route, pair_pack_of(d, r, dropout), tail) == want, (name, mode)
        if mode == "f32":      # no x3 or pair route, no tail launch, whatever the descriptor offers
            assert route in (IGEMM, DIRECT_1X1) and tail == 0, name
    routes = {split[0] for _, _, _, split, _ in TABLE.values()}
    assert routes == set(range(7))


@pytest.mark.parametrize("mode", ["bf16x3", "f32"], indirect=True)
def test_the_workspace_query_is_zero_exactly_off_the_fp32_kernel(mode):
    """hdiff_conv2d_fwd_workspace asks the same function without a range struct: 0 for DIRECT_1X1, X3_1X1 and the three X3_* routes."""
    lib = hdiff_amd.lib()
    seen = set()
    for name, (d, _, _, _, _) in TABLE.items():
        route, _ = route_of(d, None, 0)
        need = C.c_int64(-1)
        assert lib.hdiff_conv2d_fwd_workspace(d, C.byref(need)) == 0, name
        assert route not in (X3_PAIRS_WORD, S2_PAIRS_WORD)  # they need a range struct
        if route != IGEMM:                                 # (IGEMM: the split-K floats configure() wants, 0 for a grid that fills the chip)
            assert need.value == 0, (name, route)
        seen.add(route)
    under = TABLE["block1 under"][0]                       # a small grid with a long channel loop: the fp32 kernel splits K
    need = C.c_int64(-1)
    assert lib.hdiff_conv2d_fwd_workspace(under, C.byref(need)) == 0 and need.value > 0
    assert seen == ({IGEMM, DIRECT_1X1} if mode == "f32" else {IGEMM, DIRECT_1X1, X3_1X1, X3_TRIPLES, X3_PAIRS_GN})


def test_the_route_entry_validates_like_the_forward_entries():
    lib = hdiff_amd.lib()
    route, tail = C.c_int(-1), C.c_int(-1)
    out = (C.byref(route), C.byref(tail))

    def refused(rc, *words):
        msg = lib.hdiff_last_error().decode()
        assert rc == INVALID, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)

    good = TABLE["block1 fills"][0]
    refused(lib.hdiff_conv2d_fwd_route(good, None, 0, None, C.byref(tail)), "conv2d_fwd_route", "null")
    refused(lib.hdiff_conv2d_fwd_route(None, None, 0, *out), "null")
    # absmax_in together with gn_scale: the word describes x, not the prologue's output
    refused(lib.hdiff_conv2d_fwd_route(good, rng(absmax_in=0x3000), 0, *out), "conv2d_fwd_range", "prologue")
    refused(lib.hdiff_conv2d_fwd_route(good, rng(absmax_out=0x2002), 0, *out), "conv2d_fwd_range", "aligned")
    refused(lib.hdiff_conv2d_fwd_route(good, rng(wp_h2_s2=P, absmax_in=0x3000), 0, *out), "conv2d_fwd_range")
    refused(lib.hdiff_conv2d_fwd_route(TABLE["head fills"][0], None, 1, *out), "conv2d_fwd_dropout", "prologue")
    refused(lib.hdiff_conv2d_fwd_route(TABLE["block1 concat fills"][0], None, 1, *out), "conv2d_fwd_dropout", "concat")
    refused(lib.hdiff_conv2d_fwd_route(good, rng(absmax_out=0x2000), 1, *out), "conv2d_fwd_route", "dropout")
    bad = conv_desc(T3, 128, 128, 24, 32, 32, CoutPad=48)
    refused(lib.hdiff_conv2d_fwd_route(bad, None, 0, *out), "conv2d_fwd:", "padded channel counts")
    assert (route.value, tail.value) == (-1, -1)           # a refused call writes nothing


def test_the_route_entry_is_declared_exported_and_bound():
    lib = hdiff_amd.lib()
    assert lib.hdiff_abi_version() == 6
    header = open(os.path.join(ROOT, "include", "hdiff.h")).read()
    names = re.findall(r"HDIFF_CONV_ROUTE_([A-Z0-9_]+) = (\d)", header)
    assert names == [("IGEMM", "0"), ("DIRECT_1X1", "1"), ("X3_1X1", "2"), ("X3_TRIPLES", "3"), ("X3_PAIRS_GN", "4"),
                     ("X3_PAIRS_WORD", "5"), ("S2_PAIRS_WORD", "6")]
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    name = "hdiff_conv2d_fwd_route"
    assert re.search(r"\b%s\s*\(" % name, header)
    assert name in set(re.findall(r" T (hdiff_[a-z0-9_]+)", nm))
    assert name in _capi.EXPORTED_SYMBOLS
    assert getattr(lib, name).restype is C.c_int
