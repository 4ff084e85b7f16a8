"""The weight gradient's dispatch without a GPU: hdiff_conv2d_wgrad_route answers, for a descriptor (fake non-null pointers, nothing
launched), which kernel hdiff_conv2d_wgrad / hdiff_conv2d_wgrad_dropout run it on.  The table lists every weight-gradient kind of
the default model (ch 128, ch_mult 1-2-2-2, two blocks per level, dropout 0.15) at 64 x 64 / batch 2 and at the levels of the
32 x 32 / batch-80 run, every kind of the second tree's default at 256 x 256 / batch 2 with the image encoder's convs, and every case
of tests/test_gpu_strided_geometry.py.  The expected values were recorded from the predicates this function replaced (the commit
before it: wgrad1x1_applicable, wgrad3x3_applicable, then `tw_log2 == 5` and in_stride), not from the function -- with one exception,
made on purpose: planes shorter than the four-row tile (VH < 4 with VW > 16) ran conv_wgrad_kernel<1> / <2>, which reads rows the
staged patch does not have; they take the generic instantiation now (SHORT_PLANES below names them)."""
import ctypes as C
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))      # _strided_geometry_cases

import hdiff_amd  # noqa: E402
from hdiff_amd import _capi  # noqa: E402
import _strided_geometry_cases as K  # noqa: E402
from _strided_geometry_cases import FAST_1X1, FAST_3X3, GENERIC, ROWS1, ROWS2, P  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


def _res_block(rows, tag, B, C0, C1, out, S, attn):
    cin = f"{C0}|{C1}" if C1 else f"{C0}"
    rows[f"{tag} block1 3x3 gn {cin}->{out} {S}x{S} B{B}"] = (K.plain_desc(3, C0, out, B, S, S, C1=C1, gn=True), 0)
    rows[f"{tag} block2 3x3 gn dropout {out}->{out} {S}x{S} B{B}"] = (K.plain_desc(3, out, out, B, S, S, gn=True), 1)
    if C0 + C1 != out:
        rows[f"{tag} shortcut 1x1 {cin}->{out} {S}x{S} B{B}"] = (K.plain_desc(1, C0, out, B, S, S, C1=C1), 0)
    if attn:
        rows[f"{tag} attention in-projection 1x1 {out}->{3 * out} {S}x{S} B{B}"] = (K.plain_desc(1, out, 3 * out, B, S, S), 0)
        rows[f"{tag} attention out-projection 1x1 {out}->{out} {S}x{S} B{B}"] = (K.plain_desc(1, out, out, B, S, S), 0)


def _unet_rows(rows, tag, B, S, *, head_in, down_attn, middle_attn, up_blocks, ch=128, ch_mult=(1, 2, 2, 2), nrb=2):
    """The weight-gradient launches of one training step, walked like UNet.__init__ / DynamicUNet.__init__ build their blocks and
    autograd.unet_forward_with_grad / dyn_unet_forward_with_grad run them; keyed by kind, so that a repeated kind is one row."""
    rows[f"{tag} head 3x3 {head_in}->{ch} {S}x{S} B{B}"] = (K.plain_desc(3, head_in, ch, B, S, S), 0)
    widths, now, last = [ch], ch, len(ch_mult) - 1
    for level, mult in enumerate(ch_mult):
        for _ in range(nrb):
            _res_block(rows, tag, B, now, 0, ch * mult, S, down_attn)
            now = ch * mult
            widths.append(now)
        if level != last:
            rows[f"{tag} DownSample 5x5/s2 {now} {S}x{S} B{B}"] = (K.s2_desc(now, now, B, S, S), 0)
            S //= 2
            widths.append(now)
    for attn in middle_attn:
        _res_block(rows, tag, B, now, 0, now, S, attn)
    for level in range(last, -1, -1):
        for _ in range(up_blocks):
            _res_block(rows, tag, B, now, widths.pop(), ch * ch_mult[level], S, False)
            now = ch * ch_mult[level]
        if level != 0:
            for i, d in enumerate(K.phase_descs(now, now, B, S, S)):
                rows[f"{tag} UpSample phase ({i >> 1}, {i & 1}) {now} {S}x{S} B{B}"] = (d, 0)
            S *= 2
            rows[f"{tag} UpSample 3x3 {now} {S}x{S} B{B}"] = (K.plain_desc(3, now, now, B, S, S), 0)
    rows[f"{tag} tail 3x3 gn {now}->3 {S}x{S} B{B}"] = (K.plain_desc(3, now, 3, B, S, S, gn=True), 0)


def _table():
    rows = {}
    a = dict(head_in=3, down_attn=True, middle_attn=(True, False), up_blocks=3)
    _unet_rows(rows, "A", 2, 64, **a)
    _unet_rows(rows, "A", 80, 32, **a)
    _unet_rows(rows, "B", 2, 256, head_in=6, down_attn=False, middle_attn=(True,) * 4, up_blocks=2)
    for cin, S in ((3, 256), (8, 128), (16, 64)):                 # ConditionalEmbedding: channels = ch / 16, doubled twice
        rows[f"B image encoder 3x3/s2 {cin}->{2 * cin if cin > 3 else 8} {S}x{S} B2"] = (K.s2_desc(cin, 2 * cin if cin > 3 else 8, 2, S, S), 0)
    for cid, kind, shape, _, _ in K.CASES:
        for i, (d, drop) in enumerate(K.case_descs(kind, shape)):
            rows[f"case {cid}" + (f" phase ({i >> 1}, {i & 1})" if kind == "tconv" else "")] = (d, drop)
    return rows


TABLE = _table()

# Recorded from the parent commit's predicates (see the module docstring); the short planes hold what the parent ran in a comment.
SHORT_PLANES = {
    "case down-4x40-short": GENERIC,                        # parent: ROWS2
    "case tconv-3x24-short phase (0, 0)": GENERIC,          # parent: ROWS1, and the three phases below
    "case tconv-3x24-short phase (0, 1)": GENERIC,
    "case tconv-3x24-short phase (1, 0)": GENERIC,
    "case tconv-3x24-short phase (1, 1)": GENERIC,
    "case enc-3to8-6x40-short": GENERIC,                    # parent: ROWS2
    "case conv3x3-gn-3x24-short": GENERIC,                  # parent: ROWS1
    "case conv1x1-2x20-short": GENERIC,                     # parent: ROWS1
    "case conv3x3-gn-dropout-3x24-short": GENERIC,          # parent: ROWS1 (the dropout instantiation)
}
EXPECTED = {
    "A head 3x3 3->128 64x64 B2": ROWS1,
    "A block1 3x3 gn 128->128 64x64 B2": FAST_3X3,
    "A block2 3x3 gn dropout 128->128 64x64 B2": FAST_3X3,
    "A attention in-projection 1x1 128->384 64x64 B2": FAST_1X1,
    "A attention out-projection 1x1 128->128 64x64 B2": FAST_1X1,
    "A DownSample 5x5/s2 128 64x64 B2": ROWS2,
    "A block1 3x3 gn 128->256 32x32 B2": FAST_3X3,
    "A block2 3x3 gn dropout 256->256 32x32 B2": FAST_3X3,
    "A shortcut 1x1 128->256 32x32 B2": FAST_1X1,
    "A attention in-projection 1x1 256->768 32x32 B2": FAST_1X1,
    "A attention out-projection 1x1 256->256 32x32 B2": FAST_1X1,
    "A block1 3x3 gn 256->256 32x32 B2": FAST_3X3,
    "A DownSample 5x5/s2 256 32x32 B2": GENERIC,
    "A block1 3x3 gn 256->256 16x16 B2": GENERIC,
    "A block2 3x3 gn dropout 256->256 16x16 B2": GENERIC,
    "A attention in-projection 1x1 256->768 16x16 B2": FAST_1X1,
    "A attention out-projection 1x1 256->256 16x16 B2": FAST_1X1,
    "A DownSample 5x5/s2 256 16x16 B2": GENERIC,
    "A block1 3x3 gn 256->256 8x8 B2": GENERIC,
    "A block2 3x3 gn dropout 256->256 8x8 B2": GENERIC,
    "A attention in-projection 1x1 256->768 8x8 B2": FAST_1X1,
    "A attention out-projection 1x1 256->256 8x8 B2": FAST_1X1,
    "A block1 3x3 gn 256|256->256 8x8 B2": GENERIC,
    "A shortcut 1x1 256|256->256 8x8 B2": FAST_1X1,
    "A UpSample phase (0, 0) 256 8x8 B2": GENERIC,
    "A UpSample phase (0, 1) 256 8x8 B2": GENERIC,
    "A UpSample phase (1, 0) 256 8x8 B2": GENERIC,
    "A UpSample phase (1, 1) 256 8x8 B2": GENERIC,
    "A UpSample 3x3 256 16x16 B2": GENERIC,
    "A block1 3x3 gn 256|256->256 16x16 B2": GENERIC,
    "A shortcut 1x1 256|256->256 16x16 B2": FAST_1X1,
    "A UpSample phase (0, 0) 256 16x16 B2": GENERIC,
    "A UpSample phase (0, 1) 256 16x16 B2": GENERIC,
    "A UpSample phase (1, 0) 256 16x16 B2": GENERIC,
    "A UpSample phase (1, 1) 256 16x16 B2": GENERIC,
    "A UpSample 3x3 256 32x32 B2": FAST_3X3,
    "A block1 3x3 gn 256|256->256 32x32 B2": FAST_3X3,
    "A shortcut 1x1 256|256->256 32x32 B2": FAST_1X1,
    "A block1 3x3 gn 256|128->256 32x32 B2": FAST_3X3,
    "A shortcut 1x1 256|128->256 32x32 B2": FAST_1X1,
    "A UpSample phase (0, 0) 256 32x32 B2": ROWS1,
    "A UpSample phase (0, 1) 256 32x32 B2": ROWS1,
    "A UpSample phase (1, 0) 256 32x32 B2": ROWS1,
    "A UpSample phase (1, 1) 256 32x32 B2": ROWS1,
    "A UpSample 3x3 256 64x64 B2": FAST_3X3,
    "A block1 3x3 gn 256|128->128 64x64 B2": FAST_3X3,
    "A shortcut 1x1 256|128->128 64x64 B2": FAST_1X1,
    "A block1 3x3 gn 128|128->128 64x64 B2": FAST_3X3,
    "A shortcut 1x1 128|128->128 64x64 B2": FAST_1X1,
    "A tail 3x3 gn 128->3 64x64 B2": ROWS1,
    "A head 3x3 3->128 32x32 B80": ROWS1,
    "A block1 3x3 gn 128->128 32x32 B80": FAST_3X3,
    "A block2 3x3 gn dropout 128->128 32x32 B80": FAST_3X3,
    "A attention in-projection 1x1 128->384 32x32 B80": FAST_1X1,
    "A attention out-projection 1x1 128->128 32x32 B80": FAST_1X1,
    "A DownSample 5x5/s2 128 32x32 B80": GENERIC,
    "A block1 3x3 gn 128->256 16x16 B80": GENERIC,
    "A block2 3x3 gn dropout 256->256 16x16 B80": GENERIC,
    "A shortcut 1x1 128->256 16x16 B80": FAST_1X1,
    "A attention in-projection 1x1 256->768 16x16 B80": FAST_1X1,
    "A attention out-projection 1x1 256->256 16x16 B80": FAST_1X1,
    "A block1 3x3 gn 256->256 16x16 B80": GENERIC,
    "A DownSample 5x5/s2 256 16x16 B80": GENERIC,
    "A block1 3x3 gn 256->256 8x8 B80": GENERIC,
    "A block2 3x3 gn dropout 256->256 8x8 B80": GENERIC,
    "A attention in-projection 1x1 256->768 8x8 B80": FAST_1X1,
    "A attention out-projection 1x1 256->256 8x8 B80": FAST_1X1,
    "A DownSample 5x5/s2 256 8x8 B80": GENERIC,
    "A block1 3x3 gn 256->256 4x4 B80": GENERIC,
    "A block2 3x3 gn dropout 256->256 4x4 B80": GENERIC,
    "A attention in-projection 1x1 256->768 4x4 B80": GENERIC,
    "A attention out-projection 1x1 256->256 4x4 B80": GENERIC,
    "A block1 3x3 gn 256|256->256 4x4 B80": GENERIC,
    "A shortcut 1x1 256|256->256 4x4 B80": GENERIC,
    "A UpSample phase (0, 0) 256 4x4 B80": GENERIC,
    "A UpSample phase (0, 1) 256 4x4 B80": GENERIC,
    "A UpSample phase (1, 0) 256 4x4 B80": GENERIC,
    "A UpSample phase (1, 1) 256 4x4 B80": GENERIC,
    "A UpSample 3x3 256 8x8 B80": GENERIC,
    "A block1 3x3 gn 256|256->256 8x8 B80": GENERIC,
    "A shortcut 1x1 256|256->256 8x8 B80": FAST_1X1,
    "A UpSample phase (0, 0) 256 8x8 B80": GENERIC,
    "A UpSample phase (0, 1) 256 8x8 B80": GENERIC,
    "A UpSample phase (1, 0) 256 8x8 B80": GENERIC,
    "A UpSample phase (1, 1) 256 8x8 B80": GENERIC,
    "A UpSample 3x3 256 16x16 B80": GENERIC,
    "A block1 3x3 gn 256|256->256 16x16 B80": GENERIC,
    "A shortcut 1x1 256|256->256 16x16 B80": FAST_1X1,
    "A block1 3x3 gn 256|128->256 16x16 B80": GENERIC,
    "A shortcut 1x1 256|128->256 16x16 B80": FAST_1X1,
    "A UpSample phase (0, 0) 256 16x16 B80": GENERIC,
    "A UpSample phase (0, 1) 256 16x16 B80": GENERIC,
    "A UpSample phase (1, 0) 256 16x16 B80": GENERIC,
    "A UpSample phase (1, 1) 256 16x16 B80": GENERIC,
    "A UpSample 3x3 256 32x32 B80": FAST_3X3,
    "A block1 3x3 gn 256|128->128 32x32 B80": FAST_3X3,
    "A shortcut 1x1 256|128->128 32x32 B80": FAST_1X1,
    "A block1 3x3 gn 128|128->128 32x32 B80": FAST_3X3,
    "A shortcut 1x1 128|128->128 32x32 B80": FAST_1X1,
    "A tail 3x3 gn 128->3 32x32 B80": ROWS1,
    "B head 3x3 6->128 256x256 B2": ROWS1,
    "B block1 3x3 gn 128->128 256x256 B2": FAST_3X3,
    "B block2 3x3 gn dropout 128->128 256x256 B2": FAST_3X3,
    "B DownSample 5x5/s2 128 256x256 B2": ROWS2,
    "B block1 3x3 gn 128->256 128x128 B2": FAST_3X3,
    "B block2 3x3 gn dropout 256->256 128x128 B2": FAST_3X3,
    "B shortcut 1x1 128->256 128x128 B2": FAST_1X1,
    "B block1 3x3 gn 256->256 128x128 B2": FAST_3X3,
    "B DownSample 5x5/s2 256 128x128 B2": ROWS2,
    "B block1 3x3 gn 256->256 64x64 B2": FAST_3X3,
    "B block2 3x3 gn dropout 256->256 64x64 B2": FAST_3X3,
    "B DownSample 5x5/s2 256 64x64 B2": ROWS2,
    "B block1 3x3 gn 256->256 32x32 B2": FAST_3X3,
    "B block2 3x3 gn dropout 256->256 32x32 B2": FAST_3X3,
    "B attention in-projection 1x1 256->768 32x32 B2": FAST_1X1,
    "B attention out-projection 1x1 256->256 32x32 B2": FAST_1X1,
    "B block1 3x3 gn 256|256->256 32x32 B2": FAST_3X3,
    "B shortcut 1x1 256|256->256 32x32 B2": FAST_1X1,
    "B UpSample phase (0, 0) 256 32x32 B2": ROWS1,
    "B UpSample phase (0, 1) 256 32x32 B2": ROWS1,
    "B UpSample phase (1, 0) 256 32x32 B2": ROWS1,
    "B UpSample phase (1, 1) 256 32x32 B2": ROWS1,
    "B UpSample 3x3 256 64x64 B2": FAST_3X3,
    "B block1 3x3 gn 256|256->256 64x64 B2": FAST_3X3,
    "B shortcut 1x1 256|256->256 64x64 B2": FAST_1X1,
    "B UpSample phase (0, 0) 256 64x64 B2": ROWS1,
    "B UpSample phase (0, 1) 256 64x64 B2": ROWS1,
    "B UpSample phase (1, 0) 256 64x64 B2": ROWS1,
    "B UpSample phase (1, 1) 256 64x64 B2": ROWS1,
    "B UpSample 3x3 256 128x128 B2": FAST_3X3,
    "B block1 3x3 gn 256|256->256 128x128 B2": FAST_3X3,
    "B shortcut 1x1 256|256->256 128x128 B2": FAST_1X1,
    "B UpSample phase (0, 0) 256 128x128 B2": ROWS1,
    "B UpSample phase (0, 1) 256 128x128 B2": ROWS1,
    "B UpSample phase (1, 0) 256 128x128 B2": ROWS1,
    "B UpSample phase (1, 1) 256 128x128 B2": ROWS1,
    "B UpSample 3x3 256 256x256 B2": FAST_3X3,
    "B block1 3x3 gn 256|256->128 256x256 B2": FAST_3X3,
    "B shortcut 1x1 256|256->128 256x256 B2": FAST_1X1,
    "B block1 3x3 gn 128|256->128 256x256 B2": FAST_3X3,
    "B shortcut 1x1 128|256->128 256x256 B2": FAST_1X1,
    "B tail 3x3 gn 128->3 256x256 B2": ROWS1,
    "B image encoder 3x3/s2 3->8 256x256 B2": ROWS2,
    "B image encoder 3x3/s2 8->16 128x128 B2": ROWS2,
    "B image encoder 3x3/s2 16->32 64x64 B2": ROWS2,
    "case down-10x40": ROWS2,
    "case down-9x37": ROWS2,
    "case down-8x136": ROWS2,
    "case down-64x64": ROWS2,
    "case tconv-5x20 phase (0, 0)": ROWS1,
    "case tconv-5x20 phase (0, 1)": ROWS1,
    "case tconv-5x20 phase (1, 0)": ROWS1,
    "case tconv-5x20 phase (1, 1)": ROWS1,
    "case tconv-7x33 phase (0, 0)": ROWS1,
    "case tconv-7x33 phase (0, 1)": ROWS1,
    "case tconv-7x33 phase (1, 0)": ROWS1,
    "case tconv-7x33 phase (1, 1)": ROWS1,
    "case tconv-32x32 phase (0, 0)": ROWS1,
    "case tconv-32x32 phase (0, 1)": ROWS1,
    "case tconv-32x32 phase (1, 0)": ROWS1,
    "case tconv-32x32 phase (1, 1)": ROWS1,
    "case enc-3to8-64x64": ROWS2,
    "case enc-8to16-9x70": ROWS2,
    # the "-fast" cases: the routes their shapes were chosen to take (both predicates are unchanged since that commit)
    "case conv3x3-gn-4x64-fast": FAST_3X3,
    "case conv3x3-gn-dropout-4x64-fast": FAST_3X3,
    "case conv1x1-8x16-fast": FAST_1X1,
    "case conv3x3-6x96-fast": FAST_3X3,
}


def workspace_of(d):
    ns, fl = C.c_int(-1), C.c_int64(-1)
    assert hdiff_amd.lib().hdiff_conv2d_wgrad_workspace(C.byref(d), C.byref(ns), C.byref(fl)) == 0
    return ns.value, fl.value


def cdiv(a, b):
    return (a + b - 1) // b


def nsplit_by_route(d, route):
    """The split counts as the kernels' own files state them: at most two full rounds of one workgroup per CU for the fast kernels
    (512 / base), three rounds' worth of the smaller generic workgroups (768 / base), never more splits than pixel tiles."""
    cin = d.C0 + d.C1
    if route == FAST_1X1:
        base, total = (d.Cout // 128) * cdiv(cin, 128), d.B * (d.H * d.W // 64)
        return max(1, min(512 // base, total))
    if route == FAST_3X3:
        base, total = (d.Cout // 128) * (cin // 32), d.B * (d.H // 2) * (d.W // 32)
        return max(1, min(512 // base, total))
    ckw = 32 if d.ntaps == 1 else 4 if d.ntaps > 9 else 16
    tw = 1
    while tw < min(d.VW, 32):
        tw *= 2
    base, total = cdiv(d.Cout, 64) * cdiv(d.CinPad, ckw), d.B * cdiv(d.VW, tw) * cdiv(d.VH, 128 // tw)
    return max(1, min(cdiv(768, base), total))


def test_every_weight_gradient_kind_takes_the_route_it_took():
    assert set(TABLE) == set(EXPECTED) | set(SHORT_PLANES) and not set(EXPECTED) & set(SHORT_PLANES)
    for name, (d, dropout) in TABLE.items():
        want = SHORT_PLANES[name] if name in SHORT_PLANES else EXPECTED[name]
        assert K.route_of(d, dropout) == want, name
    assert {*EXPECTED.values(), *SHORT_PLANES.values()} == set(range(5))
    # every production row is a plane at least as tall as its tile: the VH >= 4 rule moved none of them
    for name, (d, _) in TABLE.items():
        assert (name in SHORT_PLANES) == (d.VW > 16 and d.VH < 4), name
        assert (name in SHORT_PLANES) <= name.startswith("case "), name


def test_the_gpu_cases_name_their_routes():
    """tests/test_gpu_strided_geometry.py asserts these per case on the GPU box; the same answers here, so that a shape that falls
    to another program is red in the CPU suite already."""
    seen = set()
    for cid, kind, shape, route, _ in K.CASES:
        for d, dropout in K.case_descs(kind, shape):
            assert K.route_of(d, dropout) == route, cid
        seen.add(route)
        assert cid.endswith("-short") == (route == GENERIC), cid
        assert cid.endswith("-fast") == (route in (FAST_1X1, FAST_3X3)), cid
    assert seen == {FAST_1X1, FAST_3X3, GENERIC, ROWS1, ROWS2}


def test_the_workspace_query_follows_the_route():
    for name, (d, dropout) in TABLE.items():
        route = K.route_of(d, dropout)
        ns, floats = workspace_of(d)
        assert ns == nsplit_by_route(d, route), (name, route, ns)
        assert floats == ns * d.ntaps * d.CinPad * d.CoutPad, name


def test_the_route_entry_validates_like_the_launching_entries():
    lib = hdiff_amd.lib()
    route = C.c_int(-1)

    def refused(rc, *words):
        msg = lib.hdiff_last_error().decode()
        assert rc == INVALID, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)

    def ask(d, dropout=0):
        return lib.hdiff_conv2d_wgrad_route(C.byref(d), dropout, C.byref(route))

    good = K.plain_desc(3, 128, 128, 2, 64, 64, gn=True)
    refused(lib.hdiff_conv2d_wgrad_route(C.byref(good), 0, None), "conv2d_wgrad_route", "null")
    refused(lib.hdiff_conv2d_wgrad_route(None, 0, C.byref(route)), "null")
    bad = K.plain_desc(3, 128, 128, 2, 64, 64)
    bad.CoutPad = 48
    refused(ask(bad), "conv2d_wgrad:", "padded channel counts")
    bad = K.plain_desc(3, 128, 128, 2, 64, 64)
    bad.in_stride = 3
    refused(ask(bad), "conv2d_wgrad:", "bad geometry")
    bad = K.plain_desc(3, 128, 128, 2, 64, 64, C1=64)
    bad.x1 = None
    refused(ask(bad), "conv2d_wgrad:", "C1 > 0 without x1")
    # the dropout form's own rules
    refused(ask(K.plain_desc(3, 128, 128, 2, 64, 64), 1), "conv2d_wgrad_dropout", "prologue")
    refused(ask(K.plain_desc(3, 64, 128, 2, 64, 64, C1=64, gn=True), 1), "conv2d_wgrad_dropout", "concat")
    refused(ask(K.plain_desc(1, 128, 128, 2, 64, 64, gn=True), 1), "conv2d_wgrad_dropout", "plain 3x3")
    # a generic launch that does not fit: nine taps at stride 2 on a 32-wide tile hold 16 channels x 9 x 65 staged columns
    wide = K.wgrad_desc(hdiff_amd.engine.conv_taps(3, 1), 32, 32, 2, 64, 64, 32, 32, 32, 32, stride=2)
    refused(ask(wide), "conv2d_wgrad:", "does not fit")
    assert route.value == -1                                # a refused call writes nothing
    assert ask(good) == 0 and route.value == FAST_3X3
    assert ask(good, 1) == 0 and route.value == FAST_3X3    # the dropout form of the fast kernel


def test_the_route_entry_is_declared_exported_and_bound():
    lib = hdiff_amd.lib()
    assert lib.hdiff_abi_version() == 6
    header = open(os.path.join(ROOT, "include", "hdiff.h")).read()
    names = re.findall(r"HDIFF_WGRAD_ROUTE_([A-Z0-9_]+) = (\d)", header)
    assert names == [("FAST_1X1", "0"), ("FAST_3X3", "1"), ("GENERIC", "2"), ("GENERIC_ROWS1", "3"), ("GENERIC_ROWS2", "4")]
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    name = "hdiff_conv2d_wgrad_route"
    assert re.search(r"\b%s\s*\(" % name, header)
    assert name in set(re.findall(r" T (hdiff_[a-z0-9_]+)", nm))
    assert name in _capi.EXPORTED_SYMBOLS
    assert getattr(lib, name).restype is C.c_int
