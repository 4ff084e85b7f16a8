"""Shared by tests/test_gpu_strided_geometry.py (which runs these shapes) and tests/test_wgrad_route_cpu.py (which pins their
weight-gradient routes without a GPU): the strided / transposed / short-plane cases, each the smallest shape at which the property
named beside it holds, and the weight-gradient descriptors their backward passes launch -- built the way autograd._run_wgrad
builds them, with fake non-null pointers (hdiff_conv2d_wgrad_route dereferences none).  The "-fast" cases put fused_conv's two fast
weight-gradient kernels (conv_wgrad3x3.hip) through the same test; tests/_wgrad_fast_cases.py probes those kernels tile by tile.

Tile facts, from the two launchers (conv_wgrad.hip, conv_igemm.hip): the pixel tile is 2^t columns x 128 / 2^t rows of the
virtual output grid (VH x VW), 2^t = VW rounded up to a power of two, 32 at most -- so VW > 16 means 4 x 32 tiles in the weight
gradient (8 x 32 in the forward once VH * VW >= 1024), the only tiles at which conv_wgrad_kernel<ROWS = in_stride> runs."""
import ctypes as C

from hdiff_amd import _capi
from hdiff_amd import engine as E

P = 0x1000            # a non-null, word-aligned "pointer"
FAST_1X1, FAST_3X3, GENERIC, ROWS1, ROWS2 = range(5)      # HDIFF_WGRAD_ROUTE_* (include/hdiff.h)
B = 2


def wgrad_desc(taps, C0, cout, Bn, H, W, VH, VW, OH, OW, *, C1=0, stride=1, out_map=(1, 0, 1, 0), gn=False):
    """The descriptor of autograd._run_wgrad for these arguments (dy of shape [Bn, cout, OH, OW])."""
    d = _capi.WgradDesc()
    cin = C0 + C1
    d.x0, d.x1, d.C0, d.C1, d.B, d.H, d.W = P, (P if C1 else None), C0, C1, Bn, H, W
    d.gn_scale, d.gn_shift = (P, P) if gn else (None, None)
    d.dy, d.Cout, d.CinPad, d.CoutPad = P, cout, E._pad(cin, 8), E._pad(cout, 64)
    d.OH, d.OW, d.VH, d.VW, d.in_stride = OH, OW, VH, VW, stride
    d.out_sy, d.out_oy, d.out_sx, d.out_ox = out_map
    d.ntaps = len(taps.dy)
    for i in range(d.ntaps):
        d.tap_dy[i], d.tap_dx[i] = taps.dy[i], taps.dx[i]
    return d


def plain_desc(k, C0, cout, Bn, H, W, *, C1=0, gn=False):
    """fused_conv's weight gradient: a k x k / stride-1 / pad k // 2 conv."""
    return wgrad_desc(E.conv_taps(k, k // 2), C0, cout, Bn, H, W, H, W, H, W, C1=C1, gn=gn)


def s2_desc(cin, cout, Bn, H, W):
    """_DownFn's and _StridedConvFn's: the 25-tap stencil at stride 2 (the image encoder's 3x3 is unpacked from its centre)."""
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return wgrad_desc(E.conv_taps(5, 2), cin, cout, Bn, H, W, OH, OW, OH, OW, stride=2)


def phase_descs(cin, cout, Bn, H, W):
    """_TConvFn's: one launch per output parity (py, px), 9 / 6 / 6 / 4 taps under the output map (2, py, 2, px)."""
    return [wgrad_desc(E.tconv_phase_taps(py, px), cin, cout, Bn, H, W, H, W, 2 * H, 2 * W, out_map=(2, py, 2, px))
            for py in (0, 1) for px in (0, 1)]


def route_of(d, dropout=0):
    lib = _capi.lib()
    route = C.c_int(-1)
    rc = lib.hdiff_conv2d_wgrad_route(C.byref(d), dropout, C.byref(route))
    assert rc == 0, lib.hdiff_last_error().decode()
    return route.value


# (id, entry point, (cin, cout, H, W), route of every weight-gradient launch, what the shape reaches).  The short planes
# (virtual output VH < 4 with VW > 16) ran ROWS1 / ROWS2 before hdiff_conv2d_wgrad_route existed: wgrad_route sends them to the
# generic instantiation, which clamps the tile row to the staged patch.
CASES = [
    # _DownFn, 32 channels: 3x3/s2 + 5x5/s2 folded into one 25-tap stride-2 conv
    ("down-10x40", "down", (32, 32, 10, 40), ROWS2,
     "5x20 outputs: one x tile with 20 of 32 columns live, a second tile row with 1 of 4 rows live; forward CK = 4 with split-K; "
     "dgrad phases on 32-wide tiles under a 2x2 output map"),
    ("down-9x37", "down", (32, 32, 9, 37), ROWS2, "odd in both directions: zero-filled dX, phases of 5x19, 5x18, 4x19, 4x18"),
    ("down-8x136", "down", (32, 32, 8, 136), ROWS2, "4x68 outputs: three x tiles, the last with 4 live columns"),
    ("down-64x64", "down", (32, 32, 64, 64), ROWS2,
     "32x32 outputs: forward and the tconv-style dgrad at WN = 2 with 20 staging slots (the limit), 16 weight-gradient tiles"),
    ("down-4x40-short", "down", (32, 32, 4, 40), GENERIC, "2x20 outputs: a plane shorter than the 4-row tile"),
    # _TConvFn, 32 -> 48 channels: four output-parity phases; dgrad = a 5x5/s2 conv over the doubled plane
    ("tconv-5x20", "tconv", (32, 48, 5, 20), ROWS1, "ROWS = 1 under the maps (2, py, 2, px), 9 / 6 / 6 / 4 taps; dgrad over 10x40"),
    ("tconv-7x33", "tconv", (32, 48, 7, 33), ROWS1, "two x tiles, the second with one live column; two tile rows"),
    ("tconv-32x32", "tconv", (32, 48, 32, 32), ROWS1, "WN = 2 phases; dgrad over 64x64 with 20 slots"),
    ("tconv-3x24-short", "tconv", (32, 48, 3, 24), GENERIC, "a plane shorter than the tile"),
    # _StridedConvFn: the image encoder's 3x3/s2 convs
    ("enc-3to8-64x64", "strided", (3, 8, 64, 64), ROWS2,
     "CinPad 8 > Cin 3: a 4-channel chunk with one channel missing and a chunk with none; forward 3x3/s2 at WN = 2"),
    ("enc-8to16-9x70", "strided", (8, 16, 9, 70), ROWS2, "odd height, 35 output columns: two x tiles, 3 live columns in the last"),
    ("enc-3to8-6x40-short", "strided", (3, 8, 6, 40), GENERIC, "3x20 outputs: a plane shorter than the tile"),
    # fused_conv on short planes: the generic kernel where ROWS = 1 ran
    ("conv3x3-gn-3x24-short", "conv3-gn", (32, 64, 3, 24), GENERIC, "GroupNorm + Swish prologue, 3 rows"),
    ("conv1x1-2x20-short", "conv1", (64, 96, 2, 20), GENERIC, "no prologue, 32-channel chunks, 2 rows"),
    ("conv3x3-gn-dropout-3x24-short", "conv3-gn-drop", (32, 64, 3, 24), GENERIC, "the dropout instantiation, 3 rows"),
    # fused_conv on the two fast kernels (conv_wgrad3x3.hip): dy = "edge" then holds the first column of the last 32-wide tile
    ("conv3x3-gn-4x64-fast", "conv3-gn", (32, 128, 4, 64), FAST_3X3, "2x2 tiles of 2x32 behind GroupNorm + Swish: every tile two borders"),
    ("conv3x3-gn-dropout-4x64-fast", "conv3-gn-drop", (32, 128, 4, 64), FAST_3X3, "the same plane in the dropout instantiation"),
    ("conv1x1-8x16-fast", "conv1", (64, 128, 8, 16), FAST_1X1, "two 64-pixel tiles per image, 64 of the 128 staged input columns dead"),
    ("conv3x3-6x96-fast", "conv3", (32, 128, 6, 96), FAST_3X3, "no prologue (the UpSample conv's form), 3x3 tiles: one interior"),
]
CASE_IDS = [c[0] for c in CASES]


def case_descs(kind, shape):
    """-> [(descriptor, dropout flag)] of the weight-gradient launches of one backward pass."""
    cin, cout, H, W = shape
    if kind == "down" or kind == "strided":
        return [(s2_desc(cin, cout, B, H, W), 0)]
    if kind == "tconv":
        return [(d, 0) for d in phase_descs(cin, cout, B, H, W)]
    if kind == "conv1":
        return [(plain_desc(1, cin, cout, B, H, W), 0)]
    if kind == "conv3":
        return [(plain_desc(3, cin, cout, B, H, W), 0)]
    return [(plain_desc(3, cin, cout, B, H, W, gn=True), 1 if kind == "conv3-gn-drop" else 0)]


def virtual_grid(kind, shape):
    """(VH, VW, output rows per virtual row, output columns per virtual column) of the weight-gradient launches."""
    cin, cout, H, W = shape
    if kind in ("down", "strided"):
        return (H - 1) // 2 + 1, (W - 1) // 2 + 1, 1, 1
    if kind == "tconv":
        return H, W, 2, 2
    return H, W, 1, 1

