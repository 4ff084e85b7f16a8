"""What the tap-column form of conv3x3_x3.hip asks of the dispatcher, pinned without a GPU beside tests/test_conv_route_cpu.py (whose
descriptors and helpers these are):

* the kernel walks a tap RECTANGLE (3x3, 3x2, 2x3, 2x2): distinct taps of the 3x3 neighbourhood that do not fill the rectangle they
  span keep the fp32 kernel, whatever packs the descriptor offers;
* its patch loads address the 16 channel planes of a chunk by a scalar base and one 32-bit byte offset per lane.  That needs
  16 planes x 4 bytes below 2^32; the forward entries refuse planes of 2^25 pixels and more outright, which is pinned here.

Each refused descriptor stands beside its accepted neighbour, so a test that passes only because nothing reaches the kernel fails."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import hdiff_amd
from hdiff_amd.engine import tconv_phase_taps

from test_conv_route_cpu import GN, IGEMM, P, PAIRS, T3, WORDS, X3_PAIRS_GN, X3_PAIRS_WORD, X3_TRIPLES, conv_desc, rng, route_of


@pytest.fixture
def mode(request):
    before = hdiff_amd.get_contraction_mode()
    hdiff_amd.set_contraction_mode(request.param)
    yield request.param
    hdiff_amd.set_contraction_mode(before)


def _phase_desc(taps, **over):
    return conv_desc(taps, 256, 256, 12, 32, 32, out_map=(2, 1, 2, 0), bias=P, wp_x3=P, **over)


def _ragged():
    """the six taps of phase (1, 0), a 2x3 or 3x2 rectangle, with one corner moved to a free cell of the 3x3 neighbourhood: still six
    distinct taps in [-1, 1]^2, spanning 3x3 and filling six of its nine cells"""
    t = tconv_phase_taps(1, 0)
    cells = {(t.dy[i], t.dx[i]) for i in range(6)}
    assert len(cells) == 6
    free = sorted((y, x) for y in (-1, 0, 1) for x in (-1, 0, 1) if (y, x) not in cells)
    t.dy[0], t.dx[0] = free[0]
    return t


@pytest.mark.parametrize("mode", ["bf16x3", "f32"], indirect=True)
def test_a_ragged_tap_list_keeps_the_fp32_kernel(mode):
    split = mode != "f32"
    full, ragged = tconv_phase_taps(1, 0), _ragged()
    # by range word, and on triples
    assert route_of(_phase_desc(full), rng(wp_h2_taps=P, **WORDS), 0)[0] == (X3_PAIRS_WORD if split else IGEMM)
    assert route_of(_phase_desc(ragged), rng(wp_h2_taps=P, **WORDS), 0) == (IGEMM, 1 if split else 0)
    assert route_of(_phase_desc(full), None, 0)[0] == (X3_TRIPLES if split else IGEMM)
    assert route_of(_phase_desc(ragged), None, 0) == (IGEMM, 0)


def test_no_plane_of_2_to_the_25_pixels_reaches_any_route():
    """The kernel's 32-bit lane offsets cover 16 channel planes because the forward entries refuse planes of 2^25 pixels and more for
    every route: the route function, which validates like them, answers the largest plane below and refuses the first one at it."""
    W = 8192
    lib = hdiff_amd.lib()
    below = conv_desc(T3, 16, 64, 1, W // 2 - 1, W, bias=P, **GN, **PAIRS)         # 2^25 - 8192 pixels
    assert route_of(below, None, 0)[0] in (X3_PAIRS_GN, IGEMM)
    at = conv_desc(T3, 16, 64, 1, W // 2, W, bias=P, **GN, **PAIRS)
    route, tail = C.c_int(-1), C.c_int(-1)
    assert lib.hdiff_conv2d_fwd_route(at, None, 0, C.byref(route), C.byref(tail)) != 0
    assert "2^25" in lib.hdiff_last_error().decode()
    assert (route.value, tail.value) == (-1, -1)
