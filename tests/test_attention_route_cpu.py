"""The attention dispatch without a GPU: hdiff_mha_flash_fwd_route and hdiff_mha_flash_bwd_route answer, for a shape (nothing
launched, no device), which kernels the launching entries run.  The expected values were recorded from the predicate cascade
these functions replaced (the commit before them: the four launch_mha_fwd_* guards behind launch_d's ladder, bwd_geometry,
h2_geometry and mha_bwd_x3_shape_ok, copied into a one-off harness), not from the functions: an attention call that falls from
fp16 pairs to bf16 triples or to the fp32 MFMA passes every tolerance test and only costs time."""
import ctypes as C
import os
import re
import subprocess

import pytest

import hdiff_amd
from hdiff_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
RUNNING_MAX, FAST_F32, X3_TRIPLES, H2_PAIRS, X3P_PAIRS, F16_SINGLE = range(6)
FUSED_F32, BWD_H2_PAIRS = range(2)
NONE, FULL, SHORT = "no workspace", "the workspace", "one byte short"

RM1, RM4 = (RUNNING_MAX, 1, 0), (RUNNING_MAX, 4, 0)
FAST, X3, H2, X3P, F16 = ((r, 4, 1) for r in (FAST_F32, X3_TRIPLES, H2_PAIRS, X3P_PAIRS, F16_SINGLE))
# name: (B, C, heads, L, want_lse, workspace, (route, nq, check) in bf16x3, in f16, in f32)
FWD_TABLE = {
    "d16 L1024 ws no-lse": (2, 128, 8, 1024, 0, FULL, H2, F16, FAST),
    "d16 L1024 ws lse": (2, 128, 8, 1024, 1, FULL, H2, H2, FAST),
    "d32 L1024 ws no-lse": (2, 256, 8, 1024, 0, FULL, X3P, F16, FAST),
    "d32 L1024 ws lse": (2, 256, 8, 1024, 1, FULL, X3P, X3P, FAST),
    "d16 L1024, no ws": (2, 128, 8, 1024, 0, NONE, X3, X3, FAST),
    "d32 L1024, no ws": (2, 256, 8, 1024, 0, NONE, X3, X3, FAST),
    "d16 L1024, ws one byte short": (2, 128, 8, 1024, 0, SHORT, X3, X3, FAST),
    "d16 L576 ws (need = 0)": (2, 128, 8, 576, 0, FULL, X3, X3, FAST),
    "d32 L576": (2, 256, 8, 576, 0, NONE, X3, X3, FAST),
    "d24 L1024": (2, 192, 8, 1024, 0, NONE, FAST, FAST, FAST),
    "d8 L1024": (2, 64, 8, 1024, 0, NONE, FAST, FAST, FAST),
    "d16 L448": (2, 128, 8, 448, 0, NONE, RM1, RM1, RM1),
    "d16 L520": (2, 128, 8, 520, 0, NONE, RM4, RM4, RM4),
    "d32 L1000": (2, 256, 8, 1000, 0, NONE, RM4, RM4, RM4),
    "d48 L1024": (2, 384, 8, 1024, 0, NONE, RM1, RM1, RM1),
    "d64 L4096": (2, 512, 8, 4096, 0, NONE, RM1, RM1, RM1),
    "one head C 32, L1024, ws, no-lse": (2, 32, 1, 1024, 0, FULL, X3P, F16, FAST),
    "one head C 64, L1024": (2, 64, 1, 1024, 0, NONE, RM1, RM1, RM1),
}

# Heads 8, C = 8 d.  name: (d, B, L, (route, nk, aligned, nsplit) in the split modes, in f32, workspace floats of the two).
# nsplit and the floats of H2_PAIRS were recorded with HDIFF_BWD_SLAB_GIB unset.
BWD_TABLE = {
    "d16 B1 L1024": (16, 1, 1024, (FUSED_F32, 1, 1, 16), (FUSED_F32, 1, 1, 16), 2097152, 2097152),
    "d16 B4 L1024": (16, 4, 1024, (BWD_H2_PAIRS, 0, 1, 4), (FUSED_F32, 1, 1, 16), 6553736, 8388608),
    "d32 B4 L1024": (32, 4, 1024, (BWD_H2_PAIRS, 0, 1, 4), (FUSED_F32, 1, 1, 16), 13107336, 16777216),
    "d16 B3 L1024 (192 blocks < 256)": (16, 3, 1024, (FUSED_F32, 1, 1, 16), (FUSED_F32, 1, 1, 16), 6291456, 6291456),
    "d16 B2 L1000": (16, 2, 1000, (FUSED_F32, 1, 0, 16), (FUSED_F32, 1, 0, 16), 4096000, 4096000),
    "d8 B1 L8192": (8, 1, 8192, (FUSED_F32, 4, 1, 32), (FUSED_F32, 4, 1, 32), 16777216, 16777216),
    "d16 B1 L8192": (16, 1, 8192, (BWD_H2_PAIRS, 0, 1, 32), (FUSED_F32, 4, 1, 32), 42467368, 33554432),
    "d24 B1 L8192": (24, 1, 8192, (FUSED_F32, 2, 1, 64), (FUSED_F32, 2, 1, 64), 100663296, 100663296),
    "d32 B1 L8192": (32, 1, 8192, (BWD_H2_PAIRS, 0, 1, 32), (FUSED_F32, 2, 1, 64), 84934696, 134217728),
    "d48 B1 L8192": (48, 1, 8192, (FUSED_F32, 1, 1, 128), (FUSED_F32, 1, 1, 128), 402653184, 402653184),
    "d16 B1 L8256": (16, 1, 8256, (FUSED_F32, 1, 1, 65), (FUSED_F32, 1, 1, 65), 68689920, 68689920),
    "d16 B16 L4096": (16, 16, 4096, (BWD_H2_PAIRS, 0, 1, 16), (FUSED_F32, 1, 1, 8), 205521416, 67108864),
    "d32 B1 L4096": (32, 1, 4096, (BWD_H2_PAIRS, 0, 1, 16), (FUSED_F32, 1, 1, 64), 25690152, 67108864),
}
SLAB_CAP_SET = "HDIFF_BWD_SLAB_GIB" in os.environ      # it moves nsplit of H2_PAIRS (and its floats): those columns are not compared


def fwd_need(B, Cc, heads, L):
    need = C.c_int64(-1)
    assert hdiff_amd.lib().hdiff_mha_flash_fwd_workspace(B, Cc, heads, L, C.byref(need)) == 0
    return need.value


def fwd_route(B, Cc, heads, L, lse, ws_bytes):
    out = [C.c_int(-1) for _ in range(3)]
    rc = hdiff_amd.lib().hdiff_mha_flash_fwd_route(B, Cc, heads, L, lse, ws_bytes, *(C.byref(v) for v in out))
    assert rc == 0, hdiff_amd.lib().hdiff_last_error().decode()
    return tuple(v.value for v in out)


def bwd_route(B, Cc, heads, L):
    out = [C.c_int(-1) for _ in range(4)]
    rc = hdiff_amd.lib().hdiff_mha_flash_bwd_route(B, Cc, heads, L, *(C.byref(v) for v in out))
    assert rc == 0, hdiff_amd.lib().hdiff_last_error().decode()
    return tuple(v.value for v in out)


@pytest.fixture
def mode(request):
    before = hdiff_amd.get_contraction_mode()
    hdiff_amd.set_contraction_mode(request.param)
    yield request.param
    hdiff_amd.set_contraction_mode(before)


@pytest.mark.parametrize("mode", ["bf16x3", "f16", "f32"], indirect=True)
def test_every_forward_shape_takes_the_route_it_took(mode):
    for name, (B, Cc, heads, L, lse, ws, bf16x3, f16, f32) in FWD_TABLE.items():
        need = fwd_need(B, Cc, heads, L)
        assert (need == 0) == ("need = 0" in name) or ws == NONE, name
        ws_bytes = {NONE: 0, FULL: need, SHORT: need - 1}[ws]
        want = {"bf16x3": bf16x3, "f16": f16, "f32": f32}[mode]
        assert fwd_route(B, Cc, heads, L, lse, ws_bytes) == want, (name, mode)
        if mode == "f32":      # no split-operand route, whatever the workspace
            assert want[0] in (RUNNING_MAX, FAST_F32), name
    seen = {a[0] for row in FWD_TABLE.values() for a in row[6:]}
    assert seen == set(range(6))
    assert {a[1:] for row in FWD_TABLE.values() for a in row[6:] if a[0] != RUNNING_MAX} == {(4, 1)}


def test_the_forward_workspace_is_nonzero_exactly_where_it_changes_a_route():
    """hdiff_mha_flash_fwd_workspace and the route function read the same sizing function: a shape has a size iff handing
    that many bytes over changes the route in some mode."""
    before = hdiff_amd.get_contraction_mode()
    try:
        for name, (B, Cc, heads, L, _, _, _, _, _) in FWD_TABLE.items():
            need = fwd_need(B, Cc, heads, L)
            changes = False
            for m in ("bf16x3", "f16", "f32"):
                hdiff_amd.set_contraction_mode(m)
                for lse in (0, 1):
                    with_ws = fwd_route(B, Cc, heads, L, lse, need if need else 1 << 40)
                    changes |= with_ws != fwd_route(B, Cc, heads, L, lse, 0)
                    if need:      # the threshold is the size itself
                        assert fwd_route(B, Cc, heads, L, lse, need - 1) == fwd_route(B, Cc, heads, L, lse, 0), name
                        assert fwd_route(B, Cc, heads, L, lse, need + 1) == with_ws, name
            assert changes == (need != 0), name
    finally:
        hdiff_amd.set_contraction_mode(before)


@pytest.mark.parametrize("mode", ["bf16x3", "f16", "f32"], indirect=True)
def test_every_backward_shape_takes_the_route_it_took(mode):
    cols = slice(0, 3) if SLAB_CAP_SET else slice(0, 4)
    for name, (d, B, L, split, f32, _, _) in BWD_TABLE.items():
        want = f32 if mode == "f32" else split
        assert bwd_route(B, 8 * d, 8, L)[cols] == want[cols], (name, mode)
        if mode == "f32":
            assert want[0] == FUSED_F32, name
    assert {row[3][0] for row in BWD_TABLE.values()} == {FUSED_F32, BWD_H2_PAIRS}
    assert {row[4][1] for row in BWD_TABLE.values()} == {1, 2, 4}


@pytest.mark.parametrize("mode", ["bf16x3", "f32"], indirect=True)
def test_the_backward_workspace_is_the_larger_need_in_every_mode(mode):
    for name, (d, B, L, split, _, floats_split, floats_f32) in BWD_TABLE.items():
        if SLAB_CAP_SET and split[0] == BWD_H2_PAIRS:
            continue
        need = C.c_int64(-1)
        assert hdiff_amd.lib().hdiff_mha_flash_bwd_workspace(B, 8 * d, 8, L, C.byref(need)) == 0, name
        assert need.value == max(floats_split, floats_f32), (name, mode)


def test_the_route_entries_validate_like_the_launching_entries():
    lib = hdiff_amd.lib()
    f = [C.c_int(-1) for _ in range(3)]
    b = [C.c_int(-1) for _ in range(4)]
    fo, bo = [C.byref(v) for v in f], [C.byref(v) for v in b]

    def refused(rc, *words):
        msg = lib.hdiff_last_error().decode()
        assert rc == INVALID, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)

    refused(lib.hdiff_mha_flash_fwd_route(2, 40, 8, 1024, 0, 0, *fo), "mha_flash_fwd:", "head dim 5")
    refused(lib.hdiff_mha_flash_fwd_route(2, 130, 8, 1024, 0, 0, *fo), "mha_flash_fwd:", "bad sizes")
    refused(lib.hdiff_mha_flash_fwd_route(0, 128, 8, 1024, 0, 0, *fo), "mha_flash_fwd:", "bad sizes")
    refused(lib.hdiff_mha_flash_fwd_route(2, 128, 8, 1024, 0, -1, *fo), "mha_flash_fwd_ws:", "size")
    for i in range(3):
        refused(lib.hdiff_mha_flash_fwd_route(2, 128, 8, 1024, 0, 0, *(None if j == i else p for j, p in enumerate(fo))),
                "mha_flash_fwd_route", "null")
    refused(lib.hdiff_mha_flash_bwd_route(2, 40, 8, 1024, *bo), "mha_flash_bwd:", "head dim 5")
    refused(lib.hdiff_mha_flash_bwd_route(2, 130, 8, 1024, *bo), "mha_flash_bwd:", "bad sizes")
    refused(lib.hdiff_mha_flash_bwd_route(65536, 128, 8, 64, *bo), "mha_flash_bwd:", "grid limits")
    refused(lib.hdiff_mha_flash_bwd_route(1, 16 * 65536, 65536, 64, *bo), "mha_flash_bwd:", "grid limits")
    for i in range(4):
        refused(lib.hdiff_mha_flash_bwd_route(2, 128, 8, 1024, *(None if j == i else p for j, p in enumerate(bo))),
                "mha_flash_bwd_route", "null")
    assert [v.value for v in f + b] == [-1] * 7              # a refused call writes nothing


def test_the_route_entries_are_declared_exported_and_bound():
    lib = hdiff_amd.lib()
    assert lib.hdiff_abi_version() == 6
    header = open(os.path.join(ROOT, "include", "hdiff.h")).read()
    assert re.findall(r"HDIFF_MHA_FWD_ROUTE_([A-Z0-9_]+) = (\d)", header) == [
        ("RUNNING_MAX", "0"), ("FAST_F32", "1"), ("X3_TRIPLES", "2"), ("H2_PAIRS", "3"), ("X3P_PAIRS", "4"), ("F16_SINGLE", "5")]
    assert re.findall(r"HDIFF_MHA_BWD_ROUTE_([A-Z0-9_]+) = (\d)", header) == [("FUSED_F32", "0"), ("H2_PAIRS", "1")]
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (hdiff_[a-z0-9_]+)", nm))
    for name in ("hdiff_mha_flash_fwd_route", "hdiff_mha_flash_bwd_route"):
        assert re.search(r"\b%s\s*\(" % name, header)
        assert name in exported
        assert name in _capi.EXPORTED_SYMBOLS
        assert getattr(lib, name).restype is C.c_int
