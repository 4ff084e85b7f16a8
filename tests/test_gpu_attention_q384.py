"""The d_head 16 fp16-pair attention forward with 384 queries per workgroup (csrc/attention_h2.hip, NQ = 6;
HDIFF_MHA_FWD_ROUTE_H2_PAIRS_Q384) against the 256-query form of the same kernel (HDIFF_MHA_FWD_ROUTE_H2_PAIRS).

Every query's arithmetic is its own: the key order, the accumulation chains and the moves of the softmax reference do not depend on
which workgroup or which of a wave's query tiles holds the query.  So the two forms must agree BIT FOR BIT in `out` and `lse2`,
also where the out-of-line reference move fires, and the 384 form's last workgroup -- L is a multiple of 256, not of 384 -- must
neither read nor write past L.  Both forms are run on a named route (hdiff_mha_flash_fwd_ws_as); the cost model that picks one for a
shape is tests/test_attention_q384_route_cpu.py's subject."""
import ctypes as C
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import hdiff_amd  # noqa: E402
from hdiff_amd import _capi  # noqa: E402
from test_gpu_ops import attention_core_ref  # noqa: E402

DEV = "cuda:0"
H2_PAIRS, H2_PAIRS_Q384 = 3, 6          # HDIFF_MHA_FWD_ROUTE_* (include/hdiff.h)
POISON = 0x7FC0DEAD                     # a quiet NaN no kernel produces
MARGIN = 4096                           # poisoned floats in front of and behind each output
# 768: two full 384-query workgroups; 1024: the last one holds 4 of its 6 query tiles per wave-quartet (256 of 384 queries);
# 512: the second one holds 128 of 384; 2560: six full ones and 256 of the seventh
LENGTHS = [768, 1024, 512, 2560]
INPUTS = ["gauss", "peaked", "late-spikes", "wide-v"]


@pytest.fixture
def pairs_mode():
    before = hdiff_amd.get_contraction_mode()
    hdiff_amd.set_contraction_mode("bf16x3")
    yield _capi.lib()
    hdiff_amd.set_contraction_mode(before)


def _inputs(name, B, Cc, L, seed):
    """tests/test_gpu_ops.py::_h2_case's recipes at this file's sizes: "peaked" -- scores with a standard deviation of 13 in the exp2
    domain, the reference moves in most stages of every workgroup, ragged ones and query tiles 4 and 5 included; "late-spikes" -- keys
    far above everything before them in the middle and at the end; "wide-v" -- V channel rows 2^30 apart."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, 3 * Cc, L, generator=g)
    if name == "peaked":
        qkv *= 3.0
    elif name == "late-spikes":
        qkv[:, Cc:2 * Cc, L // 2 + 5] *= 25.0
        qkv[:, Cc:2 * Cc, L - 3] *= 40.0
    elif name == "wide-v":
        qkv[:, 2 * Cc:] *= torch.exp2(torch.linspace(-15.0, 15.0, Cc))[None, :, None]
    return qkv


def _guarded(n):
    """n floats with MARGIN poisoned floats on either side (and poisoned themselves): (whole buffer as int32, the n floats)"""
    raw = torch.full((n + 2 * MARGIN,), POISON, dtype=torch.int32, device=DEV)
    return raw, raw.view(torch.float32)[MARGIN:MARGIN + n]


def _run(lib, d_qkv, heads, route):
    """the call on a named route: (out, lse2) after checking that the margins still hold the poison and the outputs none of it"""
    B, C3, L = d_qkv.shape
    Cc = C3 // 3
    need = C.c_int64(-1)
    _capi.check(lib.hdiff_mha_flash_fwd_workspace(B, Cc, heads, L, C.byref(need)), "mha ws query")
    assert need.value > 0
    ws = torch.empty(need.value // 4 + 1, device=DEV)
    o_raw, o = _guarded(B * Cc * L)
    l_raw, lse = _guarded(B * heads * L)
    _capi.check(lib.hdiff_mha_flash_fwd_ws_as(d_qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), B, Cc, heads, L, ws.data_ptr(), need.value,
                                              route, torch.cuda.current_stream().cuda_stream), "mha on a named route")
    torch.cuda.synchronize()
    for raw, n, what in ((o_raw, o.numel(), "out"), (l_raw, lse.numel(), "lse2")):
        assert bool((raw[:MARGIN] == POISON).all()) and bool((raw[MARGIN + n:] == POISON).all()), f"{what}: a write outside the tensor (route {route})"
        assert not bool((raw[MARGIN:MARGIN + n] == POISON).any()), f"{what}: an element was not written (route {route})"
    return o.view(B, Cc, L), lse.view(B, heads, L)


@pytest.mark.parametrize("name", INPUTS)
@pytest.mark.parametrize("L", LENGTHS)
def test_384_queries_per_workgroup_gives_the_bits_of_256(L, name, pairs_mode):
    lib = pairs_mode
    B, Cc, heads = 2, 32, 2
    d_qkv = _inputs(name, B, Cc, L, seed=1000 + L + INPUTS.index(name)).to(DEV)
    o4, l4 = _run(lib, d_qkv, heads, H2_PAIRS)
    o6, l6 = _run(lib, d_qkv, heads, H2_PAIRS_Q384)
    assert torch.isfinite(o4).all() and torch.isfinite(l4).all() and torch.isfinite(o6).all() and torch.isfinite(l6).all()
    diff_o = (o4.view(torch.int32) != o6.view(torch.int32))
    diff_l = (l4.view(torch.int32) != l6.view(torch.int32))
    where = lambda m: sorted({int(q) for q in m.nonzero()[:, -1].tolist()})[:8]
    assert not bool(diff_o.any()), (int(diff_o.sum()), "first queries", where(diff_o))
    assert not bool(diff_l.any()), (int(diff_l.sum()), "first queries", where(diff_l))


def test_384_route_error_against_float64_is_fp32_class(pairs_mode):
    """The suite's gate for the split-operand attention kernels (tests/test_gpu_ops.py): error against float64 <= 1.25x rms / 2x worst of
    the fp32-MFMA kernel's on the same inputs -- on the new route at a ragged length (1024 = 2 x 384 + 256), heads = 8, batch 2."""
    lib = pairs_mode
    d, L, B, heads = 16, 1024, 2, 8
    qkv = torch.randn(B, 3 * heads * d, L, generator=torch.Generator().manual_seed(100 + d + L))
    ref = attention_core_ref(qkv, heads).double()
    d_qkv = qkv.to(DEV)
    o6, _ = _run(lib, d_qkv, heads, H2_PAIRS_Q384)
    hdiff_amd.set_contraction_mode("f32")
    o_f32 = torch.empty(B, heads * d, L, device=DEV)
    _capi.check(lib.hdiff_mha_flash_fwd(d_qkv.data_ptr(), o_f32.data_ptr(), None, B, heads * d, heads, L, torch.cuda.current_stream().cuda_stream), "mha f32")
    torch.cuda.synchronize()
    rms = lambda t: (t.double().cpu() - ref).pow(2).mean().sqrt().item()
    worst = lambda t: (t.double().cpu() - ref).abs().max().item()
    print(f"q384 L={L}: rms {rms(o6):.3e} (fp32-MFMA kernel {rms(o_f32):.3e}), worst {worst(o6):.3e} ({worst(o_f32):.3e})")
    assert not torch.equal(o6, o_f32), "the fp16-pair kernel did not run"
    assert rms(o6) <= 1.25 * rms(o_f32) + 1e-12, (rms(o6), rms(o_f32))
    assert worst(o6) <= 2.0 * worst(o_f32) + 1e-12, (worst(o6), worst(o_f32))
