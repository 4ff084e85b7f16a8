"""Which of its two forms the d_head 16 fp16-pair attention forward runs in, without a GPU: hdiff_mha_flash_fwd_route answers
HDIFF_MHA_FWD_ROUTE_H2_PAIRS (256 queries per workgroup) or _H2_PAIRS_Q384 (384) by a cost model written out here a second time:
cost = rounds x queries per workgroup, rounds = ceil(pairs ceil(L / QB) / (2 x 256 CUs)), the 384 form's cost times G, its measured
time per query against the 256 form's (profiles/attention_fwd_q384.txt); the 384 form only where it is cheaper."""
import ctypes as C

import pytest

import hdiff_amd

RUNNING_MAX, FAST_F32, X3_TRIPLES, H2_PAIRS, X3P_PAIRS, F16_SINGLE, H2_PAIRS_Q384 = range(7)
G = 0.963
CUS = 256


def model(B, heads, L):
    pairs, slots = B * heads, 2 * CUS
    rounds = lambda qb: -(-(pairs * -(-L // qb)) // slots)
    return H2_PAIRS_Q384 if G * rounds(384) * 384 < rounds(256) * 256 else H2_PAIRS


def need(B, Cc, heads, L):
    n = C.c_int64(-1)
    assert hdiff_amd.lib().hdiff_mha_flash_fwd_workspace(B, Cc, heads, L, C.byref(n)) == 0
    return n.value


def route(B, Cc, heads, L, lse, ws_bytes):
    out = [C.c_int(-1) for _ in range(3)]
    rc = hdiff_amd.lib().hdiff_mha_flash_fwd_route(B, Cc, heads, L, lse, ws_bytes, *(C.byref(v) for v in out))
    assert rc == 0, hdiff_amd.lib().hdiff_last_error().decode()
    return tuple(v.value for v in out)


@pytest.fixture
def mode(request):
    before = hdiff_amd.get_contraction_mode()
    hdiff_amd.set_contraction_mode(request.param)
    yield request.param
    hdiff_amd.set_contraction_mode(before)


@pytest.mark.parametrize("mode", ["bf16x3", "f16", "f32"], indirect=True)
def test_the_benchmark_launch_takes_the_384_form(mode):
    """bench.py's d_head 16 attention: 2 x 8 samples, C 128, heads 8, L 65536 -- 43 rounds of 384 against 64 of 256"""
    B, Cc, heads, L = 16, 128, 8, 65536
    assert model(B, heads, L) == H2_PAIRS_Q384
    n = need(B, Cc, heads, L)
    want = {"bf16x3": (H2_PAIRS_Q384, 4, 1), "f16": (F16_SINGLE, 4, 1), "f32": (FAST_F32, 4, 1)}[mode]
    assert route(B, Cc, heads, L, 0, n) == want
    if mode == "f16":      # with a log-sum-exp the f16 mode runs the pair kernel
        assert route(B, Cc, heads, L, 1, n) == (H2_PAIRS_Q384, 4, 1)


def test_the_route_follows_the_cost_model_and_needs_the_workspace():
    before = hdiff_amd.get_contraction_mode()
    hdiff_amd.set_contraction_mode("bf16x3")
    try:
        seen = set()
        for B in (1, 2, 3, 8, 16, 32):
            for L in (512, 768, 1024, 2560, 4096, 16384, 36864, 65536):
                for lse in (0, 1):
                    n = need(B, 128, 8, L)
                    assert n > 0
                    want = model(B, 8, L)
                    assert route(B, 128, 8, L, lse, n) == (want, 4, 1), (B, L, lse)
                    # no workspace, or one byte short: the kernel that splits in its loop, never the 384 form
                    assert route(B, 128, 8, L, lse, 0) == (X3_TRIPLES, 4, 1), (B, L)
                    assert route(B, 128, 8, L, lse, n - 1) == (X3_TRIPLES, 4, 1), (B, L)
                    seen.add(want)
        assert seen == {H2_PAIRS, H2_PAIRS_Q384}
        # one round of either form: 256 queries cost less than 384 G (a tie in rounds never goes to 384)
        assert model(2, 8, 1024) == H2_PAIRS and model(1, 8, 4096) == H2_PAIRS
        # 4 rounds of 256 against 3 of 384: 1024 < 1152 G
        assert model(16, 8, 4096) == H2_PAIRS
        # d_head 32 has one form
        assert route(2, 256, 8, 1024, 0, need(2, 256, 8, 1024)) == (X3P_PAIRS, 4, 1)
    finally:
        hdiff_amd.set_contraction_mode(before)


def test_a_named_route_is_refused_unless_it_is_a_form_of_the_calls_own():
    """hdiff_mha_flash_fwd_ws_as validates before it launches: fake pointers, no device"""
    lib = hdiff_amd.lib()
    P = 0x1000
    before = hdiff_amd.get_contraction_mode()
    try:
        hdiff_amd.set_contraction_mode("bf16x3")

        def refused(rc, *words):
            msg = lib.hdiff_last_error().decode()
            assert rc == -1, (rc, msg)
            for w in words:
                assert w in msg, (w, msg)

        # d_head 32 runs X3P_PAIRS: neither pair form of d_head 16 is a form of it
        n32 = need(2, 256, 8, 1024)
        refused(lib.hdiff_mha_flash_fwd_ws_as(P, P, None, 2, 256, 8, 1024, P, n32, H2_PAIRS_Q384, None), "mha_flash_fwd_ws_as", "route 6")
        # no workspace: the call's route is X3_TRIPLES
        refused(lib.hdiff_mha_flash_fwd_ws_as(P, P, None, 2, 128, 8, 1024, None, 0, H2_PAIRS_Q384, None), "mha_flash_fwd_ws_as", "route 6")
        n16 = need(2, 128, 8, 1024)
        refused(lib.hdiff_mha_flash_fwd_ws_as(P, P, None, 2, 128, 8, 1024, P, n16, X3_TRIPLES, None), "mha_flash_fwd_ws_as", "route 2")
        refused(lib.hdiff_mha_flash_fwd_ws_as(P, P, None, 2, 128, 8, 1024, P, n16, -1, None), "mha_flash_fwd_ws_as")
        refused(lib.hdiff_mha_flash_fwd_ws_as(P, P, None, 2, 128, 8, 1024, None, n16, H2_PAIRS, None), "workspace")
        hdiff_amd.set_contraction_mode("f32")      # the fp32 mode has no pair route to name
        refused(lib.hdiff_mha_flash_fwd_ws_as(P, P, None, 2, 128, 8, 1024, P, n16, H2_PAIRS_Q384, None), "mha_flash_fwd_ws_as", "route 6")
    finally:
        hdiff_amd.set_contraction_mode(before)
