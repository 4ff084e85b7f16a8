"""Host-side pins of the score and loss workspaces (no GPU).  The seven files that share ``csrc/reduce.h`` size their scratch from
``parts_for`` and ``Carver`` (``csrc/common.h``); callers allocate exactly what the queries answer, and the kernels address the
regions by the same layout, so sizes and region order are part of the behaviour.  Every number below was read from commit 346fdb9,
the last one in which each file carried its own part-count function, ``take`` lambda and ``align256``; all calls returned 0."""
import ctypes as C
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hdiff_amd  # noqa: E402
from hdiff_amd import _capi  # noqa: E402

PINNED = {
    "hdiff_quality_workspace": {(1, 7, 7): 100096, (1, 64, 64): 100096, (3, 100, 37): 297216, (8, 256, 256): 807936,
                                (2, 1000, 1000): 271104},
    "hdiff_uciqe_workspace": {(1, 1, 1): 99840, (1, 64, 64): 164864, (3, 100, 37): 473600, (8, 256, 256): 9186048,
                              (2, 1000, 1000): 32217600},
    "hdiff_l1_mean_workspace": {(1,): 256, (2048,): 256, (2049,): 256, (10 ** 6,): 2048, (2 ** 40,): 2048},
    "hdiff_lpips_layer_workspace": {(1, 1, 1, 1): 256, (2, 64, 33, 47): 256, (1, 512, 256, 256): 2048},
    "hdiff_kid_workspace": {(2, 2): 256, (50, 70): 256, (70, 50): 256, (1000, 33): 8704},
    "hdiff_smooth_l1_tap_workspace": {(1, 1): 256, (4, 98688): 1792, (256, 2 ** 20): 131072},
    # one double per workgroup of the loss tail: not a multiple of 256, and it stays that way
    "hdiff_train_b_loss_workspace": {(1,): 8, (256,): 8, (257,): 16, (10 ** 7,): 8192},
}


@pytest.mark.parametrize("query", sorted(PINNED))
def test_workspace_sizes_are_those_of_346fdb9(query):
    lib = hdiff_amd.lib()
    for args, want in PINNED[query].items():
        need = C.c_int64(-1)
        assert getattr(lib, query)(*args, C.byref(need)) == 0, (query, args, lib.hdiff_last_error())
        assert need.value == want, (query, args, need.value, want)


def test_msssim_l1_workspace_sizes_are_those_of_346fdb9():
    """(saved, scratch) bytes of the default msssim_config().  The scratch is max(forward, backward): the backward's coefficient maps
    win at every size but the smallest, where the forward's two regions show -- the L1 planes padded to 256 bytes, then the partial
    sums, whose end is NOT padded."""
    from hdiff_amd.autograd import msssim_config
    lib = hdiff_amd.lib()
    cfg = msssim_config()
    for (B, H, W), want in {(1, 32, 32): (143360, 86016), (2, 100, 37): (1036000, 621600), (1, 1, 1): (140, 264),
                            (1, 2, 3): (840, 504)}.items():
        d = cfg.desc(B, 3, H, W)
        saved, scratch = C.c_int64(-1), C.c_int64(-1)
        assert lib.hdiff_msssim_l1_workspace(C.byref(d), C.byref(saved), C.byref(scratch)) == 0
        assert (saved.value, scratch.value) == want, ((B, H, W), saved.value, scratch.value, want)


def test_select_regions_keep_their_size():
    """The UIQM workspace holds 4 selects of 16 bytes per image and the UCIQE workspace 2 of 24 (csrc/radix_select.h asserts both
    sizes): with N = 17 the select region is 1088 resp. 816 bytes, and either padded size differs from what a struct 8 bytes larger
    or smaller would give."""
    lib = hdiff_amd.lib()
    a, b = C.c_int64(-1), C.c_int64(-1)
    assert lib.hdiff_quality_workspace(17, 64, 64, C.byref(a)) == 0 and lib.hdiff_quality_workspace(16, 64, 64, C.byref(b)) == 0
    assert (a.value, b.value) == (1676544, 1576960)
    assert lib.hdiff_uciqe_workspace(17, 64, 64, C.byref(a)) == 0 and lib.hdiff_uciqe_workspace(16, 64, 64, C.byref(b)) == 0
    assert (a.value, b.value) == (2788352, 2623744)


def test_one_definition_of_each_shared_piece():
    """The reading check of the refactor: csrc/ defines each shared piece once, and no header is included inside a namespace."""
    csrc = _capi.CSRC
    texts = {n: open(os.path.join(csrc, n)).read() for n in sorted(os.listdir(csrc)) if n.endswith((".h", ".hip"))}
    whole = "\n".join(texts.values())
    for pattern in (r"double block_sum_all\(", r"double block_sum_to0\(", r"double sum_partials\(", r"unsigned key_of\(float",
                    r"unsigned long long key_of\(double", r"void select_scan\(", r"int64_t align256\(", r"bool non_finite\(",
                    r"int parts_for\(", r"int check_sizes\("):
        assert len(re.findall(pattern, whole)) == 1, pattern
    assert not os.path.exists(os.path.join(csrc, "quality_common.h"))
    for name, text in texts.items():
        depth = 0
        for line in text.split("\n"):
            code = line.split("//")[0]
            if re.match(r"\s*#\s*include", code):
                assert depth == 0, (name, line)
            depth += code.count("{") - code.count("}")
