"""Shared by tests/test_attn_f32_cases_cpu.py, tests/test_gpu_attention_f32.py and tools/attn_f32_error_ratio.py: the fp32-input
attention kernels (mha_flash_fwd_kernel, mha_flash_fwd_fast_kernel in csrc/attention.hip, mha_bwd_fused_kernel in
csrc/attention_bwd.hip) are the yardstick of every split-operand attention test; this is what they are themselves held to.
  * CASES: the smallest shapes that launch every instantiation as the MAIN kernel, with the route each call must take,
  * input families beyond randn (those of _attn_bwd_cases plus all-negative, late-spike, one-hot-dO); every (sample, head) pair
    of a batch is a copy of one of three base pairs, so the float64 reference is three pairs per case,
  * definition(): the textbook formulas of one pair, in float64 (ref64) and in torch float32 on the CPU (yard32), with defect
    models for the CPU test,
  * gate(): O, lse2, dQ, dK, dV each against its own magnitude, max and rms error <= max(margin x the fp32 CPU definition's same
    statistic, one fp32 ulp of max|ref|).
Importable without a GPU; run_f32() alone touches one."""
import ctypes as C
import functools
import math
from collections import namedtuple

import torch

import _attn_bwd_cases as K

DEV = "cuda:0"
YARD = 4.0                # the project's margin over an fp32 CPU definition (tests/test_gpu_dino.py, tests/test_gpu_perceptual.py)
ROOM = 1.5                # over a measured worst ratio: seed-to-seed (and BLAS-to-BLAS) variation of a ratio of two maxima
# The kernels' worst measured ratio to the fp32 CPU definition on the MI355X, the larger of the max and the rms error's, over every
# run of RUNS (profiles/attention_f32_error_ratio.txt, tools/attn_f32_error_ratio.py).  The kernels are honest above YARD in several
# cells: every error is <= 3e-4 (all-negative dQ), else <= 2e-5 of the tensor's magnitude, and an emulation of their summation
# order in torch fp32 shows the same cells.  What carries it (see the profile): the backward recomputes P = exp2(s2 - lse2) from an
# fp32 lse2 with the scores accumulated on top of -lse2, while torch's softmax is exact where one score dominates (late-spike dV,
# peaked dV: |s2| ~ 200, one ulp there is 1.5e-5) and uses the SAME P in O and in dS, so that rowsum(dS) vanishes to 1e-7 where the
# kernel's is the forward's O error against a recomputed P -- which K's common component multiplies (all-negative dQ: -3u is 15 x
# the part of K that the true dQ is made of); one-hot-dO has a single query row, nothing averages.  A cell's margin is
# max(YARD, ROOM x its measured worst ratio); the yardstick stays the fp32 CPU definition.
MEASURED = {
    "plain": {"O": 4.13, "lse2": 3.13, "dQ": 6.07, "dK": 7.17, "dV": 6.13},
    "peaked": {"O": 1.62, "lse2": 1.40, "dQ": 4.83, "dK": 4.36, "dV": 9.35},
    "wide-V": {"O": 6.21, "lse2": 1.60, "dQ": 4.07, "dK": 3.91, "dV": 3.16},
    "loud-dO-pixel": {"O": 1.66, "lse2": 1.11, "dQ": 4.72, "dK": 4.94, "dV": 3.85},
    "tiny-dO": {"O": 2.58, "lse2": 1.52, "dQ": 2.92, "dK": 3.61, "dV": 5.64},
    "zero-dO-head": {"O": 2.91, "lse2": 1.87, "dQ": 3.48, "dK": 2.69, "dV": 4.34},
    "all-negative": {"O": 2.88, "lse2": 1.13, "dQ": 24.11, "dK": 1.69, "dV": 1.75},
    "late-spike": {"O": 2.67, "lse2": 2.42, "dQ": 3.35, "dK": 2.47, "dV": 69.34},
    "one-hot-dO": {"O": 6.17, "lse2": 1.19, "dQ": 7.15, "dK": 24.48, "dV": 15.53},
}


def margin_of(family, name):
    return max(YARD, ROOM * MEASURED[family][name])


LOG2E = 1.4426950408889634
TENSORS = ("O", "lse2", "dQ", "dK", "dV")
RUNNING_MAX, FAST_F32 = 0, 1                       # HDIFF_MHA_FWD_ROUTE_*
ALL_D = (4, 8, 12, 16, 24, 32, 48, 64)
CANARY = 256                                        # floats in front of and behind every output
CANARY_BITS = 0x5EEDC0DE                            # as a float: 3.4e18, finite

# fwd: (route, nq, check) of hdiff_mha_flash_fwd_route with lse; bwd: (nk, aligned, nsplit) of hdiff_mha_flash_bwd_route, both in f32 mode
Case = namedtuple("Case", "L B heads D fwd bwd")
RM1, RM4, FAST = (RUNNING_MAX, 1, 0), (RUNNING_MAX, 4, 0), (FAST_F32, 4, 1)


def _rows():
    for D in ALL_D:      # dQ goes straight into dqkv (one key range), batch stride 3CL
        yield Case(64, 2, 8, D, RM1, (1, 1, 1))
    for D in ALL_D:      # two key tiles, the last with 36 live keys; two key ranges of one block
        yield Case(100, 1, 8, D, RM1, (1, 0, 2))
    for D in ALL_D:      # forward: 3 query blocks of 256, the last with 64 live queries; backward: 9 key blocks, 2 per range, the last range has one
        yield Case(576, 16, 8, D, FAST if D < 48 else RM1, (1, 1, 5))
    for D in ALL_D:      # 600 = 9 x 64 + 24: ragged last query block and key tile; 10 key blocks, 2 per range, the last with 24 live keys
        yield Case(600, 16, 8, D, RM4 if D < 48 else RM1, (1, 0, 5))
    for D in (24, 32):   # two key tiles per wave: the PIPELINED / KT_FENCE forms, 3 blocks per range
        yield Case(4224, 8, 8, D, FAST, (2, 1, 11))
    for D in (4, 8, 12, 16):     # four key tiles per wave: TWO_AHEAD with 68 query tiles, 2 blocks per range, the last range one
        yield Case(4352, 8, 8, D, FAST, (4, 1, 9))
    for D in (16, 32):   # L % (64 nk) != 0 falls back to 64-key blocks, aligned
        yield Case(4160, 8, 8, D, FAST, (1, 1, 13))
    for D, fwd in ((16, RM4), (64, RM1)):           # 667 = 23 x 29 = 10 x 64 + 27, L % 4 != 0: scalar loads and stores, 11 key blocks, 6 ranges
        yield Case(667, 16, 8, D, fwd, (1, 0, 6))
    yield Case(600, 16, 1, 32, RM4, (1, 0, 10))     # AttnBlock's flash route: strides with one head
    yield Case(600, 128, 1, 64, RM1, (1, 0, 5))     # more samples than heads in blockIdx.z


CASES = tuple(_rows())
OLD_FAMILIES = ("plain", "peaked", "wide-V", "loud-dO-pixel", "tiny-dO", "zero-dO-head")      # _attn_bwd_cases.make_case
NEW_FAMILIES = ("all-negative", "late-spike", "one-hot-dO")
FAMILIES = OLD_FAMILIES + NEW_FAMILIES


def _runs():
    """(case, family) of the GPU module: plain everywhere; the other families at d_head 8, 16, 32, 64 with 8 heads at L 576 and 600;
    the new families also at one long case of two and of four key tiles per wave"""
    for c in CASES:
        yield c, "plain"
    for c in CASES:
        if c.heads == 8 and c.L in (576, 600) and c.D in (8, 16, 32, 64):
            for f in FAMILIES[1:]:
                yield c, f
    for c in CASES:
        if (c.L, c.D) in ((4224, 32), (4352, 16)):
            for f in NEW_FAMILIES:
                yield c, f


RUNS = tuple(_runs())


def case_id(c):
    return "L%d-B%d-h%d-d%d" % (c.L, c.B, c.heads, c.D)


def last_tile(L):
    """first position of the last (ragged, where L % 64 != 0) tile of 64"""
    return 64 * ((L - 1) // 64)


SPIKE_ROWS = lambda L: (7, L // 2, L - 2)          # queries whose late spike is certain: first block, middle, last tile


@functools.lru_cache(maxsize=None)
def base_pairs(family, D, L):
    """three (sample, head) pairs: qkv [3, 3D, L] (rows q | k | v) and dO [3, D, L], fp32, seeded by (family, D, L)"""
    g = torch.Generator().manual_seed(1009 * FAMILIES.index(family) + 31 * D + L)
    if family in OLD_FAMILIES:
        qkv, d_o = K.make_case(family, D, L, 3, 1, g)
        if family == "zero-dO-head":
            d_o[2] = 0.0                                  # base pair 2 is the silent one
        return qkv.contiguous(), d_o.contiguous()
    qkv = torch.randn(3, 3 * D, L, generator=g) * 1.3
    d_o = torch.randn(3, D, L, generator=g)
    if family == "all-negative":
        # q = u + 0.3 randn, k = -3u + 0.3 randn: every real score sits near -3 |u|^2 / sqrt(D), far below the 0 of a padded key.
        # u ~ 1.5 randn per pair, brought to its expected length 1.5 sqrt(D): at D = 8 |u|^2 would otherwise spread by a factor of 3
        # either way and the family's claim (tests/test_attn_f32_cases_cpu.py) would hold or not by the seed
        u = torch.randn(3, D, 1, generator=g)
        u = u * (1.5 * math.sqrt(D) / u.norm(dim=1, keepdim=True))
        qkv[:, :D] = u + 0.3 * torch.randn(3, D, L, generator=g)
        qkv[:, D:2 * D] = -3.0 * u + 0.3 * torch.randn(3, D, L, generator=g)
    elif family == "late-spike":
        # key 5 (first tile) and key L - 3 (last tile) carry 10 sqrt(D) and 45 sqrt(D) in channel 0: scores 10 q0 and 45 q0 (nats).
        # A query with q0 = 3.5 sees the last tile beat the first tile's maximum by ~120 nats = 175 log2 units (> 2^7: the fixed-
        # reference kernel overflows, poisons the row and leaves it to its check pass; the running-max kernel rescales by exp2(-175)
        # = 0); the randn queries around q0 = 0 keep rows where the spike shares its weight, so the gradients are not all rounding
        qkv[:, D, 5] = 10.0 * math.sqrt(D)
        qkv[:, D, L - 3] = 45.0 * math.sqrt(D)
        for q in SPIKE_ROWS(L):
            qkv[:, 0, q] = 3.5
    elif family == "one-hot-dO":
        d_o.zero_()
        for p in range(3):
            d_o[p, (1 + p) % D, L - 2 - p] = 1.5          # a single (channel, query), inside the last tile
    else:
        raise KeyError(family)
    return qkv.contiguous(), d_o.contiguous()


def split_pair(qkv, d_o, p):
    D = d_o.shape[1]
    return qkv[p, :D], qkv[p, D:2 * D], qkv[p, 2 * D:], d_o[p]


def pair_index(B, heads):
    """base pair of every (b, h): neighbouring heads differ"""
    return (torch.arange(B * heads) % 3).view(B, heads)


def make_batch(case, family, device="cpu"):
    """qkv [B, 3C, L], dO [B, C, L] of a case: pair (b, h) is base pair (b * heads + h) % 3"""
    qkv3, do3 = base_pairs(family, case.D, case.L)
    qkv3, do3 = qkv3.to(device), do3.to(device)
    idx = pair_index(case.B, case.heads).to(device).flatten()
    D, L, B, H = case.D, case.L, case.B, case.heads
    thirds = qkv3.view(3, 3, D, L)[idx].view(B, H, 3, D, L).permute(0, 2, 1, 3, 4)      # [B, 3, heads, D, L]
    return thirds.reshape(B, 3 * H * D, L).contiguous(), do3[idx].view(B, H * D, L).contiguous()


DEFECTS = ("pad0", "skip-last-query-tile", "skip-last-key-block-dQ", "drop-slab", "dK-unscaled-channel", "lse2-off")


def definition(q, k, v, d_o, dtype, chunk=1024, defect=None, slab=None):
    """The textbook formulas of one pair (q, k, v, dO: [D, L]) evaluated in `dtype`, query-chunked:
         S = Q K^T / sqrt(D), P = softmax(S), O = P V, lse2 = log2 sum exp S (what the kernels store),
         dP = dO V^T, dS = P o (dP - rowsum(dO o O)), dQ = dS K / sqrt(D), dK = dS^T Q / sqrt(D), dV = P^T dO
    -> {"O", "dQ", "dK", "dV": [D, L], "lse2": [L]}.  defect: one of DEFECTS, a model of a kernel bug (CPU test only);
    slab = (first key, keys) of the key range that "drop-slab" leaves out of dQ."""
    D, L = q.shape
    Q, Kk, V, dO = (t.to(dtype).t().contiguous() for t in (q, k, v, d_o))
    scale = 1.0 / math.sqrt(D)
    if defect == "pad0":                       # keys up to the next multiple of 64 admitted with score 0 (zero K, zero V)
        pad = torch.zeros(-L % 64, D, dtype=dtype)
        Kk, V = torch.cat([Kk, pad]), torch.cat([V, pad])
    nk = Kk.shape[0]
    O = torch.empty(L, D, dtype=dtype); lse2 = torch.empty(L, dtype=dtype)
    dQ = torch.empty(L, D, dtype=dtype); dK = torch.zeros(nk, D, dtype=dtype); dV = torch.zeros(nk, D, dtype=dtype)
    for i in range(0, L, chunk):
        s = slice(i, min(L, i + chunk))
        S = (Q[s] @ Kk.t()) * scale
        P = torch.softmax(S, dim=-1)
        O[s] = P @ V
        lse2[s] = torch.logsumexp(S, dim=-1) * LOG2E
        dP = dO[s] @ V.t()
        dS = P * (dP - (dO[s] * O[s]).sum(-1, keepdim=True))
        dSq, dSk, Pk = dS, dS, P
        if defect == "skip-last-key-block-dQ":
            dSq = dS.clone(); dSq[:, last_tile(L):] = 0
        if defect == "drop-slab":
            dSq = dS.clone(); dSq[:, slab[0]:slab[0] + slab[1]] = 0
        if defect == "skip-last-query-tile":
            live = (torch.arange(s.start, s.stop) < last_tile(L)).to(dtype)[:, None]
            dSk, Pk = dS * live, P * live
        dQ[s] = (dSq @ Kk) * scale
        dK += (dSk.t() @ Q[s]) * scale
        dV += Pk.t() @ dO[s]
    dK, dV = dK[:L].clone(), dV[:L]
    if defect == "dK-unscaled-channel":
        dK[:, 0] *= math.sqrt(D)
    if defect == "lse2-off":
        lse2 = lse2 + 2.0 ** -12
    return {"O": O.t().contiguous(), "lse2": lse2, "dQ": dQ.t().contiguous(), "dK": dK.t().contiguous(), "dV": dV.t().contiguous()}


@functools.lru_cache(maxsize=None)
def references(family, D, L):
    """(ref64, yard32): per base pair the definition in float64 and in float32; computed once per (family, D, L), never written to"""
    qkv, d_o = base_pairs(family, D, L)
    ref = [definition(*split_pair(qkv, d_o, p), torch.float64) for p in range(3)]
    yard = [definition(*split_pair(qkv, d_o, p), torch.float32) for p in range(3)]
    return ref, yard


def scores64(family, D, L, p):
    """float64 scores [L, L] of base pair p in the log2 domain the kernels work in"""
    qkv, d_o = base_pairs(family, D, L)
    q, k, _, _ = split_pair(qkv, d_o, p)
    return (q.double().t() @ k.double()) * (LOG2E / math.sqrt(D))


def ulp32(x):
    """one fp32 ulp of |x| (0 at 0: a tensor whose reference is all zero must be exactly zero)"""
    if x == 0.0:
        return 0.0
    return 2.0 ** (max(math.frexp(x)[1] - 1, -126) - 23)


def _stats(t, ref, per_row):
    e = t.double() - ref
    dims = (-1,) if per_row else tuple(range(e.dim()))
    return e.abs().amax(dims).reshape(-1), e.pow(2).mean(dims).sqrt().reshape(-1), ref.abs().amax(dims).reshape(-1)


def gate(got, ref64, yard32, family="plain", margin=None):
    """One pair: got, ref64, yard32 are {name: CPU tensor} over TENSORS.  For every tensor, against its own magnitude:
         max |got - ref64| <= max(margin * max |yard32 - ref64|, ulp32(max |ref64|)),  and the same for the rms error,
    margin = margin_of(family, tensor) unless given.
    wide-V: O is gated per channel row (V's channels are 2^30 apart), the yardstick's statistic per row likewise.
    -> {name: {"max", "rms": error, "max_x", "rms_x": its ratio to the yardstick's (inf where that is 0 and the error is not),
               "mag"}}; raises AssertionError naming every tensor that fails."""
    report, fails = {}, []
    for name in TENSORS:
        mg = margin_of(family, name) if margin is None else margin
        g, r, y = got[name].detach().cpu(), ref64[name], yard32[name]
        assert g.shape == r.shape and r.dtype == torch.float64, (name, g.shape, r.shape, r.dtype)
        if not torch.isfinite(g).all():
            fails.append(f"{name}: not finite")
            continue
        per_row = family == "wide-V" and name == "O"
        gmax, grms, mag = _stats(g, r, per_row)
        ymax, yrms, _ = _stats(y, r, per_row)
        floor = torch.tensor([ulp32(m) for m in mag.tolist()], dtype=torch.float64)
        ratio = lambda a, b: float((torch.where(a == 0, torch.zeros_like(a), a / b.clamp_min(1e-300))).max())
        report[name] = {"max": float(gmax.max()), "rms": float(grms.max()), "max_x": ratio(gmax, ymax), "rms_x": ratio(grms, yrms),
                        "mag": float(mag.max())}
        for what, e, ye in (("max", gmax, ymax), ("rms", grms, yrms)):
            bound = torch.maximum(mg * ye, floor)
            bad = e > bound
            if bad.any():
                i = int((e / bound.clamp_min(1e-300)).argmax())
                fails.append(f"{name}{'[row %d]' % i if per_row else ''}: {what} error {e[i].item():.3e} > bound {bound[i].item():.3e} "
                             f"(fp32 CPU definition {ye[i].item():.3e}, ulp {floor[i].item():.3e}, max|ref| {mag[i].item():.3e})")
    assert not fails, f"{family}: " + "; ".join(fails)
    return report


def fwd_route(lib, c):
    out = [C.c_int(-1) for _ in range(3)]
    assert lib.hdiff_mha_flash_fwd_route(c.B, c.heads * c.D, c.heads, c.L, 1, 0, *(C.byref(v) for v in out)) == 0
    return tuple(v.value for v in out)


def bwd_route(lib, c):
    """(route, nk, aligned, nsplit)"""
    out = [C.c_int(-1) for _ in range(4)]
    assert lib.hdiff_mha_flash_bwd_route(c.B, c.heads * c.D, c.heads, c.L, *(C.byref(v) for v in out)) == 0
    return tuple(v.value for v in out)


def bwd_workspace(lib, c):
    need = C.c_int64(-1)
    assert lib.hdiff_mha_flash_bwd_workspace(c.B, c.heads * c.D, c.heads, c.L, C.byref(need)) == 0
    return need.value


def _guarded(n):
    """a payload of n floats pre-filled with NaN, between two canaries: (whole buffer, payload view)"""
    buf = torch.full((n + 2 * CANARY,), CANARY_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
    buf[CANARY:CANARY + n] = float("nan")
    return buf, buf[CANARY:CANARY + n]


def _canaries_intact(buf, n):
    bits = buf.view(torch.int32)
    return bool((bits[:CANARY] == CANARY_BITS).all()) and bool((bits[CANARY + n:] == CANARY_BITS).all())


def run_f32(lib, case, qkv, d_o, lse_shift=0.0):
    """hdiff_mha_flash_fwd (with lse) and hdiff_mha_flash_bwd through the C ABI in f32 mode on device tensors.  Every output and the
    workspace is a slice of a larger buffer between canaries, pre-filled with NaN: afterwards o, lse2, delta, dqkv are finite
    everywhere and no canary has changed.  Asserts the routes of the call are the table's.  lse_shift: added to lse2 between the two
    calls (the negative control).  -> {"o" [B, C, L], "lse2" [B, heads, L], "dqkv" [B, 3C, L]}"""
    B, H, D, L = case.B, case.heads, case.D, case.L
    Cc = H * D
    s = torch.cuda.current_stream().cuda_stream
    before = lib.hdiff_get_contraction_mode()
    try:
        assert lib.hdiff_set_contraction_mode(0) == 0
        assert fwd_route(lib, case) == case.fwd, (case, fwd_route(lib, case))
        assert bwd_route(lib, case) == (0,) + case.bwd, (case, bwd_route(lib, case))
        need = bwd_workspace(lib, case)
        sizes = {"o": B * Cc * L, "lse2": B * H * L, "delta": B * H * L, "dqkv": 3 * B * Cc * L, "ws": need}
        bufs = {n: _guarded(sz) for n, sz in sizes.items()}
        p = {n: v[1] for n, v in bufs.items()}
        assert lib.hdiff_mha_flash_fwd(qkv.data_ptr(), p["o"].data_ptr(), p["lse2"].data_ptr(), B, Cc, H, L, s) == 0
        if lse_shift:
            p["lse2"] += lse_shift
        assert lib.hdiff_mha_flash_bwd(qkv.data_ptr(), p["o"].data_ptr(), d_o.data_ptr(), p["lse2"].data_ptr(), p["delta"].data_ptr(),
                                       p["dqkv"].data_ptr(), p["ws"].data_ptr(), B, Cc, H, L, s) == 0
        torch.cuda.synchronize()
    finally:
        lib.hdiff_set_contraction_mode(before)
    for n, (buf, pay) in bufs.items():
        assert _canaries_intact(buf, sizes[n]), f"{n}: a canary next to the buffer was written"
        if n != "ws":
            assert bool(torch.isfinite(pay).all()), f"{n}: an element was not written, or is not finite"
    return {"o": p["o"].view(B, Cc, L), "lse2": p["lse2"].view(B, H, L), "dqkv": p["dqkv"].view(B, 3 * Cc, L)}


def pairs_of(out, case):
    """the results per (sample, head) pair: {name: [B, heads, D, L]} (lse2: [B, heads, L])"""
    B, H, D, L = case.B, case.heads, case.D, case.L
    g = out["dqkv"].view(B, 3, H, D, L)
    return {"O": out["o"].view(B, H, D, L), "lse2": out["lse2"], "dQ": g[:, 0], "dK": g[:, 1], "dV": g[:, 2]}
