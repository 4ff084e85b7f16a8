"""Shared by tests/test_attn_bwd_h2_cases_cpu.py, tests/test_gpu_attn_bwd_h2.py and tools/attn_bwd_error_ratio.py: the split-operand
attention backward (csrc/attention_bwd_h2.hip: mha_bwd_h2p_kernel at d_head 16, mha_bwd_h2_kernel<32> at d_head 32) where a workgroup
walks a key range of MORE THAN ONE block of 256 keys -- the first block stores its dQ slab, every later block runs the other
instantiation (sweep<false> / the !first_kb path): it adds to the slab in L2, reuses the LDS tile buffers, reloads the stationary
operands and resets the dK / dV accumulators.
  * CASES: the smallest shapes at which mha_bwd_h2_key_ranges gives per = 2, 3, 4 blocks per range (B * heads >= 64, so that 16
    ranges are wanted), the per = 1 partner of the first, and AttnBlock's one-head strides,
  * the input families of _attn_bwd_cases / _attn_f32_cases plus block-seam; every (sample, head) pair of a batch is a copy of one
    of three base pairs,
  * forward64() / backward(): the backward ALONE -- O and lse2 come from the float64 definition rounded to fp32, the kernels and the
    reference consume the same rounded values -- in float64 (the reference) and in torch float32 (the fp32 CPU definition), with
    models of the defects a later block can have,
  * gate(): dQ, dK, dV against float64 as ratios to a yardstick's error: the contract of tests/test_gpu_backward.py, unchanged.
Importable without a GPU; run_bwd() alone touches one."""
import ctypes as C
import functools
import math
from collections import namedtuple

import torch

import _attn_f32_cases as F

DEV = F.DEV
KB = 256                                            # keys per block of both kernels
LOG2E = F.LOG2E
TENSORS = ("dQ", "dK", "dV")
FUSED_F32, H2_PAIRS = 0, 1                          # HDIFF_MHA_BWD_ROUTE_*
CANARY, CANARY_BITS = F.CANARY, F.CANARY_BITS

# per: key blocks per range, nsplit: ranges, of hdiff_mha_flash_bwd_route in the split modes with HDIFF_BWD_SLAB_GIB unset
Case = namedtuple("Case", "name L B heads D per nsplit")


def _rows():
    for D in (16, 32):
        yield Case("seam2", 4352, 8, 8, D, 2, 9)        # 17 blocks: one non-first block per range, the last range has a single block
        yield Case("seam3", 8448, 8, 8, D, 3, 11)       # 33 blocks: two non-first blocks per range, every range full
        yield Case("seam4", 12544, 8, 8, D, 4, 13)      # 49 blocks: the production-like per >= 4, the last range is short (one block)
        yield Case("alone", 4352, 1, 8, D, 1, 17)       # the pairs of seam2 with one block per range
    yield Case("one-head", 4352, 64, 1, 32, 2, 9)       # heads = 1, C = 32: AttnBlock's strides, more samples than heads


CASES = tuple(_rows())
OLD_FAMILIES = ("plain", "peaked", "wide-V", "loud-dO-pixel", "zero-dO-head")      # _attn_bwd_cases.make_case
F32_FAMILIES = ("late-spike", "one-hot-dO")                                         # _attn_f32_cases
FAMILIES = OLD_FAMILIES + F32_FAMILIES + ("block-seam",)
UNMEASURED = F32_FAMILIES + ("block-seam",)         # no ratio of this kernel had been measured on them before this module
SEAM_KEYS = (KB - 1, KB, 4095, 4096)                # block-seam at L = 4352, per = 2: last key of a range's first block | first key of its
                                                    # second block; last key of range 7 | the single-block last range
SPIKE = 4.0                                         # x sqrt(D) in channel 0 of K: a score of 14 nats for a query with q0 = 3.5


def seam_rows(L):
    """query rows of the first two and the last two tiles of 32: what the pipeline's prologue and drain iterations handle"""
    return (0, 31, 32, L - 33, L - 1)


def _runs():
    for c in CASES:
        yield c, "plain"
    for c in CASES:
        if c.name in ("seam2", "one-head"):
            for f in FAMILIES[1:]:
                yield c, f


RUNS = tuple(_runs())


def case_id(c):
    return "%s-d%d" % (c.name, c.D)


def find(name, D):
    return next(c for c in CASES if (c.name, c.D) == (name, D))


def ref_pairs(c):
    """the base pairs that are compared with float64"""
    return (0,) if c.name == "seam4" else (0, 1, 2)


def blocks(c):
    return c.L // KB


@functools.lru_cache(maxsize=None)
def base_pairs(family, D, L):
    """three (sample, head) pairs: qkv [3, 3D, L] (rows q | k | v) and dO [3, D, L], fp32 on the CPU, seeded by (family, D, L)"""
    if family != "block-seam":
        return F.base_pairs(family, D, L)
    assert L > SEAM_KEYS[-1] + KB - 1 and L % KB == 0
    g = torch.Generator().manual_seed(7919 + 31 * D + L)
    qkv = torch.randn(3, 3 * D, L, generator=g) * 1.3
    noise = torch.randn(3, D, L, generator=g)
    d_o = torch.zeros(3, D, L)
    qkv[:, D, SEAM_KEYS[0]] = SPIKE * math.sqrt(D)
    for key in SEAM_KEYS[1:]:                       # one K row at all four: each owns a quarter of their mass, V and so dP differ
        qkv[:, D:2 * D, key] = qkv[:, D:2 * D, SEAM_KEYS[0]]
    for q in seam_rows(L):
        qkv[:, 0, q] = 3.5
        d_o[:, :, q] = noise[:, :, q]
    return qkv.contiguous(), d_o.contiguous()


def make_batch(case, family, device="cpu"):
    """qkv [B, 3C, L], dO [B, C, L]: pair (b, h) is base pair (b * heads + h) % 3"""
    qkv3, do3 = base_pairs(family, case.D, case.L)
    return _spread(case, qkv3.to(device).view(3, 3, case.D, case.L), 3), _spread(case, do3.to(device), 1)


def _spread(case, base, thirds):
    """base [3, (thirds,) D, L] -> [B, thirds * C, L] by F.pair_index"""
    B, H, D, L = case.B, case.heads, case.D, case.L
    idx = F.pair_index(B, H).to(base.device).flatten()
    if thirds == 1:
        return base[idx].view(B, H * D, L).contiguous()
    return base[idx].view(B, H, thirds, D, L).permute(0, 2, 1, 3, 4).reshape(B, thirds * H * D, L).contiguous()


def forward64(q, k, v, chunk=1024):
    """O [D, L] and lse2 [L] of one pair (q, k, v: [D, L]) from the float64 definition, ROUNDED TO FP32: what every backward here is fed"""
    D, L = q.shape
    Q, Kk, V = (t.double().t().contiguous() for t in (q, k, v))
    O = torch.empty(L, D, dtype=torch.float64, device=q.device)
    lse2 = torch.empty(L, dtype=torch.float64, device=q.device)
    for i in range(0, L, chunk):
        S = (Q[i:i + chunk] @ Kk.t()).div_(math.sqrt(D))
        m = S.amax(-1, keepdim=True)
        E = S.sub_(m).exp_()                             # one exp per score: the float64 softmax is the cost of every reference here
        z = E.sum(-1, keepdim=True)
        O[i:i + chunk] = (E @ V) / z
        lse2[i:i + chunk] = (m + z.log()).squeeze(-1) * LOG2E
    return O.t().float().contiguous(), lse2.float()


DEFECTS = ("dQ-drops-later-blocks", "dQ-block-twice", "stale-KV", "no-reset", "skip-last-range")


def backward(q, k, v, d_o, o, lse2, dtype, chunk=1024, defect=None, per=None):
    """The backward of one pair as a function of (q, k, v, dO, O, lse2), all [D, L] / [L] fp32, evaluated in `dtype`, query-chunked:
         P = exp2(Q K^T log2(e) / sqrt(D) - lse2), dP = dO V^T, dS = P o (dP - rowsum(dO o O)),
         dQ = dS K / sqrt(D), dK = dS^T Q / sqrt(D), dV = P^T dO                                   -> {"dQ", "dK", "dV": [D, L]}
    defect: one of DEFECTS, a model of what a block behind the first of its key range can get wrong (CPU test only), with `per`
    blocks of KB keys per range; the block hit is the second of range 0 -- keys KB ... 2 KB - 1 --, the range hit is range 0:
      dQ-drops-later-blocks  dQ lacks every non-first block of the range (the L2 add did not happen)
      dQ-block-twice         the block is added to the dQ slab twice
      stale-KV               dK / dV of the block come from the previous block's K and V (stationary operands not reloaded)
      no-reset               dK / dV of the block also carry the previous block's sums (accumulators not reset)
      skip-last-range        the last range is not run: no dK / dV there, its keys missing from dQ"""
    D, L = q.shape
    Q, Kk, V, dO, O = (t.to(dtype).t().contiguous() for t in (q, k, v, d_o, o))
    lse = lse2.to(dtype)
    scale = 1.0 / math.sqrt(D)
    delta = (dO * O).sum(-1)
    dQ = torch.empty(L, D, dtype=dtype, device=q.device)
    dK, dV = torch.zeros_like(dQ), torch.zeros_like(dQ)
    nkb = L // KB
    last = ((nkb - 1) // per) * per * KB if per else None          # first key of the last range
    for i in range(0, L, chunk):
        s = slice(i, min(L, i + chunk))
        P = (Q[s] @ Kk.t()).mul_(LOG2E * scale).sub_(lse[s, None]).exp2_()
        dS = (dO[s] @ V.t()).sub_(delta[s, None]).mul_(P)
        dSq = dS
        if defect == "dQ-drops-later-blocks":
            dSq = dS.clone(); dSq[:, KB:per * KB] = 0
        elif defect == "dQ-block-twice":
            dSq = dS.clone(); dSq[:, KB:2 * KB] *= 2
        elif defect == "skip-last-range":
            dSq = dS.clone(); dSq[:, last:] = 0
        dQ[s] = (dSq @ Kk) * scale
        dK += (dS.t() @ Q[s]) * scale
        dV += P.t() @ dO[s]
    if defect == "stale-KV":              # P and dS of a key depend on its own K and V row only (lse2 and delta are inputs)
        dK[KB:2 * KB] = dK[:KB]; dV[KB:2 * KB] = dV[:KB]
    elif defect == "no-reset":
        dK[KB:2 * KB] += dK[:KB]; dV[KB:2 * KB] += dV[:KB]
    elif defect == "skip-last-range":
        dK[last:] = 0; dV[last:] = 0
    else:
        assert defect is None or defect in DEFECTS, defect
    return {"dQ": dQ.t().contiguous(), "dK": dK.t().contiguous(), "dV": dV.t().contiguous()}


@functools.lru_cache(maxsize=None)
def forwards(family, D, L, device="cpu"):
    """(O [3, D, L], lse2 [3, L]) of the three base pairs, fp32 on `device`; computed once, never written to"""
    qkv, d_o = base_pairs(family, D, L)
    qkv = qkv.to(device)
    outs = [forward64(*F.split_pair(qkv, d_o, p)[:3]) for p in range(3)]
    return torch.stack([o for o, _ in outs]), torch.stack([l for _, l in outs])


@functools.lru_cache(maxsize=None)
def reference(family, D, L, p, device="cpu"):
    """the float64 backward of base pair p; computed once per (family, D, L, p), never written to.  seam2, alone and one-head share
    them where (D, L) agree"""
    qkv, d_o = base_pairs(family, D, L)
    o, lse2 = forwards(family, D, L, device)
    return backward(*F.split_pair(qkv.to(device), d_o.to(device), p), o[p], lse2[p], torch.float64)


@functools.lru_cache(maxsize=None)
def yard32(family, D, L, p):
    """the fp32 CPU definition of base pair p: the same formulas in torch float32 on the CPU"""
    qkv, d_o = base_pairs(family, D, L)
    o, lse2 = forwards(family, D, L, "cpu")
    return backward(*F.split_pair(qkv, d_o, p), o[p], lse2[p], torch.float32)


@functools.lru_cache(maxsize=None)
def dq_block_terms(family, D, L, p, device="cpu"):
    """sum over the key blocks b of |dQ_b|, dQ_b = dS[:, block b] K[block b] / sqrt(D) -- the fp32 numbers that the slab adds and the
    reduce kernel sum, whatever the key ranges -- of base pair p in float64: [D, L]"""
    qkv, d_o = base_pairs(family, D, L)
    o, lse2 = forwards(family, D, L, device)
    q, k, v, do = F.split_pair(qkv.to(device), d_o.to(device), p)
    Q, Kk, V, dO, O = (t.double().t().contiguous() for t in (q, k, v, do, o[p]))
    scale = 1.0 / math.sqrt(D)
    delta = (dO * O).sum(-1)
    out = torch.empty(L, D, dtype=torch.float64, device=q.device)
    for i in range(0, L, 1024):
        s = slice(i, min(L, i + 1024))
        P = (Q[s] @ Kk.t()).mul_(LOG2E * scale).sub_(lse2[p, s, None].double()).exp2_()
        dS = (dO[s] @ V.t()).sub_(delta[s, None]).mul_(P)
        out[s] = torch.einsum("qbk,bkd->qbd", dS.view(-1, L // KB, KB), Kk.view(L // KB, KB, D)).abs().sum(1) * scale
    return out.t().contiguous()


def seam_mass(D, L, p):
    """block-seam, base pair p: for every row of seam_rows(L) the softmax mass that the keys SEAM_KEYS own together, from float64 scores"""
    qkv, d_o = base_pairs("block-seam", D, L)
    q, k, _, _ = F.split_pair(qkv, d_o, p)
    S = (q.double().t()[list(seam_rows(L))] @ k.double()) / math.sqrt(D)
    return torch.softmax(S, dim=-1)[:, list(SEAM_KEYS)].sum(-1)


# The contract of the kernel against float64, as ratios to the fp32-input kernel's error on the same inputs
# (tests/test_gpu_backward.py: test_attention_backward_fp16_pairs_error_class_every_pair and ..._ranges), unchanged:
ALL_RMS, ALL_WORST = 1.25, 3.0                      # over all referenced pairs
PAIR_RMS_PLAIN, PAIR_WORST_PLAIN = 1.25, 4.0        # one pair, plain
PAIR_RMS_RANGE = 4.0                                # one pair, every other family
WORST_OF_MAG = 2e-5                                 # worst error over the tensor's magnitude, every other family
ROOM = F.ROOM
# Cells of UNMEASURED families in which the correct kernel exceeds a constant above: (family, tensor, check) -> the worst ratio
# measured on the MI355X (profiles/attention_bwd_h2_multiblock_error_ratio.txt, tools/attn_bwd_error_ratio.py multiblock); the
# cell's margin is max(contract, ROOM x measured).  tests/test_gpu_attn_bwd_h2.py states the cause of each.
MEASURED = {
    ("late-spike", "dV", "all-rms"): 1.342,
    ("block-seam", "dK", "all-rms"): 3.188, ("block-seam", "dK", "pair-rms"): 7.697,
    ("block-seam", "dV", "all-rms"): 3.340, ("block-seam", "dV", "pair-rms"): 4.704,
}
YARD = F.YARD               # a cell that carries a measurement is also held to the fp32 CPU definition, at the project's margin over one
CHECKS = ("all-rms", "all-worst", "pair-rms", "pair-worst", "worst-of-mag")


def margin_of(family, name, check):
    contract = {"all-rms": ALL_RMS, "all-worst": ALL_WORST, "pair-rms": PAIR_RMS_PLAIN if family == "plain" else PAIR_RMS_RANGE,
                "pair-worst": PAIR_WORST_PLAIN if family == "plain" else None,
                "worst-of-mag": None if family == "plain" else WORST_OF_MAG}[check]
    if contract is None:
        return None
    m = MEASURED.get((family, name, check))
    assert m is None or family in UNMEASURED, "only a family without an earlier measurement may carry one"
    return contract if m is None else max(contract, ROOM * m)


def _err(t, ref):
    e = t.double() - ref
    return e.pow(2).sum().item(), e.abs().max().item(), e.numel()


def gate(got, yard, ref, family, enforce=True):
    """got, yard, ref: [{name: [D, L]}] over the referenced pairs (ref in float64).  For dQ, dK, dV, with x = got's statistic of the
    error against ref and y = yard's:
       over all pairs   rms x <= 1.25 y, worst x <= 3 y
       one pair         plain: rms x <= 1.25 y, worst x <= 4 y;  the other families: rms x <= 4 y
       the other families: worst x <= 2e-5 max |ref| over all pairs
    (each constant replaced by margin_of() where MEASURED has the cell).  A statistic that is 0 for the yardstick must be 0.
    -> {name: {check: the largest x / y (worst-of-mag: x / max |ref|; 0 / 0 counts as 0), "mag"}}; raises AssertionError naming every
    failure unless enforce is False (the measuring tool)."""
    assert len(got) == len(yard) == len(ref) and len(ref) >= 1
    report, fails = {}, []
    div = lambda a, b: a / b if b else (0.0 if a == 0 else float("inf"))
    for name in TENSORS:
        for r in ref:
            assert r[name].dtype == torch.float64
        if not all(bool(torch.isfinite(g[name]).all()) for g in got):
            fails.append(f"{name}: not finite")
            continue
        eg = [_err(g[name], r[name]) for g, r in zip(got, ref)]
        ey = [_err(y[name], r[name]) for y, r in zip(yard, ref)]
        n = sum(e[2] for e in eg)
        mag = max(r[name].abs().max().item() for r in ref)
        worst = max(e[1] for e in eg)
        checks = [("all-rms", "all pairs", math.sqrt(sum(e[0] for e in eg) / n), math.sqrt(sum(e[0] for e in ey) / n)),
                  ("all-worst", "all pairs", worst, max(e[1] for e in ey)), ("worst-of-mag", "all pairs", worst, mag)]
        for p, (a, b) in enumerate(zip(eg, ey)):
            checks.append(("pair-rms", "pair %d" % p, math.sqrt(a[0] / a[2]), math.sqrt(b[0] / b[2])))
            checks.append(("pair-worst", "pair %d" % p, a[1], b[1]))
        rep = {"mag": mag}
        for check, where, a, b in checks:
            rep[check] = max(rep.get(check, 0.0), div(a, b))
            mg = margin_of(family, name, check)
            if mg is not None and not a <= mg * b:
                fails.append(f"{name} {check} ({where}): {a:.3e} > {mg:g} x {b:.3e}")
        report[name] = rep
    assert not (enforce and fails), f"{family}: " + "; ".join(fails)
    return report


def bwd_route(lib, c):
    """(route, nk, aligned, nsplit) in the library's current contraction mode"""
    out = [C.c_int(-1) for _ in range(4)]
    assert lib.hdiff_mha_flash_bwd_route(c.B, c.heads * c.D, c.heads, c.L, *(C.byref(v) for v in out)) == 0
    return tuple(v.value for v in out)


def run_bwd(lib, case, qkv, o, d_o, lse2, mode):
    """hdiff_mha_flash_bwd through the C ABI in contraction mode `mode` (0: the fp32-input kernel, 1: the split-operand kernels) on device
    tensors.  dqkv, delta and the workspace -- exactly hdiff_mha_flash_bwd_workspace floats -- are slices of larger buffers between
    canaries; dqkv and the workspace are pre-filled with NaN (a slab word that is added to before it was stored comes out NaN).
    Afterwards every canary is intact and dqkv and delta hold no NaN.  -> dqkv [B, 3C, L]"""
    B, H, D, L = case.B, case.heads, case.D, case.L
    Cc = H * D
    s = torch.cuda.current_stream().cuda_stream
    before = lib.hdiff_get_contraction_mode()
    try:
        assert lib.hdiff_set_contraction_mode(mode) == 0
        sizes = {"delta": B * H * L, "dqkv": 3 * B * Cc * L, "ws": F.bwd_workspace(lib, case)}
        bufs = {n: F._guarded(sz) for n, sz in sizes.items()}
        p = {n: v[1] for n, v in bufs.items()}
        assert lib.hdiff_mha_flash_bwd(qkv.data_ptr(), o.data_ptr(), d_o.data_ptr(), lse2.data_ptr(), p["delta"].data_ptr(),
                                       p["dqkv"].data_ptr(), p["ws"].data_ptr(), B, Cc, H, L, s) == 0
        torch.cuda.synchronize()
    finally:
        lib.hdiff_set_contraction_mode(before)
    for n, (buf, pay) in bufs.items():
        assert F._canaries_intact(buf, sizes[n]), f"{n}: a canary next to the buffer was written"
        if n != "ws":
            assert not bool(torch.isnan(pay).any()), f"{n}: an element was not written, or is NaN"
    return p["dqkv"].view(B, 3 * Cc, L)


def device_inputs(case, family):
    """(qkv, O, dO, lse2) of a case on the GPU: O and lse2 are the float64 definition's, rounded to fp32"""
    qkv, d_o = make_batch(case, family, DEV)
    o3, lse3 = forwards(family, case.D, case.L, DEV)
    idx = F.pair_index(case.B, case.heads).to(DEV).flatten()
    return qkv, _spread(case, o3, 1), d_o, lse3[idx].view(case.B, case.heads, case.L).contiguous()


def pairs_of(dqkv, case):
    """{name: [B * heads, D, L]} of a result"""
    B, H, D, L = case.B, case.heads, case.D, case.L
    g = dqkv.view(B, 3, H, D, L)
    return {n: g[:, i].reshape(B * H, D, L) for i, n in enumerate(TENSORS)}


def measure(lib, case, family, with_yard=False):
    """Both kernels on the case's inputs against float64 (reference on the GPU): -> (report of gate() with the fp32-input kernel as the
    yardstick, the same with the fp32 CPU definition as the yardstick or None, the split-operand kernel's {name: [B * heads, D, L]}).
    The figures, not a verdict: gate() does not enforce here."""
    qkv, o, d_o, lse2 = device_inputs(case, family)
    h2 = pairs_of(run_bwd(lib, case, qkv, o, d_o, lse2, 1), case)
    f32 = pairs_of(run_bwd(lib, case, qkv, o, d_o, lse2, 0), case)
    ps = ref_pairs(case)
    ref = [reference(family, case.D, case.L, p, DEV) for p in ps]
    got = [{n: h2[n][p] for n in TENSORS} for p in ps]
    rep = gate(got, [{n: f32[n][p] for n in TENSORS} for p in ps], ref, family, enforce=False)
    rep_yard = None
    if with_yard:
        cpu_ref = [{n: r[n].cpu() for n in TENSORS} for r in ref]
        rep_yard = gate([{n: g[n].cpu() for n in TENSORS} for g in got], [yard32(family, case.D, case.L, p) for p in ps], cpu_ref, family,
                        enforce=False)
    return rep, rep_yard, h2
