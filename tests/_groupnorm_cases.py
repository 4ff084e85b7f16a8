"""Shared by tests/test_groupnorm_cases_cpu.py and tests/test_gpu_groupnorm.py: seeded GroupNorm(32, C) inputs with adverse
statistics (a mean far from zero, an outlier at the element gn_stats_kernel would take as its pivot, zero variance, ...), the
float64 references of the statistics (csrc/groupnorm.hip) and of the backward (the formulas in the header of
csrc/groupnorm_bwd.hip), and the gates both tests hold results to.  Plain torch on the CPU; nothing here touches a GPU."""
import math

import torch

G = 32
EPS = 1e-5
MIN_SLICE = 4096         # gn_stats_kernel's GN_MIN_SLICE: the fewest elements of a plane a split covers
U = 2.0 ** -24           # unit roundoff of fp32

FAMILIES = ("benign", "offset", "neg-offset", "pivot-spike-30", "pivot-spike-3000", "spike-elsewhere", "channel-steps",
            "constant", "constant-but-one", "tiny", "large")
BWD_FAMILIES = ("benign", "offset", "pivot-spike-3000", "channel-steps", "constant-but-one")
DA_KINDS = ("randn", "one-hot", "ones")

# (C0, C1, HW, B, nsplit)
SHAPES = [
    (32, 0, 64, 2, 1),        # cpg 1, fewer elements than threads
    (96, 0, 25, 2, 1),        # scalar loads, cpg 3
    (128, 0, 1024, 1, 1),     # cpg 4
    (256, 128, 64, 2, 1),     # groups of 12 straddle the seam at 256
    (128, 0, 4096, 1, 1),     # largest plane with the fused finalize
    (32, 0, 8192, 1, 2),      # smallest plane for which the product picks nsplit = 2
    (64, 0, 100, 2, 3),       # C ABI only: more splits than the plane is worth (a split covers >= MIN_SLICE elements of a
    (32, 0, 8, 1, 4),         # plane): one partial holds the slice, the others are empty
    (64, 0, 99, 2, 3),        # C ABI only: the same on scalar loads (HW % 4 != 0)
    (64, 0, 99, 2, 2),
    (32, 0, 6000, 1, 2),      # C ABI only: uneven partials, 4096 + 1904 elements per plane
    (32, 0, 8190, 1, 2),      # C ABI only: uneven scalar partials, 4096 + 4094, the second off a 16-byte boundary
    (32, 0, 8192, 1, 3),      # C ABI only: two full partials and an empty one
]
BWD_SHAPES = SHAPES[:6]       # nsplit plays no part in the backward


def product_nsplit(HW):
    """what Plan.gn_scale_shift and autograd._gn_stats pick"""
    return max(1, min(32, HW // 4096))


def shape_id(s):
    return "C%d+%d-HW%d-B%d-ns%d" % s


def slices(HW, nsplit):
    """[(first element, elements)] of a channel plane per split, as gn_stats_kernel cuts it: float4 units when HW % 4 == 0,
    per = max(ceil(units / nsplit), MIN_SLICE elements), lo = s * per; (None, 0) for an empty slice"""
    w = 4 if HW % 4 == 0 else 1
    units = HW // w
    per = max((units + nsplit - 1) // nsplit, MIN_SLICE // w)
    out = []
    for s in range(nsplit):
        lo, hi = s * per, min(units, (s + 1) * per)
        out.append((None, 0) if lo >= units else (w * lo, w * (hi - lo)))
    return out


def pivot_indices(HW, nsplit):
    """per split, the element of a channel plane at which the split's slice begins (None for an empty slice)"""
    return [first for first, _ in slices(HW, nsplit)]


def make_x(family, B, C, HW, G=G, seed=0, nsplit=1):
    """fp32 [B, C, HW]"""
    g = torch.Generator().manual_seed(seed)
    cpg = C // G
    n = torch.randn(B, C, HW, generator=g)
    if family == "benign":
        x = n
    elif family == "offset":
        x = 100.0 + 0.01 * n
    elif family == "neg-offset":
        x = -1000.0 + n
    elif family in ("pivot-spike-30", "pivot-spike-3000"):
        x = n
        spike = 30.0 if family.endswith("-30") else 3000.0
        for idx in pivot_indices(HW, nsplit):
            if idx is not None:
                x[:, 0::cpg, idx] = spike              # the first channel of every group
    elif family == "spike-elsewhere":
        x = n
        x[:, cpg - 1::cpg, HW - 1] = 3000.0            # the last element of every group's last channel
    elif family == "channel-steps":
        c = torch.arange(C)
        step = 50.0 * (1.0 - 2.0 * (c % 2)) * (c % cpg).float() / cpg
        x = n + step[None, :, None]
    elif family in ("constant", "constant-but-one"):
        x = torch.full((B, C, HW), 3.25)
        if family == "constant-but-one":
            x[:, (cpg // 2)::cpg, HW // 2] = 4.25      # one element of every group
    elif family == "tiny":
        x = 1e-4 * n
    elif family == "large":
        x = 1e4 * n
    else:
        raise KeyError(family)
    return x.float().contiguous()


def make_affine(C, seed, equal_gamma=False):
    g = torch.Generator().manual_seed(seed + 7919)
    gamma = torch.full((C,), 1.5) if equal_gamma else torch.randn(C, generator=g)
    return gamma.float(), torch.randn(C, generator=g).float()


def make_dA(kind, B, C, HW, seed):
    g = torch.Generator().manual_seed(seed + 104729)
    if kind == "randn":
        return torch.randn(B, C, HW, generator=g)
    if kind == "one-hot":                              # one nonzero element per sample
        d = torch.zeros(B, C, HW)
        for b in range(B):
            d[b, (5 + 11 * b) % C, (3 + 7 * b) % HW] = 2.0
        return d
    if kind == "ones":                                 # with equal gamma the three terms of the affine dx cancel to ~0
        return torch.ones(B, C, HW)
    raise KeyError(kind)


def ref_stats(x, G=G, eps=EPS, gamma=None, beta=None):
    """float64 statistics of the fp32 input cast up: dict of mean, rstd, std [B, G] and scale, shift [B, C]"""
    B, C, HW = x.shape
    cpg = C // G
    xd = x.double().view(B, G, cpg * HW)
    mean = xd.mean(-1)
    var = (xd - mean[..., None]).pow(2).mean(-1)
    rstd = 1.0 / torch.sqrt(var + eps)
    gam = torch.ones(C, dtype=torch.float64) if gamma is None else gamma.double()
    bet = torch.zeros(C, dtype=torch.float64) if beta is None else beta.double()
    scale = rstd.repeat_interleave(cpg, 1) * gam[None]
    shift = bet[None] - mean.repeat_interleave(cpg, 1) * scale
    return {"mean": mean, "rstd": rstd, "std": var.sqrt(), "scale": scale, "shift": shift}


def two_pass_fp32(x, gamma, beta, G=G, eps=EPS):
    """The same four results by the corrected two-pass algorithm in fp32 torch -- what correct fp32 code reaches.  Pass 1: a
    mean m0.  Pass 2: the sums of d = x - m0 and of d^2; mean = m0 + mean(d), var = mean(d^2) - mean(d)^2.  (The correction
    matters for the mean alone: a plain fp32 mean of values near 100 is a few ulp off, more than the gate's 2 * 2^-24 |ref|.)"""
    B, C, HW = x.shape
    cpg = C // G
    xr = x.view(B, G, cpg * HW)
    m0 = xr.mean(-1)
    d = xr - m0[..., None]
    md = d.mean(-1)
    mean = m0 + md
    var = (d.pow(2).mean(-1) - md * md).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32))
    scale = rstd.repeat_interleave(cpg, 1) * gamma[None]
    shift = beta[None] - mean.repeat_interleave(cpg, 1) * scale
    assert scale.dtype == torch.float32 and shift.dtype == torch.float32
    return mean, rstd, scale, shift


def forward_gate_report(got, ref, beta, constant, eps=EPS):
    """got: mean, rstd (either may be None), scale, shift as CPU tensors.  -> (list of failures, {name: worst error / bound})
      |rstd - ref| <= 2e-5 ref                          the suite's single-op tolerance
      |mean - ref| <= 2 * 2^-24 |ref| + 2e-5 std        storage rounding + the same 2e-5 in units of the standard deviation
                                                        (sqrt(eps) in place of std where the variance is exactly 0)
      |scale - ref| <= 2e-5 |ref| + 1e-30,  |shift - ref| <= 3e-5 (|beta| + |mean * scale|), each per element"""
    mean, rstd, scale, shift = got
    cpg = ref["scale"].shape[1] // ref["mean"].shape[1]
    std = torch.full_like(ref["std"], math.sqrt(eps)) if constant else ref["std"]
    checks = []
    if rstd is not None:
        checks.append(("rstd", rstd, ref["rstd"], 2e-5 * ref["rstd"]))
    if mean is not None:
        checks.append(("mean", mean, ref["mean"], 2 * U * ref["mean"].abs() + 2e-5 * std))
    checks.append(("scale", scale, ref["scale"], 2e-5 * ref["scale"].abs() + 1e-30))
    mean_scale = ref["mean"].repeat_interleave(cpg, 1) * ref["scale"]
    checks.append(("shift", shift, ref["shift"], 3e-5 * (beta.double().abs()[None] + mean_scale.abs())))
    fails, ratios = [], {}
    for name, g_, r_, bound in checks:
        g_ = g_.detach().cpu().double()
        assert g_.shape == r_.shape, (name, g_.shape, r_.shape)
        if not torch.isfinite(g_).all():
            fails.append(f"{name}: not finite")
            ratios[name] = float("inf")
            continue
        ratio = ((g_ - r_).abs() / bound)
        ratios[name] = ratio.max().item()
        if name == "rstd":
            ratios["rstd_rel"] = ((g_ - r_).abs() / r_).max().item()
        if ratios[name] > 1.0:
            i = ratio.argmax().item()
            fails.append(f"{name}: |err| {(g_ - r_).abs().flatten()[i].item():.3e} > bound {bound.flatten()[i].item():.3e} "
                         f"at flat index {i} (ref {r_.flatten()[i].item():.6e}, {ratios[name]:.1f} x the bound)")
    return fails, ratios


def ref_bwd(x, dA, mean32, rstd32, gamma, beta, swish):
    """The formulas of csrc/groupnorm_bwd.hip in float64, with the GIVEN fp32 mean / rstd [B, G] taken as exact inputs (that is
    the operation the kernel performs):
        y = xhat * gamma + beta,  dy = dA * sigmoid(y) * (1 + y * (1 - sigmoid(y)))  (dy = dA without the Swish)
        dgamma[c] = sum dy * xhat,  dbeta[c] = sum dy
        dx = rstd * (gamma * dy - mean_g(gamma * dy) - xhat * mean_g(gamma * dy * xhat))
    -> dict: dx [B, C, HW], dgamma, dbeta [C], T = |rs gamma dy| + |rs m1| + |rs xhat m2| per element, and per channel
       sum_abs_dy = sum |dy|, sum_abs_dyx = sum |dy * xhat| (over samples and positions)."""
    B, C, HW = x.shape
    Gn = mean32.shape[1]
    cpg = C // Gn
    xd, dAd = x.double(), dA.double()
    mu = mean32.double().repeat_interleave(cpg, 1)[:, :, None]
    rs = rstd32.double().repeat_interleave(cpg, 1)[:, :, None]
    ga, be = gamma.double()[None, :, None], beta.double()[None, :, None]
    xh = (xd - mu) * rs
    if swish:
        y = xh * ga + be
        sg = torch.sigmoid(y)
        dy = dAd * sg * (1.0 + y * (1.0 - sg))
    else:
        dy = dAd
    gdy = ga * dy
    m1 = gdy.view(B, Gn, -1).mean(-1).repeat_interleave(cpg, 1)[:, :, None]
    m2 = (gdy * xh).view(B, Gn, -1).mean(-1).repeat_interleave(cpg, 1)[:, :, None]
    return {"dx": rs * (gdy - m1 - xh * m2),
            "dgamma": (dy * xh).sum((0, 2)), "dbeta": dy.sum((0, 2)),
            "T": (rs * gdy).abs() + (rs * m1).abs().expand_as(xh) + (rs * xh * m2).abs(),
            "sum_abs_dy": dy.abs().sum((0, 2)), "sum_abs_dyx": (dy * xh).abs().sum((0, 2))}
