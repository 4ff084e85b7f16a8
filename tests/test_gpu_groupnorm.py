"""GroupNorm(32, C) kernels (csrc/groupnorm.hip, csrc/groupnorm_bwd.hip) against float64 at adverse statistics: a mean far
from zero, an outlier at the first element of a workgroup's slice (where zero-padded conv stacks put theirs, and where
gn_stats_kernel takes its pivot unless the element is atypical of the slice), zero variance, variance far below eps, several
partials per (sample, group) merged by Chan's formula, empty partials.  Inputs, references and gates:
tests/_groupnorm_cases.py; that fp32 can meet the forward gates is shown without a GPU in tests/test_groupnorm_cases_cpu.py.

Forward gates (every family x every shape, every entry point):
    |rstd - ref| <= 2e-5 ref,   |mean - ref| <= 2 * 2^-24 |ref| + 2e-5 std,
    |scale - ref| <= 2e-5 |ref| + 1e-30   and   |shift - ref| <= 3e-5 (|beta| + |mean * scale|)   per element.
Backward gates (the given fp32 mean / rstd are exact inputs of the reference, as they are of the kernel):
    |dx - ref| <= 5e-5 max T over the (sample, group), T = |rs gamma dy| + |rs m1| + |rs xhat m2|: groups are independent
        problems, so one loud group does not widen another's bound, and a reference that cancels to ~0 keeps its bound;
    |dbeta_c - ref| <= 64 * 2^-24 max_c sum |dy|,   |dgamma_c - ref| <= 64 * 2^-24 max_c sum |dy * xhat|
        (HW <= 8192, B <= 2: at most 32 adds on a thread's chain + eight tree levels + B, doubled for the product rounding;
        a worst-case count, not a measurement).
"""
import ctypes as C
import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _groupnorm_cases as GC  # noqa: E402
import hdiff_amd  # noqa: E402,F401
from hdiff_amd import _capi, autograd as A, engine as E  # noqa: E402

DEV = "cuda:0"
G, EPS = GC.G, GC.EPS


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def case(family, shape):
    """CPU tensors, computed once and shared (never modified): x [B, C, HW], gamma, beta, the float64 statistics"""
    C0, C1, HW, B, nsplit = shape
    Ct = C0 + C1
    x = GC.make_x(family, B, Ct, HW, seed=Ct + HW, nsplit=nsplit)
    gamma, beta = GC.make_affine(Ct, seed=Ct + HW)
    return x, gamma, beta, GC.ref_stats(x, G, EPS, gamma, beta)


def split_to_device(x, C0, C1):
    x0 = x[:, :C0].contiguous().to(DEV)
    x1 = x[:, C0:].contiguous().to(DEV) if C1 else None
    return x0, x1


def expected_counts(HW, nsplit, cpg):
    return [float(n * cpg) for _, n in GC.slices(HW, nsplit)]


def stats_then_finalize(x0, x1, gamma, beta, B, HW, nsplit):
    """hdiff_gn_stats + hdiff_gn_finalize -> mean, rstd, scale, shift, workspace"""
    lib = _capi.lib()
    C0, C1 = x0.shape[1], 0 if x1 is None else x1.shape[1]
    Ct = C0 + C1
    ws = torch.full((B * G * nsplit * 3,), 7.0, device=DEV)      # a stale count of an empty slice would enter the merge
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    mean, rstd, scale, shift = nan(B, G), nan(B, G), nan(B, Ct), nan(B, Ct)
    _capi.check(lib.hdiff_gn_stats(_ptr(x0), _ptr(x1), C0, C1, B, HW, G, nsplit, ws.data_ptr(), _stream()), "gn_stats")
    _capi.check(lib.hdiff_gn_finalize(ws.data_ptr(), B, Ct, G, nsplit, gamma.data_ptr(), beta.data_ptr(), C.c_float(EPS),
                                      scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), rstd.data_ptr(), _stream()),
                "gn_finalize")
    torch.cuda.synchronize()
    return mean, rstd, scale, shift, ws


def one_call_scale_shift(x0, x1, gamma, beta, B, HW, nsplit):
    """hdiff_gn_scale_shift: the fused finalize when nsplit == 1, else the streaming pass + the merge kernel"""
    lib = _capi.lib()
    C0, C1 = x0.shape[1], 0 if x1 is None else x1.shape[1]
    Ct = C0 + C1
    ws = torch.full((B * G * nsplit * 3,), 7.0, device=DEV)
    scale, shift = torch.full((B, Ct), float("nan"), device=DEV), torch.full((B, Ct), float("nan"), device=DEV)
    _capi.check(lib.hdiff_gn_scale_shift(_ptr(x0), _ptr(x1), C0, C1, B, HW, G, nsplit, ws.data_ptr(), gamma.data_ptr(),
                                         beta.data_ptr(), C.c_float(EPS), scale.data_ptr(), shift.data_ptr(), _stream()),
                "gn_scale_shift")
    torch.cuda.synchronize()
    return scale, shift


def plan_scale_shift(x0, x1, gamma, beta, B, HW):
    plan = E.Plan(DEV)
    sc, sh = plan.gn_scale_shift(x0, x1, gamma, beta, B, HW)
    plan.run()
    torch.cuda.synchronize()
    return sc.clone(), sh.clone()


@pytest.mark.parametrize("shape", GC.SHAPES, ids=GC.shape_id)
@pytest.mark.parametrize("family", GC.FAMILIES)
def test_forward_statistics_against_float64(family, shape):
    """Every entry point on every family x shape.  While gn_stats_kernel took the slice's first element as its pivot without
    checking it against the rest of the slice, the `pivot-spike` families missed the rstd gate at every shape with >= 768
    elements per group, worst |rstd - ref| / ref = 1.57e-3 (pivot-spike-3000, C128+0-HW4096-B1-ns1).

    While a split could be as short as one float4 of a plane, `offset` and `neg-offset` also missed it wherever several
    short partials were merged: 4.96e-5 (offset, HW 100, 3 splits), 2.04e-4 (offset, HW 8, 4 splits), 3.91e-5 and 5.03e-5
    (offset, HW 99, 3 and 2 splits), 2.39e-5 (neg-offset, HW 8, 4 splits), all measured on the MI355X.  A partial's mean is
    one fp32 number, and its rounding (half an ulp of 100 = 3.8e-6, against a standard deviation of 0.01) enters Chan's merge
    as 2 n_s (mean_s - mean) * rounding: (|mean| / std) * 2^-24 / sqrt(n_s) of the variance.  A split now covers at least 4096
    elements of a plane (GC.MIN_SLICE), the shortest the planner makes; there the same family is at 3.1e-6."""
    C0, C1, HW, B, nsplit = shape
    Ct, cpg = C0 + C1, (C0 + C1) // G
    x, gamma, beta, ref = case(family, shape)
    x0, x1 = split_to_device(x, C0, C1)
    d_gamma, d_beta = gamma.to(DEV), beta.to(DEV)
    got = {}
    mean, rstd, scale, shift, ws = stats_then_finalize(x0, x1, d_gamma, d_beta, B, HW, nsplit)
    got["gn_stats + gn_finalize"] = (mean, rstd, scale, shift)
    # every partial carries its element count, the empty ones 0
    counts = ws.view(B * G, nsplit, 3)[:, :, 0].cpu()
    assert counts.eq(torch.tensor(expected_counts(HW, nsplit, cpg))[None]).all(), counts[0]
    sc1, sh1 = one_call_scale_shift(x0, x1, d_gamma, d_beta, B, HW, nsplit)
    got["gn_scale_shift"] = (None, None, sc1, sh1)
    assert torch.equal(sc1, scale) and torch.equal(sh1, shift), "the two launch forms differ in bits"
    if nsplit == GC.product_nsplit(HW):                           # the shape as the product runs it
        got["Plan.gn_scale_shift"] = (None, None) + plan_scale_shift(x0, x1, d_gamma, d_beta, B, HW)
        sc3, sh3, mean3, rstd3 = A._gn_stats(x0, x1, d_gamma, d_beta, B, HW)
        torch.cuda.synchronize()
        got["autograd._gn_stats"] = (mean3, rstd3, sc3, sh3)
    failures = []
    for name, res in got.items():
        fails, ratios = GC.forward_gate_report(tuple(None if t is None else t.cpu() for t in res), ref, beta,
                                               constant=family == "constant")
        print(f"{family} {GC.shape_id(shape)} {name}: worst error / bound " +
              ", ".join(f"{k} {v:.3g}" for k, v in ratios.items() if k != "rstd_rel") +
              (f"; worst |rstd - ref| / ref {ratios['rstd_rel']:.3e}" if "rstd_rel" in ratios else ""))
        failures += [f"{name}: {f}" for f in fails]
    assert not failures, failures


@pytest.mark.parametrize("shape", [(128, 0, 1024, 2, 1), (256, 128, 64, 2, 1), (32, 0, 8192, 2, 2)], ids=GC.shape_id)
@pytest.mark.parametrize("family", ["benign", "offset", "pivot-spike-3000"])
def test_statistics_of_a_sample_do_not_depend_on_the_batch(family, shape):
    """Sample 1 of a batch of two and the same sample alone: the same bits, with one partial per (sample, group) and with two."""
    C0, C1, HW, B, nsplit = shape
    assert nsplit == GC.product_nsplit(HW)
    x, gamma, beta, _ = case(family, shape)
    d_gamma, d_beta = gamma.to(DEV), beta.to(DEV)
    x0, x1 = split_to_device(x, C0, C1)
    y0, y1 = split_to_device(x[1:2], C0, C1)
    both = stats_then_finalize(x0, x1, d_gamma, d_beta, 2, HW, nsplit)[:4]
    alone = stats_then_finalize(y0, y1, d_gamma, d_beta, 1, HW, nsplit)[:4]
    for name, a, b in zip(("mean", "rstd", "scale", "shift"), both, alone):
        assert torch.isfinite(b).all() and torch.equal(a[1:2], b), name
    for name, a, b in zip(("scale", "shift"), one_call_scale_shift(x0, x1, d_gamma, d_beta, 2, HW, nsplit),
                          one_call_scale_shift(y0, y1, d_gamma, d_beta, 1, HW, nsplit)):
        assert torch.equal(a[1:2], b) and torch.equal(b, alone[2 if name == "scale" else 3]), name
    for name, a, b in zip(("scale", "shift", "mean", "rstd"), A._gn_stats(x0, x1, d_gamma, d_beta, 2, HW),
                          A._gn_stats(y0, y1, d_gamma, d_beta, 1, HW)):
        assert torch.equal(a[1:2], b), ("autograd", name)
    for name, a, b in zip(("scale", "shift"), plan_scale_shift(x0, x1, d_gamma, d_beta, 2, HW),
                          plan_scale_shift(y0, y1, d_gamma, d_beta, 1, HW)):
        assert torch.equal(a[1:2], b), ("Plan", name)


def run_gn_bwd(kind, x0, x1, dA, mean, rstd, gamma, beta, B, HW):
    """kind 'swish': hdiff_gn_swish_bwd on the (virtual concat) input; 'affine': hdiff_gn_affine_bwd on one tensor"""
    lib = _capi.lib()
    C0, C1 = x0.shape[1], 0 if x1 is None else x1.shape[1]
    Ct = C0 + C1
    ws = torch.full((2 * B * Ct + 2 * B * G,), float("nan"), device=DEV)
    dx0 = torch.full_like(x0, float("nan"))
    dx1 = None if x1 is None else torch.full_like(x1, float("nan"))
    dgamma, dbeta = torch.full((Ct,), float("nan"), device=DEV), torch.full((Ct,), float("nan"), device=DEV)
    if kind == "swish":
        _capi.check(lib.hdiff_gn_swish_bwd(_ptr(x0), _ptr(x1), C0, C1, B, HW, G, dA.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                           gamma.data_ptr(), beta.data_ptr(), ws.data_ptr(), _ptr(dx0), _ptr(dx1),
                                           dgamma.data_ptr(), dbeta.data_ptr(), _stream()), "gn_swish_bwd")
    else:
        assert x1 is None
        _capi.check(lib.hdiff_gn_affine_bwd(_ptr(x0), Ct, B, HW, G, dA.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                            gamma.data_ptr(), beta.data_ptr(), ws.data_ptr(), _ptr(dx0), dgamma.data_ptr(),
                                            dbeta.data_ptr(), _stream()), "gn_affine_bwd")
    torch.cuda.synchronize()
    dx = dx0 if dx1 is None else torch.cat([dx0, dx1], 1)
    return dx.cpu().double(), dgamma.cpu().double(), dbeta.cpu().double()


@pytest.mark.parametrize("shape", GC.BWD_SHAPES, ids=GC.shape_id)
@pytest.mark.parametrize("family", GC.BWD_FAMILIES)
@pytest.mark.parametrize("da_kind", GC.DA_KINDS)
def test_backward_against_float64(da_kind, family, shape):
    C0, C1, HW, B, _ = shape
    Ct, cpg = C0 + C1, (C0 + C1) // G
    x, gamma, beta, ref = case(family, shape)
    if da_kind == "ones":
        gamma, _ = GC.make_affine(Ct, seed=0, equal_gamma=True)   # equal gamma: the affine dx cancels to ~0
    dA = GC.make_dA(da_kind, B, Ct, HW, seed=Ct + HW)
    mean32, rstd32 = ref["mean"].float(), ref["rstd"].float()     # the statistics, rounded to what the kernel is handed
    dev = lambda t: t.contiguous().to(DEV)
    d_dA, d_mean, d_rstd, d_gamma, d_beta = dev(dA), dev(mean32), dev(rstd32), dev(gamma), dev(beta)
    failures = []
    for kind in ("swish", "affine"):
        want = GC.ref_bwd(x, dA, mean32, rstd32, gamma, beta, swish=kind == "swish")
        x0, x1 = split_to_device(x, C0, C1) if kind == "swish" else (x.to(DEV), None)
        dx, dgamma, dbeta = run_gn_bwd(kind, x0, x1, d_dA, d_mean, d_rstd, d_gamma, d_beta, B, HW)
        t_max = want["T"].view(B, G, cpg * HW).amax(-1)            # per (sample, group)
        bound_dx = (5e-5 * t_max).repeat_interleave(cpg, 1)[:, :, None]
        err_dx = (dx - want["dx"]).abs()
        bound_b = 64 * GC.U * want["sum_abs_dy"].max().item()
        bound_g = 64 * GC.U * want["sum_abs_dyx"].max().item()
        err_b, err_g = (dbeta - want["dbeta"]).abs().max().item(), (dgamma - want["dgamma"]).abs().max().item()
        worst_dx = (err_dx / bound_dx.clamp_min(1e-300)).max().item()
        print(f"{kind} {family} {da_kind} {GC.shape_id(shape)}: dx worst error / bound {worst_dx:.3g} (max |dx ref| "
              f"{want['dx'].abs().max().item():.3e}, max T {t_max.max().item():.3e}), dbeta {err_b:.3e} / {bound_b:.3e}, "
              f"dgamma {err_g:.3e} / {bound_g:.3e}")
        if not (torch.isfinite(dx).all() and torch.isfinite(dgamma).all() and torch.isfinite(dbeta).all()):
            failures.append(f"{kind}: not finite")
            continue
        if not (err_dx <= bound_dx).all():
            failures.append(f"{kind}: dx error {worst_dx:.3g} x the bound")
        if not err_b <= bound_b:
            failures.append(f"{kind}: dbeta error {err_b:.3e} > {bound_b:.3e}")
        if not err_g <= bound_g:
            failures.append(f"{kind}: dgamma error {err_g:.3e} > {bound_g:.3e}")
    assert not failures, failures


@pytest.mark.parametrize("offset", [0.0, 1000.0])
@pytest.mark.parametrize("Cc", [3, 40])
@pytest.mark.parametrize("HW", [25, 64, 1024])
def test_bias_addvec_grad_both_routes(HW, Cc, offset):
    """hdiff_bias_addvec_grad with dvec (one workgroup per plane, then the sum over the batch) and without (one kernel that
    walks the batch) against float64 sums, each output within 64 * 2^-24 of the sum of its terms' magnitudes; the two routes
    add in different orders, so their dbias agree within that bound, not in bits."""
    B = 3
    g = torch.Generator().manual_seed(HW + Cc)
    dy = (offset + torch.randn(B, Cc, HW, generator=g)).float()
    d_dy = dy.to(DEV)
    lib = _capi.lib()
    dvec, dbias_a, dbias_b = (torch.full(s, float("nan"), device=DEV) for s in ((B, Cc), (Cc,), (Cc,)))
    _capi.check(lib.hdiff_bias_addvec_grad(d_dy.data_ptr(), B, Cc, HW, dvec.data_ptr(), dbias_a.data_ptr(), _stream()), "planes")
    _capi.check(lib.hdiff_bias_addvec_grad(d_dy.data_ptr(), B, Cc, HW, None, dbias_b.data_ptr(), _stream()), "single")
    torch.cuda.synchronize()
    want_vec, mag_vec = dy.double().sum(-1), dy.double().abs().sum(-1)
    want_bias, mag_bias = want_vec.sum(0), mag_vec.sum(0)
    dvec, dbias_a, dbias_b = dvec.cpu().double(), dbias_a.cpu().double(), dbias_b.cpu().double()
    k = 64 * GC.U
    print(f"bias_addvec_grad HW {HW} C {Cc} offset {offset}: error / bound: dvec {((dvec - want_vec).abs() / (k * mag_vec)).max():.3g}, "
          f"dbias (planes) {((dbias_a - want_bias).abs() / (k * mag_bias)).max():.3g}, "
          f"dbias (single) {((dbias_b - want_bias).abs() / (k * mag_bias)).max():.3g}, "
          f"between routes {((dbias_a - dbias_b).abs() / (k * mag_bias)).max():.3g}")
    assert ((dvec - want_vec).abs() <= k * mag_vec).all()
    assert ((dbias_a - want_bias).abs() <= k * mag_bias).all()
    assert ((dbias_b - want_bias).abs() <= k * mag_bias).all()
    assert ((dbias_a - dbias_b).abs() <= k * mag_bias).all()
