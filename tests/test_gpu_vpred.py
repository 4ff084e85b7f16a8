"""GPU: v-prediction and min-SNR weighting in the image-conditioned tree against their definition (tests/_vpred_def.py) -- the loss
tail ``hdiff_train_b_tail_fwd / _bwd`` in every combination of its three arguments, the sampler's conversion ``hdiff_v_to_eps`` bit
for bit, the trainer's five terms on the small DynamicUNet, every sampling loop of a ``prediction="v"`` sampler against its CPU loop,
the launch lists, and the training / evaluation drivers.

The gates of the tail are those of ``test_loss_tail_kernel_against_float64_torch`` (tests/test_gpu_train_b.py).  The gate of the loop
tests is not a constant: the unchanged eps sampler's own trajectory error against ``oracle.cpu_path_b.sampler_forward`` is measured on
the same fixture (``_gate_b`` of tests/test_gpu_dpmpp.py, shared and computed once), and a v loop may show ``max(2 * e_ddim, FLOOR)``
against ITS CPU loop -- the conversion adds two roundings per element and step.  Both figures are printed before the assertion; the
values measured on an MI355X are in profiles/vpred.txt."""
import ctypes as C
import functools
import os
import shutil
import types

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning"), pytest.mark.filterwarnings("ignore::UserWarning")]

import hdiff_amd  # noqa: E402,F401
from hdiff_amd import _capi  # noqa: E402
from hdiff_amd import autograd as AG  # noqa: E402
from hdiff_amd.diffusion import Diffusion as DD  # noqa: E402
from hdiff_amd.diffusion import Evaluate as EV  # noqa: E402
from hdiff_amd.diffusion import Train as TR  # noqa: E402
from oracle import cpu_path_b as OB  # noqa: E402

import _dpmpp_def as PD  # noqa: E402
import _posterior_def as PO  # noqa: E402
import _tiled_def as TD  # noqa: E402
import _vpred_def as V  # noqa: E402
import test_gpu_dpmpp as DP  # noqa: E402      (the small model, the loop inputs and the eps sampler's own error: built once, shared)
from test_gpu_train_b_driver import as_is, config, data_root, load  # noqa: E402,F401

DEV = "cuda:0"
GAMMA = 5.0
SENTINEL = 777.0


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return (got - ref).abs().max().item() / (ref.abs().max().item() + 1e-12)


@functools.lru_cache(maxsize=None)
def _tables():
    betas, ab = V.schedule()
    sa32, s1m32 = V.tables32(ab)
    w = {p: V.weights(ab, GAMMA, p).float() for p in ("eps", "v")}
    return betas, ab, sa32, s1m32, w


# ----------------------------------------------------------------------------------------------------------------------
# 1. the loss tail
# ----------------------------------------------------------------------------------------------------------------------
TAIL_SHAPES = {(2, 5, 7): [3, 870], (3, 9, 29): [0, 499, 999]}       # 783 pixels: three whole workgroups of 256 and a ragged one


@functools.lru_cache(maxsize=None)
def _tail_inputs(shape):
    """out, noise, y_t, gt, t and three incoming gradients on the CPU; zero, tiny and zero-gt pixels planted as in
    test_loss_tail_kernel_against_float64_torch (both eps branches of F.normalize / cosine_similarity)."""
    B, H, W = shape
    g = torch.Generator().manual_seed(B * 100 + H)
    out = torch.randn(B, 3, H, W, generator=g)
    noise = torch.randn(B, 3, H, W, generator=g)
    y_t = torch.randn(B, 3, H, W, generator=g)
    gt = torch.rand(B, 3, H, W, generator=g) * 2 - 1
    out[0, :, 0, 0] = 0.0; y_t[0, :, 0, 0] = 0.0
    out[0, :, 0, 1] = 0.0; y_t[0, :, 0, 1] = torch.tensor([1e-15, -2e-15, 3e-15])
    out[0, :, 0, 2] = 0.0; y_t[0, :, 0, 2] = torch.tensor([1e-21, 2e-21, -1e-21])
    out[1, :, 1, 1] = 0.0; y_t[1, :, 1, 1] = torch.tensor([1e-9, 1e-9, -2e-9])
    gt[1, :, 2, 3] = 0.0
    t = torch.tensor(TAIL_SHAPES[shape])
    d_mse = torch.randn(out.shape, generator=g)
    d_y0 = torch.randn(out.shape, generator=g) * 10
    return out, noise, y_t, gt, t, d_mse, d_y0, torch.tensor(0.7)


def _run_tail(entry, out, noise, y_t, gt, t, sa, s1m, d_mse, d_y0, d_col, prediction="eps", w=None, div=255.0):
    """``entry``: "tail" (the new pair, with the three arguments) or "loss" (the pair from before them).  Device tensors in, device
    tensors out: (mse, y0, col, d_out)."""
    lib, s = _capi.lib(), _stream()
    B, _, H, W = out.shape
    mse, y0, col = torch.empty_like(out), torch.empty_like(out), torch.empty((), device=DEV)
    nb = C.c_int64(0)
    _capi.check(lib.hdiff_train_b_loss_workspace(B * H * W, C.byref(nb)))
    ws = torch.empty(nb.value // 4, device=DEV)
    d = torch.empty_like(out)
    ptr = lambda x: None if x is None else x.data_ptr()                                          # noqa: E731
    rest = (gt.data_ptr(), t.data_ptr(), sa.data_ptr(), s1m.data_ptr(), 1000, B, H * W)
    fwd = (out.data_ptr(), noise.data_ptr(), y_t.data_ptr()) + rest + (mse.data_ptr(), y0.data_ptr(), col.data_ptr(), ws.data_ptr())
    bwd = (out.data_ptr(), noise.data_ptr(), y0.data_ptr()) + rest + (ptr(d_mse), ptr(d_y0), ptr(d_col), d.data_ptr())
    if entry == "loss":
        _capi.check(lib.hdiff_train_b_loss_fwd(*fwd, s), "train_b_loss_fwd")
        _capi.check(lib.hdiff_train_b_loss_bwd(*bwd, s), "train_b_loss_bwd")
    else:
        extra = (AG.PREDICTION_CODES[prediction], ptr(w), C.c_float(div))
        _capi.check(lib.hdiff_train_b_tail_fwd(*fwd, *extra, s), "train_b_tail_fwd")
        _capi.check(lib.hdiff_train_b_tail_bwd(*bwd, *extra, s), "train_b_tail_bwd")
    torch.cuda.synchronize()
    return mse, y0, col, d


@pytest.mark.parametrize("weighting", [None, "min_snr"])
@pytest.mark.parametrize("prediction", ["eps", "v"])
@pytest.mark.parametrize("shape", list(TAIL_SHAPES))
def test_tail_kernels_against_the_float64_definition(shape, prediction, weighting):
    """mse and y0 within 1e-6 relative, col within 1e-6, d_out within 1e-4 |want| + 1e-5 median |want| of the definition, at both
    divisors and with each incoming gradient absent in turn; the colour term and its gradient start from the kernel's own y0."""
    _, _, sa32, s1m32, wtab = _tables()
    out, noise, y_t, gt, t, d_mse, d_y0, d_col = _tail_inputs(shape)
    w32 = wtab[prediction] if weighting else None
    dev = lambda x: None if x is None else x.to(DEV)                                             # noqa: E731
    fixed = [x.to(DEV) for x in (out, noise, y_t, gt, t, sa32, s1m32)]
    for div in (255.0, 1.0):
        want = V.tail(prediction, out, noise, y_t, gt, t, sa32, s1m32, w32, div)
        for absent in (None, "d_mse", "d_y0", "d_col"):
            grads = {"d_mse": d_mse, "d_y0": d_y0, "d_col": d_col}
            if absent:
                grads[absent] = None
            mse, y0, col, got = _run_tail("tail", *fixed, *(dev(grads[k]) for k in ("d_mse", "d_y0", "d_col")), prediction, dev(w32), div)
            tag = (shape, prediction, weighting, div, absent)
            e_mse, e_y0 = _rel(mse, want["mse"]), _rel(y0, want["y0"])
            col64, _ = V.colour(y0, gt)
            want_d = V.d_out(prediction, out, noise, y_t, gt, t, sa32, s1m32, w32, div, y0, *(grads[k] for k in ("d_mse", "d_y0", "d_col")))
            err = (got.cpu().double() - want_d).abs()
            tol = 1e-4 * want_d.abs() + 1e-5 * want_d.abs().median()
            print(f"{tag}: mse {e_mse:.2e}  y0 {e_y0:.2e}  col {abs(col.item() - col64.item()):.2e}  d_out worst err/tol "
                  f"{(err / tol.clamp_min(1e-300)).max().item():.2e}")
            assert e_mse < 1e-6 and e_y0 < 1e-6, tag
            assert abs(col.item() - col64.item()) < 1e-6, tag
            assert not (err > tol).any(), tag
            assert (y0[0, :, 0, 0] == 0).all()
            if absent is None and div == 255.0:
                assert want_d[0, :, 0, 1].abs().min() > 1e3          # the tiny pixels really carry the large eps-branch gradients
        if weighting:                                                # the weight reached the mse term, and that term alone
            plain = V.tail(prediction, out, noise, y_t, gt, t, sa32, s1m32, None, div)
            assert torch.equal(plain["y0"], want["y0"]) and not torch.equal(plain["mse"], want["mse"])


def test_tail_bits():
    """In v mode at y0_div = 1, y0 is the fp32 expression a * y_t - s * out (two products, one difference) bit for bit; with the three
    arguments at their defaults the new entry points give the bits of the old ones on all four outputs; two runs are identical."""
    _, _, sa32, s1m32, wtab = _tables()
    for shape in TAIL_SHAPES:
        out, noise, y_t, gt, t, d_mse, d_y0, d_col = _tail_inputs(shape)
        dev = [x.to(DEV) for x in (out, noise, y_t, gt, t, sa32, s1m32, d_mse, d_y0, d_col)]
        _, y0, _, _ = _run_tail("tail", *dev, "v", None, 1.0)
        assert torch.equal(y0.cpu().view(torch.int32), V.v_y0_fp32(out, y_t, t, sa32, s1m32).view(torch.int32)), shape
        old = _run_tail("loss", *dev)
        new = _run_tail("tail", *dev, "eps", None, 255.0)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(old, new)), shape
        for prediction, w, div in (("v", wtab["v"].to(DEV), 255.0), ("eps", wtab["eps"].to(DEV), 1.0)):
            one = _run_tail("tail", *dev, prediction, w, div)
            two = _run_tail("tail", *dev, prediction, w, div)
            assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(one, two)), (shape, prediction)


def test_autograd_tail_reaches_the_new_entry_points_only_when_asked():
    """``train_b_loss_tail`` with the three arguments at their defaults returns the bits of the call without them (the old pair);
    with any of them set it returns the new pair's."""
    _, _, sa32, s1m32, wtab = _tables()
    out, noise, y_t, gt, t, d_mse, d_y0, d_col = (x.to(DEV) for x in _tail_inputs((2, 5, 7)))
    sa, s1m = sa32.to(DEV), s1m32.to(DEV)

    def run(**kw):
        o = out.clone().requires_grad_(True)
        mse, y0, col = AG.train_b_loss_tail(o, noise, y_t, gt, t, sa, s1m, **kw)
        ((mse * d_mse).sum() + (y0 * d_y0).sum() + col * d_col).backward()
        return mse.detach(), y0.detach(), col.detach(), o.grad

    plain, defaults = run(), run(prediction="eps", weight_tab=None, y0_div=255.0)
    assert all(torch.equal(a, b) for a, b in zip(plain, defaults))
    assert all(torch.equal(a, b) for a, b in zip(plain, _run_tail("loss", out, noise, y_t, gt, t, sa, s1m, d_mse, d_y0, d_col)))
    w = wtab["v"].to(DEV)
    assert all(torch.equal(a, b) for a, b in zip(run(prediction="v", weight_tab=w, y0_div=1.0),
                                                 _run_tail("tail", out, noise, y_t, gt, t, sa, s1m, d_mse, d_y0, d_col, "v", w, 1.0)))


# ----------------------------------------------------------------------------------------------------------------------
# 2. hdiff_v_to_eps
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_per", [105, 3 * 16 * 16, 3 * 24 * 44])      # 105 = 3 * 5 * 7: odd, rows start off the 16-byte grid
def test_v_to_eps_bit_for_bit(n_per):
    _, _, sa32, s1m32, _ = _tables()
    g = torch.Generator().manual_seed(n_per)
    out, y = torch.randn(3, n_per, generator=g), torch.randn(3, n_per, generator=g)
    out[1, n_per // 2] = float("nan")
    t = torch.tensor([0, 499, 999])
    want = V.v_to_eps_fp32(out, y, t, sa32, s1m32)
    assert bool(torch.isnan(want[1, n_per // 2])) and int(torch.isnan(want).sum()) == 1
    sa, s1m, td = sa32.to(DEV), s1m32.to(DEV), t.to(DEV)
    for pad in (8, 5):                          # a 16-byte aligned base (quads) and one that is only 4-byte aligned (element by element)
        buf = torch.full((3 * n_per + 2 * pad,), SENTINEL, device=DEV)
        o = buf[pad:pad + 3 * n_per].view(3, n_per)
        o.copy_(out)
        ybuf = torch.full((3 * n_per + 2 * pad,), SENTINEL, device=DEV)
        yd = ybuf[pad:pad + 3 * n_per].view(3, n_per)
        yd.copy_(y)
        _capi.check(_capi.lib().hdiff_v_to_eps(o.data_ptr(), yd.data_ptr(), td.data_ptr(), sa.data_ptr(), s1m.data_ptr(), 1000, 3, n_per,
                                               _stream()), "v_to_eps")
        torch.cuda.synchronize()
        got = o.cpu()
        same = (got.view(torch.int32) == want.view(torch.int32)) | (torch.isnan(got) & torch.isnan(want))
        assert bool(same.all()), (n_per, pad, int((~same).sum()))
        assert int(torch.isnan(got).sum()) == 1, "a NaN stays in its own element"
        assert bool((buf[:pad] == SENTINEL).all()) and bool((buf[pad + 3 * n_per:] == SENTINEL).all()), (n_per, pad)
        assert torch.equal(yd.cpu(), y), "y is read only"


# ----------------------------------------------------------------------------------------------------------------------
# 3. the trainer
# ----------------------------------------------------------------------------------------------------------------------
def _pos_a(y0, gt):
    """Stand-ins for the two callables (sums of non-negative terms: no cancellation in their fp32 means); their gradient reaches the
    model through y_0_pred."""
    return ((y0 - gt) ** 2).mean() * 40.0


def _pos_b(y0, gt):
    return ((y0 * 255.0 - gt) ** 2).mean() * 0.1


def _trainer_batch():
    g = torch.Generator().manual_seed(31)
    gt = torch.randint(0, 256, (2, 3, 16, 16), generator=g).float()
    inp = torch.randint(0, 256, (2, 3, 16, 16), generator=g).float()
    return gt, inp, torch.tensor([100, 870]), torch.randn(2, 3, 16, 16, generator=g)


def _grads(m):
    return {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in m.named_parameters()}


def test_trainer_v_min_snr_terms_and_gradients():
    """The five returned terms of prediction="v", loss_weighting="min_snr" against the definition applied to the model's own output.
    mse and col under the tail's gates; the two stand-in terms are fp32 means of 1536 non-negative values of a y0 that is itself
    within 1e-6 (relative to its largest value) of the definition's: 2e-6 from y0 entering squared plus 11 * 2^-24 from the pairwise
    sum, gated at 1e-5 relative; ``loss`` is their sum, gated the same way."""
    _, _, sa32, s1m32, wtab = _tables()
    m = DP._small_b()[0].train()
    try:
        gt, inp, t, noise = _trainer_batch()
        seen = []
        hook = m.register_forward_hook(lambda mod, args, out: seen.append(out.detach().cpu()))
        kw = dict(dino_loss=_pos_a, msssim_loss=_pos_b)
        tr = DD.GaussianDiffusionTrainer(m, V.B1, V.BT, V.T, prediction="v", loss_weighting="min_snr", snr_gamma=GAMMA, **kw).to(DEV)
        m.zero_grad(set_to_none=True)
        terms = tr(gt.to(DEV), inp.to(DEV), 0, t=t.to(DEV), noise=noise.to(DEV), context_zero=True)
        hook.remove()
        terms[0].mean().backward()
        g_v = _grads(m)
        eps_tr = DD.GaussianDiffusionTrainer(m, V.B1, V.BT, V.T, **kw).to(DEV)
        m.zero_grad(set_to_none=True)
        eps_tr(gt.to(DEV), inp.to(DEV), 0, t=t.to(DEV), noise=noise.to(DEV), context_zero=True)[0].mean().backward()
        g_eps = _grads(m)
    finally:
        m.eval()
        m.zero_grad(set_to_none=True)
    (out,) = seen
    gt1 = (gt / 255.0) * 2 - 1
    a, s = sa32[t].view(-1, 1, 1, 1), s1m32[t].view(-1, 1, 1, 1)
    y_t = a * gt1 + s * noise                                            # q_sample, fp32 as the kernel forms it
    want = V.tail("v", out, noise, y_t, gt1, t, sa32, s1m32, wtab["v"], 255.0)
    loss, mse, dino, msssim, col = (v.detach().cpu() for v in terms)
    col64, _ = V.colour(want["y0"].float(), gt1)
    dino64, ms64 = _pos_a(want["y0"], gt1.double()) * 0.5, _pos_b(want["y0"], gt1.double()) * 0.0045
    loss64 = want["mse"] + dino64 + ms64 + col64
    figures = dict(mse=_rel(mse, want["mse"]), col=abs(col.item() - col64.item()), dino=abs(dino.item() - dino64.item()) / dino64.item(),
                   msssim=abs(msssim.item() - ms64.item()) / ms64.item(), loss=_rel(loss, loss64))
    print("trainer v + min_snr vs the definition: " + "  ".join(f"{k} {v:.2e}" for k, v in figures.items()))
    assert tuple(loss.shape) == tuple(mse.shape) == (2, 3, 16, 16) and col.dim() == 0
    assert figures["mse"] < 1e-6 and figures["col"] < 1e-6
    assert figures["dino"] < 1e-5 and figures["msssim"] < 1e-5 and figures["loss"] < 1e-5
    # the v weights are below 1 everywhere (gamma / (snr + 1) at t = 100, snr / (snr + 1) at t = 870): not the unweighted map
    assert _rel(mse, V.tail("v", out, noise, y_t, gt1, t, sa32, s1m32, None, 255.0)["mse"]) > 1e-2
    have = [n for n, g in g_eps.items() if g is not None]
    assert have and all(g_v[n] is not None and bool(torch.isfinite(g_v[n]).all()) for n in have)
    assert any(not torch.equal(g_v[n], g_eps[n]) for n in have)


def test_trainer_with_the_arguments_at_their_defaults_is_the_trainer_without_them():
    m = DP._small_b()[0].train()
    try:
        gt, inp, t, noise = (x.to(DEV) for x in _trainer_batch())
        runs = []
        for kw in ({}, dict(prediction="eps", loss_weighting=None, snr_gamma=5.0, y0_divisor=255.0)):
            tr = DD.GaussianDiffusionTrainer(m, V.B1, V.BT, V.T, dino_loss=_pos_a, msssim_loss=_pos_b, **kw).to(DEV)
            m.zero_grad(set_to_none=True)
            terms = tr(gt, inp, 0, t=t, noise=noise, context_zero=True)
            terms[0].mean().backward()
            runs.append(([v.detach().clone() for v in terms], _grads(m)))
    finally:
        m.eval()
        m.zero_grad(set_to_none=True)
    (terms_a, grads_a), (terms_b, grads_b) = runs
    assert all(torch.equal(a, b) for a, b in zip(terms_a, terms_b))
    assert list(grads_a) == list(grads_b)
    for n in grads_a:
        assert (grads_a[n] is None) == (grads_b[n] is None) and (grads_a[n] is None or torch.equal(grads_a[n], grads_b[n])), n


# ----------------------------------------------------------------------------------------------------------------------
# 4. the sampling loops of a v sampler
# ----------------------------------------------------------------------------------------------------------------------
S, TILE, OVERLAP = DP.DDIM_STEP, DP.TILE, DP.OVERLAP
TAU = list(range(0, 1000, 1000 // S))
ETA = 0.5


def _sampler_v(T=V.T):
    return DD.GaussianDiffusionSampler(DP._small_b()[0], V.B1, V.BT, T, prediction="v").to(DEV)


def _model_eps(T=V.T):
    """The small DynamicUNet on the CPU (the oracle's forward) read as a v network, as the reference-shaped ``model_eps(x6, t)``."""
    _, ocfg, sd = DP._small_b()
    sa32, s1m32 = V.tables32(V.schedule(n=T)[1])
    return V.as_eps_model(lambda x6, t: OB.dyn_unet_forward(sd, ocfg, x6, t), sa32, s1m32)


def _names(samp):
    return [op[0] for op in next(iter(samp._plans.values())).plan.ops]


def _randn(n, seed, offset):
    out = torch.empty(n, device=DEV)
    _capi.check(_capi.lib().hdiff_randn(out.data_ptr(), n, C.c_uint64(seed), C.c_uint64(offset), _stream()), "randn")
    return out


def _report(path, e, limit, e_ddim):
    print(f"tree B v sampler, {path}: eps sampler vs oracle {e_ddim:.3e}   v loop vs its CPU loop {e:.3e}   gate {limit:.3e}")


def test_v_ddim_and_dpmpp_loops_graph_and_one_window():
    img, y_T = DP._inputs_b(24, 40)
    limit, e_ddim = DP._gate_b()
    ab = V.schedule()[1]
    samp = _sampler_v()
    d_img, d_y = img.to(DEV), y_T.to(DEV)
    tau_l = PD.logsnr_steps(DP.BETAS, S, 1)
    tab = PD.table(DP.BETAS, tau_l, 1, float(PD.alphas_bar(DP.BETAS)[0])).float()
    with torch.no_grad():
        refs = {"ddim": V.ddim_loop(_model_eps(), img / 255.0, y_T, ab, TAU),
                "dpmpp2m": V.dpmpp_loop(_model_eps(), img / 255.0, y_T, tau_l, tab, PD.update)}
        for solver in ("ddim", "dpmpp2m"):
            kw = dict(ddim=True, ddim_step=S, y_T=d_y, solver=solver)
            got, got_w = [], []
            eager = samp(d_img, trajectory=got, **kw)
            graph = samp(d_img, **kw)
            assert next(iter(samp._plans.values())).plan.graph.value, "the second call replays a captured step"
            one_window = samp(d_img, trajectory=got_w, tile=64, **kw)
            e = DP._traj_error(got, refs[solver])
            _report(f"{solver} 24x40", e, limit, e_ddim)
            assert e <= limit, (solver, e, limit)
            assert torch.equal(eager.cpu(), torch.clip(got[-1].cpu(), -1, 1))
            assert torch.equal(graph, eager), "hipGraph replay and eager launches must agree bit for bit"
            assert torch.equal(one_window, eager) and all(torch.equal(a, b) for a, b in zip(got_w, got)), "one window is the untiled path"
        # the conversion is not a no-op: the eps sampler on the same weights goes elsewhere from the first step on
        eps_first = []
        DP._sampler_b()(d_img, ddim=True, ddim_step=S, y_T=d_y, trajectory=eps_first)
        assert DP._traj_error(eps_first, refs["ddim"]) > 1e-2


def test_v_eta_loop_with_a_seed_and_posterior():
    img, y_T = DP._inputs_b(24, 40)
    limit, e_ddim = DP._gate_b()
    ab = V.schedule()[1]
    per, seed, ids = 3 * 24 * 40, 11, [4, 8]
    row_seeds = [PO.seed_of(seed, i, 0) for i in ids]
    drawn = [torch.stack([_randn(per, s, k) for s in row_seeds]).view(2, 3, 24, 40).cpu() for k in range(S - 1, -1, -1)]
    samp = _sampler_v()
    d_img = img.to(DEV)
    kw = dict(ddim=True, ddim_step=S, y_T=y_T.to(DEV), eta=ETA, seed=seed, image_ids=ids)
    with torch.no_grad():
        ref = V.ddim_loop(_model_eps(), img / 255.0, y_T, ab, TAU, ETA, drawn)
        got = []
        eager = samp(d_img, trajectory=got, **kw)
        graph = samp(d_img, **kw)
        names = _names(samp)
        # posterior(K = 2) is forward on the repeated images
        K = 2
        pairs = [(i, r) for i in ids for r in range(K)]
        y_rows = torch.stack([_randn(per, PO.seed_of(seed, i, r), PO.Y_T_OFFSET) for i, r in pairs]).view(4, 3, 24, 40)
        post = samp.posterior(d_img, K, ddim_step=S, eta=ETA, seed=seed, image_ids=ids, keep_samples=True)
        post_names = _names(samp)
        one = samp(d_img.repeat_interleave(K, dim=0), ddim=True, ddim_step=S, y_T=y_rows, eta=ETA, seed=seed, image_ids=pairs)
    e = DP._traj_error(got, ref)
    _report(f"eta={ETA} seeded 24x40", e, limit, e_ddim)
    assert e <= limit, (e, limit)
    assert names.count("hdiff_v_to_eps") == 1 and names[-2] == "hdiff_ddim_eta_step" and post_names == names
    assert torch.equal(graph, eager), "hipGraph replay and eager launches must agree bit for bit"
    assert torch.equal(post.samples.view(4, 3, 24, 40).view(torch.int32), one.view(torch.int32))
    want_m, want_s = PO.stats(post.samples.cpu().view(2, K, per))
    assert torch.equal(post.mean.cpu().view(2, per), want_m) and torch.equal(post.std.cpu().view(2, per), want_s)


def test_v_tiled_loop_chunks_and_graph():
    img, y_T = DP._inputs_b(24, 44)
    limit, e_ddim = DP._gate_b()
    ab = V.schedule()[1]
    samp = _sampler_v()
    d_img = img.to(DEV)
    kw = dict(ddim=True, ddim_step=S, y_T=y_T.to(DEV), tile=TILE, tile_overlap=OVERLAP)
    with torch.no_grad():
        ref = V.tiled_ddim_loop(_model_eps(), img / 255.0, y_T, ab, TAU, TD.Layout(24, 44, TILE, OVERLAP), TD.windows, TD.blend)
        got, got7 = [], []
        eager = samp(d_img, trajectory=got, **kw)
        graph = samp(d_img, **kw)
        chunked = samp(d_img, trajectory=got7, tile_batch=7, **kw)
        sp = next(iter(samp._plans.values()))
        assert [n for _, n in sp.chunks] == [7, 7, 6]
        chunked_graph = samp(d_img, tile_batch=7, **kw)
    e, e7 = DP._traj_error(got, ref), DP._traj_error(got7, ref)
    _report("tile=16 overlap=8 24x44", e, limit, e_ddim)
    _report("tile=16 overlap=8 24x44, tile_batch=7", e7, limit, e_ddim)
    assert e <= limit and e7 <= limit, (e, e7, limit)
    assert torch.equal(eager.cpu(), torch.clip(got[-1].cpu(), -1, 1))
    assert torch.equal(graph, eager), "hipGraph replay and eager launches must agree bit for bit"
    assert torch.equal(chunked_graph, chunked)


def test_v_ancestral_loop_T8():
    img, y_T = DP._inputs_b(24, 40)
    limit, e_ddim = DP._gate_b()
    T8 = 8
    g = torch.Generator().manual_seed(17)
    noise = [torch.randn(2, 3, 24, 40, generator=g) for _ in range(T8 - 1)]
    samp = _sampler_v(T8)
    d_img, d_y = img.to(DEV), y_T.to(DEV)
    with torch.no_grad():
        ref = V.ancestral_loop(_model_eps(T8), img / 255.0, y_T, V.schedule(n=T8)[0], noise + [None])
        got = []
        out = samp(d_img, y_T=d_y, noise_by_step=[z.to(DEV) for z in noise], trajectory=got)
        names = _names(samp)
        # drawn in the kernel: eager launches (a trajectory is asked for) and the replayed graph see the same seed
        torch.manual_seed(7)
        eager = samp(d_img, y_T=d_y, trajectory=[])
        torch.manual_seed(7)
        graph = samp(d_img, y_T=d_y)
        assert next(iter(samp._plans.values())).plan.graph.value
    assert len(got) == len(ref) == T8
    e = max(((a.cpu() - b).abs().max() / max(1.0, b.abs().max().item())).item() for a, b in zip(got, ref))
    _report(f"ancestral T={T8} 24x40", e, limit, e_ddim)
    assert e <= limit, (e, limit)
    assert names[0] == "hdiff_fill_t" and names[-3:] == ["hdiff_v_to_eps", "hdiff_ddpm_step", "hdiff_step_decrement"]
    assert torch.equal(out.cpu(), torch.clip(got[-1].cpu(), -1, 1))
    assert torch.equal(graph, eager), "hipGraph replay and eager launches must agree bit for bit"


# ----------------------------------------------------------------------------------------------------------------------
# 5. launch lists
# ----------------------------------------------------------------------------------------------------------------------
def test_op_lists():
    """A v plan's launches are the eps plan's with exactly one hdiff_v_to_eps directly behind the UNet's (per chunk when tiled); a
    sampler built with prediction="eps" is the sampler built without the argument."""
    dev = torch.device(DEV)
    sb, sv = DP._sampler_b(), _sampler_v()
    makes = {
        "ddim": lambda s: DD._StepPlan(s, 2, 24, 40, dev, S),
        "dpmpp2m": lambda s: DD._StepPlan(s, 2, 24, 40, dev, S, solver="dpmpp2m"),
        "eta": lambda s: DD._StepPlan(s, 2, 24, 40, dev, S, eta=ETA),
        "ancestral": lambda s: DD._StepPlan(s, 2, 24, 40, dev, None),
        "tiled": lambda s: DD._TiledStepPlan(s, 2, 24, 44, dev, S, TILE, OVERLAP, None),
        "tiled chunks": lambda s: DD._TiledStepPlan(s, 2, 24, 44, dev, S, TILE, OVERLAP, 7),
        "tiled dpmpp2m chunks": lambda s: DD._TiledStepPlan(s, 2, 24, 44, dev, S, TILE, OVERLAP, 7, solver="dpmpp2m"),
    }
    for tag, make in makes.items():
        pe, pv = make(sb), make(sv)
        a, b = [op[0] for op in pe.plan.ops], [op[0] for op in pv.plan.ops]
        unet = [op[0] for op in pv.unet.plan.ops]
        chunks = len(getattr(pv, "chunks", [None]))
        assert "hdiff_v_to_eps" not in a and b.count("hdiff_v_to_eps") == chunks, tag
        assert [n for n in b if n != "hdiff_v_to_eps"] == a, tag
        for i, n in enumerate(b):
            if n == "hdiff_v_to_eps":
                assert b[i - len(unet):i] == unet, (tag, "the conversion sits directly behind the UNet's launches")
                args = pv.plan.ops[i][2]
                assert args[0] == pv.unet.out.data_ptr() and args[1] == pv.unet.y.data_ptr() and args[2] == pv.unet.t.data_ptr(), tag
                assert args[5:] == (1000, pv.n_slots, 3 * pv.th * pv.tw), tag
    img, y_T = (x.to(DEV) for x in DP._inputs_b(24, 40))
    named = DD.GaussianDiffusionSampler(DP._small_b()[0], V.B1, V.BT, V.T, prediction="eps").to(DEV)
    with torch.no_grad():
        plain = sb(img, ddim=True, ddim_step=S, y_T=y_T)
        same = named(img, ddim=True, ddim_step=S, y_T=y_T)
        other = sv(img, ddim=True, ddim_step=S, y_T=y_T)
    (key, _), = sb._plans.items()
    (key_named, _), = named._plans.items()
    (key_v, _), = sv._plans.items()
    assert torch.equal(plain, same) and _names(named) == _names(sb) and key_named == key and len(key) == 14
    assert key_v == key + (("prediction", "v"),) and not torch.equal(other, plain)


# ----------------------------------------------------------------------------------------------------------------------
# 6. the drivers
# ----------------------------------------------------------------------------------------------------------------------
def _final(out):
    ck = os.path.join(str(out), "ckpt")
    return load(os.path.join(ck, TR.final_name(2, "HICRD", "LoLI"))), load(os.path.join(ck, TR.STATE_FILE))


def test_drivers_train_resume_and_evaluate_a_v_run(data_root, tmp_path, monkeypatch):   # noqa: F811
    """A two-epoch run (one per stage) with prediction="v": it writes prediction.json, resumes bit for bit, refuses to resume as
    "eps", and Evaluate.test on its checkpoint -- with no ``prediction`` key -- builds a sampler whose plan holds the conversion."""
    kw = dict(epochs_stage_1=1, epochs_stage_2=1, ema_decay=None, prediction="v", loss_weighting="min_snr")
    settings = {"prediction": "v", "loss_weighting": "min_snr", "snr_gamma": 5.0, "y0_divisor": 255.0}
    full = TR.train(config(data_root, tmp_path / "full", **kw))
    ck = os.path.join(str(tmp_path / "full"), "ckpt")
    assert sorted(os.listdir(ck)) == TR.expected_files(config(data_root, tmp_path / "full", **kw)) and "prediction.json" in os.listdir(ck)
    assert os.path.join(ck, "prediction.json") in full["files"] and EV.read_prediction(os.path.join(ck, "prediction.json")) == settings
    weights, state = _final(tmp_path / "full")
    assert state["prediction"] == settings and full["finished"]
    torch.load(os.path.join(ck, TR.final_name(2, "HICRD", "LoLI")), map_location="cpu")       # still a plain state dict
    # interrupted after the first epoch, resumed: the same bits
    part = TR.train(config(data_root, tmp_path / "run", max_epochs=1, **kw))
    assert not part["finished"]
    state_path = os.path.join(str(tmp_path / "run"), "ckpt", TR.STATE_FILE)
    with pytest.raises(RuntimeError, match="prediction"):
        TR.train(config(data_root, tmp_path / "run", resume=state_path, **dict(kw, prediction="eps")))
    with pytest.raises(RuntimeError, match="loss_weighting"):
        TR.train(config(data_root, tmp_path / "run", resume=state_path, **dict(kw, loss_weighting=None)))
    rest = TR.train(config(data_root, tmp_path / "run", resume=state_path, **kw))
    weights_r, state_r = _final(tmp_path / "run")
    assert rest["finished"] and rest["losses"] == full["losses"] and rest["validation"] == full["validation"]
    assert list(weights) == list(weights_r) and all(torch.equal(weights[k], weights_r[k]) for k in weights)
    assert sorted(os.listdir(os.path.join(str(tmp_path / "run"), "ckpt"))) == sorted(os.listdir(ck))
    # Evaluate.test
    built = []

    class Recording(DD.GaussianDiffusionSampler):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            built.append(self)

    monkeypatch.setattr(DD, "GaussianDiffusionSampler", Recording)
    path = os.path.join(ck, TR.final_name(2, "HICRD", "LoLI"))
    base = {**vars(config(data_root, tmp_path / "full")), "pretrained_path": path, "ddim_step": 2, "result_root": str(tmp_path / "result")}
    results = EV.test(types.SimpleNamespace(**base), None)
    assert built[-1].prediction == "v" and _names(built[-1]).count("hdiff_v_to_eps") == 1 and results["HICRD"]["n"] == 2
    with pytest.raises(ValueError, match="prediction"):
        EV.test(types.SimpleNamespace(**base, prediction="eps"), None)
    # the same file away from its prediction.json is taken for what every checkpoint was before: that is why the file is written
    os.makedirs(str(tmp_path / "moved"))
    moved = shutil.copy(path, str(tmp_path / "moved"))
    EV.test(types.SimpleNamespace(**{**base, "pretrained_path": moved}), None)
    assert built[-1].prediction == "eps" and "hdiff_v_to_eps" not in _names(built[-1])
