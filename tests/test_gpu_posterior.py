"""GPU: multi-sample posterior sampling of the image-conditioned sampler -- the three kernels bit for bit against their definitions
(tests/_posterior_def.py), ``forward`` unchanged without the new arguments, the loop with ``eta`` against the reference-shaped CPU
loop, ``posterior`` against one ``forward`` on the repeated images, and the evaluation / transfer drivers.

The gate of the loop test is not a constant: in the same test the deterministic DDIM loop's error against ITS CPU loop (the oracle's
``sampler_forward``) is measured on the same fixture, and the loop with ``eta`` may show twice that -- its step adds one product and
one sum per element to DDIM's.  Both figures are printed before the assertion; the values measured on an MI355X are in
profiles/posterior_sampling.txt."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hdiff_amd  # noqa: E402,F401
from hdiff_amd import _capi  # noqa: E402
from hdiff_amd import transfer as T  # noqa: E402
from hdiff_amd.diffusion import Diffusion as DD  # noqa: E402
from hdiff_amd.diffusion import Evaluate as EV  # noqa: E402
from oracle import cpu_path_b as OB  # noqa: E402

import _posterior_def as P  # noqa: E402

DEV = "cuda:0"
B1, BT, TT, S, ETA = 1e-4, 0.02, 1000, 4, 0.5
TAU = list(range(0, 1000, 250))
N_PER = (1, 3, 4, 5, 105, 1027)                       # 105 = 3 * 5 * 7; 1027: more than one workgroup's quads with rows = 3
SEEDS = (3, 2 ** 63 + 11, 0xFFFFFFFFFFFFFFFF)         # one above 2^63, one with every bit set
SENTINEL = 777.0


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _i32(v):
    return torch.tensor([v], dtype=torch.int32, device=DEV)


def _seed_tensor(seeds):
    return torch.tensor([P.as_int64(s) for s in seeds], dtype=torch.int64).to(DEV)


def _randn(n, seed, offset):
    out = torch.empty(n, device=DEV)
    _capi.check(_capi.lib().hdiff_randn(out.data_ptr(), n, C.c_uint64(seed), C.c_uint64(offset), _stream()), "randn")
    return out


def _padded(rows, n_per, pad):
    """A [rows, n_per] view that starts ``pad`` floats into a sentinel-filled buffer (pad = 5: a base that is only 4-byte aligned)."""
    buf = torch.full((rows * n_per + 2 * pad,), SENTINEL, device=DEV)
    return buf, buf[pad:pad + rows * n_per].view(rows, n_per)


def _untouched(buf, rows, n_per, pad):
    return bool((buf[:pad] == SENTINEL).all()) and bool((buf[pad + rows * n_per:] == SENTINEL).all())


# ----------------------------------------------------------------------------------------------------------------------
# 1. hdiff_randn_rows
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_per", N_PER)
def test_randn_rows_are_randn_of_each_seed(n_per):
    sd = _seed_tensor(SEEDS)
    for offset in (P.Y_T_OFFSET, 2):
        for pad in (8, 5):
            buf, out = _padded(3, n_per, pad)
            _capi.check(_capi.lib().hdiff_randn_rows(out.data_ptr(), 3, n_per, sd.data_ptr(), C.c_uint64(offset), _stream()),
                        "randn_rows")
            for r, s in enumerate(SEEDS):
                assert torch.equal(out[r].view(torch.int32), _randn(n_per, s, offset).view(torch.int32)), (n_per, offset, pad, r)
            assert _untouched(buf, 3, n_per, pad), (n_per, pad)
    assert bool(torch.isfinite(out).all())


# ----------------------------------------------------------------------------------------------------------------------
# 2. hdiff_ddim_eta_step
# ----------------------------------------------------------------------------------------------------------------------
def _eta_step(y, eps, noise, out, dtab, seeds, n_per, k, flag, rows):
    ctr = _i32(k)
    _capi.check(_capi.lib().hdiff_ddim_eta_step(y.data_ptr(), eps.data_ptr(), None if noise is None else noise.data_ptr(),
                                                out.data_ptr(), dtab.data_ptr(), None if seeds is None else seeds.data_ptr(), n_per,
                                                ctr.data_ptr(), S, flag.data_ptr(), rows, _stream()), "ddim_eta_step")


@functools.lru_cache(maxsize=None)
def _tables():
    betas = torch.linspace(B1, BT, TT).double()
    tab = P.eta_table(betas, TAU, ETA).float()
    tab0 = P.eta_table(betas, TAU, 0.0).float()
    return tab, tab.to(DEV).contiguous(), tab0, tab0.to(DEV).contiguous()


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("n_per", N_PER)
def test_eta_step_bit_exact(n_per, rows):
    tab, dtab, tab0, dtab0 = _tables()
    g = torch.Generator().manual_seed(100 * n_per + rows)
    y, eps, z = (torch.randn(rows, n_per, generator=g) * s for s in (1.5, 1.0, 1.0))
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    sd = _seed_tensor(SEEDS[:rows])
    for k in (S - 1, 0):                                     # the first step and the last: noise is added at both
        want = P.eta_step(y, eps, z, tab[k])
        for pad in (8, 5):                                   # 16-byte aligned, and a base that is only 4-byte aligned
            (by, dy), (be, de), (bz, dz), (bo, do) = (_padded(rows, n_per, pad) for _ in range(4))
            dy.copy_(y); de.copy_(eps); dz.copy_(z)
            _eta_step(dy, de, dz, do, dtab, None, n_per, k, flag, rows)                    # injected noise, out of place
            assert torch.equal(do.cpu(), want), (n_per, rows, k, pad)
            assert _untouched(bo, rows, n_per, pad) and torch.equal(dy.cpu(), y)
            _eta_step(dy, de, dz, dy, dtab, sd, n_per, k, flag, rows)                      # in place (seeds given, noise wins)
            assert torch.equal(dy.cpu(), want) and _untouched(by, rows, n_per, pad)
            dy.copy_(y)
            _eta_step(dy, de, None, do, dtab, sd, n_per, k, flag, rows)                    # drawn: the hdiff_randn rows
            drawn = torch.stack([_randn(n_per, s, k) for s in SEEDS[:rows]]).cpu()
            assert torch.equal(do.cpu(), P.eta_step(y, eps, drawn, tab[k])), (n_per, rows, k, pad)
        # c1 = 0: hdiff_ddim_step's result, whatever is drawn
        dy, de, do, ref = y.to(DEV), eps.to(DEV), torch.empty(rows, n_per, device=DEV), torch.empty(rows, n_per, device=DEV)
        _eta_step(dy, de, None, do, dtab0, sd, n_per, k, flag, rows)
        tab4 = dtab0[:, [0, 1, 2, 4]].contiguous()
        _capi.check(_capi.lib().hdiff_ddim_step(dy.data_ptr(), de.data_ptr(), ref.data_ptr(), tab4.data_ptr(), _i32(k).data_ptr(), S,
                                                flag.data_ptr(), rows * n_per, _stream()), "ddim_step")
        assert torch.equal(do, ref), (n_per, rows, k)
    assert int(flag.item()) == 0


def test_eta_step_nan_stays_in_its_row():
    tab, dtab, _, _ = _tables()
    n_per, rows = 105, 3
    g = torch.Generator().manual_seed(9)
    y, eps, z = (torch.randn(rows, n_per, generator=g) for _ in range(3))
    y[1, 17] = float("nan")
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = torch.empty(rows, n_per, device=DEV)
    _eta_step(y.to(DEV), eps.to(DEV), z.to(DEV), out, dtab, None, n_per, 2, flag, rows)
    want, got = P.eta_step(y, eps, z, tab[2]), out.cpu()
    assert int(flag.item()) == 1
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and int(torch.isnan(got).sum()) == 1 and bool(torch.isnan(got[1, 17]))
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])


# ----------------------------------------------------------------------------------------------------------------------
# 3. hdiff_sample_stats
# ----------------------------------------------------------------------------------------------------------------------
def _stats(x):
    B, K, n = x.shape
    mean, std = torch.full((B, n), SENTINEL, device=DEV), torch.full((B, n), SENTINEL, device=DEV)
    _capi.check(_capi.lib().hdiff_sample_stats(x.data_ptr(), B, K, n, mean.data_ptr(), std.data_ptr(), _stream()), "sample_stats")
    return mean.cpu(), std.cpu()


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("n", [1, 5, 1027])
@pytest.mark.parametrize("K", [1, 2, 3, 33])
def test_sample_stats_bit_exact(K, n, B):
    g = torch.Generator().manual_seed(1000 * K + 10 * n + B)
    x = torch.randn(B, K, n, generator=g) * 0.7 + 0.3 * torch.randn(B, 1, n, generator=g)
    mean, std = _stats(x.to(DEV))
    want_m, want_s = P.stats(x)
    assert torch.equal(mean, want_m) and torch.equal(std, want_s), (K, n, B)
    if K == 1:
        assert torch.equal(mean, x[:, 0]) and bool((std == 0).all())
    same = x[:, :1].expand(B, K, n).contiguous()                    # identical replicas: the spread is exactly 0
    mean, std = _stats(same.to(DEV))
    assert torch.equal(mean, x[:, 0]) and bool((std == 0).all())


def test_sample_stats_nan_spoils_its_image_only():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 3, 105, generator=g)
    clean_m, clean_s = P.stats(x)
    x[0, 1, 40] = float("nan")
    mean, std = _stats(x.to(DEV))
    assert bool(torch.isnan(mean[0, 40])) and bool(torch.isnan(std[0, 40]))
    assert int(torch.isnan(mean).sum()) == 1 and int(torch.isnan(std).sum()) == 1
    assert torch.equal(mean[1], clean_m[1]) and torch.equal(std[1], clean_s[1])


# ----------------------------------------------------------------------------------------------------------------------
# the small tree-B model at 16 x 16
# ----------------------------------------------------------------------------------------------------------------------
H = W = 16
PER = 3 * H * W


@functools.lru_cache(maxsize=None)
def _small():
    from _tree_b_small import load_small_dyn_unet
    _, cfg, m, sd = load_small_dyn_unet()
    ocfg = OB.DynUNetConfig(T=cfg["T"], ch=cfg["ch"], ch_mult=tuple(cfg["ch_mult"]), num_res_blocks=cfg["num_res_blocks"])
    return m.to(DEV), ocfg, sd


def _sampler(cls=DD.GaussianDiffusionSampler):
    return cls(_small()[0], B1, BT, TT).to(DEV)


@functools.lru_cache(maxsize=None)
def _inputs():
    g = torch.Generator().manual_seed(11)
    return torch.randint(0, 256, (2, 3, H, W), generator=g).float(), torch.randn(2, 3, H, W, generator=g)


def _names(samp):
    return [op[0] for op in next(iter(samp._plans.values())).plan.ops]


def _parent_names(samp, B):
    """The launch list of the plan the call built before ``eta`` existed: fill t, the UNet, the DDIM update, the counter."""
    unet = [op[0] for op in samp.model.plan_for(B, H, W, torch.device(DEV), True).plan.ops]
    return ["hdiff_fill_from_table"] + unet + ["hdiff_ddim_step", "hdiff_step_decrement"]


# ----------------------------------------------------------------------------------------------------------------------
# 4. forward without the new arguments
# ----------------------------------------------------------------------------------------------------------------------
def test_forward_is_unchanged_without_eta():
    img, y = (t.to(DEV) for t in _inputs())
    samp = _sampler()
    with torch.no_grad():
        plain = samp(img, ddim=True, ddim_step=S, y_T=y)
        (key, sp), = samp._plans.items()
        names = _names(samp)
        with_eta = samp(img, ddim=True, ddim_step=S, y_T=y, eta=0.0)
        (key2, sp2), = samp._plans.items()
    assert torch.equal(plain.view(torch.int32), with_eta.view(torch.int32))
    assert sp2 is sp and key2 == key and len(key) == 14, "eta=0.0 must reuse the plan of the call without it"
    assert names == _names(samp) == _parent_names(samp, 2)
    assert "hdiff_ddim_eta_step" not in names and not hasattr(sp, "seeds") and tuple(sp.tab.shape) == (S, 4)
    # seed= alone changes where y_T comes from and nothing else: the same plan, fed the rows hdiff_randn draws under the seeds
    y_rows = torch.stack([_randn(PER, P.seed_of(7, i, 0), P.Y_T_OFFSET) for i in (5, 9)]).view(2, 3, H, W)
    with torch.no_grad():
        torch.manual_seed(1)
        seeded = samp(img, ddim=True, ddim_step=S, seed=7, image_ids=[5, 9])
        torch.manual_seed(2)
        again = samp(img, ddim=True, ddim_step=S, seed=7, image_ids=[5, 9])
        given = samp(img, ddim=True, ddim_step=S, y_T=y_rows)
    assert torch.equal(seeded, given) and torch.equal(again, given) and next(iter(samp._plans.values())) is sp


# ----------------------------------------------------------------------------------------------------------------------
# 5. the loop with eta
# ----------------------------------------------------------------------------------------------------------------------
def _traj_error(got, ref):
    assert len(got) == len(ref) == S
    return max(((g.cpu() - r).abs().max() / max(1.0, r.abs().max().item())).item() for g, r in zip(got, ref))


def test_eta_loop_against_the_cpu_loop():
    _, ocfg, sd = _small()
    img, y_T = _inputs()
    samp = _sampler()
    kw = dict(ddim=True, ddim_step=S, y_T=y_T.to(DEV))
    seed, ids = 11, [4, 8]
    row_seeds = [P.seed_of(seed, i, 0) for i in ids]
    drawn = [torch.stack([_randn(PER, s, k) for s in row_seeds]).view(2, 3, H, W).cpu() for k in range(S - 1, -1, -1)]
    g = torch.Generator().manual_seed(12)
    injected = [torch.randn(2, 3, H, W, generator=g) for _ in range(S)]
    model = lambda x6, t: OB.dyn_unet_forward(sd, ocfg, x6, t)                                        # noqa: E731
    with torch.no_grad():
        ref0, got0 = [], []
        OB.sampler_forward(sd, ocfg, B1, BT, TT, img, y_T, ddim=True, ddim_step=S, trajectory=ref0)
        samp(img.to(DEV), trajectory=got0, **kw)
        e_ddim = _traj_error(got0, ref0)
        got_i, got_d = [], []
        out_i = samp(img.to(DEV), eta=ETA, noise_by_step=[z.to(DEV) for z in injected], trajectory=got_i, **kw)
        out_d = samp(img.to(DEV), eta=ETA, seed=seed, image_ids=ids, trajectory=got_d, **kw)
        names = _names(samp)
        graph = samp(img.to(DEV), eta=ETA, seed=seed, image_ids=ids, **kw)
        ref_i = P.eta_loop(model, img / 255.0, y_T, samp.alphas_bar.cpu(), TAU, ETA, injected)
        ref_d = P.eta_loop(model, img / 255.0, y_T, samp.alphas_bar.cpu(), TAU, ETA, drawn)
    e_i, e_d = _traj_error(got_i, ref_i), _traj_error(got_d, ref_d)
    limit = 2.0 * e_ddim
    print(f"tree B 16x16, {S} steps: ddim loop vs oracle {e_ddim:.3e}   eta={ETA} injected {e_i:.3e}   drawn {e_d:.3e}   gate {limit:.3e}")
    assert names == _parent_names(samp, 2)[:-2] + ["hdiff_ddim_eta_step", "hdiff_step_decrement"]
    assert torch.equal(out_i.cpu(), torch.clip(got_i[-1].cpu(), -1, 1)) and torch.equal(out_d.cpu(), torch.clip(got_d[-1].cpu(), -1, 1))
    assert torch.equal(graph, out_d), "hipGraph replay and eager launches must agree bit for bit"
    assert not torch.equal(got_d[0], got0[0]), "the first step already adds noise"
    assert e_i <= limit and e_d <= limit, (e_i, e_d, limit)


# ----------------------------------------------------------------------------------------------------------------------
# 6. posterior
# ----------------------------------------------------------------------------------------------------------------------
class _Spy(DD.GaussianDiffusionSampler):
    """Records, at the start of every chunk's loop, the plan's state and seeds."""

    def _run(self, sp, y_buffer, n_steps, *a, **k):
        self.seen.append((y_buffer.clone(), sp.seeds.clone() if hasattr(sp, "seeds") else None, sp.B))
        return super()._run(sp, y_buffer, n_steps, *a, **k)


def test_posterior_is_one_forward_on_the_repeated_images():
    img, _ = _inputs()
    img = img.to(DEV)
    seed, ids, K = 7, [5, 9], 3
    samp = _sampler()
    pairs = [(i, r) for i in ids for r in range(K)]
    y_T = torch.stack([_randn(PER, P.seed_of(seed, i, r), P.Y_T_OFFSET) for i, r in pairs]).view(6, 3, H, W)
    with torch.no_grad():
        post = samp.posterior(img, K, ddim_step=S, eta=ETA, seed=seed, image_ids=ids, keep_samples=True)
        names = _names(samp)
        one = samp(img.repeat_interleave(K, dim=0), ddim=True, ddim_step=S, y_T=y_T, eta=ETA, seed=seed, image_ids=pairs)
        assert len(samp._plans) == 1 and _names(samp) == names, "posterior and forward share the plan"
        no_keep = samp.posterior(img, K, ddim_step=S, eta=ETA, seed=seed, image_ids=ids)
    assert tuple(post.samples.shape) == (2, K, 3, H, W) and tuple(post.mean.shape) == tuple(post.std.shape) == (2, 3, H, W)
    assert torch.equal(post.samples.view(6, 3, H, W).view(torch.int32), one.view(torch.int32))
    want_m, want_s = P.stats(post.samples.cpu().view(2, K, PER))
    assert torch.equal(post.mean.cpu().view(2, PER), want_m) and torch.equal(post.std.cpu().view(2, PER), want_s)
    assert float(post.samples.abs().max()) <= 1.0 and float(post.mean.abs().max()) <= 1.0 and float(post.std.max()) > 0
    assert no_keep.samples is None and torch.equal(no_keep.mean, post.mean) and torch.equal(no_keep.std, post.std)
    # eager launches give the bits of the captured loop
    eager = _sampler()
    eager.GRAPH_MIN_STEPS = S + 1
    with torch.no_grad():
        post_e = eager.posterior(img, K, ddim_step=S, eta=ETA, seed=seed, image_ids=ids, keep_samples=True)
    assert not next(iter(eager._plans.values())).plan.graph.value and next(iter(samp._plans.values())).plan.graph.value
    assert torch.equal(post_e.samples, post.samples) and torch.equal(post_e.mean, post.mean) and torch.equal(post_e.std, post.std)


def test_posterior_chunks_prefixes_and_padding():
    img, _ = _inputs()
    img = img.to(DEV)
    seed, ids = 7, [5, 9]
    whole, chunked, two = _sampler(_Spy), _sampler(_Spy), _sampler(_Spy)
    for s in (whole, chunked, two):
        s.seen = []
    kw = dict(ddim_step=S, eta=ETA, seed=seed, image_ids=ids, keep_samples=True)
    with torch.no_grad():
        p6 = whole.posterior(img, 3, **kw)
        p4 = chunked.posterior(img, 3, sample_batch=4, **kw)
        p2 = two.posterior(img, 2, sample_batch=4, **kw)
        torch.manual_seed(1)
        again = chunked.posterior(img, 3, sample_batch=4, **kw)
    assert [b for _, _, b in whole.seen] == [6] and [b for _, _, b in chunked.seen[:2]] == [4, 4] and [b for _, _, b in two.seen] == [4]
    # K = 2 at plan batch 4 is the first two samples of K = 3 at plan batch 4
    assert torch.equal(p2.samples.view(torch.int32), p4.samples[:, :2].contiguous().view(torch.int32))
    assert torch.equal(again.samples, p4.samples), "nothing is read from torch's generator"
    # chunks 4 + 2 padded: y_T and the seeds of every sample are those of the unchunked run; the padding repeats the last sample
    (y6, s6, _), (ya, sa, _), (yb, sb, _) = whole.seen[0], chunked.seen[0], chunked.seen[1]
    assert torch.equal(torch.cat([ya, yb[:2]]).view(torch.int32), y6.view(torch.int32))
    assert torch.equal(torch.cat([sa, sb[:2]]), s6) and s6.tolist() == [P.as_int64(P.seed_of(seed, i, r)) for i in ids for r in range(3)]
    assert torch.equal(yb[2], yb[1]) and torch.equal(yb[3], yb[1]) and sb[2:].tolist() == [sb[1].item()] * 2
    for r, s in enumerate(P.seed_of(seed, i, r) for i in ids for r in range(3)):
        assert torch.equal(y6[r].reshape(-1), _randn(PER, s, P.Y_T_OFFSET))
    # ... and so is the first step's noise: the rows hdiff_randn_rows draws under the recorded seeds at the first counter value
    first = [torch.empty(int(s.numel()), PER, device=DEV) for s in (s6, sa, sb)]
    for out, s in zip(first, (s6, sa, sb)):
        _capi.check(_capi.lib().hdiff_randn_rows(out.data_ptr(), int(s.numel()), PER, s.data_ptr(), C.c_uint64(S - 1), _stream()),
                    "randn_rows")
    assert torch.equal(torch.cat([first[1], first[2][:2]]), first[0])
    # the same samples through another plan batch: the same draws, the model's own rounding apart
    gap = (p4.samples - p6.samples).abs().max().item()
    print(f"posterior: plan batch 4 (chunks 4 + 2) vs plan batch 6, max |difference| of the samples {gap:.3e}")
    assert gap <= 1e-3
    with torch.no_grad():            # the deterministic multistep solver: the samples differ through y_T alone
        pd = whole.posterior(img, 2, ddim_step=S, solver="dpmpp2m", seed=seed, keep_samples=True)
    assert "hdiff_dpmpp_step" in _names(whole) and not torch.equal(pd.samples[:, 0], pd.samples[:, 1])


# ----------------------------------------------------------------------------------------------------------------------
# 7. evaluate(samples=3)
# ----------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def _pairs():
    g = torch.Generator().manual_seed(5)
    return [(torch.randint(0, 256, (2, 3, H, W), generator=g, dtype=torch.uint8),
             torch.randint(0, 256, (2, 3, H, W), generator=g, dtype=torch.uint8), [f"img_{2 * i}.png", f"img_{2 * i + 1}.png"])
            for i in range(2)]


def test_evaluate_with_samples(tmp_path):
    from PIL import Image
    samp, batches = _sampler(), _pairs()
    d1, d2 = str(tmp_path / "one"), str(tmp_path / "two")
    torch.manual_seed(1)
    res = EV.evaluate(samp, batches, ddim_step=S, samples=3, eta=ETA, sample_seed=2, save_dir=d1)
    torch.manual_seed(2)
    res2 = EV.evaluate(samp, batches, ddim_step=S, samples=3, eta=ETA, sample_seed=2, save_dir=d2)
    plain_keys = {"n", "per_image", "psnr", "ssim", "uiqm", "uicm", "uism", "uiconm"}
    assert set(res) == plain_keys | {"samples", "per_sample", "sample_avg", "sample_std", "uncertainty"}
    assert res["n"] == 4 and res["samples"] == 3 and 0 < res["uncertainty"] < 1
    cols = ("psnr", "ssim", "uiqm", "uicm", "uism", "uiconm")
    assert set(res["per_sample"]) == set(res["sample_avg"]) == set(res["sample_std"]) == set(cols)
    for c in cols:
        v = res["per_sample"][c]
        assert len(v) == 3
        if np.isfinite(v).all():
            assert abs(res["sample_avg"][c] - float(np.mean(v))) <= 1e-12 * max(1.0, abs(float(np.mean(v))))
            assert abs(res["sample_std"][c] - float(np.std(v, ddof=1))) <= 1e-12 * max(1.0, float(np.std(v, ddof=1)))
    assert np.isfinite(res["per_sample"]["psnr"]).all() and res["sample_std"]["psnr"] > 0
    assert _same(res, res2), "the result must not depend on torch's generator"
    lines = [ln for ln in open(os.path.join(d1, "res.txt")).read().split("\n") if ln]
    assert [ln[:ln.index(":") + 1] for ln in lines] == P.res_keys([k for k, _ in EV.RES_KEYS])
    values = {ln[:ln.index(":")]: ln[ln.index(":") + 1:] for ln in lines}
    assert values["samples"] == "3" and values["psnr_orgin_avg"] == str(res["psnr"]) and values["uncertainty_avg"] == str(res["uncertainty"])
    assert values["psnr_sample_avg"] == str(res["sample_avg"]["psnr"]) and values["ssim_sample_std"] == str(res["sample_std"]["ssim"])
    assert open(os.path.join(d1, "res.txt"), "rb").read() == open(os.path.join(d2, "res.txt"), "rb").read()
    assert sorted(os.listdir(d1)) == sorted([f"img_{i}.png" for i in range(4)] + ["res.txt", "std"])
    assert sorted(os.listdir(os.path.join(d1, "std"))) == [f"img_{i}.png" for i in range(4)]
    # the files: the mean image and rint(255 * clamp(std_gain * std / 2, 0, 1)) of the posterior of each batch under its set indices
    with torch.no_grad():
        post = samp.posterior(batches[1][0].to(DEV).float(), 3, ddim_step=S, eta=ETA, seed=2, image_ids=[2, 3])
    want_std = (255.0 * (4.0 * post.std / 2).clamp(0, 1)).round().to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()
    want_mean = (255.0 * ((post.mean + 1) / 2).clamp(0, 1)).round().to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()
    for j, i in enumerate((2, 3)):
        assert np.array_equal(np.asarray(Image.open(os.path.join(d1, "std", f"img_{i}.png"))), want_std[j])
        assert np.array_equal(np.asarray(Image.open(os.path.join(d1, f"img_{i}.png"))), want_mean[j])
    # the batch size moves no image's noise: one image per batch gives the same draws through another plan batch, so the scores
    # agree to the model's rounding (not bit for bit: another batch size may round another way), far inside the draw-to-draw spread
    singles = [(a[i:i + 1], b[i:i + 1], n[i:i + 1]) for a, b, n in batches for i in range(2)]
    res1 = EV.evaluate(samp, singles, ddim_step=S, samples=3, eta=ETA, sample_seed=2)
    gap = abs(res1["psnr"] - res["psnr"])
    print(f"evaluate(samples=3): psnr {res['psnr']:.6f} at batch 2, {res1['psnr']:.6f} at batch 1; draw-to-draw std {res['sample_std']['psnr']:.3e}")
    assert gap <= 1e-2 * res["sample_std"]["psnr"]


def test_evaluate_without_samples_writes_what_it_wrote(tmp_path):
    """The loop as it stood before ``samples=`` -- one sampler call per batch under torch's generator, one meter, ``RES_KEYS`` -- written
    out here, gives the bytes ``evaluate`` writes without the new arguments."""
    from hdiff_amd import quality as Q
    samp, batches = _sampler(), _pairs()
    got_dir, want_dir = str(tmp_path / "got"), str(tmp_path / "want")
    calls = []
    samp.posterior = lambda *a, **k: calls.append(1)                 # must never be reached
    torch.manual_seed(21)
    res = EV.evaluate(samp, batches, ddim_step=S, save_dir=got_dir)
    torch.manual_seed(21)
    meter = Q.QualityMeter()
    os.makedirs(want_dir)
    with torch.no_grad():
        for inp, target, _ in batches:
            out = samp(inp.to(DEV).float(), ddim=True, unconditional_guidance_scale=1, ddim_step=S)
            meter.update((out + 1) / 2, target.to(DEV).float() / 255)
    want = meter.compute()
    EV.write_res(os.path.join(want_dir, "res.txt"), want, EV.RES_KEYS)
    assert not calls and set(res) == set(want)
    assert open(os.path.join(got_dir, "res.txt"), "rb").read() == open(os.path.join(want_dir, "res.txt"), "rb").read()
    assert sorted(os.listdir(got_dir)) == sorted([f"img_{i}.png" for i in range(4)] + ["res.txt"])
    assert _names(samp) == _parent_names(samp, 2)


# ----------------------------------------------------------------------------------------------------------------------
# 8. GuidedEnhancer(samples=2)
# ----------------------------------------------------------------------------------------------------------------------
def test_guided_enhancer_fits_on_the_mean():
    import _transfer_def as TD
    samp = _sampler()
    img = torch.from_numpy(TD.u8_fixture((H, W), (45, 61))[0]).to(DEV)
    enhance = T.GuidedEnhancer(samp, size=H, radius=2, eps=1e-3, samples=2, eta=ETA, seed=3, ddim_step=S)
    got = enhance(img)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (45, 61, 3)
    low = T.resample(img, H)
    with torch.no_grad():
        post = samp.posterior(low[None], 2, ddim_step=S, eta=ETA, seed=3)
    pred01 = ((post.mean + 1) / 2).clamp(0, 1)
    want = T.guided_apply(T.guided_fit(low[None] / 255, pred01, radius=2, eps=1e-3)[0], img)
    assert torch.equal(got, want)
    assert "hdiff_ddim_eta_step" in _names(samp)
    # without the argument: one plain sampler call, the plan of the call as it was
    y_T = torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(3)).to(DEV)
    calls = []
    samp.posterior = lambda *a, **k: calls.append(1)
    plain = T.GuidedEnhancer(samp, size=H, radius=2, eps=1e-3, ddim_step=S, y_T=y_T)(img)
    with torch.no_grad():
        out = samp(low[None], ddim=True, ddim_step=S, y_T=y_T)
    want = T.guided_apply(T.guided_fit(low[None] / 255, ((out + 1) / 2).clamp(0, 1), radius=2, eps=1e-3)[0], img)
    assert not calls and torch.equal(plain, want) and _names(samp) == _parent_names(samp, 1)
