"""GPU: DPM-Solver++(2M) sampling (``solver="dpmpp2m"``) of both samplers -- the three update kernels bit for bit against the fp32
definition (tests/_dpmpp_def.py), the loop bookkeeping of the label-conditioned one, both whole loops against their CPU loops
(the oracle's UNet + the definition's update), graph replay, the history across calls, and what must not have changed.

Gates of the loop tests are not constants: in the same test the existing DDIM sampler's error against its own CPU loop is measured,
and the new solver may be twice that, floored at 2e-5 (fp32 roundings of a handful of steps) -- the update adds one product and
one sum per element to DDIM's, and carries one more rounded state.  Tree A measures max |got - ref| per step, as
tests/test_gpu_ddim_a.py does; tree B the relative measure of ``gate()`` in tests/test_gpu_tiled.py.  Every figure is printed before
it is asserted; the values measured on an MI355X are in profiles/dpmpp.txt."""
import ctypes as C
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import hdiff_amd  # noqa: E402
from hdiff_amd import _capi  # noqa: E402
from hdiff_amd.DiffusionFreeGuidence import DiffusionCondition as DC  # noqa: E402
from hdiff_amd.DiffusionFreeGuidence import ModelCondition as MC  # noqa: E402
from hdiff_amd.DiffusionFreeGuidence import TrainCondition as TC  # noqa: E402
from hdiff_amd.diffusion import Diffusion as DD  # noqa: E402
from hdiff_amd.diffusion import Evaluate as EV  # noqa: E402
from oracle import cpu_path as O  # noqa: E402
from oracle import cpu_path_b as OB  # noqa: E402

import _ddim_a_def as D  # noqa: E402
import _dpmpp_def as P  # noqa: E402
import _tiled_def as TD  # noqa: E402
import test_gpu_ddim_a as DA  # noqa: E402      (the TRAJ fixture: model, x_T, labels -- built once, shared)

DEV = "cuda:0"
T, S = 1000, 10
BETAS = torch.linspace(1e-4, 0.02, T).double()
N = 2 * 3 * 5 * 7 + 1                                   # 211: 52 whole quads and a tail of 3
FLOOR = 2e-5


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _i32(v):
    return torch.tensor([v], dtype=torch.int32, device=DEV)


def _tab(shift):
    """(fp32 table on the CPU, the same on the device) of the S logSNR steps of the default schedule."""
    final = 1.0 if shift == 0 else float(P.alphas_bar(BETAS)[0])
    tab = P.table(BETAS, P.logsnr_steps(BETAS, S, shift), shift, final).float()
    return tab, tab.to(DEV).contiguous()


def _cfg_step(x, ec, eu, out, prev, dtab, k, w, clip, flag, n=N):
    ctr = _i32(k)
    _capi.check(_capi.lib().hdiff_cfg_dpmpp_step(x.data_ptr(), ec.data_ptr(), eu.data_ptr(), out.data_ptr(), prev.data_ptr(),
                                                 dtab.data_ptr(), ctr.data_ptr(), S, C.c_double(w), int(clip), flag.data_ptr(), n,
                                                 _stream()), "cfg_dpmpp_step")


def _b_step(y, eps, out, prev, dtab, k, clip, flag, n=N):
    ctr = _i32(k)
    _capi.check(_capi.lib().hdiff_dpmpp_step(y.data_ptr(), eps.data_ptr(), out.data_ptr(), prev.data_ptr(), dtab.data_ptr(),
                                             ctr.data_ptr(), S, int(clip), flag.data_ptr(), n, _stream()), "dpmpp_step")


# ----------------------------------------------------------------------------------------------------------------------
# a. the three kernels, bit for bit
# ----------------------------------------------------------------------------------------------------------------------
def _check_update_kernel(run, shift, want_eps):
    """``run(x, prev, k, clip, flag) -> None`` updates the device tensors x and prev in place; ``want_eps`` is the definition's eps."""
    g = torch.Generator().manual_seed(7 + shift)
    x, prev = torch.randn(N, generator=g), torch.randn(N, generator=g)
    tab, _ = _tab(shift)
    assert float(tab[5, P.C_]) != 0 and float(tab[S - 1, P.C_]) == 0 and float(tab[0, P.C_]) == 0
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    clipped = 0
    for clip in (False, True):
        # a middle row reads the history; rows S-1 and 0 do not; a counter outside [0, S) is clamped into the table
        for k, as_k in ((5, 5), (0, 0), (-7, 0), (10 ** 6, S - 1)):
            dx, dp = x.to(DEV), prev.to(DEV)
            ptr = dx.data_ptr()
            run(dx, dp, k, clip, flag)
            v, x0 = P.update(x, want_eps, prev, tab[as_k], clip)
            assert dx.data_ptr() == ptr and torch.equal(dx.cpu(), v), (k, clip)
            assert torch.equal(dp.cpu(), x0), (k, clip)
            clipped += int((((x - want_eps * tab[as_k][0]) / tab[as_k][1]).abs() > 1).sum()) if clip else 0
        # row S-1 with a history full of NaN: it is not read
        dx, dp = x.to(DEV), torch.full((N,), float("nan"), device=DEV)
        run(dx, dp, S - 1, clip, flag)
        v, x0 = P.update(x, want_eps, None, tab[S - 1], clip)
        assert torch.isfinite(dx).all() and torch.equal(dx.cpu(), v) and torch.equal(dp.cpu(), x0), clip
    assert clipped > 100 and int(flag.item()) == 0
    # a NaN in x sets the flag, with and without the clip, and stays where it is
    bad = x.clone()
    bad[N - 2] = float("nan")                              # in the tail
    for clip in (False, True):
        flag.zero_()
        dx, dp = bad.to(DEV), prev.to(DEV)
        run(dx, dp, 5, clip, flag)
        assert int(flag.item()) == 1 and int(torch.isnan(dx).sum()) == 1 and bool(torch.isnan(dx[N - 2])), clip


@pytest.mark.parametrize("w", [0.0, 1.8])
def test_cfg_dpmpp_step_bit_exact(w):
    g = torch.Generator().manual_seed(1)
    ec, eu = torch.randn(N, generator=g), torch.randn(N, generator=g)
    dec, deu = ec.to(DEV), eu.to(DEV)
    _, dtab = _tab(0)
    _check_update_kernel(lambda dx, dp, k, clip, flag: _cfg_step(dx, dec, deu, dx, dp, dtab, k, w, clip, flag), 0,
                         P.guided_eps(ec, eu, w))
    # buffers that are not 16-byte aligned take the element-wise path: the same bits
    tab, _ = _tab(0)
    x, prev = torch.randn(N, generator=g), torch.randn(N, generator=g)
    pad = [torch.cat([torch.zeros(1), t]).to(DEV) for t in (x, ec, eu, prev)]
    dx, dc, du, dp = [t[1:] for t in pad]
    assert dx.data_ptr() % 16 == 4
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    _cfg_step(dx, dc, du, dx, dp, dtab, 5, w, True, flag)
    v, x0 = P.update(x, P.guided_eps(ec, eu, w), prev, tab[5], True)
    assert torch.equal(dx.cpu(), v) and torch.equal(dp.cpu(), x0) and all(float(t[0]) == 0 for t in pad)


def test_dpmpp_step_bit_exact():
    g = torch.Generator().manual_seed(2)
    eps = torch.randn(N, generator=g)
    de = eps.to(DEV)
    _, dtab = _tab(1)
    _check_update_kernel(lambda dy, dp, k, clip, flag: _b_step(dy, de, dy, dp, dtab, k, clip, flag), 1, eps)


class Tables:
    """Device tables of a window layout, as the sampler builds them."""

    def __init__(self, lay):
        i32 = dict(dtype=torch.int32, device=DEV)
        self.oy, self.ox = torch.tensor(lay.oy, **i32), torch.tensor(lay.ox, **i32)
        self.fy, self.cy, self.wy = lay.fy.to(DEV), lay.cy.to(DEV), lay.wy.to(DEV).contiguous()
        self.fx, self.cx, self.wx = lay.fx.to(DEV), lay.cx.to(DEV), lay.wx.to(DEV).contiguous()


def _tile_step(y, eps_w, prev, tb, dtab, k, clip, flag, B, lay):
    ctr = _i32(k)
    _capi.check(_capi.lib().hdiff_tile_dpmpp_step(
        y.data_ptr(), eps_w.data_ptr(), prev.data_ptr(), tb.fy.data_ptr(), tb.cy.data_ptr(), tb.wy.data_ptr(), tb.oy.data_ptr(),
        tb.fx.data_ptr(), tb.cx.data_ptr(), tb.wx.data_ptr(), tb.ox.data_ptr(), dtab.data_ptr(), ctr.data_ptr(), S, int(clip),
        flag.data_ptr(), B, 3, lay.H, lay.W, lay.ny, lay.nx, lay.th, lay.tw, _stream()), "tile_dpmpp_step")


def test_tile_dpmpp_step_bit_exact_and_one_window():
    g = torch.Generator().manual_seed(3)
    tab, dtab = _tab(1)
    lay = TD.Layout(24, 44, 16, 8)
    assert {1, 2, 3, 6} <= set((lay.cy[:, None] * lay.cx[None, :]).unique().tolist())
    tb = Tables(lay)
    y, prev = torch.randn(2, 3, 24, 44, generator=g), torch.randn(2, 3, 24, 44, generator=g)
    eps_w = torch.randn(20, 3, 16, 16, generator=g)
    eps = TD.blend(eps_w, 2, lay)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    for clip in (False, True):
        for k, as_k in ((5, 5), (0, 0), (99, S - 1), (-3, 0)):
            dy, dp, de = y.to(DEV), prev.to(DEV), eps_w.to(DEV)
            _tile_step(dy, de, dp, tb, dtab, k, clip, flag, 2, lay)
            v, x0 = P.update(y, eps, prev, tab[as_k], clip)
            assert torch.equal(dy.cpu(), v) and torch.equal(dp.cpu(), x0) and torch.equal(de.cpu(), eps_w), (k, clip)
        dy, dp = y.to(DEV), torch.full_like(y, float("nan")).to(DEV)
        _tile_step(dy, eps_w.to(DEV), dp, tb, dtab, S - 1, clip, flag, 2, lay)
        v, x0 = P.update(y, eps, None, tab[S - 1], clip)
        assert torch.isfinite(dy).all() and torch.equal(dy.cpu(), v) and torch.equal(dp.cpu(), x0), clip
    assert int(flag.item()) == 0
    # one NaN in a window raises the flag and reaches exactly the pixels that window element covers
    bad = eps_w.clone()
    bad[13, 1, 5, 9] = float("nan")                        # window (b, iy, ix) = (1, 0, 3): pixel (5, 24 + 9)
    dy, dp = y.to(DEV), prev.to(DEV)
    _tile_step(dy, bad.to(DEV), dp, tb, dtab, 5, False, flag, 2, lay)
    nan = torch.isnan(dy.cpu())
    assert int(flag.item()) == 1 and int(nan.sum()) == 1 and bool(nan[1, 1, 5, 33])
    # and a NaN in y
    flag.zero_()
    bad_y = y.clone()
    bad_y[0, 2, 23, 43] = float("nan")
    dy = bad_y.to(DEV)
    _tile_step(dy, eps_w.to(DEV), prev.to(DEV), tb, dtab, 5, True, flag, 2, lay)
    assert int(flag.item()) == 1 and int(torch.isnan(dy).sum()) == 1
    # 7x5 image, tile 16: one window smaller than the tile, weight 1.0 -- hdiff_dpmpp_step bit for bit
    lay1 = TD.Layout(7, 5, 16, 2)
    tb1 = Tables(lay1)
    y1, e1, p1 = [torch.randn(2, 3, 7, 5, generator=g) for _ in range(3)]
    flag1 = torch.zeros(1, dtype=torch.int32, device=DEV)
    for clip in (False, True):
        for k in (S - 1, 5, 0):
            dy, dp, de = y1.to(DEV), p1.to(DEV), e1.to(DEV)
            old, old_p = y1.to(DEV), p1.to(DEV)
            _b_step(old, de, old, old_p, dtab, k, clip, flag1, n=y1.numel())
            _tile_step(dy, de, dp, tb1, dtab, k, clip, flag1, 2, lay1)
            v, x0 = P.update(y1, e1, p1, tab[k], clip)
            assert torch.equal(dy, old) and torch.equal(dp, old_p) and torch.equal(dy.cpu(), v) and torch.equal(dp.cpu(), x0), (k, clip)
    assert int(flag1.item()) == 0


# ----------------------------------------------------------------------------------------------------------------------
# b. the loop's bookkeeping (tree A)
# ----------------------------------------------------------------------------------------------------------------------
def test_step_loop_bookkeeping():
    g = torch.Generator().manual_seed(4)
    B, per, w = 3, 3 * 40 * 36, 1.8
    n = B * per
    tau = [3, 110, 290, 530, 999]
    Sn = len(tau)
    x, ec, eu = [torch.randn(n, generator=g) for _ in range(3)]
    tab = P.table(BETAS, tau).float()
    dtab, dtau = tab.to(DEV).contiguous(), torch.tensor(tau, dtype=torch.int64, device=DEV)
    dec, deu = ec.to(DEV), eu.to(DEV)
    cur = x.to(DEV)
    prev = torch.full((n,), float("nan"), device=DEV)      # what an earlier call may have left
    ctr = _i32(Sn - 1)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    done = torch.zeros(1, dtype=torch.int32, device=DEV)
    t_next = torch.full((2 * B,), -5, dtype=torch.int64, device=DEV)
    xin = torch.zeros(2 * n, device=DEV)
    d = _capi.CfgDpmppLoopDesc()
    d.x, d.eps_c, d.eps_u, d.x_next, d.x0_prev = cur.data_ptr(), dec.data_ptr(), deu.data_ptr(), cur.data_ptr(), prev.data_ptr()
    d.tab, d.t_tab, d.step_ptr, d.nsteps, d.clip_x0 = dtab.data_ptr(), dtau.data_ptr(), ctr.data_ptr(), Sn, 0
    d.w, d.nan_flag, d.n = w, flag.data_ptr(), n
    d.x_dup0, d.x_dup1, d.t_next, d.t_count = xin.data_ptr(), xin.data_ptr() + 4 * n, t_next.data_ptr(), 2 * B
    d.done_counter = done.data_ptr()
    lib = _capi.lib()
    want, want_prev = x, None
    eps = P.guided_eps(ec, eu, w)
    for k in range(Sn - 1, -1, -1):                       # five eager launches, no reset in between
        _capi.check(lib.hdiff_cfg_dpmpp_step_loop(C.byref(d), _stream()), "cfg_dpmpp_step_loop")
        torch.cuda.synchronize()
        want, want_prev = P.update(want, eps, want_prev, tab[k], False)
        assert torch.equal(cur.cpu(), want) and torch.equal(prev.cpu(), want_prev), k
        assert torch.equal(xin[:n], cur) and torch.equal(xin[n:], cur), k
        assert int(ctr.item()) == k - 1
        assert t_next.tolist() == [tau[max(k - 1, 0)]] * (2 * B), k
        assert int(done.item()) == 0 and int(flag.item()) == 0          # the counter wrapped back by itself


# ----------------------------------------------------------------------------------------------------------------------
# c. the whole loop, tree A
# ----------------------------------------------------------------------------------------------------------------------
def _traj_tau(spacing):
    betas = torch.linspace(*DA.TRAJ_BETA, DA.TRAJ["T"]).double()
    return P.logsnr_steps(betas, DA.TRAJ_S) if spacing == "logsnr" else D.timesteps(DA.TRAJ["T"], DA.TRAJ_S)


@functools.lru_cache(maxsize=None)
def _traj_references(spacing, w, clip):
    """-> (the 2M loop's states, the DDIM loop's states on the same time steps), on the CPU: eps from the oracle's UNet and
    guidance, the definitions' updates.  Computed once per case, shared by both contraction modes, never modified."""
    _, sd, x_T, labels, _ = DA._traj_model()
    cfg = O.UNetConfig(T=DA.TRAJ["T"], num_labels=DA.TRAJ["num_labels"], ch=DA.TRAJ["ch"], ch_mult=tuple(DA.TRAJ["ch_mult"]),
                       num_res_blocks=DA.TRAJ["num_res_blocks"])
    betas = torch.linspace(*DA.TRAJ_BETA, DA.TRAJ["T"]).double()
    tau = _traj_tau(spacing)
    tab2m, tab1 = P.table(betas, tau).float(), D.table(betas, tau, 0.0).float()

    def eps_of(x, k):
        t = torch.full((x.shape[0],), tau[k], dtype=torch.long)
        return O.cfg_eps(O.unet_forward(sd, cfg, x, t, labels), O.unet_forward(sd, cfg, x, t, torch.zeros_like(labels)), w)

    x2, x1, prev, s2, s1 = x_T, x_T, None, [], []
    with torch.no_grad():
        for k in range(DA.TRAJ_S - 1, -1, -1):
            x2, prev = P.update(x2, eps_of(x2, k), prev, tab2m[k], clip)
            x1 = D.update(x1, eps_of(x1, k), None, tab1[k], k, clip)
            s2.append(x2)
            s1.append(x1)
    return tuple(s2), tuple(s1)


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("w", [0.0, 1.8])
@pytest.mark.parametrize("spacing", ["uniform", "logsnr"])
def test_trajectory_against_the_oracle(spacing, w, clip, mode):
    """Every pre-clip state against the CPU loop, max |got - ref| per step; gate: twice the DDIM loop's own largest error on the
    same time steps, measured here, floored at 2e-5.  Measured on an MI355X: see profiles/dpmpp.txt."""
    m, _, x_T, labels, _ = DA._traj_model()
    ref2m, ref1 = _traj_references(spacing, w, clip)
    tau = _traj_tau(spacing)
    x_T, labels = x_T.to(DEV), labels.to(DEV)
    before = hdiff_amd.get_contraction_mode()
    hdiff_amd.set_contraction_mode(mode)
    try:
        samp = DC.GaussianDiffusionSampler(m, *DA.TRAJ_BETA, DA.TRAJ["T"], w=w).to(DEV)
        t2, t1 = [], []
        with torch.no_grad():
            kw = dict(ddim_steps=DA.TRAJ_S, clip_x0=clip, solver="dpmpp2m", spacing=spacing)
            y_eager = samp(x_T, labels, trajectory=t2, **kw)
            y_graph = samp(x_T, labels, **kw)
            samp(x_T, labels, timesteps=tau, clip_x0=clip, trajectory=t1)                 # DDIM on the same steps: the yardstick
            samp(-x_T, labels, **kw)                                                      # leaves another history behind
            y_again = samp(x_T, labels, **kw)
            y_fresh = DC.GaussianDiffusionSampler(m, *DA.TRAJ_BETA, DA.TRAJ["T"], w=w).to(DEV)(x_T, labels, **kw)
    finally:
        hdiff_amd.set_contraction_mode(before)
    assert len(t2) == len(t1) == DA.TRAJ_S
    e2, e1 = [DA.maxerr(a, b) for a, b in zip(t2, ref2m)], [DA.maxerr(a, b) for a, b in zip(t1, ref1)]
    limit = max(2.0 * max(e1), FLOOR)
    print(f"dpmpp2m trajectory spacing={spacing} w={w} clip_x0={clip} {mode}: tau {tau}")
    print("   dpmpp2m per-step max err", ["%.2e" % e for e in e2])
    print("   ddim    per-step max err", ["%.2e" % e for e in e1], f"  gate {limit:.2e}")
    assert max(e2) <= limit, (max(e2), limit)
    assert float(y_graph.min()) >= -1 and float(y_graph.max()) <= 1
    assert torch.equal(y_eager, torch.clip(t2[-1], -1, 1))
    assert torch.equal(y_eager, y_graph), "graph replay must reproduce the eager launches bit for bit"
    assert torch.equal(y_again, y_graph) and torch.equal(y_fresh, y_graph), "the x0 history leaked from one call into the next"


# ----------------------------------------------------------------------------------------------------------------------
# d. the whole loop, tree B
# ----------------------------------------------------------------------------------------------------------------------
B1, BT, DDIM_STEP, TILE, OVERLAP, SEED = 1e-4, 0.02, 5, 16, 8, 11


@functools.lru_cache(maxsize=None)
def _small_b():
    from _tree_b_small import load_small_dyn_unet
    _, cfg, m, sd = load_small_dyn_unet()
    ocfg = OB.DynUNetConfig(T=cfg["T"], ch=cfg["ch"], ch_mult=tuple(cfg["ch_mult"]), num_res_blocks=cfg["num_res_blocks"])
    return m.to(DEV), ocfg, sd


def _inputs_b(H, W):
    g = torch.Generator().manual_seed(SEED)
    img = torch.randint(0, 256, (2, 3, H, W), generator=g).float()
    return img, torch.randn(2, 3, H, W, generator=g)


def _sampler_b():
    return DD.GaussianDiffusionSampler(_small_b()[0], B1, BT, T).to(DEV)


def _traj_error(got, ref):
    assert len(got) == len(ref) == DDIM_STEP
    return max(((g.cpu() - r).abs().max() / max(1.0, r.abs().max().item())).item() for g, r in zip(got, ref))


@functools.lru_cache(maxsize=None)
def _gate_b():
    """-> (gate, the untiled DDIM sampler's own error against oracle.cpu_path_b.sampler_forward on 24x40): the rule of ``gate()`` in
    tests/test_gpu_tiled.py."""
    _, ocfg, sd = _small_b()
    img, y_T = _inputs_b(24, 40)
    ref, got = [], []
    with torch.no_grad():
        OB.sampler_forward(sd, ocfg, B1, BT, T, img, y_T, ddim=True, ddim_step=DDIM_STEP, trajectory=ref)
        _sampler_b()(img.to(DEV), ddim=True, ddim_step=DDIM_STEP, y_T=y_T.to(DEV), trajectory=got)
    e = _traj_error(got, ref)
    return max(2.0 * e, FLOOR), e


@functools.lru_cache(maxsize=None)
def _definition_b(H, W, tiled):
    """The CPU loop's pre-clip trajectory: the oracle's DynamicUNet (on the windows and blended when ``tiled``), the definition's
    time steps, table and update.  Computed once, shared, never modified."""
    _, ocfg, sd = _small_b()
    img, y = _inputs_b(H, W)
    img = img / 255.0
    tau = P.logsnr_steps(BETAS, DDIM_STEP, 1)
    tab = P.table(BETAS, tau, 1, float(P.alphas_bar(BETAS)[0])).float()
    lay = TD.Layout(H, W, TILE, OVERLAP) if tiled else None
    cond_w = TD.windows(img, lay) if tiled else None
    prev, traj = None, []
    with torch.no_grad():
        for k in range(DDIM_STEP - 1, -1, -1):
            if tiled:
                t = torch.full((cond_w.shape[0],), tau[k], dtype=torch.long)
                eps = TD.blend(OB.dyn_unet_forward(sd, ocfg, torch.cat([cond_w, TD.windows(y, lay)], dim=1).float(), t), 2, lay)
            else:
                t = torch.full((2,), tau[k], dtype=torch.long)
                eps = OB.dyn_unet_forward(sd, ocfg, torch.cat([img, y], dim=1).float(), t)
            y, prev = P.update(y, eps, prev, tab[k], False)
            traj.append(y)
    return tuple(traj)


def test_tree_b_untiled_loop_graph_and_one_window():
    img, y_T = _inputs_b(24, 40)
    img, y_T = img.to(DEV), y_T.to(DEV)
    limit, e_ddim = _gate_b()
    samp = _sampler_b()
    kw = dict(ddim=True, ddim_step=DDIM_STEP, y_T=y_T, solver="dpmpp2m")
    with torch.no_grad():
        got, got_w = [], []
        eager = samp(img, trajectory=got, **kw)
        graph = samp(img, **kw)
        names = [op[0] for op in next(iter(samp._plans.values())).plan.ops]
        one_window = samp(img, trajectory=got_w, tile=64, **kw)
        one_window_graph = samp(img, tile=64, tile_overlap=0, tile_batch=2, **kw)
        samp(255 - img, **kw)                                                 # leaves another history behind
        again = samp(img, **kw)
        explicit = samp(img, ddim=True, y_T=y_T, solver="dpmpp2m", timesteps=DD.logsnr_timesteps(samp.betas, DDIM_STEP, shift=1))
    e = _traj_error(got, _definition_b(24, 40, False))
    print(f"tree B untiled 24x40: ddim sampler vs oracle {e_ddim:.3e}   dpmpp2m vs its CPU loop {e:.3e}   gate {limit:.3e}")
    assert names.count("hdiff_dpmpp_step") == 1 and "hdiff_ddim_step" not in names
    assert e <= limit, (e, limit)
    assert torch.equal(eager.cpu(), torch.clip(got[-1].cpu(), -1, 1))
    assert torch.equal(graph, eager), "hipGraph replay and eager launches must agree bit for bit"
    assert torch.equal(one_window, eager) and all(torch.equal(a, b) for a, b in zip(got_w, got)), "one window is the untiled path"
    assert torch.equal(one_window_graph, eager)
    assert torch.equal(again, eager) and torch.equal(explicit, eager)


def test_tree_b_tiled_loop_chunks_and_graph():
    img, y_T = _inputs_b(24, 44)
    img, y_T = img.to(DEV), y_T.to(DEV)
    limit, _ = _gate_b()
    ref = _definition_b(24, 44, True)
    samp = _sampler_b()
    kw = dict(ddim=True, ddim_step=DDIM_STEP, y_T=y_T, solver="dpmpp2m", tile=TILE, tile_overlap=OVERLAP)
    with torch.no_grad():
        got, got7 = [], []
        eager = samp(img, trajectory=got, **kw)
        graph = samp(img, **kw)
        names = [op[0] for op in next(iter(samp._plans.values())).plan.ops]
        chunked = samp(img, trajectory=got7, tile_batch=7, **kw)
        sp = next(iter(samp._plans.values()))
        assert [n for _, n in sp.chunks] == [7, 7, 6]
        chunked_graph = samp(img, tile_batch=7, **kw)
    e, e7 = _traj_error(got, ref), _traj_error(got7, ref)
    e_batches = _traj_error(got7, [t.cpu() for t in got])
    print(f"tree B tiled 24x44: dpmpp2m vs its CPU loop {e:.3e}   tile_batch=7 {e7:.3e}   between the two {e_batches:.3e}   gate {limit:.3e}")
    assert names.count("hdiff_tile_dpmpp_step") == 1 and "hdiff_tile_ddim_step" not in names
    assert e <= limit and e7 <= limit and e_batches <= limit, (e, e7, e_batches, limit)
    assert torch.equal(eager.cpu(), torch.clip(got[-1].cpu(), -1, 1))
    assert torch.equal(graph, eager), "hipGraph replay and eager launches must agree bit for bit"
    assert torch.equal(chunked_graph, chunked)


# ----------------------------------------------------------------------------------------------------------------------
# e. what has not changed, the f16 mode, the drivers, the launch count
# ----------------------------------------------------------------------------------------------------------------------
def test_solver_ddim_is_the_call_without_the_argument():
    m, _, x_T, labels, _ = DA._traj_model()
    x_T, labels = x_T.to(DEV), labels.to(DEV)
    samp = DC.GaussianDiffusionSampler(m, *DA.TRAJ_BETA, DA.TRAJ["T"], w=1.8).to(DEV)
    with torch.no_grad():
        plain = samp(x_T, labels, ddim_steps=4)
        assert torch.equal(samp(x_T, labels, ddim_steps=4, solver="ddim"), plain)
        assert torch.equal(samp(x_T, labels, ddim_steps=4, solver="ddim", spacing="uniform"), plain)
        assert not torch.equal(samp(x_T, labels, ddim_steps=4, solver="dpmpp2m", spacing="uniform"), plain)
        assert torch.equal(samp(x_T, labels, ddim_steps=4), plain)                                   # and after the other solver
        torch.manual_seed(3); anc = samp(x_T, labels)
        torch.manual_seed(3); assert torch.equal(samp(x_T, labels, solver="ddim"), anc)
    img, y_T = _inputs_b(24, 40)
    img, y_T = img.to(DEV), y_T.to(DEV)
    sb = _sampler_b()
    with torch.no_grad():
        plain = sb(img, ddim=True, ddim_step=DDIM_STEP, y_T=y_T)
        assert torch.equal(sb(img, ddim=True, ddim_step=DDIM_STEP, y_T=y_T, solver="ddim"), plain)
        assert torch.equal(sb(img, ddim=True, ddim_step=DDIM_STEP, y_T=y_T, solver="ddim", spacing="uniform"), plain)
        assert torch.equal(sb(img, ddim=True, y_T=y_T, timesteps=list(range(0, 1000, 200))), plain)   # the same steps, given as a list
        assert not torch.equal(sb(img, ddim=True, ddim_step=DDIM_STEP, y_T=y_T, solver="dpmpp2m", spacing="uniform"), plain)
        assert torch.equal(sb(img, ddim=True, ddim_step=DDIM_STEP, y_T=y_T), plain)


def test_nan_and_f16_mode():
    m, _, x_T, labels, _ = DA._traj_model()
    samp = DC.GaussianDiffusionSampler(m, *DA.TRAJ_BETA, DA.TRAJ["T"], w=1.8).to(DEV)
    bad = x_T.clone().to(DEV)
    bad[0, 0, 0, 0] = float("nan")
    for kw in (dict(ddim_steps=4, solver="dpmpp2m"), dict(ddim_steps=4, solver="dpmpp2m", clip_x0=True)):
        with torch.no_grad(), pytest.raises(AssertionError, match="nan in tensor."):
            samp(bad, labels.to(DEV), **kw)
    # the opt-in f16 mode at a shape that reaches its attention kernel (d_head 16, L = 1024)
    torch.manual_seed(5)
    big = MC.UNet(T=20, num_labels=3, ch=128, ch_mult=[1, 2], num_res_blocks=1, dropout=0.0).eval().to(DEV)
    samp = DC.GaussianDiffusionSampler(big, 1e-4, 0.028, 20, w=1.8).to(DEV)
    x_T = torch.randn(1, 3, 32, 32, generator=torch.Generator().manual_seed(2)).to(DEV)
    before = hdiff_amd.get_contraction_mode()
    hdiff_amd.set_contraction_mode("f16")
    try:
        with torch.no_grad():
            y = samp(x_T, torch.tensor([2], device=DEV), ddim_steps=4, solver="dpmpp2m")
            bad = x_T.clone()
            bad[0, 1, 3, 3] = float("nan")
            with pytest.raises(AssertionError, match="nan in tensor."):
                samp(bad, torch.tensor([2], device=DEV), ddim_steps=4, solver="dpmpp2m")
    finally:
        hdiff_amd.set_contraction_mode(before)
    assert torch.isfinite(y).all() and float(y.min()) >= -1 and float(y.max()) <= 1 and float(y.abs().max()) > 0


def test_one_step_has_no_more_launches_than_a_ddim_step():
    m, _, _, _, _ = DA._traj_model()
    samp = DC.GaussianDiffusionSampler(m, *DA.TRAJ_BETA, DA.TRAJ["T"], w=1.8).to(DEV)
    sp = DC._SamplerPlan(samp, 2, 16, 16, torch.device(DEV))
    ddim_names = [op[0] for op in sp.variant(False, 0, ((1, 3, 7), 0.0, False)).ops]
    names = [op[0] for op in sp.variant(False, 0, ((1, 3, 7), 0.0, False), "dpmpp2m").ops]
    assert ddim_names[-1] == "hdiff_cfg_ddim_step_loop" and names[-1] == "hdiff_cfg_dpmpp_step_loop"
    assert names[:-1] == ddim_names[:-1] and len(names) <= len(ddim_names)
    sb = _sampler_b()
    dev = torch.device(DEV)
    for make in (lambda solver: DD._StepPlan(sb, 2, 24, 40, dev, DDIM_STEP, solver=solver),
                 lambda solver: DD._TiledStepPlan(sb, 2, 24, 44, dev, DDIM_STEP, TILE, OVERLAP, 7, solver=solver)):
        a, b = [op[0] for op in make("ddim").plan.ops], [op[0] for op in make("dpmpp2m").plan.ops]
        assert len(b) <= len(a) and [n.replace("dpmpp", "ddim") for n in b] == a and a != b


def test_drivers_reach_the_new_step(tmp_path, monkeypatch):
    # Evaluate.evaluate: the plan the sampler is left with holds the new update
    sb = _sampler_b()
    g = torch.Generator().manual_seed(5)
    batches = [(torch.randint(0, 256, (2, 3, 32, 32), generator=g, dtype=torch.uint8),
                torch.randint(0, 256, (2, 3, 32, 32), generator=g, dtype=torch.uint8))]
    torch.manual_seed(21)
    res = EV.evaluate(sb, batches, ddim_step=4, solver="dpmpp2m")
    names = [op[0] for op in next(iter(sb._plans.values())).plan.ops]
    assert res["n"] == 2 and "hdiff_dpmpp_step" in names and "hdiff_ddim_step" not in names
    torch.manual_seed(21)
    EV.evaluate(sb, batches, ddim_step=4)
    names = [op[0] for op in next(iter(sb._plans.values())).plan.ops]
    assert "hdiff_ddim_step" in names and "hdiff_dpmpp_step" not in names
    # TrainCondition.eval: the keys arrive as keywords, and the variant that ran ends in the new update
    cfg = {
        "state": "eval", "epoch": 10, "batch_size": 4, "T": 6, "channel": 32, "channel_mult": [1, 2], "num_res_blocks": 1,
        "dropout": 0.0, "lr": 2e-4, "multiplier": 2.5, "beta_1": 1e-4, "beta_T": 0.028, "img_size": 16, "grad_clip": 1.,
        "device": DEV, "w": 1.8, "save_dir": str(tmp_path / "ckpt"), "training_load_weight": None,
        "test_load_weight": "ckpt_0_.pt", "sampled_dir": str(tmp_path / "samples"),
        "sampledNoisyImgName": "noisy.png", "sampledImgName": "sampled.png", "nrow": 4,
        "dataset": "synthetic", "num_labels": 3, "num_workers": 0,
    }
    os.makedirs(cfg["save_dir"])
    torch.manual_seed(0)
    torch.save(TC._denoiser(cfg, "cpu").state_dict(), os.path.join(cfg["save_dir"], "ckpt_0_.pt"))
    seen = []

    class Recording(DC.GaussianDiffusionSampler):
        def forward(self, x_T, labels, **kw):
            out = super().forward(x_T, labels, **kw)
            (variant,) = next(iter(self._splans.values()))._variants.values()
            seen.append((kw, variant.ops[-1][0]))
            return out

    monkeypatch.setattr(TC, "GaussianDiffusionSampler", Recording)
    imgs = TC.eval(dict(cfg, ddim_steps=4, ddim_solver="dpmpp2m"))
    assert tuple(imgs.shape) == (4, 3, 16, 16) and float(imgs.min()) >= 0 and float(imgs.max()) <= 1
    assert seen[-1] == (dict(ddim_steps=4, eta=0.0, clip_x0=False, solver="dpmpp2m"), "hdiff_cfg_dpmpp_step_loop")
    TC.eval(dict(cfg, ddim_steps=3, ddim_solver="dpmpp2m", ddim_spacing="uniform", ddim_clip_x0=True))
    assert seen[-1] == (dict(ddim_steps=3, eta=0.0, clip_x0=True, solver="dpmpp2m", spacing="uniform"), "hdiff_cfg_dpmpp_step_loop")
    TC.eval(dict(cfg, ddim_steps=4))
    assert seen[-1] == (dict(ddim_steps=4, eta=0.0, clip_x0=False), "hdiff_cfg_ddim_step_loop")
