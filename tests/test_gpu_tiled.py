"""GPU checks of overlapping-window DDIM sampling (``GaussianDiffusionSampler.forward(tile=...)`` of the image-conditioned
tree): the two kernels bit for bit against their fp32 definition, one window against the untiled path bit for bit, and the loop
against its CPU definition (tests/_tiled_def.py) on a size the untiled sampler refuses, eager, through the hipGraph and in chunks.

Gate of the loop tests (``gate()``): the same measure -- for each step k of the pre-clip trajectory
``e_k = max|got - ref| / max(1, max|ref|)``, the largest over k -- taken for the existing untiled sampler against
``oracle.cpu_path_b.sampler_forward`` on a 24x40 input with the same model, schedule and seed; the tiled loop must stay within
2x that, with a floor of 2e-5.  The blend is a convex combination, so it adds no amplification of its own; the factor 2 allows
for different inputs and a few more roundings per pixel.  On the two CPU definitions the plain unweighted average over the
covering windows differs from the weighted blend by 7.1e-02 in this measure (seed 11), so a wrong weight table cannot pass.
The refusal of 24x44 in one piece is asserted on a model that halves three times, as the default model does (``deeper_sampler``):
the small fixture halves twice and takes that size, which is also why the untiled oracle can serve as the yardstick of the gate.
The tests print every figure before asserting; the values measured on an MI355X are in profiles/tiled_sampling.txt."""
import functools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hdiff_amd  # noqa: E402,F401
from hdiff_amd import _capi  # noqa: E402
from hdiff_amd.diffusion.Diffusion import GaussianDiffusionSampler  # noqa: E402
from oracle import cpu_path_b as OB  # noqa: E402

import _tiled_def as TD  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BETA_1, BETA_T, T_STEPS, DDIM_STEP = 1e-4, 0.02, 1000, 5
TILE, OVERLAP = 16, 8
SEED = 11


def stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def load_cfg():
    from _tree_b_small import load_small_dyn_unet
    return load_small_dyn_unet()


@functools.lru_cache(maxsize=None)
def small_model():
    _, cfg, m, sd = load_cfg()
    ocfg = OB.DynUNetConfig(T=cfg["T"], ch=cfg["ch"], ch_mult=tuple(cfg["ch_mult"]), num_res_blocks=cfg["num_res_blocks"])
    return m.to(DEV), ocfg, sd


def inputs(H, W):
    g = torch.Generator().manual_seed(SEED)
    img = torch.randint(0, 256, (2, 3, H, W), generator=g).float()
    return img, torch.randn(2, 3, H, W, generator=g)


@functools.lru_cache(maxsize=None)
def definition(weighted=True):
    """The CPU definition's pre-clip trajectory on 2x3x24x44 (computed once, shared, never modified)."""
    _, ocfg, sd = small_model()
    img, y_T = inputs(24, 44)
    traj = []
    with torch.no_grad():
        TD.tiled_sampler_forward(sd, ocfg, BETA_1, BETA_T, T_STEPS, img, y_T, DDIM_STEP, TILE, OVERLAP, trajectory=traj,
                                 weighted=weighted)
    return tuple(traj)


def traj_error(got, ref):
    assert len(got) == len(ref) == DDIM_STEP
    return max(((g.cpu() - r).abs().max() / max(1.0, r.abs().max().item())).item() for g, r in zip(got, ref))


def sampler():
    m, _, _ = small_model()
    return GaussianDiffusionSampler(m, BETA_1, BETA_T, T_STEPS).to(DEV)


def deeper_sampler():
    """A sampler around the small model's shape with one more level, i.e. the three halvings of the default model's short up
    path.  The small fixture itself halves twice (44 -> 22 -> 11 -> 22 -> 44) and so takes 24x44 in one piece; a model that
    halves three times refuses it, and that refusal is what the test asserts."""
    from hdiff_amd.diffusion.Model import DynamicUNet
    _, cfg, _, _ = load_cfg()
    torch.manual_seed(SEED)
    m = DynamicUNet(**dict(cfg, ch_mult=list(cfg["ch_mult"]) + [cfg["ch_mult"][-1]])).eval().to(DEV)
    return GaussianDiffusionSampler(m, BETA_1, BETA_T, T_STEPS).to(DEV)


@functools.lru_cache(maxsize=None)
def gate():
    """-> (gate, the untiled sampler's error): see the module docstring."""
    _, ocfg, sd = small_model()
    img, y_T = inputs(24, 40)
    ref, got = [], []
    with torch.no_grad():
        OB.sampler_forward(sd, ocfg, BETA_1, BETA_T, T_STEPS, img, y_T, ddim=True, ddim_step=DDIM_STEP, trajectory=ref)
        sampler()(img.to(DEV), ddim=True, ddim_step=DDIM_STEP, y_T=y_T.to(DEV), trajectory=got)
    e = traj_error(got, ref)
    return max(2.0 * e, 2e-5), e


class Tables:
    """Device tables of a layout, as the sampler builds them."""

    def __init__(self, lay):
        i32 = dict(dtype=torch.int32, device=DEV)
        self.oy, self.ox = torch.tensor(lay.oy, **i32), torch.tensor(lay.ox, **i32)
        self.fy, self.cy, self.wy = lay.fy.to(DEV), lay.cy.to(DEV), lay.wy.to(DEV).contiguous()
        self.fx, self.cx, self.wx = lay.fx.to(DEV), lay.cx.to(DEV), lay.wx.to(DEV).contiguous()


def run_tile_step(y, eps_w, tb, tab, k, flag, B, lay):
    step = torch.tensor([k], dtype=torch.int32, device=DEV)
    _capi.check(_capi.lib().hdiff_tile_ddim_step(
        y.data_ptr(), eps_w.data_ptr(), tb.fy.data_ptr(), tb.cy.data_ptr(), tb.wy.data_ptr(), tb.oy.data_ptr(), tb.fx.data_ptr(),
        tb.cx.data_ptr(), tb.wx.data_ptr(), tb.ox.data_ptr(), tab.data_ptr(), step.data_ptr(), int(tab.shape[0]), flag.data_ptr(),
        B, 3, lay.H, lay.W, lay.ny, lay.nx, lay.th, lay.tw, stream()), "tile_ddim_step")


def test_tile_gather_equals_slicing():
    lib = _capi.lib()
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 3, 24, 44, generator=g)
    lay = TD.Layout(24, 44, TILE, OVERLAP)
    want = TD.windows(x, lay)
    tb, dx = Tables(lay), x.to(DEV)
    for w0, n_slots in ((0, 20), (0, 7), (7, 7), (14, 7), (19, 3)):              # (14, 7): six windows and one padding slot
        out = torch.full((n_slots, 3, 16, 16), float("nan"), device=DEV)
        _capi.check(lib.hdiff_tile_gather(dx.data_ptr(), out.data_ptr(), tb.oy.data_ptr(), tb.ox.data_ptr(), 2, 3, 24, 44, lay.ny,
                                          lay.nx, 16, 16, w0, n_slots, stream()), "tile_gather")
        idx = [min(w0 + s, 19) for s in range(n_slots)]
        assert torch.equal(out.cpu(), want[idx]), (w0, n_slots)
    # one window smaller than the tile, and the copy form the sampler stores a chunk's estimates with
    x1 = torch.randn(2, 3, 7, 5, generator=g)
    zero = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = torch.empty(2, 3, 7, 5, device=DEV)
    _capi.check(lib.hdiff_tile_gather(x1.to(DEV).data_ptr(), out.data_ptr(), zero.data_ptr(), zero.data_ptr(), 2, 3, 7, 5, 1, 1, 7, 5,
                                      0, 2, stream()), "tile_gather")
    assert torch.equal(out.cpu(), x1)
    # origins outside the tensor are clamped into it, not read
    bad = torch.tensor([-5, 1000], dtype=torch.int32, device=DEV)
    out = torch.empty(4, 3, 16, 16, device=DEV)
    _capi.check(lib.hdiff_tile_gather(dx.data_ptr(), out.data_ptr(), bad.data_ptr(), bad.data_ptr(), 1, 3, 24, 44, 2, 2, 16, 16, 0, 4,
                                      stream()), "tile_gather")
    assert torch.equal(out[0].cpu(), x[0, :, 0:16, 0:16]) and torch.equal(out[3].cpu(), x[0, :, 8:24, 28:44])


def test_tile_ddim_step_bit_exact_in_place_and_nan_flag():
    g = torch.Generator().manual_seed(1)
    tab = OB.ddim_coefficients(OB.sampler_schedule(BETA_1, BETA_T, T_STEPS), DDIM_STEP)
    d_tab = tab.to(DEV).contiguous()
    lay = TD.Layout(24, 44, TILE, OVERLAP)
    cover = lay.cy[:, None] * lay.cx[None, :]
    assert {1, 2, 3, 6} <= set(cover.unique().tolist())
    tb = Tables(lay)
    y, eps_w = torch.randn(2, 3, 24, 44, generator=g), torch.randn(20, 3, 16, 16, generator=g)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    for k in range(DDIM_STEP):                                     # every row of the table; each step starts from the last
        d_y, d_e = y.to(DEV), eps_w.to(DEV)
        ptr = d_y.data_ptr()
        run_tile_step(d_y, d_e, tb, d_tab, k, flag, 2, lay)
        want = TD.ddim_update(y, TD.blend(eps_w, 2, lay), tab[k])
        assert d_y.data_ptr() == ptr and torch.equal(d_y.cpu(), want), k
        assert torch.equal(d_e.cpu(), eps_w)
        y = want
    assert int(flag.item()) == 0
    # a step counter outside the table is clamped, like hdiff_ddim_step's
    d_y = y.to(DEV)
    run_tile_step(d_y, eps_w.to(DEV), tb, d_tab, 99, flag, 2, lay)
    assert torch.equal(d_y.cpu(), TD.ddim_update(y, TD.blend(eps_w, 2, lay), tab[DDIM_STEP - 1]))
    # one NaN in a window raises the flag and reaches exactly the pixels that window element covers
    bad = eps_w.clone()
    bad[13, 1, 5, 9] = float("nan")                                # window (b, iy, ix) = (1, 0, 3): pixel (5, 24 + 9)
    d_y = y.to(DEV)
    run_tile_step(d_y, bad.to(DEV), tb, d_tab, 2, flag, 2, lay)
    assert int(flag.item()) == 1
    nan = torch.isnan(d_y.cpu())
    assert int(nan.sum()) == 1 and bool(nan[1, 1, 5, 33])
    # 7x5 image, tile 16: one window smaller than the tile, weight 1.0 -- hdiff_ddim_step bit for bit
    lay1 = TD.Layout(7, 5, TILE, 2)
    tb1 = Tables(lay1)
    y1, e1 = torch.randn(2, 3, 7, 5, generator=g), torch.randn(2, 3, 7, 5, generator=g)
    flag1 = torch.zeros(1, dtype=torch.int32, device=DEV)
    for k in range(DDIM_STEP):
        d_y, d_e, old = y1.to(DEV), e1.to(DEV), torch.empty(2, 3, 7, 5, device=DEV)
        step = torch.tensor([k], dtype=torch.int32, device=DEV)
        _capi.check(_capi.lib().hdiff_ddim_step(d_y.data_ptr(), d_e.data_ptr(), old.data_ptr(), d_tab.data_ptr(), step.data_ptr(),
                                                DDIM_STEP, flag1.data_ptr(), y1.numel(), stream()), "ddim_step")
        run_tile_step(d_y, d_e, tb1, d_tab, k, flag1, 2, lay1)
        assert torch.equal(d_y, old) and torch.equal(old.cpu(), TD.ddim_update(y1, e1, tab[k])), k
    assert int(flag1.item()) == 0
    bad1 = e1.clone()
    bad1[1, 2, 6, 4] = float("nan")                                # the last element of the last window
    d_y = y1.to(DEV)
    run_tile_step(d_y, bad1.to(DEV), tb1, d_tab, 0, flag1, 2, lay1)
    nan = torch.isnan(d_y.cpu())
    assert int(flag1.item()) == 1 and int(nan.sum()) == 1 and bool(nan[1, 2, 6, 4])


def test_one_window_is_the_untiled_path_bit_for_bit():
    img, y_T = inputs(24, 40)
    img, y_T = img.to(DEV), y_T.to(DEV)
    samp = sampler()
    with torch.no_grad():
        t_old, t_new = [], []
        eager_old = samp(img, ddim=True, ddim_step=DDIM_STEP, y_T=y_T, trajectory=t_old)
        eager_new = samp(img, ddim=True, ddim_step=DDIM_STEP, y_T=y_T, trajectory=t_new, tile=64)
        assert torch.equal(eager_new, eager_old) and len(t_new) == len(t_old) == DDIM_STEP
        assert all(torch.equal(a, b) for a, b in zip(t_new, t_old))
        graph_old = samp(img, ddim=True, ddim_step=DDIM_STEP, y_T=y_T)
        graph_new = samp(img, ddim=True, ddim_step=DDIM_STEP, y_T=y_T, tile=64)
        assert torch.equal(graph_new, graph_old) and torch.equal(graph_old, eager_old)
        assert torch.equal(samp(img, ddim=True, ddim_step=DDIM_STEP, y_T=y_T, tile=64, tile_overlap=0, tile_batch=2), graph_old)


def test_tiled_loop_matches_its_definition_on_a_size_three_halvings_refuse():
    img, y_T = inputs(24, 44)
    samp = sampler()
    with torch.no_grad(), pytest.raises(RuntimeError, match="must match the size of tensor b"):
        deeper_sampler()(img.to(DEV), ddim=True, ddim_step=DDIM_STEP, y_T=y_T.to(DEV))   # 44 -> 22 -> 11 -> 6 -> 12 -> 24 -> 48
    limit, e_untiled = gate()
    ref = definition()
    got = []
    with torch.no_grad():
        out = samp(img.to(DEV), ddim=True, ddim_step=DDIM_STEP, y_T=y_T.to(DEV), trajectory=got, tile=TILE, tile_overlap=OVERLAP)
    e_tiled = traj_error(got, ref)
    e_plain = traj_error(definition(weighted=False), ref)
    print(f"untiled sampler vs oracle (24x40): {e_untiled:.3e}   tiled loop vs definition (24x44): {e_tiled:.3e}   gate {limit:.3e}   "
          f"plain average vs weighted definition: {e_plain:.3e}")
    assert all(tuple(t.shape) == (2, 3, 24, 44) for t in got) and all(torch.isfinite(r).all() for r in ref)
    assert e_plain > 10 * limit, "the input cannot tell a wrong weight table from the right one: choose another seed"
    assert e_tiled <= limit, (e_tiled, limit)
    assert torch.equal(out.cpu(), torch.clip(got[-1].cpu(), -1, 1))


def test_graph_equals_eager_and_chunks_stay_within_the_gate():
    img, y_T = inputs(24, 44)
    img, y_T = img.to(DEV), y_T.to(DEV)
    samp = sampler()
    limit, _ = gate()
    ref = definition()
    kw = dict(ddim=True, ddim_step=DDIM_STEP, y_T=y_T, tile=TILE, tile_overlap=OVERLAP)
    with torch.no_grad():
        traj = []
        eager = samp(img, trajectory=traj, **kw)
        graph = samp(img, **kw)
        assert torch.equal(graph, eager), "hipGraph replay and eager launches must agree bit for bit"
        got = []
        chunked = samp(img, trajectory=got, tile_batch=7, **kw)
        sp = next(iter(samp._plans.values()))
        assert [n for _, n in sp.chunks] == [7, 7, 6] and sp.n_slots == 7        # the last chunk carries one padding slot
        e_chunked = traj_error(got, ref)
        print(f"tile_batch=7 vs definition: {e_chunked:.3e}   gate {limit:.3e}")
        assert e_chunked <= limit, (e_chunked, limit)
        a = samp(img, tile_batch=7, **kw)
        b = samp(img, tile_batch=7, **kw)
        assert torch.equal(a, b) and torch.equal(a, chunked), "the chunked loop must be bitwise repeatable, graph and eager"
