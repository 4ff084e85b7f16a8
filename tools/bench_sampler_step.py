"""Bench tool: per-launch time of the samplers' update kernels (csrc/sampler_step.hip) through _capi, for whichever library
HDIFF_LIB names (default: the tree's libhdiff.so) -- so the same script times this tree and a library built from another revision.

  [HDIFF_LIB=/path/to/libhdiff.so] python tools/bench_sampler_step.py

Method: hip events around 200 back-to-back launches after 20 warm-up launches, median of five such repeats, one JSON line per entry
point.  Untiled kernels: n = 8 * 3 * 256 * 256, the headline state; window kernels: B = 1, 3 x 512 x 512 with tile 256, overlap 32.
The seven single-step entry points run at a fixed position (k = 100 of 1000) with the kernel drawing its own noise where it adds
any; the three `_loop` entry points of the label-conditioned sampler -- the same kernels with the captured loop's bookkeeping, as
the sampler launches them -- count down from 999, re-armed before every repeat.  Updates are out of place where the entry point
allows it, so the state stays finite over the launches (a NaN would add the flag's atomics to the time)."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_sampler_step.py needs an MI355X (there is no CPU path to time)")

from hdiff_amd import _capi, schedules  # noqa: E402
from hdiff_amd.diffusion.Diffusion import tile_origins, tile_weights  # noqa: E402

LAUNCHES, WARMUP, REPEATS = 200, 20, 5
T, K, W_GUIDE, SEED = 1000, 100, 1.8, 42
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
lib = _capi.lib()
stream = torch.cuda.current_stream(dev).cuda_stream
g = torch.Generator().manual_seed(0)


def rand(*shape):
    return torch.randn(*shape, generator=g).to(dev)


i32 = dict(dtype=torch.int32, device=dev)
betas = torch.linspace(1e-4, 0.02, T).double()
tau = list(range(T))
ddim5 = schedules.ddim_table(betas, tau, 1.0).float().contiguous().to(dev)             # eta = 1: every step above 0 adds noise
ddim4 = schedules.ddim_table(betas, tau, 0.0)[:, :4].float().contiguous().to(dev)  # the image-conditioned step's four columns
dpmpp = schedules.dpmpp_table(betas, tau).float().contiguous().to(dev)
t_tab = torch.tensor(tau, dtype=torch.int64, device=dev)
alphas = 1. - betas
ab = torch.cumprod(alphas, dim=0)
c1 = torch.sqrt(1. / alphas)
c2 = (c1 * (1. - alphas) / torch.sqrt(1. - ab)).float().to(dev)
c1, sigma = c1.float().to(dev), torch.sqrt(betas.float()).to(dev)
step, flag = torch.tensor([K], **i32), torch.zeros(1, **i32)
done = torch.zeros(1, **i32)

# untiled: the headline state
B, n = 8, 8 * 3 * 256 * 256
x, ec, eu, out, hist = rand(n), rand(n), rand(n), torch.empty(n, device=dev), torch.zeros(n, device=dev)
x2, t2 = torch.empty(2 * n, device=dev), torch.zeros(2 * B, dtype=torch.int64, device=dev)   # the next UNet input and time vector

# windows
H = Wd = 512
TILE, OVERLAP = 256, 32
oy, ox = tile_origins(H, TILE, OVERLAP), tile_origins(Wd, TILE, OVERLAP)
fy, cy, wy = tile_weights(H, TILE, OVERLAP)
fx, cx, wx = tile_weights(Wd, TILE, OVERLAP)
ny, nx = len(oy), len(ox)
doy, dox = torch.tensor(oy, **i32), torch.tensor(ox, **i32)
fy, cy, wy, fx, cx, wx = fy.to(dev), cy.to(dev), wy.float().to(dev).contiguous(), fx.to(dev), cx.to(dev), wx.float().to(dev).contiguous()
y_img, hist_img, eps_w = rand(3 * H * Wd), torch.zeros(3 * H * Wd, device=dev), rand(ny * nx * 3 * TILE * TILE)
tables = (fy, cy, wy, doy, fx, cx, wx, dox)


def loop_desc(cls, **extra):
    d = cls()
    d.x, d.eps_c, d.eps_u, d.x_next = x.data_ptr(), ec.data_ptr(), eu.data_ptr(), out.data_ptr()
    d.step_ptr, d.w, d.nan_flag, d.n = step.data_ptr(), W_GUIDE, flag.data_ptr(), n
    d.x_dup0, d.x_dup1, d.t_next, d.t_count = x2.data_ptr(), x2.data_ptr() + 4 * n, t2.data_ptr(), 2 * B
    d.done_counter = done.data_ptr()
    for name, v in extra.items():
        setattr(d, name, v)
    return d


ddpm_d = loop_desc(_capi.DdpmLoopDesc, noise=None, seed=SEED, coeff1=c1.data_ptr(), coeff2=c2.data_ptr(), sigma=sigma.data_ptr(), T=T)
ddim_d = loop_desc(_capi.CfgDdimLoopDesc, noise=None, seed=SEED, tab=ddim5.data_ptr(), t_tab=t_tab.data_ptr(), nsteps=T, clip_x0=0)
dpmpp_d = loop_desc(_capi.CfgDpmppLoopDesc, x0_prev=hist.data_ptr(), tab=dpmpp.data_ptr(), t_tab=t_tab.data_ptr(), nsteps=T, clip_x0=0)

P = lambda t: t.data_ptr()  # noqa: E731
CASES = [   # (entry point, first value of the counter, the launch)
    ("hdiff_ddpm_step", K, lambda: lib.hdiff_ddpm_step(P(x), P(ec), P(eu), None, P(out), P(c1), P(c2), P(sigma), P(step), T,
                                                      C.c_double(W_GUIDE), C.c_uint64(SEED), P(flag), n, stream)),
    ("hdiff_cfg_ddim_step", K, lambda: lib.hdiff_cfg_ddim_step(P(x), P(ec), P(eu), None, P(out), P(ddim5), P(step), T,
                                                              C.c_double(W_GUIDE), 0, C.c_uint64(SEED), P(flag), n, stream)),
    ("hdiff_cfg_dpmpp_step", K, lambda: lib.hdiff_cfg_dpmpp_step(P(x), P(ec), P(eu), P(out), P(hist), P(dpmpp), P(step), T,
                                                                C.c_double(W_GUIDE), 0, P(flag), n, stream)),
    ("hdiff_ddpm_step_loop", T - 1, lambda: lib.hdiff_ddpm_step_loop(C.byref(ddpm_d), stream)),
    ("hdiff_cfg_ddim_step_loop", T - 1, lambda: lib.hdiff_cfg_ddim_step_loop(C.byref(ddim_d), stream)),
    ("hdiff_cfg_dpmpp_step_loop", T - 1, lambda: lib.hdiff_cfg_dpmpp_step_loop(C.byref(dpmpp_d), stream)),
    ("hdiff_ddim_step", K, lambda: lib.hdiff_ddim_step(P(x), P(ec), P(out), P(ddim4), P(step), T, P(flag), n, stream)),
    ("hdiff_dpmpp_step", K, lambda: lib.hdiff_dpmpp_step(P(x), P(ec), P(out), P(hist), P(dpmpp), P(step), T, 0, P(flag), n, stream)),
    ("hdiff_tile_ddim_step", K, lambda: lib.hdiff_tile_ddim_step(P(y_img), P(eps_w), *map(P, tables), P(ddim4), P(step), T,
                                                                P(flag), 1, 3, H, Wd, ny, nx, TILE, TILE, stream)),
    ("hdiff_tile_dpmpp_step", K, lambda: lib.hdiff_tile_dpmpp_step(P(y_img), P(eps_w), P(hist_img), *map(P, tables), P(dpmpp),
                                                                  P(step), T, 0, P(flag), 1, 3, H, Wd, ny, nx, TILE, TILE, stream)),
]

for name, first, launch in CASES:
    def run(count):
        step.fill_(first)
        done.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(count):
            _capi.check(launch(), name)
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) * 1e3 / count

    y_img.copy_(rand(3 * H * Wd))
    run(WARMUP)
    us = sorted(run(LAUNCHES) for _ in range(REPEATS))
    assert int(flag.item()) == 0, f"{name}: the state went NaN, the time includes the flag's atomics"
    print(json.dumps({"entry": name, "us_per_launch_median": round(us[REPEATS // 2], 3), "us_min": round(us[0], 3),
                      "us_max": round(us[-1], 3), "launches": LAUNCHES, "repeats": REPEATS, "lib": os.path.basename(_capi.LIB_PATH),
                      "gpu": torch.cuda.get_device_name(dev)}), flush=True)
