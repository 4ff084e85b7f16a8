"""TEST INFRASTRUCTURE ONLY -- the definition of overlapping-window DDIM sampling (``GaussianDiffusionSampler.forward(tile=...)``
of hdiff_amd/diffusion/Diffusion.py) on the CPU, in torch fp32.

Per step: every window of the full-size ``y_t`` and of the conditioning image is cropped, the stacked windows go through
``oracle.cpu_path_b.dyn_unet_forward`` in one batch, the noise estimates are blended with ``tile_weights`` -- for each pixel the
sum over the covering windows, rows outer, columns inner, ascending, of ``(ay * ax) * eps``, the first product initialising the
sum -- and the reference's DDIM update (oracle ``ddim_coefficients`` / ``ddim_sequence``) is applied to the full image."""
import torch

from oracle import cpu_path_b as OB

from hdiff_amd.diffusion.Diffusion import tile_origins, tile_weights


class Layout:
    """Window layout of a [B, C, H, W] tensor: origins and the (first, count, fp32 weight) tables per axis."""

    def __init__(self, H, W, tile, overlap):
        self.H, self.W, self.th, self.tw = H, W, min(tile, H), min(tile, W)
        self.oy, self.ox = tile_origins(H, tile, overlap), tile_origins(W, tile, overlap)
        self.ny, self.nx = len(self.oy), len(self.ox)
        self.fy, self.cy, wy = tile_weights(H, tile, overlap)
        self.fx, self.cx, wx = tile_weights(W, tile, overlap)
        self.wy, self.wx = wy.float(), wx.float()            # normalised in float64, cast to fp32 once


def windows(x, lay):
    """[B, C, H, W] -> [B * ny * nx, C, th, tw], window index (b * ny + iy) * nx + ix."""
    return torch.stack([x[b, :, oy:oy + lay.th, ox:ox + lay.tw] for b in range(x.shape[0]) for oy in lay.oy for ox in lay.ox])


def blend(eps_w, B, lay, weighted=True):
    """The blended noise estimate [B, C, H, W] of the windows' estimates eps_w [B * ny * nx, C, th, tw].  ``weighted=False`` is
    the plain average over the covering windows (what a wrong weight table would give) -- used to show that the gate of the
    GPU test can tell the two apart."""
    Cc = eps_w.shape[1]
    e = eps_w.view(B, lay.ny, lay.nx, Cc, lay.th, lay.tw)
    oy, ox = torch.tensor(lay.oy), torch.tensor(lay.ox)
    py, px = torch.arange(lay.H), torch.arange(lay.W)
    acc = None
    for jy in range(3):
        iy = torch.clamp(lay.fy.long() + jy, max=lay.ny - 1)
        ly = torch.clamp(py - oy[iy], 0, lay.th - 1)
        for jx in range(3):
            ix = torch.clamp(lay.fx.long() + jx, max=lay.nx - 1)
            lx = torch.clamp(px - ox[ix], 0, lay.tw - 1)
            v = e[:, iy[:, None], ix[None, :], :, ly[:, None], lx[None, :]].permute(2, 3, 0, 1)      # [H, W, B, C] -> [B, C, H, W]
            if weighted:
                term = (lay.wy[:, jy][:, None] * lay.wx[:, jx][None, :]) * v
            else:
                term = v
            if acc is None:
                acc = term                                    # (0, 0) covers every pixel: count >= 1 on both axes
            else:
                on = (jy < lay.cy)[:, None] & (jx < lay.cx)[None, :]
                acc = torch.where(on, acc + term, acc)
    if not weighted:
        acc = acc / (lay.cy[:, None] * lay.cx[None, :]).float()
    return acc


def ddim_update(y, eps, row):
    """Diffusion.py:259-263 with eta = 0, row = [sqrt(1 - at), sqrt(at), sqrt(at_next), c2] in fp32."""
    y0 = (y - eps * row[0]) / row[1]
    return row[2] * y0 + row[3] * eps


def tiled_sampler_forward(sd, cfg, beta_1, beta_T, T, input_image, y_T, ddim_step, tile, overlap, trajectory=None, weighted=True):
    """-> the image clipped to [-1, 1]; ``trajectory`` collects the full-size pre-clip y_t after every step."""
    sched = OB.sampler_schedule(beta_1, beta_T, T)
    tab = OB.ddim_coefficients(sched, ddim_step)
    img = input_image.float() / 255.0
    B, _, H, W = img.shape
    lay = Layout(H, W, tile, overlap)
    cond_w = windows(img, lay)
    y = y_T
    for k, (i, _) in enumerate(OB.ddim_sequence(ddim_step)):
        t = torch.full((cond_w.shape[0],), i, dtype=torch.long)
        eps_w = OB.dyn_unet_forward(sd, cfg, torch.cat([cond_w, windows(y, lay)], dim=1).float(), t)
        y = ddim_update(y, blend(eps_w, B, lay, weighted), tab[k])
        if trajectory is not None:
            trajectory.append(y)
    return torch.clip(y, -1, 1)
