"""Shared by tests/test_wgrad_fast_cases_cpu.py (no GPU) and tests/test_gpu_wgrad_fast.py: the cases, split counts, one-hot probes,
references and gates for the two fast weight-gradient kernels of conv_wgrad3x3.hip (conv_wgrad3x3_kernel: 2 x 32 pixel tiles,
32 input x 128 output channels per workgroup; conv_wgrad1x1_kernel: 64 consecutive pixels of the flattened plane, 128 x 128 channels).

Both kernels accumulate in fp32 MFMA and hdiff_conv_wgrad_unpack adds the splits' slabs in split order.  With ONE operand one-hot
per channel (a single +-2^e, e in [-3, 3]) every dW element is one exact product plus zeros, so the expected tensor is known bit for
bit, whatever the split count:

  dy_probes   dY[b_co, co, y_co, x_co] = v_co, zero elsewhere, the activation dense:
              dW[co, ci, ky, kx] = v_co * Apad[b_co, ci, y_co + ky - 1, x_co + kx - 1]      (1x1: v_co * X[b_co, ci, p_co])
  x_probes    X[b_ci, ci, y_ci, x_ci] = v_ci, zero elsewhere, dY dense:
              dW[co, ci, ky, kx] = v_ci * dY[b_ci, co, y_ci - ky + 1, x_ci - kx + 1], zero outside the plane

The position tables hit all four corner pixels and one interior pixel of every tile of every image (1x1: pixels 0, 3, 4 and 63 of
every 64-pixel tile -- both ends of the first 16-byte load, the start of the second, the tile's last -- and one other); `uncovered`
is the condition the tests hold them to.

Gates (none comes from a kernel's output):
  exact           torch.equal -- the probes without prologue.
  activation      behind GroupNorm + Swish (and dropout) the activation itself is rounded:  |got - ref| <= (8 + 4 |v|) 2^-24 |ref|
                  per element, v = x * scale + shift the pre-activation.  One rounding in the fma; Swish's relative condition number is
                  at most 1 + |v|; __expf adds (|v| + 2) ulp (the rounded v * log2(e), then v_exp_f32), the reciprocal 1 ulp, two
                  multiplies follow (by v, by 1 / keep): (1 + |v|) + (|v| + 2) + 1 + 2 = 6 + 2 |v| units of 2^-24, so the gate has
                  about 2 x slack.  Padding and dropped elements: exactly 0.
  dense, per op   1e-4 * max |ref| + 1e-6, the weight-gradient gate of tests/test_gpu_backward.py.
  dense, sum      the worst case of an fp32 sum, per element: (pixels of the longest split + nsplit) 2^-24 sum |dY * A| (float64, over
                  the element's own terms), plus 2^-24 sum (8 + 4 |v|) |dY * A| behind a prologue.  Loose by about sqrt(K) -- and still
                  a whole tile's contribution away from a tile that was skipped, counted twice or read from a stale buffer.

`simulate` is the kernels' formula in float64 with one defect built in; the CPU test shows that the gates reject each."""
import collections
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _strided_geometry_cases as K  # noqa: E402

U = 2.0 ** -24          # unit roundoff of fp32
TILE = 64               # pixels per tile, both kernels

Case = collections.namedtuple("Case", "id route k C0 C1 cout H W B tiles odd what")

# odd: a split count that does not divide the tile count -- the splits walk different numbers of tiles, the deepest two (3 and 6
# tiles, where no such count gives more) or three: both buffer parities are used and the last `more` is false at different depths
CASES = [
    Case("3x3-2x32", K.FAST_3X3, 3, 32, 0, 256, 2, 32, 3, 3, 2,
         "the tile is the plane: top, bottom, left and right padding at once; two output-channel workgroups (co0 = 128)"),
    Case("3x3-4x64", K.FAST_3X3, 3, 64, 32, 128, 4, 64, 3, 12, 5,
         "2x2 tiles, each two borders and two interior seams; three input-channel workgroups, the last reading x1 (another batch stride)"),
    Case("3x3-6x96", K.FAST_3X3, 3, 32, 0, 128, 6, 96, 2, 18, 7, "3x3 tiles: one fully interior tile per image"),
    Case("1x1-8x8", K.FAST_1X1, 1, 32, 0, 128, 8, 8, 5, 5, 2, "one tile per image; 96 of the workgroup's 128 input columns are dead"),
    Case("1x1-seam", K.FAST_1X1, 1, 40, 24, 128, 8, 16, 3, 6, 4,
         "the concat seam off the 16-row staging grid; the two sources have different batch strides"),
    Case("1x1-160", K.FAST_1X1, 1, 96, 64, 256, 16, 16, 2, 8, 3,
         "two input-channel workgroups, the second with 32 live channels; two output-channel workgroups"),
]
CASE_IDS = [c.id for c in CASES]
CASES_3X3 = [c.id for c in CASES if c.k == 3]
CASES_DROPOUT = ["3x3-2x32", "3x3-6x96"]          # the dropout form takes no concat input
CASES_CONCAT = [c.id for c in CASES if c.C1]
SPLITS = ("one", "odd", "all")                    # "all" = total_tiles, which is also the library's own answer for every case here
DROP_P = 0.15                                     # keep 0.85


def case(cid):
    return CASES[CASE_IDS.index(cid)]


def cin_of(c):
    return c.C0 + c.C1


def desc(c, gn=False):
    return K.plain_desc(c.k, c.C0, c.cout, c.B, c.H, c.W, C1=c.C1, gn=gn)


def nsplit_of(c, which):
    return {"one": 1, "odd": c.odd, "all": c.tiles}[which]


def tiles_per_image(c):
    return (c.H // 2) * (c.W // 32) if c.k == 3 else c.H * c.W // TILE


def tiles_of_split(c, nsplit, split):
    """the tiles (numbered through the batch) workgroup `split` walks, in order"""
    return list(range(split, c.B * tiles_per_image(c), nsplit))


def longest_split(c, nsplit):
    return -(-c.B * tiles_per_image(c) // nsplit)


def tile_pixels(c, ti):
    """the 64 (y, x) of tile ti of an image, in the kernel's pixel order"""
    if c.k == 3:
        ty, tx = divmod(ti, c.W // 32)
        return [(2 * ty + r, 32 * tx + j) for r in range(2) for j in range(32)]
    return [divmod(TILE * ti + j, c.W) for j in range(TILE)]


def corner_slots(c):
    """positions inside a tile every table set must hit: the four corners / pixels 0, 3, 4, 63"""
    return (0, 31, 32, 63) if c.k == 3 else (0, 3, 4, 63)


def interior_slots(c):
    """3x3: neither the first nor the last column of the tile; 1x1: any other pixel"""
    if c.k == 3:
        return [j for j in range(TILE) if 1 <= j % 32 <= 30]
    return [j for j in range(TILE) if j not in corner_slots(c)]


# ---- position tables and probes ---------------------------------------------------------------------------------------------------
Table = collections.namedtuple("Table", "b y x v")          # per channel: image, row, column (int64) and value (float64)
Probe = collections.namedtuple("Probe", "x0 x1 dy table")   # float32 operands of one launch


def _randint(g, n):
    return int(torch.randint(0, n, (1,), generator=g).item())


def tables(c, nchan, seed):
    """-> [Table]: as many rounds as the required positions (five per tile) need at nchan channels per round; channels left over
    in a round probe random pixels; which channel probes which position is a seeded permutation."""
    g = torch.Generator().manual_seed(seed)
    inner = interior_slots(c)
    req = []
    for b in range(c.B):
        for ti in range(tiles_per_image(c)):
            px = tile_pixels(c, ti)
            req += [(b,) + px[j] for j in corner_slots(c)]
            req.append((b,) + px[inner[_randint(g, len(inner))]])
    req = [req[i] for i in torch.randperm(len(req), generator=g).tolist()]
    out = []
    for r in range(-(-len(req) // nchan)):
        chunk = req[r * nchan:(r + 1) * nchan]
        while len(chunk) < nchan:
            chunk.append((_randint(g, c.B), _randint(g, c.H), _randint(g, c.W)))
        chunk = [chunk[i] for i in torch.randperm(nchan, generator=g).tolist()]
        pos = torch.tensor(chunk, dtype=torch.int64)
        e = torch.randint(-3, 4, (nchan,), generator=g).double()
        s = torch.randint(0, 2, (nchan,), generator=g).double() * 2 - 1
        out.append(Table(pos[:, 0], pos[:, 1], pos[:, 2], s * torch.exp2(e)))
    return out


def uncovered(c, tabs):
    """the tile-corner pixels the tables leave out, and the tiles without an interior hit: [(image, tile, what)]"""
    hit = set()
    for t in tabs:
        hit |= set(zip(t.b.tolist(), t.y.tolist(), t.x.tolist()))
    missing = []
    for b in range(c.B):
        for ti in range(tiles_per_image(c)):
            px = tile_pixels(c, ti)
            missing += [(b, ti, "pixel %d" % j) for j in corner_slots(c) if (b,) + px[j] not in hit]
            if not any((b,) + px[j] in hit for j in interior_slots(c)):
                missing.append((b, ti, "interior"))
    return missing


def dense_inputs(c, seed):
    """seeded randn x0, x1 (None without a concat input) and dY"""
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(c.B, c.C0, c.H, c.W, generator=g)
    x1 = torch.randn(c.B, c.C1, c.H, c.W, generator=g) if c.C1 else None
    dy = torch.randn(c.B, c.cout, c.H, c.W, generator=g)
    return x0, x1, dy


def one_hot(c, nchan, t):
    z = torch.zeros(c.B, nchan, c.H, c.W)
    z[t.b, torch.arange(nchan), t.y, t.x] = t.v.float()
    return z


def dy_probes(c, seed):
    x0, x1, _ = dense_inputs(c, seed)
    return [Probe(x0, x1, one_hot(c, c.cout, t), t) for t in tables(c, c.cout, seed + 1)]


def x_probes(c, seed):
    _, _, dy = dense_inputs(c, seed)
    out = []
    for t in tables(c, cin_of(c), seed + 2):
        x = one_hot(c, cin_of(c), t)
        out.append(Probe(x[:, :c.C0].contiguous(), x[:, c.C0:].contiguous() if c.C1 else None, dy, t))
    return out


def cat(x0, x1):
    return x0 if x1 is None else torch.cat([x0, x1], dim=1)


def expected_dy_probe(c, act, t):
    """act: the [B, Cin, H, W] tensor the conv read (the ACTIVATED one behind a prologue) -> float64 dW"""
    a = act.double()
    dw = torch.zeros(c.cout, cin_of(c), c.k, c.k, dtype=torch.float64)
    if c.k == 1:
        dw[:, :, 0, 0] = t.v[:, None] * a[t.b, :, t.y, t.x]
        return dw
    ap = F.pad(a, (1, 1, 1, 1))                  # the conv pads the activated tensor with zeros
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = t.v[:, None] * ap[t.b, :, t.y + ky, t.x + kx]
    return dw


def expected_x_probe(c, dy, t):
    d = dy.double()
    dw = torch.zeros(c.cout, cin_of(c), c.k, c.k, dtype=torch.float64)
    if c.k == 1:
        dw[:, :, 0, 0] = (t.v[:, None] * d[t.b, :, t.y, t.x]).t()
        return dw
    dp = F.pad(d, (1, 1, 1, 1))
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = (t.v[:, None] * dp[t.b, :, t.y - ky + 2, t.x - kx + 2]).t()
    return dw


# ---- float64 references -----------------------------------------------------------------------------------------------------------
def activation_f64(x, scale, shift, keep=None, inv_keep=1.0):
    """-> (swish(v) [* keep * inv_keep], v) with v = x * scale + shift, scale / shift per (sample, channel); all float64"""
    v = x.double() * scale.double()[:, :, None, None] + shift.double()[:, :, None, None]
    a = v * torch.sigmoid(v)
    if keep is not None:
        a = a * keep.double() * float(inv_keep)
    return a, v


def wgrad_f64(c, act, dy):
    a, d = act.double(), dy.double()
    if c.k == 1:
        return torch.einsum("bohw,bchw->oc", d, a)[:, :, None, None].clone()
    ap = F.pad(a, (1, 1, 1, 1))
    dw = torch.empty(c.cout, cin_of(c), 3, 3, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = torch.einsum("bohw,bchw->oc", d, ap[:, :, ky:ky + c.H, kx:kx + c.W])
    return dw


# ---- gates ------------------------------------------------------------------------------------------------------------------------
def exact(got, want):
    """bit for bit: want is float64 and, for a probe without prologue, a float32 value"""
    return torch.equal(got.detach().cpu().double(), want)


def activation_ratio(got, ref, vabs):
    """-> (worst err / gate over the elements with ref != 0, whether every element with ref == 0 is exactly 0); vabs: |v| of the
    one activation element behind each dW element (expected_dy_probe of |v| with unit values)"""
    got = got.detach().cpu().double()
    live = ref != 0
    zeros_exact = bool((got[~live] == 0).all())
    gate = (8 + 4 * vabs[live]) * U * ref[live].abs()
    return ((got[live] - ref[live]).abs() / gate).max().item(), zeros_exact


def dense_ratios(c, got, ref, abs_sum, nsplit, act_sum=None):
    """-> (err / per-op gate, worst err / summation bound); abs_sum = wgrad_f64(|A|, |dY|), act_sum = wgrad_f64((8 + 4 |v|) |A|, |dY|)"""
    err = (got.detach().cpu().double() - ref).abs()
    r_op = err.max().item() / (1e-4 * ref.abs().max().item() + 1e-6)
    bound = (TILE * longest_split(c, nsplit) + nsplit) * U * abs_sum
    if act_sum is not None:
        bound = bound + U * act_sum
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return r_op, r.max().item()


# ---- the kernels' formula with one defect built in --------------------------------------------------------------------------------
DEFECTS = ("shift", "skip", "twice", "stride")


def simulate(c, act, dy, defect=None, nsplit=1):
    """float64 dW of act [B, Cin, H, W] and dy, as a kernel would give it that
      shift   staged the patch one column off (1x1: one pixel off in the flattened plane),
      skip    left out the last tile of split 0 (nsplit splits),
      twice   counted that tile twice,
      stride  stepped x1 from image to image by x0's batch stride (wrapping inside x1)."""
    a, d = act.double(), dy.double()
    if defect == "shift":
        flat = a.reshape(c.B, cin_of(c), -1) if c.k == 1 else a
        a = F.pad(flat, (1, 0))[..., :-1].reshape(a.shape)
    elif defect == "stride":
        assert c.C1
        hw = c.H * c.W
        flat = a[:, c.C0:].contiguous().reshape(-1)
        idx = (torch.arange(c.B)[:, None, None] * (c.C0 * hw) + torch.arange(c.C1)[None, :, None] * hw + torch.arange(hw)[None, None, :])
        a = torch.cat([a[:, :c.C0], flat[idx % flat.numel()].reshape(c.B, c.C1, c.H, c.W)], dim=1)
    elif defect in ("skip", "twice"):
        t = tiles_of_split(c, nsplit, 0)[-1]
        b, ti = divmod(t, tiles_per_image(c))
        ys, xs = zip(*tile_pixels(c, ti))
        d = d.clone()
        d[b, :, list(ys), list(xs)] *= 0.0 if defect == "skip" else 2.0
    else:
        assert defect is None
    return wgrad_f64(c, a, d)
