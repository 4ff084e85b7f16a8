"""GPU checks of the guided full-resolution transfer (csrc/transfer.hip, hdiff_amd/transfer.py) and of its hook into the evaluation
loop, against the float64 definitions of tests/_transfer_def.py.

Gates.  Resample and fit work in double and round once: every value is the definition's fp32 value or a float next to it (one
rounding plus double-precision noise; the definition's own order sensitivity is zero ulps, tests/test_transfer_cpu.py).  The apply is
fp32: |q - q64| <= 16 * 2^-24 * S, S the interpolated magnitude sum -- at most sixteen fp32 roundings separate the loads from the
store (two per tap weight, three lerps per plane, the three multiply-adds).  A uint8 result equals the definition's byte, or differs
by exactly one where the definition lies within that bound of a half-integer, for at most 0.5 % of a case's bytes (the cap is checked
for the definition alone in tests/test_transfer_cpu.py).  Every test prints its figures before asserting."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hdiff_amd  # noqa: E402,F401
from hdiff_amd import _capi  # noqa: E402
from hdiff_amd import transfer as T  # noqa: E402
from hdiff_amd.diffusion import Evaluate as EV  # noqa: E402

import _transfer_def as TD  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL_F32, SENTINEL_U8, PAD = -777.25, 171, 64
BETA_1, BETA_T = 1e-4, 0.02
ALL_APPLY_SIZES = TD.APPLY_SIZES + TD.EXTRA_APPLY_SIZES


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.uint8).numpy().copy()


# ---------------------------------------------------------------------------------------------------------------- resample
@pytest.mark.parametrize("big,small", [((7, 5), (3, 2)), ((20, 31), (32, 32)), ((97, 131), (33, 40)), ((403, 302), (8, 8)),
                                       ((1, 300), (1, 7)), ((64, 64), (64, 64))])
def test_resample_against_the_definition(big, small):
    img = np.random.default_rng(big[0] + big[1]).integers(0, 256, size=big + (3,), dtype=np.uint8)
    want = TD.resample64(img, small)
    n = 3 * small[0] * small[1]
    buf = torch.full((n + 2 * PAD,), SENTINEL_F32, dtype=torch.float32, device=DEV)
    img_d = torch.from_numpy(img).to(DEV)
    need = C.c_int64(0)
    _capi.check(_capi.lib().hdiff_resample_workspace(big[0], big[1], small[0], small[1], C.byref(need)), "resample_workspace")
    scratch = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    _capi.check(_capi.lib().hdiff_resample_u8(img_d.data_ptr(), big[0], big[1], buf[PAD:].data_ptr(), small[0], small[1],
                                              scratch.data_ptr(), stream()), "resample_u8")
    host = buf.cpu().numpy()
    got = host[PAD:PAD + n].reshape((3,) + small)
    ok = TD.adjacent_or_equal(got, want)
    print(f"{big} -> {small}: {int((got != want.astype(np.float32)).sum())} of {n} values are the neighbour of the definition's")
    assert ok.all()
    assert (host[:PAD] == SENTINEL_F32).all() and (host[PAD + n:] == SENTINEL_F32).all()
    assert np.array_equal(bits(T.resample(img_d, small)), got.view(np.int32))             # the module's call is the same call
    if big == small:
        assert np.array_equal(got, img.transpose(2, 0, 1).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------- fit
def fit_pair(N, h, w, seed=0):
    rng = np.random.default_rng(100 * seed + 7 * h + w)
    I = rng.random((N, 3, h, w)).astype(np.float32)
    mixed = np.clip(np.einsum("cj,njyx->ncyx", TD.COLOUR_MATRIX, I.astype(np.float64)), 0, 1)
    p = np.clip(mixed ** 0.8 + 0.05 * rng.standard_normal((N, 3, h, w)), 0, 1).astype(np.float32)
    assert np.isfinite(p).all()
    return I, p


@pytest.mark.parametrize("eps", [1e-2, 1e-3, 1e-4])
@pytest.mark.parametrize("N,h,w,r", [(1, 1, 1, 1), (1, 5, 7, 2), (2, 16, 19, 3), (3, 33, 40, 8), (1, 12, 9, 20), (1, 64, 70, 1)])
def test_fit_against_the_definition(N, h, w, r, eps):
    I, p = fit_pair(N, h, w)
    want = np.stack([TD.fit64(a, b, r, eps) for a, b in zip(I, p)])
    got = T.guided_fit(torch.from_numpy(I).to(DEV), torch.from_numpy(p).to(DEV), radius=r, eps=eps).cpu().numpy()
    assert got.shape == (N, 12, h, w) and got.dtype == np.float32
    off = int((got != want.astype(np.float32)).sum())
    print(f"N {N} {h}x{w} r {r} eps {eps:g}: {off} of {got.size} coefficients are the neighbour of the definition's")
    assert TD.adjacent_or_equal(got, want).all()
    if r >= max(h, w):
        assert (got.view(np.int32) == got.view(np.int32)[:, :, :1, :1]).all()


def test_fit_of_a_constant_target():
    I, _ = fit_pair(1, 12, 15)
    const = np.array([0.25, 0.6180339887, 0.9], dtype=np.float32)
    p = np.broadcast_to(const[None, :, None, None], I.shape).copy()
    got = T.guided_fit(torch.from_numpy(I).to(DEV), torch.from_numpy(p).to(DEV), radius=3, eps=1e-3).cpu().numpy()[0]
    print(f"constant target: max |a| {np.abs(got[:9]).max():.2e}, b - const {[float(np.abs(got[9 + c] - const[c]).max()) for c in range(3)]}")
    assert np.abs(got[:9]).max() <= 1e-9
    for c in range(3):
        assert np.abs(got[9 + c] - const[c]).max() <= float(np.spacing(const[c]))


# ---------------------------------------------------------------------------------------------------------------- apply, fp32
@functools.lru_cache(maxsize=None)
def f32_case(small, large):
    """Three images' random coefficients and full-size planes, and the definition's (q, S) for each."""
    rng = np.random.default_rng(31 * large[0] + large[1])
    coef = rng.standard_normal((3, 12) + small).astype(np.float32)
    full = (rng.random((3, 3) + large) * 1.4 - 0.2).astype(np.float32)
    defs = [TD.apply64(coef[n], full[n].astype(np.float64)) for n in range(3)]
    return coef, full, np.stack([d[0] for d in defs]), np.stack([d[1] for d in defs])


def apply_f32_raw(coef_d, full_d, out_ptr, N, clamp):
    h, w = (int(v) for v in coef_d.shape[-2:])
    H, W = (int(v) for v in full_d.shape[-2:])
    _capi.check(_capi.lib().hdiff_guided_apply_f32(coef_d.data_ptr(), h, w, full_d.data_ptr(), out_ptr, N, H, W, int(clamp), stream()),
                "guided_apply_f32")


@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("small,large", ALL_APPLY_SIZES)
def test_apply_f32_against_the_definition(small, large, N, clamp):
    coef, full, q64, S = f32_case(small, large)
    coef, full, q64, S = coef[:N], full[:N], q64[:N], S[:N]
    want = np.clip(q64, 0, 1) if clamp else q64
    n = full.size
    coef_d, full_d = torch.from_numpy(coef).to(DEV), torch.from_numpy(full).to(DEV)
    buf = torch.full((n + 2 * PAD,), SENTINEL_F32, dtype=torch.float32, device=DEV)
    apply_f32_raw(coef_d, full_d, buf[PAD:].data_ptr(), N, clamp)
    host = buf.cpu().numpy()
    got = host[PAD:PAD + n].reshape(full.shape)
    ratio = float((np.abs(got.astype(np.float64) - want) / (TD.APPLY_FACTOR * S)).max())
    print(f"{small} -> {large} N {N} clamp {clamp}: largest |q - q64| is {ratio:.3f} of the bound 16 * 2^-24 * S")
    assert ratio <= 1.0
    assert (host[:PAD] == SENTINEL_F32).all() and (host[PAD + n:] == SENTINEL_F32).all()
    assert np.array_equal(bits(T.guided_apply(coef_d, full_d, clamp=clamp)), got.view(np.int32))
    in_place = full_d.clone()
    apply_f32_raw(coef_d, in_place, in_place.data_ptr(), N, clamp)
    assert np.array_equal(bits(in_place), got.view(np.int32))


# ---------------------------------------------------------------------------------------------------------------- apply, uint8
@functools.lru_cache(maxsize=None)
def u8_case(small, large):
    img, low, target = TD.u8_fixture(small, large)
    coef = TD.fit(low, target, TD.FIXTURE_RADIUS, TD.FIXTURE_EPS)
    v, S = TD.apply_u8_64(coef, img)
    return img, coef, v, S


@pytest.mark.parametrize("offsets", [(0, 0), (1, 1), (3, 1)])
@pytest.mark.parametrize("small,large", ALL_APPLY_SIZES)
def test_apply_u8_against_the_definition(small, large, offsets):
    """``offsets``: where the image and the result start in their buffers, in bytes -- equal (words can be moved) or not."""
    img, coef, v, S = u8_case(small, large)
    n = img.size
    coef_d = torch.from_numpy(coef).to(DEV)
    src = torch.full((n + 2 * PAD,), SENTINEL_U8, dtype=torch.uint8, device=DEV)
    dst = torch.full((n + 2 * PAD,), SENTINEL_U8, dtype=torch.uint8, device=DEV)
    a, b = PAD + offsets[0], PAD + offsets[1]
    src[a:a + n] = torch.from_numpy(img.reshape(-1)).to(DEV)
    _capi.check(_capi.lib().hdiff_guided_apply_u8(coef_d.data_ptr(), small[0], small[1], src[a:].data_ptr(), dst[b:].data_ptr(), large[0],
                                                  large[1], stream()), "guided_apply_u8")
    host = dst.cpu().numpy()
    got = host[b:b + n].reshape(img.shape)
    want = np.rint(v)
    diff = got.astype(np.float64) - want
    excused = TD.tie_excused(v, S)
    share = float(((diff != 0) & excused).mean())
    print(f"{small} -> {large} offsets {offsets}: {int((diff != 0).sum())} of {n} bytes differ from the definition's; {100 * share:.3f} % excused")
    assert ((diff == 0) | ((np.abs(diff) == 1) & excused)).all()
    assert share <= 0.005
    assert (host[:b] == SENTINEL_U8).all() and (host[b + n:] == SENTINEL_U8).all()
    assert (src.cpu().numpy()[a:a + n] == img.reshape(-1)).all()
    if offsets == (0, 0):
        img_d = torch.from_numpy(img).to(DEV)
        assert np.array_equal(bits(T.guided_apply(coef_d, img_d)), got)
        _capi.check(_capi.lib().hdiff_guided_apply_u8(coef_d.data_ptr(), small[0], small[1], img_d.data_ptr(), img_d.data_ptr(), large[0],
                                                      large[1], stream()), "guided_apply_u8")
        assert np.array_equal(bits(img_d), got)                                # in place


# ---------------------------------------------------------------------------------------------------------------- whole path
def whole_path(I_d, p_d, full_d):
    coef = T.guided_fit(I_d, p_d, radius=3, eps=1e-3)
    return coef, T.guided_apply(coef, full_d)


def test_repeatable_and_independent_of_the_batch():
    I, p = fit_pair(3, 16, 19, seed=1)
    full = np.random.default_rng(3).random((3, 3, 45, 61)).astype(np.float32)
    I_d, p_d, full_d = (torch.from_numpy(v).to(DEV) for v in (I, p, full))
    coef, out = whole_path(I_d, p_d, full_d)
    again = whole_path(I_d, p_d, full_d)
    assert np.array_equal(bits(coef), bits(again[0])) and np.array_equal(bits(out), bits(again[1]))
    alone = whole_path(I_d[1:2].clone(), p_d[1:2].clone(), full_d[1:2].clone())
    assert np.array_equal(bits(coef[1:2]), bits(alone[0])) and np.array_equal(bits(out[1:2]), bits(alone[1]))
    spoiled = I_d.clone()
    spoiled[0, 1, 7, 9] = float("nan")
    coef_nan, out_nan = whole_path(spoiled, p_d, full_d)
    assert np.isnan(coef_nan[0].cpu().numpy()).any()
    assert np.array_equal(bits(coef_nan[1:]), bits(coef[1:])) and np.array_equal(bits(out_nan[1:]), bits(out[1:]))


def test_fit_and_apply_are_legal_under_stream_capture():
    lib = _capi.lib()
    small, large = (16, 19), (45, 61)
    img, low, target = TD.u8_fixture(small, large)
    low_d, target_d, img_d = torch.from_numpy(low)[None].to(DEV), torch.from_numpy(target)[None].to(DEV), torch.from_numpy(img).to(DEV)
    eager = T.guided_apply(T.guided_fit(low_d, target_d, radius=2, eps=1e-3)[0], img_d)
    need = C.c_int64(0)
    _capi.check(lib.hdiff_guided_workspace(1, small[0], small[1], C.byref(need)), "guided_workspace")
    scratch = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    xi, xp, xf = torch.zeros_like(low_d), torch.zeros_like(target_d), torch.zeros_like(img_d)
    coef, out = torch.zeros(1, 12, *small, device=DEV), torch.zeros_like(img_d)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        s = torch.cuda.current_stream().cuda_stream
        _capi.check(lib.hdiff_guided_fit(xi.data_ptr(), xp.data_ptr(), 1, small[0], small[1], 2, 1e-3, coef.data_ptr(), scratch.data_ptr(), s),
                    "guided_fit")
        _capi.check(lib.hdiff_guided_apply_u8(coef.data_ptr(), small[0], small[1], xf.data_ptr(), out.data_ptr(), large[0], large[1], s),
                    "guided_apply_u8")
    xi.copy_(low_d)
    xp.copy_(target_d)
    xf.copy_(img_d)
    for _ in range(2):                                                # the second replay starts from a used workspace
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(out), bits(eager))


# ---------------------------------------------------------------------------------------------------------------- enhancer, evaluation
@functools.lru_cache(maxsize=None)
def small_sampler():
    from _tree_b_small import load_small_dyn_unet
    from hdiff_amd.diffusion.Diffusion import GaussianDiffusionSampler
    _, cfg, m, _ = load_small_dyn_unet()
    return GaussianDiffusionSampler(m.to(DEV), BETA_1, BETA_T, cfg["T"]).to(DEV)


def test_guided_enhancer_is_its_five_steps():
    sampler = small_sampler()
    img = torch.from_numpy(TD.u8_fixture((32, 32), (97, 131))[0]).to(DEV)
    y_T = torch.randn(1, 3, 32, 32, generator=torch.Generator().manual_seed(3)).to(DEV)
    enhance = T.GuidedEnhancer(sampler, size=32, radius=2, eps=1e-3, ddim_step=2, y_T=y_T)
    got = enhance(img)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (97, 131, 3) and got.device == img.device
    low = T.resample(img, 32)
    with torch.no_grad():
        out = sampler(low[None], ddim=True, ddim_step=2, y_T=y_T)
    pred01 = ((out + 1) / 2).clamp(0, 1)
    want = T.guided_apply(T.guided_fit(low[None] / 255, pred01, radius=2, eps=1e-3)[0], img)
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(enhance(img)), bits(want))            # the cached workspaces give the same bytes
    changed = int((got != img).sum())
    print(f"enhancer: {changed} of {got.numel()} bytes differ from the input")
    assert changed > 0


def test_evaluate_writes_full_size_results_and_nothing_else_changes(tmp_path):
    from PIL import Image
    sampler = small_sampler()
    g = torch.Generator().manual_seed(5)
    sizes = ((45, 61), (97, 131), (40, 33), (64, 64))
    originals = [torch.from_numpy(TD.u8_fixture((32, 32), s, seed=i)[0]) for i, s in enumerate(sizes)]
    originals[1] = originals[1].to(DEV)                              # on the host or on the device
    batches, with_full = [], []
    for i in range(2):
        b = (torch.randint(0, 256, (2, 3, 32, 32), generator=g, dtype=torch.uint8),
             torch.randint(0, 256, (2, 3, 32, 32), generator=g, dtype=torch.uint8), [f"img_{2 * i}.png", f"img_{2 * i + 1}.png"])
        batches.append(b)
        with_full.append(b + (originals[2 * i:2 * i + 2],))
    plain_dir, full_dir, collected = str(tmp_path / "plain"), str(tmp_path / "full"), []
    torch.manual_seed(21)
    plain = EV.evaluate(sampler, batches, ddim_step=2, save_dir=plain_dir)
    torch.manual_seed(21)
    res = EV.evaluate(sampler, with_full, ddim_step=2, save_dir=full_dir, transfer=(2, 1e-3), collect=collected)
    assert set(res) == set(plain) and res["n"] == plain["n"] == 4
    assert np.array_equal(res["per_image"].view(np.int64), plain["per_image"].view(np.int64))
    assert all(res[k] == plain[k] for k in res if k != "per_image")
    assert sorted(os.listdir(full_dir)) == sorted(os.listdir(plain_dir) + ["full"])
    for name in os.listdir(plain_dir):
        assert open(os.path.join(plain_dir, name), "rb").read() == open(os.path.join(full_dir, name), "rb").read(), name
    assert sorted(os.listdir(os.path.join(full_dir, "full"))) == [f"img_{i}.png" for i in range(4)]
    for i, (b, out) in enumerate((b, o) for b, o in zip(batches, collected) for _ in range(2)):
        k = i % 2
        coef = T.guided_fit(b[0].to(DEV).float() / 255, ((out + 1) / 2).clamp(0, 1), radius=2, eps=1e-3)
        want = T.guided_apply(coef[k], originals[i].to(DEV)).cpu().numpy()
        got = np.asarray(Image.open(os.path.join(full_dir, "full", f"img_{i}.png")))
        assert got.shape == sizes[i] + (3,) and got.dtype == np.uint8
        assert np.array_equal(got, want)
