"""GPU checks of the device quality scores (csrc/quality.hip, hdiff_amd/quality.py) and of the evaluation loop built on them
(hdiff_amd/diffusion/Evaluate.py).

Gates.  PSNR / SSIM against ``metrics.psnr`` / ``metrics.ssim`` on the same fp32 ``clip * 255`` arrays: |dSSIM| <= 1e-9 and
|dPSNR| <= 1e-9 dB -- both sides hold the moments in double; the worst-case summation bound is 48 * 2^-53 * sum(x^2) / 49 against
C2 = 58.5, about 1e-11, so the gate leaves two orders of margin and still sees a wrong tap.  UIQM against the float64-sum definition
(tests/_uiqm_def.py): uicm, uiconm and uiqm within 1e-11 relative (only the order of double sums and the last bits of ``log`` differ),
uism within 2e-6 relative (``hypotf`` and the scale may differ from numpy's by an fp32 ulp on a block extremum, which moves a block's
log(hi / lo) by <= 1.2e-7 on values of 6-18); against the pinned ``uw_metrics`` functions all four within 2e-6 relative (their UICM
adds the kept samples in an fp32 running sum: <= 2.3e-8 at these sizes, tests/test_quality_cpu.py).  Every test prints its figures
before asserting; the values measured on an MI355X are in profiles/device_quality.txt."""
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hdiff_amd  # noqa: E402,F401
from hdiff_amd import metrics as M  # noqa: E402
from hdiff_amd import quality as Q  # noqa: E402
from hdiff_amd import uw_metrics as U  # noqa: E402
from hdiff_amd.diffusion import Evaluate as EV  # noqa: E402

import _uiqm_def as D  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAIR_GATE = 1e-9
DEF_GATE, UISM_GATE, PINNED_GATE = 1e-11, 2e-6, 2e-6
BETA_1, BETA_T = 1e-4, 0.02


def to_dev(imgs):
    """HWC fp32 images -> [N, 3, H, W] on the device."""
    return torch.from_numpy(np.stack([np.ascontiguousarray(i.transpose(2, 0, 1)) for i in imgs])).to(DEV)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int64).numpy().copy()


def rel(a, b):
    return 0.0 if a == b else abs(a - b) / abs(b)          # equal values (0 against 0 among them) have no gap


def pair_batch(H, W):
    """Three (prediction, target) pairs; the second pair spills outside [0, 1] on both sides."""
    rng = np.random.default_rng(7 * H + W)
    a = [D.image(k, H, W) for k in ("smooth", "noise", "sat")]
    b = [(x + 0.1 * rng.standard_normal(x.shape)).astype(np.float32) for x in a]
    a[1], b[1] = (a[1] * 1.5 - 0.2).astype(np.float32), (b[1] * 1.5 - 0.3).astype(np.float32)
    assert a[1].min() < 0 and a[1].max() > 1
    return a, b


def host_pair(pred, target):
    p, t = D.scaled(pred), D.scaled(target)
    return M.psnr(t, p, 255.0), M.ssim(t, p, 255.0, channel_axis=2)


@functools.lru_cache(maxsize=None)
def uiqm_host(size):
    """Per image of the four kinds at one size: (definition, pinned functions); computed once, shared, never modified."""
    out = []
    for img in D.images(*size):
        x = D.scaled(img)
        out.append((D.uiqm_def(x), (U.uicm(x), U.uism(x), U.uiconm(x, 8), U.getUIQM(x))))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def uiqm_device(size):
    return torch.stack(Q.uiqm(to_dev(D.images(*size))), dim=1).cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- PSNR / SSIM
@pytest.mark.parametrize("size", [(7, 7), (8, 13), (33, 39), (40, 71)])
def test_psnr_ssim_against_the_host_definition(size):
    a, b = pair_batch(*size)
    psnr, ssim = Q.psnr_ssim(to_dev(a), to_dev(b))
    assert psnr.dtype == torch.float64 and ssim.dtype == torch.float64 and psnr.shape == (3,)
    psnr, ssim = psnr.cpu().numpy(), ssim.cpu().numpy()
    assert np.isfinite(psnr).all() and np.isfinite(ssim).all(), (psnr, ssim)      # max() below would skip a NaN gap
    worst = [0.0, 0.0]
    for i in range(3):
        rp, rs = host_pair(a[i], b[i])
        worst = [max(worst[0], abs(psnr[i] - rp)), max(worst[1], abs(ssim[i] - rs))]
        print(f"{size} image {i}: psnr {psnr[i]:.12f} (host {rp:.12f})  ssim {ssim[i]:.15f} (host {rs:.15f})")
    print(f"{size}: worst |dPSNR| {worst[0]:.2e} dB, worst |dSSIM| {worst[1]:.2e}")
    assert worst[0] <= PAIR_GATE and worst[1] <= PAIR_GATE, worst


def test_identical_images_and_one_pixel():
    a, _ = pair_batch(33, 39)
    x = to_dev(a)
    psnr, ssim = Q.psnr_ssim(x, x.clone())
    print("identical:", psnr.tolist(), ssim.tolist())
    assert torch.isinf(psnr).all() and (psnr > 0).all()
    assert (ssim == 1.0).all()
    b = [v.copy() for v in a]
    b[2][17, 20, 1] = 0.25 if abs(a[2][17, 20, 1] - 0.25) > 0.1 else 0.75
    psnr, ssim = Q.psnr_ssim(x, to_dev(b))
    rp, rs = host_pair(a[2], b[2])
    print("one pixel:", psnr.tolist(), ssim.tolist(), rp, rs)
    assert torch.isinf(psnr[:2]).all() and (ssim[:2] == 1.0).all()
    assert np.isfinite(psnr[2].item()) and abs(psnr[2].item() - rp) <= PAIR_GATE and abs(ssim[2].item() - rs) <= PAIR_GATE


# ---------------------------------------------------------------------------------------------------------------- UIQM
@pytest.mark.parametrize("size", D.SIZES)
def test_uiqm_against_the_definition_and_the_pinned_functions(size):
    got = uiqm_device(size)
    assert got.shape == (4, 4) and np.isfinite(got).all(), got                    # max() below would skip a NaN gap
    worst_def, worst_pin = [0.0] * 4, [0.0] * 4
    for i, (kind, (want, pinned)) in enumerate(zip(D.KINDS, uiqm_host(size))):
        for j, name in enumerate(("uicm", "uism", "uiconm", "uiqm")):
            worst_def[j] = max(worst_def[j], rel(got[i, j], want[j]))
            worst_pin[j] = max(worst_pin[j], rel(got[i, j], pinned[j]))
        print(f"{size} {kind}: device {got[i].tolist()}  definition {list(want)}")
    print(f"{size}: worst relative gap to the definition (uicm, uism, uiconm, uiqm) {[f'{v:.2e}' for v in worst_def]}; "
          f"to uw_metrics {[f'{v:.2e}' for v in worst_pin]}")
    assert worst_def[0] <= DEF_GATE and worst_def[2] <= DEF_GATE and worst_def[3] <= DEF_GATE, worst_def
    assert worst_def[1] <= UISM_GATE, worst_def
    assert max(worst_pin) <= PINNED_GATE, worst_pin


def test_constant_channel_gives_nan_sharpness_only():
    imgs = D.images(19, 27)[:2]
    imgs[1] = imgs[1].copy()
    imgs[1][:, :, 1] = np.float32(100.0 / 255.0)
    got = torch.stack(Q.uiqm(to_dev(imgs)), dim=1).cpu().numpy()
    x = D.scaled(imgs[1])
    print("constant channel:", got[1].tolist(), U.uicm(x), U.uiconm(x, 8))
    assert np.isnan(got[1, 1]) and np.isnan(got[1, 3])
    assert rel(got[1, 0], D.uicm_def(x)) <= DEF_GATE and rel(got[1, 2], D.uiconm_def(x)) <= DEF_GATE
    assert rel(got[1, 0], U.uicm(x)) <= PINNED_GATE and rel(got[1, 2], U.uiconm(x, 8)) <= PINNED_GATE
    assert np.array_equal(got[0], uiqm_device((19, 27))[0])          # the image beside it is untouched


# ---------------------------------------------------------------------------------------------------------------- batches
def six(pred, target):
    """[N, 6] int64 bit patterns of (psnr, ssim, uicm, uism, uiconm, uiqm)."""
    return np.concatenate([bits(torch.stack(Q.psnr_ssim(pred, target), dim=1)), bits(torch.stack(Q.uiqm(pred), dim=1))], axis=1)


def test_scores_do_not_depend_on_the_batch_and_repeat():
    a, b = pair_batch(40, 71)
    pa, pb = to_dev(a), to_dev(b)
    whole = six(pa, pb)
    assert np.array_equal(whole, six(pa, pb))                         # two runs are bit-identical
    for i in range(3):
        alone = six(pa[i:i + 1].contiguous(), pb[i:i + 1].contiguous())
        assert np.array_equal(alone[0], whole[i]), i
        for place in range(3):
            order = [(i + k - place) % 3 for k in range(3)]           # image i as entry `place` of a batch of 3
            moved = six(pa[order].contiguous(), pb[order].contiguous())
            assert np.array_equal(moved[place], alone[0]), (i, place)


def test_one_nan_pixel_spoils_its_image_alone():
    a, b = pair_batch(40, 71)
    pa, pb = to_dev(a), to_dev(b)
    clean = six(pa, pb)
    bad = pa.clone()
    bad[1, 2, 33, 64] = float("nan")
    got = six(bad, pb)
    as_float = got.view(np.float64)
    print("nan pixel:", as_float[1].tolist())
    assert np.isnan(as_float[1]).all()
    assert np.array_equal(got[0], clean[0]) and np.array_equal(got[2], clean[2])
    bad = pa.clone()
    bad[0, 0, 0, 0] = float("inf")
    as_float = six(bad, pb).view(np.float64)
    assert np.isnan(as_float[0]).all() and not np.isnan(as_float[1:]).any()


def test_calls_are_legal_under_stream_capture():
    """Neither call allocates or synchronises: both are captured into one graph (workspace and outputs allocated before), and the
    replay on other inputs gives the eager results bit for bit."""
    import ctypes as C
    from hdiff_amd import _capi
    lib = hdiff_amd.lib()
    a, b = pair_batch(33, 39)
    pa, pb = to_dev(a), to_dev(b)
    eager = six(pa, pb)
    need = C.c_int64(0)
    _capi.check(lib.hdiff_quality_workspace(3, 33, 39, C.byref(need)), "quality_workspace")
    scratch = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    xa, xb = torch.zeros_like(pa), torch.zeros_like(pb)
    pair = torch.zeros(3, 2, dtype=torch.float64, device=DEV)
    four = torch.zeros(3, 4, dtype=torch.float64, device=DEV)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        s = torch.cuda.current_stream().cuda_stream
        _capi.check(lib.hdiff_psnr_ssim(xb.data_ptr(), xa.data_ptr(), 3, 33, 39, pair.data_ptr(), scratch.data_ptr(), s), "psnr_ssim")
        _capi.check(lib.hdiff_uiqm(xa.data_ptr(), 3, 33, 39, four.data_ptr(), scratch.data_ptr(), s), "uiqm")
    xa.copy_(pa)
    xb.copy_(pb)
    for _ in range(2):                                                # the second replay starts from a used workspace
        pair.zero_()
        four.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(np.concatenate([bits(pair), bits(four)], axis=1), eager)


# ---------------------------------------------------------------------------------------------------------------- meter
def host_rows(preds, targets):
    """[n, 6] (psnr, ssim, uiqm, uicm, uism, uiconm) by the host functions; NaN pairs where there is no target."""
    rows = []
    for p, t in zip(preds, targets):
        x = D.scaled(p)
        ps = host_pair(p, t) if t is not None else (float("nan"), float("nan"))
        rows.append([ps[0], ps[1], U.getUIQM(x), U.uicm(x), U.uism(x), U.uiconm(x, 8)])
    return np.asarray(rows)


def check_against_host(res, want, what):
    per = res["per_image"]
    assert per.shape == want.shape and per.dtype == np.float64
    paired = ~np.isnan(want[:, 0])
    for j, k in enumerate(Q.COLUMNS):
        col = want[paired, j] if j < 2 else want[:, j]
        mean = float(col.sum() / col.size)
        gap = abs(res[k] - mean) if j < 2 else rel(res[k], mean)
        print(f"{what} {k}: device mean {res[k]!r}  host mean {mean!r}  gap {gap:.2e}")
        assert gap <= (PAIR_GATE if j < 2 else PINNED_GATE), (k, res[k], mean)
    assert np.array_equal(np.isnan(per[:, :2]), np.isnan(want[:, :2]))


def test_quality_meter_accumulates_and_grows():
    a, b = pair_batch(19, 27)
    c = D.images(19, 27)
    meter = Q.QualityMeter(capacity=2)
    meter.update(to_dev(a), to_dev(b))                                # 3 rows: past the initial capacity at once
    meter.update(to_dev(c[:2]).double(), to_dev(b[:2]))               # other float dtypes are converted; 5 rows: grows again
    meter.update(to_dev(c[3:4]).permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2))     # non-contiguous, no target
    assert len(meter) == 6
    res = meter.compute()
    assert res["n"] == 6
    check_against_host(res, host_rows(a + c[:2] + c[3:4], b + b[:2] + [None]), "meter")
    x = to_dev(a[:1])
    inf_meter = Q.QualityMeter()
    inf_meter.update(x, x.clone())
    inf_meter.update(to_dev(a[1:2]), to_dev(b[1:2]))
    assert inf_meter.compute()["psnr"] == float("inf")                # as the reference's sum(list) / len(list)


# ---------------------------------------------------------------------------------------------------------------- evaluation loop
@functools.lru_cache(maxsize=None)
def small_model():
    from _tree_b_small import load_small_dyn_unet
    _, cfg, m, sd = load_small_dyn_unet()
    return cfg, m.to(DEV), sd


def parse_res(path):
    lines = [ln for ln in open(path).read().split("\n") if ln]
    assert [ln.split(":")[0] + ":" for ln in lines] == [k for k, _ in EV.RES_KEYS]
    return {ln.split(":")[0]: float(ln.split(":")[1]) for ln in lines}


def test_evaluate_scores_what_the_sampler_returns(tmp_path):
    from hdiff_amd.diffusion.Diffusion import GaussianDiffusionSampler
    cfg, model, _ = small_model()
    assert cfg["T"] == 1000
    sampler = GaussianDiffusionSampler(model, BETA_1, BETA_T, cfg["T"]).to(DEV)
    g = torch.Generator().manual_seed(5)
    batches = [(torch.randint(0, 256, (2, 3, 32, 32), generator=g, dtype=torch.uint8),
                torch.randint(0, 256, (2, 3, 32, 32), generator=g, dtype=torch.uint8), [f"img_{2 * i}.png", f"img_{2 * i + 1}.png"])
               for i in range(2)]
    collected, save_dir = [], str(tmp_path / "plain")
    torch.manual_seed(21)
    res = EV.evaluate(sampler, batches, ddim_step=2, collect=collected, save_dir=save_dir)
    assert res["n"] == 4 and len(collected) == 2 and collected[0].shape == (2, 3, 32, 32)
    # the images as the meter received them (the device's own `(out + 1) / 2` and `target / 255`), scored by the host functions
    preds = [((o + 1) / 2).cpu()[i].permute(1, 2, 0).numpy() for o in collected for i in range(2)]
    targets = [(t.to(DEV).float() / 255).cpu()[i].permute(1, 2, 0).numpy() for _, t, _ in batches for i in range(2)]
    check_against_host(res, host_rows(preds, targets), "evaluate")
    parsed = parse_res(os.path.join(save_dir, "res.txt"))
    assert parsed == {k[:-1]: res[name] for k, name in EV.RES_KEYS}
    from PIL import Image
    for i, p in enumerate(preds):
        got = np.asarray(Image.open(os.path.join(save_dir, f"img_{i}.png")))
        assert got.shape == (32, 32, 3) and got.dtype == np.uint8
        assert np.abs(got.astype(np.float64) - np.clip(p, 0, 1) * 255.0).max() <= 0.5 + 1e-4       # rounded to nearest
    torch.manual_seed(21)
    tiled = EV.evaluate(sampler, batches, ddim_step=2, tile=32)     # one window is the untiled path bit for bit
    assert np.array_equal(bits(torch.from_numpy(tiled["per_image"])), bits(torch.from_numpy(res["per_image"])))
    assert all(tiled[k] == res[k] for k in Q.COLUMNS)
    assert not os.path.exists(str(tmp_path / "res.txt"))


def test_reference_shaped_test_routine(tmp_path, monkeypatch):
    from PIL import Image
    cfg, _, sd = small_model()
    root = tmp_path / "data"
    rng = np.random.default_rng(9)
    for sub, ext in (("Test/low", "jpg"), ("Test/high", "jpg"), ("Test/testA", "png"), ("Test/testB", "png")):
        os.makedirs(root / sub)
        for name in ("one", "two"):
            low = rng.integers(0, 256, (4, 4, 3), dtype=np.uint8)    # a few colour patches, enlarged
            Image.fromarray(low).resize((24, 20), Image.BILINEAR).save(str(root / sub / f"{name}.{ext}"))

    def to_32(image):
        """An albumentations-style pipeline, as the sets take it: HWC uint8 array -> {"image": CHW uint8 tensor}, 32x32."""
        img = Image.fromarray(image).resize((32, 32), Image.BILINEAR)
        return {"image": torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).permute(2, 0, 1)}
    ckpt = tmp_path / "ckpt_small.pt"
    torch.save({"module." + k: v for k, v in sd.items()}, str(ckpt))
    monkeypatch.chdir(tmp_path)
    config = types.SimpleNamespace(underwater_data_name="HICRD", atmospheric_data_name="LoLI", dataset_root=str(root), T=cfg["T"],
                                   channel=cfg["ch"], channel_mult=cfg["ch_mult"], num_res_blocks=cfg["num_res_blocks"],
                                   pretrained_path=str(ckpt), beta_1=BETA_1, beta_T=BETA_T, ddim_step=2, batch_size=2,
                                   device_list=[DEV], transforms=to_32)
    torch.manual_seed(4)
    results = EV.test(config, None)
    assert set(results) == {"HICRD", "LoLI"}
    for name, ext in (("HICRD", "png"), ("LoLI", "jpg")):
        folder = tmp_path / "output" / "result" / "ckpt_small.pt" / name
        assert sorted(os.listdir(folder)) == sorted([f"one.{ext}", f"two.{ext}", "res.txt"])
        parsed = parse_res(str(folder / "res.txt"))
        print(name, parsed)
        assert results[name]["n"] == 2 and all(np.isfinite(v) for v in parsed.values()), parsed
        assert parsed == {k[:-1]: results[name][v] for k, v in EV.RES_KEYS}
