"""GPU checks of the device NIQE (csrc/niqe.hip, hdiff_amd/quality.py) and of what the evaluation loop does with it
(hdiff_amd/diffusion/Evaluate.py: ``evaluate(niqe=...)``), against the float64 definition tests/_niqe_def.py.

Gates.  ``alpha`` is a table entry and must equal the definition's exactly: the fixtures (``_niqe_def.image`` at the seeds below) keep
every ``rn`` at least 1e-9 (relative) from a decision midpoint of the table, which tests/test_niqe_cpu.py asserts, and the device's
``rn`` differs from the definition's by the order of a block's sums, about 1e-13.  Every other feature and ``sharp``: within
``1e-11 * max(1, |definition|)``, the gate the UCIQE tests use for double sums taken in another order.  Moments: 1e-11 relative of
the largest entry.  Score: ``4 * 1e-11 * cond((cov_pris + cov) / 2)`` relative (floor 1e-10), first-order perturbation of the quadratic
form by moment errors of the size the moments gate allows; computed in the test from the definition's matrices.

Every fixture carries noise on every pixel: a constant non-zero block has a rounding residue for sigma and therefore finite,
rounding-dependent features in any implementation; such blocks are in no comparison here.  Every test prints its figures before
asserting; the values measured on an MI355X are in profiles/device_niqe.txt."""
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
from hdiff_amd import quality as Q  # noqa: E402
from hdiff_amd.diffusion import Evaluate as EV  # noqa: E402

import _niqe_def as D  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = 1e-11
ALPHA = [0, 2, 6, 10, 14, 18, 20, 24, 28, 32]
OTHER = [c for c in range(36) if c not in ALPHA]


def to_dev(imgs):
    return torch.from_numpy(np.stack(imgs)).to(DEV)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int64).numpy().copy()


@functools.lru_cache(maxsize=None)
def fixture(seed, H, W, noise=0.04):
    img = D.image(seed, H, W, noise)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def def_features(seed, H, W, patch, quantize, noise=0.04):
    """(feats, sharp) of one fixture by the definition; computed once, shared, never modified."""
    feats, sharp, _ = D.features(fixture(seed, H, W, noise), patch, quantize)
    feats.setflags(write=False)
    sharp.setflags(write=False)
    return feats, sharp


def host_moments(t):
    """[N, 1333] device rows -> list of (mean, cov, count)."""
    rows = t.cpu().numpy()
    return [(r[:36], r[36:-1].reshape(36, 36), int(r[-1])) for r in rows]


def device_moments(feats, sharp, threshold=0.0):
    out = torch.empty(feats.shape[0], Q.NIQE_MOMENTS, dtype=torch.float64, device=feats.device)
    Q._niqe_moments_into(feats, sharp, threshold, out)
    return out


def moment_gaps(got, want):
    (gm, gc, gn), (wm, wc, wn) = got, want
    assert gn == wn, (gn, wn)
    return float(np.abs(gm - wm).max() / np.abs(wm).max()), float(np.abs(gc - wc).max() / np.abs(wc).max())


# ---------------------------------------------------------------------------------------------------------------- features
@pytest.mark.parametrize("quantize", [True, False])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("patch,H,W", D.FEATURE_CASES)
def test_features_against_the_definition(patch, H, W, batch, quantize):
    seeds = D.FEATURE_SEEDS[:batch]
    feats, sharp = Q.niqe_features(to_dev([fixture(s, H, W) for s in seeds]), patch=patch, quantize=quantize)
    P = (H // patch) * (W // patch)
    assert feats.shape == (batch, P, 36) and sharp.shape == (batch, P) and feats.dtype == sharp.dtype == torch.float64
    feats, sharp = feats.cpu().numpy(), sharp.cpu().numpy()
    worst = worst_sharp = 0.0
    for i, s in enumerate(seeds):
        want, want_sharp = def_features(s, H, W, patch, quantize)
        assert np.isfinite(want).all() and np.isfinite(feats[i]).all()
        worst = max(worst, float((np.abs(feats[i][:, OTHER] - want[:, OTHER]) / np.maximum(1.0, np.abs(want[:, OTHER]))).max()))
        worst_sharp = max(worst_sharp, float((np.abs(sharp[i] - want_sharp) / np.maximum(1.0, np.abs(want_sharp))).max()))
        wrong = int((feats[i][:, ALPHA] != want[:, ALPHA]).sum())
        print(f"patch {patch} {H}x{W} batch {batch} quantize {quantize} image {i}: alpha mismatches {wrong} of {P * 10}")
        assert wrong == 0
    print(f"patch {patch} {H}x{W} batch {batch} quantize {quantize}: worst feature gap {worst:.2e}, worst sharp gap {worst_sharp:.2e}")
    assert worst <= GATE and worst_sharp <= GATE


# ---------------------------------------------------------------------------------------------------------------- moments
def half_zero(seed=D.ZERO_SEED, H=64, W=160):
    img = fixture(seed, H, W).copy()
    img[:, :, :W // 2] = 0.0
    return img


def test_dropped_rows():
    """The left half is exact zero: blocks (and their scale-2 counterparts) that lie inside it beyond the supports of the window and of
    the reduction have sigma = 0, m = 0, neither negative nor positive values, and so non-finite rows.  They leave the moments."""
    img = half_zero()
    want_feats, _, _ = D.features(img, 16)
    ok = D.valid_rows(want_feats)
    assert 0 < (~ok).sum() < ok.size and ok.sum() >= 2
    feats, sharp = Q.niqe_features(to_dev([img]), patch=16)
    assert np.array_equal(np.isfinite(feats[0].cpu().numpy()).all(axis=1), ok)
    got = host_moments(device_moments(feats, sharp))[0]
    want = D.moments(want_feats[ok])
    gaps = moment_gaps(got, want)
    print(f"half-zero image: {int(ok.sum())} of {ok.size} rows valid; moment gaps (mean, cov) {gaps}")
    assert max(gaps) <= GATE
    model = Q.NIQEModel(*score_model()[:2], patch=16)
    value = float(Q.niqe(to_dev([img]), model)[0])
    want_score = D.score(model.mean, model.cov, *want)
    print(f"half-zero image: score {value!r}, definition {want_score!r}")
    assert np.isfinite(value) and np.isfinite(want_score)


@pytest.mark.parametrize("threshold", [0.0, 0.75])
@pytest.mark.parametrize("patch,H,W", D.FEATURE_CASES[:2] + [(16, 64, 160)])
def test_moments_against_the_definition(patch, H, W, threshold):
    seeds = D.FEATURE_SEEDS
    feats, sharp = Q.niqe_features(to_dev([fixture(s, H, W) for s in seeds]), patch=patch)
    got = host_moments(device_moments(feats, sharp, threshold))
    keep = torch.empty(feats.shape[:2], dtype=torch.int32, device=DEV)
    _capi.check(hdiff_amd.lib().hdiff_niqe_keep(feats.data_ptr(), sharp.data_ptr(), len(seeds), int(feats.shape[1]), threshold,
                                                keep.data_ptr(), None), "niqe_keep")
    keep = keep.cpu().numpy().astype(bool)
    for i, s in enumerate(seeds):
        want_feats, want_sharp = def_features(s, H, W, patch, True)
        ok = D.valid_rows(want_feats, want_sharp, threshold)
        assert np.array_equal(keep[i], ok), (i, keep[i], ok)
        gaps = moment_gaps(got[i], D.moments(want_feats[ok]))
        print(f"patch {patch} {H}x{W} threshold {threshold} image {i}: {int(ok.sum())} rows; moment gaps (mean, cov) {gaps}")
        assert max(gaps) <= GATE


# ---------------------------------------------------------------------------------------------------------------- score, fit
@functools.lru_cache(maxsize=None)
def score_model():
    """The pristine model by the definition: six seeded 96 x 128 images at patch = 16."""
    mu, cov, kept = D.fit([fixture(s, 96, 128, D.CLEAN_NOISE) for s in D.FIT_SEEDS], 16)
    mu.setflags(write=False)
    cov.setflags(write=False)
    return mu, cov, kept


def test_score_end_to_end():
    mu, cov, _ = score_model()
    model = Q.NIQEModel(mu, cov, patch=16)
    imgs = [fixture(D.SCORE_SEED, 96, 128, D.CLEAN_NOISE), fixture(D.SCORE_SEED, 96, 128, D.NOISY_NOISE)]
    got = Q.niqe(to_dev(imgs), model)
    assert got.dtype == torch.float64 and got.shape == (2,)
    got = got.cpu().numpy()
    for i, img in enumerate(imgs):
        feats, _, _ = D.features(img, 16)
        mean, c, n = D.moments(feats[D.valid_rows(feats)])
        want = D.score(mu, cov, mean, c, n)
        bound = max(4 * GATE * float(np.linalg.cond((cov + c) / 2.0)), 1e-10)
        gap = abs(got[i] - want) / abs(want)
        print(f"score image {i}: device {got[i]!r} definition {want!r} gap {gap:.2e} bound {bound:.2e} ratio {gap / bound:.2e}")
        assert gap <= bound
    assert got[0] < got[1]                                            # the noisier image scores worse


def test_fit_on_the_device():
    mu, cov, kept = score_model()
    imgs = [fixture(s, 96, 128, D.CLEAN_NOISE) for s in D.FIT_SEEDS]
    x = to_dev(imgs)
    feats, sharp = Q.niqe_features(x, patch=16)
    keep = torch.empty(feats.shape[:2], dtype=torch.int32, device=DEV)
    _capi.check(hdiff_amd.lib().hdiff_niqe_keep(feats.data_ptr(), sharp.data_ptr(), 6, 48, 0.75, keep.data_ptr(), None), "niqe_keep")
    assert np.array_equal(keep.cpu().numpy().astype(bool), np.stack(kept))
    whole = Q.NIQEModel.fit([x], patch=16)
    gaps = (float(np.abs(whole.mean - mu).max() / np.abs(mu).max()), float(np.abs(whole.cov - cov).max() / np.abs(cov).max()))
    print(f"fit: {int(np.stack(kept).sum())} rows kept; gaps (mean, cov) {gaps}")
    assert max(gaps) <= GATE and whole.patch == 16
    for cut in ([x[:2], x[2:]], [x[i] for i in range(6)], [x[:1], x[1:2].contiguous(), x[2:5], x[5]]):
        other = Q.NIQEModel.fit(cut, patch=16)
        assert np.array_equal(other.mean.view(np.int64), whole.mean.view(np.int64))
        assert np.array_equal(other.cov.view(np.int64), whole.cov.view(np.int64))
    odd = to_dev([fixture(D.FIT_SEEDS[0], 43, 61, D.CLEAN_NOISE)])      # images of another size join the same bank
    mixed = Q.NIQEModel.fit([x[:3], odd, x[3:]], patch=16)
    want_mu, want_cov, _ = D.fit(imgs[:3] + [fixture(D.FIT_SEEDS[0], 43, 61, D.CLEAN_NOISE)] + imgs[3:], 16)
    assert np.abs(mixed.mean - want_mu).max() / np.abs(want_mu).max() <= GATE
    assert np.abs(mixed.cov - want_cov).max() / np.abs(want_cov).max() <= GATE


# ---------------------------------------------------------------------------------------------------------------- invariants
def rows_of(x, patch=16):
    feats, sharp = Q.niqe_features(x, patch=patch)
    return bits(feats), bits(sharp), bits(device_moments(feats, sharp))


def test_repeatable_and_independent_of_the_batch():
    x = to_dev([fixture(s, 48, 64) for s in D.FEATURE_SEEDS] + [fixture(D.SCORE_SEED, 48, 64)])
    whole = rows_of(x)
    again = rows_of(x)
    assert all(np.array_equal(a, b) for a, b in zip(whole, again))
    alone = rows_of(x[2:3].contiguous())
    assert all(np.array_equal(a[0], w[2]) for a, w in zip(alone, whole))
    moved = rows_of(x[[2, 0, 1, 3]].contiguous())
    assert all(np.array_equal(m[0], w[2]) for m, w in zip(moved, whole))


def test_a_nan_pixel_spoils_its_own_image_only():
    mu, cov, _ = score_model()
    model = Q.NIQEModel(mu, cov, patch=16)
    x = to_dev([fixture(s, 48, 64) for s in D.FEATURE_SEEDS])
    clean = Q.niqe(x, model)
    bad = x.clone()
    bad[1, 2, 20, 33] = float("nan")
    got = Q.niqe(bad, model)
    print("clean", clean.tolist(), "with a NaN pixel in image 1", got.tolist())
    assert torch.isnan(got[1]) and torch.isfinite(clean).all()
    assert np.array_equal(bits(got[[0, 2]]), bits(clean[[0, 2]]))
    meter = Q.QualityMeter(niqe=model)
    meter.update(bad)
    res = meter.compute()
    assert res["niqe_undefined"] == 1 and np.isnan(res["per_image"][1, -1])
    assert res["niqe"] == float(np.sum(res["per_image"][[0, 2], -1]) / 2)


def test_meter_update_under_capture_and_without_niqe():
    mu, cov, _ = score_model()
    model = Q.NIQEModel(mu, cov, patch=16)
    pred = to_dev([fixture(s, 48, 64) for s in D.FEATURE_SEEDS])
    target = to_dev([fixture(s, 48, 64, D.CLEAN_NOISE) for s in D.FEATURE_SEEDS])
    eager, plain = Q.QualityMeter(niqe=model), Q.QualityMeter()
    eager.update(pred, target)
    plain.update(pred, target)
    res_eager, res_plain = eager.compute(), plain.compute()
    as_bits = lambda a: np.ascontiguousarray(a).view(np.int64)      # noqa: E731
    # without niqe=: the six columns of before, equal to the direct calls bit for bit, and the same dict keys
    assert set(res_plain) == {"n", "per_image"} | set(Q.COLUMNS) and res_plain["per_image"].shape == (3, 6)
    psnr, ssim = Q.psnr_ssim(pred, target)
    uicm, uism, uiconm, uiqm = Q.uiqm(pred)
    direct = torch.stack([psnr, ssim, uiqm, uicm, uism, uiconm], dim=1).cpu().numpy()
    assert np.array_equal(as_bits(res_plain["per_image"]), as_bits(direct))
    assert np.array_equal(as_bits(res_eager["per_image"][:, :6]), as_bits(res_plain["per_image"]))
    assert eager.columns == Q.COLUMNS + Q.NIQE_COLUMNS and set(res_eager) == set(res_plain) | {"niqe", "niqe_undefined"}
    assert np.array_equal(as_bits(res_eager["per_image"][:, -1]), as_bits(Q.niqe(pred, model).cpu().numpy()))
    # one captured update replays the eager bits
    xa, ta = torch.zeros_like(pred), torch.zeros_like(target)
    captured = Q.QualityMeter(niqe=model)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        captured.update(xa, ta)
    xa.copy_(pred)
    ta.copy_(target)
    graph.replay()
    torch.cuda.synchronize()
    res = captured.compute()
    assert np.array_equal(as_bits(res["per_image"]), as_bits(res_eager["per_image"]))
    with pytest.raises(ValueError, match="patch"):
        Q.QualityMeter(niqe=Q.NIQEModel(mu, cov, patch=96)).update(pred)


# ---------------------------------------------------------------------------------------------------------------- evaluation loop
def res_lines(path):
    lines = [ln for ln in open(path).read().split("\n") if ln]
    return [ln.split(":")[0] + ":" for ln in lines], {ln.split(":")[0]: float(ln.split(":")[1]) for ln in lines}


def stand_in_sampler(inp, **kw):
    img = inp / 255
    return 2 * (0.7 * img + 0.3 * img.mean(dim=1, keepdim=True)) - 1


def test_evaluate_scores_model_sized_and_full_size_results(tmp_path):
    from PIL import Image
    mu, cov, _ = score_model()
    model = Q.NIQEModel(mu, cov, patch=16)
    path = str(tmp_path / "pristine.npz")
    model.save(path)
    batches = []
    for k, (H, W) in enumerate(((40, 56), (48, 72))):
        full = torch.from_numpy((fixture(D.FEATURE_SEEDS[k], H, W) * 255).round().astype(np.uint8).transpose(1, 2, 0).copy())
        small = torch.from_numpy((fixture(D.FEATURE_SEEDS[k], 32, 32) * 255).round().astype(np.uint8))
        batches.append((small[None].to(DEV), small[None].to(DEV), [f"img{k}.png"], [full]))
    save_dir = str(tmp_path / "out")
    res = EV.evaluate(stand_in_sampler, batches, ddim_step=2, save_dir=save_dir, transfer=(2, 1e-3), niqe=path)
    keys, parsed = res_lines(os.path.join(save_dir, "res.txt"))
    assert keys == [k for k, _ in EV.RES_KEYS] + ["niqe_orgin_avg:", "niqe_full_orgin_avg:"]
    assert parsed["niqe_orgin_avg"] == res["niqe"] and parsed["niqe_full_orgin_avg"] == res["niqe_full"]
    assert res["per_image"].shape == (2, 7) and res["niqe_undefined"] == 0 and res["niqe_full_undefined"] == 0
    scores = []
    for k, (H, W) in enumerate(((40, 56), (48, 72))):
        written = np.asarray(Image.open(os.path.join(save_dir, "full", f"img{k}.png")))
        assert written.shape == (H, W, 3)
        x = torch.from_numpy(written.copy()).to(DEV).permute(2, 0, 1).unsqueeze(0).float() / 255
        scores.append(float(Q.niqe(x, model)[0]))
    print("niqe", res["niqe"], "niqe_full", res["niqe_full"], scores)
    assert res["niqe_full_per_image"] == scores and res["niqe_full"] == sum(scores) / 2 and np.isfinite(scores).all()
    plain_dir = str(tmp_path / "plain")
    plain = EV.evaluate(stand_in_sampler, batches, ddim_step=2, save_dir=plain_dir, transfer=(2, 1e-3))
    assert "niqe" not in plain and "niqe_full" not in plain and plain["per_image"].shape == (2, 6)
    assert res_lines(os.path.join(plain_dir, "res.txt"))[0] == [k for k, _ in EV.RES_KEYS]
    with pytest.raises(ValueError, match="patch"):
        EV.evaluate(stand_in_sampler, batches, ddim_step=2, niqe=Q.NIQEModel(mu, cov, patch=64))


def test_fit_niqe_and_the_configuration_keys(tmp_path, monkeypatch):
    """``fit_niqe`` on the targets of both sets equals ``NIQEModel.fit`` on the same images bit for bit and writes a loadable file;
    ``inference`` with ``niqe`` / ``niqe_model`` / ``full_resolution`` writes both lines for both sets."""
    import types
    from PIL import Image
    from _tree_b_small import load_small_dyn_unet
    _, cfg, _, sd = load_small_dyn_unet()
    root = tmp_path / "data"
    folders = (("Train/low", "jpg", 0.15), ("Train/high", "jpg", 0.01), ("Train/trainA_paired", "png", 0.15),
               ("Train/trainB_paired", "png", 0.01), ("Val/low", "jpg", 0.15), ("Val/high", "jpg", 0.01), ("Val/valA", "png", 0.15),
               ("Val/valB", "png", 0.01))
    for sub, ext, noise in folders:
        os.makedirs(root / sub)
        for k, name in enumerate(("one", "two", "three")):
            img = (fixture(D.FIT_SEEDS[k], 40, 56, noise) * 255).round().astype(np.uint8).transpose(1, 2, 0)
            Image.fromarray(img).save(str(root / sub / f"{name}.{ext}"))

    def to_32(image):
        return {"image": torch.from_numpy(np.ascontiguousarray(image[:32, :32])).permute(2, 0, 1)}      # a crop: the noise stays
    ckpt = tmp_path / "ckpt_small.pt"
    torch.save({"module." + k: v for k, v in sd.items()}, str(ckpt))
    monkeypatch.chdir(tmp_path)
    config = types.SimpleNamespace(underwater_data_name="HICRD", atmospheric_data_name="LoLI", dataset_root=str(root), T=cfg["T"],
                                   channel=cfg["ch"], channel_mult=cfg["ch_mult"], num_res_blocks=cfg["num_res_blocks"],
                                   pretrained_path=str(ckpt), beta_1=1e-4, beta_T=0.02, ddim_step=2, batch_size=2,
                                   device_list=[DEV], transforms=to_32, result_root=str(tmp_path / "results"))
    path = str(tmp_path / "pristine.npz")
    model = EV.fit_niqe(config, out=path, patch=16)
    targets = [torch.from_numpy(np.asarray(Image.open(str(root / sub / f"{name}.{ext}")).convert("RGB"))[:32, :32].copy())
               for sub, ext in (("Train/trainB_paired", "png"), ("Train/high", "jpg")) for name in ("one", "three", "two")]      # sorted
    direct = Q.NIQEModel.fit([torch.stack(targets).permute(0, 3, 1, 2).to(DEV).float() / 255], patch=16)
    assert np.array_equal(model.mean.view(np.int64), direct.mean.view(np.int64))
    assert np.array_equal(model.cov.view(np.int64), direct.cov.view(np.int64))
    loaded = Q.NIQEModel.load(path, patch=16)
    assert np.array_equal(loaded.mean, model.mean) and np.array_equal(loaded.cov, model.cov) and loaded.quantize is True
    config.niqe, config.niqe_model, config.full_resolution, config.transfer_radius = True, path, True, 2
    torch.manual_seed(4)
    results = EV.inference(config)
    for name in ("HICRD", "LoLI"):
        folder = tmp_path / "results" / "ckpt_small.pt" / name
        keys, parsed = res_lines(str(folder / "res.txt"))
        print(name, parsed)
        assert keys == [k for k, _ in EV.RES_KEYS] + ["niqe_orgin_avg:", "niqe_full_orgin_avg:"]
        assert results[name]["per_image"].shape == (3, 7) and len(results[name]["niqe_full_per_image"]) == 3
        assert np.isfinite(parsed["niqe_orgin_avg"]) and np.isfinite(parsed["niqe_full_orgin_avg"])
        assert len(os.listdir(folder / "full")) == 3
    config.niqe_model = None
    with pytest.raises(ValueError, match="niqe_model"):
        EV.inference(config)
