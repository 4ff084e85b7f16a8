"""GPU checks of the device UCIQE (csrc/uciqe.hip, hdiff_amd/quality.py) and of what the evaluation loops do with it
(hdiff_amd/diffusion/Evaluate.py: ``evaluate(uciqe=True)``, ``inference``).

Gate.  sc, conl, us and uciqe against the float64 definition (tests/_uciqe_def.py) within 1e-11 relative: both sides sum in double, the
worst-case summation bound at the largest size is 8 640 * 2^-53, about 1e-12, and ``pow`` / ``cbrt`` differ in the last bits; this is
the project's DEF_GATE for the same kind of comparison and leaves one order of margin.  Every test prints its figures before
asserting; the values measured on an MI355X are in profiles/device_uciqe.txt."""
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
from hdiff_amd import quality as Q  # noqa: E402
from hdiff_amd import uw_metrics as U  # noqa: E402
from hdiff_amd.diffusion import Evaluate as EV  # noqa: E402

import _uciqe_def as UD  # noqa: E402
import _uiqm_def as D  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DEF_GATE = 1e-11
BETA_1, BETA_T = 1e-4, 0.02
NAMES = ("sc", "conl", "us", "uciqe")


def to_dev(imgs):
    """HWC fp32 images -> [N, 3, H, W] on the device."""
    return torch.from_numpy(np.stack([np.ascontiguousarray(i.transpose(2, 0, 1)) for i in imgs])).to(DEV)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int64).numpy().copy()


def rel(a, b):
    return 0.0 if a == b else abs(a - b) / abs(b)          # equal values (0 against 0 among them) have no gap


def device_rows(x, scale=1.0):
    """[N, 4] float64 (sc, conl, us, uciqe) on the host."""
    out = Q.uciqe(x, scale=scale)
    assert all(o.dtype == torch.float64 and o.shape == (x.shape[0],) for o in out)
    return torch.stack(out, dim=1).cpu().numpy()


def definition(img, scale=1.0):
    return UD.uciqe_def(np.ascontiguousarray(img.transpose(2, 0, 1)), scale)


@functools.lru_cache(maxsize=None)
def definition_rows(size, scale):
    """The four kinds at one size by the definition; computed once, shared, never modified."""
    return tuple(definition(img, scale) for img in D.images(*size))


def worst_gaps(got, want, what):
    assert np.isfinite(got).all(), (what, got)                        # max() below would skip a NaN gap
    worst = [0.0] * 4
    for i in range(len(want)):
        for j in range(4):
            worst[j] = max(worst[j], rel(got[i, j], want[i][j]))
        print(f"{what} image {i}: device {got[i].tolist()}  definition {list(want[i])}")
    print(f"{what}: worst relative gap to the definition (sc, conl, us, uciqe) {[f'{v:.2e}' for v in worst]}")
    return worst


# ---------------------------------------------------------------------------------------------------------------- definition
# (8, 13): top = 1; (16, 24), (19, 27), (40, 71): no multiple of any tile; (72, 120): 8 640 pixels, several workgroups per image
@pytest.mark.parametrize("size,scale", [((8, 13), 1.0), ((16, 24), 1.0), ((19, 27), 1.0), ((40, 71), 1.0), ((72, 120), 1.0),
                                        ((19, 27), 255.0)])
def test_uciqe_against_the_definition(size, scale):
    got = device_rows(to_dev(D.images(*size)), scale)
    assert got.shape == (4, 4)
    worst = worst_gaps(got, definition_rows(size, scale), f"{size} scale {scale:g}")
    assert max(worst) <= DEF_GATE, worst


def two_level(H=16, W=24, count=150):
    img = np.empty((H * W, 3), dtype=np.float32)
    img[:count] = (0.9, 0.4, 0.1)
    img[count:] = (0.2, 0.5, 0.3)
    return img.reshape(H, W, 3)


def test_ties_at_the_cuts():
    """Both tails of the two-level image lie entirely inside ties: conl is the difference of the two L values."""
    img = two_level()
    got = device_rows(to_dev([img, D.image("ties", 16, 24)]))
    want = definition(img)
    host = U.nmetrics(np.clip(img, 0, 1).astype(np.float64))[1]
    levels = [float(UD.lab_def(np.asarray(c, dtype=np.float32).astype(np.float64).reshape(3, 1, 1))[0][0, 0])
              for c in ((0.9, 0.4, 0.1), (0.2, 0.5, 0.3))]
    step = max(levels) - min(levels)
    print(f"two levels: device {got[0].tolist()}  definition {list(want)}  host uciqe {host!r}  L levels {levels}")
    assert np.isfinite(got).all()
    assert round(host, 4) == 11.2528
    assert rel(got[0, 1], step) <= DEF_GATE and rel(want[1], step) <= DEF_GATE
    assert max(rel(got[0, j], want[j]) for j in range(4)) <= DEF_GATE
    ties = definition_rows((16, 24), 1.0)[D.KINDS.index("ties")]
    assert max(rel(got[1, j], ties[j]) for j in range(4)) <= DEF_GATE


def test_fewer_than_fifty_pixels_have_no_tails():
    imgs = D.images(7, 7)
    got = device_rows(to_dev(imgs))
    for i, img in enumerate(imgs):
        want = definition(img)
        print(f"7x7 image {i}: device {got[i].tolist()}  definition {list(want)}")
        assert np.isnan(got[i, 1]) and np.isnan(got[i, 3]) and np.isnan(want[1]) and np.isnan(want[3])
        assert np.isfinite(got[i, 0]) and np.isfinite(got[i, 2])
        assert rel(got[i, 0], want[0]) <= DEF_GATE and rel(got[i, 2], want[2]) <= DEF_GATE


# ---------------------------------------------------------------------------------------------------------------- batches
def four(x, scale=1.0):
    return bits(torch.stack(Q.uciqe(x, scale=scale), dim=1))


def test_scores_do_not_depend_on_the_batch_and_repeat():
    imgs = D.images(40, 71) + [D.image("smooth", 40, 71)[::-1].copy()]
    x = to_dev(imgs)
    whole = four(x)
    assert np.array_equal(whole, four(x))                             # two calls are bit-identical
    alone = four(x[2:3].contiguous())
    assert np.array_equal(alone[0], whole[2])
    for place in (0, 4):                                              # image 2 as the first and as the last of a batch of 5
        order = [(2 + k - place) % 5 for k in range(5)]
        moved = four(x[order].contiguous())
        assert np.array_equal(moved[place], alone[0]), place


def test_one_non_finite_pixel_spoils_its_image_alone():
    x = to_dev(D.images(40, 71))
    clean = four(x)
    bad = x.clone()
    bad[1, 2, 33, 64] = float("nan")
    bad[3, 0, 0, 0] = float("inf")
    got = four(bad)
    as_float = got.view(np.float64)
    print("non-finite pixels:", as_float.tolist())
    assert np.isnan(as_float[1]).all() and np.isnan(as_float[3]).all()
    assert np.array_equal(got[0], clean[0]) and np.array_equal(got[2], clean[2])
    assert not np.isnan(clean.view(np.float64)).any()


def test_call_is_legal_under_stream_capture():
    """The call neither allocates nor synchronises: it is captured into a graph (one stream, a linear graph; workspace and output
    allocated before), and the replay on other inputs gives the eager result bit for bit."""
    import ctypes as C
    from hdiff_amd import _capi
    lib = hdiff_amd.lib()
    px = to_dev(D.images(33, 39)[:3])
    eager = four(px)
    need = C.c_int64(0)
    _capi.check(lib.hdiff_uciqe_workspace(3, 33, 39, C.byref(need)), "uciqe_workspace")
    scratch = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    xa = torch.zeros_like(px)
    out = torch.zeros(3, 4, dtype=torch.float64, device=DEV)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        s = torch.cuda.current_stream().cuda_stream
        _capi.check(lib.hdiff_uciqe(xa.data_ptr(), 3, 33, 39, 1.0, out.data_ptr(), scratch.data_ptr(), s), "uciqe")
    xa.copy_(px)
    for _ in range(2):                                                # the second replay starts from a used workspace
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(out), eager)


# ---------------------------------------------------------------------------------------------------------------- meter
def test_quality_meter_with_and_without_uciqe():
    rng = np.random.default_rng(11)
    a = D.images(19, 27)
    b = [(x + 0.1 * rng.standard_normal(x.shape)).astype(np.float32) for x in a]
    updates = [(to_dev(a[:3]), to_dev(b[:3])), (to_dev(a[2:4]), to_dev(b[2:4])), (to_dev(b[1:2]), None)]
    plain, full, scaled = Q.QualityMeter(capacity=2), Q.QualityMeter(capacity=2, uciqe=True), Q.QualityMeter(uciqe=True, uciqe_scale=255.0)
    for pred, target in updates:                                      # 3, 5, 6 rows: past the capacity of 2 at once, then again
        for meter in (plain, full, scaled):
            meter.update(pred, target)
    res_plain, res_full, res_scaled = plain.compute(), full.compute(), scaled.compute()
    assert res_plain["per_image"].shape == (6, 6) and set(res_plain) == {"n", "per_image"} | set(Q.COLUMNS)
    assert res_full["per_image"].shape == (6, 10) and set(res_full) == set(res_plain) | set(Q.UCIQE_COLUMNS)
    as_bits = lambda arr: np.ascontiguousarray(arr).view(np.int64)      # noqa: E731  (NaN pairs compare by bit pattern)
    assert np.array_equal(as_bits(res_full["per_image"][:, :6]), as_bits(res_plain["per_image"]))
    direct = np.concatenate([device_rows(pred) for pred, _ in updates])            # (sc, conl, us, uciqe)
    assert np.array_equal(as_bits(res_full["per_image"][:, 6:]), as_bits(direct[:, [3, 0, 1, 2]]))
    direct255 = np.concatenate([device_rows(pred, 255.0) for pred, _ in updates])
    assert np.array_equal(as_bits(res_scaled["per_image"][:, 6:]), as_bits(direct255[:, [3, 0, 1, 2]]))
    for j, k in enumerate(Q.UCIQE_COLUMNS):
        col = res_full["per_image"][:, 6 + j]
        assert res_full[k] == float(np.sum(col) / col.size), k
    for k in Q.COLUMNS:
        assert res_full[k] == res_plain[k] or (np.isnan(res_full[k]) and np.isnan(res_plain[k])), k


# ---------------------------------------------------------------------------------------------------------------- evaluation loops
@functools.lru_cache(maxsize=None)
def small_model():
    from _tree_b_small import load_small_dyn_unet
    _, cfg, m, sd = load_small_dyn_unet()
    return cfg, m.to(DEV), sd


def res_lines(path):
    lines = [ln for ln in open(path).read().split("\n") if ln]
    return [ln.split(":")[0] + ":" for ln in lines], {ln.split(":")[0]: float(ln.split(":")[1]) for ln in lines}


def stand_in_sampler(inp, **kw):
    """(out + 1) / 2 is a smoothed copy of the input image: image-like content without a model."""
    img = inp / 255
    return 2 * (0.5 * img + 0.5 * img.mean(dim=1, keepdim=True)) - 1


def test_evaluate_reports_uciqe_only_when_asked(tmp_path):
    g = torch.Generator().manual_seed(5)
    batches = [(torch.randint(0, 256, (2, 3, 32, 32), generator=g, dtype=torch.uint8).to(DEV),
                torch.randint(0, 256, (2, 3, 32, 32), generator=g, dtype=torch.uint8).to(DEV)) for _ in range(2)]
    with_dir, without_dir, collected = str(tmp_path / "with"), str(tmp_path / "without"), []
    res = EV.evaluate(stand_in_sampler, batches, ddim_step=2, save_dir=with_dir, uciqe=True, collect=collected)
    assert res["n"] == 4 and res["per_image"].shape == (4, 10)
    direct = np.concatenate([device_rows((o + 1) / 2) for o in collected])
    assert np.array_equal(res["per_image"][:, 6], direct[:, 3]) and np.isfinite(direct).all()
    assert res["uciqe"] == float(np.sum(res["per_image"][:, 6]) / 4)
    keys, parsed = res_lines(os.path.join(with_dir, "res.txt"))
    assert keys == ["psnr_orgin_avg:", "ssim_orgin_avg:", "uiqm_orgin_avg:", "uciqe_orgin_avg:", "uism_orgin_avg:", "uicm_orgin_avg:",
                    "uiconm_orgin_avg:"]
    assert parsed == {k[:-1]: res[name] for k, name in EV.RES_KEYS_UCIQE}
    plain = EV.evaluate(stand_in_sampler, batches, ddim_step=2, save_dir=without_dir)
    assert plain["per_image"].shape == (4, 6) and "uciqe" not in plain
    keys, parsed = res_lines(os.path.join(without_dir, "res.txt"))
    assert keys == [k for k, _ in EV.RES_KEYS] and parsed == {k[:-1]: plain[name] for k, name in EV.RES_KEYS}
    assert np.array_equal(plain["per_image"], res["per_image"][:, :6])
    scaled = EV.evaluate(stand_in_sampler, batches, ddim_step=2, uciqe=True, uciqe_scale=255.0)
    print("uciqe", res["uciqe"], "at scale 255", scaled["uciqe"])
    assert scaled["uciqe"] > 10 * res["uciqe"]


def test_reference_shaped_inference_routine(tmp_path, monkeypatch):
    from PIL import Image
    from hdiff_amd import datasets
    cfg, _, sd = small_model()
    root = tmp_path / "data"
    rng = np.random.default_rng(9)
    for sub, ext in (("Val/low", "jpg"), ("Val/high", "jpg"), ("Val/valA", "png"), ("Val/valB", "png")):      # no Train, no Test
        os.makedirs(root / sub)
        for name in ("one", "two", "three"):
            low = rng.integers(0, 256, (4, 4, 3), dtype=np.uint8)    # a few colour patches, enlarged
            Image.fromarray(low).resize((24, 20), Image.BILINEAR).save(str(root / sub / f"{name}.{ext}"))

    def to_32(image):
        img = Image.fromarray(image).resize((32, 32), Image.BILINEAR)
        return {"image": torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).permute(2, 0, 1)}
    tasks = []

    class UnderwaterSpy(datasets.Underwater_Dataset):
        def __init__(self, *args, **kw):
            tasks.append(("underwater", kw.get("task")))
            super().__init__(*args, **kw)

    class AtmosphericSpy(datasets.Atmospheric_Dataset):
        def __init__(self, *args, **kw):
            tasks.append(("atmospheric", kw.get("task")))
            super().__init__(*args, **kw)
    monkeypatch.setattr(datasets, "Underwater_Dataset", UnderwaterSpy)
    monkeypatch.setattr(datasets, "Atmospheric_Dataset", AtmosphericSpy)
    ckpt = tmp_path / "ckpt_small.pt"
    torch.save({"module." + k: v for k, v in sd.items()}, str(ckpt))
    monkeypatch.chdir(tmp_path)
    config = types.SimpleNamespace(underwater_data_name="HICRD", atmospheric_data_name="LoLI", dataset_root=str(root), T=cfg["T"],
                                   channel=cfg["ch"], channel_mult=cfg["ch_mult"], num_res_blocks=cfg["num_res_blocks"],
                                   pretrained_path=str(ckpt), beta_1=BETA_1, beta_T=BETA_T, ddim_step=2, batch_size=2,
                                   device_list=[DEV], transforms=to_32, result_root=str(tmp_path / "results"), uciqe=True)
    torch.manual_seed(4)
    results = EV.inference(config, None)
    assert tasks == [("underwater", "val"), ("atmospheric", "val")]
    assert set(results) == {"HICRD", "LoLI"}
    for name, ext in (("HICRD", "png"), ("LoLI", "jpg")):
        folder = tmp_path / "results" / "ckpt_small.pt" / name
        assert sorted(os.listdir(folder)) == sorted([f"one.{ext}", f"two.{ext}", f"three.{ext}", "res.txt"])
        keys, parsed = res_lines(str(folder / "res.txt"))
        print(name, parsed)
        assert keys == [k for k, _ in EV.RES_KEYS_UCIQE]
        assert results[name]["n"] == 3 and results[name]["per_image"].shape == (3, 10)      # the last batch is short, not dropped
        assert all(np.isfinite(v) for v in parsed.values()), parsed
        assert parsed == {k[:-1]: results[name][v] for k, v in EV.RES_KEYS_UCIQE}
    del config.uciqe                                                  # without the key: the six lines of before
    config.result_root = str(tmp_path / "plain")
    torch.manual_seed(4)
    plain = EV.inference(config)
    keys, _ = res_lines(str(tmp_path / "plain" / "ckpt_small.pt" / "HICRD" / "res.txt"))
    assert keys == [k for k, _ in EV.RES_KEYS] and plain["HICRD"]["per_image"].shape == (3, 6)
