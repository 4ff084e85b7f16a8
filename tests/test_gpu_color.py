"""GPU checks of the device colour differences (csrc/color_diff.hip, hdiff_amd/quality.py: ``color_difference``, ``ciede2000_lab``,
``QualityMeter(color=True)``) and of what the evaluation loop does with them (``Evaluate.evaluate(color=True)``).

Gates.  ``ciede2000_lab`` on the 34 published pairs (tests/golden/ciede2000_sharma.json): within 6e-5 of the table (its rounding to
four decimals plus slack) and within 1e-12 relative of the float64 definition (tests/_color_def.py).  The four scores of an image
against the definition within 1e-11 relative, the project's gate for its double scores: both sides sum in double, the worst-case
summation bound at the largest size is 8 640 * 2^-53, about 1e-12, and ``pow`` / ``cbrt`` / ``atan2`` / ``cos`` / ``sin`` / ``exp`` differ in
the last bits.  tests/test_color_cpu.py holds every fixture to its hue-branch margins, so that no branch can flip inside that gate.
Every test prints its figures before asserting; the values measured on an MI355X are in profiles/device_color.txt."""
import ctypes as C
import functools
import json
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

import _color_def as D  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DEF_GATE = 1e-11
TABLE_GATE = 6e-5
LAB_GATE = 1e-12
NAMES = ("de00", "de00_p95", "de76", "angular")
# (8, 13): less than one workgroup; (33, 47): odd sizes, a ragged last block; (72, 120): 8 640 pixels, several workgroups per image.
# Three pairs per size: the independent draw, the same pair swapped (the same margins), and a near-identical pair.
BATCHES = {(8, 13): ((8, 13, 2000, False), (8, 13, 2004, True)), (33, 47): ((33, 47, 2003, False), (33, 47, 2005, True)),
           (72, 120): ((72, 120, 2001, False), (72, 120, 2002, True))}


def rel(a, b):
    return 0.0 if a == b else abs(a - b) / abs(b)          # equal values (0 against 0 among them) have no gap


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int64).numpy().copy()


def dev(images):
    """A list of fp32 [3, H, W] arrays -> [N, 3, H, W] on the device."""
    return torch.from_numpy(np.stack(images)).to(DEV)


@functools.lru_cache(maxsize=None)
def pairs(size):
    """The three (prediction, target) pairs of one size; computed once, shared, never modified."""
    independent, near = BATCHES[size]
    assert independent in D.FIXTURES and near in D.FIXTURES
    p, t = D.fixture(*independent)
    return ((p, t), (t, p), D.fixture(*near))


@functools.lru_cache(maxsize=None)
def definition_rows(size):
    return tuple(D.color_def(p, t) for p, t in pairs(size))


def device_rows(pred, target):
    """[N, 4] float64 on the host."""
    out = Q.color_difference(pred, target)
    assert len(out) == 4 and all(o.dtype == torch.float64 and o.shape == (pred.shape[0],) for o in out)
    return torch.stack(out, dim=1).cpu().numpy()


def four(pred, target):
    return bits(torch.stack(Q.color_difference(pred, target), dim=1))


def batch(size):
    return dev([p for p, _ in pairs(size)]), dev([t for _, t in pairs(size)])


def within_gate(got, want, what):
    gaps = [rel(float(g), float(w)) for g, w in zip(got, want)]
    print(f"{what}: device {[float(g) for g in got]}  definition {[float(w) for w in want]}  relative gaps {[f'{g:.2e}' for g in gaps]}")
    assert np.isfinite(np.asarray(got, dtype=np.float64)).all(), (what, got)
    assert max(gaps) <= DEF_GATE, (what, gaps)
    return max(gaps)


# ---------------------------------------------------------------------------------------------------------------- the formula
def test_ciede2000_lab_on_the_published_table():
    rows = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "ciede2000_sharma.json")))["pairs"], dtype=np.float64)
    lab1, lab2, want = rows[:, :3].copy(), rows[:, 3:6].copy(), rows[:, 6]
    got = Q.ciede2000_lab(torch.from_numpy(lab1).to(DEV), torch.from_numpy(lab2).to(DEV))
    assert got.dtype == torch.float64 and got.shape == (34,)
    got = got.cpu().numpy()
    by_def = D.ciede2000_lab_def(lab1, lab2)
    to_table, to_def = np.abs(got - want), np.abs(got - by_def) / by_def
    for i in range(34):
        print(f"pair {i + 1}: device {got[i]!r}  definition {by_def[i]!r}  table {want[i]}")
    print(f"worst deviation from the table {to_table.max():.3e}; worst relative gap to the definition {to_def.max():.3e}")
    assert to_table.max() <= TABLE_GATE and to_def.max() <= LAB_GATE
    swapped = Q.ciede2000_lab(torch.from_numpy(lab2).to(DEV), torch.from_numpy(lab1).to(DEV)).cpu().numpy()
    assert (np.abs(swapped - got) <= 1e-13 * got).all()


# ---------------------------------------------------------------------------------------------------------------- definition
@pytest.mark.parametrize("size", sorted(BATCHES))
def test_scores_and_map_against_the_definition(size):
    pred, target = batch(size)
    out = Q.color_difference(pred, target, with_map=True)
    assert len(out) == 5 and out[4].dtype == torch.float32 and out[4].shape == (3, 1) + size
    got = torch.stack(out[:4], dim=1).cpu().numpy()
    worst = max(within_gate(got[i], definition_rows(size)[i], f"{size} pair {i}") for i in range(3))
    print(f"{size}: worst relative gap to the definition {worst:.2e}")
    assert np.array_equal(bits(torch.stack(out[:4], dim=1)), four(pred, target))      # the map changes no score
    maps = out[4].cpu().numpy()
    for i, (p, t) in enumerate(pairs(size)):
        want = D.pixels_def(p, t)[0].astype(np.float32)                # rounded once to fp32
        steps = np.abs(maps[i, 0].view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        print(f"{size} pair {i}: map pixels that differ from the rounded definition {int((steps > 0).sum())}, largest step {int(steps.max())}")
        assert steps.max() <= 1                                         # that value, or its neighbour


PAIR_A = ((0.2, 0.5, 0.3), (0.25, 0.45, 0.3))
PAIR_B = ((0.9, 0.4, 0.1), (0.5, 0.4, 0.3))


def two_pair_image(count_b, H=8, W=13):
    """(prediction, target): `count_b` pixels of pair B scattered among pixels of pair A."""
    where = np.zeros(H * W, dtype=bool)
    where[np.random.default_rng(7).permutation(H * W)[:count_b]] = True
    p, t = np.empty((3, H * W), dtype=np.float32), np.empty((3, H * W), dtype=np.float32)
    for c in range(3):
        p[c] = np.where(where, np.float32(PAIR_B[0][c]), np.float32(PAIR_A[0][c]))
        t[c] = np.where(where, np.float32(PAIR_B[1][c]), np.float32(PAIR_A[1][c]))
    return p.reshape(3, H, W), t.reshape(3, H, W)


def test_percentile_inside_ties():
    """n = 104: the percentile is element 98.  With 14 copies of the larger value it lies among them, with 4 among the smaller."""
    single = [D.pixels_def(np.asarray(a, dtype=np.float32).reshape(3, 1, 1), np.asarray(b, dtype=np.float32).reshape(3, 1, 1))
              for a, b in (PAIR_A, PAIR_B)]
    value_a, value_b = float(single[0][0][0, 0]), float(single[1][0][0, 0])
    for _, _, _, _, terms in single:                                   # neither pair sits at a hue branch
        assert abs(abs(float(terms["h1"][0, 0] - terms["h2"][0, 0])) - 180.0) > 1.0 and float(terms["cc"][0, 0]) > 1.0
    assert value_b > 2 * value_a > 0
    images = [two_pair_image(14), two_pair_image(4)]
    got = device_rows(dev([p for p, _ in images]), dev([t for _, t in images]))
    print(f"pair A {value_a!r}, pair B {value_b!r}; device p95 with 14 B {got[0, 1]!r}, with 4 B {got[1, 1]!r}")
    assert rel(got[0, 1], value_b) <= DEF_GATE and rel(got[1, 1], value_a) <= DEF_GATE
    for i, (p, t) in enumerate(images):
        within_gate(got[i], D.color_def(p, t), f"two-pair image {i}")


def test_identical_images_give_exactly_zero():
    pred, _ = batch((33, 47))
    got = device_rows(pred, pred.clone())
    print("identical:", got.tolist())
    assert np.array_equal(got, np.zeros((3, 4)))


def test_grey_ramps_and_a_black_prediction():
    H, W = 8, 13
    ramp = (np.float32(0.05) + np.float32(0.95) * (np.arange(H * W, dtype=np.float32) / np.float32(H * W - 1))).reshape(1, H, W)
    grey = np.repeat(ramp, 3, axis=0)
    darker = grey * np.float32(0.6)
    black = np.zeros_like(grey)
    noisy = D.fixture(H, W, 2000)[1]
    preds, targets = [grey, black, black], [darker, noisy, black]
    got = device_rows(dev(preds), dev(targets))
    want = [D.color_def(p, t) for p, t in zip(preds, targets)]
    assert got[0, 3] == 0.0 and want[0][3] == 0.0                       # parallel vectors: exactly
    within_gate(got[0, :3], want[0][:3], "grey ramp against a darker one")
    assert np.isnan(got[1, 3]) and np.isnan(want[1][3])                 # no pixel counts
    within_gate(got[1, :3], want[1][:3], "black prediction")
    assert np.array_equal(got[2, :3], np.zeros(3)) and np.isnan(got[2, 3])


# ---------------------------------------------------------------------------------------------------------------- batches
def test_one_non_finite_pixel_spoils_its_image_alone():
    pred, target = batch((33, 47))
    clean = four(pred, target)
    for which in (0, 1):                                                # in the prediction, then in the target
        tensors = [pred.clone(), target.clone()]
        tensors[which][1, 2, 20, 41] = float("nan") if which == 0 else float("inf")
        got = four(*tensors)
        as_float = got.view(np.float64)
        print("non-finite pixel in", ("prediction", "target")[which], as_float.tolist())
        assert np.isnan(as_float[1]).all()
        assert np.array_equal(got[0], clean[0]) and np.array_equal(got[2], clean[2])
    assert not np.isnan(clean.view(np.float64)).any()


def test_scores_do_not_depend_on_the_batch_and_repeat():
    pred, target = batch((72, 120))
    whole = four(pred, target)
    assert np.array_equal(whole, four(pred, target))                    # two calls are bit-identical
    alone = four(pred[2:3].contiguous(), target[2:3].contiguous())
    assert np.array_equal(alone[0], whole[2])
    five_p, five_t = torch.cat([pred, pred[:2]]), torch.cat([target, target[:2]])
    for place in (0, 4):                                                # image 2 as the first and as the last of a batch of 5
        order = [(2 + k - place) % 5 for k in range(5)]
        moved = four(five_p[order].contiguous(), five_t[order].contiguous())
        assert np.array_equal(moved[place], alone[0]), place


def test_call_is_legal_under_stream_capture():
    """The call neither allocates nor synchronises: it is captured into a graph (one stream, a linear graph; workspace and outputs
    allocated before), and the replay on other inputs gives the eager result bit for bit."""
    lib = hdiff_amd.lib()
    pred, target = batch((33, 47))
    eager = four(pred, target)
    need = C.c_int64(0)
    _capi.check(lib.hdiff_color_diff_workspace(3, 33, 47, C.byref(need)), "color_diff_workspace")
    scratch = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    pa, ta = torch.zeros_like(pred), torch.zeros_like(target)
    out = torch.zeros(3, 4, dtype=torch.float64, device=DEV)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        s = torch.cuda.current_stream().cuda_stream
        _capi.check(lib.hdiff_color_diff(pa.data_ptr(), ta.data_ptr(), 3, 33, 47, out.data_ptr(), None, scratch.data_ptr(), s),
                    "color_diff")
    pa.copy_(pred)
    ta.copy_(target)
    for _ in range(2):                                                # the second replay starts from a used workspace
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(out), eager)


# ---------------------------------------------------------------------------------------------------------------- meter
def as_bits(arr):
    return np.ascontiguousarray(arr).view(np.int64)                    # NaN pairs compare by bit pattern


def test_quality_meter_with_and_without_colour():
    pred, target = batch((33, 47))
    updates = [(pred, target), (pred[1:3].contiguous(), None), (target[:1].contiguous(), pred[:1].contiguous())]
    plain, colour, both = Q.QualityMeter(capacity=2), Q.QualityMeter(capacity=2, color=True), Q.QualityMeter(uciqe=True, color=True)
    for p, t in updates:                                              # 3, 5, 6 rows: past the capacity of 2 at once, then again
        for meter in (plain, colour, both):
            meter.update(p, t)
    res_plain, res_colour, res_both = plain.compute(), colour.compute(), both.compute()
    assert colour.columns == Q.COLUMNS + Q.COLOR_COLUMNS and both.columns == Q.COLUMNS + Q.UCIQE_COLUMNS + Q.COLOR_COLUMNS
    assert plain.columns == Q.COLUMNS and set(res_plain) == {"n", "per_image"} | set(Q.COLUMNS) and res_plain["per_image"].shape == (6, 6)
    assert res_colour["per_image"].shape == (6, 10) and set(res_colour) == set(res_plain) | set(Q.COLOR_COLUMNS)
    assert res_both["per_image"].shape == (6, 14) and set(res_both) == set(res_colour) | set(Q.UCIQE_COLUMNS)
    # a meter without color= produces the rows of the direct calls, as it always did; the colour meter's first six are the same
    direct = []
    for p, t in updates:
        pair = torch.stack(Q.psnr_ssim(p, t), dim=1).cpu().numpy() if t is not None else np.full((p.shape[0], 2), np.nan)
        parts = torch.stack(Q.uiqm(p), dim=1).cpu().numpy()           # (uicm, uism, uiconm, uiqm)
        direct.append(np.concatenate([pair, parts[:, [3, 0, 1, 2]]], axis=1))
    direct = np.concatenate(direct)
    finite = ~np.isnan(direct)
    assert np.array_equal(np.isnan(res_plain["per_image"]), ~finite)
    assert np.array_equal(as_bits(res_plain["per_image"])[finite], as_bits(direct)[finite])
    assert np.array_equal(as_bits(res_colour["per_image"][:, :6]), as_bits(res_plain["per_image"]))
    assert np.array_equal(as_bits(res_both["per_image"][:, :6]), as_bits(res_plain["per_image"]))
    # the colour columns: the direct call's where there was a target, NaN where there was none
    want = np.concatenate([device_rows(p, t) if t is not None else np.full((p.shape[0], 4), np.nan) for p, t in updates])
    for res, at in ((res_colour, 6), (res_both, 10)):
        block = res["per_image"][:, at:at + 4]
        assert np.isnan(block[3:5]).all() and np.isfinite(block[[0, 1, 2, 5]]).all()
        assert np.array_equal(as_bits(block)[[0, 1, 2, 5]], as_bits(want)[[0, 1, 2, 5]])
        for j, k in enumerate(Q.COLOR_COLUMNS):
            col = block[[0, 1, 2, 5], j]
            assert res[k] == float(np.sum(col) / col.size), k         # over the images that had a target, like PSNR
    for k in Q.COLUMNS:
        assert res_colour[k] == res_plain[k] or (np.isnan(res_colour[k]) and np.isnan(res_plain[k])), k
    unpaired = Q.QualityMeter(color=True)
    unpaired.update(pred, None)
    assert all(np.isnan(unpaired.compute()[k]) for k in Q.COLOR_COLUMNS)


# ---------------------------------------------------------------------------------------------------------------- evaluation
def stand_in_sampler(inp, **kw):
    """(out + 1) / 2 is a smoothed copy of the input image: image-like content without a model."""
    img = inp / 255
    return 2 * (0.5 * img + 0.5 * img.mean(dim=1, keepdim=True)) - 1


def res_lines(path):
    lines = [ln for ln in open(path).read().split("\n") if ln]
    return [ln.split(":")[0] + ":" for ln in lines], {ln.split(":")[0]: float(ln.split(":")[1]) for ln in lines}


def test_evaluate_reports_the_colour_scores_only_when_asked(tmp_path):
    g = torch.Generator().manual_seed(5)
    batches = [(torch.randint(0, 256, (2, 3, 8, 13), generator=g, dtype=torch.uint8).to(DEV),
                torch.randint(0, 256, (2, 3, 8, 13), generator=g, dtype=torch.uint8).to(DEV)) for _ in range(2)]
    with_dir, without_dir, collected = str(tmp_path / "with"), str(tmp_path / "without"), []
    res = EV.evaluate(stand_in_sampler, batches, ddim_step=2, save_dir=with_dir, color=True, collect=collected)
    assert res["n"] == 4 and res["per_image"].shape == (4, 10) and {"ciede2000", "ciede2000_p95", "deltae76", "angular"} <= set(res)
    direct = np.concatenate([device_rows((o + 1) / 2, b[1].float() / 255) for o, b in zip(collected, batches)])
    assert np.array_equal(res["per_image"][:, 6:], direct) and np.isfinite(direct).all()
    for j, k in enumerate(Q.COLOR_COLUMNS):
        assert res[k] == float(np.sum(direct[:, j]) / 4)
    keys, parsed = res_lines(os.path.join(with_dir, "res.txt"))
    assert keys == [k for k, _ in EV.RES_KEYS] + ["ciede2000_orgin_avg:", "ciede2000_p95_orgin_avg:", "deltae76_orgin_avg:",
                                                  "angular_orgin_avg:"]
    for k, name in EV.RES_KEYS + EV.RES_KEYS_COLOR:                    # (UISM of so small an image may be NaN)
        assert parsed[k[:-1]] == res[name] or (np.isnan(parsed[k[:-1]]) and np.isnan(res[name])), k
    plain = EV.evaluate(stand_in_sampler, batches, ddim_step=2, save_dir=without_dir)
    assert plain["per_image"].shape == (4, 6) and not set(Q.COLOR_COLUMNS) & set(plain)
    assert np.array_equal(as_bits(plain["per_image"]), as_bits(res["per_image"][:, :6]))
    text = open(os.path.join(without_dir, "res.txt")).read()
    assert text == "".join("\n" + key + str(plain[k]) for key, k in EV.RES_KEYS)      # without color=: the file of before, byte for byte
    assert open(os.path.join(with_dir, "res.txt")).read().startswith(text)
