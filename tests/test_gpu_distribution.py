"""GPU checks of the set-level scores (csrc/distribution.hip, hdiff_amd/quality.py: ``moments``, ``kid_sums``, ``kid``,
``DinoFeatures``, ``DistributionMeter``) and of what ``diffusion/Evaluate.py`` does with them.

Gates.  The moments are compared with the float64 definition (tests/_distribution_def.py) BIT FOR BIT: the kernel adds the rows in
the definition's order and rounds where it rounds.  The three kernel sums of KID are compared within 1e-11 relative: the dot products
run in the definition's order, but the pairs are added workgroup by workgroup, and the sums are of positive terms (the features are
positive), so the summation bound for the largest case, 130 * 130 pairs, is 1.7e4 * 2^-53 = 2e-12.  Every test prints its figures before
asserting."""
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
from hdiff_amd.dino import DinoV2Features  # noqa: E402
from hdiff_amd.diffusion import Evaluate as EV  # noqa: E402

import _distribution_def as DD  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]
DEV = "cuda:0"
SUM_GATE = 1e-11
TOKENS = 7                                   # L of the strided class-token layout: 1 + 2 x 3 patches
MOMENT_SHAPES = [(2, 1), (3, 5), (65, 48), (130, 65), (7, 384)]
KID_SHAPES = [(2, 2, 1), (3, 5, 7), (65, 64, 48), (130, 70, 65)]


def bits(t):
    if torch.is_tensor(t):
        t = t.detach().cpu().contiguous().numpy()
    return np.ascontiguousarray(t, dtype=np.float64).view(np.int64).copy()


def rel(a, b):
    return 0.0 if a == b else abs(a - b) / abs(b)


def on_device(x: np.ndarray, layout: str) -> torch.Tensor:
    """The rows as a device tensor: contiguous, or as the class-token view ``t[:, :, 0]`` of a ``(n, d, L)`` tensor (``ch_stride = L``,
    ``row_stride = d * L``) whose other positions hold other numbers."""
    if layout == "rows":
        return torch.from_numpy(np.array(x)).to(DEV)
    n, d = x.shape
    full = np.random.default_rng(n * 1000 + d).standard_normal((n, d, TOKENS)).astype(np.float32)
    full[:, :, 0] = x
    view = torch.from_numpy(full).to(DEV)[:, :, 0]
    assert view.stride() == (d * TOKENS, TOKENS)
    return view


@functools.lru_cache(maxsize=None)
def moment_case(n, d):
    x = DD.offset_features(n, d, 100 + n + d)
    x.setflags(write=False)
    return x, DD.moments_def(x)


@functools.lru_cache(maxsize=None)
def kid_case(n, m, d):
    a, b = DD.positive_features(n, d, 200 + n), DD.positive_features(m, d, 300 + m)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b, DD.kid_sums_def(a, b)


# ---------------------------------------------------------------------------------------------------------------- moments
@pytest.mark.parametrize("layout", ["rows", "class_token"])
@pytest.mark.parametrize("shape", MOMENT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_moments_match_the_definition_bit_for_bit(shape, layout):
    x, (mean, cov) = moment_case(*shape)
    n, got_mean, got_cov = Q.moments(on_device(x, layout))
    assert n == shape[0] and got_mean.dtype == torch.float64 and got_cov.shape == (shape[1], shape[1])
    gm, gc = got_mean.cpu().numpy(), got_cov.cpu().numpy()
    print(f"{shape} {layout}: mean gap {np.abs(gm - mean).max():.1e}, cov gap {np.abs(gc - cov).max():.1e} at largest entry "
          f"{np.abs(cov).max():.3e}")
    assert np.array_equal(bits(gm), bits(mean))
    assert np.array_equal(bits(gc), bits(cov))                          # every entry, both halves
    assert np.array_equal(bits(gc), bits(gc.T))


def test_moments_edge_cases():
    x, _ = moment_case(65, 48)
    n, mean, cov = Q.moments(on_device(x[:1], "rows"))
    assert n == 1 and torch.isnan(cov).all() and torch.isfinite(mean).all()
    assert np.array_equal(bits(mean), bits(x[0].astype(np.float64)))
    spoiled = x.copy()
    spoiled[10, 5] = np.nan                                             # one NaN in one row: channel 5 of every statistic
    want_mean, want_cov = DD.moments_def(spoiled)
    _, mean, cov = Q.moments(on_device(spoiled, "class_token"))
    gm, gc = mean.cpu().numpy(), cov.cpu().numpy()
    touched = np.zeros((48, 48), dtype=bool)
    touched[5, :] = touched[:, 5] = True
    assert np.isnan(gm[5]) and np.isfinite(np.delete(gm, 5)).all()
    assert np.isnan(gc[touched]).all() and np.isfinite(gc[~touched]).all()
    assert np.array_equal(np.isnan(want_cov), touched)
    assert np.array_equal(bits(gc[~touched]), bits(want_cov[~touched])) and np.array_equal(bits(np.delete(gm, 5)), bits(np.delete(want_mean, 5)))
    whole_row = x.copy()
    whole_row[3, :] = np.nan
    _, mean, cov = Q.moments(on_device(whole_row, "rows"))
    assert torch.isnan(mean).all() and torch.isnan(cov).all()


# ---------------------------------------------------------------------------------------------------------------- KID
@pytest.mark.parametrize("shape", KID_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}")
def test_kid_sums_against_the_definition(shape):
    a, b, want = kid_case(*shape)
    got = Q.kid_sums(on_device(a, "rows"), on_device(b, "rows")).cpu().numpy()
    gaps = [rel(float(g), w) for g, w in zip(got, want)]
    print(f"{shape}: sums {got.tolist()} definition {list(want)} rel {[f'{g:.1e}' for g in gaps]}")
    assert all(w > 0 for w in want)
    assert max(gaps) <= SUM_GATE
    n, m = shape[0], shape[1]
    score, score_def = Q.kid(on_device(a, "rows"), on_device(b, "rows")), DD.kid_from_sums(want, n, m)
    size = want[0] / (n * (n - 1)) + want[1] / (m * (m - 1)) + 2 * want[2] / (n * m)
    assert abs(score - score_def) <= SUM_GATE * size


def test_kid_sums_leave_the_diagonal_out():
    """n = 2: the sum over i != j is twice ONE kernel value."""
    a, b, _ = kid_case(2, 2, 1)
    got = Q.kid_sums(on_device(a, "rows"), on_device(b, "rows")).cpu().numpy()
    kaa, kbb, kab = DD.kernel_matrix(a, a), DD.kernel_matrix(b, b), DD.kernel_matrix(a, b)
    print(f"sums {got.tolist()}; 2 k(a0, a1) = {2 * kaa[0, 1]!r}, with the diagonal {kaa.sum()!r}")
    assert got[0] == 2 * kaa[0, 1] and got[1] == 2 * kbb[0, 1]
    assert kaa.sum() > 1.5 * got[0]                                    # the diagonal would not go unnoticed
    assert rel(float(got[2]), float(kab.sum())) <= SUM_GATE
    a3, b5, _ = kid_case(3, 5, 7)
    one_row = Q.kid_sums(on_device(a3[:1], "rows"), on_device(b5, "rows")).cpu().numpy()
    assert one_row[0] == 0.0 and one_row[1] > 0 and np.isnan(Q.kid(on_device(a3[:1], "rows"), on_device(b5, "rows")))


@pytest.mark.parametrize("shape", KID_SHAPES[1:], ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}")
def test_kid_sums_invariances(shape):
    a, b, _ = kid_case(*shape)
    first = bits(Q.kid_sums(on_device(a, "rows"), on_device(b, "rows")))
    again = bits(Q.kid_sums(on_device(a, "rows"), on_device(b, "rows")))
    strided = bits(Q.kid_sums(on_device(a, "class_token"), on_device(b, "class_token")))
    mixed = bits(Q.kid_sums(on_device(a, "class_token"), on_device(b, "rows")))
    swapped = bits(Q.kid_sums(on_device(b, "rows"), on_device(a, "rows")))
    assert np.array_equal(first, again), "not repeatable"
    assert np.array_equal(first, strided) and np.array_equal(first, mixed), "the layout changed the sums"
    assert np.array_equal(swapped, first[[1, 0, 2]]), "swapping the sets must swap the triple bit for bit"
    spoiled = a.copy()
    spoiled[1, 0] = np.nan
    got = Q.kid_sums(on_device(spoiled, "rows"), on_device(b, "rows")).cpu().numpy()
    assert np.isnan(got[0]) and np.isnan(got[2]) and bits(got[1:2]) == first[1]
    assert np.isnan(Q.kid(on_device(spoiled, "rows"), on_device(b, "rows")))


def test_calls_are_legal_under_stream_capture():
    """Neither call allocates or synchronises: both are captured into one graph (outputs and workspace allocated before) and the
    replay on other inputs gives the eager results bit for bit."""
    lib = hdiff_amd.lib()
    a, b, _ = kid_case(65, 64, 48)
    xa, xb = on_device(a, "class_token"), on_device(b, "rows")
    eager_sums = bits(Q.kid_sums(xa, xb))
    _, mean, cov = Q.moments(xa)
    eager_mean, eager_cov = bits(mean), bits(cov)
    n, m, d = 65, 64, 48
    need = C.c_int64(0)
    _capi.check(lib.hdiff_kid_workspace(n, m, C.byref(need)), "kid_workspace")
    scratch = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    base_a = torch.zeros(n, d, TOKENS, device=DEV)
    sa, sb = base_a[:, :, 0], torch.zeros(m, d, device=DEV)
    out = torch.zeros(3, dtype=torch.float64, device=DEV)
    gmean, gcov = torch.zeros(d, dtype=torch.float64, device=DEV), torch.zeros(d, d, dtype=torch.float64, device=DEV)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        s = torch.cuda.current_stream().cuda_stream
        _capi.check(lib.hdiff_feat_moments(sa.data_ptr(), n, d, sa.stride(0), sa.stride(1), gmean.data_ptr(), gcov.data_ptr(), s),
                    "feat_moments")
        _capi.check(lib.hdiff_kid_sums(sa.data_ptr(), n, sb.data_ptr(), m, d, sa.stride(0), sa.stride(1), sb.stride(0), sb.stride(1),
                                       out.data_ptr(), scratch.data_ptr(), s), "kid_sums")
    sa.copy_(xa)
    sb.copy_(xb)
    for _ in range(2):                                                # the second replay starts from a used workspace
        out.zero_()
        gcov.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(out), eager_sums)
        assert np.array_equal(bits(gmean), eager_mean) and np.array_equal(bits(gcov), eager_cov)


# ---------------------------------------------------------------------------------------------------------------- the meter
@functools.lru_cache(maxsize=None)
def small_trunk():
    torch.manual_seed(3)
    return DinoV2Features(embed_dim=32, depth=2, heads=2).to(DEV)


def images(n, seed, H=32, W=46):
    """[n, 3, 32, 46] in [0, 1]: the trunk takes 2 pixels off every edge, which leaves 28 x 42 = 2 x 3 patches (7 tokens)."""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 3, H, W, generator=g).to(DEV)


def test_dino_features_normalise_and_read_the_class_token_in_place():
    """The scaled input is within 1 ulp of ``(x - mean) / std`` computed in float64 and rounded to fp32, mean and std being the
    fp32 constants the kernel is handed (against the decimal 0.485 a pixel that equals the fp32 mean would be 5e-9 off a result of
    0, for any kernel).  The kernel rounds twice, the difference and the quotient: at most 0.5 + 0.56 ulp from the exact value."""
    trunk = small_trunk()
    x = images(3, 1)
    feats = Q.DinoFeatures(trunk)
    scaled = feats.scaled(x)
    mean = np.asarray(DD.IMAGENET_MEAN, dtype=np.float32).astype(np.float64).reshape(1, 3, 1, 1)
    std = np.asarray(DD.IMAGENET_STD, dtype=np.float32).astype(np.float64).reshape(1, 3, 1, 1)
    want = ((x.cpu().numpy().astype(np.float64) - mean) / std).astype(np.float32)
    got = scaled.cpu().numpy()
    ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    same_sign = np.signbit(got) == np.signbit(want)
    print(f"scaled input: worst {ulps[same_sign].max()} ulp from (x - mean) / std in float64; {int((~same_sign).sum())} sign flips")
    assert same_sign.all() and ulps.max() <= 1
    f = feats(x)
    assert f.shape == (3, 32) and f.dtype == torch.float32 and f.stride() == (32 * TOKENS, TOKENS)      # the view nf[:, :, 0]
    assert torch.equal(f, trunk(scaled, ["head"])[0])
    plain = Q.DinoFeatures(trunk, normalize=False)(x)
    assert torch.equal(plain, trunk(x, ["head"])[0]) and not torch.equal(plain, f)
    assert Q.DinoFeatures(trunk).name == trunk.model_name


def test_unloaded_trunk_warns_once():
    torch.manual_seed(4)
    fresh = Q.DinoFeatures(DinoV2Features(embed_dim=32, depth=1, heads=2).to(DEV))
    with pytest.warns(RuntimeWarning, match="no weights were loaded") as caught:
        fresh(images(1, 2))
        fresh(images(1, 3))
    assert len([w for w in caught if "no weights were loaded" in str(w.message)]) == 1


def test_meter_does_not_depend_on_how_the_set_is_cut():
    trunk = small_trunk()
    pred, ref = images(6, 5), images(6, 6)
    whole = Q.DistributionMeter(Q.DinoFeatures(trunk))
    whole.update(pred, ref)
    pieces = Q.DistributionMeter(Q.DinoFeatures(trunk), capacity=2)      # 2, 5, 6 rows: the banks grow twice
    for lo, hi in ((0, 2), (2, 5), (5, 6)):
        pieces.update(pred[lo:hi], ref[lo:hi])
    a, b = whole.compute(), pieces.compute()
    print(f"one update of 6: fd {a['fd']!r} kid {a['kid']!r}; updates of 2, 3, 1: fd {b['fd']!r} kid {b['kid']!r}")
    assert a["n_pred"] == b["n_pred"] == 6 and a["n_ref"] == b["n_ref"] == 6 and a["features"] == trunk.model_name
    assert np.isfinite(a["fd"]) and np.isfinite(a["kid"])
    assert bits(np.array([a["fd"], a["kid"]])).tolist() == bits(np.array([b["fd"], b["kid"]])).tolist()
    # the definitions on the trunk's own class tokens
    feats = Q.DinoFeatures(trunk)
    fa, fb = feats(pred).cpu().numpy(), feats(ref).cpu().numpy()
    (ma, ca), (mb, cb) = DD.moments_def(fa), DD.moments_def(fb)
    assert a["fd"] == Q.frechet_from_moments(ma, ca, mb, cb)
    sums = DD.kid_sums_def(fa, fb)
    size = sum(abs(s) / c for s, c in zip(sums, (30, 30, 18)))
    print(f"kid against the definition: {a['kid']!r} {DD.kid_from_sums(sums, 6, 6)!r}, terms of size {size:.3e}")
    assert abs(a["kid"] - DD.kid_from_sums(sums, 6, 6)) <= SUM_GATE * size


def test_meter_with_a_plain_callable():
    """A callable that returns fixed tensors: the meter without the trunk, unpaired sets of different sizes, NaN handling."""
    a, b, _ = kid_case(65, 64, 48)
    ta, tb = on_device(a, "rows"), on_device(b, "class_token")
    queue = []

    def fixed(img):
        return queue.pop(0)

    img = lambda n: torch.zeros(n, 3, 8, 8, device=DEV)                # noqa: E731
    meter = Q.DistributionMeter(fixed, capacity=4)
    queue += [ta[:40], ta[40:], tb[:1], tb[1:]]
    meter.update(img(40))
    meter.update(img(25), None)
    meter.add_reference(img(1))
    short = meter.compute()                                            # one reference row: no covariance, no pair
    assert short["n_pred"] == 65 and short["n_ref"] == 1 and np.isnan(short["fd"]) and np.isnan(short["kid"])
    meter.add_reference(img(63))
    res = meter.compute()
    assert res["n_pred"] == 65 and res["n_ref"] == 64 and res["features"] == "fixed"
    _, ma, ca = Q.moments(ta)
    _, mb, cb = Q.moments(tb)
    assert res["fd"] == Q.frechet_from_moments(ma, ca, mb, cb) and res["kid"] == Q.kid(ta, tb)
    assert res["fd"] > 0
    with pytest.raises(RuntimeError, match="width"):
        queue.append(torch.zeros(2, 47, device=DEV))
        meter.update(img(2))
    with pytest.raises(RuntimeError, match="feature extractor"):
        queue.append(torch.zeros(3, 48, device=DEV))
        meter.update(img(2))
    assert meter.compute()["n_pred"] == 65
    bad = ta[:2].clone()
    bad[1, 7] = float("inf")
    queue.append(bad)
    meter.update(img(2))
    res = meter.compute()
    assert res["n_pred"] == 67 and np.isnan(res["fd"]) and np.isnan(res["kid"])


# ---------------------------------------------------------------------------------------------------------------- evaluation loop
class Recorder:
    """Stands in for the loaded library and notes the name of every entry that is called."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if not name.startswith("hdiff_"):
            return fn

        def call(*args):
            self.calls.append(name)
            return fn(*args)
        return call


def stand_in_sampler(inp, **kw):
    """(out + 1) / 2 is a smoothed copy of the input image: image-like content without a model."""
    img = inp / 255
    return 2 * (0.5 * img + 0.5 * img.mean(dim=1, keepdim=True)) - 1


def res_lines(path):
    lines = [ln for ln in open(path).read().split("\n") if ln]
    return [ln.split(":")[0] + ":" for ln in lines], {ln.split(":")[0]: float(ln.split(":")[1]) for ln in lines}


def test_evaluate_reports_the_set_scores_only_when_asked(tmp_path, monkeypatch):
    import _perceptual_def as PD
    g = torch.Generator().manual_seed(5)
    batches = [(torch.randint(0, 256, (n, 3, 32, 46), generator=g, dtype=torch.uint8).to(DEV),
                torch.randint(0, 256, (n, 3, 32, 46), generator=g, dtype=torch.uint8).to(DEV)) for n in (2, 3)]
    feats = Q.DinoFeatures(small_trunk())
    recorder = Recorder(hdiff_amd.lib())
    monkeypatch.setattr(_capi, "_lib", recorder)

    def recorded(run):
        recorder.calls = []
        out = run()
        return out, list(recorder.calls)

    def parent_loop():
        """What ``evaluate`` did per batch before it knew of ``distribution``: the quality meter's update and nothing else."""
        meter = Q.QualityMeter()
        with torch.no_grad():
            for inp, target in batches:
                meter.update((stand_in_sampler(inp.float()) + 1) / 2, target.float() / 255)
        res = meter.compute()
        EV.write_res(str(tmp_path / "parent.txt"), res, EV.RES_KEYS)
        return res

    dirs = {k: str(tmp_path / k) for k in ("plain", "with", "both")}
    parent, parent_calls = recorded(parent_loop)
    plain, plain_calls = recorded(lambda: EV.evaluate(stand_in_sampler, batches, ddim_step=2, save_dir=dirs["plain"]))
    res, with_calls = recorded(lambda: EV.evaluate(stand_in_sampler, batches, ddim_step=2, save_dir=dirs["with"], distribution=feats))
    new = {"hdiff_feat_moments", "hdiff_kid_workspace", "hdiff_kid_sums"}
    assert plain_calls == parent_calls and len(parent_calls) > 0, "without the argument the launch list must be the parent's"
    assert not new & set(plain_calls) and new <= set(with_calls)
    assert not any("dino" in c or "layernorm" in c or c == "hdiff_scale_input" for c in plain_calls)
    plain_bytes = open(os.path.join(dirs["plain"], "res.txt"), "rb").read()
    assert plain_bytes == open(str(tmp_path / "parent.txt"), "rb").read()
    assert "fd" not in plain and "kid" not in plain and set(plain) == set(parent)
    # with the argument: the two lines come last, the rest of the file is the plain one
    with_bytes = open(os.path.join(dirs["with"], "res.txt"), "rb").read()
    assert with_bytes.startswith(plain_bytes) and len(with_bytes) > len(plain_bytes)
    keys, parsed = res_lines(os.path.join(dirs["with"], "res.txt"))
    assert keys == [k for k, _ in EV.RES_KEYS] + ["fd_orgin_avg:", "kid_orgin_avg:"]
    assert parsed["fd_orgin_avg"] == res["fd"] and parsed["kid_orgin_avg"] == res["kid"]
    assert np.isfinite(res["fd"]) and res["fd"] > 0 and np.isfinite(res["kid"]) and res["n"] == 5
    direct = Q.DistributionMeter(feats)
    for inp, target in batches:
        direct.update((stand_in_sampler(inp.float()) + 1) / 2, target.float() / 255)
    want = direct.compute()
    assert (res["fd"], res["kid"]) == (want["fd"], want["kid"])
    # a meter passed in goes on filling; with LPIPS as well its line precedes the two
    metric = Q.LPIPS(PD.state_dict_of(PD.VGG_CFGS["vgg16"], PD.make_weights(PD.VGG_CFGS["vgg16"], 1)), PD.make_lin(1)).to(DEV)
    held = Q.DistributionMeter(feats)
    both = EV.evaluate(stand_in_sampler, batches, ddim_step=2, save_dir=dirs["both"], lpips=metric, uciqe=True, distribution=held)
    keys, parsed = res_lines(os.path.join(dirs["both"], "res.txt"))
    assert keys == [k for k, _ in EV.RES_KEYS_UCIQE] + ["lpips_orgin_avg:", "fd_orgin_avg:", "kid_orgin_avg:"]
    assert (both["fd"], both["kid"]) == (want["fd"], want["kid"]) and parsed["lpips_orgin_avg"] == both["lpips"]
    assert held.compute()["n_pred"] == 5
